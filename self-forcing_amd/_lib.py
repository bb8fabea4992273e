"""ctypes binding of the C-ABI in include/sf_hip.h (self-forcing_amd/csrc/libsf_hip.so).

There is no fallback: if the library is missing, loading raises with the build command.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from typing import Optional

# A default for the HIP runtime, set before anything has initialised it (it reads the variable once, at start-up; a value
# the user has set wins): with the runtime's default signal pool a steady stream of ~430 launches per forward keeps one of
# its helper threads spinning for signals to come free -- 0.83 of a host core per process, measured on MI355X / ROCm 7.0
# (bench.py: host_busy_cores_by_thread); with 256 or more signals in the pool that thread idles (0.004).  Together with
# the wrapper's pacing (wan_wrapper.py) a rank needs 0.17 of a core instead of 1.0-1.7; throughput is unchanged.
# (The C library itself reads no environment variables; this is the Python host layer configuring the runtime under it.)
os.environ.setdefault("ROC_SIGNAL_POOL_SIZE", "1024")

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIB_PATH = os.environ.get("SF_HIP_LIB") or os.path.join(CSRC, "libsf_hip.so")   # SF_HIP_LIB: alternate builds (kernel ablation timing)

ABI_VERSION = 11
FP8_AMAX_PARTS = 1024   # SF_FP8_AMAX_PARTS: scratch floats per segment behind the scales of sf_quantize_fp8

# epilogue codes (enum sf_epilogue)
EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_RESID, EPI_BIAS_GATE_RESID, EPI_F32 = 0, 1, 2, 3, 4
# enum sf_conv_epilogue
CONV_BIAS, CONV_BIAS_RESID, CONV_BIAS_CLAMP_F32 = 0, 1, 2
VAE_MAX_STAGES = 4
# enum sf_taehv_epilogue
TAEHV_EPILOGUES = {"bias_relu": 0, "bias_resid_relu": 1, "plain": 2, "relu": 3, "head_f32": 4, "latent_f32": 5}
TAEHV_STAGES, TAEHV_BLOCKS = 3, 3
# enum sf_taehv_pixel_dtype
TAEHV_PIXEL_DTYPES = {"bfloat16": 0, "float32": 1}
# enum sf_pose_dtype
POSE_DTYPES = {"uint8": 0, "float32": 1, "bfloat16": 2}
POSE_CONVS = 6
# enum sf_jpeg_subsampling / sf_jpeg_dtype / sf_jpeg_range / sf_jpeg_status
JPEG_SUBSAMPLINGS = {"420": 0, "444": 1}
JPEG_DTYPES = {"uint8": 0, "float32": 1, "bfloat16": 2}
JPEG_RANGES = {(-1, 1): 0, (0, 1): 1}
JPEG_STATUS = {1: "an interval outgrew its worst-case slot", 2: "a coefficient is outside the baseline range",
               4: "the files do not fit the output buffer"}
# enum sf_jpeg_decode_sampling / sf_jpeg_layout / sf_jpeg_decode_status; SF_JPEG_DECODE_FILE_BYTES
JPEG_DECODE_SAMPLINGS = {"420": 0, "444": 1, "422": 2, "gray": 3}
JPEG_LAYOUTS = {"hwc": 0, "pose": 1, "chw": 2}
JPEG_DECODE_STATUS = {1: "a bit pattern that is no Huffman code", 2: "a zero run past the 63rd coefficient", 4: "a truncated restart interval",
                      8: "a wrong number of restart markers"}
JPEG_DECODE_FILE_BYTES = 8960
# enum sf_resize_filter; SF_RESIZE_MAX_RATIO (layouts and output types are the decoder's: JPEG_LAYOUTS, JPEG_DTYPES)
RESIZE_FILTERS = {"bilinear": 0, "bicubic": 1}
RESIZE_MAX_RATIO = 8
# enum sf_yuv_format / sf_yuv_chroma; SF_YUV_MAX_SIZE (yuv_reference.FORMATS / CHROMAS / MAX_SIZE hold the same values)
YUV_FORMATS = {"i420": 0, "nv12": 1, "i422": 2, "i444": 3, "gray": 4, "yuyv": 5, "uyvy": 6}
YUV_CHROMAS = {"nearest": 0, "triangle": 1}
YUV_MAX_SIZE = 16384
# SF_POSE_RENDER_MAX_PEOPLE / _MAX_SIZE / _MAX_COORD (layouts and output types are the decoder's too)
POSE_RENDER_MAX_PEOPLE, POSE_RENDER_MAX_SIZE, POSE_RENDER_MAX_COORD = 8, 4096, 8191
POSE_RETARGET_MAX_RATE, POSE_RETARGET_MAX_FRAMES = 65535, 1 << 20   # SF_POSE_RETARGET_MAX_RATE / _MAX_FRAMES
POSE_SMOOTH_MAX_GAP = 65535                                         # sf_pose_smooth_args.max_gap
POSE_TRACK_MAX_AGE, POSE_TRACK_STATE_WORDS = 65535, 40              # sf_pose_track_args.max_age; the words of a row of its state
# SF_POSE_BOXES_MAX_* / SF_POSE_CROP_MAX_* / SF_POSE_SIMCC_*; enum sf_pose_simcc_dtype (the crop's output types are JPEG_DTYPES' two float ones)
POSE_BOXES_MAX_ANCHORS, POSE_BOXES_MAX_STRIDES, POSE_BOXES_MAX_CLASSES, POSE_BOXES_MAX_FRAMES = 16384, 4, 255, 65535
POSE_CROP_MAX_SIZE, POSE_CROP_MAX_FRAME, POSE_SIMCC_POINTS, POSE_SIMCC_MAX_BINS = 1024, 16384, 133, 65536
POSE_SIMCC_DTYPES = {"float32": 0, "float16": 1}
# enum sf_clip_dtype
CLIP_DTYPES = {"float32": 0, "bfloat16": 1}
ACT_NONE, ACT_SILU, ACT_GELU = 0, 1, 2
# enum sf_attn_structure / sf_gemm_structure
ATTN_STRUCTURES = {"auto": 0, "r64": 1, "w8": 2, "w4": 3}
CONV_STRUCTURES = {"auto": 0, "igemm": 1, "halo": 2}
GEMM_STRUCTURES = {"auto": 0, "t128": 1, "pp256": 2, "pp128": 3, "pp224": 4, "pp192": 5}


class GemmArgs(C.Structure):
    _fields_ = [
        ("a", C.c_void_p), ("w", C.c_void_p), ("bias", C.c_void_p), ("out", C.c_void_p),
        ("resid", C.c_void_p), ("gate_mod", C.c_void_p), ("gate_e0", C.c_void_p),
        ("gate_group_stride", C.c_int64), ("rows_per_group", C.c_int32),
        ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32),
        ("lda", C.c_int32), ("ldw", C.c_int32), ("ldo", C.c_int32), ("ldr", C.c_int32),
        ("epilogue", C.c_int32), ("batch", C.c_int32),
        ("a_bstride", C.c_int64), ("w_bstride", C.c_int64), ("o_bstride", C.c_int64), ("r_bstride", C.c_int64),
        ("structure", C.c_int32),
    ]


class AttentionArgs(C.Structure):
    _fields_ = ([(n, C.c_void_p) for n in ("q", "k", "v", "out")]
                + [(n, C.c_int32) for n in ("B", "H", "Lq", "Lk")]
                + [(n, C.c_int64) for n in ("q_stride", "q_bstride", "kv_stride", "kv_bstride", "o_stride", "o_bstride")]
                + [("structure", C.c_int32), ("accumulate", C.c_int32), ("keys", C.c_void_p), ("log2w", C.c_void_p)])


class LayerWeights(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in (
        "modulation", "norm3_w", "norm3_b", "qkv_w", "qkv_b", "norm_q_w", "norm_k_w", "o_w", "o_b",
        "cq_w", "cq_b", "ckv_w", "ckv_b", "cnorm_q_w", "cnorm_k_w", "co_w", "co_b",
        "ffn0_w", "ffn0_b", "ffn2_w", "ffn2_b")]


class LayerFp8(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in (
        "qkv_q", "o_q", "cq_q", "ckv_q", "co_q", "ffn0_q", "ffn2_q",
        "qkv_s", "o_s", "cq_s", "ckv_s", "co_s", "ffn0_s", "ffn2_s")]


# (field of sf_model / sf_layer_fp8 without its _q / _s suffix, the reference Linear(s) it stands for); a stacked weight
# carries one scale per reference Linear
FP8_MODEL_LINEARS = (("text0", ("text_embedding.0",)), ("text2", ("text_embedding.2",)), ("time0", ("time_embedding.0",)),
                     ("time2", ("time_embedding.2",)), ("tproj", ("time_projection.1",)), ("head", ("head.head",)),
                     ("pose", ("pose_proj",)))
FP8_LAYER_LINEARS = (("qkv", ("self_attn.q", "self_attn.k", "self_attn.v")), ("o", ("self_attn.o",)), ("cq", ("cross_attn.q",)),
                     ("ckv", ("cross_attn.k", "cross_attn.v")), ("co", ("cross_attn.o",)), ("ffn0", ("ffn.0",)), ("ffn2", ("ffn.2",)))


class Model(C.Structure):
    _fields_ = (
        [(n, C.c_int32) for n in ("dim", "ffn_dim", "num_heads", "num_layers", "in_dim", "out_dim",
                                  "freq_dim", "text_dim", "text_len")]
        + [("eps", C.c_float)]
        + [(n, C.c_void_p) for n in ("patch_w", "patch_b", "text0_w", "text0_b", "text2_w", "text2_b",
                                     "time0_w", "time0_b", "time2_w", "time2_b", "tproj_w", "tproj_b",
                                     "head_w", "head_b", "head_mod", "pose_w", "pose_b")]
        + [("pose_dim", C.c_int32)]
        + [("layers_host", C.POINTER(LayerWeights)),
           ("rope_cos", C.c_void_p), ("rope_sin", C.c_void_p),
           ("sched_sigmas", C.c_void_p), ("sched_timesteps", C.c_void_p),
           ("n_table", C.c_int32)]
        # ABI 10: FP8 linear layers (all zero = bf16)
        + [("fp8", C.c_int32)]
        + [(n + "_q", C.c_void_p) for n, _ in FP8_MODEL_LINEARS]
        + [(n + "_s", C.c_void_p) for n, _ in FP8_MODEL_LINEARS]
        + [("layers_fp8_host", C.POINTER(LayerFp8))]
    )


class ForwardArgs(C.Structure):
    _fields_ = [
        ("batch", C.c_int32), ("frames", C.c_int32), ("lat_h", C.c_int32), ("lat_w", C.c_int32),
        ("groups", C.c_int32),
        ("noisy", C.c_void_p), ("timestep", C.c_void_p), ("t_is_int64", C.c_int32),
        ("prompt_embeds", C.c_void_p), ("init_cross", C.c_int32), ("add_condition", C.c_void_p),
        ("k_cache_host", C.POINTER(C.c_void_p)), ("v_cache_host", C.POINTER(C.c_void_p)),
        ("ck_cache_host", C.POINTER(C.c_void_p)), ("cv_cache_host", C.POINTER(C.c_void_p)),
        ("cache_tokens", C.c_int64),
        ("sink_tokens", C.c_int32), ("evict", C.c_int32), ("keep", C.c_int32),
        ("write_start", C.c_int32), ("attn_start", C.c_int32), ("attn_end", C.c_int32),
        ("start_frame", C.c_int32),
        ("evict_scratch", C.c_void_p), ("evict_scratch_bytes", C.c_size_t),
        ("cache_only", C.c_int32),
        ("flow_out", C.c_void_p), ("x0_out", C.c_void_p),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
        ("kv_index_out", C.c_void_p), ("global_end", C.c_int64),
    ]


class I2VLayer(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("kvimg_w", "kvimg_b", "norm_k_img_w")]


class I2VModel(C.Structure):
    _fields_ = ([("clip_dim", C.c_int32), ("clip_len", C.c_int32), ("img_eps", C.c_float)]
                + [(n, C.c_void_p) for n in ("img_ln0_w", "img_ln0_b", "img_fc1_w", "img_fc1_b", "img_fc2_w", "img_fc2_b",
                                             "img_ln1_w", "img_ln1_b")]
                + [("layers_host", C.POINTER(I2VLayer))])


class I2VArgs(C.Structure):
    _fields_ = [("clip_feature", C.c_void_p), ("y", C.c_void_p),
                ("y_bstride", C.c_int64), ("y_cstride", C.c_int64), ("y_fstride", C.c_int64), ("y_channels", C.c_int32),
                ("kimg_cache_host", C.POINTER(C.c_void_p)), ("vimg_cache_host", C.POINTER(C.c_void_p))]


class ForwardCall(C.Structure):
    _fields_ = [("passes", C.POINTER(ForwardArgs) * 2), ("n_passes", C.c_int32), ("cross_keys", C.c_void_p), ("cross_log2w", C.c_void_p),
                ("i2v_model", C.POINTER(I2VModel)), ("i2v_args", C.POINTER(I2VArgs))]


class ConvArgs(C.Structure):
    _fields_ = (
        [(n, C.c_void_p) for n in ("x", "w", "bias", "out", "resid", "out_f32")]
        + [(n, C.c_int32) for n in ("Tout", "H", "W", "Hin", "Win", "Cin", "Cout", "kt", "kh", "kw", "upsample",
                                    "t_in_offset", "ldw", "ldo", "ldr", "out_frame_offset", "interleave_c", "epilogue", "structure")]
        + [("norm_out", C.c_void_p), ("norm_gamma", C.c_void_p), ("norm_ld", C.c_int32), ("norm_frame_offset", C.c_int32)]
        + [("stride_hw", C.c_int32), ("stride_t", C.c_int32)]
    )


class VaeConv(C.Structure):
    _fields_ = [("w", C.c_void_p), ("bias", C.c_void_p)] + [(n, C.c_int32) for n in ("cin", "cout", "kt", "kh", "kw", "ldw")]


class VaeResBlock(C.Structure):
    _fields_ = [("gamma1", C.c_void_p), ("gamma2", C.c_void_p), ("conv1", VaeConv), ("conv2", VaeConv), ("shortcut", VaeConv)]


class VaeModel(C.Structure):
    _fields_ = [
        ("z_dim", C.c_int32), ("n_stages", C.c_int32), ("res_per_stage", C.c_int32),
        ("temporal_up", C.c_int32 * VAE_MAX_STAGES),
        ("latent_mean", C.c_void_p), ("latent_std", C.c_void_p), ("conv2_w", C.c_void_p), ("conv2_b", C.c_void_p),
        ("conv1", VaeConv), ("mid0", VaeResBlock), ("mid2", VaeResBlock),
        ("attn_gamma", C.c_void_p), ("attn_qk_w", C.c_void_p), ("attn_qk_b", C.c_void_p),
        ("attn_v_w", C.c_void_p), ("attn_v_b", C.c_void_p), ("attn_proj_w", C.c_void_p), ("attn_proj_b", C.c_void_p),
        ("res_host", C.POINTER(VaeResBlock)),
        ("time_conv", VaeConv * VAE_MAX_STAGES), ("up_conv", VaeConv * VAE_MAX_STAGES),
        ("head_gamma", C.c_void_p), ("head_conv", VaeConv),
    ]


class VaeEncoder(C.Structure):
    _fields_ = [
        ("z_dim", C.c_int32), ("n_stages", C.c_int32), ("res_per_stage", C.c_int32),
        ("temporal_down", C.c_int32 * VAE_MAX_STAGES),
        ("latent_mean", C.c_void_p), ("latent_std", C.c_void_p), ("conv1_w", C.c_void_p), ("conv1_b", C.c_void_p),
        ("in_conv", VaeConv), ("res_host", C.POINTER(VaeResBlock)),
        ("down_conv", VaeConv * VAE_MAX_STAGES), ("time_conv", VaeConv * VAE_MAX_STAGES),
        ("mid0", VaeResBlock), ("mid2", VaeResBlock),
        ("attn_gamma", C.c_void_p), ("attn_qk_w", C.c_void_p), ("attn_qk_b", C.c_void_p),
        ("attn_v_w", C.c_void_p), ("attn_v_b", C.c_void_p), ("attn_proj_w", C.c_void_p), ("attn_proj_b", C.c_void_p),
        ("head_gamma", C.c_void_p), ("head_conv", VaeConv),
    ]


class TaehvConvArgs(C.Structure):
    _fields_ = ([(n, C.c_void_p) for n in ("x", "w", "bias", "out", "resid", "out_f32")]
                + [(n, C.c_int32) for n in ("Tout", "H", "W", "Cin", "Cout", "kt", "upsample", "ldw", "ldo", "ldr", "tgrow", "epilogue", "clamp")])


class TaehvLayer(C.Structure):
    _fields_ = [("w", C.c_void_p), ("bias", C.c_void_p)] + [(n, C.c_int32) for n in ("cin", "cout", "kt", "ldw")]


class TaehvModel(C.Structure):
    _fields_ = [("z_dim", C.c_int32), ("in_conv", TaehvLayer), ("block", ((TaehvLayer * 3) * TAEHV_BLOCKS) * TAEHV_STAGES),
                ("exit_conv", TaehvLayer * TAEHV_STAGES), ("tgrow", C.c_int32 * TAEHV_STAGES), ("head", TaehvLayer)]


class TaehvDownConvArgs(C.Structure):
    _fields_ = ([(n, C.c_void_p) for n in ("x", "w", "out")]
                + [(n, C.c_int32) for n in ("Tout", "H", "W", "Cin", "Cout", "kt", "ldw", "ldo")])


class TaehvEncoder(C.Structure):
    _fields_ = [("stem", TaehvLayer), ("down", TaehvLayer * TAEHV_STAGES), ("block", ((TaehvLayer * 3) * TAEHV_BLOCKS) * TAEHV_STAGES),
                ("head", TaehvLayer)]


class PoseRenderArgs(C.Structure):
    _fields_ = ([("keypoints", C.c_void_p), ("out", C.c_void_p)]
                + [(n, C.c_int32) for n in ("F", "P", "H", "W", "layout", "dtype", "normalized")]
                + [("score_threshold", C.c_float)])


class PoseRetargetArgs(C.Structure):
    _fields_ = ([(n, C.c_void_p) for n in ("src", "first", "ref", "out")]
                + [("src0", C.c_int64), ("out0", C.c_int64)]
                + [(n, C.c_int32) for n in ("n_src", "n_out", "people", "ref_people", "num", "den")]
                + [(n, C.c_float) for n in ("src_sx", "src_sy", "ref_sx", "ref_sy", "score_threshold")]
                + [("align", C.c_int32)])


class PoseSmoothArgs(C.Structure):
    _fields_ = ([(n, C.c_void_p) for n in ("src", "out", "state")]
                + [("n", C.c_int32), ("people", C.c_int32)]
                + [(n, C.c_float) for n in ("period", "min_cutoff", "beta", "kd", "score_threshold")]
                + [("max_gap", C.c_int32)])


class PoseTrackArgs(C.Structure):
    _fields_ = ([(n, C.c_void_p) for n in ("src", "out", "ids", "state", "assign")]
                + [(n, C.c_int32) for n in ("n", "people", "slots", "min_points", "min_common", "max_age")]
                + [(n, C.c_float) for n in ("gate2", "score_threshold")])


class PoseBoxesArgs(C.Structure):
    _fields_ = ([(n, C.c_void_p) for n in ("head", "boxes", "count", "scratch")]
                + [(n, C.c_int32) for n in ("F", "A", "C", "P", "in_h", "in_w", "n_strides")]
                + [("strides", C.c_int32 * POSE_BOXES_MAX_STRIDES)]
                + [("class_index", C.c_int32), ("decoded", C.c_int32)]
                + [(n, C.c_float) for n in ("ratio", "score_threshold", "iou_threshold")])


class PoseCropArgs(C.Structure):
    _fields_ = ([(n, C.c_void_p) for n in ("frames", "boxes", "count", "out")]
                + [(n, C.c_int32) for n in ("F", "P", "H", "W", "layout", "out_h", "out_w", "dtype", "bgr")]
                + [("padding", C.c_float), ("mean", C.c_float * 3), ("std", C.c_float * 3)])


class PoseSimccArgs(C.Structure):
    _fields_ = ([(n, C.c_void_p) for n in ("simcc_x", "simcc_y", "boxes", "count", "out", "order")]
                + [(n, C.c_int32) for n in ("F", "P", "H", "W", "Wx", "Wy", "dtype", "out_h", "out_w", "normalized")]
                + [(n, C.c_float) for n in ("padding", "split_ratio", "neck_threshold")])


class PoseConvArgs(C.Structure):
    _fields_ = ([(n, C.c_void_p) for n in ("x", "w", "bias", "out")]
                + [(n, C.c_int32) for n in ("T", "H", "W", "Cin", "Cout", "kt", "stride_t", "stride_s", "ldw", "ldo", "silu")])


class PoseWindow(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("x_t0", "t_end", "closed", "t_out0", "n_out")]


class PosePushPlan(C.Structure):
    _fields_ = [("first", C.c_int32 * (POSE_CONVS + 1)), ("count", C.c_int32 * (POSE_CONVS + 1))]


class PoseLayer(C.Structure):
    _fields_ = [("w", C.c_void_p), ("bias", C.c_void_p)] + [(n, C.c_int32) for n in ("cin", "cout", "kt", "stride_t", "stride_s", "ldw", "silu")]


class PoseModel(C.Structure):
    _fields_ = [("conv", PoseLayer * POSE_CONVS), ("embed_w", C.c_void_p), ("embed_b", C.c_void_p), ("pose_dim", C.c_int32),
                ("ref_conv", PoseLayer * POSE_CONVS)]


class T5Layer(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("norm1_w", "qk_w", "v_w", "o_w", "norm2_w", "gate_w", "fc1_w", "fc2_w", "pos_emb")]


class T5Model(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("vocab", "dim", "dim_attn", "dim_ffn", "num_heads", "num_layers", "num_buckets")]
                + [("eps", C.c_float), ("token_embedding", C.c_void_p), ("layers_host", C.POINTER(T5Layer)),
                   ("final_norm_w", C.c_void_p)])


class ClipLayer(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("norm1_w", "norm1_b", "qkv_w", "qkv_b", "proj_w", "proj_b", "norm2_w", "norm2_b",
                                          "fc1_w", "fc1_b", "fc2_w", "fc2_b")]


class ClipModel(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("image_size", "patch", "dim", "heads", "mlp_dim", "layers_built")]
                + [("eps", C.c_float)]
                + [(n, C.c_void_p) for n in ("patch_w", "cls", "pos", "pre_norm_w", "pre_norm_b")]
                + [("layers_host", C.POINTER(ClipLayer))])


# name -> (restype, argtypes); every symbol include/sf_hip.h declares
_vp, _i, _i64, _f, _sz = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_size_t
SIGNATURES = {
    "sf_abi_version": (C.c_int, []),
    "sf_last_error": (C.c_char_p, []),
    "sf_gemm_bf16": (C.c_int, [C.POINTER(GemmArgs), _vp]),
    "sf_small_linear": (C.c_int, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "sf_quantize_fp8": (C.c_int, [_vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    "sf_gemm_fp8": (C.c_int, [C.POINTER(GemmArgs), _vp, _i, _vp, _vp]),
    "sf_small_linear_fp8": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "sf_sinusoid_embedding": (C.c_int, [_vp, _i, _vp, _i, _i, _vp]),
    "sf_layernorm_modulate": (C.c_int, [_vp, _vp, _i, _i, _f, _vp, _vp, _vp, _vp, _i64, _i, _vp]),
    "sf_layernorm_affine": (C.c_int, [_vp, _vp, _vp, _vp, _i, _i, _f, _vp]),
    "sf_rmsnorm": (C.c_int, [_vp, _i, _vp, _vp, _i, _i, _i, _f, _vp]),
    "sf_qkv_norm_rope_cache": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i64,
                                         _i, _i, _f, _vp]),
    "sf_kv_evict": (C.c_int, [_vp, _i, _i64, _i, _i, _i, _i, _vp, _sz, _vp]),
    "sf_kv_rope_shift": (C.c_int, [_vp, _i, _i64, _i, _i64, _i64, _vp, _vp, _i, _vp]),
    "sf_attention": (C.c_int, [C.POINTER(AttentionArgs), _vp]),
    "sf_cross_fold_scan": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), _i, _i, _i, _i, _vp, _vp, _vp]),
    "sf_patchify": (C.c_int, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "sf_unpatchify_x0": (C.c_int, [_vp, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "sf_add_noise": (C.c_int, [_vp, _vp, _vp, _i, _vp, _vp, _i, _vp, _i, _i64, _vp]),
    "sf_lincomb_bf16": (C.c_int, [_vp, C.POINTER(C.c_void_p), C.POINTER(C.c_float), _i, _i64, _vp]),
    "sf_dit_workspace_bytes": (C.c_size_t, [C.POINTER(Model), C.POINTER(I2VModel), _i, _i, _i, _i, _i]),
    "sf_dit_forward": (C.c_int, [C.POINTER(Model), C.POINTER(ForwardCall), _vp]),
    "sf_patchify_i2v": (C.c_int, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i64, _i64, _i64, _vp]),
    "sf_layernorm_rows": (C.c_int, [_vp, _vp, _vp, _vp, _i, _i, _f, _vp]),
    "sf_i2v_assemble_y": (C.c_int, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i64, _i64, _i, _vp]),
    "sf_conv_igemm": (C.c_int, [C.POINTER(ConvArgs), _vp]),
    "sf_conv_pick_nt": (C.c_int, [_i]),
    "sf_rmsnorm_silu_cl": (C.c_int, [_vp, _vp, _vp, _i64, _i, _i, _vp]),
    "sf_softmax_rows": (C.c_int, [_vp, _i64, _vp, _i64, _i, _i, _i, _f, _vp]),
    "sf_vae_prepare_latent": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "sf_vae_state_bytes": (C.c_size_t, [C.POINTER(VaeModel), _i, _i, _i]),
    "sf_vae_scratch_bytes": (C.c_size_t, [C.POINTER(VaeModel), _i, _i, _i]),
    "sf_vae_reset": (C.c_int, [C.POINTER(VaeModel), _vp, _sz, _i, _i, _i, _vp]),
    "sf_vae_decode_frames": (C.c_int, [C.POINTER(VaeModel), _vp, _sz, _vp, _sz, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "sf_vae_prepare_pixels": (C.c_int, [_vp, _i, _i64, _vp, _i, _i, _i, _i, _vp]),
    "sf_vae_finish_latent": (C.c_int, [_vp, _i, _i, _vp, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "sf_vae_encode_state_bytes": (C.c_size_t, [C.POINTER(VaeEncoder), _i, _i, _i]),
    "sf_vae_encode_scratch_bytes": (C.c_size_t, [C.POINTER(VaeEncoder), _i, _i, _i]),
    "sf_vae_encode_reset": (C.c_int, [C.POINTER(VaeEncoder), _vp, _sz, _i, _i, _i, _vp]),
    "sf_vae_encode_frames": (C.c_int, [C.POINTER(VaeEncoder), _vp, _sz, _vp, _sz, _vp, _i, _i64, _i, _i, _i, _i, _i, _i, _i, _vp,
                                       _vp]),
    "sf_taehv_conv": (C.c_int, [C.POINTER(TaehvConvArgs), _vp]),
    "sf_taehv_pick_nt": (C.c_int, [_i]),
    "sf_taehv_prepare_latent": (C.c_int, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "sf_taehv_state_bytes": (C.c_size_t, [C.POINTER(TaehvModel), _i, _i]),
    "sf_taehv_scratch_bytes": (C.c_size_t, [C.POINTER(TaehvModel), _i, _i, _i]),
    "sf_taehv_reset": (C.c_int, [C.POINTER(TaehvModel), _vp, _sz, _i, _i, _vp]),
    "sf_taehv_decode_frames": (C.c_int, [C.POINTER(TaehvModel), _vp, _sz, _vp, _sz, _vp, _i, _i, _i, _i, _vp, _vp]),
    "sf_taehv_encode_stem": (C.c_int, [_vp, _i, _i64, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "sf_taehv_down_conv": (C.c_int, [C.POINTER(TaehvDownConvArgs), _vp]),
    "sf_taehv_encode_state_bytes": (C.c_size_t, [C.POINTER(TaehvEncoder), _i, _i]),
    "sf_taehv_encode_scratch_bytes": (C.c_size_t, [C.POINTER(TaehvEncoder), _i, _i, _i]),
    "sf_taehv_encode_reset": (C.c_int, [C.POINTER(TaehvEncoder), _vp, _sz, _i, _i, _vp]),
    "sf_taehv_encode_frames": (C.c_int, [C.POINTER(TaehvEncoder), _vp, _sz, _vp, _sz, _vp, _i, _i64, _i, _i, _i, _i, _vp, _vp]),
    "sf_pose_out_size": (C.c_int, [_i, _i, _i]),
    "sf_pose_conv": (C.c_int, [C.POINTER(PoseConvArgs), _vp]),
    "sf_pose_conv_window": (C.c_int, [C.POINTER(PoseConvArgs), C.POINTER(PoseWindow), _vp]),
    "sf_pose_prepare": (C.c_int, [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "sf_pose_patch_embed": (C.c_int, [_vp, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp]),
    "sf_pose_scratch_bytes": (C.c_size_t, [C.POINTER(PoseModel), _i, _i, _i]),
    "sf_pose_embed": (C.c_int, [C.POINTER(PoseModel), _vp, _i, _i, _i, _i, _vp, _sz, _vp, _i64, _vp]),
    "sf_pose_embed_ref": (C.c_int, [C.POINTER(PoseModel), _vp, _i, _i, _i, _vp, _sz, _vp, _vp]),
    "sf_pose_stream_plan": (C.c_int, [_i, _i, _i, C.POINTER(PosePushPlan)]),
    "sf_pose_stream_state_bytes": (C.c_size_t, [C.POINTER(PoseModel), _i, _i]),
    "sf_pose_stream_scratch_bytes": (C.c_size_t, [C.POINTER(PoseModel), _i, _i, _i]),
    "sf_pose_stream_push": (C.c_int, [C.POINTER(PoseModel), _vp, _i, _vp, _i, _i, _i, _i, _i, _vp, _sz, _vp, _i64, C.POINTER(C.c_int32), _vp]),
    "sf_jpeg_workspace_bytes": (C.c_size_t, [_i, _i, _i, _i, _i]),
    "sf_jpeg_transform": (C.c_int, [_vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "sf_jpeg_entropy": (C.c_int, [_vp, _i, _i, _i, _i, _i, _i, _vp, _sz, _vp, _sz, _vp, _vp, _vp]),
    "sf_jpeg_encode_frames": (C.c_int, [_vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _sz, _vp, _sz, _vp, _vp, _vp]),
    "sf_jpeg_decode_workspace_bytes": (C.c_size_t, [_i, _i, _i, _i, _i]),
    "sf_jpeg_decode_entropy": (C.c_int, [_vp, _sz, _i, _i, _i, _i, _i, _vp, _sz, _vp, _vp, _vp]),
    "sf_jpeg_decode_pixels": (C.c_int, [_vp, _vp, _sz, _vp, _i, _i, _i, _i, _vp, _sz, _vp, _i, _i, _vp]),
    "sf_jpeg_decode_frames": (C.c_int, [_vp, _sz, _vp, _i, _i, _i, _i, _i, _vp, _sz, _vp, _i, _i, _vp, _vp]),
    "sf_resize_kernel_size": (C.c_int, [_i, _i, _i]),
    "sf_resize_frames": (C.c_int, [_vp, _i, _i, _i, _i, C.POINTER(C.c_int32), _vp, _vp, _vp, _vp, _i, _vp, _i, _i, _i, _i, _vp]),
    "sf_yuv_frame_bytes": (C.c_size_t, [_i, _i, _i]),
    "sf_yuv_decode_frames": (C.c_int, [_vp, _i, _i, _i, _i, C.POINTER(C.c_int32), _i, _vp, _i, _i, _vp]),
    "sf_yuv_encode_frames": (C.c_int, [_vp, _i, _i, _i, _i, _i, C.POINTER(C.c_int32), _vp, _i, _vp]),
    "sf_pose_render_frames": (C.c_int, [C.POINTER(PoseRenderArgs), _vp]),
    "sf_pose_retarget_frames": (C.c_int, [C.POINTER(PoseRetargetArgs), _vp]),
    "sf_pose_retarget_plan": (C.c_int, [_i64, _i64, _i, _i, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "sf_pose_smooth_frames": (C.c_int, [C.POINTER(PoseSmoothArgs), _vp]),
    "sf_pose_smooth_state_bytes": (C.c_size_t, [_i]),
    "sf_pose_track_frames": (C.c_int, [C.POINTER(PoseTrackArgs), _vp]),
    "sf_pose_track_state_bytes": (C.c_size_t, [_i]),
    "sf_pose_boxes_decode": (C.c_int, [C.POINTER(PoseBoxesArgs), _vp]),
    "sf_pose_boxes_scratch_bytes": (C.c_size_t, [_i, _i]),
    "sf_pose_crop_people": (C.c_int, [C.POINTER(PoseCropArgs), _vp]),
    "sf_pose_simcc_decode": (C.c_int, [C.POINTER(PoseSimccArgs), _vp]),
    "sf_embedding_gather": (C.c_int, [_vp, _vp, _vp, _i, _i, _i, _vp]),
    "sf_t5_softmax_bias": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "sf_mul_bf16": (C.c_int, [_vp, _vp, _vp, _i64, _vp]),
    "sf_zero_masked_rows": (C.c_int, [_vp, _vp, _i, _i, _vp]),
    "sf_t5_workspace_bytes": (C.c_size_t, [C.POINTER(T5Model), _i, _i]),
    "sf_t5_encode": (C.c_int, [C.POINTER(T5Model), _vp, _vp, _vp, _i, _i, _vp, _vp, _sz, _vp]),
    "sf_clip_preprocess": (C.c_int, [_vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "sf_clip_embed_norm": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _f, _vp]),
    "sf_clip_add_layernorm": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i, _i, _f, _vp]),
    "sf_clip_attention": (C.c_int, [_vp, _vp, _i, _i, _i, _vp]),
    "sf_clip_gelu": (C.c_int, [_vp, _vp, _i64, _vp]),
    "sf_clip_workspace_bytes": (C.c_size_t, [C.POINTER(ClipModel), _i]),
    "sf_clip_encode": (C.c_int, [C.POINTER(ClipModel), _vp, _i, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "sf_probe_mfma": (C.c_int, [_i, _i, _i, _vp, _vp, C.POINTER(C.c_double), _vp]),
    "sf_probe_copy": (C.c_int, [_vp, _vp, _sz, _vp]),
}

_lib: Optional[C.CDLL] = None


class SfHipError(RuntimeError):
    pass


def build(verbose: bool = False) -> str:
    """Compile every HIP source for gfx950 into csrc/libsf_hip.so (hipcc cross-compiles without
    a GPU)."""
    cmd = ["make", "-C", CSRC, "-j8"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if verbose or res.returncode != 0:
        print(res.stdout)
        print(res.stderr)
    if res.returncode != 0:
        raise SfHipError(f"building {LIB_PATH} failed (exit {res.returncode})")
    return LIB_PATH


def lib() -> C.CDLL:
    """The loaded C-ABI library; raises (never falls back) when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SfHipError(
            f"{LIB_PATH} not found: the HIP extension is not built. Run "
            f"`python -c 'import __graft_entry__ as g; g.build()'` (or `make -C {CSRC}`). "
            "There is no CPU/eager fallback for this path.")
    handle = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(handle, name)  # AttributeError if the library lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    ver = handle.sf_abi_version()
    if ver != ABI_VERSION:
        raise SfHipError(f"{LIB_PATH}: ABI version {ver}, expected {ABI_VERSION}; rebuild")
    _lib = handle
    return handle


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = lib().sf_last_error()
        raise SfHipError(f"{what or 'sf_hip'} failed (rc={rc}): {msg.decode() if msg else '?'}")
