"""MI355X-native implementation of Self-Forcing's chunk-wise autoregressive denoising
rollout (the `WanDiffusionWrapper` / `CausalInferencePipeline` hot path).

Host code is Python; all device work is hand-written HIP for gfx950 behind the C-ABI
declared in `include/sf_hip.h` (built into `self-forcing_amd/csrc/libsf_hip.so`).
There is no CPU or eager-PyTorch fallback: the compute entry points raise when the
library has not been built.
"""
from .weights import (WanShape, WAN_1_3B, WAN_14B, WAN_REDUCED, WAN_I2V_14B, WAN_I2V_REDUCED, NAMED_SHAPES, synth_state_dict,  # noqa: F401
                      param_shapes, merge_lora, strip_prefix, synth_lora_state_dict, apply_lora_file,
                      load_lora_file, lora_target_linears)
from .kvcache import CachePlan, plan_cache_update  # noqa: F401
from .scheduler import FlowMatchScheduler  # noqa: F401
from .wan_wrapper import WanDiffusionWrapper  # noqa: F401
from .pipeline import CausalInferencePipeline  # noqa: F401
from .harness import SyntheticTextEncoder, FixedTextEncoder, IdentityVAE  # noqa: F401
from .concurrent import RolloutPool  # noqa: F401
from .vae_weights import (VaeShape, WAN_VAE, VAE_REDUCED, synth_vae_state_dict, vae_param_shapes,  # noqa: F401
                          encoder_param_shapes, vae_encode_flops)
from .vae import WanVAEWrapper, WanVAEDecoder, WanVAEEncoder, repack_conv  # noqa: F401
from .taehv_weights import taehv_param_shapes, synth_taehv_state_dict, taehv_decode_flops  # noqa: F401
from .taehv_weights import taehv_encoder_param_shapes, synth_taehv_encoder_state_dict, taehv_encode_flops  # noqa: F401
from .taehv import TAEHVWrapper, TAEHVDecoder, TAEHVEncoder  # noqa: F401
from . import taehv_weights  # noqa: F401
from .pose_weights import pose_param_shapes, synth_pose_state_dict, pose_plan, pose_embed_flops, pose_embed_bytes  # noqa: F401
from .pose import PoseEmbedder, PoseStream  # noqa: F401
from . import pose_weights  # noqa: F401
from .jpeg import JpegDecoder, JpegEncoder  # noqa: F401
from . import jpeg_reference, mjpeg  # noqa: F401
from .resize import FrameResizer  # noqa: F401
from . import resize, resize_reference  # noqa: F401
from .yuv import YuvDecoder, YuvEncoder  # noqa: F401
from . import yuv, yuv_reference, y4m  # noqa: F401
from .pose_keypoints import KeypointChain  # noqa: F401
from .pose_render import PoseRenderer  # noqa: F401
from . import pose_keypoints, pose_render, pose_render_reference  # noqa: F401
from .pose_retarget import PoseRetargeter, PoseRetargetStream  # noqa: F401
from . import pose_retarget, pose_retarget_reference  # noqa: F401
from .pose_smooth import PoseSmoother, PoseSmoothStream  # noqa: F401
from . import pose_smooth, pose_smooth_reference  # noqa: F401
from .pose_track import PoseTracker, PoseTrackStream  # noqa: F401
from . import pose_track, pose_track_reference  # noqa: F401
from .pose_estimate import PoseEstimator, keypoint_feed  # noqa: F401
from . import pose_estimate, pose_estimate_reference  # noqa: F401
from .t5_weights import T5Shape, UMT5_XXL, T5_REDUCED, synth_t5_state_dict, t5_param_shapes  # noqa: F401
from .text_encoder import WanTextEncoder, UMT5Encoder, relative_position_buckets  # noqa: F401
from .clip_weights import ClipVisionShape, CLIP_VIT_H_14, CLIP_REDUCED, clip_param_shapes, synth_clip_state_dict  # noqa: F401
from .clip import CLIPModel, CLIPVisionEncoder  # noqa: F401
from . import clip_weights, clip_reference, i2v_reference  # noqa: F401
from . import unipc  # noqa: F401
from .diffusion_pipeline import CausalDiffusionInferencePipeline  # noqa: F401
from .i2v_condition import I2VConditioner  # noqa: F401
from .unipc import FlowUniPCMultistepScheduler  # noqa: F401
from . import ops, _lib, torch_ops, text_encoder, distributed  # noqa: F401

__all__ = ["WanShape", "WAN_1_3B", "WAN_14B", "WAN_REDUCED", "NAMED_SHAPES", "synth_state_dict",
           "param_shapes", "merge_lora", "strip_prefix", "synth_lora_state_dict", "apply_lora_file", "load_lora_file",
           "lora_target_linears", "CachePlan", "plan_cache_update",
           "FlowMatchScheduler", "WanDiffusionWrapper", "CausalInferencePipeline",
           "SyntheticTextEncoder", "FixedTextEncoder", "IdentityVAE", "RolloutPool", "ops", "torch_ops",
           "VaeShape", "WAN_VAE", "VAE_REDUCED", "synth_vae_state_dict", "vae_param_shapes", "WanVAEWrapper",
           "TAEHVWrapper", "TAEHVDecoder", "taehv_param_shapes", "synth_taehv_state_dict", "taehv_decode_flops",
           "TAEHVEncoder", "taehv_encoder_param_shapes", "synth_taehv_encoder_state_dict", "taehv_encode_flops",
           "JpegEncoder", "JpegDecoder", "jpeg_reference", "mjpeg", "FrameResizer", "resize_reference", "YuvDecoder", "YuvEncoder", "yuv", "yuv_reference", "y4m", "KeypointChain", "pose_keypoints", "PoseRenderer", "pose_render", "pose_render_reference", "PoseRetargeter", "PoseRetargetStream", "pose_retarget", "pose_retarget_reference", "PoseSmoother", "PoseSmoothStream", "pose_smooth", "pose_smooth_reference", "PoseTracker", "PoseTrackStream", "pose_track", "pose_track_reference", "PoseEstimator", "keypoint_feed", "pose_estimate", "pose_estimate_reference", "PoseEmbedder", "PoseStream", "pose_param_shapes", "synth_pose_state_dict", "pose_plan", "pose_embed_flops", "pose_embed_bytes",
           "WanVAEDecoder", "repack_conv", "T5Shape", "UMT5_XXL", "T5_REDUCED", "synth_t5_state_dict", "t5_param_shapes",
           "WanTextEncoder", "UMT5Encoder", "relative_position_buckets", "FlowUniPCMultistepScheduler", "CausalDiffusionInferencePipeline",
           "ClipVisionShape", "CLIP_VIT_H_14", "CLIP_REDUCED", "clip_param_shapes", "synth_clip_state_dict", "CLIPModel", "CLIPVisionEncoder",
           "clip_weights", "clip_reference", "WAN_I2V_14B", "WAN_I2V_REDUCED", "i2v_reference", "I2VConditioner"]
