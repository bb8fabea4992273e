#!/usr/bin/env python
"""Batch generation driver for the hot path (counterpart of the reference's inference.py:39-196,
written fresh: the fork's own CLI passes keyword arguments `CausalInferencePipeline.inference`
does not accept).

    python generate.py --config_path cfg.yaml --data_path prompts.txt --output_folder out [--random_init_seed 0]
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 generate.py ...

Keeps the reference's semantics: OmegaConf-style merge of a default config under the run config,
`DistributedSampler(shuffle=False, drop_last=True)` prompt sharding (rank r takes r, r+W, ...),
seed = `--seed + rank`, noise `[num_samples, num_output_frames, 16, 60, 104]` bf16 drawn per prompt,
one barrier after set-up.  It writes LATENTS (`<idx>-<sample>.pt`) and, when a VAE is given
(`--vae_path Wan2.1_VAE.pth`, loaded with weights_only=True, or `--vae_random_init_seed N`; or the TAEHV tiny
decoder for a fast preview, `--taehv_path taew2_1.pth` / `--taehv_random_init_seed N`), the decoded
video as a uint8 tensor [T, H, W, 3] (`<idx>-<sample>.video.pt`: what the reference hands to
`write_video`, inference.py:186-196).  `--video_format mjpeg` writes a file that plays instead: `<idx>-<sample>.avi`,
Motion-JPEG at 16 frames/s (the reference's `write_video` rate), every frame encoded on the GPU by `JpegEncoder`
(`--jpeg_quality`, `--jpeg_subsampling`) with the demo's truncation (demo.py:166-167) of the decoder's [-1, 1] output,
recovered from the returned [0, 1] video as 2 v - 1.  The umT5 encoder is
outside this path, so embeddings are synthetic unless `--prompt_embeds` (a .pt dict prompt -> [L, 4096]
tensor) is given.  A config WITHOUT `denoising_step_list` selects the multi-step classifier-free-guidance sampler
(`CausalDiffusionInferencePipeline`), as inference.py:62-67 does; it needs `num_train_timestep`, `timestep_shift`,
`guidance_scale` and `negative_prompt`.

`--pose_path` drives the generation with a pose clip, under either pipeline: a `.pt` (dict) or `.npy` (pickled dict)
holding `dwpose_data` [3, F, H, W] and `random_ref_dwpose` [H, W, 3] in 0..255, embedded on the GPU by `PoseEmbedder`
with the weights of `--pose_weights_path` (a file with `dwpose_embedding.*` / `randomref_embedding_pose.*` tensors) or
`--pose_random_init_seed N`.  `--pose_path clip.avi` takes the clip as a Motion-JPEG AVI instead (what `--video_format mjpeg`
writes, or a skeleton renderer's output), with `--ref_pose_path ref.jpg` as `random_ref_dwpose`: the frames are read by
`mjpeg.read_avi` and decoded on the GPU by `JpegDecoder`, with no host decode.  `--pose_resize stretch|cover` resizes both on
the GPU to the output size (`FrameResizer`: Pillow's antialiased bilinear, bit for bit), so a clip of any size can drive the
generation; the default `none` takes them as they are.  `--pose_path clip.npz --ref_pose_path ref.npz` takes KEYPOINTS instead of
frames: the array `keypoints` (a `.npy` file holds the array itself), float [F, P, 134, 3] or [F, 134, 3] = (x, y, score) in DWPose's
whole-body order, in [0, 1] (`--pose_pixel_coords`: in pixels of the output); the ref file holds one frame, [P, 134, 3] or [134, 3].
`PoseRenderer` draws them on the GPU at the output size, so `--pose_resize` does not apply to them.
`--pose_align` first gives the driving skeleton the reference person's proportions and position, `--pose_fps N[/D]` resamples keypoints
recorded at another frame rate to the pipeline's 16 frames/s, and `--pose_source_size HxW` names the size of the video they come from
where its aspect differs from the output's: all three run on the GPU in `PoseRetargeter`, between the upload and the renderer.
`--pose_smooth MIN_CUTOFF[,BETA[,D_CUTOFF]]` steadies jittery keypoints with a One-Euro filter per point and `--pose_hold N` bridges up to N
frames in which a point is missing, both on the GPU in `PoseSmoother`, in front of the retargeter; the reference file is never smoothed.
`--pose_track [SLOTS]` first puts each person of a multi-person keypoint file into one stable slot across frames (`PoseTracker`, on the GPU,
in front of the smoother), for detectors that list the people of a frame in detection order; `--pose_track_gate G` is how far a person may
move between matches, in diagonals of its own body box, and `--pose_track_age N` how many frames a slot waits for its person.  The
reference file is never tracked.
`--open_length` (few-step configs with a rolling KV cache, `local_attn_size` in `model_kwargs`) lets the pose clip decide the length
instead of `--num_output_frames`: the clip goes piece by piece into `CausalInferencePipeline.open_session`, which generates until it
ends -- past the 1024 frames of the RoPE tables too -- and the files are written as usual (`pt` and `mjpeg`).

`--i2v` (inference.py:83-90, 136-149) reads `--data_path` as a TextImagePairDataset directory -- one
`target_crop_info_<ratio>.json` listing `file_name` / `caption` entries, images under `<ratio>/` --, encodes each
image with the VAE encoder (so it needs a VAE with encoder weights: `--vae_path`, `--vae_random_init_seed`, a
`--taehv_path` checkpoint that holds the `encoder.*` tensors, as taew2_1.pth does, or `--taehv_random_init_seed`) as the
first latent frame and draws noise for the `num_output_frames - 1` frames after it.  Single process only, as in the
reference.

`--input_image PATH` is the other image conditioning: the i2v MODEL TYPE (a generator whose shape says so, selected by
`model_name: Wan2.1-I2V-14B` in the config's `model_kwargs`), under either pipeline.  The image is resized to the output
size and handed to the pipeline's `inference(input_image=...)`, which encodes it with the CLIP image encoder (`--clip_path`
checkpoint or `--clip_random_init_seed N`) and the VAE encoder (the Wan VAE with encoder weights: `--vae_path` or
`--vae_random_init_seed`) into the generator's `clip_feature` and `y` -- the few-step pipeline chunk by chunk, as the
rollout needs it.  `--i2v` stays "first frame as initial latent" of a t2v model.
"""
import argparse
import glob
import json
import os
import re
import sys

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
POSE_TARGET_FPS = 16    # the generator's timeline: what --pose_fps is resampled to
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import self_forcing_amd as sfa  # noqa: E402
from self_forcing_amd.config import is_few_step, load_config  # noqa: E402
from self_forcing_amd.sharding import read_prompts, shard_indices  # noqa: E402


class TableTextEncoder:
    """prompt -> precomputed embedding (zero padded to text_len)."""

    def __init__(self, table, text_len, text_dim, device):
        self.table, self.text_len, self.text_dim, self.device = table, text_len, text_dim, device

    def __call__(self, text_prompts):
        out = torch.zeros(len(text_prompts), self.text_len, self.text_dim, dtype=torch.bfloat16)
        for i, p in enumerate(text_prompts):
            e = self.table[p].to(torch.bfloat16)
            out[i, :e.shape[0]] = e[:self.text_len]
        return {"prompt_embeds": out.to(self.device)}


def read_image_pairs(data_dir: str, eval_first_n: int = 0):
    """TextImagePairDataset's layout (utils/dataset.py:199-250): [(image path, caption)]."""
    metas = glob.glob(os.path.join(data_dir, "target_crop_info_*.json"))
    if len(metas) != 1:
        raise SystemExit(f"{data_dir}: expected exactly one target_crop_info_*.json, found {len(metas)}")
    ratio = os.path.splitext(os.path.basename(metas[0]))[0].split("_")[-1]
    with open(metas[0]) as f:
        items = json.load(f)
    if eval_first_n > 0:
        items = items[:eval_first_n]
    pairs = [(os.path.join(data_dir, ratio, it["file_name"]), it["caption"]) for it in items]
    for path, _ in pairs:
        if not os.path.exists(path):
            raise SystemExit(f"image not found: {path}")
    return pairs


def load_image(path: str, height: int, width: int) -> torch.Tensor:
    """Resize((height, width)) bilinear, ToTensor, Normalize([0.5], [0.5]) (inference.py:84-88) -> [3, H, W] in [-1, 1]."""
    import numpy as np
    from PIL import Image
    img = Image.open(path).convert("RGB").resize((width, height), Image.BILINEAR)
    x = torch.from_numpy(np.asarray(img, dtype=np.uint8).copy()).permute(2, 0, 1).float() / 255.0
    return (x - 0.5) / 0.5


def load_pose(path: str):
    """(dwpose_data [3, F, H, W], random_ref_dwpose [H, W, 3]) from a .pt dict or a .npy holding a pickled dict."""
    if path.endswith(".npy"):
        import numpy as np
        d = np.load(path, allow_pickle=True).item()
    else:
        d = torch.load(path, map_location="cpu", weights_only=True)
    missing = [k for k in ("dwpose_data", "random_ref_dwpose") if k not in d]
    if missing:
        raise SystemExit(f"{path}: no {' / '.join(missing)} in the pose file")
    return tuple(torch.as_tensor(d[k]) for k in ("dwpose_data", "random_ref_dwpose"))


def pose_file_kind(path: str) -> str:
    """"mjpeg" (.avi), "y4m" (.y4m; a FIFO or /dev/stdin is one with --pose_format y4m), "keypoints" (.npz, or a .npy that holds a plain array) or "dict" (.pt, or a .npy that holds a pickled dict)."""
    low = path.lower()
    if low.endswith(".avi"):
        return "mjpeg"
    if low.endswith(".y4m"):
        return "y4m"
    if low.endswith(".npz"):
        return "keypoints"
    if low.endswith(".npy"):
        import numpy as np
        try:
            np.load(path, mmap_mode="r", allow_pickle=False)
        except (ValueError, EOFError):                             # an object array: the pickled dict (or no .npy file at all)
            return "dict"
        return "keypoints"
    return "dict"


def read_keypoints(path: str, one_frame: bool = False):
    """float32 [F, P, 134, 3] from the array `keypoints` of a .npz or the array a .npy holds; `one_frame`: the file holds a single
    frame, [P, 134, 3] or [134, 3] (or [1, P, 134, 3])."""
    import numpy as np
    d = np.load(path, allow_pickle=False)
    if hasattr(d, "files"):
        if "keypoints" not in d.files:
            raise SystemExit(f"{path}: no array 'keypoints' in the file (it holds {', '.join(d.files) or 'nothing'})")
        d = d["keypoints"]
    k = np.asarray(d, dtype=np.float32)
    if one_frame and k.ndim in (2, 3):
        k = k.reshape((1,) * (4 - k.ndim) + k.shape)
    try:
        frames, people = sfa.pose_render_reference.check_keypoints_shape(k.shape)
    except ValueError as e:
        raise SystemExit(f"{path}: {e}")
    if one_frame and frames != 1:
        raise SystemExit(f"{path}: the reference pose is one frame of keypoints, the file holds {frames}")
    return k.reshape(frames, people, 134, 3)


def load_pose_keypoints(clip_path: str, ref_path: str, device, size, normalized: bool = True, align: bool = False, source_fps=None, source_size=None,
                        smooth=None, hold: int = 0, track=None):
    """(dwpose_data uint8 [3, F, H, W], random_ref_dwpose uint8 [H, W, 3]) on `device`, drawn there from two keypoint files.
    With `track` = a dict of `PoseTracker.track` arguments (slots, gate, max_age; an empty one for the defaults) the clip first
    goes through `PoseTracker`.  With `smooth` = (min_cutoff[, beta[, d_cutoff]]) or `hold` > 0 it then goes through `PoseSmoother` at `source_fps`
    (POSE_TARGET_FPS when none is given); with `align`, a `source_fps` or a `source_size` it then goes through
    `PoseRetargeter` (to the pipeline's POSE_TARGET_FPS).  The reference pose is drawn from the reference keypoints as they
    are: it is neither tracked, smoothed nor moved."""
    renderer = sfa.PoseRenderer(device=device)
    clip, ref = read_keypoints(clip_path), read_keypoints(ref_path, one_frame=True)
    ref_frame = renderer.render(ref, size, "hwc", normalized=normalized)[0]
    fps = POSE_TARGET_FPS if source_fps is None else source_fps
    stages = {}
    try:
        if track is not None:
            stages["tracker"] = sfa.PoseTracker(device=device).open_stream(**track)
        if smooth is not None or hold:
            stages["smoother"] = sfa.PoseSmoother(device=device).open_stream(fps, *(smooth or ()), max_gap=hold)
        if align or source_fps is not None or source_size is not None:
            stages["retargeter"] = sfa.PoseRetargeter(device=device).open_stream(ref[0], size, source_fps=fps, target_fps=POSE_TARGET_FPS, align=align,
                                                                                 normalized=normalized, source_size=source_size)
        chain = sfa.KeypointChain(**stages)
        clip = chain.push(clip)
    except ValueError as e:
        raise SystemExit(f"{clip_path}: {e}")
    return renderer.render(clip, size, "pose", normalized=normalized and not chain.in_pixels), ref_frame


def load_pose_mjpeg(clip_path: str, ref_path: str, device, size=None, fit: str = "stretch"):
    """(dwpose_data uint8 [3, F, H, W], random_ref_dwpose uint8 [H, W, 3]) on `device` from an MJPEG AVI and a JPEG file;
    with `size` both are resized to it on the device (antialiased bilinear, Pillow's bits on the decoded samples)."""
    decoder = sfa.JpegDecoder(device=device)
    frames = sfa.mjpeg.read_avi(clip_path)
    if not frames:
        raise SystemExit(f"{clip_path}: no video frames (00dc chunks) in the file")
    with open(ref_path, "rb") as fh:
        ref = fh.read()
    try:
        return decoder.decode(frames, layout="pose", size=size, fit=fit), decoder.decode([ref], layout="hwc", size=size, fit=fit)[0]
    except ValueError as e:
        raise SystemExit(f"{clip_path} / {ref_path}: {e}")


def open_pose_y4m(path: str):
    """A `y4m.Y4mReader` over --pose_path (a file, a FIFO or /dev/stdin), its header read."""
    try:
        return sfa.y4m.Y4mReader(path)
    except ValueError as e:
        raise SystemExit(f"{path}: {e}")


def pose_y4m_feed(reader, decoder, a, size, fit, frames_per_piece=16):
    """The reader's frames as pose pieces uint8 [3, n, H, W] on the device, each read and decoded when it is asked for."""
    return sfa.yuv.frame_feed(reader, decoder, reader.fmt, (reader.height, reader.width), frames_per_piece, "pose", size, a.pose_yuv_matrix or "bt601",
                              reader.range, a.pose_yuv_chroma or "triangle", fit=fit)


def load_pose_ref(ref_path: str, device, size=None, fit: str = "stretch"):
    """random_ref_dwpose uint8 [H, W, 3] on `device` from a JPEG file, resized to `size` if one is given."""
    with open(ref_path, "rb") as fh:
        ref = fh.read()
    try:
        return sfa.JpegDecoder(device=device).decode([ref], layout="hwc", size=size, fit=fit)[0]
    except ValueError as e:
        raise SystemExit(f"{ref_path}: {e}")


def check_pose_flags(ap, a):
    """The parser's checks of the pose flags, each ending in `ap.error`: (the kind of --pose_path as `pose_file_kind` names it, None without
    one; --pose_source_size as (hs, ws); --pose_smooth / --pose_hold as the smoother's tuple; the --pose_track flags as the tracker's dict), each
    None where the flags do not ask for it."""
    retarget_flags = (("--pose_align", a.pose_align), ("--pose_fps", a.pose_fps is not None), ("--pose_source_size", a.pose_source_size is not None))
    smooth_flags = (("--pose_smooth", a.pose_smooth is not None), ("--pose_hold", a.pose_hold is not None))       # they do not retarget
    track_flags = (("--pose_track", a.pose_track is not None), ("--pose_track_gate", a.pose_track_gate is not None),
                   ("--pose_track_age", a.pose_track_age is not None))                                               # nor do these
    pose_kind = pose_source_size = pose_smooth = pose_track = None
    if a.pose_path or a.pose_weights_path or a.pose_random_init_seed is not None:
        if not a.pose_path or (a.pose_weights_path is None) == (a.pose_random_init_seed is None):
            ap.error("pose conditioning needs --pose_path and exactly one of --pose_weights_path / --pose_random_init_seed")
        if not os.path.exists(a.pose_path):
            ap.error(f"--pose_path {a.pose_path}: no such file (a .pt / .npy dict with dwpose_data and random_ref_dwpose; few-step and "
                     "multi-step configs both take it)")
        pose_kind = "y4m" if a.pose_format == "y4m" else pose_file_kind(a.pose_path)
        if a.ref_pose_path and pose_kind == "dict":
            ap.error("--ref_pose_path goes with an MJPEG --pose_path (.avi) or a keypoint one (.npz / .npy array); a .pt / .npy dict holds its own "
                     "random_ref_dwpose")
        if pose_kind == "mjpeg" and not a.ref_pose_path:
            ap.error("--pose_path clip.avi needs --ref_pose_path: the JPEG file that is random_ref_dwpose")
        if pose_kind == "y4m" and not a.ref_pose_path:
            ap.error("--pose_path clip.y4m needs --ref_pose_path: the JPEG file that is random_ref_dwpose")
        if pose_kind != "y4m" and (a.pose_yuv_matrix or a.pose_yuv_chroma):
            ap.error("--pose_yuv_matrix and --pose_yuv_chroma go with a YUV4MPEG2 --pose_path (.y4m, or --pose_format y4m)")
        if pose_kind == "keypoints" and not a.ref_pose_path:
            ap.error("--pose_path with keypoints needs --ref_pose_path: a .npz / .npy with one frame of keypoints, drawn as random_ref_dwpose")
        if pose_kind != "dict" and not os.path.exists(a.ref_pose_path):
            ap.error(f"--ref_pose_path {a.ref_pose_path}: no such file")
        if pose_kind == "keypoints" and pose_file_kind(a.ref_pose_path) != "keypoints":
            ap.error(f"--ref_pose_path {a.ref_pose_path}: keypoints (.npz / .npy array) expected beside a keypoint --pose_path")
        if a.pose_pixel_coords and pose_kind != "keypoints":
            ap.error("--pose_pixel_coords goes with a keypoint --pose_path (.npz / .npy array)")
        for flag, given in retarget_flags + smooth_flags + track_flags:
            if given and pose_kind != "keypoints":
                ap.error(f"{flag} goes with a keypoint --pose_path (.npz / .npy array)")
        if a.pose_fps is not None:
            try:
                sfa.pose_retarget_reference.rate(a.pose_fps, POSE_TARGET_FPS)
            except ValueError as e:
                ap.error(f"--pose_fps {a.pose_fps}: {e}")
        if a.pose_source_size is not None:
            m = re.fullmatch(r"(\d+)x(\d+)", a.pose_source_size)
            if not m or not int(m.group(1)) or not int(m.group(2)):
                ap.error(f"--pose_source_size {a.pose_source_size}: HxW expected, two positive integers, e.g. 720x1280")
            pose_source_size = (int(m.group(1)), int(m.group(2)))
        if a.pose_smooth is not None or a.pose_hold is not None:
            try:
                pose_smooth = () if a.pose_smooth is None else tuple(float(v) for v in a.pose_smooth.split(","))
                if a.pose_smooth is not None and not 1 <= len(pose_smooth) <= 3:
                    raise ValueError("one to three numbers expected")
            except ValueError as e:
                ap.error(f"--pose_smooth {a.pose_smooth}: MIN_CUTOFF[,BETA[,D_CUTOFF]] expected, e.g. 1.0,0.05 ({e})")
            try:
                sfa.pose_smooth_reference.prepare(POSE_TARGET_FPS if a.pose_fps is None else a.pose_fps, *pose_smooth, max_gap=a.pose_hold or 0)
            except ValueError as e:
                ap.error(f"--pose_smooth {a.pose_smooth} --pose_hold {a.pose_hold}: {e}")
        if any(given for _, given in track_flags):
            if a.pose_track is None:
                ap.error("--pose_track_gate and --pose_track_age go with --pose_track")
            try:
                slots = int(a.pose_track) if a.pose_track else None                                                   # "": the people per frame
            except ValueError:
                ap.error(f"--pose_track {a.pose_track}: SLOTS expected, an integer in 1..8")
            pose_track = {name: value for name, value in (("slots", slots), ("gate", a.pose_track_gate), ("max_age", a.pose_track_age))
                          if value is not None}
            try:
                tracked = sfa.pose_track_reference.prepare(**pose_track)
            except ValueError as e:
                ap.error(f"--pose_track {a.pose_track} --pose_track_gate {a.pose_track_gate} --pose_track_age {a.pose_track_age}: {e}")
            if sfa.KeypointChain.bridges_two_people(a.pose_hold or 0, tracked.max_age):
                ap.error(f"--pose_hold {a.pose_hold} exceeds --pose_track_age {tracked.max_age}: a tracker's slot is empty for max_age + 1 frames "
                         f"between two different people, so a longer hold could smooth one person towards another")
    elif a.pose_format != "auto" or a.pose_yuv_matrix or a.pose_yuv_chroma:
        ap.error("--pose_format, --pose_yuv_matrix and --pose_yuv_chroma need --pose_path")
    elif a.ref_pose_path:
        ap.error("--ref_pose_path needs --pose_path clip.avi or keypoints (.npz / .npy array)")
    elif a.pose_pixel_coords:
        ap.error("--pose_pixel_coords needs a keypoint --pose_path")
    else:
        for flag, given in retarget_flags + smooth_flags + track_flags:
            if given:
                ap.error(f"{flag} needs a keypoint --pose_path")
    return pose_kind, pose_source_size, pose_smooth, pose_track


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config_path", required=True)
    ap.add_argument("--default_config_path", default=None)
    ap.add_argument("--checkpoint_path", default=None, help=".pt with 'generator' / 'generator_ema' state dicts, or a .safetensors file")
    ap.add_argument("--use_ema", action="store_true")
    ap.add_argument("--random_init_seed", type=int, default=None, help="seeded random weights instead of a checkpoint")
    ap.add_argument("--data_path", required=True, help="one prompt per line; with --i2v a TextImagePairDataset directory")
    ap.add_argument("--i2v", action="store_true", help="image-to-video: encode each image as the first latent frame")
    ap.add_argument("--input_image", default=None, help="condition an i2v-type generator on this image (CLIP + VAE encoder)")
    ap.add_argument("--clip_path", default=None, help="--input_image: the CLIP image encoder's checkpoint")
    ap.add_argument("--clip_random_init_seed", type=int, default=None, help="--input_image: seeded random CLIP weights instead")
    ap.add_argument("--eval_first_n", type=int, default=0)
    ap.add_argument("--prompt_embeds", default=None)
    ap.add_argument("--output_folder", required=True)
    ap.add_argument("--num_output_frames", type=int, default=21)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--num_samples", type=int, default=1)
    ap.add_argument("--latent_height", type=int, default=60)
    ap.add_argument("--latent_width", type=int, default=104)
    ap.add_argument("--vae_path", default=None, help="Wan2.1_VAE.pth: decode the latents to pixels")
    ap.add_argument("--sampling_steps", type=int, default=0, help="multi-step sampler only: override its 50 steps")
    ap.add_argument("--vae_random_init_seed", type=int, default=None,
                    help="seeded random VAE weights instead (decoder; with --i2v the encoder too)")
    ap.add_argument("--taehv_path", default=None,
                    help="taew2_1.pth: decode with the TAEHV tiny decoder instead (fast preview; not with --vae_path / --vae_random_init_seed)")
    ap.add_argument("--taehv_random_init_seed", type=int, default=None, help="seeded random TAEHV decoder weights instead (with --i2v the encoder too)")
    ap.add_argument("--fp8", action="store_true",
                    help="FP8 linear layers in the generator (the reference's enable_fp8 / torchao PerTensor quantisation)")
    ap.add_argument("--pose_path", default=None,
                    help=".pt / .npy dict with dwpose_data [3, F, H, W] and random_ref_dwpose [H, W, 3], an MJPEG .avi, or keypoints: a .npz with the "
                         "array 'keypoints' [F, P, 134, 3] / a .npy array (both with --ref_pose_path)")
    ap.add_argument("--ref_pose_path", default=None,
                    help="--pose_path clip.avi: the JPEG file that is random_ref_dwpose; --pose_path clip.npz / .npy: one frame of keypoints (.npz / .npy)")
    ap.add_argument("--pose_pixel_coords", action="store_true",
                    help="keypoint --pose_path: x and y are pixels of the output (8 x the latent size), not fractions of it in [0, 1]")
    ap.add_argument("--pose_align", action="store_true",
                    help="keypoint --pose_path: give the driving skeleton the proportions and position of the --ref_pose_path person on the GPU "
                         "(PoseRetargeter) before it is drawn")
    ap.add_argument("--pose_fps", default=None, metavar="N[/D]",
                    help=f"keypoint --pose_path: the frame rate of the keypoints, e.g. 30 or 30000/1001; they are resampled on the GPU to the "
                         f"pipeline's {POSE_TARGET_FPS} frames/s")
    ap.add_argument("--pose_source_size", default=None, metavar="HxW",
                    help="keypoint --pose_path: the size of the video the keypoints come from, where its aspect differs from the output's: they are "
                         "scaled by the heights, not stretched")
    ap.add_argument("--pose_smooth", default=None, metavar="MIN_CUTOFF[,BETA[,D_CUTOFF]]",
                    help=f"keypoint --pose_path: steady jittery keypoints on the GPU (PoseSmoother, a One-Euro filter per point) before anything "
                         f"else: the cutoff of a point at rest in Hz (lower is steadier and lags more), how fast the cutoff grows with the point's "
                         f"speed (default 0) and the cutoff of the speed estimate in Hz (default 1); the rate is --pose_fps, else {POSE_TARGET_FPS}")
    ap.add_argument("--pose_hold", type=int, default=None, metavar="N",
                    help="keypoint --pose_path: bridge up to N frames in a row in which a point is missing with its last smoothed position "
                         "(PoseSmoother; with no --pose_smooth the filter runs at its defaults)")
    ap.add_argument("--pose_track", nargs="?", const="", default=None, metavar="SLOTS",
                    help="keypoint --pose_path: put each person into one stable slot across frames on the GPU (PoseTracker) before anything else, "
                         "for keypoints whose people are listed in detection order; SLOTS (1..8) is the number of people kept at once, by default "
                         "the number of people per frame in the file")
    ap.add_argument("--pose_track_gate", type=float, default=None, metavar="G",
                    help="--pose_track: how far a person may move between two matches, in diagonals of its own body box (default 0.5)")
    ap.add_argument("--pose_track_age", type=int, default=None, metavar="N",
                    help="--pose_track: the frames a slot waits for its person before it is freed (default 2); keep --pose_hold at or below it")
    ap.add_argument("--pose_resize", choices=("none", "stretch", "cover"), default="none",
                    help="--pose_path clip.avi: resize the clip and --ref_pose_path on the GPU to the output size (8 x the latent size): stretch, or "
                         "cover = the largest centred crop with the output's aspect ratio; none: their size must be the output size.  Does not apply "
                         "to keypoints (.npz / .npy array), which are drawn at the output size")
    ap.add_argument("--pose_format", choices=("auto", "y4m"), default="auto",
                    help="auto: the kind of --pose_path is read from its name; y4m: it is a YUV4MPEG2 stream whatever it is called -- a FIFO or "
                         "/dev/stdin, e.g. ffmpeg -i dance.mp4 -f yuv4mpegpipe - | generate.py --pose_path /dev/stdin --pose_format y4m ...")
    ap.add_argument("--pose_yuv_matrix", choices=("bt601", "bt709"), default=None, help="--pose_path clip.y4m: the clip's colour matrix (default bt601)")
    ap.add_argument("--pose_yuv_chroma", choices=("triangle", "nearest"), default=None,
                    help="--pose_path clip.y4m: how subsampled chroma is up-sampled (default triangle, libjpeg's filter)")
    ap.add_argument("--pose_weights_path", default=None, help="pose embedding weights (dwpose_embedding.* / randomref_embedding_pose.*)")
    ap.add_argument("--pose_random_init_seed", type=int, default=None, help="seeded random pose embedding weights instead")
    ap.add_argument("--open_length", action="store_true",
                    help="few-step configs with a rolling KV cache (local_attn_size in model_kwargs): let the pose clip of --pose_path decide the "
                         "length, not --num_output_frames -- the clip is fed piece by piece to CausalInferencePipeline.open_session, which goes on "
                         "until it ends")
    ap.add_argument("--video_format", choices=("pt", "mjpeg", "y4m"), default="pt",
                    help="pt: <idx>-<sample>.video.pt (uint8 tensor); mjpeg: <idx>-<sample>.avi, JPEG frames encoded on the GPU, 16 frames/s; "
                         "y4m: <idx>-<sample>.y4m, raw i420 frames converted on the GPU, 16 frames/s (with --open_length written chunk by chunk)")
    ap.add_argument("--yuv_matrix", choices=("bt601", "bt709"), default="bt601", help="--video_format y4m: the colour matrix")
    ap.add_argument("--yuv_range", choices=("limited", "full"), default="limited", help="--video_format y4m: the sample range")
    ap.add_argument("--jpeg_quality", type=int, default=90, help="--video_format mjpeg: 1..100")
    ap.add_argument("--jpeg_subsampling", choices=("420", "444"), default="420", help="--video_format mjpeg: chroma subsampling")
    a = ap.parse_args()
    if not 1 <= a.jpeg_quality <= 100:
        ap.error("--jpeg_quality must be 1..100")
    pose_kind, pose_source_size, pose_smooth, pose_track = check_pose_flags(ap, a)
    if a.open_length and not a.pose_path:
        ap.error("--open_length needs --pose_path: the pose clip decides the length of the video")
    if a.open_length and a.i2v:
        ap.error("--open_length starts from noise: not together with --i2v (an initial latent)")
    if a.pose_resize != "none" and not (a.pose_path and (a.pose_path.lower().endswith(".avi") or pose_kind == "y4m")):
        ap.error("--pose_resize goes with an MJPEG --pose_path (.avi); a .pt / .npy dict is taken at the size it has, keypoints are drawn at the "
                 "output size")
    if a.input_image:
        if (a.clip_path is None) == (a.clip_random_init_seed is None):
            ap.error("--input_image needs exactly one of --clip_path / --clip_random_init_seed")
        if not a.vae_path and a.vae_random_init_seed is None:
            ap.error("--input_image needs a VAE with encoder weights: --vae_path or --vae_random_init_seed")
        if a.i2v:
            ap.error("--input_image (the i2v model type) and --i2v (first frame as initial latent) are different paths: pick one")
    if a.taehv_path and a.taehv_random_init_seed is not None:
        ap.error("--taehv_path and --taehv_random_init_seed are mutually exclusive")
    if (a.taehv_path or a.taehv_random_init_seed is not None) and (a.vae_path or a.vae_random_init_seed is not None):
        ap.error("--taehv_path / --taehv_random_init_seed choose the decoder: not together with --vae_path / --vae_random_init_seed")

    # inference.py:39-45: one process per GPU under torch.distributed.run, RCCL for the start / end barriers only
    from self_forcing_amd.distributed import RankGroup, env_rank_world
    rank, local_rank, world = env_rank_world()
    if a.i2v:
        if world > 1:
            raise SystemExit("I2V does not support distributed inference yet (inference.py:83)")
        if not a.vae_path and a.vae_random_init_seed is None and not a.taehv_path and a.taehv_random_init_seed is None:
            raise SystemExit("--i2v needs a VAE with encoder weights: --vae_path, --vae_random_init_seed, --taehv_path or --taehv_random_init_seed")
    torch.cuda.set_device(local_rank)
    grp = RankGroup(backend="nccl", device=torch.device(f"cuda:{local_rank}"))
    device = torch.device(f"cuda:{local_rank}")
    torch.manual_seed(a.seed + rank)
    torch.set_grad_enabled(False)

    cfg = load_config(a.config_path, a.default_config_path)
    kwargs = dict(cfg.get("model_kwargs") or {})
    if a.open_length and (not is_few_step(cfg) or kwargs.get("local_attn_size", -1) == -1):
        raise SystemExit("--open_length needs a few-step config with a rolling KV cache (model_kwargs.local_attn_size > 0): with global attention "
                         "the cache holds every frame and the length is bounded by it")
    if a.checkpoint_path:
        if a.checkpoint_path.endswith(".safetensors"):
            from safetensors.torch import load_file
            sd = load_file(a.checkpoint_path)
        else:
            ck = torch.load(a.checkpoint_path, map_location="cpu", weights_only=True)
            sd = ck["generator_ema" if a.use_ema else "generator"] if "generator" in ck or "generator_ema" in ck else ck
        gen = sfa.WanDiffusionWrapper(**kwargs, is_causal=True, state_dict=sd, device=device, fp8=a.fp8)
    elif a.pose_path and a.random_init_seed is not None and kwargs.get("model_name", "Wan2.1-T2V-1.3B") in sfa.NAMED_SHAPES:
        # seeded weights with the pose_proj Linear the pose tokens go through.  pose_proj is drawn behind every t2v tensor and
        # in front of an i2v shape's img_emb / k_img / v_img tensors: a t2v generator's other weights are those of the same
        # seed without a pose clip, an i2v generator's image-branch weights are not
        sd = sfa.synth_state_dict(sfa.NAMED_SHAPES[kwargs.get("model_name", "Wan2.1-T2V-1.3B")], seed=a.random_init_seed, pose=True)
        gen = sfa.WanDiffusionWrapper(**kwargs, is_causal=True, state_dict=sd, device=device, fp8=a.fp8)
    else:
        gen = sfa.WanDiffusionWrapper(**kwargs, is_causal=True, random_init_seed=a.random_init_seed, device=device, fp8=a.fp8)
    shape = gen.model.shape
    if a.i2v:
        pairs = read_image_pairs(a.data_path, a.eval_first_n)
        prompts = [c for _, c in pairs]
    else:
        prompts = read_prompts(a.data_path, a.eval_first_n)
    if a.prompt_embeds:
        enc = TableTextEncoder(torch.load(a.prompt_embeds, map_location="cpu", weights_only=True), shape.text_len, shape.text_dim, device)
    else:
        enc = sfa.SyntheticTextEncoder(shape.text_len, shape.text_dim, device=device)
    vae = sfa.IdentityVAE()
    if a.vae_path:
        vae = sfa.WanVAEWrapper(torch.load(a.vae_path, map_location="cpu", weights_only=True), device=device)
    elif a.vae_random_init_seed is not None:
        vae = sfa.WanVAEWrapper(sfa.synth_vae_state_dict(sfa.WAN_VAE, seed=a.vae_random_init_seed, encoder=a.i2v or bool(a.input_image)),
                                device=device)
    if a.taehv_path:
        vae = sfa.TAEHVWrapper(checkpoint_path=a.taehv_path, device=device)
    elif a.taehv_random_init_seed is not None:
        tsd = sfa.synth_taehv_state_dict(seed=a.taehv_random_init_seed)
        if a.i2v:
            tsd.update(sfa.synth_taehv_encoder_state_dict(seed=a.taehv_random_init_seed))
        vae = sfa.TAEHVWrapper(tsd, device=device)
    if a.i2v and isinstance(vae, sfa.TAEHVWrapper) and vae.encoder is None:
        raise SystemExit(f"--i2v needs the TAEHV encoder, but {a.taehv_path} holds no encoder.* tensors (taew2_1.pth does)")
    decode = not isinstance(vae, sfa.IdentityVAE)
    jpeg = sfa.JpegEncoder(a.jpeg_quality, a.jpeg_subsampling, device=device) if decode and a.video_format == "mjpeg" else None
    yuv = sfa.YuvEncoder("i420", a.yuv_matrix, a.yuv_range, value_range=(0, 1), device=device) if decode and a.video_format == "y4m" else None
    few_step = is_few_step(cfg)        # inference.py:62-67: few-step rollout iff the config has denoising_step_list
    pose_embedder = None
    if a.pose_path:
        weights = a.pose_weights_path if a.pose_weights_path else sfa.synth_pose_state_dict(seed=a.pose_random_init_seed)
        pose_embedder = sfa.PoseEmbedder(weights, device=device, strict=cfg.get("pose_weights_strict", True))
        if pose_kind == "mjpeg":
            pose_size = None if a.pose_resize == "none" else (8 * a.latent_height, 8 * a.latent_width)
            pose_data = load_pose_mjpeg(a.pose_path, a.ref_pose_path, device, pose_size, "stretch" if pose_size is None else a.pose_resize)
        elif pose_kind == "y4m":
            pose_size = None if a.pose_resize == "none" else (8 * a.latent_height, 8 * a.latent_width)
            pose_fit = "stretch" if pose_size is None else a.pose_resize
            yuv_decoder = sfa.YuvDecoder(device)
            ref_pose_y4m = load_pose_ref(a.ref_pose_path, device, pose_size, pose_fit)
            pose_data = None
            if not a.open_length:        # the whole clip, read and decoded piece by piece
                try:
                    pieces = list(pose_y4m_feed(open_pose_y4m(a.pose_path), yuv_decoder, a, pose_size, pose_fit))
                except ValueError as e:
                    raise SystemExit(f"{a.pose_path}: {e}")
                if not pieces:
                    raise SystemExit(f"{a.pose_path}: no frames in the stream")
                pose_data = (torch.cat(pieces, dim=1), ref_pose_y4m)
        elif pose_kind == "keypoints":
            pose_data = load_pose_keypoints(a.pose_path, a.ref_pose_path, device, (8 * a.latent_height, 8 * a.latent_width), not a.pose_pixel_coords,
                                            a.pose_align, a.pose_fps, pose_source_size, pose_smooth, a.pose_hold or 0, pose_track)
        else:
            pose_data = load_pose(a.pose_path)
    image_encoder = input_image = None
    if a.input_image:
        if gen.model.model_type != "i2v":
            raise SystemExit(f"--input_image needs a generator of the i2v model type, this one is {gen.model.model_type!r}")
        clip_shape = sfa.CLIP_VIT_H_14 if shape.clip_dim == sfa.CLIP_VIT_H_14.dim else sfa.CLIP_REDUCED
        if a.clip_path:
            image_encoder = sfa.CLIPModel(device=device, checkpoint_path=a.clip_path, shape=clip_shape)
        else:
            image_encoder = sfa.CLIPModel(device=device, state_dict=sfa.synth_clip_state_dict(clip_shape, a.clip_random_init_seed), shape=clip_shape)
        input_image = load_image(a.input_image, 8 * a.latent_height, 8 * a.latent_width)
    if few_step:
        pipe = sfa.CausalInferencePipeline(cfg, device, generator=gen, text_encoder=enc, vae=vae, image_encoder=image_encoder,
                                           pose_embedder=pose_embedder)
    else:                              # 50-step UniPC sampler with classifier-free guidance
        for key in ("num_train_timestep", "timestep_shift", "guidance_scale", "negative_prompt"):
            if key not in cfg:
                raise SystemExit(f"config has neither denoising_step_list nor {key}: cannot build a sampler from it")
        pipe = sfa.CausalDiffusionInferencePipeline(cfg, device, generator=gen, text_encoder=enc, vae=vae, pose_embedder=pose_embedder,
                                                    image_encoder=image_encoder)
        if a.sampling_steps:
            pipe.sampling_steps = a.sampling_steps

    if rank == 0:
        os.makedirs(a.output_folder, exist_ok=True)
    grp.barrier()

    live_y4m_used = False
    for idx in shard_indices(len(prompts), rank, world):
        initial = None
        if a.i2v:   # inference.py:136-149: the encoded image is the first latent frame of every sample
            image = load_image(pairs[idx][0], 8 * a.latent_height, 8 * a.latent_width)
            image = image[None, :, None].to(device=device, dtype=torch.bfloat16)              # [1, 3, 1, H, W]
            initial = vae.encode_to_latent(image).to(device=device, dtype=torch.bfloat16)
            initial = initial.repeat(a.num_samples, 1, 1, 1, 1)
            torch.save(initial[0].cpu(), os.path.join(a.output_folder, f"{idx}.initial_latent.pt"))
        n_noise = a.num_output_frames - (1 if a.i2v else 0)
        noise = torch.randn([a.num_samples, n_noise, 16, a.latent_height, a.latent_width], device=device, dtype=torch.bfloat16)
        dwpose, ref_pose = pose_data if a.pose_path and pose_data is not None else (None, None)
        if a.open_length:      # the clip as a feed of 16-frame pieces; the session ends with it
            if pose_kind == "y4m":         # the reader is the live source: frames are read as the session asks for them
                if live_y4m_used and not os.path.isfile(a.pose_path):
                    raise SystemExit(f"{a.pose_path} is a live source and has been consumed by the first prompt; --open_length takes one prompt per rank from it")
                live_y4m_used = True
                pose_feed, ref_pose = pose_y4m_feed(open_pose_y4m(a.pose_path), yuv_decoder, a, pose_size, pose_fit), ref_pose_y4m
            else:
                pose_feed = iter(dwpose.split(16, dim=1))
            session = pipe.open_session([prompts[idx]] * a.num_samples, (a.latent_height, a.latent_width), batch_size=a.num_samples,
                                        pose_feed=pose_feed, random_ref_dwpose=ref_pose, input_image=input_image, frame_encoder=yuv)
            if yuv is None:
                chunks = [(lat, pixels) for _, lat, pixels in session]
                latents, video = torch.cat([c[0] for c in chunks], dim=1), torch.cat([c[1] for c in chunks], dim=1)
            else:                          # every chunk's frames go to the files as they arrive: the pixels are not kept
                writers, kept, video = None, [], None
                for _, lat, pixels, frames in session:
                    if writers is None:
                        writers = [sfa.y4m.Y4mWriter(os.path.join(a.output_folder, f"{idx}-{s}.y4m"), pixels.shape[-1], pixels.shape[-2], 16, "i420", a.yuv_range)
                                   for s in range(a.num_samples)]
                    t = pixels.shape[1]
                    for s, wr in enumerate(writers):
                        wr.write(frames[s * t:(s + 1) * t])
                    kept.append(lat)
                    video = pixels
                for wr in writers or []:
                    wr.close()
                latents = torch.cat(kept, dim=1)
        elif few_step:
            video, latents = pipe.inference(noise=noise, text_prompts=[prompts[idx]] * a.num_samples, initial_latent=initial,
                                            return_latents=True, input_image=input_image, dwpose_data=dwpose, random_ref_dwpose=ref_pose)
        else:
            video, latents = pipe.inference(noise, [prompts[idx]] * a.num_samples, input_image, dwpose, ref_pose, initial_latent=initial,
                                            return_latents=True)
        for s in range(a.num_samples):
            torch.save(latents[s].cpu(), os.path.join(a.output_folder, f"{idx}-{s}.pt"))
            if yuv is not None:
                if not a.open_length:
                    with sfa.y4m.Y4mWriter(os.path.join(a.output_folder, f"{idx}-{s}.y4m"), video.shape[-1], video.shape[-2], 16, "i420", a.yuv_range) as wr:
                        wr.write(yuv.encode(video[s].float()))
            elif jpeg is not None:
                frames = jpeg.encode(video[s].float() * 2 - 1)
                sfa.mjpeg.write_avi(os.path.join(a.output_folder, f"{idx}-{s}.avi"), frames, 16, video.shape[-1], video.shape[-2])
            elif decode:   # [T, 3, H, W] in [0, 1] -> [T, H, W, 3] uint8 (inference.py:186-187)
                torch.save((255.0 * video[s].permute(0, 2, 3, 1)).to(torch.uint8).cpu(), os.path.join(a.output_folder, f"{idx}-{s}.video.pt"))
        if rank == 0:
            print(f"[generate] prompt {idx}: latents {tuple(latents.shape)}" + (f", video {tuple(video.shape)}" if decode else ""), flush=True)
    grp.finish()


if __name__ == "__main__":
    main()
