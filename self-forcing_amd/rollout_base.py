"""What `CausalInferencePipeline` and `CausalDiffusionInferencePipeline` both are: a causal generator with its text encoder and
VAE, the lazily loaded CLIP image encoder and pose embedder, the causal hyper-parameters, the KV / cross-attention cache sets
and the split of a clip into warm-up blocks and denoising chunks.  A subclass names its device field and its cache sets."""
from __future__ import annotations

import inspect
from typing import List, Optional, Tuple

import torch

from .kvcache import new_crossattn_cache, new_kv_cache, reset_kv_indices
from .wan_wrapper import WanDiffusionWrapper


def chunk_plan(num_frames: int, num_input_frames: int, independent_first_frame: bool, num_frame_per_block: int) -> Tuple[List[int], List[int]]:
    """(the warm-up block lengths over the `num_input_frames` frames of an initial latent, the denoising chunk lengths over the
    `num_frames` frames of the noise): blocks of `num_frame_per_block`, behind one single frame when `independent_first_frame`
    -- the first frame of the initial latent if there is one, else of the noise."""
    first = [1] if independent_first_frame else []
    warm_up = []
    if num_input_frames:
        assert (num_input_frames - len(first)) % num_frame_per_block == 0
        warm_up, first = first + [num_frame_per_block] * ((num_input_frames - len(first)) // num_frame_per_block), []
    assert (num_frames - len(first)) % num_frame_per_block == 0
    return warm_up, first + [num_frame_per_block] * ((num_frames - len(first)) // num_frame_per_block)


class RolloutBase(torch.nn.Module):
    _device_field = "device"                 # the attribute that holds the pipeline's torch.device
    _cache_sets = ()                         # (kv cache attribute, cross-attention cache attribute) per condition
    _image_user = "input_image"              # who asks for the CLIP image encoder, in the message of `_image_encoder`
    _no_i2v_hint = ""                        # appended to the refusal of an image by a generator without the i2v branch
    torch_dtype = torch.bfloat16

    def __init__(self, args, device, generator=None, text_encoder=None, vae=None, image_encoder=None, pose_embedder=None):
        super().__init__()
        setattr(self, self._device_field, torch.device(device))
        self.generator = WanDiffusionWrapper(**getattr(args, "model_kwargs", {}), is_causal=True, device=device) \
            if generator is None else generator
        # as the reference (causal_inference.py:19-23): build the default components when none is injected; they load
        # the reference's default checkpoints (weights-only) and raise FileNotFoundError when those are absent
        if text_encoder is None:
            from .text_encoder import WanTextEncoder
            text_encoder = WanTextEncoder(device=device)
        if vae is None:
            from .vae import WanVAEWrapper
            vae = WanVAEWrapper(device=device)
        self.text_encoder = text_encoder
        self.vae = vae
        # image / pose conditioning: injected, or loaded lazily on first need from args.clip_checkpoint_path /
        # args.pose_weights_path (causal_diffusion_inference.py:59-61, :329-331)
        self.image_encoder = image_encoder
        self.clip_checkpoint_path = getattr(args, "clip_checkpoint_path", None)
        self.pose_embedder = pose_embedder
        self.pose_weights_path = getattr(args, "pose_weights_path", None)
        self.pose_weights_strict = getattr(args, "pose_weights_strict", True)
        self.pose_weights_loaded = pose_embedder is not None

        # causal hyper-parameters (causal_inference.py:25-45)
        self.args = args
        self.num_transformer_blocks = self.generator.model.num_layers
        self.frame_seq_length = 1560  # refined from the latent size at inference()
        self.num_frame_per_block = getattr(args, "num_frame_per_block", 1)
        self.independent_first_frame = args.independent_first_frame
        self.local_attn_size = self.generator.model.local_attn_size
        if self.num_frame_per_block > 1:
            self.generator.model.num_frame_per_block = self.num_frame_per_block
        # context / warm-up passes only update the KV cache; a generator that advertises `cache_only`
        # (ours) may skip what nothing reads.  Foreign generators are called exactly as the reference does.
        try:
            self._cache_only_kw = {"cache_only": True} if "cache_only" in inspect.signature(self.generator.forward).parameters else {}
        except (TypeError, ValueError):
            self._cache_only_kw = {}
        for names in self._cache_sets:
            for name in names:
                setattr(self, name, None)
        self._cache_key = None

    # ------------------------------------------------------------------------------------------ image / pose conditioning
    def _pose_embedder(self):
        """The injected pose embedder, or the one loaded from args.pose_weights_path on first need (:59-61, :329-331)."""
        if self.pose_embedder is None:
            if self.pose_weights_path is None:
                raise ValueError("dwpose_data needs pose weights: set args.pose_weights_path or construct the pipeline with pose_embedder=")
            from .pose import PoseEmbedder
            self.pose_embedder = PoseEmbedder(self.pose_weights_path, device=getattr(self, self._device_field), strict=self.pose_weights_strict)
            self.pose_weights_loaded = True
        return self.pose_embedder

    def _pose_tokens(self, dwpose_data: torch.Tensor):
        """`dwpose_embedding` over the clip (:337-340) as (tokens [1, F'*h*w, 5120], (F', h, w)); the weights load once."""
        return self._pose_embedder().embed(dwpose_data)

    def _image_encoder(self):
        if self.image_encoder is None:
            if self.clip_checkpoint_path is None:
                raise ValueError(f"{self._image_user} needs the CLIP image encoder: set args.clip_checkpoint_path or construct the pipeline "
                                 "with image_encoder=")
            from .clip import CLIPModel
            self.image_encoder = CLIPModel(dtype=self.torch_dtype, device=getattr(self, self._device_field),
                                           checkpoint_path=self.clip_checkpoint_path)
        return self.image_encoder

    # ------------------------------------------------------------------------------------------ caches
    def _cache_tokens(self, total_frames: Optional[int] = None) -> int:
        """Cache capacity in tokens.  The reference uses 32760 (= 21 frames x 1560) or
        local_attn_size x 1560 (causal_inference.py:283-288); here: frames x tokens-per-frame of the
        actual latent, never less than what the rollout needs."""
        if self.local_attn_size != -1:
            return self.local_attn_size * self.frame_seq_length
        return max(21, total_frames or 0) * self.frame_seq_length

    def _initialize_kv_cache(self, batch_size, dtype, device, cache_tokens: Optional[int] = None):
        """Per-GPU KV caches, same dict schema as causal_inference.py:278-298 (`kvcache.new_kv_cache`)."""
        if cache_tokens is None:
            cache_tokens = self._cache_tokens()
        for kv, _ in self._cache_sets:
            setattr(self, kv, new_kv_cache(self.generator.model.shape, self.num_transformer_blocks, batch_size, cache_tokens, dtype, device))

    def _initialize_crossattn_cache(self, batch_size, dtype, device):
        """causal_inference.py:300-312."""
        for _, cross in self._cache_sets:
            setattr(self, cross, new_crossattn_cache(self.generator.model.shape, self.num_transformer_blocks, batch_size, dtype, device))

    def _reset_kv_indices(self):
        for kv, _ in self._cache_sets:
            reset_kv_indices(getattr(self, kv))

    def _prepare_caches(self, batch_size, total_frames, dtype, device):
        """(Re)initialise the caches for a clip (causal_inference.py:111-132): allocate when the batch size, the capacity or
        the device changed, else clear `is_init` and reset the indices."""
        key = (batch_size, self._cache_tokens(total_frames), device)
        if getattr(self, self._cache_sets[0][0]) is None or self._cache_key != key:
            self._initialize_kv_cache(batch_size, dtype, device, cache_tokens=key[1])
            self._initialize_crossattn_cache(batch_size, dtype, device)
            self._cache_key = key
        else:
            for block_index in range(self.num_transformer_blocks):
                for _, cross in self._cache_sets:
                    getattr(self, cross)[block_index]["is_init"] = False
            self._reset_kv_indices()
