"""What every device-resident model class shares (the DiT, the VAE halves, TAEHV, the pose front end, umT5): the tensors
its C descriptor points into, the state-dict check in front of the upload, and the byte buffers the C calls work in."""
from __future__ import annotations

from typing import Callable, Dict, List, Optional

import torch

from . import _lib

Tensor = torch.Tensor


class DeviceModel:
    def __init__(self, device):
        self.device = torch.device(device)
        self._keep: List[Tensor] = []      # every device tensor the C struct points into, in upload order
        self._scratch: Dict[tuple, Tensor] = {}

    def _dev(self, t: Tensor, dtype=torch.bfloat16) -> Tensor:
        t = t.detach().to(device=self.device, dtype=dtype).contiguous()
        self._keep.append(t)
        return t

    def param_bytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in self._keep)

    @staticmethod
    def _check_state_dict(sd: Dict[str, Tensor], need: Dict[str, tuple], whose: Optional[str] = None, what: str = "tensors") -> None:
        """`need`: a *_param_shapes dict.  KeyError "<whose> lacks N <what>, e.g. ..." for absent names (with `whose`;
        without, an absent name is the plain KeyError of the lookup), ValueError for a wrong shape."""
        if whose is not None:
            missing = [k for k in need if k not in sd]
            if missing:
                raise KeyError(f"{whose} lacks {len(missing)} {what}, e.g. {missing[:4]}")
        for k, shp in need.items():
            if tuple(sd[k].shape) != tuple(shp):
                raise ValueError(f"{k}: expected shape {shp}, got {tuple(sd[k].shape)}")

    def _stream_bytes(self, key: tuple, nbytes: Callable[[], int], zero_is_error: Optional[str] = None, keep_one: bool = False) -> Tensor:
        """The uint8 buffer of `key` on the current stream, sized by `nbytes()` (a *_bytes C call) on first use: concurrent
        work on different HIP streams shares the weights but must not share activations.  `zero_is_error`: the name of
        that C call where 0 reports an error; `keep_one`: drop every other buffer first."""
        key = key + (torch.cuda.current_stream(self.device).cuda_stream,)
        buf = self._scratch.get(key)
        if buf is None:
            if keep_one:
                self._scratch.clear()
            n = int(nbytes())
            if n == 0 and zero_is_error:
                _lib.check(-1, zero_is_error)
            buf = self._scratch[key] = torch.empty(n, dtype=torch.uint8, device=self.device)
        return buf
