"""Staging of host arrays on the GPU for the plugins: which device, and arrays as the contiguous device tensors the
entry points of gtsfm_amd.device take."""
from typing import Optional, Sequence, Union

import numpy as np
import torch

from gtsfm_amd import native

ArrayLike = Union[np.ndarray, torch.Tensor, Sequence]


def cuda_device(like: Optional[object] = None) -> torch.device:
    """The device a plugin works on: that of `like` when it is a tensor already on a GPU, else the current one.
    Raises NativeError without a GPU."""
    native.require_gpu()
    if isinstance(like, torch.Tensor) and like.is_cuda:
        return like.device
    return torch.device("cuda")


def to_device(a: ArrayLike, dev: torch.device, dtype: Optional[torch.dtype] = None,
              shape: Optional[Sequence[int]] = None) -> torch.Tensor:
    """`a` (array, sequence or tensor) as a contiguous tensor on `dev`, cast to `dtype` and reshaped to `shape` when
    given. A tensor that already is all that comes back as it is, without a copy. A numpy uint32 array asked for as
    int32 is reinterpreted, not converted: keypoint indices travel as the int32 tensors the kernels read as uint32."""
    if not isinstance(a, torch.Tensor):
        arr = np.ascontiguousarray(a)
        a = torch.from_numpy(arr.view(np.int32) if arr.dtype == np.uint32 and dtype == torch.int32 else arr)
    t = a.to(device=dev, dtype=dtype)
    return (t if shape is None else t.reshape(shape)).contiguous()


def mask_to_device(a: ArrayLike, dev: torch.device, n: int) -> torch.Tensor:
    """A (n,) mask of any dtype (non-zero = set) as the uint8 device tensor the kernels take."""
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    return (t.to(dev).reshape(n) != 0).to(torch.uint8).contiguous()
