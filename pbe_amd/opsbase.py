"""What every wrapper module over the C-ABI shares (ops.py: the model and sampler path, ops_picture.py: uint8 pictures and masks):
the operand checks, the per-device scratch cache and the small ctypes helpers."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import lib as _l

_ws = {}                  # (device index, name) -> uint8 scratch tensor, see workspace


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _req(t: torch.Tensor, dtype, what: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _l.PbeError(f"{what}: expected a tensor on the GPU (the HIP path has no CPU fallback)")
    if t.dtype != dtype:
        raise _l.PbeError(f"{what}: expected dtype {dtype}, got {t.dtype}")
    return t


def _h(t, what):
    return _req(t, torch.float16, what)


def _f(t, what):
    return _req(t, torch.float32, what)


def workspace(device, name: str, need: int, floor: int = 0) -> torch.Tensor:
    """The scratch buffer `name` of `device`: one uint8 tensor per (device.index, name), kept from call to call (ops on one stream run
    in order, so one buffer is enough) and replaced by max(need, floor) bytes only where it is missing or shorter than `need`.  The
    names and floors are a contract: tests poison a buffer by its key."""
    key = (device.index, name)
    ws = _ws.get(key)
    if ws is None or ws.numel() < need:
        ws = torch.empty(max(need, floor), dtype=torch.uint8, device=device)
        _ws[key] = ws
    return ws


def out_tensor(what: str, out: Optional[torch.Tensor], shape, dtype, device) -> torch.Tensor:
    """`out` checked (on the GPU, dtype, shape, contiguous, on `device`), or a new tensor where it is None."""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    _req(out, dtype, f"{what} out")
    if tuple(out.shape) != tuple(shape) or not out.is_contiguous() or out.device != device:
        raise _l.PbeError(f"{what}: out must be a contiguous {dtype} {tuple(shape)} tensor on {device}, got {tuple(out.shape)}")
    return out


def floats3(values):
    """Three floats as the (c_float * 3) array an entry point takes."""
    return (C.c_float * 3)(*[float(v) for v in values])
