"""What the operator modules share in front of a C entry point: the size query of a `*_workspace_bytes` function, the scratch tensor it
sizes, and the two tensor normalisations the kernels' addressing asks for."""
import ctypes

import torch

from .. import _lib

psz = ctypes.POINTER(ctypes.c_size_t)
ptr = _lib.ptr


def stream(t):
    """the current stream of t's device, as the C entry points take it"""
    return _lib.current_stream(t.device)


def workspace_bytes(fn_name, *dims) -> int:
    """The byte count the library's size query `fn_name(*dims, size_t* out)` answers (host arithmetic: no GPU needed)."""
    nb = ctypes.c_size_t(0)
    _lib.check(getattr(_lib.lib(), fn_name)(*dims, ctypes.byref(nb)), fn_name)
    return int(nb.value)


def scratch(fn_name, dev, *dims):
    """A uint8 workspace of workspace_bytes(fn_name, *dims) on `dev`, at least 16 bytes (a zero-size query still yields a pointer)."""
    return torch.empty(max(workspace_bytes(fn_name, *dims), 16), dtype=torch.uint8, device=dev)


def f32c(t: torch.Tensor) -> torch.Tensor:
    """`t` as contiguous fp32 (itself when it already is)."""
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def rows16(x):
    """a 2-D tensor as the row kernels address it: unit column stride, row stride and base multiples of 16 bytes; else a copy"""
    es = x.element_size()
    if x.stride(1) != 1 or (x.shape[0] > 1 and (x.stride(0) < x.shape[1] or (x.stride(0) * es) % 16 != 0)) or x.data_ptr() % 16 != 0:
        x = x.contiguous()
    return x
