"""Argument helpers of the Python layer: the one tensor check, allocation, and the pointers the C entry points take.

torch is imported here, on first use, and nowhere else in the package outside dist.py: importing the package does not load it, and
the numpy-only paths never do.  Dtypes travel by name ("int32", "float32", "uint8", ...) so that callers need no torch of their own.
"""
from __future__ import annotations

import ctypes as C
from typing import Sequence

import numpy as np

from ._capi import RtError

_torch_module = None


def _torch():
    global _torch_module
    if _torch_module is None:
        import torch

        _torch_module = torch
    return _torch_module


def _dtype(dtype):
    return getattr(_torch(), dtype) if isinstance(dtype, str) else dtype


def _tensor(t, name, dtype, shape, cuda=True, contiguous=True, optional=False):
    """THE check of a tensor argument: ``t`` must be a torch tensor of ``dtype`` (by name) whose shape matches the pattern ``shape`` —
    a fixed integer must match, None accepts any extent; ``shape=None`` accepts any shape — on the device (``cuda``) and contiguous
    (``contiguous``).  ``optional`` lets None through.  Returns ``t``; raises ValueError naming the parameter, dtype and shape."""
    if t is None and optional:
        return None
    torch = _torch()
    if torch.is_tensor(t) and t.dtype == getattr(torch, dtype) and (t.is_cuda or not cuda) and (not contiguous or t.is_contiguous()):
        if shape is None:
            return t
        extents = t.shape
        if len(extents) == len(shape):
            for have, want in zip(extents, shape):
                if want is not None and have != want:
                    break
            else:
                return t
    raise ValueError(_expected(name, dtype, shape, cuda, contiguous))


def _expected(name, dtype, shape, cuda, contiguous):
    extents = "of any shape" if shape is None else "(" + ", ".join("N" if e is None else str(e) for e in shape) + ("," if len(shape) == 1 else "") + ")"
    return f"{name} must be a {'contiguous ' if contiguous else ''}{extents} {dtype} {'CUDA ' if cuda else ''}tensor"


def _new(shape, dtype, device):
    """an uninitialised tensor, dtype by name"""
    return _torch().empty(shape, dtype=_dtype(dtype), device=device)


def _allocator(device):
    """new(shape, dtype) on ``device``: what the loops make their buffers with"""
    return lambda shape, dtype: _new(shape, dtype, device)


def _out_tensor(out, shape, dtype, device, name="out"):
    """``out`` if the caller gave one — it must be a contiguous CUDA tensor of this shape and dtype — or a new one on ``device``"""
    return _new(shape, dtype, device) if out is None else _tensor(out, name, dtype, shape)


def _on_stream(stream):
    """``with _on_stream(stream):`` — ``stream`` (default: the current one) as torch's current stream: what is allocated inside is
    tied to it by the caching allocator, what torch enqueues inside goes to it"""
    torch = _torch()
    return torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream())


def _stream_ptr(stream):
    """``stream`` (default: torch's current stream) as the void pointer the C entry points take"""
    s = stream if stream is not None else _torch().cuda.current_stream()
    return C.c_void_p(s.cuda_stream)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _count_ptr(ray_count):
    """the pointer of a cast counter, or None: any int64 CUDA tensor with one element, whatever its shape"""
    if ray_count is None:
        return None
    if _tensor(ray_count, "ray_count", "int64", None, contiguous=False).numel() != 1:
        raise ValueError("ray_count must be a 1-element int64 CUDA tensor")
    return _p(ray_count)


def _words(t, name):
    """a contiguous CUDA tensor of 4-byte elements, one or two dimensional: (records, words per record)"""
    if not (_torch().is_tensor(t) and t.is_cuda and t.is_contiguous() and t.element_size() == 4 and t.dim() in (1, 2)):
        raise ValueError(f"{name} must be a contiguous CUDA tensor of 4-byte elements, (N,) or (N, words)")
    return t.shape[0], (1 if t.dim() == 1 else t.shape[1])


def _plane_words(shape, strides, whole_words=True):
    """The pixel stride, in 4-byte words, of a plane of (..., width) words whose pixels are taken in row order — ``strides`` in words — or
    None when the last dimension is not contiguous or the leading dimensions do not advance by ONE stride from pixel to pixel: what lets a
    strided view of records be handed to C as a base pointer and a record stride."""
    if not whole_words or len(shape) != len(strides) or len(shape) < 1:
        return None
    width = shape[-1]
    if width > 1 and strides[-1] != 1:
        return None
    pixel, expect = None, None
    for extent, stride in zip(reversed(shape[:-1]), reversed(strides[:-1])):
        if extent == 1:
            continue
        if pixel is None:
            pixel = stride
        elif stride != expect:
            return None
        expect = stride * extent
    return width if pixel is None else (pixel if pixel > 0 else None)


def _host_records(a, dtype, words, name):
    a = np.asarray(a)
    if a.dtype == dtype:
        return np.ascontiguousarray(a).reshape(-1)
    if a.ndim == 2 and a.shape[1] == words and a.dtype.itemsize == 4:
        return np.ascontiguousarray(a).view(dtype).reshape(-1)
    raise ValueError(f"{name}: expected a {'HIT' if words == 13 else 'RAY'}_DTYPE array or an (N, {words}) array of 4-byte words")


def _host_column(a, dtype, n, name):
    a = np.asarray(a)
    if not (a.dtype.kind in dtype[0] and a.dtype.itemsize == 4 and a.shape == (n,)):
        raise ValueError(f"{name}: expected an ({n},) array of {dtype[1]}")
    return np.ascontiguousarray(a)


# ---- what the hit-sample modules (hemisphere, environment, lobes, arealights, textures, _opened) share ----

def _samples(spp):
    spp = int(spp)
    if spp < 0:
        raise ValueError("spp must not be negative")
    return spp


def _below_2_32(count, what, where=""):
    """a sequence's refusal of a batch no call of the library takes, raised before its workspace is looked at or made"""
    if count >= 1 << 32:
        raise RtError(-5, f"2^32 {what} or more{where}")


def _zeroed_out(out, n, device, stream):
    """the (N, 3) float32 a sequence ADDS to: ``out`` as given, checked, or a new zeroed tensor made with ``stream`` current"""
    if out is not None:
        return _tensor(out, "out", "float32", (n, 3))
    with _on_stream(stream):
        return _new((n, 3), "float32", device).zero_()


def _room(workspace, cls, sizes, wanted, device, stream):
    """A sequence's workspace: ``workspace`` if it is a ``cls`` whose attributes hold at least ``sizes`` (name -> extent; the names are
    the constructor's parameters too), else ValueError("workspace must be " + wanted); None: a new cls(device=device, **sizes),
    allocated with ``stream`` as torch's current stream — the caching allocator then ties the blocks to it."""
    if workspace is None:
        with _on_stream(stream):
            return cls(device=device, **sizes)
    if not isinstance(workspace, cls) or any(getattr(workspace, name) < extent for name, extent in sizes.items()):
        raise ValueError("workspace must be " + wanted)
    return workspace


def _void(a):
    """a numpy array (or None) as the void pointer the CPU forms take"""
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _host(a, dtype, shape, name, optional=False):
    """a contiguous numpy array of ``dtype`` and ``shape`` for a CPU form: integers of the same size are viewed, anything else is
    converted"""
    if a is None and optional:
        return None
    a = np.ascontiguousarray(a)
    if a.dtype != dtype:
        a = a.view(dtype) if a.dtype.itemsize == np.dtype(dtype).itemsize and a.dtype.kind in "iu" and np.dtype(dtype).kind in "iu" else a.astype(dtype)
    if a.shape != shape:
        raise ValueError(f"{name}: expected an array of shape {shape}")
    return a


def _aligned_bytes(size):
    """``size`` zero bytes, 8-byte aligned"""
    return np.zeros((size + 7) // 8, dtype=np.uint64).view(np.uint8)[:size]


def _box3(v, name):
    a = np.asarray(v, dtype=np.float32).reshape(-1)
    if a.shape != (3,):
        raise ValueError(f"{name} must hold 3 floats")
    return (C.c_float * 3)(*a.tolist())


def _f3(v: Sequence[float]):
    return (C.c_float * 3)(*[float(x) for x in v])
