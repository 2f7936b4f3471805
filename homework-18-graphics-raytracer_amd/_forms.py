"""The two forms of an image query: NUMPY (arrays, ``rt_X_cpu`` in librt_host.so: the CPU definition) and CUDA (tensors, ``rt_X`` in
librt_amd.so, stream-ordered).  A query's two C entry points take the same arguments in the same order, so its Python side is one
body ``_x(form, ...)`` written against the operations below, and two public wrappers that call it with their form and the operands
only that form has (``out``, ``temp``, ``stream``).

    plane(x, name, kind, n, width)              (pointer, pixel stride in words) of a guide plane — compact or a strided view of
                                                records — or (None, 0) for None; ``kind``: "f" float32, "i" 4-byte integers
    required(x, name, kind, n, width)           the same for a plane that must be given
    compact(x, name, rows, cols, width, record) the pointer of a compact operand: rows * cols pixels of ``width`` float32, or of a
                                                record type (label, numpy dtype, device dtype, words): numpy arrays are made
                                                contiguous, tensors must be (rows, cols[, width]) or (rows * cols, words)
    out(given, shape, dtype, like, name, stream, record)
                                                an output: ``given`` (checked), or a new zeroed array, or a new tensor on ``like``'s
                                                device made with ``stream`` current
    ptr(x)                                      the pointer of what ``out`` returned, None for None
    call(entry, stream, *args)                  the library call and its status check; the device form appends the stream

NUMPY never imports torch or loads librt_amd.so; CUDA imports torch on first use, through ``_args``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi
from ._args import _new, _on_stream, _p, _plane_words, _stream_ptr, _tensor

DEMODULATE = 3  # RT_DENOISE_DEMODULATE


class _Numpy:
    def plane(self, a, name, kind, n, width):
        if a is None:
            return None, 0
        a = np.asarray(a)
        if a.dtype.kind in ("f" if kind == "f" else "iu") and a.dtype.itemsize == 4 and a.size == n * width and (
                width == 1 or (a.ndim >= 1 and a.shape[-1] == width)):
            stride = _plane_words(a.shape if width > 1 else a.shape + (1,), [s // 4 for s in a.strides] + ([] if width > 1 else [1]),
                                  all(s % 4 == 0 for s in a.strides))
            if stride is not None:
                return C.c_void_p(a.ctypes.data), stride
        raise ValueError(f"{name}: expected {n} pixels of {width} 4-byte {'floats' if kind == 'f' else 'integers'}, the last dimension contiguous "
                         "and one pixel stride of whole words")

    def required(self, a, name, kind, n, width):
        if a is None:
            raise ValueError(f"{name}: expected a plane, not None")
        return self.plane(a, name, kind, n, width)

    def compact(self, a, name, rows, cols, width=1, record=None):
        a, n = np.asarray(a), rows * cols
        if record is not None:
            if a.dtype != record[1] or a.size != n:
                raise ValueError(f"{name}: expected {n} {record[0]} records")
        elif a.dtype != np.float32 or a.size != n * width or (width > 1 and a.ndim and a.shape[-1] != width):
            raise ValueError(f"{name}: expected {n} pixels of {width} float32" if width > 1 else f"{name}: expected {n} float32")
        return np.ascontiguousarray(a).ctypes.data_as(C.c_void_p)  # the pointer object keeps the array alive

    def out(self, given, shape, dtype, like=None, name="out", stream=None, record=None):
        dtype = np.dtype(dtype if record is None else record[1])
        if given is None:
            return np.zeros(shape, dtype=dtype)
        if not (isinstance(given, np.ndarray) and given.dtype == dtype and given.shape == tuple(shape) and given.flags.c_contiguous and given.flags.writeable):
            raise ValueError(f"{name}: expected a writable C-contiguous {dtype} array of shape {tuple(shape)}")
        return given

    def ptr(self, a):
        return None if a is None else C.c_void_p(a.ctypes.data)

    def call(self, entry, stream, *args):
        _capi.check_host(getattr(_capi.host_lib(), entry + "_cpu")(*args))


class _Cuda:
    _DTYPES = {"f": "float32", "i": "int32"}

    def plane(self, t, name, kind, n, width):
        if t is None:
            return None, 0
        dtype = self._DTYPES[kind]
        _tensor(t, name, dtype, None, contiguous=False)
        if t.numel() == n * width and (width == 1 or (t.dim() >= 1 and t.shape[-1] == width)):
            stride = _plane_words(tuple(t.shape) if width > 1 else tuple(t.shape) + (1,), list(t.stride()) + ([] if width > 1 else [1]), True)
            if stride is not None:
                return _p(t), stride
        raise ValueError(f"{name} must be a {dtype} CUDA tensor of {n} pixels x {width}, the last dimension contiguous and one pixel stride")

    def required(self, t, name, kind, n, width):
        if t is None:
            raise ValueError(f"{name} must be a {self._DTYPES[kind]} CUDA tensor, not None")
        return self.plane(t, name, kind, n, width)

    def compact(self, t, name, rows, cols, width=1, record=None):
        if record is not None:
            return _p(_tensor(t, name, record[2], (rows * cols, record[3])))
        return _p(_tensor(t, name, "float32", (rows, cols, width) if width > 1 else (rows, cols)))

    def out(self, given, shape, dtype, like=None, name="out", stream=None, record=None):
        if record is not None:
            shape, dtype = (shape[0] * shape[1], record[3]), record[2]
        if given is not None:
            return _tensor(given, name, dtype, shape)
        with _on_stream(stream):  # the caching allocator ties the new block to the stream
            return _new(shape, dtype, like.device)

    ptr = staticmethod(_p)

    def call(self, entry, stream, *args):
        _capi.check(getattr(_capi.amd_lib(), entry)(*args, _stream_ptr(stream)))


NUMPY, CUDA = _Numpy(), _Cuda()


def denoise_guides(form, n, normal, position, albedo, valid):
    """DenoiseGuides of ``form``'s planes"""
    g = _capi.DenoiseGuides()
    g.normal, g.normal_stride = form.plane(normal, "normal", "f", n, 3)
    g.position, g.position_stride = form.plane(position, "position", "f", n, 3)
    g.albedo, g.albedo_stride = form.plane(albedo, "albedo", "f", n, 3)
    g.valid, g.valid_stride = form.plane(valid, "valid", "i", n, 1)
    return g


def temporal_guides(form, g, n):
    """TemporalGuides of a ``temporal.Guides`` of ``form``'s planes, or of None"""
    c = _capi.TemporalGuides()
    if g is not None:
        c.normal, c.normal_stride = form.plane(g.normal, "normal", "f", n, 3)
        c.position, c.position_stride = form.plane(g.position, "position", "f", n, 3)
        c.object, c.object_stride = form.plane(g.object, "object", "i", n, 1)
        c.valid, c.valid_stride = form.plane(g.valid, "valid", "i", n, 1)
    return c
