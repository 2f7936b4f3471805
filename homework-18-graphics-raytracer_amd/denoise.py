"""The denoiser: an edge-avoiding A-Trous filter on guide planes (include/rt_amd.h "denoise queries").

    atrous / atrous_numpy     Dammertz et al. 2010, one level per kernel launch: a 5 x 5 B3-spline stencil with holes, each tap weighed by
                              how far its colour, shading normal and position are from the centre's; a fixed order, so CUDA tensors
                              (librt_amd.so) and numpy arrays (librt_host.so, the CPU definition) give the same bits
    temp_bytes                the scratch plane a call of two or more levels needs
    denoise_frame             materials.primary_surfaces -> atrous with that record's shading normal, position, albedo and valid views

Guide planes may be strided views of records (the last dimension contiguous, the pixel stride a whole number of 4-byte words), so the
views of ``PrimarySurfaces`` are passed where they lie.  A public submodule (``rt.denoise``): its names are not re-exported at the top
level.  Like the rest of the package it loads torch on first use only.

The default sigmas are starting points, not tuned constants: SIGMA_COLOR 1.0 because radiance before post_process is of order 1 here (it
halves with every level, as in the paper, so the wide levels do not blur what the narrow ones settled), SIGMA_NORMAL 0.3 because unit normals
more than about 35 degrees apart then weigh under 2 %, SIGMA_POSITION 1.0 scene unit because the reference scene's objects are a few
units across.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi
from ._args import _on_stream, _out_tensor, _p, _plane_words, _stream_ptr, _tensor
from ._capi import Camera, Frame
from ._world import Scene
from .materials import primary_surfaces

__all__ = ["atrous", "atrous_numpy", "temp_bytes", "denoise_frame"]

SIGMA_COLOR, SIGMA_NORMAL, SIGMA_POSITION = 1.0, 0.3, 1.0
_DEMODULATE = 3  # RT_DENOISE_DEMODULATE


def temp_bytes(rows: int, cols: int) -> int:
    """The bytes of ``temp`` for a call of two or more levels (rt_denoise_temp_bytes): one colour plane."""
    return int(_capi.amd_lib().rt_denoise_temp_bytes(int(rows), int(cols)))


def _params(levels, first_level, sigma_color, sigma_normal, sigma_position, demodulate):
    return _capi.DenoiseParams(float(sigma_color), float(sigma_normal), float(sigma_position), int(first_level), int(levels),
                               _DEMODULATE if demodulate is True else int(demodulate))


def _np_plane(a, name, kinds, n, width):
    """a numpy guide plane: its address and its pixel stride in words (the last dimension contiguous, rows * cols pixels in row order)"""
    if a is None:
        return None, 0
    a = np.asarray(a)
    if a.dtype.kind in kinds and a.dtype.itemsize == 4 and a.size == n * width and (width == 1 or (a.ndim >= 1 and a.shape[-1] == width)):
        stride = _plane_words(a.shape if width > 1 else a.shape + (1,), [s // 4 for s in a.strides] + ([] if width > 1 else [1]),
                              all(s % 4 == 0 for s in a.strides))
        if stride is not None:
            return C.c_void_p(a.ctypes.data), stride
    raise ValueError(f"{name}: expected {n} pixels of {width} 4-byte {'floats' if 'f' in kinds else 'integers'}, the last dimension contiguous "
                     "and one pixel stride of whole words")


def _np_guides(n, normal, position, albedo, valid):
    """DenoiseGuides of numpy planes (``svgf`` builds its guides here too)"""
    g = _capi.DenoiseGuides()
    g.normal, g.normal_stride = _np_plane(normal, "normal", "f", n, 3)
    g.position, g.position_stride = _np_plane(position, "position", "f", n, 3)
    g.albedo, g.albedo_stride = _np_plane(albedo, "albedo", "f", n, 3)
    g.valid, g.valid_stride = _np_plane(valid, "valid", "iu", n, 1)
    return g


def atrous_numpy(color, rows: int, cols: int, normal=None, position=None, albedo=None, valid=None, levels: int = 5, first_level: int = 0,
                 sigma_color: float = SIGMA_COLOR, sigma_normal: float = SIGMA_NORMAL, sigma_position: float = SIGMA_POSITION, demodulate=False):
    """The CPU definition (rt_denoise_atrous_cpu, librt_host.so; no device, no torch): ``color`` rows * cols pixels of 3 float32;
    ``normal`` / ``position`` / ``albedo`` the same or strided record views, ``valid`` rows * cols 4-byte integers (0: the pixel is neither
    filtered nor a source), any of them None.  Runs ``levels`` levels from ``first_level`` (step 1 << level, first_level + levels <= 6);
    a sigma of ``math.inf`` switches its term off.  ``demodulate``: divide by (albedo + 1e-3) going in and multiply coming out (True), or
    the RT_DENOISE_DEMODULATE_IN (1) / _OUT (2) bits for a caller who runs the levels in calls of their own.  Returns a new (rows, cols, 3)
    float32 array; ``color`` is not written."""
    rows, cols = int(rows), int(cols)
    n = rows * cols
    c = np.asarray(color)
    if c.dtype != np.float32 or c.size != n * 3 or (c.ndim and c.shape[-1] != 3):
        raise ValueError(f"color: expected {n} pixels of 3 float32")
    c = np.ascontiguousarray(c)
    g = _np_guides(n, normal, position, albedo, valid)
    out = np.zeros((rows, cols, 3), dtype=np.float32)
    temp = np.zeros((rows, cols, 3), dtype=np.float32) if int(levels) >= 2 else None
    p = _params(levels, first_level, sigma_color, sigma_normal, sigma_position, demodulate)
    _capi.check_host(_capi.host_lib().rt_denoise_atrous_cpu(C.c_void_p(c.ctypes.data), C.byref(g), C.byref(p), rows, cols, C.c_void_p(out.ctypes.data),
                                                            None if temp is None else C.c_void_p(temp.ctypes.data)))
    return out


def _plane(t, name, dtype, n, width):
    """a CUDA guide plane through THE tensor check: its address and its pixel stride in words"""
    if t is None:
        return None, 0
    _tensor(t, name, dtype, None, contiguous=False)
    if t.numel() == n * width and (width == 1 or (t.dim() >= 1 and t.shape[-1] == width)):
        stride = _plane_words(tuple(t.shape) if width > 1 else tuple(t.shape) + (1,), list(t.stride()) + ([] if width > 1 else [1]), True)
        if stride is not None:
            return _p(t), stride
    raise ValueError(f"{name} must be a {dtype} CUDA tensor of {n} pixels x {width}, the last dimension contiguous and one pixel stride")


def _guides(n, normal, position, albedo, valid):
    """DenoiseGuides of CUDA planes"""
    g = _capi.DenoiseGuides()
    g.normal, g.normal_stride = _plane(normal, "normal", "float32", n, 3)
    g.position, g.position_stride = _plane(position, "position", "float32", n, 3)
    g.albedo, g.albedo_stride = _plane(albedo, "albedo", "float32", n, 3)
    g.valid, g.valid_stride = _plane(valid, "valid", "int32", n, 1)
    return g


def atrous(color, rows: int, cols: int, normal=None, position=None, albedo=None, valid=None, levels: int = 5, first_level: int = 0,
           sigma_color: float = SIGMA_COLOR, sigma_normal: float = SIGMA_NORMAL, sigma_position: float = SIGMA_POSITION, demodulate=False,
           out=None, temp=None, stream=None):
    """atrous_numpy on the device (rt_denoise_atrous), bit for bit: ``color`` a contiguous (rows, cols, 3) float32 CUDA tensor, the guides
    float32 (``valid``: int32) CUDA tensors, contiguous or strided views such as those of ``materials.PrimarySurfaces``.  Returns ``out``, a
    (rows, cols, 3) float32 CUDA tensor (allocated if None); ``temp`` (the same shape; allocated if None and levels >= 2) is scratch.
    One kernel launch per level, stream-ordered on ``stream`` (default: torch's current stream), capturable when ``out`` and ``temp`` are
    given.  ``color`` is not written; ``out`` and ``temp`` must be other tensors than ``color`` and each other."""
    rows, cols = int(rows), int(cols)
    n = rows * cols
    _tensor(color, "color", "float32", (rows, cols, 3))
    g = _guides(n, normal, position, albedo, valid)
    with _on_stream(stream):
        out = _out_tensor(out, (rows, cols, 3), "float32", color.device)
        if temp is not None or int(levels) >= 2:
            temp = _out_tensor(temp, (rows, cols, 3), "float32", color.device, name="temp")
    p = _params(levels, first_level, sigma_color, sigma_normal, sigma_position, demodulate)
    _capi.check(_capi.amd_lib().rt_denoise_atrous(_p(color), C.byref(g), C.byref(p), rows, cols, _p(out), _p(temp), _stream_ptr(stream)))
    return out


def denoise_frame(scene: Scene, camera: Camera, frame: Frame, image, stream=None, **params):
    """Denoise ``image``, a (rows, cols, 3) float32 CUDA tensor rendered from ``camera`` over ``frame``: materials.primary_surfaces, then
    ``atrous`` guided by that record's shading normal, position, albedo and valid views where they lie — four calls on ``stream``
    (default: torch's current stream).  ``params``: atrous's keywords (levels, sigmas, demodulate, out, temp).  Pixels whose primary ray
    hit nothing pass through."""
    with _on_stream(stream):
        s = primary_surfaces(scene, camera, frame, stream=stream)
        return atrous(image, frame.rows, frame.cols, normal=s.shading_normal, position=s.position, albedo=s.albedo, valid=s.valid, stream=stream,
                      **params)
