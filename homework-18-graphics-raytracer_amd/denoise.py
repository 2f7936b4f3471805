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

from . import _capi
from ._args import _on_stream
from ._capi import Camera, Frame
from ._forms import CUDA, DEMODULATE, NUMPY, denoise_guides
from ._world import Scene
from .materials import primary_surfaces

__all__ = ["atrous", "atrous_numpy", "temp_bytes", "denoise_frame"]

SIGMA_COLOR, SIGMA_NORMAL, SIGMA_POSITION = 1.0, 0.3, 1.0


def temp_bytes(rows: int, cols: int) -> int:
    """The bytes of ``temp`` for a call of two or more levels (rt_denoise_temp_bytes): one colour plane."""
    return int(_capi.amd_lib().rt_denoise_temp_bytes(int(rows), int(cols)))


def _params(levels, first_level, sigma_color, sigma_normal, sigma_position, demodulate):
    return _capi.DenoiseParams(float(sigma_color), float(sigma_normal), float(sigma_position), int(first_level), int(levels),
                               DEMODULATE if demodulate is True else int(demodulate))


def _atrous(form, color, rows, cols, normal, position, albedo, valid, params, out=None, temp=None, stream=None):
    rows, cols = int(rows), int(cols)
    c = form.compact(color, "color", rows, cols, 3)
    g = denoise_guides(form, rows * cols, normal, position, albedo, valid)
    out = form.out(out, (rows, cols, 3), "float32", color, stream=stream)
    if temp is not None or params.n_levels >= 2:
        temp = form.out(temp, (rows, cols, 3), "float32", color, "temp", stream)
    form.call("rt_denoise_atrous", stream, c, C.byref(g), C.byref(params), rows, cols, form.ptr(out), form.ptr(temp))
    return out


def atrous_numpy(color, rows: int, cols: int, normal=None, position=None, albedo=None, valid=None, levels: int = 5, first_level: int = 0,
                 sigma_color: float = SIGMA_COLOR, sigma_normal: float = SIGMA_NORMAL, sigma_position: float = SIGMA_POSITION, demodulate=False):
    """The CPU definition (rt_denoise_atrous_cpu, librt_host.so; no device, no torch): ``color`` rows * cols pixels of 3 float32;
    ``normal`` / ``position`` / ``albedo`` the same or strided record views, ``valid`` rows * cols 4-byte integers (0: the pixel is neither
    filtered nor a source), any of them None.  Runs ``levels`` levels from ``first_level`` (step 1 << level, first_level + levels <= 6);
    a sigma of ``math.inf`` switches its term off.  ``demodulate``: divide by (albedo + 1e-3) going in and multiply coming out (True), or
    the RT_DENOISE_DEMODULATE_IN (1) / _OUT (2) bits for a caller who runs the levels in calls of their own.  Returns a new (rows, cols, 3)
    float32 array; ``color`` is not written."""
    return _atrous(NUMPY, color, rows, cols, normal, position, albedo, valid,
                   _params(levels, first_level, sigma_color, sigma_normal, sigma_position, demodulate))


def atrous(color, rows: int, cols: int, normal=None, position=None, albedo=None, valid=None, levels: int = 5, first_level: int = 0,
           sigma_color: float = SIGMA_COLOR, sigma_normal: float = SIGMA_NORMAL, sigma_position: float = SIGMA_POSITION, demodulate=False,
           out=None, temp=None, stream=None):
    """atrous_numpy on the device (rt_denoise_atrous), bit for bit: ``color`` a contiguous (rows, cols, 3) float32 CUDA tensor, the guides
    float32 (``valid``: int32) CUDA tensors, contiguous or strided views such as those of ``materials.PrimarySurfaces``.  Returns ``out``, a
    (rows, cols, 3) float32 CUDA tensor (allocated if None); ``temp`` (the same shape; allocated if None and levels >= 2) is scratch.
    One kernel launch per level, stream-ordered on ``stream`` (default: torch's current stream), capturable when ``out`` and ``temp`` are
    given.  ``color`` is not written; ``out`` and ``temp`` must be other tensors than ``color`` and each other."""
    return _atrous(CUDA, color, rows, cols, normal, position, albedo, valid,
                   _params(levels, first_level, sigma_color, sigma_normal, sigma_position, demodulate), out, temp, stream)


def denoise_frame(scene: Scene, camera: Camera, frame: Frame, image, stream=None, **params):
    """Denoise ``image``, a (rows, cols, 3) float32 CUDA tensor rendered from ``camera`` over ``frame``: materials.primary_surfaces, then
    ``atrous`` guided by that record's shading normal, position, albedo and valid views where they lie — four calls on ``stream``
    (default: torch's current stream).  ``params``: atrous's keywords (levels, sigmas, demodulate, out, temp).  Pixels whose primary ray
    hit nothing pass through."""
    with _on_stream(stream):
        s = primary_surfaces(scene, camera, frame, stream=stream)
        return atrous(image, frame.rows, frame.cols, normal=s.shading_normal, position=s.position, albedo=s.albedo, valid=s.valid, stream=stream,
                      **params)
