"""The variance-guided filter: the spatial half of SVGF on the temporal records (include/rt_amd.h "variance-guided filter queries").

    variance / variance_numpy   a luminance variance per pixel that is usable at every history length: the temporal one (moment2 -
                                moment1^2 of the record) where the history is at least ``min_length`` frames long, else the variance of
                                the first moments in the 7 x 7 neighbourhood, weighed by normal and position and inflated by
                                min_length / length — so a pixel that just reset no longer reads as converged
    atrous / atrous_numpy       Schied et al. 2017: the 5 x 5 B3-spline A-Trous stencil of ``rt.denoise`` with the colour term replaced by
                                |luminance difference| / (sigma_luminance * sqrt(3 x 3 prefiltered variance)), the variance filtered
                                along with the colour (weights squared) from level to level; returns (color, variance)
    temp_bytes                  the scratch a call of two or more levels needs
    filter_frame                temporal.accumulate_frame -> variance on the new records -> atrous on the records' colour where it lies

A fixed order of single f32 operations, so CUDA tensors (librt_amd.so) and numpy arrays (librt_host.so, the CPU definition) give the same
bits.  Guide planes — and the colour — may be strided views of records, as in ``rt.denoise``.  A public submodule (``rt.svgf``): its names
are not re-exported at the top level.  Like the rest of the package it loads torch on first use only.

SIGMA_LUMINANCE 4.0 and MIN_LENGTH 4 are the paper's values (its sigma_l, and the four frames below which it estimates the variance
spatially): starting points, not tuned constants.  4 standard deviations of luminance noise weigh e^-1, so noise within a surface passes
while an edge many deviations high does not; with fewer than 4 frames two moments say little about a variance.  The normal and position
sigmas are ``rt.denoise``'s, for its reasons.  ``demodulate`` divides the colour by albedo inside the filter: the variance given must then be of
the demodulated colour — the history's moments are of the colour as accumulated, so ``filter_frame`` leaves it off.
"""
from __future__ import annotations

import ctypes as C

from . import _capi
from ._args import _on_stream
from ._capi import Camera, Frame
from ._forms import CUDA, DEMODULATE, NUMPY, denoise_guides
from ._world import Scene
from .denoise import SIGMA_NORMAL, SIGMA_POSITION
from .temporal import _HISTORY, History, accumulate_frame

__all__ = ["variance", "variance_numpy", "atrous", "atrous_numpy", "temp_bytes", "filter_frame"]

SIGMA_LUMINANCE, MIN_LENGTH = 4.0, 4


def temp_bytes(rows: int, cols: int, levels: int) -> int:
    """The bytes of ``temp`` for a call of ``levels`` levels (rt_svgf_temp_bytes): 0 for one level."""
    return int(_capi.amd_lib().rt_svgf_temp_bytes(int(rows), int(cols), int(levels)))


def _temp_words(n, levels):
    """rt_svgf_temp_bytes in 4-byte words, without loading librt_amd.so (the numpy path needs no HIP runtime): csrc/rt_svgf.h svgf_temp_words"""
    return n * (0 if levels < 2 else 4 if levels == 2 else 5)


def _variance_params(sigma_normal, sigma_position, min_length):
    return _capi.SvgfVarianceParams(float(sigma_normal), float(sigma_position), int(min_length), 0)


def _atrous_params(levels, first_level, sigma_luminance, sigma_normal, sigma_position, demodulate):
    return _capi.SvgfAtrousParams(float(sigma_luminance), float(sigma_normal), float(sigma_position), int(first_level), int(levels),
                                  DEMODULATE if demodulate is True else int(demodulate))


def _variance(form, history, rows, cols, normal, position, valid, params, out=None, stream=None):
    rows, cols = int(rows), int(cols)
    h = form.compact(history, "history", rows, cols, record=_HISTORY)
    g = denoise_guides(form, rows * cols, normal, position, None, valid)
    out = form.out(out, (rows, cols), "float32", history, stream=stream)
    form.call("rt_svgf_variance", stream, h, C.byref(g), C.byref(params), rows, cols, form.ptr(out))
    return out


def _atrous(form, color, variance, rows, cols, normal, position, albedo, valid, params, out, variance_out, temp=None, stream=None):
    """``variance_out``: False for none, else as ``out``"""
    rows, cols = int(rows), int(cols)
    n = rows * cols
    c, c_stride = form.required(color, "color", "f", n, 3)
    v = form.compact(variance, "variance", rows, cols)
    g = denoise_guides(form, n, normal, position, albedo, valid)
    words = _temp_words(n, params.n_levels)
    out = form.out(out, (rows, cols, 3), "float32", color, stream=stream)
    variance_out = None if variance_out is False else form.out(variance_out, (rows, cols), "float32", color, "variance_out", stream)
    if temp is not None or words:
        temp = form.out(temp, (words,), "float32", color, "temp", stream)
    form.call("rt_svgf_atrous", stream, c, c_stride, v, C.byref(g), C.byref(params), rows, cols, form.ptr(out), form.ptr(variance_out), form.ptr(temp))
    return out, variance_out


def variance_numpy(history, rows: int, cols: int, normal=None, position=None, valid=None, min_length: int = MIN_LENGTH,
                   sigma_normal: float = SIGMA_NORMAL, sigma_position: float = SIGMA_POSITION):
    """The CPU definition (rt_svgf_variance_cpu, librt_host.so; no device, no torch): ``history`` rows * cols HISTORY_DTYPE records as
    ``temporal.accumulate_numpy`` returns them; ``normal`` / ``position`` rows * cols pixels of 3 float32, compact or strided record
    views, ``valid`` rows * cols 4-byte integers, any of them None.  Returns a new (rows, cols) float32 array; nothing given is written."""
    return _variance(NUMPY, history, rows, cols, normal, position, valid, _variance_params(sigma_normal, sigma_position, min_length))


def variance(history, rows: int, cols: int, normal=None, position=None, valid=None, min_length: int = MIN_LENGTH,
             sigma_normal: float = SIGMA_NORMAL, sigma_position: float = SIGMA_POSITION, out=None, stream=None):
    """variance_numpy on the device (rt_svgf_variance), bit for bit: ``history`` a contiguous (rows * cols, 8) int32 CUDA tensor of
    history records (``temporal.History.records``); the guides float32 (``valid``: int32) CUDA tensors, contiguous or strided views.
    Returns ``out``, a (rows, cols) float32 CUDA tensor (allocated if None).  One kernel launch, stream-ordered on ``stream`` (default:
    torch's current stream), capturable when ``out`` is given."""
    return _variance(CUDA, history, rows, cols, normal, position, valid, _variance_params(sigma_normal, sigma_position, min_length), out, stream)


def atrous_numpy(color, variance, rows: int, cols: int, normal=None, position=None, albedo=None, valid=None, levels: int = 5, first_level: int = 0,
                 sigma_luminance: float = SIGMA_LUMINANCE, sigma_normal: float = SIGMA_NORMAL, sigma_position: float = SIGMA_POSITION,
                 demodulate=False, variance_out: bool = True):
    """The CPU definition (rt_svgf_atrous_cpu, librt_host.so; no device, no torch): ``color`` rows * cols pixels of 3 float32, compact or
    a strided view such as ``records["color"]``; ``variance`` rows * cols float32 (variance_numpy's); the guides as in
    ``denoise.atrous_numpy``.  Runs ``levels`` levels from ``first_level`` (step 1 << level, first_level + levels <= 6) with the same
    ``sigma_luminance`` at each; a sigma of ``math.inf`` switches its term off.  ``demodulate`` as in ``denoise.atrous_numpy``.  Returns
    (color, variance): new (rows, cols, 3) and (rows, cols) float32 arrays, the second None without ``variance_out``.  Nothing given is
    written."""
    return _atrous(NUMPY, color, variance, rows, cols, normal, position, albedo, valid,
                   _atrous_params(levels, first_level, sigma_luminance, sigma_normal, sigma_position, demodulate), None, None if variance_out else False)


def atrous(color, variance, rows: int, cols: int, normal=None, position=None, albedo=None, valid=None, levels: int = 5, first_level: int = 0,
           sigma_luminance: float = SIGMA_LUMINANCE, sigma_normal: float = SIGMA_NORMAL, sigma_position: float = SIGMA_POSITION, demodulate=False,
           out=None, variance_out=None, temp=None, stream=None):
    """atrous_numpy on the device (rt_svgf_atrous), bit for bit: ``color`` a float32 CUDA tensor of rows * cols pixels x 3, contiguous or
    a strided view such as ``History.views()[0]``; ``variance`` a contiguous (rows, cols) float32 CUDA tensor; the guides float32
    (``valid``: int32) CUDA tensors, contiguous or strided views.  Returns (out, variance_out): (rows, cols, 3) and (rows, cols) float32
    CUDA tensors, allocated if None; ``variance_out=False`` for none.  ``temp``: a contiguous float32 CUDA tensor of temp_bytes(rows,
    cols, levels) / 4 elements, allocated if None and levels >= 2.  One kernel launch per level, stream-ordered on ``stream`` (default:
    torch's current stream), capturable when ``out``, ``variance_out`` and ``temp`` are given.  The inputs are not written; outputs and
    scratch must be other tensors than the inputs and each other."""
    return _atrous(CUDA, color, variance, rows, cols, normal, position, albedo, valid,
                   _atrous_params(levels, first_level, sigma_luminance, sigma_normal, sigma_position, demodulate), out, variance_out, temp, stream)


def filter_frame(scene: Scene, camera: Camera, frame: Frame, image, history: History, stream=None, min_length: int = MIN_LENGTH, **params):
    """One frame of the whole filter on ``stream`` (default: torch's current stream): ``temporal.accumulate_frame`` of ``image`` into
    ``history``, then ``variance`` on the records it wrote, then ``atrous`` on the colour inside those records, both guided by the shading
    normal, position and valid views of the surfaces the push computed (they are not cast again; atrous is given their albedo too).  ``params``: atrous's keywords (levels,
    sigmas, out, variance_out, temp); the normal and position sigmas go to both calls.  Returns (color, variance) as atrous does.
    Pixels whose primary ray hit nothing pass through.  The history is not changed by the filter."""
    with _on_stream(stream):
        color, _, _ = accumulate_frame(scene, camera, frame, image, history, stream=stream)
        s = history._previous[0]
        guides = dict(normal=s.shading_normal, position=s.position, valid=s.valid)
        shared = {k: params[k] for k in ("sigma_normal", "sigma_position") if k in params}
        v = variance(history.records, history.rows, history.cols, min_length=min_length, stream=stream, **guides, **shared)
        return atrous(color, v, history.rows, history.cols, albedo=s.albedo, stream=stream, **guides, **params)
