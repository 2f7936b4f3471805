"""History rectification: the colour-box clamp and the filtered feedback (include/rt_amd.h "history rectification queries").

    bounds / bounds_numpy          per pixel, the box mean +- gamma * deviation of the colour and its luminance over the (2 radius + 1)^2
                                   neighbourhood of the CURRENT frame; a neighbour counts when it is valid and of the same object
    accumulate_bounded / accumulate_bounded_numpy
                                   ``temporal.accumulate`` with the reprojected history clamped into that box before the blend: a
                                   history the current frame contradicts — a light moved, a shadow left — is pulled to the box's edge,
                                   its second moment follows its first, and its length is cut to ``clamped_length`` so that it answers
                                   quickly; also returns how many of the four channels were clamped per pixel
    feedback / feedback_numpy      a filtered colour written over the colour of the history records, moments and lengths untouched:
                                   SVGF's feedback of the first A-Trous level
    BOX_DTYPE                      the 32-byte box (rt_temporal_box) as a numpy dtype
    filter_frame                   the whole sequence: primary_surfaces -> motion -> bounds -> accumulate_bounded -> svgf.variance ->
                                   svgf.atrous level 0 -> feedback -> svgf.atrous levels 1 ..

A fixed order of single f32 operations, so CUDA tensors (librt_amd.so) and numpy arrays (librt_host.so, the CPU definition) give the same
bits.  Colour and guide planes may be strided views of records, as in ``rt.denoise``.  A public submodule (``rt.rectify``): its names are
not re-exported at the top level.  Like the rest of the package it loads torch on first use only.

GAMMA, RADIUS and CLAMPED_LENGTH are starting points, not tuned constants.  RADIUS 1 is the 3 x 3 window every TAA uses.  GAMMA 1 is
the value variance clipping is usually run at (Salvi 2016): of nine samples none lies further than sqrt(8) = 2.83 deviations from their
mean, so one deviation does cut into the noise of a history that is right — on the static frames of DESIGN.md 3.25's sequence it clamps
705 of 4 096 pixels — and lets go of a history that is wrong within a few frames.  The clamp is not free and neither is the feedback:
the same section records that in the region whose shading changed the filter WITHOUT feedback comes closer than with it.  CLAMPED_LENGTH 4 is
``svgf.MIN_LENGTH``: a contradicted history blends at 1 / 4, and ``svgf.variance`` takes it for short exactly as long as it is.
DESIGN.md 3.25 has what these and their neighbours give on a stepped sequence.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi, svgf
from ._args import _on_stream, _out_tensor
from ._capi import Camera, Frame
from ._forms import CUDA, NUMPY, temporal_guides
from ._world import Scene
from .materials import primary_surfaces
from .temporal import _HISTORY, ALPHA_MIN, HISTORY_DTYPE, MAX_LENGTH, NORMAL_MIN, POSITION_MAX, Guides, History, _params

__all__ = ["bounds", "bounds_numpy", "accumulate_bounded", "accumulate_bounded_numpy", "feedback", "feedback_numpy", "BOX_DTYPE", "GAMMA",
           "RADIUS", "CLAMPED_LENGTH", "filter_frame"]

GAMMA, RADIUS, CLAMPED_LENGTH = 1.0, 1, 4
BOX_DTYPE = np.dtype([("lo", "<f4", (4,)), ("hi", "<f4", (4,))])
_BOX = ("BOX_DTYPE", BOX_DTYPE, "float32", 8)  # the record type of _forms' compact and out


def _bounds_params(gamma, radius):
    return _capi.BoundsParams(float(gamma), int(radius), 0)


def _bounds(form, color, rows, cols, object, valid, params, out=None, stream=None):
    rows, cols = int(rows), int(cols)
    n = rows * cols
    c, c_stride = form.required(color, "color", "f", n, 3)
    o, o_stride = form.plane(object, "object", "i", n, 1)
    v, v_stride = form.plane(valid, "valid", "i", n, 1)
    out = form.out(out, (rows, cols), None, color, stream=stream, record=_BOX)
    form.call("rt_temporal_bounds", stream, c, c_stride, o, o_stride, v, v_stride, C.byref(params), rows, cols, form.ptr(out))
    return out


def _accumulate_bounded(form, color, motion, rows, cols, history, box, current, previous, params, clamped_length, out, variance, clamped, counts,
                        stream=None):
    """``variance``, ``clamped``: False for none, else as ``out``; ``counts``: the dtype of ``clamped``"""
    rows, cols = int(rows), int(cols)
    c = form.compact(color, "color", rows, cols, 3)
    m = form.compact(motion, "motion", rows, cols, 2)
    h = form.compact(history, "history", rows, cols, record=_HISTORY)
    b = form.compact(box, "box", rows, cols, record=_BOX)
    cur, prev = temporal_guides(form, current, rows * cols), temporal_guides(form, previous, rows * cols)
    out = form.out(out, (rows, cols), None, color, stream=stream, record=_HISTORY)
    variance = None if variance is False else form.out(variance, (rows, cols), "float32", color, "variance", stream)
    clamped = None if clamped is False else form.out(clamped, (rows, cols), counts, color, "clamped", stream)
    form.call("rt_temporal_accumulate_bounded", stream, c, m, C.byref(cur), C.byref(prev), C.byref(params), rows, cols, h, form.ptr(out), form.ptr(variance),
              b, int(clamped_length), form.ptr(clamped))
    return out, variance, clamped


def _feedback(form, color, history, rows, cols, valid, stream=None):
    """``history`` is written in place"""
    rows, cols = int(rows), int(cols)
    c, c_stride = form.required(color, "color", "f", rows * cols, 3)
    v, v_stride = form.plane(valid, "valid", "i", rows * cols, 1)
    form.call("rt_temporal_feedback", stream, c, c_stride, v, v_stride, rows, cols, form.compact(history, "history", rows, cols, record=_HISTORY))


def bounds_numpy(color, rows: int, cols: int, object=None, valid=None, gamma: float = GAMMA, radius: int = RADIUS):
    """The CPU definition (rt_temporal_bounds_cpu, librt_host.so; no device, no torch): ``color`` rows * cols pixels of 3 float32, compact
    or a strided record view; ``object`` / ``valid`` rows * cols 4-byte integers, compact or strided, or None.  Returns a new (rows, cols)
    BOX_DTYPE array: ``lo`` and ``hi`` of the three colour channels and, last, of the luminance; (-inf, +inf) where ``valid`` is 0.
    Nothing given is written."""
    return _bounds(NUMPY, color, rows, cols, object, valid, _bounds_params(gamma, radius))


def bounds(color, rows: int, cols: int, object=None, valid=None, gamma: float = GAMMA, radius: int = RADIUS, out=None, stream=None):
    """bounds_numpy on the device (rt_temporal_bounds), bit for bit: ``color`` a float32 CUDA tensor of rows * cols pixels x 3, contiguous
    or a strided view; ``object`` / ``valid`` int32 CUDA tensors, contiguous or strided views such as those of
    ``materials.PrimarySurfaces``.  Returns ``out``, a contiguous (rows * cols, 8) float32 CUDA tensor of boxes — lo[4], hi[4] — allocated
    if None.  One kernel launch, stream-ordered on ``stream`` (default: torch's current stream), capturable when ``out`` is given."""
    return _bounds(CUDA, color, rows, cols, object, valid, _bounds_params(gamma, radius), out, stream)


def accumulate_bounded_numpy(color, motion, rows: int, cols: int, history, box, current: Guides = None, previous: Guides = None,
                             normal_min: float = NORMAL_MIN, position_max: float = POSITION_MAX, alpha_min: float = ALPHA_MIN,
                             max_length: int = MAX_LENGTH, clamped_length: int = CLAMPED_LENGTH, variance: bool = True):
    """The CPU definition (rt_temporal_accumulate_bounded_cpu, librt_host.so; no device, no torch): ``temporal.accumulate_numpy`` with
    ``box``, rows * cols BOX_DTYPE records (bounds_numpy's of ``color``, or your own), clamping the gathered history before the blend, and
    ``clamped_length`` (0 .. max_length; 0: lengths are not cut).  Returns (history_out, variance, clamped): as accumulate_numpy, and a
    (rows, cols) uint32 array of how many of the four channels the clamp changed.  Nothing given is written."""
    return _accumulate_bounded(NUMPY, color, motion, rows, cols, history, box, current, previous, _params(normal_min, position_max, alpha_min, max_length),
                               clamped_length, None, None if variance else False, None, "uint32")


def accumulate_bounded(color, motion, rows: int, cols: int, history, box, current: Guides = None, previous: Guides = None,
                       normal_min: float = NORMAL_MIN, position_max: float = POSITION_MAX, alpha_min: float = ALPHA_MIN, max_length: int = MAX_LENGTH,
                       clamped_length: int = CLAMPED_LENGTH, out=None, variance=None, clamped=None, stream=None):
    """accumulate_bounded_numpy on the device (rt_temporal_accumulate_bounded), bit for bit: the tensors of ``temporal.accumulate``, and
    ``box`` a contiguous (rows * cols, 8) float32 CUDA tensor (``bounds``'s).  ``clamped``: a (rows, cols) int32 CUDA tensor, allocated if
    None, or False for none.  Returns (out, variance, clamped).  One kernel launch, stream-ordered on ``stream`` (default: torch's current
    stream), capturable when ``out``, ``variance`` and ``clamped`` are given."""
    return _accumulate_bounded(CUDA, color, motion, rows, cols, history, box, current, previous, _params(normal_min, position_max, alpha_min, max_length),
                               clamped_length, out, variance, clamped, "int32", stream)


def feedback_numpy(color, history, rows: int, cols: int, valid=None):
    """The CPU definition (rt_temporal_feedback_cpu, librt_host.so; no device, no torch): a COPY of ``history`` (rows * cols HISTORY_DTYPE
    records) whose colour is ``color`` — rows * cols pixels of 3 float32, compact or strided, the raw words — where the record's length is
    not 0 and ``valid`` (rows * cols 4-byte integers, or None) is not 0.  Returns the new (rows, cols) array; nothing given is written."""
    NUMPY.compact(history, "history", int(rows), int(cols), record=_HISTORY)
    out = np.array(history, dtype=HISTORY_DTYPE, order="C").reshape(int(rows), int(cols))  # the copy is what the call writes
    _feedback(NUMPY, color, out, rows, cols, valid)
    return out


def feedback(color, history, rows: int, cols: int, valid=None, stream=None):
    """feedback_numpy on the device (rt_temporal_feedback), bit for bit, IN PLACE: ``history`` a contiguous (rows * cols, 8) int32 CUDA
    tensor of history records (``temporal.History.records``), ``color`` a float32 CUDA tensor of rows * cols pixels x 3, contiguous or a
    strided view, ``valid`` an int32 CUDA tensor or None.  Returns ``history``.  One kernel launch, stream-ordered on ``stream`` (default:
    torch's current stream), capturable."""
    _feedback(CUDA, color, history, rows, cols, valid, stream)
    return history


def filter_frame(scene: Scene, camera: Camera, frame: Frame, image, history: History, stream=None, gamma: float = GAMMA, radius: int = RADIUS,
                 clamped_length: int = CLAMPED_LENGTH, min_length: int = svgf.MIN_LENGTH, levels: int = 5, box=None, clamped=None, first=None,
                 **params):
    """One frame of the whole spatiotemporal filter on ``stream`` (default: torch's current stream): ``materials.primary_surfaces``, then
    ``bounds`` of ``image`` by object and valid, ``history.push`` with that box (motion, accumulate_bounded), ``svgf.variance`` on the new
    records, ``svgf.atrous`` level 0 on the colour inside them, ``feedback`` of that level into ``history.records`` — the next frame's
    history is the filtered colour — and ``svgf.atrous`` levels 1 .. ``levels`` - 1 on level 0's output.  The guides are those of
    ``svgf.filter_frame``.  ``box`` / ``clamped``: tensors for ``bounds`` and the clamp counts, allocated if None; ``first``: (out,
    variance_out) of level 0, allocated if None; ``params``: the other keywords of ``svgf.atrous`` (sigmas, out, variance_out, temp), the
    normal and position sigmas going to ``svgf.variance`` too.  ``demodulate`` is refused (ValueError): the moments in the records are of the
    colour as accumulated, so the variance is not that of a demodulated colour, and a level 0 that is fed back would have to leave the
    filter modulated while the levels after it start demodulated again — ``svgf.atrous`` in calls of your own does that if you want it.
    Returns (color, variance, clamped)."""
    levels = int(levels)
    if params.get("demodulate"):
        raise ValueError("demodulate: not with filter_frame — the history's moments are of the colour as accumulated; run svgf.atrous yourself")
    params = {k: w for k, w in params.items() if k != "demodulate"}
    with _on_stream(stream):
        s = primary_surfaces(scene, camera, frame, stream=stream)
        box = bounds(image, history.rows, history.cols, object=s.object_index, valid=s.valid, gamma=gamma, radius=radius, out=box, stream=stream)
        clamped = _out_tensor(clamped, (history.rows, history.cols), "int32", image.device, name="clamped")
        color, _, _ = history.push(s, camera, frame, image, stream=stream, box=box, clamped_length=clamped_length, clamped=clamped)
        guides = dict(normal=s.shading_normal, position=s.position, valid=s.valid)
        shared = {k: params[k] for k in ("sigma_normal", "sigma_position") if k in params}
        v = svgf.variance(history.records, history.rows, history.cols, min_length=min_length, stream=stream, **guides, **shared)
        sigmas = {k: w for k, w in params.items() if k.startswith("sigma_")}
        out0, var0 = (None, None) if first is None else first
        level0 = dict(out=params.get("out"), variance_out=params.get("variance_out")) if levels == 1 else dict(out=out0, variance_out=var0)
        color, v = svgf.atrous(color, v, history.rows, history.cols, albedo=s.albedo, levels=1, first_level=0, stream=stream, **guides, **sigmas, **level0)
        feedback(color, history.records, history.rows, history.cols, valid=s.valid, stream=stream)
        if levels > 1:
            color, v = svgf.atrous(color, v, history.rows, history.cols, albedo=s.albedo, levels=levels - 1, first_level=1, stream=stream, **guides, **params)
        return color, v, clamped
