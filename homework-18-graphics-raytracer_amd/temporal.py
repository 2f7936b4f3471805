"""Temporal accumulation: reprojected history with luminance moments (include/rt_amd.h "temporal queries").

    motion / motion_numpy          where each pixel's surface point was in the previous frame: its position projected through the previous
                                   camera, (px, py) in previous-frame pixel coordinates, NaN where the pixel is invalid or behind that camera
    accumulate / accumulate_numpy  the previous frame's history records gathered bilinearly from there — a tap is dropped when its object,
                                   shading normal or position disagrees — and blended with the current colour; with the first two moments
                                   of luminance, the history length and a per-pixel luminance variance
    HISTORY_DTYPE                  the 32-byte history record (rt_temporal_pixel) as a numpy dtype
    Guides                         the four guide planes of one frame; ``Guides.of(surfaces)`` takes them from a ``PrimarySurfaces``
    History                        the two ping-pong record arrays, the variance plane and the previous frame's surfaces and camera
    accumulate_frame               materials.primary_surfaces -> History.push, on one stream

A fixed order of single f32 operations, so CUDA tensors (librt_amd.so) and numpy arrays (librt_host.so, the CPU definition) give the same
bits.  Guide planes may be strided views of records, as in ``rt.denoise``.  A public submodule (``rt.temporal``): its names are not
re-exported at the top level.  Like the rest of the package it loads torch on first use only.

The default parameters are starting points, not tuned constants: NORMAL_MIN 0.9 because unit shading normals more than about 25 degrees
apart are then taken for another surface; POSITION_MAX 0.1 scene unit because the reference scene's objects are a few units across and
a pixel's footprint on them is of the order of a hundredth; ALPHA_MIN 0.05 so that a change of lighting fades in within about twenty
frames; MAX_LENGTH 32 because beyond it 1 / n lies below ALPHA_MIN anyway and the length stays a small integer.

For moving geometry pass ``motion``/``accumulate`` the position plane that says where each point was in the previous frame:
``rt.moving.previous_positions`` derives it from the scene updates, and ``History.push`` takes it as ``position_was``.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import numpy as np

from . import _capi
from ._args import _on_stream, _torch
from ._capi import Camera, Frame
from ._forms import CUDA, NUMPY, temporal_guides
from ._world import Scene
from .materials import primary_surfaces

__all__ = ["motion", "motion_numpy", "accumulate", "accumulate_numpy", "HISTORY_DTYPE", "Guides", "History", "accumulate_frame"]

NORMAL_MIN, POSITION_MAX, ALPHA_MIN, MAX_LENGTH = 0.9, 0.1, 0.05, 32
HISTORY_DTYPE = np.dtype([("color", "<f4", (3,)), ("moment1", "<f4"), ("moment2", "<f4"), ("length", "<u4"), ("reserved", "<u4", (2,))])
_RECORD_WORDS = 8
_HISTORY = ("HISTORY_DTYPE", HISTORY_DTYPE, "int32", _RECORD_WORDS)  # the record type of _forms' compact and out


class Guides(NamedTuple):
    """The guide planes of one frame: ``normal`` and ``position`` 3 float32 per pixel, ``object`` and ``valid`` one 4-byte integer, each
    compact or a strided view of records, or None.  A plane other than ``valid`` is given for both frames of a call or for neither."""
    normal: object = None
    position: object = None
    object: object = None
    valid: object = None

    @classmethod
    def of(cls, surfaces) -> "Guides":
        """the shading normal, position, object index and valid views of a ``materials.PrimarySurfaces``, where they lie"""
        return cls(surfaces.shading_normal, surfaces.position, surfaces.object_index, surfaces.valid)


def _params(normal_min, position_max, alpha_min, max_length):
    return _capi.TemporalParams(float(normal_min), float(position_max), float(alpha_min), int(max_length), 0)


def _full(frame: Frame):
    if (frame.x0, frame.y0, frame.x1, frame.y1, frame.y_step) != (0, 0, frame.width, frame.height, 1):
        raise ValueError("frame must be the full frame (x0 = y0 = 0, x1 = width, y1 = height, y_step = 1)")
    return int(frame.height), int(frame.width)


def _motion(form, position, camera, frame, valid, out=None, stream=None):
    rows, cols = _full(frame)
    p, p_stride = form.required(position, "position", "f", rows * cols, 3)
    v, v_stride = form.plane(valid, "valid", "i", rows * cols, 1)
    out = form.out(out, (rows, cols, 2), "float32", position, stream=stream)
    form.call("rt_temporal_motion", stream, p, p_stride, v, v_stride, C.byref(camera), C.byref(frame), form.ptr(out))
    return out


def _accumulate(form, color, motion, rows, cols, history, current, previous, params, out, variance, stream=None):
    """``variance``: False for none, else as ``out``"""
    rows, cols = int(rows), int(cols)
    c = form.compact(color, "color", rows, cols, 3)
    m = form.compact(motion, "motion", rows, cols, 2)
    h = form.compact(history, "history", rows, cols, record=_HISTORY)
    cur, prev = temporal_guides(form, current, rows * cols), temporal_guides(form, previous, rows * cols)
    out = form.out(out, (rows, cols), None, color, stream=stream, record=_HISTORY)
    variance = None if variance is False else form.out(variance, (rows, cols), "float32", color, "variance", stream)
    form.call("rt_temporal_accumulate", stream, c, m, C.byref(cur), C.byref(prev), C.byref(params), rows, cols, h, form.ptr(out), form.ptr(variance))
    return out, variance


def motion_numpy(position, camera: Camera, frame: Frame, valid=None):
    """The CPU definition (rt_temporal_motion_cpu, librt_host.so; no device, no torch): ``position`` frame.height * frame.width pixels of
    3 float32 — compact or a strided record view — projected through ``camera`` over the full frame ``frame``, both of the PREVIOUS
    frame; ``valid`` the same number of 4-byte integers or None.  Returns a new (rows, cols, 2) float32 array of (px, py), NaN where
    valid is 0 or the point is not in front of the camera."""
    return _motion(NUMPY, position, camera, frame, valid)


def motion(position, camera: Camera, frame: Frame, valid=None, out=None, stream=None):
    """motion_numpy on the device (rt_temporal_motion), bit for bit: ``position`` a float32 CUDA tensor (``valid``: int32), contiguous or
    a strided view such as ``PrimarySurfaces.position``.  Returns ``out``, a (rows, cols, 2) float32 CUDA tensor (allocated if None).  One
    kernel launch, stream-ordered on ``stream`` (default: torch's current stream), capturable when ``out`` is given."""
    return _motion(CUDA, position, camera, frame, valid, out, stream)


def accumulate_numpy(color, motion, rows: int, cols: int, history, current: Guides = None, previous: Guides = None,
                     normal_min: float = NORMAL_MIN, position_max: float = POSITION_MAX, alpha_min: float = ALPHA_MIN, max_length: int = MAX_LENGTH,
                     variance: bool = True):
    """The CPU definition (rt_temporal_accumulate_cpu, librt_host.so; no device, no torch): ``color`` rows * cols pixels of 3 float32,
    ``motion`` of 2 float32 (motion_numpy's, or your own), ``history`` rows * cols HISTORY_DTYPE records of the previous frame (zeros: no
    history), ``current`` / ``previous`` the Guides of the two frames (``current.position`` is where the point WAS: the plane given to
    motion).  Returns (history_out, variance): a new (rows, cols) HISTORY_DTYPE array and a (rows, cols) float32 array, or None without
    ``variance``.  Nothing given is written."""
    return _accumulate(NUMPY, color, motion, rows, cols, history, current, previous, _params(normal_min, position_max, alpha_min, max_length),
                       None, None if variance else False)


def accumulate(color, motion, rows: int, cols: int, history, current: Guides = None, previous: Guides = None, normal_min: float = NORMAL_MIN,
               position_max: float = POSITION_MAX, alpha_min: float = ALPHA_MIN, max_length: int = MAX_LENGTH, out=None, variance=None,
               stream=None):
    """accumulate_numpy on the device (rt_temporal_accumulate), bit for bit: ``color`` a contiguous (rows, cols, 3) float32 CUDA tensor,
    ``motion`` (rows, cols, 2); ``history`` and ``out`` contiguous (rows * cols, 8) int32 CUDA tensors of history records, two different
    tensors; the guides float32 (``object``, ``valid``: int32) CUDA tensors, contiguous or strided views.  ``variance``: a (rows, cols)
    float32 CUDA tensor, allocated if None, or False for none.  Returns (out, variance).  One kernel launch, stream-ordered on ``stream``
    (default: torch's current stream), capturable when ``out`` and ``variance`` are given."""
    return _accumulate(CUDA, color, motion, rows, cols, history, current, previous, _params(normal_min, position_max, alpha_min, max_length),
                       out, variance, stream)


class History:
    """The state temporal accumulation carries from frame to frame, on the device: two (rows * cols, 8) int32 arrays of history records
    that ``push`` ping-pongs, the variance and motion planes, and the previous frame's PrimarySurfaces and camera, kept alive because the
    next push reads their planes in place.  ``params``: accumulate's keywords (normal_min, position_max, alpha_min, max_length)."""

    def __init__(self, rows: int, cols: int, device=None, **params):
        torch = _torch()
        self.rows, self.cols = int(rows), int(cols)
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else device
        n = self.rows * self.cols
        self._records = [torch.zeros((n, _RECORD_WORDS), dtype=torch.int32, device=device) for _ in range(2)]
        self.variance = torch.zeros((self.rows, self.cols), dtype=torch.float32, device=device)
        self.motion = torch.zeros((self.rows, self.cols, 2), dtype=torch.float32, device=device)
        self.params = dict(params)
        self.frames = 0
        self._previous = None  # (surfaces, camera, frame) of the last push

    @property
    def records(self):
        """the records the last push wrote: a (rows * cols, 8) int32 CUDA tensor (view it as HISTORY_DTYPE on the host)"""
        return self._records[self.frames % 2]

    def views(self):
        """(color, variance, length) of the last push: views of the records, (rows, cols, 3) float32 and (rows, cols) int32, and the variance"""
        torch = _torch()
        r = self.records.view(self.rows, self.cols, _RECORD_WORDS)
        return r[..., 0:3].view(torch.float32), self.variance, r[..., 5]

    def push(self, surfaces, camera: Camera, frame: Frame, image, stream=None, position_was=None, box=None, clamped_length=0, clamped=None):
        """Accumulate ``image``, a (rows, cols, 3) float32 CUDA tensor rendered from ``camera`` over the full frame ``frame`` whose
        ``surfaces`` are its ``materials.primary_surfaces``: motion through the previous push's camera, then accumulate against the
        previous push's surfaces and records — two kernel launches on ``stream``.  The first push finds no history: every pixel resets.
        ``position_was``: for a scene that moved since the previous push, the plane of where each pixel's point was then
        (``moving.previous_positions`` of ``surfaces.hits``), projected and compared instead of ``surfaces.position``.
        ``box``: a (rows * cols, 8) float32 CUDA tensor of colour boxes (``rectify.bounds`` of ``image``): the accumulate is then
        ``rectify.accumulate_bounded`` with ``clamped_length`` and ``clamped``, which clamps the history into them.
        Returns (color, variance, length): views of the new records and the variance plane, valid until the push after the next."""
        if _full(frame) != (self.rows, self.cols):
            raise ValueError(f"frame must be {self.cols} x {self.rows}")
        prev_surfaces, prev_camera, prev_frame = self._previous if self._previous is not None else (surfaces, camera, frame)
        cur = Guides.of(surfaces)
        if position_was is not None:
            cur = cur._replace(position=position_was)
        motion(cur.position, prev_camera, prev_frame, valid=cur.valid, out=self.motion, stream=stream)
        args = (image, self.motion, self.rows, self.cols, self._records[self.frames % 2])
        keywords = dict(current=cur, previous=Guides.of(prev_surfaces), out=self._records[(self.frames + 1) % 2], variance=self.variance, stream=stream,
                        **self.params)
        if box is None:
            accumulate(*args, **keywords)
        else:
            from .rectify import accumulate_bounded  # rectify imports this module

            accumulate_bounded(*args, box, clamped_length=clamped_length, clamped=clamped, **keywords)
        self.frames += 1
        self._previous = (surfaces, Camera.from_buffer_copy(camera), Frame.from_buffer_copy(frame))
        return self.views()


def accumulate_frame(scene: Scene, camera: Camera, frame: Frame, image, history: History, stream=None):
    """``materials.primary_surfaces`` of ``camera`` over ``frame``, then ``history.push`` of ``image``: five calls on ``stream`` (default:
    torch's current stream).  Returns what push returns: (color, variance, length)."""
    with _on_stream(stream):
        s = primary_surfaces(scene, camera, frame, stream=stream)
        return history.push(s, camera, frame, image, stream=stream)
