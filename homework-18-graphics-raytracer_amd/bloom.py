"""Bloom: the highlights of a finished frame spread over their surroundings (include/rt_amd.h "bloom queries") — the step the reference's
post_process leaves as a TODO, between ``post_process_device`` and ``encode_srgb8_device``.

    bloom / bloom_numpy       what lies above a luma threshold (a soft knee around it) is halved ``levels`` times under a [1 3 3 1] tent,
                              summed back up level by level under a bilinear tent and added to the colour; 2 x levels kernel launches in
                              a fixed order, so CUDA tensors (librt_amd.so) and numpy arrays (librt_host.so, the CPU definition) give
                              the same bits
    temp_bytes                the scratch a call needs: the levels of the pyramid, one after the other
    finish_frame              post_process_device -> bloom -> encode_srgb8_device on one stream

The colour may be a strided view of records, as in ``rt.denoise``: the colour inside history records is read where it lies.  A public
submodule (``rt.bloom``): its names are not re-exported at the top level.  Like the rest of the package it loads torch on first use only.

The defaults are starting points, not tuned constants: THRESHOLD 1.0 because post_process puts the 99th-percentile luma at 1.0, so about
one pixel in a hundred glows — the ones the encode would clip; KNEE 0.5 so that a pixel just under the threshold already glows a little
and a highlight does not switch on between two frames; INTENSITY 0.5 because the composite adds intensity times the AVERAGE of the
levels' blurs, and half of that keeps a lamp's halo below the lamp; LEVELS 5 reaches 32 pixels each way, a fortieth of a 1080p frame's
width.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi
from ._args import _on_stream
from ._forms import CUDA, NUMPY
from ._post import encode_srgb8_device, post_process_device

__all__ = ["bloom", "bloom_numpy", "temp_bytes", "finish_frame"]

THRESHOLD, KNEE, INTENSITY, LEVELS = 1.0, 0.5, 0.5, 5
MAX_LEVELS = 8  # RT_BLOOM_MAX_LEVELS


def temp_bytes(rows: int, cols: int, levels: int = LEVELS) -> int:
    """The bytes of ``temp`` for a call of ``levels`` levels on a rows x cols image (rt_bloom_temp_bytes): level j has
    ceil(rows_{j-1} / 2) x ceil(cols_{j-1} / 2) pixels of 3 float32.  0 for a ``levels`` the call refuses."""
    return int(_capi.amd_lib().rt_bloom_temp_bytes(int(rows), int(cols), int(levels)))


def _temp_floats(rows, cols, levels):
    """temp_bytes / 4 without the device library; the entry point refuses levels outside 1 .. 8, the scratch is sized for the nearest first"""
    floats = 0
    for _ in range(min(max(int(levels), 1), MAX_LEVELS)):
        rows, cols = (rows + 1) // 2, (cols + 1) // 2
        floats += rows * cols * 3
    return floats


def _bloom(form, color, threshold, knee, intensity, levels, out=None, temp=None, stream=None):
    shape = tuple(np.shape(color)) if form is NUMPY else tuple(getattr(color, "shape", ()))
    if len(shape) != 3 or shape[2] != 3:
        raise ValueError("color: expected a (rows, cols, 3) float32 image, compact or a strided view of records")
    rows, cols = int(shape[0]), int(shape[1])
    c, c_stride = form.required(color, "color", "f", rows * cols, 3)
    params = _capi.BloomParams(float(threshold), float(knee), float(intensity), int(levels))
    out = form.out(out, (rows, cols, 3), "float32", color, stream=stream)
    temp = form.out(temp, (_temp_floats(rows, cols, levels),), "float32", color, "temp", stream)
    form.call("rt_bloom", stream, c, c_stride, C.byref(params), rows, cols, form.ptr(temp), form.ptr(out))
    return out


def bloom_numpy(color, threshold: float = THRESHOLD, knee: float = KNEE, intensity: float = INTENSITY, levels: int = LEVELS, out=None):
    """The CPU definition (rt_bloom_cpu, librt_host.so; no device, no torch): ``color`` a (rows, cols, 3) float32 array, compact or a
    strided view of records (the last dimension contiguous, one pixel stride of whole words).  A pixel glows by how far its luma
    (post_process's) lies above ``threshold``, softened over ``knee`` either side of it; ``threshold`` ``math.inf`` or ``intensity`` 0
    returns the colour's values.  A pixel that is not finite glows nowhere and stays what it is.  ``levels`` 1 .. 8.  Returns ``out``, a
    (rows, cols, 3) float32 array (new if None); it may be ``color`` itself when that is compact."""
    return _bloom(NUMPY, color, threshold, knee, intensity, levels, out)


def bloom(color, threshold: float = THRESHOLD, knee: float = KNEE, intensity: float = INTENSITY, levels: int = LEVELS, out=None, temp=None,
          stream=None):
    """bloom_numpy on the device (rt_bloom), bit for bit: ``color`` a (rows, cols, 3) float32 CUDA tensor, contiguous or a strided view
    of records.  Returns ``out``, a contiguous (rows, cols, 3) float32 CUDA tensor (allocated if None; it may be ``color`` itself when
    that is contiguous); ``temp`` (``temp_bytes(rows, cols, levels) // 4`` float32; allocated if None) is scratch.  2 x ``levels``
    kernel launches, stream-ordered on ``stream`` (default: torch's current stream), capturable when ``out`` and ``temp`` are given."""
    return _bloom(CUDA, color, threshold, knee, intensity, levels, out, temp, stream)


def finish_frame(img, threshold: float = THRESHOLD, knee: float = KNEE, intensity: float = INTENSITY, levels: int = LEVELS, out=None,
                 temp=None, stream=None):
    """The end of a frame on the device, all on ``stream`` (default: torch's current stream): ``post_process_device`` on ``img`` (a
    contiguous (rows, cols, 3) float32 CUDA tensor, divided IN PLACE by its 99th-percentile luma), ``bloom`` of it with these keywords,
    ``encode_srgb8_device`` of the result.  Returns (rgb8, linear): the (rows, cols, 3) uint8 sRGB image and the linear image after
    bloom (``out``, allocated if None; ``img`` itself may be given)."""
    with _on_stream(stream):
        post_process_device(img, stream=stream)
        linear = bloom(img, threshold, knee, intensity, levels, out=out, temp=temp, stream=stream)
        return encode_srgb8_device(linear, stream=stream), linear
