"""Guided upsampling: a low-resolution radiance carried onto full-resolution guide planes (include/rt_amd.h "guided upsampling queries").

    guided / guided_numpy     Kopf et al. 2007, one kernel launch: every output pixel gathers the (2 radius)^2 low-resolution pixels around
                              its position under a tent, each weighed by how far its shading normal and position are from the output
                              pixel's own, and only those of its own object; with ``demodulate`` the low colour is divided by the LOW
                              albedo going in and multiplied by the FULL albedo coming out, so texture returns at full resolution; a
                              fixed order, so CUDA tensors (librt_amd.so) and numpy arrays (librt_host.so, the CPU definition) give the
                              same bits
    Guides                    the guide planes of one resolution, all optional: normal, position, albedo, valid, object
    low_frame                 the full frame of ceil(width / scale) x ceil(height / scale) pixels at the same depth
    low_rays                  that frame's primary rays through the centres of the scale x scale blocks, where the definition places
                              a low pixel
    render_upsampled          primary_surfaces of the frame and of low_rays -> trace_rays of low_rays -> guided

Colour and guide planes may be strided views of records, as in ``rt.denoise``: the views of ``materials.PrimarySurfaces`` and the colour
inside history records are passed where they lie.  A public submodule (``rt.upsample``): its names are not re-exported at the top level.
Like the rest of the package it loads torch on first use only.

The default sigmas are ``rt.denoise``'s, for its reasons.  SCALE 2 renders a quarter of the radiance; RADIUS 1 is the bilinear footprint,
RADIUS 2 a tent twice as wide that still finds a source of the pixel's own object where the four nearest belong to its neighbour.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

from . import _capi
from ._args import _new, _on_stream, _torch
from ._capi import Camera, Frame
from ._forms import CUDA, DEMODULATE, NUMPY, denoise_guides
from ._queries import cast_rays, trace_rays
from ._world import Scene
from .denoise import SIGMA_NORMAL, SIGMA_POSITION
from .film import camera_rays_offset
from .materials import SURFACE_WORDS, PrimarySurfaces, material_hits, primary_surfaces

__all__ = ["guided", "guided_numpy", "Guides", "low_frame", "low_rays", "render_upsampled"]

SCALE, RADIUS = 2, 1


class Guides(NamedTuple):
    """The guide planes of one resolution; any of them may be None.  normal / position / albedo: 3 float32 per pixel; valid / object: one
    4-byte integer per pixel; compact or strided record views."""
    normal: object = None
    position: object = None
    albedo: object = None
    valid: object = None
    object: object = None

    @classmethod
    def of(cls, s) -> "Guides":
        """the planes of a ``materials.PrimarySurfaces``"""
        return cls(s.shading_normal, s.position, s.albedo, s.valid, s.object_index)


def _low_size(extent: int, scale: int) -> int:
    """ceil(extent / scale): the rows or columns of the low-resolution image"""
    return (int(extent) + int(scale) - 1) // int(scale)


def low_frame(frame: Frame, scale: int = SCALE) -> Frame:
    """The full frame of ceil(width / scale) x ceil(height / scale) pixels at ``frame``'s depth: what the radiance is rendered over."""
    return Frame.full(_low_size(frame.width, scale), _low_size(frame.height, scale), frame.max_depth)


def _params(scale, radius, sigma_normal, sigma_position, demodulate):
    return _capi.UpsampleParams(float(sigma_normal), float(sigma_position), int(scale), int(radius),
                                DEMODULATE if demodulate is True else int(demodulate))


def _sizes(rows, cols, scale):
    rows, cols = int(rows), int(cols)
    s = int(scale) if int(scale) >= 1 else 1  # the entry point refuses a scale outside 2 .. 4; the planes are sized for it first
    return rows, cols, rows * cols, _low_size(rows, s) * _low_size(cols, s)


def _guided(form, color_lo, rows, cols, low, full, scale, params, out=None, stream=None):
    rows, cols, n, n_lo = _sizes(rows, cols, scale)
    low, full = low or Guides(), full or Guides()
    c, c_stride = form.required(color_lo, "color_lo", "f", n_lo, 3)
    g_lo = denoise_guides(form, n_lo, low.normal, low.position, low.albedo, low.valid)
    g_hi = denoise_guides(form, n, full.normal, full.position, full.albedo, full.valid)
    o_lo, o_lo_stride = form.plane(low.object, "low.object", "i", n_lo, 1)
    o_hi, o_hi_stride = form.plane(full.object, "full.object", "i", n, 1)
    out = form.out(out, (rows, cols, 3), "float32", color_lo, stream=stream)
    form.call("rt_upsample_guided", stream, c, c_stride, C.byref(g_lo), o_lo, o_lo_stride, C.byref(g_hi), o_hi, o_hi_stride, C.byref(params), rows, cols,
              form.ptr(out))
    return out


def guided_numpy(color_lo, rows: int, cols: int, low: Guides = None, full: Guides = None, scale: int = SCALE, radius: int = RADIUS,
                 sigma_normal: float = SIGMA_NORMAL, sigma_position: float = SIGMA_POSITION, demodulate=True):
    """The CPU definition (rt_upsample_guided_cpu, librt_host.so; no device, no torch): ``color_lo`` ceil(rows / scale) * ceil(cols / scale)
    pixels of 3 float32, compact or a strided record view; ``low`` / ``full`` the Guides of the low and of the OUTPUT resolution.
    ``demodulate``: True for both directions, or the RT_DENOISE_DEMODULATE_IN (1) / _OUT (2) bits; it needs the albedo plane of the
    side it touches.  A sigma of ``math.inf`` switches its term off.  Returns a new (rows, cols, 3) float32 array; nothing given is
    written."""
    return _guided(NUMPY, color_lo, rows, cols, low, full, scale, _params(scale, radius, sigma_normal, sigma_position, demodulate))


def guided(color_lo, rows: int, cols: int, low: Guides = None, full: Guides = None, scale: int = SCALE, radius: int = RADIUS,
           sigma_normal: float = SIGMA_NORMAL, sigma_position: float = SIGMA_POSITION, demodulate=True, out=None, stream=None):
    """guided_numpy on the device (rt_upsample_guided), bit for bit: ``color_lo`` a float32 CUDA tensor of the low image's pixels x 3,
    contiguous or a strided view; the Guides float32 (``valid`` / ``object``: int32) CUDA tensors, contiguous or strided views such as
    those of ``materials.PrimarySurfaces`` (``Guides.of``).  Returns ``out``, a (rows, cols, 3) float32 CUDA tensor (allocated if None),
    which must be another tensor than ``color_lo``.  One kernel launch, stream-ordered on ``stream`` (default: torch's current stream),
    capturable when ``out`` is given."""
    return _guided(CUDA, color_lo, rows, cols, low, full, scale, _params(scale, radius, sigma_normal, sigma_position, demodulate), out, stream)


def _whole_blocks(frame, scale):
    scale = int(scale)
    if not (frame.x0 == 0 and frame.y0 == 0 and frame.x1 == frame.width and frame.y1 == frame.height and frame.y_step == 1):
        raise ValueError("frame: the low-resolution rays need a full frame (Frame.full), not a tile or a row band")
    if scale < 1 or frame.width % scale or frame.height % scale:
        raise ValueError(f"frame: width {frame.width} and height {frame.height} must be multiples of scale {scale}")
    return scale


def low_rays(camera: Camera, frame: Frame, scale: int = SCALE, stream=None):
    """The primary rays of ``low_frame(frame, scale)`` through the CENTRES of the scale x scale blocks of ``frame``'s pixels, where step 2
    of the definition places a low pixel: ``film.camera_rays_offset`` with the offset (scale - 1) / (2 scale) of a low pixel both ways.
    The camera shoots a pixel's ray through its integer coordinate, so low pixel j then looks at output coordinate
    j scale + (scale - 1) / 2; without the offset it would look where output pixel j scale looks.  For scale 2 and 4 the rays are, bit for
    bit, those of ``frame`` through those positions (every operand scales by a power of two).  ``frame`` must be a full frame whose
    width and height are multiples of ``scale`` (ValueError otherwise): only then do the two frames cover the same field of view.
    Returns (low frame, (rows_lo * cols_lo, 11) int32 rt_ray records)."""
    scale = _whole_blocks(frame, scale)
    lo = low_frame(frame, scale)
    with _on_stream(stream):
        offsets = _new((1, lo.rows * lo.cols, 2), "float32", "cuda").fill_((scale - 1) / (2 * scale))
        return lo, camera_rays_offset(camera, lo, offsets, stream=stream)


def _surfaces_of(scene, rays, frame, stream):
    """materials.primary_surfaces for rays of the caller's: the same two calls and the same views of their records"""
    hits = cast_rays(scene, rays, stream=stream)
    surfaces = material_hits(scene, hits, stream=stream)
    h, s = hits.view(frame.rows, frame.cols, 13), surfaces.view(frame.rows, frame.cols, SURFACE_WORDS)
    f32 = lambda t: t.view(_torch().float32)
    return PrimarySurfaces(rays, hits, surfaces, f32(h[..., 12]), f32(h[..., 3:6]), f32(h[..., 6:9]), f32(s[..., 14:17]), f32(s[..., 3:6]), h[..., 2], s[..., 17])


def render_upsampled(scene: Scene, camera: Camera, frame: Frame, scale: int = SCALE, stream=None, **params):
    """A Whitted frame whose radiance is traced at 1 / ``scale`` of the resolution each way, all on ``stream`` (default: torch's current
    stream): ``materials.primary_surfaces`` over ``frame``; ``low_rays`` — one ray per scale x scale block, through its centre —, their
    hits and surfaces (``cast_rays``, ``materials.material_hits``: a PrimarySurfaces of the low image) and their radiance (``trace_rays`` at ``frame``'s depth: ray_trace's own value); and ``guided`` with both
    records' planes.  ``frame`` must be a full frame whose width and height are multiples of ``scale`` (ValueError otherwise);
    ``guided`` itself takes any size.  ``params``: guided's other keywords (radius, sigmas, demodulate, out).  Returns (image, radiance,
    low_surfaces, surfaces): the (rows, cols, 3) image before post_process, the (rows / scale, cols / scale, 3) low-resolution radiance,
    and the PrimarySurfaces of the low and of the full resolution.  Stochastic epochs are not offered: ``focus_rays`` and
    ``render_distributed`` shoot through integer pixel coordinates only, which would leave the low image (scale - 1) / 2 output pixels
    off the block centres."""
    scale = _whole_blocks(frame, scale)
    with _on_stream(stream):
        lo, rays = low_rays(camera, frame, scale, stream=stream)
        s_hi = primary_surfaces(scene, camera, frame, stream=stream)
        s_lo = _surfaces_of(scene, rays, lo, stream)
        radiance = trace_rays(scene, rays, lo.max_depth, stream=stream).view(lo.rows, lo.cols, 3)
        image = guided(radiance, frame.rows, frame.cols, low=Guides.of(s_lo), full=Guides.of(s_hi), scale=scale, stream=stream, **params)
        return image, radiance, s_lo, s_hi
