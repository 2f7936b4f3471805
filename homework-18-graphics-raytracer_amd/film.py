"""The film: sub-pixel camera rays and filtered accumulation (include/rt_amd.h "film queries").

    offsets / offsets_numpy          where in its pixel each of a pixel's spp samples is taken: a counter hash of the global pixel index
    camera_rays_offset (/ _numpy)    Camera::shoot (src/main.rs:83-99) through those positions, sample-major
    Film                             PhotonAccumulator::accumulate_weight (src/photon.rs:30-33) behind a box, tent or Mitchell filter:
                                     a gather in a fixed order, bit-identical on numpy arrays (librt_host.so) and CUDA tensors (librt_amd.so)
    render_supersampled              offsets -> camera_rays_offset -> trace_rays -> splat -> resolve: an antialiased Whitted frame

Everything is sample-major: sample s of compact pixel i is record s * n_pixels + i.  A public submodule (``rt.film``): its names are not
re-exported at the top level.  Like the rest of the package it loads torch on first use only.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi
from ._args import _new, _on_stream, _out_tensor, _p, _stream_ptr, _tensor, _torch
from ._capi import Camera, Frame
from ._queries import RAY_DTYPE, trace_rays
from ._world import Scene

__all__ = ["PATTERNS", "FILTERS", "offsets", "offsets_numpy", "camera_rays_offset", "camera_rays_offset_numpy", "Film", "render_supersampled"]

PATTERNS = {"center": 0, "uniform": 1, "stratified": 2}  # RT_FILM_CENTER / _UNIFORM / _STRATIFIED
FILTERS = {"box": 0, "tent": 1, "mitchell": 2}           # RT_FILM_BOX / _TENT / _MITCHELL


def _code(table, name, what):
    if name not in table:
        raise ValueError(f"{what} must be one of {', '.join(repr(k) for k in table)}")
    return table[name]


def _np_ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def offsets_numpy(frame: Frame, spp: int, pattern: str = "stratified", seed: int = 0) -> np.ndarray:
    """The sample positions of a frame or tile on the host (rt_film_offsets_host, the CPU definition): an (spp, rows * cols, 2) float32
    array of (dx, dy) in pixels, each in [-0.5, 0.5].  ``pattern``: "center" (all zero), "uniform" (any spp) or "stratified" (spp = k * k,
    k <= 8).  The hash is keyed by the pixel's index in the whole image, so a tile gets the offsets its pixels have in the full frame."""
    out = np.zeros((int(spp), frame.rows * frame.cols, 2), dtype=np.float32)
    _capi.check_host(_capi.host_lib().rt_film_offsets_host(C.byref(frame), int(spp), _code(PATTERNS, pattern, "pattern"), int(seed) & 0xFFFFFFFF,
                                                           _np_ptr(out)))
    return out


def offsets(frame: Frame, spp: int, pattern: str = "stratified", seed: int = 0, out=None, stream=None):
    """offsets_numpy on the device (rt_film_offsets), bit for bit: returns ``out``, an (spp, rows * cols, 2) float32 CUDA tensor (allocated if
    None).  Stream-ordered on ``stream`` (default: torch's current stream)."""
    out = _out_tensor(out, (int(spp), frame.rows * frame.cols, 2), "float32", "cuda")
    _capi.check(_capi.amd_lib().rt_film_offsets(C.byref(frame), int(spp), _code(PATTERNS, pattern, "pattern"), int(seed) & 0xFFFFFFFF, _p(out),
                                                _stream_ptr(stream)))
    return out


def camera_rays_offset(camera: Camera, frame: Frame, offsets, out=None, stream=None):
    """Camera::shoot through (x + dx, y + dy) for every sample (rt_camera_rays_offset): ``offsets`` an (spp, rows * cols, 2) float32 CUDA
    tensor (``offsets()``, or positions of the caller's own); returns ``out``, an (spp * rows * cols, 11) int32 CUDA tensor of rt_ray records,
    sample-major, as ``camera_rays`` writes them.  With zero offsets it is ``camera_rays`` repeated spp times, byte for byte."""
    n = frame.rows * frame.cols
    spp = _tensor(offsets, "offsets", "float32", (None, n, 2)).shape[0]
    out = _out_tensor(out, (spp * n, 11), "int32", offsets.device)
    _capi.check(_capi.amd_lib().rt_camera_rays_offset(C.byref(camera), C.byref(frame), _p(offsets), spp, _p(out), _stream_ptr(stream)))
    return out


def camera_rays_offset_numpy(camera: Camera, frame: Frame, offsets_np) -> np.ndarray:
    """Host-buffer convenience (rt_camera_rays_offset_host, synchronous): ``offsets_np`` an (spp, rows * cols, 2) float32 array; returns
    the rays as a RAY_DTYPE structured array of spp * rows * cols records."""
    n = frame.rows * frame.cols
    a = np.asarray(offsets_np)
    if a.dtype != np.float32 or a.ndim != 3 or a.shape[1:] != (n, 2):
        raise ValueError(f"offsets: expected an (spp, {n}, 2) float32 array")
    a = np.ascontiguousarray(a)
    rays = np.zeros(a.shape[0] * n, dtype=RAY_DTYPE)
    _capi.check(_capi.amd_lib().rt_camera_rays_offset_host(C.byref(camera), C.byref(frame), _np_ptr(a), a.shape[0], _np_ptr(rays)))
    return rays


class Film:
    """A filtered accumulator over a compact image of rows x cols pixels: ``sum`` (rows, cols, 3) and ``weight`` (rows, cols), float32,
    as PhotonAccumulator holds them — numpy arrays with ``device="cpu"`` (librt_host.so), CUDA tensors otherwise (librt_amd.so), with the
    same bits.  ``filter``: "box", "tent" or "mitchell"; ``radius`` in pixels, 0 < radius <= 4.  A box of radius 0.5 is
    PhotonAccumulator.accumulate.  The image is one array: samples beyond its edge do not exist (no halos between bands).

    On a device the constructor allocates ``sum`` and ``weight`` and enqueues their zero fill on torch's CURRENT stream, as
    PhotonAccumulator does: construct the film inside ``with torch.cuda.stream(s):`` when ``splat`` will be given ``stream=s``, or make
    ``s`` wait for the current stream first."""

    def __init__(self, rows: int, cols: int, filter: str = "tent", radius: float = 1.0, device: str = "cpu"):
        self.rows, self.cols, self.device = int(rows), int(cols), device
        self.filter, self.radius = _code(FILTERS, filter, "filter"), float(radius)
        if device == "cpu":
            self.sum = np.zeros((self.rows, self.cols, 3), dtype=np.float32)
            self.weight = np.zeros((self.rows, self.cols), dtype=np.float32)
        else:
            self.sum = _new((self.rows, self.cols, 3), "float32", device).zero_()
            self.weight = _new((self.rows, self.cols), "float32", device).zero_()

    def splat(self, samples, offsets, valid=None, stream=None) -> None:
        """accumulate_weight for every sample that counts (rt_film_splat / rt_film_splat_host): ``samples`` (spp, rows * cols, 3) float32,
        ``offsets`` (spp, rows * cols, 2) float32, ``valid`` (spp, rows * cols) uint8 or None (every sample counts) — numpy arrays on a
        "cpu" film, CUDA tensors otherwise.  Samples are applied in the order s, then row, then column of the source pixel, so one call
        with spp samples equals spp calls with one each."""
        n = self.rows * self.cols
        if self.device == "cpu":
            samples, offsets = np.asarray(samples), np.asarray(offsets)
            if samples.dtype != np.float32 or samples.ndim != 3 or samples.shape[1:] != (n, 3):
                raise ValueError(f"samples: expected an (spp, {n}, 3) float32 array")
            spp = samples.shape[0]
            if offsets.dtype != np.float32 or offsets.shape != (spp, n, 2):
                raise ValueError(f"offsets: expected an ({spp}, {n}, 2) float32 array")
            if valid is not None:
                valid = np.asarray(valid)
                if valid.dtype != np.uint8 or valid.shape != (spp, n):
                    raise ValueError(f"valid: expected an ({spp}, {n}) uint8 array")
                valid = np.ascontiguousarray(valid)
            samples, offsets = np.ascontiguousarray(samples), np.ascontiguousarray(offsets)
            _capi.check_host(_capi.host_lib().rt_film_splat_host(self.rows, self.cols, _np_ptr(samples), _np_ptr(valid), _np_ptr(offsets), spp,
                                                                 self.filter, self.radius, _np_ptr(self.sum), _np_ptr(self.weight)))
            return
        spp = _tensor(samples, "samples", "float32", (None, n, 3)).shape[0]
        _tensor(offsets, "offsets", "float32", (spp, n, 2))
        _tensor(valid, "valid", "uint8", (spp, n), optional=True)
        _capi.check(_capi.amd_lib().rt_film_splat(self.rows, self.cols, _p(samples), _p(valid), _p(offsets), spp, self.filter, self.radius,
                                                  _p(self.sum), _p(self.weight), _stream_ptr(stream)))

    def resolve(self, stream=None):
        """into_rgb_internal (src/photon.rs:15-23): sum / weight as a (rows, cols, 3) float32 image, black where weight < f32::EPSILON."""
        n = self.rows * self.cols
        if self.device == "cpu":
            out = np.empty((self.rows, self.cols, 3), dtype=np.float32)
            _capi.host_lib().rt_accumulator_resolve(_np_ptr(self.sum), _np_ptr(self.weight), n, _np_ptr(out))
            return out
        out = _new((self.rows, self.cols, 3), "float32", self.device)
        _capi.check(_capi.amd_lib().rt_accumulator_resolve_device(_p(self.sum), _p(self.weight), n, _p(out), _stream_ptr(stream)))
        return out


def render_supersampled(scene: Scene, camera: Camera, frame: Frame, spp: int, pattern: str = "stratified", seed: int = 0, filter: str = "tent",
                        radius: float = 1.0, stream=None):
    """A supersampled Whitted frame: offsets -> camera_rays_offset -> trace_rays(depth frame.max_depth) -> Film.splat -> Film.resolve, all on
    ``stream`` (default: torch's current stream), on which the returned (rows, cols, 3) float32 CUDA image before post_process is ready;
    every buffer, the film's zero fill included, is made with ``stream`` as torch's current stream.  ``frame`` must be a full frame (the filter reads
    across pixel borders, and a tile has no halo).

    A sample counts when all three of its channels are FINITE.  This is deliberately not the reference's ``is_normal`` filter
    (src/main.rs:1131), which would also drop zero, that is black, samples: along an edge against a black background the surviving
    samples would all be the bright ones, and the edge would stay as hard as without supersampling."""
    if not (frame.x0 == 0 and frame.y0 == 0 and frame.x1 == frame.width and frame.y1 == frame.height and frame.y_step == 1):
        raise ValueError("render_supersampled takes a full frame (x0 = y0 = 0, x1 = width, y1 = height, y_step = 1)")
    torch = _torch()
    n = frame.rows * frame.cols
    # everything is allocated, and the film's zero fill enqueued, with `stream` as torch's current stream: the caching allocator ties the
    # blocks to it, so what is freed on return is not handed out again while the calls below are still pending
    with _on_stream(stream):
        off = offsets(frame, spp, pattern, seed, stream=stream)
        rays = camera_rays_offset(camera, frame, off, stream=stream)
        rgb = trace_rays(scene, rays, frame.max_depth, stream=stream)
        valid = torch.isfinite(rgb).all(dim=1).to(torch.uint8).view(int(spp), n)
        film = Film(frame.rows, frame.cols, filter, radius, device=rgb.device)
        film.splat(rgb.view(int(spp), n, 3), off, valid, stream=stream)
        return film.resolve(stream=stream)
