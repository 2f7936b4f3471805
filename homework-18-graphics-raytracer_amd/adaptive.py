"""Adaptive sampling: a sample budget per pixel, the ragged list it asks for, and the film on such a list (include/rt_amd.h "adaptive
sampling queries").

    budget / budget_numpy            how many samples each pixel gets next, from a mean, a variance and a count plane: the relative
                                     standard error of the mean times ``gain``, between ``min_count`` and ``max_count``
    sample_list / sample_list_numpy  the ragged, PIXEL-MAJOR list of those samples as a ``SampleList``: ``start`` (n + 1), ``pixel`` and
                                     ``sample`` (capacity), ``total`` (listed, asked for); ``list_temp_bytes`` sizes its scratch
    offsets_listed (/ _numpy)        where in its pixel each listed sample is taken: ``film.offsets``' hash of (global pixel, seed, sample)
    camera_rays_listed (/ _numpy)    Camera::shoot through those positions; the all-zero ray beyond the list
    splat_listed (/ _numpy)          ``film.Film.splat`` on a list: equal counts give its bits
    render_pass                      list -> offsets -> rays -> trace_rays -> finite test -> splat_listed, on one stream
    render_adaptive                  a uniform first pass and ``passes`` budgeted ones on running luminance moments

Integer planes are int32 CUDA tensors or 4-byte integer numpy arrays holding the u32 words of the C interface.  A fixed order of single
operations, so CUDA tensors (librt_amd.so) and numpy arrays (librt_host.so, the CPU definition) give the same bits.  A public submodule
(``rt.adaptive``): its names are not re-exported at the top level.  Like the rest of the package it loads torch on first use only.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi
from ._args import _new, _on_stream, _out_tensor, _p, _stream_ptr, _tensor, _torch
from ._capi import Camera, Frame
from ._forms import CUDA, NUMPY
from ._post import luma_row
from ._queries import RAY_DTYPE, trace_rays
from ._world import Scene
from .film import FILTERS, PATTERNS, Film, _code, _np_ptr

__all__ = ["SAMPLE_MAX", "GAIN", "EPSILON", "SampleList", "budget", "budget_numpy", "list_temp_bytes", "sample_list", "sample_list_numpy",
           "offsets_listed", "offsets_listed_numpy", "camera_rays_listed", "camera_rays_listed_numpy", "splat_listed", "splat_listed_numpy",
           "render_pass", "render_adaptive"]

SAMPLE_MAX = 64  # RT_SAMPLE_MAX
# starting points, not tuned constants: with GAIN 32 a pixel whose mean is known to 1/8 asks for 4 samples; EPSILON keeps black pixels finite
GAIN, EPSILON = 32.0, 1e-2


class SampleList:
    """What ``sample_list`` returns: ``start`` (n + 1,), ``pixel`` and ``sample`` (capacity,), ``total`` (2,): records listed, records asked
    for — numpy uint32 arrays or int32 CUDA tensors — and ``capacity``, ``n`` as integers.  ``total`` stays where the list is; reading it is
    the caller's host visit."""

    def __init__(self, start, pixel, sample, total, capacity: int, n: int):
        self.start, self.pixel, self.sample, self.total, self.capacity, self.n = start, pixel, sample, total, int(capacity), int(n)


def _budget_params(gain, epsilon, min_count, max_count):
    return _capi.SampleBudgetParams(float(gain), float(epsilon), int(min_count), int(max_count), 0)


def _budget(form, n, m, v, count, valid, params, shape, dtype, like, out=None, stream=None):
    """``m``, ``v``: the (pointer, stride) of mean and variance, which each form sizes and refuses in its own words"""
    c, c_stride = form.plane(count, "count", "i", n, 1)
    w, w_stride = form.plane(valid, "valid", "i", n, 1)
    out = form.out(out, shape, dtype, like, stream=stream)
    form.call("rt_sample_budget", stream, *m, *v, c, c_stride, w, w_stride, C.byref(params), n, form.ptr(out))
    return out


def budget_numpy(mean, variance, count=None, valid=None, gain: float = GAIN, epsilon: float = EPSILON, min_count: int = 1,
                 max_count: int = SAMPLE_MAX) -> np.ndarray:
    """The CPU definition (rt_sample_budget_cpu, librt_host.so; no device, no torch): ``mean`` / ``variance`` float32 planes of one word
    per pixel, ``count`` / ``valid`` 4-byte integer planes or None (count 1 everywhere; every pixel valid) — compact, or strided views
    such as ``history["moment1"]`` of ``temporal.HISTORY_DTYPE`` records.  Returns a new uint32 array of ``mean``'s shape: 0 where
    ``valid`` is 0, ``max_count`` where ``count`` is 0 or the estimate is not a number, else ``min_count`` + the truncated
    ``gain * sqrt(variance / count) / (|mean| + epsilon)``, at most ``max_count``."""
    shape = np.asarray(mean).shape
    n = int(np.asarray(mean).size)
    m, v = NUMPY.plane(mean, "mean", "f", n, 1), NUMPY.plane(variance, "variance", "f", n, 1)
    if m[0] is None or v[0] is None:
        raise ValueError("mean and variance: expected planes, not None")
    return _budget(NUMPY, n, m, v, count, valid, _budget_params(gain, epsilon, min_count, max_count), shape, "uint32", None)


def budget(mean, variance, count=None, valid=None, gain: float = GAIN, epsilon: float = EPSILON, min_count: int = 1, max_count: int = SAMPLE_MAX,
           out=None, stream=None):
    """budget_numpy on the device (rt_sample_budget), bit for bit: float32 / int32 CUDA tensors, contiguous or strided views of records.
    Returns ``out``, a contiguous (n,) int32 CUDA tensor (allocated if None).  One kernel launch, stream-ordered on ``stream`` (default:
    torch's current stream), capturable when ``out`` is given."""
    _tensor(mean, "mean", "float32", None, contiguous=False)
    n = mean.numel()
    m, v = CUDA.plane(mean, "mean", "f", n, 1), CUDA.required(variance, "variance", "f", n, 1)
    return _budget(CUDA, n, m, v, count, valid, _budget_params(gain, epsilon, min_count, max_count), (n,), "int32", mean, out, stream)


def list_temp_bytes(n: int) -> int:
    """the bytes of scratch ``sample_list`` needs for n pixels (rt_sample_list_temp_bytes: host arithmetic)"""
    return int(_capi.amd_lib().rt_sample_list_temp_bytes(int(n)))


def _np_words(a, name, n):
    a = np.asarray(a)
    if not (a.dtype.kind in "iu" and a.dtype.itemsize == 4 and a.size == n):
        raise ValueError(f"{name}: expected {n} 4-byte integers")
    return np.ascontiguousarray(a).reshape(-1)


def sample_list_numpy(counts, capacity=None, first=None) -> SampleList:
    """The CPU definition (rt_sample_list_cpu, librt_host.so; no device, no torch): ``counts`` n 4-byte integers, each read as at most
    SAMPLE_MAX; ``capacity`` the room in ``pixel`` / ``sample`` (None: exactly the sum); ``first`` a contiguous uint32 or int32 array of n
    first sample indices, ADVANCED IN PLACE by what was listed, or None (every pixel starts at sample 0)."""
    c = np.asarray(counts)
    n = int(c.size)
    c = _np_words(c, "counts", n)
    if capacity is None:
        capacity = int(np.minimum(c.view(np.uint32), SAMPLE_MAX).sum(dtype=np.uint64))
    capacity = int(capacity)
    if first is not None and not (isinstance(first, np.ndarray) and first.dtype.kind in "iu" and first.dtype.itemsize == 4 and first.size == n
                                  and first.flags.c_contiguous):
        raise ValueError(f"first: expected a contiguous array of {n} 4-byte integers (it is advanced in place)")
    room = max(capacity, 0) if capacity < (1 << 32) else 0
    start, total = np.zeros(n + 1, dtype=np.uint32), np.zeros(2, dtype=np.uint32)
    pixel, sample = np.zeros(room, dtype=np.uint32), np.zeros(room, dtype=np.uint32)
    _capi.check_host(_capi.host_lib().rt_sample_list_cpu(_np_ptr(c), n, capacity, _np_ptr(first), _np_ptr(start), _np_ptr(pixel) if room else None,
                                                         _np_ptr(sample) if room else None, _np_ptr(total)))
    return SampleList(start, pixel, sample, total, capacity, n)


def sample_list(counts, capacity: int, first=None, out: SampleList = None, temp=None, stream=None) -> SampleList:
    """sample_list_numpy on the device (rt_sample_list), bit for bit: ``counts`` a contiguous (n,) int32 CUDA tensor, ``first`` the same
    or None, ``capacity`` an integer.  ``out``: a SampleList of this n and capacity to write into; ``temp``: a uint8 CUDA tensor of at
    least ``list_temp_bytes(n)`` bytes; both allocated if None.  Three kernel launches, stream-ordered on ``stream`` (default: torch's
    current stream), no host visit: ``total`` stays on the device.  Capturable at once when ``out`` and ``temp`` are given."""
    _tensor(counts, "counts", "int32", (None,))
    n, capacity = counts.shape[0], int(capacity)
    _tensor(first, "first", "int32", (n,), optional=True)
    need = list_temp_bytes(n)
    room = capacity if 0 <= capacity < (1 << 32) else 0
    with _on_stream(stream):
        if out is None:
            out = SampleList(_new((n + 1,), "int32", counts.device), _new((room,), "int32", counts.device), _new((room,), "int32", counts.device),
                             _new((2,), "int32", counts.device), capacity, n)
        elif not (isinstance(out, SampleList) and out.n == n and out.capacity == capacity):
            raise ValueError(f"out must be a SampleList of {n} pixels and capacity {capacity}")
        if temp is None:
            temp = _new((max(need, 4),), "uint8", counts.device)
    _tensor(out.start, "out.start", "int32", (n + 1,))
    _tensor(out.pixel, "out.pixel", "int32", (room,))
    _tensor(out.sample, "out.sample", "int32", (room,))
    _tensor(out.total, "out.total", "int32", (2,))
    _tensor(temp, "temp", "uint8", (None,))
    _capi.check(_capi.amd_lib().rt_sample_list(_p(counts), n, capacity, _p(first), _p(out.start), _p(out.pixel) if room else None,
                                               _p(out.sample) if room else None, _p(out.total), _p(temp), temp.numel(), _stream_ptr(stream)))
    return out


def _np_list(sl, name="sample_list"):
    if not (isinstance(sl, SampleList) and isinstance(sl.start, np.ndarray)):
        raise ValueError(f"{name}: expected a SampleList of numpy arrays (sample_list_numpy's)")
    return (_np_words(sl.start, "start", sl.n + 1), _np_words(sl.pixel, "pixel", sl.capacity), _np_words(sl.sample, "sample", sl.capacity),
            _np_words(sl.total, "total", 2))


def _cuda_list(sl, name="sample_list"):
    if not isinstance(sl, SampleList) or isinstance(sl.start, np.ndarray):
        raise ValueError(f"{name} must be a SampleList of CUDA tensors (sample_list's)")
    _tensor(sl.start, "start", "int32", (sl.n + 1,))
    _tensor(sl.pixel, "pixel", "int32", (sl.capacity,))
    _tensor(sl.sample, "sample", "int32", (sl.capacity,))
    _tensor(sl.total, "total", "int32", (2,))
    return sl


def offsets_listed_numpy(frame: Frame, sample_list: SampleList, pattern: str = "uniform", seed: int = 0) -> np.ndarray:
    """The CPU definition (rt_film_offsets_listed_cpu): a (capacity, 2) float32 array of (dx, dy); record j < total[0] has the offset
    ``film.offsets`` gives sample ``sample[j]`` of pixel ``pixel[j]``; NaN from the total on and for a pixel the frame does not have.
    ``pattern``: "center" or "uniform" ("stratified" is refused: a ragged pass has no k x k)."""
    start, pixel, sample, total = _np_list(sample_list)
    out = np.zeros((sample_list.capacity, 2), dtype=np.float32)
    _capi.check_host(_capi.host_lib().rt_film_offsets_listed_cpu(C.byref(frame), _code(PATTERNS, pattern, "pattern"), int(seed) & 0xFFFFFFFF, _np_ptr(pixel),
                                                                 _np_ptr(sample), _np_ptr(total), sample_list.capacity, _np_ptr(out)))
    return out


def offsets_listed(frame: Frame, sample_list: SampleList, pattern: str = "uniform", seed: int = 0, out=None, stream=None):
    """offsets_listed_numpy on the device (rt_film_offsets_listed), bit for bit: returns ``out``, a (capacity, 2) float32 CUDA tensor
    (allocated if None).  One kernel launch, stream-ordered, capturable when ``out`` is given."""
    sl = _cuda_list(sample_list)
    with _on_stream(stream):
        out = _out_tensor(out, (sl.capacity, 2), "float32", sl.start.device)
    _capi.check(_capi.amd_lib().rt_film_offsets_listed(C.byref(frame), _code(PATTERNS, pattern, "pattern"), int(seed) & 0xFFFFFFFF, _p(sl.pixel), _p(sl.sample),
                                                       _p(sl.total), sl.capacity, _p(out), _stream_ptr(stream)))
    return out


def camera_rays_listed_numpy(camera: Camera, frame: Frame, offsets, sample_list: SampleList) -> np.ndarray:
    """The CPU definition (rt_camera_rays_listed_cpu): the rays of the listed samples as a RAY_DTYPE array of ``capacity`` records, each
    ``film.camera_rays_offset``'s record of its pixel; the all-zero ray from the total on and for a pixel the frame does not have."""
    start, pixel, sample, total = _np_list(sample_list)
    off = np.asarray(offsets)
    if off.dtype != np.float32 or off.shape != (sample_list.capacity, 2):
        raise ValueError(f"offsets: expected a ({sample_list.capacity}, 2) float32 array")
    off = np.ascontiguousarray(off)
    rays = np.zeros(sample_list.capacity, dtype=RAY_DTYPE)
    _capi.check_host(_capi.host_lib().rt_camera_rays_listed_cpu(C.byref(camera), C.byref(frame), _np_ptr(off), _np_ptr(pixel), _np_ptr(total),
                                                                sample_list.capacity, _np_ptr(rays)))
    return rays


def camera_rays_listed(camera: Camera, frame: Frame, offsets, sample_list: SampleList, out=None, stream=None):
    """camera_rays_listed_numpy on the device (rt_camera_rays_listed), bit for bit: ``offsets`` a (capacity, 2) float32 CUDA tensor;
    returns ``out``, a (capacity, 11) int32 CUDA tensor of rt_ray records (allocated if None)."""
    sl = _cuda_list(sample_list)
    _tensor(offsets, "offsets", "float32", (sl.capacity, 2))
    with _on_stream(stream):
        out = _out_tensor(out, (sl.capacity, 11), "int32", offsets.device)
    _capi.check(_capi.amd_lib().rt_camera_rays_listed(C.byref(camera), C.byref(frame), _p(offsets), _p(sl.pixel), _p(sl.total), sl.capacity, _p(out),
                                                      _stream_ptr(stream)))
    return out


def splat_listed_numpy(film: Film, samples, offsets, sample_list: SampleList, valid=None, max_count: int = SAMPLE_MAX) -> None:
    """The CPU definition (rt_film_splat_listed_cpu) on a ``device="cpu"`` film: ``samples`` (capacity, 3) float32, ``offsets``
    (capacity, 2) float32, ``valid`` (capacity,) uint8 or None.  ``max_count``: a bound on every pixel's count, 1 .. SAMPLE_MAX."""
    if film.device != "cpu":
        raise ValueError("splat_listed_numpy takes a film with device='cpu'")
    start, _, _, _ = _np_list(sample_list)
    cap = sample_list.capacity
    if start.size != film.rows * film.cols + 1:
        raise ValueError(f"sample_list: expected a list of {film.rows * film.cols} pixels")
    samples, offsets = np.asarray(samples), np.asarray(offsets)
    if samples.dtype != np.float32 or samples.shape != (cap, 3):
        raise ValueError(f"samples: expected a ({cap}, 3) float32 array")
    if offsets.dtype != np.float32 or offsets.shape != (cap, 2):
        raise ValueError(f"offsets: expected a ({cap}, 2) float32 array")
    if valid is not None:
        valid = np.asarray(valid)
        if valid.dtype != np.uint8 or valid.shape != (cap,):
            raise ValueError(f"valid: expected a ({cap},) uint8 array")
        valid = np.ascontiguousarray(valid)
    samples, offsets = np.ascontiguousarray(samples), np.ascontiguousarray(offsets)
    _capi.check_host(_capi.host_lib().rt_film_splat_listed_cpu(film.rows, film.cols, _np_ptr(samples), _np_ptr(valid), _np_ptr(offsets), _np_ptr(start), cap,
                                                               int(max_count), film.filter, film.radius, _np_ptr(film.sum), _np_ptr(film.weight)))


def splat_listed(film: Film, samples, offsets, sample_list: SampleList, valid=None, max_count: int = SAMPLE_MAX, stream=None) -> None:
    """``film.splat`` for the samples of a list (rt_film_splat_listed / rt_film_splat_listed_cpu), numpy or CUDA like the film itself:
    sample s of pixel q is record ``start[q] + s``.  With every count equal to spp the film gets ``Film.splat``'s bits."""
    if film.device == "cpu":
        return splat_listed_numpy(film, samples, offsets, sample_list, valid, max_count)
    sl = _cuda_list(sample_list)
    if sl.n != film.rows * film.cols:
        raise ValueError(f"sample_list must list {film.rows * film.cols} pixels")
    _tensor(samples, "samples", "float32", (sl.capacity, 3))
    _tensor(offsets, "offsets", "float32", (sl.capacity, 2))
    _tensor(valid, "valid", "uint8", (sl.capacity,), optional=True)
    _capi.check(_capi.amd_lib().rt_film_splat_listed(film.rows, film.cols, _p(samples), _p(valid), _p(offsets), _p(sl.start), sl.capacity, int(max_count),
                                                     film.filter, film.radius, _p(film.sum), _p(film.weight), _stream_ptr(stream)))


def _full(frame):
    if not (frame.x0 == 0 and frame.y0 == 0 and frame.x1 == frame.width and frame.y1 == frame.height and frame.y_step == 1):
        raise ValueError("a listed pass takes a full frame (x0 = y0 = 0, x1 = width, y1 = height, y_step = 1)")


def render_pass(scene: Scene, camera: Camera, frame: Frame, film: Film, counts, first=None, pattern: str = "uniform", seed: int = 0, capacity=None,
                stream=None):
    """One ragged pass into ``film`` (a CUDA film of the frame's size): sample_list -> offsets_listed -> camera_rays_listed ->
    trace_rays(depth frame.max_depth) -> finite test -> splat_listed, all on ``stream`` (default: torch's current stream).  ``counts``: an
    (n,) int32 CUDA tensor; ``first``: the same, advanced in place, or None.  With ``capacity=None`` the number of records asked for is
    read back ONCE (a list call of capacity 0, then the host visit) and exactly that many rays are traced; with a ``capacity`` there is
    no host visit and ``capacity`` records are traced, the ones beyond the list being all-zero rays nobody reads.  A sample counts when
    its three channels are finite, as in ``film.render_supersampled``.  Returns (sample_list, offsets, rgb)."""
    _full(frame)
    torch = _torch()
    if film.device == "cpu" or (film.rows, film.cols) != (frame.rows, frame.cols):
        raise ValueError("film must be a CUDA film of the frame's rows x cols")
    with _on_stream(stream):
        if capacity is None:
            probe = sample_list(counts, 0, first=None, stream=stream)
            capacity = int(probe.total[1].item()) & 0xFFFFFFFF
        sl = sample_list(counts, capacity, first=first, stream=stream)
        off = offsets_listed(frame, sl, pattern, seed, stream=stream)
        rays = camera_rays_listed(camera, frame, off, sl, stream=stream)
        if sl.capacity == 0:
            return sl, off, _new((0, 3), "float32", rays.device)
        rgb = trace_rays(scene, rays, frame.max_depth, stream=stream)
        valid = torch.isfinite(rgb).all(dim=1).to(torch.uint8)
        splat_listed(film, rgb, off, sl, valid, SAMPLE_MAX, stream=stream)
        return sl, off, rgb


def render_adaptive(scene: Scene, camera: Camera, frame: Frame, passes: int, first_spp: int, params: dict = None, pattern: str = "uniform", seed: int = 0,
                    filter: str = "tent", radius: float = 1.0, capacity=None, stream=None):
    """An adaptively sampled Whitted frame on ``stream``: a uniform pass of ``first_spp`` samples per pixel, then ``passes`` passes whose
    counts are ``budget`` of the running luminance mean, variance and sample count of what each pixel has taken so far (``params``: the
    keywords of ``budget`` — gain, epsilon, min_count, max_count).  The moments are kept with torch operations in sample order (this is
    the convenience, not the ABI).  ``capacity``: as in ``render_pass``, for the budgeted passes.  Returns (image, film, taken): the
    resolved (rows, cols, 3) image before post_process, the film, and the (n,) int32 count of samples taken per pixel."""
    _full(frame)
    torch = _torch()
    first_spp, passes, params = int(first_spp), int(passes), dict(params or {})
    if not 1 <= first_spp <= SAMPLE_MAX:
        raise ValueError(f"first_spp must be in 1 .. {SAMPLE_MAX}")
    n = frame.rows * frame.cols
    with _on_stream(stream):
        device = torch.device("cuda", torch.cuda.current_device())
        film = Film(frame.rows, frame.cols, filter, radius, device=device)
        taken = torch.zeros(n, dtype=torch.int32, device=device)
        s1, s2, lived = (torch.zeros(n, dtype=torch.float32, device=device) for _ in range(3))
        row = torch.tensor(luma_row(), dtype=torch.float32, device=device)
        counts = torch.full((n,), first_spp, dtype=torch.int32, device=device)
        most = first_spp
        for k in range(passes + 1):
            sl, _, rgb = render_pass(scene, camera, frame, film, counts, first=taken, pattern=pattern, seed=seed,
                                     capacity=n * first_spp if k == 0 else capacity, stream=stream)
            if sl.capacity:
                lum = (rgb * row).sum(dim=1)
                ok = torch.isfinite(rgb).all(dim=1)
                lum = torch.where(ok, lum, torch.zeros_like(lum))
                begin, end = sl.start[:-1].long(), sl.start[1:].long()
                for s in range(most):  # sample order: the same sums on every run
                    j = begin + s
                    has = j < end
                    j = torch.where(has, j, torch.zeros_like(j))
                    has = has & ok[j]
                    v = torch.where(has, lum[j], torch.zeros_like(s1))
                    s1, s2, lived = s1 + v, s2 + v * v, lived + has.to(torch.float32)
            if k == passes:
                break
            live = torch.clamp(lived, min=1.0)
            mean = s1 / live
            variance = torch.clamp(s2 / live - mean * mean, min=0.0)
            counts = budget(mean, variance, count=lived.to(torch.int32), stream=stream, **params)
            most = int(params.get("max_count", SAMPLE_MAX))
        return film.resolve(stream=stream), film, taken
