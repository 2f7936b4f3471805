"""The two render loops over a frame or tile — the Whitted pass and the stochastic (depth-of-field) epochs — with their
generators and the process-wide switches."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi
from ._args import _count_ptr, _new, _out_tensor, _p, _stream_ptr, _tensor
from ._capi import Camera, Frame
from ._world import Scene

def render_whitted(scene: Scene, camera: Camera, frame: Frame, out=None, ray_count=None, stream=None):
    """Whitted pass over one tile into device memory (src/main.rs:1090-1104).

    ``out``: torch float32 CUDA tensor of shape (rows, cols, 3) (allocated if None).
    ``ray_count``: torch int64 CUDA tensor with one element that the cast count is added to.
    Stream-ordered on ``stream`` (default: torch's current stream); returns ``out``.
    """
    rows, cols = frame.rows, frame.cols
    out = _new((rows, cols, 3), "float32", "cuda") if out is None else _tensor(out, "out", "float32", None)
    if out.numel() != rows * cols * 3:
        raise ValueError("out must be a contiguous float32 CUDA tensor with rows*cols*3 elements")
    cnt_ptr = _count_ptr(ray_count)
    _capi.check(
        _capi.amd_lib().rt_render_whitted(
            scene._h, C.byref(camera), C.byref(frame), _p(out), cnt_ptr, _stream_ptr(stream)
        )
    )
    return out


def render_whitted_numpy(scene: Scene, camera: Camera, frame: Frame):
    """Host-buffer convenience (rt_render_whitted_host): returns (rgb[rows, cols, 3] float32, casts)."""
    rows, cols = frame.rows, frame.cols
    img = np.empty((rows, cols, 3), dtype=np.float32)
    casts = C.c_ulonglong(0)
    _capi.check(
        _capi.amd_lib().rt_render_whitted_host(scene._h, C.byref(camera), C.byref(frame), img.ctypes.data_as(C.c_void_p), C.byref(casts))
    )
    return img, int(casts.value)

class Rng:
    """Device-resident per-pixel IsaacRng states of one tile (src/main.rs:1117-1127); rt_rng_create/destroy."""

    def __init__(self, frame: Frame):
        self.frame = frame
        self.count = frame.rows * frame.cols
        self._h = C.c_void_p()
        _capi.check(_capi.amd_lib().rt_rng_create(C.byref(frame), C.byref(self._h)))

    @classmethod
    def seeded(cls, seeds) -> "Rng":
        """Generators that belong to no frame (rt_rng_create_seeded): generator i is IsaacRng::new_from_u64(seeds[i]); ``seeds`` is a
        sequence or array of integers below 2^64.  Rng(frame) is the case seeds[p] = y * 2^33 + x in the tile's row order."""
        a = np.ascontiguousarray(np.asarray(seeds, dtype=np.uint64).reshape(-1))
        self = cls.__new__(cls)
        self.frame = None
        self.count = int(a.shape[0])
        self._h = C.c_void_p()
        _capi.check(_capi.amd_lib().rt_rng_create_seeded(a.ctypes.data_as(C.c_void_p), self.count, C.byref(self._h)))
        return self

    def download(self) -> np.ndarray:
        words = _capi.amd_lib().rt_rng_state_words()
        st = np.empty((self.count, words), dtype=np.uint32)
        _capi.check(_capi.amd_lib().rt_rng_download(self._h, st.ctypes.data_as(C.c_void_p)))
        return st

    def upload(self, states) -> None:
        """The inverse of download (rt_rng_upload): (count, rt_rng_state_words) uint32 records in the reference's layout; the next call
        continues exactly from them.  Synchronises."""
        words = _capi.amd_lib().rt_rng_state_words()
        a = np.asarray(states)
        if not (a.dtype == np.uint32 and a.shape == (self.count, words)):
            raise ValueError(f"expected a ({self.count}, {words}) uint32 array")
        a = np.ascontiguousarray(a)
        _capi.check(_capi.amd_lib().rt_rng_upload(self._h, a.ctypes.data_as(C.c_void_p)))

    def close(self) -> None:
        h, self._h = getattr(self, "_h", None), None
        if h:
            _capi.amd_lib().rt_rng_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def render_distributed(scene: Scene, camera: Camera, frame: Frame, rng: Rng, n_epochs: int = 1, focus: float = 3.0,
                       blur: float = 0.04, accum=None, samples=None, valid=None, ray_count=None, stream=None):
    """`n_epochs` passes of the distributed/DoF closure (src/main.rs:1131-1161) over one tile, on the device.

    accum   (rows, cols, 3) f32 CUDA tensor or None: surviving samples are added in epoch order.
    samples (n_epochs, rows, cols, 3) f32 / valid (n_epochs, rows, cols) u8 CUDA tensors or None: raw samples + filter.
    """
    rows, cols = frame.rows, frame.cols
    _tensor(accum, "accum", "float32", (rows, cols, 3), optional=True)
    _tensor(samples, "samples", "float32", (n_epochs, rows, cols, 3), optional=True)
    _tensor(valid, "valid", "uint8", (n_epochs, rows, cols), optional=True)
    _capi.check(
        _capi.amd_lib().rt_render_distributed(scene._h, C.byref(camera), C.byref(frame), float(focus), float(blur), rng._h,
                                              int(n_epochs), _p(accum), _p(samples), _p(valid), _p(ray_count), _stream_ptr(stream))
    )
    return accum if accum is not None else samples


def focus_rays(camera: Camera, frame: Frame, rng: Rng, focus: float = 3.0, blur: float = 0.04, out=None, stream=None):
    """Camera::shoot_focus (src/main.rs:101-127) of every pixel of a frame or tile as an (rows * cols, 11) int32 CUDA tensor of rt_ray
    records in compact row order (rt_focus_rays): the two lens draws come from the pixel's generator in ``rng`` (the frame's Rng, or a
    seeded one of as many generators), which advances — bit for bit the ray render_distributed casts first in that epoch."""
    n = frame.rows * frame.cols
    out = _out_tensor(out, (n, 11), "int32", "cuda")
    _capi.check(_capi.amd_lib().rt_focus_rays(C.byref(camera), C.byref(frame), float(focus), float(blur), rng._h, _p(out),
                                              _stream_ptr(stream)))
    return out

def render_distributed_numpy(scene: Scene, camera: Camera, frame: Frame, rng: Rng, n_epochs: int, img: np.ndarray,
                             focus: float = 3.0, blur: float = 0.04) -> int:
    """`n_epochs` epochs of the stochastic loop added into the host image `img` ((rows, cols, 3) f32, in place):
    rt_render_distributed_host, the form a host-resident `img` binds (src/main.rs:1131-1167).  Returns the cast count."""
    if not (img.dtype == np.float32 and img.flags.c_contiguous and img.shape == (frame.rows, frame.cols, 3)):
        raise ValueError("expected a contiguous (rows, cols, 3) float32 array")
    casts = C.c_ulonglong(0)
    _capi.check(_capi.amd_lib().rt_render_distributed_host(scene._h, C.byref(camera), C.byref(frame), float(focus), float(blur), rng._h,
                                                           int(n_epochs), img.ctypes.data_as(C.c_void_p), C.byref(casts)))
    return int(casts.value)


def set_option(name: str, value=None) -> None:
    """A process-wide switch of librt_amd.so (include/rt_amd.h rt_set_option): an integer named like the environment variable that
    seeds it (the environment is read once per process); None unsets it.  None of them changes a result."""
    _capi.check(_capi.amd_lib().rt_set_option(name.encode(), None if value is None else str(int(value)).encode()))


class options:
    """`with rt.options(RT_AMD_DIST_PIPELINE=0, RT_AMD_DIST_WS_MB=16): ...` — switches set for the block, unset after it."""

    def __init__(self, **switches):
        self._switches = switches

    def __enter__(self):
        for k, v in self._switches.items():
            set_option(k, v)
        return self

    def __exit__(self, *exc):
        for k in self._switches:
            set_option(k, None)
        return False
