"""After the render: post_process, the sRGB encode, the photon accumulator and the PNG writer — on numpy arrays or on the device."""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np

from . import _capi
from ._args import _new, _p, _stream_ptr, _torch

def post_process_device(img, divisor=None, stream=None):
    """In-place p99-luma normalisation of a (rows, cols, 3) f32 CUDA tensor (src/main.rs:748-762), on the device."""
    torch = _torch()
    assert img.is_cuda and img.dtype == torch.float32 and img.is_contiguous() and img.shape[-1] == 3
    _capi.check(_capi.amd_lib().rt_post_process_device(_p(img), img.numel() // 3, _p(divisor), _stream_ptr(stream)))
    return img


def encode_srgb8_device(img, out=None, stream=None):
    """Linear f32 -> sRGB u8 on the device (src/image.rs:55-66)."""
    torch = _torch()
    assert img.is_cuda and img.dtype == torch.float32 and img.is_contiguous()
    out = _new(img.shape, "uint8", img.device) if out is None else out
    _capi.check(_capi.amd_lib().rt_encode_srgb8_device(_p(img), img.numel(), _p(out), _stream_ptr(stream)))
    return out


class PhotonAccumulator:
    """src/photon.rs:9-34 (defined but unused by the reference's main()): per-pixel running sum and weight,
    resolved to sum / weight — a true average over the epochs of the stochastic pass, as the alternative to main()'s
    sum-and-renormalise.  Works on numpy arrays (librt_host.so) or CUDA tensors (librt_amd.so), bit-identically."""

    def __init__(self, rows: int, cols: int, device: str = "cpu"):
        self.rows, self.cols, self.device = rows, cols, device
        if device == "cpu":
            self.sum = np.zeros((rows, cols, 3), dtype=np.float32)
            self.weight = np.zeros((rows, cols), dtype=np.float32)
        else:
            self.sum, self.weight = _new((rows, cols, 3), "float32", device).zero_(), _new((rows, cols), "float32", device).zero_()

    def accumulate(self, samples, valid, stream=None) -> None:
        """accumulate() for every sample whose filter flag is set: samples (n_epochs, rows, cols, 3) f32, valid
        (n_epochs, rows, cols) u8 — the `samples` / `valid` outputs of render_distributed — in epoch order."""
        n_epochs = int(samples.shape[0])
        assert tuple(samples.shape) == (n_epochs, self.rows, self.cols, 3) and tuple(valid.shape) == (n_epochs, self.rows, self.cols)
        n_pixels = self.rows * self.cols
        if self.device == "cpu":
            assert samples.dtype == np.float32 and valid.dtype == np.uint8 and samples.flags.c_contiguous and valid.flags.c_contiguous
            _capi.host_lib().rt_accumulate(samples.ctypes.data_as(C.c_void_p), valid.ctypes.data_as(C.c_void_p), n_epochs, n_pixels,
                                           self.sum.ctypes.data_as(C.c_void_p), self.weight.ctypes.data_as(C.c_void_p))
        else:
            torch = _torch()
            assert samples.is_cuda and samples.dtype == torch.float32 and samples.is_contiguous()
            assert valid.is_cuda and valid.dtype == torch.uint8 and valid.is_contiguous()
            _capi.check(_capi.amd_lib().rt_accumulate_device(_p(samples), _p(valid), n_epochs, n_pixels,
                                                            _p(self.sum), _p(self.weight),
                                                            _stream_ptr(stream)))

    def resolve(self, stream=None):
        """into_rgb_internal: sum / weight, black where nothing was accumulated."""
        n_pixels = self.rows * self.cols
        if self.device == "cpu":
            out = np.empty((self.rows, self.cols, 3), dtype=np.float32)
            _capi.host_lib().rt_accumulator_resolve(self.sum.ctypes.data_as(C.c_void_p), self.weight.ctypes.data_as(C.c_void_p), n_pixels,
                                                    out.ctypes.data_as(C.c_void_p))
            return out
        out = _new((self.rows, self.cols, 3), "float32", self.device)
        _capi.check(_capi.amd_lib().rt_accumulator_resolve_device(_p(self.sum), _p(self.weight), n_pixels,
                                                                 _p(out), _stream_ptr(stream)))
        return out


def post_process(img: np.ndarray) -> float:
    """In-place p99-luma normalisation, src/main.rs:748-762.  Returns the divisor (0 = untouched)."""
    assert img.dtype == np.float32 and img.flags.c_contiguous and img.shape[-1] == 3
    return float(_capi.host_lib().rt_post_process(img.ctypes.data_as(C.c_void_p), img.size // 3))


def luma_row() -> tuple:
    """The three f32 luma weights of post_process: luma = (w0 * r + w1 * g) + w2 * b."""
    row = (C.c_float * 3)()
    _capi.host_lib().rt_luma_row(row)
    return (float(row[0]), float(row[1]), float(row[2]))


def encode_srgb8(img: np.ndarray) -> np.ndarray:
    """Linear f32 -> sRGB u8, src/image.rs:55-66."""
    assert img.dtype == np.float32 and img.flags.c_contiguous
    out = np.empty(img.shape, dtype=np.uint8)
    _capi.host_lib().rt_encode_srgb8(img.ctypes.data_as(C.c_void_p), img.size, out.ctypes.data_as(C.c_void_p))
    return out


def write_to_file(path: str, rgb8: np.ndarray) -> None:
    """RGB8 PNG via a temporary file + rename, src/main.rs:764-776."""
    assert rgb8.dtype == np.uint8 and rgb8.ndim == 3 and rgb8.shape[2] == 3 and rgb8.flags.c_contiguous
    _capi.check_host(_capi.host_lib().rt_write_png(str(Path(path)).encode(), rgb8.ctypes.data_as(C.c_void_p), rgb8.shape[1], rgb8.shape[0]))
