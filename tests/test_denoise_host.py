"""Denoise queries on the host (include/rt_amd.h "denoise queries"): rt_denoise_atrous_cpu of librt_host.so, the CPU definition, held
against a numpy restatement — bit for bit where every exponential is exactly 1, to the derived tolerance of _denoise_support where it
is not — and against the exact consequences of the definition.  The device is held against this CPU form by tests/test_gpu_denoise.py."""
import ctypes as C

import numpy as np
import pytest

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import _capi, denoise
from _denoise_support import (ATOL, F32, FINITE_SIGMAS, IMAGES, INF, LEVELS, RTOL, bits, case_data, embed, exp_unit, level_sigma_color,
                              restate_level, synthetic_regions)

OFF = dict(sigma_color=INF, sigma_normal=INF, sigma_position=INF)
FINITE = dict(sigma_color=FINITE_SIGMAS[0], sigma_normal=FINITE_SIGMAS[1], sigma_position=FINITE_SIGMAS[2])


@pytest.mark.parametrize("with_valid", [False, True])
@pytest.mark.parametrize("rows,cols", IMAGES)
def test_stencil_is_the_restated_b3_spline_bit_for_bit(rows, cols, with_valid):
    color, normal, position, _, valid = case_data(rows, cols)
    flags = valid if with_valid else None
    for level in LEVELS:  # steps up to 32: larger than every image here on at least one axis
        got = denoise.atrous_numpy(color, rows, cols, normal=normal, position=position, valid=flags, levels=1, first_level=level, **OFF)
        want = restate_level(color, rows, cols, level, (INF, INF, INF), normal, position, flags, exp=exp_unit)
        assert np.array_equal(bits(got.reshape(-1, 3)), bits(want)), level


@pytest.mark.parametrize("rows,cols", IMAGES)
def test_weights_level_by_level_to_the_derived_tolerance(rows, cols):
    color, normal, position, _, valid = case_data(rows, cols)
    image = color
    for level in LEVELS:  # the input of level l is the CPU form's own output of level l - 1: nothing compounds
        got = denoise.atrous_numpy(image, rows, cols, normal=normal, position=position, valid=valid, levels=1, first_level=level, **FINITE).reshape(-1, 3)
        want = restate_level(image, rows, cols, level, FINITE_SIGMAS, normal, position, valid)
        assert (image >= 0).all() and image.max() < 4.0
        assert np.allclose(got, want, rtol=RTOL, atol=ATOL), (level, np.abs(got - want).max())
        image = got


@pytest.mark.parametrize("value", [1.0, 0.5])
def test_a_constant_image_returns_itself(value):
    rows, cols = 23, 37
    _, normal, position, _, valid = case_data(rows, cols)
    image = np.full((rows * cols, 3), value, dtype=F32)
    got = denoise.atrous_numpy(image, rows, cols, normal=normal, position=position, valid=valid, levels=6, **FINITE)
    assert np.array_equal(bits(got.reshape(-1, 3)), bits(image))


def test_invalid_pixels_pass_through_and_contribute_nothing():
    rows, cols = 23, 37
    color, normal, position, albedo, valid = case_data(rows, cols)
    kw = dict(normal=normal, position=position, albedo=albedo, valid=valid, levels=4, demodulate=True, **FINITE)
    got = denoise.atrous_numpy(color, rows, cols, **kw).reshape(-1, 3)
    off = valid == 0
    assert off.any() and np.array_equal(bits(got[off]), bits(color[off]))
    other = color.copy()
    other[off] = np.random.default_rng(1).random((int(off.sum()), 3), dtype=F32) * F32(100.0)
    other[np.flatnonzero(off)[::3], 1] = np.nan
    again = denoise.atrous_numpy(other, rows, cols, **kw).reshape(-1, 3)
    assert np.array_equal(bits(again[~off]), bits(got[~off])) and np.array_equal(bits(again[off]), bits(other[off]))


def test_a_valid_nan_pixel_passes_through_like_an_invalid_one():
    rows, cols = 23, 37
    color, normal, position, _, valid = case_data(rows, cols)
    color, valid = color.copy(), valid.copy()
    q = 11 * cols + 18
    valid[q] = 1
    color[q, 1] = np.nan
    kw = dict(normal=normal, position=position, levels=3, **FINITE)
    got = denoise.atrous_numpy(color, rows, cols, valid=valid, **kw).reshape(-1, 3)
    assert np.array_equal(bits(got[q]), bits(color[q]))
    valid[q] = 0
    marked = denoise.atrous_numpy(color, rows, cols, valid=valid, **kw).reshape(-1, 3)
    assert np.array_equal(bits(got), bits(marked)) and not np.isnan(np.delete(got, q, axis=0)).any()


def test_no_leak_across_a_hard_edge():
    rows, cols = 24, 40
    left = (np.arange(rows * cols) % cols) < cols // 2
    image = np.where(left[:, None], F32(2.0), F32(0.25)).astype(F32).repeat(3, axis=1)
    normal = np.where(left[:, None], np.array([1, 0, 0], dtype=F32), np.array([0, 1, 0], dtype=F32)).astype(F32)
    got = denoise.atrous_numpy(image, rows, cols, normal=normal, levels=6, sigma_color=INF, sigma_normal=0.1, sigma_position=INF)
    assert np.array_equal(bits(got.reshape(-1, 3)), bits(image))  # x = 2 / 0.1^2 = 200 > 100: cross-edge weights are +0


@pytest.mark.parametrize("demodulate", [False, True])
def test_strided_guides_equal_compact_guides(demodulate):
    rows, cols = 23, 37
    color, normal, position, albedo, valid = case_data(rows, cols)
    _, _, (s_normal, s_position, s_albedo, s_valid) = embed(normal, position, albedo, valid)
    assert s_normal.strides == (72, 4) and s_position.strides == (52, 4) and s_valid.strides == (72,)
    kw = dict(levels=3, first_level=1, demodulate=demodulate, **FINITE)
    compact = denoise.atrous_numpy(color, rows, cols, normal=normal, position=position, albedo=albedo, valid=valid, **kw)
    strided = denoise.atrous_numpy(color, rows, cols, normal=s_normal, position=s_position, albedo=s_albedo, valid=s_valid, **kw)
    assert np.array_equal(bits(compact), bits(strided))
    shaped = denoise.atrous_numpy(color.reshape(rows, cols, 3), rows, cols, normal=s_normal.reshape(rows, cols, 3), position=s_position,
                                  albedo=albedo.reshape(rows, cols, 3), valid=s_valid.reshape(rows, cols), **kw)
    assert np.array_equal(bits(compact), bits(shaped))


@pytest.mark.parametrize("demodulate", [False, True])
def test_one_call_of_n_levels_is_n_calls_of_one(demodulate):
    """as include/rt_amd.h says a caller does it: level j with first_level + j, sigma_color * 2^-j, and the demodulation bits on the
    first (IN, 1) and the last (OUT, 2) call only"""
    rows, cols, first, n = 23, 37, 1, 4
    color, normal, position, albedo, valid = case_data(rows, cols)
    guides = dict(normal=normal, position=position, albedo=albedo, valid=valid, sigma_normal=FINITE_SIGMAS[1], sigma_position=FINITE_SIGMAS[2])
    once = denoise.atrous_numpy(color, rows, cols, levels=n, first_level=first, sigma_color=FINITE_SIGMAS[0], demodulate=demodulate, **guides)
    image = color
    for j in range(n):
        flags = ((1 if j == 0 else 0) | (2 if j == n - 1 else 0)) if demodulate else 0
        image = denoise.atrous_numpy(image, rows, cols, levels=1, first_level=first + j, sigma_color=float(level_sigma_color(FINITE_SIGMAS[0], j)),
                                     demodulate=flags, **guides)
    assert np.array_equal(bits(once), bits(image))
    assert (bits(once) != bits(color.reshape(rows, cols, 3))).any()


def test_it_denoises():
    """four constant regions plus Gaussian noise, five levels, the default sigmas: strictly closer to the clean image than the input
    (the measured ratio is in DESIGN.md 3.21; no ratio is asserted)"""
    clean, noisy, normal, position = synthetic_regions()
    got = denoise.atrous_numpy(noisy, 64, 64, normal=normal, position=position, levels=5).reshape(-1, 3)
    before = float(((noisy.astype(np.float64) - clean) ** 2).mean())
    after = float(((got.astype(np.float64) - clean) ** 2).mean())
    print(f"denoise: mse noisy {before:.6g} -> filtered {after:.6g}, ratio {after / before:.4f}")
    assert after < before


# ---- refusals: the one check of rt_denoise.h behind the CPU form and, before any device work, both entry points of librt_amd.so ----

def _call(entry, color, g, p, rows, cols, out, temp):
    if entry == "cpu":
        lib = _capi.host_lib()
        return lib.rt_denoise_atrous_cpu(color, C.byref(g) if g else None, C.byref(p) if p else None, rows, cols, out, temp), lib.rt_host_last_error().decode()
    lib = _capi.amd_lib()
    if entry == "device":
        return lib.rt_denoise_atrous(color, C.byref(g) if g else None, C.byref(p) if p else None, rows, cols, out, temp, None), lib.rt_last_error().decode()
    return lib.rt_denoise_atrous_host(color, C.byref(g) if g else None, C.byref(p) if p else None, rows, cols, out), lib.rt_last_error().decode()


def _good():
    return _capi.DenoiseGuides(), _capi.DenoiseParams(1.0, 1.0, 1.0, 0, 2, 0)


A, B, T = C.c_void_p(4096), C.c_void_p(8192), C.c_void_p(12288)  # never dereferenced: every call below is refused on its arguments


def _cases():
    def params(**kw):
        g, p = _good()
        for k, v in kw.items():
            setattr(p, k, v)
        return g, p

    def guides(**kw):
        g, p = _good()
        for k, v in kw.items():
            setattr(g, k, v)
        return g, p

    yield "null color", (None, *_good(), 4, 4, B, T), "color"
    yield "null out", (A, *_good(), 4, 4, None, T), "out"
    yield "null guides", (A, None, _good()[1], 4, 4, B, T), "guides"
    yield "null params", (A, _good()[0], None, 4, 4, B, T), "params"
    yield "2^32 pixels", (A, *_good(), 1 << 16, 1 << 16, B, T), "rows * cols"
    yield "too many levels", (A, *params(first_level=3, n_levels=4), 4, 4, B, T), "first_level + n_levels"
    yield "first level 6", (A, *params(first_level=6, n_levels=1), 4, 4, B, T), "first_level + n_levels"
    yield "no level", (A, *params(n_levels=0), 4, 4, B, T), "n_levels"
    yield "zero sigma", (A, *params(sigma_color=0.0), 4, 4, B, T), "sigma_color"
    yield "negative sigma", (A, *params(sigma_normal=-1.0), 4, 4, B, T), "sigma_normal"
    yield "nan sigma", (A, *params(sigma_position=float("nan")), 4, 4, B, T), "sigma_position"
    yield "unknown flag", (A, *params(flags=4), 4, 4, B, T), "flags"
    yield "demodulation without albedo", (A, *params(flags=3), 4, 4, B, T), "albedo"
    yield "normal stride", (A, *guides(normal=4096, normal_stride=2), 4, 4, B, T), "normal_stride"
    yield "position stride", (A, *guides(position=4096, position_stride=0), 4, 4, B, T), "position_stride"
    yield "albedo stride", (A, *guides(albedo=4096, albedo_stride=1), 4, 4, B, T), "albedo_stride"
    yield "valid stride", (A, *guides(valid=4096, valid_stride=0), 4, 4, B, T), "valid_stride"
    yield "out is color", (A, *_good(), 4, 4, A, T), "out"
    yield "null temp", (A, *_good(), 4, 4, B, None), "temp"
    yield "temp is color", (A, *_good(), 4, 4, B, A), "temp"
    yield "temp is out", (A, *_good(), 4, 4, B, B), "temp"


CASES = list(_cases())


# rt_denoise_atrous_host takes no temp: the round trip makes its own
ENTRY_CASES = [(e, c) for e in ("cpu", "device", "host") for c in CASES if not (e == "host" and "temp" in c[0])]


@pytest.mark.parametrize("entry,case", ENTRY_CASES, ids=[f"{e}-{c[0]}" for e, c in ENTRY_CASES])
def test_refusals_return_a_status_and_name_the_argument(entry, case):
    name, args, word = case
    status, text = _call(entry, *args)
    who = {"cpu": "rt_denoise_atrous_cpu", "device": "rt_denoise_atrous", "host": "rt_denoise_atrous_host"}[entry]
    assert status == -1 and text.startswith(who + ": ") and word in text, (status, text)


def test_an_empty_image_is_ok_and_the_wrappers_raise():
    g, p = _good()
    for entry in ("cpu", "device", "host"):
        assert _call(entry, None, g, p, 0, 7, None, None)[0] == 0
    color, normal, _, _, _ = case_data(23, 37)
    with pytest.raises(rt.RtError, match="first_level"):
        denoise.atrous_numpy(color, 23, 37, levels=7)
    with pytest.raises(rt.RtError, match="sigma_color"):
        denoise.atrous_numpy(color, 23, 37, sigma_color=0.0)
    with pytest.raises(rt.RtError, match="albedo"):
        denoise.atrous_numpy(color, 23, 37, demodulate=True)
    with pytest.raises(ValueError, match="normal"):
        denoise.atrous_numpy(color, 23, 37, normal=normal[:, :2])
    with pytest.raises(ValueError, match="normal"):
        denoise.atrous_numpy(color, 23, 37, normal=np.asfortranarray(normal))
    with pytest.raises(ValueError, match="color"):
        denoise.atrous_numpy(color.astype(np.float64), 23, 37)
    assert denoise.temp_bytes(23, 37) == 23 * 37 * 12
