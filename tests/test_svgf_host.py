"""Variance-guided filter queries on the host (include/rt_amd.h "variance-guided filter queries"): rt_svgf_variance_cpu and
rt_svgf_atrous_cpu of librt_host.so, the CPU definition, held against the numpy restatement of _svgf_support — bit for bit where every
exponential is exactly 1, to the derived tolerances where it is not — and against the exact consequences of the definition.  The device
is held against these CPU forms by tests/test_gpu_svgf.py."""
import ctypes as C

import numpy as np
import pytest

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import _capi, denoise, svgf, temporal
import _temporal_support
from _denoise_support import embed, synthetic_regions
from _svgf_support import (ATROUS_ATOL, ATROUS_RTOL, ESTIMATE_ATOL, F32, FINITE_SIGMAS, HISTORY, IMAGES, INF, LEVELS, MIN_LENGTH, VARIANCE_ATOL,
                           VARIANCE_RTOL, bits, case_data, exp_unit, restate_level, restate_variance, vpos)

OFF = dict(sigma_luminance=INF, sigma_normal=INF, sigma_position=INF)
FINITE = dict(sigma_luminance=FINITE_SIGMAS[0], sigma_normal=FINITE_SIGMAS[1], sigma_position=FINITE_SIGMAS[2])
GUIDE_SIGMAS = dict(sigma_normal=FINITE_SIGMAS[1], sigma_position=FINITE_SIGMAS[2])


def same(a, b):
    return np.array_equal(bits(np.asarray(a).reshape(-1)), bits(np.asarray(b).reshape(-1)))


# ---- rt_svgf_variance_cpu ----

@pytest.mark.parametrize("with_valid", [False, True])
@pytest.mark.parametrize("rows,cols", IMAGES)
def test_variance_is_the_restatement_bit_for_bit_without_guides(rows, cols, with_valid):
    _, _, history, _, _, _, valid = case_data(rows, cols)
    flags = valid if with_valid else None
    for min_length in (1, 2, MIN_LENGTH, 7):
        got = svgf.variance_numpy(history, rows, cols, valid=flags, min_length=min_length)
        want = restate_variance(history, rows, cols, valid=flags, min_length=min_length, exp=exp_unit)
        assert same(got, want), min_length
    lengths = history["length"][valid != 0] if with_valid else history["length"]
    assert rows * cols < 7 or {0, 1, MIN_LENGTH - 1, MIN_LENGTH} <= set(history["length"].tolist()) and (lengths < MIN_LENGTH).any()


@pytest.mark.parametrize("rows,cols", IMAGES)
def test_variance_with_guides_bit_for_bit_when_every_exponent_is_zero(rows, cols):
    _, _, history, normal, position, _, valid = case_data(rows, cols)
    got = svgf.variance_numpy(history, rows, cols, normal=normal, position=position, valid=valid, sigma_normal=INF, sigma_position=INF)
    want = restate_variance(history, rows, cols, normal, position, valid, exp=exp_unit)
    assert same(got, want)


@pytest.mark.parametrize("rows,cols", IMAGES)
def test_variance_weights_to_the_derived_tolerance_and_through_record_strides(rows, cols):
    _, _, history, normal, position, albedo, valid = case_data(rows, cols)
    got = svgf.variance_numpy(history, rows, cols, normal=normal, position=position, valid=valid, **GUIDE_SIGMAS).reshape(-1)
    want = restate_variance(history, rows, cols, normal, position, valid, sigmas=FINITE_SIGMAS[1:])
    worst = float(np.abs(got - want).max())
    print(f"svgf variance {rows} x {cols}: largest difference {worst:.3g} (bound {ESTIMATE_ATOL:.3g})")
    assert np.allclose(got, want, rtol=0.0, atol=ESTIMATE_ATOL), worst
    _, _, (s_normal, s_position, _, s_valid) = embed(normal, position, albedo, valid)
    assert s_normal.strides == (72, 4) and s_position.strides == (52, 4) and s_valid.strides == (72,)
    strided = svgf.variance_numpy(history, rows, cols, normal=s_normal, position=s_position, valid=s_valid, **GUIDE_SIGMAS)
    assert same(strided, got)


def test_min_length_1_is_the_temporal_variance_plane():
    rows, cols = 33, 65
    color, history, cur, prev = _temporal_support.case_data(rows, cols)
    guides = lambda p: temporal.Guides(p.normal, p.position, p.object, p.valid)
    records, plane = temporal.accumulate_numpy(color, _temporal_support.motion_field(rows, cols, "fractional"), rows, cols, history, guides(cur), guides(prev),
                                               **_temporal_support.PARAMS)
    assert (records["length"] > 1).any() and (records["length"] == 1).any() and (plane > 0).any()
    # every record accumulate writes has length >= 1; the valid plane is left out because accumulate writes a variance for invalid pixels too
    got = svgf.variance_numpy(records, rows, cols, normal=cur.normal, position=cur.position, min_length=1, **GUIDE_SIGMAS)
    assert same(got, plane)


def test_long_histories_do_not_look_at_the_guides():
    rows, cols = 23, 37
    _, _, history, normal, position, _, valid = case_data(rows, cols)
    plain = svgf.variance_numpy(history, rows, cols, valid=valid).reshape(-1)
    guided = svgf.variance_numpy(history, rows, cols, normal=normal, position=position, valid=valid, **GUIDE_SIGMAS).reshape(-1)
    nans = svgf.variance_numpy(history, rows, cols, normal=np.full_like(normal, np.nan), position=position, valid=valid, **GUIDE_SIGMAS).reshape(-1)
    long = (history["length"] >= MIN_LENGTH) & (valid != 0)
    short = (history["length"] > 0) & (history["length"] < MIN_LENGTH) & (valid != 0)
    t = history["moment2"] - history["moment1"] * history["moment1"]
    assert long.any() and same(plain[long], guided[long]) and same(plain[long], nans[long]) and same(plain[long], np.where(t > 0, t, F32(0))[long])
    assert (bits(plain[short]) != bits(guided[short])).any() and not nans[short].any()  # a NaN exponent skips every tap: wsum = 0 writes +0
    assert not plain[valid == 0].any() and not plain[history["length"] == 0].any()


# ---- rt_svgf_atrous_cpu ----

def guides_of(rows, cols, strided=False, flags=True):
    _, _, _, normal, position, albedo, valid = case_data(rows, cols)
    if strided:
        normal, position, albedo, valid = embed(normal, position, albedo, valid)[2]
    return dict(normal=normal, position=position, albedo=albedo, valid=valid if flags else None)


@pytest.mark.parametrize("with_valid", [False, True])
@pytest.mark.parametrize("rows,cols", IMAGES)
def test_atrous_is_the_restatement_bit_for_bit_when_every_exponent_is_zero(rows, cols, with_valid):
    color, variance, _, _, _, _, _ = case_data(rows, cols)
    g = guides_of(rows, cols, flags=with_valid)
    plain = dict(normal=g["normal"], position=g["position"], valid=g["valid"])
    chain_c, chain_v = color, variance
    for level in LEVELS:  # each level alone, and the chain of restated levels for the call of all six below
        got_c, got_v = svgf.atrous_numpy(color, variance, rows, cols, levels=1, first_level=level, **g, **OFF)
        want_c, want_v = restate_level(color, variance, rows, cols, level, (INF, INF, INF), exp=exp_unit, **plain)
        assert same(got_c, want_c) and same(got_v, want_v), level
        chain_c, chain_v = restate_level(chain_c, chain_v, rows, cols, level, (INF, INF, INF), exp=exp_unit, **plain)
    got_c, got_v = svgf.atrous_numpy(color, variance, rows, cols, levels=6, **g, **OFF)
    assert same(got_c, chain_c) and same(got_v, chain_v)


@pytest.mark.parametrize("demodulate", [False, True])
@pytest.mark.parametrize("rows,cols", IMAGES)
def test_atrous_weights_level_by_level_to_the_derived_tolerance(rows, cols, demodulate):
    color, variance, history, normal, position, albedo, valid = case_data(rows, cols)
    g = guides_of(rows, cols)
    image, var = color, variance
    for level in LEVELS:  # the input of level l is the CPU form's own output of level l - 1: nothing compounds
        got_c, got_v = svgf.atrous_numpy(image, var, rows, cols, levels=1, first_level=level, demodulate=demodulate, **g, **FINITE)
        want_c, want_v = restate_level(image, var, rows, cols, level, FINITE_SIGMAS, normal, position, albedo, valid, demodulate, demodulate)
        got_c, got_v = got_c.reshape(-1, 3), got_v.reshape(-1)
        seen = image / (albedo + F32(1e-3)) if demodulate else image  # what the derivation asks of the inputs
        assert np.nanmin(seen) >= 0 and np.nanmax(seen) < 40.0 and np.nanmax(vpos(var)) < 2.0
        assert np.array_equal(np.isnan(got_c), np.isnan(want_c)) and np.array_equal(np.isnan(got_v), np.isnan(want_v))
        dc, dv = float(np.nanmax(np.abs(got_c - want_c))), float(np.nanmax(np.abs(got_v - want_v)))
        print(f"svgf atrous {rows} x {cols} level {level}: largest differences colour {dc:.3g}, variance {dv:.3g}")
        assert np.allclose(got_c, want_c, rtol=ATROUS_RTOL, atol=ATROUS_ATOL, equal_nan=True), (level, dc)
        assert np.allclose(got_v, want_v, rtol=VARIANCE_RTOL, atol=VARIANCE_ATOL, equal_nan=True), (level, dv)
        image, var = got_c, got_v
    # the colour where it lies in the records, stride 8, gives the bits of the compact plane
    compact = svgf.atrous_numpy(color, variance, rows, cols, levels=3, first_level=1, demodulate=demodulate, **g, **FINITE)
    inside = svgf.atrous_numpy(history["color"], variance, rows, cols, levels=3, first_level=1, demodulate=demodulate, **g, **FINITE)
    assert history["color"].strides == (32, 4) and same(compact[0], inside[0]) and same(compact[1], inside[1])


@pytest.mark.parametrize("demodulate", [False, True])
def test_strided_guides_equal_compact_guides(demodulate):
    rows, cols = 23, 37
    color, variance, _, _, _, _, _ = case_data(rows, cols)
    kw = dict(levels=3, first_level=1, demodulate=demodulate, **FINITE)
    compact = svgf.atrous_numpy(color, variance, rows, cols, **guides_of(rows, cols), **kw)
    strided = svgf.atrous_numpy(color, variance, rows, cols, **guides_of(rows, cols, strided=True), **kw)
    assert same(compact[0], strided[0]) and same(compact[1], strided[1])


@pytest.mark.parametrize("variance_out", [True, False])
@pytest.mark.parametrize("demodulate", [False, True])
def test_one_call_of_n_levels_is_n_chained_calls_of_one(demodulate, variance_out):
    """level j with first_level + j and the demodulation bits on the first (IN, 1) and the last (OUT, 2) call only; without
    variance_out the call of n levels keeps its variance in the scratch and the colour must not change"""
    rows, cols, first = 23, 37, 1
    color, variance, _, _, _, _, _ = case_data(rows, cols)
    g = guides_of(rows, cols)
    for n in (2, 3, 4):
        once = svgf.atrous_numpy(color, variance, rows, cols, levels=n, first_level=first, demodulate=demodulate, variance_out=variance_out, **g, **FINITE)
        image, var = color, variance
        for j in range(n):
            flags = ((1 if j == 0 else 0) | (2 if j == n - 1 else 0)) if demodulate else 0
            image, var = svgf.atrous_numpy(image, var, rows, cols, levels=1, first_level=first + j, demodulate=flags, **g, **FINITE)
        assert same(once[0], image), n
        assert same(once[1], var) if variance_out else once[1] is None, n
        assert (bits(once[0]) != bits(color.reshape(rows, cols, 3))).any()


@pytest.mark.parametrize("config", [dict(strided=False, flags=True, demodulate=False), dict(strided=True, flags=True, demodulate=True),
                                    dict(strided=False, flags=False, demodulate=True), dict(strided=True, flags=False, demodulate=False)])
@pytest.mark.parametrize("rows,cols", IMAGES)
def test_an_infinite_luminance_sigma_gives_the_bits_of_the_denoise_filter(rows, cols, config):
    color, variance, _, _, _, _, _ = case_data(rows, cols)  # finite or NaN colours
    g = guides_of(rows, cols, config["strided"], config["flags"])
    kw = dict(levels=6, demodulate=config["demodulate"], sigma_normal=FINITE_SIGMAS[1], sigma_position=FINITE_SIGMAS[2])
    got, _ = svgf.atrous_numpy(color, variance, rows, cols, sigma_luminance=INF, **g, **kw)
    want = denoise.atrous_numpy(color, rows, cols, sigma_color=INF, **g, **kw)
    assert same(got, want) and np.isnan(got).any()


def test_inputs_are_never_written():
    rows, cols = 23, 37
    color, variance, history, normal, position, albedo, valid = (np.array(a) for a in case_data(rows, cols))
    keep = [a.copy() for a in (color, variance, history, normal, position, albedo, valid)]
    svgf.variance_numpy(history, rows, cols, normal=normal, position=position, valid=valid, **GUIDE_SIGMAS)
    svgf.atrous_numpy(color, variance, rows, cols, normal=normal, position=position, albedo=albedo, valid=valid, levels=5, demodulate=True, **FINITE)
    svgf.atrous_numpy(history["color"], variance, rows, cols, valid=valid, levels=2, **FINITE)
    for now, before in zip((color, variance, history, normal, position, albedo, valid), keep):
        assert now.tobytes() == before.tobytes()


def test_invalid_pixels_pass_through_payload_and_all_and_contribute_nothing():
    rows, cols = 23, 37
    color, variance, _, _, _, _, valid = case_data(rows, cols)
    color, variance = color.copy(), variance.copy()
    off = valid == 0
    first = np.flatnonzero(off)[:3]
    color.view(np.uint32)[first[0], 1] = 0x7FC12345  # NaN payloads, a negative variance and -0 on invalid pixels
    variance.view(np.uint32)[first[1]] = 0xFFC00077
    variance[first[2]] = -0.0
    kw = dict(levels=4, demodulate=True, **guides_of(rows, cols), **FINITE)
    got_c, got_v = (a.reshape(rows * cols, -1) for a in svgf.atrous_numpy(color, variance, rows, cols, **kw))
    assert off.any() and same(got_c[off], color[off]) and same(got_v[off], variance[off])
    other_c, other_v = color.copy(), variance.copy()
    other_c[off] = np.random.default_rng(1).random((int(off.sum()), 3), dtype=F32) * F32(100.0)
    other_v[off] = 1e6
    again_c, again_v = (a.reshape(rows * cols, -1) for a in svgf.atrous_numpy(other_c, other_v, rows, cols, **kw))
    assert same(again_c[~off], got_c[~off]) and same(again_v[~off], got_v[~off]) and same(again_c[off], other_c[off])


def test_zero_variance_keeps_a_pixel():
    """a variance plane of +0 gives sl = sigma_luminance * 1e-6 = 4e-6: with neighbouring luminances more than 1e-3 apart every tap but
    the centre has x > 100 and weight +0, so a valid pixel's colour comes back within one product and one divide rounding of the centre
    tap, 2u = 2^-23 relative; the test allows 2^-22"""
    rows, cols = 23, 37
    _, _, _, normal, position, _, valid = case_data(rows, cols)
    i = np.arange(rows * cols)
    base = (F32(0.5) + (((i // cols) * 7 + (i % cols) * 3) % 64).astype(F32) * F32(0.02)).astype(F32)  # neighbours in the 5 x 5 differ by >= 0.02
    color = np.stack([base, base * F32(1.25), base * F32(0.75)], axis=1).astype(F32)
    lum = _temporal_support.luminance(color).reshape(rows, cols)
    for dr in range(-2, 3):
        for dc in range(-2, 3):
            if (dr, dc) != (0, 0):
                a, b = lum[max(dr, 0):rows + min(dr, 0), max(dc, 0):cols + min(dc, 0)], lum[max(-dr, 0):rows + min(-dr, 0), max(-dc, 0):cols + min(-dc, 0)]
                assert np.abs(a - b).min() > 1e-3
    got, var = svgf.atrous_numpy(color, np.zeros(rows * cols, dtype=F32), rows, cols, normal=normal, position=position, valid=valid, levels=1,
                                 sigma_luminance=svgf.SIGMA_LUMINANCE)
    got = got.reshape(-1, 3)
    ok = valid != 0
    assert np.abs(got[ok] / color[ok] - 1).max() <= 2.0 ** -22 and not var.reshape(-1)[ok].any()
    assert same(got[~ok], color[~ok])


def noise_sequence():
    """synthetic_regions (64 x 64, sigma 0.2) as three frames of fresh noise on one clean image, accumulated with integer motion (every
    pixel reprojects onto itself) -> (clean, records, normal, position)"""
    clean, _, normal, position = synthetic_regions()
    n = 64 * 64
    r, c = np.meshgrid(np.arange(64), np.arange(64), indexing="ij")
    motion = np.stack([c.reshape(-1), r.reshape(-1)], axis=1).astype(F32)
    g = np.random.default_rng(17)
    guides = temporal.Guides(normal=normal, position=position)
    records = np.zeros(n, dtype=HISTORY)
    for _ in range(3):
        noisy = (clean + g.normal(0.0, 0.2, clean.shape).astype(F32)).astype(F32)
        records, _ = temporal.accumulate_numpy(noisy, motion, 64, 64, records, guides, guides)
    return clean, records.reshape(-1), normal, position


def test_it_denoises_the_accumulated_image():
    """three accumulated frames (lengths 3 < MIN_LENGTH: the spatial estimate), then five levels at the default sigmas: strictly closer to
    the clean image than the accumulated one (the measured values are in DESIGN.md 3.23; no ratio is asserted)"""
    clean, records, normal, position = noise_sequence()
    assert (records["length"] == 3).all()
    variance = svgf.variance_numpy(records, 64, 64, normal=normal, position=position)
    got, _ = svgf.atrous_numpy(records["color"], variance, 64, 64, normal=normal, position=position, levels=5)
    before = float(((records["color"].astype(np.float64) - clean) ** 2).mean())
    after = float(((got.reshape(-1, 3).astype(np.float64) - clean) ** 2).mean())
    print(f"svgf: mse accumulated {before:.6g} -> filtered {after:.6g}, ratio {after / before:.4f}; mean variance {float(variance.mean()):.6g}")
    assert (variance > 0).all() and after < before


# ---- refusals: the one check per call of rt_svgf.h behind the CPU form and, before any device work, both entry points of librt_amd.so ----

A, B, V, W, T, H8 = (C.c_void_p(4096 * k) for k in range(1, 7))  # never dereferenced: every call below is refused on its arguments


def _ref(x):
    return C.byref(x) if x is not None else None


def _call_atrous(entry, color, stride, variance, g, p, rows, cols, out, variance_out, temp):
    if entry == "cpu":
        lib = _capi.host_lib()
        return lib.rt_svgf_atrous_cpu(color, stride, variance, _ref(g), _ref(p), rows, cols, out, variance_out, temp), lib.rt_host_last_error().decode()
    lib = _capi.amd_lib()
    if entry == "device":
        return lib.rt_svgf_atrous(color, stride, variance, _ref(g), _ref(p), rows, cols, out, variance_out, temp, None), lib.rt_last_error().decode()
    return lib.rt_svgf_atrous_host(color, stride, variance, _ref(g), _ref(p), rows, cols, out, variance_out), lib.rt_last_error().decode()


def _call_variance(entry, history, g, p, rows, cols, out):
    if entry == "cpu":
        lib = _capi.host_lib()
        return lib.rt_svgf_variance_cpu(history, _ref(g), _ref(p), rows, cols, out), lib.rt_host_last_error().decode()
    lib = _capi.amd_lib()
    if entry == "device":
        return lib.rt_svgf_variance(history, _ref(g), _ref(p), rows, cols, out, None), lib.rt_last_error().decode()
    return lib.rt_svgf_variance_host(history, _ref(g), _ref(p), rows, cols, out), lib.rt_last_error().decode()


def _atrous_cases():
    def good(params=(), guides=()):
        g, p = _capi.DenoiseGuides(), _capi.SvgfAtrousParams(1.0, 1.0, 1.0, 0, 3, 0)
        for k, v in dict(params).items():
            setattr(p, k, v)
        for k, v in dict(guides).items():
            setattr(g, k, v)
        return g, p

    yield "null guides", (A, 3, V, None, good()[1], 4, 4, B, W, T), "guides"
    yield "null params", (A, 3, V, good()[0], None, 4, 4, B, W, T), "params"
    yield "2^32 pixels", (A, 3, V, *good(), 1 << 16, 1 << 16, B, W, T), "rows * cols"
    yield "no level", (A, 3, V, *good(dict(n_levels=0)), 4, 4, B, W, T), "n_levels"
    yield "too many levels", (A, 3, V, *good(dict(first_level=3, n_levels=4)), 4, 4, B, W, T), "first_level + n_levels"
    yield "zero sigma", (A, 3, V, *good(dict(sigma_luminance=0.0)), 4, 4, B, W, T), "sigma_luminance"
    yield "negative sigma", (A, 3, V, *good(dict(sigma_normal=-1.0)), 4, 4, B, W, T), "sigma_normal"
    yield "nan sigma", (A, 3, V, *good(dict(sigma_position=float("nan"))), 4, 4, B, W, T), "sigma_position"
    yield "unknown flag", (A, 3, V, *good(dict(flags=4)), 4, 4, B, W, T), "flags"
    yield "demodulation without albedo", (A, 3, V, *good(dict(flags=1)), 4, 4, B, W, T), "albedo"
    yield "color stride", (A, 2, V, *good(), 4, 4, B, W, T), "color_stride"
    yield "normal stride", (A, 3, V, *good(guides=dict(normal=4096, normal_stride=2)), 4, 4, B, W, T), "normal_stride"
    yield "position stride", (A, 3, V, *good(guides=dict(position=4096, position_stride=0)), 4, 4, B, W, T), "position_stride"
    yield "albedo stride", (A, 3, V, *good(guides=dict(albedo=4096, albedo_stride=1)), 4, 4, B, W, T), "albedo_stride"
    yield "valid stride", (A, 3, V, *good(guides=dict(valid=4096, valid_stride=0)), 4, 4, B, W, T), "valid_stride"
    yield "null color", (None, 3, V, *good(), 4, 4, B, W, T), "color"
    yield "null variance", (A, 3, None, *good(), 4, 4, B, W, T), "variance"
    yield "null out", (A, 3, V, *good(), 4, 4, None, W, T), "out"
    yield "out is color", (A, 3, V, *good(), 4, 4, A, W, T), "out must not be"
    yield "out is variance", (A, 3, V, *good(), 4, 4, V, W, T), "out must not be"
    yield "variance_out is variance", (A, 3, V, *good(), 4, 4, B, V, T), "variance_out must not be"
    yield "variance_out is out", (A, 3, V, *good(), 4, 4, B, B, T), "variance_out must not be"
    yield "null temp", (A, 3, V, *good(), 4, 4, B, W, None), "temp"
    yield "temp is color", (A, 3, V, *good(), 4, 4, B, W, A), "temp must not be"
    yield "temp is out", (A, 3, V, *good(), 4, 4, B, W, B), "temp must not be"
    yield "temp is variance_out", (A, 3, V, *good(), 4, 4, B, W, W), "temp must not be"


def _variance_cases():
    def good(params=(), guides=()):
        g, p = _capi.DenoiseGuides(), _capi.SvgfVarianceParams(1.0, 1.0, 4, 0)
        for k, v in dict(params).items():
            setattr(p, k, v)
        for k, v in dict(guides).items():
            setattr(g, k, v)
        return g, p

    yield "null guides", (H8, None, good()[1], 4, 4, W), "guides"
    yield "null params", (H8, good()[0], None, 4, 4, W), "params"
    yield "2^32 pixels", (H8, *good(), 1 << 16, 1 << 16, W), "rows * cols"
    yield "zero sigma", (H8, *good(dict(sigma_normal=0.0)), 4, 4, W), "sigma_normal"
    yield "nan sigma", (H8, *good(dict(sigma_position=float("nan"))), 4, 4, W), "sigma_position"
    yield "min_length 0", (H8, *good(dict(min_length=0)), 4, 4, W), "min_length"
    yield "flags", (H8, *good(dict(flags=1)), 4, 4, W), "flags"
    yield "normal stride", (H8, *good(guides=dict(normal=4096, normal_stride=2)), 4, 4, W), "normal_stride"
    yield "valid stride", (H8, *good(guides=dict(valid=4096, valid_stride=0)), 4, 4, W), "valid_stride"
    yield "null history", (None, *good(), 4, 4, W), "history"
    yield "null variance_out", (H8, *good(), 4, 4, None), "variance_out"
    yield "variance_out is history", (H8, *good(), 4, 4, H8), "variance_out must not be"
    yield "misaligned history", (C.c_void_p(4096 * 6 + 8), *good(), 4, 4, W), "16-byte aligned"


ATROUS_CASES = [(e, c) for e in ("cpu", "device", "host") for c in _atrous_cases() if not (e == "host" and "temp" in c[0])]
VARIANCE_CASES = [(e, c) for e in ("cpu", "device", "host") for c in _variance_cases() if e == "device" or "misaligned" not in c[0]]


@pytest.mark.parametrize("entry,case", ATROUS_CASES, ids=[f"{e}-{c[0]}" for e, c in ATROUS_CASES])
def test_atrous_refusals_return_a_status_and_name_the_argument(entry, case):
    name, args, word = case
    status, text = _call_atrous(entry, *args)
    who = {"cpu": "rt_svgf_atrous_cpu", "device": "rt_svgf_atrous", "host": "rt_svgf_atrous_host"}[entry]
    assert status == -1 and text.startswith(who + ": ") and word in text, (status, text)


@pytest.mark.parametrize("entry,case", VARIANCE_CASES, ids=[f"{e}-{c[0]}" for e, c in VARIANCE_CASES])
def test_variance_refusals_return_a_status_and_name_the_argument(entry, case):
    name, args, word = case
    status, text = _call_variance(entry, *args)
    who = {"cpu": "rt_svgf_variance_cpu", "device": "rt_svgf_variance", "host": "rt_svgf_variance_host"}[entry]
    assert status == -1 and text.startswith(who + ": ") and word in text, (status, text)


def test_an_empty_image_is_ok_and_the_wrappers_raise():
    g = _capi.DenoiseGuides()
    for entry in ("cpu", "device", "host"):
        assert _call_atrous(entry, None, 3, None, g, _capi.SvgfAtrousParams(1.0, 1.0, 1.0, 0, 3, 0), 0, 7, None, None, None)[0] == 0
        assert _call_variance(entry, None, g, _capi.SvgfVarianceParams(1.0, 1.0, 4, 0), 7, 0, None)[0] == 0
    color, variance, history, normal, _, _, _ = case_data(23, 37)
    with pytest.raises(rt.RtError, match="first_level"):
        svgf.atrous_numpy(color, variance, 23, 37, levels=7)
    with pytest.raises(rt.RtError, match="sigma_luminance"):
        svgf.atrous_numpy(color, variance, 23, 37, sigma_luminance=0.0)
    with pytest.raises(rt.RtError, match="albedo"):
        svgf.atrous_numpy(color, variance, 23, 37, demodulate=True)
    with pytest.raises(rt.RtError, match="min_length"):
        svgf.variance_numpy(history, 23, 37, min_length=0)
    with pytest.raises(ValueError, match="normal"):
        svgf.atrous_numpy(color, variance, 23, 37, normal=normal[:, :2])
    with pytest.raises(ValueError, match="variance"):
        svgf.atrous_numpy(color, variance[:-1], 23, 37)
    with pytest.raises(ValueError, match="color"):
        svgf.atrous_numpy(color.astype(np.float64), variance, 23, 37)
    with pytest.raises(ValueError, match="history"):
        svgf.variance_numpy(history[:-1], 23, 37)
    assert [svgf.temp_bytes(23, 37, k) for k in (1, 2, 3, 6)] == [0, 23 * 37 * 16, 23 * 37 * 20, 23 * 37 * 20]
