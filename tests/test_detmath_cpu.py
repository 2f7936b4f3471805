"""rt_detmath.h on the host: accuracy against binary64 libm rounded once, agreement with glibc's f32 libm,
and the C99 special cases; at the switch points of its algorithms (tests/_detmath_support.py) accuracy against a 200-bit reference
(mpmath) rounded once to f32, subnormal results included; the binary64 intermediates against the same reference; and the f64 divide
and square root against exact integer arithmetic.  (Device == host bit-for-bit is tests/test_gpu_detmath.py.)

This file needs mpmath (it comes with sympy, which torch depends on): it is the high-precision judge, and there is no fallback."""
import ctypes as C
import math

import mpmath
import numpy as np
import pytest

from homework_18_graphics_raytracer_amd import _capi
import _detmath_support as S
import _oracle

OPS = S.OPS


def ev(op, x, y=None):
    x = np.ascontiguousarray(x, dtype=np.float32)
    y = np.zeros_like(x) if y is None else np.ascontiguousarray(y, dtype=np.float32)
    out = np.empty_like(x)
    _capi.check(_capi.amd_lib().rt_math_eval_host(OPS[op], x.ctypes.data, y.ctypes.data, out.ctypes.data, x.size))
    return out


def ulp_diff(a, b):
    ia = a.view(np.int32).astype(np.int64)
    ib = b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)


RNG = np.random.default_rng(42)
N = 400_000


def _check(got, want64, min_exact=0.99999):
    want = want64.astype(np.float32)
    ok = np.isfinite(want) & (np.abs(want) > 1e-37)
    d = ulp_diff(got[ok], want[ok])
    assert d.max() <= 1, f"max ulp diff {d.max()}"
    assert np.mean(d == 0) >= min_exact, f"exact fraction {np.mean(d == 0)}"


@pytest.mark.parametrize("name,fn", [("sin", np.sin), ("cos", np.cos), ("tan", np.tan)])
def test_trig_is_correctly_rounded_almost_always(name, fn):
    x = np.concatenate([RNG.uniform(-8, 8, N), RNG.uniform(-70, 70, N), RNG.uniform(-1e5, 1e5, N),
                        RNG.uniform(-1e-3, 1e-3, N)]).astype(np.float32)
    _check(ev(name, x), fn(x.astype(np.float64)))


def test_trig_huge_arguments_use_payne_hanek():
    x = (RNG.uniform(1, 2, N) * 2.0 ** RNG.integers(20, 127, N)).astype(np.float32)
    x *= RNG.choice([-1, 1], N).astype(np.float32)
    _check(ev("sin", x), np.sin(x.astype(np.float64)), min_exact=0.9999)
    _check(ev("cos", x), np.cos(x.astype(np.float64)), min_exact=0.9999)


def test_fused_sincos_equals_sin_and_cos_bit_for_bit():
    """The kernels call sincosf (one argument reduction for both); the oracle calls sinf and cosf."""
    bits = RNG.integers(0, 2**32, size=N, dtype=np.uint64).astype(np.uint32).view(np.float32)
    x = np.concatenate([bits, RNG.uniform(-8, 8, N).astype(np.float32), RNG.uniform(-1e5, 1e5, N).astype(np.float32),
                        (RNG.uniform(1, 2, N) * 2.0 ** RNG.integers(20, 127, N)).astype(np.float32),
                        np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 0.78539816, 1.5707964, 3.1415927, -3.1415927], dtype=np.float32)])
    for fused, plain in (("sincos_sin", "sin"), ("sincos_cos", "cos")):
        a, b = ev(fused, x), ev(plain, x)
        assert np.array_equal(np.isnan(a), np.isnan(b))
        ok = ~np.isnan(a)
        assert np.array_equal(a[ok].view(np.uint32), b[ok].view(np.uint32))


def test_acos_atan2():
    x = np.concatenate([RNG.uniform(-1, 1, N), 1 - RNG.uniform(0, 1e-4, N), -1 + RNG.uniform(0, 1e-4, N)]).astype(np.float32)
    _check(ev("acos", x), np.arccos(x.astype(np.float64)))
    y = RNG.normal(0, 1, N).astype(np.float32)
    z = RNG.normal(0, 1, N).astype(np.float32)
    _check(ev("atan2", y, z), np.arctan2(y.astype(np.float64), z.astype(np.float64)))


def test_pow_including_the_specular_regime():
    # smoothness 1e-5 gives exponents ~99988 on bases just under 1 (materials.rs:60-63)
    b = np.concatenate([RNG.uniform(0, 1, N), 1 - RNG.uniform(0, 2e-4, N), RNG.uniform(0, 50, N)]).astype(np.float32)
    e = np.concatenate([RNG.choice([1.0, 0.99999988, 4.9999971, 99.0, 1000.0, 1.0000001, 0.41666666], N),
                        RNG.choice([99988.08, 999.88, 99.0], N), RNG.uniform(-5, 5, N)]).astype(np.float32)
    with np.errstate(all="ignore"):
        _check(ev("pow", b, e), np.power(b.astype(np.float64), e.astype(np.float64)), min_exact=0.9999)


def test_agrees_with_glibc_libm_to_one_ulp():
    x = RNG.uniform(-70, 70, N).astype(np.float32)
    for name in ("sin", "cos"):
        assert ulp_diff(ev(name, x), _oracle.math(name, x, kind="libm")).max() <= 1
    u = RNG.uniform(-1, 1, N).astype(np.float32)
    assert ulp_diff(ev("acos", u), _oracle.math("acos", u, kind="libm")).max() <= 1
    b = RNG.uniform(0, 1, N).astype(np.float32)
    e = RNG.choice([1.0, 4.9999971, 99.0, 1000.0, 99988.08], N).astype(np.float32)
    g, l = ev("pow", b, e), _oracle.math("pow", b, e, kind="libm")
    big = np.abs(l) > 1e-30
    assert ulp_diff(g[big], l[big]).max() <= 1


def test_oracle_detmath_build_calls_the_same_functions():
    x = RNG.uniform(-70, 70, 10000).astype(np.float32)
    assert np.array_equal(ev("sin", x).view(np.uint32), _oracle.math("sin", x).view(np.uint32))


def test_special_cases_follow_c99():
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    f = lambda *v: np.array(v, dtype=np.float32)
    assert np.isnan(ev("sin", f(inf, -inf, nan))).all() and np.isnan(ev("cos", f(inf, nan))).all()
    s = ev("sin", f(0.0, -0.0))
    assert s[0] == 0 and not np.signbit(s[0]) and np.signbit(s[1])
    assert ev("cos", f(0.0))[0] == 1.0
    a = ev("acos", f(1.0, -1.0, 0.0, 1.0000001, -1.5, nan))
    assert a[0] == 0 and a[1] == np.float32(np.pi) and a[2] == np.float32(np.pi / 2) and np.isnan(a[3:]).all()
    t = ev("atan2", f(0.0, -0.0, 0.0, -0.0, 1.0, -1.0, inf, inf, 1.0, 1.0), f(1.0, 1.0, -1.0, -1.0, 0.0, 0.0, inf, -inf, inf, -inf))
    pi = np.float32(np.pi)
    want = f(0.0, -0.0, pi, -pi, pi / 2, -pi / 2, pi / 4, 3 * np.pi / 4, 0.0, pi)
    assert np.array_equal(t, want) and np.signbit(t[1])
    p = ev("pow", f(nan, 1.0, 0.0, 0.0, -0.0, -0.0, -8.0, -8.0, -1.0, 0.5, 2.0, inf, 0.0, 2.0, 2.0),
           f(0.0, nan, 2.5, -1.0, 3.0, -3.0, 3.0, 0.5, inf, inf, inf, -1.0, 0.0, 200.0, -200.0))
    assert p[0] == 1 and p[1] == 1 and p[2] == 0 and p[3] == inf and p[4] == 0 and np.signbit(p[4]) and p[5] == -inf
    assert p[6] == -512 and np.isnan(p[7]) and p[8] == 1 and p[9] == 0 and p[10] == inf and p[11] == 0 and p[12] == 1
    assert p[13] == inf and p[14] == 0


def test_round_half_away_from_zero_without_double_rounding():
    x = np.array([0.5, -0.5, 1.5, 2.5, 0.49999997, -0.49999997, 8388607.5, 1e10, -0.2, np.nan], dtype=np.float32)
    r = ev("round", x)
    assert r[:9].tolist() == [1, -1, 2, 3, 0, -0.0, 8388608, 1e10, -0.0] and np.isnan(r[9])
    y = RNG.uniform(-300, 300, N).astype(np.float32)
    assert np.array_equal(ev("round", y), np.where(y >= 0, np.floor(y.astype(np.float64) + 0.5), -np.floor(-y.astype(np.float64) + 0.5)).astype(np.float32))


# ---- the switch points of the algorithms, against a 200-bit reference rounded once ------------------------------------------
#
# The judge is mpmath at 200 bits, not numpy's f64 libm: next to a multiple of pi/2, and for powers with exponents near 10^5, a
# binary64 result is itself within a few of its ulps of an f32 rounding boundary.  The bound is the header's own claim ("correctly
# rounded except within about 2^-24 ulp of a boundary"): at most 1 ulp, results in the subnormal range, at overflow and at underflow
# included.  The share of exactly rounded results is printed (and recorded in DESIGN.md "Numerics"), not asserted.

MP = mpmath.mp.clone()
MP.prec = 200


def _round_f32(v):
    """An mpf rounded once (nearest, ties to even) to binary32, gradual underflow and overflow included, as a Python float."""
    sign, man, exp, bc = v._mpf_
    if man == 0:
        return float(v)  # zero, infinities, NaN
    e = exp + bc - 1                          # floor(log2 |v|)
    if e > 127 or e < -151:                   # beyond 2^128; below half the smallest subnormal
        r = math.inf if e > 127 else 0.0
        return -r if sign else r
    q = max(e, -126) - 23                     # the exponent of the f32 quantum at |v|
    shift = q - exp
    if shift <= 0:
        n = man << -shift
    else:
        n, rem = man >> shift, man & ((1 << shift) - 1)
        half = 1 << (shift - 1)
        if rem > half or (rem == half and n & 1):
            n += 1
    r = math.ldexp(n, q) if n < (1 << 24) or q < 104 else math.inf  # n == 2^24 at q == 104 is 2^128: FLT_MAX's tie goes up
    return -r if sign else r


def _report(name, got, want):
    """got against the once-rounded reference: at most 1 ulp everywhere; prints the share that is exact."""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{name}: NaN where the reference has none, or the reverse"
    ok = ~np.isnan(want)
    d = ulp_diff(got[ok], want[ok])
    print(f"{name}: {ok.sum()} results, exactly rounded {np.mean(d == 0):.6f}, max ulp {d.max()}")
    worst = np.argmax(d)
    assert d.max() <= 1, f"{name}: max ulp diff {d.max()} (got {got[ok][worst]!r}, reference {want[ok][worst]!r})"


_TRIG_REF = {}


def _trig_reference():
    """sin, cos and tan of every finite non-zero |x| of the trig set, computed once for the three tests that need them."""
    if not _TRIG_REF:
        x = S.trig_edges()
        ax = np.unique(np.abs(x[np.isfinite(x) & (x != 0)]))
        s, c, t = np.empty_like(ax), np.empty_like(ax), np.empty_like(ax)
        for i, v in enumerate(ax):
            cv, sv = MP.cos_sin(MP.mpf(float(v)))
            s[i], c[i], t[i] = _round_f32(sv), _round_f32(cv), _round_f32(sv / cv)
        _TRIG_REF.update(ax=ax, sin=s, cos=c, tan=t)
    return _TRIG_REF


@pytest.mark.parametrize("op", ["sin", "cos", "tan", "sincos_sin", "sincos_cos"])
def test_trig_edges_within_one_ulp(op):
    ref = _trig_reference()
    x = S.trig_edges()
    got = ev(op, x)
    ordinary = np.isfinite(x) & (x != 0)
    assert np.isnan(got[~np.isfinite(x)]).all()
    zero = x == 0
    want0 = np.ones_like(x[zero]) if op.endswith("cos") else x[zero]  # cos(+-0) = 1; sin and tan keep the signed zero
    assert np.array_equal(got[zero].view(np.uint32), want0.view(np.uint32))
    xo = x[ordinary]
    w = ref[op.split("_")[-1]][np.searchsorted(ref["ax"], np.abs(xo))]
    want = w if op.endswith("cos") else np.copysign(w, xo) * np.sign(w)  # sin and tan are odd
    _report(op, got[ordinary], want)


def test_acos_edges_within_one_ulp():
    x = S.acos_edges()
    got = ev("acos", x)
    inside = np.abs(x) <= 1  # false for NaN
    assert np.isnan(got[~inside]).all()
    want = np.array([_round_f32(MP.acos(MP.mpf(float(v)))) for v in x[inside]], dtype=np.float32)
    _report("acos", got[inside], want)
    assert got[x == 1].view(np.uint32).tolist() == [0] * np.count_nonzero(x == 1)  # +0, not -0


def test_atan2_edges_within_one_ulp():
    y, x = S.atan2_edges()
    got = ev("atan2", y, x)
    ordinary = np.isfinite(y) & np.isfinite(x) & (y != 0) & (x != 0)
    # zeros, infinities and NaN: C99 F.9.1.4, whose results are 0, pi/4, pi/2, 3pi/4 and pi with a sign — Python's atan2 follows it
    want = np.array([math.atan2(float(a), float(b)) for a, b in zip(y[~ordinary], x[~ordinary])]).astype(np.float32)
    assert np.array_equal(np.isnan(got[~ordinary]), np.isnan(want))
    keep = ~np.isnan(want)
    assert np.array_equal(got[~ordinary][keep].view(np.uint32), want[keep].view(np.uint32))
    # the rest by symmetry from |y|, x
    yo, xo = y[ordinary], x[ordinary]
    pairs, inv = np.unique(np.stack([np.abs(yo), xo]), axis=1, return_inverse=True)
    ref = np.array([_round_f32(MP.atan2(MP.mpf(float(a)), MP.mpf(float(b)))) for a, b in pairs.T], dtype=np.float32)
    _report("atan2", got[ordinary], np.copysign(ref[inv.ravel()], yo))


def _pow_reference(x, y):
    out = np.empty(x.size, dtype=np.float32)
    for i, (a, b) in enumerate(zip(x.astype(np.float64), y.astype(np.float64))):
        if not (math.isfinite(a) and math.isfinite(b)) or a == 0 or b == 0 or abs(a) == 1:
            # C99 F.9.4.4: every result here is 0, 1, an infinity or a NaN, exactly, and libm's binary64 pow follows the table
            with np.errstate(all="ignore"):
                out[i] = np.power(a, b)
        elif a < 0 and not b.is_integer():
            out[i] = np.nan
        else:
            v = _round_f32(MP.power(MP.mpf(abs(a)), MP.mpf(b)))
            out[i] = -v if a < 0 and int(b) % 2 else v
    return out


def test_pow_edges_within_one_ulp():
    """The overflow cut, ln FLT_MAX, the subnormal band down to half the smallest subnormal and the underflow cut among them:
    nothing below 1e-37 is left out."""
    x, y = S.pow_edges()
    got, want = ev("pow", x, y), _pow_reference(x, y)
    _report("pow", got, want)
    sub = ~np.isnan(want) & (np.abs(want) < np.float32(1.17549435e-38))
    _report("pow, zero and subnormal results", got[sub], want[sub])
    exact = ~np.isfinite(want) | (want == 0) | (np.abs(want) == 1)  # the special cases, overflow and underflow: signs included
    assert np.array_equal(got[exact & ~np.isnan(want)].view(np.uint32) >> 31, want[exact & ~np.isnan(want)].view(np.uint32) >> 31)


def test_round_and_classification_edges_are_exact():
    x = S.round_edges()
    xd = x.astype(np.float64)
    want = (np.sign(xd) * np.floor(np.abs(xd) + 0.5)).astype(np.float32)  # |x| + 0.5 is exact in binary64
    got = ev("round", x)
    ok = ~np.isnan(x)
    assert np.isnan(got[~ok]).all() and np.array_equal(got[ok], want[ok])
    assert np.array_equal(np.signbit(got[ok]), np.signbit(x[ok]))  # -0.2 -> -0.0
    x = S.classify_edges()
    with np.errstate(invalid="ignore"):  # a signalling NaN is among them
        xd = x.astype(np.float64)
        as_i32 = np.where(np.isnan(xd), 0, np.clip(np.trunc(xd), -2147483648.0, 2147483647.0)).astype(np.int64).astype(np.int32)
    assert np.array_equal(ev("f32_as_i32", x).view(np.int32), as_i32)
    e = (x.view(np.uint32) >> 23) & 0xFF
    assert np.array_equal(ev("is_normal", x), ((e != 0) & (e != 255)).astype(np.float32))
    finite = np.isfinite(xd)
    whole = finite & (np.abs(xd) >= 1) & (np.floor(xd) == xd)
    with np.errstate(invalid="ignore"):
        odd = whole & (np.abs(xd) < 2.0 ** 24) & (np.mod(np.abs(xd), 2) == 1)
    cls = np.where(np.abs(xd) >= 2.0 ** 24, 2, np.where(odd, 1, np.where(whole, 2, 0)))  # what f32_int_class says of inf and NaN too
    assert np.array_equal(ev("int_class", x)[finite], cls[finite].astype(np.float32))


def test_f64_divide_and_sqrt_are_correctly_rounded_on_the_host():
    a, b = S.exact_operands()
    q = S.eval64("host", "div", a, b)
    assert np.array_equal(S.bits64(q), S.bits64(np.array([S.exact_div(x, y) for x, y in zip(a, b)])))
    for v in (a, b):
        r = S.eval64("host", "sqrt", v)
        assert np.array_equal(S.bits64(r), S.bits64(np.array([S.exact_sqrt(x) for x in v])))


def test_f64_primitives_on_the_host():
    """What the device is compared with: narrowing, rounding to i32 and the i64 conversion against their definitions."""
    a = S.narrow_operands()
    with np.errstate(over="ignore", invalid="ignore"):
        assert S.same_bits_or_both_nan(S.eval64("host", "narrow", a), a.astype(np.float32).astype(np.float64)).all()
    a = S.round_i32_operands()
    assert np.array_equal(S.eval64("host", "round_i32", a), np.floor(a + 0.5))  # the header's definition: floor(t + 0.5) in binary64
    a = S.from_i64_operands()
    want = np.array([float(int(v)) for v in S.bits64(a).view(np.int64)])  # Python rounds an int to nearest even exactly
    assert np.array_equal(S.eval64("host", "from_i64", a), want)


# The header claims a relative error below 2^-48 for its binary64 intermediates.  Measured on every 8th operand of the sets and on
# every operand at their switch points (the k steps of exp_mid, log_pos's sqrt(2) switch and 1, atan_unit's sixteenths) (printed
# below, recorded in DESIGN.md "Numerics"): INTERMEDIATE_BOUND is asserted because the measurements stay under it with room.
INTERMEDIATE_BOUND = 2.0 ** -48


def _relative_error(got, ref):
    worst = MP.mpf(0)
    for g, r in zip(got, ref):
        if r != 0:
            worst = max(worst, abs((MP.mpf(float(g)) - r) / r))
    return float(worst)


@pytest.mark.parametrize("op", ["exp_mid", "log_pos", "atan2_upper"])
def test_binary64_intermediates_meet_the_headers_claim(op):
    if op == "atan2_upper":
        y, x = S.atan2_upper_operands()
        with np.errstate(divide="ignore"):
            fits = (y > 0) & (x != 0) & np.isfinite(y) & np.isfinite(x) & (np.abs(np.log2(y) - np.log2(np.abs(x))) <= 300)
        # quotients no smaller than widened f32 operands give: beyond them y/|x| is a subnormal double
        sy, sx = S.atan2_upper_switch_points()
        y, x = np.concatenate([y[fits][::8], sy]), np.concatenate([x[fits][::8], sx])
        got = S.eval64("host", op, y, x)
        ref = [MP.atan2(MP.mpf(float(a)), MP.mpf(float(b))) for a, b in zip(y, x)]
    else:
        a = np.concatenate([S.exp_mid_operands()[::8], S.exp_mid_switch_points()] if op == "exp_mid" else
                           [S.log_pos_operands()[::8], S.log_pos_switch_points()])
        got = S.eval64("host", op, a)
        fn = MP.exp if op == "exp_mid" else MP.log
        ref = [fn(MP.mpf(float(v))) for v in a]
    err = _relative_error(got, ref)
    print(f"{op}: {len(ref)} operands, largest relative error 2^{math.log2(err):.2f}")
    assert err < INTERMEDIATE_BOUND
