"""Device rt_detmath == host rt_detmath, bit for bit, and the IEEE primitives that rests on, on gfx950: f32/f64 divide and square root
(against the host and against exact integer arithmetic), the f64 -> f32 narrowing into subnormals, and the i64 -> f64 and f64 -> i32
conversions.  The operand sets are tests/_detmath_support.py's; tests/test_detmath_cpu.py checks the host against a high-precision
reference on the same sets."""
import numpy as np
import pytest

import _detmath_support as S

pytestmark = pytest.mark.gpu

OPS = S.OPS
NEW_F32_OPS = ["f32_as_i32", "is_normal", "int_class"]


def _both(op, x, y):
    return S.eval32("host", op, x, y).view(np.uint32), S.eval32("device", op, x, y).view(np.uint32)


def _inputs(rng, n):
    """A mix: uniform bit patterns (all exponents, NaN, inf, denormals), values near 1, and ordinary ranges."""
    bits = rng.integers(0, 2**32, size=n, dtype=np.uint64).astype(np.uint32).view(np.float32)
    near1 = (1.0 + rng.normal(0, 1e-3, n)).astype(np.float32)
    mid = rng.uniform(-100, 100, n).astype(np.float32)
    unit = rng.uniform(-1, 1, n).astype(np.float32)
    special = np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, 0.5, 2.0, 1e-45, -1e-45, 3.4e38, 1e-38], dtype=np.float32)
    return np.concatenate([bits, near1, mid, unit, np.resize(special, n)])


def _edges(op):
    """The boundary set of an f32 op as (x, y), or None."""
    if op in ("sin", "cos", "tan", "sincos_sin", "sincos_cos"):
        x = S.trig_edges()
    elif op == "acos":
        x = S.acos_edges()
    elif op == "atan2":
        return S.atan2_edges()
    elif op == "pow":
        return S.pow_edges()
    elif op == "round":
        x = S.round_edges()
    elif op in NEW_F32_OPS:
        x = S.classify_edges()
    else:
        return None
    return x, np.zeros_like(x)


def _exact_nan(op, x, y):
    """Where the exact result of an f64_* op is a NaN, the only place its two platforms may differ (in the payload)."""
    with np.errstate(invalid="ignore"):
        xd, yd = x.astype(np.float64), y.astype(np.float64)
        prod = xd * yd  # exact: 24 x 24 bits
    if op.startswith("f64_div"):
        return np.isnan(xd) | np.isnan(yd) | ((xd == 0) & (yd == 0)) | (np.isinf(xd) & np.isinf(yd))
    return np.isnan(prod) | (prod < 0)  # -0.0 is not < 0: sqrt(-0.0) is -0.0, bit for bit


@pytest.mark.parametrize("op", list(OPS))
def test_device_matches_host_bitwise(op):
    rng = np.random.default_rng(1234 + OPS[op])
    n = 1 << 18
    x = _inputs(rng, n)
    y = _inputs(rng, n)
    rng.shuffle(y)
    if op == "pow":
        # also the regime the renderer uses: base in [0,1], huge exponents (materials.rs:63, smoothness 1e-5)
        xb = rng.uniform(0, 1, n).astype(np.float32)
        yb = rng.choice(np.array([1.0, 4.9999995, 99.0, 1000.0, 99988.0, 1.0000001, 0.41666666], dtype=np.float32), n)
        x = np.concatenate([x, xb, (1.0 - rng.uniform(0, 1e-3, n)).astype(np.float32)])
        y = np.concatenate([y, yb, yb])
    edges = _edges(op)
    if edges is not None:
        x = np.concatenate([x, edges[0]])
        y = np.concatenate([y, edges[1]])
    h, d = _both(op, x, y)
    if op.startswith("f64_"):
        # the two halves of a binary64 are not NaN-classifiable as f32: a mismatch is excused only where the exact result is a NaN,
        # and there both sides must show one (an all-ones exponent in the hi half)
        excused = _exact_nan(op, x, y)
        bad = (h != d) & ~excused
        assert not bad.any(), f"{op}: {bad.sum()} finite mismatches, e.g. x={x[bad][:3]!r} y={y[bad][:3]!r} host={h[bad][:3]} dev={d[bad][:3]}"
        hi = op[:-2] + "hi"
        hh, dh = (h, d) if op == hi else _both(hi, x[excused], y[excused])
        if op == hi:
            hh, dh = hh[excused], dh[excused]
        assert ((hh & 0x7FF00000) == 0x7FF00000).all() and ((dh & 0x7FF00000) == 0x7FF00000).all(), f"{op}: a NaN result is not one"
        return
    if op in NEW_F32_OPS:
        # an integer, 0/1 or a class, never a computed NaN: f32_as_i32's negative and saturated results only read as one, so every bit counts
        bad = h != d
        assert not bad.any(), f"{op}: {bad.sum()} mismatches, e.g. x={x[bad][:3]!r} host={h[bad][:3]} dev={d[bad][:3]}"
        return
    # NaN payloads may differ between platforms; compare NaN-ness there
    hn = np.isnan(h.view(np.float32))
    dn = np.isnan(d.view(np.float32))
    assert np.array_equal(hn, dn)
    mism = (h != d) & ~hn
    assert not mism.any(), f"{op}: {mism.sum()} mismatches, e.g. x={x[mism][:3]!r} y={y[mism][:3]!r} host={h[mism][:3]} dev={d[mism][:3]}"


OPERANDS64 = {"div": S.div_operands, "sqrt": S.sqrt_operands, "narrow": S.narrow_operands, "round_i32": S.round_i32_operands,
              "from_i64": S.from_i64_operands, "exp_mid": S.exp_mid_operands, "log_pos": S.log_pos_operands,
              "atan2_upper": S.atan2_upper_operands}


@pytest.mark.parametrize("op", list(S.OPS64))
def test_device_matches_host_bitwise_64(op):
    """The binary64 primitives and intermediates, all 64 bits, no tolerance; a NaN only has to be a NaN on both sides."""
    ops = OPERANDS64[op]()
    a, b = ops if isinstance(ops, tuple) else (ops, None)
    h, d = S.eval64("host", op, a, b), S.eval64("device", op, a, b)
    bad = ~S.same_bits_or_both_nan(h, d)
    bb = a[bad][:3] if b is None else b[bad][:3]
    assert not bad.any(), (f"{op}: {bad.sum()} of {a.size} differ, e.g. a={S.bits64(a[bad][:3])} b={S.bits64(bb)} "
                           f"host={S.bits64(h[bad][:3])} dev={S.bits64(d[bad][:3])}")


def test_device_divide_and_sqrt_are_correctly_rounded():
    """Device == host only moves trust to x86: the two software expansions against exact integer arithmetic."""
    a, b = S.exact_operands()
    q = S.eval64("device", "div", a, b)
    want = np.array([S.exact_div(x, y) for x, y in zip(a, b)])
    assert np.array_equal(S.bits64(q), S.bits64(want)), f"divide: {np.count_nonzero(q != want)} of {a.size} not correctly rounded"
    for v in (a, b):
        r = S.eval64("device", "sqrt", v)
        want = np.array([S.exact_sqrt(x) for x in v])
        assert np.array_equal(S.bits64(r), S.bits64(want)), f"sqrt: {np.count_nonzero(r != want)} of {v.size} not correctly rounded"
