"""Operand sets for the rt_detmath tests, shared by tests/test_gpu_detmath.py (device == host, bit for bit) and
tests/test_detmath_cpu.py (host against a high-precision reference): the switch points of csrc/rt_detmath.h's algorithms with their
neighbours, the operands of the binary64 primitives under them, and exact integer references for the f64 divide and square root.

Every set is built from fixed patterns and a seeded generator, so both files (and both machines) see the same operands."""
import math
from fractions import Fraction
from functools import lru_cache

import numpy as np

from homework_18_graphics_raytracer_amd import _capi

# rt_math_op / rt_math64_op of include/rt_amd.h
OPS = {"sin": 0, "cos": 1, "tan": 2, "acos": 3, "atan2": 4, "pow": 5, "f32_div": 6, "f32_sqrt": 7,
       "f64_sqrt_hi": 8, "f64_sqrt_lo": 9, "f64_div_hi": 10, "f64_div_lo": 11, "round": 12, "sincos_sin": 13, "sincos_cos": 14,
       "f32_as_i32": 15, "is_normal": 16, "int_class": 17}
OPS64 = {"div": 0, "sqrt": 1, "narrow": 2, "round_i32": 3, "from_i64": 4, "exp_mid": 5, "log_pos": 6, "atan2_upper": 7}

NEIGHBOURS = 64  # patterns taken each side of a switch point


def eval32(where, op, x, y=None):
    """rt_math_eval_<where>(op) on f32 arrays; where is "host" or "device"."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    y = np.zeros_like(x) if y is None else np.ascontiguousarray(y, dtype=np.float32)
    out = np.empty_like(x)
    fn = getattr(_capi.amd_lib(), f"rt_math_eval_{where}")
    _capi.check(fn(OPS[op], x.ctypes.data, y.ctypes.data, out.ctypes.data, x.size))
    return out


def eval64(where, op, a, b=None):
    """rt_math_eval64_<where>(op) on f64 arrays (bit patterns pass through untouched)."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.zeros_like(a) if b is None else np.ascontiguousarray(b, dtype=np.float64)
    out = np.empty_like(a)
    fn = getattr(_capi.amd_lib(), f"rt_math_eval64_{where}")
    _capi.check(fn(OPS64[op], a.ctypes.data, b.ctypes.data, out.ctypes.data, a.size))
    return out


def f32(bits):
    return np.asarray(bits, dtype=np.uint32).view(np.float32)


def bits32(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def f64(bits):
    return np.asarray(bits, dtype=np.uint64).view(np.float64)


def bits64(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def neighbours(patterns, k=NEIGHBOURS, both_signs=True):
    """The f32 values whose magnitudes' patterns lie within k of each given pattern's, in both signs or in the pattern's own."""
    p = np.asarray(patterns, dtype=np.int64).reshape(-1, 1)
    u = np.clip((p & 0x7FFFFFFF) + np.arange(-k, k + 1, dtype=np.int64), 0, 0x7FFFFFFF)
    if both_signs:
        u = np.concatenate([u.ravel(), u.ravel() | 0x80000000])
    else:
        u = (u | (p & 0x80000000)).ravel()  # the sign each pattern came with
    return u.astype(np.uint32).view(np.float32)


def step64(a, steps):
    """Doubles `steps` ulps from each a (finite, away from zero), every pairing: a[:, None] moved by steps[None, :]."""
    b = bits64(a).astype(np.int64).reshape(-1, 1)
    s = np.asarray(steps, dtype=np.int64).reshape(1, -1)
    return (b + s).ravel().view(np.float64)  # the pattern order of one sign is the value order of |a|


def full_mantissa(rng, n, e_lo, e_hi):
    """Doubles with all 52 fraction bits random, exponents uniform in [e_lo, e_hi] (unbiased, normal range), positive."""
    frac = rng.integers(0, 1 << 52, size=n, dtype=np.uint64)
    e = rng.integers(e_lo + 1023, e_hi + 1023 + 1, size=n, dtype=np.uint64)
    return ((e << np.uint64(52)) | frac).view(np.float64)


def same_bits_or_both_nan(h, d):
    """Mask of elements where two results are the same bit pattern, or both a NaN (payloads may differ between platforms)."""
    return (h.view(h.dtype.str.replace("f", "u")) == d.view(d.dtype.str.replace("f", "u"))) | (np.isnan(h) & np.isnan(d))


# ---- the f32 boundary sets ------------------------------------------------------------------------------------------------

PI = Fraction(int("3141592653589793238462643383279502884197169399375105820974944592307816406286208998628034825342117067"), 10 ** 99)


def _f32_below(q):
    """The largest positive f32 <= the positive rational q."""
    x = np.float32(float(q))
    while Fraction(float(x)) > q:
        x = np.nextafter(x, np.float32(0))
    while Fraction(float(np.nextafter(x, np.float32(np.inf)))) <= q:
        x = np.nextafter(x, np.float32(np.inf))
    return x


@lru_cache(maxsize=None)
def trig_edges():
    """sin / cos / tan / sincos: the reduction's two cuts and FLT_MAX, the f32 values next to multiples of pi/2 (where the reduction
    cancels hardest), and every exponent of the Payne-Hanek range with empty, full and random mantissas (every idx and shift of the
    2/pi table)."""
    rng = np.random.default_rng(20240)
    pats = [0x3F490FDA, 0x49800000, 0x7F7FFFFF]
    ks = list(range(1, 65)) + [1 << j for j in range(7, 21)]
    for k in ks:
        lo = _f32_below(k * PI / 2)
        pats += [int(bits32(lo)[0]), int(bits32(lo)[0]) + 1]  # the two f32 values nearest k*pi/2 are the ones around it
    e = np.arange(147, 255, dtype=np.uint32)
    pats += list(e << 23) + list((e << 23) | 0x7FFFFF)
    x = [neighbours(pats)]
    # the first odd multiples of pi/2 past the 2^20 cut: Payne-Hanek's smallest arguments at their hardest cancellation (and where a
    # Cody-Waite reduction carried beyond the cut would have to keep a 21-bit k times PIO2_1 exact)
    past = [int(bits32(_f32_below(k * PI / 2))[0]) for k in range((1 << 20) + 1, (1 << 20) + 2048, 2)]
    x.append(neighbours(past + [p + 1 for p in past], k=0))
    mant = rng.integers(0, 1 << 23, size=(e.size, 1000), dtype=np.uint32)
    sign = rng.integers(0, 2, size=mant.shape, dtype=np.uint32) << 31
    x.append(((e[:, None] << 23) | mant | sign).ravel().view(np.float32))
    x.append(f32([0, 0x80000000, 1, 0x80000001, 0x007FFFFF, 0x00800000, 0x7F800000, 0xFF800000, 0x7FC00000]))
    return np.concatenate(x)


@lru_cache(maxsize=None)
def acos_edges():
    """acos: +-1 with their neighbours (beyond them the domain error), +-0 and subnormals, the normal/subnormal edge."""
    rng = np.random.default_rng(20241)
    sub = rng.integers(1, 1 << 23, size=512, dtype=np.uint32)
    return np.concatenate([neighbours([0x3F800000, 0, 0x00800000, 0x3F000000]), f32(sub), f32(sub | np.uint32(0x80000000)),
                           f32([0x7FC00000, 0x7F800000, 0xFF800000])])


SPECIALS = f32([0, 0x80000000, 0x3F800000, 0xBF800000, 0x7F800000, 0xFF800000, 0x7FC00000, 1, 0x80000001, 0x00800000, 0x80800000,
                0x7F7FFFFF, 0xFF7FFFFF, 0x3F000000, 0xBF000000, 0x40000000, 0xC0000000])


def _cross(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return np.repeat(a, b.size), np.tile(b, a.size)


@lru_cache(maxsize=None)
def atan2_edges():
    """atan2(y, x): quotients at j/16 for odd j (atan_unit's t*8 at a half-integer) from either side of the y <= |x| branch, y == |x|,
    and the signed-zero / infinity / NaN table of C99 F.9.1.4 as a full cross of special values."""
    rng = np.random.default_rng(20242)
    ys, xs = [], []
    m = np.concatenate([[1, 3, 0x7FFFF], rng.integers(1, 1 << 19, size=5)]).astype(np.float64)
    scale = 2.0 ** np.array([0, -20, 17, -100, 90, -130, 3, -7])  # 2^-130: small is a subnormal f32 for small m, still exact
    for j in range(1, 16, 2):
        big = (16.0 * m * scale).astype(np.float32)   # exact: m < 2^19
        small = (j * m * scale).astype(np.float32)    # exact: j*m < 2^23, so small / big == j/16 exactly
        for a, b in ((small, big), (big, small)):     # (y, x): quotient y/x, then x/y
            an = neighbours(bits32(a), both_signs=True).reshape(2, a.size, -1)
            for sy in (0, 1):
                for sx in (1.0, -1.0):
                    ys.append(an[sy].ravel())
                    xs.append(np.repeat(b * np.float32(sx), an.shape[2]))
    r = f32(rng.integers(0x00000001, 0x7F800000, size=64, dtype=np.uint32))
    rn = neighbours(bits32(r)).reshape(2, r.size, -1)
    for sy in (0, 1):
        for sx in (1.0, -1.0):
            ys.append(rn[sy].ravel())
            xs.append(np.repeat(r * np.float32(sx), rn.shape[2]))
    sy_, sx_ = _cross(SPECIALS, SPECIALS)
    ys.append(sy_)
    xs.append(sx_)
    return np.concatenate(ys), np.concatenate(xs)


POW_CUTS = (100.0, 88.72, -87.34, -103.97, -110.0)  # z > 100 -> inf; ln FLT_MAX; ln of the smallest normal; ln 2^-150; z < -110 -> 0


@lru_cache(maxsize=None)
def pow_edges():
    """pow(x, y): y * ln x around the cuts of powf and the overflow / subnormal / underflow band between them, exp_mid's k steps
    (2^(k + 1/2)), bases around log_pos's sqrt(2) switch, exponents around 2^23 and 2^24 (odd, even, non-integer) under negative
    bases, and the C99 F.9.4.4 table as a full cross of special values."""
    rng = np.random.default_rng(20243)
    xs, ys = [], []
    bases = np.concatenate([[2.0, 0.5, 10.0, 0.1, 1.5, 3.0, 0.75, 1.0009766, 0.99902344, 1e-30, 1e30, 1.00001, 0.99999],
                            rng.uniform(0, 1, 8), rng.uniform(1, 50, 8)]).astype(np.float32)
    ln = np.log(bases.astype(np.float64))
    targets = np.concatenate([POW_CUTS, np.linspace(-110.5, -86.5, 97), np.linspace(88.0, 100.5, 26)])
    for t in targets:
        y0 = (t / ln).astype(np.float32)
        k = NEIGHBOURS if t in POW_CUTS else 2
        yn = neighbours(bits32(y0), k=k, both_signs=False).reshape(y0.size, -1)
        xs.append(np.repeat(bases, yn.shape[1]))
        ys.append(yn.ravel())
    # 2^(k + 1/2): z / ln 2 is a half-integer up to rounding, so neighbouring exponents fall on both sides of a k step
    half = np.arange(-151, 129, dtype=np.float64) + 0.5
    hn = neighbours(bits32(half.astype(np.float32)), k=4, both_signs=False)
    xs.append(np.full(hn.size, 2.0, dtype=np.float32))
    ys.append(hn)
    # bases next to sqrt(2) * 2^e: their f64 mantissas bracket log_pos's 0x1.6a09e667f3bcd (0x3fb504f3 is sqrt(2) rounded to f32)
    e = np.array([1, 64, 100, 126, 127, 128, 150, 200, 254], dtype=np.int64)
    bn = neighbours((e << 23) | 0x3504F3, both_signs=False)
    bsub = f32((0x3504F3 >> np.arange(1, 6)).astype(np.uint32))  # subnormal f32 bases are normal doubles with the same leading bits
    bn = np.concatenate([bn, bsub, f32(bits32(bsub) + np.uint32(1))])
    for yv in (0.5, 2.0, 3.3, -1.7, 0.41666666):
        xs.append(bn)
        ys.append(np.full(bn.size, yv, dtype=np.float32))
    # integer classification of the exponent under a negative base
    yn = np.concatenate([neighbours([0x4B000000, 0x4B800000, 0x4A800000, 0x3F800000, 0x40400000]), f32([0x7F7FFFFF, 0xFF7FFFFF])])
    for xv in (-1.0, -1.0000001, -0.99999994, -2.0, -0.5, -1.000001, -0.0, -np.inf, -1e-45, 1.0000001, 0.99999994):
        xs.append(np.full(yn.size, xv, dtype=np.float32))
        ys.append(yn)
    sx, sy = _cross(np.concatenate([SPECIALS, f32([0x41000000, 0xC1000000])]),
                    np.concatenate([SPECIALS, np.array([3.0, -3.0, 2.5, -2.5, 200.0, -200.0, 16777216.0, 16777218.0, 8388609.0], dtype=np.float32)]))
    xs.append(sx)
    ys.append(sy)
    return np.concatenate(xs), np.concatenate(ys)


@lru_cache(maxsize=None)
def round_edges():
    """f_round: ties k + 1/2 up to 2^23 (the small k, the powers of two, random k over the whole range and in its last binade), and
    2^23 itself (from where every f32 is an integer) with its neighbours."""
    rng = np.random.default_rng(20244)
    k = np.concatenate([np.arange(0, 1024), (1 << np.arange(10, 23)) - 1, 1 << np.arange(10, 23), [(1 << 23) - 1, (1 << 23) - 2],
                        rng.integers(1 << 10, 1 << 23, size=4096), (1 << 22) + rng.integers(0, 1 << 22, size=2048)])
    ties = (k.astype(np.float64) + 0.5).astype(np.float32)  # exact below 2^23
    return np.concatenate([neighbours(bits32(ties), k=2), neighbours([0x4B000000, 0x3F000000, 0x3F800000, 0, 0x4F000000]),
                           f32([0x7F800000, 0xFF800000, 0x7FC00000])])


@lru_cache(maxsize=None)
def classify_edges():
    """f32_as_i32 / is_normal / f32_int_class: +-2^31 (the saturation), NaN and infinities, the normal/subnormal edge, the largest
    finite, 2^23 and 2^24 (the last odd integer, the first exponent that is always even), and small integers and halves."""
    small = np.arange(-64, 65, dtype=np.float32) * np.float32(0.5)
    return np.concatenate([neighbours([0x4F000000, 0x00800000, 0, 0x7F800000, 0x4B000000, 0x4B800000, 0x3F800000, 0x4E800000]), small,
                           f32([0x7FC00000, 0xFFC00000, 0x7F800001, 0x7F800000, 0xFF800000])])


# ---- operands of the binary64 ops --------------------------------------------------------------------------------------------

N64 = 1 << 16  # per kind of operand; four kinds or so per op


def _patterns64(rng, n):
    return rng.integers(0, 1 << 64, size=n, dtype=np.uint64).view(np.float64)


def _signed(rng, a):
    return a * rng.choice(np.array([-1.0, 1.0]), a.size)


@lru_cache(maxsize=None)
def div_operands():
    """a / b: random patterns; full mantissas over the whole exponent range; quotients in the subnormal range and around overflow."""
    rng = np.random.default_rng(20250)
    a, b = [_patterns64(rng, N64)], [_patterns64(rng, N64)]
    a.append(_signed(rng, full_mantissa(rng, N64, -1022, 1023)))
    b.append(_signed(rng, full_mantissa(rng, N64, -1022, 1023)))
    a.append(_signed(rng, full_mantissa(rng, N64, 0, 0)))          # quotient in [1/2, 2): the plain last-bit rounding
    b.append(_signed(rng, full_mantissa(rng, N64, 0, 0)))
    ea = rng.integers(-1022, -40, size=N64)
    lo = full_mantissa(rng, N64, 0, 0) * 2.0 ** ea                 # quotient exponent -1080..-1018: subnormal, and rounded there
    a.append(_signed(rng, lo))
    b.append(full_mantissa(rng, N64, 0, 0) * 2.0 ** (ea + rng.integers(1018, 1081, size=N64)).clip(-1022, 1023))
    eb = rng.integers(-1022, 0, size=N64 // 2)
    b.append(full_mantissa(rng, N64 // 2, 0, 0) * 2.0 ** eb)       # quotient exponent 1020..1026: around overflow
    a.append(_signed(rng, full_mantissa(rng, N64 // 2, 0, 0) * 2.0 ** (eb + rng.integers(1020, 1027, size=N64 // 2)).clip(-1022, 1023)))
    sa, sb = _cross_64([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, 5e-324, -5e-324, 2.2250738585072014e-308, 1.7976931348623157e308, 3.0])
    a.append(sa)
    b.append(sb)
    return np.concatenate(a), np.concatenate(b)


def _cross_64(v):
    v = np.asarray(v, dtype=np.float64)
    return np.repeat(v, v.size), np.tile(v, v.size)


@lru_cache(maxsize=None)
def sqrt_operands():
    """d_sqrt(a): random patterns (half of them negative: NaN), full mantissas over the whole range, subnormal operands, squares of
    53-bit values a step either side (roots next to a rounding boundary), and the signed zeros and infinities."""
    rng = np.random.default_rng(20251)
    a = [_patterns64(rng, N64), full_mantissa(rng, N64, -1022, 1023), full_mantissa(rng, N64, 0, 1)]
    a.append(rng.integers(1, 1 << 52, size=N64 // 2, dtype=np.uint64).view(np.float64))  # subnormal operands
    r = full_mantissa(rng, N64 // 4, -400, 400)
    a.append(step64(r * r, [-2, -1, 0, 1, 2]))
    a.append(np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 5e-324, 1.0, 4.0, 2.0, 1.7976931348623157e308, 2.2250738585072014e-308, -1.0]))
    return np.concatenate(a)


@lru_cache(maxsize=None)
def narrow_operands():
    """(float)a: doubles within a few f64 ulps of f32 values and of the midpoints between neighbouring f32 values (exact ties and
    both sides of them, the kept bit even and odd), over normal and subnormal f32 results, at FLT_MAX (the tie with 2^128) and at half
    the smallest subnormal; random patterns; full mantissas over the whole f64 range (overflow, underflow)."""
    rng = np.random.default_rng(20252)
    p = np.concatenate([rng.integers(0x00800000, 0x7F7FFFFF, size=6000, dtype=np.int64),  # normal results
                        rng.integers(0, 0x00800000, size=4000, dtype=np.int64),             # subnormal results
                        np.arange(0, 300), np.arange(0x007FFF00, 0x00800100),               # the smallest; the subnormal/normal edge
                        np.arange(0x7F7FFF00, 0x7F7FFFFF)])                                 # up to FLT_MAX's lower neighbour
    lo = f32(p.astype(np.uint32)).astype(np.float64)
    hi = f32((p + 1).astype(np.uint32)).astype(np.float64)
    tie = lo + (hi - lo) * 0.5  # exact: neighbouring f32 values and their midpoint have at most 25 significant bits
    top = np.array([3.4028234663852886e38, 3.4028235677973366e38, 2.0 ** 128])  # FLT_MAX, its tie with 2^128, 2^128
    tiny = np.array([2.0 ** -150, 2.0 ** -149, 2.0 ** -151, 2.0 ** -126])
    steps = np.arange(-3, 4)
    near = np.concatenate([step64(tie[tie > 0], steps), step64(lo[lo > 0], steps), step64(top, steps), step64(tiny, steps)])
    wide = full_mantissa(rng, N64, -1022, 1023)
    band = full_mantissa(rng, N64, -160, -120)  # results from zero through the subnormals to small normals
    a = np.concatenate([near, wide, band, full_mantissa(rng, N64 // 4, 120, 130)])
    a = np.concatenate([a, -a, _patterns64(rng, N64), np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 5e-324, -5e-324])])
    return a


@lru_cache(maxsize=None)
def round_i32_operands():
    """d_round_to_i32(a), |a| < 2^31 - 1: k + 1/2 and its two neighbours for positive and negative k (small, random, powers of two),
    integers and their neighbours, random values, and the last doubles inside +-(2^31 - 1)."""
    rng = np.random.default_rng(20253)
    k = np.concatenate([np.arange(-2048, 2048), rng.integers(-(1 << 31) + 2, (1 << 31) - 2, size=N64),
                        (1 << np.arange(1, 31)), -(1 << np.arange(1, 31)), (1 << np.arange(1, 31)) - 1, 1 - (1 << np.arange(1, 31))]).astype(np.float64)
    half = k + 0.5  # exact: |k| < 2^31
    a = [step64(half[half != 0], [-1, 0, 1]), step64(k[k != 0], [-1, 0, 1]), rng.uniform(-2147483646.0, 2147483646.0, N64),
         rng.uniform(-4.0, 4.0, N64), rng.normal(0, 1e-3, 4096), np.array([0.0, -0.0, 0.5, -0.5, 5e-324, -5e-324, 0.49999999999999994, -0.49999999999999994])]
    a.append(step64(np.array([2147483647.0, -2147483647.0]), -np.arange(1, NEIGHBOURS + 1)))  # towards zero from +-(2^31 - 1)
    a = np.concatenate(a)
    assert (np.abs(a) < 2147483647.0).all()
    return a


@lru_cache(maxsize=None)
def from_i64_operands():
    """(double)(int64_t)bits: random patterns; integers of more than 53 significant bits with the round bit set and clear, with and
    without sticky bits below it, the kept bit even and odd, positive and negative; INT64_MIN, INT64_MAX and the other ends."""
    rng = np.random.default_rng(20254)
    n = N64
    width = rng.integers(54, 64, size=n).astype(np.uint64)                  # significant bits, 54..63
    top = rng.integers(1 << 52, 1 << 53, size=n, dtype=np.uint64)           # the 53 bits kept
    drop = width - np.uint64(53)                                            # bits dropped, 1..10
    rnd = rng.integers(0, 2, size=n, dtype=np.uint64) << (drop - np.uint64(1))
    sticky_kind = rng.integers(0, 3, size=n)                                # none, one, random
    below = (np.uint64(1) << (drop - np.uint64(1))) - np.uint64(1)
    sticky = np.where(sticky_kind == 0, np.uint64(0), np.where(sticky_kind == 1, np.minimum(np.uint64(1), below), rng.integers(0, 1 << 10, size=n, dtype=np.uint64) & below))
    v = ((top << drop) | rnd | sticky).astype(np.int64)
    v = np.concatenate([v, -v])
    ends = np.array([-(1 << 63), (1 << 63) - 1, -(1 << 63) + 1, 0, 1, -1, (1 << 53) + 1, (1 << 53) - 1, -(1 << 53) - 1, (1 << 54) + 2, (1 << 54) + 6,
                     (1 << 63) - 512, (1 << 63) - 513, -(1 << 63) + 512, -(1 << 63) + 513, 1 << 62, (1 << 32) - 1, 1 << 32, -(1 << 32)], dtype=np.int64)
    small = rng.integers(-(1 << 40), 1 << 40, size=n // 4, dtype=np.int64)
    return np.concatenate([rng.integers(0, 1 << 64, size=n, dtype=np.uint64), v.view(np.uint64), ends.view(np.uint64), small.view(np.uint64)]).view(np.float64)


LN2 = 0.6931471805599453


def exp_mid_switch_points():
    """(k + 1/2) ln 2 with its neighbours, where d_round_to_i32 steps exp_mid's k."""
    return step64((np.arange(-288, 288) + 0.5) * LN2, np.arange(-NEIGHBOURS, NEIGHBOURS + 1))


@lru_cache(maxsize=None)
def exp_mid_operands():
    """exp_mid(a), |a| <= 200: uniform, small, and the switch points."""
    rng = np.random.default_rng(20255)
    a = np.concatenate([rng.uniform(-200, 200, 3 * N64), rng.normal(0, 1e-3, 4096), exp_mid_switch_points(),
                        np.array([0.0, -0.0, 200.0, -200.0, 100.0, -110.0, 88.72, -87.34, -103.97, 5e-324])])
    assert (np.abs(a) <= 200.0).all()
    return a


def log_pos_switch_points():
    """Mantissas around log_pos's 0x1.6a09e667f3bcd switch at many exponents, and the neighbours of 1."""
    biased = (np.concatenate([np.arange(-1022, 1024, 31), [-1, 0, 1, 1023]]) + 1023).astype(np.uint64)
    sw = (biased << np.uint64(52)) | np.uint64(0x6A09E667F3BCD)
    return np.concatenate([step64(f64(sw), np.arange(-NEIGHBOURS, NEIGHBOURS + 1)), step64(np.array([1.0]), np.arange(-NEIGHBOURS, NEIGHBOURS + 1))])


@lru_cache(maxsize=None)
def log_pos_operands():
    """log_pos(a), a normal double > 0: full mantissas over the whole range, values around 1, and the switch points."""
    rng = np.random.default_rng(20256)
    a = np.concatenate([full_mantissa(rng, 2 * N64, -1022, 1023), full_mantissa(rng, N64, -1, 0), 1.0 + rng.normal(0, 1e-6, N64 // 2),
                        log_pos_switch_points(),
                        np.array([2.2250738585072014e-308, 1.7976931348623157e308, 2.0, 0.5, 1.401298464324817e-45])])
    assert (a >= 2.2250738585072014e-308).all() and np.isfinite(a).all()
    return a


def _sixteenths(m):
    """(y, x) with y/|x| and |x|/y at j/16 for odd j (atan_unit's t*8 at a half-integer) and at 1, from 16m and j*m, with neighbours."""
    st = np.arange(-NEIGHBOURS // 4, NEIGHBOURS // 4 + 1)
    y, x = [], []
    for j in list(range(1, 16, 2)) + [16]:  # 16: y == |x|
        small, big = step64(j * m, st), np.repeat(16.0 * m, st.size)  # j*m < 2^52: exact
        for sx in (1.0, -1.0):
            y += [small, big]
            x += [big * sx, small * sx]
    return y, x


def _sixteenth_multipliers():
    return np.random.default_rng(20259).integers(1 << 40, 1 << 48, size=256).astype(np.float64)


def atan2_upper_switch_points():
    """The sixteenths of the first 16 multipliers of atan2_upper_operands(), whole."""
    y, x = _sixteenths(_sixteenth_multipliers()[:16])
    return np.concatenate(y), np.concatenate(x)


@lru_cache(maxsize=None)
def atan2_upper_operands():
    """atan2_upper(y, x), y >= 0: full mantissas of like and of very different magnitude, quotients at the odd sixteenths and y == |x|
    with neighbours, and the zero / infinity operands its domain allows."""
    rng = np.random.default_rng(20257)
    y = [full_mantissa(rng, N64, -3, 3), full_mantissa(rng, N64, -1022, 1023), full_mantissa(rng, N64, -40, 40)]
    x = [_signed(rng, full_mantissa(rng, N64, -3, 3)), _signed(rng, full_mantissa(rng, N64, -1022, 1023)), _signed(rng, full_mantissa(rng, N64, -40, 40))]
    sy, sx = _sixteenths(_sixteenth_multipliers())
    y, x = y + sy, x + sx
    fin = np.array([1.0, 0.3, 1e300, 1e-300, 5e-324])
    y += [np.zeros(fin.size * 2), np.concatenate([fin, fin]), np.concatenate([fin, fin]), np.full(fin.size * 2, np.inf), np.concatenate([fin, fin])]  # y = 0; x = 0; x infinite; y infinite; plain
    x += [np.concatenate([fin, -fin]), np.concatenate([0.0 * fin, -0.0 * fin]), np.concatenate([fin * np.inf, -fin * np.inf]), np.concatenate([fin, -fin]), np.concatenate([fin[::-1], -fin[::-1]])]
    y, x = np.concatenate(y), np.concatenate(x)
    assert (y >= 0).all() and not (np.isinf(y) & np.isinf(x)).any() and not ((y == 0) & (x == 0)).any()
    return y, x


# ---- exact references for the two software expansions ----------------------------------------------------------------------


def _mant(x):
    """x = m * 2^e with m a 53-bit integer, for a positive normal double."""
    m, e = math.frexp(x)
    return int(m * (1 << 53)), e - 53


def exact_div(a, b):
    """The correctly rounded (nearest, ties to even) a / b of positive normal doubles with a normal quotient, by integer arithmetic."""
    (ma, ea), (mb, eb) = _mant(a), _mant(b)
    s = 52 if ma >= mb else 53  # so that the integer quotient has exactly 53 bits
    n, r = divmod(ma << s, mb)
    if 2 * r > mb or (2 * r == mb and n & 1):
        n += 1
    return math.ldexp(n, ea - eb - s)


def exact_sqrt(a):
    """The correctly rounded square root of a positive normal double, by math.isqrt on the scaled mantissa."""
    m, e = _mant(a)
    s = 52 if (e - 52) % 2 == 0 else 53  # m << s lies in [2^104, 2^106) with an even exponent: its integer root has exactly 53 bits
    big = m << s
    r = math.isqrt(big)
    assert r.bit_length() == 53
    if big - r * r > r:  # big > (r + 1/2)^2 = r^2 + r + 1/4; a tie is impossible for an integer radicand
        r += 1
    return math.ldexp(r, (e - s) // 2)


@lru_cache(maxsize=None)
def exact_operands():
    """A few thousand full-mantissa normal operands whose quotient and root are normal too."""
    rng = np.random.default_rng(20258)
    n = 4096
    a = np.concatenate([full_mantissa(rng, n // 2, 0, 0), full_mantissa(rng, n // 2, -500, 500)])
    b = np.concatenate([full_mantissa(rng, n // 2, 0, 0), full_mantissa(rng, n // 2, -500, 500)])
    return a, b
