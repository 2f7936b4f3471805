"""Shared test support for the guided upsampling queries: the cases, the guide data compact and embedded in records, the numpy restatement
of the definition (include/rt_amd.h "guided upsampling queries"), a literal bilinear interpolation, the synthetic truth of the "it
upsamples" test, and the tolerance of the finite-sigma test with its derivation.

The restatement does the definition's f32 operations in the definition's order, element-wise over the output image for one tap at a
time, so with an exponential that returns the same bits it equals the CPU form bit for bit.

THE TOLERANCE OF THE FINITE-SIGMA TEST (RTOL).  u = 2^-24.  The two sides differ in ONE operation: the restatement takes e from np.exp in
float64 rounded to float32, the CPU form from rtdm::exp_mid (relative error < 2^-48 in binary64) rounded to float32; both round a
binary64 value within 2^-48 of the true one, so the two e differ by at most 1 ulp, a relative 2^-23 = 2u.  The two tents t_y and t_x and
their product T = t_y * t_x are the same operations on the same integers on both sides: the same bits.  The case data keeps every
exponent below 14 (unit normals: dist2 <= 4, / 0.8^2 = 6.25; positions in [0, 3)^3: dist2 <= 27, / 2^2 = 6.75), so every e is a normal
number above 2^-21 and "1 ulp" is a relative 2u throughout.  Colours, albedos and weights are non-negative, so nothing cancels.  Then
    w = fl(T * e)            differs by 2u from e, plus one rounding on each side:               4u
    q_k * w                  one more rounding on each side:                                      6u
    numerator, <= 16 terms   either side's recursive sum is within 15u of the exact sum of ITS terms (15 adds), so between the
                             sides 6u + 2 * 15u:                                                 36u
    denominator              4u + 2 * 15u:                                                       34u
    the divide               one rounding on each side:                                           2u
    the remodulation         one product rounding on each side (albedo + 1e-3f is the same bits): 2u
74u to first order; RTOL = 80u leaves the second-order terms (below 74^2 u^2 < 2^-35) room.  The demodulation going in is the same
operations on the same inputs on both sides.  No absolute floor is needed: a channel is +0 on one side only if every term is, on both.
"""
import functools

import numpy as np

F32 = np.float32
INF = float("inf")
U = 2.0 ** -24
RTOL = 80 * U
FINITE_SIGMAS = (0.8, 2.0)  # normal, position: exponents from 0 to 13 on the case data
COLOR_MAX = 4.0
EPS = F32(1e-3)
SCALES = (2, 3, 4)
HOST_SIZES = [(1, 1), (2, 2), (7, 5), (17, 13), (31, 18)]  # (rows, cols) of the OUTPUT; several are no multiple of any scale
HIT_WORDS, SURFACE_WORDS, POSITION_AT, NORMAL_AT, ALBEDO_AT, VALID_AT, OBJECT_AT = 13, 18, 3, 14, 3, 17, 2
DEMOD_IN, DEMOD_OUT = 1, 2


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def low(extent, s):
    return (extent + s - 1) // s


@functools.lru_cache(maxsize=None)
def case_data(rows, cols, seed=11):
    """rows x cols pixels: colour in [0, 4), unit normals, positions in [0, 3)^3, albedo in [0.1, 1), valid with about a fifth of its words
    cleared, objects 0 .. 2 in vertical bands with a ragged edge; shared and left unchanged (copy before writing)"""
    g = np.random.default_rng(seed + 1000 * rows + cols)
    n = rows * cols
    color = (g.random((n, 3), dtype=F32) * F32(COLOR_MAX)).astype(F32)
    normal = g.standard_normal((n, 3)).astype(F32)
    normal = (normal / np.maximum(np.sqrt((normal * normal).sum(axis=1, keepdims=True)), F32(1e-6))).astype(F32)
    position = (g.random((n, 3), dtype=F32) * F32(3.0)).astype(F32)
    albedo = (F32(0.1) + g.random((n, 3), dtype=F32) * F32(0.9)).astype(F32)
    valid = (g.random(n) >= 0.2).astype(np.uint32)
    c = np.tile(np.arange(cols), rows)
    obj = np.minimum((3 * c + g.integers(0, 2, n)) // max(cols, 1), 2).astype(np.uint32)
    for a in (color, normal, position, albedo, valid, obj):
        a.setflags(write=False)
    return color, normal, position, albedo, valid, obj


def embed(normal, position, albedo, valid, obj):
    """the same guides inside (n, 13) and (n, 18) float32 records at primary_surfaces' offsets, the other words filled with a pattern;
    returns the strided views (normal, position, albedo, valid, object) into them"""
    n = normal.shape[0]
    hits = np.full((n, HIT_WORDS), 123.25, dtype=F32)
    surfaces = np.full((n, SURFACE_WORDS), -7.5, dtype=F32)
    hits[:, POSITION_AT:POSITION_AT + 3] = position
    hits.view(np.uint32)[:, OBJECT_AT] = obj
    surfaces[:, NORMAL_AT:NORMAL_AT + 3] = normal
    surfaces[:, ALBEDO_AT:ALBEDO_AT + 3] = albedo
    surfaces.view(np.uint32)[:, VALID_AT] = valid
    return (surfaces[:, NORMAL_AT:NORMAL_AT + 3], hits[:, POSITION_AT:POSITION_AT + 3], surfaces[:, ALBEDO_AT:ALBEDO_AT + 3],
            surfaces.view(np.uint32)[:, VALID_AT], hits.view(np.uint32)[:, OBJECT_AT])


def exp_numpy(x):
    """e of the definition with np.exp in float64, rounded once to float32 (within 1 ulp of the CPU form's)"""
    return np.exp(-x.astype(np.float64)).astype(F32)


def exp_unit(x):
    """e when every exponent is +0 (all sigmas +inf): exactly 1"""
    assert not (x != 0).any()
    return np.ones_like(x)


def dist2(a, b):
    d = a - b
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def axis(extent, s, radius):
    """step 2 along one axis and the tents of step 3: (b, [t of dr = -(R - 1) .. R]) for every output coordinate"""
    r = np.arange(extent, dtype=np.int64)
    a = 2 * r + 1 - s
    b = a // (2 * s)  # numpy's // floors
    f = (a - 2 * s * b).astype(F32) / F32(2 * s)
    return b, [F32(1) - np.abs(F32(dr) - f) / F32(radius) for dr in range(-(radius - 1), radius + 1)]


def restate(color_lo, rows, cols, s, radius, sigmas=(INF, INF), lo=None, hi=None, flags=0, exp=exp_numpy):
    """the definition: color_lo (rows_lo * cols_lo, 3) float32 -> (rows * cols, 3); lo / hi: dicts of the planes normal, position, albedo,
    valid, object that are given; sigmas: (normal, position)"""
    lo, hi = lo or {}, hi or {}
    rl, cl = low(rows, s), low(cols, s)
    c_raw = np.asarray(color_lo, dtype=F32).reshape(rl, cl, 3)
    with np.errstate(all="ignore"):
        c = c_raw / (np.asarray(lo["albedo"], dtype=F32).reshape(rl, cl, 3) + EPS) if flags & DEMOD_IN else c_raw
        ok_lo = np.ones((rl, cl), dtype=bool) if lo.get("valid") is None else np.asarray(lo["valid"]).reshape(rl, cl) != 0
        ok_hi = np.ones((rows, cols), dtype=bool) if hi.get("valid") is None else np.asarray(hi["valid"]).reshape(rows, cols) != 0
        both = lambda k: lo.get(k) is not None and hi.get(k) is not None
        planes = {k: (np.asarray(lo[k]).reshape(rl, cl, -1), np.asarray(hi[k]).reshape(rows, cols, -1)) for k in ("normal", "position", "object") if both(k)}
        sn2, sp2 = (F32(v) * F32(v) for v in sigmas)
        by, ty = axis(rows, s, radius)
        bx, tx = axis(cols, s, radius)
        total = np.zeros((rows, cols, 3), dtype=F32)
        wsum = np.zeros((rows, cols), dtype=F32)
        for kr, dr in enumerate(range(-(radius - 1), radius + 1)):
            for kc, dc in enumerate(range(-(radius - 1), radius + 1)):
                qr, qc = np.broadcast_arrays((by + dr)[:, None], (bx + dc)[None, :])
                t_y, t_x = np.broadcast_arrays(ty[kr][:, None], tx[kc][None, :])
                inside = (qr >= 0) & (qr < rl) & (qc >= 0) & (qc < cl)
                qr, qc = np.clip(qr, 0, rl - 1), np.clip(qc, 0, cl - 1)
                cq = c[qr, qc]
                x = np.zeros((rows, cols), dtype=F32)
                if "normal" in planes:
                    x = x + dist2(planes["normal"][1], planes["normal"][0][qr, qc]) / sn2
                if "position" in planes:
                    x = x + dist2(planes["position"][1], planes["position"][0][qr, qc]) / sp2
                take = (t_y > 0) & (t_x > 0) & inside & ok_lo[qr, qc] & np.isfinite(cq).all(axis=-1) & (x >= 0)
                if "object" in planes:
                    take &= planes["object"][0][qr, qc][..., 0] == planes["object"][1][..., 0]
                e = np.where(x > 100, F32(0), exp(np.where(take & (x <= 100), x, F32(0)))).astype(F32)
                w = (t_y * t_x) * e
                total = np.where(take[..., None], total + np.where(take[..., None], cq, F32(0)) * w[..., None], total)
                wsum = np.where(take, wsum + w, wsum)
        out = total / wsum[..., None]
        if flags & DEMOD_OUT:
            out = out * (np.asarray(hi["albedo"], dtype=F32).reshape(rows, cols, 3) + EPS)
    filtered = ok_hi & (wsum > 0)
    return np.where(filtered[..., None], bits(out.astype(F32)), bits(nearest(c_raw, rows, cols, s))).view(F32).reshape(rows * cols, 3)


def nearest(color_lo, rows, cols, s):
    """nearest replication: output (r, c) is low (r / s, c / s); the raw words"""
    c = np.asarray(color_lo, dtype=F32).reshape(low(rows, s), low(cols, s), 3)
    return c[(np.arange(rows) // s)[:, None], (np.arange(cols) // s)[None, :]]


def bilinear(color_lo, rows, cols, s):
    """the bilinear interpolation of a low image whose pixel j has its centre at output coordinate j s + (s - 1) / 2, written out: the two
    rows and two columns around the output pixel, weights (1 - f) and 1 - (1 - f), renormalised where a neighbour lies outside"""
    rl, cl = low(rows, s), low(cols, s)
    c = np.asarray(color_lo, dtype=F32).reshape(rl, cl, 3)
    out = np.zeros((rows, cols, 3), dtype=F32)
    one = F32(1)
    for r in range(rows):
        a = 2 * r + 1 - s
        y0 = a // (2 * s)
        fy = F32(a - 2 * s * y0) / F32(2 * s)
        wy = [(y0, one - np.abs(F32(0) - fy) / one), (y0 + 1, one - np.abs(F32(1) - fy) / one)]
        for col in range(cols):
            a = 2 * col + 1 - s
            x0 = a // (2 * s)
            fx = F32(a - 2 * s * x0) / F32(2 * s)
            wx = [(x0, one - np.abs(F32(0) - fx) / one), (x0 + 1, one - np.abs(F32(1) - fx) / one)]
            total, wsum = np.zeros(3, dtype=F32), F32(0)
            for y, v in wy:
                for x, h in wx:
                    if 0 <= y < rl and 0 <= x < cl and v > 0 and h > 0:
                        w = F32(v * h) * one
                        total = total + c[y, x] * w
                        wsum = F32(wsum + w)
            out[r, col] = total / wsum
    return out


def synthetic_truth(rows=48, cols=64, s=2):
    """A smooth irradiance ramp times an albedo checker of 3-pixel squares, two objects whose edge lies at column 27 (no multiple of 2,
    3 or 4) with irradiance and albedo of their own.  The low image samples the truth where step 2 puts a low pixel's centre (for an
    even s between four output pixels: the mean of those four guides and colours would be another choice; here the low planes are the
    truth's formulas evaluated AT the centre, as a renderer would).  Returns (truth (rows, cols, 3), color_lo, lo planes, hi planes)."""
    def planes(y, x):
        obj = (x >= 27.0).astype(np.uint32)
        irradiance = (F32(0.5) + F32(0.01) * y.astype(F32) + F32(0.02) * x.astype(F32)) * np.where(obj == 1, F32(2.5), F32(1))
        check = ((np.floor(y / 3) + np.floor(x / 3)) % 2).astype(F32)
        albedo = np.stack([F32(0.2) + F32(0.6) * check, F32(0.8) - F32(0.5) * check, np.where(obj == 1, F32(0.9), F32(0.3)) + 0 * check], axis=-1).astype(F32)
        color = (irradiance[..., None] * (albedo + EPS)).astype(F32)
        normal = np.where(obj[..., None] == 1, np.array([0, 0, 1], dtype=F32), np.array([1, 0, 0], dtype=F32)) + 0 * albedo
        position = np.stack([x, y, 5.0 * obj], axis=-1).astype(F32) * F32(0.05)
        return color, dict(normal=normal.astype(F32).reshape(-1, 3), position=position.reshape(-1, 3), albedo=albedo.reshape(-1, 3),
                           object=obj.reshape(-1), valid=np.ones(obj.size, dtype=np.uint32))
    y, x = np.meshgrid(np.arange(rows, dtype=np.float64), np.arange(cols, dtype=np.float64), indexing="ij")
    truth, hi = planes(y, x)
    yl, xl = np.meshgrid(np.arange(low(rows, s)) * s + (s - 1) / 2, np.arange(low(cols, s)) * s + (s - 1) / 2, indexing="ij")
    color_lo, lo = planes(yl, xl)
    return truth, color_lo.reshape(-1, 3), lo, hi
