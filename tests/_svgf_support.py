"""Shared test support for the variance-guided filter queries: the case data, the numpy float32 restatements of rt_svgf_variance and of one
level of rt_svgf_atrous (include/rt_amd.h "variance-guided filter queries"), and the tolerances of the finite-sigma tests with their
derivations.

The restatements do the definition's f32 operations in the definition's order, element-wise over the image for one tap at a time;
numpy's float32 +, -, *, / and sqrt are IEEE single operations, so with an exponential that returns the same bits they equal the CPU
forms bit for bit.

THE TOLERANCES OF THE FINITE-SIGMA TESTS.  u = 2^-24.  As in _denoise_support the restatement takes e from np.exp in float64 rounded to
float32 and the CPU form from rtdm::exp_mid rounded to float32: both round a binary64 value within 2^-48 of the true one, so the two e
differ by at most 1 ulp, a relative 2u.  NOTHING ELSE differs between the two sides: the 3 x 3 prefilter (products by exact powers of
two, adds, one divide), the square root (np.sqrt and rtdm::f_sqrt are both the correctly rounded IEEE root), sl and therefore every
exponent x are the same operations on the same inputs and come out with the same bits — so the prefilter and the root add 0 to the
bounds below, and both sides take the same side of every x >= 0 and x > 100 test.

  rt_svgf_atrous, colour (ATROUS_RTOL, ATROUS_ATOL).  w = fl((h * h) * e): the two sides' w differ by at most 2u (from e) + 2u (one
  product rounding on either side) = 4u.  For non-negative colours every term of sum_k and wsum is non-negative, so either side's
  numerator is within (25 + 1) u of its exact sum of terms (one product rounding, at most 25 adds) and its denominator within 25 u.
  Between the sides: numerators 4u + 2 * 26u = 56u, denominators 4u + 2 * 25u = 54u, one divide each 2u, and on a remodulating level one
  more product each 2u: 114u < 128u = 2^-17 relative; the absolute floor for channels near zero is the same bound times the largest
  colour the filter sees, COLOR_MAX / (least albedo + 1e-3) < 4 / 0.1 = 40.
  rt_svgf_atrous, variance (VARIANCE_RTOL, VARIANCE_ATOL).  V_q >= 0 after vpos, so vsum too is a sum of non-negative terms V_q * (w * w).
  The exact w^2 of the two sides differ by 2 * 4u = 8u; either side's vsum is within (2 + 25) u of its exact sum (the w * w product, the
  V * (w w) product, at most 25 adds): 8u + 2 * 27u = 62u between the sides.  The denominators wsum differ by 54u as above, so wsum *
  wsum by 2 * 54u + 2u = 110u, and the variance divide adds 2u: 62 + 110 + 2 = 174u < 256u = 2^-16 relative; the absolute floor is that
  bound times the largest variance of the case data, VARIANCE_MAX.  A weight whose e is subnormal, or a w * w that underflows, has lost
  its relative accuracy but lies below 2^-126 beside a centre tap of (9/64)^2: it moves nothing above the floor.
  rt_svgf_variance (ESTIMATE_ATOL).  w = e with no product: the sides' w differ by 2u.  The case data's moments are non-negative, so s1,
  s2 and wsum are sums of non-negative terms over at most 49 taps: either side within (1 + 48) u of its exact sum, the sides 2u + 98u =
  100u apart for s1 and s2 and 98u for wsum; a1 and a2 then 100 + 98 + 2 = 200u apart.  v = a2 - a1 * a1 cancels, so the bound is
  absolute: |d a2| <= 200u * a2, |d (a1 * a1)| <= (400 + 2) u * a1^2, the subtraction 2u * a2; with a1 <= MOMENT1_MAX = 1 and a2 <=
  MOMENT2_MAX = 1.5 that is (300 + 402 + 3) u = 705u.  The clamp at 0 does not widen it; the factor min_length / length <= min_length =
  4 (with its two roundings, relative 2u of a v <= 1.5) does: 4 * 705u + 12u = 2832u < 4096u = 2^-12, absolute.
"""
import functools

import numpy as np

from _denoise_support import EPS, F32, H, INF, case_data as denoise_case_data, dist2, exp_numpy, exp_unit
from _temporal_support import HISTORY, luminance

IMAGES = [(1, 1), (1, 70), (70, 1), (23, 37)]
LEVELS = [0, 1, 2, 3, 4, 5]
MIN_LENGTH = 4
FINITE_SIGMAS = (2.5, 0.8, 2.0)  # luminance, normal, position: exponents from 0 to beyond 100 on the case data
VARIANCE_MAX, MOMENT1_MAX, MOMENT2_MAX = 2.0, 1.0, 1.5
ATROUS_RTOL, ATROUS_ATOL = 2.0 ** -17, 2.0 ** -17 * 40.0
VARIANCE_RTOL, VARIANCE_ATOL = 2.0 ** -16, 2.0 ** -16 * VARIANCE_MAX
ESTIMATE_ATOL = 2.0 ** -12
HK = np.array([1 / 4, 1 / 2, 1 / 4], dtype=F32)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@functools.lru_cache(maxsize=None)
def case_data(rows, cols, seed=13):
    """_denoise_support's case (colour in [0, 4), unit normals, positions, albedo in [0.1, 1), valid with about a quarter cleared) with a
    few NaN colours on valid and on cleared pixels; a variance plane in [0, 2) that includes +0, NaN and negative values; and history
    records with lengths 0 .. 6 (so 0, 1, MIN_LENGTH - 1 and MIN_LENGTH occur), moment1 in [0, 1), moment2 in [0, 1.5) and the colour
    inside.  Returns (color, variance, history, normal, position, albedo, valid); shared and left unchanged (copy before writing)."""
    color, normal, position, albedo, valid = denoise_case_data(rows, cols)
    g = np.random.default_rng(seed + 1000 * rows + cols)
    n = rows * cols
    color = color.copy()
    for q in sorted({0, n // 3, n // 2 + 1, n - 1}):
        color[q % n, q % 3] = np.nan
    variance = (g.random(n, dtype=F32) * F32(VARIANCE_MAX)).astype(F32)
    variance[::5] = 0.0
    variance[3::11] = np.nan
    variance[4::7] = -0.5
    history = np.zeros(n, dtype=HISTORY)
    history["color"] = color
    history["moment1"] = g.random(n, dtype=F32) * F32(MOMENT1_MAX)
    history["moment2"] = g.random(n, dtype=F32) * F32(MOMENT2_MAX)
    history["length"] = g.integers(0, 7, n)
    history["length"][:7] = [1, 0, MIN_LENGTH - 1, MIN_LENGTH, 6, 2, 5][:n]
    for a in (color, variance, history):
        a.setflags(write=False)
    return color, variance, history, normal, position, albedo, valid


def vpos(v):
    with np.errstate(invalid="ignore"):
        return np.where(v >= 0, v, F32(0)).astype(F32)


def _shifted(rows, cols, dr, dc):
    r, c = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    qr, qc = r + dr, c + dc
    inside = (qr >= 0) & (qr < rows) & (qc >= 0) & (qc < cols)
    return inside, np.clip(qr, 0, rows - 1), np.clip(qc, 0, cols - 1)


def _exponent(take, x, exp):
    return np.where(x > 100, F32(0), exp(np.where(take & (x <= 100), x, F32(0)))).astype(F32)


def restate_variance(history, rows, cols, normal=None, position=None, valid=None, min_length=MIN_LENGTH, sigmas=(INF, INF), exp=exp_numpy):
    """steps 1 to 3 of rt_svgf_variance -> (rows * cols,) float32"""
    h = np.asarray(history).reshape(rows, cols)
    m1, m2, length = h["moment1"].astype(F32), h["moment2"].astype(F32), h["length"]
    ok = length != 0
    if valid is not None:
        ok &= np.asarray(valid).reshape(rows, cols) != 0
    nrm = None if normal is None else np.asarray(normal, dtype=F32).reshape(rows, cols, 3)
    pos = None if position is None else np.asarray(position, dtype=F32).reshape(rows, cols, 3)
    sn2, sp2 = (F32(v) * F32(v) for v in sigmas)
    s1, s2, wsum = (np.zeros((rows, cols), dtype=F32) for _ in range(3))
    with np.errstate(all="ignore"):
        for dr in range(-3, 4):
            for dc in range(-3, 4):
                inside, qr, qc = _shifted(rows, cols, dr, dc)
                x = np.zeros((rows, cols), dtype=F32)
                if nrm is not None:
                    x = x + dist2(nrm, nrm[qr, qc]) / sn2
                if pos is not None:
                    x = x + dist2(pos, pos[qr, qc]) / sp2
                take = inside & ok[qr, qc] & (x >= 0)
                w = _exponent(take, x, exp)
                s1 = np.where(take, s1 + m1[qr, qc] * w, s1)
                s2 = np.where(take, s2 + m2[qr, qc] * w, s2)
                wsum = np.where(take, wsum + w, wsum)
        safe = np.where(wsum > 0, wsum, F32(1))
        a1, a2 = s1 / safe, s2 / safe
        v = a2 - a1 * a1
        v = np.where(v > 0, v, F32(0)).astype(F32)
        spatial = np.where(wsum > 0, v * (F32(min_length) / np.maximum(length, 1).astype(F32)), F32(0))
        t = m2 - m1 * m1
        temporal = np.where(t > 0, t, F32(0))
        out = np.where(~ok, F32(0), np.where(length >= min_length, temporal, spatial))
    return out.astype(F32).reshape(-1)


def restate_level(color, variance, rows, cols, level, sigmas, normal=None, position=None, albedo=None, valid=None, demod_in=False, demod_out=False,
                  exp=exp_numpy):
    """one level of rt_svgf_atrous: color (rows * cols, 3), variance (rows * cols,) -> the same shapes; sigmas: (luminance, normal, position)"""
    s = 1 << level
    raw = np.ascontiguousarray(color, dtype=F32).reshape(rows, cols, 3)
    vraw = np.ascontiguousarray(variance, dtype=F32).reshape(rows, cols)
    ok = np.ones((rows, cols), dtype=bool) if valid is None else (np.asarray(valid).reshape(rows, cols) != 0)
    nrm = None if normal is None else np.asarray(normal, dtype=F32).reshape(rows, cols, 3)
    pos = None if position is None else np.asarray(position, dtype=F32).reshape(rows, cols, 3)
    alb = None if albedo is None else np.asarray(albedo, dtype=F32).reshape(rows, cols, 3)
    sl_, sn, sp = (F32(v) for v in sigmas)
    sn2, sp2 = sn * sn, sp * sp
    with np.errstate(all="ignore"):
        c = (raw / (alb + EPS)).astype(F32) if demod_in else raw
        lum = luminance(c).astype(F32)
        V = vpos(vraw)
        gs, ks = np.zeros((rows, cols), dtype=F32), np.zeros((rows, cols), dtype=F32)
        for dr in range(-1, 2):
            for dc in range(-1, 2):
                inside, qr, qc = _shifted(rows, cols, dr, dc)
                take = inside & ok[qr, qc]
                k = HK[dr + 1] * HK[dc + 1]
                gs = np.where(take, gs + k * V[qr, qc], gs)
                ks = np.where(take, ks + k, ks)
        g = np.where(ks > 0, gs / np.where(ks > 0, ks, F32(1)), F32(0)).astype(F32)
        sl = (sl_ * (np.sqrt(g) + F32(1e-6))).astype(F32)
        total = np.zeros((rows, cols, 3), dtype=F32)
        vsum, wsum = np.zeros((rows, cols), dtype=F32), np.zeros((rows, cols), dtype=F32)
        for dr in range(-2, 3):
            for dc in range(-2, 3):
                inside, qr, qc = _shifted(rows, cols, dr * s, dc * s)
                cq = c[qr, qc]
                x = np.abs(lum - lum[qr, qc]) / sl
                if nrm is not None:
                    x = x + dist2(nrm, nrm[qr, qc]) / sn2
                if pos is not None:
                    x = x + dist2(pos, pos[qr, qc]) / sp2
                take = inside & ok & ok[qr, qc] & (x >= 0)
                w = (H[dr + 2] * H[dc + 2]) * _exponent(take, x, exp)
                total = np.where(take[..., None], total + cq * w[..., None], total)
                vsum = np.where(take, vsum + V[qr, qc] * (w * w), vsum)
                wsum = np.where(take, wsum + w, wsum)
        filtered = ok & (wsum > 0)
        safe = np.where(filtered, wsum, F32(1))
        o = total / safe[..., None]
        if demod_out:
            o = o * (alb + EPS)
        out = np.where(filtered[..., None], o.astype(F32).view(np.uint32), raw.view(np.uint32)).view(F32)
        vout = np.where(filtered, (vsum / (safe * safe)).astype(F32).view(np.uint32), vraw.view(np.uint32)).view(F32)
    return out.reshape(rows * cols, 3), vout.reshape(-1)
