"""Shared test support for the denoise queries: the cases, the guide data compact and embedded in records, the numpy restatement of one
level of the definition (include/rt_amd.h "denoise queries"), and the tolerance of the weights test with its derivation.

The restatement does the definition's f32 operations in the definition's order, element-wise over the image for one tap at a time, so
with an exponential that returns the same bits it equals the CPU form bit for bit.

THE TOLERANCE OF THE WEIGHTS TEST (RTOL, ATOL).  With finite sigmas the restatement takes e from np.exp in float64 rounded to float32;
the CPU form takes it from rtdm::exp_mid (relative error < 2^-48 in binary64) rounded to float32.  Both round a binary64 value within
2^-48 of the true one, so the two e differ by at most 1 ulp, a relative 2^-23 = 2u with u = 2^-24.  Everything else is the same
operations on the same inputs.  For non-negative colours every term of sum_k and wsum is non-negative, so the recursively summed
numerator of either side is within (25 + 1) u of its exact sum of terms (one product rounding, at most 25 adds), and so is the
denominator with 25 u.  Between the two sides: the weights w = (h * h) * e differ by 2u from e plus u from the changed rounding of the
product, 3u; the numerators then differ by at most 3u + 2 * 26u = 55u, the denominators by 3u + 2 * 25u = 53u, and each divide adds
u: (55 + 53 + 2) u = 110 u < 128 u = 2^-17 relative.  A weight whose e is subnormal (87 < x <= 100) has coarser ulps, but it is below
2^-126 beside a centre tap of weight 9/64, so it moves nothing; the absolute floor for channels near zero is the same bound times the
largest input, 2^-17 * 4.
"""
import functools

import numpy as np

F32 = np.float32
IMAGES = [(1, 1), (1, 70), (70, 1), (23, 37)]
LEVELS = [0, 1, 2, 3, 4, 5]
INF = float("inf")
FINITE_SIGMAS = (1.5, 0.8, 2.0)  # colour, normal, position: exponents from 0 to beyond 100 on the case data
COLOR_MAX = 4.0
RTOL = 2.0 ** -17
ATOL = 2.0 ** -17 * COLOR_MAX
H = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16], dtype=F32)
EPS = F32(1e-3)
# where primary_surfaces' views lie in the records (words): position in rt_hit, the others in rt_surface
HIT_WORDS, SURFACE_WORDS, POSITION_AT, NORMAL_AT, ALBEDO_AT, VALID_AT = 13, 18, 3, 14, 3, 17


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@functools.lru_cache(maxsize=None)
def case_data(rows, cols, seed=7):
    """colour in [0, 4), unit normals, positions in [0, 3)^3, albedo in [0.1, 1), valid with about a quarter of its words cleared;
    shared and left unchanged (copy before writing)"""
    g = np.random.default_rng(seed + 1000 * rows + cols)
    n = rows * cols
    color = (g.random((n, 3), dtype=F32) * F32(COLOR_MAX)).astype(F32)
    normal = g.standard_normal((n, 3)).astype(F32)
    normal = (normal / np.maximum(np.sqrt((normal * normal).sum(axis=1, keepdims=True)), F32(1e-6))).astype(F32)
    position = (g.random((n, 3), dtype=F32) * F32(3.0)).astype(F32)
    albedo = (F32(0.1) + g.random((n, 3), dtype=F32) * F32(0.9)).astype(F32)
    valid = (g.random(n) >= 0.25).astype(np.uint32)
    for a in (color, normal, position, albedo, valid):
        a.setflags(write=False)
    return color, normal, position, albedo, valid


def embed(normal, position, albedo, valid):
    """the same guides inside (n, 13) and (n, 18) float32 records at primary_surfaces' offsets, the other words filled with a pattern;
    returns (hits, surfaces) and the strided views (normal, position, albedo, valid) into them"""
    n = normal.shape[0]
    hits = np.full((n, HIT_WORDS), 123.25, dtype=F32)
    surfaces = np.full((n, SURFACE_WORDS), -7.5, dtype=F32)
    hits[:, POSITION_AT:POSITION_AT + 3] = position
    surfaces[:, NORMAL_AT:NORMAL_AT + 3] = normal
    surfaces[:, ALBEDO_AT:ALBEDO_AT + 3] = albedo
    surfaces.view(np.uint32)[:, VALID_AT] = valid
    return hits, surfaces, record_views(hits, surfaces)


def record_views(hits, surfaces):
    return (surfaces[:, NORMAL_AT:NORMAL_AT + 3], hits[:, POSITION_AT:POSITION_AT + 3], surfaces[:, ALBEDO_AT:ALBEDO_AT + 3],
            surfaces.view(np.uint32)[:, VALID_AT])


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


def restate_level(image, rows, cols, level, sigmas, normal=None, position=None, valid=None, exp=exp_numpy):
    """one level of the definition, no demodulation: image (rows * cols, 3) float32 -> the same shape; sigmas: (sc, sn, sp) OF THIS LEVEL"""
    s = 1 << level
    c = np.asarray(image, dtype=F32).reshape(rows, cols, 3)
    ok = np.ones((rows, cols), dtype=bool) if valid is None else (np.asarray(valid).reshape(rows, cols) != 0)
    nrm = None if normal is None else np.asarray(normal, dtype=F32).reshape(rows, cols, 3)
    pos = None if position is None else np.asarray(position, dtype=F32).reshape(rows, cols, 3)
    sc2, sn2, sp2 = (F32(v) * F32(v) for v in sigmas)
    r, col = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    total = np.zeros((rows, cols, 3), dtype=F32)
    wsum = np.zeros((rows, cols), dtype=F32)
    with np.errstate(all="ignore"):
        for dr in range(-2, 3):
            for dc in range(-2, 3):
                qr, qc = r + dr * s, col + dc * s
                inside = (qr >= 0) & (qr < rows) & (qc >= 0) & (qc < cols)
                qr, qc = np.clip(qr, 0, rows - 1), np.clip(qc, 0, cols - 1)
                cq = c[qr, qc]
                x = dist2(c, cq) / sc2
                if nrm is not None:
                    x = x + dist2(nrm, nrm[qr, qc]) / sn2
                if pos is not None:
                    x = x + dist2(pos, pos[qr, qc]) / sp2
                take = inside & ok & ok[qr, qc] & (x >= 0)
                e = np.where(x > 100, F32(0), exp(np.where(take & (x <= 100), x, F32(0)))).astype(F32)
                w = (H[dr + 2] * H[dc + 2]) * e
                total = np.where(take[..., None], total + cq * w[..., None], total)
                wsum = np.where(take, wsum + w, wsum)
        out = np.where((ok & (wsum > 0))[..., None], total / wsum[..., None], c)
    return out.astype(F32).reshape(rows * cols, 3)


def level_sigma_color(sigma_color, j):
    """the colour sigma of level j (0-based) of a call: an exact multiply by a power of two"""
    return F32(sigma_color) * (F32(1.0) / F32(1 << j))


def synthetic_regions(size=64, noise=0.2, seed=3):
    """four constant quadrants with distinct colours, unit normals and positions, plus fixed-seed Gaussian noise: (clean, noisy, normal,
    position), each (size * size, 3) float32"""
    g = np.random.default_rng(seed)
    r, c = np.meshgrid(np.arange(size), np.arange(size), indexing="ij")
    region = ((r >= size // 2) * 2 + (c >= size // 2)).reshape(-1)
    colors = np.array([[0.9, 0.2, 0.1], [0.1, 0.8, 0.3], [0.2, 0.3, 0.9], [0.7, 0.7, 0.6]], dtype=F32)
    normals = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0]], dtype=F32)
    base = np.array([[0, 0, 0], [10, 0, 0], [0, 10, 0], [0, 0, 10]], dtype=F32)
    clean = colors[region]
    noisy = (clean + g.normal(0.0, noise, clean.shape).astype(F32)).astype(F32)
    position = (base[region] + np.stack([c.reshape(-1), r.reshape(-1), np.zeros(size * size)], axis=1).astype(F32) * F32(0.01)).astype(F32)
    return clean, noisy, normals[region], position
