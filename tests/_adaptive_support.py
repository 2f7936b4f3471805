"""Shared test support for the adaptive sampling queries: the budget, the list and the listed splat restated in numpy and plain Python,
the permutation between the sample-major and the pixel-major layout, and the cases."""
import functools

import numpy as np

from homework_18_graphics_raytracer_amd import adaptive
from _film_support import F32

U32 = np.uint32
SAMPLE_MAX = 64
LIST_SIZES = [1, 255, 256, 257, 4099, 70001]
SPLAT_IMAGES = [(1, 1), (15, 15), (16, 16), (17, 17), (16, 33), (48, 40)]
SPLAT_RADII = [0.5, 1.0, 2.0, 3.0, 4.0]  # reach 1, 2, 3, 4 and 5
ZERO_RAY = np.zeros(11, dtype=U32)


def bits(a):
    return np.ascontiguousarray(a).view(U32)


def same_or_both_nan(got, want):
    g, w = np.ascontiguousarray(got, dtype=F32), np.ascontiguousarray(want, dtype=F32)
    return g.shape == w.shape and bool(((bits(g) == bits(w)) | (np.isnan(g) & np.isnan(w))).all())


# ---- rt_sample_budget ----

def budget_restated(mean, variance, count, valid, gain, epsilon, min_count, max_count):
    """the six steps of include/rt_amd.h, element-wise in float32"""
    mean, variance = np.asarray(mean, dtype=F32), np.asarray(variance, dtype=F32)
    count = np.ones(mean.shape, dtype=U32) if count is None else np.asarray(count).astype(U32)
    with np.errstate(all="ignore"):
        e = np.sqrt(variance / np.maximum(count, 1).astype(F32)) / (np.abs(mean) + F32(epsilon))
        t = e * F32(gain)
    span = max_count - min_count
    below = t < F32(span)  # false for a NaN
    out = U32(min_count) + np.where(below, np.where(below, t, F32(0)).astype(U32), U32(span))
    out = np.where(count == 0, U32(max_count), out)
    if valid is not None:
        out = np.where(np.asarray(valid) == 0, U32(0), out)
    return out.astype(U32)


def budget_case(n, seed=5):
    """mean, variance, count, valid with every special value of the definition somewhere"""
    rng = np.random.default_rng(seed)
    mean = (rng.random(n, dtype=F32) - F32(0.3)) * F32(2.0)
    variance = rng.random(n, dtype=F32) * F32(0.5)
    count = rng.integers(0, 9, n).astype(U32)
    valid = (rng.random(n) >= 0.2).astype(U32)
    special = [F32(0.0), F32(-1.0), F32(np.nan), F32(np.inf), F32(1e30)]
    for k, v in enumerate(special):
        variance[k::23] = v
    mean[3::31] = F32(0.0)
    mean[4::37] = F32(np.nan)
    return mean, variance, count, valid


# ---- rt_sample_list ----

def list_restated(counts, capacity, first=None):
    """start, pixel, sample, total and the advanced first, from numpy.cumsum"""
    c = np.minimum(np.asarray(counts).astype(np.uint64), SAMPLE_MAX)
    s = np.concatenate([[0], np.cumsum(c, dtype=np.uint64)]).astype(np.uint64)
    start = np.minimum(s, np.uint64(capacity)).astype(U32)
    listed = int(start[-1])
    got = np.diff(start.astype(np.int64))
    pixel = np.repeat(np.arange(c.size, dtype=U32), got)
    f = np.zeros(c.size, dtype=U32) if first is None else np.asarray(first).astype(U32)
    sample = (np.arange(listed, dtype=np.int64) - np.repeat(start[:-1].astype(np.int64), got) + np.repeat(f.astype(np.int64), got)).astype(U32)
    return start, pixel, sample, np.array([listed, int(s[-1])], dtype=U32), (f + got.astype(U32)).astype(U32)


def same_list(sl, want, first=None):
    """a SampleList of numpy arrays against list_restated's tuple; entries at and beyond total[0] are unspecified"""
    start, pixel, sample, total, advanced = want
    listed = int(total[0])
    ok = (np.array_equal(bits(sl.start), start) and np.array_equal(bits(sl.total), total) and np.array_equal(bits(sl.pixel)[:listed], pixel)
          and np.array_equal(bits(sl.sample)[:listed], sample))
    return ok and (first is None or np.array_equal(bits(first), advanced))


@functools.lru_cache(maxsize=None)
def counts_case(n, kind):
    rng = np.random.default_rng(n * 7 + len(kind))
    if kind == "zeros":
        c = np.zeros(n, dtype=U32)
    elif kind == "full":
        c = np.full(n, SAMPLE_MAX, dtype=U32)
    elif kind == "single":  # one 64 among zeros, last of its 256-pixel step: what the binary search can get wrong
        c = np.zeros(n, dtype=U32)
        c[min(n - 1, 255)] = SAMPLE_MAX
        if n > 300:
            c[256] = SAMPLE_MAX
    elif kind == "above":  # counts above 64 are read as 64
        c = rng.integers(0, 200, n).astype(U32)
        c[::5] = U32(0xFFFFFFFF)
    else:
        c = rng.integers(0, SAMPLE_MAX + 1, n).astype(U32)
    c.setflags(write=False)
    return c


# ---- the layouts ----

def to_pixel_major(a):
    """(spp, n, k) sample-major -> (n * spp, k) pixel-major: record i * spp + s is sample s of pixel i"""
    a = np.asarray(a)
    if a.ndim == 2:
        return np.ascontiguousarray(a.T).reshape(-1)
    return np.ascontiguousarray(a.transpose(1, 0, 2)).reshape(-1, a.shape[2])


# ---- rt_film_splat_listed ----

def filter_scalar(name, d, radius):
    d, radius = F32(d), F32(radius)
    if name == "box":
        return F32(1.0)
    if name == "tent":
        return F32(F32(1.0) - F32(abs(d)) / radius)
    x = F32(F32(2.0) * F32(abs(d)) / radius)
    if x < F32(1.0):
        return F32((F32(F32(F32(F32(7.0) * x) - F32(12.0)) * x * x) + F32(16.0) / F32(3.0)) / F32(6.0))
    return F32((F32(F32(F32(F32(F32(F32(-7.0) / F32(3.0) * x) + F32(12.0)) * x) - F32(20.0)) * x) + F32(32.0) / F32(3.0)) / F32(6.0))


def splat_listed_literal(rows, cols, samples, valid, offsets, start, capacity, max_count, name, radius, total, weight):
    """The definition as a literal loop over output pixels, every operation an np.float32 scalar operation"""
    total, weight = np.array(total, dtype=F32), np.array(weight, dtype=F32)
    rad = F32(radius)
    reach = int(np.ceil(rad + F32(0.5)))
    lo = np.minimum(start.astype(np.int64), capacity)
    for r in range(rows):
        for c in range(cols):
            acc, w_sum = [total[r, c, k] for k in range(3)], weight[r, c]
            for s in range(max_count):
                for dr in range(-reach, reach + 1):
                    for dc in range(-reach, reach + 1):
                        qr, qc = r + dr, c + dc
                        if not (0 <= qr < rows and 0 <= qc < cols):
                            continue
                        q = qr * cols + qc
                        if s >= max(lo[q + 1] - lo[q], 0):
                            continue
                        rec = lo[q] + s
                        if valid is not None and valid[rec] == 0:
                            continue
                        ddx, ddy = F32(F32(dc) + offsets[rec, 0]), F32(F32(dr) + offsets[rec, 1])
                        if not (-rad <= ddx < rad and -rad <= ddy < rad):
                            continue
                        w = F32(filter_scalar(name, ddx, radius) * filter_scalar(name, ddy, radius))
                        for k in range(3):
                            acc[k] = F32(acc[k] + F32(samples[rec, k] * w))
                        w_sum = F32(w_sum + w)
            total[r, c], weight[r, c] = acc, w_sum
    return total, weight


@functools.lru_cache(maxsize=None)
def splat_case(rows, cols, most, seed=0):
    """random counts 0 .. most, their list, and one record per listed sample: samples, flags (a quarter cleared), offsets (some on a
    border, some beyond the pixel) and a running (sum, weight); read-only"""
    rng = np.random.default_rng(rows * 1000 + cols * 10 + most + seed)
    n = rows * cols
    counts = rng.integers(0, most + 1, n).astype(U32)
    sl = adaptive.sample_list_numpy(counts)
    cap = sl.capacity
    samples = rng.random((cap, 3), dtype=F32) * F32(4.0)
    valid = (rng.random(cap) >= 0.25).astype(np.uint8)
    offsets = rng.random((cap, 2), dtype=F32) - F32(0.5)
    pick = rng.random((cap, 2))
    offsets[pick < 0.03] = F32(-0.5)
    offsets[(pick >= 0.03) & (pick < 0.06)] = F32(0.5)
    offsets[(pick >= 0.06) & (pick < 0.09)] *= F32(3.0)
    total = rng.random((rows, cols, 3), dtype=F32)
    weight = rng.random((rows, cols), dtype=F32)
    for a in (counts, samples, valid, offsets, total, weight):
        a.setflags(write=False)
    return counts, sl, samples, valid, offsets, total, weight


def host_splat_listed(rows, cols, samples, valid, offsets, sl, name, radius, total=None, weight=None, max_count=SAMPLE_MAX):
    from homework_18_graphics_raytracer_amd import film

    f = film.Film(rows, cols, name, radius)
    if total is not None:
        f.sum[...] = total
        f.weight[...] = weight
    adaptive.splat_listed(f, samples, offsets, sl, valid, max_count)
    return f.sum, f.weight
