"""Shared test support for the history rectification queries: the numpy float32 restatements of rt_temporal_bounds,
rt_temporal_accumulate_bounded and rt_temporal_feedback (include/rt_amd.h "history rectification queries"), the case data, and a small
sequence whose shading changes while its geometry does not.

The restatements do the definition's f32 operations in the definition's order, element-wise over the image for one tap at a time;
numpy's float32 +, -, *, / and sqrt are IEEE single operations, so they equal the CPU forms bit for bit — no tolerance anywhere.  The
gather of the bounded accumulate is restated here once more (steps 1 to 3 and H of _temporal_support.restate_accumulate, which returns
only the blended records): the library must not restate it, a test may.
"""
import functools

import numpy as np

from _denoise_support import synthetic_regions
from _svgf_support import _shifted, vpos
from _temporal_support import F32, HISTORY, Planes, _plane, dot, floor_f32, luminance

BOX = np.dtype([("lo", "<f4", (4,)), ("hi", "<f4", (4,))])
IMAGES = [(1, 1), (1, 17), (17, 1), (16, 16), (17, 33)]
RADII = [1, 2, 3]
INF = F32(np.inf)


def bits(a):
    a = np.ascontiguousarray(a)
    if a.dtype in (HISTORY, BOX):
        return a.view(np.uint32).reshape(-1, 8)
    return a.view(np.uint32)


def same_or_both_nan(a, b):
    """bit-identical, except that a NaN that went through arithmetic is compared as "a NaN" (its sign and payload differ by machine)"""
    a, b = np.ascontiguousarray(a).view(F32).reshape(-1), np.ascontiguousarray(b).view(F32).reshape(-1)
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


@functools.lru_cache(maxsize=None)
def case_data(rows, cols, seed=29):
    """(color, object, valid): colours in [0, 2) with a NaN, an infinity and a -0.0 in sources; objects in blocks of 5 x 3; about a sixth
    of the valid words cleared, the first pixel kept valid.  Shared and left unchanged."""
    g = np.random.default_rng(seed + 1000 * rows + cols)
    n = rows * cols
    r, c = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    color = (g.random((n, 3), dtype=F32) * F32(2.0)).astype(F32)
    color[n // 2, 1] = np.nan
    color[n // 3, 0] = np.inf
    color[(2 * n) // 3] = [-0.0, 0.0, -0.0]
    color[n - 1, 2] = -0.0
    obj = ((r // 5 + c // 3) % 3).reshape(-1).astype(np.uint32)
    valid = (g.random(n) >= 1 / 6).astype(np.uint32)
    valid[0] = 1
    for a in (color, obj, valid):
        a.setflags(write=False)
    return color, obj, valid


def embed(color, obj, valid, words=11):
    """the three planes inside one (n, words) record array with a sentinel pattern between the fields: strided views (color, object, valid)"""
    n = color.shape[0]
    rec = np.full((n, words), -123.5, dtype=F32)
    rec[:, 1:4] = color
    rec.view(np.uint32)[:, 6] = obj
    rec.view(np.uint32)[:, 9] = valid
    return rec, (rec[:, 1:4], rec.view(np.uint32)[:, 6], rec.view(np.uint32)[:, 9])


def channels(color, rows, cols):
    c = np.asarray(color, dtype=F32).reshape(rows, cols, 3)
    with np.errstate(all="ignore"):
        return np.concatenate([c, luminance(c)[..., None]], axis=2).astype(F32)


def window(rows, cols, radius, obj, ok):
    """for every tap in order: (take, qr, qc) — which sources count for which centre"""
    for dr in range(-radius, radius + 1):
        for dc in range(-radius, radius + 1):
            inside, qr, qc = _shifted(rows, cols, dr, dc)
            take = inside & ok[qr, qc]
            if obj is not None:
                take &= obj[qr, qc] == obj
            yield take, qr, qc


def restate_bounds(color, rows, cols, object=None, valid=None, gamma=1.0, radius=1):
    """steps 1 to 7 of rt_temporal_bounds -> (rows * cols,) BOX"""
    x = channels(color, rows, cols)
    ok = np.ones((rows, cols), dtype=bool) if valid is None else (np.asarray(valid).reshape(rows, cols) != 0)
    obj = None if object is None else np.asarray(object).reshape(rows, cols)
    s, v = np.zeros((rows, cols, 4), dtype=F32), np.zeros((rows, cols, 4), dtype=F32)
    k = np.zeros((rows, cols), dtype=np.int64)
    with np.errstate(all="ignore"):
        for take, qr, qc in window(rows, cols, radius, obj, ok):
            s = np.where(take[..., None], s + x[qr, qc], s)
            k = k + take
        kf = np.maximum(k, 1).astype(F32)[..., None]
        mean = s / kf
        for take, qr, qc in window(rows, cols, radius, obj, ok):
            d = x[qr, qc] - mean
            v = np.where(take[..., None], v + d * d, v)
        var = vpos(v / kf)
        sd = np.sqrt(var)
        half = F32(gamma) * sd
        out = np.zeros((rows, cols), dtype=BOX)
        out["lo"] = np.where(ok[..., None], mean - half, -INF)
        out["hi"] = np.where(ok[..., None], mean + half, INF)
    return out.reshape(-1)


def infinite_boxes(n):
    b = np.zeros(n, dtype=BOX)
    b["lo"], b["hi"] = -np.inf, np.inf
    return b


def clamp(x, lo, hi):
    with np.errstate(invalid="ignore"):
        below, above = x < lo, x > hi
    return np.where(below, lo, np.where(above, hi, x)).astype(F32), below | above


def restate_accumulate_bounded(color, motion, rows, cols, history, box, cur=None, prev=None, normal_min=0.9, position_max=0.1, alpha_min=0.05,
                               max_length=32, clamped_length=0):
    """rt_temporal_accumulate's steps 1 to 3 and H, the three operations of the box, then its blend -> (history_out (n,) HISTORY, variance
    (n,) float32, clamped (n,) uint32)"""
    cur, prev = cur or Planes(), prev or Planes()
    n = rows * cols
    C = np.array(color, dtype=F32).reshape(n, 3)
    L = luminance(C)
    px, py = np.array(motion, dtype=F32).reshape(n, 2).T
    h = np.array(history).reshape(n)
    b = np.array(box).reshape(n)
    cn, cp, co, cv = _plane(cur.normal, n, 3), _plane(cur.position, n, 3), _plane(cur.object, n, 1), _plane(cur.valid, n, 1)
    qn, qp, qo, qv = _plane(prev.normal, n, 3), _plane(prev.position, n, 3), _plane(prev.object, n, 1), _plane(prev.valid, n, 1)
    pm2 = F32(position_max) * F32(position_max)
    with np.errstate(all="ignore"):
        gather = (px >= F32(-1)) & (px < F32(cols)) & (py >= F32(-1)) & (py < F32(rows))
        if cv is not None:
            gather &= cv != 0
        sx, sy = np.where(gather, px, F32(0)), np.where(gather, py, F32(0))
        fx, fy = floor_f32(sx), floor_f32(sy)
        wx, wy = sx - fx, sy - fy
        x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
        total = np.zeros((n, 3), dtype=F32)
        s1, s2, bsum = np.zeros(n, dtype=F32), np.zeros(n, dtype=F32), np.zeros(n, dtype=F32)
        least = np.full(n, 0xFFFFFFFF, dtype=np.uint64)
        for j in (0, 1):
            for i in (0, 1):
                w = ((wx if i else F32(1) - wx) * (wy if j else F32(1) - wy)).astype(F32)
                x, y = x0 + i, y0 + j
                take = gather & (w > 0) & (x >= 0) & (x < cols) & (y >= 0) & (y < rows)
                q = np.clip(y, 0, rows - 1) * cols + np.clip(x, 0, cols - 1)
                hq = h[q]
                if qv is not None:
                    take &= qv[q] != 0
                take &= hq["length"] != 0
                if qo is not None:
                    take &= qo[q] == co
                if qn is not None:
                    take &= dot(cn, qn[q]) >= F32(normal_min)
                if qp is not None:
                    d = cp - qp[q]
                    take &= dot(d, d) <= pm2
                total = np.where(take[:, None], total + w[:, None] * hq["color"], total)
                s1 = np.where(take, s1 + w * hq["moment1"], s1)
                s2 = np.where(take, s2 + w * hq["moment2"], s2)
                bsum = np.where(take, bsum + w, bsum)
                least = np.where(take, np.minimum(least, hq["length"].astype(np.uint64)), least)
        blend = bsum > 0
        length = np.where(least >= max_length, max_length, least + 1).astype(np.uint32)
        safe = np.where(blend, bsum, F32(1))
        H, M1, M2 = (total / safe[:, None]).astype(F32), (s1 / safe).astype(F32), (s2 / safe).astype(F32)
        # the three operations
        H, changed3 = clamp(H, b["lo"][:, :3], b["hi"][:, :3])
        M1c, changed1 = clamp(M1, b["lo"][:, 3], b["hi"][:, 3])
        M2 = np.where(changed1, M2 + (M1c * M1c - M1 * M1), M2).astype(F32)
        M1 = M1c
        count = (changed3.sum(axis=1) + changed1).astype(np.uint32)
        if clamped_length:
            length = np.where(count != 0, np.minimum(length, clamped_length), length).astype(np.uint32)
        # the blend
        inv = F32(1) / length.astype(F32)
        alpha = np.where(inv > F32(alpha_min), inv, F32(alpha_min)).astype(F32)
        keep = F32(1) - alpha
        out = np.zeros(n, dtype=HISTORY)
        oc = H * keep[:, None] + C * alpha[:, None]
        m1 = M1 * keep + L * alpha
        m2 = M2 * keep + (L * L) * alpha
        out["color"].view(np.uint32)[:] = np.where(blend[:, None], oc.astype(F32).view(np.uint32), C.view(np.uint32))
        out["moment1"] = np.where(blend, m1, L)
        out["moment2"] = np.where(blend, m2, L * L)
        out["length"] = np.where(blend, length, 1)
        v = out["moment2"] - out["moment1"] * out["moment1"]
        variance = np.where(blend & (v > 0), v, F32(0)).astype(F32)
    return out, variance, np.where(blend, count, 0).astype(np.uint32)


def restate_feedback(color, history, valid=None):
    """rt_temporal_feedback -> a new (n,) HISTORY array"""
    out = np.array(history).reshape(-1).copy()
    c = np.ascontiguousarray(np.asarray(color, dtype=F32).reshape(-1, 3))
    take = out["length"] != 0
    if valid is not None:
        take &= np.asarray(valid).reshape(-1) != 0
    words = out["color"].view(np.uint32).copy()
    words[take] = c.view(np.uint32)[take]
    out["color"] = words.view(F32)
    return out


# ---- a sequence whose shading changes and whose geometry does not ----

SIZE, SIGMA, FRAMES, STEP_FRAME, STEP_REGION, STEP_FACTOR = 64, 0.2, 10, 6, 3, 0.4


def identity_motion(rows, cols):
    r, c = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    return np.stack([c.reshape(-1), r.reshape(-1)], axis=1).astype(F32)


@functools.lru_cache(maxsize=None)
def stepped_sequence(noise=SIGMA, seed=41):
    """_denoise_support.synthetic_regions (64 x 64, four constant quadrants) over FRAMES frames; from frame STEP_FRAME on the brightness of
    quadrant STEP_REGION is multiplied by STEP_FACTOR — a light went out, nothing moved.  Fresh fixed-seed Gaussian noise of sigma `noise`
    per frame.  Returns (clean [frame] (n, 3), noisy [frame] (n, 3), region (n,) uint32, normal, position); shared and left unchanged."""
    base, _, normal, position = synthetic_regions(SIZE, noise)
    r, c = np.meshgrid(np.arange(SIZE), np.arange(SIZE), indexing="ij")
    region = ((r >= SIZE // 2) * 2 + (c >= SIZE // 2)).reshape(-1).astype(np.uint32)
    g = np.random.default_rng(seed)
    clean, noisy = [], []
    for f in range(FRAMES):
        image = base.copy()
        if f >= STEP_FRAME:
            image[region == STEP_REGION] *= F32(STEP_FACTOR)
        image = image.astype(F32)
        frame = (image + g.normal(0.0, noise, image.shape).astype(F32)).astype(F32) if noise else image.copy()
        image.setflags(write=False), frame.setflags(write=False)
        clean.append(image), noisy.append(frame)
    return clean, noisy, region, normal, position
