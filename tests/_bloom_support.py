"""What the bloom tests share: the definition of include/rt_amd.h "bloom queries" restated in numpy float32 — every step there is a single
f32 operation, and numpy rounds each elementwise float32 operation once, the divide included, so the restatement gives the definition's
bits — and the case data."""
import functools

import numpy as np

import homework_18_graphics_raytracer_amd as rt

F32 = np.float32
THREE = F32(3.0)
SIZES = [(1, 1), (2, 2), (3, 5), (16, 16), (17, 17), (31, 18), (33, 65)]
LEVELS = [1, 2, 5]
KNEES = [0.0, 0.5]
RECORD_WORDS = 8


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_or_both_nan(a, b):
    """bit-identical, except that a NaN that went through arithmetic is "a NaN" (its sign and payload differ by machine)"""
    a, b = np.ascontiguousarray(a, dtype=F32).reshape(-1), np.ascontiguousarray(b, dtype=F32).reshape(-1)
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def half(n):
    return (n + 1) // 2


def level_sizes(rows, cols, levels):
    """[(rows_1, cols_1), ..., (rows_L, cols_L)]"""
    sizes = []
    for _ in range(levels):
        rows, cols = half(rows), half(cols)
        sizes.append((rows, cols))
    return sizes


def temp_bytes(rows, cols, levels):
    return sum(r * c * 12 for r, c in level_sizes(rows, cols, levels))


@functools.lru_cache(maxsize=None)
def case_data(rows, cols, seed=31):
    """a positive (rows, cols, 3) image with lumas below 0.9, in which about 2 % of the pixels (and always the first) are lifted above
    the threshold 1.0 by factors from 1.5 to 1000: several scales of excess.  Shared and left unchanged (copy before writing)."""
    g = np.random.default_rng(seed + 1000 * rows + cols)
    color = (F32(0.05) + g.random((rows, cols, 3), dtype=F32) * F32(0.8)).astype(F32)
    lifted = g.random((rows, cols)) < 0.02
    lifted[0, 0] = True
    factor = np.array([1.5, 4.0, 30.0, 1000.0], dtype=F32)[g.integers(0, 4, size=(rows, cols))]
    color[lifted] = (color[lifted] * F32(24.0) * factor[lifted][:, None]).astype(F32)  # every channel at least 0.05 * 24 * 1.5 = 1.8
    color.setflags(write=False)
    return color


def in_records(color, fill=3.5):
    """(records, the view of the colour inside them): RECORD_WORDS words per pixel, the colour first, as in history records"""
    records = np.full(color.shape[:2] + (RECORD_WORDS,), fill, dtype=F32)
    records[..., :3] = color
    return records, records[..., :3]


# ---- the definition, step by step ----

def bright(c, threshold, knee):
    w0, w1, w2 = (F32(w) for w in rt.luma_row())
    with np.errstate(all="ignore"):
        l = (w0 * c[..., 0] + w1 * c[..., 1]) + w2 * c[..., 2]
        finite = ((c - c) == 0).all(axis=-1)
        s = l - F32(threshold)
        if knee > 0:
            k = F32(knee)
            t = np.fmin(np.fmax(s + k, F32(0)), F32(2) * k)
            q = (t * t) / (F32(4) * k)
            m = np.fmax(s, q)
        else:
            m = s
        glows = finite & (l > 0) & (m > 0)
        scaled = c * (m / l)[..., None]
    return np.where(glows[..., None], scaled, F32(0)).astype(F32)


def tent4(s0, s1, s2, s3):
    return (s0 + THREE * s1) + (THREE * s2 + s3)


def down(S):
    R, C = S.shape[:2]
    rows = [np.clip(2 * np.arange(half(R)) - 1 + k, 0, R - 1) for k in range(4)]
    cols = [np.clip(2 * np.arange(half(C)) - 1 + k, 0, C - 1) for k in range(4)]
    h = [tent4(*(S[rows[kr]][:, cols[kc]] for kc in range(4))) for kr in range(4)]
    return (tent4(*h) * F32(1.0 / 64.0)).astype(F32)


def up(X, R, C):
    def near_far(n, coarse):
        i = np.arange(n)
        near = i >> 1
        return near, np.clip(near + np.where(i & 1, 1, -1), 0, coarse - 1)

    (nr, fr), (nc, fc) = near_far(R, X.shape[0]), near_far(C, X.shape[1])
    h_near = THREE * X[nr][:, nc] + X[nr][:, fc]
    h_far = THREE * X[fr][:, nc] + X[fr][:, fc]
    return ((THREE * h_near + h_far) * F32(1.0 / 16.0)).astype(F32)


def bloom_restated(color, threshold=1.0, knee=0.5, intensity=0.5, levels=5):
    color = np.asarray(color, dtype=F32)
    rows, cols = color.shape[:2]
    with np.errstate(all="ignore"):
        D, S = [], bright(color, threshold, knee)
        for _ in range(levels):
            S = down(S)
            D.append(S)
        U = D[-1]
        for j in range(levels - 2, -1, -1):
            U = D[j] + up(U, *D[j].shape[:2])
        g = F32(intensity) / F32(levels)
        return (color + g * up(U, rows, cols)).astype(F32)
