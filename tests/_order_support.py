"""Shared test support for record ordering: the coherence keys restated in numpy and the sort's size constants."""
import numpy as np


F32 = np.float32


def _cell(t):
    t = np.asarray(t, dtype=F32)
    with np.errstate(invalid="ignore"):
        inside = (t >= 0) & (t < 63)
        return np.where(t >= 63, 63, np.where(inside, np.where(inside, t, 0).astype(np.uint32), 0)).astype(np.uint32)


def _spread(v, step):
    r = np.zeros_like(v)
    for k in range(6):
        r |= ((v >> k) & 1) << (step * k)
    return r


def box_scale(lo, hi):
    lo, hi = np.asarray(lo, dtype=F32), np.asarray(hi, dtype=F32)
    with np.errstate(all="ignore"):
        return np.where(hi > lo, F32(64.0) / (hi - lo), F32(0.0)).astype(F32)


def key_cells(rays, lo, hi):
    """(x, y, z, u, v) of (N, 11) rt_ray words"""
    r = np.ascontiguousarray(rays).view(np.uint32).reshape(-1, 11)
    o, d = r[:, 0:3].view(F32), r[:, 3:6].view(F32)
    lo, scale = np.asarray(lo, dtype=F32), box_scale(lo, hi)
    with np.errstate(all="ignore"):
        xyz = [_cell((o[:, a] - lo[a]) * scale[a]) for a in range(3)]
        dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
        s = (np.abs(dx) + np.abs(dy)) + np.abs(dz)
        px, py = dx / s, dy / s
        sg = lambda x: np.where(x >= 0, F32(1.0), F32(-1.0)).astype(F32)
        fx, fy = (F32(1.0) - np.abs(py)) * sg(px), (F32(1.0) - np.abs(px)) * sg(py)
        fold = dz < 0  # strict: -0.0 and NaN do not fold
        px, py = np.where(fold, fx, px).astype(F32), np.where(fold, fy, py).astype(F32)
        u = _cell((px * F32(0.5) + F32(0.5)) * F32(64.0))
        v = _cell((py * F32(0.5) + F32(0.5)) * F32(64.0))
    return xyz[0], xyz[1], xyz[2], u, v


def numpy_keys(rays, lo, hi, flags=0):
    x, y, z, u, v = key_cells(rays, lo, hi)
    ocode = _spread(x, 3) | (_spread(y, 3) << 1) | (_spread(z, 3) << 2)
    dcode = _spread(u, 2) | (_spread(v, 2) << 1)
    return ((dcode << 18) | ocode if flags & 1 else (ocode << 12) | dcode).astype(np.uint32)


SORT_STEP, SORT_MAX_TILES, SORT_BUCKETS = 2048, 1024, 257  # csrc/rt_order_query.hip RT_SORT_STEP, RT_SORT_MAX_TILES, RT_SORT_BUCKETS


def sort_tile(n):
    """csrc/rt_order_query.hip sort_tile restated: (entries per tile, tiles) for a list of capacity n"""
    tile = -(-n // SORT_MAX_TILES)
    tile = max(-(-tile // SORT_STEP) * SORT_STEP, SORT_STEP)
    return tile, -(-n // tile)


# capacity: (tile, tiles) — the sizes at which the sort takes another path (tests/test_gpu_order_queries.py sorts them)
SORT_LARGE = {1 << 21: (2048, 1024),            # the full bucket table in the scan; still one step per tile
              (1 << 21) + 1: (4096, 513),       # two steps; the last tile holds a single entry
              3 * (1 << 21) + 77: (8192, 769)}  # four steps; a ragged last tile
