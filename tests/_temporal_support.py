"""Shared test support for the temporal queries: the images, the coordinate fields, guide and history data compact and embedded in
records, the numpy float32 restatement of the definition (include/rt_amd.h "temporal queries"), and the bound of the projection test with
its derivation.

The restatement does the definition's f32 operations in the definition's order, element-wise over the image for one tap at a time;
numpy's float32 +, -, *, / and sqrt are IEEE single operations, so it equals the CPU form bit for bit.  tan(fovy / 2) alone is not
numpy's: the library takes it from its own rt_detmath.h, which the oracle exposes (_oracle.math).

THE BOUND OF THE PROJECTION TEST (PROJECTION_BOUND).  Positions are float32 roundings of points on the rays of the 64 x 48 pixel centres of
the reference camera at 16 distances from 0.5 to 50.  The same seven steps are done in binary64 from a binary64 camera basis (np.tan,
np.sqrt) on the same float32 positions, and compared with the float32 restatement.  What separates the two: the basis is rounded to
float32 (relative 2^-24 per operation, about ten operations deep: ~1e-6 relative on clip, times height_f / 2 = 24 pixels of lever),
v = P - origin cancels up to one digit at distance 0.5, the dots and the divide add a few 2^-24 each, and px = clip * 48 + 32 rounds at
ulp(64) / 2 = 3.8e-6.  Measured here on the CPU, binary64 against the float32 restatement: PROJECTION_MEASURED = 1.15e-5 pixels (the
test prints the figures of the run).  The test asserts four times that, PROJECTION_BOUND = 4.6e-5 pixels, for motion_numpy against the
binary64 projection, and for the round trip back to the pixel centre (x, y): there the rounding of the position to float32 comes on
top (2^-24 relative of coordinates up to 50, mostly along the ray, where it does not move the projection); measured 3.05e-5 pixels.
"""
import functools

import numpy as np

import _oracle

F32 = np.float32
IMAGES = [(1, 1), (1, 70), (67, 3), (33, 65)]
PROJECTION_MEASURED = 1.15e-5
PROJECTION_BOUND = 4 * PROJECTION_MEASURED
NAN_WORD = np.uint32(0x7FC00000)
# where primary_surfaces' views lie in the records (words): position and object in rt_hit, normal and valid in rt_surface
HIT_WORDS, SURFACE_WORDS, POSITION_AT, OBJECT_AT, NORMAL_AT, VALID_AT = 13, 18, 3, 2, 14, 17
PARAMS = dict(normal_min=0.6, position_max=0.16, alpha_min=0.125, max_length=4)  # each test rejects a fair share of the case data's taps
HISTORY = np.dtype([("color", "<f4", (3,)), ("moment1", "<f4"), ("moment2", "<f4"), ("length", "<u4"), ("reserved", "<u4", (2,))])


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype != HISTORY else a.view(np.uint32).reshape(-1, 8)


def special_values(cols):
    """coordinates the float tests of step 1 must sort: exactly -1, just below cols, beyond -1, huge, infinite, NaN, -0.0, and the edges"""
    return np.array([-1.0, np.nextafter(F32(cols), F32(0)), -1.5, np.nextafter(F32(-1), F32(-2)), 1e30, np.inf, -np.inf, np.nan, -0.0, float(cols),
                     -0.25, cols - 0.5], dtype=F32)


N_SPECIAL = 12
FIELDS = ["integer", "fractional"] + [f"special{k}" for k in range(N_SPECIAL)]


@functools.lru_cache(maxsize=None)
def motion_field(rows, cols, kind):
    """(rows * cols, 2) float32 (px, py): the pixel's own integer coordinates; those plus offsets in (-1.6, 1.6); or the fractional field
    with special value (i + k) mod 12 in x (even pixels) or y (odd pixels) — every special meets every image, the 1 x 1 one included"""
    g = np.random.default_rng(11 + 1000 * rows + cols)
    r, c = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    m = np.stack([c.reshape(-1), r.reshape(-1)], axis=1).astype(F32)
    if kind != "integer":
        m = (m + (g.random(m.shape, dtype=F32) * F32(3.2) - F32(1.6))).astype(F32)
        m[::5] = np.round(m[::5])  # and some integer coordinates away from the pixel's own
    if kind.startswith("special"):
        k = int(kind[7:])
        i = np.arange(rows * cols)
        sx, sy = special_values(cols), special_values(rows)
        m[i % 2 == 0, 0] = sx[(i[i % 2 == 0] + k) % N_SPECIAL]
        m[i % 2 == 1, 1] = sy[(i[i % 2 == 1] + k) % N_SPECIAL]
    m.setflags(write=False)
    return m


class Planes:
    """the guides of one frame as four arrays (or None)"""

    def __init__(self, normal=None, position=None, object=None, valid=None):
        self.normal, self.position, self.object, self.valid = normal, position, object, valid


@functools.lru_cache(maxsize=None)
def case_data(rows, cols, seed=5):
    """(color, history, current Planes, previous Planes): colours in [0, 2) with one NaN; history records with lengths 0 .. 6, a few NaN
    colours; objects in blocks of 4 x 4, normals from a palette by block plus jitter, positions on a jittered 0.1 grid; about a sixth of
    either frame's valid words cleared.  Shared and left unchanged."""
    g = np.random.default_rng(seed + 1000 * rows + cols)
    n = rows * cols
    r, c = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    r, c = r.reshape(-1), c.reshape(-1)
    color = (g.random((n, 3), dtype=F32) * F32(2.0)).astype(F32)
    color[n // 2, 1] = np.nan
    history = np.zeros(n, dtype=HISTORY)
    history["color"] = g.random((n, 3), dtype=F32) * F32(2.0)
    history["moment1"] = g.random(n, dtype=F32)
    history["moment2"] = g.random(n, dtype=F32) * F32(1.5)
    history["length"] = g.integers(0, 7, n)
    history["color"][n // 3, 2] = np.nan
    history["moment1"][(2 * n) // 3] = np.nan
    palette = np.array([[0, 0, 1], [0, 0.6, 0.8], [0.8, 0, 0.6], [1, 0, 0]], dtype=F32)

    def planes(shift):
        block = ((r + shift) // 4 + c // 4) % 4
        normal = palette[block] + (g.random((n, 3), dtype=F32) * F32(0.3) - F32(0.15))
        normal = (normal / np.sqrt((normal * normal).sum(axis=1, keepdims=True))).astype(F32)
        position = (np.stack([c, r, np.zeros(n)], axis=1).astype(F32) * F32(0.1) + g.random((n, 3), dtype=F32) * F32(0.06)).astype(F32)
        return Planes(normal, position, (block % 3).astype(np.uint32), (g.random(n) >= 1 / 6).astype(np.uint32))

    cur, prev = planes(0), planes(1)
    for a in (color, history, cur.normal, cur.position, cur.object, cur.valid, prev.normal, prev.position, prev.object, prev.valid):
        a.setflags(write=False)
    return color, history, cur, prev


def embed(p):
    """the planes inside (n, 13) and (n, 18) float32 records at primary_surfaces' offsets, the other words a pattern: strided views"""
    n = p.normal.shape[0]
    hits = np.full((n, HIT_WORDS), 123.25, dtype=F32)
    surfaces = np.full((n, SURFACE_WORDS), -7.5, dtype=F32)
    hits[:, POSITION_AT:POSITION_AT + 3] = p.position
    hits.view(np.uint32)[:, OBJECT_AT] = p.object
    surfaces[:, NORMAL_AT:NORMAL_AT + 3] = p.normal
    surfaces.view(np.uint32)[:, VALID_AT] = p.valid
    return hits, surfaces, record_views(hits, surfaces)


def record_views(hits, surfaces):
    return Planes(surfaces[:, NORMAL_AT:NORMAL_AT + 3], hits[:, POSITION_AT:POSITION_AT + 3], hits.view(np.uint32)[:, OBJECT_AT],
                  surfaces.view(np.uint32)[:, VALID_AT])


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def luminance(c):
    return (F32(0.2126) * c[..., 0] + F32(0.7152) * c[..., 1]) + F32(0.0722) * c[..., 2]


def floor_f32(x):
    """the definition's floor: the truncation, less one where it lies above x"""
    t = np.trunc(x).astype(np.int64).astype(F32)
    return np.where(t > x, t - F32(1), t).astype(F32)


def _plane(a, n, width):
    return None if a is None else np.array(a).reshape(n, width) if width > 1 else np.array(a).reshape(n)


def restate_accumulate(color, motion, rows, cols, history, cur=None, prev=None, normal_min=0.9, position_max=0.1, alpha_min=0.05, max_length=32):
    """steps 1 to 5 of the definition -> (history_out (n,) HISTORY, variance (n,) float32)"""
    cur, prev = cur or Planes(), prev or Planes()
    n = rows * cols
    C = np.array(color, dtype=F32).reshape(n, 3)
    L = luminance(C)
    px, py = np.array(motion, dtype=F32).reshape(n, 2).T
    h = np.array(history).reshape(n)
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
                b = ((wx if i else F32(1) - wx) * (wy if j else F32(1) - wy)).astype(F32)
                x, y = x0 + i, y0 + j
                take = gather & (b > 0) & (x >= 0) & (x < cols) & (y >= 0) & (y < rows)
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
                total = np.where(take[:, None], total + b[:, None] * hq["color"], total)
                s1 = np.where(take, s1 + b * hq["moment1"], s1)
                s2 = np.where(take, s2 + b * hq["moment2"], s2)
                bsum = np.where(take, bsum + b, bsum)
                least = np.where(take, np.minimum(least, hq["length"].astype(np.uint64)), least)
        blend = bsum > 0
        length = np.where(least >= max_length, max_length, least + 1).astype(np.uint32)
        inv = F32(1) / length.astype(F32)
        alpha = np.where(inv > F32(alpha_min), inv, F32(alpha_min)).astype(F32)
        keep = F32(1) - alpha
        safe = np.where(blend, bsum, F32(1))
        out = np.zeros(n, dtype=HISTORY)
        oc = (total / safe[:, None]) * keep[:, None] + C * alpha[:, None]
        m1 = (s1 / safe) * keep + L * alpha
        m2 = (s2 / safe) * keep + (L * L) * alpha
        out["color"].view(np.uint32)[:] = np.where(blend[:, None], oc.astype(F32).view(np.uint32), C.view(np.uint32))
        out["moment1"] = np.where(blend, m1, L)
        out["moment2"] = np.where(blend, m2, L * L)
        out["length"] = np.where(blend, length, 1)
        v = out["moment2"] - out["moment1"] * out["moment1"]
        variance = np.where(blend & (v > 0), v, F32(0)).astype(F32)
    return out, variance


def camera_basis(camera, frame, dtype=F32):
    """make_kernel_frame's basis in `dtype`: float32 with the library's own tangent (bit-identical), or binary64 with np.tan"""
    T = dtype
    v = lambda a: np.array(list(a), dtype=T)
    norm = lambda a: a * (T(1) / np.sqrt(dot(a, a)))
    toward = norm(v(camera.toward))
    right = norm(np.cross(toward, v(camera.up)).astype(T)) if T is np.float64 else norm(cross_f32(toward, v(camera.up)))
    up = norm(np.cross(right, toward).astype(T)) if T is np.float64 else norm(cross_f32(right, toward))
    half = T(camera.fovy) / T(2)
    th = T(np.tan(half)) if T is np.float64 else _oracle.math("tan", np.array([half], dtype=F32))[0]
    return dict(origin=v(camera.center) + toward * T(camera.near), x=th * right, y=th * up, toward=toward,
                half_width=T(frame.width) / T(2), half_height=T(frame.height) / T(2), height_f=T(frame.height))


def cross_f32(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], dtype=F32)


def restate_motion(position, camera, frame, valid=None, dtype=F32):
    """the seven steps -> (n, 2) in `dtype`; NaN where invalid or z > 0 is false"""
    T = dtype
    k = camera_basis(camera, frame, T)
    n = frame.width * frame.height
    P = np.array(position).reshape(n, 3).astype(T)
    with np.errstate(all="ignore"):
        v = P - k["origin"]
        z = dot(v, k["toward"])
        tt = dot(k["x"], k["x"])
        zt = z * tt
        clip_x = dot(v, k["x"]) / zt
        clip_y = dot(v, k["y"]) / zt
        px = clip_x * k["height_f"] + k["half_width"]
        py = k["half_height"] - clip_y * k["height_f"]
    ok = z > 0
    if valid is not None:
        ok &= np.array(valid).reshape(n) != 0
    out = np.stack([px, py], axis=1).astype(T)
    if T is F32:
        out.view(np.uint32)[~ok] = NAN_WORD
    else:
        out[~ok] = np.nan
    return out


def pixel_positions(camera, frame, distances):
    """float32 points on the ray of every pixel centre (x, y) of the full frame — primary_ray_through restated in binary64 — at
    distances[i mod len]: (n, 3) float32"""
    k = camera_basis(camera, frame, np.float64)
    y, x = np.meshgrid(np.arange(frame.height, dtype=np.float64), np.arange(frame.width, dtype=np.float64), indexing="ij")
    clip_y = (k["half_height"] - y.reshape(-1)) / k["height_f"]
    clip_x = (x.reshape(-1) - k["half_width"]) / k["height_f"]
    d = clip_x[:, None] * k["x"] + clip_y[:, None] * k["y"] + k["toward"]
    d /= np.sqrt((d * d).sum(axis=1, keepdims=True))
    t = np.asarray(distances, dtype=np.float64)[np.arange(d.shape[0]) % len(distances)]
    return (k["origin"] + d * t[:, None]).astype(F32)
