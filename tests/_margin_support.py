"""Shared test support for the shortcuts that skip work of a certain outcome (csrc/rt_device_scene.h bq / q_miss, csrc/rt_shade.h
cos_in / cos_out and pow_underflows_to_zero): what rt_scene_describe_filters says they were given, binary32 restatements of their
compares in the device's operation order (csrc/rt_vec.h: no FMA, dot summed x, y, z), and generators of inputs that sit at the
margins.  Every generator returns a label per case and asserts its own coverage: one that cannot fill a bucket fails."""
import ctypes as C

import numpy as np

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import _capi
from homework_18_graphics_raytracer_amd._capi import Light, Material, SceneDesc, Sphere

F32 = np.float32
EPS = F32(1.1920928955078125e-7)  # std::f32::EPSILON
INF = F32(np.inf)


# ---- what the shortcuts were given ----


def describe_filters(desc):
    """rt_scene_describe_filters (host only): (tri (T, 4) f32: bcx bcy bcz bq, q_miss (S,) f32, light (L, 2) f32: cos_in cos_out,
    filter_origin2 as an f32)"""
    tri = np.zeros((desc.n_triangles, 4), dtype=F32)
    sph = np.zeros(desc.n_spheres, dtype=F32)
    lights = np.zeros((desc.n_lights, 2), dtype=F32)
    o2 = C.c_float(0.0)
    p = lambda a: C.c_void_p(a.ctypes.data) if a.size else None
    _capi.check(_capi.amd_lib().rt_scene_describe_filters(C.byref(desc), p(tri), p(sph), p(lights), C.byref(o2)))
    return tri, sph, lights, F32(o2.value)


def plain_material():
    m = Material()
    m.diffuse_fn = m.normal_fn = 0
    m.normal = (0.0, 0.0, 1.0)
    m.diffuse_color = (0.8, 0.7, 0.6)
    m.specular_color = (0.5, 0.5, 0.5)
    m.shiness, m.smoothness, m.transparency, m.refraction_index, m.opaque_decay = 0.3, 0.2, 0.0, 1.0, 0.0
    return m


def spheres_desc(radii):
    """a scene of nothing but one sphere per radius, at the origin"""
    arr = (Sphere * len(radii))()
    for k, r in enumerate(np.asarray(radii, dtype=F32)):
        arr[k].object_index = 0
        arr[k].center = (0.0, 0.0, 0.0)
        arr[k].radius = r
    mats = (Material * 1)(plain_material())
    d = SceneDesc(None, 0, arr, len(radii), mats, 1, None, 0)
    d._keepalive = (arr, mats)
    return d


def spot(angle, origin=(0.0, 0.0, 0.0), direction=(0.0, -1.0, 0.0), softness=1.0):
    l = Light()
    l.kind, l.has_origin = 1, 1
    l.origin = tuple(float(v) for v in origin)
    l.direction = tuple(float(v) for v in direction)
    l.angle = F32(angle)
    l.softness = softness
    l.color = (1.0, 0.9, 0.8)
    return l


def lights_desc(lights):
    arr = (Light * len(lights))(*lights)
    mats = (Material * 1)(plain_material())
    d = SceneDesc(None, 0, None, 0, mats, 1, arr, len(lights))
    d._keepalive = (arr, mats)
    return d


# ---- binary32 by hand ----


def steps(x, k):
    """x moved by k binary32 steps towards +inf (k < 0: towards -inf), through zero; x finite"""
    i = np.asarray(x, dtype=F32).view(np.int32).astype(np.int64)
    s = np.where(i < 0, -(i & 0x7FFFFFFF), i) + np.asarray(k, dtype=np.int64)
    back = np.where(s < 0, (-s) | 0x80000000, s).astype(np.uint32)
    return back.view(F32)


def steps_between(a, b):
    """the number of binary32 steps from a up to b"""
    o = lambda v: (lambda i: np.where(i < 0, -(i & 0x7FFFFFFF), i))(np.asarray(v, dtype=F32).view(np.int32).astype(np.int64))
    return o(b) - o(a)


def dot32(a, b):
    """csrc/rt_vec.h dot: (a.x * b.x + a.y * b.y) + a.z * b.z, every operation rounded to binary32"""
    a, b = np.asarray(a, dtype=F32), np.asarray(b, dtype=F32)
    with np.errstate(all="ignore"):
        return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross32(a, b):
    a, b = np.asarray(a, dtype=F32), np.asarray(b, dtype=F32)
    with np.errstate(all="ignore"):
        return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                         a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def magnitude32(a):
    with np.errstate(all="ignore"):
        return np.sqrt(dot32(a, a))


def normalize32(a):
    a = np.asarray(a, dtype=F32)
    with np.errstate(all="ignore"):
        return a * (F32(1.0) / magnitude32(a))[..., None]


def math_host(op, x, y=None):
    """rt_math_eval_host: the product's own rtdm:: functions on the CPU (3 acos, 5 pow)"""
    x = np.ascontiguousarray(x, dtype=F32)
    y = np.zeros_like(x) if y is None else np.ascontiguousarray(y, dtype=F32)
    out = np.empty_like(x)
    _capi.check(_capi.amd_lib().rt_math_eval_host(op, x.ctypes.data, y.ctypes.data, out.ctypes.data, x.size))
    return out


ACOS, POW = 3, 5


def pow_skipped(x, y):
    """csrc/rt_shade.h pow_underflows_to_zero in binary32: one multiply and one subtract"""
    x, y = np.asarray(x, dtype=F32), np.asarray(y, dtype=F32)
    with np.errstate(all="ignore"):
        return (x >= F32(0.0)) & (x < F32(1.0)) & (y > F32(0.0)) & (y <= F32(3.0e38)) & ((x == F32(0.0)) | (y * (x - F32(1.0)) < F32(-111.0)))


SMOOTHNESS = (0.0, 1e-38, 1e-7, 1e-5, 0.01, 0.2, 1.0)


def phong_exponents():
    """get_specular's 1 / (smoothness + EPSILON) for the smoothness values above, then the predicate's own upper bound for y, the next
    binary32 above it and +inf"""
    with np.errstate(all="ignore"):
        ys = [F32(1.0) / (F32(s) + EPS) for s in SMOOTHNESS]
    return ys + [F32(3.0e38), steps(F32(3.0e38), 1)[()], INF]


def threshold_base(y):
    """the binary32 x nearest to 1 - 111 / y: where y (x - 1) crosses -111"""
    with np.errstate(all="ignore"):
        return F32(1.0 - 111.0 / float(y)) if float(y) > 0.0 else F32(1.0)


# ---- crafted inputs: the per-triangle bounding-sphere rejection ----

GRID = 2.0 ** -10
# name, the shape in its plane in units of 2^-10, does the triangle get the rejection (rt_api_layout.hip: an angle of at least 0.0201 rad, a
# radius within [1e-3, 0.5] of the extent 4), how far a copy is shifted in the plane (units)
SHAPES = (
    ("equilateral", ((0, 0), (1024, 0), (512, 887)), True, 16),
    ("right", ((0, 0), (1024, 0), (0, 768)), True, 16),                  # squared sides 1, 0.5625 and their exact sum
    ("obtuse150", ((0, 0), (1024, 0), (-887, 512)), True, 16),
    ("sliver0.0200", ((0, 0), (3950, 0), (3950, 79)), False, 16),        # atan(79 / 3950) = 0.019997
    ("sliver0.0202", ((0, 0), (3960, 0), (3960, 80)), True, 16),         # atan(80 / 3960) = 0.020199
    ("radius0.00098", ((0, 0), (8, 0), (0, 1)), False, 1),               # half the hypotenuse sqrt(65) / 2048 = 0.000984 x 4
    ("radius0.00101", ((0, 0), (8, 0), (0, 2)), True, 1),                # sqrt(68) / 2048 = 0.0010066 x 4
    ("radius0.499", ((-1445, -1445), (1445, -1445), (-1445, 1445)), True, 16),   # 2890 sqrt(2) / 2048 = 0.49891 x 4
    ("radius0.501", ((-1451, -1451), (1451, -1451), (-1451, 1451)), False, 16),  # 2902 sqrt(2) / 2048 = 0.50098 x 4
)
COPIES = 12
CLUSTERED = ("equilateral", "right", "obtuse150", "radius0.00101")


class RejectionWorld:
    """.world, .desc; per triangle: .shape (index into SHAPES, -1 the anchor), .lone, .axis (the plane's normal axis), .tris (T, 3, 3) f64"""


def rejection_world(scale=1.0):
    """Extent 4 (times `scale`): per shape class one object of 12 index-adjacent copies (turned by quarter turns about the plane normal,
    shifted in the plane and stacked 2^-5 apart: a clustered leaf where all 12 get the rejection) and one lone copy in an object of its
    own between other classes' objects (a plain leaf), then a triangle with a vertex at (4, 4, 4) that fixes the extent.  scale == 1:
    every coordinate is a multiple of 2^-10."""
    r = RejectionWorld()
    r.world = rt.World()
    shape, lone, axis, tris = [], [], [], []

    def embed(uv, h, a):
        p = np.zeros((3, 3))
        p[:, a], p[:, (a + 1) % 3], p[:, (a + 2) % 3] = h, uv[:, 0], uv[:, 1]
        return p * GRID * scale

    def copy_of(ci, k, h):
        uv = np.array(SHAPES[ci][1], dtype=np.float64)
        for _ in range(k % 4):
            uv = np.stack([-uv[:, 1], uv[:, 0]], axis=1)
        g = SHAPES[ci][3]
        return embed(uv + np.array([(k % 3 - 1) * g, ((k // 3) % 3 - 1) * g]), h, ci % 3)

    def push(obj, p, ci, is_lone):
        obj.push_flat_triangle(p.tolist(), [(0.0, 0.0), (1.0, 0.0), (0.0, 1.0)])
        shape.append(ci); lone.append(is_lone); axis.append(ci % 3 if ci >= 0 else -1); tris.append(p)

    n = len(SHAPES)
    for ci in range(n):
        obj = r.world.push_object(plain_material())
        base = -3072 + 640 * ci
        for k in range(COPIES):
            push(obj, copy_of(ci, k, base + 32 * k), ci, False)
        other = (ci + 4) % n
        push(r.world.push_object(plain_material()), copy_of(other, 5, -3072 + 640 * other + 480), other, True)
    push(r.world.push_object(plain_material()), np.array([[4.0, 4.0, 4.0], [4.0, 3.5, 4.0], [3.5, 4.0, 4.0]]) * scale, -1, True)
    sun = Light()
    sun.kind, sun.direction, sun.color = 0, (0.3, -0.8, 0.5), (1.0, 0.9, 0.8)
    r.world.push_light(sun)
    lamp = Light()
    lamp.kind, lamp.has_origin, lamp.origin, lamp.color = 2, 1, (0.5 * scale, 3.0 * scale, -1.0 * scale), (0.6, 0.6, 0.9)
    r.world.push_light(lamp)
    r.desc = r.world.desc()
    r.shape, r.lone, r.axis, r.tris = np.array(shape), np.array(lone), np.array(axis), np.array(tris)
    r.filters = describe_filters(r.desc)
    assert r.desc.n_triangles == r.tris.shape[0] <= 200
    if scale == 1.0:
        assert np.array_equal(r.tris, np.round(r.tris / GRID) * GRID) and r.filters[3] == F32(256.0)
        on = np.isfinite(r.filters[0][:, 3])
        for ci, (name, _, expect, _) in enumerate(SHAPES):  # which classes carry a finite bq: every copy, or none
            assert (on[r.shape == ci] == expect).all(), (name, on[r.shape == ci])
        # which walk meets them: the 12 copies of a class in CLUSTERED are one clustered leaf with a pair-wise dealing; the stacks of the
        # 0.0202 sliver and of the 0.499 radius get the rejection but no node (their common sphere exceeds half the extent: node_stats),
        # so they and every lone copy lie in plain leaves, which the wave-uniform loop visits
        from _scenes import nodes_of
        nodes = nodes_of(r.desc)
        leaf = np.full(r.tris.shape[0], -1)
        for k, (first, count, *_rest) in enumerate(nodes):
            leaf[first:first + count] = k
        assert (leaf >= 0).all()
        for ci, (name, _, expect, _) in enumerate(SHAPES):
            stack = np.flatnonzero((r.shape == ci) & ~r.lone)
            rows = nodes[np.unique(leaf[stack])]
            if name in CLUSTERED:
                assert rows.shape[0] == 1 and rows[0, 0] == stack[0] and rows[0, 1] == COPIES and rows[0, 2] != 0 and rows[0, 4] != 0, (name, rows)
            else:
                assert (rows[:, 2] == 0).all(), (name, rows)
        assert (nodes[leaf[r.lone], 2] == 0).all()
    return r


def plane_of(tris):
    """n and d of every triangle as rt_api_layout.hip makes them, in binary32"""
    v = np.asarray(tris, dtype=F32)
    n = normalize32(cross32(v[:, 1] - v[:, 0], v[:, 2] - v[:, 1]))
    return n, dot32(n, v[:, 0])


def restate_rejection(n, d_plane, bc, bq, o, d, origin2):
    """the compares of the three walkers for one (ray, triangle) pair per row (rt_cast.h cast_pairs: `hb.w < q && 1.0e30f > q &&
    filter_ok`): (q, q > bq, dot(o, o) <= filter_origin2)"""
    with np.errstate(all="ignore"):
        t = (d_plane - dot32(n, o)) / dot32(n, d)
        p = o + d * t[:, None]
        w = p - bc
        q = (w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2]
        return q, q > bq, dot32(o, o) <= origin2


INCIDENCE = (1.0, 0.1, 2e-3)
LENGTHS = (1.0, 0.3, 2.5)
ORIGINS = ("0.1 x extent away", "inside 4 x extent", "outside 4 x extent", "100 x extent away")


class Cases:
    """.rays (N, 11) uint32 rt_ray records, .labels, one per case, and what the generator restated"""


def rejection_rays(rw, seed=30):
    """For every triangle with a finite bq, rays through in-plane targets — each vertex and each edge midpoint moved in and out by
    R 2^-k (k = 6, 10, 14, 18, 22), every edge extended beyond both ends by 0.01 R, R, 10 R and 100 R, eight points on each of the circles
    |p - bc|^2 = bq (1 -+ 2^-20) — from four origins each (ORIGINS; the middle two at |o|^2 = filter_origin2 (1 -+ 2^-20)), the incidence
    |n.d| / |d|, the length |d| and the face mode taking turns through all 27 combinations.  The circle targets are met head-on
    (incidence 1: the plane point is the target's own binary32 coordinates, so the restated |p - bc|^2 stays within 2^-18 of bq)."""
    g = np.random.default_rng(seed)
    tri4, _, _, origin2 = rw.filters
    extent = 4.0
    n32, d32 = plane_of(rw.tris)
    o_all, d_all, mode_all, tri_all, labels = [], [], [], [], []
    turn = 0
    for i in np.flatnonzero(np.isfinite(tri4[:, 3])):
        v = rw.tris[i]
        nrm = n32[i].astype(np.float64)
        bc, bq = tri4[i, :3].astype(np.float64), float(tri4[i, 3])
        radius = np.sqrt(bq / (1.05 * 1.0001))
        unit = lambda a: a / np.linalg.norm(a)
        targets = []
        for a in range(3):
            A, B, Cc = v[a], v[(a + 1) % 3], v[(a + 2) % 3]
            bis, mid, out = unit(unit(B - A) + unit(Cc - A)), 0.5 * (A + B), unit(np.cross(B - A, nrm))
            for k in (6, 10, 14, 18, 22):
                for s in (1.0, -1.0):
                    targets.append((f"vertex {a} {'+' if s > 0 else '-'} R 2^-{k}", A + s * radius * 2.0 ** -k * bis, None))
                    targets.append((f"midpoint {a} {'+' if s > 0 else '-'} R 2^-{k}", mid + s * radius * 2.0 ** -k * out, None))
            for f in (0.01, 1.0, 10.0, 100.0):
                targets.append((f"edge {a} beyond its end by {f} R", B + f * radius * unit(B - A), None))
                targets.append((f"edge {a} before its start by {f} R", A - f * radius * unit(B - A), None))
        eu, ev = unit(v[1] - v[0]), unit(np.cross(nrm, v[1] - v[0]))
        for s in (-1.0, 1.0):
            for j in range(8):
                th = (j + 0.5) * np.pi / 4 + 0.1
                rho = np.sqrt(bq * (1.0 + s * 2.0 ** -20))
                targets.append((f"circle bq (1 {'+' if s > 0 else '-'} 2^-20) point {j}", bc + rho * (np.cos(th) * eu + np.sin(th) * ev), 0))
        for name, P, fixed in targets:
            for oi, oname in enumerate(ORIGINS):
                inc = INCIDENCE[turn % 3 if fixed is None else fixed]
                length, mode = LENGTHS[(turn // 3) % 3], (turn // 9) % 3
                turn += 1
                side = 1.0 if (turn // 27) % 2 else -1.0
                phi = g.uniform(0, 2 * np.pi)
                along = -side * inc * nrm + (np.sqrt(1.0 - inc * inc) * (np.cos(phi) * eu + np.sin(phi) * ev) if inc < 1.0 else 0.0)
                if oi == 0:
                    L = 0.1 * extent
                elif oi == 3:
                    L = 100.0 * extent
                else:  # |P - L along|^2 = filter_origin2 (1 -+ 2^-20): the positive root
                    want = float(origin2) * (1.0 + (-1.0 if oi == 1 else 1.0) * 2.0 ** -20)
                    b, c = np.dot(P, along), np.dot(P, P) - want
                    L = b + np.sqrt(max(b * b - c, 0.0))  # a target far outside that sphere: the origin nearest to it
                o_all.append(P - L * along); d_all.append(along * length); mode_all.append(mode); tri_all.append(i)
                cls = SHAPES[rw.shape[i]][0] if rw.shape[i] >= 0 else "anchor"
                labels.append(f"triangle {i} ({cls}{', lone' if rw.lone[i] else ''}): {name}; origin {oname}; incidence {inc}; |d| {length}; face {mode}")
    c = Cases()
    o, d, c.tri = np.array(o_all).astype(F32), np.array(d_all).astype(F32), np.array(tri_all)
    c.rays = np.zeros((o.shape[0], 11), dtype=np.uint32)
    c.rays[:, 0:3], c.rays[:, 3:6], c.rays[:, 6] = o.view(np.uint32), d.view(np.uint32), mode_all
    c.labels = labels
    c.q, c.beyond, c.filter_ok = restate_rejection(n32[c.tri], d32[c.tri], tri4[c.tri, :3], tri4[c.tri, 3], o, d, origin2)
    c.bq = tri4[c.tri, 3]
    with np.errstate(all="ignore"):
        c.close = np.abs(c.q.astype(np.float64) / c.bq.astype(np.float64) - 1.0) <= 2.0 ** -18
    # coverage: per shape class with the rejection and per origin class as the walkers see it (may the ray use the rejection at all), the
    # compare comes out either way at least 64 times, and either way at least 64 times within 2^-18 of bq
    c.counts = {}
    for ci, (name, _, expect, _) in enumerate(SHAPES):
        if not expect:
            continue
        of_class = rw.shape[c.tri] == ci
        for ok in (True, False):
            for beyond in (True, False):
                rows = of_class & (c.filter_ok == ok) & (c.beyond == beyond)
                key = (name, "near origin" if ok else "far origin", "q > bq" if beyond else "q <= bq")
                c.counts[key] = (int(rows.sum()), int((rows & c.close).sum()))
                assert rows.sum() >= 64 and (rows & c.close).sum() >= 64, (key, c.counts[key])
                assert set(c.rays[rows & c.close, 6]) == {0, 1, 2} and len(set(np.round(magnitude32(d[rows & c.close]), 3))) == 3, key
    # the two origins at 4 x extent come out on both sides of the compare with filter_origin2, within 2^-18 of it
    o2 = dot32(o, o).astype(np.float64) / float(origin2)
    edge = np.abs(o2 - 1.0) <= 2.0 ** -18
    assert (edge & c.filter_ok).sum() >= 64 and (edge & ~c.filter_ok).sum() >= 64
    return c


def scaled_batch(cases, scale, n=2048):
    """the first n rays of a batch for the world scaled by `scale`: origins scaled, directions kept"""
    rays = cases.rays[:n].copy()
    rays[:, 0:3] = (rays[:, 0:3].view(F32).astype(np.float64) * scale).astype(F32).view(np.uint32)
    return rays


# ---- crafted inputs: rays tangent to spheres ----

# the first four only have to come out as the oracle has them (q_miss is +inf for each: the root always decides); they come first in the
# sphere array so that what they make of a ray — a NaN or infinite distance — is replaced by any hit of the three that follow
ODD_RADII = (np.nan, -1.0, 0.0, 3e19)
TANGENT_RADII = (1e-30, 2.0 ** -20, 0.35)
BUCKETS = ("q < r2", "q == r2", "r2 < q <= q_miss", "q > q_miss by at most 8 steps", "q far above q_miss")


def tangent_world():
    w = rt.World()
    centres = [(0.5, 0.25, -1.0), (-0.75, 0.5, 0.25), (1.0, -0.5, 0.5), (0.25, 0.25, 0.25), (2.0 ** -12, 0.0, 2.0 ** -13), (0.0, 0.0, 0.0), (1.5, 0.75, -0.5)]
    for c, r in zip(centres, ODD_RADII + TANGENT_RADII):
        w.push_object(plain_material()).push_sphere(c, float(r))
    sun = Light()
    sun.kind, sun.direction, sun.color = 0, (0.3, -0.8, 0.5), (1.0, 0.9, 0.8)
    w.push_light(sun)
    return w, np.array(centres, dtype=np.float64)


def tangent_rays(world, centres, seed=31, per_bucket=128):
    """Rays whose line passes a sphere at lsd = radius (1 + k 2^-24) / |d| for small k, many more than needed; the restated
    q = |cross(c - o, d)|^2 (rt_cast.h cast_finish) puts each into a bucket and the first per_bucket of each bucket are kept, the face
    modes and |d| = 1, 0.3, 2.5 taking turns.  Radii 0.35 and 2^-20 fill all five buckets; for 1e-30 the square underflows to r2 = 0 and
    q_miss is the smallest subnormal: q, a sum of squares, is never below r2, and the other four buckets are filled with rays built for
    them (q == 0, q == 2^-149, the next eight subnormals, far above).
    The batch: whole waves of 64 from `q > q_miss by at most 8 steps` alone (the skip is taken), the same with one lane from another bucket,
    then everything else shuffled."""
    g = np.random.default_rng(seed)
    desc = world.desc()
    q_miss = describe_filters(desc)[1]
    assert np.isinf(q_miss[:len(ODD_RADII)]).all() and np.isfinite(q_miss[len(ODD_RADII):]).all()
    picked = {}
    for si, radius in enumerate(TANGENT_RADII, start=len(ODD_RADII)):
        n = 60000
        c = centres[si]
        r32 = F32(radius)
        with np.errstate(all="ignore"):
            r2 = r32 * r32
        length = np.array(LENGTHS)[np.arange(n) % 3]
        k = g.integers(-24, 25, n)
        k[n // 2:] = g.integers(-4000000, 4000000, n - n // 2)  # the far half: up to a quarter of the radius off
        dirs = g.normal(size=(n, 3))
        dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
        side = np.cross(dirs, g.normal(size=(n, 3)))
        side /= np.linalg.norm(side, axis=1, keepdims=True)
        rho = float(r32) * (1.0 + k * 2.0 ** -24) / length
        if radius < 2.0 ** -20:  # a quarter of this radius off squares to zero all the same: anywhere from 1e-20 to 1e-3 off instead
            rho[n // 2:] = 10.0 ** g.uniform(-20.0, -3.0, n - n // 2)
        back = float(r32) * g.uniform(2.0, 6.0, n) if radius < 0.1 else g.uniform(0.5, 3.0, n)
        o = (c + rho[:, None] * side - back[:, None] * dirs).astype(F32)
        d = (dirs * length[:, None]).astype(F32)
        with np.errstate(all="ignore"):
            cr = cross32(np.asarray(c, dtype=F32) - o, d)
            q = dot32(cr, cr)
        qm = q_miss[si]
        above = steps_between(np.full(n, qm, dtype=F32), q)
        bucket = np.where(q < r2, 0, np.where(q == r2, 1, np.where(q <= qm, 2, np.where(above <= 8, 3, 4))))
        for b in range(5):
            rows = np.flatnonzero(bucket == b)
            needed = radius >= 2.0 ** -20 or b != 0  # r2 = 0 and q is a sum of squares: never below it
            if radius < 2.0 ** -20 and b in (1, 2, 3):
                # q is then one of the first subnormals: d along x or z and the origin beside the line through the centre by y0 alone
                # (centre.y == 0, so c.y - o.y is y0 exactly) leave the cross product the single component y0 |d|, whose square
                # rounds to m 2^-149: m = 0 (the line through the centre), m = 1 (q == q_miss), m = 2 .. 9 (up to 8 steps above)
                rows = np.arange(per_bucket)
                m = np.zeros(per_bucket) if b == 1 else g.uniform(0.6, 1.4, per_bucket) if b == 2 else g.uniform(1.6, 9.4, per_bucket)
                ax = np.where((rows // 2) % 2, 0, 2)
                d[rows] = 0.0
                d[rows, ax] = length[rows].astype(F32) * np.where(rows % 2, 1, -1)
                o[rows] = np.asarray(c, dtype=F32)
                o[rows, ax] -= (d[rows, ax] * F32(4.0)).astype(F32)
                o[rows, 1] = (np.sqrt(m * 2.0 ** -149) / length[rows] * np.where((rows // 4) % 2, 1, -1)).astype(F32)
                with np.errstate(all="ignore"):
                    cr = cross32(np.asarray(c, dtype=F32) - o[rows], d[rows])
                    qb = dot32(cr, cr)
                assert c[1] == 0.0 and (np.where(qb == r2, 1, np.where(qb <= qm, 2, np.where(steps_between(np.full(per_bucket, qm, dtype=F32), qb) <= 8, 3, 4))) == b).all()
            assert not needed or rows.size >= per_bucket, (radius, BUCKETS[b], rows.size)
            rows = rows[:per_bucket]
            mode = (np.arange(rows.size) // 3) % 3
            assert rows.size < 9 or (len(set(mode)) == 3 and len(set(np.round(np.linalg.norm(d[rows], axis=1), 3))) == 3) or not needed
            picked[(si, b)] = (o[rows].copy(), d[rows].copy(), mode)
    # the batch
    o_all, d_all, m_all, labels = [], [], [], []

    def put(si, b, j):
        o, d, mode = picked[(si, b)]
        j = j % o.shape[0]
        o_all.append(o[j]); d_all.append(d[j]); m_all.append(mode[j])
        labels.append(f"sphere {si} radius {(ODD_RADII + TANGENT_RADII)[si]}: {BUCKETS[b]}, ray {j}")

    for si in (4, 5, 6):
        for j in range(128):  # two whole waves just above q_miss
            put(si, 3, j)
        for wave, b in enumerate((0, 1, 2, 2) if si != 4 else (1, 1, 2, 2)):  # four waves with exactly one lane from another bucket
            for lane in range(64):
                put(si, b if lane == (17 * wave + 5) % 64 else 3, 64 * wave + lane)
    rest = [(si, b, j) for (si, b), v in picked.items() for j in range(v[0].shape[0])]
    for idx in g.permutation(len(rest)):
        put(*rest[idx])
    c = Cases()
    o, d = np.array(o_all, dtype=F32), np.array(d_all, dtype=F32)
    c.rays = np.zeros((o.shape[0], 11), dtype=np.uint32)
    c.rays[:, 0:3], c.rays[:, 3:6], c.rays[:, 6] = o.view(np.uint32), d.view(np.uint32), m_all
    c.labels = labels
    c.counts = {(TANGENT_RADII[si - len(ODD_RADII)], BUCKETS[b]): v[0].shape[0] for (si, b), v in picked.items()}
    assert c.rays.shape[0] <= 8192
    return c


# ---- crafted inputs: Phong highlights at the underflow ----


def highlight_cases(seed=32):
    """Surface records (18 words, a constant material) with the smoothness values above, normal (0, 0, 1), the light along the normal and
    the view (sqrt(1 - z^2), 0, z), so that get_specular's rv is z exactly: z over the 256 binary32 neighbours on each side of 1 - 111 / y,
    and over 64 on each side of exp(-110 / y) and exp(-103.97 / y), where powf itself cuts and where the power really underflows.
    Returns (surfaces (N, 18) uint32, view (N, 3), light_dirs (1, N, 3), labels, skipped): whole waves in which pow_underflows_to_zero holds
    for all 64 lanes, waves with one lane for which it does not, then everything shuffled."""
    g = np.random.default_rng(seed)
    zs, ss, names = [], [], []
    for s in SMOOTHNESS:
        with np.errstate(all="ignore"):
            y = F32(1.0) / (F32(s) + EPS)
        for what, base, reach in (("1 - 111 / y", threshold_base(y), 256), ("exp(-110 / y)", F32(np.exp(-110.0 / float(y))), 64),
                                  ("exp(-103.97 / y)", F32(np.exp(-103.97 / float(y))), 64)):
            z = steps(base, np.arange(-reach, reach + 1))
            z = z[(z >= F32(-1.0)) & (z <= F32(1.0))]
            zs.append(z); ss.append(np.full(z.shape, s, dtype=F32))
            names += [f"smoothness {s}: z = {what} {int(k):+d} steps" for k in steps_between(base, z)]
    z, s = np.concatenate(zs), np.concatenate(ss)
    with np.errstate(all="ignore"):
        y = F32(1.0) / (s + EPS)
    skipped = pow_skipped(np.maximum(z, F32(0.0)), y)
    t, f = np.flatnonzero(skipped), np.flatnonzero(~skipped)
    near = np.abs(steps_between(np.array([threshold_base(v) for v in y]), z)) <= 256
    assert (skipped & near).sum() >= 512 and (~skipped & near).sum() >= 512
    # nearest to the threshold first: the whole-wave skip is taken at the margin itself
    t_near = t[np.argsort(np.abs(steps_between(np.array([threshold_base(v) for v in y[t]]), z[t])), kind="stable")]
    order = list(t_near[:256])
    for wave in range(4):
        lanes = list(t_near[256 + 63 * wave:256 + 63 * (wave + 1)])
        lanes.insert((19 * wave + 3) % 64, f[(97 * wave) % f.size])
        order += lanes
    order += list(g.permutation(z.size))
    order = np.array(order)
    assert skipped[order[:256]].all() and all((~skipped[order[256 + 64 * w:320 + 64 * w]]).sum() == 1 for w in range(4))
    z, s = z[order], s[order]
    n = z.size
    surf = np.zeros((n, 18), dtype=np.uint32)
    fl = np.zeros((n, 17), dtype=F32)
    fl[:, 2] = 1.0                      # the material's normal
    fl[:, 3:6] = (0.8, 0.7, 0.6)        # diffuse
    fl[:, 6] = 0.3                      # shiness
    fl[:, 7:10] = (0.5, 0.25, 1.0)      # specular colour
    fl[:, 10] = s
    fl[:, 12] = 1.0
    fl[:, 16] = 1.0                     # shading normal (0, 0, 1)
    surf[:, :17], surf[:, 17] = fl.view(np.uint32), 1
    with np.errstate(all="ignore"):
        view = np.stack([np.sqrt(F32(1.0) - z * z), np.zeros(n, dtype=F32), z], axis=1).astype(F32)
    dirs = np.tile(np.array([0, 0, 1], dtype=F32), (1, n, 1))
    return surf, view, dirs, [names[k] for k in order], skipped[order]


# ---- crafted inputs: points at the edge of a spot light's cone ----

CONE_SPREADS = (0.9, 0.0009, 0.0011, 0.012, 3.13, 3.139, 3.141, 4.0, 0.0, -0.5, np.nan, np.inf)
CONE_DISTANCES = (0.5, 3.0, 40.0)
CONE_BUCKETS = ("x > cos_in", "cos_out <= x <= cos_in", "x < cos_out")


def cone_world():
    """the only occluder is a floor far below (y = -100); one spot light per spread of CONE_SPREADS above it, each with a non-unit axis
    of its own"""
    w = rt.World()
    w.push_object(plain_material()).push_square([(-200, -100, -200), (-200, -100, 200), (200, -100, 200), (200, -100, -200)], [(0, 0), (0, 1), (1, 1), (1, 0)])
    g = np.random.default_rng(33)
    for k, s in enumerate(CONE_SPREADS):
        axis = g.normal(size=3)
        axis[1] = -abs(axis[1]) - 0.5
        w.push_light(spot(s, origin=(3.0 * (k % 4) - 4.5, 5.0 + 2.0 * (k // 4), 1.5 * (k % 3) - 1.5), direction=axis * g.uniform(0.2, 3.0),
                          softness=(0.5, 1.0, 2.0)[k % 3]))
    return w


def restate_cone_x(light, positions):
    """light_asks' x = dot(axis, offset) / (|axis| |offset|) in binary32 (csrc/rt_shade.h)"""
    axis = np.array(light.direction[:], dtype=F32)
    offset = np.asarray(positions, dtype=F32) - np.array(light.origin[:], dtype=F32)
    with np.errstate(all="ignore"):
        return dot32(axis[None], offset) / (magnitude32(axis) * magnitude32(offset))


def light_gives(light, positions):
    """orc_light_directional at every position: does the oracle's approximate_into_directional return a light"""
    import _oracle

    lib = _oracle.lib()
    d, c, o, h = (C.c_float * 3)(), (C.c_float * 3)(), (C.c_float * 3)(), C.c_int(0)
    return np.array([bool(lib.orc_light_directional(C.byref(light), (C.c_float * 3)(*p), d, c, o, C.byref(h))) for p in np.asarray(positions, dtype=F32)])


def cone_points(light, aux, seed=0):
    """Positions on circles about the light's axis at the angles spread + j 2e-6, |j| <= 200, at the distances 0.5, 3 and 40, the azimuth
    moving on by the golden angle; then, 0.02 and 0.05 rad to either side of the spread, four azimuths per distance, so that the two
    shortcut branches are met at every light that has them; a NaN or infinite spread gets one point on each side of the axis.  Returns
    (positions (N, 3) f32, normals facing the light, labels, bucket of CONE_BUCKETS per point from the restated x, the oracle's answer)
    and asserts: all three buckets hold 64 points where 401 steps of 2e-6 reach beyond the 1e-4 in cosine (sin(spread) > 0.3), the
    middle bucket holds 64 wherever the shortcut is on, and — wherever it is on — 16 points of the middle bucket lie on each side of the
    edge as the oracle reports it."""
    spread = float(F32(light.angle))
    axis = np.array(light.direction[:], dtype=np.float64)
    a = axis / np.linalg.norm(axis)
    e1 = np.cross(a, [0.0, 0.0, 1.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(a, e1)
    origin = np.array(light.origin[:], dtype=np.float64)
    theta, dist, labels = [], [], []
    if np.isfinite(spread):
        for j in range(-200, 201):
            for dd in CONE_DISTANCES:
                theta.append(spread + j * 2e-6); dist.append(dd); labels.append(f"spread {spread}: angle spread {j:+d} x 2e-6, distance {dd}")
        for off in (-0.05, -0.02, 0.02, 0.05):
            for dd in CONE_DISTANCES:
                for _ in range(4):
                    theta.append(spread + off); dist.append(dd); labels.append(f"spread {spread}: angle spread {off:+}, distance {dd}")
    else:
        theta, dist, labels = [0.3, -0.3], [3.0, 3.0], [f"spread {spread}: 0.3 rad to one side of the axis", f"spread {spread}: 0.3 rad to the other side"]
    theta, dist = np.array(theta), np.array(dist)
    phi = (seed + np.arange(theta.size)) * 2.399963229728653
    direction = np.cos(theta)[:, None] * a + np.sin(theta)[:, None] * (np.cos(phi)[:, None] * e1 + np.sin(phi)[:, None] * e2)
    pos = (origin + dist[:, None] * direction).astype(F32)
    offset = pos.astype(np.float64) - np.array(light.origin[:], dtype=F32).astype(np.float64)
    normal = (-offset / np.linalg.norm(offset, axis=1, keepdims=True)).astype(F32)
    x = restate_cone_x(light, pos)
    with np.errstate(invalid="ignore"):
        bucket = np.where(x > aux[0], 0, np.where(x < aux[1], 2, 1))
    some = light_gives(light, pos)
    on = np.isfinite(aux[0])
    counts = [int((bucket == b).sum()) for b in range(3)]
    if on and np.sin(spread) > 0.3:
        assert min(counts) >= 64, (spread, counts)
    if on:
        band = bucket == 1
        assert counts[1] >= 64 and (band & some).sum() >= 16 and (band & ~some).sum() >= 16, (spread, counts, (band & some).sum(), (band & ~some).sum())
        with np.errstate(invalid="ignore"):  # the shortcut's claim on the oracle's side: x > cos_in is inside, -1 <= x < cos_out outside
            assert some[bucket == 0].all() and not some[(bucket == 2) & (x >= F32(-1.0))].any(), spread
    else:
        assert counts[0] == 0 and counts[2] == 0
    return pos, normal, labels, bucket, some


def cone_edge_view(spread=0.9, axis=(1.0, 2.0, 3.0), scale=0.37):
    """A square 1.5 in front of a spot light, facing it, and a very narrow camera beside the light aimed at a point of the circle in
    which the cone's edge crosses the square: the 16 x 16 frame is 4e-3 across, the band between cos_out and cos_in about 1e-3 of it"""
    w = rt.World()
    ob = w.push_object(plain_material())
    o = np.array([0.3, 1.0, -0.2])
    dn = np.array(axis, float)
    dn /= np.linalg.norm(dn)
    c = o + 1.5 * dn
    a = np.cross(dn, [0, 1, 0])
    a /= np.linalg.norm(a)
    b = np.cross(dn, a)
    corners = [c - 3 * a - 3 * b, c - 3 * a + 3 * b, c + 3 * a + 3 * b, c + 3 * a - 3 * b]
    ob.push_square([tuple(p) for p in corners], [(0, 0), (0, 1), (1, 1), (1, 0)])
    w.push_light(spot(spread, origin=o, direction=np.array(axis, float) * scale))
    cam = _capi.Camera()
    eye = o + 0.4 * a + 0.3 * b
    target = c + 1.5 * np.tan(spread) * (0.8 * a + 0.6 * b)
    t = target - eye
    cam.center = tuple(eye)
    cam.toward = tuple(t / np.linalg.norm(t))
    cam.up = tuple(b)
    cam.near = -0.1
    cam.fovy = float(F32(2 * np.arctan(2e-3 / np.linalg.norm(t))))
    return w, cam
