"""Shared test support for the motion queries: the numpy restatement of the definition (include/rt_amd.h "motion queries"), the moved
scenes, the rays that reach every primitive, and the bound of the rigid-motion test with its derivation.

The restatement does the definition's f32 operations in the definition's order, element-wise over the records; numpy's float32 +, -, *, /
and sqrt are IEEE single operations, so it equals the CPU form bit for bit.  With dtype=np.float64 the same steps run in binary64 from
the same float32 inputs.

THE BOUND OF THE RIGID-MOTION TEST (RIGID_BOUND).  The 40-triangle scene and the camera are moved by one rigid motion — a rotation of
0.07 rad with a shift of about 0.3, and that shift alone —; the hits are the oracle's casts of the moved camera's 64 x 48 pixel centres
on the moved scene; their was-positions are projected through the camera before the move (_temporal_support.restate_motion).  Measured
on the CPU: the float32 chain (restatement, then the float32 projection) against the same steps in binary64 from the same float32 hits
and vertices.  What separates the two: the triangle's n, e and area are float32 (2^-24 relative per operation, about ten deep), the
signed areas cancel near an edge, the three divides and the weighted sum add a few 2^-24 of |m| ~ 0.4 each, and the projection's own
error (_temporal_support: 1.15e-5 pixels on its data) comes on top.  RIGID_MEASURED = 1.08e-5 pixels, rounded up, for either motion (the test prints
the figures of the run and fails if the run's is larger); the test asserts four times that, RIGID_BOUND = 4.32e-5 pixels, for the
distance of each asserted pixel's projected was-position from its own centre.  That distance also holds what the chain starts from —
the hit position is the cast's float32 result, and the moved vertices and camera are float32 roundings of the rigid motion: a few ulp of
coordinates of 2 to 6 against a pixel footprint of about 0.07 — which is what the factor four is for; the run measured 2.29e-5 pixels
(rotation, pixels on triangles) and 1.53e-5 (translation, all valid pixels).  Under the rotation only pixels on triangles are asserted:
rt_sphere has no orientation and the definition models no rotation of one.
"""
import ctypes as C
import functools

import numpy as np

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import _capi
import _records
import _scenes
from _scene_update_support import arrays_of, desc_with, dome_world, flat, small_rotation, transformed

F32 = np.float32
NAN_WORD = np.uint32(0x7FC00000)
RIGID_MEASURED = 1.08e-5
RIGID_BOUND = 4 * RIGID_MEASURED
RIGID_ROWS, RIGID_COLS = 48, 64


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def restate(verts, spheres, was_verts, was_spheres, hits, dtype=F32):
    """verts / was_verts: (N, 3, 8) or (N, 3, 3) float32 vertices now and kept; spheres / was_spheres: (M, 5) records now (index bits, centre,
    radius) and (M, 4) kept (centre, radius); hits: (n, 13) words.  Returns (n, 3): uint32 words for float32, float64 values otherwise."""
    T = dtype
    h = np.ascontiguousarray(hits).view(np.uint32).reshape(-1, 13)
    n = h.shape[0]
    kind, index = h[:, 0], h[:, 1].astype(np.int64)
    P_words = h[:, 3:6].copy()
    P = P_words.view(F32).astype(T)
    out = np.full((n, 3), np.nan, dtype=T)
    exact = np.zeros(n, dtype=bool)  # the raw words of P
    verts, was_verts = np.asarray(verts, dtype=F32)[:, :, :3], np.asarray(was_verts, dtype=F32)[:, :, :3]
    tri = (kind == 1) & (index < verts.shape[0])
    with np.errstate(all="ignore"):
        if tri.any():
            i, p = index[tri], P[tri]
            v, q = verts[i].astype(T), was_verts[i].astype(T)
            v0, v1, v2 = v[:, 0], v[:, 1], v[:, 2]
            c = cross(v1 - v0, v2 - v1)
            nrm = c * (T(1) / np.sqrt(dot(c, c)))[:, None]
            e0, e1, e2 = v2 - v1, v0 - v2, v1 - v0
            area = dot(cross(v1 - v0, v2 - v0), nrm)
            m = q - v
            a0, a1, a2 = dot(cross(e0, p - v1), nrm), dot(cross(e1, p - v2), nrm), dot(cross(e2, p - v0), nrm)
            b0, b1, b2 = (a0 / area)[:, None], (a1 / area)[:, None], (a2 / area)[:, None]
            out[tri] = p + ((m[:, 0] * b0 + m[:, 1] * b1) + m[:, 2] * b2)
            exact[np.flatnonzero(tri)[(m == 0).all(axis=(1, 2))]] = True
        spheres = np.asarray(spheres, dtype=F32).reshape(-1, 5)
        sph = (kind == 0) & (index < spheres.shape[0])
        if sph.any():
            i, p = index[sph], P[sph]
            now, kept = spheres[i][:, 1:5].astype(T), np.asarray(was_spheres, dtype=F32).reshape(-1, 4)[i].astype(T)
            s = (kept[:, 3] / now[:, 3])[:, None]
            out[sph] = kept[:, :3] + (p - now[:, :3]) * s
            exact[np.flatnonzero(sph)[(kept == now).all(axis=1)]] = True
    if T is not F32:
        out[exact] = P[exact]
        return out
    words = out.view(np.uint32).copy()
    words[~(tri | sph)] = NAN_WORD
    words[exact] = P_words[exact]
    return words


def same_words(got, want):
    """bit patterns equal; a NaN the arithmetic produced equals any NaN (its payload is the hardware's)"""
    g, w = np.asarray(got).view(np.uint32).reshape(-1, 3), np.asarray(want).view(np.uint32).reshape(-1, 3)
    return (g == w) | (np.isnan(g.view(F32)) & np.isnan(w.view(F32)))


def kept_of(verts, spheres):
    """what rt_scene_keep_positions keeps of a description, as the CPU form takes it: (N, 9) and (M, 4) float32"""
    return (np.ascontiguousarray(np.asarray(verts, dtype=F32)[:, :, :3]).reshape(-1, 9),
            np.ascontiguousarray(np.asarray(spheres, dtype=F32).reshape(-1, 5)[:, 1:5]))


def cpu(desc, was_triangles, was_spheres, hits, stride=3, fill=None):
    """rt_previous_positions_cpu raw: (status, message, (n, stride) uint32 words that started as `fill`)"""
    lib = _capi.host_lib()
    h = np.ascontiguousarray(hits).view(np.uint32).reshape(-1, 13)
    out = np.full((h.shape[0], stride), 0 if fill is None else fill, dtype=np.uint32)
    ptr = lambda a: None if a is None else C.c_void_p(np.ascontiguousarray(a).ctypes.data)
    wt = None if was_triangles is None else np.ascontiguousarray(was_triangles, dtype=F32)
    ws = None if was_spheres is None else np.ascontiguousarray(was_spheres, dtype=F32)
    rc = lib.rt_previous_positions_cpu(C.byref(desc), ptr(wt), ptr(ws), ptr(h), h.shape[0], ptr(out), stride)
    return rc, lib.rt_host_last_error().decode(), out


# ---- scenes ----


def small_world():
    return _scenes.random_world(11, 40, 3)


RIGID_ROT = small_rotation((0.3, 1.0, -0.2), 0.07)
RIGID_SHIFT = np.array([0.25, -0.1, 0.15])


def rigid(verts, spheres, rot=RIGID_ROT, shift=RIGID_SHIFT):
    """the whole scene moved by one rigid motion: (verts, spheres), float32"""
    s = np.array(spheres, dtype=F32).reshape(-1, 5)
    s[:, 1:4] = (s[:, 1:4].astype(np.float64) @ rot.T + shift).astype(F32)
    return transformed(np.asarray(verts, dtype=F32), rot, shift), s


def rigid_camera(camera, rot=RIGID_ROT, shift=RIGID_SHIFT):
    cam = rt.Camera.from_buffer_copy(camera)
    cam.center = tuple((rot @ np.array(list(camera.center), dtype=np.float64) + shift).astype(F32).tolist())
    cam.toward = tuple((rot @ np.array(list(camera.toward), dtype=np.float64)).astype(F32).tolist())
    cam.up = tuple((rot @ np.array(list(camera.up), dtype=np.float64)).astype(F32).tolist())
    return cam


def jittered(verts, seed=3, sigma=0.02, which=slice(None)):
    """a deformation: every vertex of triangles `which` moved on its own, face normals recomputed"""
    v = np.array(verts, dtype=F32)
    g = np.random.default_rng(seed)
    v[which, :, :3] += g.normal(0, sigma, v[which, :, :3].shape).astype(F32)
    return flat(v)


# ---- the cases: what moved between the keep and the query ----


@functools.lru_cache(maxsize=None)
def base(which="small"):
    """(world, description, vertices, spheres) of the unmoved scene; read-only"""
    w = small_world() if which == "small" else dome_world()
    d = w.desc()
    _, verts, sph = arrays_of(d)
    verts.setflags(write=False)
    sph.setflags(write=False)
    return w, d, verts, sph


@functools.lru_cache(maxsize=None)
def moved(name):
    """(description now, vertices now, spheres now, hits on it) of a case: the kept positions are base()'s"""
    _, d, verts, sph = base("dome" if name == "dome deformed" else "small")
    v, s = np.array(verts), np.array(sph)
    if name == "one vertex":
        v[7, 1, :3] += np.array([0.05, -0.02, 0.03], dtype=np.float32)
    elif name in ("deformed", "dome deformed"):
        v = jittered(verts)
    elif name == "sphere moved and rescaled":
        s[1, 1:4] += np.array([0.1, 0.05, -0.2], dtype=np.float32)
        s[1, 4] *= np.float32(1.25)
        s[2, 4] *= np.float32(0.5)  # rescaled in place
    elif name == "rigid":
        v, s = rigid(verts, sph)
    elif name == "degenerate":
        s[0, 4] = 0.0  # a current radius of 0: the scale is a divide by zero
        v[5, 2] = v[5, 1]  # two equal vertices: no normal, no area
        v[6, 0, :3] += np.float32(0.01)
    elif name != "nothing":
        raise KeyError(name)
    now = desc_with(d, verts=v, spheres=s)
    hits = _records.oracle_hits(now, case_rays(now, v, s))
    if name == "degenerate":  # nothing hits a degenerate primitive: records that name them, at positions of their neighbours
        h = hits[hits[:, 0] == 1][:4].copy()
        h[:2, 1], h[2:, 1] = 5, 6
        z = hits[hits[:, 0] == 0][:1].copy()
        z[:, 1] = 0
        hits = np.concatenate([hits, h, z])
    hits.setflags(write=False)
    return now, v, s, hits


CASES = ["nothing", "one vertex", "deformed", "dome deformed", "sphere moved and rescaled", "rigid", "degenerate"]


# ---- rays ----


def primitive_rays(verts, spheres):
    """two rays per primitive, started next to it: at a triangle's centroid from 0.004 in front and behind (front- and back-face hits), at a
    sphere from outside towards the centre and from the centre outwards (a back-face hit)"""
    v = np.asarray(verts, dtype=np.float64)[:, :, :3]
    c = v.mean(axis=1)
    n = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 1])
    with np.errstate(invalid="ignore"):  # a degenerate triangle has no normal; nothing is hit from it
        n /= np.linalg.norm(n, axis=1, keepdims=True)
    s = np.asarray(spheres, dtype=np.float64).reshape(-1, 5)
    u = np.random.default_rng(9).normal(size=(s.shape[0], 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    origins = np.concatenate([c + 0.004 * n, c - 0.004 * n, s[:, 1:4] + u * (s[:, 4:5] + 0.004), s[:, 1:4]])
    directions = np.concatenate([-n, n, -u, u])
    return _records.ray_records(origins, directions, rt.BOTH)


def case_rays(desc, verts, spheres, camera=None):
    """a 16 x 12 frame, random rays (every face mode, exclusions) and the rays next to every primitive"""
    cam = _scenes.camera(2) if camera is None else camera
    return np.concatenate([_records.camera_rays_cpu(cam, 16, 12), _records.source_b(desc, 5, 160), primitive_rays(verts, spheres)])


def special_hits(hits, n_triangles, n_spheres):
    """records that are no hit of the scene: RT_HIT_NONE, kind 7, index == n_triangles, index == n_spheres, a huge index — each with a
    position that must not show in the output"""
    h = np.ascontiguousarray(hits).view(np.uint32).reshape(-1, 13)
    tri, sph = h[h[:, 0] == 1][0].copy(), h[h[:, 0] == 0][0].copy()
    bad = [tri.copy() for _ in range(6)]
    bad[0][0] = _records.NONE
    bad[1][0] = 7
    bad[2][1] = n_triangles
    bad[3] = sph.copy()
    bad[3][1] = n_spheres
    bad[4][1] = 0xFFFFFFFF
    bad[5] = sph.copy()
    bad[5][1] = 0x80000000
    return np.stack(bad)


def payload_hits(hits):
    """a triangle and a sphere record whose position holds a NaN with a payload, -0.0 and a denormal"""
    h = np.ascontiguousarray(hits).view(np.uint32).reshape(-1, 13)
    out = np.stack([h[h[:, 0] == 1][0].copy(), h[h[:, 0] == 0][0].copy()])
    out[:, 3:6] = np.array([0x7FC12345, 0x80000000, 0x00000001], dtype=np.uint32)
    return out
