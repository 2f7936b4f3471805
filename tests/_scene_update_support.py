"""Shared test support for scene updates: the dome scenes, their node trees, and the expected refit structure of the large dome."""
import ctypes as C

import numpy as np

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import _capi
import _scenes


CONE = 0xFFFFFFFF


def arrays_of(desc):
    """(object index per triangle, vertices (N, 3, 8) float32, spheres (M, 5) float32 with the index bits in column 0): copies"""
    raw = np.frombuffer(C.string_at(desc.triangles, desc.n_triangles * C.sizeof(_capi.Triangle)), dtype=np.uint32).reshape(-1, 25)
    sph = np.frombuffer(C.string_at(desc.spheres, desc.n_spheres * C.sizeof(_capi.Sphere)), dtype=np.float32).reshape(-1, 5)
    return raw[:, 0].copy(), raw[:, 1:].copy().view(np.float32).reshape(-1, 3, 8), sph.copy()


def desc_with(desc, verts=None, spheres=None, lights=None, materials=None):
    """a description like `desc` with some arrays replaced (counts and object indices stay)"""
    obj, v0, s0 = arrays_of(desc)
    verts = v0 if verts is None else verts
    raw = np.empty((len(obj), 25), dtype=np.uint32)
    raw[:, 0] = obj
    raw[:, 1:] = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 24).view(np.uint32)
    tris = (_capi.Triangle * len(obj)).from_buffer_copy(raw.tobytes())
    sph = (_capi.Sphere * desc.n_spheres).from_buffer_copy(np.ascontiguousarray(s0 if spheres is None else spheres, dtype=np.float32).tobytes())
    mats = (_capi.Material * desc.n_materials)(*(materials if materials is not None else [desc.materials[i] for i in range(desc.n_materials)]))
    lts = (_capi.Light * desc.n_lights)(*(lights if lights is not None else [desc.lights[i] for i in range(desc.n_lights)]))
    out = _capi.SceneDesc(tris, len(obj), sph, desc.n_spheres, mats, desc.n_materials, lts, desc.n_lights)
    out._keepalive = (tris, sph, mats, lts)
    return out


def nodes_of(desc):
    """rt_scene_describe_nodes: rows of (first, count, n_normals, skip_to, dealing word, 0)"""
    lib = _capi.amd_lib()
    n = C.c_uint32(0)
    _capi.check(lib.rt_scene_describe_nodes(C.byref(desc), None, 0, C.byref(n)))
    words = (C.c_uint32 * (6 * n.value))()
    _capi.check(lib.rt_scene_describe_nodes(C.byref(desc), words, n.value, C.byref(n)))
    return np.frombuffer(words, dtype=np.uint32).reshape(-1, 6).copy()


def flat(verts):
    """face-normal vertices: positions kept, normals = the face normal, uvs kept"""
    v = np.array(verts, dtype=np.float32)
    n = np.cross(v[:, 1, :3] - v[:, 0, :3], v[:, 2, :3] - v[:, 1, :3]).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        n = n / np.linalg.norm(n, axis=1, keepdims=True)
    v[:, :, 3:6] = np.nan_to_num(n)[:, None, :].astype(np.float32)
    return v


BOX, DOME, SQUARE = slice(2, 14), slice(14, 214), slice(214, 216)


def dome_triangles(centre=(0.4, 0.2, -0.3), radius=0.9, half_angle=0.6, bulge=1.0, grid=10):
    """grid x grid quads over a spherical cap around +y (10: 200 triangles) whose normals stay within half_angle of the axis; with
    bulge < 1 the cap is flattened along y and its normals lie closer to the axis"""
    c = np.array(centre)
    g = np.linspace(-half_angle, half_angle, grid + 1)

    def p(i, j):
        a, b = g[i], g[j]
        d = np.array([np.sin(a) * np.cos(b), bulge * np.cos(a) * np.cos(b), np.sin(b)])
        return c + radius * d / np.linalg.norm(d) if bulge == 1.0 else c + radius * d

    tris = []
    for i in range(grid):
        for j in range(grid):
            q = [p(i, j), p(i, j + 1), p(i + 1, j + 1), p(i + 1, j)]
            tris += [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
    return np.array(tris)


def dome_world(**dome_args):
    rng = np.random.default_rng(77)
    w = rt.World()
    w.push_object(_scenes.material(rng, "plain")).push_square([(-4, -0.5, -4), (-4, -0.5, 4), (4, -0.5, 4), (4, -0.5, -4)], [(0, 0), (0, 1), (1, 0), (0, 1)])
    box = w.push_object(_scenes.material(rng, "plain"))
    for tri in _scenes._box((-1.2, 0.1, 0.6), (0.4, 0.5, 0.3), _scenes._rotation(rng)):
        box.push_flat_triangle(tri, rng.uniform(0, 1, (3, 2)).tolist())
    dome = w.push_object(_scenes.material(rng, "plain"))
    for tri in dome_triangles(**dome_args):
        dome.push_flat_triangle(tri.tolist(), rng.uniform(0, 1, (3, 2)).tolist())
    w.push_object(_scenes.material(rng, "plain")).push_square([(1.0, 0.0, 1.0), (1.0, 0.0, 2.0), (2.0, 0.0, 2.0), (2.0, 0.0, 1.0)], [(0, 0), (0, 1), (1, 1), (1, 0)])
    for _ in range(2):
        w.push_object(_scenes.material(rng, "plain")).push_sphere(tuple(rng.uniform(-1.5, 1.5, 3) + np.array([0, 0.6, 0])), float(rng.uniform(0.2, 0.5)))
    for i in range(3):
        w.push_light(_scenes.light(rng, i % 3))
    return w


LARGE_GRID, LARGE_BULGE = 40, 0.8
LARGE = slice(14, 14 + 2 * LARGE_GRID * LARGE_GRID)
REFIT_WAVE_MAX = 1024  # csrc/rt_api_internal.h RT_REFIT_WAVE_MAX: a node of more triangles is refitted by refit_nodes<256>


def range_ends(nodes):
    """one past the last triangle below each node of the pre-order array (columns first, count, ..., skip_to as rt_scene_describe_nodes
    gives them): a leaf's range is [first, first + count), an inner node's runs to the largest end among the nodes before its skip_to
    (rt_scene_create's rule for the ranges the refit works on)"""
    end = nodes[:, 0].astype(np.int64) + nodes[:, 1]
    for k in np.flatnonzero(nodes[:, 1] == 0):
        end[k] = max(end[k], end[k + 1:nodes[k, 3]].max())
    return end


def large_dome_parts():
    """(world, description, vertices) of the large world, with its structure asserted: needs no GPU.  With the 10 x 10 dome's plain cap
    (bulge 1) the corner faces of a 40 x 40 grid at half-angle 0.6 lie 47 degrees off the axis, where the cone's K reaches 1 and
    rt_scene_create emits no root; flattened to 0.8 the root qualifies."""
    w = dome_world(grid=LARGE_GRID, bulge=LARGE_BULGE)
    d = w.desc()
    obj, verts, _ = arrays_of(d)
    assert len(obj) == LARGE.stop + 2 and (obj[LARGE] == 2).all() and obj[LARGE.stop] == 3
    large_dome_structure(nodes_of(d))
    return w, d, verts


def large_dome_structure(nodes, rooted=True):
    """the tree over the large dome: leaves of 16 below inner nodes of 256 triangles, below (if `rooted`) a root of 3200 that qualifies"""
    end = range_ends(nodes)
    inside = (nodes[:, 0] >= LARGE.start) & (end <= LARGE.stop)
    inner = inside & (nodes[:, 1] == 0)
    below = end - nodes[:, 0]
    big = np.flatnonzero(inner & (below > REFIT_WAVE_MAX))
    assert (big.size >= 1) == rooted, nodes[inner]
    if rooted:
        assert nodes[big[0], 0] == LARGE.start and end[big[0]] == LARGE.stop and nodes[big[0], 2] == CONE, nodes[big[0]]
        nested = [j for j in np.flatnonzero(inner) if big[0] < j < nodes[big[0], 3]]
        assert len(nested) >= 2 and all(16 < below[j] <= REFIT_WAVE_MAX and nodes[j, 2] == CONE for j in nested), nodes[nested]  # two inner levels
    leaves = nodes[inside & (nodes[:, 1] != 0)]
    assert (leaves[:, 1] <= 16).all() and leaves[:, 1].sum() == LARGE.stop - LARGE.start
    return end


def small_rotation(axis, angle):
    k = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(angle) * kx + (1 - np.cos(angle)) * kx @ kx


def large_case(name, va, a):
    """(description B, the updated triangles, whether a fresh B has A's tree) of the three cases on the large dome; what each is meant
    to reach is asserted on the description alone, without a GPU"""
    rows = lambda nodes: nodes[:, [0, 1, 3]]
    na = nodes_of(a)
    vb = va.copy()
    if name == "whole dome moved":  # translated and rotated a little, inside the creation box: every node of the tree, the root's cone turns
        touched, centre = LARGE, np.array([0.4, 0.2, -0.3])
        rot = small_rotation((1.0, 0.3, -0.5), 0.12)
        vb[LARGE] = transformed(va[LARGE], rot, centre - rot @ centre + np.array([0.15, 0.1, -0.2]))
        assert np.abs(vb[:, :, :3]).max() <= np.abs(va[:, :, :3]).max()
        nb = nodes_of(desc_with(a, verts=vb))
        assert np.array_equal(nb, na)
    elif name == "band nudged":  # 40 leaves under four of the 256-triangle nodes: 8 plane directions each become 16, a cone
        touched = slice(LARGE.start + 200, LARGE.start + 840)
        rng = np.random.default_rng(31)
        vb[touched, :, :3] += rng.normal(0, 0.0005, (touched.stop - touched.start, 3, 3)).astype(np.float32)
        vb[touched] = flat(vb[touched])
        nb = nodes_of(desc_with(a, verts=vb))
        assert np.array_equal(rows(nb), rows(na))
        changed = np.flatnonzero(nb[:, 2] != na[:, 2])
        assert len(changed) >= 38 and (na[changed, 2] == 8).all() and (nb[changed, 2] == CONE).all(), (na[changed], nb[changed])
        assert len({int(np.flatnonzero((na[:k, 1] == 0))[-1]) for k in changed}) >= 3  # ... under different inner nodes
    elif name == "leaf crumpled":  # each triangle of one leaf turned 69 degrees about its centroid, to alternating sides: no cone holds them
        touched = slice(LARGE.start + 1600 + 48, LARGE.start + 1600 + 64)
        for i, t in enumerate(range(touched.start, touched.stop)):
            rot = small_rotation((1.0, 0.0, 0.0) if i % 4 < 2 else (0.0, 0.0, 1.0), 1.2 if i % 2 else -1.2)
            centroid = va[t, :, :3].astype(np.float64).mean(axis=0)
            vb[t:t + 1] = transformed(va[t:t + 1], rot, centroid - rot @ centroid)
        nb = nodes_of(desc_with(a, verts=vb))
        ea, eb = large_dome_structure(na), large_dome_structure(nb, rooted=False)
        key = lambda nodes, end: {(int(n[0]), int(n[1]), int(e)): n for n, e in zip(nodes, end)}
        ka, kb = key(na, ea), key(nb, eb)
        gone = sorted(set(ka) - set(kb))
        # the leaf stays a node of its own, now plain; the root and the inner node above it are gone, every other node is as it was
        assert kb[(touched.start, 16, touched.stop)][2] == 0 and ka[(touched.start, 16, touched.stop)][2] == 8
        assert len(gone) == 2 and all(c == 0 and f <= touched.start and touched.stop <= e for f, c, e in gone), gone
        assert gone[0] == (LARGE.start, 0, LARGE.stop) and set(kb) <= set(ka)
        assert all((kb[k][2] == ka[k][2]) or k[0] == touched.start for k in kb)
    else:
        raise KeyError(name)
    same_tree = name != "leaf crumpled"
    return desc_with(a, verts=vb), vb, touched, same_tree


LARGE_CASES = ["whole dome moved", "band nudged", "leaf crumpled"]


def transformed(verts, rot, shift):
    out = verts.copy()
    out[:, :, :3] = (verts[:, :, :3].astype(np.float64) @ rot.T + shift).astype(np.float32)
    return flat(out)
