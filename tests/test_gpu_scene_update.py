"""Scene updates (include/rt_amd.h rt_scene_update_*): a scene created from description A, rendered once on the stream (so that its
workspaces exist and are reused) and then updated to B gives, bit for bit, what a scene freshly created from B gives — a 64x48 depth-5
Whitted frame with its cast count, rt_cast_rays on 20 000 random rays plus rays grazing the moved triangles' bounding spheres (NaN
distances compared as bits), two depth-of-field epochs at 32x24 with samples, flags, generator records and casts — under the default
walker and under the breadth-first one.  One Whitted frame per case is also compared with the oracle's render of B.  The node cases
also read the device's node records back (rt_diag_scene_nodes) and compare them with the fresh scene's word for word: outputs alone
cannot tell a refit that keeps a node's rejection alive from one that switches every node to "always visit".  A dome of 3200
triangles reaches the workgroup refit (a node above RT_REFIT_WAVE_MAX = 1024 triangles) and a tree of two inner levels."""
import ctypes as C

import numpy as np
import pytest

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import _capi
import _oracle
import _scenes
from _scene_update_support import arrays_of, BOX, CONE, desc_with, DOME, dome_world, flat, LARGE, large_case, LARGE_CASES, large_dome_parts, nodes_of, range_ends, SQUARE, transformed

pytestmark = pytest.mark.gpu

FRAME = rt.Frame.full(64, 48, 5)
TILE = rt.Frame.full(32, 24, 5)
WALKERS = [{}, {"RT_AMD_BFS_WALK_TRIANGLES": 1}]


# ---- the test world: floor, box, a 200-triangle dome (inner node + leaves of 16), an axis-aligned square, spheres ---------------


@pytest.fixture(scope="module")
def dome():
    w = dome_world()
    d = w.desc()
    obj, verts, _ = arrays_of(d)
    assert len(obj) == 216 and (obj[DOME] == 2).all() and (obj[SQUARE] == 3).all()
    nodes = nodes_of(d)
    inner = nodes[(nodes[:, 1] == 0)]
    assert len(inner) >= 1 and inner[0, 0] == DOME.start, nodes  # the dome is a tree: an inner node over leaves of 16
    assert (nodes[(nodes[:, 0] >= DOME.start) & (nodes[:, 0] < DOME.stop) & (nodes[:, 1] != 0)][:, 1] <= 16).all()
    assert inner[0, 2] == CONE  # 100 plane directions below it: a cone
    assert (nodes[nodes[:, 0] == DOME.start + 16][:, 2] == 8).all()  # a leaf: 8 quads, each one plane direction — explicit normals
    return w, d, verts


# ---- the large world: the same with a dome of 40 x 40 quads — a root above 1024 triangles over inner nodes of 256 over leaves of 16 -----


@pytest.fixture(scope="module")
def large_dome():
    return large_dome_parts()


# ---- outputs of a scene ---------------------------------------------------------------------------------------------------------

def bounding_spheres(verts):
    """per run of 16 triangles, and of all: (centre, radius) of the bounding box's sphere"""
    out = []
    for lo in list(range(0, len(verts), 16)) + [None]:
        p = (verts if lo is None else verts[lo:lo + 16])[:, :, :3].reshape(-1, 3).astype(np.float64)
        p = p[np.isfinite(p).all(axis=1)]
        c = 0.5 * (p.min(axis=0) + p.max(axis=0))
        out.append((c, np.linalg.norm(p - c, axis=1).max()))
    return out


def query_rays(seed, moved_a, moved_b):
    """20 000 random rays, and rays that graze the bounding spheres of the moved triangles before and after: tangent to the sphere,
    just inside, just outside and at the 5 % margin the node test folds in"""
    import torch

    rng = np.random.default_rng(seed)
    o = rng.uniform(-3.5, 3.5, (20000, 3)) + np.array([0, 1.0, 0])
    d = rng.normal(0, 1, (20000, 3))
    d[:2000] = np.array([0.3, 0.5, -0.2]) - o[:2000] + rng.normal(0, 0.6, (2000, 3))
    os_, ds = [o], [d]
    for c, r in bounding_spheres(moved_a) + bounding_spheres(moved_b):
        for scale in (0.97, 1.0, 1.0247, 1.05, 1.08):
            eye = c + rng.normal(0, 1, (12, 3)) * 2.5
            u = np.cross(c - eye, rng.normal(0, 1, (12, 3)))
            u /= np.linalg.norm(u, axis=1, keepdims=True)
            os_.append(eye)
            ds.append(c + r * scale * u - eye)
    o, d = np.concatenate(os_).astype(np.float32), np.concatenate(ds).astype(np.float32)
    face = rng.integers(0, 3, len(o)).astype(np.int32)
    return rt.make_rays(torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda(), face=torch.from_numpy(face).cuda())


def outputs(scene, cam, rays, stream):
    import torch

    with torch.cuda.stream(stream):
        cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        img = rt.render_whitted(scene, cam, FRAME, ray_count=cnt)
        hits = rt.cast_rays(scene, rays)
        rng = rt.Rng(TILE)
        samples = torch.empty((2, TILE.rows, TILE.cols, 3), dtype=torch.float32, device="cuda")
        valid = torch.empty((2, TILE.rows, TILE.cols), dtype=torch.uint8, device="cuda")
        cnt2 = torch.zeros(1, dtype=torch.int64, device="cuda")
        rt.render_distributed(scene, cam, TILE, rng, 2, samples=samples, valid=valid, ray_count=cnt2)
    stream.synchronize()
    return {"whitted": img.cpu().numpy().view(np.uint32), "casts": int(cnt.item()), "hits": hits.cpu().numpy(),
            "samples": samples.cpu().numpy().view(np.uint32), "valid": valid.cpu().numpy(), "rng": rng.download(), "dist_casts": int(cnt2.item())}


def assert_same(got, want, what):
    for key in want:
        assert np.array_equal(got[key], want[key]), (what, key)


# ---- the node records of a scene ------------------------------------------------------------------------------------------------

INF_BITS = 0x7F800000
AXIS_STEP = 2.0 ** -23  # one rounding step of a binary32 component of a unit vector, absolute
K2_RELATIVE = 3e-4


def records_of(scene):
    """rt_diag_scene_nodes: (the pre-order records (N, 40), the level-order records (N, 40), the 16-byte pieces (3 N + 2 T, 4)) as
    uint32; the scene's stream is synchronised"""
    lib = _capi.amd_lib()
    out = []
    for which in range(3):
        n = C.c_size_t(0)
        _capi.check(lib.rt_diag_scene_nodes(scene._h, which, None, 0, C.byref(n)))
        buf = np.empty(n.value, dtype=np.uint32)
        _capi.check(lib.rt_diag_scene_nodes(scene._h, which, buf.ctypes.data_as(C.c_void_p), n.value, C.byref(n)))
        out.append(buf)
    return out[0].reshape(-1, 40), out[1].reshape(-1, 40), out[2].reshape(-1, 4)


def level_order(seg):
    """the pre-order index of the node at each level-order position (rt_scene_create): the top-level nodes, then every inner node's
    children one after the other"""
    count, skip_to, n = seg[:, 1], seg[:, 7], len(seg)
    order, k = [], 0
    while k < n:
        order.append(k)
        k = int(skip_to[k])
    at = 0
    while at < len(order):
        k = order[at]
        j = k + 1
        while count[k] == 0 and j < skip_to[k] and j < n:
            order.append(j)
            j = int(skip_to[j])
        at += 1
    assert sorted(order) == list(range(n))
    return np.asarray(order, dtype=np.int64)


# per node, the words of its three places side by side: what is fixed at creation, and what a refit derives from the triangles
STATS_PLACES = (0, 37, 74)  # where the pre-order record's, the level-order record's and the pieces' words start in a row of `stats`
CONE_COLUMNS = [base + 5 + k for base in (0, 37) for k in range(4)] + [79, 80, 81, 82]  # normals[0][0..3]: the axis and K^2


def node_table(rec):
    seg, bfs, soa = rec
    n = len(seg)
    at = np.empty(n, dtype=np.int64)
    at[level_order(seg)] = np.arange(n)
    b, p0, p1, p2 = bfs[at], soa[at], soa[n + at], soa[2 * n + at]
    topo = np.concatenate([seg[:, [0, 1, 7]], b[:, [0, 1, 7]], p0[:, :2], p1[:, 3:]], axis=1)  # first, count, skip_to / children
    stats = np.concatenate([seg[:, 2:7], seg[:, 8:], b[:, 2:7], b[:, 8:], p0[:, 2:], p1[:, :3], p2], axis=1)
    assert stats.shape[1] == 83
    return topo, stats, range_ends(seg[:, [0, 1, 2, 7]]), soa[3 * n:]


CONE_FIGURES = {"nodes": 0, "words": 0, "differ": 0, "axis": 0.0, "k2": 0.0}


def compare_records(updated, fresh_from, fresh_to, touched, same_tree, what):
    """the records of `updated` (created as `fresh_from` was, then updated) against those of `fresh_to`, node by node: all words bit for
    bit but a cone's axis and K^2 — the device adds the normals up in another order than rt_scene_create: a component of the rounded
    axis moves by one rounding step at most (2^-23 absolute), the half-angle with it by sqrt(3) 2^-23 rad at most, K^2 (K >= 1.01e-3)
    by 3e-4 relative at most.  Nodes are matched by (first, count, end of range); a node of the updated scene
      - that is plain in `fresh_from` is never refitted and stays as it is there,
      - whose counterpart in `fresh_to` qualifies has its words — so it qualifies too,
      - whose counterpart is a plain leaf, or that has none and lies over a touched triangle, is always visited (n_normals 0, r2_hi +inf),
      - that has none and lies over no touched triangle has the words of `fresh_from`."""
    (tu, su, eu, triu), (ta, sa, ea, _), (tb, sb, eb, trib) = (node_table(records_of(s)) for s in (updated, fresh_from, fresh_to))
    assert np.array_equal(tu, ta), (what, "first, count, skip_to are fixed at creation")
    assert np.array_equal(triu, trib), (what, "the triangles' planes and bounding spheres")
    key_b = {(int(t[0]), int(t[1]), int(e)): j for j, (t, e) in enumerate(zip(tb, eb))}
    if same_tree:
        assert np.array_equal(ta[:, :3], tb[:, :3]), (what, "the fresh scene has the same tree")
    cone_cols = np.asarray(CONE_COLUMNS)
    k2_cols = cone_cols[3::4]
    for k in range(len(tu)):
        node = (what, k, tuple(int(x) for x in tu[k, :3]), int(eu[k]))
        j = key_b.get((int(tu[k, 0]), int(tu[k, 1]), int(eu[k])))
        if sa[k, 0] == 0:
            want = sa[k]
        elif j is not None and sb[j, 0] != 0:
            want = sb[j]
            assert (su[k, STATS_PLACES] == want[0]).all(), (node, "qualifies in the fresh scene, so in the updated one", su[k, STATS_PLACES], want[0])
        elif j is not None or (tu[k, 0] < touched.stop and eu[k] > touched.start):
            assert (su[k, STATS_PLACES] == 0).all() and (su[k, [p + 1 for p in STATS_PLACES]] == INF_BITS).all(), (node, "always visited", su[k])
            continue
        else:
            want = sa[k]
        exact = np.ones(83, dtype=bool)
        if want[0] == CONE:
            exact[cone_cols] = False
            got_f, want_f = su[k, cone_cols].view(np.float32).astype(np.float64), want[cone_cols].view(np.float32).astype(np.float64)
            diff = np.abs(got_f - want_f)
            is_k2 = np.isin(cone_cols, k2_cols)
            rel = diff[is_k2] / want_f[is_k2]
            CONE_FIGURES["nodes"] += 1
            CONE_FIGURES["words"] += cone_cols.size
            CONE_FIGURES["differ"] += int((su[k, cone_cols] != want[cone_cols]).sum())
            CONE_FIGURES["axis"] = max(CONE_FIGURES["axis"], float(diff[~is_k2].max()))
            CONE_FIGURES["k2"] = max(CONE_FIGURES["k2"], float(rel.max()))
            assert (diff[~is_k2] <= AXIS_STEP).all() and (rel <= K2_RELATIVE).all(), (node, "cone", got_f, want_f)
        bad = np.flatnonzero((su[k] != want) & exact)
        assert bad.size == 0, (node, "columns", bad, su[k, bad], want[bad])
    print(f"{what}: cone words so far: {CONE_FIGURES['differ']} of {CONE_FIGURES['words']} in {CONE_FIGURES['nodes']} nodes differ, "
          f"axis by at most {CONE_FIGURES['axis']:.3e} (bound {AXIS_STEP:.3e}), K^2 by at most {CONE_FIGURES['k2']:.3e} relative (bound {K2_RELATIVE:.1e})")


def check_update(desc_a, desc_b, cam, update, moved, seed=1, stream=None, back=False, records=None):
    """A rendered, updated to B by `update(scene, stream)`, against a fresh B under both walkers and against the oracle; with `back`,
    updated to A again by `back(scene, stream)` against a fresh A (what was disqualified qualifies again).  `records`: (the triangles
    the update touches, whether a fresh B has A's tree) — then the node records are compared as well (compare_records)."""
    import torch

    _, va, _ = arrays_of(desc_a)
    _, vb, _ = arrays_of(desc_b)
    rays = query_rays(seed, va[moved], vb[moved])
    want_img, want_casts = _oracle.render_whitted(desc_b, cam, FRAME)
    for opts in WALKERS:
        s = stream if stream is not None else torch.cuda.current_stream()
        with rt.options(**opts):  # the switch is read when a scene is created
            scene, fresh_b, fresh_a = rt.Scene(desc_a), rt.Scene(desc_b), rt.Scene(desc_a)
        before = outputs(scene, cam, rays, s)  # the workspaces of this stream exist from here on
        update(scene, s)
        got = outputs(scene, cam, rays, s)
        assert not (np.array_equal(got["whitted"], before["whitted"]) and np.array_equal(got["hits"], before["hits"])), ("the update shows", opts)
        assert_same(got, outputs(fresh_b, cam, rays, s), ("updated against fresh", opts))
        assert np.array_equal(got["whitted"], want_img.view(np.uint32)) and got["casts"] == want_casts, ("oracle", opts)
        if records:
            compare_records(scene, fresh_a, fresh_b, records[0], records[1], ("records, updated against fresh", opts))
        if back:
            back(scene, s)
            again = outputs(scene, cam, rays, s)
            if records:
                compare_records(scene, fresh_a, fresh_a, records[0], True, ("records, back against fresh", opts))
            assert_same(again, outputs(fresh_a, cam, rays, s), ("back against fresh", opts))
            assert_same(again, before, ("back against before", opts))
        for sc in (scene, fresh_a, fresh_b):
            sc.close()


def vertex_update(first, verts, as_numpy=False):
    import torch

    def go(scene, stream):
        with torch.cuda.stream(stream):
            scene.update_vertices(first, verts if as_numpy else torch.from_numpy(np.ascontiguousarray(verts, dtype=np.float32)).cuda(), stream=stream)
    return go


# ---- the cases ------------------------------------------------------------------------------------------------------------------

def test_clustered_leaves_on_a_second_stream():
    """clustered_world: 12-triangle boxes, one rotated and translated; first > 0, count < all, on a non-default stream"""
    import torch

    w = _scenes.clustered_world(11, n_boxes=4)
    a = w.desc()
    _, va, _ = arrays_of(a)
    box = slice(2 + 12, 2 + 24)
    rng = np.random.default_rng(5)
    centre = va[box, :, :3].reshape(-1, 3).mean(axis=0)
    rot = _scenes._rotation(rng)
    vb = va.copy()
    vb[box] = transformed(va[box], rot, centre - rot @ centre + np.array([0.5, 0.3, -0.4]))
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    check_update(a, desc_with(a, verts=vb), _scenes.camera(11), vertex_update(box.start, vb[box]), box, stream=stream,
                 back=vertex_update(box.start, va[box], as_numpy=True))


def test_node_tree_explicit_normals_and_cone(dome):
    """a leaf of the dome (8 quads: 8 plane directions, explicit normals) with every triangle nudged a little: 16 plane directions, a
    cone — and back: the number of directions crosses 8 both ways.  A second leaf is flattened into one plane (8 -> 1)."""
    w, a, va = dome
    leaf, other = slice(DOME.start + 16, DOME.start + 32), slice(DOME.start + 32, DOME.start + 48)
    rng = np.random.default_rng(13)
    vb = va.copy()
    vb[leaf, :, :3] += rng.normal(0, 0.002, (16, 3, 3)).astype(np.float32)
    vb[other, :, 1] = np.float32(1.25)  # y = const: one plane direction
    both = slice(leaf.start, other.stop)
    vb[both] = flat(vb[both])
    nodes = nodes_of(desc_with(a, verts=vb))
    assert nodes[nodes[:, 0] == leaf.start][0, 2] == CONE and nodes[nodes[:, 0] == other.start][0, 2] == 1  # what a fresh B has there
    same_tree = np.array_equal(nodes[:, [0, 1, 3]], nodes_of(a)[:, [0, 1, 3]])
    check_update(a, desc_with(a, verts=vb), _scenes.camera(3), vertex_update(both.start, vb[both]), DOME, seed=2, back=vertex_update(both.start, va[both]),
                 records=(both, same_tree))


def test_node_tree_cone_beyond_60_degrees(dome):
    """a leaf crumpled until its normals spread beyond 60 degrees: the leaf and the inner node above it fail and are always visited"""
    w, a, va = dome
    leaf = slice(DOME.start + 48, DOME.start + 64)
    rng = np.random.default_rng(9)
    vb = va.copy()
    vb[leaf, :, :3] += rng.normal(0, 0.25, (16, 3, 3)).astype(np.float32)
    vb[leaf] = flat(vb[leaf])
    nodes = nodes_of(desc_with(a, verts=vb))
    assert not ((nodes[:, 1] == 0) & (nodes[:, 0] == DOME.start)).any()  # a fresh B has no inner node over the dome any more
    check_update(a, desc_with(a, verts=vb), _scenes.camera(4), vertex_update(leaf.start, vb[leaf]), DOME, seed=3, back=vertex_update(leaf.start, va[leaf]),
                 records=(leaf, False))


@pytest.mark.parametrize("name", LARGE_CASES)
def test_large_dome_workgroup_refit_and_two_inner_levels(large_dome, name):
    """the dome of 3200 triangles: its root is refitted by a workgroup (refit_nodes<256>: the LDS stage of the reductions, loops that wrap,
    representative rounds across four waves), the nodes below by a wave.  The whole dome moved; a band across four inner nodes nudged
    (leaves go from explicit normals to a cone); one leaf crumpled beyond 60 degrees (the leaf, its inner node and the root are always
    visited, and qualify again on the way back) — frames, hits and samples as everywhere, and the node records word for word."""
    w, a, va = large_dome
    b, vb, touched, same_tree = large_case(name, va, a)
    check_update(a, b, _scenes.camera(3), vertex_update(touched.start, vb[touched]), LARGE, seed=8 + LARGE_CASES.index(name),
                 back=vertex_update(touched.start, va[touched]), records=(touched, same_tree))


def test_disqualified_triangles_and_back(dome):
    """one triangle collapsed to a line, one a sliver under 1.15 degrees, one with a NaN vertex — in the box and in two leaves of the dome:
    their nodes are always visited; back to A they qualify again"""
    w, a, va = dome
    vb = va.copy()
    line, sliver, nan = BOX.start + 3, DOME.start + 5, DOME.start + 100
    vb[line, 2, :3] = 0.5 * (vb[line, 0, :3] + vb[line, 1, :3])
    vb[sliver, 2, :3] = vb[sliver, 0, :3] + (vb[sliver, 1, :3] - vb[sliver, 0, :3]) * np.float32(0.5) + np.float32(0.003) * (vb[sliver, 2, :3] - vb[sliver, 0, :3])
    vb[nan, 1, 0] = np.nan
    vb[[line, sliver]] = flat(vb[[line, sliver]])
    e0, e1 = vb[sliver, 1, :3] - vb[sliver, 0, :3], vb[sliver, 2, :3] - vb[sliver, 0, :3]
    assert np.degrees(np.arctan2(np.linalg.norm(np.cross(e0, e1)), e0 @ e1)) < 1.15
    whole = slice(BOX.start, DOME.stop)

    def update(scene, stream):  # three calls, one triangle each
        for k in (line, sliver, nan):
            vertex_update(k, vb[k:k + 1])(scene, stream)

    check_update(a, desc_with(a, verts=vb), _scenes.camera(5), update, whole, seed=4, back=vertex_update(whole.start, va[whole]))


def test_plane_sharing_cleared_and_restored(dome):
    """the halves of the axis-aligned square moved apart (only the FIRST half is updated: the second one's FOLLOWS / WEAK bit is one
    past the range) and together again"""
    w, a, va = dome
    vb = va.copy()
    vb[SQUARE.start, :, 1] += np.float32(0.3)
    first = slice(SQUARE.start, SQUARE.start + 1)
    check_update(a, desc_with(a, verts=vb), _scenes.axis_camera((1.5, 1.0, 4.0)), vertex_update(first.start, vb[first]), SQUARE, seed=5,
                 back=vertex_update(first.start, va[first]))


def test_outside_the_creation_box(dome):
    """the box scaled about the origin until its coordinates pass three times the extent the scene was created with"""
    w, a, va = dome
    extent = np.abs(va[:, :, :3]).max()
    vb = va.copy()
    scale = np.float32(3.5 * extent / np.abs(va[BOX, :, :3]).max())
    vb[BOX, :, :3] *= scale
    assert np.abs(vb[BOX, :, :3]).max() > 3 * extent
    check_update(a, desc_with(a, verts=vb), _scenes.camera(6), vertex_update(BOX.start, vb[BOX]), BOX, seed=6, back=vertex_update(BOX.start, va[BOX]))


def test_reference_scene_spheres_lights_materials():
    """the reference scene: spheres moved, lights and materials replaced, against a fresh scene and the oracle"""
    import torch

    w = rt.reference_world()
    a = w.desc()
    _, va, sa = arrays_of(a)
    rng = np.random.default_rng(21)
    sb = sa.copy()
    sb[:, 1:4] += rng.uniform(-0.3, 0.3, (len(sb), 3)).astype(np.float32)
    sb[:, 4] *= rng.uniform(0.7, 1.3, len(sb)).astype(np.float32)
    lights = [_scenes.light(rng, (i + 1) % 3) for i in range(a.n_lights)]
    mats = [a.materials[i] for i in range(a.n_materials)]
    mats[1:3] = [_scenes.material(rng), _scenes.material(rng)]
    b = desc_with(a, spheres=sb, lights=lights, materials=mats)

    def update(scene, stream):
        junk = sb.copy()
        junk[:, 0] = np.float32(1e9)  # object_index in the input is ignored
        with torch.cuda.stream(stream):
            scene.update_spheres(1, junk[1:], stream=stream)
            scene.update_spheres(0, torch.from_numpy(junk[:1]).cuda(), stream=stream)
        scene.update_lights(0, lights, stream=stream)
        scene.update_materials(1, mats[1:3], stream=stream)

    def back(scene, stream):
        scene.update_spheres(0, sa, stream=stream)
        scene.update_lights(0, [a.lights[i] for i in range(a.n_lights)], stream=stream)
        scene.update_materials(0, [a.materials[i] for i in range(a.n_materials)], stream=stream)

    check_update(a, b, rt.reference_camera(), update, slice(0, len(va)), seed=7, back=back)


def test_a_captured_frame_replays_on_the_updated_scene(dome):
    """a frame captured into a graph before the update and replayed after it is the fresh scene's frame: the scene's pointers and the
    by-value KernelScene did not change.  A vertex update itself is captured too, once the scene's first one has run."""
    import torch

    w, a, va = dome
    rng = np.random.default_rng(2)
    rot = _scenes._rotation(rng)
    vb = va.copy()
    vb[DOME] = transformed(va[DOME], rot, np.array([0.2, 0.5, 0.1]) - rot @ np.array([0.4, 0.2, -0.3]) + np.array([0.4, 0.2, -0.3]))
    cam = _scenes.camera(8)
    for opts in WALKERS:
        with rt.options(**opts):
            scene, fresh_a, fresh_b = rt.Scene(a), rt.Scene(a), rt.Scene(desc_with(a, verts=vb))
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        dev_b = torch.from_numpy(np.ascontiguousarray(vb[DOME])).cuda()
        dev_a = torch.from_numpy(np.ascontiguousarray(va[DOME])).cuda()
        dev = dev_b.clone()
        with torch.cuda.stream(stream):
            out = torch.empty((FRAME.rows, FRAME.cols, 3), dtype=torch.float32, device="cuda")
            rt.render_whitted(scene, cam, FRAME, out=out, stream=stream)  # uncaptured first: the workspace
            stream.synchronize()
            frame_graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(frame_graph, stream=stream):
                rt.render_whitted(scene, cam, FRAME, out=out, stream=stream)
            scene.update_vertices(DOME.start, dev, stream=stream)  # the scene's first update allocates: not captured
            update_graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(update_graph, stream=stream):
                scene.update_vertices(DOME.start, dev, stream=stream)
            for source, fresh in ((dev_b, fresh_b), (dev_a, fresh_a), (dev_b, fresh_b)):
                dev.copy_(source)
                update_graph.replay()
                out.fill_(7.0)
                frame_graph.replay()
                stream.synchronize()
                want = rt.render_whitted(fresh, cam, FRAME, stream=stream)
                stream.synchronize()
                assert np.array_equal(out.cpu().numpy().view(np.uint32), want.cpu().numpy().view(np.uint32)), opts
        for sc in (scene, fresh_a, fresh_b):
            sc.close()


def test_argument_checks_in_order():
    """with a scene at hand: the range (in 64 bits), then the empty range, then the null data pointer; lights and materials validated
    as rt_scene_create validates them, nothing written"""
    import torch

    lib = _capi.amd_lib()
    w = _scenes.clustered_world(2, n_boxes=2)
    d = w.desc()
    scene = rt.Scene(w)
    cam = _scenes.camera(2)
    want, casts = rt.render_whitted_numpy(scene, cam, FRAME)
    ptr = C.c_void_p(16)  # never dereferenced
    for name, have in (("rt_scene_update_vertices", d.n_triangles), ("rt_scene_update_spheres", d.n_spheres)):
        fn = getattr(lib, name)
        assert fn(scene._h, have, 1, ptr, None) == -1 and b"beyond" in lib.rt_last_error(), name
        assert fn(scene._h, 0xFFFFFFFF, 0xFFFFFFFF, ptr, None) == -1 and b"beyond" in lib.rt_last_error(), name  # no 32-bit wrap
        assert fn(scene._h, have + 1, 0, None, None) == -1 and b"beyond" in lib.rt_last_error(), name  # before the empty range
        assert fn(scene._h, have, 0, None, None) == 0 and fn(scene._h, 0, 0, None, None) == 0, name  # nothing to do
        assert fn(scene._h, 0, 1, None, None) == -1 and b"null data" in lib.rt_last_error(), name
    lights, mats = (_capi.Light * 1)(d.lights[0]), (_capi.Material * 1)(d.materials[0])
    for fn, have, good in ((lib.rt_scene_update_lights, d.n_lights, lights), (lib.rt_scene_update_materials, d.n_materials, mats)):
        assert fn(scene._h, have, 1, good, None) == -1 and b"beyond" in lib.rt_last_error()
        assert fn(scene._h, have, 0, None, None) == 0
        assert fn(scene._h, 0, 1, None, None) == -1 and b"null data" in lib.rt_last_error()
    two = (_capi.Light * 2)(d.lights[1], d.lights[0])
    two[1].kind = 3
    assert lib.rt_scene_update_lights(scene._h, 0, 2, two, None) == -1 and b"unknown light kind" in lib.rt_last_error()
    twom = (_capi.Material * 2)(d.materials[1], d.materials[0])
    twom[1].normal_fn = 2
    assert lib.rt_scene_update_materials(scene._h, 0, 2, twom, None) == -1 and b"unknown material function" in lib.rt_last_error()
    torch.cuda.synchronize()
    got, got_casts = rt.render_whitted_numpy(scene, cam, FRAME)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and got_casts == casts  # nothing was written
