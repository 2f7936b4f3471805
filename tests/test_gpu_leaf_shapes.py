"""Every clustered-leaf size and node-tree shape through every cast: the scenes of tests/_scenes.py leaf_size_world (both kinds per
count), tree_shape_world and big_tree_world — whose node arrays tests/test_leaf_shape_scenes.py pins without a GPU — against the
oracle's World::cast (orc_cast) and its siblings, bit for bit with NaN equal to NaN (test_gpu_ray_query.same_hits,
test_gpu_hit_queries.assert_parity, test_gpu_scene_sizes._same).

Ray batches are laid out in WAVES of 64 consecutive records (numpy, fixed seeds), and what a wave is for is checked from the
reference side alone (check_claims: float64 geometry and the oracle's hits) before any GPU result is read.  Per branch of
cast_pairs (csrc/rt_cast.h), the waves that reach it and the input condition that proves it:

  pair-wise dealing, every (K, ck, R)   "sparse" and "edge" waves, one of each per leaf of the leaf-size worlds (all 35 dealings of
                                        the counts 8 .. 64 and those of the remainder leaves 1 .. 7): 1 .. 24 rays whose oracle hit
                                        lies in the leaf; every other ray of the wave passes the leaf's box centre at more than twice
                                        the box diagonal (its line misses the node's sphere), from an origin within 3.9 scene extents
                                        (the rejection filter applies), with |n.d| > 1e-2 |d| for every face normal and, for a cone,
                                        |a.d| beyond the cone's bound: it does not need the leaf.  So exactly 1 .. 24 lanes need it.
  lanes past R * ck                     the same waves on the leaves whose dealing has R * ck < 64 (ck = 9, R = 7: 63 lanes, ...).
  ragged last chunk                     "edge" waves aim at the first and last triangle of the last chunk (and of the first), and
                                        exclude them with each face value; K * ck > count for 31 of the counts.
  more than 24 needing lanes            "dense" waves: all 64 rays hit the leaf (12 leaf sizes over the dealings, tree and remainder
                                        leaves among them): the leaf is run wave-uniformly.
  the drain                             "deck" waves: 2 .. 24 rays through the middle of 64, 21, 49 parallel triangles and of 24
                                        identical ones; the number of (ray, triangle) pairs whose plane point is strictly inside
                                        the triangle is counted in float64: 65 .. 128 (drained once) or more than 128 (several times).
                                        With identical triangles the last index must win.
  the equal-distance merge              "dup" waves (tree-shape world): rays from both sides at the 7-triangle plain runs that repeat
                                        triangles of the clustered slab24 before and after it in index order; the oracle's hit is
                                        the later index each time (asserted), which is the pair-wise key once and the wave-uniform
                                        running best once.
  the NaN fallback                      "nan" waves: rays lying in a deck plane exactly (n.d = 0, d - n.o = 0); the oracle's distance
                                        is NaN (asserted).
  helping tail lanes                    every batch has 64 k + 1 records and is cast at that length and at 64 k: the last wave is one
                                        ray aimed into the 49-triangle leaf (K = 7) and 63 idle lanes that help.

Two scratch layouts instantiate cast_pairs.  PairLdsSlim (plane records fetched from global memory with `pair ? local : 0u`):
cast_rays_kernel and camera-ray casts of csrc/rt_query.hip (rt.cast_rays), and the hit-query kernels of csrc/rt_hit_query.hip
(rt.shade_hits, rt.refract_rays) — test_cast_rays and test_hit_queries.  PairLds (plane records staged in LDS):
dist_chain_kernel of csrc/rt_distributed.hip, the split organisation of rt.render_distributed — test_renders "split".  The Whitted
render kernels and the fused stochastic kernel walk the same node array wave-uniformly or breadth-first."""
import itertools

import numpy as np
import pytest

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import _capi
import _oracle
import _scenes
import _hit_support as hq
import _records as rec
from _scenes import dealing

pytestmark = pytest.mark.gpu
FRONT, BACK, BOTH = 0, 1, 2
NONE = 0xFFFFFFFF
AIMED, THROUGH, OTHER, DECK, IN_PLANE, UNCLAIMED = 1, 2, 0, 3, 4, 5  # what a ray is in its wave
DENSE_COUNTS = (8, 9, 13, 21, 29, 36, 49, 50, 57, 64)


class Geo:
    """float64 geometry of a Shapes world: triangles, centroids, unit face normals, the leaves of its node array"""

    def __init__(self, s):
        self.s = s
        self.desc = s.world.desc()
        self.nodes = _scenes.nodes_of(self.desc)
        self.tris = s.tris.astype(np.float64)
        self.centroids = self.tris.mean(1)
        n = np.cross(self.tris[:, 1] - self.tris[:, 0], self.tris[:, 2] - self.tris[:, 1])
        self.normals = n / np.linalg.norm(n, axis=1, keepdims=True)
        self.extent = float(np.abs(self.tris).max())
        self.leaves = [(int(r[0]), int(r[1]), int(r[2])) for r in self.nodes if r[1] != 0]
        self.run = {name: (first, count) for name, first, count, _ in s.runs}

    def leaf_at(self, tri):
        return next(l for l in self.leaves if l[0] <= tri < l[0] + l[1])

    def box(self, first, count):
        p = self.tris[first:first + count].reshape(-1, 3)
        lo, hi = p.min(0), p.max(0)
        return (lo + hi) / 2, float(np.linalg.norm(hi - lo))

    def far_from(self, first, count):
        """triangles whose centroid is, horizontally, beyond 2.6 box diagonals + 0.6 of the leaf's box centre"""
        c, diag = self.box(first, count)
        h = np.hypot(self.centroids[:, 0] - c[0], self.centroids[:, 2] - c[2])
        far = np.flatnonzero(h > 2.6 * diag + 0.6)
        assert far.size, "nothing is far from this leaf"
        return far


def rays_to(geo, g, tri, role, side=1.0, exclude="random", narrow=False):
    """one ray per entry of `tri`, towards a random interior point of that triangle from 0.5 .. 1 above it (side -1: below), at most 17
    degrees off the vertical; narrow: from 1.5 .. 2 above, nearly vertical, towards the middle (for the decks).  exclude "random": as test_gpu_ray_query.random_rays — none, a sphere, a triangle (never the target; some out of range)."""
    tri = np.asarray(tri, dtype=np.int64)
    n = tri.size
    w = (0.25 + 0.25 * g.dirichlet((1, 1, 1), n)) if narrow else (0.15 + 0.55 * g.dirichlet((1, 1, 1), n))
    target = (geo.tris[tri] * w[:, :, None]).sum(1)
    h = g.uniform(1.5, 2.0, n) if narrow else g.uniform(0.5, 1.0, n)
    lean = 0.02 if narrow else 0.3
    o = target + np.stack([g.uniform(-lean, lean, n) * h, side * h, g.uniform(-lean, lean, n) * h], 1)
    d = target - o
    # the far rays are not unit length; the others are: World::cast's sphere test takes |d| = 1 for granted, and a longer or shorter ray
    # from below a sphere can "hit" it, which would take the ray away from the leaf it is aimed at
    d *= (g.choice([1.0, 0.3, 2.5], n) if role == OTHER else 1.0 / np.linalg.norm(d, axis=1))[:, None]
    face = g.choice([FRONT, BOTH] if side > 0 else [BACK, BOTH], n)
    nt, ns = int(geo.desc.n_triangles), int(geo.desc.n_spheres)
    kind = g.choice([-1, rt.SPHERE, rt.TRIANGLE], n, p=[0.4, 0.2, 0.4])
    index = np.where(kind == rt.TRIANGLE, g.integers(0, nt + 3, n), g.integers(0, ns + 3, n))
    index[g.random(n) < 0.02] = 0x7FFFFFF0
    clash = (kind == rt.TRIANGLE) & (index == tri)
    index[clash] = (tri[clash] + 1) % nt
    ex_face = g.integers(0, 3, n)
    if exclude is None:
        kind = np.full(n, -1)
    return dict(o=o, d=d, face=face, kind=kind, index=index, ex_face=ex_face, role=np.full(n, role), target=tri)


def excluding(r, index, ex_face):
    r = dict(r)
    r["kind"] = np.full(r["target"].size, rt.TRIANGLE)
    r["index"] = np.asarray(index, dtype=np.int64)
    r["ex_face"] = np.asarray(ex_face, dtype=np.int64)
    return r


def cat(parts):
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


class Batch:
    def __init__(self, geo, seed):
        self.geo = geo
        self.g = np.random.default_rng(seed)
        self.parts = []
        self.waves = []  # (kind, leaf first, leaf count, claim)

    def wave(self, kind, leaf, mine, claim=0):
        """`mine` and rays at triangles far from the leaf, 64 in all, in a random lane order"""
        n = mine["role"].size
        assert 1 <= n <= 64
        if n < 64:
            far = self.geo.far_from(leaf[0], leaf[1])
            mine = cat([mine, rays_to(self.geo, self.g, self.g.choice(far, 64 - n), OTHER)])
        order = self.g.permutation(64)
        self.parts.append({k: v[order] for k, v in mine.items()})
        self.waves.append((kind, leaf[0], leaf[1], claim))

    def finish(self, tail):
        self.parts.append(tail)
        r = cat(self.parts)
        self.role, self.target = r["role"], r["target"]
        self.rays = rec.ray_records(r["o"], r["d"], r["face"], (r["kind"], r["index"], r["ex_face"]))
        assert self.rays.shape[0] == 64 * len(self.waves) + 1
        return self


def sparse_and_edge(b, leaf, m):
    """two waves for one leaf: m rays at random triangles of it; then its chunk edges — the first and last triangle of the first and of
    the last chunk — plainly, excluding another edge triangle with each face value, excluding themselves on the side they are not
    hit from, and (THROUGH) excluding themselves for good, with Front and with Both"""
    geo, g = b.geo, b.g
    first, count, _ = leaf
    b.wave("sparse", leaf, rays_to(geo, g, first + g.integers(0, count, m), AIMED))
    k, ck, _ = dealing(count)
    edges = first + np.array(sorted({0, min(ck, count) - 1, (k - 1) * ck, count - 1}))
    e = edges.size
    parts = [rays_to(geo, g, edges, AIMED, exclude=None)]
    if count > 1:
        parts.append(excluding(rays_to(geo, g, edges, AIMED), np.roll(edges, 1) if e > 1 else edges + 1, np.arange(e) % 3))
        parts.append(excluding(rays_to(geo, g, edges, AIMED), np.roll(edges, -1) if e > 1 else edges + 1, (np.arange(e) + 1) % 3))
    parts.append(excluding(rays_to(geo, g, edges, AIMED), edges, np.full(e, BACK)))
    parts.append(excluding(rays_to(geo, g, edges[-2:], THROUGH), edges[-2:], [FRONT, BOTH][:edges[-2:].size]))
    mine = cat(parts)
    mine["face"][mine["role"] == THROUGH] = BOTH
    b.wave("edge", leaf, mine)


def deck_waves(b, name, counts):
    geo, g = b.geo, b.g
    first, count = geo.run[name]
    for m in counts:
        pairs = m * count
        b.wave("deck", (first, count), rays_to(geo, g, np.full(m, first), DECK, narrow=True, exclude=None), claim=128 if pairs > 128 else 64 if pairs > 64 else 0)


def in_plane(geo, g, name, layers):
    """rays IN the plane of a deck triangle: origin.y on the plane, direction.y = 0 — n.d = 0 and d - n.o = 0 exactly, t = 0 / 0.  Every
    other horizontal triangle of the scene has n.d = 0 too: below the ray's plane t = -inf (rejected), above it t = +inf, NaN areas, accepted
    — and `nearest_t < t` lets a later +inf replace the NaN.  So the cast ends on the NaN when no triangle after the ray's own lies above
    its plane (the decks are the scene's last runs); for the other rays no claim is made (UNCLAIMED)."""
    first, count = geo.run[name]
    tri = first + np.asarray(layers)
    c = geo.centroids[tri]
    o = np.stack([c[:, 0] + 0.25, geo.tris[tri, 0, 1], c[:, 2] + 1.0], 1)  # from beyond the last row, over the patches: the decks stand
    d = np.tile([-0.25, 0.0, -1.0], (tri.size, 1))                         # side by side with their planes at the same heights
    n = tri.size
    last = np.array([not (geo.tris[t + 1:, 0, 1] > geo.tris[t, 0, 1]).any() for t in tri])
    return dict(o=o, d=d, face=np.where(np.arange(n) % 2 == 1, FRONT, BOTH), kind=np.full(n, -1), index=np.zeros(n, dtype=np.int64),
                ex_face=np.zeros(n, dtype=np.int64), role=np.where(last, IN_PLANE, UNCLAIMED), target=tri)


def leaf_batch(geo, seed):
    b = Batch(geo, seed)
    decks = {geo.run[name][0] for name, _, _ in _scenes.DECKS}
    for k, leaf in enumerate(geo.leaves):
        if leaf[0] not in decks:
            sparse_and_edge(b, leaf, 1 + (7 * k + seed) % 24)
    patches = {first for name, first, _, _ in geo.s.runs if name.startswith("patch")}
    dense = [l for l in geo.leaves if l[1] in DENSE_COUNTS and l[0] in patches]
    dense += [l for l in geo.leaves if l[0] == geo.run["tree64+3"][0] + 64 or l[0] == geo.run["tree64+6"][0] + 16]  # a remainder and a tree leaf
    assert len(dense) >= 12
    for leaf in dense:
        b.wave("dense", leaf, rays_to(geo, b.g, leaf[0] + b.g.integers(0, leaf[1], 64), AIMED))
    deck_waves(b, "deck64", (2, 3, 8, 24))
    deck_waves(b, "deck21", (3, 4, 8, 24))  # 3 x 21 = 63 pairs: the list just short of its first drain
    deck_waves(b, "deck49", (2, 3, 8, 24))
    deck_waves(b, "deck0", (3, 8, 24))
    for name, layers in (("deck64", [63, 20, 63]), ("deck21", [20, 12]), ("deck0", [5, 23])):
        b.wave("nan", geo.run[name], in_plane(geo, b.g, name, layers))
    first, count = geo.run["patch49"]
    return b.finish(rays_to(geo, b.g, [first + 48], AIMED, exclude=None))


def special_leaves(geo, names):
    """per named run: its last leaf, and — where the run has more than 16 leaves — its 17th (257th) too"""
    out = []
    for name, nth in names:
        first, count = geo.run[name]
        mine = [l for l in geo.leaves if first <= l[0] < first + count]
        out.append(mine[nth])
    return out


def tree_batch(geo, seed, special, per_run):
    b = Batch(geo, seed)
    g = b.g
    for name, first, count, _ in geo.s.runs:  # random triangles of every object, a wave at a time: aimed at it, the rest elsewhere
        for _ in range(per_run):
            m = int(g.integers(1, 25))
            far = np.flatnonzero(np.linalg.norm(geo.centroids - geo.centroids[first + count // 2], axis=1) > 0.5)
            b.parts.append(rays_to(geo, g, np.r_[first + g.integers(0, count, m), g.choice(far, 64 - m)][g.permutation(64)], OTHER))
            b.waves.append(("run", first, count, 0))
    for leaf in special:
        if leaf[2] != 0:
            b.wave("sparse", leaf, rays_to(geo, g, leaf[0] + g.integers(0, leaf[1], int(g.integers(1, 25))), AIMED))
        b.wave("dense" if leaf[2] != 0 else "run", leaf, rays_to(geo, g, leaf[0] + g.integers(0, leaf[1], 64), AIMED if leaf[2] != 0 else OTHER))
    if _scenes.DUP_OF in geo.run:
        slab = geo.run[_scenes.DUP_OF]
        both = slab[0] + np.r_[0:7, 10:17]
        for up, down in ((both, both[3:10]), (both[4:11], both)):
            mine = cat([rays_to(geo, g, up, AIMED, side=1.0), rays_to(geo, g, down, AIMED, side=-1.0)])
            b.wave("dup", slab + (1,), mine)
    first, count = geo.s.runs[0][1:3]
    return b.finish(rays_to(geo, g, [first + count - 1], OTHER, exclude=None))


def line_distance(c, o, d):
    return np.linalg.norm(np.cross(c - o, d), axis=1) / np.linalg.norm(d, axis=1)


def check_claims(geo, b, want):
    """what each wave is for, from the inputs (as binary32 records, in float64) and the oracle's hits alone"""
    o = b.rays[:, 0:3].copy().view(np.float32).astype(np.float64)
    d = b.rays[:, 3:6].copy().view(np.float32).astype(np.float64)
    hit_tri = np.where(want[:, 0] == rt.TRIANGLE, want[:, 1].astype(np.int64), -1)
    for w, (kind, first, count, claim) in enumerate(b.waves):
        rows = np.arange(64 * w, 64 * w + 64)
        role = b.role[rows]
        mine, other = rows[role != OTHER], rows[role == OTHER]
        if kind == "run":
            continue
        aimed = rows[role == AIMED]
        if kind == "dup":
            slab, a, c = geo.run[_scenes.DUP_OF][0], geo.run["dupA"][0], geo.run["dupB"][0]
            j = b.target[aimed] - slab
            later = np.where(j < 7, slab + j, c + j - 10)  # dupA < slab24 < dupB in index order: the later of the two copies wins
            assert np.array_equal(hit_tri[aimed], later), (w, hit_tri[aimed], later)
            assert np.array_equal(geo.tris[a:a + 7], geo.tris[slab:slab + 7]) and set(want[aimed, 11]) == {0, 1}  # from both sides
        else:
            inside = (hit_tri[aimed] >= first) & (hit_tri[aimed] < first + count)
            assert inside.all(), (kind, w, count, "aimed rays whose oracle hit is outside the leaf", aimed[~inside], hit_tri[aimed[~inside]])
        through = rows[role == THROUGH]
        assert (hit_tri[through] != b.target[through]).all()
        if kind == "dense":
            assert aimed.size == 64
            continue
        assert 1 <= mine.size <= 24, (kind, w, mine.size)
        centre, diag = geo.box(first, count)
        assert (line_distance(centre, o[other], d[other]) > 2 * diag).all(), (kind, w, "a far ray passes the leaf")
        assert ((o[other] ** 2).sum(1) < (3.9 * geo.extent) ** 2).all()
        dl = np.linalg.norm(d[other], axis=1)
        n = geo.normals[first:first + count]
        assert (np.abs(d[other] @ n.T) > 1e-2 * dl[:, None]).all(), (kind, w, "a far ray is nearly parallel to a face")
        # a cone leaf is tested on its axis a (the mean normal) and half-angle theta: steep means |a.d| >= (1.01e-3 + sin theta) / cos theta |d|
        axis = (n * np.sign(n @ n[0])[:, None]).sum(0)
        axis /= np.linalg.norm(axis)
        theta = np.arccos(np.clip(np.abs(n @ axis).min(), -1, 1)) + 1e-5
        bound = (1.01e-3 + np.sin(theta)) / np.cos(theta) * 1.0001
        assert (np.abs(d[other] @ axis) > 1.02 * bound * dl).all(), (kind, w, "a far ray is inside the leaf's cone band")
        if kind == "deck":
            rays = rows[role == DECK]
            p = geo.tris[first:first + count]
            t = (p[None, :, 0, 1] - o[rays, None, 1]) / d[rays, None, 1]  # planes y = const
            x, z = o[rays, None, 0] + d[rays, None, 0] * t, o[rays, None, 2] + d[rays, None, 2] * t
            ok = t > 0
            for u, v in ((0, 1), (1, 2), (2, 0)):  # strictly on the inner side of each edge (the winding makes the normal +y)
                ex, ez = p[None, :, v, 0] - p[None, :, u, 0], p[None, :, v, 2] - p[None, :, u, 2]
                ok &= ez * (x - p[None, :, u, 0]) - ex * (z - p[None, :, u, 2]) > 1e-9
            pairs = int(ok.sum())
            assert pairs == rays.size * count, (w, pairs)
            if claim:
                assert pairs > claim and (claim == 128 or pairs <= 128), (w, pairs, claim)
            else:
                assert pairs <= 64
            if first == geo.run.get("deck0", (-1,))[0]:
                assert (hit_tri[rays] == first + count - 1).all()  # identical triangles: the last index
        if kind == "nan":
            rays = rows[role == IN_PLANE]
            assert np.isnan(want[rays, 12].view(np.float32)).all(), (w, want[rays])
    last = b.rays.shape[0] - 1
    if b.role[last] == AIMED:
        first, count, _ = geo.leaf_at(int(b.target[last]))
        assert first <= hit_tri[last] < first + count and dealing(count)[0] == 7


class Case:
    pass


_cases = {}


def case(name):
    """the world, its batch, the oracle's hits and the checked claims: made once per world"""
    if name not in _cases:
        c = Case()
        if name in ("leaf0", "leaf1"):
            c.geo = Geo(_scenes.leaf_size_world(int(name[-1])))
            c.batch = leaf_batch(c.geo, 10 + int(name[-1]))
        elif name == "tree":
            c.geo = Geo(_scenes.tree_shape_world())
            special = special_leaves(c.geo, [("tree65", -1), ("tree81", -1), ("tree255", -1), ("tree257", 16), ("tree272", 16), ("tree273", 16),
                                             ("tree273", 17), (f"crumpled{_scenes.CRUMPLED}", 16)])
            c.batch = tree_batch(c.geo, 20, special, 3)
        else:
            c.geo = Geo(_scenes.big_tree_world())
            special = special_leaves(c.geo, [("tree4096", -1), ("tree4112", 255), ("tree4112", 256)])
            c.batch = tree_batch(c.geo, 30, special, 12)
        c.want = rec.oracle_hits(c.geo.desc, c.batch.rays)
        check_claims(c.geo, c.batch, c.want)
        _cases[name] = c
    return _cases[name]


def describe(b, bad):
    """the waves of the first few differing records"""
    out = []
    for r in bad[:4]:
        w = int(r) // 64
        out.append((int(r), b.waves[w] if w < len(b.waves) else "tail", int(b.role[r])))
    return out


MODES = {"default": ({}, {}), "wave_uniform": ({}, {"RT_AMD_QUERY_WAVE_UNIFORM": 1}), "bfs": ({"RT_AMD_BFS_WALK_TRIANGLES": 1}, {}),
         "bfs_cap96": ({"RT_AMD_BFS_WALK_TRIANGLES": 1, "RT_AMD_DIAG_BFS_CAP": 96}, {}), "no_bfs": ({"RT_AMD_BFS_WALK_TRIANGLES": 0}, {})}
CAST_CASES = list(itertools.product(("leaf0", "leaf1", "tree", "big"), ("default", "wave_uniform", "bfs", "bfs_cap96"))) + [("big", "no_bfs")]


@pytest.mark.parametrize("world,mode", CAST_CASES)
def test_cast_rays(world, mode):
    """rt.cast_rays: pair-wise (default below the breadth-first switch; "no_bfs" for the world above it), wave-uniform, breadth-first and
    breadth-first with lists that overflow, at 64 k + 1 and at 64 k records"""
    c = case(world)
    import torch

    torch.cuda.set_device(0)
    create, call = MODES[mode]
    with rt.options(**create):
        scene = rt.Scene(c.geo.s.world)
        with rt.options(**call):
            n = c.batch.rays.shape[0]
            full = rec.dev(c.batch.rays)
            got = [rt.cast_rays(scene, full), rt.cast_rays(scene, full[:n - 1].contiguous())]
            torch.cuda.synchronize()
    for g, length in zip(got, (n, n - 1)):
        ok = rec.same_hits(g.cpu().numpy(), c.want[:length])
        bad = np.flatnonzero(~ok)
        assert ok.all(), f"{world} {mode} n={length}: {bad.size} differ: {describe(c.batch, bad)}: got {g.cpu().numpy().view(np.uint32)[bad[:1]]} want {c.want[bad[:1]]}"


@pytest.mark.parametrize("world", ["leaf0", "leaf1"])
def test_hit_queries(world):
    """rt.shade_hits and rt.refract_rays on the hits of the whole batch: shadow casts with the hit triangle excluded, and the glass walk,
    which starts inside a clustered leaf for the hits on transparent patches"""
    c = case(world)
    import torch

    torch.cuda.set_device(0)
    desc = c.geo.desc
    rays, hits = c.batch.rays, c.want
    finite = np.isfinite(hits[:, rec.FLOAT_WORDS].view(np.float32)).all(axis=1)
    rows = np.flatnonzero((hits[:, 0] <= 1) & finite)
    glass = np.array([desc.materials[int(o)].transparency > 0.0 for o in hits[rows, 2]])
    clustered = np.array([c.geo.leaf_at(int(t))[2] != 0 for t in hits[rows, 1]])
    assert (glass & clustered).sum() > 500 and (~glass).sum() > 500
    want = hq.oracle_queries(desc, rays, hits, rows=rows)
    # the patches are sheets: a walk that starts in one casts once, inside, with its own triangle excluded, and leaves for good
    assert (want.kind[rows] != NONE).all()
    assert want.shade_casts[rows].sum() > rows.size  # shadow rays were cast
    scene = rt.Scene(c.geo.s.world)
    sub_rays, sub_hits = rays[rows], hits[rows]
    got = hq.gpu_queries(scene, rec.dev(sub_rays), rec.dev(sub_hits))
    w = hq.Want()
    w.rows = np.arange(rows.size)
    for name in ("shade", "shade_casts", "reflect", "kind", "travel", "escape"):
        setattr(w, name, getattr(want, name)[rows])
    hq.assert_parity(got, w, sub_hits, world)


def _variant(v):
    _capi.check(_capi.amd_lib().rt_set_variant(v))


@pytest.mark.parametrize("world,what", [("leaf0", "whitted"), ("leaf0", "split"), ("leaf0", "fused"), ("leaf1", "split"), ("tree", "whitted"), ("big", "whitted")])
def test_renders(world, what):
    """a 64 x 48 frame from the world's camera: the Whitted render in variants 18 and 2, and two epochs of the stochastic pass, split
    (dist_chain_kernel: cast_pairs over PairLds) and fused — values, valid flags, generator records and cast counts"""
    import torch

    torch.cuda.set_device(0)
    c = case(world)
    desc, cam = c.geo.desc, c.geo.s.camera
    frame = rt.Frame.full(64, 48, 5)
    scene = rt.Scene(c.geo.s.world)
    lib = _capi.amd_lib()
    if what == "whitted":
        want, wcasts = _oracle.render_whitted(desc, cam, frame)
        assert (want.reshape(-1, 3).max(axis=1) > 0).mean() > 0.05, "the camera sees too little"
        for variant in (18, 2):
            _variant(variant)
            try:
                got, casts = rt.render_whitted_numpy(scene, cam, frame)
            finally:
                _variant(_capi.DEFAULT_VARIANT)
            same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
            assert same.all() and casts == wcasts, (variant, int((~same).sum()), casts, wcasts)
        return
    lib.rt_set_distributed_split(1 if what == "split" else 0)
    try:
        rng = rt.Rng(frame)
        samples = torch.empty((2, frame.rows, frame.cols, 3), dtype=torch.float32, device="cuda")
        valid = torch.empty((2, frame.rows, frame.cols), dtype=torch.uint8, device="cuda")
        cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        rt.render_distributed(scene, cam, frame, rng, 2, samples=samples, valid=valid, ray_count=cnt)
        torch.cuda.synchronize()
    finally:
        lib.rt_set_distributed_split(-1)
    st = _oracle.rng_init(frame)
    ws, wv, wcasts = _oracle.render_distributed(desc, cam, frame, st, 2)
    got = samples.cpu().numpy()
    same = (got.view(np.uint32) == ws.view(np.uint32)) | (np.isnan(got) & np.isnan(ws))
    assert same.all() and np.array_equal(valid.cpu().numpy(), wv) and int(cnt.item()) == wcasts, (int((~same).sum()), int(cnt.item()), wcasts)
    assert np.array_equal(rng.download(), st)
