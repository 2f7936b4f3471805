"""Mesh ordering on the device (include/rt_amd.h rt_triangle_keys, rt_order_triangles, rt_order_triangles_host): the keys against the
numpy restatement of tests/test_mesh_order_abi.py bit for bit; the permutation against two numpy stable argsorts, twice, gathered and
from a captured graph; and what the order is for — the shuffled sweep mesh in the literal scene, ordered on the device: the ordered
scene is bit-identical to the oracle's cast of the ORDERED description (rt_cast_rays, a Whitted frame and its cast count), and mapped
back through the permutation it agrees with the shuffled scene except where two triangles are hit at the same distance (the reference
keeps the later one, main.rs:229-233: a tie changes the triangle, never the distance).  Under the pair-wise and the wave-uniform walk
at 2 332 triangles and under the breadth-first walk at 9 244.  Floats are compared as bit patterns.

The seeds of the ray batches were kept after the same comparison between the oracle's casts of the two descriptions, on the CPU: at
2 332 triangles none of 23 100 records differ, at 9 244 triangles none of 7 500 (random rays do not meet an edge exactly), and the same
holds for the rays reflected off their hits."""
import ctypes as C

import numpy as np
import pytest

import homework_18_graphics_raytracer_amd as rt
import _oracle
import _hit_support as hq
import _mesh_order_support as mo
from _records import dev, ray_records, same_hits, source_b, torch_device, u32

pytestmark = pytest.mark.gpu
F32 = np.float32
SENTINEL = 0x5A5A5A5A
NONE = 0xFFFFFFFF


# ---- keys ----

def special_triangles():
    """64 hand-made triangles: NaN and infinite coordinates, centroids on box_lo, on box_hi and beyond both, -0.0, degenerate ones,
    then large random ones (most centroids outside the box)"""
    nan, inf = np.nan, np.inf
    lo, hi = mo.LO, mo.HI
    mid = (0.0, 1.0, 4.0)
    cases = [(lo, lo, lo), (hi, hi, hi), (mid, mid, mid), ((-3, 0, 0), (3, 0, 0), (0, 3, 12)), ((-9, 9, 4),) * 3, ((9, -9, 1e30),) * 3,
             ((nan, 0, 0), (0, inf, 0), (0, 0, -inf)), ((inf, 0, 0), (-inf, 0, 0), (0, 0, 0)), ((nan, nan, nan),) * 3,
             ((-0.0, -0.0, -0.0),) * 3, ((0.0, -0.0, 0.0), (-0.0, 0.0, -0.0), (0.0, 0.0, -0.0)), ((1e38, 1e38, 1e38),) * 3,
             ((-1e38, 3e38, 1.0), (-3e38, 3e38, 2.0), (-3e38, 3e38, 3.0)), ((1e-40, -1e-40, 1e-45),) * 3,
             (lo, hi, mid), (hi, lo, lo), ((2.0, 3.0, 8.0), (2.0, 3.0, 8.0), (1.9999999, 2.9999998, 7.9999995)),
             ((-2.0, -1.0, 0.0), (-2.0, -1.0, 0.0), (-2.0000002, -1.0000001, -1e-45))]
    g = np.random.default_rng(64)
    raw = np.concatenate([mo._triangle(*c, obj=k % 5) for k, c in enumerate(cases)])
    more = np.zeros((64 - raw.shape[0], 25), dtype=np.uint32)
    more[:, 0] = g.integers(0, 1 << 32, more.shape[0], dtype=np.uint64).astype(np.uint32)
    more[:, 1:] = g.normal(0, 4, (more.shape[0], 24)).astype(F32).view(np.uint32)
    return np.concatenate([raw, more])


KEY_BOXES = [(mo.LO, mo.HI), ((-2, 1, 0), (2, 1, 8)),            # a zero-extent axis: hi == lo
             ((-2, np.nan, 0), (2, 3, np.nan)),                  # NaN bounds
             ((0, 0, 0), (-1, np.inf, 1e-30)), ((-np.inf, -1, -1), (1, 1, 1))]


@pytest.mark.parametrize("n", [1, 64, 65, 2304 + 64])
def test_keys_equal_the_numpy_restatement(tmp_path, n):
    torch = torch_device()
    world, natural, _, mesh = mo.sweep(3, tmp_path)
    everything = np.concatenate([special_triangles(), natural[mesh]])
    assert everything.shape[0] == 2304 + 64
    raw = everything[:n]
    tris_t = dev(raw)
    for box in [world.bounds()] + KEY_BOXES:
        keys = torch.full((n + 1,), SENTINEL, dtype=torch.int32, device="cuda")
        objects = torch.full((n + 1,), SENTINEL, dtype=torch.int32, device="cuda")
        rt.triangle_keys(tris_t, box[0], box[1], out=keys[:n], objects=objects[:n])
        got, want = u32(keys), mo.numpy_keys(raw, box[0], box[1])
        bad = np.flatnonzero(got[:n] != want)
        assert bad.size == 0, (box, bad[:4], got[bad[:4]], want[bad[:4]], raw[bad[:2]])
        assert np.array_equal(u32(objects)[:n], raw[:, 0])
        assert got[n] == SENTINEL and u32(objects)[n] == SENTINEL
        assert np.array_equal(u32(rt.triangle_keys(tris_t, box[0], box[1]))[:n], want)  # without the object words
    if n > 2304:
        keys = mo.numpy_keys(raw[64:], *world.bounds())
        assert np.unique(keys).size > 500  # the mesh spreads over the grid: the key is not a constant


# ---- the permutation ----

def interleaved_objects(tmp_path):
    """three objects whose triangles are interleaved: two copies of the 2 304-triangle mesh at different offsets (objects 0 and 2) and
    five triangles of object 1"""
    _, natural, _, mesh = mo.sweep(3, tmp_path)
    a, b = natural[mesh].copy(), natural[mesh].copy()
    a[:, 0], b[:, 0] = 0, 2
    shift = np.asarray((1.75, -0.5, 0.25), dtype=F32)
    for v in range(3):
        b[:, 1 + 8 * v:4 + 8 * v] = (b[:, 1 + 8 * v:4 + 8 * v].view(F32) + shift).view(np.uint32)
    small = np.concatenate([mo._triangle((k, 0, 0), (k, 1, 0), (k, 0, 1), obj=1) for k in range(5)])
    raw = np.concatenate([a, small, b])
    return raw[np.random.default_rng(3).permutation(raw.shape[0])]


def test_permutation_of_interleaved_objects(tmp_path):
    torch = torch_device()
    raw = interleaved_objects(tmp_path)
    n = raw.shape[0]
    p = raw[:, 1:].copy().view(F32).reshape(n, 3, 8)[:, :, :3].reshape(-1, 3)
    lo, hi = p.min(0), p.max(0)
    want = mo.numpy_perm(raw, lo, hi, 3)
    tris_t = dev(raw)
    need = rt.order_triangles_temp_bytes(n)
    perm = torch.full((n + 1,), SENTINEL, dtype=torch.int32, device="cuda")
    ordered = torch.full((n + 1, 25), SENTINEL, dtype=torch.int32, device="cuda")
    temp = torch.full((need + 4,), 0x5A, dtype=torch.uint8, device="cuda")
    got = rt.order_triangles(tris_t, lo, hi, 3, out=perm[:n], ordered=ordered[:n], temp=temp[:need])
    first = u32(got).copy()
    assert np.array_equal(first, want), np.flatnonzero(first != want)[:5]
    assert np.array_equal(np.sort(first), np.arange(n, dtype=np.uint32))            # a permutation
    objects = raw[first, 0]
    assert (np.diff(objects.astype(np.int64)) >= 0).all() and np.bincount(objects).tolist() == [2304, 5, 2304]  # contiguous, ascending
    assert (np.diff(raw[first, 0] == 1) != 0).sum() == 2
    assert u32(ordered)[:n].tobytes() == raw[first].tobytes()                         # byte for byte
    assert u32(perm)[n] == SENTINEL and (u32(ordered)[n] == SENTINEL).all() and (temp[need:].cpu().numpy() == 0x5A).all()
    assert np.array_equal(u32(tris_t), raw)                                           # the input is only read
    # a second run, with a workspace of its own and no gather
    assert np.array_equal(u32(rt.order_triangles(tris_t, lo, hi, 3)), first)
    # the host form
    h_perm, h_ordered = np.zeros(n, dtype=np.uint32), np.zeros((n, 25), dtype=np.uint32)
    box = [(C.c_float * 3)(*[float(x) for x in v]) for v in (lo, hi)]
    rt._capi.check(rt._capi.amd_lib().rt_order_triangles_host(raw.ctypes.data_as(C.c_void_p), n, box[0], box[1], 3, h_perm.ctypes.data_as(C.c_void_p),
                                                              h_ordered.ctypes.data_as(C.c_void_p)))
    assert np.array_equal(h_perm, first) and np.array_equal(h_ordered, raw[first])
    # captured, without an earlier call on the stream, and replayed on other triangles
    perm.fill_(0)
    ordered.fill_(0)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            rt.order_triangles(tris_t, lo, hi, 3, out=perm[:n], ordered=ordered[:n], temp=temp[:need])
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(u32(perm)[:n], first) and u32(ordered)[:n].tobytes() == raw[first].tobytes()
    other = raw[np.random.default_rng(4).permutation(n)]
    tris_t.copy_(dev(other))
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    again = mo.numpy_perm(other, lo, hi, 3)
    assert np.array_equal(u32(perm)[:n], again) and u32(ordered)[:n].tobytes() == other[again].tobytes()


def test_world_ordered(tmp_path):
    world, natural, _, _ = mo.sweep(3, tmp_path)
    new, perm = world.ordered()
    d, e = world.desc(), new.desc()
    assert perm.dtype == np.uint32 and np.array_equal(perm, mo.numpy_perm(natural, *world.bounds(), d.n_materials))
    assert np.array_equal(mo.raw_of(e), natural[perm])
    for field, count, record in (("spheres", "n_spheres", rt._capi.Sphere), ("materials", "n_materials", rt._capi.Material),
                                 ("lights", "n_lights", rt._capi.Light)):
        assert getattr(d, count) == getattr(e, count)
        size = getattr(d, count) * C.sizeof(record)
        assert C.string_at(getattr(d, field), size) == C.string_at(getattr(e, field), size), field
    assert np.array_equal(mo.raw_of(d), natural)  # the world itself is unchanged
    box = ((-1.0, 0.0, -1.0), (2.0, 2.0, 1.0))
    assert np.array_equal(world.ordered(box)[1], mo.numpy_perm(natural, box[0], box[1], d.n_materials))


# ---- the scene ----

def grazing_rays(raw, seed, max_runs=100):
    """rays tangent to the bounding spheres of runs of 16 triangles — just inside, on, and at the margins the node test folds in"""
    g = np.random.default_rng(seed)
    v = raw[:, 1:].copy().view(F32).reshape(-1, 3, 8)[:, :, :3].astype(np.float64)
    runs = list(range(0, len(v), 16))
    origins, directions = [], []
    for lo in runs[::max(1, len(runs) // max_runs)]:
        p = v[lo:lo + 16].reshape(-1, 3)
        c = 0.5 * (p.min(0) + p.max(0))
        r = np.linalg.norm(p - c, axis=1).max()
        for scale in (0.97, 1.0, 1.0247, 1.05, 1.08):
            eye = c + g.normal(0, 1, (4, 3)) * 2.5
            u = np.cross(c - eye, g.normal(0, 1, (4, 3)))
            u /= np.linalg.norm(u, axis=1, keepdims=True)
            origins.append(eye)
            directions.append(c + r * scale * u - eye)
    o, d = np.concatenate(origins), np.concatenate(directions)
    return ray_records(o, d, g.integers(0, 3, len(o)))


LEVELS = {3: (20_000, rt.Frame.full(64, 36, 5)), 4: (5_000, rt.Frame.full(32, 18, 5))}
_cases = {}


def case(level, tmp_path):
    """the shuffled sweep scene, the device's order of it, the two scenes, and a batch of rays in both numberings"""
    if level not in _cases:
        torch = torch_device()
        world, natural, shuffled, mesh = mo.sweep(level, tmp_path)
        base = world.desc()
        lo, hi = world.bounds()
        ordered_t = torch.empty((shuffled.shape[0], 25), dtype=torch.int32, device="cuda")
        perm = u32(rt.order_triangles(dev(shuffled), lo, hi, base.n_materials, ordered=ordered_t)).copy()
        assert np.array_equal(perm, mo.numpy_perm(shuffled, lo, hi, base.n_materials))
        ordered = u32(ordered_t).copy()
        assert np.array_equal(ordered, shuffled[perm])
        c = type("Case", (), {})()
        c.perm, c.shuffled_desc, c.ordered_desc = perm, mo.desc_with(base, shuffled), mo.desc_with(base, ordered)
        c.shuffled_scene, c.ordered_scene = rt.Scene(c.shuffled_desc), rt.Scene(c.ordered_desc)
        c.rays_shuffled = np.concatenate([source_b(c.shuffled_desc, 500 + level, LEVELS[level][0]), grazing_rays(ordered, level),
                                          grazing_rays(shuffled, 10 + level, max_runs=8)])
        c.rays_ordered = rt.order_rays(c.rays_shuffled, perm).view(np.uint32).reshape(-1, 11)
        _cases[level] = c
    return _cases[level]


def assert_tie_rule(got, want, what):
    """records equal except at ties: where two records differ, both are hits with the same distance bits; at most 1 % differ"""
    got, want = np.asarray(got).view(np.uint32).reshape(-1, 13), np.asarray(want).view(np.uint32).reshape(-1, 13)
    differ = np.flatnonzero(~same_hits(got, want))
    print(f"{what}: {differ.size} of {got.shape[0]} records differ")
    bad = [i for i in differ if got[i, 0] == NONE or want[i, 0] == NONE or got[i, 12] != want[i, 12]]
    assert not bad, (what, len(bad), bad[:5], got[bad[:2]], want[bad[:2]])
    assert differ.size <= 0.01 * got.shape[0], (what, differ.size)
    return differ


def same_image(a, b):
    return ((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all()


@pytest.mark.parametrize("level", [3, 4])
def test_ordered_scene_equals_the_oracle_on_the_ordered_description(tmp_path, level):
    """level 3: 2 332 triangles, the pair-wise and the wave-uniform walk; level 4: 9 244, above RT_AMD_BFS_WALK_TRIANGLES, the
    breadth-first walk (and the wave-uniform one for the per-pixel kernel)"""
    c = case(level, tmp_path)
    assert c.ordered_desc.n_triangles == 36 * 4 ** level + 28
    want = hq.check(c.ordered_scene, c.ordered_desc, dev(c.rays_ordered), f"level {level}")  # default and wave-uniform, bit for bit
    assert (want[:, 0] == NONE).sum() > 0 and (want[:, 0] == rt.TRIANGLE).sum() > 1000
    camera, frame = rt.reference_camera(), LEVELS[level][1]
    image, casts = _oracle.render_whitted(c.ordered_desc, camera, frame)
    lib = rt._capi.amd_lib()
    for variant in (18, 2):
        rt._capi.check(lib.rt_set_variant(variant))
        try:
            got, got_casts = rt.render_whitted_numpy(c.ordered_scene, camera, frame)
        finally:
            rt._capi.check(lib.rt_set_variant(rt._capi.DEFAULT_VARIANT))
        assert same_image(got, image) and got_casts == casts, (level, variant, got_casts, casts)


@pytest.mark.parametrize("level", [3, 4])
def test_ordered_and_shuffled_scene_agree_except_at_ties(tmp_path, level):
    c = case(level, tmp_path)
    on_shuffled = u32(rt.cast_rays(c.shuffled_scene, dev(c.rays_shuffled)))
    on_ordered = u32(rt.cast_rays(c.ordered_scene, dev(c.rays_ordered)))
    back = rt.unorder_hits(on_ordered, c.perm)
    differ = assert_tie_rule(back, on_shuffled, f"level {level}")
    assert (on_shuffled[:, 0] == rt.TRIANGLE).sum() > 1000
    # the ordered scene's own numbering is another one: without the mapping most triangle hits name another triangle
    assert (on_ordered[:, 1] != on_shuffled[:, 1]).sum() > 1000 > differ.size


@pytest.mark.parametrize("level", [3, 4])
def test_exclusions_through_the_permutation(tmp_path, level):
    """rays reflected off hits on the shuffled scene exclude the triangle they leave: mapped forward with order_rays they must leave
    the same triangle of the ordered scene"""
    c = case(level, tmp_path)
    rays_t = dev(c.rays_shuffled)
    hits_t = rt.cast_rays(c.shuffled_scene, rays_t)
    reflected = u32(rt.reflect_rays(rt.Hits(hits_t), rays_t))
    live = u32(hits_t)[:, 0] != NONE
    reflected = reflected[live]
    assert (reflected[:, 7] != 0).all() and (reflected[:, 8] == rt.TRIANGLE).sum() > 1000
    want = u32(rt.cast_rays(c.shuffled_scene, dev(reflected)))
    forward = rt.order_rays(reflected, c.perm).view(np.uint32).reshape(-1, 11)
    on_triangle = reflected[:, 8] == rt.TRIANGLE
    assert np.array_equal(c.perm[forward[on_triangle, 9]], reflected[on_triangle, 9])
    assert np.array_equal(forward[~on_triangle], reflected[~on_triangle])
    got = rt.unorder_hits(u32(rt.cast_rays(c.ordered_scene, dev(forward))), c.perm)
    assert_tie_rule(got, want, f"level {level}, reflected")
    # without the mapping the exclusion names another triangle: some ray hits the surface it leaves
    unmapped = rt.unorder_hits(u32(rt.cast_rays(c.ordered_scene, dev(reflected))), c.perm).view(np.uint32).reshape(-1, 13)
    assert (~same_hits(unmapped, want)).sum() > (~same_hits(got.view(np.uint32).reshape(-1, 13), want)).sum()
