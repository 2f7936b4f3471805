"""The tree loop on the device (include/rt_amd.h rt_tree_gate, rt_tree_split, rt_tree_spawn, rt_tree_gather, rt_tree_fold): every glue
kernel against a numpy restatement on one real level that holds every branch, and rt.trace_rays_levels — ray_trace written one level
of the recursion tree at a time from the public calls alone — against rt_trace_rays and against the oracle's orc_ray_trace: values
and cast count, on a stream of its own under torch's synchronisation check, with too small a level, on a scene walked breadth-first
and from a captured graph.  Everything is compared bit for bit as u32 words, NaN equal to NaN and -0.0 different from +0.0.  Every
parity test passes an explicit level capacity of min(n * 2^L, 8n) and asserts that the overflow word is 0: no ray is left out of a
comparison, and a level that did not fit fails instead of hiding."""
import ctypes as C

import numpy as np
import pytest

import homework_18_graphics_raytracer_amd as rt
import _oracle
import _hit_support as hq
from _records import dev, host, same_f32, source_b, tessellated_scene, torch_device, u32

pytestmark = pytest.mark.gpu
NONE = 0xFFFFFFFF
F32 = np.float32
T = F32(0.001)  # main.rs:467
SENTINEL = 0x5A5A5A5A


def _none_hits(n):
    h = np.zeros((n, 13), dtype=np.uint32)
    h[:, 0] = NONE
    return h


def _word(torch, value):
    return torch.tensor([value], dtype=torch.int64, device="cuda").to(torch.int32)


@pytest.fixture(scope="module")
def ref():
    torch = torch_device()
    world = rt.reference_world()
    desc = world.desc()
    cam = rt.camera_rays(rt.reference_camera(), rt.Frame.full(160, 90, 5))
    torch.cuda.synchronize()
    rays = np.concatenate([u32(cam), source_b(desc, 33, 3000)])
    return world, desc, rt.Scene(world), rays


def _material_table(desc):
    m = np.array([[desc.materials[i].shiness, desc.materials[i].transparency, desc.materials[i].opaque_decay] for i in range(desc.n_materials)],
                 dtype=np.float32)
    return m[:, 0], m[:, 1], m[:, 2]


# ---- 1. every glue kernel against numpy, on one real level ----

@pytest.mark.parametrize("depth_left", [1, 0])
def test_glue_kernels_against_numpy_on_every_branch(ref, depth_left):
    torch = torch_device()
    _, desc, scene, rays = ref
    live_n = rays.shape[0]
    pad = 150
    n = live_n + pad  # the capacity; the records at and beyond live_n are dead, and look alive: copies of real records
    g = np.random.default_rng(7)
    rays_all = np.concatenate([rays, rays[-pad:]])
    contribution = g.choice(np.array([1.0, 0.5, 0.002, 0.0005, np.nan, 0.0], dtype=np.float32), n, p=[0.55, 0.2, 0.1, 0.08, 0.05, 0.02]).astype(np.float32)
    contribution[live_n:] = F32(1.0)
    rays_t, con_t, count_t = dev(rays_all), torch.tensor(contribution, device="cuda"), _word(torch, live_n)
    alive = np.arange(n) < live_n

    # gate
    flags_t = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    hits_t = torch.full((n, 13), SENTINEL, dtype=torch.int32, device="cuda")
    rt.tree_gate(con_t, count_t, flags_t, hits_t)
    torch.cuda.synchronize()
    with np.errstate(invalid="ignore"):
        passed = alive & ~(contribution < T)
    assert np.array_equal(host(flags_t), passed.astype(np.uint8))
    assert np.array_equal(u32(hits_t), _none_hits(n))
    assert passed[np.isnan(contribution) & alive].all() and not passed[live_n:].any()
    flags_all, _ = rt.tree_gate(con_t)  # no count: the capacity
    torch.cuda.synchronize()
    with np.errstate(invalid="ignore"):
        assert np.array_equal(host(flags_all), (~(contribution < T)).astype(np.uint8))

    # the roots that passed are cast; the dead records get hits that look alive
    index_t, sel_t = rt.select_records(flags_t)
    rt.cast_rays_indexed(scene, rays_t, index_t, sel_t, hits_t)
    full = u32(rt.cast_rays(scene, rays_t))
    torch.cuda.synchronize()
    hits = u32(hits_t).copy()
    assert np.array_equal(hits, np.where(passed[:, None], full, _none_hits(n)))
    hits[live_n:] = full[live_n:]
    foreign = np.flatnonzero(passed & (hits[:, 0] <= 1))[5:25]  # records a caller got wrong: no hit
    hits[foreign[:10], 0] = 7
    hits[foreign[10:], 2] = desc.n_materials
    hits_t = dev(hits)

    # split
    shiness, transparency, decay_of = _material_table(desc)
    live = alive & (hits[:, 0] <= 1) & (hits[:, 2] < desc.n_materials)
    obj = np.where(live, hits[:, 2], 0)
    one = F32(1.0)
    sc = np.where(live, (one - shiness[obj]) * (one - transparency[obj]), F32(0.0)).astype(np.float32)
    rc = np.where(live, shiness[obj] * (one - transparency[obj]), F32(0.0)).astype(np.float32)
    fc = np.where(live, transparency[obj], F32(0.0)).astype(np.float32)
    decay = np.where(live, decay_of[obj], F32(0.0)).astype(np.float32)
    with np.errstate(invalid="ignore"):
        want_shade = live & (contribution * sc >= T)
        want_reflect = live & (depth_left > 0) & (contribution * rc >= T)
        want_refract = live & (depth_left > 0) & (contribution * fc > T)
    outs = [torch.full((n, 13), SENTINEL, dtype=torch.int32, device="cuda") for _ in range(3)]
    weights_t = torch.full((n, 4), 7.0, dtype=torch.float32, device="cuda")
    hs_t, hr_t, hf_t, _ = rt.tree_split(scene, hits_t, con_t, depth_left, count_t, outs[0], outs[1], outs[2], weights_t)
    torch.cuda.synchronize()
    for got, want, name in ((hs_t, want_shade, "shade"), (hr_t, want_reflect, "reflect"), (hf_t, want_refract, "refract")):
        assert np.array_equal(u32(got), np.where(want[:, None], hits, _none_hits(n))), name
    assert np.array_equal(u32(weights_t), np.stack([sc, rc, fc, decay], axis=1).view(np.uint32))

    # the three queries, then spawn
    cur = rt.shade_hits(scene, hs_t, rays_t)
    reflected_t = rt.reflect_rays(hr_t, rays_t)
    refr = rt.refract_rays(scene, hf_t, rays_t)
    sflags_t = torch.full((2 * n,), 9, dtype=torch.uint8, device="cuda")
    child_t = torch.full((2 * n, 3), 7.0, dtype=torch.float32, device="cuda")
    rt.tree_spawn(hr_t, refr.kind, sflags_t, child_t)
    torch.cuda.synchronize()
    kind = u32(refr.kind)
    escaped = kind == 0
    assert not (escaped & ~want_refract).any()
    want_flags = np.stack([want_reflect, escaped], axis=1).reshape(-1).astype(np.uint8)
    assert np.array_equal(host(sflags_t), want_flags)
    assert (u32(child_t) == 0).all()

    branches = {"shade only": live & want_shade & ~want_reflect & ~escaped, "reflection child": want_reflect, "refraction escaped": escaped,
                "refraction not escaped": want_refract & ~escaped, "a miss": passed & (hits[:, 0] == NONE), "a gated root": alive & ~passed,
                "NaN contribution": live & np.isnan(contribution), "shade not wanted": live & ~want_shade, "foreign record": alive & ~live & passed & (hits[:, 0] != NONE),
                "beyond the count": ~alive & (hits[:, 0] <= 1)}
    if depth_left <= 0:
        for name in ("reflection child", "refraction escaped", "refraction not escaped"):
            assert not branches.pop(name).any(), name
    sizes = {k: int(v.sum()) for k, v in branches.items()}
    print(f"depth_left {depth_left}: branches of the glue test:", sizes)
    assert all(v > 0 for v in sizes.values()), sizes

    # select + gather: everything fits, then too small a level
    cand_t, found_t = rt.select_records(sflags_t)
    torch.cuda.synchronize()
    cand = np.flatnonzero(want_flags)
    assert int(host(found_t)[0]) == cand.size and np.array_equal(host(cand_t)[:cand.size], cand.astype(np.int32))
    reflected, escape = u32(reflected_t), u32(refr.rays)

    def gather(max_count, index_t=cand_t, found=found_t, overflow0=3):
        cap = max(max_count, 1)
        out = (torch.full((cap, 11), SENTINEL, dtype=torch.int32, device="cuda"), torch.full((cap,), 7.0, dtype=torch.float32, device="cuda"),
               torch.full((cap,), SENTINEL, dtype=torch.int32, device="cuda"), torch.full((1,), SENTINEL, dtype=torch.int32, device="cuda"))
        overflow = _word(torch, overflow0)
        rt.tree_gather(index_t, found, reflected_t, refr.rays, con_t, weights_t, overflow, max_count, *out)
        torch.cuda.synchronize()
        return u32(out[0]), host(out[1]), u32(out[2]), int(host(out[3])[0]), int(host(overflow)[0]) - overflow0

    def check_gather(got, index, kept, what):
        c = index[:kept].astype(np.int64)
        ok = c < 2 * n
        p, slot = np.where(ok, c >> 1, 0), (c & 1).astype(bool)
        want_rays = np.where(ok[:, None], np.where(slot[:, None], escape[p], reflected[p]), 0).astype(np.uint32)
        with np.errstate(all="ignore"):
            want_con = np.where(ok, contribution[p] * np.where(slot, fc[p], rc[p]), F32(0.0)).astype(np.float32)
        assert np.array_equal(got[0][:kept], want_rays), what
        assert same_f32(got[1][:kept], want_con).all(), what
        assert np.array_equal(got[2][:kept], np.where(ok, c, NONE).astype(np.uint32)), what
        assert (got[0][kept:] == SENTINEL).all() and (got[2][kept:] == SENTINEL).all(), what  # beyond the count: not written
        assert got[3] == kept, what

    got = gather(2 * n)
    check_gather(got, cand, cand.size, "everything fits")
    assert got[4] == 0
    if cand.size:
        small = cand.size // 3 + 1
        got = gather(small)
        check_gather(got, cand, small, "a level too small")
        assert got[4] == cand.size - small
        got = gather(0)
        assert got[3] == 0 and got[4] == cand.size and (got[0] == SENTINEL).all()
        wild = np.concatenate([cand, np.zeros(2 * n - cand.size, dtype=cand.dtype)])  # the list has room for every candidate: 2n entries
        wild[::7] = 2 * n + g.integers(0, 1000, wild[::7].size)  # no candidate of this level
        wild[1] = NONE
        got = gather(2 * n, index_t=torch.tensor(wild.astype(np.uint32).view(np.int32), device="cuda"))
        check_gather(got, wild, cand.size, "indices that name no candidate")
        got = gather(2 * n, found=_word(torch, 5 * n))  # a count above the number of candidates there can be: clipped to 2n
        assert got[3] == 2 * n and got[4] == 0

    # fold: the children's values hold NaN, -0.0, infinities and subnormals
    child = g.normal(0.0, 1.0, (2 * n, 3)).astype(np.float32)
    child[g.random((2 * n, 3)) < 0.05] = np.nan
    child[g.random((2 * n, 3)) < 0.05] = F32(-0.0)
    child[g.random((2 * n, 3)) < 0.02] = np.inf
    child[g.random((2 * n, 3)) < 0.02] = F32(1e-41)
    child_t = torch.tensor(child, device="cuda")
    shade, travel = host(cur), host(refr.travel)
    live_fold = alive & (hits[:, 0] <= 1)  # the fold has no scene: a foreign object_index has black shade and zero weights
    want = np.zeros((n, 3), dtype=np.float32)
    with np.errstate(all="ignore"):
        if depth_left <= 0:
            want[live_fold] = shade[live_fold]
        else:
            power = hq._pow_host(decay, travel)
            reflection = child[0::2]
            refraction = np.where(escaped[:, None], child[1::2] * power[:, None], F32(0.0)).astype(np.float32)
            value = (shade * sc[:, None] + reflection * rc[:, None]) + refraction * fc[:, None]
            want[live_fold] = value[live_fold]

    def fold(parent_np, n_out, count=count_t):
        out = torch.full((n_out, 3), 7.0, dtype=torch.float32, device="cuda")
        parent = None if parent_np is None else torch.tensor(parent_np.astype(np.uint32).view(np.int32), device="cuda")
        below = depth_left > 0
        rt.tree_fold(hits_t, depth_left, cur, out, count, weights_t if below else None, refr.kind if below else None, refr.travel if below else None,
                     child_t if below else None, parent)
        torch.cuda.synchronize()
        return host(out)

    seven = np.full(3, 7.0, dtype=np.float32)
    got = fold(None, n)
    bad = np.flatnonzero(~same_f32(got[:live_n], want[:live_n]).all(axis=1))
    assert bad.size == 0, f"{bad.size} folded values differ, first {bad[:3]}: {got[bad[:2]]} want {want[bad[:2]]}"
    assert (got[live_n:] == seven).all()  # dead records write nothing
    assert (got[:live_n][~live_fold[:live_n]].view(np.uint32) == 0).all()  # black is +0.0
    slots = g.permutation(3 * n)[:n]  # every record its own slot of a larger array, as a child level has
    slots[11] = 3 * n + 5  # a parent outside the array: nothing is written
    slots[12] = NONE
    got = fold(slots, 3 * n)
    rows = np.setdiff1d(np.arange(live_n), [11, 12])
    assert same_f32(got[slots[rows]], want[rows]).all()
    rest = np.setdiff1d(np.arange(3 * n), slots[rows])
    assert (got[rest] == seven).all()
    got = fold(None, n, count=None)  # no count: the capacity
    live_all = hits[:, 0] <= 1
    with np.errstate(all="ignore"):
        want_all = np.where(live_all[:, None], shade if depth_left <= 0 else value, F32(0.0)).astype(np.float32)
    assert same_f32(got, want_all).all()


# ---- 2, 3. composition: trace_rays_levels == trace_rays == the oracle ----

def _capacity(n):
    return lambda level: min(n << level, 8 * n)


def _levels(scene, rays_t, depth, contribution, torch, stream=None, capacity=None, check=False, counts=None):
    n = rays_t.shape[0]
    out = torch.full((n, 3), 7.0, dtype=torch.float32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    overflow = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    if not check:
        torch.cuda.set_sync_debug_mode("error")  # any synchronising torch call inside the loop raises
    try:
        rt.trace_rays_levels(scene, rays_t, depth, contribution, out=out, ray_count=cnt, stream=stream,
                             level_capacity=capacity if capacity is not None else _capacity(n), check=check, overflow=overflow, level_counts=counts)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    return host(out), int(host(cnt)[0]), int(host(overflow)[0])


def _fused(scene, rays_t, depth, contribution, torch):
    """rt_trace_rays; a per-ray contribution as one call per distinct value"""
    n = rays_t.shape[0]
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    if not torch.is_tensor(contribution):
        out = rt.trace_rays(scene, rays_t, depth, contribution, ray_count=cnt)
        torch.cuda.synchronize()
        return host(out), int(host(cnt)[0])
    c = u32(contribution)
    out = np.zeros((n, 3), dtype=np.float32)
    for bits in np.unique(c):
        rows = np.flatnonzero(c == bits)
        part = rt.trace_rays(scene, rays_t[torch.tensor(rows, device="cuda")].contiguous(), depth, float(np.uint32(bits).view(np.float32)), ray_count=cnt)
        torch.cuda.synchronize()
        out[rows] = host(part)
    return out, int(host(cnt)[0])


def _assert_same(got, want, what):
    bad = np.flatnonzero(~same_f32(got[0], want[0]).all(axis=1))
    assert bad.size == 0, f"{what}: {bad.size} of {got[0].shape[0]} rays differ, first {bad[:5]}: {got[0][bad[:2]]} want {want[0][bad[:2]]}"
    assert got[1] == want[1], (what, "casts", got[1], want[1])


def _mixed(n, torch):
    g = np.random.default_rng(3)
    c = g.choice(np.array([1.0, 0.5, 0.0005, np.nan], dtype=np.float32), n).astype(np.float32)
    return torch.tensor(c, device="cuda")


@pytest.mark.parametrize("depth", [-3, 0, 1, 5, 8])
@pytest.mark.parametrize("contribution", [1.0, 0.5, 0.0005, float("nan"), "per ray"])
def test_levels_equal_trace_rays(ref, depth, contribution):
    """camera rays plus random rays, on a stream of their own, nothing read back and no synchronisation inside the loop"""
    torch = torch_device()
    _, _, scene, rays = ref
    rays_t = dev(rays)
    n = rays.shape[0]
    con = _mixed(n, torch) if contribution == "per ray" else contribution
    want = _fused(scene, rays_t, depth, con, torch)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    counts = torch.zeros(max(depth, 0) + 1, dtype=torch.int32, device="cuda")
    got = _levels(scene, rays_t, depth, con, torch, stream=side, counts=counts)
    print(f"depth {depth} contribution {contribution}: casts {got[1]} (rt_trace_rays {want[1]}), records per level {host(counts).tolist()} of {n}")
    assert got[2] == 0, ("overflow", got[2])
    _assert_same(got, want, (depth, contribution))
    if contribution == 0.0005:  # every root gated: black, nothing cast
        assert got[1] == 0 and (got[0].view(np.uint32) == 0).all()
    again = _levels(scene, rays_t, depth, con, torch, check=True)  # the default stream, the overflow word read back
    _assert_same(again, want, (depth, contribution, "default stream"))


@pytest.mark.parametrize("depth", [0, 5, 8])
def test_levels_equal_the_oracle(ref, depth):
    """a sample of the rays against orc_ray_trace directly, with a contribution per ray"""
    torch = torch_device()
    _, desc, scene, rays = ref
    g = np.random.default_rng(depth)
    rows = np.sort(g.choice(rays.shape[0], 2400, replace=False))
    sample = np.ascontiguousarray(rays[rows])
    con = g.choice(np.array([1.0, 0.5, 0.03, 0.0005], dtype=np.float32), rows.size).astype(np.float32)
    got = _levels(scene, dev(sample), depth, torch.tensor(con, device="cuda"), torch)
    assert got[2] == 0
    orays = (_oracle.OrcRay * rows.size).from_buffer(sample)
    want = np.zeros((rows.size, 3), dtype=np.float32)
    buf = (C.c_float * 3)()
    casts = C.c_uint64(0)
    total = 0
    lib = _oracle.lib()
    for i in range(rows.size):
        lib.orc_ray_trace(C.byref(desc), C.byref(orays[i]), depth, float(con[i]), buf, C.byref(casts))
        want[i] = np.frombuffer(buf, dtype=np.float32)
        total += casts.value
    _assert_same(got, (want, total), ("oracle", depth))


# ---- 4. a level that is too small ----

def test_overflow_is_counted_and_raised(ref):
    torch = torch_device()
    _, _, scene, rays = ref
    rays_t = dev(rays)
    n = rays.shape[0]
    want = _fused(scene, rays_t, 5, 1.0, torch)
    got = _levels(scene, rays_t, 5, 1.0, torch, capacity=n // 4)  # completes; the parents of the dropped children see black
    assert got[2] > 0
    assert not same_f32(got[0], want[0]).all() and got[1] < want[1]
    with pytest.raises(rt.RtError):
        _levels(scene, rays_t, 5, 1.0, torch, capacity=n // 4, check=True)
    with pytest.raises(rt.RtError):
        rt.trace_rays_levels(scene, rays_t, 5, level_capacity=lambda level: 0)  # no room for any child
    torch.cuda.synchronize()
    again = _levels(scene, rays_t, 5, 1.0, torch)
    assert again[2] == 0
    _assert_same(again, want, "after an overflow")


# ---- 5. a scene walked breadth-first ----

def test_levels_on_a_scene_walked_breadth_first(tmp_path):
    torch = torch_device()
    big, cam = tessellated_scene(tmp_path, 4)
    desc = big.desc()
    assert desc.n_triangles == 36 * 4 ** 4 + 28  # above rt_scene_create's default switch (8 192 triangles)
    with rt.options(RT_AMD_BFS_WALK_TRIANGLES=8192):  # read when the scene is created
        scene = rt.Scene(big)
    rays = np.concatenate([u32(rt.camera_rays(cam, rt.Frame.full(64, 48, 3))), source_b(desc, 52, 1000)])
    rays_t = dev(rays)
    n = rays.shape[0]
    want = _fused(scene, rays_t, 3, 1.0, torch)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    warm = torch.empty((8 * n, 13), dtype=torch.int32, device="cuda")
    with torch.cuda.stream(side):  # the one uncaptured call the indexed cast's record lists need on that stream, at the largest level's size
        flags = torch.ones(8 * n, dtype=torch.uint8, device="cuda")
        index, count = rt.select_records(flags, stream=side)
        rt.cast_rays_indexed(scene, rays_t.repeat(8, 1), index, count, warm, stream=side)
    side.synchronize()
    got = _levels(scene, rays_t, 3, 1.0, torch, stream=side)
    assert got[2] == 0
    _assert_same(got, want, "breadth-first scene")


# ---- 6. the whole loop in a graph ----

def test_levels_in_a_graph(ref):
    torch = torch_device()
    _, desc, scene, rays = ref
    rays_t = dev(rays)
    n = rays.shape[0]
    other = np.concatenate([rays[5000:], source_b(desc, 34, 5000)])
    assert other.shape[0] == n
    want, want_other = _fused(scene, rays_t, 5, 1.0, torch), _fused(scene, dev(other), 5, 1.0, torch)
    out = torch.full((n, 3), 7.0, dtype=torch.float32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    overflow = torch.zeros(1, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    run = lambda: rt.trace_rays_levels(scene, rays_t, 5, 1.0, out=out, ray_count=cnt, stream=stream, level_capacity=_capacity(n), check=False,
                                       overflow=overflow)
    with torch.cuda.stream(stream):
        run()  # uncaptured: the selection's scratch of this stream
        stream.synchronize()
        _assert_same((host(out), int(host(cnt)[0])), want, "uncaptured")
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            run()
    torch.cuda.synchronize()
    for replay, (source, expect) in enumerate(((rays, want), (other, want_other), (other, want_other))):
        rays_t.copy_(dev(source))
        out.fill_(7.0)
        cnt.zero_()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        _assert_same((host(out), int(host(cnt)[0])), expect, f"replay {replay}")
    assert int(host(overflow)[0]) == 0
