"""The level loop on the device (include/rt_amd.h rt_select_records, rt_cast_rays_indexed, rt_level_*): the selection against
numpy.flatnonzero, the indexed cast against rt_cast_rays, every glue kernel against a numpy restatement on records that hold every
branch, and rt.trace_rays_distributed_levels — the loop written from the public calls alone — against rt_trace_rays_distributed on
identically seeded generators: samples, flags, accumulated image, cast count and generator records, bit for bit; under torch's
synchronisation check and on a stream of its own.  Every comparison of floats is of bit patterns: -0.0 differs from +0.0; NaNs are
compared as bits where a kernel only moves them, as NaNs where it computes them."""
import numpy as np
import pytest

import homework_18_graphics_raytracer_amd as rt
import _scenes
import _scatter_support as sq
from _records import dev, host, same_f32, source_b, torch_device, u32

pytestmark = pytest.mark.gpu
NONE = 0xFFFFFFFF
F32 = np.float32


@pytest.fixture(scope="module")
def ref():
    world = rt.reference_world()
    desc = world.desc()
    rays, hits, classes = sq.chosen_rays(desc)
    return world, desc, rt.Scene(world), rays, hits, classes


# ---- selection ----

def _select(flags_np, torch):
    flags = torch.tensor(flags_np, device="cuda")
    n = flags_np.shape[0]
    index = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    count = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    rt.select_records(flags, index, count)
    torch.cuda.synchronize()
    return host(index), int(host(count)[0])


def _check_select(flags_np, torch, what):
    want = np.flatnonzero(flags_np)
    index, count = _select(flags_np, torch)
    assert count == want.size, (what, count, want.size)
    assert np.array_equal(index[:count], want.astype(np.int32)), what
    again, count2 = _select(flags_np, torch)
    assert count2 == count and np.array_equal(again[:count], index[:count]), what  # the same flags, the same output


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 256 * 5 + 1, 256 * 16 + 1, 4096, 4097, (1 << 22) + 37])
def test_selection_against_flatnonzero(n):
    torch = torch_device()
    g = np.random.default_rng(n)
    _check_select(np.zeros(n, dtype=np.uint8), torch, "all zero")
    _check_select(np.ones(n, dtype=np.uint8), torch, "all one")
    for density in (0.01, 0.5, 0.99):
        _check_select((g.random(n) < density).astype(np.uint8), torch, density)
    other = np.where(g.random(n) < 0.5, g.integers(2, 256, n), 0).astype(np.uint8)  # flag bytes other than 1
    _check_select(other, torch, "bytes other than 1")


def test_selection_on_an_unaligned_array_and_in_a_graph():
    torch = torch_device()
    g = np.random.default_rng(5)
    n = 10_001
    base = (g.random(n + 3) < 0.4).astype(np.uint8)
    whole = torch.tensor(base, device="cuda")
    for off in (1, 2, 3):  # the flags start off a dword boundary: the byte loads
        flags = whole[off:off + n]
        assert flags.data_ptr() % 4 == off and flags.is_contiguous()
        index, count = rt.select_records(flags)
        torch.cuda.synchronize()
        want = np.flatnonzero(base[off:off + n])
        assert int(host(count)[0]) == want.size and np.array_equal(host(index)[:want.size], want.astype(np.int32)), off
    # captured after an uncaptured call on the same stream; replayed on new flags
    flags = torch.tensor(base[:n], device="cuda")
    index = torch.zeros(n, dtype=torch.int32, device="cuda")
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        rt.select_records(flags, index, count)  # allocates the scratch of this stream
        stream.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            rt.select_records(flags, index, count)
    torch.cuda.synchronize()
    fresh = (g.random(n) < 0.7).astype(np.uint8)
    flags.copy_(torch.tensor(fresh, device="cuda"))
    index.fill_(-1)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    want = np.flatnonzero(fresh)
    assert int(host(count)[0]) == want.size and np.array_equal(host(index)[:want.size], want.astype(np.int32))


# ---- indexed cast ----

SENTINEL = 0x5A5A5A5A


def _indexed(scene, rays_t, index_np, count, max_count, torch):
    n = rays_t.shape[0]
    out = torch.full((n, 13), SENTINEL, dtype=torch.int32, device="cuda")
    index = torch.tensor(np.asarray(index_np, dtype=np.int64).astype(np.uint32).view(np.int32), device="cuda")
    cnt = torch.tensor([count], dtype=torch.int64, device="cuda").to(torch.int32)
    casts = torch.full((1,), 1000, dtype=torch.int64, device="cuda")
    rt.cast_rays_indexed(scene, rays_t, index, cnt, out, max_count=max_count, ray_count=casts)
    torch.cuda.synchronize()
    return u32(out), int(host(casts)[0]) - 1000


def _check_indexed(scene, rays, what, torch):
    n = rays.shape[0]
    rays_t = dev(rays)
    want = u32(rt.cast_rays(scene, rays_t))
    assert (want[:, 0] == NONE).sum() > 0 and (want[:, 0] != NONE).sum() > 0, what
    g = np.random.default_rng(11)
    sentinel = np.uint32(0x5A5A5A5A)

    def check(index, count, max_count, label):
        got, casts = _indexed(scene, rays_t, index, count, max_count, torch)
        used = np.asarray(index[:min(count, max_count)], dtype=np.int64)
        named = np.unique(used[(used >= 0) & (used < n)])
        rest = np.setdiff1d(np.arange(n), named)
        assert np.array_equal(got[named], want[named]), (what, label)  # bits, NaN distances included
        assert (got[rest] == sentinel).all(), (what, label)
        assert casts == int(((used >= 0) & (used < n)).sum()), (what, label, casts)

    subset = np.flatnonzero(g.random(n) < 0.37)
    check(subset, subset.size, subset.size, "ascending subset")
    perm = g.permutation(subset)
    check(perm, perm.size, perm.size, "permuted, duplicate-free")
    wild = perm.copy()
    wild[::5] = n + g.integers(0, 1000, wild[::5].size)  # out of range: skipped
    wild[3] = 0xFFFFFFFF
    check(wild, wild.size, wild.size, "out-of-range indices")
    check(perm, 0, perm.size, "device count 0")
    check(perm, perm.size + 999, perm.size - 70, "device count above max_count")
    check(perm, 65, perm.size, "one wave and a lane")


@pytest.mark.parametrize("wave_uniform", [None, 1])
@pytest.mark.parametrize("which", ["reference", "random 3", "random 8"])
def test_indexed_cast_against_cast_rays(ref, which, wave_uniform):
    torch = torch_device()
    if which == "reference":
        _, _, scene, rays, _, _ = ref
    else:
        world = _scenes.random_world(int(which.split()[1]), 40, 4)
        scene = rt.Scene(world)
        rays = source_b(world.desc(), 21, 3000)
    with rt.options(RT_AMD_QUERY_WAVE_UNIFORM=wave_uniform):
        _check_indexed(scene, rays, (which, wave_uniform), torch)


def test_indexed_cast_on_a_scene_walked_breadth_first(ref):
    torch = torch_device()
    world, _, _, rays, _, _ = ref
    with rt.options(RT_AMD_BFS_WALK_TRIANGLES=1):  # read when the scene is created
        scene = rt.Scene(world)
    _check_indexed(scene, rays, "breadth-first", torch)


# ---- glue and fold ----

def _alive(t, c):
    with np.errstate(invalid="ignore"):
        return (t != NONE) & ~(c <= 0)


def _none_hits(n):
    h = np.zeros((n, 13), dtype=np.uint32)
    h[:, 0] = NONE
    return h


def test_glue_and_fold_against_numpy_on_every_branch(ref):
    """one real level of the chosen batch (which takes every branch of main.rs:556-613), plus records a caller may hold: a NaN cosine,
    a cosine of -0.0, a dead record, a type that is none of the three"""
    torch = torch_device()
    _, _, scene, rays, _, _ = ref
    n = rays.shape[0]
    rays_t = dev(rays)
    hits_t = rt.cast_rays(scene, rays_t)
    rng, _ = sq.seeded(n)
    sc = rt.scatter_hits(scene, hits_t, rays_t, rng)
    torch.cuda.synchronize()
    t, c = u32(sc.type).copy(), host(sc.cosine).copy()
    live = np.flatnonzero(t != NONE)
    g = np.random.default_rng(2)
    nan_rows, negzero_rows, junk_rows = live[10:40], live[50:60], live[70:80]
    c[nan_rows] = np.nan
    c[negzero_rows] = F32(-0.0)
    t[junk_rows] = 3
    type_t, cos_t = dev(t), torch.tensor(c, device="cuda")
    hits = u32(hits_t)
    alive = _alive(t, c)
    dr, fr = alive & (t <= 1), alive & (t == 2)
    assert alive[nan_rows].all() and not alive[negzero_rows].any()

    # split
    h_refl_t, h_refr_t = rt.level_split(hits_t, type_t, cos_t)
    torch.cuda.synchronize()
    assert np.array_equal(u32(h_refl_t), np.where(dr[:, None], hits, _none_hits(n)))
    assert np.array_equal(u32(h_refr_t), np.where(fr[:, None], hits, _none_hits(n)))

    # join
    reflected_t = rt.reflect_rays(h_refl_t, sc.rays)
    refr = rt.refract_rays(scene, h_refr_t, sc.rays)
    next_t, next_hits_t, flags_t = rt.level_join(type_t, cos_t, reflected_t, refr.kind, refr.rays)
    torch.cuda.synchronize()
    kind = u32(refr.kind)
    escaped = fr & (kind == 0)
    to_cast = dr | escaped
    want_next = np.where(dr[:, None], u32(reflected_t), np.where(escaped[:, None], u32(refr.rays), 0)).astype(np.uint32)
    assert np.array_equal(u32(next_t), want_next)
    assert np.array_equal(host(flags_t), to_cast.astype(np.uint8))
    assert np.array_equal(u32(next_hits_t), _none_hits(n))

    # select + indexed cast, then close
    index, count = rt.select_records(flags_t)
    rt.cast_rays_indexed(scene, next_t, index, count, next_hits_t)
    closed_t = rt.level_close(hits_t, type_t, cos_t, next_hits_t)
    torch.cuda.synchronize()
    next_hits = u32(next_hits_t)
    full = u32(rt.cast_rays(scene, next_t))
    assert np.array_equal(next_hits, np.where(to_cast[:, None], full, _none_hits(n)))
    found = next_hits[:, 0] <= 1
    missed = dr & ~found
    assert np.array_equal(u32(closed_t), np.where(missed[:, None], hits, _none_hits(n)))

    branches = {"diffuse": alive & (t == 0), "reflection": alive & (t == 1), "refraction": fr, "black cosine": (t != NONE) & ~alive,
                "NaN cosine": np.isnan(c) & (t <= 2), "next hit": dr & found, "next miss": missed, "escaped-hit": escaped & found,
                "escaped-miss": escaped & ~found, "infinite": fr & (kind == 1), "trapped": fr & (kind == 2), "dead record": t == NONE}
    sizes = {k: int(v.sum()) for k, v in branches.items()}
    print("branches of the glue test:", sizes)
    assert all(v > 0 for v in sizes.values()), sizes

    # fold: real factors and shades, a value with NaN, -0.0, infinities and subnormals in it
    factor_t = rt.scatter_factors(scene, hits_t, rays_t, type_t, next_t, refr.travel)
    shade_next_t = rt.shade_hits(scene, next_hits_t, next_t)
    shade_missed_t = rt.shade_hits(scene, closed_t, sc.rays)
    value = g.normal(0.0, 1.0, (n, 3)).astype(np.float32)
    value[g.random((n, 3)) < 0.05] = np.nan
    value[g.random((n, 3)) < 0.05] = F32(-0.0)
    value[g.random((n, 3)) < 0.02] = np.inf
    value[g.random((n, 3)) < 0.02] = F32(1e-41)
    value_t = torch.tensor(value, device="cuda")
    torch.cuda.synchronize()
    factor, shade_next, shade_missed = host(factor_t), host(shade_next_t), host(shade_missed_t)
    rt.level_fold(type_t, cos_t, next_hits_t, factor_t, shade_next_t, shade_missed_t, value_t)
    torch.cuda.synchronize()
    want = np.zeros((n, 3), dtype=np.float32)
    half = F32(0.5)
    with np.errstate(all="ignore"):
        mix = dr & found
        s = value[mix] * factor[mix]
        want[mix] = shade_next[mix] + (s - shade_next[mix]) * half
        add = fr & found
        want[add] = (value[add] + shade_next[add]) * factor[add, 0:1]
        want[missed] = shade_missed[missed]
    got = host(value_t)
    bad = np.flatnonzero(~same_f32(got, want).all(axis=1))
    assert bad.size == 0, f"{bad.size} folded values differ, first {bad[:3]} types {t[bad[:3]]}: {got[bad[:2]]} want {want[bad[:2]]}"
    assert (got[~alive].view(np.uint32) == 0).all() and (got[junk_rows].view(np.uint32) == 0).all()  # black is +0.0

    # finish: filter and accumulation
    accum = g.normal(0.0, 1.0, (n, 3)).astype(np.float32)
    accum_t = torch.tensor(accum, device="cuda")
    valid_t = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    rt.level_finish(value_t, accum_t, valid_t)
    only_t = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    rt.level_finish(value_t, None, only_t)
    torch.cuda.synchronize()
    ok = sq.is_normal(got).all(axis=1)
    assert 0 < ok.sum() < n
    assert np.array_equal(host(valid_t), ok.astype(np.uint8)) and np.array_equal(host(only_t), ok.astype(np.uint8))
    with np.errstate(all="ignore"):
        want_accum = np.where(ok[:, None], accum + got, accum)
    assert np.array_equal(host(accum_t).view(np.uint32), want_accum.view(np.uint32))
    rng.close()


# ---- composition ----

def _fused(scene, rays_t, depth, rng, epochs, torch, accum0=None):
    n = rays_t.shape[0]
    samples = torch.full((epochs, n, 3), 7.0, dtype=torch.float32, device="cuda")
    valid = torch.full((epochs, n), 9, dtype=torch.uint8, device="cuda")
    accum = torch.zeros((n, 3), dtype=torch.float32, device="cuda") if accum0 is None else accum0.clone()
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    rt.trace_rays_distributed(scene, rays_t, depth, rng, epochs, accum=accum, samples=samples, valid=valid, ray_count=cnt)
    torch.cuda.synchronize()
    return host(samples), host(valid), host(accum), int(host(cnt)[0])


def _levels(scene, rays_t, depth, rng, epochs, torch, accum0=None, stream=None, checked=True):
    n = rays_t.shape[0]
    samples = torch.full((epochs, n, 3), 7.0, dtype=torch.float32, device="cuda")
    valid = torch.full((epochs, n), 9, dtype=torch.uint8, device="cuda")
    accum = torch.zeros((n, 3), dtype=torch.float32, device="cuda") if accum0 is None else accum0.clone()
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    if checked:
        torch.cuda.set_sync_debug_mode("error")  # any synchronising torch call inside the loop raises
    try:
        rt.trace_rays_distributed_levels(scene, rays_t, depth, rng, epochs, accum=accum, samples=samples, valid=valid, ray_count=cnt, stream=stream)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    return host(samples), host(valid), host(accum), int(host(cnt)[0])


def _same_run(a, b, what):
    bad = np.flatnonzero(~same_f32(a[0], b[0]).all(axis=2).all(axis=0))
    assert bad.size == 0, f"{what}: {bad.size} rays' samples differ, first {bad[:5]}: {a[0][:, bad[:2]]} want {b[0][:, bad[:2]]}"
    assert np.array_equal(a[1], b[1]), what
    assert same_f32(a[2], b[2]).all(), what
    assert a[3] == b[3], (what, a[3], b[3])


def _compose(scene, rays, depth, epochs, what):
    torch = torch_device()
    n = rays.shape[0]
    rays_t = dev(rays)
    rng_a, _ = sq.seeded(n)
    rng_b, _ = sq.seeded(n)
    want = _fused(scene, rays_t, depth, rng_b, epochs, torch)
    got = _levels(scene, rays_t, depth, rng_a, epochs, torch)
    print(f"{what} depth {depth}: casts {got[3]} (fused call {want[3]}), valid samples {int(got[1].sum())} of {got[1].size}")
    _same_run(got, want, (what, depth))
    assert np.array_equal(rng_a.download(), rng_b.download()), (what, depth)
    rng_a.close()
    rng_b.close()


@pytest.mark.parametrize("depth", [0, 1, 5, 8])
def test_levels_equal_the_fused_call_on_the_reference_scene(ref, depth):
    """the chosen-rays batch (every branch, by the oracle: test_gpu_scatter_queries) followed by a small frame's camera rays, 3 epochs"""
    _, _, scene, rays, _, _ = ref
    _compose(scene, rays, depth, 3, "reference scene")


@pytest.mark.parametrize("depth", [1, 8])
def test_levels_equal_the_fused_call_on_a_scene_walked_breadth_first(ref, depth):
    world, _, _, rays, _, _ = ref
    with rt.options(RT_AMD_BFS_WALK_TRIANGLES=1):
        scene = rt.Scene(world)
    _compose(scene, rays, depth, 3, "breadth-first scene")


def test_levels_fused_levels_on_one_rng(ref):
    """continuation: a levels call, a fused call and a levels call on one rt_rng equal three fused calls on its twin; accum goes on"""
    torch = torch_device()
    _, _, scene, rays, _, _ = ref
    rays_t = dev(rays)
    n = rays.shape[0]
    rng_a, _ = sq.seeded(n)
    rng_b, _ = sq.seeded(n)
    acc_a = acc_b = None
    for step, runner in enumerate((_levels, _fused, _levels)):
        got = runner(scene, rays_t, 5, rng_a, 2, torch, accum0=acc_a)
        want = _fused(scene, rays_t, 5, rng_b, 2, torch, accum0=acc_b)
        _same_run(got, want, ("continuation", step))
        assert np.array_equal(rng_a.download(), rng_b.download()), step
        acc_a, acc_b = torch.tensor(got[2], device="cuda"), torch.tensor(want[2], device="cuda")
    rng_a.close()
    rng_b.close()


def test_levels_on_a_stream_of_their_own_and_outputs_one_at_a_time(ref):
    """every library call on a non-default stream gives the same bits; so do accum alone and samples alone"""
    torch = torch_device()
    _, _, scene, rays, _, _ = ref
    rays_t = dev(rays)
    n = rays.shape[0]
    rng_a, _ = sq.seeded(n)
    rng_b, _ = sq.seeded(n)
    want = _levels(scene, rays_t, 5, rng_b, 2, torch)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    got = _levels(scene, rays_t, 5, rng_a, 2, torch, stream=side)
    _same_run(got, want, "side stream")
    assert np.array_equal(rng_a.download(), rng_b.download())
    rng_c, _ = sq.seeded(n)
    rng_d, _ = sq.seeded(n)
    accum = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
    rt.trace_rays_distributed_levels(scene, rays_t, 5, rng_c, 2, accum=accum)
    samples = torch.zeros((2, n, 3), dtype=torch.float32, device="cuda")
    rt.trace_rays_distributed_levels(scene, rays_t, 5, rng_d, 2, samples=samples)
    torch.cuda.synchronize()
    assert same_f32(host(accum), want[2]).all() and same_f32(host(samples), want[0]).all()
    for r in (rng_a, rng_b, rng_c, rng_d):
        r.close()
