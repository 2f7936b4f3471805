"""Area-light queries on the device (include/rt_amd.h rt_area_light_rays / rt_area_light_terms / rt_area_light_fold) and the loop built
from them (arealights.shade_hits_soft).  With radius 0 they are the light queries and rt_shade_hits; with a radius every value is what
the light queries give for the scene whose lights were moved to the samples — samples that the CPU form of the sampler gives bit for
bit.  The batch is made on the CPU with the oracle, once per module.  Every comparison is of u32 words."""
import numpy as np
import pytest

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import arealights
from _area_light_support import POINT, displaced, make_batch, run_area
from _light_support import run_pieces
from _records import dev, host, torch_device

pytestmark = pytest.mark.gpu
UNIFORM, STRATIFIED = arealights.UNIFORM, arealights.STRATIFIED
RADII = (0.0, 0.3, 0.5, 0.05)
TILTED = (0.2, 0.3, 0.5, 0.05)  # the directional light without origin displaced as well


@pytest.fixture(scope="module")
def ref():
    return make_batch()


def words(a):
    """an array of 4-byte elements as u32 words; flags (uint8) as they are"""
    a = np.ascontiguousarray(a)
    return a if a.dtype.itemsize == 1 else a.view(np.uint32)


def same(a, b):
    a, b = words(a), words(b)
    return a.shape == b.shape and bool((a == b).all())


def first_difference(a, b):
    a, b = words(a).reshape(-1), words(b).reshape(-1)
    bad = np.flatnonzero(a != b)
    return f"{bad.size} of {a.size} words differ, first at {bad[:5]}: {a[bad[:5]]} want {b[bad[:5]]}"


def assert_same(got, want, what):
    assert same(got, want), f"{what}: {first_difference(got, want)}"


def fused(scene, hits_t, rays_t):
    torch = torch_device()
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    out = rt.shade_hits(scene, hits_t, rays_t, ray_count=cnt)
    torch.cuda.synchronize()
    return host(out), int(host(cnt)[0])


def soft(scene, hits_t, rays_t, radii, spp, pattern=STRATIFIED, seed=0, ids=None, lights_per_pass=None, visibility=False):
    """the loop, with every synchronising torch call inside it an error: no host visit hides there"""
    torch = torch_device()
    n = hits_t.shape[0]
    out = torch.full((n, 3), 7.0, dtype=torch.float32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    vis = torch.full((scene.n_lights * n,), 7.0, dtype=torch.float32, device="cuda") if visibility else None
    radii_t = torch.tensor(np.asarray(radii, dtype=np.float32), device="cuda")
    ids_t = None if ids is None else torch.tensor(np.asarray(ids).astype(np.uint32).view(np.int32), device="cuda")
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        arealights.shade_hits_soft(scene, hits_t, rays_t, radii_t, spp, pattern, seed, ids_t, out=out, visibility=vis, ray_count=cnt,
                                   lights_per_pass=lights_per_pass)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    return host(out), int(host(cnt)[0]), (None if vis is None else host(vis).reshape(scene.n_lights, n))


def area_fold(scene, hits_t, g, spp, visibility=True):
    torch = torch_device()
    n = hits_t.shape[0]
    asks, sample, sh, lit, dif, spe = g.t
    out = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
    vis = torch.full((lit.shape[0] // spp,), 7.0, dtype=torch.float32, device="cuda") if visibility else None
    arealights.fold(scene, hits_t, lit, dif, spe, out, spp, visibility=vis)
    torch.cuda.synchronize()
    return host(out), (None if vis is None else host(vis))


def test_radius_0_with_one_sample_is_the_light_queries(ref):
    """1. asks, shadow rays, lit, diffuse and specular are rt_light_rays' / rt_light_terms' word for word, the fold rt_light_fold's, and
    the loop rt_shade_hits' in values and cast count — on a batch with misses and with records a caller got wrong"""
    torch = torch_device()
    scene = rt.Scene(ref.world)
    n = ref.n
    hits_t, rays_t = dev(ref.foreign), dev(ref.rays)
    want = run_pieces(scene, hits_t, rays_t)
    for pattern in (UNIFORM, STRATIFIED):
        got = run_area(scene, hits_t, rays_t, [0.0] * 4, 1, pattern, seed=3)
        for name in ("asks", "shadow_rays", "shadow_hits", "lit", "diffuse", "specular"):
            assert_same(getattr(got, name), getattr(want, name), name)
        assert got.casts == want.casts > 0
        stored = np.array([ref.desc.lights[0].direction[:]] + [ref.desc.lights[l].origin[:] for l in (1, 2, 3)], dtype=np.float32)
        assert_same(got.sample.reshape(4, n, 3), np.broadcast_to(stored[:, None, :], (4, n, 3)), "sample")  # also for records that are no hit
    assert set(np.unique(got.asks)) <= {0, 1} and set(np.unique(got.lit)) <= {0, 1} and not (got.diffuse == 99.0).any()
    assert (got.asks.reshape(4, n)[:, ref.no_hit] == 0).all() and (got.shadow_rays.reshape(4, n, 11)[:, ref.no_hit] == 0).all()
    assert all((got.lit.reshape(4, n)[l] == 1).any() for l in range(4)) and (got.asks > got.lit).any()  # every light lights something; some pairs are occluded
    out = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
    out[torch.tensor(ref.no_hit, device="cuda")] = 99.0
    mine = out.clone()
    rt.light_fold(scene, hits_t, want.t[1], want.t[2], want.t[3], out)
    arealights.fold(scene, hits_t, got.t[3], got.t[4], got.t[5], mine, 1)
    torch.cuda.synchronize()
    assert_same(host(mine), host(out), "fold")
    assert (host(mine)[ref.no_hit] == 99.0).all()  # "no hit": not written
    want_out, want_casts = fused(scene, hits_t, rays_t)
    got_out, got_casts, _ = soft(scene, hits_t, rays_t, [0.0] * 4, 1, UNIFORM)
    assert_same(got_out, want_out, "shade_hits_soft against rt_shade_hits")
    assert got_casts == want_casts == want.casts


def test_radius_0_with_four_samples_is_shade_hits(ref):
    """2. four identical samples and an exact division by 4: rt_shade_hits' values, four times its casts"""
    torch_device()
    scene = rt.Scene(ref.world)
    hits_t, rays_t = dev(ref.foreign), dev(ref.rays)
    want_out, want_casts = fused(scene, hits_t, rays_t)
    for pattern in (UNIFORM, STRATIFIED):
        got_out, got_casts, vis = soft(scene, hits_t, rays_t, [0.0, -1.0, np.nan, 0.0], 4, pattern, seed=9, visibility=True)
        assert_same(got_out, want_out, f"pattern {pattern}")
        assert got_casts == 4 * want_casts
        assert set(np.unique(vis)) == {0.0, 1.0} and (vis[:, ref.no_hit] == 0.0).all()


@pytest.mark.parametrize("radii", [RADII, TILTED])
def test_the_samples_are_the_cpu_forms(ref, radii):
    """3. d_sample against rt_area_light_samples_cpu, word for word: distinct ids, uniform and stratified"""
    torch_device()
    scene = rt.Scene(ref.world)
    n = ref.n
    hits_t, rays_t = dev(ref.foreign), dev(ref.rays)
    ids = (np.arange(n, dtype=np.uint32) * np.uint32(2654435761)) ^ np.uint32(0x80000001)  # distinct, some above 2^31
    assert np.unique(ids).size == n
    for pattern in (UNIFORM, STRATIFIED):
        got = run_area(scene, hits_t, rays_t, radii, 4, pattern, seed=77, ids=ids)
        assert_same(got.sample.reshape(4, 4, n, 3), arealights.samples_numpy(ref.world, radii, n, 4, pattern, seed=77, ids=ids), f"pattern {pattern}")
    got = run_area(scene, hits_t, rays_t, radii, 4, UNIFORM, seed=77)  # ids None: the record's number
    assert_same(got.sample.reshape(4, 4, n, 3), arealights.samples_numpy(ref.world, radii, n, 4, UNIFORM, seed=77), "ids None")
    part = run_area(scene, hits_t, rays_t, radii[1:3], 4, UNIFORM, seed=77, first=1, count=2)
    for name in ("sample", "asks", "shadow_rays", "lit", "diffuse", "specular"):
        whole = getattr(got, name)
        assert_same(getattr(part, name), whole.reshape(4, 4, n, *whole.shape[1:])[:, 1:3].reshape(-1, *whole.shape[1:]), f"lights 1 .. 3: {name}")


def test_displaced_lights_against_the_light_queries(ref):
    """4. with one id for every record all records share the displacement of each (light, sample): plane s of the area outputs is
    rt_light_rays / rt_light_terms on the scene whose lights were moved there with Scene.update_lights.  Then three records of a run
    with distinct ids, against the runs whose constant id is theirs: the per-record path hangs on the same oracle"""
    torch_device()
    scene = rt.Scene(ref.world)
    n, spp, seed = ref.n, 4, 21
    hits_t, rays_t = dev(ref.foreign), dev(ref.rays)
    ids = np.arange(n, dtype=np.uint32) * np.uint32(7919) + np.uint32(11)
    distinct = run_area(scene, hits_t, rays_t, TILTED, spp, STRATIFIED, seed=seed, ids=ids)
    asked = np.flatnonzero((distinct.asks.reshape(spp, 4, n) == 1).all(axis=(0, 1)))
    records = asked[[0, asked.size // 2, -1]]  # lit by every light's every sample... at least asked for
    assert asked.size >= 3
    names = ("asks", "shadow_rays", "lit", "diffuse", "specular")
    planes = lambda a: a.reshape(spp, 4 * n, *a.shape[1:])
    stored = displaced(ref.desc, [ref.desc.lights[l].origin[:] if l else ref.desc.lights[0].direction[:] for l in range(4)])
    try:
        for constant, record in [(5, None)] + [(int(ids[r]), int(r)) for r in records]:
            got = run_area(scene, hits_t, rays_t, TILTED, spp, STRATIFIED, seed=seed, ids=np.full(n, constant, dtype=np.uint32))
            points = arealights.samples_numpy(ref.world, TILTED, 1, spp, STRATIFIED, seed=seed, ids=[constant])[:, :, 0]  # (spp, 4, 3)
            assert_same(got.sample.reshape(spp, 4, n, 3), np.broadcast_to(points[:, :, None, :], (spp, 4, n, 3)), f"id {constant}: sample")
            for s in range(spp):
                scene.update_lights(0, displaced(ref.desc, points[s]))
                want = run_pieces(scene, hits_t, rays_t)
                for name in names:
                    assert_same(planes(getattr(got, name))[s], getattr(want, name), f"id {constant}, sample {s}: {name}")
                assert (want.lit == 1).any() and (want.asks > want.lit).any()
            scene.update_lights(0, stored)  # the next run samples the lights as they were
            if record is not None:
                for name in names + ("sample",):
                    a, b = getattr(distinct, name), getattr(got, name)
                    entry = lambda x: x.reshape(spp, 4, n, *x.shape[1:])[:, :, record]
                    assert_same(entry(a), entry(b), f"record {record} of the distinct-ids run: {name}")
        assert not same(planes(got.shadow_rays)[0], planes(got.shadow_rays)[1])  # the samples differ
    finally:
        scene.update_lights(0, stored)
    back = run_area(scene, hits_t, rays_t, [0.0] * 4, 1, UNIFORM)
    fresh = run_area(rt.Scene(ref.world), hits_t, rays_t, [0.0] * 4, 1, UNIFORM)
    assert_same(back.diffuse, fresh.diffuse, "the lights are restored")


def test_ranges_of_lights_give_the_same_sum(ref):
    """5. lights_per_pass 1, 2 and all: the same words"""
    torch_device()
    scene = rt.Scene(ref.world)
    hits_t, rays_t = dev(ref.foreign), dev(ref.rays)
    ids = np.arange(ref.n) * 3 + 1
    whole = soft(scene, hits_t, rays_t, TILTED, 4, STRATIFIED, seed=5, ids=ids, visibility=True)
    assert not same(whole[0], fused(scene, hits_t, rays_t)[0])
    for per_pass in (1, 2, 3):
        part = soft(scene, hits_t, rays_t, TILTED, 4, STRATIFIED, seed=5, ids=ids, lights_per_pass=per_pass, visibility=True)
        assert_same(part[0], whole[0], f"lights_per_pass={per_pass}: out")
        assert_same(part[2], whole[2], f"lights_per_pass={per_pass}: visibility")
        assert part[1] == whole[1]


def numpy_fold(shiness, valid, lit, diffuse, specular, spp, lights, n):
    """the definition, in f32 operations in the stated order"""
    lit, diffuse, specular = lit.reshape(spp, lights, n), diffuse.reshape(spp, lights, n, 3), specular.reshape(spp, lights, n, 3)
    out, vis = np.zeros((n, 3), dtype=np.float32), np.zeros((lights, n), dtype=np.float32)
    one, count = np.float32(1.0), np.float32(spp)
    for i in np.flatnonzero(valid):
        total = np.zeros(3, dtype=np.float32)
        for l in range(lights):
            acc_d = acc_s = None
            k = 0
            for s in range(spp):
                if lit[s, l, i]:
                    acc_d = diffuse[s, l, i] if acc_d is None else acc_d + diffuse[s, l, i]
                    acc_s = specular[s, l, i] if acc_s is None else acc_s + specular[s, l, i]
                    k += 1
            vis[l, i] = np.float32(k) / count
            if k:
                total = (total + (acc_d / count) * (one - shiness[i])) + (acc_s / count) * shiness[i]
        out[i] = total
    return out, vis


def test_the_fold_is_its_definition(ref):
    """6. a numpy restatement on the device's lit / diffuse / specular gives out and visibility word for word; the floor hits hold
    records whose point light has some samples unlit and records with all of them unlit"""
    torch_device()
    scene = rt.Scene(ref.world)
    for hits, rays, spp in ((np.concatenate([ref.floor_hits, ref.hits[:200]]), np.concatenate([ref.floor_rays, ref.rays[:200]]), 16),
                            (ref.hits, ref.rays, 4)):
        n = hits.shape[0]
        hits_t = dev(hits)
        g = run_area(scene, hits_t, dev(rays), RADII, spp, STRATIFIED, seed=1, ids=np.arange(n) + 100)
        out, vis = area_fold(scene, hits_t, g, spp)
        valid = (hits[:, 0] <= 1) & (hits[:, 2] < ref.desc.n_materials)
        shiness = np.array([ref.desc.materials[int(o)].shiness if v else 0.0 for o, v in zip(hits[:, 2], valid)], dtype=np.float32)
        want_out, want_vis = numpy_fold(shiness, valid, g.lit, g.diffuse, g.specular, spp, 4, n)
        assert_same(out, want_out, f"{n} records, spp {spp}: out")
        assert_same(vis.reshape(4, n), want_vis, f"{n} records, spp {spp}: visibility")
        if spp == 16:
            point = want_vis[POINT, :ref.floor_hits.shape[0]]
            assert ((point > 0) & (point < 1)).any() and (point == 0).any() and (point == 1).any(), point
        assert (want_vis[:, ~valid] == 0).all()
        out2, none = area_fold(scene, hits_t, g, spp, visibility=False)  # d_visibility NULL
        assert none is None and same(out2, out)


def test_caller_written_samples(ref):
    """7. d_sample is the caller's: a fixed point for one light changes that light's terms only"""
    torch_device()
    scene = rt.Scene(ref.world)
    n, spp = ref.n, 4
    hits_t, rays_t = dev(ref.hits), dev(ref.rays)
    base = run_area(scene, hits_t, rays_t, RADII, spp, UNIFORM, seed=2)
    own = base.sample.reshape(spp, 4, n, 3).copy()
    own[:, 2] = np.array([1.5, 3.5, 1.0], dtype=np.float32)  # the spot light, somewhere else
    g = run_area(scene, hits_t, rays_t, RADII, spp, UNIFORM, seed=2, sample_override=own.reshape(-1, 3))
    entries = lambda a: a.reshape(spp, 4, n, *a.shape[1:])
    changed = False
    for name in ("lit", "diffuse", "specular"):
        a, b = entries(getattr(base, name)), entries(getattr(g, name))
        for l in (0, 1, 3):
            assert_same(b[:, l], a[:, l], f"light {l}: {name}")
        changed |= not same(b[:, 2], a[:, 2])
    assert changed


def test_a_penumbra_under_the_occluder(ref):
    """8. the point light above the box, hits on the floor, 16 stratified samples: hard with radius 0, soft with radius 0.5"""
    torch_device()
    scene = rt.Scene(ref.world)
    hits_t, rays_t = dev(ref.floor_hits), dev(ref.floor_rays)
    ids = np.arange(ref.floor_hits.shape[0]) + 1000
    hard = soft(scene, hits_t, rays_t, [0.0] * 4, 16, STRATIFIED, seed=8, ids=ids, visibility=True)[2][POINT]
    assert set(np.unique(hard)) == {0.0, 1.0}, np.unique(hard)
    radii = [0.0, 0.0, 0.0, 0.5]
    out, casts, vis = soft(scene, hits_t, rays_t, radii, 16, STRATIFIED, seed=8, ids=ids, visibility=True)
    point = vis[POINT]
    print("visibility of the point light along x:", dict(zip(np.round(ref.floor_x[:41], 2).tolist(), point[:41].tolist())))
    assert ((point > 0.0) & (point < 1.0)).any()
    assert (point[np.abs(ref.floor_x) >= 1.6] == 1.0).all() and (point[np.abs(ref.floor_x) <= 0.2] == 0.0).all()
    assert set(np.unique(point * 16)) <= set(range(17))
    again = soft(scene, hits_t, rays_t, radii, 16, STRATIFIED, seed=8, ids=ids, visibility=True)
    assert same(again[0], out) and same(again[2], vis) and again[1] == casts  # the same bits on every run
    other = soft(scene, hits_t, rays_t, radii, 16, STRATIFIED, seed=9, ids=ids, visibility=True)
    assert not same(other[0], out)


def test_the_three_calls_in_a_graph(ref):
    """9. rays, terms and fold captured into one graph on a side stream; replayed onto cleared outputs they give the eager results"""
    torch = torch_device()
    scene = rt.Scene(ref.world)
    n, spp = ref.n, 4
    hits_t, rays_t = dev(ref.foreign), dev(ref.rays)
    eager = run_area(scene, hits_t, rays_t, TILTED, spp, STRATIFIED, seed=6)
    eager_out, eager_vis = area_fold(scene, hits_t, eager, spp)
    asks, sample, sh, lit, dif, spe = (t.clone() for t in eager.t)
    sr = torch.empty((asks.shape[0], 11), dtype=torch.int32, device="cuda")
    radii_t = torch.tensor(np.asarray(TILTED, dtype=np.float32), device="cuda")
    out = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
    vis = torch.zeros((4 * n,), dtype=torch.float32, device="cuda")
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            arealights.rays(scene, hits_t, rays_t, radii_t, spp, STRATIFIED, 6, None, out_rays=sr, out_asks=asks, out_sample=sample, stream=stream)
            arealights.terms(scene, hits_t, rays_t, asks, sample, sh, spp, out_lit=lit, out_diffuse=dif, out_specular=spe, stream=stream)
            arealights.fold(scene, hits_t, lit, dif, spe, out, spp, visibility=vis, stream=stream)
    torch.cuda.synchronize()
    for t in (sr, asks, sample, lit, dif, spe, out, vis):
        t.zero_()
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    for name, t in (("shadow_rays", sr), ("asks", asks), ("sample", sample), ("lit", lit), ("diffuse", dif), ("specular", spe)):
        assert_same(host(t), getattr(eager, name), f"replay: {name}")
    assert_same(host(out), eager_out, "replay: out")
    assert_same(host(vis), eager_vis, "replay: visibility")
