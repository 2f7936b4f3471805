"""Light queries on the device (include/rt_amd.h rt_light_rays / rt_light_terms / rt_light_fold) and the loop built from them
(rt.shade_hits_by_light): the loop against rt_shade_hits and the oracle's orc_get_shade, values and cast count; the pieces against the
oracle light by light; a caller's subset of lights; records a caller got wrong; other scenes; a scene walked breadth-first; graph
capture.  The batches and everything expected of them are made on the CPU with the oracle alone, once per module.  Every comparison is
of f32 bit patterns: any NaN equals any NaN, -0.0 differs from +0.0."""
import ctypes as C

import numpy as np
import pytest

import homework_18_graphics_raytracer_amd as rt
import _oracle
import _scenes
from _light_support import dist32, make_batch, oracle_shade, reference_rays, run_pieces, with_lights
from _records import camera_rays_cpu, dev, host, same_f32, same_rays, source_b, tessellated_scene, torch_device, valid_rows

pytestmark = pytest.mark.gpu
NONE = 0xFFFFFFFF
BACK = 1


# ---- the expected side: the oracle alone, on the CPU ----


@pytest.fixture(scope="module")
def ref():
    world = rt.reference_world()
    b = make_batch(world, reference_rays(world.desc()), per_light=True)
    b.world = world
    assert 2500 <= b.valid.sum() <= 3500, b.valid.sum()
    # the whole scene lies inside the spot light's cone (60 degrees from (0, 10, 0) downwards): the few hits outside it are far-away ones
    spot = [l for l in range(b.desc.n_lights) if b.desc.lights[l].kind == 1][0]
    b.outside_cone = np.flatnonzero(b.valid & ~light_of(b.desc, spot, b.hits[:, 3:6].view(np.float32))[0])
    assert b.outside_cone.size >= 3, b.outside_cone
    return b


# ---- the device side ----


def fused(scene, hits_t, rays_t):
    torch = torch_device()
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    out = rt.shade_hits(scene, hits_t, rays_t, ray_count=cnt)
    torch.cuda.synchronize()
    return host(out), int(host(cnt)[0])


def by_light(scene, hits_t, rays_t, lights_per_pass=None, stream=None):
    """the loop, with every synchronising torch call inside it an error: no host visit hides there"""
    torch = torch_device()
    n = hits_t.shape[0]
    out = torch.full((n, 3), 7.0, dtype=torch.float32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        rt.shade_hits_by_light(scene, hits_t, rays_t, out=out, ray_count=cnt, stream=stream, lights_per_pass=lights_per_pass)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    return host(out), int(host(cnt)[0])


def assert_shade(got, want, what):
    bad = np.flatnonzero(~same_f32(got[0], want[0]).all(axis=1))
    assert bad.size == 0, f"{what}: {bad.size} of {want[0].shape[0]} differ, first rows {bad[:5]}: {got[0][bad[:2]]} want {want[0][bad[:2]]}"
    assert got[1] == want[1], (what, "casts", got[1], want[1])


def assert_identity(scene, b, rows, what, passes=(None, 1)):
    hits_t, rays_t = dev(b.hits[rows]), dev(b.rays[rows])
    want = (b.shade[rows], int(b.casts[rows].sum()))
    assert_shade(fused(scene, hits_t, rays_t), want, f"{what}: rt_shade_hits against the oracle")
    for per_pass in passes:
        assert_shade(by_light(scene, hits_t, rays_t, per_pass), want, f"{what}: the loop, lights_per_pass={per_pass}")


@pytest.mark.parametrize("size", [1, 63, 64, 65, 4011])
def test_the_loop_is_shade_hits(ref, size):
    """1. shade_hits_by_light == rt.shade_hits == orc_get_shade, values and cast count, with all lights in one pass and with one light
    per pass; the smaller batches are taken with a stride, so that each holds camera, random and inside-the-glass records"""
    torch_device()
    scene = rt.Scene(ref.world)
    rows = np.arange(size) * (ref.n // size)
    if size == 1:
        rows = np.flatnonzero(ref.casts == ref.casts.max())[:1]  # one record that casts for as many lights as any does
    assert ref.valid[rows].any() and ref.casts[rows].sum() > 0
    assert_identity(scene, ref, rows, f"{size} records")


def light_of(desc, l, positions):
    """orc_light_directional at every position: (some, direction, has_origin, origin)"""
    lib = _oracle.lib()
    n = positions.shape[0]
    some, direction = np.zeros(n, dtype=bool), np.zeros((n, 3), dtype=np.float32)
    has_origin, origin = np.zeros(n, dtype=bool), np.zeros((n, 3), dtype=np.float32)
    d, c, o, h = (C.c_float * 3)(), (C.c_float * 3)(), (C.c_float * 3)(), C.c_int(0)
    light = desc.lights[l]
    for i in range(n):
        p = (C.c_float * 3)(*positions[i])
        if lib.orc_light_directional(C.byref(light), p, d, c, o, C.byref(h)):
            some[i], direction[i], has_origin[i], origin[i] = True, d[:], bool(h.value), o[:]
    return some, direction, has_origin, origin


def test_the_pieces_against_the_oracle(ref):
    """2. per light: the flags are the cast counts of orc_get_shade on the scene holding that light alone; the shadow rays are made of
    the hit and orc_light_directional; d_lit is the reference's occlusion rule evaluated with orc_cast of that ray; the two terms,
    weighted in numpy f32, are that one-light scene's orc_get_shade"""
    torch_device()
    desc, n = ref.desc, ref.n
    scene = rt.Scene(ref.world)
    assert desc.n_lights == 3 and sorted(desc.lights[l].kind for l in range(3)) == [0, 1, 2]  # one light of each kind
    g = run_pieces(scene, dev(ref.hits), dev(ref.rays))
    pos = ref.hits[:, 3:6].view(np.float32)
    shiness = np.array([desc.materials[int(o)].shiness if v else 0.0 for o, v in zip(ref.hits[:, 2], ref.valid)], dtype=np.float32)
    lib = _oracle.lib()
    total = 0
    for l in range(3):
        plane = slice(l * n, (l + 1) * n)
        asks, rays_l = g.asks[plane], g.shadow_rays[plane]
        alone_shade, alone_casts = ref.alone[l]
        assert set(np.unique(alone_casts)) <= {0, 1}
        assert np.array_equal(asks, alone_casts.astype(np.uint8)), (l, np.flatnonzero(asks != alone_casts)[:5])
        a = np.flatnonzero(asks == 1)
        total += a.size
        some, direction, has_origin, origin = light_of(desc, l, pos)
        assert some[a].all()
        want_rays = np.zeros((n, 11), dtype=np.uint32)
        want_rays[a, 0:3] = ref.hits[a, 3:6]  # origin = the hit's position
        want_rays[a, 3:6] = (-direction[a]).view(np.uint32)  # direction = -light.direction
        want_rays[a, 6], want_rays[a, 7], want_rays[a, 10] = BACK, 1, BACK
        want_rays[a, 8], want_rays[a, 9] = ref.hits[a, 0], ref.hits[a, 1]  # the exclusion is the hit's primitive
        bad = np.flatnonzero(~same_rays(rays_l, want_rays))
        assert bad.size == 0, (l, bad[:5], rays_l[bad[:1]], want_rays[bad[:1]])
        want_dist = np.where(has_origin, dist32(pos, origin), np.float32(np.inf)).astype(np.float32)
        want_dist[asks == 0] = 0.0
        assert same_f32(g.distance[plane], want_dist).all(), l
        # the reference's rule (main.rs:435-448) with the oracle's cast of that ray
        occluded = np.zeros(n, dtype=bool)
        orays = (_oracle.OrcRay * n).from_buffer(rays_l.copy())
        h = _oracle.OrcHit()
        for i in a:
            if lib.orc_cast(C.byref(desc), C.byref(orays[i]), C.byref(h)):
                occluded[i] = (not has_origin[i]) or bool(dist32(pos[i], np.array(h.position[:], dtype=np.float32)) < dist32(pos[i], origin[i]))
        want_lit = (asks == 1) & ~occluded
        assert np.array_equal(g.lit[plane], want_lit.astype(np.uint8)), (l, np.flatnonzero(g.lit[plane] != want_lit)[:5])
        dark = ~want_lit
        assert (g.diffuse[plane][dark].view(np.uint32) == 0).all() and (g.specular[plane][dark].view(np.uint32) == 0).all(), l
        with np.errstate(all="ignore"):
            one = np.float32(1.0)
            mine = (np.float32(0.0) + g.diffuse[plane] * (one - shiness)[:, None]) + g.specular[plane] * shiness[:, None]
        bad = np.flatnonzero(ref.valid & ~same_f32(mine, alone_shade).all(axis=1))
        assert bad.size == 0, (l, bad[:5], mine[bad[:2]], alone_shade[bad[:2]])
        # the batch holds what it was chosen for
        kinds = {"lit": int(want_lit.sum()), "occluded": int(((asks == 1) & occluded).sum()), "not asked": int((ref.valid & (asks == 0)).sum())}
        if desc.lights[l].kind == 1:
            kinds["outside the cone"] = int((ref.valid & ~some).sum())
        print(f"light {l} kind {desc.lights[l].kind}: {kinds} of {int(ref.valid.sum())} hits")
        assert all(v > 0 for v in kinds.values()), (l, kinds)
    assert g.casts == total == int(ref.casts.sum())  # the outside check of the shadow-cast count: the existing cast call counted them
    assert (g.asks.reshape(3, n)[:, ~ref.valid] == 0).all() and (g.lit.reshape(3, n)[:, ~ref.valid] == 0).all()


def fold(scene, hits_t, g_t, n, rgb=None):
    torch = torch_device()
    asks, lit, dif, spe = g_t
    out = torch.zeros((n, 3), dtype=torch.float32, device="cuda") if rgb is None else rgb
    rt.light_fold(scene, hits_t, lit, dif, spe, out)
    torch.cuda.synchronize()
    return host(out)


def test_a_subset_of_lights(ref):
    """3. a caller's light linking: with one light's flags zeroed the fold is orc_get_shade on the scene without that light"""
    torch_device()
    n = ref.n
    scene = rt.Scene(ref.world)
    hits_t, rays_t = dev(ref.hits), dev(ref.rays)
    base = run_pieces(scene, hits_t, rays_t)
    for drop in range(3):
        asks = base.asks.copy()
        asks[drop * n:(drop + 1) * n] = 0
        g = run_pieces(scene, hits_t, rays_t, asks_override=asks)
        want = oracle_shade(with_lights(ref.desc, [l for l in range(3) if l != drop]), ref.rays, ref.hits)
        assert_shade((fold(scene, hits_t, g.t, n), g.casts), (want[0], int(want[1].sum())), f"without light {drop}")
        assert (g.lit[drop * n:(drop + 1) * n] == 0).all()


def test_foreign_records(ref):
    """4. records a caller got wrong, outputs filled with a sentinel first.  Validation, not an attempt at a fault: nothing in the
    kernels is indexed with an unchecked field"""
    torch = torch_device()
    desc = ref.desc
    scene = rt.Scene(ref.world)
    rows = np.flatnonzero(ref.valid & (ref.casts > 0))[:: 29][:65]  # one full wave plus one lane
    assert rows.size == 65
    rows[[1, 2, 5]] = ref.outside_cone[:3]  # with hits outside the spot light's cone among them
    rays, hits = ref.rays[rows].copy(), ref.hits[rows].copy()
    nan, inf = (np.array([v], dtype=np.float32).view(np.uint32)[0] for v in (np.nan, np.inf))
    hits[3, 0] = 7                      # kind 7: no hit
    hits[10, 2] = desc.n_materials      # object_index >= n_materials: no hit
    hits[64, 0] = NONE                  # a miss, in the tail wave
    hits[20, 11] = 5                    # face 5: read as Back
    hits[30, 1] = 0x7FFFFFF0            # an index outside its array: only ever an exclusion, and as one excludes nothing
    hits[40, 3:6] = nan
    hits[41, 3:6] = inf
    hits[42, 6:9] = nan
    hits[43, 6:9] = inf
    no_hit = np.array([3, 10, 64])
    n = 65
    hits_t, rays_t = dev(hits), dev(rays)
    g = run_pieces(scene, hits_t, rays_t)
    planes = lambda a: a.reshape(3, n, *a.shape[1:])
    assert (planes(g.asks)[:, no_hit] == 0).all() and (planes(g.shadow_rays)[:, no_hit] == 0).all() and (planes(g.distance)[:, no_hit] == 0).all()
    assert (planes(g.lit)[:, no_hit] == 0).all()
    assert (planes(g.diffuse)[:, no_hit].view(np.uint32) == 0).all() and (planes(g.specular)[:, no_hit].view(np.uint32) == 0).all()
    assert set(np.unique(g.asks)) <= {0, 1} and set(np.unique(g.lit)) <= {0, 1}  # no sentinel left anywhere
    assert not (g.shadow_rays == 0x5A5A5A5A).any() and not (g.diffuse == 99.0).any() and not (g.specular == 99.0).any()
    # the fold adds to the valid records and leaves the others alone
    rgb = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
    rgb[torch.tensor(no_hit, device="cuda")] = 99.0
    got = fold(scene, hits_t, g.t, n, rgb)
    assert (got[no_hit] == 99.0).all()
    oracle_ok = np.setdiff1d(np.arange(n), np.concatenate([no_hit, [20]]))  # the oracle's Face enum has no value 5
    want, want_casts = oracle_shade(desc, rays, hits, rows=oracle_ok)
    bad = oracle_ok[~same_f32(got[oracle_ok], want[oracle_ok]).all(axis=1)]
    assert bad.size == 0, (bad, got[bad[:2]], want[bad[:2]])
    as_back = hits.copy()
    as_back[20, 11] = 1
    want20, casts20 = oracle_shade(desc, rays, as_back, rows=[20])
    assert same_f32(got[20], want20[20]).all()
    assert g.casts == int(want_casts.sum()) + int(casts20.sum())
    assert_shade(by_light(scene, hits_t, rays_t), fused(scene, hits_t, rays_t), "the loop against rt_shade_hits on the foreign batch")
    # caller-set flags: every pair of a valid record asked for, also where the light gives None or faces away.  None gives lit 0, a
    # cosine that is not positive gives black terms, and the fold does not change
    valid = valid_rows(desc, hits)
    forced = np.tile(valid.astype(np.uint8), 3)
    f = run_pieces(scene, hits_t, rays_t, asks_override=forced)
    pos = hits[:, 3:6].view(np.float32)
    n_none = n_away = 0
    for l in range(3):
        some = light_of(desc, l, pos)[0]
        none = valid & ~some
        away = valid & some & (planes(g.asks)[l] == 0)
        n_none, n_away = n_none + int(none.sum()), n_away + int(away.sum())
        assert (planes(f.lit)[l][none] == 0).all(), l
        assert (planes(f.diffuse)[l][none | away].view(np.uint32) == 0).all() and (planes(f.specular)[l][none | away].view(np.uint32) == 0).all(), l
    assert n_none >= 3 and n_away > 0, (n_none, n_away)
    assert (planes(f.lit)[:, no_hit] == 0).all()
    rgb = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
    again = fold(scene, hits_t, f.t, n, rgb)
    keep = np.setdiff1d(np.arange(n), no_hit)
    assert same_f32(again[keep], got[keep]).all() and (again[no_hit].view(np.uint32) == 0).all()
    # ranges of lights: (0, 1), (1, 2) and (0, 3) are planes of one another, and a fold over ranges in order is the fold over all
    whole = run_pieces(scene, hits_t, rays_t, 0, 3)
    rgb = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
    for first, count in ((0, 1), (1, 2)):
        part = run_pieces(scene, hits_t, rays_t, first, count)
        sel = slice(first * n, (first + count) * n)
        assert np.array_equal(part.asks, whole.asks[sel]) and same_rays(part.shadow_rays, whole.shadow_rays[sel]).all()
        assert np.array_equal(part.lit, whole.lit[sel]) and same_f32(part.diffuse, whole.diffuse[sel]).all() and same_f32(part.specular, whole.specular[sel]).all()
        fold(scene, hits_t, part.t, n, rgb)
    assert same_f32(host(rgb)[keep], got[keep]).all()
    # a range past the scene's lights is refused with a message, by every call that takes one; a scene without lights is RT_OK
    lib = rt._capi.amd_lib()
    p = lambda t: C.c_void_p(t.data_ptr())
    asks_t, lit_t, dif_t, spe_t = whole.t
    sr_t, sh_t = dev(whole.shadow_rays), dev(whole.shadow_hits)
    for first, count in ((0, 4), (3, 1), (2, 2), (0xFFFFFFFF, 1), (1, 0xFFFFFFFF // n - 1)):
        assert lib.rt_light_rays(scene._h, p(hits_t), p(rays_t), n, first, count, p(sr_t), p(asks_t), None, None) == -1, (first, count)
        assert b"lights" in lib.rt_last_error()
        assert lib.rt_light_terms(scene._h, p(hits_t), p(rays_t), n, first, count, p(asks_t), p(sh_t), p(lit_t), p(dif_t), p(spe_t), None) == -1
        assert b"lights" in lib.rt_last_error()
    with pytest.raises(rt.RtError):
        rt.light_rays(scene, hits_t, rays_t, 2, 2)
    assert lib.rt_light_rays(scene._h, p(hits_t), p(rays_t), n, 3, 0, p(sr_t), p(asks_t), None, None) == 0  # an empty range at the end
    dark = rt.Scene(with_lights(desc, []))
    assert dark.n_lights == 0
    assert lib.rt_light_rays(dark._h, p(hits_t), p(rays_t), n, 0, 0, p(sr_t), p(asks_t), None, None) == 0
    assert lib.rt_light_rays(dark._h, p(hits_t), p(rays_t), n, 0, 1, p(sr_t), p(asks_t), None, None) == -1
    out, casts = by_light(dark, hits_t, rays_t)
    assert (out.view(np.uint32) == 0).all() and casts == 0
    assert_shade((out, casts), fused(dark, hits_t, rays_t), "a scene without lights")
    torch.cuda.synchronize()


def test_other_scenes():
    """5. behind_spot_world (a spot light whose acos is NaN for some pixels: the light asks, with a NaN colour) and a random world with
    five lights, so that lights_per_pass = 2 ends on a short pass"""
    torch_device()
    world, cam = _scenes.behind_spot_world()
    b = make_batch(world, camera_rays_cpu(cam, 48, 36))
    assert np.isnan(b.shade).any() and b.valid.sum() > 1000  # the case is there
    assert_identity(rt.Scene(world), b, np.arange(b.n), "behind_spot_world")
    world = _scenes.random_world(7, 40, 3, n_lights=5)
    desc = world.desc()
    b = make_batch(world, np.concatenate([camera_rays_cpu(_scenes.camera(7), 32, 24), source_b(desc, 8, 500)]))
    assert desc.n_lights == 5 and b.valid.sum() > 500 and b.casts.max() >= 3
    assert_identity(rt.Scene(world), b, np.arange(b.n), "random_world, 5 lights", passes=(None, 1, 2))


def test_a_scene_walked_breadth_first(tmp_path):
    """6. the 9 244-triangle scene of tests/test_gpu_hit_queries.py, created under the breadth-first switch: the shadow casts of the
    loop go through rt_cast_rays_indexed and take that walk; rt_shade_hits' do not.  Same values, same count"""
    torch_device()
    big, cam = tessellated_scene(tmp_path, 4)
    desc = big.desc()
    assert desc.n_triangles == 36 * 4 ** 4 + 28  # above rt_scene_create's default switch (8 192 triangles)
    with rt.options(RT_AMD_BFS_WALK_TRIANGLES=8192):  # read when the scene is created
        scene = rt.Scene(big)
    b = make_batch(big, np.concatenate([camera_rays_cpu(cam, 24, 18), source_b(desc, 51, 300)]))
    assert b.valid.sum() >= 300 and b.casts.sum() > 300
    # the first uncaptured call on the stream makes the record lists of the walk; the second finds them
    assert_identity(scene, b, np.arange(b.n), "9 244 triangles", passes=(None, None, 1))


def test_the_loop_in_a_graph(ref):
    """7. after one uncaptured call (rt_select_records' scratch on that stream) the loop is captured with its cast count and replayed
    with other records copied into the same buffers, on a stream of its own"""
    torch = torch_device()
    scene = rt.Scene(ref.world)
    n = 1500
    first, second = np.arange(n), np.arange(n) + ref.n - n  # camera rays; random rays and rays inside the glass
    hits_t, rays_t = dev(ref.hits[first]), dev(ref.rays[first])
    out = torch.full((n, 3), 7.0, dtype=torch.float32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    mode = torch.cuda.get_sync_debug_mode()

    def run():
        torch.cuda.set_sync_debug_mode("error")
        try:
            rt.shade_hits_by_light(scene, hits_t, rays_t, out=out, ray_count=cnt, stream=stream)
        finally:
            torch.cuda.set_sync_debug_mode(mode)

    with torch.cuda.stream(stream):
        run()  # uncaptured: the selection's scratch of this stream
        stream.synchronize()
        assert_shade((host(out), int(host(cnt)[0])), (ref.shade[first], int(ref.casts[first].sum())), "uncaptured")
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            run()
    torch.cuda.synchronize()
    for replay, rows in enumerate((first, second, second)):
        hits_t.copy_(dev(ref.hits[rows]))
        rays_t.copy_(dev(ref.rays[rows]))
        out.fill_(7.0)
        cnt.zero_()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert_shade((host(out), int(host(cnt)[0])), (ref.shade[rows], int(ref.casts[rows].sum())), f"replay {replay}")
