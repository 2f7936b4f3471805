"""Connection queries on the device (include/rt_amd.h rt_path_connect / rt_path_settle / rt_path_weigh_escape) and the loop built from
them (paths.trace_paths(nee=True)).  Every device result is the CPU form's word for word, on more than one workgroup with a partial last
wave, on one wave, on one path and on lists; slots that are not listed, not alive or not asking keep their sentinel and the record is
never written; one connect is the six calls it fuses, run on the device; the loop with connections has the lobe-only loop's mean and
less variance under a sky with a small sun, with and without glass, replays from a graph, allocates nothing and without light is the
lobe-only loop bit for bit; and a diffuse furnace returns pi * c * L.  The hits are the reference scene's primary hits of a 48 x 27
frame — spheres, triangles, glass, bump-mapped materials and misses — made once per module."""
import math

import numpy as np
import pytest

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import environment as E, lobes as L, materials, paths as P
from homework_18_graphics_raytracer_amd._capi import Light, Material
import _connect_support as CS
import _path_support as PS
from _lobe_support import assert_same
from _records import dev, host, ray_records, torch_device, u32

pytestmark = pytest.mark.gpu
F32 = np.float32
WIDTH, HEIGHT = 48, 27
MIDDLE = (HEIGHT // 2) * WIDTH
SHAPES = [(87, 3), (64, 1), (1, 1)]  # roots x samples: 261 paths — two workgroups, a partial last wave —, one wave exactly, one path
OFF = P.NO_ROULETTE
POISON, POISON_BYTE, POISON_F = 0x5A5A5A5A, 0x5A, F32(7.0)


def ids_of(n):
    return (np.arange(n, dtype=np.uint32) * np.uint32(2654435761)) ^ np.uint32(0x80000001)


def as_i32(a):
    return torch_device().tensor(np.ascontiguousarray(a).view(np.int32), device="cuda")


class Batch:
    pass


@pytest.fixture(scope="module")
def ref():
    torch = torch_device()
    b = Batch()
    b.world = rt.reference_world()
    b.scene = rt.Scene(b.world)
    b.rays_t = rt.camera_rays(rt.reference_camera(), rt.Frame.full(WIDTH, HEIGHT, 0))
    b.rays = u32(b.rays_t)
    b.hits_t = rt.cast_rays(b.scene, b.rays_t)
    b.hits, b.n = u32(b.hits_t).copy(), WIDTH * HEIGHT
    b.surfaces = host(materials.material_hits(b.scene, b.hits_t)).view(materials.SURFACE_DTYPE).reshape(-1)
    b.valid = b.surfaces["valid"] != 0
    b.geometric = np.ascontiguousarray(b.hits[:, 6:9]).view(F32)
    b.view = -np.ascontiguousarray(b.rays[:, 3:6]).view(F32)
    window = b.valid[MIDDLE:MIDDLE + 87]
    assert window.any() and not window.all() and (b.surfaces["transparency"][b.valid] > 0).any() and (b.surfaces["shiness"][b.valid] > 0).any()
    b.skies = {}
    for name, img in (("sun", CS.sun_sky()), ("half", CS.half_sky()), ("dark", CS.dark_sky())):
        b.skies[name] = (img, E.table_numpy(img), E.Environment(torch.tensor(img, device="cuda"), 0.0, 1.0, E.NEAREST))
    return b


def lists_of(m, rng):
    """(index, count) of the device's list convention: all slots, count 0, count < M, and indices >= M that name nothing"""
    yield None, None
    if m > 1:
        half = rng.permutation(m)[:max(1, m // 2)].astype(np.uint32)
        yield half, 0
        yield half, max(1, len(half) // 2)
        beyond = half.copy()
        beyond[::3] = m + 5 + np.arange(len(beyond[::3]), dtype=np.uint32)
        yield beyond, m + 1000


def listed_slots(index, count, m):
    if index is None:
        return np.ones(m, dtype=bool)
    named = index[:min(count, m, len(index))]
    return np.isin(np.arange(m), named[named < m])


def device_list(index, count, m):
    if index is None:
        return None, None
    padded = np.full(m, 0xFFFFFFFF, dtype=np.uint32)
    padded[:len(index)] = index
    return as_i32(padded), as_i32(np.array([count], dtype=np.uint32))


def shadow_rays_of(hits, dirs, asks, touched):
    """rt_hemisphere_rays' ray along ``dirs`` where a slot asks, zero words where a touched slot does not, the sentinel elsewhere"""
    m = hits.shape[0]
    rays = np.full((m, 11), POISON, dtype=np.uint32)
    rays[touched] = 0
    live = touched & (asks == 1)
    rays[live, 0:3] = hits[live, 3:6]
    rays[live, 3:6] = dirs[live].view(np.uint32)
    rays[live, 6], rays[live, 7], rays[live, 10] = 1, 1, 1
    rays[live, 8], rays[live, 9] = hits[live, 0], hits[live, 1]
    return rays


@pytest.mark.parametrize("heuristic", [P.BALANCE, P.POWER], ids=["balance", "power"])
@pytest.mark.parametrize("roots,spp", SHAPES)
def test_the_three_calls_are_their_cpu_forms_and_write_nothing_else(ref, roots, spp, heuristic):
    torch = torch_device()
    m = roots * spp
    rows = np.tile(np.arange(MIDDLE, MIDDLE + roots), spp)
    rng = np.random.default_rng(m + heuristic)
    hits, incoming, surfaces, view = ref.hits[rows], ref.rays[rows], ref.surfaces[rows], ref.view[rows]
    hits_t, incoming_t = dev(hits), dev(incoming)
    asked = weighed_some = 0
    for sky in ("sun", "half", "dark"):
        img, table, env = ref.skies[sky]
        for case, (index, count) in enumerate(lists_of(m, rng)):
            kind, bounce, seed = (P.SHADING, P.GEOMETRIC)[case % 2], case % 3, 500 + case
            what = f"{roots} x {spp}, {sky}, list {case}"
            before = PS.records(roots, spp, ids_of(roots), (rng.random((m, 3)) * 2).astype(F32), bounce)
            before["pdf"] = np.where(rng.random(m) < 0.2, 0.0, rng.random(m) * 3 + 0.01).astype(F32)
            if m > 8:
                before["flags"][6] = P.DARK  # a path that ended before: listed or not, nothing of it moves
            listed = listed_slots(index, count, m)
            touched = listed & ((before["flags"] & P.ALIVE) != 0)
            index_t, count_t = device_list(index, count, m)
            paths_t = as_i32(before.view(np.uint32).reshape(m, 8))
            # connect
            rays_t = torch.full((m, 11), POISON, dtype=torch.int32, device="cuda")
            asks_t = torch.full((m,), POISON_BYTE, dtype=torch.uint8, device="cuda")
            pending_t = torch.full((m, 3), float(POISON_F), dtype=torch.float32, device="cuda")
            P.connect(ref.scene, env, paths_t, hits_t, incoming_t, index_t, count_t, seed, kind, heuristic, False, None, rays_t, asks_t, pending_t)
            torch.cuda.synchronize()
            with np.errstate(all="ignore"):
                dirs, asks, pending = P.connect_numpy(surfaces, view, img, table, before, index, count, seed, ref.geometric[rows] if kind == P.GEOMETRIC else None,
                                                      heuristic, asks=np.full(m, POISON_BYTE, np.uint8), pending=np.full((m, 3), POISON_F, F32))
            assert_same(host(asks_t), asks, "asks: " + what)
            assert_same(host(pending_t), pending, "pending: " + what, nan_ok=True)
            assert_same(u32(rays_t), shadow_rays_of(hits, dirs, asks, touched), "shadow rays: " + what)
            assert_same(u32(paths_t), before.view(np.uint32).reshape(m, 8), "connect wrote the record: " + what)
            assert ((asks != POISON_BYTE) == touched).all() and (pending[asks != 1] == POISON_F).all(), what
            assert sky != "dark" or not (asks == 1).any()
            asked += int((asks == 1).sum())
            # settle, on what a cast of the asking rays finds (the sentinels cleared first: an unlisted slot asks nothing in the loop)
            asks_t = torch.where(asks_t == 1, asks_t, torch.zeros_like(asks_t))
            asks[asks != 1] = 0
            if m > 3:
                asks_t[3], asks[3] = 1, 1  # an ask outside some lists: it stays
            clean_t = torch.where((asks_t == 1)[:, None] & (rays_t != POISON), rays_t, torch.zeros_like(rays_t)).contiguous()
            shadow_t = rt.cast_rays(ref.scene, clean_t)
            start = rng.random((m, 3)).astype(F32)
            radiance_t = torch.tensor(start, device="cuda")
            P.settle(paths_t, asks_t, pending_t, radiance_t, shadow_t, index_t, count_t)
            torch.cuda.synchronize()
            want_asks, want_radiance = P.settle_numpy(asks, host(pending_t), start, u32(shadow_t), index, count)
            assert_same(host(asks_t), want_asks, "settled asks: " + what)
            assert_same(host(radiance_t), want_radiance, "settled radiance: " + what, nan_ok=True)
            assert (want_radiance[~listed] == start[~listed]).all() and (want_asks[~listed] == asks[~listed]).all() and not want_asks[listed].any()
            # weigh_escape
            emitted = (rng.random((m, 3)) * 4).astype(F32)
            emitted_t = torch.tensor(emitted, device="cuda")
            P.weigh_escape(env, paths_t, hits_t, incoming_t, emitted_t, index_t, count_t, heuristic)
            torch.cuda.synchronize()
            want = P.weigh_escape_numpy(img, table, before, hits, incoming, emitted, index, count, heuristic)
            assert_same(host(emitted_t), want, "weighed: " + what)
            assert_same(u32(paths_t), before.view(np.uint32).reshape(m, 8), "weigh_escape wrote the record: " + what)
            kept = ~touched | (hits[:, 0] <= 1) | (before["pdf"] == 0)
            assert (want[kept] == emitted[kept]).all() and (sky != "dark" or (want == emitted).all())
            weighed_some += int((want != emitted).any(axis=1).sum())
    assert m < 64 or (asked > 0 and weighed_some > 0)


@pytest.mark.parametrize("bounce", [0, 2])
def test_one_connect_is_the_six_calls_it_fuses(ref, bounce):
    """environment.rays (UNIFORM, the bounce's seed) -> material_hits -> probe_surfaces -> environment_pdf -> lobes.pdf -> mis_weigh, then
    beta * and environment.fold's association, on the device, against one connect: bit for bit; the shadow ray is rt_hemisphere_rays'"""
    torch = torch_device()
    n = 261
    rows = slice(MIDDLE, MIDDLE + n)
    rng = np.random.default_rng(bounce)
    hits_t, incoming_t = ref.hits_t[rows].contiguous(), ref.rays_t[rows].contiguous()
    view_t = (-incoming_t[:, 3:6].view(torch.float32)).contiguous()
    for sky, heuristic in (("sun", P.BALANCE), ("half", P.POWER)):
        _, _, env = ref.skies[sky]
        seed, ids = 0xABCD0000 + bounce, ids_of(n)
        before = PS.records(n, 1, ids, 1.0 if bounce == 0 else (rng.random((n, 3)) * 2).astype(F32), bounce)
        rays_t, asks_t, dirs_t, radiance_t, _ = E.rays(ref.scene, env, hits_t, 1, E.UNIFORM, PS.seed_of(seed, bounce), as_i32(ids), E.SHADING)
        surfaces_t = materials.material_hits(ref.scene, hits_t)
        diffuse_t, specular_t = materials.probe_surfaces(surfaces_t, view_t, dirs_t.view(1, n, 3))
        p_env_t, _ = L.environment_pdf(env, dirs_t)
        p_lobe_t = L.pdf(surfaces_t, view_t, dirs_t.view(1, n, 3))
        w_t = torch.zeros((n,), dtype=torch.float32, device="cuda")
        L.mis_weigh(p_env_t, 1, p_lobe_t, 1, heuristic, False, w_t, radiance_t)
        t_t = (torch.tensor(before["beta"], device="cuda") * radiance_t).contiguous()
        both_t = (asks_t != 0) & torch.isfinite(w_t)
        want_pending_t = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
        E.fold(ref.scene, hits_t, both_t.to(torch.uint8), 1, t_t, diffuse_t.view(n, 3), specular_t.view(n, 3), want_pending_t)
        got_rays_t, got_asks_t, got_pending_t = P.connect(ref.scene, env, as_i32(before.view(np.uint32).reshape(n, 8)), hits_t, incoming_t, None, None, seed,
                                                          P.SHADING, heuristic)
        torch.cuda.synchronize()
        ask = host(both_t)
        what = f"bounce {bounce}, {sky}"
        assert_same(host(got_asks_t), ask.astype(np.uint8), "asks: " + what)
        assert_same(host(got_pending_t)[ask], host(want_pending_t)[ask], "pending: " + what)
        assert_same(u32(got_rays_t)[ask], u32(rays_t)[ask], "the shadow ray: " + what)
        assert not u32(got_rays_t)[~ask].any() and ask.sum() > n // 4 and (host(w_t)[ask] < 1).any()


# ---- the loop ----

def per_path_luminance(w, m):
    lum = host(w.radiance[:m]).astype(np.float64) @ CS.LUMA
    assert np.isfinite(lum).all()
    return lum


def test_the_loop_with_connections_keeps_the_mean_and_cuts_the_variance(ref):
    """48 x 27, 64 paths per pixel, 2 bounces, the sun sky, no roulette.  Measured on an MI355X: see DESIGN.md §3.37."""
    torch = torch_device()
    n, spp, bounces, seed = ref.n, 64, 2, 23
    m = n * spp
    _, _, env = ref.skies["sun"]
    for transmission, rounds in ((False, 11), (True, 2)):
        w = P.workspace(n, "cuda", spp, ref.scene, transmission, nee=True)
        runs = {}
        for nee in (True, False):
            out_t = P.trace_paths(ref.scene, ref.hits_t, ref.rays_t, spp, bounces, env, OFF, 0.05, seed, workspace=w, transmission=transmission,
                                  walk_rounds=rounds, nee=nee)
            torch.cuda.synchronize()
            runs[nee] = CS.moments(per_path_luminance(w, m))
            assert np.isfinite(host(out_t)).all() and not host(w.asks[:m]).any()
        distance = CS.sigmas(runs[True], runs[False])
        print(f"trace_paths, transmission {transmission}: mean {runs[True][0]:.6f} with connections, {runs[False][0]:.6f} without, {distance:.3f} combined "
              f"standard errors; per-path variance {runs[True][2]:.6f} against {runs[False][2]:.6f}: ratio {runs[False][2] / runs[True][2]:.2f}")
        assert distance <= 5, f"the frame means differ by {distance:.3f} combined standard errors: {runs}"
        if not transmission:
            assert runs[True][2] < runs[False][2], runs


def test_the_loop_repeats_replays_allocates_nothing_and_is_the_old_loop_without_light(ref):
    torch = torch_device()
    n, spp, bounces, seed = ref.n, 4, 2, 29
    _, _, env = ref.skies["sun"]
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        w = P.workspace(n, "cuda", spp, ref.scene, nee=True)
        out_t = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
        run = lambda: P.trace_paths(ref.scene, ref.hits_t, ref.rays_t, spp, bounces, env, 1, 0.3, seed, None, out_t, True, stream, w, nee=True, heuristic=P.POWER)
        run()  # the eager call: the table is built here, select_records and the indexed casts have run once
        stream.synchronize()
        first = host(out_t)
        out_t.zero_()
        before = torch.cuda.memory_allocated()
        run()
        assert torch.cuda.memory_allocated() == before  # a workspace and out: nothing is allocated
        stream.synchronize()
        assert_same(host(out_t), first, "the same bits twice", nan_ok=True)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            run()
        for _ in range(2):
            out_t.zero_()
            stream.synchronize()
            graph.replay()
            stream.synchronize()
            assert_same(host(out_t), first, "a replay", nan_ok=True)
    assert np.isfinite(first[ref.valid]).all() and first[ref.valid].any()
    # a sky without light: no connection asks and no escape is weighed, so the bits are the lobe-only loop's
    _, _, dark = ref.skies["dark"]
    with_nee = P.trace_paths(ref.scene, ref.hits_t, ref.rays_t, spp, bounces, dark, 1, 0.3, seed, nee=True)
    without = P.trace_paths(ref.scene, ref.hits_t, ref.rays_t, spp, bounces, dark, 1, 0.3, seed)
    torch.cuda.synchronize()
    assert_same(host(with_nee), host(without), "without light", nan_ok=True)


# ---- the furnace ----

def test_a_diffuse_furnace_returns_pi_c_l(ref):
    """A diffuse square under a constant sky L: the connection settled at bounce 0 plus the weighed escape deposited at bounce 1 is
    pi * c * L in expectation (the Phong terms are the reference's, not normalised); the mean over 64 x 261 paths lies within 5 standard
    errors per channel.  And on the CPU forms the two balance weights of a direction add up to 1."""
    torch = torch_device()
    roots, spp = 261, 64
    m = roots * spp
    c, sky = np.array([0.7, 0.4, 0.2]), np.array([1.5, 2.0, 0.25])
    material = Material()
    material.normal, material.diffuse_color, material.specular_color = (0.0, 0.0, 1.0), tuple(c), (0.0, 0.0, 0.0)
    material.shiness, material.smoothness, material.refraction_index = 0.0, 1.0, 1.0
    world = rt.World()
    world.push_object(material).push_square([(-50.0, 0.0, -50.0), (-50.0, 0.0, 50.0), (50.0, 0.0, 50.0), (50.0, 0.0, -50.0)], [(0, 0), (0, 1), (1, 1), (1, 0)])
    light = Light()
    light.kind, light.color, light.direction = 0, (0.0, 0.0, 0.0), (0.0, -1.0, 0.0)
    world.push_light(light)
    scene = rt.Scene(world)
    img = np.broadcast_to(sky.astype(F32), (CS.HEIGHT, CS.WIDTH, 3)).copy()
    env = E.Environment(torch.tensor(img, device="cuda"), 0.0, 1.0, E.NEAREST)
    rng = np.random.default_rng(17)
    origins = np.column_stack([rng.uniform(-3, 3, roots), np.full(roots, 2.0), rng.uniform(-3, 3, roots)]).astype(F32)
    directions = np.column_stack([rng.uniform(-0.4, 0.4, roots), np.full(roots, -1.0), rng.uniform(-0.4, 0.4, roots)])
    directions = (directions / np.linalg.norm(directions, axis=1, keepdims=True)).astype(F32)
    rays_t = dev(ray_records(origins, directions)).repeat(spp, 1).contiguous()
    hits_t = rt.cast_rays(scene, rays_t)
    assert (u32(hits_t)[:, 0] <= 1).all()
    paths_t, radiance_t = P.begin(roots, spp, as_i32(ids_of(roots)))
    shadow_rays_t, asks_t, pending_t = P.connect(scene, env, paths_t, hits_t, rays_t, seed=3)
    next_rays_t, alive_t = P.advance(scene, paths_t, hits_t, rays_t, radiance_t, None, seed=3, rr_start=OFF)
    P.settle(paths_t, asks_t, pending_t, radiance_t, rt.cast_rays(scene, shadow_rays_t))
    vertices_t = rt.cast_rays(scene, next_rays_t)
    emitted_t = E.lookup(env, next_rays_t, vertices_t)
    P.weigh_escape(env, paths_t, vertices_t, next_rays_t, emitted_t)
    P.advance(scene, paths_t, vertices_t, next_rays_t, radiance_t, emitted_t, seed=3, rr_start=OFF, last=True)
    torch.cuda.synchronize()
    radiance = host(radiance_t).astype(np.float64)
    assert host(alive_t).mean() > 0.99 and (u32(vertices_t)[:, 0] > 1).all() and not host(asks_t).any() and np.isfinite(radiance).all()
    want = math.pi * c * sky
    for channel in range(3):
        mean, error, _ = CS.moments(radiance[:, channel])
        print(f"furnace, channel {channel}: mean {mean:.6f}, pi c L {want[channel]:.6f}, {abs(mean - want[channel]) / error:.3f} standard errors")
        assert abs(mean - want[channel]) <= 5 * error, (channel, mean, want[channel], error)
    CS.check_weights_add_up(img)
