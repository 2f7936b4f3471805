"""Light-connection queries on the device (include/rt_amd.h rt_path_connect_lights / rt_path_settle_lights) and the loop built from them
(paths.trace_paths(light_nee=True)).  Both device calls are their CPU forms word for word on every output, on one path, around the wave
size, on more than one workgroup and on a batch of 4 099, unlisted and listed with the count on the device, with and without radii and
weights, at bounces 0 and 2, inside guard words; with one light the loop is the shade_hits loop bit for bit, with glass and with sky
connections too; with three lights it has the shade_hits loop's mean; with radii it has shade_hits_soft's mean and a penumbra; and it
repeats, replays from a graph, allocates nothing and leaves the loop without the option alone.  The hits are the primary hits of 48 x 27
frames of a random world (64 triangles, 4 spheres, 3 lights) and of the reference scene, made once per module."""
import numpy as np
import pytest

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import arealights, environment as E, materials, paths as P
from homework_18_graphics_raytracer_amd._opened import shade_hits_by_light
from homework_18_graphics_raytracer_amd._queries import cast_rays_indexed, select_records
import _connect_support as CS
import _light_connect_support as LC
import _scenes
from _light_support import with_lights
from _lobe_support import assert_same
from _records import dev, host, torch_device, u32

pytestmark = pytest.mark.gpu
F32 = np.float32
WIDTH, HEIGHT = 48, 27
GUARD = 16  # rows of guard words on either side of every output
POISON, POISON_BYTE, POISON_F = 0x5A5A5A5A, 0x5A, F32(7.0)
OFF = P.NO_ROULETTE


def as_i32(a):
    return torch_device().tensor(np.ascontiguousarray(a).view(np.int32), device="cuda")


class Batch:
    pass


def primary(world, camera):
    b = Batch()
    b.world, b.desc = world, world.desc()
    b.scene = rt.Scene(world)
    b.rays_t = rt.camera_rays(camera, rt.Frame.full(WIDTH, HEIGHT, 0))
    b.hits_t = rt.cast_rays(b.scene, b.rays_t)
    b.rays, b.hits, b.n = u32(b.rays_t), u32(b.hits_t).copy(), WIDTH * HEIGHT
    b.surfaces = host(materials.material_hits(b.scene, b.hits_t)).view(materials.SURFACE_DTYPE).reshape(-1)
    b.valid = b.surfaces["valid"] != 0
    b.positions = np.ascontiguousarray(b.hits[:, 3:6]).view(F32)
    b.view = -np.ascontiguousarray(b.rays[:, 3:6]).view(F32)
    assert b.valid.any() and not b.valid.all()
    return b


@pytest.fixture(scope="module")
def rand():
    b = primary(_scenes.random_world(11, 64, 4, n_lights=3), _scenes.camera(2))
    assert sorted(b.desc.lights[l].kind for l in range(3)) == [0, 1, 2]
    return b


@pytest.fixture(scope="module")
def ref():
    return primary(rt.reference_world(), rt.reference_camera())


def guarded(torch, rows, cols, dtype, fill):
    """(the whole tensor, the rows between the guards): a contiguous slice the call is given"""
    shape = (rows + 2 * GUARD,) if cols is None else (rows + 2 * GUARD, cols)
    whole = torch.full(shape, fill, dtype=dtype, device="cuda")
    return whole, whole[GUARD:GUARD + rows]


def guards_hold(whole, fill):
    h = host(whole)
    return (h[:GUARD] == fill).all() and (h[-GUARD:] == fill).all()


def shadow_rays_of(hits, dirs, asks, touched):
    """rt_light_rays' ray along ``dirs`` where a slot asks, zero words where a touched slot does not, the sentinel elsewhere"""
    rays = np.full((hits.shape[0], 11), POISON, dtype=np.uint32)
    rays[touched] = 0
    live = touched & (asks == 1)
    rays[live, 0:3] = hits[live, 3:6]
    rays[live, 3:6] = dirs[live].view(np.uint32)
    rays[live, 6], rays[live, 7], rays[live, 10] = 1, 1, 1
    rays[live, 8], rays[live, 9] = hits[live, 0], hits[live, 1]
    return rays


@pytest.mark.parametrize("m", [1, 63, 64, 65, 259, 4099])
def test_both_calls_are_their_cpu_forms_inside_their_guards(rand, m):
    torch = torch_device()
    roots, spp = (37, 7) if m == 259 else (m, 1)  # 259: sample indices above 0
    rows = np.tile((np.arange(roots) * 5 + 300) % rand.n, spp)
    rng = np.random.default_rng(m)
    hits, incoming, surfaces, positions, view = rand.hits[rows], rand.rays[rows], rand.surfaces[rows], rand.positions[rows], rand.view[rows]
    hits_t, incoming_t = dev(hits), dev(incoming)
    radii, weights = np.array([0.4, float("nan"), 0.25], dtype=F32), np.array([2.0, 1.0, 0.5], dtype=F32)
    asked = occluded = 0
    for case in range(8):
        is_listed, given, bounce = bool(case & 1), bool(case & 2), 2 if case & 4 else 0
        what = f"{m} paths, {'listed' if is_listed else 'unlisted'}, radii and weights {'given' if given else 'NULL'}, bounce {bounce}"
        seed = 900 + case
        before = P.begin_numpy(roots, spp, LC.ids_of(roots))[0]
        before["beta"] = (rng.random((m, 3)) * 2).astype(F32)
        before["bounce"] |= np.uint32(bounce)
        if m > 8:
            before["flags"][6] = P.DARK  # a path that ended before: listed or not, nothing of it moves
        index = count = index_t = count_t = None
        listed = np.ones(m, dtype=bool)
        if is_listed:
            index = rng.permutation(m)[:max(1, (m + 1) // 2)].astype(np.uint32)
            index[::5] = m + 3 + np.arange(len(index[::5]), dtype=np.uint32)  # indices that name nothing
            if m == 1:
                index[:] = 0
            count = max(1, len(index) - 1)  # shorter than the array: the last entry is not listed
            named = index[:count]
            listed = np.isin(np.arange(m), named[named < m])
            padded = np.full(m, 0xFFFFFFFF, dtype=np.uint32)
            padded[:len(index)] = index
            index_t, count_t = as_i32(padded), as_i32(np.array([count], dtype=np.uint32))
        touched = listed & ((before["flags"] & P.ALIVE) != 0)
        paths_t = as_i32(before.view(np.uint32).reshape(m, 8))
        rays_w, rays_t = guarded(torch, m, 11, torch.int32, POISON)
        asks_w, asks_t = guarded(torch, m, None, torch.uint8, POISON_BYTE)
        pending_w, pending_t = guarded(torch, m, 3, torch.float32, float(POISON_F))
        reach_w, reach_t = guarded(torch, m, None, torch.float32, float(POISON_F))
        chosen_w, chosen_t = guarded(torch, m, None, torch.int32, POISON)
        P.connect_lights(rand.scene, paths_t, hits_t, incoming_t, index_t, count_t, seed, dev_f(radii) if given else None, dev_f(weights) if given else None, 0,
                         None, rays_t, asks_t, pending_t, reach_t, chosen_t)
        torch.cuda.synchronize()
        with np.errstate(all="ignore"):
            dirs, asks, pending, reach, chosen = P.connect_lights_numpy(
                surfaces, positions, view, rand.world, before, index, count, seed, radii if given else None, weights if given else None,
                asks=np.full(m, POISON_BYTE, np.uint8), pending=np.full((m, 3), POISON_F, F32), reach=np.full(m, POISON_F, F32),
                chosen=np.full(m, POISON, np.uint32))
        assert_same(host(asks_t), asks, "asks: " + what)
        assert_same(host(pending_t), pending, "pending: " + what, nan_ok=True)
        assert_same(host(reach_t), reach, "reach: " + what, nan_ok=True)
        assert_same(u32(chosen_t), chosen, "chosen: " + what)
        assert_same(u32(rays_t), shadow_rays_of(hits, dirs, asks, touched), "shadow rays: " + what)
        assert_same(u32(paths_t), before.view(np.uint32).reshape(m, 8), "connect_lights wrote the record: " + what)
        assert ((asks != POISON_BYTE) == touched).all() and (pending[asks != 1] == POISON_F).all() and (reach[asks != 1] == POISON_F).all(), what
        assert guards_hold(rays_w, POISON) and guards_hold(asks_w, POISON_BYTE) and guards_hold(pending_w, POISON_F) and guards_hold(reach_w, POISON_F) \
            and guards_hold(chosen_w, POISON), what
        asked += int((asks == 1).sum())
        # settle, on what a cast of the asking rays finds (the sentinels cleared first: an unlisted slot asks nothing in the loop)
        asks_t.copy_(torch.where(asks_t == 1, asks_t, torch.zeros_like(asks_t)))
        asks[asks != 1] = 0
        clean_t = torch.where((asks_t == 1)[:, None], rays_t, torch.zeros_like(rays_t)).contiguous()
        shadow_t = rt.cast_rays(rand.scene, clean_t)
        start = rng.random((m, 3)).astype(F32)
        radiance_w, radiance_t = guarded(torch, m, 3, torch.float32, float(POISON_F))
        radiance_t.copy_(torch.tensor(start, device="cuda"))
        shadow_or_none = None if case == 7 else shadow_t
        P.settle_lights(paths_t, asks_t, clean_t, reach_t, pending_t, radiance_t, shadow_or_none, index_t, count_t)
        torch.cuda.synchronize()
        want_asks, want_radiance = P.settle_lights_numpy(asks, u32(clean_t), host(reach_t), host(pending_t), start, None if case == 7 else u32(shadow_t), index, count)
        assert_same(host(asks_t), want_asks, "settled asks: " + what)
        assert_same(host(radiance_t), want_radiance, "settled radiance: " + what, nan_ok=True)
        assert (want_radiance[~listed] == start[~listed]).all() and (want_asks[~listed] == asks[~listed]).all() and not want_asks[listed].any()
        assert guards_hold(radiance_w, POISON_F) and guards_hold(asks_w, POISON_BYTE), what
        occluded += int(((asks == 1) & listed & (want_radiance == start).all(axis=1)).sum())
    assert m < 64 or (asked > 0 and occluded > 0)


def dev_f(a):
    return torch_device().tensor(np.ascontiguousarray(a, dtype=F32), device="cuda")


def test_the_device_settlement_is_get_shades_occlusion_rule():
    torch = torch_device()

    def settle(asks, rays, reach, pending, radiance, hits, index, count):
        m = len(asks)
        asks_t, radiance_t = torch.tensor(asks, device="cuda"), dev_f(radiance)
        index_t = count_t = None
        if index is not None:
            padded = np.full(m, 0xFFFFFFFF, dtype=np.uint32)
            padded[:len(index)] = index
            index_t, count_t = as_i32(padded), as_i32(np.array([count], dtype=np.uint32))
        P.settle_lights(as_i32(np.zeros((m, 8), np.uint32)), asks_t, dev(rays), dev_f(reach), dev_f(pending), radiance_t, None if hits is None else dev(hits),
                        index_t, count_t)
        torch.cuda.synchronize()
        return host(asks_t), host(radiance_t)

    LC.check_settlement(settle, "settle_lights")


# ---- the loop ----

def finite_throughputs(w, m):
    beta = host(w.paths[:m]).view(F32)[:, :3]
    return np.isfinite(beta).all()


@pytest.mark.parametrize("variant", ["plain", "glass", "sky"])
def test_with_one_light_the_loop_is_the_shade_hits_loop(rand, variant):
    torch = torch_device()
    n, spp, bounces, seed = rand.n, 4, 3, 41
    m = n * spp
    transmission, nee = variant == "glass", variant == "sky"
    env = E.Environment(torch.tensor(CS.sun_sky(), device="cuda"), 0.0, 1.0, E.NEAREST) if nee else None
    for l in range(3):
        scene = rt.Scene(with_lights(rand.desc, [l]))
        w = P.workspace(n, "cuda", spp, scene, transmission, nee, light_nee=True)
        common = dict(env=env, seed=seed, workspace=w, transmission=transmission, walk_rounds=2, nee=nee)
        plain = host(P.trace_paths(scene, rand.hits_t, rand.rays_t, spp, bounces, **common))
        torch.cuda.synchronize()
        assert finite_throughputs(w, m)
        connected = host(P.trace_paths(scene, rand.hits_t, rand.rays_t, spp, bounces, light_nee=True, **common))
        torch.cuda.synchronize()
        assert finite_throughputs(w, m) and np.isfinite(plain).all() and plain[rand.valid].any()
        assert_same(connected, plain, f"{variant}, the light of kind {rand.desc.lights[l].kind} alone")
        assert not host(w.light_asks[:m]).any()


def per_path_luminance(w, m):
    lum = host(w.radiance[:m]).astype(np.float64) @ CS.LUMA
    assert np.isfinite(lum).all()
    return lum


def test_with_three_lights_the_loop_keeps_the_mean(ref):
    """48 x 27, 64 paths per pixel, 2 bounces, radius 0, no roulette.  Measured on an MI355X: see DESIGN.md §3.38."""
    torch = torch_device()
    n, spp, bounces, seed = ref.n, 64, 2, 23
    m = n * spp
    assert ref.scene.n_lights == 3
    w = P.workspace(n, "cuda", spp, ref.scene, light_nee=True)
    runs = {}
    for light_nee in (True, False):
        out_t = P.trace_paths(ref.scene, ref.hits_t, ref.rays_t, spp, bounces, None, OFF, 0.05, seed, workspace=w, light_nee=light_nee)
        torch.cuda.synchronize()
        runs[light_nee] = CS.moments(per_path_luminance(w, m))
        assert np.isfinite(host(out_t)).all() and not host(w.light_asks[:m]).any()
    distance = CS.sigmas(runs[True], runs[False])
    print(f"trace_paths, three lights: mean {runs[True][0]:.6f} with light connections, {runs[False][0]:.6f} with shade_hits, {distance:.3f} combined standard "
          f"errors; per-path variance {runs[True][2]:.6f} against {runs[False][2]:.6f}")
    assert distance <= 5, f"the frame means differ by {distance:.3f} combined standard errors: {runs}"


def test_with_radii_the_shadows_are_shade_hits_softs_and_have_a_penumbra(ref):
    """max_bounces 0, 64 paths per pixel against arealights.shade_hits_soft at 64 stratified samples on the same hits.  The combined
    standard error is the loop's alone, from its per-path radiance: shade_hits_soft returns pixel means, and leaving its own (smaller:
    stratified, every light in every sample) error out only tightens the bound.  The penumbra: with one light (one-hot weights, so nothing
    is chosen at random) the share of a pixel's paths that are lit is 0 or 1 at radius 0 and takes values in between at the edge of a
    shadow with a radius.  Measured on an MI355X: see DESIGN.md §3.38."""
    torch = torch_device()
    n, spp, seed = ref.n, 64, 7
    m = n * spp
    radii = np.array([0.3, 0.3, 0.3], dtype=F32)
    w = P.workspace(n, "cuda", spp, ref.scene, light_nee=True)
    out_t = P.trace_paths(ref.scene, ref.hits_t, ref.rays_t, spp, 0, None, OFF, 0.05, seed, workspace=w, light_nee=True, light_radii=dev_f(radii))
    torch.cuda.synchronize()
    mine = CS.moments(per_path_luminance(w, m))
    soft = host(arealights.shade_hits_soft(ref.scene, ref.hits_t, ref.rays_t, dev_f(radii), 64, arealights.STRATIFIED, 5)).astype(np.float64) @ CS.LUMA
    assert_same((host(out_t).astype(np.float64) @ CS.LUMA > 0)[~ref.valid], np.zeros((~ref.valid).sum(), bool), "a miss stays dark")
    distance = abs(mine[0] - soft.mean()) / mine[1]
    print(f"soft shadows: frame mean {mine[0]:.6f} with light connections, {soft.mean():.6f} from shade_hits_soft, {distance:.3f} standard errors")
    assert distance <= 5, (mine, soft.mean())
    found = []
    for l in range(3):
        one_hot = np.zeros(3, dtype=F32)
        one_hot[l] = 1
        share = {}
        for name, r in (("hard", None), ("soft", dev_f(radii))):
            P.trace_paths(ref.scene, ref.hits_t, ref.rays_t, spp, 0, None, OFF, 0.05, seed, workspace=w, light_nee=True, light_radii=r, light_weights=dev_f(one_hot))
            torch.cuda.synchronize()
            lit = (host(w.radiance[:m]) != 0).any(axis=1).reshape(spp, HEIGHT, WIDTH)
            share[name] = lit.mean(axis=0)
        assert np.isin(share["hard"], (0.0, 1.0)).all()  # one light, a point: every path of a pixel gets the same answer
        for row in range(HEIGHT):
            hard, soft_row = np.unique(share["hard"][row]), np.unique(share["soft"][row])
            if len(hard) == 2 and len(soft_row) > len(hard):
                found.append((l, row, len(hard), len(soft_row)))
    print(f"penumbra: (light, row, distinct shares at radius 0, with a radius) {found[:6]} ... {len(found)} rows")
    assert found


def existing_sequence(scene, hits_t, rays_t, spp, bounces, seed, rr_start, rr_floor):
    """trace_paths' documented sequence without any option, from the public calls"""
    torch = torch_device()
    n = hits_t.shape[0]
    m = n * spp
    paths_t, radiance_t = P.begin(n, spp)
    vertices, rays = hits_t.repeat(spp, 1).contiguous(), rays_t.repeat(spp, 1).contiguous()
    emitted = torch.zeros((m, 3), dtype=torch.float32, device="cuda")
    listed = counted = None
    for b in range(bounces + 1):
        shade_hits_by_light(scene, vertices, rays, out=emitted)
        next_rays, alive = P.advance(scene, paths_t, vertices, rays, radiance_t, emitted, listed, counted, seed, P.SHADING, rr_start, rr_floor, b == bounces)
        if b == bounces:
            break
        listed, counted = select_records(alive)
        cast_rays_indexed(scene, next_rays, listed, counted, vertices)
        rays = next_rays
    return P.resolve(radiance_t, n, spp)


def test_the_loop_repeats_replays_allocates_nothing_and_leaves_the_old_loop_alone(ref):
    torch = torch_device()
    n, spp, bounces, seed = ref.n, 4, 2, 29
    radii, weights = dev_f([0.2, 0.0, 0.1]), dev_f([1.0, 2.0, 1.5])
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        w = P.workspace(n, "cuda", spp, ref.scene, light_nee=True, chosen=True)
        out_t = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
        run = lambda: P.trace_paths(ref.scene, ref.hits_t, ref.rays_t, spp, bounces, None, 1, 0.3, seed, None, out_t, True, stream, w, light_nee=True,
                                    light_radii=radii, light_weights=weights)
        run()  # the eager call: select_records and the indexed casts have run once
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
    chosen = u32(w.light_chosen[:n * spp])
    assert ((chosen < 3) | (chosen == P.NO_LIGHT)).all() and (chosen < 3).any()
    # without the option the loop is the existing sequence, call for call
    without = P.trace_paths(ref.scene, ref.hits_t, ref.rays_t, spp, bounces, None, 1, 0.3, seed, workspace=w)
    want = existing_sequence(ref.scene, ref.hits_t, ref.rays_t, spp, bounces, seed, 1, 0.3)
    torch.cuda.synchronize()
    assert_same(host(without), host(want), "light_nee False is the existing sequence", nan_ok=True)
