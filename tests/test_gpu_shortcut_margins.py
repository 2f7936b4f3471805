"""The shortcuts that skip work of a certain outcome, held to the oracle on inputs aimed at their margins (tests/_margin_support.py):
the per-triangle bounding-sphere rejection through the three walkers and the persistent kernel's cast, the sphere miss ahead of the
square root, the spot cone's edge through the per-light kernels, the all-lights loop and the two render loops, and the Phong power's
underflow.  Every comparison is of uint32 views against the oracle (oracle_hits, orc_ray_trace, orc_light_directional, orc_get_shade,
the oracle's frames, expected_probe): there is no tolerance.  The generators assert their own coverage on the CPU; on a mismatch the label of the
first differing case is printed."""
import ctypes as C

import numpy as np
import pytest

import homework_18_graphics_raytracer_amd as rt
import _margin_support as M
import _oracle
from _light_support import oracle_shade, run_pieces, with_lights
from _material_support import expected_probe, hit_record
from _records import camera_rays_cpu, dev, host, oracle_hits, same_f32, same_hits, torch_device
from _trace_support import _check

pytestmark = pytest.mark.gpu
F32 = np.float32
BATCH = 8192
WALKERS = ("pair-wise", "wave-uniform", "breadth-first")


def oracle_trace(desc, rays, depth=0, contribution=1.0):
    rays = np.ascontiguousarray(rays).view(np.uint32).reshape(-1, 11).copy()
    n = rays.shape[0]
    orays = (_oracle.OrcRay * n).from_buffer(rays)
    rgb, buf, casts, total = np.zeros((n, 3), dtype=F32), (C.c_float * 3)(), C.c_uint64(0), 0
    lib = _oracle.lib()
    for i in range(n):
        lib.orc_ray_trace(C.byref(desc), C.byref(orays[i]), depth, contribution, buf, C.byref(casts))
        rgb[i] = buf[:]
        total += casts.value
    return rgb, total


def cast(world, rays, walker):
    """rt_cast_rays of the batch, at most BATCH rays a call, through one of the three walkers"""
    torch = torch_device()
    opts = {"RT_AMD_BFS_WALK_TRIANGLES": 1} if walker == "breadth-first" else {}
    with rt.options(**opts):
        scene = rt.Scene(world)
        with rt.options(**({"RT_AMD_QUERY_WAVE_UNIFORM": 1} if walker == "wave-uniform" else {})):
            out = [rt.cast_rays(scene, dev(rays[k:k + BATCH])) for k in range(0, rays.shape[0], BATCH)]
        torch.cuda.synchronize()
    return np.concatenate([host(o).view(np.uint32) for o in out])


def assert_hits(got, want, labels, what):
    bad = np.flatnonzero(~same_hits(got, want))
    assert bad.size == 0, f"{what}: {bad.size} of {want.shape[0]} differ, first: {labels[bad[0]]}: got {got[bad[0]]} want {want[bad[0]]}"


def assert_trace(world, desc, rays, labels, what):
    torch = torch_device()
    scene = rt.Scene(world)
    want, want_casts = oracle_trace(desc, rays)
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    out = [rt.trace_rays(scene, dev(rays[k:k + BATCH]), 0, 1.0, ray_count=count) for k in range(0, rays.shape[0], BATCH)]
    torch.cuda.synchronize()
    got = np.concatenate([host(o) for o in out])
    bad = np.flatnonzero(~same_f32(got, want).all(axis=1))
    assert bad.size == 0, f"{what}: {bad.size} of {want.shape[0]} differ, first: {labels[bad[0]]}: got {got[bad[0]]} want {want[bad[0]]}"
    assert int(count.item()) == want_casts, (what, int(count.item()), want_casts)


# ---- the per-triangle bounding-sphere rejection ----


@pytest.fixture(scope="module")
def rejection():
    rw = M.rejection_world()
    cases = M.rejection_rays(rw)
    cases.want = oracle_hits(rw.desc, cases.rays)
    # what the oracle accepts uses how much of the 5 %: |p - bc|^2 / bq of the hits on the triangle aimed at (a report, not a check)
    on_target = (cases.want[:, 0] == 1) & (cases.want[:, 1] == cases.tri)
    assert on_target.sum() >= 1000
    ratio = cases.q[on_target].astype(np.float64) / cases.bq[on_target].astype(np.float64)
    below, above = ratio[ratio <= 1.0], ratio[ratio > 1.0]
    print(f"margin: rejection: {int(on_target.sum())} of {cases.want.shape[0]} rays are accepted by the triangle they aim at; largest |p - bc|^2 / bq "
          f"among them {below.max():.6f}" + (f"; {above.size} accepts above bq (rays that may not use the rejection), smallest {above.min():.6f}" if above.size else "; none above bq"))
    for key, v in cases.counts.items():
        print("margin: rejection:", key, v)
    # an accept beyond bq can only be a ray that may not use the rejection: the claim the 1.05 rests on, on the oracle's side
    assert not (on_target & cases.beyond & cases.filter_ok & np.isfinite(cases.q)).any()
    return rw, cases


@pytest.mark.parametrize("walker", WALKERS)
def test_rejection_rays(rejection, walker):
    rw, cases = rejection
    assert_hits(cast(rw.world, cases.rays, walker), cases.want, cases.labels, f"rejection rays, {walker}")


def test_rejection_rays_in_the_persistent_kernel(rejection):
    """the same rays through rt_trace_rays at depth 0: the persistent kernel's instantiation of the cast, then get_shade's shadow casts"""
    rw, cases = rejection
    assert_trace(rw.world, rw.desc, cases.rays, cases.labels, "rejection rays, rt_trace_rays")


@pytest.mark.parametrize("extent, on", [(0.99e10, True), (1.01e10, False)])
def test_rejection_switches_off_above_an_extent_of_1e10(rejection, extent, on):
    scale = extent / 4.0
    big = M.rejection_world(scale)
    finite = np.isfinite(big.filters[0][:, 3])
    expect = np.array([k >= 0 and M.SHAPES[k][2] for k in big.shape])
    assert finite[expect].all() == on and not finite[~expect & (big.shape >= 0)].any() and (on or not finite.any())
    rays = M.scaled_batch(rejection[1], scale)
    assert_hits(cast(big.world, rays, "pair-wise"), oracle_hits(big.desc, rays), rejection[1].labels, f"extent {extent}")


# ---- the sphere miss ahead of the square root ----


@pytest.fixture(scope="module")
def tangent():
    world, centres = M.tangent_world()
    cases = M.tangent_rays(world, centres)
    cases.want = oracle_hits(world.desc(), cases.rays)
    for si in (5, 6):  # the rays aimed inside each of the two ordinary spheres do hit it
        assert ((cases.want[:, 0] == 0) & (cases.want[:, 1] == si)).sum() >= 64
    for key, v in cases.counts.items():
        print("margin: tangent:", key, v)
    return world, cases


@pytest.mark.parametrize("walker", WALKERS)
def test_tangent_rays(tangent, walker):
    world, cases = tangent
    assert_hits(cast(world, cases.rays, walker), cases.want, cases.labels, f"tangent rays, {walker}")


def test_tangent_rays_in_the_persistent_kernel(tangent):
    world, cases = tangent
    assert_trace(world, world.desc(), cases.rays, cases.labels, "tangent rays, rt_trace_rays")


# ---- the spot cone's edge ----


@pytest.fixture(scope="module")
def cone():
    """hand-made hits at the points of cone_points, each facing its light, looked at along the normal; orc_get_shade of the whole scene,
    and of the scene holding one light alone on that light's own points"""
    c = M.Cases()
    c.world = M.cone_world()
    c.desc = c.world.desc()
    aux = M.describe_filters(c.desc)[2]
    hits, rays, c.labels, owner, buckets = [], [], [], [], []
    for l in range(c.desc.n_lights):
        pos, normal, labels, bucket, some = M.cone_points(c.desc.lights[l], aux[l], seed=1000 * l)
        print(f"margin: cone: spread {M.CONE_SPREADS[l]}: {dict(zip(M.CONE_BUCKETS, (int((bucket == b).sum()) for b in range(3))))}; the oracle gives a light at "
              f"{int(some.sum())} of {some.size}, at {int((some & (bucket == 1)).sum())} of the middle bucket")
        hits += [hit_record(1, 0, 0, normal[i], position=pos[i]) for i in range(pos.shape[0])]
        r = np.zeros((pos.shape[0], 11), dtype=np.uint32)
        r[:, 0:3], r[:, 3:6] = (pos + normal).view(np.uint32), (-normal).view(np.uint32)
        rays.append(r); c.labels += labels; owner += [l] * pos.shape[0]; buckets.append(bucket)
    c.hits, c.rays, c.owner = np.stack(hits), np.concatenate(rays), np.array(owner)
    c.shade, c.casts = oracle_shade(c.desc, c.rays, c.hits)
    c.alone = {l: oracle_shade(with_lights(c.desc, [l]), c.rays, c.hits, rows=np.flatnonzero(c.owner == l)) for l in range(c.desc.n_lights)}
    assert (c.casts > 0).sum() > 1000 and c.shade.any()
    return c


def test_cone_points_in_the_all_lights_loop(cone):
    torch = torch_device()
    scene = rt.Scene(cone.world)
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    out = [rt.shade_hits(scene, dev(cone.hits[k:k + BATCH]), dev(cone.rays[k:k + BATCH]), ray_count=count) for k in range(0, cone.hits.shape[0], BATCH)]
    torch.cuda.synchronize()
    got = np.concatenate([host(o) for o in out])
    bad = np.flatnonzero(~same_f32(got, cone.shade).all(axis=1))
    assert bad.size == 0, f"rt_shade_hits: {bad.size} of {got.shape[0]} differ, first: {cone.labels[bad[0]]}: got {got[bad[0]]} want {cone.shade[bad[0]]}"
    assert int(count.item()) == int(cone.casts.sum())


def test_cone_points_light_by_light(cone):
    """rt_light_rays' flag is orc_get_shade's cast count on the scene holding that light alone, and rt_light_terms' two terms, weighted in
    numpy f32, are its value: on the light's own points; the casts of all lights on all points add up to the whole scene's"""
    torch_device()
    scene = rt.Scene(cone.world)
    n, total = cone.hits.shape[0], 0
    shiness = F32(cone.desc.materials[0].shiness)
    for k in range(0, n, BATCH):
        rows = np.arange(k, min(n, k + BATCH))
        g = run_pieces(scene, dev(cone.hits[rows]), dev(cone.rays[rows]))
        total += g.casts
        for l in range(cone.desc.n_lights):
            own = np.flatnonzero(cone.owner[rows] == l)
            if own.size == 0:
                continue
            plane = l * rows.size + own
            want_shade, want_casts = cone.alone[l]
            bad = np.flatnonzero(g.asks[plane] != want_casts[rows[own]])
            assert bad.size == 0, f"rt_light_rays: {bad.size} flags differ, first: {cone.labels[rows[own[bad[0]]]]}: got {g.asks[plane][bad[0]]}"
            with np.errstate(all="ignore"):
                mine = (F32(0.0) + g.diffuse[plane] * (F32(1.0) - shiness)) + g.specular[plane] * shiness
            bad = np.flatnonzero(~same_f32(mine, want_shade[rows[own]]).all(axis=1))
            assert bad.size == 0, f"rt_light_terms: {bad.size} differ, first: {cone.labels[rows[own[bad[0]]]]}: got {mine[bad[0]]} want {want_shade[rows[own[bad[0]]]]}"
    assert total == int(cone.casts.sum())


@pytest.fixture(scope="module")
def edge_view():
    """the oracle's side of the 16 x 16 view: lit and unlit pixels, and pixels whose restated x lies between cos_out and cos_in"""
    world, cam = M.cone_edge_view()
    desc = world.desc()
    aux = M.describe_filters(desc)[2][0]
    hits = oracle_hits(desc, camera_rays_cpu(cam, 16, 16))
    assert (hits[:, 0] == 1).all()
    x = M.restate_cone_x(desc.lights[0], hits[:, 3:6].view(F32))
    counts = (int((x > aux[0]).sum()), int(((x >= aux[1]) & (x <= aux[0])).sum()), int((x < aux[1]).sum()))
    image, _ = _oracle.render_whitted(desc, cam, rt.Frame.full(16, 16, 3))
    lit = (image != 0).any(axis=2)
    print(f"margin: cone: the 16 x 16 view: pixels per bucket {dict(zip(M.CONE_BUCKETS, counts))}; {int(lit.sum())} lit, {int((~lit).sum())} unlit")
    assert min(counts) >= 1 and lit.sum() >= 16 and (~lit).sum() >= 16
    return world, cam


def test_cone_edge_in_a_whitted_frame(edge_view):
    world, cam = edge_view
    _check(world, cam, rt.Frame.full(16, 16, 3))


def test_cone_edge_in_a_depth_of_field_epoch(edge_view):
    torch = torch_device()
    world, cam = edge_view
    scene = rt.Scene(world)
    tile = rt.Frame.full(16, 16, 3)
    rng = rt.Rng(tile)
    samples = torch.empty((1, 16, 16, 3), dtype=torch.float32, device="cuda")
    valid = torch.empty((1, 16, 16), dtype=torch.uint8, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    rt.render_distributed(scene, cam, tile, rng, 1, focus=1.5, blur=1e-4, samples=samples, valid=valid, ray_count=count)
    torch.cuda.synchronize()
    states = _oracle.rng_init(tile)
    want_s, want_v, want_c = _oracle.render_distributed(world.desc(), cam, tile, states, 1, focus=1.5, blur=1e-4)
    lit = (want_s[0] != 0).any(axis=2)
    assert lit.sum() >= 16 and (~lit).sum() >= 16  # the blurred rays still straddle the edge
    assert same_f32(host(samples), want_s).all() and np.array_equal(host(valid), want_v)
    assert np.array_equal(rng.download(), states) and int(count.item()) == want_c


# ---- the Phong power's underflow ----


def test_highlights_at_the_underflow():
    torch = torch_device()
    surfaces, view, dirs, labels, skipped = M.highlight_cases()
    want = expected_probe(surfaces, view, dirs)
    assert (want[1][0][skipped].view(np.uint32) == 0).all() and (want[1][0][~skipped] != 0).any()
    f = lambda a: torch.tensor(np.ascontiguousarray(a, dtype=F32), device="cuda")
    d, s = rt.materials.probe_surfaces(dev(surfaces), f(view), f(dirs))
    torch.cuda.synchronize()
    for name, g, w in zip(("diffuse", "specular"), (host(d), host(s)), want):
        bad = np.flatnonzero(~same_f32(g[0], w[0]).all(axis=1))
        assert bad.size == 0, f"highlights: {name} differs in {bad.size} of {len(labels)}, first: {labels[bad[0]]}: got {g[0][bad[0]]} want {w[0][bad[0]]}"
    print(f"margin: highlights: {len(labels)} records, the predicate true for {int(skipped.sum())}")
