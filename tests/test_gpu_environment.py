"""Environment queries on the device (include/rt_amd.h rt_environment_lookup / _table / _rays / _fold) and what is built from them
(environment.sky_hits, environment.miss_radiance, environment.trace_rays_levels).  Every device result is the CPU form's word for word;
the shadow rays are tied to rt_light_rays, the fold to rt_area_light_fold, the tree loop to rt_trace_rays; the two sequences replay
from a graph; and every operand of every call sits between poisoned guards that must come back untouched.  The hits are the reference
scene's primary hits of a 48 x 27 frame — spheres, triangles, bump-mapped materials and misses — made once per module."""
import numpy as np
import pytest

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import arealights, environment as E, materials
from homework_18_graphics_raytracer_amd._capi import Light
import _guard_support as G
import _scenes
from _records import NONE, dev, host, ray_records, torch_device, u32

pytestmark = pytest.mark.gpu
F32 = np.float32
WIDTH, HEIGHT = 48, 27
MIDDLE = (HEIGHT // 2) * WIDTH
T = E.ROW_TILE
TABLE_SIZES = [(1, 1), (3, 2), (64, 4), (65, 4), (T, 2), (T + 1, 2), (2 * T + 3, 3), (5, 1), (5, 257)]  # (width, height)
BATCHES = [1, 63, 64, 65, 257]


def image(width, height, seed, plain=False):
    """a random image; unless plain, with texels that may not be sampled — NaN, Inf, negative, zero — and one row without light"""
    rng = np.random.default_rng(seed)
    img = rng.random((height, width, 3), dtype=F32) * F32(4)
    if not plain and width * height >= 6:
        flat = img.reshape(-1, 3)
        k = rng.permutation(flat.shape[0])[:4]
        flat[k[0], 1], flat[k[1], 0], flat[k[2]], flat[k[3]] = np.nan, np.inf, -1.0, 0.0
        if height >= 3:
            img[height // 2] = 0
    return img


def env_of(img, rotation=0.0, scale=1.0, filter=E.BILINEAR):
    torch = torch_device()
    return E.Environment(torch.tensor(img, device="cuda"), rotation, scale, filter)


def words(a):
    a = np.ascontiguousarray(a)
    return a if a.dtype.itemsize == 1 else a.view(np.uint32)


def assert_same(got, want, what):
    g, w = words(got), words(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.flatnonzero(g.reshape(-1) != w.reshape(-1))
    assert bad.size == 0, f"{what}: {bad.size} of {g.size} words differ, first at {bad[:5]}: {g.reshape(-1)[bad[:5]]} want {w.reshape(-1)[bad[:5]]}"


class Batch:
    pass


@pytest.fixture(scope="module")
def ref():
    torch_device()
    b = Batch()
    b.world = rt.reference_world()
    b.scene = rt.Scene(b.world)
    b.rays_t = rt.camera_rays(rt.reference_camera(), rt.Frame.full(WIDTH, HEIGHT, 0))
    hits = u32(rt.cast_rays(b.scene, b.rays_t)).copy()
    solid = np.flatnonzero(hits[MIDDLE:MIDDLE + 64, 0] <= 1)
    hits[MIDDLE + solid[1], 2] = 9999  # a hit whose object_index names no material: "no hit" to every call
    b.broken = MIDDLE + int(solid[1])
    b.hits, b.hits_t = hits, dev(hits)
    b.n = hits.shape[0]
    b.surfaces_t = materials.material_hits(b.scene, b.hits_t)
    b.surfaces = host(b.surfaces_t).view(materials.SURFACE_DTYPE).reshape(-1)
    b.valid = b.surfaces["valid"] != 0
    b.shading = np.ascontiguousarray(b.surfaces["shading_normal"])
    b.geometric = np.ascontiguousarray(hits[:, 6:9]).view(F32)
    b.view_t = (-b.rays_t[:, 3:6].view(torch_device().float32)).contiguous()
    assert b.valid[MIDDLE] and not b.valid[b.broken] and not b.valid[MIDDLE:MIDDLE + 257].all() and b.valid.sum() > 600
    b.img = image(16, 8, 5)
    b.env = env_of(b.img, 0.3, 1.5)
    b.table = E.table_numpy(b.img)
    return b


# ---- the table ----

@pytest.mark.parametrize("width,height", TABLE_SIZES)
def test_the_table_is_the_cpu_forms(width, height):
    """every word, at one column, below, at and above one tile of the row scan, over two tiles, and at one, two and 257 rows (two
    tiles of the scan over the rows)"""
    torch = torch_device()
    for seed, plain in ((1, False), (2, True)):
        img = image(width, height, seed, plain)
        env = env_of(img)
        got = torch.full((E.table_bytes(width, height),), 0x5A, dtype=torch.uint8, device="cuda")
        E.table(env, out=got)
        torch.cuda.synchronize()
        assert_same(host(got), E.table_numpy(img), f"table {width} x {height}")
    dark = env_of(np.zeros((height, width, 3), dtype=F32))
    fields = E.table_fields(dark.table(), width, height)
    assert fields["total"] == 0 and fields["w_max"] == 0 and not fields["C"].any() and not fields["M"].any()


# ---- the lookup ----

def directions(n, seed):
    rng = np.random.default_rng(seed)
    d = rng.normal(0, 1, (n, 3)).astype(F32) * F32(3)
    special = [(0, 0, 0), (np.nan, 1, 0), (np.inf, 0, 1), (0, 1, 0), (0, -1, 0), (1, 0, 0), (-1, 0, -0.0), (-1, 0, 0.0)]
    for k, v in enumerate(special[:max(n - 1, 0)]):
        d[k + 1] = v
    return d


@pytest.mark.parametrize("n", BATCHES)
def test_the_lookup_is_the_cpu_forms(ref, n):
    torch = torch_device()
    d = directions(n, n)
    rays = ray_records(np.zeros((n, 3), dtype=F32), d)
    rays_t = dev(rays)
    hits = ref.hits[MIDDLE:MIDDLE + n]
    parent = np.random.default_rng(n).permutation(2 * n)[:n].astype(np.uint32)
    parent[0] = NONE
    for filter in (E.NEAREST, E.BILINEAR):
        env = env_of(ref.img, 0.3, 1.5, filter)
        with np.errstate(all="ignore"):
            assert_same(host(E.lookup(env, rays_t)), E.lookup_numpy(ref.img, rays, 0.3, 1.5, filter), "every record")
            # with hits: a hit's slot keeps the sentinel
            out = torch.full((n, 3), 99.0, dtype=torch.float32, device="cuda")
            E.lookup(env, rays_t, dev(hits), out=out)
            want = E.lookup_numpy(ref.img, rays, 0.3, 1.5, filter, hits=hits, out=np.full((n, 3), 99.0, dtype=F32))
            assert_same(host(out), want, "with hits")
            assert (host(out)[hits[:, 0] <= 1] == 99.0).all() and (n < 63 or (host(out)[hits[:, 0] > 1] != 99.0).any())
            # with parents, a count and an output that is too short: slots at or beyond n_out are not written, 0xffffffff folds nowhere
            count = max(n - 3, 1)
            short = (3 * n) // 2
            out = torch.full((short, 3), 99.0, dtype=torch.float32, device="cuda")
            E.lookup(env, rays_t, count=torch.tensor([count], dtype=torch.int32, device="cuda"), parent=dev(parent), out=out)
            want = E.lookup_numpy(ref.img, rays, 0.3, 1.5, filter, count=count, parent=parent, out=np.full((short, 3), 99.0, dtype=F32))
            assert_same(host(out), want, "with parents")
            written = np.zeros(short, dtype=bool)
            written[parent[:count][parent[:count] < short]] = True
            assert (host(out)[~written] == 99.0).all()


# ---- rays and fold ----

def run_rays(scene, env, hits_t, spp, pattern, seed, ids, kind, table=None):
    torch = torch_device()
    m = spp * hits_t.shape[0]
    rays = torch.full((m, 11), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    asks = torch.full((m,), 0x5A, dtype=torch.uint8, device="cuda")
    dirs = torch.full((m, 3), 99.0, dtype=torch.float32, device="cuda")
    radiance = torch.full((m, 3), 99.0, dtype=torch.float32, device="cuda")
    texel = torch.full((m,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    ids_t = None if ids is None else torch.tensor(np.asarray(ids).astype(np.uint32).view(np.int32), device="cuda")
    E.rays(scene, env, hits_t, spp, pattern, seed, ids_t, kind, table, rays, asks, dirs, radiance, texel)
    torch.cuda.synchronize()
    return (u32(rays), host(asks), host(dirs), host(radiance), u32(texel)), (rays, asks, dirs, radiance, texel)


def ids_of(n):
    return (np.arange(n, dtype=np.uint32) * np.uint32(2654435761)) ^ np.uint32(0x80000001)


def want_rays(hits, asks, dirs, spp):
    n = hits.shape[0]
    want = np.zeros((spp, n, 11), dtype=np.uint32)
    want[..., 0:3] = hits[None, :, 3:6]
    want[..., 3:6] = dirs.reshape(spp, n, 3).view(np.uint32)
    want[..., 6], want[..., 7], want[..., 8], want[..., 9], want[..., 10] = 1, 1, hits[None, :, 0], hits[None, :, 1], 1
    want[asks.reshape(spp, n) == 0] = 0
    return want.reshape(spp * n, 11)


@pytest.mark.parametrize("n", BATCHES)
def test_rays_and_fold_are_the_cpu_forms(ref, n):
    """dirs, asks, radiance and texel against samples_numpy, the rays restated from them, then the casts, the probes and the fold
    against fold_numpy: 1, 4 and 16 samples, both patterns, both normals, with and without ids"""
    torch = torch_device()
    rows = slice(MIDDLE, MIDDLE + n)
    hits_t, hits, valid = ref.hits_t[rows].contiguous(), ref.hits[rows], ref.valid[rows]
    asked = opened = blocked = 0
    for spp in (1, 4, 16):
        for pattern in (E.UNIFORM, E.STRATIFIED):
            kind = (spp + pattern) % 2
            normals = (ref.shading, ref.geometric)[kind][rows]
            ids = ids_of(n) if spp != 4 else None
            (rays, asks, dirs, radiance, texel), (rays_t, asks_t, dirs_t, radiance_t, _) = run_rays(ref.scene, ref.env, hits_t, spp, pattern, 11 + spp, ids, kind)
            with np.errstate(all="ignore"):
                want = E.samples_numpy(ref.img, ref.table, normals, spp, pattern, 11 + spp, ids, 0.3, 1.5)
            for a in want:
                a[:, ~valid] = 0
            what = f"spp {spp}, pattern {pattern}, kind {kind}"
            assert_same(dirs.reshape(spp, n, 3), want[0], "dirs: " + what)
            assert_same(radiance.reshape(spp, n, 3), want[1], "radiance: " + what)
            assert_same(texel.reshape(spp, n), want[2], "texel: " + what)
            assert_same(asks.reshape(spp, n), want[3], "asks: " + what)
            assert_same(rays, want_rays(hits, asks, dirs, spp), "rays: " + what)
            asked += int(asks.sum())
            # the casts, the probes, the fold
            sh_t = torch.full((spp * n, 13), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
            index, count = rt.select_records(asks_t)
            rt.cast_rays_indexed(ref.scene, rays_t, index, count, sh_t)
            diffuse_t, specular_t = materials.probe_surfaces(ref.surfaces_t[rows].contiguous(), ref.view_t[rows].contiguous(), dirs_t.view(spp, n, 3))
            rgb = np.random.default_rng(spp).random((n, 3), dtype=F32)
            shiness = np.ascontiguousarray(ref.surfaces["shiness"][rows])
            for shadow in (sh_t, None):
                out_t, open_t = torch.tensor(rgb, device="cuda"), torch.full((spp * n,), 0x5A, dtype=torch.uint8, device="cuda")
                E.fold(ref.scene, hits_t, asks_t, spp, radiance_t, diffuse_t, specular_t, out_t, shadow, open_t)
                torch.cuda.synchronize()
                with np.errstate(all="ignore"):
                    want_open, want_rgb = E.fold_numpy(valid, shiness, asks, spp, radiance, host(diffuse_t), host(specular_t), rgb,
                                                       None if shadow is None else u32(shadow))
                assert_same(host(open_t), want_open, "open: " + what)
                assert_same(host(out_t), want_rgb, "rgb: " + what)
                assert_same(host(out_t)[~valid], rgb[~valid], "a record that is no hit is not written")
                if shadow is not None:
                    opened += int(want_open.sum())
                    blocked += int(asks.sum() - want_open.sum())
    assert asked > 0 and (n < 63 or (opened > 0 and blocked > 0))


def test_a_table_of_another_size_and_a_dark_sky_ask_nothing(ref):
    hits_t = ref.hits_t[MIDDLE:MIDDLE + 65].contiguous()
    torch = torch_device()
    other = ref.env.table().clone()
    other.view(torch.int32)[0] = 15  # the header names another width
    for env, table in ((ref.env, other), (env_of(np.zeros((8, 16, 3), dtype=F32)), None)):
        got, _ = run_rays(ref.scene, env, hits_t, 4, E.UNIFORM, 1, None, E.SHADING, table)
        assert all(not a.any() for a in got)


# ---- anchors to existing calls ----

def test_the_shadow_rays_are_the_light_queries(ref):
    """four hits x two samples: rt_light_rays on a directional light whose direction is -dir gives the same ray and the same flag"""
    torch = torch_device()
    scene = rt.Scene(ref.world)
    spp = 2
    got, _ = run_rays(scene, ref.env, ref.hits_t, spp, E.UNIFORM, 5, None, E.SHADING)
    rays, asks, dirs = (a.reshape(spp, ref.n, *a.shape[1:]) for a in got[:3])
    both = np.flatnonzero(ref.valid & (asks == 1).all(axis=0))
    mixed = np.flatnonzero(ref.valid & (asks.sum(axis=0) == 1))
    records = [int(both[0]), int(both[-1]), int(mixed[0]), int(mixed[-1])]
    stored = ref.world.desc().lights[0]
    seen = set()
    try:
        for i in records:
            for s in range(spp):
                l = Light()
                l.kind, l.has_origin, l.origin = 0, 0, (0.0, 0.0, 0.0)
                l.direction = tuple(float(-v) for v in dirs[s, i])
                l.angle, l.softness, l.color = 0.5, 1.0, (1.0, 1.0, 1.0)
                scene.update_lights(0, [l])
                want, want_asks, _ = rt.light_rays(scene, ref.hits_t[i:i + 1].contiguous(), ref.rays_t[i:i + 1].contiguous(), 0, 1)
                torch.cuda.synchronize()
                assert int(host(want_asks)[0]) == int(asks[s, i]), (i, s)
                assert_same(rays[s, i], u32(want)[0], f"record {i}, sample {s}: ray")
                seen.add(int(asks[s, i]))
    finally:
        scene.update_lights(0, [stored])
    assert seen == {0, 1}


def test_the_fold_with_unit_radiance_is_the_area_lights(ref):
    torch = torch_device()
    spp, n = 4, ref.n
    _, (rays_t, asks_t, dirs_t, _, _) = run_rays(ref.scene, ref.env, ref.hits_t, spp, E.STRATIFIED, 2, None, E.SHADING)
    sh_t = torch.full((spp * n, 13), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    index, count = rt.select_records(asks_t)
    rt.cast_rays_indexed(ref.scene, rays_t, index, count, sh_t)
    diffuse_t, specular_t = materials.probe_surfaces(ref.surfaces_t, ref.view_t, dirs_t.view(spp, n, 3))
    start = torch.tensor(np.random.default_rng(0).random((n, 3), dtype=F32), device="cuda")
    got, open_t = start.clone(), torch.empty((spp * n,), dtype=torch.uint8, device="cuda")
    E.fold(ref.scene, ref.hits_t, asks_t, spp, torch.ones((spp * n, 3), dtype=torch.float32, device="cuda"), diffuse_t, specular_t, got, sh_t, open_t)
    want = start.clone()
    arealights.fold(ref.scene, ref.hits_t, open_t, diffuse_t.view(spp * n, 3), specular_t.view(spp * n, 3), want, spp)
    torch.cuda.synchronize()
    assert 0 < int(open_t.sum()) < int(asks_t.sum())
    assert_same(host(got), host(want), "fold(radiance = 1) against rt_area_light_fold(lit = open)")


def frame_rays(width=40, height=30):
    return rt.camera_rays(rt.reference_camera(), rt.Frame.full(width, height, 0))


def test_a_black_sky_in_the_tree_loop_is_trace_rays(ref):
    torch = torch_device()
    rays_t = frame_rays()
    n = rays_t.shape[0]
    env = env_of(np.zeros((4, 8, 3), dtype=F32))
    a, b = (torch.zeros(1, dtype=torch.int64, device="cuda") for _ in range(2))
    want = rt.trace_rays(ref.scene, rays_t, 3, ray_count=a)
    got = E.trace_rays_levels(ref.scene, rays_t, 3, ray_count=b, level_capacity=lambda level: 2 * n, environment=env)
    plain = E.trace_rays_levels(ref.scene, rays_t, 3, level_capacity=lambda level: 2 * n)
    torch.cuda.synchronize()
    assert_same(host(got), host(want), "values")
    assert_same(host(plain), host(want), "environment=None")
    assert int(a.item()) == int(b.item()) > n


def test_depth_0_is_the_shade_or_the_sky(ref):
    torch = torch_device()
    rays_t = frame_rays()
    hit = u32(rt.cast_rays(ref.scene, rays_t))[:, 0] <= 1
    got = host(E.trace_rays_levels(ref.scene, rays_t, 0, environment=ref.env))
    want = host(rt.trace_rays(ref.scene, rays_t, 0))
    want[~hit] = E.lookup_numpy(ref.img, u32(rays_t), 0.3, 1.5, E.BILINEAR)[~hit]
    assert hit.any() and (~hit).any() and want[~hit].any()
    assert_same(got, want, "depth 0")


def test_a_mirror_returns_the_sky_it_reflects(ref):
    """one triangle, shiness 1, transparency 0, depth 1: (shade * sc + L * rc) + 0 * fc from tree_split's weights and lookup_numpy of
    reflect_rays' output; the ray that misses the triangle returns the sky behind it"""
    torch = torch_device()
    rng = np.random.default_rng(4)
    m = _scenes.material(rng, "plain")
    m.shiness, m.transparency = 1.0, 0.0
    world = rt.World()
    world.push_object(m).push_flat_triangle([(-4, -3, -3), (4, -3, -3), (0, 5, -3.5)], [(0, 0), (1, 0), (0, 1)])
    world.push_light(_scenes.light(rng, 0))
    scene = rt.Scene(world)
    d = np.array([(0.1, 0.05, -1), (-0.3, 0.2, -1), (0.2, -0.3, -1), (0, 0.4, -1), (0.5, 0, -1), (0, 0, 1)], dtype=F32)
    rays = ray_records(np.zeros((6, 3), dtype=F32), d)
    rays_t = dev(rays)
    got = host(E.trace_rays_levels(scene, rays_t, 1, environment=ref.env))
    hits_t = rt.cast_rays(scene, rays_t)
    hit = u32(hits_t)[:, 0] <= 1
    assert hit[:5].all() and not hit[5]
    h_shade, h_reflect, _, weights = rt.tree_split(scene, hits_t, torch.ones(6, dtype=torch.float32, device="cuda"), 1)
    shade = host(rt.shade_hits(scene, h_shade, rays_t))
    reflected = u32(rt.reflect_rays(h_reflect, rays_t))
    w = host(weights)
    sc, rc, fc = w[:, 0:1], w[:, 1:2], w[:, 2:3]
    assert (sc[:5] == 0).all() and (rc[:5] == 1).all() and (fc[:5] == 0).all()
    sky = E.lookup_numpy(ref.img, reflected, 0.3, 1.5, E.BILINEAR)
    want = (shade * sc + sky * rc) + np.zeros((6, 3), dtype=F32) * fc
    want[5] = E.lookup_numpy(ref.img, rays[5:], 0.3, 1.5, E.BILINEAR)[0]
    assert want.dtype == F32 and want[:5].any()
    assert_same(got, want, "the mirror")


# ---- capture ----

def test_the_sequences_replay_from_a_graph(ref):
    torch = torch_device()
    n, spp = ref.n, 4
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        w = E.workspace(n, "cuda", spp)
        sky, behind = torch.zeros((n, 3), dtype=torch.float32, device="cuda"), torch.zeros((n, 3), dtype=torch.float32, device="cuda")
        hits = torch.empty((n, 13), dtype=torch.int32, device="cuda")

        def run():
            sky.zero_()
            E.sky_hits(ref.scene, ref.env, ref.hits_t, ref.view_t, spp, sky, E.STRATIFIED, 3, stream=stream, workspace=w)
            E.miss_radiance(ref.scene, ref.env, ref.rays_t, behind, hits, stream=stream)

        run()  # the warm-up: the table, the selection's totals and the cast's lists are made here
        stream.synchronize()
        want = host(sky).copy(), host(behind).copy()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            run()
        sky.fill_(7.0)
        behind.fill_(7.0)
        graph.replay()
        stream.synchronize()
    assert want[0].any() and want[1].any()
    assert_same(host(sky), want[0], "sky_hits replayed")
    miss = ref.hits[:, 0] > 1
    miss[ref.broken] = False  # the cast's own record there is a hit
    assert_same(host(behind)[miss], want[1][miss], "miss_radiance replayed")
    assert (host(behind)[~miss] == 7.0).all()  # a hit's slot is left as it was


# ---- no call writes outside its operands ----

def test_every_operand_stays_between_its_guards(ref):
    torch = torch_device()
    n, spp, width, height = 65, 4, 2 * T + 3, 3
    img = image(width, height, 9)
    env = env_of(img, 0.3, 1.5)
    held = []

    def operand(shape, dtype):
        count = int(np.prod(shape))
        size = torch.empty((), dtype=dtype).element_size()
        payload = (count * size + 3) // 4
        whole, view = G.guarded(payload, G.SENTINEL, form="cuda")
        held.append((whole, G.guard_words(payload), payload))
        return view.view(torch.uint8)[:count * size].view(dtype).view(*shape)

    table = operand((E.table_bytes(width, height),), torch.uint8)  # at table_bytes exactly
    E.table(env, out=table)
    hits_t = ref.hits_t[MIDDLE:MIDDLE + n].contiguous()
    m = spp * n
    rays, asks, dirs = operand((m, 11), torch.int32), operand((m,), torch.uint8), operand((m, 3), torch.float32)
    radiance, texel = operand((m, 3), torch.float32), operand((m,), torch.int32)
    E.rays(ref.scene, env, hits_t, spp, E.UNIFORM, 1, None, E.SHADING, table, rays, asks, dirs, radiance, texel)
    diffuse_t, specular_t = materials.probe_surfaces(ref.surfaces_t[MIDDLE:MIDDLE + n].contiguous(), ref.view_t[MIDDLE:MIDDLE + n].contiguous(), dirs.view(spp, n, 3))
    rgb, open_t = operand((n, 3), torch.float32), operand((m,), torch.uint8)
    rgb.zero_()
    E.fold(ref.scene, hits_t, asks, spp, radiance, diffuse_t, specular_t, rgb, None, open_t)
    out = operand((n, 3), torch.float32)
    E.lookup(env, ref.rays_t[MIDDLE:MIDDLE + n].contiguous(), out=out)
    torch.cuda.synchronize()
    assert_same(host(table), E.table_numpy(img), "the guarded table")
    assert asks.any() and np.isfinite(host(out)).any()
    for whole, guard, payload in held:
        w = u32(whole)
        assert (w[:guard] == G.SENTINEL).all() and (w[guard + payload:] == G.SENTINEL).all(), "a store outside an operand"
