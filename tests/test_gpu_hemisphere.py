"""Hemisphere queries on the device (include/rt_amd.h rt_hemisphere_rays / rt_hemisphere_fold) and the loops built from them
(hemisphere.ambient_hits, hemisphere.indirect_hits).  The directions are the CPU form's word for word, the rays are restated field by
field and tied to rt_light_rays on a directional light of direction -dir, the fold is the CPU form's word for word, and a floor inside
a sphere gives ambient values that are exact.  The hits are the reference scene's primary hits of a 48 x 27 frame — spheres, triangles,
glass, bump-mapped materials and misses — made once per module.  Every comparison is of u32 words."""
import numpy as np
import pytest

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import hemisphere, materials
from homework_18_graphics_raytracer_amd._capi import Light
import _scenes
from _records import dev, host, oracle_hits, ray_records, same_f32, torch_device, u32, valid_rows

pytestmark = pytest.mark.gpu
UNIFORM, STRATIFIED = hemisphere.UNIFORM, hemisphere.STRATIFIED
SHADING, GEOMETRIC = hemisphere.SHADING, hemisphere.GEOMETRIC
F32 = np.float32
WIDTH, HEIGHT = 48, 27
MIDDLE = (HEIGHT // 2) * WIDTH  # the slices start in the middle row: objects, not sky
SIZES = [1, 63, 64, 65, 256, 257, WIDTH * HEIGHT]  # below, at and above a wave and a workgroup; the whole frame is six workgroups


class Batch:
    pass


@pytest.fixture(scope="module")
def ref():
    torch_device()
    b = Batch()
    b.world = rt.reference_world()
    b.scene = rt.Scene(b.world)
    b.rays_t = rt.camera_rays(rt.reference_camera(), rt.Frame.full(WIDTH, HEIGHT, 0))
    b.hits_t = rt.cast_rays(b.scene, b.rays_t)
    b.hits = u32(b.hits_t).copy()
    b.n = b.hits.shape[0]
    b.surfaces = host(materials.material_hits(b.scene, b.hits_t)).view(materials.SURFACE_DTYPE).reshape(-1)
    b.valid = b.surfaces["valid"] != 0
    b.shading = np.ascontiguousarray(b.surfaces["shading_normal"])
    b.geometric = np.ascontiguousarray(b.hits[:, 6:9]).view(F32)
    assert b.n == 1296 and 600 <= b.valid.sum() < b.n  # hits, and misses
    assert set(np.unique(b.hits[b.valid, 0])) == {0, 1}  # spheres and triangles
    b.bumped = b.valid & (b.shading.view(np.uint32) != b.geometric.view(np.uint32)).any(axis=1)
    assert (b.bumped & (b.hits[:, 0] == 0)).any()  # a bump-mapped sphere
    assert b.valid[MIDDLE] and not b.valid[MIDDLE:MIDDLE + 257].all()
    return b


def words(a):
    a = np.ascontiguousarray(a)
    return a if a.dtype.itemsize == 1 else a.view(np.uint32)


def assert_same(got, want, what):
    g, w = words(got), words(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.flatnonzero(g.reshape(-1) != w.reshape(-1))
    assert bad.size == 0, f"{what}: {bad.size} of {g.size} words differ, first at {bad[:5]}: {g.reshape(-1)[bad[:5]]} want {w.reshape(-1)[bad[:5]]}"


def ids_of(n):
    ids = (np.arange(n, dtype=np.uint32) * np.uint32(2654435761)) ^ np.uint32(0x80000001)  # distinct, some above 2^31
    assert np.unique(ids).size == n
    return ids


def run_rays(scene, hits_t, spp, pattern, seed, ids, kind):
    """rt_hemisphere_rays with every output filled with a sentinel first: (rays, asks, dirs) on the host, and the tensors"""
    torch = torch_device()
    m = spp * hits_t.shape[0]
    rays = torch.full((m, 11), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    asks = torch.full((m,), 0x5A, dtype=torch.uint8, device="cuda")
    dirs = torch.full((m, 3), 99.0, dtype=torch.float32, device="cuda")
    ids_t = None if ids is None else torch.tensor(np.asarray(ids).astype(np.uint32).view(np.int32), device="cuda")
    hemisphere.rays(scene, hits_t, spp, pattern, seed, ids_t, kind, out_rays=rays, out_asks=asks, out_dirs=dirs)
    torch.cuda.synchronize()
    return (u32(rays), host(asks), host(dirs)), (rays, asks, dirs)


def check_rays(hits, valid, normals, spp, got):
    """d_rays and d_asks restated field by field from d_dirs"""
    rays, asks, dirs = got
    n = hits.shape[0]
    d = dirs.reshape(spp, n, 3)
    nn = normals[None]
    with np.errstate(all="ignore"):
        dot = (d[..., 0] * nn[..., 0] + d[..., 1] * nn[..., 1]) + d[..., 2] * nn[..., 2]  # rt_vec.h's order, each step rounded to f32
    assert dot.dtype == F32
    want_asks = (~(dot <= 0)) & valid[None]
    assert_same(asks.reshape(spp, n), want_asks.astype(np.uint8), "asks")
    r = rays.reshape(spp, n, 11)
    want = np.zeros((spp, n, 11), dtype=np.uint32)
    want[..., 0:3] = hits[None, :, 3:6]      # the origin words are the hit's
    want[..., 3:6] = d.view(np.uint32)       # the direction is d_dirs
    want[..., 6] = 1                         # Back
    want[..., 7] = 1                         # an exclusion ...
    want[..., 8] = hits[None, :, 0]          # ... { kind, index, Back }
    want[..., 9] = hits[None, :, 1]
    want[..., 10] = 1
    want[~want_asks] = 0                     # un-asked and "no hit" entries are zero words
    assert_same(r, want, "rays")
    assert (words(d)[:, ~valid] == 0).all()  # "no hit": zero words in d_dirs
    return want_asks


@pytest.mark.parametrize("n", SIZES)
def test_directions_and_rays(ref, n):
    """d_dirs equals dirs_numpy on rt_material_hits' shading_normal (kind 0) and on hit.normal (kind 1), word for word; the rays and
    the flags are restated from them"""
    start = 0 if n == ref.n else MIDDLE
    rows = slice(start, start + n)
    hits_t, hits, valid = ref.hits_t[rows].contiguous(), ref.hits[rows], ref.valid[rows]
    asked = 0
    for spp in (1, 4, 9, 64):
        for pattern in (UNIFORM, STRATIFIED):
            for kind, normals in ((SHADING, ref.shading[rows]), (GEOMETRIC, ref.geometric[rows])):
                ids = ids_of(n) if (spp + pattern + kind) % 2 else None  # explicit ids in half of the cases
                got, _ = run_rays(ref.scene, hits_t, spp, pattern, 17 + spp, ids, kind)
                with np.errstate(all="ignore"):
                    want = hemisphere.dirs_numpy(normals, spp, pattern, 17 + spp, ids)
                want[:, ~valid] = 0
                assert_same(got[2].reshape(spp, n, 3), want, f"dirs: spp {spp}, pattern {pattern}, kind {kind}")
                asked += check_rays(hits, valid, normals, spp, got).sum()
    assert asked > 0
    if n >= 256:
        got, _ = run_rays(ref.scene, hits_t, 4, UNIFORM, 3, np.arange(n), SHADING)
        none, _ = run_rays(ref.scene, hits_t, 4, UNIFORM, 3, None, SHADING)
        for a, b in zip(got, none):
            assert_same(a, b, "ids 0 .. n - 1 against NULL ids")


def test_the_tie_to_the_light_queries(ref):
    """three records x two samples, one of them on a bump-mapped sphere: rt_light_rays on a directional light without origin whose
    direction is -dir gives the same ray and the same ask bit"""
    torch = torch_device()
    scene = rt.Scene(ref.world)
    spp = 2
    got, _ = run_rays(scene, ref.hits_t, spp, UNIFORM, 5, ids_of(ref.n), SHADING)
    rays, asks, dirs = (a.reshape(spp, ref.n, *a.shape[1:]) for a in got)
    sphere = np.flatnonzero(ref.bumped & (ref.hits[:, 0] == 0) & (asks == 1).all(axis=0))
    triangle = np.flatnonzero(ref.valid & (ref.hits[:, 0] == 1))
    records = [int(sphere[sphere.size // 2]), int(triangle[0]), int(triangle[-1])]
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
                want_rays, want_asks, _ = rt.light_rays(scene, ref.hits_t[i:i + 1].contiguous(), ref.rays_t[i:i + 1].contiguous(), 0, 1)
                torch.cuda.synchronize()
                assert_same(rays[s, i], u32(want_rays)[0], f"record {i}, sample {s}: ray")
                assert int(host(want_asks)[0]) == int(asks[s, i]), (i, s)
                seen.add(int(asks[s, i]))
    finally:
        scene.update_lights(0, [stored])
    assert 1 in seen


def shadow_casts(scene, rays_t, asks_t):
    """select_records -> cast_rays_indexed on a sentinel-filled output, and the number of casts"""
    torch = torch_device()
    sh = torch.full((rays_t.shape[0], 13), 0x5A5A5A5A, dtype=torch.int32, device="cuda")  # kind 0x5a5a5a5a: neither 0 nor 1
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    index, count = rt.select_records(asks_t)
    rt.cast_rays_indexed(scene, rays_t, index, count, sh, ray_count=cnt)
    torch.cuda.synchronize()
    return sh, int(host(cnt)[0])


def device_fold(scene, hits_t, asks_t, spp, sh_t, max_distance, radiance_t, rgb):
    torch = torch_device()
    n = hits_t.shape[0]
    open_t = torch.full((spp * n,), 0x5A, dtype=torch.uint8, device="cuda")
    ambient_t = torch.full((n,), 7.0, dtype=torch.float32, device="cuda")
    out_t = None if rgb is None else torch.tensor(rgb, device="cuda")
    hemisphere.fold(scene, hits_t, asks_t, spp, sh_t, max_distance, radiance_t, out_t, open_t, ambient_t)
    torch.cuda.synchronize()
    return host(open_t), host(ambient_t), (None if out_t is None else host(out_t))


@pytest.mark.parametrize("n,spp", [(1296, 4), (257, 16), (65, 1)])
def test_the_fold_is_the_cpu_forms(ref, n, spp):
    """open, ambient and rgb against fold_numpy, word for word: with and without shadow hits, max_distance inf and finite, on an rgb
    that was not zero before"""
    torch = torch_device()
    start = 0 if n == ref.n else MIDDLE
    rows = slice(start, start + n)
    hits_t, hits, valid = ref.hits_t[rows].contiguous(), ref.hits[rows], ref.valid[rows]
    colour, shiness = np.ascontiguousarray(ref.surfaces["diffuse_color"][rows]), np.ascontiguousarray(ref.surfaces["shiness"][rows])
    (_, asks, _), (rays_t, asks_t, _) = run_rays(ref.scene, hits_t, spp, STRATIFIED, 9, ids_of(n), SHADING)
    sh_t, casts = shadow_casts(ref.scene, rays_t, asks_t)
    sh = u32(sh_t)
    assert casts == asks.sum() > 0
    answered = (asks == 1) & (sh[:, 0] <= 1)
    assert answered.any() and ((asks == 1) & ~answered).any()  # some directions are blocked, some are not
    rng = np.random.default_rng(n)
    radiance = rng.uniform(0, 3, (spp * n, 3)).astype(F32)
    radiance[asks == 0] = np.nan  # never read
    rgb = rng.uniform(0, 1, (n, 3)).astype(F32)
    radiance_t = torch.tensor(radiance, device="cuda")
    d = sh[answered, 3:6].view(F32) - np.repeat(hits[None, :, 3:6], spp, axis=0).reshape(-1, 3)[answered].view(F32)
    finite = float(np.median(np.sqrt((d.astype(np.float64) ** 2).sum(axis=1))))  # between the occluders: some nearer, some farther
    ambients = {}
    for shadow in (True, False):
        for max_distance in (np.inf, finite):
            want = hemisphere.fold_numpy(hits, valid, colour, shiness, asks, spp, sh if shadow else None, max_distance, radiance, rgb)
            got = device_fold(ref.scene, hits_t, asks_t, spp, sh_t if shadow else None, max_distance, radiance_t, rgb)
            for name, g, w in zip(("open", "ambient", "rgb"), got, want):
                assert_same(g, w, f"shadow hits {shadow}, max_distance {max_distance}: {name}")
            assert not np.isnan(got[2]).any()
            assert (words(got[2])[~valid] == words(rgb)[~valid]).all() and (got[1][~valid] == 0).all()  # "no hit": not written, ambient 0
            ambients[shadow, max_distance] = got[1]
    assert (ambients[True, np.inf] <= ambients[True, finite]).all() and (ambients[True, np.inf] < ambients[True, finite]).any()
    assert_same(ambients[False, np.inf], ambients[False, finite], "NULL shadow hits: max_distance is not looked at")
    # without the bounce: the same flags, no rgb
    got = device_fold(ref.scene, hits_t, asks_t, spp, sh_t, np.inf, None, None)
    assert got[2] is None
    assert_same(got[1], ambients[True, np.inf], "ambient without the bounce")


# ---- closed forms: a floor through the centre of a sphere ----

R = 2.0


def floor_world(with_sphere):
    rng = np.random.default_rng(3)
    w = rt.World()
    plain = _scenes.material(rng, "plain")
    plain.transparency = 0.0
    w.push_object(plain).push_square([(-3, 0, -3), (-3, 0, 3), (3, 0, 3), (3, 0, -3)], [(0, 0), (0, 1), (1, 0), (0, 1)])
    if with_sphere:
        w.push_object(_scenes.material(rng, "plain")).push_sphere((0.0, 0.0, 0.0), R)
    l = Light()
    l.kind, l.has_origin, l.direction, l.color = 0, 0, (0.0, -1.0, 0.0), (1.0, 1.0, 1.0)
    w.push_light(l)
    return w


def oracle_answers(desc, rays, asks):
    """orc_cast of every asked ray: (answered, distance from the ray's origin)"""
    hits = oracle_hits(desc, rays[asks == 1])
    d = hits[:, 3:6].view(F32).astype(np.float64) - rays[asks == 1][:, 0:3].view(F32).astype(np.float64)
    return hits[:, 0] <= 1, np.sqrt((d * d).sum(axis=1))


def test_closed_forms_are_exact():
    """a floor through the centre of a sphere of radius R, hits on the floor within R / 4 of the centre: alone every direction is open;
    inside the sphere every direction meets its inner side — a back face, which a Back ray sees — at a distance between 3R/4 and 5R/4,
    so max_distance inf closes every sample and R/2 opens every one.  The three cases are confirmed by the oracle's cast first."""
    torch_device()
    alone, inside = floor_world(False), floor_world(True)
    xs = (np.arange(5) - 2) * 0.14 + 0.03
    origins = np.array([(x, 0.5, z + 0.05) for z in xs for x in xs], dtype=F32)  # clear of the quad's diagonal
    assert (np.sqrt(origins[:, 0] ** 2 + origins[:, 2] ** 2) <= R / 4).all()
    primary = ray_records(origins, np.tile(np.array([0.0, -1.0, 0.0], dtype=F32), (origins.shape[0], 1)))
    hits = oracle_hits(alone.desc(), primary)
    assert valid_rows(alone.desc(), hits).all() and (hits[:, 0] == 1).all()
    hits_t = dev(hits)
    n = hits.shape[0]
    for spp, pattern in ((16, STRATIFIED), (7, UNIFORM)):
        for world, max_distance, want in ((alone, np.inf, 1.0), (inside, np.inf, 0.0), (inside, R / 2, 1.0)):
            scene = rt.Scene(world)
            (rays, asks, _), _ = run_rays(scene, hits_t, spp, pattern, 1, None, SHADING)
            assert (asks == 1).all()  # every direction leaves the floor: no u_0 of this seed rounds to 1
            answered, distance = oracle_answers(world.desc(), rays, asks)
            if world is alone:
                assert not answered.any()
            else:
                assert answered.all() and (distance > 0.75 * R - 1e-3).all() and (distance < 1.25 * R + 1e-3).all()
            got = hemisphere.ambient_hits(scene, hits_t, spp, max_distance, pattern, 1)
            assert (host(got) == F32(want)).all(), (spp, max_distance, host(got))
            assert host(got).shape == (n,)


# ---- the loops ----


def no_sync(fn):
    """fn() with every synchronising torch call inside it an error: no host visit hides there"""
    torch = torch_device()
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = fn()
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    return out


def test_ambient_hits_is_the_sequence(ref):
    """ambient_hits equals the calls written out one by one, and casts one ray per set flag"""
    torch = torch_device()
    spp, seed, n = 4, 21, ref.n
    ids = ids_of(n)
    ids_t = torch.tensor(ids.view(np.int32), device="cuda")
    (_, asks, _), (rays_t, asks_t, _) = run_rays(ref.scene, ref.hits_t, spp, STRATIFIED, seed, ids, GEOMETRIC)
    sh_t, casts = shadow_casts(ref.scene, rays_t, asks_t)
    for max_distance in (np.inf, 1.5):
        want_open, want_ambient, _ = device_fold(ref.scene, ref.hits_t, asks_t, spp, sh_t, max_distance, None, None)
        out = torch.full((n,), 7.0, dtype=torch.float32, device="cuda")
        flags = torch.full((spp * n,), 0x5A, dtype=torch.uint8, device="cuda")
        cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        w = hemisphere.workspace(n, "cuda", spp)
        got = no_sync(lambda: hemisphere.ambient_hits(ref.scene, ref.hits_t, spp, max_distance, STRATIFIED, seed, ids_t, GEOMETRIC, out=out, open=flags,
                                                      ray_count=cnt, workspace=w))
        assert got is out
        assert_same(host(out), want_ambient, f"max_distance {max_distance}: ambient")
        assert_same(host(flags), want_open, f"max_distance {max_distance}: open")
        assert int(host(cnt)[0]) == casts == int(asks.sum())
    values = np.unique(want_ambient)
    assert values.size > 2 and set(values * spp) <= set(range(spp + 1))
    fresh = no_sync(lambda: hemisphere.ambient_hits(ref.scene, ref.hits_t, spp, 1.5, STRATIFIED, seed, ids_t, GEOMETRIC))  # its own buffers
    assert_same(host(fresh), want_ambient, "without a workspace")


def test_indirect_hits_is_trace_rays_folded(ref):
    """indirect_hits on a zeroed out equals fold_numpy fed with trace_rays' output"""
    torch = torch_device()
    spp, seed, depth, n = 4, 8, 2, ref.n
    (_, asks, _), (rays_t, _, _) = run_rays(ref.scene, ref.hits_t, spp, STRATIFIED, seed, None, SHADING)
    radiance = host(rt.trace_rays(ref.scene, rays_t, depth, 1.0))
    colour, shiness = np.ascontiguousarray(ref.surfaces["diffuse_color"]), np.ascontiguousarray(ref.surfaces["shiness"])
    zero = np.zeros((n, 3), dtype=F32)
    _, _, want = hemisphere.fold_numpy(ref.hits, ref.valid, colour, shiness, asks, spp, None, np.inf, radiance, zero)
    out = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
    w = hemisphere.workspace(n, "cuda", spp)
    got = no_sync(lambda: hemisphere.indirect_hits(ref.scene, ref.hits_t, spp, depth, 1.0, out, STRATIFIED, seed, workspace=w))
    assert got is out
    assert same_f32(host(out), want).all()
    lit = (host(out) != 0).any(axis=1)
    assert lit.any() and not lit[~ref.valid].any()  # light arrives from other surfaces; "no hit" records stay as they were
    fresh = no_sync(lambda: hemisphere.indirect_hits(ref.scene, ref.hits_t, spp, depth, 1.0, None, STRATIFIED, seed))  # a new, zeroed out
    assert same_f32(host(fresh), want).all()


def test_rays_and_fold_in_a_graph(ref):
    """rays -> fold(shadow_hits=None) captured into one graph on a side stream, with no call of either before it on a scene of its own;
    replayed onto cleared outputs it gives the uncaptured bits.  A chain: the graph has no parallel branches."""
    torch = torch_device()
    scene = rt.Scene(ref.world)
    spp, n = 4, ref.n
    m = spp * n
    rays = torch.empty((m, 11), dtype=torch.int32, device="cuda")
    asks, open_ = torch.empty((m,), dtype=torch.uint8, device="cuda"), torch.empty((m,), dtype=torch.uint8, device="cuda")
    dirs = torch.empty((m, 3), dtype=torch.float32, device="cuda")
    ambient = torch.empty((n,), dtype=torch.float32, device="cuda")
    outs = (rays, asks, dirs, open_, ambient)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            hemisphere.rays(scene, ref.hits_t, spp, STRATIFIED, 6, None, SHADING, out_rays=rays, out_asks=asks, out_dirs=dirs, stream=stream)
            hemisphere.fold(scene, ref.hits_t, asks, spp, open=open_, ambient=ambient, stream=stream)
    torch.cuda.synchronize()
    for t in outs:
        t.zero_()
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    replayed = [host(t).copy() for t in outs]
    (e_rays, e_asks, e_dirs), (_, asks_t, _) = run_rays(scene, ref.hits_t, spp, STRATIFIED, 6, None, SHADING)
    e_open, e_ambient, _ = device_fold(scene, ref.hits_t, asks_t, spp, None, np.inf, None, None)
    for name, got, want in zip(("rays", "asks", "dirs", "open", "ambient"), replayed, (e_rays, e_asks, e_dirs, e_open, e_ambient)):
        assert_same(got, want, f"replay: {name}")
    assert (e_open == e_asks).all() and e_asks.any()
