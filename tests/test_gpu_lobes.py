"""Lobe queries on the device (include/rt_amd.h rt_lobe_rays / rt_lobe_pdf / rt_environment_pdf / rt_mis_weigh) and what is built from
them (lobes.glossy_hits, lobes.sky_hits_mis).  Every device result is the CPU form's word for word; a scene without shiness gets
rt_hemisphere_rays' words; the sampler's density is rt_lobe_pdf of its directions; sky_hits_mis without lobe samples is
environment.sky_hits; glossy_hits is its sequence call by call and environment.fold_numpy of its intermediates; both sequences replay
from a graph; and every operand of every new call sits between poisoned guards that must come back untouched.  The hits are the
reference scene's primary hits of a 48 x 27 frame — spheres, triangles, bump-mapped materials and misses — made once per module."""
import ctypes as C

import numpy as np
import pytest

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import environment as E, hemisphere, lobes as L, materials
import _guard_support as G
import _scenes  # noqa: F401  (the scene builders' module, as the environment tests import it)
from _lobe_support import assert_same
from _records import dev, host, torch_device, u32

pytestmark = pytest.mark.gpu
F32 = np.float32
WIDTH, HEIGHT = 48, 27
MIDDLE = (HEIGHT // 2) * WIDTH
BATCHES = [1, 63, 64, 65, 257]
SAMPLES = [(1, L.UNIFORM), (4, L.STRATIFIED), (5, L.UNIFORM), (64, L.STRATIFIED)]
SKIES = [(8, 4), (37, 19)]


def sky(width, height, seed):
    rng = np.random.default_rng(seed)
    img = rng.random((height, width, 3), dtype=F32) * F32(4)
    flat = img.reshape(-1, 3)
    k = rng.permutation(flat.shape[0])[:3]
    flat[k[0], 1], flat[k[1]], flat[k[2]] = np.nan, -1.0, 0.0  # texels that may not be sampled
    return img


def env_of(img, rotation=0.0, scale=1.0, filter=E.NEAREST):
    return E.Environment(torch_device().tensor(img, device="cuda"), rotation, scale, filter)


def ids_of(n):
    return (np.arange(n, dtype=np.uint32) * np.uint32(2654435761)) ^ np.uint32(0x80000001)


class Batch:
    pass


@pytest.fixture(scope="module")
def ref():
    torch = torch_device()
    b = Batch()
    b.world = rt.reference_world()
    b.scene = rt.Scene(b.world)
    b.rays_t = rt.camera_rays(rt.reference_camera(), rt.Frame.full(WIDTH, HEIGHT, 0))
    hits = u32(rt.cast_rays(b.scene, b.rays_t)).copy()
    solid = np.flatnonzero(hits[MIDDLE:MIDDLE + 64, 0] <= 1)
    hits[MIDDLE + solid[1], 2] = 9999  # a hit whose object_index names no material: "no hit" to every call
    b.plain_t = dev(hits)  # ... and nothing else out of the ordinary
    hits[MIDDLE + solid[2], 6:9] = np.array([np.nan, 0, 1], dtype=F32).view(np.uint32)  # a NaN normal passes through the arithmetic
    b.broken, b.nan = MIDDLE + int(solid[1]), MIDDLE + int(solid[2])
    b.hits, b.hits_t, b.n = hits, dev(hits), hits.shape[0]
    b.surfaces_t = materials.material_hits(b.scene, b.hits_t)
    b.surfaces = host(b.surfaces_t).view(materials.SURFACE_DTYPE).reshape(-1)
    b.valid = b.surfaces["valid"] != 0
    b.geometric = np.ascontiguousarray(hits[:, 6:9]).view(F32)
    b.view_t = (-b.rays_t[:, 3:6].view(torch.float32)).contiguous()
    b.view = host(b.view_t)
    assert b.valid[MIDDLE] and not b.valid[b.broken] and not b.valid[MIDDLE:MIDDLE + 257].all() and b.valid.sum() > 600
    assert (b.surfaces["shiness"][b.valid] > 0).any()
    b.img = sky(16, 8, 5)
    b.env = env_of(b.img, 0.3, 1.5)
    return b


def run_rays(scene, hits_t, incoming_t, spp, pattern, seed, ids, kind):
    torch = torch_device()
    m = spp * hits_t.shape[0]
    rays = torch.full((m, 11), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    asks, lobe = torch.full((m,), 0x5A, dtype=torch.uint8, device="cuda"), torch.full((m,), 0x5A, dtype=torch.uint8, device="cuda")
    dirs, pdf = torch.full((m, 3), 99.0, dtype=torch.float32, device="cuda"), torch.full((m,), 99.0, dtype=torch.float32, device="cuda")
    ids_t = None if ids is None else torch.tensor(np.asarray(ids).astype(np.uint32).view(np.int32), device="cuda")
    L.rays(scene, hits_t, incoming_t, spp, pattern, seed, ids_t, kind, rays, asks, dirs, pdf, lobe)
    torch.cuda.synchronize()
    return rays, asks, dirs, pdf, lobe


def want_rays(hits, asks, dirs, spp):
    n = hits.shape[0]
    want = np.zeros((spp, n, 11), dtype=np.uint32)
    want[..., 0:3] = hits[None, :, 3:6]
    want[..., 3:6] = dirs.reshape(spp, n, 3).view(np.uint32)
    want[..., 6], want[..., 7], want[..., 8], want[..., 9], want[..., 10] = 1, 1, hits[None, :, 0], hits[None, :, 1], 1
    want[asks.reshape(spp, n) == 0] = 0
    return want.reshape(spp * n, 11)


# ---- bits ----

@pytest.mark.parametrize("n", BATCHES)
def test_rays_and_pdf_are_the_cpu_forms(ref, n):
    """dirs, pdf, lobe and asks against rays_numpy, the rays restated from them, and rt_lobe_pdf against pdf_numpy and against the
    sampler's own density: every sample count and pattern, both normals, with and without ids, NaN and "no hit" records among them"""
    rows = slice(MIDDLE, MIDDLE + n)
    hits_t, hits, valid = ref.hits_t[rows].contiguous(), ref.hits[rows], ref.valid[rows]
    incoming_t, view, view_t = ref.rays_t[rows].contiguous(), ref.view[rows], ref.view_t[rows].contiguous()
    surfaces, surfaces_t = ref.surfaces[rows], ref.surfaces_t[rows].contiguous()
    asked = speculars = 0
    for spp, pattern in SAMPLES:
        for kind in (L.SHADING, L.GEOMETRIC):
            ids = ids_of(n) if spp != 4 else None
            rays_t, asks_t, dirs_t, pdf_t, lobe_t = run_rays(ref.scene, hits_t, incoming_t, spp, pattern, 11 + spp, ids, kind)
            with np.errstate(all="ignore"):
                want = L.rays_numpy(surfaces, view, spp, pattern, 11 + spp, ids, ref.geometric[rows] if kind == L.GEOMETRIC else None)
            what = f"n {n}, spp {spp}, pattern {pattern}, kind {kind}"
            for got, w, name in zip((dirs_t, pdf_t, lobe_t, asks_t), want, ("dirs", "pdf", "lobe", "asks")):
                assert_same(host(got).reshape(w.shape), w, f"{name}: {what}", nan_ok=name in ("dirs", "pdf"))
            assert_same(u32(rays_t), want_rays(hits, host(asks_t), host(dirs_t), spp), "rays: " + what)  # the device's own dirs: bit for bit
            assert not host(dirs_t).reshape(spp, n, 3)[:, ~valid].any() and not host(pdf_t).reshape(spp, n)[:, ~valid].any()
            asked += int(host(asks_t).sum())
            speculars += int(host(lobe_t).sum())
            if kind == L.SHADING:  # the two pdf calls agree, and the device call is its CPU form
                again = L.pdf(surfaces_t, view_t, dirs_t.view(spp, n, 3))
                assert_same(host(again), host(pdf_t), "rt_lobe_pdf of the sampler's directions: " + what, nan_ok=True)
                with np.errstate(all="ignore"):
                    assert_same(host(again).reshape(spp, n), L.pdf_numpy(surfaces, view, host(dirs_t).reshape(spp, n, 3)), "pdf_numpy: " + what, nan_ok=True)
    assert asked > 0 and (n < 63 or speculars > 0)


@pytest.mark.parametrize("n", BATCHES)
@pytest.mark.parametrize("width,height", SKIES)
def test_the_environment_pdf_and_the_weights_are_the_cpu_forms(n, width, height):
    torch = torch_device()
    img = sky(width, height, n)
    rng = np.random.default_rng(n + width)
    k = 3 * n
    d = (rng.normal(size=(k, 3)) * 3).astype(F32)
    special = [(0, 0, 0), (np.nan, 1, 0), (np.inf, 0, 1), (0, 1, 0), (0, -1, 0), (1, 0, 0), (-1, 0, -0.0), (-1, 0, 0.0)]
    d[1:1 + min(len(special), k - 1)] = special[:k - 1]
    table = E.table_numpy(img)
    env = env_of(img, 0.3)
    pdf_t = torch.full((k,), 99.0, dtype=torch.float32, device="cuda")
    texel_t = torch.full((k,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    L.environment_pdf(env, torch.tensor(d, device="cuda"), None, pdf_t, texel_t)
    want, want_texel = L.environment_pdf_numpy(img, table, d, 0.3)
    assert_same(host(pdf_t), want, "environment pdf")
    assert_same(u32(texel_t), want_texel, "texel")
    alone = L.environment_pdf(env, torch.tensor(d, device="cuda"), want_texel=False)  # d_texel NULL
    assert alone[1] is None
    assert_same(host(alone[0]), want, "without a texel output")
    other = env.table().clone()
    other.view(torch.int32)[0] = width + 1  # the header names another size
    assert not host(L.environment_pdf(env, torch.tensor(d, device="cuda"), other)[0]).any()
    # the weights, with pdfs that are zero, negative, NaN and Inf among them
    own, theirs = want.copy(), (10.0 ** rng.uniform(-3, 3, k)).astype(F32)
    own[:min(4, k)] = np.array([0.0, -1.0, np.nan, np.inf], dtype=F32)[:k]
    rgb = rng.random((k, 3), dtype=F32)
    for heuristic in (L.BALANCE, L.POWER):
        for divide in (False, True):
            for other_pdf, n_other in ((theirs, 16), (theirs, 0), (None, 4)):
                w_t, rgb_t = torch.full((k,), 99.0, dtype=torch.float32, device="cuda"), torch.tensor(rgb, device="cuda")
                L.mis_weigh(torch.tensor(own, device="cuda"), 4, None if other_pdf is None else torch.tensor(other_pdf, device="cuda"), n_other, heuristic,
                            divide, w_t, rgb_t)
                with np.errstate(all="ignore"):
                    want_w, want_rgb = L.mis_weigh_numpy(own, 4, other_pdf, n_other, heuristic, divide, rgb)
                what = f"heuristic {heuristic}, divide {divide}, n_other {n_other}"
                assert_same(host(w_t), want_w, "w: " + what)
                assert G.same_or_both_nan(host(rgb_t), want_rgb), "rgb: " + what


# ---- anchors to existing calls ----

def test_without_shiness_the_rays_are_the_hemisphere_queries(ref):
    torch = torch_device()
    scene = rt.Scene(ref.world)
    desc = ref.world.desc()
    mats = (type(desc.materials[0]) * desc.n_materials)()
    for m in range(desc.n_materials):
        C.memmove(C.byref(mats[m]), C.byref(desc.materials[m]), C.sizeof(mats[m]))
        mats[m].shiness = 0.0
    scene.update_materials(0, mats)
    for spp, pattern in SAMPLES:
        for kind in (L.SHADING, L.GEOMETRIC):
            rays_t, asks_t, dirs_t, pdf_t, lobe_t = run_rays(scene, ref.plain_t, ref.rays_t, spp, pattern, 3, None, kind)
            want = hemisphere.rays(scene, ref.plain_t, spp, pattern, 3, None, kind)
            torch.cuda.synchronize()
            what = f"spp {spp}, pattern {pattern}, kind {kind}"
            assert_same(u32(rays_t), u32(want[0]), "rays: " + what)
            assert_same(host(asks_t), host(want[1]), "asks: " + what)
            assert_same(host(dirs_t), host(want[2]), "dirs: " + what)
            assert not host(lobe_t).any() and host(asks_t).any()


def test_without_lobe_samples_sky_hits_mis_is_sky_hits(ref):
    torch = torch_device()
    for spp, pattern in ((4, L.STRATIFIED), (5, L.UNIFORM)):
        want = E.sky_hits(ref.scene, ref.env, ref.hits_t, ref.view_t, spp, None, pattern, 7)
        got = L.sky_hits_mis(ref.scene, ref.env, ref.hits_t, ref.rays_t, spp, 0, L.BALANCE, None, pattern, 7)
        torch.cuda.synchronize()
        assert host(want).any()
        assert_same(host(got), host(want), f"spp_env {spp}, spp_lobe 0")
    # ... and both halves together light the hits, and not as the environment's half alone does (a lobe sample may look a NaN texel
    # up, which no table sample draws: those few hits are NaN)
    both = L.sky_hits_mis(ref.scene, ref.env, ref.hits_t, ref.rays_t, 4, 4, L.POWER, None, L.STRATIFIED, 7)
    torch.cuda.synchronize()
    lit = host(both)[ref.valid]
    assert np.isfinite(lit).mean() > 0.9 and (host(both)[~ref.valid] == 0).all()
    assert (lit != host(got)[ref.valid]).any()


def test_glossy_hits_is_its_sequence_and_the_environment_fold(ref):
    torch = torch_device()
    n, spp, depth = ref.n, 4, 2
    start = np.random.default_rng(2).random((n, 3), dtype=F32)
    got = L.glossy_hits(ref.scene, ref.hits_t, ref.rays_t, spp, depth, 1.0, torch.tensor(start, device="cuda"), L.STRATIFIED, 9)
    # call by call
    rays_t, asks_t, dirs_t, pdf_t, _ = L.rays(ref.scene, ref.hits_t, ref.rays_t, spp, L.STRATIFIED, 9)
    radiance_t = rt.trace_rays(ref.scene, rays_t, depth, 1.0)
    surfaces_t = materials.material_hits(ref.scene, ref.hits_t)
    diffuse_t, specular_t = materials.probe_surfaces(surfaces_t, ref.view_t, dirs_t.view(spp, n, 3))
    L.mis_weigh(pdf_t, 1, None, 0, L.BALANCE, True, None, radiance_t)
    out_t = torch.tensor(start, device="cuda")
    E.fold(ref.scene, ref.hits_t, asks_t, spp, radiance_t, diffuse_t, specular_t, out_t)
    torch.cuda.synchronize()
    assert_same(host(got), host(out_t), "call by call")
    with np.errstate(all="ignore"):
        _, want = E.fold_numpy(ref.valid, ref.surfaces["shiness"], host(asks_t), spp, host(radiance_t), host(diffuse_t), host(specular_t), start)
    assert G.same_or_both_nan(host(got), want)
    assert (host(got)[ref.valid] != start[ref.valid]).any() and (host(got)[~ref.valid] == start[~ref.valid]).all()


# ---- capture ----

def test_the_sequences_replay_from_a_graph(ref):
    """both sequences captured on a side stream with no call before the capture — glossy_hits' new calls around an uncaptured
    trace_rays, which has capture rules of its own.  Every call follows the one before it on one stream: the graphs are chains."""
    torch = torch_device()
    n, spp = ref.n, 4
    m = spp * n
    env = env_of(ref.img, 0.3, 1.5)
    table = env.table()  # the table is the caller's, built once per image
    want_sky = host(L.sky_hits_mis(ref.scene, env, ref.hits_t, ref.rays_t, spp, spp, L.BALANCE, None, L.STRATIFIED, 3))
    want_glossy = host(L.glossy_hits(ref.scene, ref.hits_t, ref.rays_t, spp, 1, 1.0, None, L.STRATIFIED, 3))
    torch.cuda.synchronize()
    assert table is env.table()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        w = L.workspace(n, "cuda", 2 * spp)
        out_sky, out_glossy = torch.zeros((n, 3), dtype=torch.float32, device="cuda"), torch.zeros((n, 3), dtype=torch.float32, device="cuda")
        stream.synchronize()
        head, tail, whole = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        with torch.cuda.graph(whole, stream=stream):
            out_sky.zero_()
            L.sky_hits_mis(ref.scene, env, ref.hits_t, ref.rays_t, spp, spp, L.BALANCE, out_sky, L.STRATIFIED, 3, view=ref.view_t, stream=stream, workspace=w)
        with torch.cuda.graph(head, stream=stream):
            L.rays(ref.scene, ref.hits_t, ref.rays_t, spp, L.STRATIFIED, 3, None, L.SHADING, w.rays[:m], w.asks[:m], w.dirs[:m], w.pdf[:m], w.lobe[:m], stream=stream)
        with torch.cuda.graph(tail, stream=stream):
            out_glossy.zero_()
            materials.material_hits(ref.scene, ref.hits_t, w.surfaces[:n], stream=stream)
            materials.probe_surfaces(w.surfaces[:n], ref.view_t, w.dirs[:m].view(spp, n, 3), w.diffuse[:m].view(spp, n, 3), w.specular[:m].view(spp, n, 3),
                                     stream=stream)
            L.mis_weigh(w.pdf[:m], 1, None, 0, L.BALANCE, True, None, w.radiance[:m], stream=stream)
            E.fold(ref.scene, ref.hits_t, w.asks[:m], spp, w.radiance[:m], w.diffuse[:m], w.specular[:m], out_glossy, None, stream=stream)
        out_sky.fill_(7.0)
        out_glossy.fill_(7.0)
        whole.replay()
        head.replay()
        rt.trace_rays(ref.scene, w.rays[:m], 1, 1.0, out=w.radiance[:m], stream=stream)
        tail.replay()
        stream.synchronize()
    assert want_sky.any() and want_glossy.any()
    assert G.same_or_both_nan(host(out_sky), want_sky), "sky_hits_mis replayed"
    assert G.same_or_both_nan(host(out_glossy), want_glossy), "glossy_hits replayed"


# ---- no call writes outside its operands ----

def test_every_operand_stays_between_its_guards(ref):
    torch = torch_device()
    n, spp, width, height = 65, 4, 37, 19
    img = sky(width, height, 9)
    env = env_of(img, 0.3, 1.5)
    held = []

    def operand(shape, dtype, fill=None):
        count = int(np.prod(shape))
        size = torch.empty((), dtype=dtype).element_size()
        payload = (count * size + 3) // 4
        whole, view = G.guarded(payload, G.SENTINEL, form="cuda")
        held.append((whole, G.guard_words(payload), payload))
        t = view.view(torch.uint8)[:count * size].view(dtype).view(*shape)
        if fill is not None:
            t.copy_(fill)
        return t

    rows = slice(MIDDLE, MIDDLE + n)
    m = spp * n
    hits_t, incoming_t = operand((n, 13), torch.int32, ref.hits_t[rows]), operand((n, 11), torch.int32, ref.rays_t[rows])
    rays, asks, dirs = operand((m, 11), torch.int32), operand((m,), torch.uint8), operand((m, 3), torch.float32)
    pdf, lobe = operand((m,), torch.float32), operand((m,), torch.uint8)
    L.rays(ref.scene, hits_t, incoming_t, spp, L.UNIFORM, 1, None, L.SHADING, rays, asks, dirs, pdf, lobe)
    surfaces, view = operand((n, 18), torch.int32, ref.surfaces_t[rows]), operand((n, 3), torch.float32, ref.view_t[rows])
    again = operand((m,), torch.float32)
    L.pdf(surfaces, view, dirs.view(spp, n, 3), L.SHADING, again)
    table = operand((E.table_bytes(width, height),), torch.uint8)  # at table_bytes exactly
    E.table(env, out=table)
    other, texel = operand((m,), torch.float32), operand((m,), torch.int32)
    L.environment_pdf(env, dirs, table, other, texel)
    weight, rgb = operand((m,), torch.float32), operand((m, 3), torch.float32, torch.ones((m, 3), device="cuda"))
    L.mis_weigh(pdf, spp, other, spp, L.BALANCE, True, weight, rgb)
    torch.cuda.synchronize()
    assert_same(host(again), host(pdf), "the guarded pdf")
    assert host(asks).any() and (host(other) > 0).any() and (host(weight) > 0).any()
    assert_same(host(table), E.table_numpy(img), "the guarded table")
    for whole, guard, payload in held:
        w = u32(whole)
        assert (w[:guard] == G.SENTINEL).all() and (w[guard + payload:] == G.SENTINEL).all(), "a store outside an operand"
