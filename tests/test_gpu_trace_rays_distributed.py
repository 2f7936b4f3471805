"""Stochastic radiance queries on the device (include/rt_amd.h rt_trace_rays_distributed, rt_focus_rays, rt_rng_create_seeded,
rt_rng_upload): distributed_ray_trace (src/main.rs:521-614) on caller-supplied rays, on generators that belong to no frame.

The oracle has orc_render_distributed (the camera only), orc_cast, orc_get_shade and the generator (orc_rng_init / orc_rng_draw_*),
and no distributed_ray_trace on a given ray, so the new paths are tied to it like this — every comparison bit for bit, NaN equal to
NaN, -0.0 not equal to +0.0:
  * seeding / upload / download against orc_rng_init and orc_rng_draw_u32;
  * rt_focus_rays + rt_trace_rays_distributed(n_epochs = 1), repeated, against orc_render_distributed epoch by epoch;
  * arbitrary rays at depth <= 0 against orc_get_shade(orc_cast(ray));
  * batches concatenated from several cameras and permuted, against the per-camera oracle results;
  * many epochs on fixed rays: against single-epoch calls, and (blur 0: the lens ray is the same every epoch) against the oracle with
    its two lens draws per epoch put into the streams on the host.
Coverage conditions are asserted on the ORACLE's outputs, so that no comparison can pass on emptiness.  Every test runs under both
organisations of the pass (rt_set_distributed_split 1 / 0)."""
import ctypes as C

import numpy as np
import pytest

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import _capi
import _oracle
import _scenes
from _records import bounds, oracle_hits, random_rays, same_bits, tessellated_world, torch_device
from _reference_support import RAND_05_NEW_FROM_U64_0

pytestmark = pytest.mark.gpu
L = _oracle._dist_lib()
WORDS = 516


@pytest.fixture(autouse=True, params=[1, 0], ids=["split", "fused"])
def organisation(request):
    lib = _capi.amd_lib()
    lib.rt_set_distributed_split(request.param)
    yield request.param
    lib.rt_set_distributed_split(-1)


@pytest.fixture(scope="module")
def ref():
    world = rt.reference_world()
    return world, world.desc(), rt.Scene(world), rt.reference_camera()


def seeds_of(frame):
    """main.rs:1119: y * 2^33 + x in the tile's row order"""
    ys = frame.y0 + np.arange(frame.rows, dtype=np.uint64) * np.uint64(frame.y_step)
    xs = frame.x0 + np.arange(frame.cols, dtype=np.uint64)
    return (ys[:, None] * np.uint64(1 << 33) + xs[None, :]).reshape(-1)


def assert_same(got, want, what=""):
    g, w = np.asarray(got, dtype=np.float32).reshape(-1, 3), np.asarray(want, dtype=np.float32).reshape(-1, 3)
    same = same_bits(g, w)
    bad = np.argwhere(~same)
    assert same.all(), f"{what}: {len(bad)} channels differ, first {bad[:3].tolist()}: got {g[bad[0][0]]} want {w[bad[0][0]]}"


def is_normal(v):
    return np.isfinite(v) & (np.abs(v) >= np.finfo(np.float32).tiny)


def trace(scene, rays, depth, rng, n_epochs=1, accum=None, want_samples=True, **kw):
    """-> samples (n_epochs, N, 3), valid (n_epochs, N), casts"""
    torch = torch_device()
    n = rays.shape[0]
    samples = torch.full((n_epochs, n, 3), 7.0, dtype=torch.float32, device="cuda") if want_samples else None
    valid = torch.full((n_epochs, n), 9, dtype=torch.uint8, device="cuda") if want_samples else None
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    rt.trace_rays_distributed(scene, rays, depth, rng, n_epochs, accum=accum, samples=samples, valid=valid, ray_count=cnt, **kw)
    torch.cuda.synchronize()
    return (samples.cpu().numpy() if want_samples else None), (valid.cpu().numpy() if want_samples else None), int(cnt.item())


def oracle_epochs(desc, cam, frame, n_epochs, focus, blur):
    """orc_render_distributed one epoch at a time: samples (E, N, 3), valid (E, N), casts per epoch, the records after every epoch"""
    st = _oracle.rng_init(frame)
    s, v, c, after = [], [], [], []
    for _ in range(n_epochs):
        es, ev, ec = _oracle.render_distributed(desc, cam, frame, st, 1, focus=focus, blur=blur)
        s.append(es.reshape(-1, 3))
        v.append(ev.reshape(-1))
        c.append(ec)
        after.append(st.copy())
    return np.stack(s), np.stack(v), c, after


def lens_draws(states, blur):
    """the two Normal(0, blur) draws of shoot_focus (main.rs:112-114) on every record, in place"""
    out = np.empty(2, dtype=np.float64)
    for rec in states:
        L.orc_rng_draw_normal(rec.ctypes.data, 0.0, float(blur), out.ctypes.data, 2)
    return states


def first_level_kinds(desc, hits, states_after_lens):
    """weighted_select (main.rs:652-666) of the first level of every ray that hit, from the oracle's cast and the oracle's generator:
    0 Diffuse, 1 Reflection, 2 Refraction"""
    kinds = set()
    draw = np.empty(1, dtype=np.float32)
    f = np.float32
    for i in np.flatnonzero(hits[:, 0] != 0xFFFFFFFF):
        m = desc.materials[int(hits[i, 2])]
        w0 = (f(1.0) - f(m.shiness)) * (f(1.0) - f(m.transparency))
        w1 = f(m.shiness) * (f(1.0) - f(m.transparency))
        w2 = f(m.transparency)
        total = f(f(f(0.0) + w0) + w1) + w2
        rec = states_after_lens[i].copy()
        L.orc_rng_draw_range_f32(rec.ctypes.data, f(0.0), f(total), draw.ctypes.data, 1)
        kinds.add(0 if draw[0] < w0 else 1 if draw[0] < f(w0 + w1) else 2)
    return kinds


def assert_coverage(desc, rays_t, valid=None, depth=0, kinds_from=None, what=""):
    """at least half of the rays hit something; at depth >= 5 at least a quarter of the samples pass the filter; with `kinds_from`
    (the records at the first level's draws) every ray type of weighted_select occurs — all on the oracle's outputs"""
    hits = oracle_hits(desc, rays_t.cpu().numpy())
    share = float((hits[:, 0] != 0xFFFFFFFF).mean())
    assert share >= 0.5, f"{what}: only {share:.2f} of the rays hit"
    if valid is not None and depth >= 5:
        assert float(np.mean(valid != 0)) >= 0.25, f"{what}: only {np.mean(valid != 0):.2f} of the samples pass the filter"
    if kinds_from is not None:
        assert first_level_kinds(desc, hits, kinds_from) == {0, 1, 2}, f"{what}: not every ray type occurs"
    return hits


# ---- 1. seeding, download, upload ----

@pytest.mark.parametrize("frame", [rt.Frame.full(40, 30, 5), rt.Frame(64, 48, 5, 3, 5, 40, 41, 2)], ids=["full", "interleaved_tile"])
def test_seeded_generators_equal_the_frames(frame):
    want = _oracle.rng_init(frame)
    seeded = rt.Rng.seeded(seeds_of(frame))
    assert np.array_equal(seeded.download(), want)
    assert np.array_equal(rt.Rng(frame).download(), want)


def test_seed_zero_and_all_ones():
    rng = rt.Rng.seeded([0, (1 << 64) - 1, 1 << 33])
    st = rng.download()
    out = np.empty(16, dtype=np.uint32)
    rec = st[0].copy()
    L.orc_rng_draw_u32(rec.ctypes.data, out.ctypes.data, 16)
    assert [int(v) for v in out] == RAND_05_NEW_FROM_U64_0  # rand's published vector for new_from_u64(0)
    assert np.array_equal(st[0], _oracle.rng_init(rt.Frame(8, 8, 5, 0, 0, 1, 1, 1))[0])
    assert np.array_equal(st[2], _oracle.rng_init(rt.Frame(8, 8, 5, 0, 1, 1, 2, 1))[0])  # the pixel (0, 1)
    # 2^64 - 1: key words 0 and 1 are both 0xffffffff — x = 2^32 - 1 of row y gives words (0xffffffff, 2y), so no frame has it;
    # pin what can be pinned: a fresh generator (index 256, a = b = c = 0), different from its neighbours, and stable under upload
    assert st[1, 515] == 256 and (st[1, 256:259] == 0).all() and not np.array_equal(st[1, :256], st[0, :256])
    rng.upload(st)
    assert np.array_equal(rng.download(), st)


def test_upload_is_the_inverse_of_download_and_the_device_continues_as_the_oracle(ref):
    world, desc, scene, cam = ref
    frame = rt.Frame.full(32, 24, 5)
    n = frame.rows * frame.cols
    rng = rt.Rng(frame)
    st = rng.download()
    rng.upload(st)
    assert np.array_equal(rng.download(), st)
    # advance the oracle's streams by counts that cross a 256-word block boundary (and by none, and by exactly one block)
    adv = st.copy()
    counts = np.random.default_rng(5).integers(200, 700, n)
    counts[:4] = (0, 256, 255, 257)
    for rec, k in zip(adv, counts):
        out = np.empty(int(k), dtype=np.uint32)
        L.orc_rng_draw_u32(rec.ctypes.data, out.ctypes.data, int(k))
    rng.upload(adv)
    assert np.array_equal(rng.download(), adv)
    # ... and the device continues from there as the oracle does: two epochs of the camera's pass on these records
    torch = torch_device()
    samples = torch.empty((2, frame.rows, frame.cols, 3), dtype=torch.float32, device="cuda")
    valid = torch.empty((2, frame.rows, frame.cols), dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    rt.render_distributed(scene, cam, frame, rng, 2, samples=samples, valid=valid, ray_count=cnt)
    torch.cuda.synchronize()
    ws, wv, wc = _oracle.render_distributed(desc, cam, frame, adv, 2)
    assert_same(samples.cpu().numpy(), ws, "after upload")
    assert np.array_equal(valid.cpu().numpy(), wv) and int(cnt.item()) == wc
    assert np.array_equal(rng.download(), adv)


def test_render_distributed_refuses_a_seeded_rng_and_other_counts(ref):
    world, desc, scene, cam = ref
    torch = torch_device()
    frame = rt.Frame.full(16, 8, 5)
    seeded = rt.Rng.seeded(seeds_of(frame))
    acc = torch.zeros((frame.rows, frame.cols, 3), dtype=torch.float32, device="cuda")
    with pytest.raises(rt.RtError) as e:
        rt.render_distributed(scene, cam, frame, seeded, 1, accum=acc)
    assert e.value.code == -1 and "different tile" in str(e.value)
    rays = rt.camera_rays(cam, rt.Frame.full(16, 7, 5))
    with pytest.raises(rt.RtError) as e:
        rt.trace_rays_distributed(scene, rays, 5, seeded, accum=torch.zeros((16 * 7, 3), dtype=torch.float32, device="cuda"))
    assert e.value.code == -1 and "different number of generators" in str(e.value)
    with pytest.raises(rt.RtError):
        rt.focus_rays(cam, rt.Frame.full(16, 7, 5), seeded)
    with pytest.raises(rt.RtError):
        rt.focus_rays(cam, rt.Frame(32, 8, 5, 16, 0, 32, 8, 1), rt.Rng(frame))  # a frame's generators, another tile of as many pixels
    assert np.array_equal(seeded.download(), _oracle.rng_init(frame))  # nothing ran


def test_argument_order_with_a_live_rng(ref):
    """the checks that follow the count (tests/test_trace_rays_distributed_abi.py pins the order up to it)"""
    world, desc, scene, cam = ref
    torch = torch_device()
    lib = _capi.amd_lib()
    rng = rt.Rng.seeded([1, 2])
    rays = rt.camera_rays(cam, rt.Frame.full(2, 1, 5))
    acc = torch.zeros((2, 3), dtype=torch.float32, device="cuda")
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())

    def dev(r=rays, epochs=1, a=acc, s=None, depth=5):
        return lib.rt_trace_rays_distributed(scene._h, p(r), 2, depth, rng._h, epochs, p(a), p(s), None, None, None)

    assert dev(r=None, a=None, depth=33, epochs=0) == 0  # nothing to do comes before all of them
    assert dev(r=None, a=None, depth=33) == -1 and b"null ray pointer" in lib.rt_last_error()
    assert dev(a=None, depth=33) == -1 and b"need d_accum or d_samples" in lib.rt_last_error()
    assert dev(depth=33) == -5 and b"RT_MAX_DEPTH" in lib.rt_last_error()
    h_rays = np.zeros(2, dtype=rt.RAY_DTYPE)
    h_acc = np.full((2, 3), 7.0, dtype=np.float32)
    host = lambda r, a, depth: lib.rt_trace_rays_distributed_host(scene._h, r, 2, depth, rng._h, 1, a, None)
    assert host(None, None, 33) == -1 and b"null ray pointer" in lib.rt_last_error()
    assert host(h_rays.ctypes.data_as(C.c_void_p), None, 33) == -1 and b"null accum pointer" in lib.rt_last_error()
    assert host(h_rays.ctypes.data_as(C.c_void_p), h_acc.ctypes.data_as(C.c_void_p), 33) == -5
    torch.cuda.synchronize()
    assert (h_acc == 7.0).all() and (acc == 0).all()
    assert np.array_equal(rng.download(), rt.Rng.seeded([1, 2]).download())  # no draw was made


# ---- 2. focus_rays + one epoch, repeated, is the oracle's pass ----

def composition(scene, desc, cam, frame, epochs, focus, blur, what, kinds=False, seeded=False):
    """E times rt_focus_rays + rt_trace_rays_distributed(n_epochs = 1) against orc_render_distributed, epoch by epoch"""
    torch = torch_device()
    ws, wv, wc, wafter = oracle_epochs(desc, cam, frame, epochs, focus, blur)
    rng = rt.Rng.seeded(seeds_of(frame)) if seeded else rt.Rng(frame)
    before = _oracle.rng_init(frame)
    casts = 0
    for e in range(epochs):
        rays = rt.focus_rays(cam, frame, rng, focus, blur)
        torch.cuda.synchronize()
        at_level = lens_draws(before.copy(), blur)
        assert np.array_equal(rng.download(), at_level), f"{what} epoch {e}: records after rt_focus_rays"
        assert_coverage(desc, rays, wv[e], frame.max_depth, at_level if kinds and e == 0 else None, f"{what} epoch {e}")
        s, v, c = trace(scene, rays, frame.max_depth, rng)
        assert_same(s[0], ws[e], f"{what} epoch {e}")
        assert np.array_equal(v[0], wv[e]), f"{what} epoch {e}: flags"
        assert np.array_equal(rng.download(), wafter[e]), f"{what} epoch {e}: records"
        casts += c
        before = wafter[e]
    assert casts == sum(wc), f"{what}: {casts} casts, oracle {sum(wc)}"


@pytest.mark.parametrize("name,frame,blur,seeded", [
    ("d5", rt.Frame.full(64, 48, 5), 0.04, False),
    ("d8_blur0", rt.Frame.full(48, 36, 8), 0.0, True),
    ("tile_step3", rt.Frame(96, 72, 5, 7, 5, 71, 70, 3), 0.04, True),
])
def test_composition_equals_the_oracle_on_the_reference_scene(ref, name, frame, blur, seeded):
    world, desc, scene, cam = ref
    composition(scene, desc, cam, frame, 3, 3.0, blur, name, kinds=True, seeded=seeded)


@pytest.mark.parametrize("sq_seed,eye,seed", [(4, (0.5, 0.5, 3.0), 1), (6, (0.5, 0.5, 1.0), 3)])
def test_composition_on_random_and_degenerate_scenes(sq_seed, eye, seed):
    """scenes of tests/_scenes.py, with the seeds and eyes under which the oracle's outputs meet the coverage conditions (of the
    squares worlds 1 .. 8 seen from z = 3 only 4 has half of its rays hit; clustered / random worlds 2 have too few samples that pass
    the filter)"""
    for name, world, cam, blur in (("squares_axis", _scenes.squares_world(sq_seed), _scenes.axis_camera(eye), 0.0),
                                   ("clustered", _scenes.clustered_world(seed, n_boxes=3), _scenes.camera(seed), 0.02),
                                   ("random", _scenes.random_world(seed, 40, 3), _scenes.camera(seed), 0.04)):
        composition(rt.Scene(world), world.desc(), cam, rt.Frame.full(48, 36, 5), 2, 3.0, blur, f"{name}{seed}")


def test_composition_on_a_scene_walked_breadth_first(tmp_path):
    """forced by RT_AMD_BFS_WALK_TRIANGLES, as tests/test_gpu_scene_sizes.py does: distributed_kernel<.., BFS, RAYS>"""
    world = tessellated_world(tmp_path, 2, True)
    with rt.options(RT_AMD_BFS_WALK_TRIANGLES=1):
        scene = rt.Scene(world)
        composition(scene, world.desc(), rt.reference_camera(), rt.Frame.full(64, 48, 5), 2, 3.0, 0.04, "bfs")
    with rt.options(RT_AMD_BFS_WALK_TRIANGLES=1, RT_AMD_DIAG_BFS_CAP=96):
        composition(rt.Scene(world), world.desc(), rt.reference_camera(), rt.Frame.full(40, 30, 5), 1, 3.0, 0.04, "bfs, short lists")


# ---- 3. arbitrary rays at depth 0 and below: get_shade(cast(ray)) ----

def oracle_shade(desc, rays_words):
    """orc_get_shade(orc_cast(ray)) or black: (N, 3) float32, casts (the primary one and get_shade's), hit mask"""
    rays = np.ascontiguousarray(rays_words).view(np.uint32).reshape(-1, 11).copy()
    n = rays.shape[0]
    orays = (_oracle.OrcRay * n).from_buffer(rays)
    lib = _oracle.lib()
    out = np.zeros((n, 3), dtype=np.float32)
    hit_mask = np.zeros(n, dtype=bool)
    h = _oracle.OrcHit()
    buf = (C.c_float * 3)()
    casts = C.c_uint64(0)
    total = 0
    for i in range(n):
        total += 1
        if lib.orc_cast(C.byref(desc), C.byref(orays[i]), C.byref(h)):
            lib.orc_get_shade(C.byref(desc), C.byref(h), C.byref(orays[i]), buf, C.byref(casts))
            out[i] = np.frombuffer(buf, dtype=np.float32)
            total += casts.value
            hit_mask[i] = True
    return out, total, hit_mask


@pytest.mark.parametrize("depth", [0, -3])
def test_arbitrary_rays_at_depth_zero_and_below(ref, depth):
    world, desc, scene, cam = ref
    centre, radius = bounds(desc)
    rays = random_rays(43, 5003, desc, centre, radius)  # not a multiple of 64; Front, Back and Both; exclusions, some out of range
    words = rays.cpu().numpy().view(np.uint32)
    assert set(np.unique(words[:, 6])) == {0, 1, 2} and (words[:, 7] == 0).any() and (words[:, 7] != 0).any()
    want, wcasts, hit_mask = oracle_shade(desc, words)
    assert hit_mask.mean() >= 0.5
    seeds = np.arange(5003, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    rng = rt.Rng.seeded(seeds)
    before = rng.download()
    s, v, casts = trace(scene, rays, depth, rng, 2)
    for e in range(2):  # no draws at depth <= 0: both epochs are the same sample
        assert_same(s[e], want, f"depth {depth} epoch {e}")
        assert np.array_equal(v[e] != 0, is_normal(want).all(axis=1))
    assert casts == 2 * wcasts
    assert np.array_equal(rng.download(), before)  # the generators are untouched


# ---- 4. the rays of a batch are independent ----

CAMERAS = [("ref", None, rt.Frame.full(40, 30, 5), 0.04), ("moved", (0.3, 0.1, 0.2), rt.Frame(64, 48, 5, 9, 2, 50, 40, 2), 0.02),
           ("near", (-0.2, 0.2, -0.4), rt.Frame.full(33, 21, 5), 0.0)]


def _per_camera(ref):
    """per camera: rays of rt_focus_rays, the seeds, the oracle's records at the first level's draws and after the epoch, and its
    samples / flags / casts of that epoch"""
    world, desc, scene, cam0 = ref
    torch = torch_device()
    parts = []
    for name, shift, frame, blur in CAMERAS:
        cam = rt.reference_camera()
        if shift is not None:
            cam.center = tuple(float(np.float32(c + d)) for c, d in zip(cam.center, shift))
        ws, wv, wc, wafter = oracle_epochs(desc, cam, frame, 1, 3.0, blur)
        rng = rt.Rng(frame)
        rays = rt.focus_rays(cam, frame, rng, 3.0, blur)
        torch.cuda.synchronize()
        at_level = lens_draws(_oracle.rng_init(frame), blur)
        assert np.array_equal(rng.download(), at_level)
        assert_coverage(desc, rays, wv[0], 5, at_level, name)
        parts.append((rays, seeds_of(frame), at_level, wafter[0], ws[0], wv[0], wc[0]))
    return parts


@pytest.mark.parametrize("take", [None, 1000, 1], ids=["all", "not_a_multiple_of_64", "single_ray"])
def test_a_permuted_batch_of_three_cameras_equals_the_per_camera_oracle(ref, take):
    world, desc, scene, cam0 = ref
    torch = torch_device()
    parts = _per_camera(ref)
    rays = torch.cat([p[0] for p in parts])
    seeds, at_level, after = (np.concatenate([p[k] for p in parts]) for k in (1, 2, 3))
    ws, wv = np.concatenate([p[4] for p in parts]), np.concatenate([p[5] for p in parts])
    n = rays.shape[0]
    assert n % 64 != 0
    perm = np.random.default_rng(77).permutation(n)
    if take is not None:
        perm = perm[:take] if take > 1 else np.array([int(np.flatnonzero(wv != 0)[5])])
    rays_p = rays[torch.tensor(perm, device="cuda")].contiguous()
    rng = rt.Rng.seeded(seeds[perm])
    assert np.array_equal(rng.download()[:, 515], np.full(len(perm), 256, dtype=np.uint32))
    rng.upload(at_level[perm])  # the streams at the point shoot_focus leaves them
    s, v, casts = trace(scene, rays_p, 5, rng)
    assert_same(s[0], ws[perm], f"permuted batch of {len(perm)}")
    assert np.array_equal(v[0], wv[perm])
    assert np.array_equal(rng.download(), after[perm])
    if take is None:
        assert casts == sum(p[6] for p in parts)
    elif take == 1:
        assert wv[perm][0] != 0 and casts >= 2


# ---- 5. epochs continue on fixed rays ----

@pytest.mark.parametrize("k", [3, 17])
def test_k_epochs_in_one_call_equal_k_calls_of_one(ref, k):
    world, desc, scene, cam = ref
    torch = torch_device()
    frame = rt.Frame.full(48, 36, 8)
    n = frame.rows * frame.cols
    rng = rt.Rng(frame)
    rays = rt.focus_rays(cam, frame, rng)
    torch.cuda.synchronize()
    start = rng.download()
    acc = torch.full((n, 3), 0.25, dtype=torch.float32, device="cuda")
    s, v, casts = trace(scene, rays, 8, rng, k, accum=acc)
    end = rng.download()
    assert_coverage(desc, rays)
    assert float(np.mean(v != 0)) >= 0.25
    assert not np.array_equal(s[0].view(np.uint32), s[1].view(np.uint32))  # the streams do move on between epochs
    rng2 = rt.Rng.seeded(np.zeros(n, dtype=np.uint64))
    rng2.upload(start)
    acc2 = torch.full((n, 3), 0.25, dtype=torch.float32, device="cuda")
    total = 0
    for e in range(k):
        s1, v1, c1 = trace(scene, rays, 8, rng2, 1, accum=acc2)
        assert_same(s1[0], s[e], f"epoch {e} of {k}")
        assert np.array_equal(v1[0], v[e])
        total += c1
    assert total == casts
    assert np.array_equal(rng2.download(), end)
    assert_same(acc2.cpu().numpy(), acc.cpu().numpy(), "accumulator")
    want = np.full((n, 3), 0.25, dtype=np.float32)
    for e in range(k):  # in epoch order
        want = np.where((v[e] != 0)[:, None], want + s[e], want)
    assert_same(acc.cpu().numpy(), want, "accumulator against the samples")


def test_epochs_beyond_the_first_against_the_oracle(ref):
    """blur 0: the lens offsets are exactly +0.0, so the oracle's ray is the same in every epoch; its two lens draws per epoch are put
    into the streams on the host (download, orc_rng_draw_normal x 2, upload)"""
    world, desc, scene, cam = ref
    torch = torch_device()
    k = 4
    frame = rt.Frame.full(48, 36, 5)
    ws, wv, wc, wafter = oracle_epochs(desc, cam, frame, k, 1.0, 0.0)
    rng = rt.Rng(frame)
    rays = rt.focus_rays(cam, frame, rng, 1.0, 0.0)  # the first epoch's draws
    torch.cuda.synchronize()
    assert_coverage(desc, rays, wv, 5, rng.download(), "blur 0")
    casts = 0
    for e in range(k):
        if e > 0:
            rng.upload(lens_draws(rng.download(), 0.0))
        s, v, c = trace(scene, rays, 5, rng)
        assert_same(s[0], ws[e], f"epoch {e}")
        assert np.array_equal(v[0], wv[e])
        assert np.array_equal(rng.download(), wafter[e])
        casts += c
    assert casts == sum(wc)


# ---- 6. switches and paths ----

def test_switches_outputs_and_the_host_entry_point(ref):
    world, desc, scene, cam = ref
    torch = torch_device()
    frame = rt.Frame.full(40, 30, 5)
    n = frame.rows * frame.cols
    k = 17  # more than one batch of 16
    rng = rt.Rng(frame)
    rays = rt.focus_rays(cam, frame, rng)
    torch.cuda.synchronize()
    start = rng.download()
    assert_coverage(desc, rays)
    acc0 = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
    s0, v0, c0 = trace(scene, rays, 5, rng, k, accum=acc0)
    end = rng.download()
    assert float(np.mean(v0 != 0)) >= 0.25
    acc0 = acc0.cpu().numpy()

    def again(what, want_samples=True, want_accum=True, **opts):
        with rt.options(**opts):
            rng.upload(start)
            acc = torch.zeros((n, 3), dtype=torch.float32, device="cuda") if want_accum else None
            s, v, c = trace(scene, rays, 5, rng, k, accum=acc, want_samples=want_samples)
        if want_samples:
            assert_same(s, s0, what)
            assert np.array_equal(v, v0), what
        if want_accum:
            assert_same(acc.cpu().numpy(), acc0, what + ": accumulator")
        assert c == c0 and np.array_equal(rng.download(), end), what

    again("again")
    again("in line", RT_AMD_DIST_PIPELINE=0)
    again("by cost", RT_AMD_DIST_BY_COST=1)
    again("never by cost", RT_AMD_DIST_BY_COST=0)
    again("no look-ahead", RT_AMD_RNG_LOOKAHEAD=0)
    again("small workspace", RT_AMD_DIST_WS_MB=1)
    again("no workspace: the one-kernel organisation", RT_AMD_DIAG_WS_REFUSE=64)
    again("bands of 64 rays", RT_AMD_DIAG_DIST_BAND_RAYS=64)
    again("bands of 448 rays", RT_AMD_DIAG_DIST_BAND_RAYS=400)
    again("accum only", want_samples=False)
    again("samples only", want_accum=False)
    # the host entry point
    rng.upload(start)
    img = np.zeros((n, 3), dtype=np.float32)
    casts = rt.trace_rays_distributed_numpy(scene, rays.cpu().numpy(), 5, rng, k, img)
    assert_same(img, acc0, "host entry point")
    assert casts == c0 and np.array_equal(rng.download(), end)
    # a frame's generators serve a batch of as many rays, and its next frame call continues from where the batch left them
    samples = torch.empty((1, frame.rows, frame.cols, 3), dtype=torch.float32, device="cuda")
    rt.render_distributed(scene, cam, frame, rng, 1, samples=samples)
    torch.cuda.synchronize()
    st = end.copy()
    ws, _, _ = _oracle.render_distributed(desc, cam, frame, st, 1)
    assert_same(samples.cpu().numpy(), ws, "the frame's pass after the batch")
    assert np.array_equal(rng.download(), st)


def test_profiling_covers_the_ray_entry_point(ref, organisation):
    world, desc, scene, cam = ref
    torch = torch_device()
    lib = _capi.amd_lib()
    frame = rt.Frame.full(40, 30, 5)
    rng = rt.Rng(frame)
    rays = rt.focus_rays(cam, frame, rng)
    ms = (C.c_double * 4)()
    launches = (C.c_uint * 4)()
    lib.rt_profile_enable(1)
    try:
        lib.rt_profile_read_distributed(ms, launches)
        trace(scene, rays, 5, rng, 2)
        assert lib.rt_profile_read_distributed(ms, launches) == 0
    finally:
        lib.rt_profile_enable(0)
    if organisation == 1:
        assert launches[1] == 1 and launches[2] == 1 and launches[3] == 1 and ms[1] > 0.0
