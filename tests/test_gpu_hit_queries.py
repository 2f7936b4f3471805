"""Hit queries on the device (include/rt_amd.h rt_shade_hits / rt_reflect_rays / rt_refract_rays): get_shade, get_reflect and
get_refract on hits that rt_cast_rays wrote, against the oracle's orc_get_shade / orc_reflect / orc_get_refract; against
rt_trace_rays at depth 0; ray_trace rebuilt from the queries one level deep against rt_trace_rays; records a caller got wrong;
both casts and a scene above the breadth-first switch; graph capture.  Every comparison is of f32 bit patterns: any NaN equals
any NaN, -0.0 differs from +0.0."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import homework_18_graphics_raytracer_amd as rt
from _hit_support import _pow_host, _some_hits, assert_parity, gpu_queries, oracle_queries
from _records import dev, ESCAPED, INFINITE, NONE, same_f32, same_rays, source_b, source_c, tessellated_scene, THRESHOLD, torch_device, TRAPPED

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


FRAME_A = (96, 72)


def test_oracle_parity():
    """1. hits from rt_cast_rays of (a) a small frame's camera rays, (b) random rays, (c) rays started inside the glass objects"""
    torch = torch_device()
    world = rt.reference_world()
    desc = world.desc()
    scene = rt.Scene(world)
    a = rt.camera_rays(rt.reference_camera(), rt.Frame.full(*FRAME_A, 5))
    torch.cuda.synchronize()
    rays = np.concatenate([a.cpu().numpy().view(np.uint32), source_b(desc, 2, 4000), source_c(desc, 3, 500)])
    rays_t = dev(rays)
    hits_t = rt.cast_rays(scene, rays_t)
    torch.cuda.synchronize()
    hits = hits_t.cpu().numpy().view(np.uint32)
    want = oracle_queries(desc, rays, hits)
    # the batch holds what it was chosen for: every kind of Refraction, and Escaped walks with at least one total reflection
    kinds = want.kind[want.rows]
    hist = {k: int((kinds == k).sum()) for k in (ESCAPED, INFINITE, TRAPPED)}
    assert all(v > 0 for v in hist.values()), hist
    esc = want.rows[kinds == ESCAPED]
    bounced = int((want.travel[esc] > want.first_inside[esc] * np.float32(1.001)).sum())
    assert bounced > 0, (hist, bounced)
    assert (hits[:, 0] == NONE).sum() > 100 and (hits[:, 0] == 0).sum() > 100 and (hits[:, 0] == 1).sum() > 100 and (hits[hits[:, 0] <= 1, 11] == 1).sum() > 100
    got = gpu_queries(scene, rays_t, hits_t)
    assert_parity(got, want, hits, "reference scene")
    assert got.refract_casts >= want.rows.size - hist[TRAPPED] and got.refract_casts <= 11 * want.rows.size
    # the host forms and the record-tensor / Hits forms agree with the device tensors
    sub = slice(FRAME_A[0] * FRAME_A[1], FRAME_A[0] * FRAME_A[1] + 1500)
    rgb, casts = rt.shade_hits_numpy(scene, hits[sub], rays[sub])
    assert same_f32(rgb, got.shade[sub]).all() and casts == int(want.shade_casts[sub].sum())
    kind, travel, escape, rcasts = rt.refract_rays_numpy(scene, hits[sub].view(rt.HIT_DTYPE).reshape(-1), rays[sub])
    assert np.array_equal(kind.view(np.uint32), got.kind[sub]) and same_f32(travel, got.travel[sub]).all()
    assert same_rays(escape.view(np.uint32).reshape(-1, 11), got.escape[sub]).all() and rcasts > 0
    # a max_distance that stops the bounces early, and one that stops nothing: still the reference's loop
    c_rows = np.arange(rays.shape[0] - 1000, rays.shape[0])
    for max_distance in (0.05, float("inf")):
        w2 = oracle_queries(desc, rays[c_rows], hits[c_rows], max_distance)
        g2 = rt.refract_rays(scene, dev(hits[c_rows]), dev(rays[c_rows]), max_distance)
        torch.cuda.synchronize()
        k2 = g2.kind.cpu().numpy().view(np.uint32)
        assert np.array_equal(k2[w2.rows], w2.kind[w2.rows]), max_distance
        e2 = w2.rows[w2.kind[w2.rows] == ESCAPED]
        assert same_f32(g2.travel.cpu().numpy()[e2], w2.travel[e2]).all() and same_rays(g2.rays.cpu().numpy()[e2], w2.escape[e2]).all()


def _contributions(desc, obj):
    """shade, reflection and refraction contribution of an object's material in f32, in the reference's order (main.rs:480, 493, 502):
    the two generative materials change only diffuse and normal, so these are constants per object"""
    m = desc.materials[int(obj)]
    sh, tr = np.float32(m.shiness), np.float32(m.transparency)
    one = np.float32(1.0)
    return (one - sh) * (one - tr), sh * (one - tr), tr


def test_depth_zero_identity():
    """2. where the hit object's shade contribution reaches THRESHOLD: rt_shade_hits(rt_cast_rays(r), r) == rt_trace_rays(r, 0)"""
    torch = torch_device()
    world = rt.reference_world()
    desc = world.desc()
    scene = rt.Scene(world)
    a = rt.camera_rays(rt.reference_camera(), rt.Frame.full(128, 96, 0))
    torch.cuda.synchronize()
    rays = np.concatenate([a.cpu().numpy().view(np.uint32), source_b(desc, 12, 3000)])
    hits = rt.cast_rays(scene, dev(rays)).cpu().numpy().view(np.uint32)
    hit = hits[:, 0] <= 1
    sc = np.array([_contributions(desc, o)[0] if h else np.float32(0.0) for o, h in zip(hits[:, 2], hit)], dtype=np.float32)
    shaded = hit & (sc >= THRESHOLD)
    glass = hit & ~shaded
    assert shaded.sum() > 3000 and glass.sum() > 100  # glass hits, where rt_trace_rays is black, are test 1's
    r_t, h_t = dev(rays[shaded]), dev(hits[shaded])
    c_shade, c_trace = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
    shade = rt.shade_hits(scene, h_t, r_t, ray_count=c_shade)
    trace = rt.trace_rays(scene, r_t, 0, ray_count=c_trace)
    torch.cuda.synchronize()
    assert same_f32(shade.cpu().numpy(), trace.cpu().numpy()).all()
    assert int(c_shade.item()) + int(shaded.sum()) == int(c_trace.item())
    black = rt.trace_rays(scene, dev(rays[glass]), 0)
    torch.cuda.synchronize()
    assert (black.cpu().numpy().view(np.uint32) == 0).all()


@pytest.mark.parametrize("depth", [5, 1])
def test_one_level_peeled(depth):
    """3. ray_trace (main.rs:466-519) rebuilt from the queries, one level: cast; per hit object shade_hits where sc >= T, reflect_rays ->
    rt_trace_rays(depth - 1, rc) where rc >= T, refract_rays -> rt_trace_rays(escape, depth - 1, fc) * pow(opaque_decay, travel) where
    fc > T; (shade * sc + reflection * rc) + refraction * fc.  Equal to rt_trace_rays(rays, depth) bit for bit, and the cast counts add
    up: primary + shade + refract + children — the only check of rt_refract_rays' count."""
    torch = torch_device()
    world = rt.reference_world()
    desc = world.desc()
    scene = rt.Scene(world)
    rays_t = rt.camera_rays(rt.reference_camera(), rt.Frame.full(160, 90, depth))
    n = rays_t.shape[0]
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    want = rt.trace_rays(scene, rays_t, depth, ray_count=cnt)
    hits_t = rt.cast_rays(scene, rays_t)
    torch.cuda.synchronize()
    want, want_casts = want.cpu().numpy(), int(cnt.item())
    hits = hits_t.cpu().numpy().view(np.uint32)
    hit = hits[:, 0] <= 1
    result = np.zeros((n, 3), dtype=np.float32)
    casts = n  # every root passes ray_trace's entry check (contribution 1.0) and casts once
    parts = {"shade": 0, "reflect": 0, "refract": 0, "escaped": 0}

    def count_of(fn):
        cnt.zero_()
        out = fn(cnt)
        torch.cuda.synchronize()
        return out, int(cnt.item())

    with np.errstate(all="ignore"):
        for obj in np.unique(hits[hit, 2]):
            rows = np.flatnonzero(hit & (hits[:, 2] == obj))
            idx = torch.tensor(rows, device="cuda")
            r_t, h_t = rays_t[idx].contiguous(), hits_t[idx].contiguous()
            sc, rc, fc = _contributions(desc, obj)
            shade = np.zeros((rows.size, 3), dtype=np.float32)
            reflection = np.zeros((rows.size, 3), dtype=np.float32)
            refraction = np.zeros((rows.size, 3), dtype=np.float32)
            if sc >= THRESHOLD:
                out, c = count_of(lambda k: rt.shade_hits(scene, h_t, r_t, ray_count=k))
                shade, casts = out.cpu().numpy(), casts + c
                parts["shade"] += rows.size
            if rc >= THRESHOLD:
                out, c = count_of(lambda k: rt.trace_rays(scene, rt.reflect_rays(h_t, r_t), depth - 1, float(rc), ray_count=k))
                reflection, casts = out.cpu().numpy(), casts + c
                parts["reflect"] += rows.size
            if fc > THRESHOLD:  # strict, main.rs:504
                refr, c = count_of(lambda k: rt.refract_rays(scene, h_t, r_t, 100.0, ray_count=k))
                casts += c
                parts["refract"] += rows.size
                esc = refr.escaped.nonzero().flatten()
                if esc.numel():
                    out, c = count_of(lambda k: rt.trace_rays(scene, refr.rays[esc].contiguous(), depth - 1, float(fc), ray_count=k))
                    casts += c
                    travel = refr.travel[esc].cpu().numpy()
                    decay = _pow_host(np.full(travel.shape, desc.materials[int(obj)].opaque_decay, dtype=np.float32), travel)
                    refraction[esc.cpu().numpy()] = out.cpu().numpy() * decay[:, None]
                    parts["escaped"] += int(esc.numel())
            result[rows] = (shade * sc + reflection * rc) + refraction * fc
    assert all(v > 0 for v in parts.values()), parts
    bad = np.flatnonzero(~same_f32(result, want).all(axis=1))
    assert bad.size == 0, f"depth {depth}: {bad.size} of {n} differ, first {bad[:5]}: {result[bad[:2]]} want {want[bad[:2]]} objects {hits[bad[:5], 2]}"
    assert casts == want_casts, (depth, casts, want_casts, parts)


def test_foreign_records():
    """4. records a caller got wrong: RT_OK, "no hit" records give black / zero / RT_HIT_NONE and add nothing to the counts, records used
    as given (an index far outside its array, NaN position and normal, a zero direction) compute what the reference computes, and the
    neighbours of a bad record are what they are in the same batch without it.  Validation, not an attempt at a fault: nothing in the
    kernels is indexed with an unchecked field."""
    torch = torch_device()
    world = rt.reference_world()
    desc = world.desc()
    scene = rt.Scene(world)
    rays, hits = _some_hits(scene, desc, 41, 65)  # one full wave plus one lane
    base = gpu_queries(scene, dev(rays), dev(hits))
    want = oracle_queries(desc, rays, hits)
    assert_parity(base, want, hits, "base batch")
    nan = np.array([np.nan], dtype=np.float32).view(np.uint32)[0]
    no_hit = {"kind 7": (0, 7), "RT_HIT_NONE": (0, NONE), "object_index = n_materials": (2, desc.n_materials), "object_index 0xffffffff": (2, NONE)}
    as_given = {"index far outside": ("hit", [1], [0x7FFFFFF0]), "index 0xffffffff": ("hit", [1], [NONE]),
                "NaN position": ("hit", [3, 4, 5], [nan] * 3), "NaN normal": ("hit", [6, 7, 8], [nan] * 3),
                "zero direction": ("ray", [3, 4, 5], [0] * 3), "face_direction 5": ("hit", [11], [5])}
    for j in (0, 17, 63, 64):
        others = np.arange(65) != j
        # what record j alone contributes to the counts
        alone = gpu_queries(scene, dev(rays[j:j + 1]), dev(hits[j:j + 1]))  # a batch of 1
        assert same_f32(alone.shade, base.shade[j:j + 1]).all() and alone.kind[0] == base.kind[j] and same_rays(alone.escape, base.escape[j:j + 1]).all()
        for what, (word, value) in no_hit.items():
            h = hits.copy()
            h[j, word] = value
            got = gpu_queries(scene, dev(rays), dev(h))
            assert (got.shade[j].view(np.uint32) == 0).all() and got.kind[j] == NONE and got.travel[j].view(np.uint32) == 0 and (got.escape[j] == 0).all(), (what, j)
            if word == 0:  # rt_reflect_rays has no scene: it tests the kind only
                assert (got.reflect[j] == 0).all(), (what, j)
            else:
                assert same_rays(got.reflect[j:j + 1], base.reflect[j:j + 1]).all(), (what, j)
            for name in ("shade", "reflect", "kind", "travel", "escape"):
                a, b = getattr(got, name)[others], getattr(base, name)[others]
                assert (same_f32(a, b) if a.dtype == np.float32 else a == b).all(), (what, j, name)
            assert got.shade_casts == base.shade_casts - alone.shade_casts and got.refract_casts == base.refract_casts - alone.refract_casts, (what, j)
        for what, (which, words, values) in as_given.items():
            h, r = hits.copy(), rays.copy()
            (h if which == "hit" else r)[j, words] = values
            got = gpu_queries(scene, dev(r), dev(h))
            for name in ("shade", "reflect", "kind", "travel", "escape"):
                a, b = getattr(got, name)[others], getattr(base, name)[others]
                assert (same_f32(a, b) if a.dtype == np.float32 else a == b).all(), (what, j, name)
            if what != "face_direction 5":  # the oracle's Face enum has no value 5; the header reads it as Back
                assert_parity(got, oracle_queries(desc, r, h), h, what)
            else:
                h[j, 11] = 1
                back = gpu_queries(scene, dev(r), dev(h))
                assert same_f32(got.shade, back.shade).all() and same_rays(got.reflect, back.reflect).all() and np.array_equal(got.kind, back.kind)
    # a whole batch of records that are no hits: nothing is cast
    h = hits.copy()
    h[:, 0] = NONE
    got = gpu_queries(scene, dev(rays), dev(h))
    assert got.shade_casts == 0 and got.refract_casts == 0 and (got.kind == NONE).all() and (got.shade.view(np.uint32) == 0).all()
    # an empty batch: RT_OK, nothing launched, outputs untouched
    lib = rt._capi.amd_lib()
    sentinel = torch.full((4, 3), 99.0, dtype=torch.float32, device="cuda")
    t = dev(hits[:4]), dev(rays[:4])
    assert lib.rt_shade_hits(scene._h, C.c_void_p(t[0].data_ptr()), C.c_void_p(t[1].data_ptr()), 0, C.c_void_p(sentinel.data_ptr()), None, None) == 0
    torch.cuda.synchronize()
    assert (sentinel.cpu().numpy() == 99.0).all()


def test_both_casts_and_a_large_scene(tmp_path):
    """5. the wave-uniform cast gives the bits of the pair-wise one, and a scene above the breadth-first switch the oracle's"""
    torch = torch_device()
    world = rt.reference_world()
    desc = world.desc()
    scene = rt.Scene(world)
    rays = source_b(desc, 2, 4000)
    rays_t = dev(rays)
    hits_t = rt.cast_rays(scene, rays_t)
    a = gpu_queries(scene, rays_t, hits_t)
    with rt.options(RT_AMD_QUERY_WAVE_UNIFORM=1):
        b = gpu_queries(scene, rays_t, hits_t)
    for name in ("shade", "reflect", "kind", "travel", "escape"):
        x, y = getattr(a, name), getattr(b, name)
        assert (same_f32(x, y) if x.dtype == np.float32 else x == y).all(), name
    assert a.shade_casts == b.shade_casts and a.refract_casts == b.refract_casts and a.shade_casts > 0 and a.refract_casts > 0
    big, cam = tessellated_scene(tmp_path, 4)
    big_desc = big.desc()
    assert big_desc.n_triangles == 36 * 4 ** 4 + 28  # above rt_scene_create's default switch (8 192 triangles)
    with rt.options(RT_AMD_BFS_WALK_TRIANGLES=8192):  # the library's default switch, set here so that no environment moves it
        big_scene = rt.Scene(big)  # the switch is read when the scene is created: this scene is walked breadth-first
    r = np.concatenate([rt.camera_rays(cam, rt.Frame.full(24, 18, 5)).cpu().numpy().view(np.uint32), source_b(big_desc, 51, 300)])
    h_t = rt.cast_rays(big_scene, dev(r))
    torch.cuda.synchronize()
    h = h_t.cpu().numpy().view(np.uint32)
    want = oracle_queries(big_desc, r, h)
    assert 300 <= want.rows.size
    for uniform in (None, 1):
        with rt.options(RT_AMD_QUERY_WAVE_UNIFORM=uniform):
            assert_parity(gpu_queries(big_scene, dev(r), h_t), want, h, f"9 244 triangles, wave-uniform {uniform}")


@pytest.mark.parametrize("band", [64, 400, 1 << 20])
def test_bands_give_the_bits_of_one_launch(band):
    """a batch beyond 2^26 records runs in bands of whole 64-record chunks; RT_AMD_DIAG_HIT_BAND_RECORDS shortens the bands (64; 400,
    rounded up to 448; one larger than the batch) so that a batch a test can hold runs in many launches: the same bits and counts,
    a tail band of fewer than 64 records included"""
    world = rt.reference_world()
    desc = world.desc()
    scene = rt.Scene(world)
    rays = np.concatenate([source_b(desc, 71, 3000), source_c(desc, 72, 337)])  # 4011 records: not a multiple of 64
    rays_t = dev(rays)
    hits_t = rt.cast_rays(scene, rays_t)
    for uniform in (None, 1):
        with rt.options(RT_AMD_QUERY_WAVE_UNIFORM=uniform):
            one = gpu_queries(scene, rays_t, hits_t)
            with rt.options(RT_AMD_DIAG_HIT_BAND_RECORDS=band):
                many = gpu_queries(scene, rays_t, hits_t)
        for name in ("shade", "reflect", "kind", "travel", "escape"):
            x, y = getattr(one, name), getattr(many, name)
            assert (same_f32(x, y) if x.dtype == np.float32 else x == y).all(), (band, uniform, name)
        assert one.shade_casts == many.shade_casts > 0 and one.refract_casts == many.refract_casts > 0, (band, uniform)
    hits = hits_t.cpu().numpy().view(np.uint32)
    assert_parity(many, oracle_queries(desc, rays, hits), hits, f"bands of {band}")


def test_graph_capture_without_a_prior_call():
    """6. rt_shade_hits uses no workspace: captured on a fresh scene with no call before it, replayed twice"""
    torch = torch_device()
    world = rt.reference_world()
    desc = world.desc()
    scene = rt.Scene(world)  # nothing has run on this scene but the cast that made the hits
    rays, hits = _some_hits(scene, desc, 61, 1000)
    rays2, hits2 = _some_hits(scene, desc, 62, 1000)
    r_t, h_t = dev(rays), dev(hits)
    out = torch.empty((1000, 3), dtype=torch.float32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rt.shade_hits(scene, h_t, r_t, out=out, ray_count=cnt)
    want1, want2 = oracle_queries(desc, rays, hits), oracle_queries(desc, rays2, hits2)
    out.fill_(7.0)
    graph.replay()
    torch.cuda.synchronize()
    first = out.cpu().numpy().copy()
    assert same_f32(first, want1.shade).all() and int(cnt.item()) == int(want1.shade_casts.sum())
    r_t.copy_(dev(rays2))
    h_t.copy_(dev(hits2))
    out.fill_(7.0)
    graph.replay()
    torch.cuda.synchronize()
    assert same_f32(out.cpu().numpy(), want2.shade).all()
    assert int(cnt.item()) == int(want1.shade_casts.sum()) + int(want2.shade_casts.sum())
    graph.replay()  # the same inputs again: identical bits
    torch.cuda.synchronize()
    assert same_f32(out.cpu().numpy(), want2.shade).all()
