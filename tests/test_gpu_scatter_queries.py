"""Scatter queries on the device (include/rt_amd.h rt_scatter_hits / rt_scatter_factors): the three draws of a level of
distributed_ray_trace on hits that rt_cast_rays wrote.  Draw accounting and the scattered direction against the oracle's generator
and helpers; distributed_ray_trace rebuilt level by level from the queries (the loop of INTEGRATION.md, the fold in numpy f32)
against rt_trace_rays_distributed — samples, flags, generator records and cast counts; index arrays; interleaving with the other
entry points that move the generators; records a caller got wrong; bands and graph capture.  Every comparison is of f32 bit
patterns: any NaN equals any NaN, -0.0 differs from +0.0.

On the cast counts.  The reference evaluates get_shade at every level's entry (main.rs:524) and uses that value only where
depth <= 0; the library and the oracle evaluate — and count — a get_shade where its value is used: at an entry with depth <= 0, as
the mix or sum operand of main.rs:571 / 590 / 605 and for a scattered hit whose next cast misses (main.rs:573, 592).  The level loop
here counts its rt_shade_hits calls the same way, which is what makes the sum of the queries' counters equal the call's."""
import ctypes as C

import numpy as np
import pytest

import homework_18_graphics_raytracer_amd as rt
import _oracle
import _scenes
import _hit_support as hq
from _records import dev, INFINITE, NONE, oracle_hits, same_f32, same_rays, source_b, torch_device, TRAPPED
from _scatter_support import chosen_rays, DIFFUSE, F32, is_normal, REFLECTION, REFRACTION, restate_level, seeded

pytestmark = pytest.mark.gpu
WORDS = 516


BRANCHES = ("diffuse", "reflection", "refraction", "black_cosine", "dr_miss", "escaped_hit", "escaped_miss", "escaped_bounced", "infinite",
            "trapped")


def run_levels(scene, rays_t, rng, depth, rng_index=None):
    """One epoch of distributed_ray_trace on every ray, level by level from the queries — the loop of INTEGRATION.md.  Records that have
    finished stay in place as "no hit" records (kind RT_HIT_NONE), which draw nothing.  -> sample (N, 3) f32, casts, branch counts"""
    torch = torch_device()
    n = rays_t.shape[0]
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")

    def counted(fn):
        cnt.zero_()
        out = fn(cnt)
        torch.cuda.synchronize()
        return out, int(cnt.item())

    def masked(hits_t, mask):
        h = hits_t.clone()
        h[~mask, 0] = rt.HIT_NONE
        return h

    casts = n
    cur_rays = rays_t
    cur_hits = rt.cast_rays(scene, cur_rays)
    live = cur_hits[:, 0] >= 0
    cur_hits = masked(cur_hits, live)
    levels = []
    seen = {k: 0 for k in ("diffuse", "reflection", "refraction", "black_cosine", "dr_miss", "escaped_hit", "escaped_miss", "escaped_bounced",
                           "infinite", "trapped")}
    for _ in range(max(depth, 0)):
        sc = rt.scatter_hits(scene, cur_hits, cur_rays, rng, rng_index=rng_index)
        alive = sc.alive
        assert bool(((sc.type != rt.HIT_NONE) == live).all())
        dr = alive & (sc.type != REFRACTION)
        fr = alive & (sc.type == REFRACTION)
        reflected = rt.reflect_rays(masked(cur_hits, dr), sc.rays)
        refr, c = counted(lambda k: rt.refract_rays(scene, masked(cur_hits, fr), sc.rays, 100.0, ray_count=k))
        casts += c
        escaped = fr & refr.escaped
        next_rays = torch.where(dr[:, None], reflected, refr.rays)
        to_cast = dr | escaped
        rows = to_cast.nonzero().flatten()
        next_hits = torch.full((n, 13), 0, dtype=torch.int32, device="cuda")
        next_hits[:, 0] = rt.HIT_NONE
        if rows.numel():
            next_hits[rows] = rt.cast_rays(scene, next_rays[rows].contiguous())
            casts += int(rows.numel())
        found = to_cast & (next_hits[:, 0] >= 0)
        next_hits = masked(next_hits, found)
        factor = rt.scatter_factors(scene, cur_hits, cur_rays, sc.type, next_rays, refr.travel)
        shade_next, c = counted(lambda k: rt.shade_hits(scene, next_hits, next_rays, ray_count=k))  # the mix / sum operand
        casts += c
        missed = dr & ~found
        shade_missed, c = counted(lambda k: rt.shade_hits(scene, masked(cur_hits, missed), sc.rays, ray_count=k))  # get_shade(&scattered_hit)
        casts += c
        torch.cuda.synchronize()
        t = sc.type.cpu().numpy()
        levels.append((t, found.cpu().numpy(), missed.cpu().numpy(), factor.cpu().numpy(), shade_next.cpu().numpy(), shade_missed.cpu().numpy()))
        lv = live.cpu().numpy()
        for name, k in (("diffuse", DIFFUSE), ("reflection", REFLECTION), ("refraction", REFRACTION)):
            seen[name] += int((lv & (t == k)).sum())
        seen["black_cosine"] += int((live & ~alive).sum())
        seen["dr_miss"] += int(missed.sum())
        seen["escaped_hit"] += int((escaped & found).sum())
        seen["escaped_miss"] += int((escaped & ~found).sum())
        seen["infinite"] += int((fr & (refr.kind == INFINITE)).sum())
        seen["trapped"] += int((fr & (refr.kind == TRAPPED)).sum())
        seen["escaped_bounced"] += c_bounced(scene, cur_hits, sc.rays, escaped, refr)
        cur_rays, cur_hits, live = next_rays, next_hits, found
    # depth <= 0: the value is get_shade(&hit) (main.rs:524-527) — evaluated, and counted, once more
    terminal, c = counted(lambda k: rt.shade_hits(scene, cur_hits, cur_rays, ray_count=k))
    casts += c
    value = terminal.cpu().numpy()
    half = F32(0.5)
    with np.errstate(all="ignore"):
        for t, found, missed, factor, shade_next, shade_missed in reversed(levels):
            new = np.zeros((n, 3), dtype=np.float32)
            mix = found & (t != REFRACTION)
            s = value[mix] * factor[mix]
            new[mix] = shade_next[mix] + (s - shade_next[mix]) * half  # palette's Mix::mix(&s, 0.5) as dist_unwind_kernel writes it
            add = found & (t == REFRACTION)
            new[add] = (value[add] + shade_next[add]) * factor[add, 0:1]
            new[missed] = shade_missed[missed]
            value = new
    return value, casts, seen


def c_bounced(scene, hits_t, scattered_t, escaped, refr):
    """Escaped walks that bounced inside: a travel distance beyond the first chord, which a max_distance of 0 measures (no bounce is
    allowed then: main.rs:378) — such a walk is Trapped under it"""
    rows = escaped.nonzero().flatten()
    if rows.numel() == 0:
        return 0
    short = rt.refract_rays(scene, hits_t[rows].contiguous(), scattered_t[rows].contiguous(), 0.0)
    return int((short.kind == TRAPPED).sum())


def compose(scene, rays, depth, epochs, what, want_branches=None):
    """`epochs` epochs of the level loop on one rt_rng against one rt_trace_rays_distributed call on an identically seeded one"""
    torch = torch_device()
    n = rays.shape[0]
    rays_t = dev(rays)
    rng_a, _ = seeded(n)
    rng_b, _ = seeded(n)
    samples = torch.full((epochs, n, 3), 7.0, dtype=torch.float32, device="cuda")
    valid = torch.full((epochs, n), 9, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    rt.trace_rays_distributed(scene, rays_t, depth, rng_b, epochs, samples=samples, valid=valid, ray_count=cnt)
    torch.cuda.synchronize()
    want, want_valid, want_casts = samples.cpu().numpy(), valid.cpu().numpy(), int(cnt.item())
    total, seen = 0, None
    for e in range(epochs):
        got, casts, s = run_levels(scene, rays_t, rng_a, depth)
        seen = s if seen is None else {k: seen[k] + s[k] for k in s}
        total += casts
        bad = np.flatnonzero(~same_f32(got, want[e]).all(axis=1))
        assert bad.size == 0, f"{what}, depth {depth}, epoch {e}: {bad.size} of {n} samples differ, first {bad[:5]}: {got[bad[:2]]} want {want[e][bad[:2]]}"
        assert np.array_equal(is_normal(got).all(axis=1), want_valid[e] != 0), (what, depth, e)
    print(f"{what} depth {depth}: casts {total} (call {want_casts}), branches {seen}")
    assert total == want_casts, (what, depth, total, want_casts)
    assert np.array_equal(rng_a.download(), rng_b.download()), (what, depth)
    if want_branches:
        missing = [k for k in want_branches if seen[k] == 0]
        assert not missing, (what, depth, missing, seen)
    rng_a.close()
    rng_b.close()


@pytest.fixture(scope="module")
def ref():
    world = rt.reference_world()
    desc = world.desc()
    rays, hits, classes = chosen_rays(desc)
    return world, desc, rt.Scene(world), rays, hits, classes


def test_the_chosen_batch_holds_every_branch_by_the_oracle(ref):
    """the reference alone (no device result) says the batch takes every branch of main.rs:556-613 at its first level"""
    _, _, _, _, _, classes = ref
    sizes = {k: int(classes[k].size) for k in BRANCHES}
    print("first level of the chosen batch, by the oracle:", sizes)
    assert all(v > 0 for v in sizes.values()), sizes


@pytest.mark.parametrize("which", ["reference", "random 3", "random 8"])
def test_draw_accounting_against_the_oracle(ref, which):
    """1. after one rt_scatter_hits every valid record's generator is the oracle's advanced by exactly three words, every other one
    is untouched; the type, the direction and the cosine are the restated ones"""
    torch = torch_device()
    if which == "reference":
        _, desc, scene, rays, _, _ = ref
    else:
        world = _scenes.random_world(int(which.split()[1]), 40, 4)
        desc, scene = world.desc(), rt.Scene(world)
        rays = source_b(desc, 21, 3000)
    n = rays.shape[0]
    rays_t = dev(rays)
    hits_t = rt.cast_rays(scene, rays_t)
    torch.cuda.synchronize()
    hits = hits_t.cpu().numpy().view(np.uint32)
    rng, states = seeded(n)
    before = states.copy()
    assert np.array_equal(rng.download(), states)
    sc = rt.scatter_hits(scene, hits_t, rays_t, rng)
    torch.cuda.synchronize()
    kind, new_dir, cosine = restate_level(desc, rays, hits, states)
    hit = hits[:, 0] <= 1
    assert hit.sum() > 500 and (~hit).sum() > 100
    assert np.array_equal(states[~hit], before[~hit]) and (states[hit, 515] != before[hit, 515]).all()
    after = rng.download()
    bad = np.flatnonzero((after != states).any(axis=1))
    assert bad.size == 0, f"{which}: {bad.size} generator records differ, first {bad[:5]} (hit: {hit[bad[:5]]})"
    got_type = sc.type.cpu().numpy().view(np.uint32)
    assert np.array_equal(got_type, kind), (which, np.flatnonzero(got_type != kind)[:5])
    assert all((kind == k).sum() > 0 for k in (DIFFUSE, REFLECTION, REFRACTION)), which
    out = sc.rays.cpu().numpy().view(np.uint32)
    want = rays.copy()
    want[:, 3:6] = new_dir.view(np.uint32)
    want[~hit] = 0
    bad = np.flatnonzero(~same_rays(out, want))
    assert bad.size == 0, f"{which}: {bad.size} scattered rays differ, first {bad[:3]}: {out[bad[:1]]} want {want[bad[:1]]}"
    assert same_f32(sc.cosine.cpu().numpy(), cosine).all(), which
    assert np.array_equal(sc.alive.cpu().numpy(), hit & ~(cosine <= 0))
    # the host form on a second, identically seeded rt_rng
    rng2, _ = seeded(n)
    t2, r2, c2 = rt.scatter_hits_numpy(scene, hits, rays, rng2)
    assert np.array_equal(t2.view(np.uint32), kind) and same_rays(r2.view(np.uint32).reshape(-1, 11), want).all() and same_f32(c2, cosine).all()
    assert np.array_equal(rng2.download(), states)
    rng.close()
    rng2.close()


@pytest.mark.parametrize("depth", [0, 1, 5, 8])
def test_composition_on_the_reference_scene(ref, depth):
    """2. the acceptance test: the level loop over three epochs equals rt_trace_rays_distributed — samples, flags, generator records and
    the cast count — on a batch that takes every branch"""
    _, _, scene, rays, _, _ = ref
    compose(scene, rays, depth, 3, "reference scene", BRANCHES if depth > 0 else None)


@pytest.mark.parametrize("depth", [0, 1, 5, 8])
def test_composition_on_a_scene_walked_breadth_first(ref, depth):
    """... and on a scene above RT_AMD_BFS_WALK_TRIANGLES, the switch lowered so that the scene stays small"""
    world, _, _, rays, _, _ = ref
    with rt.options(RT_AMD_BFS_WALK_TRIANGLES=1):  # read when the scene is created: the reference scene, walked breadth-first
        scene = rt.Scene(world)
    assert world.desc().n_triangles >= 1
    compose(scene, rays, depth, 3, "breadth-first scene", BRANCHES if depth > 0 else None)


def test_index_array_permuted_and_compacted(ref):
    """3. the same level with the records permuted and the dead ones dropped, each on its own generator through d_rng_index: per
    generator the same outputs and the same generator records as the identity run"""
    torch = torch_device()
    _, _, scene, rays, _, _ = ref
    n = rays.shape[0]
    rays_t = dev(rays)
    hits_t = rt.cast_rays(scene, rays_t)
    rng_a, _ = seeded(n)
    rng_b, _ = seeded(n)
    one = rt.scatter_hits(scene, hits_t, rays_t, rng_a)
    torch.cuda.synchronize()
    hit = (hits_t[:, 0] >= 0).cpu().numpy()
    g = np.random.default_rng(9)
    rows = g.permutation(np.flatnonzero(hit))  # compacted: hits only, in a random order
    assert 64 < rows.size < n
    idx = torch.tensor(rows.astype(np.int32), device="cuda")
    sel = torch.tensor(rows, device="cuda")
    two = rt.scatter_hits(scene, hits_t[sel].contiguous(), rays_t[sel].contiguous(), rng_b, rng_index=idx)
    torch.cuda.synchronize()
    assert np.array_equal(two.type.cpu().numpy(), one.type.cpu().numpy()[rows])
    assert same_rays(two.rays.cpu().numpy(), one.rays.cpu().numpy()[rows]).all()
    assert same_f32(two.cosine.cpu().numpy(), one.cosine.cpu().numpy()[rows]).all()
    assert np.array_equal(rng_a.download(), rng_b.download())
    # a second level on the same streams, the records in yet another order and every second one masked by an index out of range
    rows2 = g.permutation(rows)
    keep = g.random(rows2.size) < 0.5
    idx2 = torch.tensor(np.where(keep, rows2, -1).astype(np.int32), device="cuda")
    sel2 = torch.tensor(rows2, device="cuda")
    before = rng_b.download()
    three = rt.scatter_hits(scene, hits_t[sel2].contiguous(), rays_t[sel2].contiguous(), rng_b, rng_index=idx2)
    h_a = hits_t.clone()
    dead = np.ones(n, dtype=bool)
    dead[rows2[keep]] = False
    h_a[torch.tensor(dead, device="cuda"), 0] = rt.HIT_NONE
    four = rt.scatter_hits(scene, h_a, rays_t, rng_a)
    torch.cuda.synchronize()
    t3 = three.type.cpu().numpy()
    assert (t3[~keep] == rt.HIT_NONE).all() and (three.rays.cpu().numpy()[~keep] == 0).all() and (three.cosine.cpu().numpy()[~keep].view(np.uint32) == 0).all()
    assert np.array_equal(t3[keep], four.type.cpu().numpy()[rows2[keep]])
    assert same_rays(three.rays.cpu().numpy()[keep], four.rays.cpu().numpy()[rows2[keep]]).all()
    after = rng_b.download()
    assert np.array_equal(after, rng_a.download())
    assert np.array_equal(after[dead], before[dead]) and (after[~dead, 515] != before[~dead, 515]).all()
    rng_a.close()
    rng_b.close()


def test_continuation_between_entry_points_and_across_blocks(ref):
    """4. rt_scatter_hits, two epochs of rt_focus_rays + rt_trace_rays_distributed (which IS rt_render_distributed's epoch, so the oracle
    has it: orc_render_distributed), rt_scatter_hits again: the records are the oracle's stream positions after every step; and 90
    calls on one small batch, so that every generator crosses a block boundary — under both forms of the refill"""
    torch = torch_device()
    _, desc, scene, rays, _, _ = ref
    cam = rt.reference_camera()
    frame = rt.Frame.full(48, 36, 5)
    n = frame.rows * frame.cols
    f_rays_t = rt.camera_rays(cam, frame)
    f_hits_t = rt.cast_rays(scene, f_rays_t)
    torch.cuda.synchronize()
    f_rays, f_hits = f_rays_t.cpu().numpy().view(np.uint32), f_hits_t.cpu().numpy().view(np.uint32)
    hits_all = oracle_hits(desc, rays[:200])
    for prepare in (None, 1, 0):
        with rt.options(RT_AMD_SCATTER_PREPARE=prepare):
            rng, states = rt.Rng(frame), _oracle.rng_init(frame)
            rt.scatter_hits(scene, f_hits_t, f_rays_t, rng)
            restate_level(desc, f_rays, f_hits, states)
            assert np.array_equal(rng.download(), states), prepare
            samples = torch.zeros((2, n, 3), dtype=torch.float32, device="cuda")
            for e in range(2):
                lens = rt.focus_rays(cam, frame, rng)
                rt.trace_rays_distributed(scene, lens, frame.max_depth, rng, 1, samples=samples[e:e + 1])
            want, _, _ = _oracle.render_distributed(desc, cam, frame, states, 2)
            torch.cuda.synchronize()
            assert same_f32(samples.cpu().numpy().reshape(2, n, 3), want.reshape(2, n, 3)).all(), prepare
            assert np.array_equal(rng.download(), states), prepare
            sc = rt.scatter_hits(scene, f_hits_t, f_rays_t, rng)
            kind, new_dir, _ = restate_level(desc, f_rays, f_hits, states)
            torch.cuda.synchronize()
            assert np.array_equal(sc.type.cpu().numpy().view(np.uint32), kind), prepare
            assert same_f32(sc.rays[:, 3:6].cpu().numpy().view(np.float32), new_dir).all(), prepare
            assert np.array_equal(rng.download(), states), prepare
            rng.close()
            hits = hits_all
            # 90 calls on 200 records: 270 words each, more than a block of 256
            m = 200
            small_r, small_h = rays[:m], hits[:m]
            r_t, h_t = dev(small_r), dev(small_h)
            rng, states = seeded(m)
            start = states[:, 515].copy()
            for k in range(90):
                sc = rt.scatter_hits(scene, h_t, r_t, rng)
                kind, new_dir, cosine = restate_level(desc, small_r, small_h, states)
                if k % 10 == 9 or k >= 80:
                    torch.cuda.synchronize()
                    assert np.array_equal(sc.type.cpu().numpy().view(np.uint32), kind), (prepare, k)
                    assert same_f32(sc.rays[:, 3:6].cpu().numpy().view(np.float32), new_dir).all(), (prepare, k)
                    assert same_f32(sc.cosine.cpu().numpy(), cosine).all(), (prepare, k)
                    assert np.array_equal(rng.download(), states), (prepare, k)
            hit = small_h[:, 0] <= 1
            assert hit.sum() > 50
            # a fresh generator's position is 256 (nothing generated yet): 270 words later every one is in its second block
            assert (start == 256).all() and (states[hit, 515] == 270 - 256).all()
            # and the render entry points go on from there
            rt.trace_rays_distributed(scene, r_t, 3, rng, 1, accum=torch.zeros((m, 3), dtype=torch.float32, device="cuda"))
            twin = rt.Rng.seeded(np.arange(m, dtype=np.uint64))
            twin.upload(states)
            rt.trace_rays_distributed(scene, r_t, 3, twin, 1, accum=torch.zeros((m, 3), dtype=torch.float32, device="cuda"))
            torch.cuda.synchronize()
            assert np.array_equal(rng.download(), twin.download()), prepare
            rng.close()
            twin.close()


def test_records_a_caller_got_wrong(ref):
    """5. a bad kind, a bad object index and a generator index out of range are "no hit": RT_HIT_NONE, an all-zero ray, cosine 0, a black
    factor and no draw; a face value above its range, an index far outside and NaN normals or directions are used as given: the three
    draws are made and NaN passes through the arithmetic as it does through the oracle's (the code is rt_trace_rays_distributed's); the
    neighbours of a bad record are what they are without it"""
    torch = torch_device()
    _, desc, scene, _, _, _ = ref
    rays, hits = hq._some_hits(scene, desc, 41, 65)  # one full wave plus one lane
    n = 65
    nan = np.array([np.nan], dtype=np.float32).view(np.uint32)[0]

    def run(h, r, index=None):
        rng, states = seeded(n)
        idx = None if index is None else torch.tensor(np.asarray(index, dtype=np.int64).astype(np.int32), device="cuda")
        h_t, r_t = dev(h), dev(r)
        sc = rt.scatter_hits(scene, h_t, r_t, rng, rng_index=idx)
        nxt = rt.reflect_rays(h_t, sc.rays)
        fac = rt.scatter_factors(scene, h_t, r_t, sc.type, nxt, torch.full((n,), 0.5, dtype=torch.float32, device="cuda"))
        torch.cuda.synchronize()
        out = (sc.type.cpu().numpy().view(np.uint32), sc.rays.cpu().numpy().view(np.uint32), sc.cosine.cpu().numpy(), fac.cpu().numpy(), rng.download())
        rng.close()
        return out, states

    base, states0 = run(hits, rays)
    kind, new_dir, cosine = restate_level(desc, rays, hits, states0.copy())
    assert np.array_equal(base[0], kind) and same_f32(base[1][:, 3:6].view(np.float32), new_dir).all() and same_f32(base[2], cosine).all()
    no_hit = {"kind 7": (0, 7), "RT_HIT_NONE": (0, NONE), "object_index = n_materials": (2, desc.n_materials), "object_index 0xffffffff": (2, NONE)}
    for j in (0, 17, 63, 64):
        others = np.arange(n) != j
        cases = [(what, word, value, None) for what, (word, value) in no_hit.items()]
        cases += [("generator index = count", None, None, n), ("generator index 0xffffffff", None, None, -1)]
        for what, word, value, g in cases:
            h = hits.copy()
            index = None
            if word is not None:
                h[j, word] = value
            else:
                index = np.arange(n)
                index[j] = g
            got, _ = run(h, rays, index)
            assert got[0][j] == NONE and (got[1][j] == 0).all() and got[2][j].view(np.uint32) == 0 and (got[3][j].view(np.uint32) == 0).all(), (what, j)
            assert np.array_equal(got[4][j], states0[j]), (what, j)  # no draw: the generator has not moved
            for a, b in zip(got, base):
                assert (same_f32(a[others], b[others]) if a.dtype == np.float32 else a[others] == b[others]).all(), (what, j)
        # used as given: the draws are made, and what comes out is what the restated level says
        as_given = {"index far outside": ("hit", [1], [0x7FFFFFF0]), "NaN normal": ("hit", [6, 7, 8], [nan] * 3), "NaN direction": ("ray", [3, 4, 5], [nan] * 3),
                    "hit face_direction 5": ("hit", [11], [5]), "ray face_direction 9": ("ray", [6], [9])}
        for what, (which, words, values) in as_given.items():
            h, r = hits.copy(), rays.copy()
            (h if which == "hit" else r)[j, words] = values
            got, st = run(h, r)
            k2, d2, c2 = restate_level(desc, r, h, st)
            assert got[0][j] == k2[j] != NONE and np.array_equal(got[4], st), (what, j)
            assert same_f32(got[1][j, 3:6].view(np.float32), d2[j]).all() and same_f32(got[2][j], c2[j]).all(), (what, j, got[1][j], d2[j])
            want_ray = r[j].copy()
            want_ray[3:6] = d2[j].view(np.uint32)
            if what == "ray face_direction 9":
                want_ray[6] = 2  # read as Both, as rt_cast_rays reads it, and written as it was read
            assert same_rays(got[1][j:j + 1], want_ray[None]).all(), (what, j)
            for a, b in zip(got, base):
                assert (same_f32(a[others], b[others]) if a.dtype == np.float32 else a[others] == b[others]).all(), (what, j)
    # an unknown type is a black factor
    h_t, r_t = dev(hits), dev(rays)
    types = torch.full((n,), 3, dtype=torch.int32, device="cuda")
    fac = rt.scatter_factors(scene, h_t, r_t, types, r_t, torch.zeros(n, dtype=torch.float32, device="cuda"))
    torch.cuda.synchronize()
    assert (fac.cpu().numpy().view(np.uint32) == 0).all()
    # identity on an rt_rng of another size is refused, an empty batch is RT_OK
    rng, _ = seeded(n + 1)
    with pytest.raises(ValueError):
        rt.scatter_hits(scene, h_t, r_t, rng)
    lib = rt._capi.amd_lib()
    p = lambda t: C.c_void_p(t.data_ptr())
    out_t, out_r = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros((n, 11), dtype=torch.int32, device="cuda")
    assert lib.rt_scatter_hits(scene._h, p(h_t), p(r_t), n, rng._h, None, p(out_t), p(out_r), None, None) == -1
    assert lib.rt_scatter_hits(scene._h, p(h_t), p(r_t), 0, rng._h, p(out_t), p(out_t), p(out_r), None, None) == 0
    rng.close()


def _factor_inputs(scene, rays):
    torch = torch_device()
    n = rays.shape[0]
    rays_t = dev(rays)
    hits_t = rt.cast_rays(scene, rays_t)
    rng, _ = seeded(n)
    sc = rt.scatter_hits(scene, hits_t, rays_t, rng)
    nxt = rt.reflect_rays(hits_t, sc.rays)
    travel = torch.tensor(np.random.default_rng(3).uniform(0.0, 4.0, n).astype(np.float32), device="cuda")
    torch.cuda.synchronize()
    rng.close()
    return hits_t, rays_t, sc.type, nxt, travel


def test_factors_against_the_oracle_in_bands_and_in_a_graph(ref):
    """6. rt_scatter_factors: the oracle's get_diffuse / get_specular / pow; identical bits with RT_AMD_DIAG_HIT_BAND_RECORDS=64 and
    inside a captured HIP graph that is replayed once; the host form"""
    torch = torch_device()
    _, desc, scene, rays, _, _ = ref
    rays = rays[3072 - 500:3072 + 3511]  # 4011 records: not a multiple of 64
    hits_t, rays_t, types, nxt, travel = _factor_inputs(scene, rays)
    one = rt.scatter_factors(scene, hits_t, rays_t, types, nxt, travel)
    torch.cuda.synchronize()
    one = one.cpu().numpy()
    hits, t, nx, tr = hits_t.cpu().numpy().view(np.uint32), types.cpu().numpy().view(np.uint32), nxt.cpu().numpy().view(np.uint32), travel.cpu().numpy()
    want = np.zeros_like(one)
    lib = _oracle.lib()
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    d3, s3 = np.zeros(3, dtype=np.float32), np.zeros(3, dtype=np.float32)
    for i in np.flatnonzero(t <= 1):
        m = desc.materials[int(hits[i, 2])]
        uv = np.ascontiguousarray(hits[i, 9:11].view(np.float32))
        normal = np.ascontiguousarray(hits[i, 6:9].view(np.float32))
        view = np.ascontiguousarray(-rays[i, 3:6].view(np.float32))
        light = np.ascontiguousarray(nx[i, 3:6].view(np.float32))
        lib.orc_diffuse_specular(C.byref(m), p(uv), p(normal), p(view), p(light), p(d3), p(s3))
        want[i] = d3 if t[i] == DIFFUSE else s3
    fr = np.flatnonzero(t == REFRACTION)
    decay = np.array([desc.materials[int(o)].opaque_decay for o in hits[fr, 2]], dtype=np.float32)
    want[fr] = _oracle.math("pow", decay, tr[fr])[:, None]
    assert all((t == k).sum() > 50 for k in (DIFFUSE, REFLECTION, REFRACTION)) and (t == NONE).sum() > 50
    bad = np.flatnonzero(~same_f32(one, want).all(axis=1))
    assert bad.size == 0, f"{bad.size} factors differ, first {bad[:3]} types {t[bad[:3]]}: {one[bad[:2]]} want {want[bad[:2]]}"
    with rt.options(RT_AMD_DIAG_HIT_BAND_RECORDS=64):
        many = rt.scatter_factors(scene, hits_t, rays_t, types, nxt, travel)
        torch.cuda.synchronize()
    assert same_f32(many.cpu().numpy(), one).all()
    host = rt.scatter_factors_numpy(scene, hits, rays, t, nx, tr)
    assert same_f32(host, one).all()
    out = torch.full((rays.shape[0], 3), 7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rt.scatter_factors(scene, hits_t, rays_t, types, nxt, travel, out=out)
    out.fill_(7.0)
    graph.replay()
    torch.cuda.synchronize()
    assert same_f32(out.cpu().numpy(), one).all()
    # rt_scatter_hits in bands: the same bits and records as one launch
    n = rays.shape[0]
    a, _ = seeded(n)
    b, _ = seeded(n)
    x = rt.scatter_hits(scene, hits_t, rays_t, a)
    with rt.options(RT_AMD_DIAG_HIT_BAND_RECORDS=64):
        y = rt.scatter_hits(scene, hits_t, rays_t, b)
        torch.cuda.synchronize()
    assert np.array_equal(x.type.cpu().numpy(), y.type.cpu().numpy()) and same_rays(x.rays.cpu().numpy(), y.rays.cpu().numpy()).all()
    assert same_f32(x.cosine.cpu().numpy(), y.cosine.cpu().numpy()).all() and np.array_equal(a.download(), b.download())
    a.close()
    b.close()
