"""Path queries on the device (include/rt_amd.h rt_path_begin / rt_path_advance / rt_path_resolve) and the loop built from them
(paths.trace_paths).  Every device result is the CPU form's word for word; slots that are not listed keep their poison and paths that
ended leave zero rays and "no hit" records; one advance is the five calls it fuses, run on the device; trace_paths is its loop call
by call, replays from a graph and without bounces is shade_hits plus the sky; Russian roulette keeps the frame's mean; and every operand
of the three calls sits between poisoned guards that must come back untouched.  The hits are the reference scene's primary hits of a
48 x 27 frame — spheres, triangles, bump-mapped materials and misses — made once per module."""
import math

import numpy as np
import pytest

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import environment as E, lobes as L, materials, paths as P
import _guard_support as G
import _path_support as PS
from _lobe_support import assert_same
from _records import dev, host, torch_device, u32

pytestmark = pytest.mark.gpu
F32 = np.float32
WIDTH, HEIGHT = 48, 27
MIDDLE = (HEIGHT // 2) * WIDTH
BATCHES = [1, 63, 64, 65, 257]
OFF = P.NO_ROULETTE
POISON, POISON_BYTE = 0x5A5A5A5A, 0x5A
NO_HIT = np.array([0xFFFFFFFF] + [0] * 12, dtype=np.uint32)
BOTH = 2  # the face of a continuation ray and of its exclusion: words 6 and 10 of the record


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
    hits = u32(rt.cast_rays(b.scene, b.rays_t)).copy()
    solid = np.flatnonzero(hits[MIDDLE:MIDDLE + 64, 0] <= 1)
    hits[MIDDLE + solid[1], 2] = 9999  # a hit whose object_index names no material: "no hit" to every call
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
    rng = np.random.default_rng(5)
    b.img = rng.random((8, 16, 3), dtype=F32) * F32(2)
    b.env = E.Environment(torch.tensor(b.img, device="cuda"), 0.3, 1.5, E.NEAREST)
    return b


def run_advance(ref, rows, before, radiance, emitted, index, count, seed, kind, rr_start, rr_floor, last):
    """the device call on poisoned outputs -> host arrays (paths, radiance, rays, alive, hits)"""
    torch = torch_device()
    n = before.shape[0]
    paths_t, radiance_t = as_i32(before.view(np.uint32).reshape(n, 8)), torch.tensor(radiance, device="cuda")
    hits_t, incoming_t = ref.hits_t[rows].clone(), ref.rays_t[rows].contiguous()
    emitted_t = None if emitted is None else torch.tensor(emitted, device="cuda")
    rays_t = torch.full((n, 11), POISON, dtype=torch.int32, device="cuda")
    alive_t = torch.full((n,), POISON_BYTE, dtype=torch.uint8, device="cuda")
    index_t = count_t = None
    if index is not None:
        padded = np.full(n, 0xFFFFFFFF, dtype=np.uint32)
        padded[:len(index)] = index
        index_t, count_t = as_i32(padded), as_i32(np.array([count], dtype=np.uint32))
    P.advance(ref.scene, paths_t, hits_t, incoming_t, radiance_t, emitted_t, index_t, count_t, seed, kind, rr_start, rr_floor, last, rays_t, alive_t)
    torch.cuda.synchronize()
    return u32(paths_t).view(P.PATH_DTYPE).reshape(-1), host(radiance_t), u32(rays_t), host(alive_t), u32(hits_t)


def same_paths(got, want, what):
    for field in ("beta", "pdf"):
        assert_same(got[field], want[field], f"{field}: {what}", nan_ok=True)
    for field in ("root", "id", "bounce", "flags"):
        assert_same(got[field], want[field], f"{field}: {what}")


def want_rays_and_hits(hits, before, after, dirs, alive, poison_dirs):
    """the next rays restated from the CPU form's directions — continuation rays: face Both, the vertex's primitive excluded for both
    faces — and the hit records: a path that ended in this call leaves zero words and a "no hit" record; a slot that was not touched
    keeps the poison and its hit"""
    n = hits.shape[0]
    touched = (alive != POISON_BYTE)
    rays = np.full((n, 11), POISON, dtype=np.uint32)
    live = touched & (alive == 1)
    rays[touched] = 0
    rays[live, 0:3] = hits[live, 3:6]
    rays[live, 3:6] = dirs[live].view(np.uint32)
    rays[live, 6], rays[live, 7], rays[live, 10] = BOTH, 1, BOTH
    rays[live, 8], rays[live, 9] = hits[live, 0], hits[live, 1]
    want_hits = hits.copy()
    want_hits[touched & ~live] = NO_HIT
    assert (dirs[~touched] == poison_dirs[~touched]).all()
    return rays, want_hits


# ---- bits ----

CASES = [  # ids, index, count, kind, rr_start, last, emitted, bounce
    dict(),
    dict(ids=True, kind=P.GEOMETRIC, bounce=1),
    dict(ids=True, rr_start=0, bounce=2),
    dict(rr_start=0, rr_floor=0.6, kind=P.GEOMETRIC),
    dict(last=True, rr_start=0),
    dict(emitted=False, ids=True, bounce=5),
    dict(index="half", count="all"),
    dict(index="half", count=0),
    dict(index="half", count=1, ids=True, rr_start=0),
    dict(index="all", count="above", bounce=3, rr_start=2),
    dict(index="beyond", count="above", ids=True),  # every third entry names a slot >= n, and the padding is read too: they name nothing
]


@pytest.mark.parametrize("n", BATCHES)
def test_the_three_calls_are_their_cpu_forms(ref, n):
    torch = torch_device()
    rows = slice(MIDDLE, MIDDLE + n)
    rng = np.random.default_rng(n)
    surfaces, view, hits = ref.surfaces[rows], ref.view[rows], ref.hits[rows]
    ended = lived = 0
    for c, case in enumerate(CASES):
        ids = ids_of(n) if case.get("ids") else None
        kind, bounce = case.get("kind", P.SHADING), case.get("bounce", 0)
        rr_start, rr_floor, last = case.get("rr_start", OFF), case.get("rr_floor", 0.05), case.get("last", False)
        seed, what = 100 + c, f"n {n}, case {case}"
        # begin: the device's records are the CPU form's, spp 3 and spp 1
        for spp in (3, 1):
            ids_t = None if ids is None else as_i32(ids)
            paths_t = torch.full((spp * n, 8), POISON, dtype=torch.int32, device="cuda")
            radiance_t = torch.full((spp * n, 3), 9.0, dtype=torch.float32, device="cuda")
            P.begin(n, spp, ids_t, paths_t, radiance_t)
            want_paths, want_radiance = P.begin_numpy(n, spp, ids)
            assert_same(u32(paths_t).reshape(-1), want_paths.view(np.uint32), "begin: " + what)
            assert_same(host(radiance_t), want_radiance, "begin's radiance: " + what)
        before = want_paths.copy()  # spp 1
        before["beta"] = (rng.random((n, 3)) * (0.5 if rr_start == 0 else 2.0)).astype(F32)  # under roulette: a chance below 1 for most
        before["bounce"] += np.uint32(bounce)
        if n > 8:
            before["flags"][6] = P.DARK  # a path that ended before: listed or not, nothing of it moves
        start = rng.random((n, 3)).astype(F32)
        emitted = None if case.get("emitted") is False else rng.random((n, 3)).astype(F32)
        index = count = None
        if case.get("index"):
            index = rng.permutation(n)[:n if case["index"] == "all" else max(1, n // 2)].astype(np.uint32)
            if case["index"] == "beyond":
                index[::3] = n + 5 + np.arange(len(index[::3]), dtype=np.uint32)
            count = {"all": len(index), "above": n + 1000}.get(case["count"], case["count"])
        got_paths, got_radiance, got_rays, got_alive, got_hits = run_advance(ref, rows, before, start, emitted, index, count, seed, kind, rr_start, rr_floor, last)
        poison_dirs = np.full((n, 3), 7.0, dtype=F32)
        with np.errstate(all="ignore"):
            want = P.advance_numpy(surfaces, view, before, start, emitted, index, count, seed, ref.geometric[rows] if kind == P.GEOMETRIC else None, rr_start,
                                   rr_floor, last, poison_dirs, np.full(n, POISON_BYTE, dtype=np.uint8))
        same_paths(got_paths, want[0], what)
        assert_same(got_radiance, want[1], "radiance: " + what, nan_ok=True)
        assert_same(got_alive, want[3], "alive: " + what)
        want_rays, want_hits = want_rays_and_hits(hits, before, want[0], want[2], want[3], poison_dirs)
        assert_same(got_rays, want_rays, "rays: " + what)
        assert_same(got_hits, want_hits, "hits: " + what)
        # what is listed and alive was touched, nothing else
        listed = np.ones(n, dtype=bool) if index is None else np.isin(np.arange(n), index[:min(count, n)])
        touched = got_alive != POISON_BYTE
        assert (touched == (listed & (before["flags"] & P.ALIVE != 0))).all(), what
        assert_same(got_paths[~touched], before[~touched], "untouched paths: " + what)
        assert (got_radiance[~touched] == start[~touched]).all()
        if emitted is None:
            assert (got_radiance == start).all()
        # how each touched path ended
        flags = got_paths["flags"]
        valid = ref.valid[rows]
        assert (flags[touched & ~valid] == P.ESCAPED).all(), what  # every miss and the record that names no material
        if last:
            assert (flags[touched & valid] == 0).all() and not (got_alive[touched] == 1).any()
        if touched[min(ref.nan - MIDDLE, n - 1)] and n > ref.nan - MIDDLE and not last:
            assert flags[ref.nan - MIDDLE] == P.DARK  # the NaN normal: no density, no question
        if rr_start == OFF and not last:
            assert not (flags[touched] & P.ROULETTE).any()
        ended += int((touched & (got_alive == 0)).sum())
        lived += int((got_alive == 1).sum())
        if rr_start == 0 and not last and n >= 63 and index is None:
            assert (flags[touched] == P.ROULETTE).any() and (got_alive == 1).any(), what
    assert ended > 0 and (n < 63 or lived > 0)
    # resolve: spp 1 and spp 5, with and without roots
    for spp in (1, 5):
        radiance = (rng.random((spp * n, 3)) * 10).astype(F32)
        start = rng.random((n + 3, 3)).astype(F32)
        root = rng.permutation(n + 3)[:n].astype(np.uint32)
        out_t = torch.tensor(start[:n], device="cuda")
        P.resolve(torch.tensor(radiance, device="cuda"), n, spp, out_t)
        assert_same(host(out_t), P.resolve_numpy(radiance, n, spp, start[:n]), f"resolve: n {n}, spp {spp}")
        assert_same(host(out_t), PS.restated_resolve(radiance, n, spp, start[:n]), f"resolve restated: n {n}, spp {spp}")
        out_t = torch.tensor(start, device="cuda")
        P.resolve(torch.tensor(radiance, device="cuda"), n, spp, out_t, as_i32(root))
        assert_same(host(out_t), P.resolve_numpy(radiance, n, spp, start, root), f"resolve with roots: n {n}, spp {spp}")


@pytest.mark.parametrize("n", BATCHES)
def test_one_advance_is_the_five_calls_it_fuses(ref, n):
    """material_hits -> lobes.rays(spp 1, UNIFORM, the bounce's seed) -> probe_surfaces -> mis_weigh(divide_by_own) -> environment.fold
    (spp 1, into zeros), on the device, against one advance without roulette: bit for bit, -0 as +0; the ray is lobes.rays' but for its
    two face words, Both where the shadow ray says Back"""
    torch = torch_device()
    rows = slice(MIDDLE, MIDDLE + n)
    rng = np.random.default_rng(n + 1)
    hits_t, incoming_t, view_t = ref.hits_t[rows].contiguous(), ref.rays_t[rows].contiguous(), ref.view_t[rows].contiguous()
    for kind, bounce, ids in ((P.SHADING, 0, None), (P.GEOMETRIC, 1, ids_of(n)), (P.SHADING, 5, ids_of(n))):
        seed = 0xABCD0000 + bounce
        before = PS.records(n, 1, ids, (rng.random((n, 3)) * 2).astype(F32), bounce)
        ids_t = None if ids is None else as_i32(ids)
        surfaces_t = materials.material_hits(ref.scene, hits_t)
        rays_t, asks_t, dirs_t, pdf_t, lobe_t = L.rays(ref.scene, hits_t, incoming_t, 1, L.UNIFORM, PS.seed_of(seed, bounce), ids_t, kind)
        diffuse_t, specular_t = materials.probe_surfaces(surfaces_t, view_t, dirs_t.view(1, n, 3))
        t_t = torch.tensor(before["beta"], device="cuda")
        L.mis_weigh(pdf_t, 1, None, 0, L.BALANCE, True, None, t_t)
        beta_t = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
        E.fold(ref.scene, hits_t, asks_t, 1, t_t, diffuse_t.view(n, 3), specular_t.view(n, 3), beta_t)
        torch.cuda.synchronize()
        beta, asks, lobe = host(beta_t), host(asks_t), host(lobe_t)
        got_paths, _, got_rays, got_alive, _ = run_advance(ref, rows, before, np.zeros((n, 3), F32), None, None, None, seed, kind, OFF, 0.05, False)
        lives = (asks != 0) & PS.positive(beta)
        what = f"n {n}, kind {kind}, bounce {bounce}"
        assert_same(got_alive, lives.astype(np.uint8), "alive: " + what)
        assert_same(PS.no_negative_zero(got_paths["beta"][lives]), PS.no_negative_zero(beta[lives]), "beta: " + what)
        assert_same(got_paths["pdf"][lives], host(pdf_t)[lives], "pdf: " + what)
        assert_same(got_paths["flags"][lives], (P.ALIVE | np.where(lobe[lives] != 0, P.SPECULAR, 0)).astype(np.uint32), "lobe: " + what)
        want_rays = u32(rays_t).copy()  # rt_lobe_rays' shadow ray with exactly its two face words replaced
        want_rays[:, 6] = want_rays[:, 10] = BOTH
        assert_same(got_rays[lives], want_rays[lives], "the continuation ray: " + what)
        assert not got_rays[~lives].any() and (got_paths["bounce"][lives] == bounce + 1).all()
        assert (got_paths["flags"][~lives] == np.where(ref.valid[rows][~lives], P.DARK, P.ESCAPED)).all()
        assert n < 63 or lives.any()


# ---- the loop ----

def loop_by_hand(ref, spp, max_bounces, env, rr_start, rr_floor, seed, out_t):
    """trace_paths again, call by call from the public functions, every buffer made here"""
    torch = torch_device()
    n, m = ref.n, spp * ref.n
    paths_t, radiance_t = P.begin(n, spp)
    vertices = ref.hits_t.repeat(spp, 1).contiguous()
    rays = ref.rays_t.repeat(spp, 1).contiguous()
    index = count = None
    for b in range(max_bounces + 1):
        emitted = rt.shade_hits(ref.scene, vertices, rays)
        if env is not None:
            E.lookup(env, rays, vertices, out=emitted)
        next_rays = torch.zeros((m, 11), dtype=torch.int32, device="cuda")
        alive = torch.zeros((m,), dtype=torch.uint8, device="cuda") if b == 0 else alive
        P.advance(ref.scene, paths_t, vertices, rays, radiance_t, emitted, index, count, seed, P.SHADING, rr_start, rr_floor, b == max_bounces, next_rays, alive)
        if b == max_bounces:
            break
        index, count = rt.select_records(alive)
        rt.cast_rays_indexed(ref.scene, next_rays, index, count, vertices)
        rays = next_rays
    P.resolve(radiance_t, n, spp, out_t)
    return paths_t, radiance_t


def test_trace_paths_is_its_loop_replays_and_starts_from_shade_hits(ref):
    torch = torch_device()
    n, spp, bounces = ref.n, 2, 3
    start = np.random.default_rng(2).random((n, 3)).astype(F32)
    want_t = torch.tensor(start, device="cuda")
    loop_by_hand(ref, spp, bounces, ref.env, 1, 0.3, 17, want_t)
    for open_casts in (True, False):
        got_t = torch.tensor(start, device="cuda")
        assert P.trace_paths(ref.scene, ref.hits_t, ref.rays_t, spp, bounces, ref.env, 1, 0.3, 17, None, got_t, open_casts) is got_t
        torch.cuda.synchronize()
        assert G.same_or_both_nan(host(got_t), host(want_t)), f"open_casts {open_casts}"
    want = host(want_t)
    assert (want[ref.valid] != start[ref.valid]).any() and np.isfinite(want[ref.valid & (np.arange(n) != ref.nan)]).all()
    # without bounces: shade_hits, plus the sky on the misses, added to out
    shade = rt.shade_hits(ref.scene, ref.hits_t, ref.rays_t)
    E.lookup(ref.env, ref.rays_t, ref.hits_t, out=shade)
    got_t = torch.tensor(start, device="cuda")
    P.trace_paths(ref.scene, ref.hits_t, ref.rays_t, 1, 0, ref.env, out=got_t)
    torch.cuda.synchronize()
    assert G.same_or_both_nan(host(got_t), (start + F32(1) * host(shade)).astype(F32))
    assert host(shade)[~ref.valid].any() and host(shade)[ref.valid].any()
    # a graph: after one eager call on the stream the whole loop is captured, and two replays give the same bits
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        w = P.workspace(n, "cuda", spp, ref.scene)
        out_t = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
        P.trace_paths(ref.scene, ref.hits_t, ref.rays_t, spp, bounces, ref.env, 1, 0.3, 17, None, out_t, True, stream, w)
        stream.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            P.trace_paths(ref.scene, ref.hits_t, ref.rays_t, spp, bounces, ref.env, 1, 0.3, 17, None, out_t, True, stream, w)
        replays = []
        for _ in range(2):
            out_t.copy_(torch.tensor(start, device="cuda"))
            stream.synchronize()
            graph.replay()
            stream.synchronize()
            replays.append(host(out_t))
    assert G.same_or_both_nan(replays[0], want) and G.same_or_both_nan(replays[1], want)


def test_roulette_keeps_the_mean(ref):
    """spp 64 and 4 bounces on the whole frame, with roulette from bounce 1 and without: the two frame-mean luminances agree within 5
    combined standard errors, each from its own run's per-path radiance"""
    torch = torch_device()
    n, spp, bounces = ref.n, 64, 4
    m = n * spp
    luma = np.array([0.2126, 0.7152, 0.0722])
    w = P.workspace(n, "cuda", spp, ref.scene)
    # the records with a NaN normal or no material give NaN or nothing in both runs alike: the mean is taken over the others
    keep = np.tile(np.arange(n) != ref.nan, spp)
    means, errors, flags = [], [], []
    for rr_start in (1, OFF):
        P.trace_paths(ref.scene, ref.hits_t, ref.rays_t, spp, bounces, ref.env, rr_start, 0.05, 23, workspace=w)
        torch.cuda.synchronize()
        per_path = host(w.radiance[:m]).astype(np.float64)[keep] @ luma
        assert np.isfinite(per_path).all()
        means.append(per_path.mean())
        errors.append(per_path.std(ddof=1) / math.sqrt(per_path.size))
        flags.append(u32(w.paths[:m]).view(P.PATH_DTYPE).reshape(-1).copy())
    played, free = flags
    # not vacuous: roulette ended paths, and paths were still alive after bounce 3 (they took a fourth bounce and met `last`)
    assert (played["flags"] == P.ROULETTE).sum() > 0 and not (free["flags"] == P.ROULETTE).any()
    assert ((played["bounce"] & 0xFFFFFF) == 4).sum() > 0 and ((played["bounce"] & 0xFFFFFF) == 4).sum() < ((free["bounce"] & 0xFFFFFF) == 4).sum()
    combined = math.sqrt(errors[0] ** 2 + errors[1] ** 2)
    sigmas = abs(means[0] - means[1]) / combined
    print(f"roulette: mean luminance {means[0]:.6f} with, {means[1]:.6f} without; {sigmas:.3f} combined standard errors "
          f"({(played['flags'] == P.ROULETTE).sum()} of {m} paths ended by roulette)")
    assert sigmas <= 5, f"the frame means differ by {sigmas:.3f} combined standard errors ({means[0]} with roulette, {means[1]} without, se {combined})"


# ---- no call writes outside its operands ----

@pytest.mark.parametrize("n", BATCHES)
def test_every_operand_stays_between_its_guards(ref, n):
    torch = torch_device()
    spp = 3
    m = spp * n
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
    ids = operand((n,), torch.int32, as_i32(ids_of(n)))
    paths_t, radiance = operand((m, 8), torch.int32), operand((m, 3), torch.float32)
    P.begin(n, spp, ids, paths_t, radiance)
    hits_t = operand((m, 13), torch.int32, ref.hits_t[rows].repeat(spp, 1))
    incoming = operand((m, 11), torch.int32, ref.rays_t[rows].repeat(spp, 1))
    emitted = operand((m, 3), torch.float32, torch.ones((m, 3), device="cuda"))
    rays, alive = operand((m, 11), torch.int32), operand((m,), torch.uint8)
    index = operand((m,), torch.int32, torch.arange(m - 1, -1, -1, dtype=torch.int32, device="cuda"))
    count = operand((1,), torch.int32, torch.tensor([m + 5], dtype=torch.int32, device="cuda"))
    P.advance(ref.scene, paths_t, hits_t, incoming, radiance, emitted, index, count, 3, P.SHADING, 0, 0.5, False, rays, alive)
    torch.cuda.synchronize()
    want = P.advance_numpy(np.tile(ref.surfaces[rows], spp), np.tile(ref.view[rows], (spp, 1)), P.begin_numpy(n, spp, ids_of(n))[0], np.zeros((m, 3), F32),
                           np.ones((m, 3), F32), seed=3, rr_start=0, rr_floor=0.5)
    assert_same(u32(paths_t).reshape(-1), want[0].view(np.uint32), "the guarded paths")
    assert_same(host(alive), want[3], "the guarded flags")
    root = operand((n,), torch.int32, torch.arange(n - 1, -1, -1, dtype=torch.int32, device="cuda"))
    rgb = operand((n, 3), torch.float32, torch.ones((n, 3), device="cuda"))
    P.resolve(radiance, n, spp, rgb, root)
    torch.cuda.synchronize()
    assert_same(host(rgb), P.resolve_numpy(want[1], n, spp, np.ones((n, 3), F32), np.arange(n - 1, -1, -1)), "the guarded rgb")
    for whole, guard, payload in held:
        w = u32(whole)
        assert (w[:guard] == G.SENTINEL).all() and (w[guard + payload:] == G.SENTINEL).all(), "a store outside an operand"
