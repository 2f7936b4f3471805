"""Refraction queries on the device (include/rt_amd.h rt_refract_enter / rt_refract_step) and the loop built from them
(rt.refract_rays_by_bounce): the loop against rt_refract_rays and the oracle's orc_get_refract — kind, travel, escape ray, cast count;
the state after the entry and after every round against get_refract replayed bounce by bounce on the CPU from the oracle's orc_cast,
orc_reflect and orc_refract_dir; records and state words a caller got wrong; a bounce limit; a scene walked breadth-first; the two level
loops with every cast opened; graph capture.  The batches and everything expected of them are made on the CPU with the oracle alone,
once per module.  Every comparison is of f32 bit patterns: any NaN equals any NaN, -0.0 differs from +0.0."""
import ctypes as C

import numpy as np
import pytest

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd._capi import Material
import _oracle
import _scenes
import _hit_support as hq
import _scatter_support as sq
from _records import camera_rays_cpu, dev, host, oracle_hits, ray_records, same_f32, same_rays, source_b, source_c, tessellated_scene, torch_device, u32
from _light_support import dist32

pytestmark = pytest.mark.gpu
NONE = 0xFFFFFFFF
ESCAPED, INFINITE, TRAPPED, WALKING = 0, 1, 2, 3
FRONT, BACK = 0, 1
ROUNDS = 11


# ---- the expected side: get_refract (main.rs:343-405) replayed one cast at a time, on the CPU, from the oracle's exports ----


def normalize32(v):
    """cgmath's normalize in f32: v * (1 / magnitude), the dot product summed left to right"""
    v = np.asarray(v, dtype=np.float32)
    with np.errstate(all="ignore"):
        return v * (np.float32(1.0) / np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]))


def ray_words(origin, direction, face, kind, index, ex_face):
    r = np.zeros(11, dtype=np.uint32)
    r[0:3] = np.asarray(origin, dtype=np.float32).view(np.uint32)
    r[3:6] = np.asarray(direction, dtype=np.float32).view(np.uint32)
    r[6], r[7], r[8], r[9], r[10] = face, 1, kind, index, ex_face
    return r


class State:
    """the five state arrays and the escape rays, as the device holds them after a call"""

    def __init__(self, n):
        self.kind = np.full(n, NONE, dtype=np.uint32)
        self.travel = np.zeros(n, dtype=np.float32)
        self.casts = np.zeros(n, dtype=np.uint32)
        self.flags = np.zeros(n, dtype=np.uint8)
        self.rays = np.zeros((n, 11), dtype=np.uint32)
        self.escape = np.zeros((n, 11), dtype=np.uint32)

    def copy(self):
        s = State(0)
        for name in ("kind", "travel", "casts", "flags", "rays", "escape"):
            setattr(s, name, getattr(self, name).copy())
        return s


def replay(desc, rays, hits, max_distance, rounds=ROUNDS):
    """states[0]: after the entry; states[r]: after r answered casts.  why[i]: how record i ended — the fixture's histogram"""
    rays = np.ascontiguousarray(rays).view(np.uint32).reshape(-1, 11).copy()
    hits = np.ascontiguousarray(hits).view(np.uint32).reshape(-1, 13).copy()
    n = rays.shape[0]
    lib = _oracle.lib()
    orays, ohits = (_oracle.OrcRay * n).from_buffer(rays), (_oracle.OrcHit * n).from_buffer(hits)
    max_distance = np.float32(max_distance)
    s = State(n)
    why = np.array(["not a hit"] * n, dtype=object)
    index = np.zeros(n, dtype=np.float32)  # the material's refraction index, per record
    v = (C.c_float * 3)()
    for i in np.flatnonzero((hits[:, 0] <= 1) & (hits[:, 2] < desc.n_materials)):
        index[i] = desc.materials[int(hits[i, 2])].refraction_index  # main.rs:354 (not generative in these scenes)
        if lib.orc_refract_dir(ohits[i].normal, orays[i].direction, float(index[i]), v):
            s.kind[i], s.flags[i] = WALKING, 1
            s.rays[i] = ray_words(ohits[i].position[:], normalize32(v[:]), BACK, hits[i, 0], hits[i, 1], FRONT)  # ray_inside
            why[i] = "walking"
        else:
            s.kind[i] = TRAPPED
            why[i] = "trapped at entry"
    states = [s.copy()]
    inside, bounce = _oracle.OrcHit(), _oracle.OrcRay()
    with np.errstate(all="ignore"):
        for _ in range(rounds):
            s.flags[:] = 0
            for i in np.flatnonzero(s.kind == WALKING):
                j = int(s.casts[i])
                s.casts[i] = j + 1
                cur = s.rays[i].copy()
                ray = _oracle.OrcRay.from_buffer(cur)
                if not lib.orc_cast(C.byref(desc), C.byref(ray), C.byref(inside)):
                    s.kind[i] = INFINITE  # main.rs:373, 383: s.rays[i] stays, the ray whose cast missed
                    why[i] = "infinite at the first cast" if j == 0 else "infinite after a bounce"
                    continue
                pos = np.array(inside.position[:], dtype=np.float32)
                if j == 0:
                    s.travel[i] = dist32(pos, hits[i, 3:6].view(np.float32))  # main.rs:375
                else:
                    s.travel[i] = s.travel[i] + dist32(cur[0:3].view(np.float32), pos)  # main.rs:385
                have_out = lib.orc_refract_dir(inside.normal, ray.direction, float(np.float32(1.0) / index[i]), v)
                if not have_out and s.travel[i] <= max_distance and j < 10:  # main.rs:378
                    lib.orc_reflect(C.byref(inside), C.byref(ray), C.byref(bounce))
                    s.rays[i] = np.frombuffer(bytes(bounce), dtype=np.uint32)
                    s.flags[i] = 1
                elif have_out:
                    s.kind[i] = ESCAPED
                    s.escape[i] = ray_words(pos, normalize32(v[:]), FRONT, inside.kind, inside.index, BACK)
                    why[i] = "escaped without a bounce" if j == 0 else "escaped after a bounce"
                else:
                    s.kind[i] = TRAPPED
                    why[i] = "trapped at the retry cap" if s.travel[i] <= max_distance else "trapped by the distance"
            states.append(s.copy())
    return states, why


def glass(index):
    m = Material()
    m.diffuse_fn = m.normal_fn = 0
    m.normal = (0.0, 0.0, 1.0)
    m.diffuse_color, m.specular_color = (0.2, 0.3, 0.4), (0.5, 0.5, 0.5)
    m.shiness, m.smoothness, m.transparency, m.refraction_index, m.opaque_decay = 0.1, 0.5, 0.9, index, 0.3
    return m


SLIM, WIDE = ((30.0, 2.0, 30.0), (0.1, 2.0, 0.1)), ((300.0, 130.0, 300.0), (6.0, 120.0, 6.0))  # (centre, half extents) of two closed boxes
THIN = ((30.0, 2.0, 40.0), 1.0)  # a sphere of a medium thinner than its surroundings (refraction index 0.6)


def fixture_world():
    """the reference scene and, far from it, two closed glass boxes 20 times as tall as wide: a ray that enters the top face steeply is
    totally reflected from side to side on its way down — in the slim box more than ten times over a few units (the retry cap), in the
    wide box over more than 100 units (max_distance) — and one that enters it gently comes out through the bottom; and a sphere with a
    refraction index below 1, which a grazing ray cannot enter at all (main.rs:356-358)"""
    world = rt.reference_world()
    world.push_object(glass(0.6)).push_sphere(*THIN)
    for centre, half in (SLIM, WIDE):
        box = world.push_object(glass(1.5))
        for tri in _scenes._box(centre, half, np.eye(3)):
            box.push_flat_triangle(tri, [(0.0, 0.0), (0.0, 1.0), (1.0, 0.0)])
    return world


def box_rays(seed, n_each):
    """rays from above onto the top faces of the two boxes, from nearly vertical to 80 degrees off"""
    g = np.random.default_rng(seed)
    out = []
    for centre, half in (SLIM, WIDE):
        c, h = np.asarray(centre), np.asarray(half)
        target = c + np.array([0.0, h[1], 0.0]) + np.stack([g.uniform(-0.8, 0.8, n_each) * h[0], np.zeros(n_each), g.uniform(-0.8, 0.8, n_each) * h[2]], axis=1)
        tilt, turn = np.radians(g.uniform(2.0, 80.0, n_each)), g.uniform(0.0, 2 * np.pi, n_each)
        d = np.stack([np.sin(tilt) * np.cos(turn), -np.cos(tilt), np.sin(tilt) * np.sin(turn)], axis=1)
        out.append(ray_records(target - d * (0.5 * h[0]), d, FRONT))
    u = g.normal(size=(n_each // 2, 3))  # towards points of the sphere's disc as seen from the origin: centre to rim
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    origins = np.asarray(THIN[0]) + u * 5.0
    side = np.cross(u, g.normal(size=u.shape))
    side /= np.linalg.norm(side, axis=1, keepdims=True)
    d = np.asarray(THIN[0]) + side * (g.uniform(0.0, 0.98, (u.shape[0], 1)) * THIN[1]) - origins
    out.append(ray_records(origins, d / np.linalg.norm(d, axis=1, keepdims=True), FRONT))
    return np.concatenate(out)


KINDS = ("not a hit", "trapped at entry", "infinite at the first cast", "escaped without a bounce", "escaped after a bounce",
         "trapped by the distance", "trapped at the retry cap")
SMALL = 0.05  # a max_distance that stops walks after their first bounces


class Batch:
    pass


def make_ref():
    """4 011 records: 48x36 camera rays, random rays, rays started inside the glass of the reference scene (sources b and c of
    tests/test_gpu_hit_queries.py), and rays into the two boxes.  Holds every kind of end, by the replay — asserted here, so that a
    fixture that lacks one cannot pass silently"""
    b = Batch()
    b.world = fixture_world()
    b.desc = b.world.desc()
    plain = rt.reference_world().desc()
    b.rays = np.concatenate([camera_rays_cpu(rt.reference_camera(), 48, 36), source_b(plain, 3, 1272), source_c(plain, 3, 237),
                             box_rays(5, 120)])
    b.n = b.rays.shape[0]
    assert b.n == 4011
    b.hits = oracle_hits(b.desc, b.rays)
    b.runs = {}
    for max_distance in (100.0, float("inf"), SMALL):
        states, why = replay(b.desc, b.rays, b.hits, max_distance)
        # the replay is get_refract: the oracle's own, in one piece, says the same
        want = hq.oracle_queries(b.desc, b.rays, b.hits, max_distance, rows=np.flatnonzero((b.hits[:, 0] <= 1) & (b.hits[:, 2] < b.desc.n_materials)))
        last = states[-1]
        assert np.array_equal(last.kind, want.kind), max_distance
        esc = last.kind == ESCAPED
        assert same_f32(last.travel[esc], want.travel[esc]).all() and same_rays(last.escape, want.escape).all(), max_distance
        assert not (last.kind == WALKING).any() and last.casts.max() <= 11
        b.runs[max_distance] = (states, why)
    hist = {k: int((b.runs[100.0][1] == k).sum()) for k in KINDS}
    print("max_distance 100:", hist)
    assert all(v > 0 for v in hist.values()), hist
    small = b.runs[SMALL][1]
    assert (small == "trapped by the distance").sum() > (b.runs[100.0][1] == "trapped by the distance").sum()
    assert (b.runs[float("inf")][1] == "trapped by the distance").sum() == 0
    assert (b.runs[100.0][0][-1].casts == 11).sum() > 0  # eleven answered casts
    return b


@pytest.fixture(scope="module")
def ref():
    return make_ref()


def final(states):
    """what rt_refract_rays reports of the last state: travel is 0 where the record did not escape"""
    last = states[-1]
    return last.kind, np.where(last.kind == ESCAPED, last.travel, np.float32(0.0)).astype(np.float32), last.escape, int(last.casts.sum())


# ---- the device side ----


def fused(scene, hits_t, rays_t, max_distance):
    torch = torch_device()
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    r = rt.refract_rays(scene, hits_t, rays_t, max_distance, ray_count=cnt)
    torch.cuda.synchronize()
    return u32(r.kind), host(r.travel), u32(r.rays), int(host(cnt)[0])


def sentinel_out(n):
    torch = torch_device()
    return rt.Refractions(torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda"), torch.full((n,), 99.0, dtype=torch.float32, device="cuda"),
                          torch.full((n, 11), 0x5A5A5A5A, dtype=torch.int32, device="cuda"))


def by_bounce(scene, hits_t, rays_t, max_distance, rounds=ROUNDS, stream=None, out=None, workspace=None, resume=False):
    """the loop, with every synchronising torch call inside it an error: no host visit hides there"""
    torch = torch_device()
    n = hits_t.shape[0]
    out = sentinel_out(n) if out is None else out
    ws = rt.refract_workspace(n, "cuda") if workspace is None else workspace
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        rt.refract_rays_by_bounce(scene, hits_t, rays_t, max_distance, ray_count=cnt, stream=stream, out=out, rounds=rounds, workspace=ws, resume=resume)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    return (u32(out.kind), host(out.travel), u32(out.rays), int(host(cnt)[0])), (out, ws)


def assert_refractions(got, want, what):
    bad = np.flatnonzero(got[0] != want[0])
    assert bad.size == 0, f"{what}: kind differs in {bad.size} of {want[0].size}, first rows {bad[:5]}: {got[0][bad[:5]]} want {want[0][bad[:5]]}"
    bad = np.flatnonzero(~same_f32(got[1], want[1]))
    assert bad.size == 0, f"{what}: travel differs in {bad.size}, first rows {bad[:5]}: {got[1][bad[:3]]} want {want[1][bad[:3]]}"
    bad = np.flatnonzero(~same_rays(got[2], want[2]))
    assert bad.size == 0, f"{what}: escape rays differ in {bad.size}, first rows {bad[:5]}: {got[2][bad[:1]]} want {want[2][bad[:1]]}"
    assert got[3] == want[3], (what, "casts", got[3], want[3])


def rows_of(b, size, why):
    """`size` rows with a stride, so that each batch holds records of every source; a single record: one that makes eleven casts"""
    if size == 1:
        return np.flatnonzero(why == "trapped at the retry cap")[:1]
    return np.arange(size) * (b.n // size)


@pytest.mark.parametrize("max_distance", [100.0, float("inf"), SMALL])
@pytest.mark.parametrize("size", [1, 63, 64, 65, 4011])
def test_the_loop_is_refract_rays(ref, size, max_distance):
    """1. refract_rays_by_bounce == rt.refract_rays == get_refract replayed on the CPU: kind, travel, escape words and cast count; and
    the casts counted per record add up to that count"""
    torch_device()
    scene = rt.Scene(ref.world)
    states, why = ref.runs[max_distance]
    rows = rows_of(ref, size, ref.runs[100.0][1])
    sub = [State(0) for _ in states]
    for s, full in zip(sub, states):
        for name in ("kind", "travel", "casts", "flags", "rays", "escape"):
            setattr(s, name, getattr(full, name)[rows])
    want = final(sub)
    assert want[3] > 0
    hits_t, rays_t = dev(ref.hits[rows]), dev(ref.rays[rows])
    assert_refractions(fused(scene, hits_t, rays_t, max_distance), want, f"{size} records, {max_distance}: rt_refract_rays against the replay")
    got, (out, ws) = by_bounce(scene, hits_t, rays_t, max_distance)
    assert_refractions(got, want, f"{size} records, {max_distance}: the loop")
    casts = u32(ws.casts)
    assert np.array_equal(casts, sub[-1].casts) and int(casts.sum()) == got[3]
    assert (host(ws.flags) == 0).all()  # nothing is left to cast


def run_rounds(scene, hits_t, rays_t, max_distance, rounds=ROUNDS, tamper=None):
    """refract_enter, then `rounds` times select_records -> cast_rays_indexed -> refract_step, every output filled with a sentinel first;
    the state downloaded after every call.  tamper(state tensors): a caller's writes between the entry and the first round"""
    torch = torch_device()
    n = hits_t.shape[0]
    i32 = torch.int32
    rays_s = torch.full((n, 11), 0x5A5A5A5A, dtype=i32, device="cuda")
    kind, casts = torch.full((n,), 0x5A5A5A5A, dtype=i32, device="cuda"), torch.full((n,), 0x5A5A5A5A, dtype=i32, device="cuda")
    travel, flags = torch.full((n,), 99.0, dtype=torch.float32, device="cuda"), torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda")
    escape = torch.full((n, 11), 0x5A5A5A5A, dtype=i32, device="cuda")
    inside = torch.full((n, 13), 0x5A5A5A5A, dtype=i32, device="cuda")  # kind 0x5a5a5a5a: neither 0 nor 1
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    got = []

    def download():
        torch.cuda.synchronize()
        s = State(0)
        s.kind, s.travel, s.casts, s.flags, s.rays, s.escape = u32(kind), host(travel), u32(casts), host(flags), u32(rays_s), u32(escape)
        s.inside, s.count = u32(inside), int(host(cnt)[0])
        got.append(s)

    rt.refract_enter(scene, hits_t, rays_t, rays_s, kind, travel, casts, flags)
    download()
    if tamper is not None:
        tamper(rays_s, kind, travel, casts, flags, inside)
    for _ in range(rounds):
        index, count = rt.select_records(flags)
        rt.cast_rays_indexed(scene, rays_s, index, count, inside, ray_count=cnt)
        rt.refract_step(scene, hits_t, inside, rays_s, kind, travel, casts, flags, max_distance, out_escape=escape)
        download()
    return got


def assert_state(got, want, what, escape_written):
    for name in ("kind", "casts", "flags"):
        bad = np.flatnonzero(getattr(got, name) != getattr(want, name))
        assert bad.size == 0, f"{what}: {name} differs in {bad.size}, first rows {bad[:5]}: {getattr(got, name)[bad[:5]]} want {getattr(want, name)[bad[:5]]}"
    bad = np.flatnonzero(~same_f32(got.travel, want.travel))
    assert bad.size == 0, f"{what}: travel differs in {bad.size}, first rows {bad[:5]}: {got.travel[bad[:3]]} want {want.travel[bad[:3]]}"
    bad = np.flatnonzero(~same_rays(got.rays, want.rays))
    assert bad.size == 0, f"{what}: the rays in flight differ in {bad.size}, first rows {bad[:5]}: {got.rays[bad[:1]]} want {want.rays[bad[:1]]}"
    # the escape ray of a record is written in the round that finishes it — zeros unless it escaped — and by nothing else
    assert same_rays(got.escape[escape_written], want.escape[escape_written]).all(), what
    assert (got.escape[~escape_written] == 0x5A5A5A5A).all(), what


@pytest.mark.parametrize("max_distance", [100.0, SMALL])
def test_every_round_against_the_replay(ref, max_distance):
    """2. after the entry and after each of the eleven steps, d_kind, d_travel, d_casts, d_flags and the words of d_rays are the CPU
    replay's; the ray an Infinite record keeps is the ray whose orc_cast misses"""
    torch_device()
    scene = rt.Scene(ref.world)
    states, why = ref.runs[max_distance]
    got = run_rounds(scene, dev(ref.hits), dev(ref.rays), max_distance)
    assert len(got) == len(states) == ROUNDS + 1
    walked = states[0].kind == WALKING
    for r, (g, w) in enumerate(zip(got, states)):
        assert_state(g, w, f"max_distance {max_distance}, after {r} rounds", walked & (w.kind != WALKING))
        assert g.count == int(w.casts.sum()), r  # what rt_cast_rays_indexed counted is the sum of d_casts, round by round
    assert (got[0].travel.view(np.uint32) == 0).all() and (got[0].casts == 0).all()
    infinite = np.flatnonzero(got[-1].kind == INFINITE)
    assert infinite.size > 0
    lib = _oracle.lib()
    h = _oracle.OrcHit()
    for i in infinite:
        words = got[-1].rays[i].copy()
        assert words[6] == BACK and words[7] == 1
        assert not lib.orc_cast(C.byref(ref.desc), C.byref(_oracle.OrcRay.from_buffer(words)), C.byref(h)), i


def test_foreign_records(ref):
    """3. records and state words a caller got wrong, outputs filled with a sentinel first: exactly the documented words are written, and
    nothing is cast for a finished record.  Validation, not an attempt at a fault: nothing in the kernels is indexed with a state word"""
    torch = torch_device()
    desc = ref.desc
    scene = rt.Scene(ref.world)
    states, why = ref.runs[100.0]
    long_walks = np.flatnonzero(states[-1].casts >= 4)
    rows = np.concatenate([np.flatnonzero(states[0].kind == WALKING)[::23][:50], long_walks[:15]])  # one full wave plus one lane
    assert rows.size == 65
    rays, hits = ref.rays[rows].copy(), ref.hits[rows].copy()
    hits[3, 0] = 7                  # kind 7: no hit
    hits[10, 2] = desc.n_materials  # object_index >= n_materials: no hit
    hits[64, 0] = NONE              # a miss, in the tail wave
    hits[30, 1] = 0x7FFFFFF0        # an index outside its array: only ever an exclusion, and as one excludes nothing
    no_hit = np.array([3, 10, 64])
    want, _ = replay(desc, rays, hits, 100.0)
    got = run_rounds(scene, dev(hits), dev(rays), 100.0)
    for r, (g, w) in enumerate(zip(got, want)):
        assert_state(g, w, f"foreign hits, after {r} rounds", (want[0].kind == WALKING) & (w.kind != WALKING))
    assert (got[-1].kind[no_hit] == NONE).all() and (got[-1].rays[no_hit] == 0).all() and (got[-1].casts[no_hit] == 0).all()
    assert (got[-1].inside[no_hit] == 0x5A5A5A5A).all()  # nothing was cast for them
    assert_refractions(by_bounce(scene, dev(hits), dev(rays), 100.0)[0], fused(scene, dev(hits), dev(rays), 100.0), "the loop against rt_refract_rays")

    # state words a caller wrote between the entry and the first round
    base = replay(desc, rays, hits, 100.0)[0]
    walking = np.flatnonzero(base[0].kind == WALKING)
    a, b, c, d, e, f = walking[[1, 5, 8, 12, 20, 33]]

    def tamper(rays_s, kind, travel, casts, flags, inside):
        kind[a] = -1          # 0xffffffff: finished, whatever the word says — but its flag is still set, so it is cast once
        kind[b] = 0x7FFF0000  # garbage: finished
        casts[c] = 10         # the retry cap is reached: this cast is the last
        casts[d] = -(1 << 31)  # 2^31: only fails `casts < 10`
        rays_s[e, 9] = 0x7FFFFFF0  # an exclusion index beyond the arrays: excludes nothing
        rays_s[f, 8] = 9      # an exclusion of no kind: excludes nothing

    t = run_rounds(scene, dev(hits), dev(rays), 100.0, tamper=tamper)
    last = t[-1]
    assert last.kind[a] == NONE and last.kind[b] == 0x7FFF0000  # left as the caller wrote them
    for i in (a, b):
        assert (last.escape[i] == 0x5A5A5A5A).all() and last.casts[i] == 0 and last.flags[i] == 0 and same_rays(last.rays[i], t[0].rays[i]).all()
        assert last.travel[i].view(np.uint32) == 0
    for i, start in ((c, 10), (d, 1 << 31)):
        assert last.casts[i] == start + 1 and last.kind[i] in (ESCAPED, INFINITE, TRAPPED), (i, last.kind[i])
        assert t[1].kind[i] == last.kind[i] and t[1].flags[i] == 0  # one cast, and the walk is over
    assert (t[1].kind[[c, d]] != WALKING).all()
    # the exclusions that exclude nothing: the oracle casts the same record and the walk goes on from what it finds
    lib = _oracle.lib()
    h = _oracle.OrcHit()
    for i in (e, f):
        words = t[0].rays[i].copy()
        words[[9] if i == e else [8]] = 0x7FFFFFF0 if i == e else 9
        hit = lib.orc_cast(C.byref(desc), C.byref(_oracle.OrcRay.from_buffer(words)), C.byref(h))
        if hit:
            assert np.array_equal(t[1].inside[i], np.frombuffer(bytes(h), dtype=np.uint32)), i
        else:
            assert t[1].inside[i, 0] == NONE and t[1].kind[i] == INFINITE, i
    others = np.setdiff1d(np.arange(65), [a, b, c, d, e, f])
    for name in ("kind", "casts", "flags"):
        assert np.array_equal(getattr(last, name)[others], getattr(base[-1], name)[others]), name
    assert same_f32(last.travel[others], base[-1].travel[others]).all() and same_rays(last.escape[others][base[0].kind[others] == WALKING],
                                                                                      base[-1].escape[others][base[0].kind[others] == WALKING]).all()

    # inside hits of garbage kind are read as a miss: a step on the sentinel records makes every walking record Infinite
    hits_t, rays_t = dev(hits), dev(rays)
    rays_s, kind, travel, casts, flags = rt.refract_enter(scene, hits_t, rays_t)
    before = u32(rays_s).copy()
    garbage = torch.full((65, 13), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    escape = rt.refract_step(scene, hits_t, garbage, rays_s, kind, travel, casts, flags, 100.0)
    torch.cuda.synchronize()
    k = u32(kind)
    assert (k[walking] == INFINITE).all() and (k[base[0].kind != WALKING] == base[0].kind[base[0].kind != WALKING]).all()
    assert (u32(casts)[walking] == 1).all() and (host(flags) == 0).all() and (u32(escape) == 0).all()
    assert np.array_equal(u32(rays_s), before) and (host(travel).view(np.uint32) == 0).all()
    # an empty batch: RT_OK, nothing launched
    assert len(rt.refract_rays_by_bounce(scene, hits_t[:0], rays_t[:0])) == 0
    torch.cuda.synchronize()


def test_a_bounce_limit_of_three_rounds(ref):
    """4. rounds=3 leaves exactly the replay's unfinished records WALKING, and eight more rounds on the same state end equal to the
    full loop"""
    torch_device()
    scene = rt.Scene(ref.world)
    states, why = ref.runs[100.0]
    hits_t, rays_t = dev(ref.hits), dev(ref.rays)
    got3, (out, ws) = by_bounce(scene, hits_t, rays_t, 100.0, rounds=3)
    after3 = states[3]
    assert np.array_equal(got3[0], after3.kind) and (after3.kind == WALKING).sum() > 0
    assert np.array_equal(host(ws.flags) != 0, after3.kind == WALKING)
    walking = after3.kind == WALKING
    assert same_f32(got3[1][walking], after3.travel[walking]).all()  # the running sum is kept for the walks that go on
    assert (got3[1][~walking & (after3.kind != ESCAPED)].view(np.uint32) == 0).all()
    assert got3[3] == int(after3.casts.sum()) and np.array_equal(u32(ws.casts), after3.casts) and same_rays(u32(ws.rays), after3.rays).all()
    got8, _ = by_bounce(scene, hits_t, rays_t, 100.0, rounds=8, out=out, workspace=ws, resume=True)
    want = final(states)
    assert_refractions((got8[0], got8[1], got8[2], got3[3] + got8[3]), want, "three rounds and eight more")
    assert np.array_equal(u32(ws.casts), states[-1].casts)


def test_a_scene_walked_breadth_first(tmp_path):
    """5. the 9 244-triangle scene of tests/test_gpu_hit_queries.py, created under the breadth-first switch: the casts of the loop go
    through rt_cast_rays_indexed and take that walk; rt_refract_rays' do not.  Same bits, same count"""
    torch_device()
    big, cam = tessellated_scene(tmp_path, 4)
    desc = big.desc()
    assert desc.n_triangles == 36 * 4 ** 4 + 28  # above rt_scene_create's default switch (8 192 triangles)
    with rt.options(RT_AMD_BFS_WALK_TRIANGLES=8192):  # read when the scene is created
        scene = rt.Scene(big)
    rays = np.concatenate([camera_rays_cpu(cam, 24, 18), source_b(desc, 51, 300), source_c(desc, 3, 40)])
    hits = oracle_hits(desc, rays)
    states, why = replay(desc, rays, hits, 100.0)
    want = final(states)
    assert (states[0].kind == WALKING).sum() >= 100 and want[3] > 150 and (states[-1].casts >= 2).sum() > 0
    hits_t, rays_t = dev(hits), dev(rays)
    assert_refractions(fused(scene, hits_t, rays_t, 100.0), want, "9 244 triangles: rt_refract_rays")
    # the first uncaptured call on the stream makes the record lists of the walk; the second finds them
    for call in range(2):
        assert_refractions(by_bounce(scene, hits_t, rays_t, 100.0)[0], want, f"9 244 triangles: the loop, call {call}")


@pytest.mark.parametrize("per_ray", [False, True])
@pytest.mark.parametrize("depth", [0, 1, 5])
def test_the_tree_loop_with_every_cast_opened(depth, per_ray):
    """6. trace_rays_levels(open_casts=True) == trace_rays, values and cast count, on a 64 x 48 camera frame"""
    torch = torch_device()
    world = rt.reference_world()
    scene = rt.Scene(world)
    rays_t = rt.camera_rays(rt.reference_camera(), rt.Frame.full(64, 48, depth))
    n = rays_t.shape[0]
    if per_ray:
        g = np.random.default_rng(9)
        contribution = torch.tensor(g.choice([1.0, 0.5, 0.02, 0.0005], n).astype(np.float32), device="cuda")
    else:
        contribution = 1.0
    cnt_a, cnt_b = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
    if per_ray:  # trace_rays takes one contribution per call
        want = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
        for value in contribution.unique().tolist():
            rows = (contribution == value).nonzero().flatten()
            want[rows] = rt.trace_rays(scene, rays_t[rows].contiguous(), depth, value, ray_count=cnt_a)
    else:
        want = rt.trace_rays(scene, rays_t, depth, ray_count=cnt_a)
    out = torch.full((n, 3), 7.0, dtype=torch.float32, device="cuda")
    overflow = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        rt.trace_rays_levels(scene, rays_t, depth, contribution, out=out, ray_count=cnt_b, level_capacity=lambda level: 2 * n, check=False,
                             overflow=overflow, open_casts=True)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    assert int(host(overflow)[0]) == 0
    bad = np.flatnonzero(~same_f32(host(out), host(want)).all(axis=1))
    assert bad.size == 0, f"depth {depth}: {bad.size} of {n} differ, first {bad[:5]}: {host(out)[bad[:2]]} want {host(want)[bad[:2]]}"
    assert int(host(cnt_b)[0]) == int(host(cnt_a)[0]) > 0, (depth, int(host(cnt_b)[0]), int(host(cnt_a)[0]))


def test_the_level_loop_with_every_cast_opened():
    """7. trace_rays_distributed_levels(open_casts=True) == trace_rays_distributed over two epochs: samples, flags, accumulated image,
    cast count and the downloaded generator records"""
    torch = torch_device()
    world = rt.reference_world()
    scene = rt.Scene(world)
    rays_t = rt.camera_rays(rt.reference_camera(), rt.Frame.full(64, 48, 5))
    n = rays_t.shape[0]
    runs = []
    for opened in (None, True):
        rng, _ = sq.seeded(n)
        samples = torch.full((2, n, 3), 7.0, dtype=torch.float32, device="cuda")
        valid = torch.full((2, n), 9, dtype=torch.uint8, device="cuda")
        accum = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
        cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        if opened is None:
            rt.trace_rays_distributed(scene, rays_t, 5, rng, 2, accum=accum, samples=samples, valid=valid, ray_count=cnt)
        else:
            mode = torch.cuda.get_sync_debug_mode()
            torch.cuda.set_sync_debug_mode("error")
            try:
                rt.trace_rays_distributed_levels(scene, rays_t, 5, rng, 2, accum=accum, samples=samples, valid=valid, ray_count=cnt, open_casts=True)
            finally:
                torch.cuda.set_sync_debug_mode(mode)
        torch.cuda.synchronize()
        runs.append((host(samples), host(valid), host(accum), int(host(cnt)[0]), rng.download()))
        rng.close()
    want, got = runs
    bad = np.flatnonzero(~same_f32(got[0], want[0]).all(axis=2).all(axis=0))
    assert bad.size == 0, f"{bad.size} rays' samples differ, first {bad[:5]}: {got[0][:, bad[:2]]} want {want[0][:, bad[:2]]}"
    assert np.array_equal(got[1], want[1]) and same_f32(got[2], want[2]).all()
    assert got[3] == want[3] > 2 * n, (got[3], want[3])
    assert np.array_equal(got[4], want[4])


def test_the_loop_in_a_graph(ref):
    """8. after one uncaptured call (rt_select_records' scratch on that stream) the loop is captured on a stream of its own, with its
    cast count, under a sync-debug mode that makes any host visit an error, and replayed twice with the same result"""
    torch = torch_device()
    scene = rt.Scene(ref.world)
    states, why = ref.runs[100.0]
    n = ref.n
    want = final(states)
    hits_t, rays_t = dev(ref.hits), dev(ref.rays)
    out, ws = sentinel_out(n), rt.refract_workspace(n, "cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    mode = torch.cuda.get_sync_debug_mode()

    def run():
        torch.cuda.set_sync_debug_mode("error")
        try:
            rt.refract_rays_by_bounce(scene, hits_t, rays_t, 100.0, ray_count=cnt, stream=stream, out=out, workspace=ws)
        finally:
            torch.cuda.set_sync_debug_mode(mode)

    def result():
        return u32(out.kind), host(out.travel), u32(out.rays), int(host(cnt)[0])

    with torch.cuda.stream(stream):
        run()  # uncaptured: the selection's scratch of this stream
        stream.synchronize()
        assert_refractions(result(), want, "uncaptured")
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            run()
    torch.cuda.synchronize()
    for replay_no in range(2):
        out.kind.fill_(0x5A5A5A5A)
        out.travel.fill_(99.0)
        out.rays.fill_(0x5A5A5A5A)
        ws.casts.fill_(77)
        cnt.zero_()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert_refractions(result(), want, f"replay {replay_no}")
        assert np.array_equal(u32(ws.casts), states[-1].casts)
