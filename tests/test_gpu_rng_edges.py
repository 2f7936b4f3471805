"""The generator's three device copies (csrc/rt_rng.h in rt_scatter_query.hip, rt_distributed_rays.hip and rt_distributed.hip) on
crafted records: generators uploaded at chosen positions with chosen words waiting (tests/_rng_support.py), so that the block
boundary, the straddle of next_u64, the switch points of next_u32x3 and standard_normal_x2, every branch of the ziggurat and every
regime of isaac_generate_staged are met on purpose.  After every call the outputs AND the downloaded records are compared with the
oracle's bit for bit, and with the restatement where it gives exact bits.  Generator g of a batch gets case g mod n_cases, so that
neighbouring lanes diverge.  Every crafted record is a valid state: position <= 256."""
import numpy as np
import pytest

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import _capi
import _oracle
import _rng_support as S
from _records import camera_rays_cpu, dev, oracle_hits, same_f32, same_rays, torch_device
from _scatter_support import restate_level

pytestmark = pytest.mark.gpu

FRAME = rt.Frame.full(13, 10, 3)  # 130 generators: two waves and two lanes
N = 130
NORMAL_POSITIONS = (0, 249, 250, 251, 252, 253, 254, 255, 256)
ACCEPT = S.CASES[0].words  # a plain accept: two words


@pytest.fixture(scope="module")
def ref():
    world = rt.reference_world()
    return world.desc(), rt.Scene(world), rt.reference_camera()


@pytest.fixture(scope="module")
def base():
    """the frame's generators with their first block generated; never written to"""
    b = np.stack([S.generated(r) for r in _oracle.rng_init(FRAME)])
    b.setflags(write=False)
    return b


@pytest.fixture(scope="module")
def hit_batch(ref):
    """130 camera rays of the reference scene that hit, with the oracle's hits"""
    desc, _, cam = ref
    rays = camera_rays_cpu(cam, 40, 30)
    hits = oracle_hits(desc, rays)
    rows = np.flatnonzero(hits[:, 0] <= 1)[::3][:N]
    assert rows.size == N
    return np.ascontiguousarray(rays[rows]), np.ascontiguousarray(hits[rows])


def split(on):
    _capi.amd_lib().rt_set_distributed_split(on)


@pytest.fixture(autouse=True)
def default_organisation():
    yield
    split(-1)


def normal_records(base, shift, slot):
    """generator g: case g mod n_cases at position NORMAL_POSITIONS[(g / n_cases + shift) mod 9], the case's words as the first (slot
    0) or — behind a plain accept — the second (slot 1) normal of the pair"""
    n_cases = len(S.CASES)
    recs = []
    for g in range(N):
        words = S.CASES[g % n_cases].words
        recs.append(S.craft(base[g], NORMAL_POSITIONS[(g // n_cases + shift) % len(NORMAL_POSITIONS)], words if slot == 0 else ACCEPT + words))
    return np.stack(recs)


# ---- next_u32x3 in rt_scatter_query.hip ----

@pytest.mark.parametrize("prepare", [0, 1])
def test_next_u32x3_at_every_switch_position(ref, base, hit_batch, prepare):
    """rt_scatter_hits draws a level's three words with next_u32x3: positions 0, 252, 253 (the last with three loads in one go), 254,
    255 and 256 (word by word across the refill), the refill in the kernel or by the prepare pass (RT_AMD_SCATTER_PREPARE).  Kinds,
    directions, cosines and records against restate_level, which draws with orc_rng_draw_u32; the words drawn against the
    restatement's reader."""
    torch = torch_device()
    desc, scene, _ = ref
    rays, hits = hit_batch
    positions = (0, 252, 253, 254, 255, 256)
    words = [0x01234567, 0x89ABCDEF, 0x7F00FF00]
    states = np.stack([S.craft(base[g], positions[g % 6], [w ^ (g * 0x01010101 & S.M32) for w in words]) for g in range(N)])
    mine = states.copy()
    for rec in mine:
        for _ in range(3):
            S.next_u32(rec)
    rng = rt.Rng(FRAME)
    rng.upload(states)
    assert np.array_equal(rng.download(), states)
    with rt.options(RT_AMD_SCATTER_PREPARE=prepare):
        sc = rt.scatter_hits(scene, dev(hits), dev(rays), rng)
        torch.cuda.synchronize()
    kind, new_dir, cosine = restate_level(desc, rays, hits, states)  # advances `states` with the oracle
    assert np.array_equal(states, mine)
    assert (states[:, S.INDEX] == [(p + 3) if p + 3 <= 256 else p + 3 - 256 for p in [positions[g % 6] for g in range(N)]]).all()
    after = rng.download()
    bad = np.flatnonzero((after != states).any(axis=1))
    assert bad.size == 0, f"records differ at generators {bad[:6]} (positions {[positions[g % 6] for g in bad[:6]]})"
    assert np.array_equal(sc.type.cpu().numpy().view(np.uint32), kind)
    want = rays.copy()
    want[:, 3:6] = new_dir.view(np.uint32)
    assert same_rays(sc.rays.cpu().numpy(), want).all()
    assert same_f32(sc.cosine.cpu().numpy(), cosine).all()
    rng.close()


# ---- standard_normal_x2 without LDS in rt_distributed_rays.hip ----

@pytest.mark.parametrize("slot", [0, 1])
@pytest.mark.parametrize("shift", range(len(NORMAL_POSITIONS)))
def test_standard_normal_x2_through_focus_rays(ref, base, shift, slot):
    """rt_focus_rays draws a pixel's two lens normals with standard_normal_x2: every crafted ziggurat case as the first or the second
    normal of the pair, at positions 0 and 249 .. 256 — four loads in one go with both accepting (<= 252), the first accepting and
    the second not (redo both from the same position), the word-by-word form (253 .. 256), a straddle inside a tail's loop.  The rays
    against shoot_focus in numpy binary32 (_rng_support.focus_rays_cpu) on the oracle's normals, the records against the oracle's, the
    normals against the restatement: the same bits where the value is u X[i], within tail_bound in the tail."""
    torch = torch_device()
    _, _, cam = ref
    states = normal_records(base, shift, slot)
    rng = rt.Rng(FRAME)
    rng.upload(states)
    rays = rt.focus_rays(cam, FRAME, rng, 3.0, 0.04)
    torch.cuda.synchronize()
    mine = states.copy()
    normals = np.stack([S.oracle_normal(rec, 2) for rec in states])
    paths = set()
    for g, rec in enumerate(mine):
        for k in range(2):
            d = S.ziggurat(rec)
            assert min(d.margins) >= S.MARGIN
            paths.add(d.branch)
            if d.exact:
                assert normals[g, k] == S.to_f64(d.value), (g, k)
            else:
                assert abs(S.MP.mpf(float(normals[g, k])) - d.value) <= S.tail_bound(d), (g, k)
    assert np.array_equal(mine, states)
    assert paths == {"accept", "tail", "wedge-accept"}
    after = rng.download()
    bad = np.flatnonzero((after != states).any(axis=1))
    assert bad.size == 0, f"records differ at generators {bad[:6]}"
    want = S.focus_rays_cpu(cam, FRAME, 3.0, 0.04, normals)
    bad = np.flatnonzero(~same_rays(rays.cpu().numpy(), want))
    assert bad.size == 0, f"rays differ at generators {bad[:6]}: {rays.cpu().numpy().view(np.uint32)[bad[:1]]} want {want[bad[:1]]}"
    rng.close()


# ---- standard_normal (fused) and standard_normal_x2 + next_u32x3 with LDS staging (chain) in rt_distributed.hip ----

def render(scene, cam, rng, epochs=2):
    torch = torch_device()
    samples = torch.empty((epochs, FRAME.rows, FRAME.cols, 3), dtype=torch.float32, device="cuda")
    valid = torch.empty((epochs, FRAME.rows, FRAME.cols), dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    rt.render_distributed(scene, cam, FRAME, rng, epochs, samples=samples, valid=valid, ray_count=cnt)
    torch.cuda.synchronize()
    return samples.cpu().numpy(), valid.cpu().numpy(), int(cnt.item())


def assert_render_equals_oracle(ref, rng, states, what):
    """two epochs of rt_render_distributed on `rng` against orc_render_distributed started from `states` (which it advances)"""
    desc, scene, cam = ref
    s, v, c = render(scene, cam, rng)
    ws, wv, wc = _oracle.render_distributed(desc, cam, FRAME, states, 2)
    bad = np.argwhere(~same_f32(s, ws))
    assert bad.size == 0, f"{what}: samples differ, first at (epoch, row, col, channel) {bad[:3].tolist()}"
    assert np.array_equal(v, wv) and c == wc, what
    after = rng.download()
    bad = np.flatnonzero((after != states).any(axis=1))
    assert bad.size == 0, f"{what}: records differ at generators {bad[:6]}"


@pytest.mark.parametrize("lookahead", [0, 1])
@pytest.mark.parametrize("organisation", [1, 0], ids=["split", "fused"])
def test_render_distributed_on_crafted_records(ref, base, organisation, lookahead):
    """a 13 x 10 frame, depth 3, two epochs, from records crafted as for rt_focus_rays (every case, both slots, positions spread over
    the lanes): samples, flags, casts and records against the oracle started from the same records"""
    split(organisation)
    with rt.options(RT_AMD_RNG_LOOKAHEAD=lookahead):
        for shift, slot in ((0, 0), (5, 1), (3, 1), (7, 0)):
            states = normal_records(base, shift, slot)
            rng = rt.Rng(FRAME)
            rng.upload(states)
            assert_render_equals_oracle(ref, rng, states, (shift, slot))
            rng.close()


@pytest.mark.parametrize("position", [256, 255])
@pytest.mark.parametrize("arrangement", ["contiguous", "spread"])
@pytest.mark.parametrize("k", [1, 8, 9, 16, 17, 64])
def test_refill_regimes_of_the_chain_kernel(ref, base, k, arrangement, position):
    """isaac_generate_staged by how many lanes of a wave run dry together: 1 .. 8 through LDS in its first pass, 9 .. 16 in a second
    pass over the same slots, more than 16 in HBM.  Look-ahead off, the split organisation without the cost order.

    Which lanes: dist_chain_kernel hands out 64-slot chunks of the frame, one chunk to one wave; on a wave's first visit all its
    lanes are idle, so lane l takes slot 64 chunk + l, and a slot is a pixel as _rng_support.chain_chunks restates (8-row bands,
    column by column).  All lanes of a wave then enter start_epoch together and the dry ones meet in the refill of its first normal:
    in each full chunk exactly k generators are at `position` — 256: used up, nothing prepared; 255: one word left, the refill
    inside next_u64 — and the others at position 0 of a generated block, far from needing one (two epochs at depth 3 use at most 26
    words).  The 13 x 10 frame has two full chunks and a last one of two pixels, where min(k, 2) are dry.  The count is what the
    ballot in isaac_generate_staged sees as long as the compiler keeps the lanes of one call site together; nothing here reads it
    back, so a different grouping would still have to give the oracle's samples and records."""
    split(1)
    states = np.stack([S.craft(base[g], 0, []) for g in range(N)])
    chunks = S.chain_chunks(FRAME.cols, FRAME.rows)
    assert [len(c) for c in chunks] == [64, 64, 2] and sorted(p for c in chunks for p in c) == list(range(N))
    for chunk in chunks:
        n, kk = len(chunk), min(k, len(chunk))
        lanes = [(5 + j) % n for j in range(kk)] if arrangement == "contiguous" else [((j * n) // kk + 3) % n for j in range(kk)]
        assert len(set(lanes)) == kk
        for lane in lanes:
            states[chunk[lane]] = S.craft(base[chunk[lane]], position, [0xDEADBEEF])
    assert ((states[:, S.INDEX] == position).sum(), (states[:, S.INDEX] == 0).sum()) == (2 * k + min(k, 2), N - 2 * k - min(k, 2))
    with rt.options(RT_AMD_RNG_LOOKAHEAD=0, RT_AMD_DIST_BY_COST=0):
        rng = rt.Rng(FRAME)
        rng.upload(states)
        assert_render_equals_oracle(ref, rng, states, (k, arrangement, position))
        rng.close()


@pytest.mark.parametrize("organisation", [1, 0], ids=["split", "fused"])
def test_upload_drops_the_prepared_bank(ref, organisation):
    """with the look-ahead on, a render leaves every generator's next block prepared in its other bank.  An upload must forget it:
    the records go back rotated by one generator and put at positions 255 / 256, so the very next draw refills — and must generate
    from the uploaded mem, not switch to the bank prepared for the generator that was there before"""
    split(organisation)
    desc, scene, cam = ref
    with rt.options(RT_AMD_RNG_LOOKAHEAD=1):
        rng = rt.Rng(FRAME)
        states = _oracle.rng_init(FRAME)
        assert_render_equals_oracle(ref, rng, states, "first render")
        got = rng.download()
        rotated = np.roll(got, 1, axis=0)
        crafted = np.stack([S.craft(rotated[g], 255 + (g & 1), [0x0F0F0F0F]) for g in range(N)])
        rng.upload(crafted)
        assert np.array_equal(rng.download(), crafted)
        assert_render_equals_oracle(ref, rng, crafted, "after the upload")
        rng.close()
