"""Record ordering on the device (include/rt_amd.h rt_ray_keys, rt_sort_records, rt_gather_records, rt_scatter_records): the keys against
the numpy restatement of tests/test_order_query_abi.py bit for bit, the sort against numpy's stable argsort on every list a caller may
hold, in place, twice, between sentinels and from a captured graph, gather and scatter against numpy fancy indexing, and the two
compositions rt.cast_rays_ordered / rt.trace_rays_ordered against rt.cast_rays / rt.trace_rays bit for bit (NaN distances included),
also under torch's synchronisation check.  Floats are compared as bit patterns."""
import numpy as np
import pytest

import homework_18_graphics_raytracer_amd as rt
import _order_support as oq
from _records import dev, host, ray_records, source_b, torch_device, u32

pytestmark = pytest.mark.gpu
F32 = np.float32
SENTINEL = 0x5A5A5A5A


def words(a):
    """a uint32 array as an int32 CUDA tensor"""
    return torch_device().tensor(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32), device="cuda")


@pytest.fixture(scope="module")
def ref():
    world = rt.reference_world()
    return world, world.desc(), rt.Scene(world), world.bounds()


# ---- keys ----

def _special_rays():
    nan, inf = np.nan, np.inf
    o = [(0, 0, 0)] * 12 + [(inf, -inf, nan), (nan, 0, inf), (-inf, inf, 0), (9, -9, 1e30), (-1e-30, 2.0, -2.0), (1.999, -1.999, 0.5)]
    d = [(0, 0, 0), (1, 1, 0.0), (1, 1, -0.0), (1, -1, nan), (nan, 1, -1), (1, nan, -1), (0, 0, -1), (-0.0, -0.0, -1), (inf, 1, 1),
         (1, 2, -inf), (1e-30, -1e-30, -1e-30), (-3, 4, -5)] + [(0.3, -0.2, -0.9)] * 6
    return ray_records(np.asarray(o, dtype=F32), np.asarray(d, dtype=F32), 0xABCDEF)


BOXES = [((-2, -2, -2), (2, 2, 2)), ((0, 0, 0), (0, -1, np.nan)), ((np.nan, -np.inf, -1), (1, np.inf, -1)), ((-1, -1, -1), (np.inf, 1e-30, 1))]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_keys_equal_the_numpy_restatement(ref, n):
    torch = torch_device()
    _, desc, _, (lo, hi) = ref
    camera = u32(rt.camera_rays(rt.reference_camera(), rt.Frame.full(64, 32, 0)))
    special = _special_rays()
    sources = {"random": source_b(desc, 100 + n, n), "camera": np.resize(camera, (n, 11)), "special": np.resize(special, (n, 11))}
    for name, rays in sources.items():
        rays_t = dev(rays)
        for box in [(lo, hi)] + (BOXES if name == "special" else []):
            for flags in (0, rt.ORDER_DIRECTION_MAJOR):
                out = torch.full((n + 1,), SENTINEL, dtype=torch.int32, device="cuda")
                rt.ray_keys(rays_t, box[0], box[1], flags, out=out[:n])
                got = u32(out)
                want = oq.numpy_keys(rays, box[0], box[1], flags)
                bad = np.flatnonzero(got[:n] != want)
                assert bad.size == 0, (name, box, flags, bad[:4], got[bad[:4]], want[bad[:4]], rays[bad[:2]])
                assert got[n] == SENTINEL


# ---- sort ----

BITS = [(0, 1), (0, 8), (0, 9), (7, 10), (12, 18), (0, 30), (0, 32), (31, 1)]


def _key_sets(n, g, only=None):
    four = np.asarray([0x00000000, 0x80000001, 0x3FF00F80, 0xFFFFFFFF], dtype=np.uint32)
    make = {
        "all equal": lambda: np.full(n, 0xA5A5A5A5, dtype=np.uint32),
        "ascending": lambda: (np.arange(n, dtype=np.uint64) * 4099 % (1 << 32)).astype(np.uint32) if n < 1000 else np.sort(g.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)),
        "descending": lambda: np.sort(g.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32))[::-1].copy(),
        "random": lambda: g.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32),
        "four values": lambda: four[g.integers(0, 4, n)],
    }
    return {name: fn() for name, fn in make.items() if only is None or name in only}


def _expected(keys, n, first, bits, index, m):
    idx = np.asarray(index[:m], dtype=np.uint32).astype(np.int64)
    valid = idx < n
    field = (keys[idx[valid]].astype(np.uint64) >> first) & ((1 << bits) - 1)
    if bits <= 16 or field.size < (1 << 20):
        order = np.argsort(field.astype(np.uint8 if bits <= 8 else np.uint16 if bits <= 16 else np.uint32), kind="stable")
    else:  # the same order from two stable argsorts of 16-bit halves, low then high: numpy sorts those several times faster
        low = np.argsort((field & 0xFFFF).astype(np.uint16), kind="stable")
        order = low[np.argsort((field[low] >> 16).astype(np.uint16), kind="stable")]
    return np.concatenate([idx[valid][order], idx[~valid]]).astype(np.uint32)


class _Sorter:
    """device buffers for lists of capacity n, with a sentinel word behind the output and behind the workspace"""

    def __init__(self, n, torch):
        self.n, self.torch = n, torch
        self.bytes = rt.sort_temp_bytes(n)
        assert self.bytes % 4 == 0
        self.out = torch.empty((n + 1,), dtype=torch.int32, device="cuda")
        self.temp = torch.empty((self.bytes + 4,), dtype=torch.uint8, device="cuda")

    def run(self, keys_t, first, bits, index_t=None, count_t=None, in_place=False):
        n = self.n
        self.out.fill_(SENTINEL)
        self.temp[self.bytes:].fill_(0x5A)
        out = index_t if in_place else self.out[:n]
        got = rt.sort_records(keys_t, first, bits, index=index_t, count=count_t, out=out, temp=self.temp[:self.bytes])
        assert got is out
        res = u32(out).copy()
        assert u32(self.out)[n] == SENTINEL and (host(self.temp[self.bytes:]) == 0x5A).all()
        return res


def _lists(n, g, torch):
    """(label, index array or None, count or None): what a caller may hold"""
    flags = (g.random(n) < 0.6).astype(np.uint8)
    sel_index, sel_count = rt.select_records(torch.tensor(flags, device="cuda"))
    perm = g.permutation(n).astype(np.uint32)
    wild = perm.copy()
    wild[::3] = (n + g.integers(0, 1000, wild[::3].size)).astype(np.uint32)  # entries >= n: last, in input order, values kept
    wild[-1] = 0xFFFFFFFF
    repeated = g.integers(0, max(n // 2, 1), n).astype(np.uint32)
    out = [("selected", sel_index, sel_count, int(flags.sum())), ("count 0", words(perm), words([0]), 0),
           ("count above n", words(perm), words([n + 12345]), n), ("count 2^32-1", words(perm), words([0xFFFFFFFF]), n),
           ("entries >= n", words(wild), None, n), ("repeated entries", words(repeated), words([max(n - 1, 0)]), max(n - 1, 0)),
           ("permuted, in place", words(perm), None, n)]
    return out


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 4097, 65537, (1 << 20) + 37])
def test_sort_against_numpy_stable_argsort(n):
    torch = torch_device()
    g = np.random.default_rng(n)
    sorter = _Sorter(n, torch)
    lists = _lists(n, g, torch)
    identity = np.arange(n, dtype=np.uint32)
    combo = 0
    for name, keys in _key_sets(n, g).items():
        keys_t = words(keys)
        for first, bits in BITS:
            what = (n, name, first, bits)
            got = sorter.run(keys_t, first, bits)
            want = _expected(keys, n, first, bits, identity, n)
            assert np.array_equal(got, want), (what, "identity", np.flatnonzero(got != want)[:5])
            if combo % 8 == 0:
                assert np.array_equal(sorter.run(keys_t, first, bits), got), (what, "twice")
            # ... and one of the caller's lists, in turn, so that every list meets several key sets and bit ranges
            label, index_t, count_t, m = lists[(combo + combo // len(BITS)) % len(lists)]
            combo += 1
            index = u32(index_t).copy()
            want = _expected(keys, n, first, bits, index, m)
            in_place = label.endswith("in place")
            work_t = index_t.clone() if in_place else index_t
            got = sorter.run(keys_t, first, bits, work_t, count_t, in_place=in_place)
            assert np.array_equal(got[:m], want), (what, label, m, np.flatnonzero(got[:m] != want)[:5])
            if not in_place:
                assert np.array_equal(u32(index_t), index), (what, label, "the input list is only read")
    seen = {lists[(c + c // len(BITS)) % len(lists)][0] for c in range(combo)}
    assert len(seen) == len(lists)


LARGE_KEYS = ("random", "four values", "all equal")
LARGE_BITS = [(0, 8), (0, 9), (0, 32)]


@pytest.mark.parametrize("n", list(oq.SORT_LARGE))
def test_sort_of_more_than_2_to_the_21_entries(n):
    """capacities at which a tile of sort_scatter_kernel is more than one 2048-entry step (a bucket's position carried from step to step,
    the waves' counts zeroed again, a ragged last step that ends at a device-side count) and at which the scan takes the whole bucket
    table — what a 4K frame of rays gets.  Lists rotate over key sets and bit ranges; every one of each is met."""
    import time

    torch = torch_device()
    t0 = time.perf_counter()
    tile, tiles = oq.sort_tile(n)
    assert (tile, tiles) == oq.SORT_LARGE[n]  # a change of the constants fails here instead of moving the test off the path
    g = np.random.default_rng(n)
    sorter = _Sorter(n, torch)
    perm = g.permutation(n).astype(np.uint32)
    wild = perm.copy()
    wild[::3] = (n + g.integers(0, 1000, wild[::3].size)).astype(np.uint32)  # the 257th bucket in every step: last, in input order
    lists = [("identity", None, None, n), ("entries >= n", words(wild), None, n), ("permuted, in place", words(perm), None, n)]
    if tile > oq.SORT_STEP:
        m = 5 * tile + oq.SORT_STEP + 5  # ends five entries into the second step of the sixth tile
        assert m < n and (m % tile) // oq.SORT_STEP == 1 and m % oq.SORT_STEP == 5
        lists.insert(2, ("count inside a later step", words(perm), words([m]), m))
    identity = np.arange(n, dtype=np.uint32)
    combo, seen = 0, set()
    for name, keys in _key_sets(n, g, only=LARGE_KEYS).items():
        keys_t = words(keys)
        for first, bits in LARGE_BITS:
            label, index_t, count_t, m = lists[(combo + combo // len(lists)) % len(lists)]
            what = (n, name, first, bits, label)
            seen |= {name, (first, bits), label}
            index = identity if index_t is None else u32(index_t).copy()
            want = _expected(keys, n, first, bits, index, m)
            in_place = label.endswith("in place")
            work_t = index_t.clone() if in_place else index_t
            got = sorter.run(keys_t, first, bits, work_t, count_t, in_place=in_place)
            assert np.array_equal(got[:m], want), (what, m, np.flatnonzero(got[:m] != want)[:5])
            if index_t is not None and not in_place:
                assert np.array_equal(u32(index_t), index), (what, "the input list is only read")
            if combo == 1:  # once per capacity: the same call again gives the same array
                assert np.array_equal(sorter.run(keys_t, first, bits, work_t, count_t, in_place=in_place)[:m], got[:m]), (what, "twice")
            combo += 1
    assert seen == set(LARGE_KEYS) | set(LARGE_BITS) | {entry[0] for entry in lists}, seen
    print(f"sort n={n} tile={tile} tiles={tiles}: {combo} sorts against numpy in {time.perf_counter() - t0:.2f} s")


def test_sort_keeps_equal_keys_in_input_order_and_groups_a_level_by_branch():
    """rt_scatter_hits' d_type with key_bits = 2: the records of each branch stay in their order"""
    torch = torch_device()
    g = np.random.default_rng(7)
    n = 10_000
    types = g.integers(0, 3, n).astype(np.uint32)
    got = u32(rt.sort_records(words(types), 0, 2))
    want = np.concatenate([np.flatnonzero(types == t) for t in range(3)]).astype(np.uint32)
    assert np.array_equal(got, want)


def test_sort_captured_into_a_graph_without_an_earlier_call():
    torch = torch_device()
    g = np.random.default_rng(9)
    n = 5000
    keys = g.integers(0, 1 << 30, n, dtype=np.uint64).astype(np.uint32)
    keys_t, index_t, count_t = words(keys), words(np.arange(n)), words([n])
    out = torch.zeros(n, dtype=torch.int32, device="cuda")
    temp = torch.empty(rt.sort_temp_bytes(n), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):  # the first call on this stream: nothing is allocated, nothing read back
            rt.sort_records(keys_t, 0, 30, index=index_t, count=count_t, out=out, temp=temp)
    torch.cuda.synchronize()

    def replay(keys, index, m):
        keys_t.copy_(words(keys))
        index_t.copy_(words(index))
        count_t.copy_(words([m]))
        out.fill_(-1)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        plain = u32(rt.sort_records(keys_t, 0, 30, index=index_t, count=count_t))
        torch.cuda.synchronize()
        want = _expected(keys, n, 0, 30, index, m)
        assert np.array_equal(u32(out)[:m], want) and np.array_equal(plain[:m], want), m

    replay(keys, np.arange(n), n)
    replay(g.integers(0, 1 << 30, n, dtype=np.uint64).astype(np.uint32), np.arange(n), n)            # new keys
    replay(keys, np.where(g.random(n) < 0.1, n + 5, g.permutation(n)).astype(np.uint32), n - 1234)  # a new list and count


# ---- gather and scatter ----

@pytest.mark.parametrize("record_bytes", [4, 12, 44, 52, 256])
@pytest.mark.parametrize("n", [1, 65, 4097])
def test_gather_and_scatter_against_fancy_indexing(n, record_bytes):
    torch = torch_device()
    g = np.random.default_rng(n * 1000 + record_bytes)
    w = record_bytes // 4
    src = g.integers(1, 1 << 32, (n, w), dtype=np.uint64).astype(np.uint32)
    src_t = words(src) if w > 1 else words(src.reshape(-1))
    shape = (lambda k: (k, w)) if w > 1 else (lambda k: (k,))
    m = n + 7  # a list longer than the array: repeats and entries >= n
    index = g.integers(0, n, m).astype(np.uint32)
    index[g.random(m) < 0.2] = n + g.integers(0, 5)
    index[0] = 0xFFFFFFFF if n > 1 else 0
    for count in (None, m, m // 2, 0, m + 100):
        live = m if count is None else min(count, m)
        count_t = None if count is None else words([count])
        out = torch.full(shape(m + 1), SENTINEL, dtype=torch.int32, device="cuda")
        rt.gather_records(src_t, words(index), count=count_t, out=out[:m])
        got = u32(out).reshape(m + 1, w)
        ok = index[:live] < n
        want = np.where(ok[:, None], src[np.where(ok, index[:live], 0)], 0)
        assert np.array_equal(got[:live], want), ("gather", count)
        assert (got[live:] == SENTINEL).all(), ("gather: nothing beyond the count", count)
    # scatter through a duplicate-free list with entries >= n: skipped; unnamed records stay
    perm = g.permutation(n).astype(np.uint32)
    sindex = np.concatenate([perm[: n // 2 + 1], np.asarray([n, n + 3, 0xFFFFFFFF], dtype=np.uint32)])
    g.shuffle(sindex)
    k = sindex.size
    data = g.integers(1, 1 << 32, (k, w), dtype=np.uint64).astype(np.uint32)
    data_t = words(data) if w > 1 else words(data.reshape(-1))
    for count in (None, k - 2, 0):
        live = k if count is None else count
        dst = torch.full(shape(n + 1), SENTINEL, dtype=torch.int32, device="cuda")
        rt.scatter_records(data_t, words(sindex), dst[:n], count=None if count is None else words([count]))
        want = np.full((n + 1, w), SENTINEL, dtype=np.uint32)
        ok = sindex[:live] < n
        want[sindex[:live][ok]] = data[:live][ok]
        assert np.array_equal(u32(dst).reshape(n + 1, w), want), ("scatter", count)
    # a repeated index: one of the sources wins, word by word, and nothing else is touched
    twice = np.zeros(64, dtype=np.uint32)
    many = g.integers(1, 1 << 32, (64, w), dtype=np.uint64).astype(np.uint32)
    dst = torch.full(shape(n + 1), SENTINEL, dtype=torch.int32, device="cuda")
    rt.scatter_records(words(many) if w > 1 else words(many.reshape(-1)), words(twice), dst[:n])
    got = u32(dst).reshape(n + 1, w)
    assert all(got[0, c] in many[:, c] for c in range(w)) and (got[1:] == SENTINEL).all()
    # scatter after gather through a permutation is the identity
    gathered = rt.gather_records(src_t, words(perm))
    back = torch.full(shape(n), SENTINEL, dtype=torch.int32, device="cuda")
    rt.scatter_records(gathered, words(perm), back)
    assert np.array_equal(u32(gathered).reshape(n, w), src[perm]) and np.array_equal(u32(back).reshape(n, w), src)


# ---- end to end ----

W, H = 160, 90


@pytest.fixture(scope="module")
def batch(ref):
    """about 20 000 rays: the camera rays of a 160 x 90 frame in a random permutation, then random rays; with what the plain calls give"""
    torch = torch_device()
    _, desc, scene, _ = ref
    g = np.random.default_rng(2024)
    perm = g.permutation(W * H)
    camera = u32(rt.camera_rays(rt.reference_camera(), rt.Frame.full(W, H, 3)))
    rays = np.concatenate([camera[perm], source_b(desc, 77, 20_000 - W * H)])
    rays_t = dev(rays)
    hits = u32(rt.cast_rays(scene, rays_t))
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    rgb = u32(rt.trace_rays(scene, rays_t, 3, ray_count=count))
    assert (hits[:, 0] == 0xFFFFFFFF).sum() > 0 and (hits[:, 0] != 0xFFFFFFFF).sum() > 0
    return perm, rays, rays_t, hits, rgb, int(host(count)[0])


def _guarded(fn, checked, torch):
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    if checked:
        torch.cuda.set_sync_debug_mode("error")  # any synchronising torch call inside raises
    try:
        out = fn()
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("checked", [False, True])
@pytest.mark.parametrize("which", ["reference", "breadth-first"])
def test_ordered_casts_equal_cast_rays(ref, batch, which, checked):
    torch = torch_device()
    world, _, scene, _ = ref
    _, rays, rays_t, hits, _, _ = batch
    if which == "breadth-first":
        with rt.options(RT_AMD_BFS_WALK_TRIANGLES=1):  # read when the scene is created
            scene = rt.Scene(world)
        assert np.array_equal(u32(rt.cast_rays(scene, rays_t)), hits)
    n = rays.shape[0]
    for flags in (0, rt.ORDER_DIRECTION_MAJOR):
        out = torch.full((n, 13), SENTINEL, dtype=torch.int32, device="cuda")
        casts = torch.zeros(1, dtype=torch.int64, device="cuda")
        workspace = rt.order_workspace(n, "cuda")
        _guarded(lambda: rt.cast_rays_ordered(scene, rays_t, flags=flags, out=out, ray_count=casts, workspace=workspace), checked, torch)
        got = u32(out)
        bad = np.flatnonzero((got != hits).any(axis=1))
        assert bad.size == 0, (which, flags, bad.size, bad[:5])  # bits, NaN distances included
        assert int(host(casts)[0]) == n
        assert np.array_equal(np.sort(u32(workspace.index)), np.arange(n, dtype=np.uint32))  # the list is a permutation
    got = _guarded(lambda: rt.cast_rays_ordered(scene, rays_t, box=((-1, -1, -1), (1, 1, 1))), checked, torch)  # a box and buffers of its own
    assert np.array_equal(u32(got), hits)


def test_ordered_casts_of_more_than_2_to_the_21_rays(ref, batch):
    """a batch whose sort takes tiles of two steps (a 4K frame's worth): the permuted camera rays over and over, then random rays"""
    torch = torch_device()
    _, desc, scene, _ = ref
    n = (1 << 21) + 4099
    assert oq.sort_tile(n) == (4096, 514)
    rays_t = dev(np.concatenate([np.resize(batch[1][:W * H], (1 << 21, 11)), source_b(desc, 78, 4099)]))
    assert rays_t.shape[0] == n
    hits = u32(rt.cast_rays(scene, rays_t))
    out = torch.full((n, 13), SENTINEL, dtype=torch.int32, device="cuda")
    workspace = rt.order_workspace(n, "cuda")
    rt.cast_rays_ordered(scene, rays_t, out=out, workspace=workspace)
    bad = np.flatnonzero((u32(out) != hits).any(axis=1))
    assert bad.size == 0, (bad.size, bad[:5])  # bits, NaN distances included
    assert (hits[:, 0] == 0xFFFFFFFF).sum() > 0 and (hits[:, 0] != 0xFFFFFFFF).sum() > 0
    assert np.array_equal(np.sort(u32(workspace.index)), np.arange(n, dtype=np.uint32))  # the list is a permutation


@pytest.mark.parametrize("checked", [False, True])
def test_ordered_traces_equal_trace_rays(ref, batch, checked):
    torch = torch_device()
    _, _, scene, _ = ref
    _, rays, rays_t, _, rgb, casts = batch
    n = rays.shape[0]
    for flags in (0, rt.ORDER_DIRECTION_MAJOR):
        out = torch.full((n, 3), 7.0, dtype=torch.float32, device="cuda")
        count = torch.zeros(1, dtype=torch.int64, device="cuda")
        _guarded(lambda: rt.trace_rays_ordered(scene, rays_t, 3, flags=flags, out=out, ray_count=count), checked, torch)
        bad = np.flatnonzero((u32(out) != rgb).any(axis=1))
        assert bad.size == 0, (flags, bad.size, bad[:5])
        assert int(host(count)[0]) == casts, (flags, int(host(count)[0]), casts)


def test_sorted_camera_rays_fill_a_wave_from_fewer_tiles(ref, batch):
    """a condition, not a measurement: after sort_records on their keys, 64 consecutive entries of the permuted 160 x 90 camera rays
    come from fewer distinct 8 x 8 pixel tiles, on average, than 64 consecutive pixels in row order (8 by construction) — the key
    as specified gives about 6.4 for this frame and camera (6.45 for one permutation, by the numpy restatement on the CPU)"""
    _, _, _, (lo, hi) = ref
    perm, rays, rays_t, _, _, _ = batch
    n = W * H
    camera_t = rays_t[:n].contiguous()

    def tiles_per_chunk(pixels):
        tile = (pixels // W // 8) * W + (pixels % W) // 8
        return float(np.mean([np.unique(tile[i:i + 64]).size for i in range(0, n, 64)]))

    keys = rt.ray_keys(camera_t, lo, hi)
    index = u32(rt.sort_records(keys, 0, 30))
    assert np.array_equal(index, np.argsort(oq.numpy_keys(rays[:n], lo, hi), kind="stable").astype(np.uint32))
    row_order, ordered, shuffled = tiles_per_chunk(np.arange(n)), tiles_per_chunk(perm[index]), tiles_per_chunk(perm)
    print(f"distinct 8x8 tiles per 64 entries: row order {row_order}, sorted {ordered}, permuted {shuffled}")
    assert row_order == 8.0
    assert ordered < row_order
