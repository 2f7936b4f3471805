"""The adaptive sampling queries on the device against the CPU definition, with no tolerance: the three list kernels at sizes around a
256-pixel step and beyond one round of the totals scan, with the grid capped so that a workgroup takes several steps; both forms of the
listed splat at the sizes where a tile can go wrong, at every reach; the two equalities with the existing film; a stream and a captured
graph whose first rt_sample_list call is the captured one; and render_pass on the reference scene.  A NaN that went through arithmetic
is compared as "a NaN"; the NaN offsets beyond a list are written as words and compared as words."""
import functools

import numpy as np
import pytest

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import adaptive, film, temporal
from _film_support import F32, case_data as film_case
from _records import torch_device
import _adaptive_support as S

pytestmark = pytest.mark.gpu

U32 = np.uint32
OPTION = "RT_AMD_DIAG_ADAPTIVE_MAX_GROUPS"
CAPS = [None, 1, 2]
FORMS = [0, 1]  # the plain and the tiled kernel
FILTER_OF = {0.5: "box", 1.0: "tent", 2.0: "mitchell", 3.0: "tent", 4.0: "mitchell"}


def dev(a):
    if a is None:
        return None
    a = np.array(a)
    return torch_device().from_numpy(a.view(np.int32) if a.dtype == U32 else a).cuda()


def host(t):
    torch_device().cuda.synchronize()
    a = t.cpu().numpy()
    return a.view(U32) if a.dtype == np.int32 else a


def capped(cap):
    return rt.options(**({OPTION: cap} if cap else {}))


def dev_list(sl):
    return adaptive.SampleList(dev(sl.start), dev(sl.pixel), dev(sl.sample), dev(sl.total), sl.capacity, sl.n)


def host_list(sl):
    return adaptive.SampleList(host(sl.start), host(sl.pixel), host(sl.sample), host(sl.total), sl.capacity, sl.n)


# ---- the budget ----

@pytest.mark.parametrize("cap", CAPS)
def test_budget_equals_the_cpu_definition(cap):
    torch = torch_device()
    for n in (1, 257, 4099):
        mean, variance, count, valid = S.budget_case(n)
        h = np.zeros(n, dtype=temporal.HISTORY_DTYPE)
        h["moment1"], h["length"] = mean, count
        d_h = dev(h.view(U32).reshape(n, 8))
        with capped(cap):
            for kw in (dict(gain=8.0, min_count=1, max_count=16), dict(gain=0.0, min_count=2, max_count=9), dict(gain=3.5, min_count=5, max_count=5)):
                want = adaptive.budget_numpy(mean, variance, count, valid, **kw)
                assert np.array_equal(host(adaptive.budget(dev(mean), dev(variance), dev(count), dev(valid), **kw)), want)
                got = adaptive.budget(d_h.view(torch.float32)[:, 3], dev(variance), d_h[:, 5], dev(valid), **kw)  # moment1 and length, stride 8
                assert np.array_equal(host(got), want)
                assert np.array_equal(host(adaptive.budget(dev(mean), dev(variance), **kw)), adaptive.budget_numpy(mean, variance, **kw))


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_budget_around_one_workgroup_of_elements_under_one_workgroup(n):
    """the element loop both libraries run: one element, a workgroup of them less one, exactly one, and one more that the only workgroup
    takes in its second stride"""
    mean, variance, count, valid = S.budget_case(n)
    kw = dict(gain=8.0, min_count=1, max_count=16)
    with capped(1):
        got = adaptive.budget(dev(mean), dev(variance), dev(count), dev(valid), **kw)
        assert np.array_equal(host(got), adaptive.budget_numpy(mean, variance, count, valid, **kw))


# ---- the list ----

@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("n", S.LIST_SIZES)
def test_list_equals_the_cpu_definition(n, cap):
    """'full': every workgroup step puts out its 16 384 records; 'single': 255 pixels of 0 and one of 64 in a step; capacities at the sum,
    one below, in the middle of a pixel and 0; first advanced.  Cap 1 and 2: a workgroup takes several steps"""
    for kind in ("zeros", "full", "single", "above", "random"):
        counts = S.counts_case(n, kind)
        asked = int(np.minimum(counts, 64).sum())
        for capacity in sorted({asked, max(asked - 1, 0), asked // 2 + 3, 0} if n <= 4099 else {asked, asked // 2 + 3}):
            first = (np.arange(n, dtype=U32) * U32(3))
            want_first = first.copy()
            want = adaptive.sample_list_numpy(counts, capacity, first=want_first)
            d_first = dev(first)
            with capped(cap):
                got = host_list(adaptive.sample_list(dev(counts), capacity, first=d_first))
            listed = int(want.total[0])
            assert np.array_equal(got.total, want.total) and np.array_equal(got.start, want.start), (kind, capacity)
            assert np.array_equal(got.pixel[:listed], want.pixel[:listed]) and np.array_equal(got.sample[:listed], want.sample[:listed]), (kind, capacity)
            assert np.array_equal(host(d_first), want_first), (kind, capacity)
    assert S.same_list(want, S.list_restated(counts, capacity, first))  # the CPU form itself, once more at this size


def test_an_empty_list_and_a_small_temp():
    torch = torch_device()
    out = adaptive.sample_list(torch.zeros(0, dtype=torch.int32, device="cuda"), 5)
    assert host(out.start).tolist() == [0] and host(out.total).tolist() == [0, 0]
    need = adaptive.list_temp_bytes(70001)
    assert need == 4 * (274 + 1) and adaptive.list_temp_bytes(0) == 0 and adaptive.list_temp_bytes(1 << 26) == 0
    with pytest.raises(rt.RtError, match="temp"):
        adaptive.sample_list(dev(S.counts_case(70001, "random")), 10, temp=torch.zeros(need - 4, dtype=torch.uint8, device="cuda"))


# ---- positions and rays ----

@pytest.mark.parametrize("cap", [None, 1])
def test_listed_offsets_and_rays_equal_the_cpu_definition(cap):
    """a tile with a row step; a pixel the tile does not have; records beyond the list"""
    frame, cam = rt.Frame(40, 30, 3, 5, 4, 22, 27, 2), rt.reference_camera()
    n = frame.rows * frame.cols
    counts = S.counts_case(n, "random") % U32(7)
    sl = adaptive.sample_list_numpy(counts, int(counts.sum()) + 300, first=(np.arange(n, dtype=U32) % U32(3)))
    sl.pixel[5] = n
    d_sl = dev_list(sl)
    for pattern in ("center", "uniform"):
        want = adaptive.offsets_listed_numpy(frame, sl, pattern, seed=77)
        with capped(cap):
            off = adaptive.offsets_listed(frame, d_sl, pattern, seed=77)
            rays = adaptive.camera_rays_listed(cam, frame, off, d_sl)
        assert np.array_equal(S.bits(host(off)), S.bits(want)), pattern
        assert np.array_equal(host(rays), adaptive.camera_rays_listed_numpy(cam, frame, want, sl).view(U32).reshape(-1, 11)), pattern


def test_listed_rays_of_equal_counts_are_the_rays_of_camera_rays_offset():
    frame, cam = rt.Frame.full(33, 17, 3), rt.reference_camera()
    n, spp = frame.rows * frame.cols, 3
    torch = torch_device()
    off = film.offsets(frame, spp, "uniform", 9)
    want = host(film.camera_rays_offset(cam, frame, off)).reshape(spp, n, 11)
    sl = adaptive.sample_list(torch.full((n,), spp, dtype=torch.int32, device="cuda"), n * spp)
    listed = adaptive.offsets_listed(frame, sl, "uniform", 9)
    assert np.array_equal(S.bits(host(listed)), S.bits(S.to_pixel_major(host(off))))
    got = host(adaptive.camera_rays_listed(cam, frame, listed, sl))
    assert np.array_equal(got, S.to_pixel_major(want))


# ---- the splat ----

@functools.lru_cache(maxsize=None)
def splat_want(rows, cols, radius):
    _, sl, samples, valid, offsets, total, weight = S.splat_case(rows, cols, 5)
    return S.host_splat_listed(rows, cols, samples, valid, offsets, sl, FILTER_OF[radius], radius, total, weight, max_count=5)


def device_splat_listed(rows, cols, samples, valid, offsets, sl, name, radius, total, weight, form, max_count, cap=None):
    f = film.Film(rows, cols, name, radius, device="cuda")
    f.sum.copy_(dev(total))
    f.weight.copy_(dev(weight))
    with rt.options(RT_AMD_FILM_SPLAT_FORM=form, **({OPTION: cap} if cap else {})):
        adaptive.splat_listed(f, dev(samples), dev(offsets), dev_list(sl), dev(valid), max_count)
    return host(f.sum), host(f.weight)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("rows,cols", S.SPLAT_IMAGES)
def test_listed_splat_equals_the_cpu_definition(rows, cols, form):
    """random counts 0 .. 5 with a valid plane, each radius class (reach 1 to 5), the whole grid and one workgroup for every tile"""
    _, sl, samples, valid, offsets, total, weight = S.splat_case(rows, cols, 5)
    for radius in S.SPLAT_RADII:
        want = splat_want(rows, cols, radius)
        for cap in (None, 1):
            got = device_splat_listed(rows, cols, samples, valid, offsets, sl, FILTER_OF[radius], radius, total, weight, form, 5, cap)
            assert np.array_equal(S.bits(got[0]), S.bits(want[0])) and np.array_equal(S.bits(got[1]), S.bits(want[1])), (radius, cap)


@pytest.mark.parametrize("form", FORMS)
def test_one_pixel_of_64_samples_beside_a_tile_border(form):
    """48 x 40, every count 0 but pixel (15, 16)'s 64: first of the tile of columns 16 .. 31, last row of its tile row, and in the halo of
    the tiles to the left and below.  Tiles whose halo holds it run all 64 sample indices — those to the left and below take the largest
    count from a pixel that is not theirs — and every other tile runs none"""
    rows, cols = 48, 40
    counts = np.zeros(rows * cols, dtype=U32)
    counts[15 * cols + 16] = 64
    sl = adaptive.sample_list_numpy(counts)
    rng = np.random.default_rng(64)
    samples = rng.random((64, 3), dtype=F32) * F32(4.0)
    offsets = rng.random((64, 2), dtype=F32) - F32(0.5)
    total, weight = np.zeros((rows, cols, 3), dtype=F32), np.zeros((rows, cols), dtype=F32)
    for name, radius in (("tent", 1.0), ("mitchell", 4.0)):
        want = S.host_splat_listed(rows, cols, samples, None, offsets, sl, name, radius, total, weight)
        assert want[1][15, 15] != 0 and want[1][15, 16] != 0 and want[1][16, 16] != 0 and want[1][16, 15] != 0  # on every side of the corner
        assert not want[1][:, 32:].any() and not want[1][32:].any()  # ... and nothing in the tiles that stage nothing
        got = device_splat_listed(rows, cols, samples, None, offsets, sl, name, radius, total, weight, form, 64)
        assert np.array_equal(S.bits(got[0]), S.bits(want[0])) and np.array_equal(S.bits(got[1]), S.bits(want[1])), name


@pytest.mark.parametrize("form", FORMS)
def test_a_start_that_is_not_a_prefix_sum_is_clamped_on_the_device(form):
    rows, cols = 17, 17
    _, sl, samples, valid, offsets, total, weight = S.splat_case(rows, cols, 3, seed=9)
    bad = adaptive.SampleList(sl.start.copy(), sl.pixel, sl.sample, sl.total, sl.capacity, sl.n)
    bad.start[3], bad.start[7], bad.start[11] = U32(0xFFFFFFFF), U32(0), U32(sl.capacity + 40)
    want = S.host_splat_listed(rows, cols, samples, valid, offsets, bad, "tent", 1.0, total, weight)
    got = device_splat_listed(rows, cols, samples, valid, offsets, bad, "tent", 1.0, total, weight, form, 64)
    assert np.array_equal(S.bits(got[0]), S.bits(want[0])) and np.array_equal(S.bits(got[1]), S.bits(want[1]))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name,radius", [("box", 0.5), ("tent", 1.0), ("mitchell", 2.0)])
def test_equal_counts_give_the_bits_of_rt_film_splat(name, radius, form):
    rows, cols, spp = 33, 17, 4
    samples, valid, offsets, total, weight = film_case(rows, cols, spp)
    f = film.Film(rows, cols, name, radius, device="cuda")
    f.sum.copy_(dev(total))
    f.weight.copy_(dev(weight))
    with rt.options(RT_AMD_FILM_SPLAT_FORM=form):
        f.splat(dev(samples), dev(offsets), dev(valid))
    sl = adaptive.sample_list_numpy(np.full(rows * cols, spp, dtype=U32))
    got = device_splat_listed(rows, cols, S.to_pixel_major(samples), S.to_pixel_major(valid), S.to_pixel_major(offsets), sl, name, radius, total, weight,
                              form, spp)
    assert np.array_equal(S.bits(got[0]), S.bits(host(f.sum))) and np.array_equal(S.bits(got[1]), S.bits(host(f.weight)))


@pytest.mark.parametrize("form", FORMS)
def test_box_centre_count_one_is_rt_accumulate_device(form):
    rows, cols = 23, 37
    n = rows * cols
    samples, valid, _, _, _ = film_case(rows, cols, 1)
    acc = rt.PhotonAccumulator(rows, cols, "cuda")
    f = film.Film(rows, cols, "box", 0.5, device="cuda")
    sl = dev_list(adaptive.sample_list_numpy(np.ones(n, dtype=U32)))
    off = adaptive.offsets_listed(rt.Frame.full(cols, rows, 3), sl, "center")
    d_samples, d_valid = dev(samples), dev(valid)
    with rt.options(RT_AMD_FILM_SPLAT_FORM=form):
        for _ in range(2):
            acc.accumulate(d_samples.view(1, rows, cols, 3), d_valid.view(1, rows, cols))
            adaptive.splat_listed(f, d_samples.view(n, 3), off, sl, d_valid.view(n), 1)
    assert np.array_equal(S.bits(host(f.sum)), S.bits(host(acc.sum))) and np.array_equal(S.bits(host(f.weight)), S.bits(host(acc.weight)))


# ---- the stream, the graph ----

def test_on_a_stream_and_in_a_captured_graph():
    """list -> offsets -> rays -> trace_rays(capacity) -> finite test -> splat with no synchronisation in between on a stream of its own;
    then the same chain captured — one stream, no parallel branches — on a SECOND fresh stream, so that the first rt_sample_list call on
    that stream is the captured one, and replayed twice on new counts"""
    torch = torch_device()
    scene, cam = rt.Scene(rt.reference_world()), rt.reference_camera()
    frame = rt.Frame.full(32, 24, 2)
    n, capacity = frame.rows * frame.cols, 2600
    rng = np.random.default_rng(3)
    all_counts = [rng.integers(0, 6, n).astype(U32) for _ in range(3)]  # about 1900 asked for
    all_counts[2][:200] = 9  # ... and one that asks for more than the capacity

    def cpu(counts):
        sl = adaptive.sample_list_numpy(counts, capacity)
        off = adaptive.offsets_listed_numpy(frame, sl, "uniform", 4)
        rays = adaptive.camera_rays_listed_numpy(cam, frame, off, sl)
        rgb, _ = rt.trace_rays_numpy(scene, rays, frame.max_depth)
        f = film.Film(frame.rows, frame.cols, "tent", 1.0)
        adaptive.splat_listed(f, rgb, off, sl, np.isfinite(rgb).all(axis=1).astype(np.uint8), 16)
        return sl.total, f.sum, f.weight

    def chain(stream, counts, f, out, temp, off, rays, rgb):
        sl = adaptive.sample_list(counts, capacity, out=out, temp=temp, stream=stream)
        adaptive.offsets_listed(frame, sl, "uniform", 4, out=off, stream=stream)
        adaptive.camera_rays_listed(cam, frame, off, sl, out=rays, stream=stream)
        rt.trace_rays(scene, rays, frame.max_depth, out=rgb, stream=stream)
        with torch.cuda.stream(stream):
            valid = torch.isfinite(rgb).all(dim=1).to(torch.uint8)
        adaptive.splat_listed(f, rgb, off, sl, valid, 16, stream=stream)

    def buffers():
        i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device="cuda")
        out = adaptive.SampleList(i32(n + 1), i32(capacity), i32(capacity), i32(2), capacity, n)
        return (film.Film(frame.rows, frame.cols, "tent", 1.0, device="cuda"), out, torch.zeros(adaptive.list_temp_bytes(n), dtype=torch.uint8, device="cuda"),
                torch.zeros((capacity, 2), dtype=torch.float32, device="cuda"), i32(capacity, 11), torch.zeros((capacity, 3), dtype=torch.float32, device="cuda"))

    def check(counts, f, out):
        total, want_sum, want_weight = cpu(counts)
        assert np.array_equal(host(out.total), total)
        assert S.same_or_both_nan(host(f.sum), want_sum) and S.same_or_both_nan(host(f.weight), want_weight)

    d_counts = dev(all_counts[0])
    bufs = buffers()
    torch.cuda.synchronize()
    chain(torch.cuda.Stream(), d_counts, *bufs)
    check(all_counts[0], bufs[0], bufs[1])

    bufs = buffers()
    stream, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    rt.trace_rays(scene, bufs[4], frame.max_depth, out=bufs[5], stream=stream)  # trace_rays' own workspace on this stream; no list call yet
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            chain(stream, d_counts, *bufs)
    torch.cuda.synchronize()
    for counts in all_counts[1:]:
        d_counts.copy_(dev(counts))
        bufs[0].sum.zero_()
        bufs[0].weight.zero_()
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            graph.replay()
        check(counts, bufs[0], bufs[1])
    assert host(bufs[1].total)[1] > host(bufs[1].total)[0] == capacity


# ---- the reference scene ----

@pytest.fixture(scope="module")
def reference():
    torch_device()
    return rt.Scene(rt.reference_world()), rt.reference_camera(), rt.Frame.full(64, 48, 5)


def test_render_pass_with_equal_counts_is_render_supersampled(reference):
    torch = torch_device()
    scene, cam, frame = reference
    n = frame.rows * frame.cols
    want = film.render_supersampled(scene, cam, frame, 4, pattern="uniform", seed=3)
    f = film.Film(frame.rows, frame.cols, "tent", 1.0, device="cuda")
    sl, _, _ = adaptive.render_pass(scene, cam, frame, f, torch.full((n,), 4, dtype=torch.int32, device="cuda"), pattern="uniform", seed=3)
    assert host(sl.total).tolist() == [4 * n, 4 * n] and sl.capacity == 4 * n
    assert np.array_equal(S.bits(host(f.resolve())), S.bits(host(want)))


def test_a_budgeted_second_pass_equals_the_cpu_sequence(reference):
    """first pass: 2 samples everywhere.  The test makes the luminance mean and variance planes of those samples with numpy and uploads
    them, so the device and the CPU sequence read the same planes; the second pass takes budget's counts and continues the sample
    indices.  gain 4, min_count 1, max_count 12: the black background has variance exactly 0 and gets 1, silhouettes get more"""
    torch = torch_device()
    scene, cam, frame = reference
    n = frame.rows * frame.cols
    kw = dict(gain=4.0, epsilon=0.05, min_count=1, max_count=12)
    dfilm = film.Film(frame.rows, frame.cols, "tent", 1.0, device="cuda")
    d_first = torch.zeros(n, dtype=torch.int32, device="cuda")
    sl1, off1, rgb1 = adaptive.render_pass(scene, cam, frame, dfilm, torch.full((n,), 2, dtype=torch.int32, device="cuda"), first=d_first, seed=5)

    # the CPU sequence, pass 1
    hfilm = film.Film(frame.rows, frame.cols, "tent", 1.0)
    first = np.zeros(n, dtype=U32)

    def cpu_pass(counts, capacity=None):
        sl = adaptive.sample_list_numpy(counts, capacity, first=first)
        off = adaptive.offsets_listed_numpy(frame, sl, "uniform", 5)
        rgb, _ = rt.trace_rays_numpy(scene, adaptive.camera_rays_listed_numpy(cam, frame, off, sl), frame.max_depth)
        adaptive.splat_listed(hfilm, rgb, off, sl, np.isfinite(rgb).all(axis=1).astype(np.uint8))
        return sl, rgb

    _, rgb = cpu_pass(np.full(n, 2, dtype=U32))
    assert S.same_or_both_nan(host(rgb1), rgb)
    assert S.same_or_both_nan(host(dfilm.sum), hfilm.sum) and S.same_or_both_nan(host(dfilm.weight), hfilm.weight)
    lum = (rgb.astype(np.float64) @ np.array([0.2126, 0.7152, 0.0722])).reshape(n, 2)
    mean = lum.mean(axis=1).astype(F32)
    variance = lum.var(axis=1).astype(F32)
    count = np.full(n, 2, dtype=U32)

    counts = adaptive.budget_numpy(mean, variance, count, **kw)
    d_counts = adaptive.budget(dev(mean), dev(variance), dev(count), **kw)
    assert np.array_equal(host(d_counts), counts)
    assert (counts == 1).any() and (counts > 1).any() and (variance[counts == 1] == 0).any()  # the condition the parameters were chosen for

    asked = int(counts.sum())
    sl2, _, _ = adaptive.render_pass(scene, cam, frame, dfilm, d_counts, first=d_first, seed=5)
    want_sl, _ = cpu_pass(counts)
    assert host(sl2.total).tolist() == [asked, asked] == want_sl.total.tolist() and sl2.capacity == asked
    assert np.array_equal(host(sl2.sample), want_sl.sample) and host(sl2.sample).min() == 2  # continued, never repeated
    assert np.array_equal(host(d_first), first) and np.array_equal(first, 2 + counts)
    assert S.same_or_both_nan(host(dfilm.sum), hfilm.sum) and S.same_or_both_nan(host(dfilm.weight), hfilm.weight)
    assert S.same_or_both_nan(host(dfilm.resolve()), hfilm.resolve())

    # a capacity above the total gives the same film as capacity=None; one below lists exactly its records
    def device_second_pass(capacity):
        f = film.Film(frame.rows, frame.cols, "tent", 1.0, device="cuda")
        sl, _, _ = adaptive.render_pass(scene, cam, frame, f, d_counts, first=torch.full((n,), 2, dtype=torch.int32, device="cuda"), seed=5, capacity=capacity)
        return sl, host(f.sum), host(f.weight)

    _, none_sum, none_weight = device_second_pass(None)
    sl_above, above_sum, above_weight = device_second_pass(asked + 777)
    assert host(sl_above.total).tolist() == [asked, asked]
    assert np.array_equal(S.bits(above_sum), S.bits(none_sum)) and np.array_equal(S.bits(above_weight), S.bits(none_weight))
    cut = asked // 2 + 1
    sl_cut, cut_sum, cut_weight = device_second_pass(cut)
    assert host(sl_cut.total).tolist() == [cut, asked] and asked > cut
    hfilm = film.Film(frame.rows, frame.cols, "tent", 1.0)
    first = np.full(n, 2, dtype=U32)
    cpu_pass(counts, cut)
    assert S.same_or_both_nan(cut_sum, hfilm.sum) and S.same_or_both_nan(cut_weight, hfilm.weight)


def test_render_adaptive_runs_and_takes_more_samples_on_edges(reference):
    scene, cam, frame = reference
    image, f, taken = adaptive.render_adaptive(scene, cam, frame, passes=1, first_spp=2, params=dict(gain=4.0, epsilon=0.05, min_count=1, max_count=12), seed=5)
    taken = host(taken)
    assert image.shape == (frame.rows, frame.cols, 3) and np.isfinite(host(image)).all()
    assert taken.min() == 3 and taken.max() > 3 and (host(f.weight) > 0).all()
