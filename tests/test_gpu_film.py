"""Film queries on the device (include/rt_amd.h "film queries"): rt_film_offsets, rt_camera_rays_offset and rt_film_splat equal their CPU
definitions bit for bit — the host forms of librt_host.so, which tests/test_film_host.py holds against numpy restatements — through both
forms of the splat kernel (RT_AMD_FILM_SPLAT_FORM), with the image taken grid-stride, on a non-default stream and inside a captured graph; and the consequences of the
definition hold on the device: box 0.5 is rt_accumulate_device, one splat of spp samples is spp splats of one.  Every comparison is of
the uint32 views: no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import film
import _oracle
from _film_support import bits, case_data, F32, FILTERS, host_splat, IMAGES, offsets_restated, SPPS
from _records import torch_device

pytestmark = pytest.mark.gpu

GPU_IMAGES = IMAGES + [(33, 17), (16, 16)]  # tile edges off and on the image edge
GPU_RADII = [0.5, 1.0, 2.0, 4.0]            # reach 1, 2, 3 and 5, the largest halo
FORMS = [0, 1]                              # the simple and the tiled kernel


def dev(a):
    return None if a is None else torch_device().from_numpy(np.array(a)).cuda()


def device_splat(rows, cols, samples, valid, offsets, name, radius, total=None, weight=None, form=None, stream=None):
    torch = torch_device()
    f = film.Film(rows, cols, name, radius, device="cuda")
    if total is not None:
        f.sum.copy_(dev(total))
        f.weight.copy_(dev(weight))
    args = (dev(samples), dev(offsets), dev(valid))
    torch.cuda.synchronize()
    with rt.options(RT_AMD_FILM_SPLAT_FORM=form):
        f.splat(*args, stream=stream)
    torch.cuda.synchronize()
    return f.sum.cpu().numpy(), f.weight.cpu().numpy()


@pytest.mark.parametrize("seed", [0, 0x9E3779B9])
@pytest.mark.parametrize("pattern,spp", [(p, s) for p in ("center", "uniform", "stratified") for s in (1, 4, 9)] + [("uniform", 3)])
def test_offsets_equal_the_host_definition(pattern, spp, seed):
    torch = torch_device()
    for frame in (rt.Frame.full(37, 23, 0), rt.Frame(37, 23, 0, 5, 3, 30, 20, 2)):
        got = film.offsets(frame, spp, pattern, seed)
        torch.cuda.synchronize()
        assert np.array_equal(bits(got.cpu().numpy()), bits(film.offsets_numpy(frame, spp, pattern, seed)))
        assert np.array_equal(bits(got.cpu().numpy()), bits(offsets_restated(frame, spp, pattern, seed)))


def test_camera_rays_offset_with_centre_offsets_is_camera_rays_repeated():
    torch = torch_device()
    cam = rt.reference_camera()
    for frame in (rt.Frame.full(37, 23, 0), rt.Frame(37, 23, 0, 5, 3, 30, 20, 2)):
        rays = film.camera_rays_offset(cam, frame, film.offsets(frame, 2, "center"))
        plain = rt.camera_rays(cam, frame)
        torch.cuda.synchronize()
        n = frame.rows * frame.cols
        assert rays.shape == (2 * n, 11)
        assert np.array_equal(rays.cpu().numpy().reshape(2, n, 11), np.stack([plain.cpu().numpy()] * 2))


def test_camera_rays_offset_equals_shoot_through_the_restated_clip():
    """Camera::shoot of the oracle (what rt_camera_rays is pinned to) on the clip coordinates of the definition, computed here in float32"""
    torch = torch_device()
    cam = rt.reference_camera()
    lib = _oracle.lib()
    for frame in (rt.Frame.full(37, 23, 0), rt.Frame(37, 23, 0, 5, 3, 30, 20, 2)):
        off = film.offsets_numpy(frame, 4, "stratified", 3)
        got = film.camera_rays_offset(cam, frame, dev(off))
        torch.cuda.synchronize()
        got = got.cpu().numpy().view(np.uint32)
        n = frame.rows * frame.cols
        ys, xs = np.meshgrid(np.arange(frame.y0, frame.y1, frame.y_step), np.arange(frame.x0, frame.x1), indexing="ij")
        height, half_h, half_w = F32(frame.height), F32(frame.height) / F32(2.0), F32(frame.width) / F32(2.0)
        want = np.zeros((4 * n, 11), dtype=np.uint32)
        clip, r = (C.c_float * 2)(), _oracle.OrcRay()
        for s in range(4):
            clip_x = ((xs.reshape(-1).astype(F32) + off[s, :, 0]) - half_w) / height
            clip_y = (half_h - (ys.reshape(-1).astype(F32) + off[s, :, 1])) / height
            for i in range(n):
                clip[0], clip[1] = clip_x[i], clip_y[i]
                lib.orc_shoot(C.byref(cam), clip, C.byref(r))
                want[s * n + i] = np.frombuffer(bytes(r), dtype=np.uint32)
        assert np.array_equal(got, want)
        # ... and the host round trip
        assert np.array_equal(film.camera_rays_offset_numpy(cam, frame, off).view(np.uint32).reshape(-1, 11), want)


@pytest.mark.parametrize("name", FILTERS)
@pytest.mark.parametrize("rows,cols", GPU_IMAGES)
def test_splat_equals_the_host_definition(rows, cols, name):
    torch = torch_device()
    stream = torch.cuda.Stream()
    for spp in SPPS:
        samples, valid, offsets, total, weight = case_data(rows, cols, spp)
        for radius in GPU_RADII:
            for flags in (valid, None):
                want = host_splat(rows, cols, samples, flags, offsets, name, radius, total, weight)
                for form in FORMS:
                    got = device_splat(rows, cols, samples, flags, offsets, name, radius, total, weight, form=form, stream=stream)
                    assert np.array_equal(bits(got[0]), bits(want[0])), (spp, radius, flags is None, form)
                    assert np.array_equal(bits(got[1]), bits(want[1])), (spp, radius, flags is None, form)


@pytest.mark.parametrize("form", FORMS)
def test_splat_at_reach_four(form):
    """radius 3.0 is reach 4, the halo width GPU_RADII leaves out; 17 x 17 is four tiles, three of them one pixel wide or tall"""
    rows, cols = 17, 17
    samples, valid, offsets, total, weight = case_data(rows, cols, 4)
    want = host_splat(rows, cols, samples, valid, offsets, "mitchell", 3.0, total, weight)
    got = device_splat(rows, cols, samples, valid, offsets, "mitchell", 3.0, total, weight, form=form)
    assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1]))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("rows,cols", [(33, 17), (70, 1)])
def test_splat_does_not_depend_on_the_launch_geometry(rows, cols, form):
    """33 x 17 is 3 workgroups of pixels or 6 tiles, 70 x 1 is 1 workgroup or 5 tiles: with at most 1, 2 or 4 workgroups launched, the rest
    of the image is taken grid-stride (RT_AMD_DIAG_FILM_MAX_GROUPS), several pixels or tiles per workgroup"""
    samples, valid, offsets, total, weight = case_data(rows, cols, 4)
    for name, radius in (("tent", 1.0), ("mitchell", 4.0)):
        want = host_splat(rows, cols, samples, valid, offsets, name, radius, total, weight)
        for cap in (1, 2, 4):
            with rt.options(RT_AMD_DIAG_FILM_MAX_GROUPS=cap):
                got = device_splat(rows, cols, samples, valid, offsets, name, radius, total, weight, form=form)
            assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1])), (name, cap)


@pytest.mark.parametrize("form", FORMS)
def test_a_nan_sample_on_the_device(form):
    rows, cols, spp = 33, 17, 4
    samples, valid, offsets, _, _ = case_data(rows, cols, spp)
    samples, valid = samples.copy(), valid.copy()
    q = 16 * cols + 15  # next to a tile corner
    samples[2, q, 1] = np.nan
    for flag in (0, 1):
        valid[2, q] = flag
        want = host_splat(rows, cols, samples, valid, offsets, "tent", 1.0)
        got = device_splat(rows, cols, samples, valid, offsets, "tent", 1.0, form=form)
        assert np.isnan(want[0]).any() == bool(flag)
        nan = np.isnan(want[0])
        assert np.array_equal(np.isnan(got[0]), nan)  # a NaN is a NaN: its payload is not compared
        assert np.array_equal(bits(got[0])[~nan], bits(want[0])[~nan]) and np.array_equal(bits(got[1]), bits(want[1]))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("rows,cols", [(23, 37), (16, 16)])
def test_box_of_radius_half_is_rt_accumulate_device(rows, cols, form):
    torch = torch_device()
    samples, valid, _, _, _ = case_data(rows, cols, 4)
    offsets = np.random.default_rng(5).random((4, rows * cols, 2), dtype=F32) - F32(0.5)  # [-0.5, 0.5)
    offsets[0, 0] = F32(-0.5)
    acc = rt.PhotonAccumulator(rows, cols, "cuda")
    f = film.Film(rows, cols, "box", 0.5, device="cuda")
    d_samples, d_valid, d_offsets = dev(samples), dev(valid), dev(offsets)
    with rt.options(RT_AMD_FILM_SPLAT_FORM=form):
        for _ in range(2):
            acc.accumulate(d_samples.view(4, rows, cols, 3), d_valid.view(4, rows, cols))
            f.splat(d_samples, d_offsets, d_valid)
    torch.cuda.synchronize()
    assert np.array_equal(bits(f.sum.cpu().numpy()), bits(acc.sum.cpu().numpy()))
    assert np.array_equal(bits(f.weight.cpu().numpy()), bits(acc.weight.cpu().numpy()))
    assert np.array_equal(bits(f.resolve().cpu().numpy()), bits(acc.resolve().cpu().numpy()))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name,radius", [("box", 0.5), ("tent", 1.0), ("mitchell", 2.0)])
def test_one_splat_of_four_samples_is_four_splats_of_one(name, radius, form):
    torch = torch_device()
    rows, cols = 33, 17
    samples, valid, offsets, total, weight = case_data(rows, cols, 4)
    once = device_splat(rows, cols, samples, valid, offsets, name, radius, total, weight, form=form)
    f = film.Film(rows, cols, name, radius, device="cuda")
    f.sum.copy_(dev(total))
    f.weight.copy_(dev(weight))
    d_samples, d_valid, d_offsets = dev(samples), dev(valid), dev(offsets)
    with rt.options(RT_AMD_FILM_SPLAT_FORM=form):
        for s in range(4):
            f.splat(d_samples[s:s + 1], d_offsets[s:s + 1], d_valid[s:s + 1])
    torch.cuda.synchronize()
    assert np.array_equal(bits(f.sum.cpu().numpy()), bits(once[0])) and np.array_equal(bits(f.weight.cpu().numpy()), bits(once[1]))


@pytest.mark.parametrize("form", FORMS)
def test_splat_in_a_captured_graph(form):
    torch = torch_device()
    rows, cols = 33, 17
    samples, valid, offsets, total, weight = case_data(rows, cols, 4)
    eager = device_splat(rows, cols, samples, valid, offsets, "mitchell", 2.0, total, weight, form=form)
    f = film.Film(rows, cols, "mitchell", 2.0, device="cuda")
    d_samples, d_valid, d_offsets = dev(samples), dev(valid), dev(offsets)
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with rt.options(RT_AMD_FILM_SPLAT_FORM=form):
        with torch.cuda.stream(stream):
            with torch.cuda.graph(graph, stream=stream):  # one stream, no parallel branches
                f.splat(d_samples, d_offsets, d_valid, stream=stream)
    torch.cuda.synchronize()
    f.sum.copy_(dev(total))  # capturing ran nothing; the replay continues from these
    f.weight.copy_(dev(weight))
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(bits(f.sum.cpu().numpy()), bits(eager[0])) and np.array_equal(bits(f.weight.cpu().numpy()), bits(eager[1]))


def test_render_supersampled():
    torch = torch_device()
    world, cam = rt.reference_world(), rt.reference_camera()
    scene = rt.Scene(world)
    frame = rt.Frame.full(48, 36, 3)
    n = frame.rows * frame.cols
    # one sample through the pixel's integer coordinate, given to its own pixel with weight 1: the Whitted frame
    plain = rt.render_whitted(scene, cam, frame)
    one = film.render_supersampled(scene, cam, frame, 1, pattern="center", filter="box", radius=0.5)
    torch.cuda.synchronize()
    plain, one = plain.cpu().numpy(), one.cpu().numpy()
    assert np.isfinite(plain).all()
    assert np.array_equal(bits(one), bits(plain))
    # four stratified samples under a tent: the host pipeline, step by step
    stream = torch.cuda.Stream()
    got = film.render_supersampled(scene, cam, frame, 4, pattern="stratified", seed=11, filter="tent", radius=1.0, stream=stream)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    off = film.offsets_numpy(frame, 4, "stratified", 11)
    rays = film.camera_rays_offset_numpy(cam, frame, off)
    rgb, _ = rt.trace_rays_numpy(scene, rays, frame.max_depth)
    host = film.Film(frame.rows, frame.cols, "tent", 1.0)
    host.splat(rgb.reshape(4, n, 3), off, np.isfinite(rgb).all(axis=1).astype(np.uint8).reshape(4, n))
    assert np.array_equal(bits(got), bits(host.resolve()))
    assert (bits(got) != bits(plain)).any(axis=-1).sum() >= 1
    with pytest.raises(ValueError):
        film.render_supersampled(scene, cam, rt.Frame(48, 36, 3, 0, 0, 48, 36, 2), 4)
