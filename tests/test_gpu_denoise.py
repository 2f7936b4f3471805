"""Denoise queries on the device (include/rt_amd.h "denoise queries"): rt_denoise_atrous equals its CPU definition rt_denoise_atrous_cpu
— which tests/test_denoise_host.py holds against a numpy restatement — bit for bit, through both kernel forms (RT_AMD_DENOISE_FORM), with
the image taken grid-stride, on a non-default stream and inside a captured graph; and denoise_frame on the reference scene equals the
CPU form on the downloaded records.  Every comparison is of the uint32 views: no tolerance anywhere."""
import ctypes as C
import functools

import numpy as np
import pytest

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import _capi, denoise, materials
from _denoise_support import ALBEDO_AT, FINITE_SIGMAS, IMAGES, LEVELS, NORMAL_AT, POSITION_AT, VALID_AT, bits, case_data, embed, record_views
from _records import torch_device

pytestmark = pytest.mark.gpu

GPU_IMAGES = IMAGES + [(40, 50)]  # more than one tile each way, no multiple of 16, smaller than the reach of levels 4 and 5
FORMS = [0, 1]                    # the simple and the tiled kernel
SIGMAS = dict(sigma_color=FINITE_SIGMAS[0], sigma_normal=FINITE_SIGMAS[1], sigma_position=FINITE_SIGMAS[2])
# what a call is given: strided guides (views of 13- and 18-word records) or compact ones, a valid plane or none, demodulation or none
CONFIGS = [dict(strided=False, flags=True, demodulate=False), dict(strided=True, flags=True, demodulate=True),
           dict(strided=False, flags=False, demodulate=True), dict(strided=True, flags=False, demodulate=False)]


@functools.lru_cache(maxsize=None)
def gpu_case(rows, cols):
    """case_data with a few NaN colours, on valid and on cleared pixels; shared, left unchanged"""
    color, normal, position, albedo, valid = case_data(rows, cols)
    color = color.copy()
    n = rows * cols
    for q in sorted({0, n // 3, n // 2 + 1, n - 1}):
        color[q % n, q % 3] = np.nan
    color.setflags(write=False)
    return color, normal, position, albedo, valid


def guides_of(rows, cols, strided, flags):
    _, normal, position, albedo, valid = gpu_case(rows, cols)
    if strided:
        normal, position, albedo, valid = embed(normal, position, albedo, valid)[2]
    return dict(normal=normal, position=position, albedo=albedo, valid=valid if flags else None)


@functools.lru_cache(maxsize=None)
def cpu_result(rows, cols, first_level, levels, strided, flags, demodulate):
    """the CPU definition, computed once per case"""
    out = denoise.atrous_numpy(gpu_case(rows, cols)[0], rows, cols, levels=levels, first_level=first_level, demodulate=demodulate,
                               **guides_of(rows, cols, strided, flags), **SIGMAS)
    out.setflags(write=False)
    return out


def dev(a):
    return None if a is None else torch_device().from_numpy(np.array(a).view(np.int32 if a.dtype == np.uint32 else a.dtype)).cuda()


def device_guides(rows, cols, strided, flags):
    """the guides on the device: compact tensors, or views of uploaded 13- and 18-word records at primary_surfaces' offsets"""
    torch = torch_device()
    _, normal, position, albedo, valid = gpu_case(rows, cols)
    if not strided:
        return dict(normal=dev(normal), position=dev(position), albedo=dev(albedo), valid=dev(valid) if flags else None)
    hits, surfaces, _ = embed(normal, position, albedo, valid)
    h, s = dev(hits), dev(surfaces)
    g = dict(normal=s[:, NORMAL_AT:NORMAL_AT + 3], position=h[:, POSITION_AT:POSITION_AT + 3], albedo=s[:, ALBEDO_AT:ALBEDO_AT + 3],
             valid=s.view(torch.int32)[:, VALID_AT] if flags else None)
    assert g["normal"].stride() == (18, 1) and g["position"].stride() == (13, 1) and g["albedo"].stride() == (18, 1)
    return g


def device_result(rows, cols, first_level, levels, strided, flags, demodulate, stream=None, out=None, temp=None):
    torch = torch_device()
    g = device_guides(rows, cols, strided, flags)
    color = dev(gpu_case(rows, cols)[0]).view(rows, cols, 3)
    torch.cuda.synchronize()
    got = denoise.atrous(color, rows, cols, levels=levels, first_level=first_level, demodulate=demodulate, out=out, temp=temp, stream=stream, **g, **SIGMAS)
    torch.cuda.synchronize()
    assert np.array_equal(bits(color.cpu().numpy().reshape(-1, 3)), bits(gpu_case(rows, cols)[0]))  # color is never written
    return got.cpu().numpy()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("rows,cols", GPU_IMAGES)
def test_device_equals_the_cpu_definition(rows, cols, form):
    calls = [(level, 1, CONFIGS[(level + k) % 4]) for level in LEVELS for k in (0, 1)] + [(0, 6, CONFIGS[1]), (0, 6, CONFIGS[0])]
    with rt.options(RT_AMD_DENOISE_FORM=form):
        for first, levels, config in calls:
            got = device_result(rows, cols, first, levels, **config)
            want = cpu_result(rows, cols, first, levels, **config)
            assert np.array_equal(bits(got), bits(want)), (first, levels, config)
    assert np.isnan(cpu_result(rows, cols, 0, 6, **CONFIGS[0])).any()  # the NaN colours passed through, payload and all


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("cap", [1, 3])
def test_result_does_not_depend_on_the_launch_geometry(form, cap):
    """40 x 50 is 8 workgroups of pixels, or 12 tiles at level 0 and 1024 residue classes at level 5: with at most 1 or 3 workgroups
    launched the rest is taken grid-stride (RT_AMD_DIAG_DENOISE_MAX_GROUPS), several pixels or tiles per workgroup"""
    rows, cols = 40, 50
    with rt.options(RT_AMD_DENOISE_FORM=form, RT_AMD_DIAG_DENOISE_MAX_GROUPS=cap):
        for config in (CONFIGS[1], CONFIGS[0]):
            got = device_result(rows, cols, 0, 6, **config)
            assert np.array_equal(bits(got), bits(cpu_result(rows, cols, 0, 6, **config))), config
        got = device_result(70, 1, 2, 1, **CONFIGS[1])
        assert np.array_equal(bits(got), bits(cpu_result(70, 1, 2, 1, **CONFIGS[1])))


def test_the_tiled_form_at_step_16_on_a_ragged_image_under_one_workgroup():
    """the stager with a step, one workgroup striding every residue class.  17 x 33 through levels 0 .. 4 and at level 4 alone: at step 16
    the image is one block of 256 x 256 pixels whose 256 classes all start inside it and reach across it with most of their 20 x 20 entries
    outside; the uniform `continue` ahead of the first barrier is taken at step 2 only, where the second block's odd columns start at
    column 33.  17 x 257 at level 4: the second block holds column 256 alone, so 15 of every 16 of its classes start outside the image
    and take the `continue` at step 16"""
    with rt.options(RT_AMD_DENOISE_FORM=1, RT_AMD_DIAG_DENOISE_MAX_GROUPS=1):
        for rows, cols, first, levels in ((17, 33, 0, 5), (17, 33, 4, 1), (17, 257, 4, 1)):
            got = device_result(rows, cols, first, levels, **CONFIGS[1])
            assert np.array_equal(bits(got), bits(cpu_result(rows, cols, first, levels, **CONFIGS[1]))), (rows, cols, first, levels)


@pytest.mark.parametrize("form", FORMS)
def test_on_a_stream_and_in_a_captured_graph(form):
    torch = torch_device()
    rows, cols = 40, 50
    config = CONFIGS[1]
    want = cpu_result(rows, cols, 0, 6, **config)
    stream = torch.cuda.Stream()
    with rt.options(RT_AMD_DENOISE_FORM=form):
        got = device_result(rows, cols, 0, 6, stream=stream, **config)
        assert np.array_equal(bits(got), bits(want))
        g = device_guides(rows, cols, config["strided"], config["flags"])
        color = dev(gpu_case(rows, cols)[0]).view(rows, cols, 3)
        out, temp = torch.zeros_like(color), torch.zeros_like(color)
        graph = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            with torch.cuda.graph(graph, stream=stream):  # one stream, no parallel branches
                denoise.atrous(color, rows, cols, levels=6, demodulate=True, out=out, temp=temp, stream=stream, **g, **SIGMAS)
        torch.cuda.synchronize()
        for _ in range(2):
            out.zero_()  # capturing ran nothing; every replay writes the whole plane again
            torch.cuda.synchronize()
            with torch.cuda.stream(stream):
                graph.replay()
            torch.cuda.synchronize()
            assert np.array_equal(bits(out.cpu().numpy()), bits(want))


def test_denoise_frame_on_the_reference_scene():
    torch = torch_device()
    world, cam = rt.reference_world(), rt.reference_camera()
    scene = rt.Scene(world)
    frame = rt.Frame.full(64, 48, 3)
    rows, cols = frame.rows, frame.cols
    stream = torch.cuda.Stream()
    image = rt.render_whitted(scene, cam, frame)
    torch.cuda.synchronize()
    kw = dict(levels=5, demodulate=True)
    got = denoise.denoise_frame(scene, cam, frame, image, stream=stream, **kw)
    s = materials.primary_surfaces(scene, cam, frame)
    torch.cuda.synchronize()
    got, plain = got.cpu().numpy(), image.cpu().numpy()
    assert np.isfinite(plain).all()
    hits = s.hits.cpu().numpy().view(np.float32)
    surfaces = s.surfaces.cpu().numpy().view(np.float32)
    normal, position, albedo, valid = record_views(hits, surfaces)
    assert int((valid != 0).sum()) > 0
    want = denoise.atrous_numpy(plain, rows, cols, normal=normal, position=position, albedo=albedo, valid=valid, **kw)
    assert np.array_equal(bits(got), bits(want))
    assert (bits(got) != bits(plain)).any() and np.array_equal(bits(got)[valid.reshape(rows, cols) == 0], bits(plain)[valid.reshape(rows, cols) == 0])
    # ... and the round trip through the kernels on host buffers
    g = _capi.DenoiseGuides(normal.ctypes.data, position.ctypes.data, albedo.ctypes.data, valid.ctypes.data, 18, 13, 18, 18)
    p = _capi.DenoiseParams(denoise.SIGMA_COLOR, denoise.SIGMA_NORMAL, denoise.SIGMA_POSITION, 0, 5, 3)
    flat = np.ascontiguousarray(plain)
    out = np.zeros_like(flat)
    for form in FORMS:
        with rt.options(RT_AMD_DENOISE_FORM=form):
            _capi.check(_capi.amd_lib().rt_denoise_atrous_host(C.c_void_p(flat.ctypes.data), C.byref(g), C.byref(p), rows, cols, C.c_void_p(out.ctypes.data)))
        assert np.array_equal(bits(out), bits(want)), form
