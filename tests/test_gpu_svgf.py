"""Variance-guided filter queries on the device (include/rt_amd.h "variance-guided filter queries"): rt_svgf_variance and rt_svgf_atrous
equal their CPU definitions — which tests/test_svgf_host.py holds against a numpy restatement — bit for bit: both A-Trous kernel forms
(RT_AMD_SVGF_FORM) and the variance kernel, with the image taken grid-stride, on a non-default stream, inside a captured graph and
through the _host forms; and filter_frame on the reference scene equals the CPU path on the downloaded records and guides.  Every
comparison is of the uint32 views: no tolerance anywhere."""
import ctypes as C
import functools

import numpy as np
import pytest

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import _capi, denoise, svgf, temporal
from _denoise_support import ALBEDO_AT, NORMAL_AT, POSITION_AT, VALID_AT, dist2, embed, record_views
from _records import torch_device
from _svgf_support import F32, FINITE_SIGMAS, HISTORY, IMAGES, LEVELS, MIN_LENGTH, bits, case_data

pytestmark = pytest.mark.gpu

GPU_IMAGES = IMAGES + [(40, 50)]  # more than one tile each way, no multiple of 16, smaller than the reach of levels 4 and 5
FORMS = [0, 1]                    # the simple and the tiled A-Trous kernel
SIGMAS = dict(sigma_luminance=FINITE_SIGMAS[0], sigma_normal=FINITE_SIGMAS[1], sigma_position=FINITE_SIGMAS[2])
GUIDE_SIGMAS = dict(sigma_normal=FINITE_SIGMAS[1], sigma_position=FINITE_SIGMAS[2])
# what a call is given: strided guides (views of 13- and 18-word records) and the colour inside the history records, or compact planes;
# a valid plane or none; demodulation or none
CONFIGS = [dict(strided=False, flags=True, demodulate=False), dict(strided=True, flags=True, demodulate=True),
           dict(strided=False, flags=False, demodulate=True), dict(strided=True, flags=False, demodulate=False)]


def guides_of(rows, cols, strided, flags, albedo=True):
    _, _, _, normal, position, alb, valid = case_data(rows, cols)
    if strided:
        normal, position, alb, valid = embed(normal, position, alb, valid)[2]
    g = dict(normal=normal, position=position, valid=valid if flags else None)
    return dict(g, albedo=alb) if albedo else g


def dev(a):
    a = np.array(a)
    if a.dtype == HISTORY:
        a = a.view(np.int32).reshape(-1, 8)
    return torch_device().from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def device_guides(rows, cols, strided, flags, albedo=True):
    """the guides on the device: compact tensors, or views of uploaded 13- and 18-word records at primary_surfaces' offsets"""
    torch = torch_device()
    _, _, _, normal, position, alb, valid = case_data(rows, cols)
    if not strided:
        g = dict(normal=dev(normal), position=dev(position), valid=dev(valid) if flags else None)
        return dict(g, albedo=dev(alb)) if albedo else g
    hits, surfaces, _ = embed(normal, position, alb, valid)
    h, s = dev(hits), dev(surfaces)
    g = dict(normal=s[:, NORMAL_AT:NORMAL_AT + 3], position=h[:, POSITION_AT:POSITION_AT + 3], valid=s.view(torch.int32)[:, VALID_AT] if flags else None)
    assert g["normal"].stride() == (18, 1) and g["position"].stride() == (13, 1)
    return dict(g, albedo=s[:, ALBEDO_AT:ALBEDO_AT + 3]) if albedo else g


def device_color(rows, cols, strided):
    """the colour on the device: a compact plane, or the view of uploaded history records (stride 8 words)"""
    torch = torch_device()
    color, _, history, _, _, _, _ = case_data(rows, cols)
    if not strided:
        return dev(color).view(rows, cols, 3), None
    records = dev(history)
    view = records.view(rows, cols, 8)[..., 0:3].view(torch.float32)
    assert view.stride()[-2:] == (8, 1)
    return view, records


# ---- rt_svgf_atrous ----

@functools.lru_cache(maxsize=None)
def cpu_atrous(rows, cols, first_level, levels, strided, flags, demodulate):
    """the CPU definition, computed once per case"""
    color, variance, history, _, _, _, _ = case_data(rows, cols)
    out = svgf.atrous_numpy(history["color"] if strided else color, variance, rows, cols, levels=levels, first_level=first_level, demodulate=demodulate,
                            **guides_of(rows, cols, strided, flags), **SIGMAS)
    return bits(out[0]), bits(out[1])


def device_atrous(rows, cols, first_level, levels, strided, flags, demodulate, stream=None):
    torch = torch_device()
    g = device_guides(rows, cols, strided, flags)
    color, keep = device_color(rows, cols, strided)
    variance = dev(case_data(rows, cols)[1]).view(rows, cols)
    torch.cuda.synchronize()
    out, var = svgf.atrous(color, variance, rows, cols, levels=levels, first_level=first_level, demodulate=demodulate, stream=stream, **g, **SIGMAS)
    torch.cuda.synchronize()
    assert np.array_equal(bits(color.cpu().numpy().reshape(-1, 3)), bits(case_data(rows, cols)[0]))  # the inputs are never written
    assert np.array_equal(bits(variance.cpu().numpy().reshape(-1)), bits(case_data(rows, cols)[1]))
    return bits(out.cpu().numpy()), bits(var.cpu().numpy())


def same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("rows,cols", GPU_IMAGES)
def test_atrous_equals_the_cpu_definition(rows, cols, form):
    calls = [(level, 1, CONFIGS[(level + k) % 4]) for level in LEVELS for k in (0, 1)] + [(0, 6, CONFIGS[1]), (0, 6, CONFIGS[0]), (1, 2, CONFIGS[2])]
    with rt.options(RT_AMD_SVGF_FORM=form):
        for first, levels, config in calls:
            assert same(device_atrous(rows, cols, first, levels, **config), cpu_atrous(rows, cols, first, levels, **config)), (first, levels, config)
    assert np.isnan(cpu_atrous(rows, cols, 0, 6, **CONFIGS[0])[0].view(F32)).any()  # the NaN colours passed through, payload and all


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("rows,cols", [(23, 37), (40, 50)])
def test_an_infinite_luminance_sigma_gives_the_bits_of_the_denoise_filter(rows, cols, form):
    """the two instantiations of the shared A-Trous kernels check each other, as the CPU forms do in the test of this name"""
    torch = torch_device()
    color = dev(case_data(rows, cols)[0]).view(rows, cols, 3)  # finite or NaN colours
    variance = dev(case_data(rows, cols)[1]).view(rows, cols)
    for config in CONFIGS:
        g = device_guides(rows, cols, config["strided"], config["flags"])
        kw = dict(levels=6, demodulate=config["demodulate"], **GUIDE_SIGMAS)
        torch.cuda.synchronize()
        with rt.options(RT_AMD_SVGF_FORM=form, RT_AMD_DENOISE_FORM=form):
            got, _ = svgf.atrous(color, variance, rows, cols, sigma_luminance=float("inf"), **g, **kw)
            want = denoise.atrous(color, rows, cols, sigma_color=float("inf"), **g, **kw)
        torch.cuda.synchronize()
        got, want = bits(got.cpu().numpy()), bits(want.cpu().numpy())
        assert np.array_equal(got, want) and np.isnan(got.view(F32)).any(), config


def test_atrous_without_a_variance_output_keeps_the_colour():
    torch = torch_device()
    rows, cols = 40, 50
    config = CONFIGS[1]
    g = device_guides(rows, cols, config["strided"], config["flags"])
    color, keep = device_color(rows, cols, True)
    variance = dev(case_data(rows, cols)[1]).view(rows, cols)
    torch.cuda.synchronize()
    for form in FORMS:
        with rt.options(RT_AMD_SVGF_FORM=form):
            out, var = svgf.atrous(color, variance, rows, cols, levels=5, demodulate=True, variance_out=False, **g, **SIGMAS)
        torch.cuda.synchronize()
        assert var is None and np.array_equal(bits(out.cpu().numpy()), cpu_atrous(rows, cols, 0, 5, **config)[0]), form


# ---- rt_svgf_variance ----

@functools.lru_cache(maxsize=None)
def one_short_tile(rows=40, cols=50):
    """case_data's history with every length raised to at least MIN_LENGTH except inside the tile of rows and columns 16 .. 31: the
    workgroups of the other tiles skip staging, next to one that stages"""
    history = np.array(case_data(rows, cols)[2])
    r, c = np.divmod(np.arange(rows * cols), cols)
    inside = (r >= 16) & (r < 32) & (c >= 16) & (c < 32)
    history["length"][~inside] = np.maximum(history["length"][~inside], MIN_LENGTH)
    assert ((history["length"] < MIN_LENGTH) & (history["length"] > 0) & inside).any() and not (history["length"][~inside] < MIN_LENGTH).any()
    history.setflags(write=False)
    return history


def history_of(rows, cols, kind):
    return one_short_tile(rows, cols) if kind == "one tile" else case_data(rows, cols)[2]


@functools.lru_cache(maxsize=None)
def cpu_variance(rows, cols, kind, strided, flags, min_length):
    return bits(svgf.variance_numpy(history_of(rows, cols, kind), rows, cols, min_length=min_length, **guides_of(rows, cols, strided, flags, albedo=False),
                                    **GUIDE_SIGMAS))


def device_variance(rows, cols, kind, strided, flags, min_length, stream=None):
    torch = torch_device()
    g = device_guides(rows, cols, strided, flags, albedo=False)
    records = dev(history_of(rows, cols, kind))
    torch.cuda.synchronize()
    out = svgf.variance(records, rows, cols, min_length=min_length, stream=stream, **g, **GUIDE_SIGMAS)
    torch.cuda.synchronize()
    assert np.array_equal(bits(records.cpu().numpy()), bits(history_of(rows, cols, kind)).reshape(-1, 8))  # the records are never written
    return bits(out.cpu().numpy())


VARIANCE_CALLS = [(strided, flags, min_length) for strided in (False, True) for flags in (False, True) for min_length in (1, MIN_LENGTH, 7)]


@pytest.mark.parametrize("rows,cols", GPU_IMAGES)
def test_variance_equals_the_cpu_definition(rows, cols):
    for call in VARIANCE_CALLS:
        assert np.array_equal(device_variance(rows, cols, "all", *call), cpu_variance(rows, cols, "all", *call)), call


def test_variance_with_short_histories_in_one_tile_only():
    for call in [(True, True, MIN_LENGTH), (False, False, MIN_LENGTH)]:
        assert np.array_equal(device_variance(40, 50, "one tile", *call), cpu_variance(40, 50, "one tile", *call)), call


# ---- the launch, the stream, the graph, the _host forms ----

@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("cap", [1, 3])
def test_result_does_not_depend_on_the_launch_geometry(form, cap):
    """40 x 50 is 8 workgroups of pixels, or 12 tiles at level 0 and 1024 residue classes at level 5, and 12 tiles of the variance kernel:
    with at most 1 or 3 workgroups launched the rest is taken grid-stride (RT_AMD_DIAG_SVGF_MAX_GROUPS), several tiles per workgroup"""
    rows, cols = 40, 50
    with rt.options(RT_AMD_SVGF_FORM=form, RT_AMD_DIAG_SVGF_MAX_GROUPS=cap):
        for config in (CONFIGS[1], CONFIGS[0]):
            assert same(device_atrous(rows, cols, 0, 6, **config), cpu_atrous(rows, cols, 0, 6, **config)), config
        assert same(device_atrous(70, 1, 2, 1, **CONFIGS[1]), cpu_atrous(70, 1, 2, 1, **CONFIGS[1]))
        for kind in ("all", "one tile"):
            assert np.array_equal(device_variance(rows, cols, kind, True, True, MIN_LENGTH), cpu_variance(rows, cols, kind, True, True, MIN_LENGTH)), kind


def test_the_tiled_form_at_step_16_on_a_ragged_image_under_one_workgroup():
    """the stager with a step, one workgroup striding every residue class.  17 x 33 through levels 0 .. 4 and at level 4 alone: at step 16
    the image is one block of 256 x 256 pixels whose 256 classes all start inside it and reach across it with most of their 20 x 20 entries
    outside; the uniform `continue` ahead of the first barrier is taken at step 2 only, where the second block's odd columns start at
    column 33.  17 x 257 at level 4: the second block holds column 256 alone, so 15 of every 16 of its classes start outside the image
    and take the `continue` at step 16"""
    with rt.options(RT_AMD_SVGF_FORM=1, RT_AMD_DIAG_SVGF_MAX_GROUPS=1):
        for rows, cols, first, levels in ((17, 33, 0, 5), (17, 33, 4, 1), (17, 257, 4, 1)):
            assert same(device_atrous(rows, cols, first, levels, **CONFIGS[1]), cpu_atrous(rows, cols, first, levels, **CONFIGS[1])), (rows, cols, first, levels)


@pytest.mark.parametrize("form", FORMS)
def test_on_a_stream_and_in_a_captured_graph(form):
    torch = torch_device()
    rows, cols = 40, 50
    config = CONFIGS[1]
    want_v = cpu_variance(rows, cols, "one tile", True, True, MIN_LENGTH)
    want = cpu_atrous(rows, cols, 0, 6, **config)
    stream = torch.cuda.Stream()
    with rt.options(RT_AMD_SVGF_FORM=form):
        assert same(device_atrous(rows, cols, 0, 6, stream=stream, **config), want)
        assert np.array_equal(device_variance(rows, cols, "one tile", True, True, MIN_LENGTH, stream=stream), want_v)
        g = device_guides(rows, cols, True, True)
        color, keep = device_color(rows, cols, True)
        records = dev(one_short_tile())
        variance = dev(case_data(rows, cols)[1]).view(rows, cols)
        estimate = torch.zeros((rows, cols), dtype=torch.float32, device="cuda")
        out, var = torch.zeros((rows, cols, 3), dtype=torch.float32, device="cuda"), torch.zeros((rows, cols), dtype=torch.float32, device="cuda")
        temp = torch.zeros(svgf.temp_bytes(rows, cols, 6) // 4, dtype=torch.float32, device="cuda")
        graph = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            with torch.cuda.graph(graph, stream=stream):  # one stream, no parallel branches
                svgf.variance(records, rows, cols, normal=g["normal"], position=g["position"], valid=g["valid"], out=estimate, stream=stream, **GUIDE_SIGMAS)
                svgf.atrous(color, variance, rows, cols, levels=6, demodulate=True, out=out, variance_out=var, temp=temp, stream=stream, **g, **SIGMAS)
        torch.cuda.synchronize()
        for _ in range(2):
            for t in (estimate, out, var):  # capturing ran nothing; every replay writes the whole planes again
                t.zero_()
            torch.cuda.synchronize()
            with torch.cuda.stream(stream):
                graph.replay()
            torch.cuda.synchronize()
            assert np.array_equal(bits(estimate.cpu().numpy()), want_v)
            assert same((bits(out.cpu().numpy()), bits(var.cpu().numpy())), want)


def test_the_host_forms_equal_the_cpu_definition():
    rows, cols = 40, 50
    color, variance, history, normal, position, albedo, valid = (np.array(a) for a in case_data(rows, cols))  # held: the calls take their addresses
    hits, surfaces, (s_normal, s_position, s_albedo, s_valid) = embed(normal, position, albedo, valid)
    g = _capi.DenoiseGuides(s_normal.ctypes.data, s_position.ctypes.data, s_albedo.ctypes.data, s_valid.ctypes.data, 18, 13, 18, 18)
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    lib = _capi.amd_lib()
    p = _capi.SvgfVarianceParams(FINITE_SIGMAS[1], FINITE_SIGMAS[2], MIN_LENGTH, 0)
    estimate = np.zeros(rows * cols, dtype=F32)
    _capi.check(lib.rt_svgf_variance_host(ptr(history), C.byref(g), C.byref(p), rows, cols, ptr(estimate)))
    assert np.array_equal(bits(estimate), cpu_variance(rows, cols, "all", True, True, MIN_LENGTH).reshape(-1))
    p = _capi.SvgfAtrousParams(*FINITE_SIGMAS, 0, 6, 3)
    out, var = np.zeros((rows, cols, 3), dtype=F32), np.zeros((rows, cols), dtype=F32)
    want = cpu_atrous(rows, cols, 0, 6, **CONFIGS[1])
    for form in FORMS:
        with rt.options(RT_AMD_SVGF_FORM=form):
            _capi.check(lib.rt_svgf_atrous_host(ptr(history), 8, ptr(variance), C.byref(g), C.byref(p), rows, cols, ptr(out), ptr(var)))
        assert same((bits(out), bits(var)), want), form


# ---- end to end on the reference scene at 64 x 48 ----

def test_filter_frame_on_the_reference_scene():
    torch = torch_device()
    scene, cam, frame = rt.Scene(rt.reference_world()), rt.reference_camera(), rt.Frame.full(64, 48, 3)
    rows, cols = frame.rows, frame.cols
    clean = rt.render_whitted(scene, cam, frame)
    torch.cuda.synchronize()
    clean = clean.cpu().numpy()
    moved = rt.Camera.from_buffer_copy(cam)
    toward, up = np.array(list(cam.toward), dtype=np.float64), np.array(list(cam.up), dtype=np.float64)
    right = np.cross(toward, up)
    right /= np.linalg.norm(right)
    for k in range(3):
        moved.center[k] = cam.center[k] + 0.3 * right[k]
    noise = np.random.default_rng(21)
    history = temporal.History(rows, cols)
    stream = torch.cuda.Stream()
    kw = dict(levels=5)
    for k, camera in enumerate([cam, cam, cam, moved]):  # three frames of a static camera, then a moved one
        image = dev((clean + noise.normal(0.0, 0.2, clean.shape).astype(F32)).astype(F32))
        torch.cuda.synchronize()  # the upload and the History's zeros are on the default stream
        color, variance = svgf.filter_frame(scene, camera, frame, image, history, stream=stream, **kw)
        torch.cuda.synchronize()
        records = history.records.cpu().numpy().view(HISTORY).reshape(-1)
        s = history._previous[0]
        normal, position, albedo, valid = record_views(s.hits.cpu().numpy().view(F32), s.surfaces.cpu().numpy().view(F32))
        guides = dict(normal=normal, position=position, valid=valid)
        estimate = svgf.variance_numpy(records, rows, cols, **guides)
        want_c, want_v = svgf.atrous_numpy(records["color"], estimate, rows, cols, **guides, **kw)
        assert np.array_equal(bits(color.cpu().numpy()), bits(want_c)) and np.array_equal(bits(variance.cpu().numpy()), bits(want_v)), k
        assert (bits(want_c) != bits(records["color"].reshape(rows, cols, 3))).any()
        off = valid.reshape(rows, cols) == 0
        assert off.any() and np.array_equal(bits(want_c)[off], bits(records["color"].reshape(rows, cols, 3))[off])
    # the moved frame: a pixel that reset has length 1 and a temporal variance of +0; the estimate gives it a variance > 0 wherever its
    # 7 x 7 neighbourhood holds any difference of luminance.  A neighbour counts when it is a tap of the definition (inside, valid) on
    # the pixel's own surface, x <= 1, so that it weighs at least e^-1 beside the centre's 1: a tap across an edge weighs e^-x and its
    # share of the sums can lie below their float32 rounding
    length, m1 = records["length"].reshape(rows, cols), records["moment1"].reshape(rows, cols)
    ok = valid.reshape(rows, cols) != 0
    reset = ok & (length == 1)
    nrm, pos = normal.reshape(rows, cols, 3), position.reshape(rows, cols, 3)
    lo, hi = m1.copy(), m1.copy()
    r, c = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    with np.errstate(all="ignore"):
        for dr in range(-3, 4):
            for dc in range(-3, 4):
                qr, qc = r + dr, c + dc
                inside = (qr >= 0) & (qr < rows) & (qc >= 0) & (qc < cols)
                qr, qc = np.clip(qr, 0, rows - 1), np.clip(qc, 0, cols - 1)
                x = dist2(nrm, nrm[qr, qc]) / (F32(svgf.SIGMA_NORMAL) * F32(svgf.SIGMA_NORMAL)) + dist2(pos, pos[qr, qc]) / (F32(svgf.SIGMA_POSITION) * F32(svgf.SIGMA_POSITION))
                take = inside & ok[qr, qc] & (x >= 0) & (x <= 1)
                lo = np.where(take, np.minimum(lo, m1[qr, qc]), lo)
                hi = np.where(take, np.maximum(hi, m1[qr, qc]), hi)
    differs = reset & (hi > lo)
    message = (f"svgf: moved camera: {int(reset.sum())} of {int(ok.sum())} valid pixels reset, {int(differs.sum())} of them with a luminance difference in "
               f"their neighbourhood, {int((estimate[differs] > 0).sum())} of those with a variance > 0; {int((length >= MIN_LENGTH).sum())} pixels kept a history "
               f"of {MIN_LENGTH} frames")
    print(message)
    assert reset.any() and differs.any() and (estimate[differs] > 0).all(), message
