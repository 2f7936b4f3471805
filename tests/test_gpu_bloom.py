"""The bloom queries on the device against the CPU definition, with no tolerance: both kernel forms, the grid free and capped to one
workgroup that strides every tile, at sizes whose levels have partial tiles on both axes with windows that stick out on all four
sides, the colour as a strided record view; the non-finite pixel and the in-place call; the _host form; on a stream and in a captured
graph; and bloom.finish_frame on the reference scene.  The reference result of a case is computed once and shared."""
import ctypes as C
import functools

import numpy as np
import pytest

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import _capi, bloom
from _records import spread, torch_device
import _bloom_support as S

pytestmark = pytest.mark.gpu

F32 = np.float32
SIZES = [(1, 1), (2, 2), (15, 15), (16, 16), (17, 17), (31, 18), (33, 65), (48, 40)]  # 33 x 65: level 1 is 17 x 33
FORM, CAP = "RT_AMD_BLOOM_FORM", "RT_AMD_DIAG_BLOOM_MAX_GROUPS"


def dev(a):
    return torch_device().from_numpy(np.array(a)).cuda()


def host(t):
    torch_device().cuda.synchronize()
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def want(rows, cols, levels, knee=0.5):
    out = bloom.bloom_numpy(S.case_data(rows, cols), knee=knee, levels=levels)
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("cap", [None, 1])
@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("rows,cols", SIZES)
def test_the_device_equals_the_cpu_definition(rows, cols, form, cap):
    """the colour compact and inside 8-word records; cap 1: one workgroup strides every tile of every level"""
    color = S.case_data(rows, cols)
    records, _ = S.in_records(color)
    d_color, d_view = dev(color), dev(records)[..., :3]
    with rt.options(**{FORM: form}, **({CAP: cap} if cap else {})):
        for levels in S.LEVELS:
            for knee in S.KNEES:
                expect = S.bits(want(rows, cols, levels, knee))
                assert np.array_equal(S.bits(host(bloom.bloom(d_color, knee=knee, levels=levels))), expect), (levels, knee)
                assert np.array_equal(S.bits(host(bloom.bloom(d_view, knee=knee, levels=levels))), expect), (levels, knee, "records")


@pytest.mark.parametrize("form", [0, 1])
def test_the_edges_of_the_host_tests_on_the_device(form):
    """a pixel that is not finite spreads nowhere and stays not finite; the in-place call gives the out-of-place bits"""
    rows, cols, levels = 33, 65, 5
    with rt.options(**{FORM: form}):
        for value in (np.nan, np.inf, -np.inf):
            color = S.case_data(rows, cols).copy()
            color[16, 33] = (5.0, value, 7.0)
            expect, got = bloom.bloom_numpy(color, levels=levels), host(bloom.bloom(dev(color), levels=levels))
            assert S.same_or_both_nan(got, expect) and not np.isfinite(got[16, 33, 1])
            others = np.ones((rows, cols), dtype=bool)
            others[16, 33] = False
            assert np.array_equal(S.bits(got)[others], S.bits(expect)[others]) and np.isfinite(got[others]).all()
        d_color = dev(S.case_data(rows, cols))
        assert bloom.bloom(d_color, levels=levels, out=d_color) is d_color
        assert np.array_equal(S.bits(host(d_color)), S.bits(want(rows, cols, levels)))


@pytest.mark.parametrize("rows,cols,levels", [(1, 1, 1), (17, 17, 5), (31, 18, 2), (48, 40, 5)])
def test_the_host_form_equals_the_device(rows, cols, levels):
    color = np.array(S.case_data(rows, cols))
    p = _capi.BloomParams(1.0, 0.5, 0.5, levels)
    out = np.zeros((rows, cols, 3), dtype=F32)
    _capi.check(_capi.amd_lib().rt_bloom_host(C.c_void_p(color.ctypes.data), 3, C.byref(p), rows, cols, None, C.c_void_p(out.ctypes.data)))
    got = host(bloom.bloom(dev(color), levels=levels))
    assert np.array_equal(S.bits(out), S.bits(got)) and np.array_equal(S.bits(out), S.bits(want(rows, cols, levels)))


def test_the_host_form_stages_a_strided_colour_to_its_last_word():
    """17 x 19, the colour 13 words apart in a host array of exactly (n - 1) * 13 + 3 words: a staged span one pixel short would lose
    the last pixel"""
    rows, cols, levels = 17, 19, 5
    held = spread(S.case_data(rows, cols).reshape(-1, 3), 13)
    assert held.size == (rows * cols - 1) * 13 + 3
    p = _capi.BloomParams(1.0, 0.5, 0.5, levels)
    out = np.zeros((rows, cols, 3), dtype=F32)
    _capi.check(_capi.amd_lib().rt_bloom_host(C.c_void_p(held.ctypes.data), 13, C.byref(p), rows, cols, None, C.c_void_p(out.ctypes.data)))
    assert np.array_equal(S.bits(out)[-1, -1], S.bits(want(rows, cols, levels))[-1, -1])
    assert np.array_equal(S.bits(out), S.bits(want(rows, cols, levels)))


def test_on_a_stream_and_in_a_captured_graph():
    """one call on a stream of its own; then the call captured with out and temp given — the plain linear sequence of its 2 L launches —
    and replayed twice on new colours"""
    torch = torch_device()
    rows, cols, levels = 48, 40, 5
    colours = [S.case_data(rows, cols, seed=k) for k in (51, 52, 53)]
    d_color = dev(colours[0])
    out = torch.zeros((rows, cols, 3), dtype=torch.float32, device="cuda")
    temp = torch.zeros((bloom.temp_bytes(rows, cols, levels) // 4,), dtype=torch.float32, device="cuda")
    stream = torch.cuda.Stream()

    def call():
        assert bloom.bloom(d_color, levels=levels, out=out, temp=temp, stream=stream) is out

    def check(color):
        assert np.array_equal(S.bits(host(out)), S.bits(bloom.bloom_numpy(color, levels=levels)))

    torch.cuda.synchronize()
    call()
    check(colours[0])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            call()
    torch.cuda.synchronize()
    for color in colours[1:]:
        d_color.copy_(dev(color))
        out.zero_()  # capturing ran nothing; every replay writes the whole plane again
        temp.fill_(float("nan"))  # and every level of the scratch before it reads it
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            graph.replay()
        check(color)


def test_finish_frame_on_the_reference_scene():
    """64 x 48, depth 5: post_process_device -> bloom -> encode_srgb8_device on one stream equals post_process -> bloom_numpy ->
    encode_srgb8 on the host, bytes and floats both; and the frame has highlights for the bloom to spread"""
    torch = torch_device()
    scene, cam, frame = rt.Scene(rt.reference_world()), rt.reference_camera(), rt.Frame.full(64, 48, 5)
    img = rt.render_whitted(scene, cam, frame)
    torch.cuda.synchronize()
    linear = img.cpu().numpy()
    stream = torch.cuda.Stream()
    rgb8, after = bloom.finish_frame(img, stream=stream)
    torch.cuda.synchronize()
    assert rt.post_process(linear) > 0.0
    expect = bloom.bloom_numpy(linear)
    assert np.array_equal(S.bits(after.cpu().numpy()), S.bits(expect)) and np.array_equal(S.bits(img.cpu().numpy()), S.bits(linear))
    assert np.array_equal(rgb8.cpu().numpy(), rt.encode_srgb8(expect))
    assert (expect > linear).any() and (expect >= linear).all()
