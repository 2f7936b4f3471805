"""Temporal queries on the device (include/rt_amd.h "temporal queries"): rt_temporal_motion and rt_temporal_accumulate equal their CPU
definitions — which tests/test_temporal_host.py holds against a numpy restatement — bit for bit, on compact planes and on strided record
views, with the image taken grid-stride by one workgroup, through the _host forms and inside a captured graph; and accumulate_frame on
the reference scene equals the CPU path fed the same device-produced guides, with the history lengths the definition implies.  Every
comparison is of the uint32 views: no tolerance anywhere."""
import ctypes as C
import functools

import numpy as np
import pytest

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import _capi, temporal
from _records import torch_device
from _temporal_support import FIELDS, HISTORY, IMAGES, NORMAL_AT, OBJECT_AT, PARAMS, POSITION_AT, VALID_AT, F32, Planes, bits, case_data, embed, motion_field

pytestmark = pytest.mark.gpu
NAMES = ("normal", "position", "object", "valid")


def dev(a):
    a = np.array(a)
    if a.dtype == HISTORY:
        a = a.view(np.int32).reshape(-1, 8)
    return torch_device().from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def host_guides(p, strided):
    p = embed(p)[2] if strided else p
    return temporal.Guides(*(getattr(p, k) for k in NAMES))


def device_guides(p, strided):
    """the guides on the device: compact tensors, or views of uploaded 13- and 18-word records at primary_surfaces' offsets"""
    torch = torch_device()
    if not strided:
        return temporal.Guides(*(dev(getattr(p, k)) for k in NAMES)), None
    hits, surfaces, _ = embed(p)
    h, s = dev(hits), dev(surfaces)
    g = temporal.Guides(s[:, NORMAL_AT:NORMAL_AT + 3], h[:, POSITION_AT:POSITION_AT + 3], h.view(torch.int32)[:, OBJECT_AT], s.view(torch.int32)[:, VALID_AT])
    assert g.normal.stride() == (18, 1) and g.position.stride() == (13, 1) and g.object.stride() == (13,) and g.valid.stride() == (18,)
    return g, (h, s)


@functools.lru_cache(maxsize=None)
def cpu_result(rows, cols, kind, strided):
    color, history, cur, prev = case_data(rows, cols)
    got, var = temporal.accumulate_numpy(color, motion_field(rows, cols, kind), rows, cols, history, host_guides(cur, strided), host_guides(prev, strided),
                                         **PARAMS)
    return bits(got.reshape(-1)), bits(var.reshape(-1))


def device_result(rows, cols, kind, strided, stream=None):
    torch = torch_device()
    color, history, cur, prev = case_data(rows, cols)
    (gc, keep_c), (gp, keep_p) = device_guides(cur, strided), device_guides(prev, strided)
    d_color, d_motion, d_history = dev(color).view(rows, cols, 3), dev(motion_field(rows, cols, kind)).view(rows, cols, 2), dev(history)
    torch.cuda.synchronize()
    out, var = temporal.accumulate(d_color, d_motion, rows, cols, d_history, gc, gp, stream=stream, **PARAMS)
    torch.cuda.synchronize()
    assert np.array_equal(bits(d_history.cpu().numpy()), bits(history))  # the input history is never written
    return bits(out.cpu().numpy()), bits(var.cpu().numpy().reshape(-1))


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("rows,cols", IMAGES)
def test_accumulate_equals_the_cpu_definition(rows, cols, strided):
    for kind in FIELDS:
        got, want = device_result(rows, cols, kind, strided), cpu_result(rows, cols, kind, strided)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), kind


@pytest.mark.parametrize("cap", [1, None])
def test_result_does_not_depend_on_the_launch_geometry(cap):
    """33 x 65 is 9 workgroups of pixels: with one workgroup launched (RT_AMD_DIAG_TEMPORAL_MAX_GROUPS=1) it strides over the whole image"""
    rows, cols = 33, 65
    with rt.options(RT_AMD_DIAG_TEMPORAL_MAX_GROUPS=cap):
        for kind, strided in (("fractional", True), ("special3", False)):
            got, want = device_result(rows, cols, kind, strided), cpu_result(rows, cols, kind, strided)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (kind, strided)
        check_motion(rows, cols)


def check_motion(rows, cols, stream=None):
    torch = torch_device()
    cam, frame = rt.reference_camera(), rt.Frame.full(cols, rows, 3)
    g = np.random.default_rng(rows * 100 + cols)
    position = (g.random((rows * cols, 3), dtype=F32) * F32(40.0) - F32(20.0)).astype(F32)
    valid = (g.random(rows * cols) >= 0.2).astype(np.uint32)
    want = temporal.motion_numpy(position, cam, frame, valid=valid)
    planes = Planes(np.zeros_like(position), position, np.zeros(rows * cols, dtype=np.uint32), valid)
    for strided in (False, True):
        gd, keep = device_guides(planes, strided)
        torch.cuda.synchronize()
        got = temporal.motion(gd.position, cam, frame, valid=gd.valid, stream=stream)
        torch.cuda.synchronize()
        assert np.array_equal(bits(got.cpu().numpy()), bits(want)), strided
    free = temporal.motion(dev(position), cam, frame)
    torch.cuda.synchronize()
    assert np.array_equal(bits(free.cpu().numpy()), bits(temporal.motion_numpy(position, cam, frame)))
    # ... and the round trip through the kernel on host buffers
    out = np.zeros((rows, cols, 2), dtype=F32)
    hits, surfaces, views = embed(planes)
    _capi.check(_capi.amd_lib().rt_temporal_motion_host(C.c_void_p(views.position.ctypes.data), 13, C.c_void_p(views.valid.ctypes.data), 18, C.byref(cam),
                                                        C.byref(frame), C.c_void_p(out.ctypes.data)))
    assert np.array_equal(bits(out), bits(want))


@pytest.mark.parametrize("rows,cols", IMAGES)
def test_motion_equals_the_cpu_definition(rows, cols):
    check_motion(rows, cols, stream=torch_device().cuda.Stream())


def test_the_host_form_equals_the_cpu_definition():
    rows, cols = 33, 65
    color, history, cur, prev = case_data(rows, cols)
    (_, _, vc), (_, _, vp) = embed(cur), embed(prev)
    m = np.array(motion_field(rows, cols, "special5"))
    gc = _capi.TemporalGuides(vc.normal.ctypes.data, vc.position.ctypes.data, vc.object.ctypes.data, vc.valid.ctypes.data, 18, 13, 13, 18)
    gp = _capi.TemporalGuides(vp.normal.ctypes.data, vp.position.ctypes.data, vp.object.ctypes.data, vp.valid.ctypes.data, 18, 13, 13, 18)
    p = _capi.TemporalParams(PARAMS["normal_min"], PARAMS["position_max"], PARAMS["alpha_min"], PARAMS["max_length"], 0)
    h_in, c = np.array(history), np.array(color)  # held: the call takes their addresses
    out, var = np.zeros(rows * cols, dtype=HISTORY), np.zeros(rows * cols, dtype=F32)
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    _capi.check(_capi.amd_lib().rt_temporal_accumulate_host(ptr(c), ptr(m), C.byref(gc), C.byref(gp), C.byref(p), rows, cols, ptr(h_in), ptr(out),
                                                            ptr(var)))
    want = cpu_result(rows, cols, "special5", True)
    assert np.array_equal(bits(out), want[0]) and np.array_equal(bits(var), want[1])


def test_in_a_captured_graph_replayed_twice():
    torch = torch_device()
    rows, cols = 33, 65
    color, history, cur, prev = case_data(rows, cols)
    (gc, keep_c), (gp, keep_p) = device_guides(cur, True), device_guides(prev, True)
    d_color, d_motion, d_history = dev(color).view(rows, cols, 3), dev(motion_field(rows, cols, "fractional")).view(rows, cols, 2), dev(history)
    out, var = torch.zeros_like(d_history), torch.zeros((rows, cols), dtype=torch.float32, device="cuda")
    want = cpu_result(rows, cols, "fractional", True)
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):  # one stream, one launch: a linear graph
            temporal.accumulate(d_color, d_motion, rows, cols, d_history, gc, gp, out=out, variance=var, stream=stream, **PARAMS)
    torch.cuda.synchronize()
    for _ in range(2):
        out.zero_()  # capturing ran nothing; every replay writes every record again
        var.fill_(-1.0)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(bits(out.cpu().numpy()), want[0]) and np.array_equal(bits(var.cpu().numpy().reshape(-1)), want[1])


# ---- end to end on the reference scene at 64 x 48 ----

def surfaces_numpy(s):
    hits, surfaces = s.hits.cpu().numpy().view(F32), s.surfaces.cpu().numpy().view(F32)
    return temporal.Guides(surfaces[:, NORMAL_AT:NORMAL_AT + 3], hits[:, POSITION_AT:POSITION_AT + 3], hits.view(np.uint32)[:, OBJECT_AT],
                           surfaces.view(np.uint32)[:, VALID_AT])


@functools.lru_cache(maxsize=None)
def reference_frame():
    torch = torch_device()
    scene, cam, frame = rt.Scene(rt.reference_world()), rt.reference_camera(), rt.Frame.full(64, 48, 3)
    clean = rt.render_whitted(scene, cam, frame)
    torch.cuda.synchronize()
    return scene, cam, frame, clean.cpu().numpy()


def noisy_frames(clean, k):
    g = np.random.default_rng(21)
    return [(clean + g.normal(0.0, 0.2, clean.shape).astype(F32)).astype(F32) for _ in range(k)]


def run_sequence(cameras, stream=None):
    """accumulate_frame over the cameras; per frame the downloaded records, variance, motion, and the guides of the frame as numpy views"""
    torch = torch_device()
    scene, _, frame, clean = reference_frame()
    history = temporal.History(frame.rows, frame.cols)
    frames = []
    for cam, image in zip(cameras, noisy_frames(clean, len(cameras))):
        d_image = dev(image)
        torch.cuda.synchronize()  # the upload and the History's zeros are on the default stream
        color, variance, length = temporal.accumulate_frame(scene, cam, frame, d_image, history, stream=stream)
        torch.cuda.synchronize()
        records = history.records.cpu().numpy().view(HISTORY).reshape(-1)
        assert np.array_equal(bits(color.cpu().numpy().reshape(-1, 3)), bits(records["color"])) and np.array_equal(length.cpu().numpy().reshape(-1), records["length"])
        frames.append(dict(image=image, records=records, variance=variance.cpu().numpy().copy(), motion=history.motion.cpu().numpy().copy(),
                           guides=surfaces_numpy(history._previous[0]), camera=cam))
    return frame, clean, frames


def check_against_the_cpu_path(frame, frames):
    """every frame's motion, records and variance equal the numpy path fed the same device-produced guides and the previous records"""
    rows, cols = frame.rows, frame.cols
    previous = np.zeros(rows * cols, dtype=HISTORY)
    for k, f in enumerate(frames):
        before = frames[k - 1] if k else f  # the first push reprojects into itself and finds an empty history
        m = temporal.motion_numpy(f["guides"].position, before["camera"], frame, valid=f["guides"].valid)
        assert np.array_equal(bits(m), bits(f["motion"])), k
        want, var = temporal.accumulate_numpy(f["image"], m, rows, cols, previous, f["guides"], before["guides"])
        assert np.array_equal(bits(want.reshape(-1)), bits(f["records"])) and np.array_equal(bits(var), bits(f["variance"])), k
        previous = f["records"]


def test_accumulate_frame_over_three_frames_of_a_static_camera():
    _, cam, _, _ = reference_frame()
    frame, clean, frames = run_sequence([cam] * 3, stream=torch_device().cuda.Stream())
    check_against_the_cpu_path(frame, frames)
    valid = frames[0]["guides"].valid != 0
    assert valid.any() and (~valid).any()
    assert (frames[0]["records"]["length"] == 1).all() and not frames[0]["variance"].any()  # the first push is all resets
    for k in (1, 2):  # the own tap is always accepted: column 0 and row 0 included
        assert (frames[k]["records"]["length"][valid] == k + 1).all(), k
        assert (frames[k]["records"]["length"][~valid] == 1).all(), k
    mse = [float(((f["records"]["color"].astype(np.float64) - clean.reshape(-1, 3)) ** 2)[valid].mean()) for f in frames]
    print(f"temporal: mse against the clean frame, frames 1..3: {mse[0]:.6g} {mse[1]:.6g} {mse[2]:.6g}; ratio frame 3 / frame 1 {mse[2] / mse[0]:.4f}")
    assert mse[2] < mse[0]


def test_a_moved_camera_resets_what_it_must():
    _, cam, _, _ = reference_frame()
    moved = rt.Camera.from_buffer_copy(cam)
    toward, up = np.array(list(cam.toward), dtype=np.float64), np.array(list(cam.up), dtype=np.float64)
    right = np.cross(toward, up)
    right /= np.linalg.norm(right)
    for k in range(3):
        moved.center[k] = cam.center[k] + 0.3 * right[k]
    frame, _, frames = run_sequence([cam, moved])
    check_against_the_cpu_path(frame, frames)
    rows, cols = frame.rows, frame.cols
    length = frames[1]["records"]["length"]
    valid = frames[1]["guides"].valid != 0
    assert (length[valid] == 1).any() and (length == 2).any()
    # a pixel whose four taps all carry another object index must reset
    m = frames[1]["motion"].reshape(-1, 2)
    ok = np.isfinite(m).all(axis=1)
    fx, fy = np.floor(np.where(ok, m[:, 0], 0)).astype(np.int64), np.floor(np.where(ok, m[:, 1], 0)).astype(np.int64)
    own, before = frames[1]["guides"].object, frames[0]["guides"].object.reshape(rows, cols)
    other = ok.copy()
    for j in (0, 1):
        for i in (0, 1):
            x, y = fx + i, fy + j
            inside = (x >= 0) & (x < cols) & (y >= 0) & (y < rows)
            other &= ~inside | (before[np.clip(y, 0, rows - 1), np.clip(x, 0, cols - 1)] != own)
    print(f"temporal: moved camera: {int((length[valid] == 1).sum())} of {int(valid.sum())} valid pixels reset, {int((other & valid).sum())} of them with "
          "another object at all four taps")
    assert (length[other] == 1).all()
