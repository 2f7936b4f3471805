"""The history rectification queries on the device against the CPU definition, with no tolerance: the box tile kernel at the sizes where a
tile can go wrong, at every radius, with the grid capped to one workgroup that strides every tile; the two per-pixel kernels at batch
sizes around a wave and a workgroup; on a stream, in a captured graph, through the _host forms; and rectify.filter_frame on the
reference scene with a light that moves between two frames.  A NaN that went through arithmetic is compared as "a NaN"."""
import ctypes as C

import numpy as np
import pytest

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import _capi, rectify, svgf, temporal
from _denoise_support import record_views
from _records import spread, torch_device
import _rectify_support as S
from _temporal_support import F32, HISTORY, PARAMS, case_data as temporal_case, embed as embed_guides, motion_field

pytestmark = pytest.mark.gpu

TILE_IMAGES = [(1, 1), (15, 15), (16, 16), (17, 17), (16, 33), (33, 16), (48, 40)]
BATCHES = [1, 63, 64, 65, 255, 256, 257, 4099]
OPTION = "RT_AMD_DIAG_RECTIFY_MAX_GROUPS"


def dev(a):
    a = np.array(a)
    if a.dtype in (HISTORY, S.BOX):
        a = a.view(np.uint32).reshape(-1, 8)
    return torch_device().from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def dev_box(box):
    return torch_device().from_numpy(np.array(box).view(F32).reshape(-1, 8)).cuda()


def guides(p):
    return temporal.Guides(p.normal, p.position, p.object, p.valid)


def dev_guides(p):
    return temporal.Guides(dev(p.normal), dev(p.position), dev(p.object), dev(p.valid))


def host(t):
    torch_device().cuda.synchronize()
    return t.cpu().numpy()


# ---- rt_temporal_bounds: the tile kernel ----

@pytest.mark.parametrize("cap", [None, 1])
@pytest.mark.parametrize("radius", S.RADII)
@pytest.mark.parametrize("rows,cols", TILE_IMAGES)
def test_bounds_equal_the_cpu_definition(rows, cols, radius, cap):
    """compact planes and strided record views, with and without the object and valid planes; cap 1: one workgroup strides every tile"""
    color, obj, valid = S.case_data(rows, cols)
    rec, _ = S.embed(color, obj, valid)
    d_rec = dev(rec)
    d_views = (d_rec[:, 1:4], d_rec.view(torch_device().int32)[:, 6], d_rec.view(torch_device().int32)[:, 9])
    with rt.options(**({OPTION: cap} if cap else {})):
        for planes in ("both", "object", "none"):
            o, v = (obj if planes != "none" else None), (valid if planes == "both" else None)
            want = rectify.bounds_numpy(color, rows, cols, object=o, valid=v, gamma=1.25, radius=radius)
            got = rectify.bounds(dev(color), rows, cols, object=None if o is None else dev(o), valid=None if v is None else dev(v), gamma=1.25, radius=radius)
            assert S.same_or_both_nan(host(got), want), planes
            got = rectify.bounds(d_views[0], rows, cols, object=None if o is None else d_views[1], valid=None if v is None else d_views[2], gamma=1.25,
                                 radius=radius)
            assert S.same_or_both_nan(host(got), want), planes


@pytest.mark.parametrize("radius", S.RADII)
def test_bounds_of_a_ragged_image_with_a_checkerboard_of_sources_under_one_workgroup(radius):
    """the halo stager, its ring and the image's edge together: 17 x 33 is 2 x 3 tiles whose last row and column are one pixel wide, one
    workgroup strides all six, every second source is cleared and the object changes across the tile border at column 16"""
    rows, cols = 17, 33
    color = S.case_data(rows, cols)[0]
    r, c = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    valid = ((r + c) % 2 == 0).reshape(-1).astype(np.uint32)
    obj = (c >= 16).reshape(-1).astype(np.uint32)
    want = rectify.bounds_numpy(color, rows, cols, object=obj, valid=valid, gamma=1.25, radius=radius)
    with rt.options(**{OPTION: 1}):
        got = rectify.bounds(dev(color), rows, cols, object=dev(obj), valid=dev(valid), gamma=1.25, radius=radius)
        assert S.same_or_both_nan(host(got), want)


# ---- rt_temporal_accumulate_bounded and rt_temporal_feedback: one thread per pixel ----

@pytest.mark.parametrize("cap", [None, 1])
@pytest.mark.parametrize("n", BATCHES)
def test_the_per_pixel_kernels_equal_the_cpu_definition(n, cap):
    """images of one row: 1, a wave and a workgroup plus or minus one, and 4099 pixels; the guides strided views of 13- and 18-word records"""
    rows, cols = 1, n
    color, history, cur, prev = temporal_case(rows, cols)
    motion = motion_field(rows, cols, "fractional")
    box = rectify.bounds_numpy(color, rows, cols, object=cur.object, valid=cur.valid, gamma=0.5, radius=1)
    want = rectify.accumulate_bounded_numpy(color, motion, rows, cols, history, box, guides(cur), guides(prev), clamped_length=2, **PARAMS)
    fed_want = rectify.feedback_numpy(color, want[0], rows, cols, valid=cur.valid)
    torch = torch_device()
    views = []
    for p in (cur, prev):
        hits, surfaces, _ = embed_guides(p)
        h, s = dev(hits), dev(surfaces)
        views.append(temporal.Guides(s[:, 14:17], h[:, 3:6], h.view(torch.int32)[:, 2], s.view(torch.int32)[:, 17]))
    with rt.options(**({OPTION: cap} if cap else {})):
        rec, var, clamped = rectify.accumulate_bounded(dev(color).view(rows, cols, 3), dev(motion).view(rows, cols, 2), rows, cols, dev(history), dev_box(box),
                                                       views[0], views[1], clamped_length=2, **PARAMS)
        assert S.same_or_both_nan(host(rec), want[0]) and S.same_or_both_nan(host(var), want[1])
        assert np.array_equal(host(clamped).view(np.uint32), want[2])
        fed = rectify.feedback(dev(color), rec, rows, cols, valid=views[0].valid)
        assert fed is rec and S.same_or_both_nan(host(fed), fed_want)
    if n >= 255:
        assert want[2].any() and (want[0]["length"] == 2).any()


def test_infinite_boxes_give_the_bits_of_accumulate():
    rows, cols = 17, 33
    color, history, cur, prev = temporal_case(rows, cols)
    motion = motion_field(rows, cols, "fractional")
    args = (dev(color).view(rows, cols, 3), dev(motion).view(rows, cols, 2), rows, cols, dev(history))
    plain, plain_var = temporal.accumulate(*args, dev_guides(cur), dev_guides(prev), **PARAMS)
    rec, var, clamped = rectify.accumulate_bounded(*args, dev_box(S.infinite_boxes(rows * cols)), dev_guides(cur), dev_guides(prev), clamped_length=2, **PARAMS)
    assert np.array_equal(S.bits(host(rec)), S.bits(host(plain))) and np.array_equal(S.bits(host(var)), S.bits(host(plain_var)))
    assert not host(clamped).any()


# ---- the stream, the graph, the _host forms ----

def test_on_a_stream_and_in_a_captured_graph():
    """no synchronisation between the three calls on a stream of their own; then {bounds, accumulate_bounded, feedback} captured — a
    linear chain, one stream, no parallel branches — and replayed twice on new colour"""
    torch = torch_device()
    rows, cols = 48, 40
    n = rows * cols
    _, history, cur, prev = temporal_case(rows, cols)
    motion = motion_field(rows, cols, "fractional")
    colours = [S.case_data(rows, cols, seed=s)[0] for s in (29, 30, 31)]

    def cpu(color):
        box = rectify.bounds_numpy(color, rows, cols, object=cur.object, valid=cur.valid)
        rec, var, clamped = rectify.accumulate_bounded_numpy(color, motion, rows, cols, history, box, guides(cur), guides(prev), **PARAMS)
        return rectify.feedback_numpy(color * F32(0.5), rec, rows, cols, valid=cur.valid), var, clamped

    g_cur, g_prev = dev_guides(cur), dev_guides(prev)
    d_color, d_half = dev(colours[0]).view(rows, cols, 3), dev(colours[0] * F32(0.5))
    d_motion, d_history = dev(motion).view(rows, cols, 2), dev(history)
    box = torch.zeros((n, 8), dtype=torch.float32, device="cuda")
    rec, var = torch.zeros((n, 8), dtype=torch.int32, device="cuda"), torch.zeros((rows, cols), dtype=torch.float32, device="cuda")
    clamped = torch.zeros((rows, cols), dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()

    def chain():
        rectify.bounds(d_color, rows, cols, object=g_cur.object, valid=g_cur.valid, out=box, stream=stream)
        rectify.accumulate_bounded(d_color, d_motion, rows, cols, d_history, box, g_cur, g_prev, out=rec, variance=var, clamped=clamped, stream=stream, **PARAMS)
        rectify.feedback(d_half, rec, rows, cols, valid=g_cur.valid, stream=stream)

    def check(color):
        want = cpu(color)
        assert S.same_or_both_nan(host(rec), want[0]) and S.same_or_both_nan(host(var), want[1]) and np.array_equal(host(clamped).view(np.uint32), want[2])

    torch.cuda.synchronize()
    chain()
    check(colours[0])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            chain()
    torch.cuda.synchronize()
    for color in colours[1:]:
        d_color.copy_(dev(color).view(rows, cols, 3))
        d_half.copy_(dev(color * F32(0.5)))
        for t in (box, rec, var, clamped):  # capturing ran nothing; every replay writes the whole planes again
            t.zero_()
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            graph.replay()
        check(color)


# ---- the host cases of tests/test_rectify_host.py on the device and through the _host forms ----

PAYLOAD_NAN = np.uint32(0x7FC12345)  # a NaN that a raw copy must keep word for word


def ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


@pytest.mark.parametrize("radius", S.RADII)
@pytest.mark.parametrize("planes", ["both", "object", "valid", "none"])
@pytest.mark.parametrize("rows,cols", S.IMAGES)
def test_bounds_on_the_host_cases(rows, cols, planes, radius):
    """1 x 1, 1 x 17, 17 x 1 (a whole halo row or column outside the image), 16 x 16, 17 x 33: the device form on compact planes and the
    _host form on strided record views against the CPU form"""
    color, obj, valid = (np.array(a) for a in S.case_data(rows, cols))  # held: the _host call takes their addresses
    o, v = (obj if planes in ("both", "object") else None), (valid if planes in ("both", "valid") else None)
    want = rectify.bounds_numpy(color, rows, cols, object=o, valid=v, gamma=1.25, radius=radius)
    got = rectify.bounds(dev(color), rows, cols, object=None if o is None else dev(o), valid=None if v is None else dev(v), gamma=1.25, radius=radius)
    assert S.same_or_both_nan(host(got), want)
    rec, (c, ro, rv) = S.embed(color, obj, valid)
    box = np.zeros(rows * cols, dtype=S.BOX)
    p = _capi.BoundsParams(1.25, radius, 0)
    _capi.check(_capi.amd_lib().rt_temporal_bounds_host(ptr(c), 11, ptr(ro if o is not None else None), 11, ptr(rv if v is not None else None), 11,
                                                        C.byref(p), rows, cols, ptr(box)))
    assert S.same_or_both_nan(box, want)


@pytest.mark.parametrize("with_valid", [False, True])
@pytest.mark.parametrize("clamped_length", [0, 2])
@pytest.mark.parametrize("field", ["integer", "fractional", "special3"])
@pytest.mark.parametrize("rows,cols", S.IMAGES)
def test_accumulate_bounded_and_feedback_on_the_host_cases(rows, cols, field, clamped_length, with_valid):
    """the device forms and the _host forms against the CPU forms; and the raw copies word for word: a reset's colour and a fed record's
    colour keep the payload of a NaN"""
    n = rows * cols
    color, history, cur, prev = temporal_case(rows, cols)
    color, history = np.array(color), np.array(history)
    color.view(np.uint32)[::37, 1] = PAYLOAD_NAN
    motion = np.array(motion_field(rows, cols, field))
    planes = [[np.array(a) for a in (p.normal, p.position, p.object, p.valid)] for p in (cur, prev)]  # held
    if not with_valid:
        planes[0][3] = planes[1][3] = None
    valid = planes[0][3]
    box = rectify.bounds_numpy(color, rows, cols, object=planes[0][2], valid=valid, gamma=0.5, radius=1).reshape(-1)
    want = rectify.accumulate_bounded_numpy(color, motion, rows, cols, history, box, temporal.Guides(*planes[0]), temporal.Guides(*planes[1]),
                                            clamped_length=clamped_length, **PARAMS)
    fed_want = rectify.feedback_numpy(color * F32(0.5), want[0], rows, cols, valid=valid)
    reset = want[0].reshape(-1)["length"] == 1  # max_length 4, clamped_length 0 or 2: a blended record is at least 2 long
    taken = np.ones(n, dtype=bool) if valid is None else valid != 0  # every written record has a length
    half = color * F32(0.5)  # a multiply by a power of two keeps a NaN's payload on this side; the copies below are compared with THIS array
    raw, raw_half = S.bits(color), S.bits(half)

    def check(rec, var, clamped, fed):
        assert S.same_or_both_nan(rec, want[0]) and S.same_or_both_nan(var, want[1]) and np.array_equal(clamped.reshape(-1), want[2].reshape(-1))
        assert np.array_equal(S.bits(rec).reshape(n, 8)[reset, :3], raw[reset])
        assert S.same_or_both_nan(fed, fed_want)
        assert np.array_equal(S.bits(fed).reshape(n, 8)[taken, :3], raw_half[taken])
        assert np.array_equal(S.bits(fed).reshape(n, 8)[:, 3:], S.bits(rec).reshape(n, 8)[:, 3:])

    device_guides = [temporal.Guides(*(None if a is None else dev(a) for a in g)) for g in planes]
    rec, var, clamped = rectify.accumulate_bounded(dev(color).view(rows, cols, 3), dev(motion).view(rows, cols, 2), rows, cols, dev(history), dev_box(box),
                                                   device_guides[0], device_guides[1], clamped_length=clamped_length, **PARAMS)
    rec_host = host(rec).copy()
    fed = rectify.feedback(dev(half), rec, rows, cols, valid=device_guides[0].valid)
    check(rec_host, host(var), host(clamped).view(np.uint32), host(fed))

    lib = _capi.amd_lib()
    g = [_capi.TemporalGuides(*(None if a is None else a.ctypes.data for a in q), 3, 3, 1, 1) for q in planes]
    tp = _capi.TemporalParams(PARAMS["normal_min"], PARAMS["position_max"], PARAMS["alpha_min"], PARAMS["max_length"], 0)
    out, var, clamped = np.zeros(n, dtype=HISTORY), np.zeros(n, dtype=F32), np.zeros(n, dtype=np.uint32)
    _capi.check(lib.rt_temporal_accumulate_bounded_host(ptr(color), ptr(motion), C.byref(g[0]), C.byref(g[1]), C.byref(tp), rows, cols, ptr(history),
                                                        ptr(out), ptr(var), ptr(box), clamped_length, ptr(clamped)))
    fed = out.copy()
    _capi.check(lib.rt_temporal_feedback_host(ptr(half), 3, ptr(valid), 1, rows, cols, ptr(fed)))
    check(out, var, clamped, fed)
    if (rows, cols, field) == (17, 33, "special3"):  # the case is not idle: payload NaNs among the resets and among the fed records
        assert (raw[reset] == PAYLOAD_NAN).any() and (raw_half[taken] == PAYLOAD_NAN).any() and (~reset).any()


def test_the_feedback_host_form_stages_strided_planes_to_their_last_word():
    """17 x 19, partial tiles: the colour 13 and the valid words 11 words apart, as strided record views lie, each in a host array of
    exactly (n - 1) * stride + width words — a staged span one pixel short would lose the last pixel, which the compact planes of the
    test above cannot show"""
    rows, cols = 17, 19
    n = rows * cols
    color, history, cur, _ = temporal_case(rows, cols)
    color, history, valid = np.array(color), np.array(history), np.array(cur.valid)
    valid[-1], history["length"][-1] = 1, 3  # the last record is fed
    want = rectify.feedback_numpy(color, history.copy(), rows, cols, valid=valid)  # the _cpu form on the same values
    c, v, fed = spread(color, 13), spread(valid, 11), history.copy()
    _capi.check(_capi.amd_lib().rt_temporal_feedback_host(ptr(c), 13, ptr(v), 11, rows, cols, ptr(fed)))
    assert np.array_equal(S.bits(fed).reshape(n, 8)[-1, :3], S.bits(color).reshape(n, 3)[-1])
    assert np.array_equal(S.bits(fed).reshape(n, 8), S.bits(want).reshape(n, 8))


# ---- end to end on the reference scene at 64 x 48: a light moves between two frames ----

def _frames(scene, cam, frame):
    """two rendered frames; between them the point light (the scene's third) moves — no geometry does"""
    torch = torch_device()
    world = rt.reference_world()  # held: the description points into it
    d = world.desc()
    first = rt.render_whitted(scene, cam, frame).clone()
    light = _capi.Light.from_buffer_copy(d.lights[2])
    light.origin[0] += 3.0
    light.origin[1] += 1.0
    light.origin[2] += 2.0
    scene.update_lights(2, [light])
    second = rt.render_whitted(scene, cam, frame).clone()
    scene.update_lights(2, [d.lights[2]])
    torch.cuda.synchronize()
    assert not torch.equal(first, second)
    return [first, second]


def test_filter_frame_on_the_reference_scene_with_a_moved_light():
    torch = torch_device()
    scene, cam, frame = rt.Scene(rt.reference_world()), rt.reference_camera(), rt.Frame.full(64, 48, 3)
    rows, cols = frame.rows, frame.cols
    images = _frames(scene, cam, frame)
    history, plain = temporal.History(rows, cols), temporal.History(rows, cols)
    records = np.zeros(rows * cols, dtype=HISTORY)
    stream = torch.cuda.Stream()
    kw = dict(levels=3)
    previous = None
    for k, image in enumerate(images):
        torch.cuda.synchronize()
        color, variance, clamped = rectify.filter_frame(scene, cam, frame, image, history, stream=stream, **kw)
        torch.cuda.synchronize()
        s = history._previous[0]
        hits, surfaces = s.hits.cpu().numpy(), s.surfaces.cpu().numpy()
        normal, position, albedo, valid = record_views(hits.view(F32), surfaces.view(F32))
        obj = hits.view(np.uint32)[:, 2]
        cur = temporal.Guides(normal, position, obj, valid)
        spatial = dict(normal=normal, position=position, valid=valid)
        img = image.cpu().numpy()
        motion = temporal.motion_numpy(position, cam, frame, valid=valid)
        box = rectify.bounds_numpy(img, rows, cols, object=obj, valid=valid)
        records, _, want_clamped = rectify.accumulate_bounded_numpy(img, motion, rows, cols, records, box, cur, previous or cur)
        v = svgf.variance_numpy(records, rows, cols, **spatial)
        level0, v0 = svgf.atrous_numpy(records["color"], v, rows, cols, levels=1, first_level=0, **spatial)
        records = rectify.feedback_numpy(level0, records, rows, cols, valid=valid)
        want_c, want_v = svgf.atrous_numpy(level0, v0, rows, cols, levels=2, first_level=1, **spatial)
        assert np.array_equal(S.bits(history.records.cpu().numpy().view(HISTORY).reshape(-1)), S.bits(records)), k
        assert np.array_equal(S.bits(color.cpu().numpy()), S.bits(want_c)) and np.array_equal(S.bits(variance.cpu().numpy()), S.bits(want_v)), k
        assert np.array_equal(clamped.cpu().numpy().view(np.uint32), want_clamped), k
        assert bool(want_clamped.any()) == (k == 1)  # the first frame resets everywhere; the moved light contradicts the history
        previous = cur
    # the same two frames with infinite boxes and no feedback: svgf.filter_frame, bit for bit
    bounded = temporal.History(rows, cols)
    inf_box = dev_box(S.infinite_boxes(rows * cols))
    for image in images:
        torch.cuda.synchronize()
        want_c, want_v = svgf.filter_frame(scene, cam, frame, image, plain, stream=stream, **kw)
        s = rt.materials.primary_surfaces(scene, cam, frame, stream=stream)
        c, _, _ = bounded.push(s, cam, frame, image, stream=stream, box=inf_box, clamped_length=rectify.CLAMPED_LENGTH)
        g = dict(normal=s.shading_normal, position=s.position, valid=s.valid)
        v = svgf.variance(bounded.records, rows, cols, stream=stream, **g)
        got_c, got_v = svgf.atrous(c, v, rows, cols, albedo=s.albedo, stream=stream, **g, **kw)
        torch.cuda.synchronize()
        assert torch.equal(bounded.records, plain.records)
        assert np.array_equal(S.bits(got_c.cpu().numpy()), S.bits(want_c.cpu().numpy())) and np.array_equal(S.bits(got_v.cpu().numpy()), S.bits(want_v.cpu().numpy()))
