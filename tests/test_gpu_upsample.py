"""The guided upsampling queries on the device against the CPU definition, with no tolerance: both kernel forms, the grid free and capped
to one workgroup that strides every tile, at output sizes whose tile windows stick out of the low image on all four sides and whose
tiles are partial; through the _host form; on a stream and in a captured graph; and upsample.render_upsampled on the reference scene.
The reference result of a case is computed once and shared."""
import ctypes as C
import functools

import numpy as np
import pytest

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import _capi, upsample
from homework_18_graphics_raytracer_amd.upsample import Guides
from _records import spread, torch_device
import _upsample_support as S

pytestmark = pytest.mark.gpu

F32 = np.float32
SIZES = [(1, 1), (2, 2), (15, 15), (16, 16), (17, 17), (16, 33), (31, 18), (48, 40)]
FORM, CAP = "RT_AMD_UPSAMPLE_FORM", "RT_AMD_DIAG_UPSAMPLE_MAX_GROUPS"
VARIANTS = [(True, 3), (True, 0), (False, 3), (False, 0)]  # (object planes, demodulation flags)
KW = dict(sigma_normal=S.FINITE_SIGMAS[0], sigma_position=S.FINITE_SIGMAS[1])


def dev(a):
    a = np.array(a)
    return torch_device().from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def host(t):
    torch_device().cuda.synchronize()
    return t.cpu().numpy()


def planes(rows, cols, s):
    """(colour, [normal, position, albedo, valid, object] of the low image, the same of the output)"""
    color, *lo = S.case_data(S.low(rows, s), S.low(cols, s), seed=11 + s)
    _, *hi = S.case_data(rows, cols)
    return color, lo, hi


def pick(g, objects):
    return Guides(*g[:4], g[4] if objects else None)


@functools.lru_cache(maxsize=None)
def want(rows, cols, s, radius, objects, flags):
    color, lo, hi = planes(rows, cols, s)
    out = upsample.guided_numpy(color, rows, cols, low=pick(lo, objects), full=pick(hi, objects), scale=s, radius=radius, demodulate=flags, **KW)
    out.setflags(write=False)
    return out


def record_views(g):
    """the planes inside 13- and 18-word records on the device, as primary_surfaces' views lie"""
    torch = torch_device()
    hits, surfaces = np.full((g[0].shape[0], S.HIT_WORDS), 123.25, dtype=F32), np.full((g[0].shape[0], S.SURFACE_WORDS), -7.5, dtype=F32)
    hits[:, S.POSITION_AT:S.POSITION_AT + 3] = g[1]
    hits.view(np.uint32)[:, S.OBJECT_AT] = g[4]
    surfaces[:, S.NORMAL_AT:S.NORMAL_AT + 3], surfaces[:, S.ALBEDO_AT:S.ALBEDO_AT + 3] = g[0], g[2]
    surfaces.view(np.uint32)[:, S.VALID_AT] = g[3]
    h, sf = dev(hits), dev(surfaces)
    return [sf[:, S.NORMAL_AT:S.NORMAL_AT + 3], h[:, S.POSITION_AT:S.POSITION_AT + 3], sf[:, S.ALBEDO_AT:S.ALBEDO_AT + 3], sf.view(torch.int32)[:, S.VALID_AT],
            h.view(torch.int32)[:, S.OBJECT_AT]]


@pytest.mark.parametrize("cap", [None, 1])
@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("radius", [1, 2])
@pytest.mark.parametrize("s", S.SCALES)
@pytest.mark.parametrize("rows,cols", SIZES)
def test_the_device_equals_the_cpu_definition(rows, cols, s, radius, form, cap):
    """the guides strided views of records, the colour inside 8-word records; cap 1: one workgroup strides every tile"""
    color, lo, hi = planes(rows, cols, s)
    records = np.full((color.shape[0], 8), 3.5, dtype=F32)
    records[:, :3] = color
    d_color, d_lo, d_hi = dev(records)[:, :3], record_views(lo), record_views(hi)
    with rt.options(**{FORM: form}, **({CAP: cap} if cap else {})):
        for objects, flags in VARIANTS:
            got = upsample.guided(d_color, rows, cols, low=pick(d_lo, objects), full=pick(d_hi, objects), scale=s, radius=radius, demodulate=flags, **KW)
            assert np.array_equal(S.bits(host(got)), S.bits(want(rows, cols, s, radius, objects, flags))), (objects, flags)


@pytest.mark.parametrize("form", [0, 1])
def test_the_edges_of_the_host_tests_on_the_device(form):
    """an invalid output pixel and a source that is not finite: the raw words with a NaN's payload, on both forms"""
    rows, cols, s = 17, 33, 2
    color, lo, hi = planes(rows, cols, s)
    color, valid = np.array(color), np.array(hi[3])
    cl = S.low(cols, s)
    color.view(np.uint32)[3 * cl + 8] = (0x7FC12345, 0xFFC00001, 0x7F800000)
    color[5 * cl + 2, 1] = np.inf
    valid[6 * cols + 17] = 0  # nearest: low (3, 8)
    hi = hi[:3] + [valid] + hi[4:]
    with rt.options(**{FORM: form}):
        for radius in (1, 2):
            expect = upsample.guided_numpy(color, rows, cols, low=Guides(*lo), full=Guides(*hi), scale=s, radius=radius, demodulate=True, **KW)
            got = host(upsample.guided(dev(color), rows, cols, low=Guides(*(dev(a) for a in lo)), full=Guides(*(dev(a) for a in hi)), scale=s, radius=radius,
                                       demodulate=True, **KW))
            assert np.array_equal(S.bits(got), S.bits(expect))
            assert np.array_equal(S.bits(got[6, 17]), np.array([0x7FC12345, 0xFFC00001, 0x7F800000], dtype=np.uint32))


@pytest.mark.parametrize("rows,cols,s,radius", [(1, 1, 2, 1), (17, 17, 3, 2), (31, 18, 4, 2), (48, 40, 2, 1)])
def test_the_host_form_equals_the_device(rows, cols, s, radius):
    color, lo, hi = planes(rows, cols, s)
    held = [np.array(a) for a in [color] + lo + hi]  # the call takes their addresses
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    g_lo = _capi.DenoiseGuides(*(a.ctypes.data for a in held[1:5]), 3, 3, 3, 1)
    g_hi = _capi.DenoiseGuides(*(a.ctypes.data for a in held[6:10]), 3, 3, 3, 1)
    p = _capi.UpsampleParams(KW["sigma_normal"], KW["sigma_position"], s, radius, 3)
    out = np.zeros((rows, cols, 3), dtype=F32)
    _capi.check(_capi.amd_lib().rt_upsample_guided_host(ptr(held[0]), 3, C.byref(g_lo), ptr(held[5]), 1, C.byref(g_hi), ptr(held[10]), 1, C.byref(p), rows, cols,
                                                        ptr(out)))
    got = upsample.guided(dev(color), rows, cols, low=Guides(*(dev(a) for a in lo)), full=Guides(*(dev(a) for a in hi)), scale=s, radius=radius, **KW)
    assert np.array_equal(S.bits(out), S.bits(host(got))) and np.array_equal(S.bits(out), S.bits(want(rows, cols, s, radius, True, 3)))


def test_the_host_form_stages_every_strided_plane_to_its_last_word():
    """17 x 19 at scale 2 — partial tiles, a 9 x 10 low image — with EVERY plane a strided record view, 11 or 13 words apart, in a host
    array of exactly (n - 1) * stride + width words: a staged span one pixel short would lose the last pixel, which the compact planes
    of the test above cannot show"""
    rows, cols, s, radius = 17, 19, 2, 2
    color, lo, hi = planes(rows, cols, s)
    assert (S.low(rows, s), S.low(cols, s)) == (9, 10)
    held = [spread(color, 13)] + [spread(a, k) for a, k in zip(lo, (11, 13, 11, 13, 11))] + [spread(a, k) for a, k in zip(hi, (13, 11, 13, 11, 13))]
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    g_lo = _capi.DenoiseGuides(*(a.ctypes.data for a in held[1:5]), 11, 13, 11, 13)
    g_hi = _capi.DenoiseGuides(*(a.ctypes.data for a in held[6:10]), 13, 11, 13, 11)
    p = _capi.UpsampleParams(KW["sigma_normal"], KW["sigma_position"], s, radius, 3)
    out = np.zeros((rows, cols, 3), dtype=F32)
    _capi.check(_capi.amd_lib().rt_upsample_guided_host(ptr(held[0]), 13, C.byref(g_lo), ptr(held[5]), 11, C.byref(g_hi), ptr(held[10]), 13, C.byref(p), rows, cols,
                                                        ptr(out)))
    expect = S.bits(want(rows, cols, s, radius, True, 3)).reshape(rows, cols, 3)  # the _cpu form on the same values
    assert np.array_equal(S.bits(out)[-1, -1], expect[-1, -1])
    assert np.array_equal(S.bits(out), expect)


def test_on_a_stream_and_in_a_captured_graph():
    """one call on a stream of its own without a synchronisation after the upload's; then the call captured — one kernel node — and
    replayed twice on new colours"""
    torch = torch_device()
    rows, cols, s, radius = 48, 40, 2, 2
    _, lo, hi = planes(rows, cols, s)
    colours = [S.case_data(S.low(rows, s), S.low(cols, s), seed=k)[0] for k in (41, 42, 43)]
    g_lo, g_hi = Guides(*(dev(a) for a in lo)), Guides(*(dev(a) for a in hi))
    d_color = dev(colours[0])
    out = torch.zeros((rows, cols, 3), dtype=torch.float32, device="cuda")
    stream = torch.cuda.Stream()

    def call():
        assert upsample.guided(d_color, rows, cols, low=g_lo, full=g_hi, scale=s, radius=radius, out=out, stream=stream, **KW) is out

    def check(color):
        expect = upsample.guided_numpy(color, rows, cols, low=Guides(*lo), full=Guides(*hi), scale=s, radius=radius, **KW)
        assert np.array_equal(S.bits(host(out)), S.bits(expect))

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
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            graph.replay()
        check(color)


def _block_centre_rays(cam, frame, s):
    """the rays of the FULL frame through the centres of its s x s blocks: pixel (s i, s j) with the offset (s - 1) / 2, for every block"""
    torch = torch_device()
    offsets = torch.full((1, frame.rows * frame.cols, 2), (s - 1) / 2, dtype=torch.float32, device="cuda")
    rays = rt.film.camera_rays_offset(cam, frame, offsets).view(frame.rows, frame.cols, 11)
    return rays[::s, ::s].reshape(-1, 11)


@pytest.mark.parametrize("s", S.SCALES)
def test_the_low_rays_go_through_the_block_centres(s):
    """Registration: low pixel j must look at output coordinate j s + (s - 1) / 2, where step 2 of the definition places it — not at
    j s, where the low frame's own integer coordinate looks.  For s = 2 and 4 every operand of the clip coordinate scales by a power of
    two, so the low rays equal the full frame's rays through the block centres bit for bit.  For s = 3 the offset 1/3 and the sum
    j + 1/3 round: the image position is off by at most ulp(16) / 2 + ulp(1/3) / 2 < 2^-20 low pixels for j < 16, the clip coordinate
    (a divide by the low height 16 and a subtraction, one rounding each, values below 1) by less than 2^-20 / 16 + 2 * 2^-24 < 2^-22, and
    a component of the unit direction (three products, two sums, a normalisation: a handful of roundings below 1) by less than
    2^-22 + 8 * 2^-24 < 2^-20.  A ray that were shot through j s instead would be (s - 1) / 2 pixels of 1 / (16 s) clip units away, at
    least 2^-6 clip units: with any field of view above a degree its direction differs by more than 2^-12, 256 times the tolerance."""
    torch = torch_device()
    cam, frame = rt.reference_camera(), rt.Frame.full(16 * s, 16 * s, 5)
    lo, rays = upsample.low_rays(cam, frame, s)
    assert (lo.width, lo.height, lo.max_depth) == (16, 16, 5) and tuple(rays.shape) == (256, 11)
    want = _block_centre_rays(cam, frame, s)
    torch.cuda.synchronize()
    got, want = rays.cpu().numpy(), want.cpu().numpy()
    assert np.array_equal(got[:, [0, 1, 2, 6, 7, 8, 9, 10]], want[:, [0, 1, 2, 6, 7, 8, 9, 10]])  # origin, face, no exclusion
    d_got, d_want = got[:, 3:6].view(F32), want[:, 3:6].view(F32)
    worst = float(np.abs(d_got.astype(np.float64) - d_want).max())
    unshifted = float(np.abs(rt.camera_rays(cam, lo).cpu().numpy()[:, 3:6].view(F32).astype(np.float64) - d_want).max())
    print(f"s={s}: direction of the low rays against the block centres' {worst:.3e}; of the low frame's own rays {unshifted:.3e}")
    if s in (2, 4):
        assert np.array_equal(S.bits(d_got), S.bits(d_want))
    else:
        assert worst < 2.0 ** -20
    assert unshifted > 2.0 ** -12  # the check sees a low image that is not registered


def test_render_upsampled_on_the_reference_scene():
    """64 x 48, depth 5, scale 2: the device sequence equals the CPU definition on the downloaded inputs bit for bit; its low surfaces
    and radiance are those of the full frame's rays through the block centres; and the result is closer to the full-resolution Whitted
    frame than nearest replication of the low image.

    Measured on an MI355X when this test was written: mean squared error against the full-resolution frame, guided 1.0458e-2, nearest
    replication 1.8841e-2.  Printed and NOT asserted: the same upsample of a low frame rendered through its own integer coordinates,
    half an output pixel off, 1.0266e-2 — lower than the registered one's.  At scale 2 that unregistered low image is a bit-exact subset
    of the point-sampled frame it is compared with (low pixel (i, j) IS full pixel (2 i, 2 j)), while the registered samples lie between
    four full pixels, and at 64 x 48 the frame is aliased enough for that to outweigh half a pixel; against the mean of 16 sub-pixel
    samples per pixel the order is the other way (7.79e-3 against 8.05e-3), and so it is against the point-sampled frame at 96 x 72
    and 192 x 144.  The comparison that isolates the registration is the next test's (DESIGN.md 3.28 has all figures)."""
    torch = torch_device()
    scene, cam, frame = rt.Scene(rt.reference_world()), rt.reference_camera(), rt.Frame.full(64, 48, 5)
    rows, cols, s = frame.rows, frame.cols, 2
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    image, radiance, s_lo, s_hi = upsample.render_upsampled(scene, cam, frame, scale=s, stream=stream)
    torch.cuda.synchronize()
    assert tuple(image.shape) == (rows, cols, 3) and tuple(radiance.shape) == (rows // s, cols // s, 3)
    centres = _block_centre_rays(cam, frame, s)
    assert torch.equal(s_lo.rays, centres) and torch.equal(s_lo.hits, rt.cast_rays(scene, centres))
    assert torch.equal(radiance.view(-1, 3).view(torch.int32), rt.trace_rays(scene, centres, frame.max_depth).view(torch.int32))

    def cpu_guides(p):
        hits, surfaces = p.hits.cpu().numpy(), p.surfaces.cpu().numpy()
        hf, sf = hits.view(F32), surfaces.view(F32)
        return Guides(sf[:, S.NORMAL_AT:S.NORMAL_AT + 3], hf[:, S.POSITION_AT:S.POSITION_AT + 3], sf[:, S.ALBEDO_AT:S.ALBEDO_AT + 3],
                      surfaces.view(np.uint32)[:, S.VALID_AT], hits.view(np.uint32)[:, S.OBJECT_AT])

    low = radiance.cpu().numpy()
    expect = upsample.guided_numpy(low.reshape(-1, 3), rows, cols, low=cpu_guides(s_lo), full=cpu_guides(s_hi), scale=s)
    assert np.array_equal(S.bits(image.cpu().numpy()), S.bits(expect))
    truth = rt.render_whitted(scene, cam, frame)
    lo_frame = upsample.low_frame(frame, s)
    off = rt.materials.primary_surfaces(scene, cam, lo_frame)
    shifted = upsample.guided(rt.render_whitted(scene, cam, lo_frame), rows, cols, low=Guides.of(off), full=Guides.of(s_hi), scale=s)
    torch.cuda.synchronize()
    truth = truth.cpu().numpy().astype(np.float64)
    mse = lambda img: float(((img.astype(np.float64) - truth) ** 2).mean())
    e_guided, e_nearest, e_shifted = mse(expect), mse(S.nearest(low, rows, cols, s)), mse(shifted.cpu().numpy())
    print(f"mse against the full-resolution frame: guided {e_guided:.6e}, nearest {e_nearest:.6e}, guided on an unregistered low frame {e_shifted:.6e}")
    assert e_guided < e_nearest


def test_registration_decides_where_both_low_images_are_samples_of_the_frame():
    """96 x 72, depth 5, scale 3.  At an odd scale the block centres are pixels of the full frame: the registered low image is the
    frame's pixels (3 i + 1, 3 j + 1), and a low frame rendered through its own integer coordinates is its pixels (3 i, 3 j).  Both are
    samples of the frame they are compared with, neither is filtered, both are upsampled onto the same full guides by the same call:
    what differs is only whether a sample is placed where it was taken or one output pixel away.  So the registered one must be closer.
    Measured on an MI355X when this test was written: 9.841e-3 against 1.4125e-2."""
    torch = torch_device()
    scene, cam, frame = rt.Scene(rt.reference_world()), rt.reference_camera(), rt.Frame.full(96, 72, 5)
    rows, cols, s = frame.rows, frame.cols, 3
    image, radiance, s_lo, s_hi = upsample.render_upsampled(scene, cam, frame, scale=s)
    truth = rt.render_whitted(scene, cam, frame)
    lo_frame = upsample.low_frame(frame, s)
    own = rt.render_whitted(scene, cam, lo_frame)
    shifted = upsample.guided(own, rows, cols, low=Guides.of(rt.materials.primary_surfaces(scene, cam, lo_frame)), full=Guides.of(s_hi), scale=s)
    torch.cuda.synchronize()
    t = truth.cpu().numpy()
    taken = t[1::s, 1::s]  # where the registered samples were taken: the same pixels up to the rounding of j + 1/3
    close = np.isclose(radiance.cpu().numpy(), taken, rtol=1e-3, atol=1e-3).all(axis=-1).mean()
    assert close > 0.95, close  # silhouettes may fall on the other side of an edge
    assert np.array_equal(S.bits(own.cpu().numpy()), S.bits(t[::s, ::s]))
    mse = lambda img: float(((img.cpu().numpy().astype(np.float64) - t) ** 2).mean())
    e_registered, e_shifted = mse(image), mse(shifted)
    print(f"mse against the full-resolution frame at scale 3: registered {e_registered:.6e}, one output pixel off {e_shifted:.6e}")
    assert e_registered < e_shifted
