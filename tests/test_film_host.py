"""Film queries on the host (include/rt_host.h rt_film_offsets_host / rt_film_splat_host, the CPU definition of include/rt_amd.h "film
queries"): the sample positions against a numpy uint32 restatement of the hash, the splat against a numpy float32 restatement that walks
the sources of a pixel in the stated order, the three consequences of the definition (box 0.5 is PhotonAccumulator.accumulate, one splat
of spp samples is spp splats of one, a sample on a pixel border lands in one pixel), NaN samples, and the argument checks.  Every
comparison is of the uint32 views: no tolerance anywhere.  No GPU is needed."""
import ctypes as C

import numpy as np
import pytest

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import _capi, film
from _film_support import bits, case_data, F32, FILTERS, host_splat, IMAGES, offsets_restated, SPPS

RADII = [0.5, 1.0, 2.0]  # reach 1, 2, 3


# ---- the sample positions ----


@pytest.mark.parametrize("seed", [0, 0x9E3779B9])
@pytest.mark.parametrize("pattern,spp", [(p, s) for p in ("center", "uniform", "stratified") for s in (1, 4, 9)] + [("uniform", 3)])
def test_offsets_equal_the_restated_hash(pattern, spp, seed):
    frame = rt.Frame.full(37, 23, 0)
    got = film.offsets_numpy(frame, spp, pattern, seed)
    assert got.shape == (spp, 37 * 23, 2) and got.dtype == F32
    assert np.array_equal(bits(got), bits(offsets_restated(frame, spp, pattern, seed)))
    assert (got >= F32(-0.5)).all() and (got <= F32(0.5)).all()
    if pattern == "center":
        assert not bits(got).any()  # +0, not -0
    elif spp > 1:
        assert not np.array_equal(got[0], got[1])


@pytest.mark.parametrize("pattern", ["uniform", "stratified"])
def test_a_tile_has_the_offsets_of_its_pixels_in_the_full_frame(pattern):
    full = rt.Frame.full(37, 23, 0)
    tile = rt.Frame(37, 23, 0, 5, 3, 30, 20, 2)
    whole = film.offsets_numpy(full, 4, pattern, 7).reshape(4, 23, 37, 2)
    part = film.offsets_numpy(tile, 4, pattern, 7).reshape(4, tile.rows, tile.cols, 2)
    assert np.array_equal(bits(part), bits(whole[:, 3:20:2, 5:30]))
    assert np.array_equal(bits(part), bits(offsets_restated(tile, 4, pattern, 7).reshape(part.shape)))


def test_offset_argument_errors():
    frame = rt.Frame.full(37, 23, 0)
    for spp in (2, 3, 81):  # no k * k with k <= 8
        with pytest.raises(rt.RtError) as e:
            film.offsets_numpy(frame, spp, "stratified")
        assert e.value.code == -1 and "k * k" in str(e.value)
    with pytest.raises(ValueError):
        film.offsets_numpy(frame, 4, "halton")
    lib = _capi.host_lib()
    out = np.zeros((4, 37 * 23, 2), dtype=F32)
    p = out.ctypes.data_as(C.c_void_p)
    assert lib.rt_film_offsets_host(None, 4, 2, 0, p) == -1 and b"null frame" in lib.rt_host_last_error()
    assert lib.rt_film_offsets_host(C.byref(frame), 0, 1, 0, p) == -1 and b"spp" in lib.rt_host_last_error()
    assert lib.rt_film_offsets_host(C.byref(frame), 4, 3, 0, p) == -1 and b"pattern" in lib.rt_host_last_error()
    assert lib.rt_film_offsets_host(C.byref(frame), 4, 2, 0, None) == -1 and b"null" in lib.rt_host_last_error()
    bad = rt.Frame(37, 23, 0, 0, 0, 38, 23, 1)
    assert lib.rt_film_offsets_host(C.byref(bad), 4, 2, 0, p) == -1 and b"bad frame" in lib.rt_host_last_error()
    assert lib.rt_film_offsets_host(C.byref(rt.Frame.full(65536, 65535, 0)), 4, 1, 0, p) == -5 and b"2^32" in lib.rt_host_last_error()
    # the device library checks the same things before any device work
    amd = _capi.amd_lib()
    assert amd.rt_film_offsets(C.byref(frame), 3, 2, 0, p, None) == -1 and b"k * k" in amd.rt_last_error()
    assert amd.rt_film_offsets(C.byref(frame), 4, 2, 0, None, None) == -1 and b"null" in amd.rt_last_error()
    assert amd.rt_camera_rays_offset(None, C.byref(frame), p, 4, p, None) == -1 and b"null" in amd.rt_last_error()
    assert amd.rt_camera_rays_offset(C.byref(rt.reference_camera()), C.byref(frame), p, 0, p, None) == -1 and b"spp" in amd.rt_last_error()
    assert amd.rt_camera_rays_offset(C.byref(rt.reference_camera()), C.byref(frame), None, 4, p, None) == -1 and b"null" in amd.rt_last_error()


# ---- the splat ----

def filter_restated(name, d, radius):
    radius = F32(radius)
    if name == "box":
        return np.ones_like(d)
    if name == "tent":
        return F32(1.0) - np.abs(d) / radius
    x = F32(2.0) * np.abs(d) / radius
    near = ((F32(7.0) * x - F32(12.0)) * x * x + F32(16.0) / F32(3.0)) / F32(6.0)
    far = (((F32(-7.0) / F32(3.0) * x + F32(12.0)) * x - F32(20.0)) * x + F32(32.0) / F32(3.0)) / F32(6.0)
    return np.where(x < F32(1.0), near, far)


def splat_restated(rows, cols, samples, valid, offsets, name, radius, total, weight):
    """The definition: s outermost, then dr, then dc, ascending; every output pixel at once (each keeps its own order), f32 throughout.
    samples (spp, n, 3), valid (spp, n) or None, offsets (spp, n, 2); returns the new (sum, weight)."""
    spp = samples.shape[0]
    reach = int(np.ceil(F32(radius) + F32(0.5)))
    total, weight = total.copy(), weight.copy()
    smp, off = samples.reshape(spp, rows, cols, 3), offsets.reshape(spp, rows, cols, 2)
    ok = np.ones((spp, rows, cols), dtype=bool) if valid is None else valid.reshape(spp, rows, cols) != 0
    r, c = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    rad = F32(radius)
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(spp):
            for dr in range(-reach, reach + 1):
                for dc in range(-reach, reach + 1):
                    qr, qc = r + dr, c + dc
                    inside = (qr >= 0) & (qr < rows) & (qc >= 0) & (qc < cols)
                    qr, qc = np.clip(qr, 0, rows - 1), np.clip(qc, 0, cols - 1)
                    ddx = F32(dc) + off[s, qr, qc, 0]
                    ddy = F32(dr) + off[s, qr, qc, 1]
                    hit = inside & ok[s, qr, qc] & (-rad <= ddx) & (ddx < rad) & (-rad <= ddy) & (ddy < rad)
                    w = (filter_restated(name, ddx, radius) * filter_restated(name, ddy, radius)).astype(F32)
                    photon = smp[s, qr, qc]
                    total = np.where(hit[..., None], total + photon * w[..., None], total)
                    weight = np.where(hit, weight + w, weight)
    assert total.dtype == F32 and weight.dtype == F32
    return total, weight


@pytest.mark.parametrize("name", FILTERS)
@pytest.mark.parametrize("rows,cols", IMAGES)
def test_splat_equals_the_restated_definition(rows, cols, name):
    for spp in SPPS:
        samples, valid, offsets, total, weight = case_data(rows, cols, spp)
        for radius in RADII:
            for flags in (valid, None):
                got = host_splat(rows, cols, samples, flags, offsets, name, radius, total, weight)
                want = splat_restated(rows, cols, samples, flags, offsets, name, radius, total, weight)
                assert np.array_equal(bits(got[0]), bits(want[0])), (spp, radius, flags is None)
                assert np.array_equal(bits(got[1]), bits(want[1])), (spp, radius, flags is None)


@pytest.mark.parametrize("name,radius", [("box", 0.5), ("tent", 1.0), ("mitchell", 2.0)])
def test_a_nan_sample_reaches_exactly_the_pixels_it_lies_in(name, radius):
    rows, cols, spp = 23, 37, 4
    samples, valid, offsets, _, _ = case_data(rows, cols, spp)
    samples, valid = samples.copy(), valid.copy()
    s, qr, qc = 2, 11, 17
    q = qr * cols + qc
    samples[s, q, 1] = np.nan
    valid[s, q] = 0
    total, weight = host_splat(rows, cols, samples, valid, offsets, name, radius)
    assert not np.isnan(total).any() and not np.isnan(weight).any()
    valid[s, q] = 1
    total, weight = host_splat(rows, cols, samples, valid, offsets, name, radius)
    reach = int(np.ceil(F32(radius) + F32(0.5)))
    r, c = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    ddx, ddy = (qc - c).astype(F32) + offsets[s, q, 0], (qr - r).astype(F32) + offsets[s, q, 1]
    rad = F32(radius)
    want = (abs(qr - r) <= reach) & (abs(qc - c) <= reach) & (-rad <= ddx) & (ddx < rad) & (-rad <= ddy) & (ddy < rad)
    assert want.sum() >= 1
    assert np.array_equal(np.isnan(total[..., 1]), want)
    assert not np.isnan(total[..., 0]).any() and not np.isnan(total[..., 2]).any() and not np.isnan(weight).any()


@pytest.mark.parametrize("rows,cols", IMAGES)
def test_box_of_radius_half_is_the_photon_accumulator(rows, cols):
    samples, valid, _, _, _ = case_data(rows, cols, 4)
    offsets = np.random.default_rng(5).random((4, rows * cols, 2), dtype=F32) - F32(0.5)  # [-0.5, 0.5)
    offsets[0, 0] = F32(-0.5)
    acc = rt.PhotonAccumulator(rows, cols, "cpu")
    f = film.Film(rows, cols, "box", 0.5)
    for _ in range(2):  # the second round continues from the first
        acc.accumulate(samples.reshape(4, rows, cols, 3), valid.reshape(4, rows, cols))
        f.splat(samples, offsets, valid)
        assert np.array_equal(bits(f.sum), bits(acc.sum)) and np.array_equal(bits(f.weight), bits(acc.weight))
    assert np.array_equal(bits(f.resolve()), bits(acc.resolve()))


@pytest.mark.parametrize("name,radius", [("box", 0.5), ("tent", 1.0), ("mitchell", 2.0)])
def test_one_splat_of_four_samples_is_four_splats_of_one(name, radius):
    rows, cols = 23, 37
    samples, valid, offsets, total, weight = case_data(rows, cols, 4)
    once = host_splat(rows, cols, samples, valid, offsets, name, radius, total, weight)
    f = film.Film(rows, cols, name, radius)
    f.sum[...] = total
    f.weight[...] = weight
    for s in range(4):
        f.splat(samples[s:s + 1], offsets[s:s + 1], valid[s:s + 1])
    assert np.array_equal(bits(f.sum), bits(once[0])) and np.array_equal(bits(f.weight), bits(once[1]))


@pytest.mark.parametrize("edge", [-0.5, 0.5])
def test_a_sample_on_a_pixel_border_lands_in_one_pixel(edge):
    rows, cols = 5, 7
    n = rows * cols
    samples, offsets, valid = np.ones((1, n, 3), dtype=F32), np.zeros((1, n, 2), dtype=F32), np.zeros((1, n), dtype=np.uint8)
    q = 2 * cols + 3
    valid[0, q] = 1
    offsets[0, q] = F32(edge)
    _, weight = host_splat(rows, cols, samples, valid, offsets, "box", 0.5)
    assert weight.sum() == 1.0 and np.count_nonzero(weight) == 1
    # the half-open support: -0.5 belongs to the sample's own pixel, +0.5 to the next one down and to the right
    assert weight[(2, 3) if edge < 0 else (3, 4)] == 1.0


def test_splat_argument_errors():
    n = 6
    samples, offsets = np.zeros((1, n, 3), dtype=F32), np.zeros((1, n, 2), dtype=F32)
    total, weight = np.zeros((2, 3, 3), dtype=F32), np.zeros((2, 3), dtype=F32)
    ps, po, pt, pw = (a.ctypes.data_as(C.c_void_p) for a in (samples, offsets, total, weight))
    host, amd = _capi.host_lib(), _capi.amd_lib()
    calls = [(lambda *a: host.rt_film_splat_host(*a), host.rt_host_last_error, b"rt_film_splat_host: "),
             (lambda *a: amd.rt_film_splat(*a, None), amd.rt_last_error, b"rt_film_splat: ")]
    for call, message, who in calls:
        for args, text in [((2, 3, ps, None, po, 1, 1, 0.0, pt, pw), b"radius"), ((2, 3, ps, None, po, 1, 1, 4.5, pt, pw), b"radius"),
                           ((2, 3, ps, None, po, 1, 1, float("nan"), pt, pw), b"radius"), ((2, 3, ps, None, po, 1, 3, 1.0, pt, pw), b"filter"),
                           ((2, 3, ps, None, po, 0, 1, 1.0, pt, pw), b"spp"), ((65536, 65536, ps, None, po, 1, 1, 1.0, pt, pw), b"2^32"),
                           ((2, 3, None, None, po, 1, 1, 1.0, pt, pw), b"null"), ((2, 3, ps, None, None, 1, 1, 1.0, pt, pw), b"null"),
                           ((2, 3, ps, None, po, 1, 1, 1.0, None, pw), b"null"), ((2, 3, ps, None, po, 1, 1, 1.0, pt, None), b"null")]:
            assert call(*args) == -1, args
            assert message().startswith(who) and text in message(), (args, message())
        assert call(0, 3, ps, None, po, 1, 1, 1.0, pt, pw) == 0  # an empty image: nothing to do
    assert not total.any() and not weight.any()
    f = film.Film(2, 3, "tent", 4.5)
    with pytest.raises(rt.RtError) as e:
        f.splat(samples, offsets)
    assert e.value.code == -1 and "radius" in str(e.value)
    with pytest.raises(ValueError):
        film.Film(2, 3, "gauss")
    with pytest.raises(ValueError):
        film.Film(2, 3).splat(samples[:, :5], offsets)
