"""The bloom queries' CPU definition (rt_bloom_cpu through bloom.bloom_numpy) against the numpy-float32 restatement of
include/rt_amd.h's steps, bit for bit, and the properties the definition promises: a constant image stays constant at every border and
odd size, no glow returns the colour, a pixel that is not finite spreads nowhere, a mirrored image gives the mirrored result, and the
call may write over its colour.  No device."""
import math

import numpy as np
import pytest

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import bloom
import _bloom_support as S

F32 = np.float32


@pytest.mark.parametrize("knee", S.KNEES)
@pytest.mark.parametrize("levels", S.LEVELS)
@pytest.mark.parametrize("rows,cols", S.SIZES)
def test_the_cpu_definition_equals_the_restatement(rows, cols, levels, knee):
    """the colour compact, and as a view inside 8-word records; 17 x 17 at 5 levels goes 9, 5, 3, 2, 1"""
    color = S.case_data(rows, cols)
    want = S.bloom_restated(color, 1.0, knee, 0.5, levels)
    assert np.array_equal(S.bits(bloom.bloom_numpy(color, knee=knee, levels=levels)), S.bits(want))
    records, view = S.in_records(color)
    assert np.array_equal(S.bits(bloom.bloom_numpy(view, knee=knee, levels=levels)), S.bits(want))
    assert (records[..., 3:] == 3.5).all() and np.array_equal(view, color)  # nothing given is written
    assert (want >= color).all() and (want > color).any()  # something glows


def test_the_restated_cases_cover_the_threshold_from_both_sides():
    """about 2 % of a case's pixels lie above the threshold, at several scales of excess; the knee reaches pixels under it"""
    color = S.case_data(33, 65)
    w = [F32(x) for x in rt.luma_row()]
    luma = (w[0] * color[..., 0] + w[1] * color[..., 1]) + w[2] * color[..., 2]
    above = luma > 1.0
    assert 0.005 < above.mean() < 0.05 and luma[above].max() / luma[above].min() > 20.0 and (luma[~above] < 0.9).all()
    assert (S.bright(color, 1.0, 0.0)[~above] == 0).all() and (S.bright(color, 1.0, 0.5)[above] > 0).all()
    soft = np.full((1, 1, 3), 0.8, dtype=F32)  # inside the knee: s = -0.2, t = 0.3, q = 0.045
    assert (S.bright(soft, 1.0, 0.5) > 0).all() and (S.bright(soft, 1.0, 0.0) == 0).all()
    assert np.array_equal(S.bits(bloom.bloom_numpy(soft, levels=1)), S.bits(S.bloom_restated(soft, levels=1)))


@pytest.mark.parametrize("levels", S.LEVELS)
@pytest.mark.parametrize("rows,cols", S.SIZES)
def test_a_constant_image_stays_constant(rows, cols, levels):
    """4.0 everywhere, threshold 1: every pixel of the output has the same bits — no edge darkens, no odd last row differs"""
    out = bloom.bloom_numpy(np.full((rows, cols, 3), 4.0, dtype=F32), threshold=1.0, levels=levels)
    assert (S.bits(out) == S.bits(out)[0, 0, 0]).all() and out[0, 0, 0] > 4.0


@pytest.mark.parametrize("rows,cols", [(1, 1), (17, 17), (31, 18)])
def test_no_glow_returns_the_colour(rows, cols):
    color = S.case_data(rows, cols)
    for kw in (dict(threshold=math.inf), dict(intensity=0.0), dict(threshold=math.inf, knee=0.0)):
        assert np.array_equal(S.bits(bloom.bloom_numpy(color, levels=5, **kw)), S.bits(color)), kw


@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("at", [(0, 0), (8, 9), (16, 17)])
def test_a_pixel_that_is_not_finite_spreads_nowhere(value, at):
    """every other pixel has the bits of the run in which that pixel is black; the pixel itself is still not finite"""
    color = S.case_data(17, 18).copy()
    color[at] = (5.0, value, 7.0)
    black = color.copy()
    black[at] = 0.0
    got, want = bloom.bloom_numpy(color, levels=5), bloom.bloom_numpy(black, levels=5)
    others = np.ones(color.shape[:2], dtype=bool)
    others[at] = False
    assert np.array_equal(S.bits(got)[others], S.bits(want)[others])
    assert not np.isfinite(got[at][1]) and np.isfinite(got[at][[0, 2]]).all() and np.isfinite(want).all()


@pytest.mark.parametrize("levels,rows,cols", [(1, 2, 6), (2, 16, 20), (5, 32, 64)])
def test_a_mirrored_image_gives_the_mirrored_result(levels, rows, cols):
    """sizes that are multiples of 2^L both ways: the tap sums are written mirror-symmetric"""
    color = np.ascontiguousarray(S.case_data(rows, cols))
    want = bloom.bloom_numpy(color, levels=levels)
    for axis in (0, 1):
        flipped = np.ascontiguousarray(np.flip(color, axis=axis))
        assert np.array_equal(S.bits(bloom.bloom_numpy(flipped, levels=levels)), S.bits(np.flip(want, axis=axis))), axis


@pytest.mark.parametrize("rows,cols,levels", [(1, 1, 1), (17, 17, 5), (33, 65, 2)])
def test_in_place_gives_the_bits_of_the_out_of_place_call(rows, cols, levels):
    color = S.case_data(rows, cols).copy()
    want = bloom.bloom_numpy(color, levels=levels)
    out = np.zeros_like(color)
    assert bloom.bloom_numpy(color, levels=levels, out=out) is out and np.array_equal(S.bits(out), S.bits(want))
    assert bloom.bloom_numpy(color, levels=levels, out=color) is color and np.array_equal(S.bits(color), S.bits(want))


def test_the_python_form_checks_its_arrays():
    color = S.case_data(3, 5)
    with pytest.raises(ValueError, match="color"):
        bloom.bloom_numpy(color.reshape(-1, 3))
    with pytest.raises(ValueError, match="color"):
        bloom.bloom_numpy(color.astype(np.float64))
    with pytest.raises(ValueError, match="out"):
        bloom.bloom_numpy(color, out=np.zeros((3, 5, 4), dtype=F32))
    records, view = S.in_records(color)
    with pytest.raises(Exception, match="out may be color only with color_stride 3"):
        bloom.bloom_numpy(view, out=np.lib.stride_tricks.as_strided(records, shape=(3, 5, 3), strides=(60, 12, 4)))
