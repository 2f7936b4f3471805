"""Temporal queries on the host (include/rt_amd.h "temporal queries"): rt_temporal_motion_cpu and rt_temporal_accumulate_cpu of
librt_host.so, the CPU definition, held bit for bit against the numpy float32 restatement of _temporal_support, against the exact
consequences of the definition, and — the projection — against binary64 to the derived bound.  The device is held against this CPU form
by tests/test_gpu_temporal.py."""
import numpy as np
import pytest

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import temporal
from _temporal_support import (F32, FIELDS, HISTORY, IMAGES, PARAMS, PROJECTION_BOUND, Planes, bits, case_data, embed, luminance, motion_field,
                               pixel_positions, restate_accumulate, restate_motion)

OFF = dict(normal_min=-2.0, position_max=float("inf"), alpha_min=0.0, max_length=1 << 20)


def guides(p, strided=False, **drop):
    if strided:
        p = embed(p)[2]
    return temporal.Guides(**{k: (None if k in drop else getattr(p, k)) for k in ("normal", "position", "object", "valid")})


def same_records(got, want):
    return np.array_equal(bits(got.reshape(-1)), bits(want.reshape(-1)))


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("rows,cols", IMAGES)
def test_accumulate_is_the_restatement_bit_for_bit(rows, cols, strided):
    color, history, cur, prev = case_data(rows, cols)
    reset = blended = 0
    for kind in FIELDS:
        m = motion_field(rows, cols, kind)
        got, var = temporal.accumulate_numpy(color, m, rows, cols, history, guides(cur, strided), guides(prev, strided), **PARAMS)
        want, want_var = restate_accumulate(color, m, rows, cols, history, cur, prev, **PARAMS)
        assert same_records(got, want) and np.array_equal(bits(var.reshape(-1)), bits(want_var)), kind
        assert not got["reserved"].any()
        blended += int((got["length"] > 1).sum())
        reset += int((got["length"] == 1).sum())
    assert reset > 0 and (blended > 0 or rows * cols == 1)


def test_special_coordinates_are_sorted_by_the_float_tests():
    """-1 exactly and just below cols gather (and find no tap with weight > 0 inside, or one), beyond them, 1e30, +-Inf and NaN reset"""
    rows, cols = 1, 70
    color = np.full((cols, 3), 0.5, dtype=F32)
    history = np.zeros(cols, dtype=HISTORY)
    history["length"] = 3
    history["color"] = 0.25
    m = np.zeros((cols, 2), dtype=F32)
    values = [-1.0, np.nextafter(F32(cols), F32(0)), -1.5, 1e30, np.inf, -np.inf, np.nan, -0.0, float(cols), 68.5, -0.5]
    m[:len(values), 0] = values
    got, _ = temporal.accumulate_numpy(color, m, rows, cols, history, **OFF)
    length = got["length"][0, :len(values)].tolist()
    #          -1: tap 0 has wx = 0   69.99..: tap 69   the rest outside or not finite   -0.0   cols   68.5  -0.5: tap 0 alone
    assert length == [1, 4, 1, 1, 1, 1, 1, 4, 1, 4, 4]
    want, _ = restate_accumulate(color, m, rows, cols, history, **OFF)
    assert same_records(got, want)


def _three_by_three():
    rows = cols = 3
    n = 9
    g = np.random.default_rng(2)
    color = g.random((n, 3), dtype=F32)
    history = np.zeros(n, dtype=HISTORY)
    history["color"], history["moment1"], history["moment2"], history["length"] = g.random((n, 3), dtype=F32), 0.5, 0.3, 2
    normal = np.tile(np.array([0, 0, 1], dtype=F32), (n, 1))
    position = g.random((n, 3), dtype=F32)
    planes = lambda: Planes(normal.copy(), position.copy(), np.full(n, 7, dtype=np.uint32), np.ones(n, dtype=np.uint32))
    return rows, cols, color, history, planes(), planes(), motion_field(rows, cols, "integer")


@pytest.mark.parametrize("cause", ["valid", "length", "object", "normal", "position"])
def test_each_rejection_cause_alone_resets_an_otherwise_accepted_tap(cause):
    rows, cols, color, history, cur, prev, m = _three_by_three()
    kw = dict(normal_min=0.9, position_max=0.01, alpha_min=0.0, max_length=8)
    base, _ = temporal.accumulate_numpy(color, m, rows, cols, history, guides(cur), guides(prev), **kw)
    assert (base["length"] == 3).all()
    q = 4
    if cause == "valid":
        prev.valid[q] = 0
    elif cause == "length":
        history["length"][q] = 0
    elif cause == "object":
        prev.object[q] = 8
    elif cause == "normal":
        prev.normal[q] = [0.6, 0, 0.8]  # dot 0.8 < 0.9
    else:
        prev.position[q, 0] += F32(0.02)
    got, var = temporal.accumulate_numpy(color, m, rows, cols, history, guides(cur), guides(prev), **kw)
    want, want_var = restate_accumulate(color, m, rows, cols, history, cur, prev, **kw)
    assert same_records(got, want) and np.array_equal(bits(var.reshape(-1)), bits(want_var))
    flat = got.reshape(-1)
    assert flat["length"][q] == 1 and np.array_equal(bits(flat["color"][q]), bits(color[q])) and var.reshape(-1)[q] == 0
    others = np.arange(9) != q
    assert same_records(flat[others], base.reshape(-1)[others])


@pytest.mark.parametrize("drop", ["normal", "position", "object", "valid"])
def test_a_null_plane_switches_its_test_off(drop):
    rows, cols = 33, 65
    color, history, cur, prev = case_data(rows, cols)
    m = motion_field(rows, cols, "fractional")
    got, var = temporal.accumulate_numpy(color, m, rows, cols, history, guides(cur, **{drop: 1}), guides(prev, **{drop: 1}), **PARAMS)
    less = lambda p: Planes(**{k: (None if k == drop else getattr(p, k)) for k in ("normal", "position", "object", "valid")})
    want, want_var = restate_accumulate(color, m, rows, cols, history, less(cur), less(prev), **PARAMS)
    assert same_records(got, want) and np.array_equal(bits(var.reshape(-1)), bits(want_var))
    full, _ = temporal.accumulate_numpy(color, m, rows, cols, history, guides(cur), guides(prev), **PARAMS)
    assert not same_records(got, full)  # the test did reject taps while it was on


def test_nan_colour_keeps_its_payload_and_nan_history_propagates():
    rows, cols = 33, 65
    color, history, cur, prev = case_data(rows, cols)
    color = color.copy()
    color.view(np.uint32)[5, 0] = 0x7FC12345
    m = motion_field(rows, cols, "integer")
    got, _ = temporal.accumulate_numpy(color, m, rows, cols, history, **OFF)
    flat = got.reshape(-1)
    n = rows * cols
    assert history["length"][n // 3] > 0 and np.isnan(flat["color"][n // 3, 2]) and not np.isnan(flat["color"][n // 3, :2]).any()
    assert np.isnan(flat["moment1"][(2 * n) // 3]) and flat["length"][(2 * n) // 3] == history["length"][(2 * n) // 3] + 1
    cleared = np.flatnonzero(history["length"] == 0)  # such a pixel resets: the raw words
    assert cleared.size and np.array_equal(bits(flat["color"][cleared]), bits(color[cleared]))
    zero = np.zeros(n, dtype=HISTORY)
    reset, _ = temporal.accumulate_numpy(color, m, rows, cols, zero, **OFF)
    assert reset.reshape(-1)["color"].view(np.uint32)[5, 0] == 0x7FC12345


# ---- the stated properties, each an equality of bits ----

def test_integer_coordinates_gather_the_previous_record_exactly():
    """all tests off and max_length huge: alpha = 1 / (length + 1); with a current colour equal to the history's the blend returns it"""
    rows, cols = 33, 65
    _, history, _, _ = case_data(rows, cols)
    history = history.copy()
    history["length"] = np.maximum(history["length"], 1)
    g = np.random.default_rng(9)
    history["color"] = g.random((rows * cols, 3), dtype=F32)  # no NaN
    history["moment1"] = g.random(rows * cols, dtype=F32)
    perm = g.permutation(rows * cols)  # every pixel looks at some other pixel's integer coordinates
    m = np.stack([perm % cols, perm // cols], axis=1).astype(F32)
    color = g.random((rows * cols, 3), dtype=F32)
    got, _ = temporal.accumulate_numpy(color, m, rows, cols, history, **OFF)
    flat = got.reshape(-1)
    H = history[perm]
    alpha = (F32(1) / (H["length"] + 1).astype(F32)).astype(F32)
    keep = F32(1) - alpha
    assert np.array_equal(bits(flat["color"]), bits(H["color"] * keep[:, None] + color * alpha[:, None]))
    assert np.array_equal(bits(flat["moment1"]), bits(H["moment1"] * keep + luminance(color) * alpha))
    assert np.array_equal(flat["length"], H["length"] + 1)


def test_alpha_min_zero_is_the_running_mean_written_as_the_blend():
    rows, cols = 33, 65
    n = rows * cols
    m = motion_field(rows, cols, "integer")
    g = np.random.default_rng(4)
    history = np.zeros(n, dtype=HISTORY)
    mean = m1 = m2 = None
    for k in range(1, 6):
        color = g.random((n, 3), dtype=F32)
        L = luminance(color)
        history, var = temporal.accumulate_numpy(color, m, rows, cols, history, **OFF)
        history = history.reshape(-1)
        if k == 1:
            mean, m1, m2 = color, L, L * L
        else:
            alpha = F32(1) / F32(k)
            keep = F32(1) - alpha
            mean, m1, m2 = mean * keep + color * alpha, m1 * keep + L * alpha, m2 * keep + (L * L) * alpha
        assert np.array_equal(bits(history["color"]), bits(mean)) and np.array_equal(bits(history["moment1"]), bits(m1)), k
        assert np.array_equal(bits(history["moment2"]), bits(m2)) and (history["length"] == k).all(), k
        v = m2 - m1 * m1
        assert np.array_equal(bits(var.reshape(-1)), bits(np.where((v > 0) & (k > 1), v, F32(0)).astype(F32))), k
    assert (var > 0).any()


def test_max_length_one_returns_the_current_frame():
    rows, cols = 33, 65
    color, history, cur, prev = case_data(rows, cols)
    history = history.copy()
    history["color"][rows * cols // 3, 2] = 1.0  # a finite history: 0 * H is 0
    history["moment1"][(2 * rows * cols) // 3] = 1.0
    color = color.copy()
    color[rows * cols // 2, 1] = 0.75
    m = motion_field(rows, cols, "fractional")
    got, var = temporal.accumulate_numpy(color, m, rows, cols, history, guides(cur), guides(prev), normal_min=0.6, position_max=0.16, alpha_min=0.0, max_length=1)
    flat = got.reshape(-1)
    L = luminance(color)
    assert np.array_equal(bits(flat["color"]), bits(color)) and (flat["length"] == 1).all()
    assert np.array_equal(bits(flat["moment1"]), bits(L)) and np.array_equal(bits(flat["moment2"]), bits(L * L))


def test_variance_is_the_clamped_second_central_moment_and_zero_on_resets():
    rows, cols = 33, 65
    color, history, cur, prev = case_data(rows, cols)
    got, var = temporal.accumulate_numpy(color, motion_field(rows, cols, "fractional"), rows, cols, history, guides(cur), guides(prev), **PARAMS)
    flat, var = got.reshape(-1), var.reshape(-1)
    with np.errstate(invalid="ignore"):
        v = flat["moment2"] - flat["moment1"] * flat["moment1"]
        want = np.where((v > 0) & (flat["length"] > 1), v, F32(0)).astype(F32)
    assert np.array_equal(bits(var), bits(want)) and (var > 0).any() and ((v < 0) & (flat["length"] > 1)).any()
    none, no_var = temporal.accumulate_numpy(color, motion_field(rows, cols, "fractional"), rows, cols, history, guides(cur), guides(prev), variance=False,
                                             **PARAMS)
    assert no_var is None and same_records(none, got)


# ---- the projection ----

@pytest.mark.parametrize("rows,cols", IMAGES)
def test_motion_is_the_restatement_bit_for_bit(rows, cols):
    cam, frame = rt.reference_camera(), rt.Frame.full(cols, rows, 3)
    g = np.random.default_rng(rows * 100 + cols)
    position = (g.random((rows * cols, 3), dtype=F32) * F32(40.0) - F32(20.0)).astype(F32)  # in front of the camera and behind it
    valid = (g.random(rows * cols) >= 0.2).astype(np.uint32)
    want = restate_motion(position, cam, frame, valid)
    got = temporal.motion_numpy(position, cam, frame, valid=valid)
    assert np.array_equal(bits(got.reshape(-1, 2)), bits(want))
    assert (rows * cols < 9) or (np.isnan(want).any() and np.isfinite(want).any())
    hits, surfaces, views = embed(Planes(np.zeros_like(position), position, np.zeros(rows * cols, dtype=np.uint32), valid))
    strided = temporal.motion_numpy(views.position, cam, frame, valid=views.valid)
    assert np.array_equal(bits(strided), bits(got))
    free = temporal.motion_numpy(position, cam, frame)
    assert np.array_equal(bits(free.reshape(-1, 2)), bits(restate_motion(position, cam, frame)))


def test_projection_accuracy_against_binary64_and_the_round_trip():
    cam, frame = rt.reference_camera(), rt.Frame.full(64, 48, 3)
    position = pixel_positions(cam, frame, np.geomspace(0.5, 50.0, 16))
    got = temporal.motion_numpy(position, cam, frame).reshape(-1, 2).astype(np.float64)
    exact = restate_motion(position, cam, frame, dtype=np.float64)
    restated = restate_motion(position, cam, frame).astype(np.float64)
    y, x = np.meshgrid(np.arange(48.0), np.arange(64.0), indexing="ij")
    centre = np.stack([x.reshape(-1), y.reshape(-1)], axis=1)
    print(f"projection: float32 restatement against binary64 {np.abs(restated - exact).max():.3g} px, motion_numpy against binary64 "
          f"{np.abs(got - exact).max():.3g} px, round trip {np.abs(got - centre).max():.3g} px; bound {PROJECTION_BOUND:.3g}")
    assert np.abs(got - exact).max() <= PROJECTION_BOUND
    assert np.abs(got - centre).max() <= PROJECTION_BOUND
    behind = (np.array(list(cam.center), dtype=F32) - np.array(list(cam.toward), dtype=F32) * F32(3.0)).reshape(1, 3)
    one = rt.Frame.full(1, 1, 3)
    assert np.isnan(temporal.motion_numpy(behind, cam, one)).all()
