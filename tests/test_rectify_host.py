"""The history rectification queries on the CPU (librt_host.so; no device): the three CPU forms against the numpy restatement of the
definition bit for bit, the consequences the header states as equalities of bits, every refusal with its status and text in order, the
Samuelson bound, and what the clamp and the feedback do to a sequence whose shading changes — asserted as orderings only."""
import ctypes as C

import numpy as np
import pytest

from homework_18_graphics_raytracer_amd import _capi, rectify, svgf, temporal

import _rectify_support as S
from _temporal_support import PARAMS, case_data as temporal_case, motion_field

INVALID, UNSUPPORTED = -1, -5


def guides(p):
    return temporal.Guides(p.normal, p.position, p.object, p.valid)


# ---- rt_temporal_bounds_cpu ----

@pytest.mark.parametrize("radius", S.RADII)
@pytest.mark.parametrize("planes", ["both", "object", "valid", "none"])
@pytest.mark.parametrize("rows,cols", S.IMAGES)
def test_bounds_equal_the_restatement(rows, cols, planes, radius):
    """the case data carries a NaN, an infinity and -0.0 in sources"""
    color, obj, valid = S.case_data(rows, cols)
    obj, valid = (obj if planes in ("both", "object") else None), (valid if planes in ("both", "valid") else None)
    got = rectify.bounds_numpy(color, rows, cols, object=obj, valid=valid, gamma=1.25, radius=radius)
    want = S.restate_bounds(color, rows, cols, obj, valid, 1.25, radius)
    assert got.shape == (rows, cols) and got.dtype == rectify.BOX_DTYPE
    assert np.array_equal(S.bits(got), S.bits(want))
    if valid is not None:
        off = valid == 0
        assert (got.reshape(-1)["lo"][off] == -np.inf).all() and (got.reshape(-1)["hi"][off] == np.inf).all()


@pytest.mark.parametrize("radius", S.RADII)
def test_bounds_read_strided_record_views(radius):
    color, obj, valid = S.case_data(17, 33)
    rec, (c, o, v) = S.embed(color, obj, valid)
    before = rec.copy()
    got = rectify.bounds_numpy(c, 17, 33, object=o, valid=v, gamma=0.75, radius=radius)
    assert np.array_equal(S.bits(got), S.bits(rectify.bounds_numpy(color, 17, 33, object=obj, valid=valid, gamma=0.75, radius=radius)))
    assert np.array_equal(rec.view(np.uint32), before.view(np.uint32))  # the sentinels between the fields, and everything else, unread or unharmed


def test_a_nan_source_reaches_every_box_that_counts_it_and_no_other():
    color, obj, _ = S.case_data(17, 33)
    got = rectify.bounds_numpy(color, 17, 33, object=obj, gamma=1.0, radius=1).reshape(17, 33)
    q = (17 * 33) // 2
    r, c = divmod(q, 33)
    o = obj.reshape(17, 33)
    for rr in range(17):
        for cc in range(33):
            counts = abs(rr - r) <= 1 and abs(cc - c) <= 1 and o[rr, cc] == o[r, c]
            assert bool(np.isnan(got[rr, cc]["lo"][1])) == counts, (rr, cc)


def test_samuelson_every_counting_source_lies_inside_a_box_of_gamma_3_radius_1():
    """no sample of k <= 9 values lies further than sqrt(k - 1) <= 2.83 population deviations from their mean; 3 leaves the f32 rounding room"""
    clean, _, region, _, _ = S.stepped_sequence(noise=0.0)
    for image in (clean[0], S.case_data(17, 33)[0][: 17 * 33]):
        rows, cols = (64, 64) if image is clean[0] else (17, 33)
        image = np.nan_to_num(np.array(image), nan=0.5, posinf=1.5)
        obj = region if rows == 64 else None
        box = rectify.bounds_numpy(image, rows, cols, object=obj, gamma=3.0, radius=1).reshape(rows, cols)
        x = S.channels(image, rows, cols)
        ok = np.ones((rows, cols), dtype=bool)
        o = None if obj is None else obj.reshape(rows, cols)
        for take, qr, qc in S.window(rows, cols, 1, o, ok):
            q = x[qr, qc]
            assert ((q >= box["lo"]) & (q <= box["hi"]))[take].all()


# ---- rt_temporal_accumulate_bounded_cpu ----

@pytest.mark.parametrize("clamped_length", [0, 2])
@pytest.mark.parametrize("field", ["integer", "fractional", "special3"])
@pytest.mark.parametrize("rows,cols", S.IMAGES)
def test_accumulate_bounded_equals_the_restatement(rows, cols, field, clamped_length):
    """the temporal case data (NaN colours and moments in the history, every guide test rejecting its share) against boxes of the current colour"""
    color, history, cur, prev = temporal_case(rows, cols)
    motion = motion_field(rows, cols, field)
    box = S.restate_bounds(color, rows, cols, cur.object, cur.valid, 0.5, 1)
    got = rectify.accumulate_bounded_numpy(color, motion, rows, cols, history, box, guides(cur), guides(prev), clamped_length=clamped_length, **PARAMS)
    want = S.restate_accumulate_bounded(color, motion, rows, cols, history, box, cur, prev, clamped_length=clamped_length, **PARAMS)
    for g, w in zip(got, want):
        assert np.array_equal(S.bits(g).reshape(-1), S.bits(w).reshape(-1))
    if (rows, cols, field) == (17, 33, "fractional"):  # the case is not idle: the clamp acts, on one channel and on all four
        assert got[2].min() == 0 and got[2].max() == 4


@pytest.mark.parametrize("rows,cols", S.IMAGES)
def test_consequences_as_equalities_of_bits(rows, cols):
    color, history, cur, prev = temporal_case(rows, cols)
    n = rows * cols
    motion = motion_field(rows, cols, "fractional")
    plain, plain_var = temporal.accumulate_numpy(color, motion, rows, cols, history, guides(cur), guides(prev), **PARAMS)
    # infinite boxes: rt_temporal_accumulate's records and variance, nothing clamped
    rec, var, clamped = rectify.accumulate_bounded_numpy(color, motion, rows, cols, history, S.infinite_boxes(n), guides(cur), guides(prev), clamped_length=2,
                                                         **PARAMS)
    assert np.array_equal(S.bits(rec), S.bits(plain)) and np.array_equal(S.bits(var), S.bits(plain_var)) and not clamped.any()
    # clamped_length = 0 leaves the lengths alone, whatever the box does
    box = S.restate_bounds(color, rows, cols, cur.object, cur.valid, 0.5, 1)
    rec0, _, clamped0 = rectify.accumulate_bounded_numpy(color, motion, rows, cols, history, box, guides(cur), guides(prev), clamped_length=0, **PARAMS)
    assert np.array_equal(rec0["length"], plain["length"])
    # a box that holds the luminance only: the colour keeps accumulate's bits; and the reverse for the second moment
    lum_only, colour_only = box.copy(), box.copy()
    lum_only["lo"][:, :3], lum_only["hi"][:, :3] = -np.inf, np.inf
    colour_only["lo"][:, 3], colour_only["hi"][:, 3] = -np.inf, np.inf
    rec1, _, _ = rectify.accumulate_bounded_numpy(color, motion, rows, cols, history, lum_only, guides(cur), guides(prev), clamped_length=0, **PARAMS)
    rec2, _, _ = rectify.accumulate_bounded_numpy(color, motion, rows, cols, history, colour_only, guides(cur), guides(prev), clamped_length=0, **PARAMS)
    assert np.array_equal(S.bits(rec1["color"]), S.bits(plain["color"]))
    assert np.array_equal(S.bits(rec2["moment1"]), S.bits(plain["moment1"])) and np.array_equal(S.bits(rec2["moment2"]), S.bits(plain["moment2"]))
    # the second moment is bitwise unchanged wherever the first was not clamped
    untouched = S.bits(rec0["moment1"]).reshape(-1) == S.bits(plain["moment1"]).reshape(-1)
    assert (S.bits(rec0["moment2"]).reshape(-1)[untouched] == S.bits(plain["moment2"]).reshape(-1)[untouched]).all()


def test_a_static_noise_free_sequence_is_never_clamped():
    """gamma 3, radius 1 on a noise-free image: the history is the image, which lies inside its own box (Samuelson); records as accumulate's"""
    clean, _, region, normal, position = S.stepped_sequence(noise=0.0)
    g = temporal.Guides(normal=normal, position=position, object=region)
    motion = S.identity_motion(64, 64)
    box = rectify.bounds_numpy(clean[0], 64, 64, object=region, gamma=3.0, radius=1)
    plain = bounded = np.zeros(64 * 64, dtype=temporal.HISTORY_DTYPE)
    for _ in range(3):
        plain, _ = temporal.accumulate_numpy(clean[0], motion, 64, 64, plain, g, g)
        bounded, _, clamped = rectify.accumulate_bounded_numpy(clean[0], motion, 64, 64, bounded, box, g, g)
        assert not clamped.any() and np.array_equal(S.bits(bounded), S.bits(plain))


# ---- rt_temporal_feedback_cpu ----

@pytest.mark.parametrize("with_valid", [False, True])
@pytest.mark.parametrize("rows,cols", S.IMAGES)
def test_feedback_equals_the_restatement_and_touches_nothing_else(rows, cols, with_valid):
    color, history, cur, _ = temporal_case(rows, cols)
    valid = cur.valid if with_valid else None
    rec, (c, _, v) = S.embed(color, cur.object, cur.valid)
    got = rectify.feedback_numpy(c, history, rows, cols, valid=v if with_valid else None).reshape(-1)
    want = S.restate_feedback(color, history, valid)
    assert np.array_equal(S.bits(got), S.bits(want))
    skipped = (history["length"] == 0) | ((valid == 0) if with_valid else False)
    assert np.array_equal(S.bits(got)[skipped], S.bits(history)[skipped])
    assert np.array_equal(S.bits(got)[:, 3:], S.bits(history)[:, 3:])  # moments, length, reserved
    assert np.array_equal(S.bits(got)[~skipped, :3], S.bits(color)[~skipped])  # the raw words: the NaN keeps its payload


# ---- what it is for: orderings on a sequence whose shading changes (the measured values are in DESIGN.md 3.25) ----

def _mse(a, b, mask=None):
    d = (np.asarray(a, dtype=np.float64).reshape(-1, 3) - b) ** 2
    return float((d if mask is None else d[mask]).mean())


def test_the_clamp_and_the_feedback_on_a_stepped_sequence():
    """64 x 64, sigma 0.2, quadrant 3 dimmed to 0.4 at frame 6 of 10, RADIUS / GAMMA / CLAMPED_LENGTH.  In frames 7 to 9, inside the
    quadrant, against the new clean image: accumulate_bounded's records are closer than accumulate's, and the output of the full sequence
    with feedback closer again; on every static frame before the step (1 to 5) the bounded records are closer than the noisy frame."""
    clean, noisy, region, normal, position = S.stepped_sequence()
    g = temporal.Guides(normal=normal, position=position, object=region)
    motion = S.identity_motion(64, 64)
    inside = region == S.STEP_REGION
    spatial = dict(normal=normal, position=position)
    plain = bounded = chain = np.zeros(64 * 64, dtype=temporal.HISTORY_DTYPE)
    for f in range(S.FRAMES):
        box = rectify.bounds_numpy(noisy[f], 64, 64, object=region)
        plain, _ = temporal.accumulate_numpy(noisy[f], motion, 64, 64, plain, g, g)
        bounded, _, _ = rectify.accumulate_bounded_numpy(noisy[f], motion, 64, 64, bounded, box, g, g)
        chain, _, _ = rectify.accumulate_bounded_numpy(noisy[f], motion, 64, 64, chain, box, g, g)
        v = svgf.variance_numpy(chain, 64, 64, **spatial)
        level0, v0 = svgf.atrous_numpy(chain["color"], v, 64, 64, levels=1, first_level=0, **spatial)
        chain = rectify.feedback_numpy(level0, chain, 64, 64)
        out, _ = svgf.atrous_numpy(level0, v0, 64, 64, levels=4, first_level=1, **spatial)
        a, b, c = _mse(plain["color"], clean[f], inside), _mse(bounded["color"], clean[f], inside), _mse(out, clean[f], inside)
        print(f"rectify: frame {f}: quadrant mse accumulate {a:.6g} bounded {b:.6g} full sequence {c:.6g}; "
              f"image mse noisy {_mse(noisy[f], clean[f]):.6g} bounded {_mse(bounded['color'], clean[f]):.6g}")
        if f > S.STEP_FRAME:
            assert b < a and c < b, f
        if 1 <= f < S.STEP_FRAME:  # the static frames; frame 0 is a reset, where the two are the same image
            assert _mse(bounded["color"], clean[f]) < _mse(noisy[f], clean[f]), f


# ---- refusals: the one check per call of rt_rectify.h behind the CPU form and, before any device work, both entry points of librt_amd.so ----

A, B, O, V, M, HI, HO = (C.c_void_p(4096 * k) for k in range(1, 8))  # never dereferenced: every call below is refused on its arguments
ODD = C.c_void_p(4096 + 8)


def _lib(entry):
    if entry == "cpu":
        lib = _capi.host_lib()
        return lib, lambda: lib.rt_host_last_error().decode()
    lib = _capi.amd_lib()
    return lib, lambda: lib.rt_last_error().decode()


def _name(base, entry):
    return base + {"cpu": "_cpu", "host": "_host", "device": ""}[entry]


def _ref(x):
    return None if x is None else C.byref(x)


def _bounds(entry, color, cs, obj, os_, valid, vs, p, rows, cols, box):
    lib, err = _lib(entry)
    args = [color, cs, obj, os_, valid, vs, _ref(p), rows, cols, box] + ([None] if entry == "device" else [])
    return getattr(lib, _name("rt_temporal_bounds", entry))(*args), err()


@pytest.mark.parametrize("entry", ["cpu", "host", "device"])
def test_bounds_refusals_in_order(entry):
    who = _name("rt_temporal_bounds", entry) + ": "
    P = _capi.BoundsParams
    good = P(1.0, 1, 0)
    # each case carries the later faults too: the first one is reported
    assert _bounds(entry, None, 0, None, 0, None, 0, None, 65536, 65536, None) == (UNSUPPORTED, who + "rows * cols: 2^32 pixels or more")
    assert _bounds(entry, None, 0, None, 0, None, 0, None, 0, 5, None)[0] == 0  # empty: nothing is looked at
    assert _bounds(entry, None, 2, O, 0, V, 0, None, 4, 4, None) == (INVALID, who + "null params")
    assert _bounds(entry, None, 2, O, 0, V, 0, P(-1.0, 0, 1), 4, 4, None) == (INVALID, who + "null color pointer")
    assert _bounds(entry, A, 2, O, 0, V, 0, P(-1.0, 0, 1), 4, 4, None) == (INVALID, who + "null box pointer")
    assert _bounds(entry, A, 2, O, 0, V, 0, P(-1.0, 0, 1), 4, 4, ODD) == (INVALID, who + "color_stride must be at least 3 words")
    assert _bounds(entry, A, 3, O, 0, V, 0, P(-1.0, 0, 1), 4, 4, ODD) == (INVALID, who + "object_stride must be at least 1 word")
    assert _bounds(entry, A, 3, O, 1, V, 0, P(-1.0, 0, 1), 4, 4, ODD) == (INVALID, who + "valid_stride must be at least 1 word")
    for radius in (0, 4):
        assert _bounds(entry, A, 3, O, 1, V, 1, P(-1.0, radius, 1), 4, 4, ODD) == (INVALID, who + "radius must be 1, 2 or 3")
    for gamma in (-1.0, float("inf"), float("nan")):
        assert _bounds(entry, A, 3, None, 0, None, 0, P(gamma, 3, 1), 4, 4, ODD) == (INVALID, who + "gamma must be >= 0 and finite")
    assert _bounds(entry, A, 3, O, 1, V, 1, P(0.0, 2, 1), 4, 4, ODD) == (INVALID, who + "flags: unknown bits (none is defined)")
    if entry == "device":
        assert _bounds(entry, A, 3, O, 1, V, 1, good, 4, 4, ODD) == (INVALID, who + "box must be 16-byte aligned")


def _accumulate(entry, color, motion, cur, prev, p, rows, cols, hin, hout, box, clamped_length):
    lib, err = _lib(entry)
    args = [color, motion, _ref(cur), _ref(prev), _ref(p), rows, cols, hin, hout, None, box, clamped_length, None] + ([None] if entry == "device" else [])
    return getattr(lib, _name("rt_temporal_accumulate_bounded", entry))(*args), err()


@pytest.mark.parametrize("entry", ["cpu", "host", "device"])
def test_accumulate_bounded_refusals_in_order(entry):
    who = _name("rt_temporal_accumulate_bounded", entry) + ": "
    g, p = _capi.TemporalGuides(), _capi.TemporalParams(0.9, 0.1, 0.05, 8, 0)
    # rt_temporal_accumulate's checks come first, with its texts
    assert _accumulate(entry, A, M, g, g, p, 65536, 65536, HI, HO, None, 9) == (UNSUPPORTED, who + "rows * cols: 2^32 pixels or more")
    assert _accumulate(entry, None, None, None, None, None, 0, 4, None, None, None, 9)[0] == 0
    assert _accumulate(entry, A, M, None, g, p, 4, 4, HI, HO, None, 9) == (INVALID, who + "null current guides")
    assert _accumulate(entry, A, M, g, g, p, 4, 4, HI, HI, None, 9) == (INVALID, who + "history_out must not be history_in")
    assert _accumulate(entry, A, M, g, g, _capi.TemporalParams(0.9, 0.1, 0.05, 8, 1), 4, 4, HI, HO, None, 9) == (INVALID, who + "flags: unknown bits (none is defined)")
    # then the box's
    assert _accumulate(entry, A, M, g, g, p, 4, 4, HI, HO, None, 9) == (INVALID, who + "null box pointer")
    if entry == "device":
        assert _accumulate(entry, A, M, g, g, p, 4, 4, HI, HO, ODD, 9) == (INVALID, who + "box must be 16-byte aligned")
    assert _accumulate(entry, A, M, g, g, p, 4, 4, HI, HO, B, 9) == (INVALID, who + "clamped_length must not exceed max_length (0: the length is not cut)")


def _feedback(entry, color, cs, valid, vs, rows, cols, history):
    lib, err = _lib(entry)
    args = [color, cs, valid, vs, rows, cols, history] + ([None] if entry == "device" else [])
    return getattr(lib, _name("rt_temporal_feedback", entry))(*args), err()


@pytest.mark.parametrize("entry", ["cpu", "host", "device"])
def test_feedback_refusals_in_order(entry):
    who = _name("rt_temporal_feedback", entry) + ": "
    assert _feedback(entry, None, 0, V, 0, 65536, 65536, None) == (UNSUPPORTED, who + "rows * cols: 2^32 pixels or more")
    assert _feedback(entry, None, 0, V, 0, 5, 0, None)[0] == 0
    assert _feedback(entry, None, 0, V, 0, 4, 4, None) == (INVALID, who + "null color pointer")
    assert _feedback(entry, A, 0, V, 0, 4, 4, None) == (INVALID, who + "null history pointer")
    assert _feedback(entry, A, 2, V, 0, 4, 4, ODD) == (INVALID, who + "color_stride must be at least 3 words")
    assert _feedback(entry, A, 3, V, 0, 4, 4, ODD) == (INVALID, who + "valid_stride must be at least 1 word")
    if entry == "device":
        assert _feedback(entry, A, 3, V, 1, 4, 4, ODD) == (INVALID, who + "history must be 16-byte aligned")


def test_the_wrappers_check_their_arrays():
    color, obj, valid = S.case_data(16, 16)
    with pytest.raises(ValueError, match="color"):
        rectify.bounds_numpy(color[:, :2], 16, 16)
    with pytest.raises(ValueError, match="object"):
        rectify.bounds_numpy(color, 16, 16, object=obj[:-1])
    with pytest.raises(ValueError, match="box"):
        rectify.accumulate_bounded_numpy(color, S.identity_motion(16, 16), 16, 16, np.zeros(256, dtype=temporal.HISTORY_DTYPE), np.zeros((256, 8), dtype=np.float32))
    with pytest.raises(ValueError, match="history"):
        rectify.feedback_numpy(color, np.zeros((256, 8), dtype=np.float32), 16, 16)
    with pytest.raises(_capi.RtError, match="radius"):
        rectify.bounds_numpy(color, 16, 16, radius=4)
