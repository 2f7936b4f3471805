"""The references of the post-stage tests (tests/_post_support.py) checked on the CPU: that each adversarial key set tells the correct
select from the wrong form it is named for, that the sort-based post_process and the host form agree, and the measurement behind the
encode tolerance.  No GPU."""
import numpy as np
import pytest

import homework_18_graphics_raytracer_amd as rt
import _post_support as ps

SETS = ps.key_sets()


def test_rank_rule_is_the_float32_one():
    assert [ps.rank_wanted(c) for c in (1, 2, 3, 99, 100, 101, 199, 200, 256, 257)] == [0, 1, 2, 98, 99, 99, 197, 198, 253, 254]
    assert ps.rank_wanted(100) == 99  # 100 * 0.99f is 99.0 in float32, the last element: a rank rule that took 98 would show here


@pytest.mark.parametrize("name", sorted(SETS))
def test_model_without_a_switch_is_the_sort(name):
    keys = SETS[name]
    key, hists = ps.radix_model(keys)
    assert key == ps.select_reference(keys)
    trace = ps.select_trace(keys)
    assert len(trace) == len(hists)
    for (hist, digit, _), seen in zip(trace, hists):
        assert np.array_equal(hist, seen) and seen[digit] > 0
    if trace:
        assert trace[3][2] < trace[3][0][trace[3][1]]  # the rank left after the last pick lies inside the last bin


def test_all_equal_sets_pick_digits_0_and_255_in_every_pass():
    digits = {name: [d for _, d, _ in ps.select_trace(SETS[name])] for name in SETS if name.startswith("all_equal")}
    assert digits["all_equal_00000000"] == [0, 0, 0, 0] and digits["all_equal_fffffffe"] == [255, 255, 255, 254]
    assert digits["all_equal_80000000"] == [0x80, 0, 0, 0]


@pytest.mark.parametrize("j", range(4))
def test_differ_in_byte_sets_have_one_full_bin_in_the_other_passes(j):
    for p, (hist, _, _) in enumerate(ps.select_trace(SETS[f"differ_in_byte_{j}"])):
        assert (np.count_nonzero(hist) == 1) == (p != j)


@pytest.mark.parametrize("p", range(4))
def test_boundary_sets_select_three_bins_and_catch_the_wrong_comparison(p):
    sets = [SETS[f"boundary_pass{p}_{n}"] for n in ("at_k", "at_k_plus_1", "at_k_minus_1")]
    picked = [ps.select_trace(s)[p][1] for s in sets]
    assert picked == [0x20, 0x10, 0x30]
    k = ps.rank_wanted(sets[0].size)
    assert [int(ps.select_trace(s)[p][0][:0x11].sum()) for s in sets] == [k, k + 1, k - 1]
    # `k <= c` for `k < c` ends with another key on the first and the third
    assert ps.radix_model(sets[0], pick_le=True)[0] != ps.select_reference(sets[0])
    assert ps.radix_model(sets[2], pick_le=True)[0] != ps.select_reference(sets[2])


@pytest.mark.parametrize("p", (1, 2, 3))
def test_decoy_sets_catch_a_mask_without_any_one_higher_byte(p):
    keys = SETS[f"decoys_pass{p}"]
    want = ps.select_reference(keys)
    assert want >> 24 == 0x80 and (want >> (24 - 8 * p)) & 0xFF == 0x40 + ps.DECOY_RANK
    top = keys >> 24
    real = ((keys >> np.uint32(32 - 8 * p)) == (want >> (32 - 8 * p))).sum()
    assert real == ps.DECOY_REAL and (top == 0x7F).sum() >= real and (top == 0x81).sum() >= real
    for j in range(p):
        assert ps.radix_model(keys, drop_mask_byte=j)[0] != want, j


def test_invalid_sets_catch_a_histogram_that_counts_invalid_keys():
    for name in ("invalid_99_percent", "invalid_but_one", "length_grid_stride"):
        good, bad = ps.radix_model(SETS[name])[1], ps.radix_model(SETS[name], count_invalid=True)[1]
        assert not np.array_equal(good[0], bad[0])  # the result is the same key (invalid keys sort last): the histogram is what differs
    assert ps.select_reference(SETS["invalid_all"]) is None and ps.select_trace(SETS["invalid_all"]) == []
    assert (SETS["invalid_99_percent"] == ps.KEY_INVALID).mean() == 0.99


def test_grid_stride_set_is_decided_beyond_the_first_stride():
    keys = SETS["length_grid_stride"]
    assert keys.size > ps.GRID_CAP
    want = ps.select_reference(keys)
    assert want in keys[ps.GRID_CAP:] and want not in keys[:ps.GRID_CAP]
    assert ps.select_reference(keys[:ps.GRID_CAP]) != want


@pytest.mark.parametrize("parts", (2, 3))
def test_bands_hold_every_key_once(parts):
    keys = SETS["length_1000"]
    bands = ps.bands_of(keys, parts)
    assert bands[-2].size == 0 and (bands[-1] == ps.KEY_INVALID).all()
    joined = np.concatenate(bands)
    assert np.array_equal(np.sort(joined[joined != ps.KEY_INVALID]), np.sort(keys[keys != ps.KEY_INVALID]))


# ---- key map and post_process ---------------------------------------------------------------------------------------------------------

def test_luma_class_image_reaches_every_class():
    row = rt.luma_row()
    luma = ps.luma_reference(ps.luma_class_image(row), row)
    normal = ps.is_normal(luma)
    b = ps.bits(luma)
    for want in (0x00800000, 0x80800000, 0x007FFFFF, 0x807FFFFF, 0x00000000, 0x7F800000, 0xFF800000, 0x34000000, 0x34000001):
        assert (b == want).any(), hex(want)
    assert not (b == 0x80000000).any()  # a -0 input gives a +0 luma: the products of the +0 channels are added to it
    assert np.isnan(luma).sum() >= 12 and normal.sum() > 40 and (~normal).sum() > 40
    assert (np.abs(luma[np.isfinite(luma)]).max() > 1e38) and normal[b == 0x00800000].all() and not normal[b == 0x007FFFFF].any()


@pytest.mark.parametrize("content", ps.POST_CONTENTS)
@pytest.mark.parametrize("shape", ps.POST_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_post_process_equals_the_sort(shape, content):
    row = rt.luma_row()
    img = ps.post_image(shape, content, row)
    want, wdiv = ps.post_process_reference(img, row)
    got = img.copy()
    div = rt.post_process(got)
    assert np.float32(div) == wdiv and np.array_equal(ps.bits(got), ps.bits(want))
    n = shape[0] * shape[1]
    luma = ps.luma_reference(img, row)
    if content in ("negative_percentile", "selected_is_epsilon", "abnormal_all"):
        assert wdiv == 0 and want is img
    if content == "negative_percentile":
        assert ((luma > 0).sum() > 0) == (n > 100)
    if content == "selected_above_epsilon":
        assert ps.bits(np.array([wdiv]))[0] == 0x34000001
    if content == "abnormal_30_percent" and n >= 100:
        assert 0.15 < (~ps.is_normal(luma)).mean() < 0.45 and wdiv > 0


# ---- the encode -----------------------------------------------------------------------------------------------------------------------

def test_encode_inputs_cover_every_transition():
    t = ps.encode_transitions()
    assert t.size == 255 and (np.diff(t) > 0).all()
    assert np.array_equal(ps.encode_reference(t), np.arange(1, 256))
    below = (ps.bits(t) - 1).view(np.float32)
    assert np.array_equal(ps.encode_reference(below), np.arange(0, 255))
    x = ps.encode_inputs()
    assert 130_000 < x.size < 150_000 and set(np.unique(ps.encode_reference(x))) == set(range(256))


def test_encode_tolerance_covers_the_branch_point():
    assert 1.1e-4 < ps.ENCODE_DELTA < 1.3e-4
    t = float(np.float32(0.0031308))
    gap = abs(255 * 12.92 * t - 255 * (1.055 * t ** (1 / 2.4) - 0.055))
    linear = 255 * 12.92 * 0.0031308 * 3 * ps.U
    assert gap < 255e-5 and gap + linear < ps.ENCODE_DELTA
    assert np.nextafter(np.float32(0.0031308), np.float32(0)) < 0.0031308  # no float between the constant and its rounding


def test_host_encode_within_the_tolerance_and_the_cap(capsys):
    x = ps.encode_inputs()
    got = rt.encode_srgb8(np.ascontiguousarray(x))
    differing, farthest = ps.check_encode(got, x)
    cap = ps.encode_excused_cap(x)
    with capsys.disabled():
        print(f"\nencode: {x.size} inputs, {int((ps.encode_distance(x) <= ps.ENCODE_DELTA).sum())} within delta={ps.ENCODE_DELTA:.3e} of an integer, "
              f"cap {cap}; host differs on {differing}, farthest {farthest:.3e}")
    assert differing <= cap
    assert farthest <= ps.ENCODE_MEASURED <= ps.ENCODE_DELTA


# ---- the accumulator ------------------------------------------------------------------------------------------------------------------

def test_accumulator_reference_known_answers():
    s = np.array([[[[1.0, 2.0, 3.0]]], [[[0.5, 0.25, 0.125]]], [[[np.nan, 100.0, 100.0]]]], dtype=np.float32)
    v = np.array([[[1]], [[1]], [[0]]], dtype=np.uint8)
    acc, w = np.zeros((1, 1, 3), np.float32), np.zeros((1, 1), np.float32)
    ps.accumulate_reference(s, v, acc, w)
    assert acc.reshape(-1).tolist() == [1.5, 2.25, 3.125] and w.item() == 2.0
    assert ps.resolve_reference(acc, w).reshape(-1).tolist() == [0.75, 1.125, 1.5625]
    weights = np.array([[0.0, 2.0 ** -24, 2.0 ** -23, 1.0]], np.float32)
    out = ps.resolve_reference(np.ones((1, 4, 3), np.float32), weights)
    assert out[0, :, 0].tolist() == [0.0, 0.0, 2.0 ** 23, 1.0]
