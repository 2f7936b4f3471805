"""The motion queries' CPU definition (rt_previous_positions_cpu, librt_host.so) against the numpy restatement of
include/rt_amd.h "motion queries", bit for bit, on oracle hits; and the property the block exists for: after a rigid motion of scene and
camera together, every pixel's was-position projects onto its own centre in the previous frame.  No device."""
import ctypes as C

import numpy as np
import pytest

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import _capi, moving
import _motion_support as ms
import _records
import _scenes
import _temporal_support as ts
from _scene_update_support import desc_with

INVALID, UNSUPPORTED = -1, -5


base, moved, CASES = ms.base, ms.moved, ms.CASES


def test_the_rays_reach_every_primitive_from_both_sides():
    _, d, verts, sph = base()
    hits = _records.oracle_hits(d, ms.primitive_rays(verts, sph))
    tri, s = hits[hits[:, 0] == 1], hits[hits[:, 0] == 0]
    assert set(tri[:, 1]) == set(range(d.n_triangles)) and set(s[:, 1]) == set(range(d.n_spheres))
    assert set(tri[:, 11]) == {0, 1} and set(s[:, 11]) == {0, 1}  # front- and back-face hits of both kinds
    frame = moved("nothing")[3]
    assert (frame[:, 0] == _records.NONE).any() and (frame[:, 0] == 0).any() and (frame[:, 0] == 1).any()


@pytest.mark.parametrize("name", CASES)
def test_cpu_form_equals_the_restatement_bit_for_bit(name):
    which = "dome" if name == "dome deformed" else "small"
    _, _, verts, sph = base(which)
    now, v, s, hits = moved(name)
    wt, ws = ms.kept_of(verts, sph)
    want = ms.restate(v, s, verts, ws, hits)
    got = moving.previous_positions_numpy(now, wt, ws, hits)
    assert np.array_equal(got.view(np.uint32), want)
    position, none = hits[:, 3:6], hits[:, 0] == _records.NONE
    assert (got.view(np.uint32)[none] == ms.NAN_WORD).all() and none.any()
    differs = (got.view(np.uint32) != position).any(axis=1) & ~none
    if name == "nothing":
        assert not differs.any()
    elif name == "one vertex":
        assert differs.any() and (hits[differs, 0] == 1).all() and (hits[differs, 1] == 7).all()
        assert differs[(hits[:, 0] == 1) & (hits[:, 1] == 7)].all()
    elif name == "sphere moved and rescaled":
        assert differs.any() and (hits[differs, 0] == 0).all() and set(hits[differs, 1]) == {1, 2}
    elif name == "degenerate":
        assert np.isnan(got[-5:-3]).all() and not np.isfinite(got[-1]).all()  # whatever the divides give: here no number
    else:
        triangles = hits[:, 0] == 1  # a deformation moves the triangles alone, the rigid motion everything
        assert differs[triangles].mean() > 0.9 and differs[hits[:, 0] == 0].all() == (name == "rigid")


def test_an_unmoved_primitive_returns_the_raw_words_of_the_position():
    _, d, verts, sph = base()
    hits = ms.payload_hits(moved("nothing")[3])
    wt, ws = ms.kept_of(verts, sph)
    got = moving.previous_positions_numpy(d, wt, ws, hits).view(np.uint32)
    assert np.array_equal(got, hits[:, 3:6]) and got[0, 0] == 0x7FC12345 and got[0, 1] == 0x80000000
    # -0.0 kept against +0.0 now compares equal to zero: still unmoved
    v = np.array(verts)
    v[hits[0, 1], 0, 0] = 0.0
    wt2 = ms.kept_of(v, sph)[0].copy()
    wt2[hits[0, 1], 0] = -0.0
    got = moving.previous_positions_numpy(desc_with(d, verts=v), wt2, ws, hits[:1]).view(np.uint32)
    assert np.array_equal(got, hits[:1, 3:6])


def test_records_that_are_no_hit_of_the_scene_get_three_nan_words():
    _, d, verts, sph = base()
    now, v, s, hits = moved("deformed")
    wt, ws = ms.kept_of(verts, sph)
    bad = ms.special_hits(hits, d.n_triangles, d.n_spheres)
    got = moving.previous_positions_numpy(now, wt, ws, bad).view(np.uint32)
    assert (got == ms.NAN_WORD).all() and np.array_equal(got, ms.restate(v, s, verts, ws, bad))


def test_stride_3_and_stride_5_with_the_other_words_left_intact():
    _, d, verts, sph = base()
    now, v, s, hits = moved("deformed")
    wt, ws = ms.kept_of(verts, sph)
    want = ms.restate(v, s, verts, ws, hits)
    rc, _, out3 = ms.cpu(now, wt, ws, hits, 3, fill=0xDEADBEEF)
    assert rc == 0 and np.array_equal(out3, want)
    rc, _, out5 = ms.cpu(now, wt, ws, hits, 5, fill=0xDEADBEEF)
    assert rc == 0 and np.array_equal(out5[:, :3], want) and (out5[:, 3:] == 0xDEADBEEF).all()


def _rigid_figures(rot, shift, spheres_too):
    """(pixels asserted, float32 against binary64, distance from the own centre, the same with the current positions) in pixels"""
    _, d, verts, sph = base()
    v, s = ms.rigid(verts, sph, rot, shift)
    now = desc_with(d, verts=v, spheres=s)
    cam_prev = _scenes.camera(2)
    cam_now = ms.rigid_camera(cam_prev, rot, shift)
    rows, cols = ms.RIGID_ROWS, ms.RIGID_COLS
    frame = rt.Frame.full(cols, rows, 3)
    hits = _records.oracle_hits(now, _records.camera_rays_cpu(cam_now, cols, rows))
    valid = (hits[:, 0] <= 1) if spheres_too else (hits[:, 0] == 1)
    wt, ws = ms.kept_of(verts, sph)
    was = moving.previous_positions_numpy(now, wt, ws, hits)
    assert np.array_equal(was.view(np.uint32), ms.restate(v, s, verts, ws, hits))
    got = ts.restate_motion(was, cam_prev, frame)[valid].astype(np.float64)
    y, x = np.divmod(np.flatnonzero(valid), cols)
    centre = np.stack([x, y], axis=1).astype(np.float64)
    # the derivation's measurement: the same steps in binary64 from the same float32 inputs
    was64 = ms.restate(v, s, verts, ws, hits, dtype=np.float64)
    got64 = ts.restate_motion(np.where(valid[:, None], was64, 1.0), cam_prev, frame, dtype=np.float64)[valid]
    current = ts.restate_motion(hits[:, 3:6].copy().view(np.float32), cam_prev, frame)[valid].astype(np.float64)
    return hits[valid, 0], np.abs(got - got64).max(), np.abs(got - centre).max(), np.abs(current - centre).max(axis=1).max()


def test_rigid_motion_of_scene_and_camera_projects_onto_the_pixels_own_centre():
    """THE property: scene and camera moved together, so nothing moved on screen, and every valid pixel's was-position projects onto the
    pixel's own centre in the previous frame.  A rotation is asserted on the pixels whose hit is on a triangle — rt_sphere has no
    orientation, the definition models none, and a point of a sphere turned about another axis than its own is a different point — and a
    translation on every valid pixel, spheres too.  The bound and its derivation: _motion_support."""
    worst = 0.0
    for name, rot, shift, spheres_too in (("rotation and translation", ms.RIGID_ROT, ms.RIGID_SHIFT, False),
                                          ("translation", np.eye(3), ms.RIGID_SHIFT, True)):
        kinds, measured, off, contrast = _rigid_figures(rot, shift, spheres_too)
        print(f"{name}: {kinds.size} pixels of {ms.RIGID_ROWS * ms.RIGID_COLS} (on triangles {(kinds == 1).sum()}, on spheres {(kinds == 0).sum()}); "
              f"float32 against binary64: {measured:.3g} pixels; from the own centre: {off:.3g} pixels (bound {ms.RIGID_BOUND:.3g}); "
              f"the current positions instead: up to {contrast:.3g} pixels")
        assert (kinds == 1).sum() > 1500 and ((kinds == 0).sum() > 500) == spheres_too
        assert off <= ms.RIGID_BOUND
        assert contrast > 0.5
        worst = max(worst, measured)
    print(f"float32 against binary64, the larger of the two: {worst:.4g} pixels (RIGID_MEASURED {ms.RIGID_MEASURED:.3g})")
    assert worst <= ms.RIGID_MEASURED  # the bound stands on this figure: a larger one means the derivation is out of date


# ---- refusals, in the stated order ----


def _call(now, wt, ws, hits, n, was, stride):
    lib = _capi.host_lib()
    rc = lib.rt_previous_positions_cpu(None if now is None else C.byref(now), wt, ws, hits, n, was, stride)
    return rc, lib.rt_host_last_error().decode()


def test_refusals_return_their_status_and_message_in_order():
    _, d, _, _ = base()
    A, B, H, W = (C.c_void_p(4096 * k) for k in (1, 2, 3, 4))  # never dereferenced: every call below is refused on its arguments
    empty = _capi.SceneDesc()
    # each case also carries every LATER fault it can, so the message shows which check came first
    cases = [
        ("2^32 records", UNSUPPORTED, (None, None, None, None, 1 << 32, None, 0), "2^32 records or more (checked first"),
        ("null scene", INVALID, (None, None, None, None, 5, None, 0), "null scene"),
        ("no kept triangles", INVALID, (d, None, B, None, 5, None, 0), "null was_triangles with n_triangles > 0"),
        ("no kept spheres", INVALID, (d, A, None, None, 5, None, 0), "null was_spheres with n_spheres > 0"),
        ("null hits", INVALID, (d, A, B, None, 5, W, 0), "null hit or was pointer"),
        ("null was", INVALID, (d, A, B, H, 5, None, 0), "null hit or was pointer"),
        ("stride", INVALID, (d, A, B, H, 5, W, 2), "was_stride must be at least 3 words"),
    ]
    for name, want, args, text in cases:
        rc, msg = _call(*args)
        assert rc == want and msg.startswith("rt_previous_positions_cpu: ") and text in msg, (name, rc, msg)
    assert _call(d, A, B, None, 0, None, 0)[0] == 0  # nothing to do: the pointers are not looked at
    assert _call(empty, None, None, None, 0, None, 0)[0] == 0  # a scene with nothing to keep needs no kept arrays
    assert _call(d, None, None, None, 0, None, 0)[0] == INVALID  # ... but "never kept" comes before "nothing to do"
    with pytest.raises(rt.RtError, match="was_triangles"):
        moving.previous_positions_numpy(d, None, np.zeros((3, 4), dtype=np.float32), np.zeros((1, 13), dtype=np.uint32))
    with pytest.raises(ValueError, match="was_spheres"):
        moving.previous_positions_numpy(d, np.zeros((40, 9), dtype=np.float32), np.zeros((2, 4), dtype=np.float32), np.zeros((1, 13), dtype=np.uint32))
