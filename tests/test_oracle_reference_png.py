"""Pin the oracle against the ONLY output artefact the reference ships for the deterministic pass:
report/out_single_epoch.png (copied verbatim to tests/golden/ref_out_single_epoch.png), a 1280x960
render at depth 5 (main.rs:1084-1085, 1098) after post_process + sRGB/u8 encode.

Measured when this test was written: 99.9997 % of the 3 686 400 channels identical, max |diff| = 1.
The residue is a dozen channels whose value sits within an f32 ulp of an integer before the truncating
u8 cast — exactly what a last-bit difference in libm's powf produces (DESIGN.md "Parity status").
"""
import numpy as np
import pytest
from PIL import Image

import homework_18_graphics_raytracer_amd as rt
import _oracle
from _reference_support import PINS, progressive_loop, REFERENCE_EPOCHS


@pytest.fixture(scope="module")
def ref_png():
    return np.asarray(Image.open(_oracle.GOLDEN / "ref_out_single_epoch.png").convert("RGB")).astype(np.int32)


@pytest.fixture(scope="module")
def setup():
    world = rt.reference_world()
    return world, rt.reference_camera(), rt.Frame.full(1280, 960, 5)


def _encode(img, kind, luma_mode=0):
    im = img.copy()
    _oracle.post_process(im, luma_mode, kind)
    return _oracle.encode_srgb8(im, kind).astype(np.int32)


def test_oracle_matches_reference_image(setup, ref_png):
    world, camera, frame = setup
    img, casts = _oracle.render_whitted(world.desc(), camera, frame)
    u8 = _encode(img, "detmath")
    diff = np.abs(u8 - ref_png)
    assert diff.max() <= 1
    assert np.mean(diff == 0) >= 0.9999, f"only {np.mean(diff == 0):.6f} of the channels identical"
    assert casts == 11594468  # pinned cast count of the reference configuration


def test_u8_conversion_truncates_and_luma_uses_palette_matrix(setup, ref_png):
    """Two crate behaviours the reference image discriminates: a rounding u8 conversion or the literal
    Rec.709 luma constants both fit the image markedly worse than what the oracle restates."""
    world, camera, frame = setup
    img, _ = _oracle.render_whitted(world.desc(), camera, frame)
    im = img.copy()
    _oracle.post_process(im, 0)
    x = im.astype(np.float64)
    e = np.where(x <= 0.0031308, 12.92 * x, 1.055 * np.power(np.maximum(x, 0), 1 / 2.4) - 0.055)
    rounded = np.clip(np.round(e * 255.0), 0, 255).astype(np.int32)
    assert np.mean(rounded == ref_png) < 0.60          # rounding: ~56 % identical
    assert np.mean(_encode(img, "detmath", 0) == ref_png) > np.mean(_encode(img, "detmath", 1) == ref_png)


def test_glibc_libm_variant_is_close_but_not_closer(setup, ref_png):
    """With glibc's libm (what a Rust build on this machine would call) the image differs from the
    deterministic-math oracle only in a few knife-edge pixels; the detmath oracle is at least as close
    to the reference image."""
    world, camera, frame = setup
    img_l, _ = _oracle.render_whitted(world.desc(), camera, frame, kind="libm")
    img_d, _ = _oracle.render_whitted(world.desc(), camera, frame, kind="detmath")
    u_l, u_d = _encode(img_l, "libm"), _encode(img_d, "detmath")
    assert np.mean(np.abs(u_l - ref_png) <= 1) >= 0.9999
    assert np.mean(u_d == ref_png) >= np.mean(u_l == ref_png)
    assert np.mean(u_l == u_d) >= 0.9995


# ---- the stochastic pass: main()'s progressive loop, pinned per pixel -------------------------------------------------
#
# report/out.png and report/out_small_blur.png (tests/golden/ref_out_distributed.png, ref_out_small_blur.png) are the
# files main() had rewritten after its SEVENTH depth-of-field epoch (the author stopped the 100-epoch loop there):
# Whitted frame -> post_process -> 7 x {one epoch of shoot_focus(3.0, blur) + distributed_ray_trace added where all three
# channels are normal, post_process} -> sRGB/u8 (main.rs:1087-1173), with blur 0.04 (main.rs:1148's literal) for out.png
# and 0.02 for out_small_blur.png.  At exactly 7 epochs the oracle reproduces both to the last u8 but for a handful of
# channels off by one; at any other epoch count 10-18 % of the channels agree.  This pins, against reference-held
# outputs: IsaacRng::new_from_u64(y * 2^33 + x) and its output order, Uniform<f32>, the ziggurat Normal and its
# regenerated tables, shoot_focus, weighted_select, scatter_hit, distributed_ray_trace, the is_normal filter, the
# accumulation into the normalised image and the in-place renormalisation.


@pytest.mark.parametrize("blur,name", PINS)
def test_oracle_progressive_loop_matches_the_reference_image_at_seven_epochs(setup, blur, name):
    world, camera, frame = setup
    ref = np.asarray(Image.open(_oracle.GOLDEN / name).convert("RGB")).astype(np.int32)
    identical = {}
    for k, u8 in progressive_loop(world, camera, frame, blur, REFERENCE_EPOCHS + 1):
        diff = np.abs(u8 - ref)
        identical[k] = float(np.mean(diff == 0))
        if k == REFERENCE_EPOCHS:
            assert diff.max() <= 1, f"max |diff| {diff.max()} at {k} epochs"
            assert identical[k] >= 0.9999, f"only {identical[k]:.6f} of the channels identical at {k} epochs"
    # an epoch count that drifts by one cannot pass: neighbours of 7 are far away
    assert identical[REFERENCE_EPOCHS - 1] < 0.5 and identical[REFERENCE_EPOCHS + 1] < 0.5, identical


def test_the_two_reference_images_differ_by_their_blur_only_in_the_stochastic_part(setup):
    """The other blur value does not reproduce either image (so `blur` is pinned, not just the epoch count)."""
    world, camera, frame = setup
    ref = np.asarray(Image.open(_oracle.GOLDEN / "ref_out_small_blur.png").convert("RGB")).astype(np.int32)
    *_, (k, u8) = progressive_loop(world, camera, frame, 0.04, REFERENCE_EPOCHS)
    assert k == REFERENCE_EPOCHS and np.mean(u8 == ref) < 0.8
