"""The HIP path against the reference's OWN outputs for the stochastic loop (main.rs:1117-1173), per pixel.

report/out.png and report/out_small_blur.png (tests/golden/ref_out_distributed.png, ref_out_small_blur.png) are what
main() had written after its seventh depth-of-field epoch, with blur 0.04 (main.rs:1148) and 0.02: Whitted frame ->
post_process -> 7 x {epoch: shoot_focus + distributed_ray_trace, is_normal filter, add, post_process} -> sRGB/u8.  The
oracle reproduces both to max |diff| 1 with >= 99.99 % of the channels identical (tests/test_oracle_reference_png.py);
here the same loop runs on the GPU, twice: through the command-line driver over the host-buffer entry points, and
entirely device-resident (render, radix-select post_process and encode on the GPU) — and must (i) meet the same bar
against the reference images and (ii) equal the oracle's u8 image exactly.  Also: rand 0.5's published
`IsaacRng::new_from_u64(0)` vector from the device's seeding.
"""
import ctypes as C
import subprocess

import numpy as np
import pytest
from PIL import Image

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import _capi
import _oracle
from _reference_support import PINS, progressive_loop, RAND_05_NEW_FROM_U64_0, REFERENCE_EPOCHS

pytestmark = pytest.mark.gpu

W, H, DEPTH = 1280, 960, 5  # main.rs:1084-1085, 1098


def _png(name_or_path):
    path = name_or_path if "/" in str(name_or_path) else _oracle.GOLDEN / name_or_path
    return np.asarray(Image.open(path).convert("RGB")).astype(np.int32)


@pytest.fixture(scope="module")
def oracle_u8():
    """The oracle's u8 image after 7 epochs for each blur (the CPU loop of test_oracle_reference_png)."""
    world, camera, frame = rt.reference_world(), rt.reference_camera(), rt.Frame.full(W, H, DEPTH)
    out = {}
    for blur, _ in PINS:
        *_, (k, u8) = progressive_loop(world, camera, frame, blur, REFERENCE_EPOCHS)
        assert k == REFERENCE_EPOCHS
        out[blur] = u8
    return out


def _check_against_reference(u8, name, oracle):
    ref = _png(name)
    diff = np.abs(u8 - ref)
    assert diff.max() <= 1, f"max |diff| {diff.max()} vs {name}"
    assert np.mean(diff == 0) >= 0.9999, f"only {np.mean(diff == 0):.6f} of the channels identical to {name}"
    assert np.array_equal(u8, oracle), "the GPU loop's u8 image differs from the oracle's"


@pytest.mark.parametrize("blur,name", PINS)
def test_rt_render_seven_epochs_reproduces_the_reference_png(tmp_path, oracle_u8, blur, name):
    out = tmp_path / "out.png"
    cmd = [str(_capi.PKG_DIR / "rt_render"), "--obj", rt.DEFAULT_OBJ, "--out", str(out), "--epochs", str(REFERENCE_EPOCHS),
           "--blur", repr(blur), "--focus", "3.0"]
    done = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert done.returncode == 0, done.stderr
    assert done.stdout.count("rays in") == 1 + REFERENCE_EPOCHS
    _check_against_reference(_png(out), name, oracle_u8[blur])


@pytest.mark.parametrize("blur,name", PINS)
def test_device_resident_loop_reproduces_the_reference_png(oracle_u8, blur, name):
    """render_whitted -> post_process_device -> 7 x {render_distributed(accum=img), post_process_device} ->
    encode_srgb8_device: nothing but the final u8 image leaves the GPU.  One epoch short or long is far away."""
    import torch

    scene, camera, frame = rt.Scene(rt.reference_world()), rt.reference_camera(), rt.Frame.full(W, H, DEPTH)
    img = rt.render_whitted(scene, camera, frame)
    rt.post_process_device(img)
    rng = rt.Rng(frame)
    ref = _png(name)
    identical = {}
    for k in range(1, REFERENCE_EPOCHS + 2):
        rt.render_distributed(scene, camera, frame, rng, 1, focus=3.0, blur=blur, accum=img)
        rt.post_process_device(img)
        if k >= REFERENCE_EPOCHS - 1:
            u8 = rt.encode_srgb8_device(img).cpu().numpy().astype(np.int32)
            identical[k] = float(np.mean(u8 == ref))
            if k == REFERENCE_EPOCHS:
                _check_against_reference(u8, name, oracle_u8[blur])
    torch.cuda.synchronize()
    assert identical[REFERENCE_EPOCHS - 1] < 0.5 and identical[REFERENCE_EPOCHS + 1] < 0.5, identical


def test_device_seeding_yields_rands_published_new_from_u64_zero_vector():
    """rt_rng_create on the single pixel (0,0) -> seed 0 (main.rs:1119): the downloaded record, drawn from with the
    reference's BlockRng order, gives rand 0.5's `test_isaac_new_uninitialized` words; after one device epoch the
    device record still equals the oracle's record advanced by the same epoch (the stream the kernels consumed)."""
    frame = rt.Frame(8, 8, 5, 0, 0, 1, 1, 1)
    rng = rt.Rng(frame)
    st = rng.download()
    assert st.shape == (1, 516)
    L = _oracle._dist_lib()
    rec = st[0].copy()
    out = np.empty(16, dtype=np.uint32)
    L.orc_rng_draw_u32(rec.ctypes.data, out.ctypes.data, 16)
    assert [int(v) for v in out] == RAND_05_NEW_FROM_U64_0

    import torch

    scene, camera = rt.Scene(rt.reference_world()), rt.reference_camera()
    samples = torch.empty((1, 1, 1, 3), dtype=torch.float32, device="cuda")
    valid = torch.empty((1, 1, 1), dtype=torch.uint8, device="cuda")
    rt.render_distributed(scene, camera, frame, rng, 1, samples=samples, valid=valid)
    torch.cuda.synchronize()
    states = _oracle.rng_init(frame)
    want_s, want_v, _ = _oracle.render_distributed(scene._desc, camera, frame, states, 1)
    assert np.array_equal(rng.download(), states)
    assert np.array_equal(samples.cpu().numpy().view(np.uint32), want_s.view(np.uint32))
