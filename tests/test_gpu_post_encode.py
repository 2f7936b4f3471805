"""rt_encode_srgb8_device at its edges: every transition of the output code with the 256 floats on either side, the branch point of the
transfer, 0 and 1, and the values a frame never holds — against the host form byte for byte and against a float64 reference within the
derived tolerance (tests/_post_support.py: ENCODE_DELTA and the cap on the bytes it excuses)."""
import numpy as np
import pytest

import homework_18_graphics_raytracer_amd as rt
import _post_support as ps

pytestmark = pytest.mark.gpu


def _device(x):
    import torch

    out = torch.full((x.size + 2,), 0xA5, dtype=torch.uint8, device="cuda")
    rt.encode_srgb8_device(torch.from_numpy(np.ascontiguousarray(x).copy()).cuda(), out=out[1:-1])
    got = out.cpu().numpy()
    assert got[0] == 0xA5 and got[-1] == 0xA5  # nothing written outside
    return got[1:-1]


def test_whole_input_set_against_host_and_float64():
    x = ps.encode_inputs()
    got = _device(x)
    assert np.array_equal(got, rt.encode_srgb8(np.ascontiguousarray(x)))
    differing, farthest = ps.check_encode(got, x)
    print(f"encode on the device: {differing} of {x.size} bytes differ from float64, farthest {farthest:.3e}, cap {ps.encode_excused_cap(x)}")
    assert differing <= ps.encode_excused_cap(x)


@pytest.mark.parametrize("length", (1, 255, 256, 257))
def test_short_lengths(length):
    x = ps.encode_inputs()
    rng = np.random.default_rng(length)
    for part in (x[:length], x[-length:], x[rng.choice(x.size, length, replace=False)]):
        got = _device(part)
        assert np.array_equal(got, rt.encode_srgb8(np.ascontiguousarray(part)))
        ps.check_encode(got, part)


def test_length_beyond_one_grid():
    """above 2048 * 256 values the kernel runs grid-stride: the input set tiled four times, then 257 more"""
    x = ps.encode_inputs()
    x = np.concatenate([np.tile(x, 4), x[1000:1257]])
    assert x.size > ps.GRID_CAP
    got = _device(x)
    assert np.array_equal(got, rt.encode_srgb8(np.ascontiguousarray(x)))
    ps.check_encode(got, x)
