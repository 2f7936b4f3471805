"""Shared test support for the reference pins: the pinned pixels, the progressive loop by the oracle, and the RNG constant."""
import numpy as np

import _oracle


REFERENCE_EPOCHS = 7
PINS = [(0.04, "ref_out_distributed.png"), (0.02, "ref_out_small_blur.png")]


_whitted_cache = {}


def _whitted_normalised(world, camera, frame):
    key = (frame.width, frame.height, frame.max_depth)
    if key not in _whitted_cache:
        img, _ = _oracle.render_whitted(world.desc(), camera, frame)
        _oracle.post_process(img)
        _whitted_cache[key] = img
    return _whitted_cache[key].copy()


def progressive_loop(world, camera, frame, blur, epochs, focus=3.0):
    """main.rs:1087-1173 on the oracle; yields (k, u8 image) after the Whitted frame (k = 0) and after every epoch."""
    img = _whitted_normalised(world, camera, frame)
    yield 0, _oracle.encode_srgb8(img).astype(np.int32)
    states = _oracle.rng_init(frame)
    for k in range(1, epochs + 1):
        s, v, _ = _oracle.render_distributed(world.desc(), camera, frame, states, 1, focus=focus, blur=blur)
        img += np.where(v[0][..., None] != 0, s[0], np.float32(0))  # main.rs:1157-1167
        _oracle.post_process(img)                                    # main.rs:1171
        yield k, _oracle.encode_srgb8(img).astype(np.int32)


# rand 0.5.x src/prng/isaac.rs, #[test] fn test_isaac_new_uninitialized: IsaacRng::new_from_u64(0), 16 x next_u32()
RAND_05_NEW_FROM_U64_0 = [
    0x71D71FD2, 0xB54ADAE7, 0xD4788559, 0xC36129FA, 0x21DC1EA9, 0x3CB879CA, 0xD83B237F, 0xFA3CE5BD,
    0x8D048509, 0xD82E9489, 0xDB452848, 0xCA20E846, 0x500F972E, 0x0EEFF940, 0x00D6B993, 0xBC12C17F,
]
