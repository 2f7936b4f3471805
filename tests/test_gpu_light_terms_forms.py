"""The three forms of get_shade's light terms (main.rs:435-459) held together: rt_light_terms, rt_area_light_terms with one sample
equal to each light's stored origin or direction, and rt_light_terms_surfaces on unedited rt_material_hits records write the same
lit, diffuse and specular words on the same hits, incoming rays, asks and shadow hits — one body (csrc/rt_light_record.h light_terms)
behind three kernels.

Pairs of the three are also compared elsewhere, on casts' own shadow hits: test_gpu_textures.py (surfaces against rt_light_terms) and
test_gpu_area_lights.py (radius 0 against the light queries).  Here the shadow hits are crafted so that every branch of the body is
taken, and the test says so before it compares."""
import numpy as np
import pytest

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import arealights, materials, textures
import _scenes
from _records import NONE, dev, host, torch_device, u32, valid_rows

pytestmark = pytest.mark.gpu
F32 = np.float32
N = 130              # two full waves and a two-lane tail
DEAD = slice(64, 128)  # the second wave: every record "no hit", so the wave takes the ballot skip
NEARER, FARTHER = F32(0.25), F32(2.0)  # where an occluder lies on the way to the light's origin, as a share of that way


def lights():
    rng = np.random.default_rng(5)
    point, with_origin, without = _scenes.light(rng, 2), _scenes.light(rng, 0), _scenes.light(rng, 0)
    with_origin.has_origin, without.has_origin = 1, 0
    return [point, with_origin, without]


def test_the_three_forms_write_the_same_words():
    torch = torch_device()
    world = _scenes.random_world(3, 40, 3, n_lights=0)
    stored = lights()
    for l in stored:
        world.push_light(l)
    desc, scene = world.desc(), rt.Scene(world)
    rays_t = rt.camera_rays(_scenes.camera(0), rt.Frame.full(13, 10, 0))
    assert rays_t.shape[0] == N
    hits = u32(rt.cast_rays(scene, rays_t)).copy()
    hits[DEAD] = 0
    hits[DEAD, 0] = NONE
    valid = valid_rows(desc, hits)
    assert valid[:64].sum() >= 8 and valid[128:].any() and not valid[DEAD].any()  # hits in the first wave and in the tail; a dead wave
    hits_t = dev(hits)
    pos = hits[:, 3:6].view(F32)

    _, asks_t, _ = rt.light_rays(scene, hits_t, rays_t)
    asks = host(asks_t).reshape(3, N).copy()
    assert not asks[:, DEAD].any()
    shadow = np.zeros((3, N, 13), dtype=np.uint32)
    shadow[:, :, 0] = NONE
    seen = dict(none=0, nearer=0, farther=0, no_origin=0)
    case = np.full((3, N), -1)
    for l, light in enumerate(stored):
        asked = np.flatnonzero(asks[l])
        assert asked.size >= 6, f"light {l} asks at {asked.size} hits"
        case[l, asked] = np.arange(asked.size) % 3  # 0: no occluder, 1: one at NEARER, 2: one at FARTHER
        towards = (np.array(list(light.origin), dtype=F32) - pos) if light.has_origin or light.kind != 0 else -np.array(list(light.direction), dtype=F32)
        for c, share in ((1, NEARER), (2, FARTHER)):
            at = np.flatnonzero(case[l] == c)
            shadow[l, at, 0] = 1
            shadow[l, at, 3:6] = (pos[at] + towards[at] * share if towards.ndim == 2 else pos[at] + towards * share).astype(F32).view(np.uint32)
        if l < 2:
            seen["none"] += int((case[l] == 0).sum())
            seen["nearer"] += int((case[l] == 1).sum())
            seen["farther"] += int((case[l] == 2).sum())
        else:
            seen["no_origin"] += int((case[l] > 0).sum())
    assert all(count >= 2 for count in seen.values()), seen  # every branch of the body has entries, beside the dead wave
    asks[:, 64:128:2] = 1  # a caller's flags on records that are no hit: asked nowhere, whatever they say
    asks_t, shadow_t = torch.tensor(asks.reshape(-1), device="cuda"), dev(shadow.reshape(-1, 13))

    plain = rt.light_terms(scene, hits_t, rays_t, asks_t, shadow_t)
    sample = np.array([list(l.origin) if l.has_origin or l.kind != 0 else list(l.direction) for l in stored], dtype=F32)
    sample_t = torch.tensor(np.repeat(sample[:, None, :], N, axis=1).reshape(-1, 3), device="cuda")
    area = arealights.terms(scene, hits_t, rays_t, asks_t, sample_t, shadow_t, 1)
    surfaces = textures.light_terms_surfaces(scene, materials.material_hits(scene, hits_t), hits_t, rays_t, asks_t, shadow_t)

    lit = host(plain[0]).reshape(3, N)
    assert not lit[:, DEAD].any() and not lit[case == 1].any() and not lit[2][case[2] > 0].any()  # dead, nearer, no origin: occluded
    assert lit[:2][case[:2] == 2].any() and lit[case == 0].any()                                   # farther, none: lit somewhere
    assert host(plain[1]).any() and host(plain[2]).any()
    for name, form in (("area", area), ("surfaces", surfaces)):
        assert np.array_equal(host(form[0]), host(plain[0])), name
        for got, want in zip(form[1:], plain[1:]):
            assert np.array_equal(host(got).view(np.int32), host(want).view(np.int32)), name
