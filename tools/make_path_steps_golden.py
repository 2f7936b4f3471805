#!/usr/bin/env python3
"""Record tests/golden/path_steps.npz: every word the eleven CPU forms of the path loop (paths.*_numpy and paths.light_seed) write for
one crafted batch of M = 67 slots, under every way of listing them.  tests/test_path_steps_golden.py runs steps() again and asks for
the same words, so a change of the loop's plumbing — the slot walk, the record codec, the surface reader — that moves a bit shows up
against words recorded before it, not against a form that shares the headers being edited.  Only the package is imported; no GPU.

    python tools/make_path_steps_golden.py        # rewrites the fixture: only for a change that is meant to move bits

The batch: dead slots (flags 0, DARK), "no hit" vertices (with and without a density in the record), glass vertices (transparency 1
and 0.5), mirrors and matte surfaces, bounce counts on both sides of rr_start; a spot, a point and a directional light.  The lists:
none (all M), an index list with a repeated entry, entries >= M and a count > M, the same list cut short, and a count of 0.
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import homework_18_graphics_raytracer_amd as rt  # noqa: E402
from homework_18_graphics_raytracer_amd import environment, paths as P  # noqa: E402
from homework_18_graphics_raytracer_amd._capi import Light  # noqa: E402
from homework_18_graphics_raytracer_amd.materials import SURFACE_DTYPE  # noqa: E402

FIXTURE = ROOT / "tests" / "golden" / "path_steps.npz"
F32, U32, U8 = np.float32, np.uint32, np.uint8
M = 67
SEED = 0xC0FFEE
NO_HIT = 0xFFFFFFFF  # RT_HIT_NONE as a u32 word
WIDE = ("all",)
DEAD, DARKENED, MISSES, MISSES_FROM_CAMERA, GLASS, HALF_GLASS = (3, 40), (11,), (5, 23, 66), (31,), (7, 50), (9, 64)


def _unit(v):
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(F32)


def lists():
    """name -> (index, count): the ways of listing the slots"""
    index = np.array([4, 7, 7, 0, 66, 67, 5, 200, 9, 0xFFFFFFFF, 23, 31, 64, 65, 50, 11, 3, 12, 1, 2], dtype=U32)
    return {"all": (None, None), "list": (index, 100), "short": (index, 6), "none": (index, 0)}


def batch():
    """the crafted slots: (surfaces, hits, incoming, view, positions, paths, radiance, emitted)"""
    rng = np.random.default_rng(20240607)
    surfaces = np.zeros(M, dtype=SURFACE_DTYPE)
    surfaces["normal"] = _unit(rng.normal(size=(M, 3)) * 0.2 + np.array([0.0, 1.0, 0.0]))
    surfaces["shading_normal"] = _unit(surfaces["normal"] + rng.normal(size=(M, 3)) * 0.05)
    surfaces["diffuse_color"] = rng.uniform(0.1, 1.0, (M, 3)).astype(F32)
    surfaces["specular_color"] = rng.uniform(0.1, 1.0, (M, 3)).astype(F32)
    surfaces["shiness"] = rng.uniform(0.0, 1.0, M).astype(F32)
    surfaces["shiness"][[1, 2]] = 0.0, 1.0  # matte, mirror
    surfaces["smoothness"] = rng.uniform(1.0, 60.0, M).astype(F32)
    surfaces["refraction_index"] = rng.uniform(1.1, 1.8, M).astype(F32)
    surfaces["opaque_decay"] = rng.uniform(0.2, 1.0, M).astype(F32)
    surfaces["transparency"][list(GLASS)] = 1.0
    surfaces["transparency"][list(HALF_GLASS)] = 0.5
    surfaces["valid"] = 1
    view = _unit(rng.normal(size=(M, 3)) * 0.4 + np.array([0.0, 1.0, 0.0]))
    positions = np.column_stack([rng.uniform(-1.5, 1.5, M), np.zeros(M), rng.uniform(-1.5, 1.5, M)]).astype(F32)

    hits = np.zeros(M, dtype=rt.HIT_DTYPE)
    hits["kind"], hits["index"], hits["object_index"] = np.arange(M) % 2, np.arange(M), 0
    hits["position"], hits["normal"] = positions, surfaces["normal"]
    hits["uv"], hits["face_direction"], hits["distance"] = rng.uniform(0, 1, (M, 2)).astype(F32), 0, rng.uniform(1, 9, M).astype(F32)
    misses = list(MISSES + MISSES_FROM_CAMERA)
    surfaces[misses] = np.zeros((), dtype=SURFACE_DTYPE)  # material_hits' record of "no hit": 18 zero words
    hits[misses] = np.zeros((), dtype=rt.HIT_DTYPE)
    hits["kind"][misses] = NO_HIT

    incoming = np.zeros(M, dtype=rt.RAY_DTYPE)
    incoming["direction"] = -view
    incoming["origin"] = positions + view * hits["distance"][:, None]
    incoming["face_direction"] = 2

    paths, radiance = P.begin_numpy(M, 1, (np.arange(M, dtype=U32) * U32(2654435761)) ^ U32(0x80000001))
    paths["beta"] = rng.uniform(0.05, 1.6, (M, 3)).astype(F32)
    paths["pdf"] = rng.uniform(0.05, 3.0, M).astype(F32)
    paths["pdf"][list(MISSES_FROM_CAMERA) + [0]] = 0.0
    paths["bounce"] |= (np.arange(M) % 6).astype(U32)
    paths["flags"][list(DEAD)] = 0
    paths["flags"][list(DARKENED)] = P.DARK
    radiance = rng.uniform(0.0, 2.0, (M, 3)).astype(F32)
    emitted = rng.uniform(0.0, 1.0, (M, 3)).astype(F32)
    return surfaces, hits, incoming, view, positions, paths, radiance, emitted


def lights():
    spot, point, directional = Light(), Light(), Light()
    spot.kind, spot.has_origin, spot.origin, spot.direction = 1, 1, (0.25, 4.0, -0.5), (0.0, -1.0, 0.0)
    spot.angle, spot.softness, spot.color = 0.9, 1.0, (1.0, 0.8, 0.6)
    point.kind, point.has_origin, point.origin, point.color = 2, 1, (1.0, 3.0, -1.0), (0.5, 0.9, 0.7)
    d = np.array([0.3, -1.0, 0.2])
    directional.kind, directional.has_origin, directional.direction, directional.color = 0, 0, tuple(d / np.linalg.norm(d)), (0.4, 0.5, 0.9)
    return [spot, point, directional]


def _words(a):
    a = np.ascontiguousarray(a)
    if a.dtype == P.PATH_DTYPE:
        return a.view(U32).reshape(-1, P.PATH_WORDS)
    return a if a.dtype == U8 else a.view(U32)


def steps():
    """name -> the words one call wrote (uint32, or uint8 for the byte arrays), in a fixed order"""
    surfaces, hits, incoming, view, positions, paths, radiance, emitted = batch()
    rng = np.random.default_rng(99)
    out = {}

    def put(name, arrays):
        for k, a in enumerate(arrays if isinstance(arrays, tuple) else (arrays,)):
            out[f"{name}.{k}"] = _words(a)

    put("begin", P.begin_numpy(5, 3, np.array([9, 8, 7, 0xFFFFFFFF, 0], dtype=U32)))
    put("begin.no_ids", P.begin_numpy(M, 1))
    out["light_seed"] = np.array([P.light_seed(s, b) for s in (0, SEED, 0xFFFFFFFF) for b in (0, 1, 5)], dtype=U32)
    resolved = rng.uniform(0, 1, (3 * 5, 3)).astype(F32)
    put("resolve", P.resolve_numpy(resolved, 5, 3))
    put("resolve.root", P.resolve_numpy(resolved, 5, 3, rng.uniform(0, 1, (8, 3)).astype(F32), np.array([7, 0, 3, 2, 5], dtype=U32)))

    texels = rng.uniform(0.0, 2.0, (4, 8, 3)).astype(F32)
    table = environment.table_numpy(texels)
    kind = np.full(M, rt.ESCAPED, dtype=U32)
    kind[[12, 7]] = rt.TRAPPED, rt.INFINITE
    travel = rng.uniform(0.0, 3.0, M).astype(F32)
    escape = rng.integers(0, 1 << 32, (M, 11), dtype=np.uint64).astype(U32)
    pending = rng.uniform(0.1, 1.0, (M, 3)).astype(F32)
    asks = (np.arange(M) % 3 != 0).astype(U8)
    shadow_hits = np.zeros(M, dtype=rt.HIT_DTYPE)
    shadow_hits["kind"] = np.where(np.arange(M) % 4 == 0, np.arange(M) % 2, NO_HIT)
    shadow_hits["position"] = positions + np.array([0.0, 1.0, 0.0], dtype=F32) * rng.uniform(0.5, 4.0, (M, 1)).astype(F32)
    shadow_rays = np.zeros(M, dtype=rt.RAY_DTYPE)
    shadow_rays["origin"], shadow_rays["direction"] = positions, (0.0, 1.0, 0.0)
    reach = rng.uniform(0.5, 4.0, M).astype(F32)
    reach[::5] = -1.0
    poison = dict(dirs=np.full((M, 3), 7, F32), asks=np.full(M, 0x5A, U8), pending=np.full((M, 3), 7, F32))
    three = lights()

    for name, (index, count) in lists().items():
        put(f"advance.{name}", P.advance_numpy(surfaces, view, paths, radiance, emitted, index, count, SEED, None, 3, 0.05, False, poison["dirs"],
                                               poison["asks"]))
        put(f"branch.{name}", P.branch_numpy(surfaces, hits, incoming, paths, index, count, SEED, False))
        put(f"transmit.{name}", P.transmit_numpy(surfaces, paths, kind, travel, escape, index, count, SEED, 3, 0.05))
        put(f"connect.{name}", P.connect_numpy(surfaces, view, texels, table, paths, index, count, SEED, None, P.BALANCE, False, **poison))
        put(f"settle.{name}", P.settle_numpy(asks, pending, radiance, shadow_hits, index, count))
        put(f"weigh_escape.{name}", P.weigh_escape_numpy(texels, table, paths, hits, incoming, emitted, index, count, P.POWER, 0.25))
        put(f"connect_lights.{name}", P.connect_lights_numpy(surfaces, positions, view, three, paths, index, count, SEED,
                                                             np.array([0.0, 0.5, 0.1], dtype=F32), np.array([1.0, 2.0, 5.0], dtype=F32), **poison,
                                                             reach=np.full(M, 7, F32), chosen=np.full(M, 0x5A5A5A5A, U32)))
        put(f"settle_lights.{name}", P.settle_lights_numpy(asks, shadow_rays, reach, pending, radiance, shadow_hits, index, count))
        if name not in WIDE:  # the calls' other arguments: where every slot is touched
            continue
        put(f"advance.{name}.last", P.advance_numpy(surfaces, view, paths, radiance, emitted, index, count, SEED, None, 3, 0.05, True))
        put(f"advance.{name}.geometric", P.advance_numpy(surfaces, view, paths, radiance, None, index, count, SEED + 1, surfaces["normal"], 0, 0.5))
        put(f"branch.{name}.last", P.branch_numpy(surfaces, hits, incoming, paths, index, count, SEED, True))
        put(f"connect.{name}.last", P.connect_numpy(surfaces, view, texels, table, paths, index, count, SEED, None, P.BALANCE, True))
        put(f"connect.{name}.power", P.connect_numpy(surfaces, view, texels, table, paths, index, count, SEED, surfaces["normal"], P.POWER, False, 0.75, 2.0))
        put(f"settle.{name}.open", P.settle_numpy(asks, pending, radiance, None, index, count))
        put(f"connect_lights.{name}.spot", P.connect_lights_numpy(surfaces, positions, view, three, paths, index, count, SEED, light_first=0, light_count=1))
        put(f"settle_lights.{name}.open", P.settle_lights_numpy(asks, shadow_rays, reach, pending, radiance, None, index, count))
    return out


if __name__ == "__main__":
    recorded = steps()
    FIXTURE.parent.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(FIXTURE, **recorded)
    print(f"{FIXTURE}: {len(recorded)} arrays, {FIXTURE.stat().st_size} bytes")
