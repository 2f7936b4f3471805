#!/usr/bin/env python3
"""Timing of the ray-query path (include/rt_amd.h rt_cast_rays): World::cast on caller-supplied rays.

    timeout -k 10 900 python tools/bench_ray_query.py [--steps 5 --warmup 1] [--no-large]

Five batches, each cast by the default kernel and with RT_AMD_QUERY_WAVE_UNIFORM=1 (every wave through cast_asm), the two
alternated call by call in this process, timed with device events after the warm-up:
    primary   the 1920 x 1080 primary rays of the reference camera (rt_camera_rays) on the reference scene
    random    2 M seeded random rays from origins in and around the reference scene (within twice its bounding radius), aimed
              at it, the three face modes, 60 % with a random triangle or sphere exclusion (some out of range)
    large     1 M such rays on the 147 484-triangle tessellated scene (tools/make_tessellated_obj.py --levels 6 --spherize), which
              the default kernel walks breadth-first (rt::cast_rays_bfs_kernel)
    random_far, large_far   the same with origins out to 4x the bounding radius: a ray that starts more than 4x the scene's extent
              from the origin may not use the exact rejections of the node walk (rt_device_scene.h filter_origin2), which is the case
              these measure
and, for scale, the Whitted frame of bench.py's headline (1920 x 1080, depth 8), timed the same way.  Both kernels' hits are compared
word for word on every batch (`agree`).  Prints one JSON line.  Kernel times: run it under rocprofv3 --kernel-trace --stats.
"""
import argparse
import json
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import _bench
import numpy as np
import torch

import homework_18_graphics_raytracer_amd as rt

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=5, help="timed calls per kernel and batch")
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--large-steps", type=int, default=2, help="timed calls per kernel on the large scene")
ap.add_argument("--random-rays", type=int, default=2_000_000)
ap.add_argument("--large-rays", type=int, default=1_000_000)
ap.add_argument("--no-large", action="store_true")
ap.add_argument("--seed", type=int, default=2024)
ap.add_argument("--lib", default=None, help="variant tag: use variants/librt_amd_<tag>.so instead of the in-tree library")
a = ap.parse_args()

if a.lib:
    import ctypes as C
    from homework_18_graphics_raytracer_amd import _capi
    _capi._amd = None
    _orig = _capi._load
    _capi._load = lambda name: C.CDLL(str(_capi.PKG_DIR / "variants" / f"librt_amd_{a.lib}.so")) if name == "librt_amd.so" else _orig(name)

torch.cuda.set_device(0)


def random_rays(seed, n, centre, radius, n_triangles, n_spheres, spread):
    g = np.random.default_rng(seed)
    origins, d = _bench.ray_arrays(g, n, centre, radius, spread)
    kind = g.choice([-1, rt.SPHERE, rt.TRIANGLE], n, p=[0.4, 0.2, 0.4])
    index = np.where(kind == rt.TRIANGLE, g.integers(0, n_triangles + 2, n), g.integers(0, n_spheres + 2, n))
    dev = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).cuda()
    return rt.make_rays(dev(origins, np.float32), dev(d, np.float32), dev(g.integers(0, 3, n), np.int64), dev(kind, np.int64),
                        dev(index, np.int64), dev(g.integers(0, 3, n), np.int64))


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def ab(scene, rays, steps, warmup):
    """the two kernels alternated: one call of each per round; returns per kernel the ms of every timed call, and whether the hits agree"""
    outs = {k: torch.empty((rays.shape[0], 13), dtype=torch.int32, device="cuda") for k in ("default", "wave_uniform")}

    def call(kind):
        with rt.options(RT_AMD_QUERY_WAVE_UNIFORM=1 if kind == "wave_uniform" else None):
            rt.cast_rays(scene, rays, out=outs[kind])

    ms = {k: [] for k in outs}
    for k in outs:
        for _ in range(warmup):
            call(k)
    for _ in range(steps):
        for k in outs:
            ms[k] += timed(lambda: call(k), 1, 0)
    torch.cuda.synchronize()
    agree = bool(torch.equal(outs["default"], outs["wave_uniform"]))
    hit = float((outs["default"][:, 0] != rt.HIT_NONE).float().mean().item())
    return ms, agree, hit


def summary(name, n, ms, agree, hit):
    out = {"rays": n, "hit_fraction": round(hit, 4), "agree": agree}
    for k, v in ms.items():
        best, med = min(v), float(np.median(v))
        out[k] = {"ms_median": round(med, 4), "ms_min": round(best, 4), "grays_per_s": round(n / med / 1e6, 3), "calls": len(v)}
    out["wave_uniform_over_default"] = round(out["wave_uniform"]["ms_median"] / out["default"]["ms_median"], 3)
    return out


result = {"tool": "bench_ray_query", "lib": a.lib or "in-tree", "device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup}
world = rt.reference_world()
desc = world.desc()
scene = rt.Scene(world)
cam = rt.reference_camera()
frame = rt.Frame.full(1920, 1080, 8)

# for scale: the Whitted frame (8.6x as many casts as its primary rays)
img = torch.empty((1080, 1920, 3), dtype=torch.float32, device="cuda")
w_ms = timed(lambda: rt.render_whitted(scene, cam, frame, out=img), a.steps, a.warmup)
result["whitted_1080p_d8_ms_median"] = round(float(np.median(w_ms)), 4)

primary = rt.camera_rays(cam, frame)
c_ms = timed(lambda: rt.camera_rays(cam, frame, out=primary), a.steps, a.warmup)
result["camera_rays_1080p_ms_median"] = round(float(np.median(c_ms)), 4)
result["primary"] = summary("primary", primary.shape[0], *ab(scene, primary, a.steps, a.warmup))
del primary

centre, radius = _bench.bounds(desc)
for key, spread in (("random", 2.0), ("random_far", 4.0)):
    rays = random_rays(a.seed, a.random_rays, centre, radius, desc.n_triangles, desc.n_spheres, spread)
    result[key] = summary(key, rays.shape[0], *ab(scene, rays, a.steps, a.warmup))
    del rays

if not a.no_large:
    with tempfile.TemporaryDirectory() as tmp:
        big = _bench.tessellated_world(tmp, 6, True)
    bdesc = big.desc()
    bscene = rt.Scene(big)
    bcentre, bradius = _bench.bounds(bdesc)
    for key, spread in (("large", 2.0), ("large_far", 4.0)):
        rays = random_rays(a.seed + 1, a.large_rays, bcentre, bradius, bdesc.n_triangles, bdesc.n_spheres, spread)
        result[key] = summary(key, rays.shape[0], *ab(bscene, rays, a.large_steps, 1))
        result[key]["triangles"] = int(bdesc.n_triangles)
        result[key]["breadth_first"] = True  # 147 484 >= the default switch of 8 192 (RT_AMD_BFS_WALK_TRIANGLES)
        del rays
print(json.dumps(result))
