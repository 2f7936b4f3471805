#!/usr/bin/env python3
"""Timing of the radiance-query path (include/rt_amd.h rt_trace_rays): ray_trace on caller-supplied rays.

    timeout -k 10 900 python tools/bench_trace_rays.py [--steps 7 --warmup 2] [--no-large]

On the reference scene at 1920 x 1080, depth 8 (bench.py's headline frame), four calls alternated call by call in this process and
timed with device events after the warm-up:
    (a) whitted   rt_render_whitted of the frame
    (b) rows      rt_trace_rays of the frame's camera rays (rt_camera_rays) in their row order: a wave's 64 rays are a 64x1 strip
    (c) tiles     the same rays permuted into the Whitted kernels' slot order (8-row bands, column-major inside a band: 8x8 tiles);
                  the permutation is made once, before the timed calls
    (d) random    2 M seeded random rays from origins within twice the scene's bounding radius, aimed at it
and a 1 M-ray batch of such random rays at depth 8 on the 147 484-triangle scene of bench.py's large_scene (tools/make_tessellated_obj.py
--levels 6, flat), which the kernels walk breadth-first.  (b) and (c) are checked against (a): the same image after + 0.0, bit for bit,
and the same cast count.  Prints one JSON line.  Kernel times: run it under rocprofv3 --kernel-trace --stats.
"""
import argparse
import json
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np
import torch

import homework_18_graphics_raytracer_amd as rt

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=7, help="timed calls per case")
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--large-steps", type=int, default=2, help="timed calls on the large scene")
ap.add_argument("--random-rays", type=int, default=2_000_000)
ap.add_argument("--large-rays", type=int, default=1_000_000)
ap.add_argument("--depth", type=int, default=8)
ap.add_argument("--no-large", action="store_true")
ap.add_argument("--seed", type=int, default=2024)
a = ap.parse_args()

torch.cuda.set_device(0)


def random_rays(seed, n, centre, radius):
    g = np.random.default_rng(seed)
    scale = np.where(g.random(n) < 0.5, g.uniform(0.0, 1.0, n), g.uniform(1.0, 2.0, n)) * radius
    u = g.normal(size=(n, 3))
    origins = centre + u / np.linalg.norm(u, axis=1, keepdims=True) * scale[:, None]
    d = centre + g.normal(0.0, radius * 0.5, (n, 3)) - origins
    d /= np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-12)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
    return rt.make_rays(dev(origins), dev(d))


def bounds(desc):
    p = [v.position[:] for i in range(desc.n_triangles) for v in desc.triangles[i].vertices]
    for i in range(desc.n_spheres):
        s = desc.spheres[i]
        p += [list(np.asarray(s.center[:]) + s.radius), list(np.asarray(s.center[:]) - s.radius)]
    p = np.asarray(p, dtype=np.float64)
    c = (p.min(0) + p.max(0)) / 2
    return c, float(np.linalg.norm(p - c, axis=1).max())


def tile_order(cols, rows):
    """position k of the Whitted kernels' slot order -> the row-order index of its pixel"""
    s = np.arange(cols * rows, dtype=np.int64)
    band = s // (cols * 8)
    r = s - band * cols * 8
    band_rows = np.minimum(8, rows - band * 8)
    col = r // band_rows
    return (band * 8 + (r - col * band_rows)) * cols + col


def one(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def alternated(cases, steps, warmup):
    """every case once per round, `steps` timed rounds after `warmup` untimed ones; returns per case the ms of every timed call"""
    for _ in range(warmup):
        for fn in cases.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in cases}
    for _ in range(steps):
        for k, fn in cases.items():
            ms[k].append(one(fn))
    return ms


def casts_of(fn, count):
    count.zero_()
    fn()
    torch.cuda.synchronize()
    return int(count.item())


def summary(n, v, casts):
    med = float(np.median(v))
    return {"rays": n, "ms_median": round(med, 4), "ms_min": round(min(v), 4), "calls": len(v), "casts": casts,
            "mrays_per_s": round(n / med / 1e3, 1), "gcasts_per_s": round(casts / med / 1e6, 3)}


result = {"tool": "bench_trace_rays", "device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup, "depth": a.depth}
world = rt.reference_world()
desc = world.desc()
scene = rt.Scene(world)
cam = rt.reference_camera()
W, H = 1920, 1080
frame = rt.Frame.full(W, H, a.depth)
rows = rt.camera_rays(cam, frame)
perm = torch.from_numpy(tile_order(W, H)).cuda()
tiles = rows[perm].contiguous()
centre, radius = bounds(desc)
rnd = random_rays(a.seed, a.random_rays, centre, radius)
img = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
out = {k: torch.empty((n, 3), dtype=torch.float32, device="cuda") for k, n in (("b_rows", W * H), ("c_tiles", W * H), ("d_random", rnd.shape[0]))}
count = torch.zeros(1, dtype=torch.int64, device="cuda")
cases = {
    "a_whitted": lambda: rt.render_whitted(scene, cam, frame, out=img),
    "b_rows": lambda: rt.trace_rays(scene, rows, a.depth, out=out["b_rows"]),
    "c_tiles": lambda: rt.trace_rays(scene, tiles, a.depth, out=out["c_tiles"]),
    "d_random": lambda: rt.trace_rays(scene, rnd, a.depth, out=out["d_random"]),
}
ms = alternated(cases, a.steps, a.warmup)
casts = {
    "a_whitted": casts_of(lambda: rt.render_whitted(scene, cam, frame, out=img, ray_count=count), count),
    "b_rows": casts_of(lambda: rt.trace_rays(scene, rows, a.depth, out=out["b_rows"], ray_count=count), count),
    "c_tiles": casts_of(lambda: rt.trace_rays(scene, tiles, a.depth, out=out["c_tiles"], ray_count=count), count),
    "d_random": casts_of(lambda: rt.trace_rays(scene, rnd, a.depth, out=out["d_random"], ray_count=count), count),
}
for k in cases:
    result[k] = summary(W * H if k != "d_random" else rnd.shape[0], ms[k], casts[k])
want = img.reshape(-1, 3).view(torch.int32)
unperm = torch.empty_like(out["c_tiles"])
unperm[perm] = out["c_tiles"]
result["b_rows"]["equals_whitted"] = bool(torch.equal((out["b_rows"] + 0.0).view(torch.int32), want)) and casts["b_rows"] == casts["a_whitted"]
result["c_tiles"]["equals_whitted"] = bool(torch.equal((unperm + 0.0).view(torch.int32), want)) and casts["c_tiles"] == casts["a_whitted"]
result["c_over_a"] = round(result["c_tiles"]["ms_median"] / result["a_whitted"]["ms_median"], 4)
result["b_over_a"] = round(result["b_rows"]["ms_median"] / result["a_whitted"]["ms_median"], 4)
result["ray_bytes_read"] = W * H * 44
del rows, tiles, rnd, out

if not a.no_large:
    with tempfile.TemporaryDirectory() as tmp:
        obj = Path(tmp) / "d6.obj"
        subprocess.run([sys.executable, str(ROOT / "tools" / "make_tessellated_obj.py"), rt.DEFAULT_OBJ, str(obj), "--levels", "6"], check=True,
                       capture_output=True)
        big = rt.reference_world(str(obj))
    bdesc = big.desc()
    bscene = rt.Scene(big)
    bcentre, bradius = bounds(bdesc)
    brays = random_rays(a.seed + 1, a.large_rays, bcentre, bradius)
    bout = torch.empty((brays.shape[0], 3), dtype=torch.float32, device="cuda")
    bms = alternated({"large": lambda: rt.trace_rays(bscene, brays, a.depth, out=bout)}, a.large_steps, 1)["large"]
    result["large"] = summary(brays.shape[0], bms, casts_of(lambda: rt.trace_rays(bscene, brays, a.depth, out=bout, ray_count=count), count))
    result["large"]["triangles"] = int(bdesc.n_triangles)
print(json.dumps(result))
