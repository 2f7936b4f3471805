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
perm = torch.from_numpy(_bench.tile_order(W, H)).cuda()
tiles = rows[perm].contiguous()
centre, radius = _bench.bounds(desc)
rnd = _bench.random_rays(a.seed, a.random_rays, centre, radius)
img = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
out = {k: torch.empty((n, 3), dtype=torch.float32, device="cuda") for k, n in (("b_rows", W * H), ("c_tiles", W * H), ("d_random", rnd.shape[0]))}
count = torch.zeros(1, dtype=torch.int64, device="cuda")
cases = {
    "a_whitted": lambda: rt.render_whitted(scene, cam, frame, out=img),
    "b_rows": lambda: rt.trace_rays(scene, rows, a.depth, out=out["b_rows"]),
    "c_tiles": lambda: rt.trace_rays(scene, tiles, a.depth, out=out["c_tiles"]),
    "d_random": lambda: rt.trace_rays(scene, rnd, a.depth, out=out["d_random"]),
}
ms = _bench.alternate(cases, a.warmup, a.steps)
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
        big = _bench.tessellated_world(tmp, 6, False)
    bdesc = big.desc()
    bscene = rt.Scene(big)
    bcentre, bradius = _bench.bounds(bdesc)
    brays = _bench.random_rays(a.seed + 1, a.large_rays, bcentre, bradius)
    bout = torch.empty((brays.shape[0], 3), dtype=torch.float32, device="cuda")
    bms = _bench.alternate({"large": lambda: rt.trace_rays(bscene, brays, a.depth, out=bout)}, 1, a.large_steps)["large"]
    result["large"] = summary(brays.shape[0], bms, casts_of(lambda: rt.trace_rays(bscene, brays, a.depth, out=bout, ray_count=count), count))
    result["large"]["triangles"] = int(bdesc.n_triangles)
print(json.dumps(result))
