#!/usr/bin/env python3
"""Timing of the stochastic radiance-query path (include/rt_amd.h rt_trace_rays_distributed, rt_focus_rays): distributed_ray_trace on
caller-supplied rays.

    timeout -k 10 900 python tools/bench_trace_rays_distributed.py [--steps 5 --warmup 2] [--out profiles/trace_rays_distributed_bench.jsonl]

On the reference scene at 1920 x 1080, depth 8, 8 epochs per timed unit (bench.py's stochastic_pass job), alternated unit by unit in
this process and timed with device events after the warm-up; medians:
    (a) frame     rt_render_distributed, 8 epochs in one call
    (b) rows      8 x (rt_focus_rays + rt_trace_rays_distributed(n_epochs = 1)) on the same pixels, rays in row order
    (c) tiles     the same with each epoch's rays gathered into the chain kernel's chunk order (8-row bands, column-major inside a
                  band: 8x8 tiles); the gather (one index_select of 44-byte records) is inside the timed unit, and generator k then
                  serves the k-th ray of that order — the same distribution as (a), not the same samples
    (e) fixed     rays of one rt_focus_rays in tile order, rt_trace_rays_distributed(n_epochs = 8) in ONE call: the kernels alone
                  against (a) — one launch set, no lens kernel, the 44-byte ray read per sample
    (d) random    2 M seeded random rays from origins within twice the scene's bounding radius, aimed at it, n_epochs = 8 in one call
(b) is checked against (a): the same samples and flags bit for bit, the same cast count, from generators seeded alike.
Prints one JSON line and, with --out, appends it to that file.  Kernel times: run it under rocprofv3 --kernel-trace --stats.
"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import _bench
import numpy as np
import torch

import homework_18_graphics_raytracer_amd as rt

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=5, help="timed units per case")
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--epochs", type=int, default=8)
ap.add_argument("--random-rays", type=int, default=2_000_000)
ap.add_argument("--depth", type=int, default=8)
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--seed", type=int, default=2024)
ap.add_argument("--out", type=str, default=None)
a = ap.parse_args()

torch.cuda.set_device(0)


W, H, E, D = a.width, a.height, a.epochs, a.depth
N = W * H
world = rt.reference_world()
desc = world.desc()
scene = rt.Scene(world)
cam = rt.reference_camera()
frame = rt.Frame.full(W, H, D)
perm = torch.from_numpy(_bench.tile_order(W, H)).cuda()
centre, radius = _bench.bounds(desc)
rnd = _bench.random_rays(a.seed, a.random_rays, centre, radius)
result = {"tool": "bench_trace_rays_distributed", "device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup,
          "depth": D, "epochs": E, "width": W, "height": H}

# ---- (b) against (a), once, before the timed part: samples, flags, casts ----
count = torch.zeros(1, dtype=torch.int64, device="cuda")
rng_a, rng_b = rt.Rng(frame), rt.Rng(frame)
s_a = torch.empty((1, H, W, 3), dtype=torch.float32, device="cuda")
v_a = torch.empty((1, H, W), dtype=torch.uint8, device="cuda")
s_b = torch.empty((1, N, 3), dtype=torch.float32, device="cuda")
v_b = torch.empty((1, N), dtype=torch.uint8, device="cuda")
rays = torch.empty((N, 11), dtype=torch.int32, device="cuda")
rt.render_distributed(scene, cam, frame, rng_a, 1, samples=s_a, valid=v_a, ray_count=count)
torch.cuda.synchronize()
casts_a = int(count.item())
count.zero_()
rt.focus_rays(cam, frame, rng_b, out=rays)
rt.trace_rays_distributed(scene, rays, D, rng_b, 1, samples=s_b, valid=v_b, ray_count=count)
torch.cuda.synchronize()
result["b_equals_a"] = bool(torch.equal(s_a.view(torch.int32).reshape(-1), s_b.view(torch.int32).reshape(-1)) and torch.equal(v_a.reshape(-1), v_b.reshape(-1))
                            and casts_a == int(count.item()))
result["casts_per_epoch"] = casts_a
del s_a, v_a, s_b, v_b

# ---- the timed units ----
rng_c, rng_e = rt.Rng(frame), rt.Rng(frame)
rng_d = rt.Rng.seeded(np.arange(rnd.shape[0], dtype=np.uint64) + np.uint64(a.seed))
acc = {k: torch.zeros((n, 3), dtype=torch.float32, device="cuda") for k, n in (("a", N), ("b", N), ("c", N), ("e", N), ("d", rnd.shape[0]))}
tiles = torch.empty_like(rays)
fixed = rt.focus_rays(cam, frame, rng_e)[perm].contiguous()


def unit_b():
    for _ in range(E):
        rt.focus_rays(cam, frame, rng_b, out=rays)
        rt.trace_rays_distributed(scene, rays, D, rng_b, 1, accum=acc["b"])


def unit_c():
    for _ in range(E):
        rt.focus_rays(cam, frame, rng_c, out=rays)
        torch.index_select(rays, 0, perm, out=tiles)
        rt.trace_rays_distributed(scene, tiles, D, rng_c, 1, accum=acc["c"])


cases = {
    "a_frame": lambda: rt.render_distributed(scene, cam, frame, rng_a, E, accum=acc["a"].view(H, W, 3)),
    "b_rows": unit_b,
    "c_tiles": unit_c,
    "e_fixed": lambda: rt.trace_rays_distributed(scene, fixed, D, rng_e, E, accum=acc["e"]),
    "d_random": lambda: rt.trace_rays_distributed(scene, rnd, D, rng_d, E, accum=acc["d"]),
}
ms = _bench.alternate(cases, a.warmup, a.steps)
for k, v in ms.items():
    n = rnd.shape[0] if k == "d_random" else N
    med = float(np.median(v))
    result[k] = {"rays": n, "ms_median": round(med, 4), "ms_min": round(min(v), 4), "ms_per_epoch": round(med / E, 4), "units": len(v),
                 "msamples_per_s": round(n * E / med / 1e3, 1)}
for k in ("b_rows", "c_tiles", "e_fixed"):
    result[k[0] + "_over_a"] = round(result[k]["ms_median"] / result["a_frame"]["ms_median"], 4)
result["ray_bytes_read_per_epoch"] = N * 44
line = json.dumps(result)
print(line)
if a.out:
    with open(a.out, "a") as f:
        f.write(line + "\n")
