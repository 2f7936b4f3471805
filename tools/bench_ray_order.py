#!/usr/bin/env python3
"""What ordering a batch on the device is worth (include/rt_amd.h "record ordering"): rt_ray_keys + rt_sort_records in front of
rt_trace_rays and rt_cast_rays, against the plain calls on the same rays in the same run.

    timeout -k 10 1200 python tools/bench_ray_order.py [--steps 7 --warmup 2] [--no-large] [--out profiles/order_bench.jsonl]

Ray sets (those of tools/bench_trace_rays.py): the 1920 x 1080 camera rays of the reference scene in row order
(case b), the same rays in a random permutation, 2 M seeded random rays (case d), and 1 M random rays on the 147 484-triangle scene,
all at depth 8.  Per ray set, alternated call by call and timed with device events after the warm-up, medians of --steps calls:
    trace           rt.trace_rays                      (the baseline: the parent's kernels, untouched)
    trace_ordered   rt.trace_rays_ordered              keys, sort, gather, rt_trace_rays, scatter — buffers made once
    cast            rt.cast_rays
    cast_ordered    rt.cast_rays_ordered               keys, sort, rt_cast_rays_indexed
    order_steps     keys + sort + gather of the rays + scatter of the values, nothing traced
The ordered results are checked against the plain ones bit for bit, cast counts included.  There is no gate: a ray set where ordering
loses is printed like the others.  Prints one JSON line per ray set and appends them to --out when given."""
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
ap.add_argument("--random-rays", type=int, default=2_000_000)
ap.add_argument("--large-rays", type=int, default=1_000_000)
ap.add_argument("--depth", type=int, default=8)
ap.add_argument("--no-large", action="store_true")
ap.add_argument("--seed", type=int, default=2024)
ap.add_argument("--out", default=None, help="a .jsonl file the result lines are appended to")
a = ap.parse_args()

torch.cuda.set_device(0)


def alternated(cases, steps, warmup):
    ms = _bench.alternate(cases, warmup, steps)
    return {k: round(float(np.median(v)), 4) for k, v in ms.items()}


def measure(name, world, scene, rays, steps):
    n = rays.shape[0]
    box = world.bounds()
    w = rt.order_workspace(n, rays.device, trace=True)
    rgb, rgb_o = (torch.empty((n, 3), dtype=torch.float32, device="cuda") for _ in range(2))
    hits, hits_o = (torch.empty((n, 13), dtype=torch.int32, device="cuda") for _ in range(2))
    cnt, cnt_o = (torch.zeros(1, dtype=torch.int64, device="cuda") for _ in range(2))

    def order_steps():
        rt.ray_keys(rays, box[0], box[1], out=w.keys)
        rt.sort_records(w.keys, 0, 30, out=w.index, temp=w.temp)
        rt.gather_records(rays, w.index, out=w.rays)
        rt.scatter_records(w.rgb, w.index, rgb_o)

    cases = {
        "trace": lambda: rt.trace_rays(scene, rays, a.depth, out=rgb),
        "trace_ordered": lambda: rt.trace_rays_ordered(scene, rays, a.depth, box=box, out=rgb_o, workspace=w),
        "cast": lambda: rt.cast_rays(scene, rays, out=hits),
        "cast_ordered": lambda: rt.cast_rays_ordered(scene, rays, box=box, out=hits_o, workspace=w),
        "order_steps": order_steps,
    }
    ms = alternated(cases, steps, a.warmup)
    rt.trace_rays(scene, rays, a.depth, out=rgb, ray_count=cnt)
    rt.trace_rays_ordered(scene, rays, a.depth, box=box, out=rgb_o, ray_count=cnt_o, workspace=w)
    rt.cast_rays(scene, rays, out=hits)
    rt.cast_rays_ordered(scene, rays, box=box, out=hits_o, workspace=w)
    torch.cuda.synchronize()
    casts = int(cnt.item())
    line = {"tool": "bench_ray_order", "device": torch.cuda.get_device_name(0), "rays_set": name, "rays": n, "depth": a.depth, "steps": steps,
            "ms_median": ms, "trace_casts": casts,
            "trace_gcasts_per_s": round(casts / ms["trace"] / 1e6, 3), "trace_ordered_gcasts_per_s": round(casts / ms["trace_ordered"] / 1e6, 3),
            "trace_ordered_over_trace": round(ms["trace_ordered"] / ms["trace"], 4), "cast_ordered_over_cast": round(ms["cast_ordered"] / ms["cast"], 4),
            "distinct_keys": int(torch.unique(w.keys).numel()),
            "trace_equal": bool(torch.equal(rgb.view(torch.int32), rgb_o.view(torch.int32))) and casts == int(cnt_o.item()),
            "cast_equal": bool(torch.equal(hits, hits_o))}
    print(json.dumps(line), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(json.dumps(line) + "\n")
    return line


world = rt.reference_world()
scene = rt.Scene(world)
W, H = 1920, 1080
rows = rt.camera_rays(rt.reference_camera(), rt.Frame.full(W, H, a.depth))
measure("b_rows", world, scene, rows, a.steps)
perm = torch.from_numpy(np.random.default_rng(a.seed).permutation(W * H)).cuda()
measure("b_rows_permuted", world, scene, rows[perm].contiguous(), a.steps)
del rows
centre, radius = _bench.bounds(world.desc())
measure("d_random", world, scene, _bench.random_rays(a.seed, a.random_rays, centre, radius), a.steps)

if not a.no_large:
    with tempfile.TemporaryDirectory() as tmp:
        big = _bench.tessellated_world(tmp, 6, False)
    bscene = rt.Scene(big)
    bcentre, bradius = _bench.bounds(big.desc())
    measure("large_random", big, bscene, _bench.random_rays(a.seed + 1, a.large_rays, bcentre, bradius), a.steps)
