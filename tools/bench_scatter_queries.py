#!/usr/bin/env python3
"""Timing of the scatter queries (include/rt_amd.h rt_scatter_hits / rt_scatter_factors) on the reference scene's primary hits at
1920 x 1080, one generator per pixel.

    python tools/bench_scatter_queries.py [--steps 7 --warmup 2] [--out profiles/scatter_query_bench.jsonl]

Every GPU step is a child process of its own under its own time limit (--step-timeout seconds); a step that fails or runs out of time
ends the run, and nothing more is started on the device.  The steps:
    kernels   records per second of rt_scatter_hits (fresh generators: no refill in the timed calls) and of rt_scatter_factors
    refill    the A/B of DESIGN.md 3.11: --refill-calls consecutive rt_scatter_hits calls on one rt_rng (every generator runs dry about
              every 85 calls, and after the first block the generators are out of step), timed as a whole, with IsaacCore::generate
              left to the kernel's lane (RT_AMD_SCATTER_PREPARE=0) and with the look-ahead pass ahead of every kernel (=1); the two runs
              are checked against each other: same types and the same generator records
    epoch     one full epoch of distributed_ray_trace at depth 8 written level by level from the queries (the loop of INTEGRATION.md, the
              fold on the device with torch) beside rt_focus_rays + rt_trace_rays_distributed(n_epochs = 1) on the same rays; the two
              are checked against each other bit for bit
No figure is a gate.  Appends one JSON line to --out and prints it.
"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import _bench

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=7, help="timed calls per case")
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--refill-calls", type=int, default=120)
ap.add_argument("--depth", type=int, default=8)
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--step", choices=["kernels", "refill", "epoch"], help="run this step in this process and print its JSON")
ap.add_argument("--step-timeout", type=int, default=240)
ap.add_argument("--out", default=str(ROOT / "profiles" / "scatter_query_bench.jsonl"))
a = ap.parse_args()
STEPS = ("kernels", "refill", "epoch")

if a.step is None:
    _bench.run_cases("bench_scatter_queries", STEPS, lambda step: ["--step", step] + _bench.options(a, "steps", "warmup", "refill_calls", "depth", "width", "height"),
                     a.step_timeout, a.out, header={"steps": a.steps, "warmup": a.warmup, "frame": [a.width, a.height], "depth": a.depth}, merge=True)
    sys.exit(0)

import numpy as np
import torch

import homework_18_graphics_raytracer_amd as rt

torch.cuda.set_device(0)
world = rt.reference_world()
scene = rt.Scene(world)
camera = rt.reference_camera()
frame = rt.Frame.full(a.width, a.height, a.depth)
N = frame.rows * frame.cols


def masked(hits, mask):
    h = hits.clone()
    h[~mask, 0] = rt.HIT_NONE
    return h


def level_loop(rays, rng, depth):
    """distributed_ray_trace on every ray, level by level; finished records stay in place as "no hit" records"""
    n = rays.shape[0]
    cur_rays, cur_hits = rays, rt.cast_rays(scene, rays)
    live = cur_hits[:, 0] >= 0
    levels = []
    for _ in range(depth):
        sc = rt.scatter_hits(scene, cur_hits, cur_rays, rng)
        alive = sc.alive
        dr, fr = alive & (sc.type != rt.REFRACTION), alive & (sc.type == rt.REFRACTION)
        reflected = rt.reflect_rays(masked(cur_hits, dr), sc.rays)
        refr = rt.refract_rays(scene, masked(cur_hits, fr), sc.rays)
        next_rays = torch.where(dr[:, None], reflected, refr.rays)
        to_cast = dr | (fr & refr.escaped)
        rows = to_cast.nonzero().flatten()
        next_hits = torch.zeros((n, 13), dtype=torch.int32, device="cuda")
        next_hits[:, 0] = rt.HIT_NONE
        next_hits[rows] = rt.cast_rays(scene, next_rays[rows].contiguous())
        found = to_cast & (next_hits[:, 0] >= 0)
        next_hits = masked(next_hits, found)
        factor = rt.scatter_factors(scene, cur_hits, cur_rays, sc.type, next_rays, refr.travel)
        shade_next = rt.shade_hits(scene, next_hits, next_rays)
        missed = dr & ~found
        shade_missed = rt.shade_hits(scene, masked(cur_hits, missed), sc.rays)
        levels.append((sc.type, found, missed, factor, shade_next, shade_missed))
        cur_rays, cur_hits, live = next_rays, next_hits, found
    value = rt.shade_hits(scene, cur_hits, cur_rays)
    for t, found, missed, factor, shade_next, shade_missed in reversed(levels):
        s = value * factor
        mixed = shade_next + (s - shade_next) * 0.5
        summed = (value + shade_next) * factor[:, 0:1]
        new = torch.where((found & (t != rt.REFRACTION))[:, None], mixed, torch.zeros_like(value))
        new = torch.where((found & (t == rt.REFRACTION))[:, None], summed, new)
        value = torch.where(missed[:, None], shade_missed, new)
    return value


out = {}
rays = rt.camera_rays(camera, frame)
hits = rt.cast_rays(scene, rays)
if a.step == "kernels":
    rng = rt.Rng(frame)
    ms = []
    for k in range(a.warmup + a.steps):  # 3 words a call: far from the end of the first block
        t = _bench.time_ms(lambda: rt.scatter_hits(scene, hits, rays, rng))
        if k >= a.warmup:
            ms.append(t)
    out["scatter_hits"] = dict(_bench.summary(ms, rate=("mrecords_per_s", N)), hits=int((hits[:, 0] >= 0).sum().item()))
    sc = rt.scatter_hits(scene, hits, rays, rng)
    nxt = rt.reflect_rays(hits, sc.rays)
    travel = torch.full((N,), 0.5, dtype=torch.float32, device="cuda")
    rgb = torch.empty((N, 3), dtype=torch.float32, device="cuda")
    fn = lambda: rt.scatter_factors(scene, hits, rays, sc.type, nxt, travel, out=rgb)
    for _ in range(a.warmup):
        fn()
    out["scatter_factors"] = _bench.summary([_bench.time_ms(fn) for _ in range(a.steps)], rate=("mrecords_per_s", N))
elif a.step == "refill":
    kept = {}
    for name, value in (("in_kernel", 0), ("prepare_pass", 1)):
        with rt.options(RT_AMD_SCATTER_PREPARE=value):
            rng = rt.Rng(frame)
            rt.scatter_hits(scene, hits, rays, rng)
            torch.cuda.synchronize()
            last = []

            def calls():
                for _ in range(a.refill_calls):
                    last[:] = [rt.scatter_hits(scene, hits, rays, rng)]

            ms = _bench.time_ms(calls)
            out["refill_" + name] = {"calls": a.refill_calls, "ms_total": round(ms, 3), "ms_per_call": round(ms / a.refill_calls, 4),
                                     "mrecords_per_s": round(N * a.refill_calls / ms / 1e3, 1)}
            kept[name] = (last[0].type.clone(), last[0].rays.clone(), torch.from_numpy(rng.download()[:4096].astype(np.int64)))
            rng.close()
    out["refill_forms_identical"] = all(bool((x == y).all()) for x, y in zip(kept["in_kernel"], kept["prepare_pass"]))
    out["refill_winner"] = "in_kernel" if out["refill_in_kernel"]["ms_total"] <= out["refill_prepare_pass"]["ms_total"] else "prepare_pass"
else:
    rng_a, rng_b = rt.Rng(frame), rt.Rng(frame)
    samples = torch.empty((1, N, 3), dtype=torch.float32, device="cuda")
    got = [None]

    def by_levels():
        got[0] = level_loop(rt.focus_rays(camera, frame, rng_a), rng_a, a.depth)

    def by_call():
        rt.trace_rays_distributed(scene, rt.focus_rays(camera, frame, rng_b), a.depth, rng_b, 1, samples=samples)

    ms = {"levels": [], "call": []}
    identical = True
    for k in range(a.warmup + a.steps):
        t_l, t_c = _bench.time_ms(by_levels), _bench.time_ms(by_call)
        identical = identical and _bench.same(got[0], samples[0])
        if k >= a.warmup:
            ms["levels"].append(t_l)
            ms["call"].append(t_c)
    out["epoch_by_levels"] = _bench.summary(ms["levels"], rate=("mrecords_per_s", N))
    out["epoch_by_call"] = _bench.summary(ms["call"], rate=("mrecords_per_s", N))
    out["epoch_levels_over_call"] = round(out["epoch_by_levels"]["ms_median"] / out["epoch_by_call"]["ms_median"], 3)
    out["epoch_identical"] = identical
    out["device"] = torch.cuda.get_device_name(0)
print(json.dumps(out))
