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
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

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
    result = {"tool": "bench_scatter_queries", "steps": a.steps, "warmup": a.warmup, "frame": [a.width, a.height], "depth": a.depth}
    try:
        result["commit"] = subprocess.run(["git", "-C", str(ROOT), "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    except OSError:
        result["commit"] = None
    for step in STEPS:
        cmd = [sys.executable, __file__, "--step", step] + [x for k in ("steps", "warmup", "refill_calls", "depth", "width", "height")
                                                            for x in ("--" + k.replace("_", "-"), str(getattr(a, k)))]
        try:
            proc = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout)
        except subprocess.TimeoutExpired:
            sys.exit(f"step {step}: no result within {a.step_timeout} s; nothing more is started")
        if proc.returncode != 0:
            sys.stderr.write(proc.stdout + proc.stderr)
            sys.exit(f"step {step}: exit status {proc.returncode}; nothing more is started")
        result.update(json.loads(proc.stdout.strip().splitlines()[-1]))
    line = json.dumps(result)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")
    print(line)
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


def one(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def stats(ms, records):
    med = float(np.median(ms))
    return {"ms_median": round(med, 4), "ms_min": round(min(ms), 4), "mrecords_per_s": round(records / med / 1e3, 1)}


def same(x, y):
    return bool(((x.view(torch.int32) == y.view(torch.int32)) | (x.isnan() & y.isnan())).all())


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
        t = one(lambda: rt.scatter_hits(scene, hits, rays, rng))
        if k >= a.warmup:
            ms.append(t)
    out["scatter_hits"] = dict(stats(ms, N), hits=int((hits[:, 0] >= 0).sum().item()))
    sc = rt.scatter_hits(scene, hits, rays, rng)
    nxt = rt.reflect_rays(hits, sc.rays)
    travel = torch.full((N,), 0.5, dtype=torch.float32, device="cuda")
    rgb = torch.empty((N, 3), dtype=torch.float32, device="cuda")
    fn = lambda: rt.scatter_factors(scene, hits, rays, sc.type, nxt, travel, out=rgb)
    for _ in range(a.warmup):
        fn()
    out["scatter_factors"] = stats([one(fn) for _ in range(a.steps)], N)
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

            ms = one(calls)
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
        t_l, t_c = one(by_levels), one(by_call)
        identical = identical and same(got[0], samples[0])
        if k >= a.warmup:
            ms["levels"].append(t_l)
            ms["call"].append(t_c)
    out["epoch_by_levels"] = stats(ms["levels"], N)
    out["epoch_by_call"] = stats(ms["call"], N)
    out["epoch_levels_over_call"] = round(out["epoch_by_levels"]["ms_median"] / out["epoch_by_call"]["ms_median"], 3)
    out["epoch_identical"] = identical
    out["device"] = torch.cuda.get_device_name(0)
print(json.dumps(out))
