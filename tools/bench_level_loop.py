#!/usr/bin/env python3
"""Timing of one epoch of distributed_ray_trace written level by level with the device-side level loop (include/rt_amd.h
rt_select_records / rt_cast_rays_indexed / rt_level_*; Python rt.trace_rays_distributed_levels), beside its two yardsticks: the fused
rt_trace_rays_distributed call, and the same loop glued with torch (masks, nonzero(), a gathered cast, the fold in torch) as
tests/test_gpu_scatter_queries.py and tools/bench_scatter_queries.py write it.

    python tools/bench_level_loop.py [--steps 5 --warmup 2] [--out profiles/level_loop_bench.jsonl]

Every GPU step is a child process of its own under its own time limit (--step-timeout seconds); a step that fails or runs out of time
ends the run, and nothing more is started on the device.  The steps, on the reference scene at depth 8:
    primary   the 1920 x 1080 primary rays
    random    2 M random rays through the scene's bounding sphere
Each reports milliseconds per epoch of the three forms (checked against each other bit for bit) and, per level, the share of the
records that the indexed cast actually casts.  No figure is a gate.  Appends one JSON line to --out and prints it.
"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import _bench

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=5, help="timed epochs per form")
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--depth", type=int, default=8)
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--random-rays", type=int, default=2_000_000)
ap.add_argument("--step", choices=["primary", "random"], help="run this step in this process and print its JSON")
ap.add_argument("--step-timeout", type=int, default=300)
ap.add_argument("--out", default=str(ROOT / "profiles" / "level_loop_bench.jsonl"))
a = ap.parse_args()
STEPS = ("primary", "random")

if a.step is None:
    _bench.run_cases("bench_level_loop", STEPS, lambda step: ["--step", step] + _bench.options(a, "steps", "warmup", "depth", "width", "height", "random_rays"),
                     a.step_timeout, a.out, header={"steps": a.steps, "warmup": a.warmup, "frame": [a.width, a.height], "depth": a.depth})
    sys.exit(0)

import numpy as np
import torch

import homework_18_graphics_raytracer_amd as rt

torch.cuda.set_device(0)
world = rt.reference_world()
scene = rt.Scene(world)
camera = rt.reference_camera()


def masked(hits, mask):
    h = hits.clone()
    h[~mask, 0] = rt.HIT_NONE
    return h


def torch_glued(rays, rng, depth, shares=None):
    """the loop as the scatter-query test writes it: masks and where() in torch, nonzero() for the rays that exist (the host waits for
    the count at every level), a gathered cast scattered back, the fold in torch"""
    n = rays.shape[0]
    cur_rays, cur_hits = rays, rt.cast_rays(scene, rays)
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
        if shares is not None:
            shares.append(round(rows.numel() / n, 4))
        next_hits = torch.zeros((n, 13), dtype=torch.int32, device="cuda")
        next_hits[:, 0] = rt.HIT_NONE
        if rows.numel():
            next_hits[rows] = rt.cast_rays(scene, next_rays[rows].contiguous())
        found = to_cast & (next_hits[:, 0] >= 0)
        next_hits = masked(next_hits, found)
        factor = rt.scatter_factors(scene, cur_hits, cur_rays, sc.type, next_rays, refr.travel)
        shade_next = rt.shade_hits(scene, next_hits, next_rays)
        missed = dr & ~found
        shade_missed = rt.shade_hits(scene, masked(cur_hits, missed), sc.rays)
        levels.append((sc.type, found, missed, factor, shade_next, shade_missed))
        cur_rays, cur_hits = next_rays, next_hits
    value = rt.shade_hits(scene, cur_hits, cur_rays)
    for t, found, missed, factor, shade_next, shade_missed in reversed(levels):
        s = value * factor
        mixed = shade_next + (s - shade_next) * 0.5
        summed = (value + shade_next) * factor[:, 0:1]
        new = torch.where((found & (t != rt.REFRACTION))[:, None], mixed, torch.zeros_like(value))
        new = torch.where((found & (t == rt.REFRACTION))[:, None], summed, new)
        value = torch.where(missed[:, None], shade_missed, new)
    return value


if a.step == "primary":
    rays = rt.camera_rays(camera, rt.Frame.full(a.width, a.height, a.depth))
else:
    g = np.random.default_rng(7)
    desc = world.desc()
    pts = np.array([list(desc.triangles[i].vertices[k].position) for i in range(desc.n_triangles) for k in range(3)], dtype=np.float64)
    centre = (pts.min(axis=0) + pts.max(axis=0)) / 2
    radius = float(np.linalg.norm(pts - centre, axis=1).max())
    o = g.normal(size=(a.random_rays, 3))
    o = centre + radius * 1.5 * o / np.linalg.norm(o, axis=1, keepdims=True)
    target = centre + radius * g.uniform(-0.6, 0.6, size=(a.random_rays, 3))
    d = target - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = rt.make_rays(torch.tensor(o.astype(np.float32), device="cuda"), torch.tensor(d.astype(np.float32), device="cuda"), face=rt.BOTH)
N = rays.shape[0]
seeds = np.arange(N, dtype=np.uint64)
rngs = {k: rt.Rng.seeded(seeds) for k in ("levels", "call", "torch")}
samples = {k: torch.empty((1, N, 3), dtype=torch.float32, device="cuda") for k in ("levels", "call")}
got = [None]
shares = []


def by_levels():
    rt.trace_rays_distributed_levels(scene, rays, a.depth, rngs["levels"], 1, samples=samples["levels"])


def by_call():
    rt.trace_rays_distributed(scene, rays, a.depth, rngs["call"], 1, samples=samples["call"])


def by_torch():
    got[0] = torch_glued(rays, rngs["torch"], a.depth, shares if not shares else None)


ms = {"levels": [], "call": [], "torch": []}
identical = True
for k in range(a.warmup + a.steps):
    t = {"levels": _bench.time_ms(by_levels), "call": _bench.time_ms(by_call), "torch": _bench.time_ms(by_torch)}
    identical = identical and _bench.same(samples["levels"][0], samples["call"][0]) and _bench.same(got[0], samples["call"][0])
    if k >= a.warmup:
        for name in ms:
            ms[name].append(t[name])
out = {"rays": N, "epoch_device_loop": _bench.summary(ms["levels"], rate=("mrecords_per_s", N)), "epoch_fused_call": _bench.summary(ms["call"], rate=("mrecords_per_s", N)), "epoch_torch_glued": _bench.summary(ms["torch"], rate=("mrecords_per_s", N))}
out["device_loop_over_fused_call"] = round(out["epoch_device_loop"]["ms_median"] / out["epoch_fused_call"]["ms_median"], 3)
out["device_loop_over_torch_glued"] = round(out["epoch_device_loop"]["ms_median"] / out["epoch_torch_glued"]["ms_median"], 3)
out["cast_share_per_level"] = shares  # of the first epoch: records the indexed cast casts / records, level 1 .. depth
out["identical"] = identical
out["device"] = torch.cuda.get_device_name(0)
print(json.dumps(out))
