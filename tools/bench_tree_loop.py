#!/usr/bin/env python3
"""Timing of ray_trace written level by level with the device-side tree loop (include/rt_amd.h rt_tree_gate / rt_tree_split /
rt_tree_spawn / rt_tree_gather / rt_tree_fold; Python rt.trace_rays_levels), beside the fused rt_trace_rays call of the same build,
and the size of every level of the recursion tree — the measurement the default level capacity comes from.

    python tools/bench_tree_loop.py [--steps 5 --warmup 2] [--out profiles/tree_loop_bench.jsonl]

Every case is a child process of its own under its own time limit (--step-timeout seconds); a case that fails or runs out of time
ends the run, and nothing more is started on the device.  The cases, on the reference scene at depth 8:
    tiles     the 1920 x 1080 camera rays in the Whitted kernels' 8x8-tile order
    random    2 M random rays through the scene's bounding sphere
Each reports milliseconds of three forms — the loop as enqueued calls, the same loop replayed from a captured graph, the fused call —
checked against each other bit for bit (values and cast count), the ratio of the loop to the fused call, and the live records of
every level divided by the number of rays (level 0: the roots that passed the entry check).  The levels are measured with room for 4n
records each and the overflow word checked; the timed loop runs with the default capacity.  No figure is a gate: the loop launches
about a dozen kernels per level and moves every record through memory; what it offers is the absence of host visits.  Appends one
JSON line to --out and prints it.
"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import _bench

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=5, help="timed calls per form")
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--depth", type=int, default=8)
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--random-rays", type=int, default=2_000_000)
ap.add_argument("--step", choices=["tiles", "random"], help="run this case in this process and print its JSON")
ap.add_argument("--step-timeout", type=int, default=300)
ap.add_argument("--out", default=str(ROOT / "profiles" / "tree_loop_bench.jsonl"))
a = ap.parse_args()
STEPS = ("tiles", "random")

if a.step is None:
    _bench.run_cases("bench_tree_loop", STEPS, lambda step: ["--step", step] + _bench.options(a, "steps", "warmup", "depth", "width", "height", "random_rays"),
                     a.step_timeout, a.out, header={"steps": a.steps, "warmup": a.warmup, "frame": [a.width, a.height], "depth": a.depth})
    sys.exit(0)

import numpy as np
import torch

import homework_18_graphics_raytracer_amd as rt

torch.cuda.set_device(0)
world = rt.reference_world()
scene = rt.Scene(world)
camera = rt.reference_camera()


if a.step == "tiles":
    rows = rt.camera_rays(camera, rt.Frame.full(a.width, a.height, a.depth))
    rays = rows[torch.from_numpy(_bench.tile_order(a.width, a.height)).cuda()].contiguous()
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
out = {k: torch.empty((N, 3), dtype=torch.float32, device="cuda") for k in ("loop", "graph", "fused")}
count = {k: torch.zeros(1, dtype=torch.int64, device="cuda") for k in out}
overflow = torch.zeros(1, dtype=torch.int32, device="cuda")
stream = torch.cuda.Stream()

# the size of every level, with room to spare and the overflow word read back
level_counts = torch.zeros(a.depth + 1, dtype=torch.int32, device="cuda")
rt.trace_rays_levels(scene, rays, a.depth, level_capacity=lambda level: min(N << level, 4 * N), level_counts=level_counts, check=True)
shares = [round(c / N, 4) for c in level_counts.cpu().tolist()]


def by_loop():
    rt.trace_rays_levels(scene, rays, a.depth, out=out["loop"], ray_count=count["loop"], stream=stream, check=False, overflow=overflow)


def by_fused():
    rt.trace_rays(scene, rays, a.depth, out=out["fused"], ray_count=count["fused"], stream=stream)


with torch.cuda.stream(stream):
    by_loop()  # uncaptured first: the selection's scratch of this stream
    by_fused()
    stream.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        rt.trace_rays_levels(scene, rays, a.depth, out=out["graph"], ray_count=count["graph"], stream=stream, check=False, overflow=overflow)
    forms = {"loop": by_loop, "graph": graph.replay, "fused": by_fused}
    ms = {k: [] for k in forms}
    identical = True
    for k in range(a.warmup + a.steps):
        for c in count.values():
            c.zero_()
        t = {name: _bench.time_ms(fn) for name, fn in forms.items()}
        identical = identical and _bench.same(out["loop"], out["fused"]) and _bench.same(out["graph"], out["fused"])
        identical = identical and count["loop"].item() == count["fused"].item() == count["graph"].item()
        if k >= a.warmup:
            for name in ms:
                ms[name].append(t[name])
res = {"rays": N, "loop": _bench.summary(ms["loop"], rate=("mrays_per_s", N)), "loop_in_a_graph": _bench.summary(ms["graph"], rate=("mrays_per_s", N)), "fused_call": _bench.summary(ms["fused"], rate=("mrays_per_s", N))}
res["loop_over_fused_call"] = round(res["loop"]["ms_median"] / res["fused_call"]["ms_median"], 3)
res["graph_over_fused_call"] = round(res["loop_in_a_graph"]["ms_median"] / res["fused_call"]["ms_median"], 3)
res["casts"] = int(count["fused"].item())
res["live_records_per_level_over_n"] = shares  # level 0 .. depth
res["level_capacity_factor"] = rt.LEVEL_CAPACITY_FACTOR
res["overflow"] = int(overflow.item())
res["identical"] = identical and res["overflow"] == 0
res["device"] = torch.cuda.get_device_name(0)
print(json.dumps(res))
