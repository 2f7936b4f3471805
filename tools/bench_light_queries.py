#!/usr/bin/env python3
"""Timing of get_shade written light by light (include/rt_amd.h rt_light_rays / rt_light_terms / rt_light_fold with rt_select_records
and rt_cast_rays_indexed between them; Python rt.shade_hits_by_light) beside the fused rt_shade_hits of the same build.

    python tools/bench_light_queries.py [--steps 7 --warmup 2] [--out profiles/light_query_bench.jsonl]

Every case is a child process of its own under its own `timeout -k 10 <--step-timeout>`; a case that fails or runs out of time ends the
run, and nothing more is started on the device.  The cases:
    tiles        the reference scene: the hits of the 1920 x 1080 camera rays in the Whitted kernels' 8x8-tile order
    random       the reference scene: the hits of 2 M random rays through the scene's bounding sphere
    spherized4   the scene around the spherized dodecahedron of 9 244 triangles, walked breadth-first: 480 x 270 camera hits
    spherized6   the same at 147 484 triangles
Each reports milliseconds (medians, device events, the forms alternated call by call) of
    shade_pairs / shade_uniform   rt_shade_hits with its pair-wise shadow casts (the default) and under RT_AMD_QUERY_WAVE_UNIFORM=1
    loop / loop_in_a_graph        rt.shade_hits_by_light as enqueued calls, and replayed from a captured graph
all four checked against each other bit for bit (values and cast count), and the ratios of the loop to the faster fused form.  No
figure is a gate.  Appends one JSON line with the commit to --out and prints it.
"""
import argparse
import json
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import _bench

STEPS = ("tiles", "random", "spherized4", "spherized6")
ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=7, help="timed calls per form")
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--random-rays", type=int, default=2_000_000)
ap.add_argument("--cases", nargs="+", choices=STEPS, default=list(STEPS))
ap.add_argument("--step", choices=STEPS, help="run this case in this process and print its JSON")
ap.add_argument("--step-timeout", type=int, default=300)
ap.add_argument("--out", default=str(ROOT / "profiles" / "light_query_bench.jsonl"))
a = ap.parse_args()

if a.step is None:
    _bench.run_cases("bench_light_queries", a.cases, lambda case: ["--step", case] + _bench.options(a, "steps", "warmup", "random_rays"), a.step_timeout, a.out,
                     header={"steps": a.steps, "warmup": a.warmup})
    sys.exit(0)

import numpy as np
import torch

import homework_18_graphics_raytracer_amd as rt

torch.cuda.set_device(0)


with tempfile.TemporaryDirectory() as tmp:
    if a.step.startswith("spherized"):
        level = int(a.step[-1])
        world = _bench.tessellated_world(tmp, level, True)
        with rt.options(RT_AMD_BFS_WALK_TRIANGLES=8192):  # the library's default switch, set here so that no environment moves it
            scene = rt.Scene(world)
        rays = rt.camera_rays(rt.reference_camera(), rt.Frame.full(480, 270, 0))
    else:
        world = rt.reference_world()
        scene = rt.Scene(world)
        if a.step == "tiles":
            rows = rt.camera_rays(rt.reference_camera(), rt.Frame.full(1920, 1080, 0))
            rays = rows[torch.from_numpy(_bench.tile_order(1920, 1080)).cuda()].contiguous()
        else:
            g = np.random.default_rng(7)
            desc = world.desc()
            pts = np.array([list(desc.triangles[i].vertices[k].position) for i in range(desc.n_triangles) for k in range(3)], dtype=np.float64)
            centre = (pts.min(axis=0) + pts.max(axis=0)) / 2
            radius = float(np.linalg.norm(pts - centre, axis=1).max())
            o = g.normal(size=(a.random_rays, 3))
            o = centre + radius * 1.5 * o / np.linalg.norm(o, axis=1, keepdims=True)
            d = centre + radius * g.uniform(-0.6, 0.6, size=(a.random_rays, 3)) - o
            d /= np.linalg.norm(d, axis=1, keepdims=True)
            rays = rt.make_rays(torch.tensor(o.astype(np.float32), device="cuda"), torch.tensor(d.astype(np.float32), device="cuda"), face=rt.BOTH)
triangles = world.desc().n_triangles
hits = rt.cast_rays(scene, rays)
N = rays.shape[0]
forms = ("shade_pairs", "shade_uniform", "loop", "loop_in_a_graph")
out = {k: torch.empty((N, 3), dtype=torch.float32, device="cuda") for k in forms}
count = {k: torch.zeros(1, dtype=torch.int64, device="cuda") for k in forms}
stream = torch.cuda.Stream()


def fused(key):
    rt.shade_hits(scene, hits, rays, out=out[key], ray_count=count[key], stream=stream)


def fused_uniform():
    with rt.options(RT_AMD_QUERY_WAVE_UNIFORM=1):
        fused("shade_uniform")


def by_loop(key="loop"):
    rt.shade_hits_by_light(scene, hits, rays, out=out[key], ray_count=count[key], stream=stream)


with torch.cuda.stream(stream):
    by_loop()  # uncaptured first: the selection's scratch of this stream and, on a scene walked breadth-first, the walk's record lists
    stream.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        by_loop("loop_in_a_graph")
    calls = {"shade_pairs": lambda: fused("shade_pairs"), "shade_uniform": fused_uniform, "loop": by_loop, "loop_in_a_graph": graph.replay}
    ms = {k: [] for k in calls}
    identical = True
    for k in range(a.warmup + a.steps):
        for c in count.values():
            c.zero_()
        t = {name: _bench.time_ms(fn) for name, fn in calls.items()}
        identical = identical and all(_bench.same(out[name], out["shade_pairs"]) for name in forms[1:])
        identical = identical and len({int(c.item()) for c in count.values()}) == 1
        if k >= a.warmup:
            for name in ms:
                ms[name].append(t[name])
res = {"triangles": triangles, "records": N, "hits": int(rt.Hits(hits).hit.sum().item()), "lights": scene.n_lights,
       "shadow_casts": int(count["shade_pairs"].item())}
for name, v in ms.items():
    res[name] = _bench.summary(v, rate=("mcasts_per_s", res["shadow_casts"]))
best = min(res["shade_pairs"]["ms_median"], res["shade_uniform"]["ms_median"])
res["fused_winner"] = "pairs" if res["shade_pairs"]["ms_median"] <= res["shade_uniform"]["ms_median"] else "uniform"
res["loop_over_fused"] = round(res["loop"]["ms_median"] / best, 3)
res["graph_over_fused"] = round(res["loop_in_a_graph"]["ms_median"] / best, 3)
res["identical"] = identical
res["device"] = torch.cuda.get_device_name(0)
print(json.dumps(res))
