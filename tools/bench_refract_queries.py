#!/usr/bin/env python3
"""Timing of get_refract written bounce by bounce (include/rt_amd.h rt_refract_enter / rt_refract_step with rt_select_records and
rt_cast_rays_indexed between them; Python rt.refract_rays_by_bounce) beside the fused rt_refract_rays of the same build, and of
rt.trace_rays_levels with and without open_casts.

    python tools/bench_refract_queries.py [--steps 7 --warmup 2] [--out profiles/refract_query_bench.jsonl]

Every case is a child process of its own under its own `timeout -k 10 <--step-timeout>`; a case that fails or runs out of time ends the
run, and nothing more is started on the device.  The scenes:
    reference    the reference scene: the 1920 x 1080 camera rays in the Whitted kernels' 8x8-tile order
    spherized4   the scene around the spherized dodecahedron of 9 244 triangles, walked breadth-first: 480 x 270 camera rays
    spherized6   the same at 147 484 triangles
and per scene two cases.  `refract_<scene>`: the glass hits of the frame (the hits whose material is transparent: what ray_trace hands
to get_refract) — milliseconds (medians, device events, the forms alternated call by call) of
    refract_pairs / refract_uniform   rt_refract_rays with its pair-wise casts (the default) and under RT_AMD_QUERY_WAVE_UNIFORM=1
    loop / loop_in_a_graph            rt.refract_rays_by_bounce as enqueued calls, and replayed from a captured graph
all four checked against each other bit for bit (kind, travel, escape ray and cast count) before anything is timed, and the ratios of
the loop to the faster fused form.  `levels_<scene>`: rt.trace_rays_levels at depth 5 with open_casts False and True, checked against
each other bit for bit (values and cast count) first.  No figure is a gate.  Appends one JSON line with the commit to --out and prints it.
"""
import argparse
import json
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import _bench

SCENES = ("reference", "spherized4", "spherized6")
STEPS = tuple(f"{kind}_{scene}" for kind in ("refract", "levels") for scene in SCENES)
ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=7, help="timed calls per form")
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--depth", type=int, default=5, help="max_depth of the trace_rays_levels cases")
ap.add_argument("--cases", nargs="+", choices=STEPS, default=list(STEPS))
ap.add_argument("--step", choices=STEPS, help="run this case in this process and print its JSON")
ap.add_argument("--step-timeout", type=int, default=300)
ap.add_argument("--out", default=str(ROOT / "profiles" / "refract_query_bench.jsonl"))
a = ap.parse_args()

if a.step is None:
    _bench.run_cases("bench_refract_queries", a.cases, lambda case: ["--step", case] + _bench.options(a, "steps", "warmup", "depth"), a.step_timeout, a.out,
                     header={"steps": a.steps, "warmup": a.warmup, "depth": a.depth})
    sys.exit(0)

import torch

import homework_18_graphics_raytracer_amd as rt

torch.cuda.set_device(0)


kind, scene_name = a.step.split("_")
with tempfile.TemporaryDirectory() as tmp:
    if scene_name.startswith("spherized"):
        level = int(scene_name[-1])
        world = _bench.tessellated_world(tmp, level, True)
        with rt.options(RT_AMD_BFS_WALK_TRIANGLES=8192):  # the library's default switch, set here so that no environment moves it
            scene = rt.Scene(world)
        rays = rt.camera_rays(rt.reference_camera(), rt.Frame.full(480, 270, 0))
    else:
        world = rt.reference_world()
        scene = rt.Scene(world)
        rows = rt.camera_rays(rt.reference_camera(), rt.Frame.full(1920, 1080, 0))
        rays = rows[torch.from_numpy(_bench.tile_order(1920, 1080)).cuda()].contiguous()
desc = world.desc()
stream = torch.cuda.Stream()
res = {"triangles": desc.n_triangles}

if kind == "refract":
    all_hits = rt.cast_rays(scene, rays)
    transparent = torch.tensor([desc.materials[o].transparency > 0.001 for o in range(desc.n_materials)], device="cuda")
    is_hit = rt.Hits(all_hits).hit
    glass = (is_hit & transparent[all_hits[:, 2].long().clamp(0, desc.n_materials - 1)]).nonzero().flatten()
    hits, rays = all_hits[glass].contiguous(), rays[glass].contiguous()
    N = hits.shape[0]
    forms = ("refract_pairs", "refract_uniform", "loop", "loop_in_a_graph")
    new = lambda: rt.Refractions(torch.empty((N,), dtype=torch.int32, device="cuda"), torch.empty((N,), dtype=torch.float32, device="cuda"),
                                 torch.empty((N, 11), dtype=torch.int32, device="cuda"))
    out = {k: new() for k in forms}
    count = {k: torch.zeros(1, dtype=torch.int64, device="cuda") for k in forms}
    space = {k: rt.refract_workspace(N, "cuda") for k in forms[2:]}

    def fused(key):
        rt.refract_rays(scene, hits, rays, 100.0, ray_count=count[key], stream=stream, out=out[key])

    def fused_uniform():
        with rt.options(RT_AMD_QUERY_WAVE_UNIFORM=1):
            fused("refract_uniform")

    def by_loop(key="loop"):
        rt.refract_rays_by_bounce(scene, hits, rays, 100.0, ray_count=count[key], stream=stream, out=out[key], workspace=space[key])

    def identical():
        ref = out[forms[0]]
        ok = all(_bench.same(out[k].kind, ref.kind) and _bench.same(out[k].travel, ref.travel) and _bench.same(out[k].rays, ref.rays) for k in forms[1:])
        return ok and len({int(c.item()) for c in count.values()}) == 1

    calls = {"refract_pairs": lambda: fused("refract_pairs"), "refract_uniform": fused_uniform, "loop": by_loop}
    res.update(records=N, frame_rays=int(all_hits.shape[0]))
else:
    N = rays.shape[0]
    forms = ("levels", "levels_open_casts")
    out = {k: torch.empty((N, 3), dtype=torch.float32, device="cuda") for k in forms}
    count = {k: torch.zeros(1, dtype=torch.int64, device="cuda") for k in forms}
    overflow = torch.zeros(1, dtype=torch.int32, device="cuda")

    def levels(key, opened):
        rt.trace_rays_levels(scene, rays, a.depth, 1.0, out=out[key], ray_count=count[key], stream=stream, check=False, overflow=overflow,
                             level_capacity=lambda level: 2 * N, open_casts=opened)

    def identical():
        return _bench.same(out["levels"], out["levels_open_casts"]) and int(count["levels"].item()) == int(count["levels_open_casts"].item()) \
            and int(overflow.item()) == 0

    calls = {"levels": lambda: levels("levels", False), "levels_open_casts": lambda: levels("levels_open_casts", True)}
    res.update(records=N, depth=a.depth)

with torch.cuda.stream(stream):
    # uncaptured first: the selection's scratch of this stream and, on a scene walked breadth-first, the walk's record lists
    for fn in calls.values():
        fn()
    stream.synchronize()
    if kind == "refract":
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            by_loop("loop_in_a_graph")
        calls["loop_in_a_graph"] = graph.replay
        for c in count.values():
            c.zero_()
        for fn in calls.values():
            fn()
        stream.synchronize()
    else:
        count["levels"].zero_()
        count["levels_open_casts"].zero_()
        for fn in calls.values():
            fn()
        stream.synchronize()
    ok = identical()  # before anything is timed
    if not ok:
        sys.exit(f"case {a.step}: the forms differ; nothing is timed")
    ms = {k: [] for k in calls}
    for k in range(a.warmup + a.steps):
        for c in count.values():
            c.zero_()
        t = {name: _bench.time_ms(fn) for name, fn in calls.items()}
        ok = ok and identical()
        if k >= a.warmup:
            for name in ms:
                ms[name].append(t[name])
res["casts"] = int(count[forms[0]].item())
for name, v in ms.items():
    res[name] = _bench.summary(v, rate=("mcasts_per_s", res["casts"]))
if kind == "refract":
    best = min(res["refract_pairs"]["ms_median"], res["refract_uniform"]["ms_median"])
    res["fused_winner"] = "pairs" if res["refract_pairs"]["ms_median"] <= res["refract_uniform"]["ms_median"] else "uniform"
    res["loop_over_fused"] = round(res["loop"]["ms_median"] / best, 3)
    res["graph_over_fused"] = round(res["loop_in_a_graph"]["ms_median"] / best, 3)
    res["casts_per_record_max"] = int(space["loop"].casts.max().item())
else:
    res["open_over_fused"] = round(res["levels_open_casts"]["ms_median"] / res["levels"]["ms_median"], 3)
res["identical"] = ok
res["device"] = torch.cuda.get_device_name(0)
print(json.dumps(res))
