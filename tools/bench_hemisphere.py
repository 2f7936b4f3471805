#!/usr/bin/env python3
"""Timing of the hemisphere queries (include/rt_amd.h rt_hemisphere_rays / rt_hemisphere_fold; Python rt.hemisphere) and the two loops
built from them, on the primary hits of the reference scene.

    python tools/bench_hemisphere.py [--steps 7 --warmup 2] [--out profiles/hemisphere_bench.jsonl]

Every case is a child process of its own under its own `timeout -k 10 <--step-timeout>`; a case that fails or runs out of time ends the
run, and nothing more is started on the device.  The cases are sample counts: spp1, spp4, spp16.  Each takes the primary hits of the
reference scene at 1920 x 1080, a stratified pattern, the shading normal, ids = the pixel index, and reports milliseconds (medians, device
events, the forms alternated call by call) of
    rays               rt_hemisphere_rays alone
    fold_ambient       rt_hemisphere_fold with the shadow hits of the sequence: open flags' share only
    fold_bounce        rt_hemisphere_fold with a radiance array: the weighted mean added to rgb
    ambient            hemisphere.ambient_hits, the whole sequence (rays -> select_records -> cast_rays_indexed -> fold)
    indirect           hemisphere.indirect_hits, the whole sequence (rays -> trace_rays at --depth -> fold)
and the casts of each loop.  The loops cost what their casts cost; no figure is a gate.  Appends one JSON line with the commit to --out and
prints it.
"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import _bench

STEPS = ("spp1", "spp4", "spp16")
ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=7, help="timed calls per form")
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--depth", type=int, default=2, help="max_depth of the bounce's trace_rays")
ap.add_argument("--cases", nargs="+", choices=STEPS, default=list(STEPS))
ap.add_argument("--step", choices=STEPS, help="run this case in this process and print its JSON")
ap.add_argument("--step-timeout", type=int, default=300)
ap.add_argument("--out", default=str(ROOT / "profiles" / "hemisphere_bench.jsonl"))
a = ap.parse_args()

if a.step is None:
    _bench.run_cases("bench_hemisphere", a.cases, lambda case: ["--step", case] + _bench.options(a, "steps", "warmup", "width", "height", "depth"),
                     a.step_timeout, a.out, header={"steps": a.steps, "warmup": a.warmup, "depth": a.depth})
    sys.exit(0)

import torch

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import hemisphere

torch.cuda.set_device(0)
spp = int(a.step[3:])
scene = rt.Scene(rt.reference_world())
rays = rt.camera_rays(rt.reference_camera(), rt.Frame.full(a.width, a.height, 0))
hits = rt.cast_rays(scene, rays)
N = rays.shape[0]
m = spp * N
ids = torch.arange(N, dtype=torch.int32, device="cuda")
ambient = torch.empty((N,), dtype=torch.float32, device="cuda")
rgb = torch.zeros((N, 3), dtype=torch.float32, device="cuda")
count = {k: torch.zeros(1, dtype=torch.int64, device="cuda") for k in ("ambient", "indirect")}
stream = torch.cuda.Stream()
with torch.cuda.stream(stream):
    w = hemisphere.workspace(N, "cuda", spp)


    def ambient_loop():
        hemisphere.ambient_hits(scene, hits, spp, float("inf"), hemisphere.STRATIFIED, 1, ids, out=ambient, ray_count=count["ambient"], stream=stream, workspace=w)


    def indirect_loop():
        hemisphere.indirect_hits(scene, hits, spp, a.depth, 1.0, rgb, hemisphere.STRATIFIED, 1, ids, ray_count=count["indirect"], stream=stream, workspace=w)


    indirect_loop()  # leaves the radiance in the workspace ...
    ambient_loop()   # ... and the shadow hits (and is the first, untimed call of the selection on this stream)
    stream.synchronize()
    casts = {k: int(v.item()) for k, v in count.items()}
    asked = int(w.asks[:m].sum().item())
    calls = {
        "rays": lambda: hemisphere.rays(scene, hits, spp, hemisphere.STRATIFIED, 1, ids, hemisphere.SHADING, w.rays[:m], w.asks[:m], w.dirs[:m], stream=stream),
        "fold_ambient": lambda: hemisphere.fold(scene, hits, w.asks[:m], spp, w.shadow_hits[:m], float("inf"), ambient=ambient, stream=stream),
        "fold_bounce": lambda: hemisphere.fold(scene, hits, w.asks[:m], spp, radiance=w.radiance[:m], out=rgb, stream=stream),
        "ambient": ambient_loop,
        "indirect": indirect_loop,
    }
    ms = _bench.alternate(calls, a.warmup, a.steps)
res = {"records": N, "hits": int(rt.Hits(hits).hit.sum().item()), "spp": spp, "depth": a.depth, "asked": asked, "casts_ambient": casts["ambient"],
       "casts_indirect": casts["indirect"], "mean_ambient": round(float(ambient.mean().item()), 4)}
for name, v in ms.items():
    res[name] = _bench.summary(v)
res["device"] = torch.cuda.get_device_name(0)
print(json.dumps(res))
