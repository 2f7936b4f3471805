#!/usr/bin/env python3
"""Timing of the area-light queries (include/rt_amd.h rt_area_light_rays / rt_area_light_terms / rt_area_light_fold; Python
rt.arealights) beside rt.shade_hits_by_light — the point-light sequence they extend — on the same hits of the same build.

    python tools/bench_area_lights.py [--steps 7 --warmup 2] [--out profiles/area_light_bench.jsonl]

Every case is a child process of its own under its own `timeout -k 10 <--step-timeout>`; a case that fails or runs out of time ends the
run, and nothing more is started on the device.  The cases are sample counts: spp1, spp4, spp16.  Each takes the primary hits of the
reference scene at 1920 x 1080, lights_per_pass = 1 (it bounds the memory: 138 B per (sample, light, hit) entry), radius 0.3 for every
light, a stratified pattern, and reports milliseconds (medians, device events, the forms alternated call by call) of
    by_light           rt.shade_hits_by_light: the yardstick, hard shadows
    soft               arealights.shade_hits_soft, the whole sequence
    rays / terms / fold   the three new calls alone, on one light's buffers of the sequence
and, at radius 0 with one sample, that the sequence gives by_light's bits and cast count.  No figure is a gate.  Appends one JSON line with
the commit to --out and prints it.
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
ap.add_argument("--cases", nargs="+", choices=STEPS, default=list(STEPS))
ap.add_argument("--step", choices=STEPS, help="run this case in this process and print its JSON")
ap.add_argument("--step-timeout", type=int, default=300)
ap.add_argument("--out", default=str(ROOT / "profiles" / "area_light_bench.jsonl"))
a = ap.parse_args()

if a.step is None:
    _bench.run_cases("bench_area_lights", a.cases, lambda case: ["--step", case] + _bench.options(a, "steps", "warmup", "width", "height"), a.step_timeout,
                     a.out, header={"steps": a.steps, "warmup": a.warmup})
    sys.exit(0)

import torch

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import arealights

torch.cuda.set_device(0)
spp = int(a.step[3:])
scene = rt.Scene(rt.reference_world())
rays = rt.camera_rays(rt.reference_camera(), rt.Frame.full(a.width, a.height, 0))
hits = rt.cast_rays(scene, rays)
N, L = rays.shape[0], scene.n_lights
ids = torch.arange(N, dtype=torch.int32, device="cuda")
radii = torch.full((L,), 0.3, dtype=torch.float32, device="cuda")
zero = torch.zeros((L,), dtype=torch.float32, device="cuda")
out = {k: torch.empty((N, 3), dtype=torch.float32, device="cuda") for k in ("by_light", "soft", "hard")}
count = {k: torch.zeros(1, dtype=torch.int64, device="cuda") for k in out}
stream = torch.cuda.Stream()
with torch.cuda.stream(stream):
    point_ws = rt.light_workspace(scene, N, "cuda", lights_per_pass=1)
    w = arealights.workspace(scene, N, "cuda", spp, lights_per_pass=1)
    m = spp * N


    def by_light():
        rt.shade_hits_by_light(scene, hits, rays, out=out["by_light"], ray_count=count["by_light"], stream=stream, lights_per_pass=1, workspace=point_ws)


    def soft(key="soft", r=radii, samples=spp):
        arealights.shade_hits_soft(scene, hits, rays, r, samples, arealights.STRATIFIED, 1, ids, out=out[key], ray_count=count[key], stream=stream,
                                   lights_per_pass=1, workspace=w)


    soft("hard", zero, 1)  # radius 0, one sample: the point-light sequence's bits (and the first, untimed call of the selection on this stream)
    by_light()
    stream.synchronize()
    casts = int(count["by_light"].item())
    identical = _bench.same(out["hard"], out["by_light"]) and int(count["hard"].item()) == casts
    soft()  # leaves the last light's buffers in the workspace: what the three calls alone are timed on
    last = L - 1
    calls = {
        "by_light": by_light,
        "soft": soft,
        "rays": lambda: arealights.rays(scene, hits, rays, radii[last:], spp, arealights.STRATIFIED, 1, ids, last, 1, w.shadow_rays[:m], w.asks[:m],
                                        w.sample[:m], stream=stream),
        "terms": lambda: arealights.terms(scene, hits, rays, w.asks[:m], w.sample[:m], w.shadow_hits[:m], spp, last, 1, w.lit[:m], w.diffuse[:m],
                                          w.specular[:m], stream=stream),
        "fold": lambda: arealights.fold(scene, hits, w.lit[:m], w.diffuse[:m], w.specular[:m], out["soft"], spp, stream=stream),
    }
    ms = _bench.alternate(calls, a.warmup, a.steps)
res = {"records": N, "hits": int(rt.Hits(hits).hit.sum().item()), "lights": L, "spp": spp, "shadow_casts_by_light": casts}
for name, v in ms.items():
    res[name] = _bench.summary(v)
res["soft_over_by_light"] = round(res["soft"]["ms_median"] / res["by_light"]["ms_median"], 3)
res["radius_0_identical"] = identical
res["device"] = torch.cuda.get_device_name(0)
print(json.dumps(res))
