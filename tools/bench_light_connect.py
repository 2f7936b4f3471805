#!/usr/bin/env python3
"""Timing of the light-connection queries (include/rt_amd.h rt_path_connect_lights / rt_path_settle_lights; Python rt.paths) on the
primary hits of the reference scene.

    python tools/bench_light_connect.py [--steps 9 --warmup 3] [--out profiles/light_connect_bench.jsonl]

Every case runs in a child process of its own under its own `timeout -k 10 <--step-timeout>`; if one fails or runs out of time the run
ends, and nothing more is started on the device.  On the 1920 x 1080 primary rays and hits, ids = the pixel index:
    lights3           the reference scene with its own three lights
    lights8           the same scene and the same paths with its lights repeated to eight
each of them:
    connect_lights    rt_path_connect_lights, bounce 0, every path alive, one path per pixel, radii given          (Mpaths/s)
    settle_lights     rt_path_settle_lights on its asks, nothing occluding
    trace_paths       paths.trace_paths, --spp samples, --bounces bounces, roulette from bounce 3: with shade_hits (open_casts off and
                      on) and with light_nee (radius 0, uniform choice); light_nee_over_plain is the ratio of the medians against the
                      faster of the two shade forms — the claim DESIGN.md 3.38 records, at three lights and at eight
    flagship          `bench.py --gpus 1 --steps 20 --warmup 5` in the same visit, its JSON line as it is
Milliseconds are medians of device events, the forms alternated call by call; settle clears its asks, so they are put back (untimed)
before every call.  No figure is a gate.  Appends one JSON line with the commit to --out and prints it.
"""
import argparse
import json
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import _bench

STEPS = ("lights3", "lights8", "flagship")
ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=9, help="timed calls per form")
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--spp", type=int, default=4)
ap.add_argument("--bounces", type=int, default=4)
ap.add_argument("--cases", nargs="+", choices=STEPS, default=list(STEPS))
ap.add_argument("--step", choices=STEPS, help="run this case in this process and print its JSON")
ap.add_argument("--step-timeout", type=int, default=300)
ap.add_argument("--out", default=str(ROOT / "profiles" / "light_connect_bench.jsonl"))
a = ap.parse_args()

if a.step is None:
    _bench.run_cases("bench_light_connect", a.cases, lambda case: ["--step", case] + _bench.options(a, "steps", "warmup", "width", "height", "spp", "bounces"),
                     a.step_timeout, a.out, header={"steps": a.steps, "warmup": a.warmup, "spp": a.spp, "bounces": a.bounces})
    sys.exit(0)

if a.step == "flagship":  # a process of its own, started from one that has not touched the device
    proc = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"], capture_output=True, text=True)
    if proc.returncode != 0:
        sys.stderr.write(proc.stdout + proc.stderr)
        sys.exit(proc.returncode)
    print(proc.stdout.strip().splitlines()[-1])
    sys.exit(0)

import numpy as np
import torch

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import paths as P
from homework_18_graphics_raytracer_amd._capi import Light, SceneDesc

torch.cuda.set_device(0)
n_lights = 3 if a.step == "lights3" else 8
world = rt.reference_world()
desc = world.desc()
lights = (Light * n_lights)(*[desc.lights[l % desc.n_lights] for l in range(n_lights)])  # the scene's own lights, repeated
wide = SceneDesc(desc.triangles, desc.n_triangles, desc.spheres, desc.n_spheres, desc.materials, desc.n_materials, lights, n_lights)
stream = torch.cuda.Stream()
with torch.cuda.stream(stream):
    scene = rt.Scene(wide)
    rays = rt.camera_rays(rt.reference_camera(), rt.Frame.full(a.width, a.height, 0))
    hits = rt.cast_rays(scene, rays)
    N, spp = rays.shape[0], a.spp
    ids = torch.arange(N, dtype=torch.int32, device="cuda")
    n_hits = int(rt.Hits(hits).hit.sum().item())
    radii = torch.full((n_lights,), 0.3, dtype=torch.float32, device="cuda")

    paths, radiance = P.begin(N, 1, ids)
    shadow_rays = torch.empty((N, 11), dtype=torch.int32, device="cuda")
    asks, pending = torch.zeros((N,), dtype=torch.uint8, device="cuda"), torch.zeros((N, 3), dtype=torch.float32, device="cuda")
    reach, asked = torch.zeros((N,), dtype=torch.float32, device="cuda"), torch.zeros((N,), dtype=torch.uint8, device="cuda")

    def put_back():
        asks.copy_(asked)

    def connect():
        P.connect_lights(scene, paths, hits, rays, None, None, 1, radii, None, 0, None, shadow_rays, asks, pending, reach, None, stream=stream)

    connect()
    asked.copy_(asks)
    m = spp * N
    rgb = torch.zeros((N, 3), dtype=torch.float32, device="cuda")
    w = P.workspace(N, "cuda", spp, scene, light_nee=True)
    loop = lambda **options: P.trace_paths(scene, hits, rays, spp, a.bounces, None, 3, 0.05, 1, ids, rgb, stream=stream, workspace=w, **options)
    calls = {
        "connect_lights": connect,
        "settle_lights": lambda: P.settle_lights(paths, asks, shadow_rays, reach, pending, radiance, None, stream=stream),
        "trace_paths": lambda: loop(open_casts=False),
        "trace_paths_open_casts": lambda: loop(open_casts=True),
        "trace_paths_light_nee": lambda: loop(light_nee=True),
    }
    for _ in range(a.warmup):
        for fn in calls.values():
            put_back()
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in calls}
    for _ in range(a.steps):
        for name, fn in calls.items():
            put_back()
            ms[name].append(_bench.time_ms(fn))
    stream.synchronize()
    plain = min(float(np.median(ms["trace_paths"])), float(np.median(ms["trace_paths_open_casts"])))
    res = {"records": N, "hits": n_hits, "lights": n_lights, "spp": spp, "bounces": a.bounces, "asks_of_bounce_0": int(asked.sum().item()),
           "connect_lights": _bench.summary(ms["connect_lights"], rate=("mpaths_s", N)),
           "settle_lights": _bench.summary(ms["settle_lights"], rate=("mpaths_s", N)),
           "trace_paths": _bench.summary(ms["trace_paths"], rate=("mpaths_s", m)),
           "trace_paths_open_casts": _bench.summary(ms["trace_paths_open_casts"], rate=("mpaths_s", m)),
           "trace_paths_light_nee": _bench.summary(ms["trace_paths_light_nee"], rate=("mpaths_s", m)),
           "light_nee_over_plain": round(float(np.median(ms["trace_paths_light_nee"])) / plain, 3)}
res["device"] = torch.cuda.get_device_name(0)
print(json.dumps(res))
