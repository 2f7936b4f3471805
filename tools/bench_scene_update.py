#!/usr/bin/env python3
"""Cost of moving one object between two frames: rt_scene_update_vertices + the next Whitted frame, beside what it replaces —
rt_scene_destroy + rt_scene_create + the first frame on the new scene (host layout, device allocation and upload, and the per-stream
workspaces allocated again with that frame).

    python tools/bench_scene_update.py [--steps 7 --warmup 2] [--out profiles/scene_update_bench.jsonl]

Every job is a child process of its own under its own `timeout -k 10 <--step-timeout>`; a job that fails or runs out of time ends the run,
and nothing more is started on the device.  The jobs: `reference` (the reference scene, 64 triangles), `spherized4` (the scene around
the spherized dodecahedron of 9 244 triangles) and `spherized6` (147 484 triangles, walked breadth-first).  In each the solid — the object
with the most triangles — is moved a little every step; the frame is 480 x 270 at depth 5.  Per job, wall-clock milliseconds from the
call to the synchronised end of the frame (medians): `update_ms` (the vertices are already on the device), `update_only_ms` (device
events around the update's kernels alone), `recreate_ms`, and their ratio.  Before anything is timed the updated scene's frame is checked
bit for bit against the fresh scene's.  No figure is a gate.  Appends one JSON line with the commit to --out and prints it.
"""
import argparse
import ctypes as C
import json
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import _bench

JOBS = ("reference", "spherized4", "spherized6")
ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=7, help="timed frames per form")
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--jobs", nargs="+", choices=JOBS, default=list(JOBS))
ap.add_argument("--job", choices=JOBS, help="run this job in this process and print its JSON")
ap.add_argument("--step-timeout", type=int, default=300)
ap.add_argument("--out", default=str(ROOT / "profiles" / "scene_update_bench.jsonl"))
a = ap.parse_args()

if a.job is None:
    _bench.run_cases("bench_scene_update", a.jobs, lambda job: ["--job", job] + _bench.options(a, "steps", "warmup"), a.step_timeout, a.out,
                     header={"steps": a.steps, "warmup": a.warmup})
    sys.exit(0)

import numpy as np
import torch

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import _capi

torch.cuda.set_device(0)
with tempfile.TemporaryDirectory() as tmp:
    if a.job.startswith("spherized"):
        level = int(a.job[-1])
        world = _bench.tessellated_world(tmp, level, True)
    else:
        world = rt.reference_world()
desc = world.desc()
camera, frame = rt.reference_camera(), rt.Frame.full(480, 270, 5)

raw = np.frombuffer(C.string_at(desc.triangles, desc.n_triangles * C.sizeof(_capi.Triangle)), dtype=np.uint32).reshape(-1, 25).copy()
solid = np.flatnonzero(raw[:, 0] == np.bincount(raw[:, 0]).argmax())
first, count = int(solid[0]), len(solid)
assert (solid == np.arange(first, first + count)).all()
base = raw[first:first + count, 1:].copy().view(np.float32).reshape(count, 3, 8)


def moved(step):
    v = base.copy()
    v[:, :, 0] += np.float32(0.02 * np.sin(0.7 * step))
    v[:, :, 1] += np.float32(0.02 * (1.0 - np.cos(0.7 * step)))
    return v


def describe(step):
    """the whole description with the solid at `step`, as rt_scene_create wants it"""
    r = raw.copy()
    r[first:first + count, 1:] = moved(step).reshape(count, 24).view(np.uint32)
    tris = (_capi.Triangle * len(r)).from_buffer_copy(r.tobytes())
    d = _capi.SceneDesc(tris, len(r), desc.spheres, desc.n_spheres, desc.materials, desc.n_materials, desc.lights, desc.n_lights)
    d._keepalive = (tris, world)
    return d


def new_scene(d):
    with rt.options(RT_AMD_BFS_WALK_TRIANGLES=8192):  # the library's default switch, set here so that no environment moves it
        return rt.Scene(d)


out = torch.empty((frame.rows, frame.cols, 3), dtype=torch.float32, device="cuda")
scene = new_scene(describe(0))
rt.render_whitted(scene, camera, frame, out=out)
scene.update_vertices(first, moved(1))  # the scene's first update uploads the node ranges
want = rt.render_whitted(new_scene(describe(1)), camera, frame).clone()
rt.render_whitted(scene, camera, frame, out=out)
torch.cuda.synchronize()
identical = bool((out.view(torch.int32) == want.view(torch.int32)).all())

update_ms, update_only_ms, recreate_ms = [], [], []
for k in range(a.warmup + a.steps):
    step = k + 2
    dev = torch.from_numpy(moved(step)).cuda()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    scene.update_vertices(first, dev)
    e1.record()
    rt.render_whitted(scene, camera, frame, out=out)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    d = describe(step)  # building the description is the caller's work either way: not timed
    old = new_scene(describe(step - 1))
    rt.render_whitted(old, camera, frame, out=out)  # a scene in use, with its workspaces: what gets destroyed
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    old.close()
    fresh = new_scene(d)
    rt.render_whitted(fresh, camera, frame, out=out)
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    fresh.close()
    if k >= a.warmup:
        update_ms.append((t1 - t0) * 1e3)
        update_only_ms.append(e0.elapsed_time(e1))
        recreate_ms.append((t3 - t2) * 1e3)

med = lambda x: float(np.median(x))
print(json.dumps({"triangles": int(desc.n_triangles), "moved_triangles": count, "identical": identical, "update_ms": round(med(update_ms), 4),
                  "update_only_ms": round(med(update_only_ms), 4), "recreate_ms": round(med(recreate_ms), 4),
                  "recreate_over_update": round(med(recreate_ms) / med(update_ms), 2)}))
