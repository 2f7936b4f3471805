#!/usr/bin/env python3
"""Timing of the motion queries (include/rt_amd.h "motion queries"; Python rt.moving): rt_previous_positions and rt_scene_keep_positions
against their traffic floor, with rt_material_hits — the existing kernel of the same shape, a per-hit gather — measured in the same
process.

    python tools/bench_motion.py [--steps 7 --warmup 2 --launches 10 --width 1920 --height 1080] [--out profiles/motion_bench.jsonl]

Four cases, each a child process of its own under its own `timeout -k 10 <--step-timeout>`; if one fails or runs out of time the run ends
there and nothing more is started:
    unmoved    nothing moved since the keep: every record takes the shortcut and returns its position
    mesh       the dodecahedron's triangles translated by --shift of the scene's radius
    all        every triangle and every sphere translated
    keep       rt_scene_keep_positions alone
The hits are the primary hits of the reference scene's camera over the frame, cast on the scene as it stands after the update.  A timed
window is --launches calls of ONE entry point back to back between two device events — the C entry point itself, its arguments made
beforehand — and is reported per call.  Per case and entry point: the median of --steps windows with their spread (max - min).  The
floor of rt_previous_positions is the hit record read (52 B) and three words written (12 B) per hit, over --hbm-tb-per-s; the scene's
records are shared by neighbouring hits and left to the caches.  No figure is a gate.  Appends one JSON line to --out and prints it,
with the commit where the tree is a git checkout and always with the hash of the kernel sources the library was built from.
"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import _bench

CASES = ("unmoved", "mesh", "all", "keep")
ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=7, help="timed windows per entry point")
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--launches", type=int, default=10, help="back-to-back calls per timed window")
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--shift", type=float, default=0.01, help="the translation between the keep and the query, in scene radii")
ap.add_argument("--hbm-tb-per-s", type=float, default=6.3, help="achievable HBM bandwidth the floor is computed with")
ap.add_argument("--child", choices=CASES, help="measure this case in this process and print its JSON")
ap.add_argument("--step-timeout", type=int, default=300)
ap.add_argument("--out", default=str(ROOT / "profiles" / "motion_bench.jsonl"))
a = ap.parse_args()

if not a.child:
    from homework_18_graphics_raytracer_amd import _capi

    _bench.run_cases("bench_motion", CASES,
                     lambda case: ["--child", case] + _bench.options(a, "steps", "warmup", "launches", "width", "height", "shift", "hbm_tb_per_s"),
                     a.step_timeout, a.out, header={"sources_sha256": _capi.sources_sha256()})
    sys.exit(0)

import ctypes as C

import numpy as np
import torch

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import _capi, moving

torch.cuda.set_device(0)
lib = _capi.amd_lib()
rows, cols = a.height, a.width
n = rows * cols
frame = rt.Frame.full(cols, rows, 3)
stream = torch.cuda.Stream()
sp = C.c_void_p(stream.cuda_stream)

world = rt.reference_world()
desc = world.desc()
scene, cam = rt.Scene(world), rt.reference_camera()
moving.keep_positions(scene)
_, radius = _bench.bounds(desc)
step = np.array([a.shift * radius, 0.0, 0.0], dtype=np.float32)
raw = np.frombuffer(C.string_at(desc.triangles, desc.n_triangles * C.sizeof(_capi.Triangle)), dtype=np.uint32).reshape(-1, 25)
verts = raw[:, 1:].copy().view(np.float32).reshape(-1, 3, 8)
mesh = int((raw[:, 0] == 0).sum())  # object 0, the imported dodecahedron: the first triangles
if a.child in ("mesh", "all"):
    count = mesh if a.child == "mesh" else verts.shape[0]
    verts[:count, :, :3] += step
    scene.update_vertices(0, np.ascontiguousarray(verts[:count]))
if a.child == "all" and desc.n_spheres:
    sph = np.frombuffer(C.string_at(desc.spheres, desc.n_spheres * C.sizeof(_capi.Sphere)), dtype=np.float32).reshape(-1, 5).copy()
    sph[:, 1:4] += step
    scene.update_spheres(0, sph)
hits = rt.cast_rays(scene, rt.camera_rays(cam, frame))
was = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
surfaces = torch.zeros((n, 18), dtype=torch.int32, device="cuda")
torch.cuda.synchronize()


def ptr(t):
    return C.c_void_p(t.data_ptr())


calls = {"material_hits": lambda: lib.rt_material_hits(scene._h, ptr(hits), n, ptr(surfaces), sp)}
if a.child == "keep":
    calls["keep_positions"] = lambda: lib.rt_scene_keep_positions(scene._h, sp)
else:
    calls["previous_positions"] = lambda: lib.rt_previous_positions(scene._h, ptr(hits), n, ptr(was), 3, sp)


def window(call):
    """milliseconds per call of --launches calls back to back"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.launches):
        _capi.check(call())
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / a.launches


ms = {k: [] for k in calls}
with torch.cuda.stream(stream):
    for k in range(a.warmup + a.steps):
        t = {name: window(call) for name, call in calls.items()}
        if k >= a.warmup:
            for name in ms:
                ms[name].append(t[name])
torch.cuda.synchronize()
h = hits.cpu().numpy().view(np.uint32)
res = {"device": torch.cuda.get_device_name(0), "rows": rows, "cols": cols, "steps": a.steps, "warmup": a.warmup, "launches_per_window": a.launches,
       "shift_radii": 0.0 if a.child in ("unmoved", "keep") else a.shift, "hbm_tb_per_s": a.hbm_tb_per_s, "triangles": int(desc.n_triangles),
       "spheres": int(desc.n_spheres), "mesh_triangles": mesh, "hits_on_triangles": int((h[:, 0] == 1).sum()), "hits_on_spheres": int((h[:, 0] == 0).sum()),
       "hits_on_the_mesh": int(((h[:, 0] == 1) & (h[:, 1] < mesh)).sum())}
if a.child != "keep":
    moved = (was.cpu().numpy().view(np.uint32) != h[:, 3:6]).any(axis=1) & (h[:, 0] <= 1)
    res["records_moved"] = int(moved.sum())
for name in calls:
    res[name] = _bench.summary(ms[name], spread=True)
if "previous_positions" in res:
    floor = n * 64
    res["previous_positions"]["floor_bytes"] = floor
    res["previous_positions"]["floor_ms"] = round(floor / (a.hbm_tb_per_s * 1e12) * 1e3, 4)
    res["previous_positions"]["times_floor"] = round(res["previous_positions"]["ms_median"] / (floor / (a.hbm_tb_per_s * 1e12) * 1e3), 2)
    res["previous_positions"]["times_material_hits"] = round(res["previous_positions"]["ms_median"] / res["material_hits"]["ms_median"], 2)
print(json.dumps(res))
