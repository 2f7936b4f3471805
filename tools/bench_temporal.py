#!/usr/bin/env python3
"""Timing of the temporal queries (include/rt_amd.h "temporal queries"; Python rt.temporal): rt_temporal_motion and rt_temporal_accumulate
against their traffic floors.

    python tools/bench_temporal.py [--steps 7 --warmup 2 --launches 10 --width 1920 --height 1080] [--out profiles/temporal_bench.jsonl]

Two cases, each a child process of its own under its own `timeout -k 10 <--step-timeout>`; if one fails or runs out of time the run ends
there and nothing more is started:
    compact    compact guide planes (strides 3, 3, 1, 1), an unchanged camera: every pixel lands within a rounding error of its own centre
    records    the guides where materials.primary_surfaces leaves them — views of rt_hit (13 words) and rt_surface (18 words) records —
               and the camera translated sideways by --shift of the scene's radius, so that coordinates are fractional and taps scatter
The image is the Whitted frame of the reference scene plus seeded Gaussian noise; the previous frame's guides are its primary surfaces
from the previous camera, and its history is one accumulate of that frame.  A timed window is --launches calls of ONE entry point back to
back between two device events — the C entry point itself, its arguments made beforehand — and is reported per call.  Per case and
entry point: the median of --steps windows with their spread (max - min), and the traffic floor over --hbm-tb-per-s.  Per pixel the
floor of accumulate is the current colour (12 B), motion (8), the current guides (normal 12, position 12, object 4, valid 4) read once,
four history records (128: neighbours share them through the caches; the floor does not assume that) and the previous guides of one
tap (32), and the record (32) and the variance (4) written: 248 B; of motion the position (12), valid (4) and the
two coordinates written (8): 24 B.  No figure is a gate.  Appends one JSON line to --out and prints it, with the commit where the tree
is a git checkout and always with the hash of the kernel sources the library was built from.
"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import _bench

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=7, help="timed windows per entry point")
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--launches", type=int, default=10, help="back-to-back calls per timed window")
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--shift", type=float, default=0.02, help="records: the camera's sideways step between the two frames, in scene radii")
ap.add_argument("--hbm-tb-per-s", type=float, default=6.3, help="achievable HBM bandwidth the floors are computed with")
ap.add_argument("--child", choices=["compact", "records"], help="measure this case in this process and print its JSON")
ap.add_argument("--step-timeout", type=int, default=300)
ap.add_argument("--out", default=str(ROOT / "profiles" / "temporal_bench.jsonl"))
a = ap.parse_args()

if not a.child:
    from homework_18_graphics_raytracer_amd import _capi

    _bench.run_cases("bench_temporal", ("compact", "records"),
                     lambda case: ["--child", case] + _bench.options(a, "steps", "warmup", "launches", "width", "height", "shift", "hbm_tb_per_s"),
                     a.step_timeout, a.out, header={"sources_sha256": _capi.sources_sha256()})
    sys.exit(0)

import ctypes as C

import numpy as np
import torch

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import _capi, materials, temporal

torch.cuda.set_device(0)
lib = _capi.amd_lib()
rows, cols = a.height, a.width
n = rows * cols
frame = rt.Frame.full(cols, rows, 3)
stream = torch.cuda.Stream()
sp = C.c_void_p(stream.cuda_stream)

world = rt.reference_world()
scene, cam = rt.Scene(world), rt.reference_camera()
before = rt.Camera.from_buffer_copy(cam)
if a.child == "records":
    _, radius = _bench.bounds(world.desc())
    toward, up = np.array(list(cam.toward)), np.array(list(cam.up))
    right = np.cross(toward, up) / np.linalg.norm(np.cross(toward, up))
    for k in range(3):
        before.center[k] = cam.center[k] - a.shift * radius * right[k]
image = rt.render_whitted(scene, cam, frame)
image = (image + 0.2 * torch.randn(image.shape, dtype=torch.float32, device="cuda", generator=torch.Generator(device="cuda").manual_seed(7))).contiguous()


def guides(s):
    g = temporal.Guides.of(s)
    if a.child == "compact":
        g = temporal.Guides(*(t.contiguous() for t in g))
    c = _capi.TemporalGuides(g.normal.data_ptr(), g.position.data_ptr(), g.object.data_ptr(), g.valid.data_ptr(), g.normal.stride(-2), g.position.stride(-2),
                             g.object.stride(-1), g.valid.stride(-1))
    return g, c


s_cur, s_prev = materials.primary_surfaces(scene, cam, frame), materials.primary_surfaces(scene, before, frame)
(t_cur, g_cur), (t_prev, g_prev) = guides(s_cur), guides(s_prev)
p = _capi.TemporalParams(temporal.NORMAL_MIN, temporal.POSITION_MAX, temporal.ALPHA_MIN, temporal.MAX_LENGTH, 0)
motion = torch.zeros((rows, cols, 2), dtype=torch.float32, device="cuda")
variance = torch.zeros((rows, cols), dtype=torch.float32, device="cuda")
empty = torch.zeros((n, 8), dtype=torch.int32, device="cuda")
history, _ = temporal.accumulate(image, temporal.motion(t_prev.position, before, frame, valid=t_prev.valid), rows, cols, empty, t_prev, t_prev)
out = torch.zeros_like(history)
torch.cuda.synchronize()


def ptr(t):
    return C.c_void_p(t.data_ptr())


calls = {
    "motion": lambda: lib.rt_temporal_motion(ptr(t_cur.position), g_cur.position_stride, ptr(t_cur.valid), g_cur.valid_stride, C.byref(before), C.byref(frame),
                                             ptr(motion), sp),
    "accumulate": lambda: lib.rt_temporal_accumulate(ptr(image), ptr(motion), C.byref(g_cur), C.byref(g_prev), C.byref(p), rows, cols, ptr(history), ptr(out),
                                                     ptr(variance), sp),
}


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
        t = {name: window(call) for name, call in calls.items()}  # motion first: accumulate reads what it wrote
        if k >= a.warmup:
            for name in ms:
                ms[name].append(t[name])
torch.cuda.synchronize()
length = out.view(rows, cols, 8)[..., 5]
valid = t_cur.valid.reshape(rows, cols) != 0
floors = {"motion": n * 24, "accumulate": n * 248}
res = {"device": torch.cuda.get_device_name(0), "rows": rows, "cols": cols, "steps": a.steps, "warmup": a.warmup, "launches_per_window": a.launches,
       "normal_stride": int(g_cur.normal_stride), "position_stride": int(g_cur.position_stride), "object_stride": int(g_cur.object_stride),
       "valid_stride": int(g_cur.valid_stride), "shift_radii": a.shift if a.child == "records" else 0.0, "hbm_tb_per_s": a.hbm_tb_per_s,
       "valid_pixels": int(valid.sum()), "blended_pixels": int((length[valid] > 1).sum())}
for name in calls:
    res[name] = _bench.summary(ms[name], spread=True)
    res[name]["floor_bytes"] = floors[name]
    res[name]["floor_ms"] = round(floors[name] / (a.hbm_tb_per_s * 1e12) * 1e3, 4)
    res[name]["times_floor"] = round(res[name]["ms_median"] / (floors[name] / (a.hbm_tb_per_s * 1e12) * 1e3), 2)
print(json.dumps(res))
