#!/usr/bin/env python3
"""Timing of the history rectification queries (include/rt_amd.h "history rectification queries"; Python rt.rectify): rt_temporal_bounds
at radius 1 and 3 against its traffic floor and against rt_svgf_variance on a frame whose tiles all stage — the existing tile kernel of
the same shape — and rt_temporal_accumulate_bounded against rt_temporal_accumulate on the same records.

    python tools/bench_rectify.py [--steps 7 --warmup 2 --launches 10 --width 1920 --height 1080] [--out profiles/rectify_bench.jsonl]

Two cases, each a child process of its own under its own `timeout -k 10 <--step-timeout>`; if one fails or runs out of time the run ends
there and nothing more is started:
    compact    compact colour, object and valid planes, compact guides
    records    the same data where it lies: guides, object and valid as views of rt_hit (13 words) and rt_surface (18 words) records
The sequence is the Whitted frame of the reference scene plus fresh seeded Gaussian noise per frame, pushed through
temporal.accumulate_frame with a static camera; frame 1's records (length 1 everywhere: every tile of rt_svgf_variance stages) are the
yardstick's input, frame 3's the accumulates'.  A timed window is --launches calls of ONE entry point back to back between two device
events and is reported per call; the calls of a group are alternated window by window.  Per case: medians of --steps windows with
their spread (max - min); rt_temporal_bounds' traffic floor — 12 + 4 + 4 bytes read and 32 written per pixel, once each, over
--hbm-tb-per-s — the multiple of it, and the ratio to the yardstick; the bounded accumulate's difference to the plain one in units of
the larger spread; rt_temporal_feedback.  No figure is a gate.  Appends one JSON line to --out and prints it.
"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import _bench

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=7, help="timed windows per call")
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--launches", type=int, default=10, help="back-to-back calls per timed window")
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--hbm-tb-per-s", type=float, default=6.3, help="achievable HBM bandwidth the floor is computed with")
ap.add_argument("--child", choices=["compact", "records"], help="measure this case in this process and print its JSON")
ap.add_argument("--step-timeout", type=int, default=300)
ap.add_argument("--out", default=str(ROOT / "profiles" / "rectify_bench.jsonl"))
a = ap.parse_args()

if not a.child:
    from homework_18_graphics_raytracer_amd import _capi

    _bench.run_cases("bench_rectify", ("compact", "records"),
                     lambda case: ["--child", case] + _bench.options(a, "steps", "warmup", "launches", "width", "height", "hbm_tb_per_s"),
                     a.step_timeout, a.out, header={"sources_sha256": _capi.sources_sha256()})
    sys.exit(0)

import ctypes as C

import torch

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import _capi, rectify, svgf, temporal

torch.cuda.set_device(0)
lib = _capi.amd_lib()
rows, cols = a.height, a.width
n = rows * cols
frame = rt.Frame.full(cols, rows, 3)
stream = torch.cuda.Stream()
sp = C.c_void_p(stream.cuda_stream)


def ptr(t):
    return C.c_void_p(t.data_ptr())


def window(call):
    """milliseconds per call of --launches calls back to back"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.launches):
        _capi.check(call())
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / a.launches


def alternate(calls):
    """{name: call} -> {name: summary}: every call once per round, alternated window by window"""
    ms = {k: [] for k in calls}
    with torch.cuda.stream(stream):
        for k in range(a.warmup + a.steps):
            t = {name: window(f) for name, f in calls.items()}
            if k >= a.warmup:
                for name in ms:
                    ms[name].append(t[name])
    torch.cuda.synchronize()
    return {name: _bench.summary(v, spread=True) for name, v in ms.items()}


scene, cam = rt.Scene(rt.reference_world()), rt.reference_camera()
clean = rt.render_whitted(scene, cam, frame)
noise = torch.Generator(device="cuda").manual_seed(7)
history = temporal.History(rows, cols)
kept = {}
for k in range(1, 4):  # a static camera: every valid pixel's own tap is accepted, so frame k leaves length k
    image = (clean + 0.2 * torch.randn(clean.shape, dtype=torch.float32, device="cuda", generator=noise)).contiguous()
    temporal.accumulate_frame(scene, cam, frame, image, history)
    kept[k] = history.records.clone()
torch.cuda.synchronize()
s = history._previous[0]
normal, position, obj, valid = s.shading_normal, s.position, s.object_index, s.valid
if a.child == "compact":
    normal, position, obj, valid = normal.contiguous(), position.contiguous(), obj.contiguous(), valid.contiguous()
image = image.view(n, 3)

# ---- rt_temporal_bounds beside rt_svgf_variance on a frame whose tiles all stage ----
box = torch.zeros((n, 8), dtype=torch.float32, device="cuda")
estimate = torch.zeros((rows, cols), dtype=torch.float32, device="cuda")
g = _capi.DenoiseGuides(normal.data_ptr(), position.data_ptr(), None, valid.data_ptr(), normal.stride(-2), position.stride(-2), 0, valid.stride(-1))
vp = _capi.SvgfVarianceParams(svgf.SIGMA_NORMAL, svgf.SIGMA_POSITION, svgf.MIN_LENGTH, 0)
bp = {r: _capi.BoundsParams(rectify.GAMMA, r, 0) for r in (1, 3)}


def bounds_call(r):
    return lambda: lib.rt_temporal_bounds(ptr(image), 3, ptr(obj), obj.stride(-1), ptr(valid), valid.stride(-1), C.byref(bp[r]), rows, cols, ptr(box), sp)


tile = alternate({"bounds_radius1": bounds_call(1), "bounds_radius3": bounds_call(3),
                  "svgf_variance_all_tiles_stage": lambda: lib.rt_svgf_variance(ptr(kept[1]), C.byref(g), C.byref(vp), rows, cols, ptr(estimate), sp)})

# ---- rt_temporal_accumulate_bounded beside rt_temporal_accumulate, and rt_temporal_feedback ----
_capi.check(bounds_call(rectify.RADIUS)())
torch.cuda.synchronize()
tg = _capi.TemporalGuides(normal.data_ptr(), position.data_ptr(), obj.data_ptr(), valid.data_ptr(), normal.stride(-2), position.stride(-2), obj.stride(-1),
                          valid.stride(-1))
tp = _capi.TemporalParams(temporal.NORMAL_MIN, temporal.POSITION_MAX, temporal.ALPHA_MIN, temporal.MAX_LENGTH, 0)
motion = history.motion
outs = [torch.zeros((n, 8), dtype=torch.int32, device="cuda") for _ in range(2)]
variance = torch.zeros((rows, cols), dtype=torch.float32, device="cuda")
clamped = torch.zeros((rows, cols), dtype=torch.int32, device="cuda")
head = (ptr(image), ptr(motion), C.byref(tg), C.byref(tg), C.byref(tp), rows, cols, ptr(kept[3]))
pixel = alternate({"accumulate": lambda: lib.rt_temporal_accumulate(*head, ptr(outs[0]), ptr(variance), sp),
                   "accumulate_bounded": lambda: lib.rt_temporal_accumulate_bounded(*head, ptr(outs[1]), ptr(variance), ptr(box), rectify.CLAMPED_LENGTH,
                                                                                    ptr(clamped), sp),
                   "feedback": lambda: lib.rt_temporal_feedback(ptr(image), 3, ptr(valid), valid.stride(-1), rows, cols, ptr(outs[1]), sp)})
floor_bytes = n * (12 + 4 + 4 + 32)
floor_ms = floor_bytes / (a.hbm_tb_per_s * 1e12) * 1e3
res = {"device": torch.cuda.get_device_name(0), "rows": rows, "cols": cols, "steps": a.steps, "warmup": a.warmup, "launches_per_window": a.launches,
       "normal_stride": int(tg.normal_stride), "object_stride": int(tg.object_stride), "valid_stride": int(tg.valid_stride),
       "hbm_tb_per_s": a.hbm_tb_per_s, "bounds_floor_bytes": floor_bytes, "bounds_floor_ms": round(floor_ms, 4),
       "clamped_pixels_share": round(float((clamped != 0).float().mean().item()), 4)}
res.update(tile)
res.update(pixel)
for r in (1, 3):
    res[f"bounds_radius{r}_over_floor"] = round(tile[f"bounds_radius{r}"]["ms_median"] / floor_ms, 2)
    res[f"bounds_radius{r}_over_svgf_variance"] = round(tile[f"bounds_radius{r}"]["ms_median"] / tile["svgf_variance_all_tiles_stage"]["ms_median"], 3)
spread = max(pixel["accumulate"]["ms_spread"], pixel["accumulate_bounded"]["ms_spread"], 1e-4)
res["bounded_minus_plain_ms"] = round(pixel["accumulate_bounded"]["ms_median"] - pixel["accumulate"]["ms_median"], 4)
res["bounded_minus_plain_over_larger_spread"] = round(res["bounded_minus_plain_ms"] / spread, 2)
print(json.dumps(res))
