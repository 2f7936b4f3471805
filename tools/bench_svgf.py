#!/usr/bin/env python3
"""Timing of the variance-guided filter queries (include/rt_amd.h "variance-guided filter queries"; Python rt.svgf): the two forms of the
A-Trous kernel against each other, against rt_denoise_atrous' tiled form on the same image, levels and guides, and against the traffic
floor; and the variance kernel on histories of different lengths.

    python tools/bench_svgf.py [--steps 7 --warmup 2 --launches 10 --width 1920 --height 1080 --levels 5] [--out profiles/svgf_bench.jsonl]

Two cases, each a child process of its own under its own `timeout -k 10 <--step-timeout>`; if one fails or runs out of time the run ends
there and nothing more is started:
    compact    compact guide planes (stride 3, valid stride 1) and a compact colour plane
    records    the same data where it lies: guides as views of rt_hit (13 words) and rt_surface (18 words) records, the colour inside
               the history records (stride 8)
The sequence is the Whitted frame of the reference scene plus fresh seeded Gaussian noise per frame, pushed through
temporal.accumulate_frame with a static camera; the filter runs on the records of frame 3.  A timed window is --launches calls of ONE
kernel form back to back between two device events — the C entry point itself, its arguments made beforehand, the switch set before
the first event — and is reported per call.  Per case: medians of --steps windows with their spread (max - min), RT_AMD_SVGF_FORM 0
(simple), 1 (tiled) and rt_denoise_atrous' tiled form alternated window by window; the ratio of the chosen form to the denoise filter;
the traffic floor — per level colour and variance read, the guides read (normal, position, valid), colour and variance written, once
each, over --hbm-tb-per-s; whether the two forms left the same bits; and rt_svgf_variance on the records of frames 1, 3 and 5 (lengths
1, 3 and 5 against MIN_LENGTH 4) with the share of its workgroups' tiles that hold no short history and skip staging, counted on the host
from the downloaded records.  No figure is a gate.  Appends one JSON line to --out and prints it.
"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import _bench

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=7, help="timed windows per form")
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--launches", type=int, default=10, help="back-to-back calls per timed window")
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--levels", type=int, default=5)
ap.add_argument("--hbm-tb-per-s", type=float, default=6.3, help="achievable HBM bandwidth the floor is computed with")
ap.add_argument("--child", choices=["compact", "records"], help="measure this case in this process and print its JSON")
ap.add_argument("--step-timeout", type=int, default=300)
ap.add_argument("--out", default=str(ROOT / "profiles" / "svgf_bench.jsonl"))
a = ap.parse_args()

if not a.child:
    from homework_18_graphics_raytracer_amd import _capi

    _bench.run_cases("bench_svgf", ("compact", "records"),
                     lambda case: ["--child", case] + _bench.options(a, "steps", "warmup", "launches", "width", "height", "levels", "hbm_tb_per_s"),
                     a.step_timeout, a.out, header={"sources_sha256": _capi.sources_sha256()})
    sys.exit(0)

import ctypes as C

import numpy as np
import torch

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import _capi, denoise, svgf, temporal

torch.cuda.set_device(0)
lib = _capi.amd_lib()
rows, cols = a.height, a.width
n = rows * cols
frame = rt.Frame.full(cols, rows, 3)
stream = torch.cuda.Stream()
sp = C.c_void_p(stream.cuda_stream)
TILE = 16


def ptr(t):
    return C.c_void_p(t.data_ptr())


def window(before, call):
    """milliseconds per call of --launches calls back to back; `before` runs ahead of the first event"""
    before()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.launches):
        _capi.check(call())
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / a.launches


def alternate(calls):
    """{name: (before, call)} -> {name: summary}: every call once per round, alternated window by window"""
    ms = {k: [] for k in calls}
    with torch.cuda.stream(stream):
        for k in range(a.warmup + a.steps):
            t = {name: window(*f) for name, f in calls.items()}
            if k >= a.warmup:
                for name in ms:
                    ms[name].append(t[name])
    torch.cuda.synchronize()
    return {name: _bench.summary(v, spread=True) for name, v in ms.items()}


def skipped_share(records, valid):
    """the share of the variance kernel's 16 x 16 tiles without a pixel that is valid, has a history and a length below MIN_LENGTH"""
    length = records.cpu().numpy().reshape(rows, cols, 8)[..., 5]
    short = (length > 0) & (length < svgf.MIN_LENGTH) & (valid.cpu().numpy().reshape(rows, cols) != 0)
    pad = np.zeros(((rows + TILE - 1) // TILE * TILE, (cols + TILE - 1) // TILE * TILE), dtype=bool)
    pad[:rows, :cols] = short
    tiles = pad.reshape(pad.shape[0] // TILE, TILE, pad.shape[1] // TILE, TILE).any(axis=(1, 3))
    return round(float(1.0 - tiles.mean()), 4)


scene, cam = rt.Scene(rt.reference_world()), rt.reference_camera()
clean = rt.render_whitted(scene, cam, frame)
noise = torch.Generator(device="cuda").manual_seed(7)
history = temporal.History(rows, cols)
kept = {}
for k in range(1, 6):  # a static camera: every valid pixel's own tap is accepted, so frame k leaves length k
    image = (clean + 0.2 * torch.randn(clean.shape, dtype=torch.float32, device="cuda", generator=noise)).contiguous()
    temporal.accumulate_frame(scene, cam, frame, image, history)
    if k in (1, 3, 5):
        kept[k] = history.records.clone()
torch.cuda.synchronize()
s = history._previous[0]
normal, position, valid = s.shading_normal, s.position, s.valid
records = kept[3]
color = records.view(rows, cols, 8)[..., 0:3].view(torch.float32)
if a.child == "compact":
    normal, position, valid, color = normal.contiguous(), position.contiguous(), valid.contiguous(), color.contiguous()
g = _capi.DenoiseGuides(normal.data_ptr(), position.data_ptr(), None, valid.data_ptr(), normal.stride(-2), position.stride(-2), 0, valid.stride(-1))
color_stride = color.stride(-2)

# ---- rt_svgf_variance on the three histories ----
vp = _capi.SvgfVarianceParams(svgf.SIGMA_NORMAL, svgf.SIGMA_POSITION, svgf.MIN_LENGTH, 0)
estimate = torch.zeros((rows, cols), dtype=torch.float32, device="cuda")
variance_calls = {f"frame{k}": ((lambda: None), (lambda r=kept[k]: lib.rt_svgf_variance(ptr(r), C.byref(g), C.byref(vp), rows, cols, ptr(estimate), sp)))
                  for k in kept}
variance_ms = alternate(variance_calls)
for k in kept:
    variance_ms[f"frame{k}"]["tiles_skipped_share"] = skipped_share(kept[k], valid)
_capi.check(lib.rt_svgf_variance(ptr(records), C.byref(g), C.byref(vp), rows, cols, ptr(estimate), None))
torch.cuda.synchronize()

# ---- rt_svgf_atrous, both forms, beside rt_denoise_atrous' tiled form ----
p = _capi.SvgfAtrousParams(svgf.SIGMA_LUMINANCE, svgf.SIGMA_NORMAL, svgf.SIGMA_POSITION, 0, a.levels, 0)
outs = {form: torch.zeros((rows, cols, 3), dtype=torch.float32, device="cuda") for form in (0, 1)}
vars_ = {form: torch.zeros((rows, cols), dtype=torch.float32, device="cuda") for form in (0, 1)}
temp = torch.zeros(max(svgf.temp_bytes(rows, cols, a.levels) // 4, 1), dtype=torch.float32, device="cuda")
plain = color.contiguous()  # rt_denoise_atrous takes a compact colour plane only
dp = _capi.DenoiseParams(denoise.SIGMA_COLOR, denoise.SIGMA_NORMAL, denoise.SIGMA_POSITION, 0, a.levels, 0)
d_out, d_temp = torch.zeros_like(plain), torch.zeros_like(plain)
torch.cuda.synchronize()


def form_calls(form):
    args = (ptr(color), color_stride, ptr(estimate), C.byref(g), C.byref(p), rows, cols, ptr(outs[form]), ptr(vars_[form]), ptr(temp), sp)
    return (lambda: rt.set_option("RT_AMD_SVGF_FORM", form)), (lambda: lib.rt_svgf_atrous(*args))


denoise_args = (ptr(plain), C.byref(g), C.byref(dp), rows, cols, ptr(d_out), ptr(d_temp), sp)
t = alternate({"simple": form_calls(0), "tiled": form_calls(1),
               "denoise_tiled": ((lambda: rt.set_option("RT_AMD_DENOISE_FORM", 1)), (lambda: lib.rt_denoise_atrous(*denoise_args)))})
rt.set_option("RT_AMD_SVGF_FORM", None)
rt.set_option("RT_AMD_DENOISE_FORM", None)
floor_bytes = a.levels * n * (12 + 4 + 12 + 12 + 4 + 12 + 4)
res = {"device": torch.cuda.get_device_name(0), "rows": rows, "cols": cols, "levels": a.levels, "steps": a.steps, "warmup": a.warmup,
       "launches_per_window": a.launches, "color_stride": int(color_stride), "normal_stride": int(g.normal_stride),
       "position_stride": int(g.position_stride), "valid_stride": int(g.valid_stride), "hbm_tb_per_s": a.hbm_tb_per_s, "floor_bytes": floor_bytes,
       "floor_ms": round(floor_bytes / (a.hbm_tb_per_s * 1e12) * 1e3, 4),
       "identical_bits": _bench.same(outs[0], outs[1]) and _bench.same(vars_[0], vars_[1]), "variance": variance_ms}
res.update(t)
spread = max(t["simple"]["ms_spread"], t["tiled"]["ms_spread"], 1e-4)
res["tiled_gain_over_larger_spread"] = round((t["simple"]["ms_median"] - t["tiled"]["ms_median"]) / spread, 2)
res["tiled_over_denoise_tiled"] = round(t["tiled"]["ms_median"] / t["denoise_tiled"]["ms_median"], 3)
res["simple_over_denoise_tiled"] = round(t["simple"]["ms_median"] / t["denoise_tiled"]["ms_median"], 3)
print(json.dumps(res))
