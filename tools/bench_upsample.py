#!/usr/bin/env python3
"""Timing of the guided upsampling query (include/rt_amd.h "guided upsampling queries"; Python rt.upsample): both kernel forms of
rt_upsample_guided against each other and against the call's traffic floor.

    python tools/bench_upsample.py [--steps 7 --warmup 2 --launches 10 --width 1920 --height 1080] [--out profiles/upsample_bench.jsonl]

Four cases — scale 2 and 4, radius 1 and 2 — each a child process of its own under its own `timeout -k 10 <--step-timeout>`; if one fails
or runs out of time the run ends there and nothing more is started.  The inputs are the reference scene's: materials.primary_surfaces at
both resolutions, their planes passed as the strided views they are (13- and 18-word records), the low-resolution Whitted frame as the
colour, demodulation on, object planes given.  A timed window is --launches calls of the entry point itself (its arguments made once)
back to back between two device events and is reported per call; the two forms (RT_AMD_UPSAMPLE_FORM 0 plain, 1 tiled) are alternated
window by window.  Per case: medians of --steps windows with their spread (max - min), that both forms returned the same bits, the traffic floor — every plane the call must read once (44 bytes
per output pixel, 56 per low pixel) and the 12 bytes per output pixel it writes, over --hbm-tb-per-s — and each form's multiple of it.
No figure is a gate.  Appends one JSON line to --out and prints it.
"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import _bench

CASES = {"scale2_radius1": (2, 1), "scale2_radius2": (2, 2), "scale4_radius1": (4, 1), "scale4_radius2": (4, 2)}

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=7, help="timed windows per form")
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--launches", type=int, default=10, help="back-to-back calls per timed window")
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--hbm-tb-per-s", type=float, default=6.3, help="achievable HBM bandwidth the floor is computed with")
ap.add_argument("--child", choices=sorted(CASES), help="measure this case in this process and print its JSON")
ap.add_argument("--step-timeout", type=int, default=120)
ap.add_argument("--out", default=str(ROOT / "profiles" / "upsample_bench.jsonl"))
a = ap.parse_args()

if not a.child:
    from homework_18_graphics_raytracer_amd import _capi

    _bench.run_cases("bench_upsample", sorted(CASES), lambda case: ["--child", case] + _bench.options(a, "steps", "warmup", "launches", "width", "height", "hbm_tb_per_s"),
                     a.step_timeout, a.out, header={"sources_sha256": _capi.sources_sha256()})
    sys.exit(0)

import ctypes as C

import torch

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import _capi, _forms, upsample
from homework_18_graphics_raytracer_amd.materials import primary_surfaces

torch.cuda.set_device(0)
scale, radius = CASES[a.child]
frame = rt.Frame.full(a.width, a.height, 3)
rows, cols = frame.rows, frame.cols
lo = upsample.low_frame(frame, scale)
scene, cam = rt.Scene(rt.reference_world()), rt.reference_camera()
s_hi, s_lo = primary_surfaces(scene, cam, frame), primary_surfaces(scene, cam, lo)
radiance = rt.render_whitted(scene, cam, lo)
g_lo, g_hi = upsample.Guides.of(s_lo), upsample.Guides.of(s_hi)
stream = torch.cuda.Stream()
outs = {form: torch.zeros((rows, cols, 3), dtype=torch.float32, device="cuda") for form in (0, 1)}
torch.cuda.synchronize()


lib = _capi.amd_lib()
sp = C.c_void_p(stream.cuda_stream)
pl = {name: _forms.denoise_guides(_forms.CUDA, g[0].shape[0] * g[0].shape[1], g.normal, g.position, g.albedo, g.valid) for name, g in (("lo", g_lo), ("hi", g_hi))}
params = _capi.UpsampleParams(upsample.SIGMA_NORMAL, upsample.SIGMA_POSITION, scale, radius, 3)


def ptr(t):
    return C.c_void_p(t.data_ptr())


def window(form):
    """milliseconds per call of --launches calls of one form back to back: the entry point itself, its arguments made once, so that a
    window holds one foreign call per launch and no tensor checks"""
    rt.set_option("RT_AMD_UPSAMPLE_FORM", form)
    out = ptr(outs[form])
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.launches):
        _capi.check(lib.rt_upsample_guided(ptr(radiance), 3, C.byref(pl["lo"]), ptr(g_lo.object), g_lo.object.stride(-1), C.byref(pl["hi"]), ptr(g_hi.object),
                                           g_hi.object.stride(-1), C.byref(params), rows, cols, out, sp))
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / a.launches


ms = {0: [], 1: []}
with torch.cuda.stream(stream):
    for k in range(a.warmup + a.steps):
        for form in (0, 1):
            t = window(form)
            if k >= a.warmup:
                ms[form].append(t)
torch.cuda.synchronize()
rt.set_option("RT_AMD_UPSAMPLE_FORM", None)
n, n_lo = rows * cols, lo.rows * lo.cols
floor_bytes = n * (44 + 12) + n_lo * 56
floor_ms = floor_bytes / (a.hbm_tb_per_s * 1e12) * 1e3
res = {"device": torch.cuda.get_device_name(0), "rows": rows, "cols": cols, "scale": scale, "radius": radius, "steps": a.steps, "warmup": a.warmup,
       "launches_per_window": a.launches, "hbm_tb_per_s": a.hbm_tb_per_s, "floor_bytes": floor_bytes, "floor_ms": round(floor_ms, 4),
       "same_bits": _bench.same(outs[0], outs[1]), "plain": _bench.summary(ms[0], spread=True), "tiled": _bench.summary(ms[1], spread=True)}
for name in ("plain", "tiled"):
    res[name + "_over_floor"] = round(res[name]["ms_median"] / floor_ms, 2)
res["tiled_over_plain"] = round(res["tiled"]["ms_median"] / res["plain"]["ms_median"], 3)
print(json.dumps(res))
