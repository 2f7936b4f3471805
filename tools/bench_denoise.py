#!/usr/bin/env python3
"""Timing of the denoise queries (include/rt_amd.h "denoise queries"; Python rt.denoise): the two forms of the A-Trous kernel against each
other and against the traffic floor.

    python tools/bench_denoise.py [--steps 7 --warmup 2 --launches 10 --width 1920 --height 1080 --levels 5] [--out profiles/denoise_bench.jsonl]

Two cases, each a child process of its own under its own `timeout -k 10 <--step-timeout>`; if one fails or runs out of time the run ends
there and nothing more is started:
    compact    rt_denoise_atrous with compact guide planes (stride 3, valid stride 1)
    records    the same data where materials.primary_surfaces leaves it: views of rt_hit (13 words) and rt_surface (18 words) records
The image is the Whitted frame of the reference scene plus seeded Gaussian noise; normal, position and valid are its primary surfaces.
A timed window is --launches calls of ONE form back to back between two device events — the C entry point itself (--levels kernel
launches per call), its arguments made beforehand, the switch set before the first event — and is reported per call.  Per case: medians
of --steps windows, RT_AMD_DENOISE_FORM 0 (simple) and 1 (tiled) alternated window by window, with their spread (max - min); the traffic
floor — per level the colour read, the guides read (normal, position, valid) and the colour written, once each, over --hbm-tb-per-s;
and whether the two forms left the same bits.  No figure is a gate.  Appends one JSON line to --out and prints it, with the commit where
the tree is a git checkout and always with the hash of the kernel sources the library was built from.
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
ap.add_argument("--out", default=str(ROOT / "profiles" / "denoise_bench.jsonl"))
a = ap.parse_args()

if not a.child:
    from homework_18_graphics_raytracer_amd import _capi

    _bench.run_cases("bench_denoise", ("compact", "records"),
                     lambda case: ["--child", case] + _bench.options(a, "steps", "warmup", "launches", "width", "height", "levels", "hbm_tb_per_s"),
                     a.step_timeout, a.out, header={"sources_sha256": _capi.sources_sha256()})
    sys.exit(0)

import ctypes as C

import torch

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import _capi, denoise, materials

torch.cuda.set_device(0)
lib = _capi.amd_lib()
rows, cols = a.height, a.width
n = rows * cols
frame = rt.Frame.full(cols, rows, 3)
stream = torch.cuda.Stream()
sp = C.c_void_p(stream.cuda_stream)


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


scene, cam = rt.Scene(rt.reference_world()), rt.reference_camera()
image = rt.render_whitted(scene, cam, frame)
image = (image + 0.2 * torch.randn(image.shape, dtype=torch.float32, device="cuda", generator=torch.Generator(device="cuda").manual_seed(7))).contiguous()
s = materials.primary_surfaces(scene, cam, frame)
normal, position, valid = s.shading_normal, s.position, s.valid
if a.child == "compact":
    normal, position, valid = normal.contiguous(), position.contiguous(), valid.contiguous()
g = _capi.DenoiseGuides(normal.data_ptr(), position.data_ptr(), None, valid.data_ptr(), normal.stride(-2), position.stride(-2), 0, valid.stride(-1))
p = _capi.DenoiseParams(denoise.SIGMA_COLOR, denoise.SIGMA_NORMAL, denoise.SIGMA_POSITION, 0, a.levels, 0)
outs = {form: torch.zeros_like(image) for form in (0, 1)}
temp = torch.zeros_like(image)
torch.cuda.synchronize()


def form_calls(form):
    args = (ptr(image), C.byref(g), C.byref(p), rows, cols, ptr(outs[form]), ptr(temp), sp)
    return (lambda: rt.set_option("RT_AMD_DENOISE_FORM", form)), (lambda: lib.rt_denoise_atrous(*args))


forms = {"simple": form_calls(0), "tiled": form_calls(1)}
ms = {k: [] for k in forms}
with torch.cuda.stream(stream):
    for k in range(a.warmup + a.steps):
        t = {name: window(*f) for name, f in forms.items()}
        if k >= a.warmup:
            for name in ms:
                ms[name].append(t[name])
torch.cuda.synchronize()
rt.set_option("RT_AMD_DENOISE_FORM", None)
t = {name: _bench.summary(v, spread=True) for name, v in ms.items()}
floor_bytes = a.levels * n * (12 + 12 + 12 + 4 + 12)
res = {"device": torch.cuda.get_device_name(0), "rows": rows, "cols": cols, "levels": a.levels, "steps": a.steps, "warmup": a.warmup,
       "launches_per_window": a.launches, "normal_stride": int(g.normal_stride), "position_stride": int(g.position_stride),
       "valid_stride": int(g.valid_stride), "hbm_tb_per_s": a.hbm_tb_per_s, "floor_bytes": floor_bytes,
       "floor_ms": round(floor_bytes / (a.hbm_tb_per_s * 1e12) * 1e3, 4), "identical_bits": _bench.same(outs[0], outs[1])}
res.update(t)
spread = max(t["simple"]["ms_spread"], t["tiled"]["ms_spread"], 1e-4)
res["tiled_gain_over_larger_spread"] = round((t["simple"]["ms_median"] - t["tiled"]["ms_median"]) / spread, 2)
print(json.dumps(res))
