#!/usr/bin/env python3
"""Timing of the bloom query (include/rt_amd.h "bloom queries"; Python rt.bloom): both forms of rt_bloom against each other and against
the call's counted traffic.

    timeout -k 10 600 python tools/bench_bloom.py [--steps 7 --warmup 2 --calls 10 --width 1920 --height 1080] [--out profiles/bloom_bench.jsonl]

Four cases — 1, 3, 5 and 8 levels — each a child process of its own under its own `timeout -k 10 <--step-timeout>`; if one fails or runs
out of time the run ends there and nothing more is started.  The image is seeded: lumas below 0.9 with about 2 % of the pixels lifted
above the threshold by factors from 1.5 to 1000, compact.  A timed window is --calls calls of the entry point itself (its arguments made
once) back to back between two device events and is reported per call and, divided by the call's 2 L launches, per launch; the two
forms (RT_AMD_BLOOM_FORM 0 plain, 1 tiled down steps) are alternated window by window.  Per case: medians of --steps windows with their
spread (max - min), that both forms returned the same bits, the counted traffic — every plane a step must read or write once — over
--hbm-tb-per-s as a floor, and each form's multiple of it.  No figure is a gate.  Appends one JSON line to --out and prints it.
"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import _bench

CASES = {"levels1": 1, "levels3": 3, "levels5": 5, "levels8": 8}

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=7, help="timed windows per form")
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--calls", type=int, default=10, help="back-to-back calls per timed window")
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--hbm-tb-per-s", type=float, default=6.3, help="achievable HBM bandwidth the floor is computed with")
ap.add_argument("--child", choices=sorted(CASES), help="measure this case in this process and print its JSON")
ap.add_argument("--step-timeout", type=int, default=120)
ap.add_argument("--out", default=str(ROOT / "profiles" / "bloom_bench.jsonl"))
a = ap.parse_args()

if not a.child:
    from homework_18_graphics_raytracer_amd import _capi

    _bench.run_cases("bench_bloom", list(CASES), lambda case: ["--child", case] + _bench.options(a, "steps", "warmup", "calls", "width", "height", "hbm_tb_per_s"),
                     a.step_timeout, a.out, header={"sources_sha256": _capi.sources_sha256()})
    sys.exit(0)

import ctypes as C

import torch

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import _capi, bloom

torch.cuda.set_device(0)
levels = CASES[a.child]
rows, cols = a.height, a.width
g = torch.Generator(device="cuda").manual_seed(31)
color = 0.05 + 0.8 * torch.rand((rows, cols, 3), generator=g, device="cuda", dtype=torch.float32)
lifted = torch.rand((rows, cols), generator=g, device="cuda") < 0.02
factor = torch.tensor([1.5, 4.0, 30.0, 1000.0], device="cuda")[torch.randint(0, 4, (rows, cols), generator=g, device="cuda")]
color = torch.where(lifted[..., None], color * 24.0 * factor[..., None], color).contiguous()
stream = torch.cuda.Stream()
outs = {form: torch.zeros((rows, cols, 3), dtype=torch.float32, device="cuda") for form in (0, 1)}
temp = torch.zeros((bloom.temp_bytes(rows, cols, levels) // 4,), dtype=torch.float32, device="cuda")
torch.cuda.synchronize()

lib = _capi.amd_lib()
sp = C.c_void_p(stream.cuda_stream)
params = _capi.BloomParams(bloom.THRESHOLD, bloom.KNEE, bloom.INTENSITY, levels)


def ptr(t):
    return C.c_void_p(t.data_ptr())


def window(form):
    """milliseconds per call of --calls calls of one form back to back: the entry point itself, its arguments made once"""
    rt.set_option("RT_AMD_BLOOM_FORM", form)
    out = ptr(outs[form])
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.calls):
        _capi.check(lib.rt_bloom(ptr(color), 3, C.byref(params), rows, cols, ptr(temp), out, sp))
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / a.calls


ms = {0: [], 1: []}
with torch.cuda.stream(stream):
    for k in range(a.warmup + a.steps):
        for form in (0, 1):
            t = window(form)
            if k >= a.warmup:
                ms[form].append(t)
torch.cuda.synchronize()
rt.set_option("RT_AMD_BLOOM_FORM", None)

# the counted traffic: a down step reads its source level once and writes its own; an up-and-add step reads the coarser level and its
# own and writes its own; the composite reads the colour and level 1 and writes the output
sizes, r, c = [rows * cols * 12], rows, cols
for _ in range(levels):
    r, c = (r + 1) // 2, (c + 1) // 2
    sizes.append(r * c * 12)
down = sum(sizes[j - 1] + sizes[j] for j in range(1, levels + 1))
up = sum(sizes[j + 1] + 2 * sizes[j] for j in range(1, levels))
composite = 2 * sizes[0] + sizes[1]
floor_bytes = down + up + composite
floor_ms = floor_bytes / (a.hbm_tb_per_s * 1e12) * 1e3
res = {"device": torch.cuda.get_device_name(0), "rows": rows, "cols": cols, "levels": levels, "launches_per_call": 2 * levels, "steps": a.steps,
       "warmup": a.warmup, "calls_per_window": a.calls, "hbm_tb_per_s": a.hbm_tb_per_s,
       "bytes": {"down": down, "up": up, "composite": composite, "pyramid": sum(sizes[1:])}, "floor_bytes": floor_bytes, "floor_ms": round(floor_ms, 4),
       "same_bits": _bench.same(outs[0], outs[1]), "plain": _bench.summary(ms[0], spread=True), "tiled": _bench.summary(ms[1], spread=True)}
for name in ("plain", "tiled"):
    res[name]["ms_per_launch"] = round(res[name]["ms_median"] / (2 * levels), 4)
    res[name + "_over_floor"] = round(res[name]["ms_median"] / floor_ms, 2)
res["tiled_over_plain"] = round(res["tiled"]["ms_median"] / res["plain"]["ms_median"], 3)
print(json.dumps(res))
