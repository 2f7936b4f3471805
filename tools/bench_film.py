#!/usr/bin/env python3
"""Timing of the film queries (include/rt_amd.h "film queries"; Python rt.film): the two forms of the splat kernel against each other and
against the traffic floor, and rt_camera_rays_offset beside rt_camera_rays at the same record count.

    python tools/bench_film.py [--steps 7 --warmup 2 --launches 10 --width 1920 --height 1080] [--out profiles/film_bench.jsonl]

Three cases, each a child process of its own under its own `timeout -k 10 <--step-timeout>`; if one fails or runs out of time the run
ends there and nothing more is started:
    tent       rt_film_splat, spp 4, tent, radius 1          through RT_AMD_FILM_SPLAT_FORM 0 (simple) and 1 (tiled)
    mitchell   rt_film_splat, spp 16, Mitchell, radius 2     likewise; random samples, stratified offsets, every flag set
    rays       rt_camera_rays_offset with spp 4, beside rt_camera_rays of a frame with 4 times the rows: the same number of records
A timed window is --launches calls of ONE form back to back between two device events — the C entry point itself, its arguments made
beforehand, the switch set before the first event — so the device has the next launch queued while it runs one and the figure is
kernel time, not host time; it is reported per launch.  Per case: medians of --steps windows, the forms alternated window by window,
with their spread (max - min).  Per splat case also the traffic floor: every input byte (12 + 8 + 1 per sample) read once plus sum and
weight (16 bytes per pixel) read and written, over --hbm-tb-per-s; and whether the two forms left the same bits.  No figure is a gate.
Appends one JSON line to --out and prints it: with the commit where the tree is a git checkout, and always with the hash of the kernel
sources the library was built from (_capi.sources_sha256), which ties the figures to a revision either way.
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
ap.add_argument("--hbm-tb-per-s", type=float, default=6.3, help="achievable HBM bandwidth the floor is computed with")
ap.add_argument("--child", choices=["tent", "mitchell", "rays"], help="measure this case in this process and print its JSON")
ap.add_argument("--step-timeout", type=int, default=300)
ap.add_argument("--out", default=str(ROOT / "profiles" / "film_bench.jsonl"))
a = ap.parse_args()

if not a.child:
    from homework_18_graphics_raytracer_amd import _capi

    _bench.run_cases("bench_film", ("tent", "mitchell", "rays"),
                     lambda case: ["--child", case] + _bench.options(a, "steps", "warmup", "launches", "width", "height", "hbm_tb_per_s"), a.step_timeout, a.out,
                     header={"sources_sha256": _capi.sources_sha256()})
    sys.exit(0)

import ctypes as C

import torch

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import _capi, film

torch.cuda.set_device(0)
lib = _capi.amd_lib()
rows, cols = a.height, a.width
n = rows * cols
frame = rt.Frame.full(cols, rows, 0)
stream = torch.cuda.Stream()
sp = C.c_void_p(stream.cuda_stream)


def ptr(t):
    return C.c_void_p(t.data_ptr())


def window(before, call):
    """milliseconds per launch of --launches calls back to back; `before` runs ahead of the first event"""
    before()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.launches):
        _capi.check(call())
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / a.launches


def alternate(forms):
    """forms: name -> (before, call); medians and spreads of the windows, alternated window by window on the stream"""
    ms = {k: [] for k in forms}
    with torch.cuda.stream(stream):
        for k in range(a.warmup + a.steps):
            t = {name: window(*f) for name, f in forms.items()}
            if k >= a.warmup:
                for name in ms:
                    ms[name].append(t[name])
    torch.cuda.synchronize()
    return {name: _bench.summary(v, spread=True) for name, v in ms.items()}


res = {"device": torch.cuda.get_device_name(0), "rows": rows, "cols": cols, "steps": a.steps, "warmup": a.warmup, "launches_per_window": a.launches}
if a.child in ("tent", "mitchell"):
    spp, name, radius = (4, "tent", 1.0) if a.child == "tent" else (16, "mitchell", 2.0)
    gen = torch.Generator(device="cuda").manual_seed(7)
    samples = torch.rand((spp, n, 3), dtype=torch.float32, device="cuda", generator=gen)
    valid = torch.ones((spp, n), dtype=torch.uint8, device="cuda")
    off = film.offsets(frame, spp, "stratified", 1)
    films = {form: film.Film(rows, cols, name, radius, device="cuda") for form in (0, 1)}
    torch.cuda.synchronize()

    def splat(form):
        f = films[form]
        args = (rows, cols, ptr(samples), ptr(valid), ptr(off), spp, f.filter, f.radius, ptr(f.sum), ptr(f.weight), sp)
        return (lambda: rt.set_option("RT_AMD_FILM_SPLAT_FORM", form)), (lambda: lib.rt_film_splat(*args))

    t = alternate({"simple": splat(0), "tiled": splat(1)})
    rt.set_option("RT_AMD_FILM_SPLAT_FORM", None)
    same = bool((films[0].sum.view(torch.int32) == films[1].sum.view(torch.int32)).all()) and \
        bool((films[0].weight.view(torch.int32) == films[1].weight.view(torch.int32)).all())
    floor_bytes = spp * n * (12 + 8 + 1) + 2 * n * 16
    res.update({"spp": spp, "filter": name, "radius": radius, "hbm_tb_per_s": a.hbm_tb_per_s, "floor_bytes": floor_bytes,
                "floor_ms": round(floor_bytes / (a.hbm_tb_per_s * 1e12) * 1e3, 4), "identical_bits": same})
    res.update(t)
    res["tiled_gain_over_simple_spread"] = round((t["simple"]["ms_median"] - t["tiled"]["ms_median"]) / max(t["simple"]["ms_spread"], 1e-4), 2)
else:
    cam = rt.reference_camera()
    off = film.offsets(frame, 4, "stratified", 1)
    rays = torch.empty((4 * n, 11), dtype=torch.int32, device="cuda")
    tall = rt.Frame.full(cols, 4 * rows, 0)
    torch.cuda.synchronize()
    res["records"] = 4 * n
    res.update(alternate({"camera_rays_offset": ((lambda: None), (lambda: lib.rt_camera_rays_offset(C.byref(cam), C.byref(frame), ptr(off), 4, ptr(rays), sp))),
                          "camera_rays": ((lambda: None), (lambda: lib.rt_camera_rays(C.byref(cam), C.byref(tall), ptr(rays), sp)))}))
print(json.dumps(res))
