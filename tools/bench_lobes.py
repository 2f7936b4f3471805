#!/usr/bin/env python3
"""Timing of the lobe queries (include/rt_amd.h rt_lobe_rays / rt_lobe_pdf / rt_environment_pdf / rt_mis_weigh; Python rt.lobes) on the
primary hits of the reference scene.

    python tools/bench_lobes.py [--steps 9 --warmup 3] [--out profiles/lobes_bench.jsonl]

The case runs in a child process of its own under its own `timeout -k 10 <--step-timeout>`; if it fails or runs out of time the run
ends, and nothing more is started on the device.  On the 1920 x 1080 primary rays and hits, --spp samples (16), stratified, ids = the
pixel index, under a --env-width x --env-height sky (2048 x 1024):
    lobe_rays         rt_lobe_rays                                                  (Msamples/s)
    lobe_pdf          rt_lobe_pdf of those directions
    environment_pdf   rt_environment_pdf of those directions
    mis_weigh         rt_mis_weigh of the two densities into a radiance array, balance, divide_by_own
    glossy_hits       lobes.glossy_hits at depth 1, the whole sequence with its trace
    sky_hits_mis      lobes.sky_hits_mis with spp / 2 samples of each kind (uniform: 8 is no square), the whole sequence with its casts
Milliseconds are medians of device events, the forms alternated call by call.  Beside each call's time stands `floor_ms`: the bytes
the call must move (stated per case in DESIGN.md 3.33) at --hbm-gbs, and `of_floor` = floor_ms / ms_median.  No figure is a gate.
Appends one JSON line with the commit to --out and prints it.
"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import _bench

STEPS = ("queries",)
ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=9, help="timed calls per form")
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--env-width", type=int, default=2048)
ap.add_argument("--env-height", type=int, default=1024)
ap.add_argument("--spp", type=int, default=16)
ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="the bandwidth the floors are computed at, GB/s")
ap.add_argument("--cases", nargs="+", choices=STEPS, default=list(STEPS))
ap.add_argument("--step", choices=STEPS, help="run this case in this process and print its JSON")
ap.add_argument("--step-timeout", type=int, default=300)
ap.add_argument("--out", default=str(ROOT / "profiles" / "lobes_bench.jsonl"))
a = ap.parse_args()

if a.step is None:
    _bench.run_cases("bench_lobes", a.cases,
                     lambda case: ["--step", case] + _bench.options(a, "steps", "warmup", "width", "height", "env_width", "env_height", "spp", "hbm_gbs"),
                     a.step_timeout, a.out, header={"steps": a.steps, "warmup": a.warmup, "spp": a.spp, "hbm_gbs": a.hbm_gbs})
    sys.exit(0)

import numpy as np
import torch

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import environment as E, lobes as L, materials

torch.cuda.set_device(0)


def with_floor(values, moved_bytes, rate=None):
    r = _bench.summary(values, rate=rate)
    r["bytes"] = int(moved_bytes)
    r["floor_ms"] = round(moved_bytes / (a.hbm_gbs * 1e9) * 1e3, 4)
    r["of_floor"] = round(r["floor_ms"] / r["ms_median"], 3)
    return r


W, H = a.env_width, a.env_height
g = np.random.default_rng(1)
sky = (g.random((H, W, 3), dtype=np.float32) ** 4 * 8).astype(np.float32)  # a few bright texels, many dim ones
stream = torch.cuda.Stream()
with torch.cuda.stream(stream):
    env = E.Environment(torch.tensor(sky, device="cuda"), 0.3, 1.0, E.NEAREST)
    scene = rt.Scene(rt.reference_world())
    rays = rt.camera_rays(rt.reference_camera(), rt.Frame.full(a.width, a.height, 0))
    hits = rt.cast_rays(scene, rays)
    N, spp = rays.shape[0], a.spp
    half = max(spp // 2, 1)
    m = spp * N
    ids = torch.arange(N, dtype=torch.int32, device="cuda")
    view = (-rays[:, 3:6].view(torch.float32)).contiguous()
    rgb = torch.zeros((N, 3), dtype=torch.float32, device="cuda")
    w = L.workspace(N, "cuda", max(spp, 2 * half))
    surfaces = materials.material_hits(scene, hits)
    table = env.table(stream)
    n_hits = int(rt.Hits(hits).hit.sum().item())

    draw = lambda: L.rays(scene, hits, rays, spp, L.STRATIFIED, 1, ids, L.SHADING, w.rays[:m], w.asks[:m], w.dirs[:m], w.pdf[:m], w.lobe[:m], stream=stream)
    draw()
    stream.synchronize()
    asked, speculars = int(w.asks[:m].sum().item()), int(w.lobe[:m].sum().item())
    calls = {
        "lobe_rays": draw,
        "lobe_pdf": lambda: L.pdf(surfaces, view, w.dirs[:m].view(spp, N, 3), L.SHADING, w.pdf[:m], stream=stream),
        "environment_pdf": lambda: L.environment_pdf(env, w.dirs[:m], table, w.pdf_other[:m], w.texel[:m], stream=stream),
        "mis_weigh": lambda: L.mis_weigh(w.pdf[:m], spp, w.pdf_other[:m], spp, L.BALANCE, True, None, w.radiance[:m], stream=stream),
        "glossy_hits": lambda: L.glossy_hits(scene, hits, rays, spp, 1, 1.0, rgb, L.STRATIFIED, 1, ids, view=view, stream=stream, workspace=w),
        "sky_hits_mis": lambda: L.sky_hits_mis(scene, env, hits, rays, half, half, L.BALANCE, rgb, L.UNIFORM, 1, ids, view=view, stream=stream,
                                               workspace=w),
    }
    ms = _bench.alternate(calls, a.warmup, a.steps)
    # per entry: the ray (44), the flag and the lobe (1 each), the direction (12) and the density (4) written; per record a hit (52) and
    # an incoming ray's direction (12) read
    drawn = 62 * m + 64 * N
    # per entry: a direction read (12), a density written (4); per record a surface (72) and a view (12) read
    density = 16 * m + 84 * N
    # per entry: a direction read (12), a density and a texel written (8); the table's two words per entry are cached at best: not counted
    under_table = 20 * m
    # per entry: two densities read (8), a radiance read and written (24)
    weighed = 32 * m
    res = {"records": N, "hits": n_hits, "spp": spp, "asked": asked, "specular": speculars,
           "lobe_rays": with_floor(ms["lobe_rays"], drawn, ("msamples_s", m)),
           "lobe_pdf": with_floor(ms["lobe_pdf"], density, ("msamples_s", m)),
           "environment_pdf": with_floor(ms["environment_pdf"], under_table, ("msamples_s", m)),
           "mis_weigh": with_floor(ms["mis_weigh"], weighed, ("msamples_s", m)),
           "glossy_hits": _bench.summary(ms["glossy_hits"], rate=("msamples_s", m)),
           "sky_hits_mis": _bench.summary(ms["sky_hits_mis"], rate=("msamples_s", 2 * half * N))}
res["device"] = torch.cuda.get_device_name(0)
print(json.dumps(res))
