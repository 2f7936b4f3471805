#!/usr/bin/env python3
"""Timing of the environment queries (include/rt_amd.h rt_environment_table / _lookup / _rays / _fold; Python rt.environment) on the
primary hits of the reference scene.

    python tools/bench_environment.py [--steps 9 --warmup 3] [--out profiles/environment_bench.jsonl]

Every case is a child process of its own under its own `timeout -k 10 <--step-timeout>`; a case that fails or runs out of time ends the
run, and nothing more is started on the device.  The cases:
    table        rt_environment_table of a --env-width x --env-height image (2048 x 1024): the three kernels and the header's memset
    queries      on the 1920 x 1080 primary rays and hits, --spp samples (16), stratified, ids = the pixel index:
                   lookup          rt_environment_lookup of every ray, NEAREST and BILINEAR   (Grays/s)
                   lookup_misses   the same with d_hits: the rays that found nothing alone
                   rays            rt_environment_rays
                   fold            rt_environment_fold with the shadow hits and the probes of the sequence
                   rays_fold       the two together                                            (Msamples/s)
                   sky_hits        environment.sky_hits, the whole sequence with its casts
Milliseconds are medians of device events, the forms alternated call by call.  Beside each time stands `floor_ms`: the bytes the call
must move (stated per case in DESIGN.md 3.32) at --hbm-gbs, and `of_floor` = floor_ms / ms_median.  No figure is a gate.  Appends one
JSON line with the commit to --out and prints it.
"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import _bench

STEPS = ("table", "queries")
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
ap.add_argument("--out", default=str(ROOT / "profiles" / "environment_bench.jsonl"))
a = ap.parse_args()

if a.step is None:
    _bench.run_cases("bench_environment", a.cases,
                     lambda case: ["--step", case] + _bench.options(a, "steps", "warmup", "width", "height", "env_width", "env_height", "spp", "hbm_gbs"),
                     a.step_timeout, a.out, header={"steps": a.steps, "warmup": a.warmup, "spp": a.spp, "hbm_gbs": a.hbm_gbs})
    sys.exit(0)

import numpy as np
import torch

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import environment as E

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
    env = E.Environment(torch.tensor(sky, device="cuda"), 0.3, 1.0, E.BILINEAR)
    if a.step == "table":
        table = torch.empty((E.table_bytes(W, H),), dtype=torch.uint8, device="cuda")
        ms = _bench.alternate({"table": lambda: E.table(env, out=table, stream=stream)}, a.warmup, a.steps)
        # the texels twice (the maximum, then the quanta), the rows written once; the marginal is H words, read and written
        res = {"width": W, "height": H, "table_bytes": int(table.numel()), "table": with_floor(ms["table"], 2 * 12 * W * H + 4 * W * H + 24 * H)}
        res["total"] = E.table_fields(table, W, H)["total"]
    else:
        scene = rt.Scene(rt.reference_world())
        rays = rt.camera_rays(rt.reference_camera(), rt.Frame.full(a.width, a.height, 0))
        hits = rt.cast_rays(scene, rays)
        N, spp = rays.shape[0], a.spp
        m = spp * N
        ids = torch.arange(N, dtype=torch.int32, device="cuda")
        view = (-rays[:, 3:6].view(torch.float32)).contiguous()
        rgb, behind = torch.zeros((N, 3), dtype=torch.float32, device="cuda"), torch.zeros((N, 3), dtype=torch.float32, device="cuda")
        casts = torch.zeros(1, dtype=torch.int64, device="cuda")
        w = E.workspace(N, "cuda", spp)
        nearest = E.Environment(env.texels, 0.3, 1.0, E.NEAREST)
        table = env.table(stream)

        def sky_loop():
            E.sky_hits(scene, env, hits, view, spp, rgb, E.STRATIFIED, 1, ids, ray_count=casts, stream=stream, workspace=w)

        sky_loop()  # leaves the rays, the shadow hits and the probes in the workspace
        stream.synchronize()
        n_hits, asked, n_casts = int(rt.Hits(hits).hit.sum().item()), int(w.asks[:m].sum().item()), int(casts.item())
        sample_rays = lambda: E.rays(scene, env, hits, spp, E.STRATIFIED, 1, ids, E.SHADING, table, w.rays[:m], w.asks[:m], w.dirs[:m], w.radiance[:m],
                                     w.texel[:m], stream=stream)
        fold = lambda: E.fold(scene, hits, w.asks[:m], spp, w.radiance[:m], w.diffuse[:m], w.specular[:m], rgb, w.shadow_hits[:m], stream=stream)
        calls = {
            "lookup_nearest": lambda: E.lookup(nearest, rays, out=behind, stream=stream),
            "lookup_bilinear": lambda: E.lookup(env, rays, out=behind, stream=stream),
            "lookup_misses": lambda: E.lookup(env, rays, hits, out=behind, stream=stream),
            "rays": sample_rays,
            "fold": fold,
            "rays_fold": lambda: (sample_rays(), fold()),
            "sky_hits": sky_loop,
        }
        ms = _bench.alternate(calls, a.warmup, a.steps)
        # per record: a ray read (44 B) and a colour written (12 B); the texels are cached.  With hits: the kind word of every record,
        # the ray and the colour of a miss
        look = 56 * N
        # per entry: the ray (44), the flag (1), the direction, the radiance (12 each) and the texel (4) written; per record a hit read (52)
        drawn = 73 * m + 52 * N
        # per entry: the flag (1), the kind word of the shadow hit where asked (4), radiance, diffuse, specular where open (36, here: where
        # asked); per record the hit (52) and the colour read and written (24)
        folded = m + 40 * asked + 76 * N
        res = {"records": N, "hits": n_hits, "spp": spp, "asked": asked, "casts": n_casts,
               "lookup_nearest": with_floor(ms["lookup_nearest"], look, ("grays_s", N / 1e3)),
               "lookup_bilinear": with_floor(ms["lookup_bilinear"], look, ("grays_s", N / 1e3)),
               "lookup_misses": with_floor(ms["lookup_misses"], 4 * N + 56 * (N - n_hits), ("grays_s", N / 1e3)),
               "rays": with_floor(ms["rays"], drawn, ("msamples_s", m)),
               "fold": with_floor(ms["fold"], folded, ("msamples_s", m)),
               "rays_fold": with_floor(ms["rays_fold"], drawn + folded, ("msamples_s", m)),
               "sky_hits": _bench.summary(ms["sky_hits"], rate=("msamples_s", m))}
res["device"] = torch.cuda.get_device_name(0)
print(json.dumps(res))
