#!/usr/bin/env python3
"""Timing of the path queries (include/rt_amd.h rt_path_begin / rt_path_advance / rt_path_resolve; Python rt.paths) on the primary
hits of the reference scene.

    python tools/bench_paths.py [--steps 9 --warmup 3] [--out profiles/paths_bench.jsonl]

The case runs in a child process of its own under its own `timeout -k 10 <--step-timeout>`; if it fails or runs out of time the run
ends, and nothing more is started on the device.  On the 1920 x 1080 primary rays and hits, one path per pixel, ids = the pixel index:
    advance           rt_path_advance, bounce 0, every path alive, no roulette          (Mpaths/s)
    unfused           the five calls it replaces: rt_material_hits -> rt_lobe_rays(spp 1) -> rt_probe_surfaces -> rt_mis_weigh
                      (divide_by_own) -> rt_environment_fold(spp 1) into a zeroed throughput
    begin, resolve    rt_path_begin and rt_path_resolve at --spp samples
    trace_paths       paths.trace_paths, --spp samples, --bounces bounces, under a --env-width x --env-height sky, roulette from bounce 3
and, from two more runs of the loop, the share of paths that are alive when bounce b begins, with roulette from bounce 1 and without.
Milliseconds are medians of device events, the forms alternated call by call; advance changes its records, so they are put back
(untimed) before every call.  Beside advance's time stands `floor_ms`: the bytes the call must move (stated in DESIGN.md 3.35) at
--hbm-gbs, and `of_floor` = floor_ms / ms_median.  No figure is a gate.  Appends one JSON line with the commit to --out and prints it.
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
ap.add_argument("--spp", type=int, default=4)
ap.add_argument("--bounces", type=int, default=4)
ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="the bandwidth the floor is computed at, GB/s")
ap.add_argument("--cases", nargs="+", choices=STEPS, default=list(STEPS))
ap.add_argument("--step", choices=STEPS, help="run this case in this process and print its JSON")
ap.add_argument("--step-timeout", type=int, default=300)
ap.add_argument("--out", default=str(ROOT / "profiles" / "paths_bench.jsonl"))
a = ap.parse_args()

if a.step is None:
    _bench.run_cases("bench_paths", a.cases,
                     lambda case: ["--step", case] + _bench.options(a, "steps", "warmup", "width", "height", "env_width", "env_height", "spp", "bounces", "hbm_gbs"),
                     a.step_timeout, a.out, header={"steps": a.steps, "warmup": a.warmup, "spp": a.spp, "bounces": a.bounces, "hbm_gbs": a.hbm_gbs})
    sys.exit(0)

import numpy as np
import torch

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import environment as E, lobes as L, materials, paths as P

torch.cuda.set_device(0)
W, H = a.env_width, a.env_height
g = np.random.default_rng(1)
sky = (g.random((H, W, 3), dtype=np.float32) ** 4 * 8).astype(np.float32)
stream = torch.cuda.Stream()
with torch.cuda.stream(stream):
    env = E.Environment(torch.tensor(sky, device="cuda"), 0.3, 1.0, E.NEAREST)
    scene = rt.Scene(rt.reference_world())
    rays = rt.camera_rays(rt.reference_camera(), rt.Frame.full(a.width, a.height, 0))
    hits = rt.cast_rays(scene, rays)
    N, spp = rays.shape[0], a.spp
    ids = torch.arange(N, dtype=torch.int32, device="cuda")
    view = (-rays[:, 3:6].view(torch.float32)).contiguous()
    emitted = rt.shade_hits(scene, hits, rays)
    n_hits = int(rt.Hits(hits).hit.sum().item())

    # the fused step and the sequence it replaces, one path per pixel
    fresh, radiance = P.begin(N, 1, ids)
    paths, vertices = fresh.clone(), hits.clone()
    next_rays, alive = torch.empty((N, 11), dtype=torch.int32, device="cuda"), torch.empty((N,), dtype=torch.uint8, device="cuda")
    lw = L.workspace(N, "cuda", 1)
    beta, beta_next = torch.ones((N, 3), dtype=torch.float32, device="cuda"), torch.zeros((N, 3), dtype=torch.float32, device="cuda")

    def put_back():
        paths.copy_(fresh)
        vertices.copy_(hits)
        beta.fill_(1.0)

    def fused():
        P.advance(scene, paths, vertices, rays, radiance, emitted, None, None, 1, P.SHADING, P.NO_ROULETTE, 0.05, False, next_rays, alive, stream=stream)

    def unfused():
        materials.material_hits(scene, hits, lw.surfaces[:N], stream=stream)
        L.rays(scene, hits, rays, 1, L.UNIFORM, 1, ids, L.SHADING, lw.rays[:N], lw.asks[:N], lw.dirs[:N], lw.pdf[:N], lw.lobe[:N], stream=stream)
        materials.probe_surfaces(lw.surfaces[:N], view, lw.dirs[:N].view(1, N, 3), lw.diffuse[:N].view(1, N, 3), lw.specular[:N].view(1, N, 3), stream=stream)
        L.mis_weigh(lw.pdf[:N], 1, None, 0, L.BALANCE, True, None, beta, stream=stream)
        beta_next.zero_()
        E.fold(scene, hits, lw.asks[:N], 1, beta, lw.diffuse[:N], lw.specular[:N], beta_next, None, stream=stream)

    m = spp * N
    many, many_radiance = P.begin(N, spp, ids)
    rgb = torch.zeros((N, 3), dtype=torch.float32, device="cuda")
    w = P.workspace(N, "cuda", spp)
    calls = {
        "advance": fused,
        "unfused": unfused,
        "begin": lambda: P.begin(N, spp, ids, many, many_radiance, stream=stream),
        "resolve": lambda: P.resolve(many_radiance, N, spp, rgb, stream=stream),
        "trace_paths": lambda: P.trace_paths(scene, hits, rays, spp, a.bounces, env, 3, 0.05, 1, ids, rgb, False, stream, w),
    }
    for _ in range(a.warmup):
        for fn in calls.values():
            put_back()
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in calls}
    for _ in range(a.steps):
        for name, fn in calls.items():
            put_back()
            ms[name].append(_bench.time_ms(fn))
    put_back()
    fused()
    stream.synchronize()
    survivors = int(alive.sum().item())

    def live_share(rr_start):
        """the share of the m paths that are alive when bounce b begins, b = 0 .. bounces: those that took at least b bounces"""
        P.trace_paths(scene, hits, rays, spp, a.bounces, env, rr_start, 0.05, 1, ids, rgb, False, stream, w)
        stream.synchronize()
        taken = (w.paths[:m, 6] & 0xFFFFFF).cpu().numpy()
        return [round(float((taken >= b).mean()), 4) for b in range(a.bounces + 1)]

    # per path: the record read and written (64), a hit (52), the incoming direction (12) and the emitted light (12) read, the radiance
    # read and written (24), the next ray (44) and the flag (1) written
    moved = 209 * N
    fused_r = _bench.summary(ms["advance"], rate=("mpaths_s", N))
    fused_r["bytes"] = int(moved)
    fused_r["floor_ms"] = round(moved / (a.hbm_gbs * 1e9) * 1e3, 4)
    fused_r["of_floor"] = round(fused_r["floor_ms"] / fused_r["ms_median"], 3)
    res = {"records": N, "hits": n_hits, "spp": spp, "bounces": a.bounces, "survivors_of_bounce_0": survivors,
           "advance": fused_r,
           "unfused": _bench.summary(ms["unfused"], rate=("mpaths_s", N)),
           "fused_over_unfused": round(float(np.median(ms["unfused"]) / np.median(ms["advance"])), 3),
           "begin": _bench.summary(ms["begin"], rate=("mpaths_s", m)),
           "resolve": _bench.summary(ms["resolve"], rate=("mpaths_s", m)),
           "trace_paths": _bench.summary(ms["trace_paths"], rate=("mpaths_s", m)),
           "live_share_roulette_from_1": live_share(1),
           "live_share_no_roulette": live_share(P.NO_ROULETTE)}
res["device"] = torch.cuda.get_device_name(0)
print(json.dumps(res))
