#!/usr/bin/env python3
"""Timing of the connection queries (include/rt_amd.h rt_path_connect / rt_path_settle / rt_path_weigh_escape; Python rt.paths) on the
primary hits of the reference scene.

    python tools/bench_connect.py [--steps 9 --warmup 3] [--out profiles/connect_bench.jsonl]

The case runs in a child process of its own under its own `timeout -k 10 <--step-timeout>`; if it fails or runs out of time the run
ends, and nothing more is started on the device.  On the 1920 x 1080 primary rays and hits, one path per pixel, ids = the pixel index,
under a --env-width x --env-height sky:
    connect           rt_path_connect, bounce 0, every path alive                       (Mpaths/s)
    unfused           the six calls it replaces: rt_environment_rays(spp 1) -> rt_material_hits -> rt_probe_surfaces ->
                      rt_environment_pdf -> rt_lobe_pdf -> rt_mis_weigh, timed in the same run (the multiply by beta and the fold
                      association, which connect also does, are not even in it)
    settle            rt_path_settle on connect's asks, nothing occluding
    weigh_escape      rt_path_weigh_escape on the same records with a density in every record
    trace_paths       paths.trace_paths, --spp samples, --bounces bounces, roulette from bounce 3, with nee and without
Milliseconds are medians of device events, the forms alternated call by call; settle clears its asks, so they are put back (untimed)
before every call.  Beside the three calls' times stands `floor_ms`: the bytes the call must move (stated in DESIGN.md 3.37) at
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
ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="the bandwidth the floors are computed at, GB/s")
ap.add_argument("--cases", nargs="+", choices=STEPS, default=list(STEPS))
ap.add_argument("--step", choices=STEPS, help="run this case in this process and print its JSON")
ap.add_argument("--step-timeout", type=int, default=300)
ap.add_argument("--out", default=str(ROOT / "profiles" / "connect_bench.jsonl"))
a = ap.parse_args()

if a.step is None:
    _bench.run_cases("bench_connect", a.cases,
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
    table = env.table(stream)
    scene = rt.Scene(rt.reference_world())
    rays = rt.camera_rays(rt.reference_camera(), rt.Frame.full(a.width, a.height, 0))
    hits = rt.cast_rays(scene, rays)
    N, spp = rays.shape[0], a.spp
    ids = torch.arange(N, dtype=torch.int32, device="cuda")
    view = (-rays[:, 3:6].view(torch.float32)).contiguous()
    n_hits = int(rt.Hits(hits).hit.sum().item())

    paths, radiance = P.begin(N, 1, ids)
    paths.view(torch.float32)[:, 3] = 0.5  # a density in every record: weigh_escape weighs every miss
    shadow_rays = torch.empty((N, 11), dtype=torch.int32, device="cuda")
    asks, pending = torch.zeros((N,), dtype=torch.uint8, device="cuda"), torch.zeros((N, 3), dtype=torch.float32, device="cuda")
    asked = torch.zeros((N,), dtype=torch.uint8, device="cuda")
    emitted = torch.ones((N, 3), dtype=torch.float32, device="cuda")
    lw = L.workspace(N, "cuda", 1)
    weight = torch.empty((N,), dtype=torch.float32, device="cuda")

    def put_back():
        asks.copy_(asked)

    def fused():
        P.connect(scene, env, paths, hits, rays, None, None, 1, P.SHADING, P.BALANCE, False, table, shadow_rays, asks, pending, stream=stream)

    def unfused():
        E.rays(scene, env, hits, 1, E.UNIFORM, 1, ids, E.SHADING, table, lw.rays[:N], lw.asks[:N], lw.dirs[:N], lw.radiance[:N], lw.texel[:N], stream=stream)
        materials.material_hits(scene, hits, lw.surfaces[:N], stream=stream)
        materials.probe_surfaces(lw.surfaces[:N], view, lw.dirs[:N].view(1, N, 3), lw.diffuse[:N].view(1, N, 3), lw.specular[:N].view(1, N, 3), stream=stream)
        L.environment_pdf(env, lw.dirs[:N], table, lw.pdf[:N], lw.texel[:N], stream=stream)
        L.pdf(lw.surfaces[:N], view, lw.dirs[:N].view(1, N, 3), L.SHADING, lw.pdf_other[:N], stream=stream)
        L.mis_weigh(lw.pdf[:N], 1, lw.pdf_other[:N], 1, L.BALANCE, False, weight, lw.radiance[:N], stream=stream)

    fused()
    asked.copy_(asks)
    m = spp * N
    rgb = torch.zeros((N, 3), dtype=torch.float32, device="cuda")
    w = P.workspace(N, "cuda", spp, nee=True)
    calls = {
        "connect": fused,
        "unfused": unfused,
        "settle": lambda: P.settle(paths, asks, pending, radiance, None, stream=stream),
        "weigh_escape": lambda: P.weigh_escape(env, paths, hits, rays, emitted, None, None, P.BALANCE, table, stream=stream),
        "trace_paths": lambda: P.trace_paths(scene, hits, rays, spp, a.bounces, env, 3, 0.05, 1, ids, rgb, False, stream, w),
        "trace_paths_nee": lambda: P.trace_paths(scene, hits, rays, spp, a.bounces, env, 3, 0.05, 1, ids, rgb, False, stream, w, nee=True),
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
    stream.synchronize()

    def with_floor(name, bytes_per_path):
        r = _bench.summary(ms[name], rate=("mpaths_s", N))
        r["bytes"] = int(bytes_per_path * N)
        r["floor_ms"] = round(r["bytes"] / (a.hbm_gbs * 1e9) * 1e3, 4)
        r["of_floor"] = round(r["floor_ms"] / r["ms_median"], 3)
        return r

    # per path — connect: the record (32), a hit (52) and the incoming direction (12) read, the shadow ray (44), the ask (1) and the
    # pending radiance (12) written; settle: the ask read and written (2), the pending radiance read (12), the radiance read and written
    # (24) — and the shadow hit's kind (4) where one is given; weigh_escape: the record (32) and the hit's kind (4) read, and for a miss
    # the incoming direction (12) read and the emitted light read and written (24)
    res = {"records": N, "hits": n_hits, "spp": spp, "bounces": a.bounces, "asks_of_bounce_0": int(asked.sum().item()),
           "connect": with_floor("connect", 153),
           "unfused": _bench.summary(ms["unfused"], rate=("mpaths_s", N)),
           "fused_over_unfused": round(float(np.median(ms["unfused"]) / np.median(ms["connect"])), 3),
           "settle": with_floor("settle", 38),
           "weigh_escape": with_floor("weigh_escape", 72),
           "trace_paths": _bench.summary(ms["trace_paths"], rate=("mpaths_s", m)),
           "trace_paths_nee": _bench.summary(ms["trace_paths_nee"], rate=("mpaths_s", m)),
           "nee_over_plain": round(float(np.median(ms["trace_paths_nee"]) / np.median(ms["trace_paths"])), 3)}
res["device"] = torch.cuda.get_device_name(0)
print(json.dumps(res))
