#!/usr/bin/env python3
"""Timing of the transmission queries (include/rt_amd.h rt_path_branch / rt_path_transmit; Python rt.paths) on the primary hits of the
reference scene.

    python tools/bench_paths_glass.py [--steps 9 --warmup 3] [--out profiles/paths_glass_bench.jsonl]

The case runs in a child process of its own under its own `timeout -k 10 <--step-timeout>`; if it fails or runs out of time the run
ends, and nothing more is started on the device.  On the 1920 x 1080 primary rays and hits, one path per pixel, ids = the pixel index:
    branch            rt_path_branch, bounce 0, every path alive                                              (Mpaths/s)
    transmit          rt_path_transmit on the walks of that branch after eleven rounds, no roulette: every slot listed
    trace_paths       paths.trace_paths without and with transmission, --spp samples, --bounces bounces, roulette from bounce 3
and, from shorter runs of the loop, the share of the paths alive when bounce b begins that transmit there.  Milliseconds are medians
of device events; the calls change their records, so these are put back (untimed) before every call.  Beside each call's time stands `floor_ms`: the bytes the call must move (stated in DESIGN.md 3.36) at
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
ap.add_argument("--spp", type=int, default=4)
ap.add_argument("--bounces", type=int, default=4)
ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="the bandwidth the floor is computed at, GB/s")
ap.add_argument("--cases", nargs="+", choices=STEPS, default=list(STEPS))
ap.add_argument("--step", choices=STEPS, help="run this case in this process and print its JSON")
ap.add_argument("--step-timeout", type=int, default=300)
ap.add_argument("--out", default=str(ROOT / "profiles" / "paths_glass_bench.jsonl"))
a = ap.parse_args()

if a.step is None:
    _bench.run_cases("bench_paths_glass", a.cases,
                     lambda case: ["--step", case] + _bench.options(a, "steps", "warmup", "width", "height", "spp", "bounces", "hbm_gbs"),
                     a.step_timeout, a.out, header={"steps": a.steps, "warmup": a.warmup, "spp": a.spp, "bounces": a.bounces, "hbm_gbs": a.hbm_gbs})
    sys.exit(0)

import numpy as np
import torch

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import paths as P

torch.cuda.set_device(0)
stream = torch.cuda.Stream()
with torch.cuda.stream(stream):
    scene = rt.Scene(rt.reference_world())
    rays = rt.camera_rays(rt.reference_camera(), rt.Frame.full(a.width, a.height, 0))
    hits = rt.cast_rays(scene, rays)
    N, spp = rays.shape[0], a.spp
    m = spp * N
    ids = torch.arange(N, dtype=torch.int32, device="cuda")
    n_hits = int(rt.Hits(hits).hit.sum().item())

    # one path per pixel: the branch of bounce 0, its walks run to their end, and the fold
    fresh, _ = P.begin(N, 1, ids)
    paths, vertices = fresh.clone(), hits.clone()
    state = P.branch(scene, paths, vertices, rays, seed=1, stream=stream)
    lobe, through, walk_rays, kind, travel, casts, walk_flags = state
    inside = torch.zeros((N, 13), dtype=torch.int32, device="cuda")
    escape = torch.zeros((N, 11), dtype=torch.int32, device="cuda")
    for _ in range(11):
        index, count = rt.select_records(walk_flags, stream=stream)
        rt.cast_rays_indexed(scene, walk_rays, index, count, inside, stream=stream)
        rt.refract_step(scene, vertices, inside, walk_rays, kind, travel, casts, walk_flags, 100.0, escape, stream=stream)
    walked_kind = kind.clone()
    next_rays, alive = torch.empty((N, 11), dtype=torch.int32, device="cuda"), torch.empty((N,), dtype=torch.uint8, device="cuda")
    stream.synchronize()
    transmitting = int(through.sum().item())
    escaped = int(((walked_kind == 0) & (through != 0)).sum().item())

    def put_back():
        paths.copy_(fresh)
        vertices.copy_(hits)
        kind.copy_(walked_kind)

    # the timed branch writes a walk state of its own, so that the timed transmit keeps the finished walks
    b_rays, b_kind, b_travel, b_casts, b_flags = walk_rays.clone(), kind.clone(), travel.clone(), casts.clone(), walk_flags.clone()

    def branch():
        P.branch(scene, paths, vertices, rays, None, None, 1, False, lobe, through, b_rays, b_kind, b_travel, b_casts, b_flags, stream=stream)

    def transmit():
        P.transmit(scene, paths, vertices, kind, travel, escape, walk_flags, None, None, 1, P.NO_ROULETTE, 0.05, next_rays, alive, stream=stream)

    rgb = torch.zeros((N, 3), dtype=torch.float32, device="cuda")
    w_plain, w_glass = P.workspace(N, "cuda", spp), P.workspace(N, "cuda", spp, transmission=True)
    calls = {
        "branch": branch,
        "transmit": transmit,
        "trace_paths": lambda: P.trace_paths(scene, hits, rays, spp, a.bounces, None, 3, 0.05, 1, ids, rgb, False, stream, w_plain),
        "trace_paths_transmission": lambda: P.trace_paths(scene, hits, rays, spp, a.bounces, None, 3, 0.05, 1, ids, rgb, False, stream, w_glass, True),
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

    # The share of the paths alive when bounce b begins that go through the glass there.  Bounce 0: the branch above.  Bounce b > 0: a
    # loop of b bounces without roulette — its last branch runs with `last`, so of the paths that took b bounces the ones it chose end
    # with flags 0 and neither byte, and the others go to advance with their lobe byte set.
    shares = []
    for b in range(a.bounces):
        if b == 0:
            shares.append(round(transmitting / N, 4))
            continue
        P.trace_paths(scene, hits, rays, spp, b, None, P.NO_ROULETTE, 0.05, 1, ids, rgb, False, stream, w_glass, True)
        stream.synchronize()
        taken, flags = (w_glass.paths[:m, 6] & 0xFFFFFF), w_glass.paths[:m, 7]
        began = (taken == b) & ((flags == 0) | (flags == P.ESCAPED))  # the paths the last bounce found alive: `last` or a miss ended them
        through_last = (w_glass.lobe[:m] == 0) & began & (flags == 0)  # of those, the ones branch ended: neither byte, flags 0
        shares.append(round(float(through_last.sum().item()) / max(int(began.sum().item()), 1), 4))

    # per path — branch: the record's second half read (16), a hit (52) and the incoming direction (12) read, two bytes (2), the walk ray
    # (44), kind, travel, casts (12) and the flag (1) written; transmit: the record read and written (64), a hit (52: the object and uv),
    # kind read and written (8), travel (4) and the escape ray (44) read, the next ray (44), the flag and the walk flag (2) written
    def with_floor(name, moved):
        r = _bench.summary(ms[name], rate=("mpaths_s", N))
        r["bytes"] = int(moved)
        r["floor_ms"] = round(moved / (a.hbm_gbs * 1e9) * 1e3, 4)
        r["of_floor"] = round(r["floor_ms"] / r["ms_median"], 3)
        return r

    res = {"records": N, "hits": n_hits, "spp": spp, "bounces": a.bounces, "transmitting_at_bounce_0": transmitting, "escaped_of_those": escaped,
           "branch": with_floor("branch", 139 * N),
           "transmit": with_floor("transmit", 218 * N),
           "trace_paths": _bench.summary(ms["trace_paths"], rate=("mpaths_s", m)),
           "trace_paths_transmission": _bench.summary(ms["trace_paths_transmission"], rate=("mpaths_s", m)),
           "transmission_over_plain": round(float(np.median(ms["trace_paths_transmission"]) / np.median(ms["trace_paths"])), 3),
           "transmit_share_per_bounce": shares}
res["device"] = torch.cuda.get_device_name(0)
print(json.dumps(res))
