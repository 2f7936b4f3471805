#!/usr/bin/env python3
"""Timing of the adaptive sampling queries (include/rt_amd.h "adaptive sampling queries"; Python rt.adaptive).

    python tools/bench_adaptive.py [--steps 7 --warmup 2 --launches 10 --width 1920 --height 1080] [--out profiles/adaptive_bench.jsonl]

Three cases, each a child process of its own under its own `timeout -k 10 <--step-timeout>`; if one fails or runs out of time the run ends
there and nothing more is started:
    list     rt_sample_list on counts all 1, all 4 and skewed (5 % of the pixels at 64, the rest 0), each beside its traffic floor: the
             counts read twice (totals, expansion), start written once, pixel and sample written once per listed record, over
             --hbm-tb-per-s
    splat    rt_film_splat_listed, equal counts 4, tent 1.0, beside rt_film_splat at spp 4 on the same samples (an unchanged kernel of
             the parent commit), both kernel forms of each
    pass     one adaptive.render_pass of the skewed counts (3.2 samples per pixel on average, capacity given: no host visit) beside
             film.render_supersampled at spp 3, the nearest uniform count; absolute and per million samples
A timed window is --launches calls back to back between two device events, reported per call; the calls of a group are alternated window
by window.  Per call: the median of --steps windows and their spread (max - min).  No figure is a gate.  Appends one JSON line to --out
and prints it.
"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import _bench

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=7, help="timed windows per call")
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--launches", type=int, default=10, help="back-to-back calls per timed window")
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--hbm-tb-per-s", type=float, default=6.3, help="achievable HBM bandwidth the floors are computed with")
ap.add_argument("--child", choices=["list", "splat", "pass"], help="measure this case in this process and print its JSON")
ap.add_argument("--step-timeout", type=int, default=300)
ap.add_argument("--out", default=str(ROOT / "profiles" / "adaptive_bench.jsonl"))
a = ap.parse_args()

if not a.child:
    from homework_18_graphics_raytracer_amd import _capi

    _bench.run_cases("bench_adaptive", ("list", "splat", "pass"),
                     lambda case: ["--child", case] + _bench.options(a, "steps", "warmup", "launches", "width", "height", "hbm_tb_per_s"),
                     a.step_timeout, a.out, header={"sources_sha256": _capi.sources_sha256()})
    sys.exit(0)

import numpy as np
import torch

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import adaptive, film

torch.cuda.set_device(0)
rows, cols = a.height, a.width
n = rows * cols
stream = torch.cuda.Stream()


def window(call, launches):
    """milliseconds per call of `launches` calls back to back"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        call()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / launches


def alternate(calls, launches=None):
    """{name: call} -> {name: summary}: every call once per round, alternated window by window"""
    launches = launches or a.launches
    ms = {k: [] for k in calls}
    with torch.cuda.stream(stream):
        for k in range(a.warmup + a.steps):
            t = {name: window(f, launches) for name, f in calls.items()}
            if k >= a.warmup:
                for name in ms:
                    ms[name].append(t[name])
    torch.cuda.synchronize()
    return {name: _bench.summary(v, spread=True) for name, v in ms.items()}


def skewed():
    c = np.zeros(n, dtype=np.int32)
    c[np.random.default_rng(1).random(n) < 0.05] = 64
    return c


res = {"device": torch.cuda.get_device_name(0), "rows": rows, "cols": cols, "steps": a.steps, "warmup": a.warmup, "launches_per_window": a.launches,
       "hbm_tb_per_s": a.hbm_tb_per_s}

if a.child == "list":
    patterns = {"ones": np.ones(n, dtype=np.int32), "fours": np.full(n, 4, dtype=np.int32), "skewed": skewed()}
    temp = torch.zeros(adaptive.list_temp_bytes(n), dtype=torch.uint8, device="cuda")
    calls, floors = {}, {}
    for name, c in patterns.items():
        total = int(c.sum())
        d = torch.from_numpy(c).cuda()
        out = adaptive.sample_list(d, total, temp=temp)
        calls[name] = (lambda d=d, total=total, out=out: adaptive.sample_list(d, total, out=out, temp=temp, stream=stream))
        floors[name] = (8 * n + 4 * (n + 1) + 8 * total, total)
    torch.cuda.synchronize()
    timed = alternate(calls)
    for name, (nbytes, total) in floors.items():
        floor_ms = nbytes / (a.hbm_tb_per_s * 1e12) * 1e3
        res[name] = dict(timed[name], records=total, floor_bytes=nbytes, floor_ms=round(floor_ms, 4), over_floor=round(timed[name]["ms_median"] / floor_ms, 2))

elif a.child == "splat":
    spp = 4
    g = torch.Generator(device="cuda").manual_seed(3)
    samples = torch.rand((spp, n, 3), dtype=torch.float32, device="cuda", generator=g)
    offsets = torch.rand((spp, n, 2), dtype=torch.float32, device="cuda", generator=g) - 0.5
    listed_samples, listed_offsets = samples.transpose(0, 1).contiguous().view(n * spp, 3), offsets.transpose(0, 1).contiguous().view(n * spp, 2)
    sl = adaptive.sample_list(torch.full((n,), spp, dtype=torch.int32, device="cuda"), n * spp)
    uniform, ragged = film.Film(rows, cols, "tent", 1.0, device="cuda"), film.Film(rows, cols, "tent", 1.0, device="cuda")
    same = {}
    for form in (0, 1):
        with rt.options(RT_AMD_FILM_SPLAT_FORM=form):
            uniform.sum.zero_(), uniform.weight.zero_(), ragged.sum.zero_(), ragged.weight.zero_()
            uniform.splat(samples, offsets)
            adaptive.splat_listed(ragged, listed_samples, listed_offsets, sl, max_count=spp)
            torch.cuda.synchronize()
            same[form] = _bench.same(uniform.sum, ragged.sum) and _bench.same(uniform.weight, ragged.weight)
            timed = alternate({"film_splat": lambda: uniform.splat(samples, offsets, stream=stream),
                               "film_splat_listed": lambda: adaptive.splat_listed(ragged, listed_samples, listed_offsets, sl, max_count=spp, stream=stream)})
        res[f"form{form}"] = dict(film_splat=timed["film_splat"], film_splat_listed=timed["film_splat_listed"], same_bits=same[form],
                                  listed_over_uniform=round(timed["film_splat_listed"]["ms_median"] / timed["film_splat"]["ms_median"], 3))

else:
    scene, cam, frame = rt.Scene(rt.reference_world()), rt.reference_camera(), rt.Frame.full(cols, rows, 5)
    counts = torch.from_numpy(skewed()).cuda()
    total = int(counts.sum().item())
    f = film.Film(rows, cols, "tent", 1.0, device="cuda")
    timed = alternate({"render_pass_skewed": lambda: adaptive.render_pass(scene, cam, frame, f, counts, capacity=total, stream=stream),
                       "render_supersampled_spp3": lambda: film.render_supersampled(scene, cam, frame, 3, pattern="uniform", stream=stream)}, launches=2)
    res.update(timed)
    res["launches_per_window"] = 2
    res["samples_skewed"], res["samples_spp3"] = total, 3 * n
    res["ms_per_msample_skewed"] = round(timed["render_pass_skewed"]["ms_median"] / (total / 1e6), 4)
    res["ms_per_msample_spp3"] = round(timed["render_supersampled_spp3"]["ms_median"] / (3 * n / 1e6), 4)
print(json.dumps(res))
