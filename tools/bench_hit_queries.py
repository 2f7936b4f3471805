#!/usr/bin/env python3
"""Timing of the hit queries (include/rt_amd.h rt_shade_hits / rt_reflect_rays / rt_refract_rays): get_shade, get_reflect and
get_refract on the hits of caller-supplied rays.

    timeout -k 10 600 python tools/bench_hit_queries.py [--steps 7 --warmup 2] [--out profiles/hit_query_bench.jsonl]

On the reference scene, three batches of rays — the 1920 x 1080 frame's camera rays in row order (a wave's 64 rays: a 64x1 strip), the
same rays in the Whitted kernels' 8x8-tile order, and 2 M seeded random rays from within twice the bounding radius — and for each,
alternated call by call in this process and timed with device events after the warm-up (medians):
    cast            rt_cast_rays
    shade_pairs     rt_shade_hits with the pair-wise shadow cast (the default)
    shade_uniform   rt_shade_hits under RT_AMD_QUERY_WAVE_UNIFORM=1
    refract_pairs / refract_uniform   rt_refract_rays likewise
    reflect         rt_reflect_rays
    trace0          rt_trace_rays at depth 0 on the same rays: the yardstick — the only thing the library offered for "direct light at
                    the hit" before, which casts the ray again and shades non-glass hits
The two shade variants are checked against each other bit for bit, and shade against trace0 where trace0 is not black by rule.
Appends one JSON line to --out and prints it.  Kernel times: run it under rocprofv3 --kernel-trace --stats.
"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import _bench
import numpy as np
import torch

import homework_18_graphics_raytracer_amd as rt

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=7, help="timed calls per case")
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--random-rays", type=int, default=2_000_000)
ap.add_argument("--seed", type=int, default=2024)
ap.add_argument("--out", default=str(ROOT / "profiles" / "hit_query_bench.jsonl"))
a = ap.parse_args()

torch.cuda.set_device(0)


count = torch.zeros(1, dtype=torch.int64, device="cuda")


def casts_of(fn):
    count.zero_()
    fn(count)
    torch.cuda.synchronize()
    return int(count.item())


def uniform(fn):
    def run(*args):
        with rt.options(RT_AMD_QUERY_WAVE_UNIFORM=1):
            return fn(*args)
    return run


def bench(scene, rays):
    n = rays.shape[0]
    hits = rt.cast_rays(scene, rays)
    rgb = {k: torch.empty((n, 3), dtype=torch.float32, device="cuda") for k in ("pairs", "uniform", "trace0")}
    refl = torch.empty((n, 11), dtype=torch.int32, device="cuda")
    shade = lambda k, c=None: rt.shade_hits(scene, hits, rays, out=rgb[k], ray_count=c)
    refract = lambda c=None: rt.refract_rays(scene, hits, rays, ray_count=c)
    cases = {
        "cast": lambda: rt.cast_rays(scene, rays, out=hits),
        "shade_pairs": lambda: shade("pairs"),
        "shade_uniform": uniform(lambda: shade("uniform")),
        "refract_pairs": refract,
        "refract_uniform": uniform(refract),
        "reflect": lambda: rt.reflect_rays(hits, rays, out=refl),
        "trace0": lambda: rt.trace_rays(scene, rays, 0, out=rgb["trace0"]),
    }
    ms = _bench.alternate(cases, a.warmup, a.steps)
    casts = {"cast": n, "shade_pairs": casts_of(lambda c: shade("pairs", c)), "shade_uniform": casts_of(uniform(lambda c: shade("uniform", c))),
             "refract_pairs": casts_of(refract), "refract_uniform": casts_of(uniform(refract)), "reflect": 0,
             "trace0": casts_of(lambda c: rt.trace_rays(scene, rays, 0, out=rgb["trace0"], ray_count=c))}
    r = {"records": n, "hits": int(rt.Hits(hits).hit.sum().item())}
    for k, v in ms.items():
        med = float(np.median(v))
        r[k] = {"ms_median": round(med, 4), "ms_min": round(min(v), 4), "casts": casts[k], "mcasts_per_s": round(casts[k] / med / 1e3, 1)}
    # the headline is the DEFAULT's (pair-wise shadow casts); the wave-uniform variant's figures stand beside it
    for tag, key in (("", "shade_pairs"), ("_uniform", "shade_uniform")):
        both = r["cast"]["ms_median"] + r[key]["ms_median"]
        r["cast_plus_shade" + tag + "_ms"] = round(both, 4)
        r["cast_plus_shade" + tag + "_mcasts_per_s"] = round((n + casts[key]) / both / 1e3, 1)
        r["cast_plus_shade" + tag + "_over_trace0"] = round(both / r["trace0"]["ms_median"], 4)
        r["shade" + tag + "_over_trace0"] = round(r[key]["ms_median"] / r["trace0"]["ms_median"], 4)
    r["shade_winner"] = "pairs" if r["shade_pairs"]["ms_median"] <= r["shade_uniform"]["ms_median"] else "uniform"
    r["refract_winner"] = "pairs" if r["refract_pairs"]["ms_median"] <= r["refract_uniform"]["ms_median"] else "uniform"
    r["shade_variants_identical"] = _bench.same(rgb["pairs"], rgb["uniform"]) and casts["shade_pairs"] == casts["shade_uniform"]
    # trace0 is black by rule on glass (shade contribution below THRESHOLD) and on misses; elsewhere it is get_shade of the same hit
    lit = (rgb["trace0"].view(torch.int32) != 0).any(dim=1)
    r["shade_equals_trace0_where_lit"] = _bench.same(rgb["pairs"][lit], rgb["trace0"][lit])
    return r


result = {"tool": "bench_hit_queries", "device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup}
world = rt.reference_world()
scene = rt.Scene(world)
W, H = 1920, 1080
rows = rt.camera_rays(rt.reference_camera(), rt.Frame.full(W, H, 0))
result["rows"] = bench(scene, rows)
tiles = rows[torch.from_numpy(_bench.tile_order(W, H)).cuda()].contiguous()
del rows
result["tiles"] = bench(scene, tiles)
del tiles
centre, radius = _bench.bounds(world.desc())
result["random"] = bench(scene, _bench.random_rays(a.seed, a.random_rays, centre, radius))
line = json.dumps(result)
Path(a.out).parent.mkdir(parents=True, exist_ok=True)
with open(a.out, "a") as f:
    f.write(line + "\n")
print(line)
