#!/usr/bin/env python3
"""Timing of the texture queries (include/rt_amd.h rt_texture_pyramid / rt_texture_footprint / rt_texture_sample / rt_texture_surfaces /
rt_light_terms_surfaces; Python rt.textures) — a large pyramid, and the lookups on the primary hits of the reference scene.

    python tools/bench_textures.py [--steps 9 --warmup 3] [--out profiles/textures_bench.jsonl]

The case runs in a child process of its own under its own `timeout -k 10 <--step-timeout>`; if it fails or runs out of time the run
ends, and nothing more is started on the device.
    pyramid                       rt_texture_pyramid of a --size x --size texture (4096): every level from level 0
    footprint                     rt_texture_footprint on the 1920 x 1080 primary hits
    sample_{nearest,bilinear,trilinear}
                                  rt_texture_sample of a --tex x --tex texture (1024), uv read inside the hit records, into a compact plane
    surfaces_{nearest,bilinear,trilinear}
                                  rt_texture_surfaces, a colour texture and a normal map of that size and filter, on every object
    material_hits                 rt_material_hits on the same hits, for scale
    shade_hits_textured / shade_hits_by_light
                                  the sequence with one binding, and the plain one
Milliseconds are medians of device events, the forms alternated call by call.  Beside each call's time stands `floor_ms`: the bytes
the call must move (stated per case below and in DESIGN.md 3.34) at --hbm-gbs, and `of_floor` = floor_ms / ms_median.  No figure is a
gate.  Appends one JSON line with the commit to --out and prints it.
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
ap.add_argument("--size", type=int, default=4096, help="the side of the pyramid's texture")
ap.add_argument("--tex", type=int, default=1024, help="the side of the sampled textures")
ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="the bandwidth the floors are computed at, GB/s")
ap.add_argument("--cases", nargs="+", choices=STEPS, default=list(STEPS))
ap.add_argument("--step", choices=STEPS, help="run this case in this process and print its JSON")
ap.add_argument("--step-timeout", type=int, default=300)
ap.add_argument("--out", default=str(ROOT / "profiles" / "textures_bench.jsonl"))
a = ap.parse_args()

if a.step is None:
    _bench.run_cases("bench_textures", a.cases, lambda case: ["--step", case] + _bench.options(a, "steps", "warmup", "width", "height", "size", "tex", "hbm_gbs"),
                     a.step_timeout, a.out, header={"steps": a.steps, "warmup": a.warmup, "size": a.size, "tex": a.tex, "hbm_gbs": a.hbm_gbs})
    sys.exit(0)

import torch

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import materials, textures as T

torch.cuda.set_device(0)


def with_floor(values, moved_bytes, rate=None):
    r = _bench.summary(values, rate=rate)
    r["bytes"] = int(moved_bytes)
    r["floor_ms"] = round(moved_bytes / (a.hbm_gbs * 1e9) * 1e3, 4)
    r["of_floor"] = round(r["floor_ms"] / r["ms_median"], 3)
    return r


FILTERS = (("nearest", T.NEAREST), ("bilinear", T.BILINEAR), ("trilinear", T.TRILINEAR))
stream = torch.cuda.Stream()
with torch.cuda.stream(stream):
    gen = torch.Generator(device="cuda").manual_seed(1)
    big = T.Texture(torch.rand((a.size, a.size, 3), generator=gen, device="cuda"), stream=stream)
    colour = {name: T.Texture(torch.rand((a.tex, a.tex, 3), generator=gen, device="cuda"), filter=f, scale=(8.0, 8.0), stream=stream) for name, f in FILTERS}
    bump = {name: T.Texture(torch.rand((a.tex, a.tex, 3), generator=gen, device="cuda") + 0.5, filter=f, scale=(8.0, 8.0), stream=stream) for name, f in FILTERS}
    scene = rt.Scene(rt.reference_world())
    rays = rt.camera_rays(rt.reference_camera(), rt.Frame.full(a.width, a.height, 0))
    hits = rt.cast_rays(scene, rays)
    N = rays.shape[0]
    n_hits = int(rt.Hits(hits).hit.sum().item())
    uv = hits.view(torch.float32)[:, 9:11]
    cone = T.footprint(scene, hits, rays, 2.0 / a.height, stream=stream)  # about a pixel's width per unit of distance
    out = torch.zeros((N, 3), dtype=torch.float32, device="cuda")
    rgb = torch.zeros((N, 3), dtype=torch.float32, device="cuda")
    surfaces = materials.material_hits(scene, hits, stream=stream)
    ws = T.workspace(scene, N, "cuda")
    binding = [T.Binding(colour["trilinear"], bump["trilinear"], T.ALL_OBJECTS, T.MODULATE | T.NORMALIZE)]
    calls = {"pyramid": lambda: T.pyramid(big, stream=stream),
             "footprint": lambda: T.footprint(scene, hits, rays, 2.0 / a.height, None, cone, stream=stream),
             "material_hits": lambda: materials.material_hits(scene, hits, surfaces, stream=stream),
             "shade_hits_textured": lambda: T.shade_hits_textured(scene, hits, rays, binding, 2.0 / a.height, out=rgb, stream=stream, workspace=ws),
             "shade_hits_by_light": lambda: rt.shade_hits_by_light(scene, hits, rays, out=rgb, stream=stream, workspace=ws.light)}
    for name, _ in FILTERS:
        calls["sample_" + name] = lambda name=name: T.sample(colour[name], uv, cone, out, stream=stream)
        calls["surfaces_" + name] = lambda name=name: T.apply(surfaces, hits, colour[name], bump[name], cone, T.ALL_OBJECTS, T.MODULATE | T.NORMALIZE,
                                                              stream=stream)
    ms = _bench.alternate(calls, a.warmup, a.steps)
    texels = a.size * a.size
    # every level but the last is read once and every level but the first written once, 12 B a texel: 12 * (4/3 + 1/3) * size^2
    built = 12 * (texels * 4 // 3 + texels // 3)
    # per record: a hit (52) and a ray's origin and direction (24) read, a float written; the primitive's vertices are cached at best
    coned = 80 * N
    # per record: a uv (8) and a footprint (4) read, a colour (12) written; the texels — 1 to 8 of them a record — are cached at best
    looked = 24 * N
    # per record: a hit's object, normal and uv (24), a footprint (4) and the 10 words that move read (40), 9 words written (36)
    edited = 104 * N
    res = {"records": N, "hits": n_hits, "size": a.size, "tex": a.tex, "levels": big.n_levels,
           "pyramid": with_floor(ms["pyramid"], built, ("mtexels_s", texels)),
           "footprint": with_floor(ms["footprint"], coned, ("mrecords_s", N)),
           "material_hits": with_floor(ms["material_hits"], (52 + 72) * N, ("mrecords_s", N)),
           "shade_hits_textured": _bench.summary(ms["shade_hits_textured"], rate=("mrecords_s", N)),
           "shade_hits_by_light": _bench.summary(ms["shade_hits_by_light"], rate=("mrecords_s", N))}
    for name, _ in FILTERS:
        res["sample_" + name] = with_floor(ms["sample_" + name], looked, ("mrecords_s", N))
        res["surfaces_" + name] = with_floor(ms["surfaces_" + name], edited, ("mrecords_s", N))
res["device"] = torch.cuda.get_device_name(0)
print(json.dumps(res))
