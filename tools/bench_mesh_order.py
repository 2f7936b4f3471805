#!/usr/bin/env python3
"""What ordering a mesh on the device is worth (include/rt_amd.h "mesh ordering"): the flat sweep mesh (tools/scene_sweep.py: the
literal scene around the dodecahedron subdivided k times) in three orders of its triangles, measured in one run.

    timeout -k 10 900 python tools/bench_mesh_order.py [--levels 4 5] [--steps 7 --warmup 2] [--out profiles/mesh_order_bench.jsonl]

Orders: natural (the subdivision emits siblings together), shuffled (the mesh's triangles in a random permutation, fixed seed — an
exporter's order; the baseline: what the library did with such a mesh before), ordered (the shuffled description through
rt_order_triangles).  Per size, alternated call by call over the three scenes and timed with device events after the warm-up, medians
of --steps calls with their spread (max - min):
    cast      rt.cast_rays on --rays random rays (the same rays for the three; triangle exclusions are not used)
    whitted   rt.render_whitted of a 480 x 270 depth-5 frame
    order     rt.order_triangles itself on the shuffled description (keys, two sorts, gather), buffers made once
The ordered scene's casts are checked against the shuffled scene's through the permutation (equal, or the same distance: a tie).  There
is no gate: the lines say what was measured.  The script ends itself after --time-limit seconds.  Prints one JSON line per size and
appends them to --out when given."""
import argparse
import ctypes as C
import json
import signal
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import _bench
import numpy as np
import torch

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import _capi

ap = argparse.ArgumentParser()
ap.add_argument("--levels", type=int, nargs="+", default=[4, 5], help="subdivision levels: 36 * 4^k + 28 triangles (4: 9 244, 5: 36 892)")
ap.add_argument("--steps", type=int, default=7, help="timed calls per case")
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--rays", type=int, default=1_000_000)
ap.add_argument("--width", type=int, default=480)
ap.add_argument("--height", type=int, default=270)
ap.add_argument("--depth", type=int, default=5)
ap.add_argument("--seed", type=int, default=2024)
ap.add_argument("--time-limit", type=int, default=840, help="seconds after which the script ends itself")
ap.add_argument("--out", default=None, help="a .jsonl file the result lines are appended to")
a = ap.parse_args()

signal.alarm(a.time_limit)
torch.cuda.set_device(0)


def raw_of(desc):
    return np.frombuffer(C.string_at(desc.triangles, desc.n_triangles * C.sizeof(_capi.Triangle)), dtype=np.uint32).reshape(-1, 25).copy()


def desc_with(desc, raw):
    tris = (_capi.Triangle * raw.shape[0]).from_buffer_copy(np.ascontiguousarray(raw, dtype=np.uint32).tobytes())
    out = _capi.SceneDesc(tris, raw.shape[0], desc.spheres, desc.n_spheres, desc.materials, desc.n_materials, desc.lights, desc.n_lights)
    out._keepalive = (tris, desc)
    return out


def alternated(cases, steps, warmup):
    ms = _bench.alternate(cases, warmup, steps)
    return ({k: round(float(np.median(v)), 4) for k, v in ms.items()}, {k: round(float(max(v) - min(v)), 4) for k, v in ms.items()})


def measure(level):
    with tempfile.TemporaryDirectory() as tmp:
        world = _bench.tessellated_world(tmp, level, False)
    base = world.desc()
    lo, hi = world.bounds()
    natural = raw_of(base)
    n = natural.shape[0]
    mesh = np.flatnonzero(natural[:, 0] == int(np.argmax(np.bincount(natural[:, 0]))))
    shuffled = natural.copy()
    shuffled[mesh] = natural[mesh[np.random.default_rng(a.seed).permutation(mesh.size)]]
    shuffled_t = torch.from_numpy(shuffled.view(np.int32)).cuda()
    perm_t = torch.empty((n,), dtype=torch.int32, device="cuda")
    ordered_t = torch.empty((n, 25), dtype=torch.int32, device="cuda")
    temp = torch.empty((rt.order_triangles_temp_bytes(n),), dtype=torch.uint8, device="cuda")
    order = lambda: rt.order_triangles(shuffled_t, lo, hi, base.n_materials, out=perm_t, ordered=ordered_t, temp=temp)
    order()
    torch.cuda.synchronize()
    perm = perm_t.cpu().numpy().view(np.uint32)
    ordered = ordered_t.cpu().numpy().view(np.uint32)
    descs = {"natural": base, "shuffled": desc_with(base, shuffled), "ordered": desc_with(base, ordered)}
    scenes = {k: rt.Scene(d) for k, d in descs.items()}
    p = natural[:, 1:].copy().view(np.float32).reshape(n, 3, 8)[:, :, :3].reshape(-1, 3).astype(np.float64)
    centre = (p.min(0) + p.max(0)) / 2
    rays = _bench.random_rays(a.seed + level, a.rays, centre, float(np.linalg.norm(p - centre, axis=1).max()))
    camera, frame = rt.reference_camera(), rt.Frame.full(a.width, a.height, a.depth)
    hits = {k: torch.empty((a.rays, 13), dtype=torch.int32, device="cuda") for k in scenes}
    image = {k: torch.empty((frame.rows, frame.cols, 3), dtype=torch.float32, device="cuda") for k in scenes}
    cast_ms, cast_spread = alternated({k: (lambda k=k: rt.cast_rays(scenes[k], rays, out=hits[k])) for k in scenes}, a.steps, a.warmup)
    frame_ms, frame_spread = alternated({k: (lambda k=k: rt.render_whitted(scenes[k], camera, frame, out=image[k])) for k in scenes}, a.steps, a.warmup)
    order_ms, order_spread = alternated({"order": order}, a.steps, a.warmup)
    # the ordered scene against the shuffled one, through the permutation: equal, or a tie of equal distance
    back = rt.unorder_hits(hits["ordered"].cpu().numpy().view(np.uint32), perm).view(np.uint32).reshape(-1, 13)
    want = hits["shuffled"].cpu().numpy().view(np.uint32)
    differ = np.flatnonzero((back != want).any(axis=1))
    ties_only = bool(((back[differ, 12] == want[differ, 12]) & (back[differ, 0] != 0xFFFFFFFF) & (want[differ, 0] != 0xFFFFFFFF)).all())
    line = {"tool": "bench_mesh_order", "device": torch.cuda.get_device_name(0), "level": level, "triangles": n, "rays": a.rays,
            "frame": [a.width, a.height, a.depth], "steps": a.steps,
            "cast_ms_median": cast_ms, "cast_ms_spread": cast_spread, "whitted_ms_median": frame_ms, "whitted_ms_spread": frame_spread,
            "order_ms_median": order_ms["order"], "order_ms_spread": order_spread["order"],
            "cast_shuffled_over_ordered": round(cast_ms["shuffled"] / cast_ms["ordered"], 3),
            "cast_ordered_over_natural": round(cast_ms["ordered"] / cast_ms["natural"], 3),
            "whitted_shuffled_over_ordered": round(frame_ms["shuffled"] / frame_ms["ordered"], 3),
            "whitted_ordered_over_natural": round(frame_ms["ordered"] / frame_ms["natural"], 3),
            "records_that_differ": int(differ.size), "ties_only": ties_only}
    print(json.dumps(line), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(json.dumps(line) + "\n")


for level in a.levels:
    measure(level)
