"""Shared support of the transmission tests: what include/rt_amd.h states about the transmission queries — the stream of the choice,
the flags — read from the header itself; the choice and the entry of the walk restated from the counter hash and the oracle's
orc_refract_dir, as the refraction tests restate them; and a crafted batch that holds every case of the choice.  No fixtures, no marks,
no GPU."""
import ctypes as C
import re
from pathlib import Path

import numpy as np

import _lobe_support as S
import _oracle
import _path_support as PS
from homework_18_graphics_raytracer_amd import paths as P
from homework_18_graphics_raytracer_amd._queries import HIT_DTYPE, RAY_DTYPE

F32 = np.float32
NONE = 0xFFFFFFFF
ESCAPED, INFINITE, TRAPPED_WALK, WALKING = 0, 1, 2, 3
FRONT, BACK = 0, 1
HEADER = (Path(__file__).resolve().parent.parent / "include" / "rt_amd.h").read_text()
BLOCK = HEADER[HEADER.index("---- transmission queries:"):HEADER.index("---- distributed (stochastic")]
TRANSMIT_STREAM = int(re.search(r"u_4 = film_u\(id, film_mix\(seed_h \^ (0x[0-9a-f]+)u\), s, 0\)", BLOCK).group(1), 16)
assert TRANSMIT_STREAM == 0x85EBCA6B


def u4(ids, seed, bounce, s):
    """the choice's uniform of the header"""
    seed_h = S.film_mix(np.uint32(PS.seed_of(seed, bounce)) ^ np.uint32(0x85EBCA6B))
    return S.film_u(ids, S.film_mix(seed_h ^ np.uint32(TRANSMIT_STREAM)), s, 0)


def normalize32(v):
    """cgmath's normalize in f32: v * (1 / magnitude), the dot product summed left to right"""
    v = np.asarray(v, dtype=F32)
    with np.errstate(all="ignore"):
        return v * (F32(1.0) / np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]))


def restated_entry(hits, incoming, index, rows):
    """rt_refract_enter's (rays, kind, flags) for the records ``rows``, from the oracle's orc_refract_dir (main.rs:354-368); every other
    record holds the finished walk"""
    hits, incoming = np.asarray(hits).view(HIT_DTYPE).reshape(-1), np.asarray(incoming).view(RAY_DTYPE).reshape(-1)
    n = hits.shape[0]
    rays, kind, flags = np.zeros((n, 11), dtype=np.uint32), np.full(n, NONE, dtype=np.uint32), np.zeros(n, dtype=np.uint8)
    lib, v = _oracle.lib(), (C.c_float * 3)()
    for i in rows:
        normal, direction = (C.c_float * 3)(*hits["normal"][i]), (C.c_float * 3)(*incoming["direction"][i])
        if lib.orc_refract_dir(normal, direction, float(index[i]), v):
            kind[i], flags[i] = WALKING, 1
            rays[i, 0:3] = hits["position"][i].view(np.uint32)
            rays[i, 3:6] = normalize32(v[:]).view(np.uint32)
            rays[i, 6:] = (BACK, 1, hits["kind"][i], hits["index"][i], FRONT)  # ray_inside
        else:
            kind[i] = TRAPPED_WALK
    return rays, kind, flags


def unit(v):
    v = np.asarray(v, dtype=np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(F32)


def crafted(n, seed):
    """(surfaces, hits, incoming): n vertices with normals all over the sphere, rays from nearly along the normal to grazing, every
    transparency the header speaks of in the first records — 0, 1, 2, NaN, 0.3 — and materials denser and thinner than their
    surroundings, so that some rays cannot enter (refract is None); records 7 and 40 are no hit"""
    rng = np.random.default_rng(seed)
    normal = unit(rng.normal(size=(n, 3)))
    s = S.flat_surfaces(n, normal, rng.random(n).astype(F32), F32(0.5))
    s["transparency"] = rng.random(n).astype(F32)
    s["transparency"][:5] = np.array([0.0, 1.0, 2.0, np.nan, 0.3], dtype=F32)
    s["refraction_index"] = np.where(rng.random(n) < 0.5, F32(1.5), F32(0.6))
    s["opaque_decay"] = rng.uniform(0.2, 0.99, n).astype(F32)
    s["valid"][[7, 40]] = 0
    hits = np.zeros(n, dtype=HIT_DTYPE)
    hits["kind"], hits["index"], hits["object_index"] = rng.integers(0, 2, n), rng.integers(0, 1000, n), rng.integers(0, 5, n)
    hits["position"], hits["normal"] = (rng.normal(size=(n, 3)) * 10).astype(F32), normal
    hits["kind"][[7, 40]] = NONE
    incoming = np.zeros(n, dtype=RAY_DTYPE)
    tangent = unit(np.cross(normal, rng.normal(size=(n, 3))))
    tilt = np.radians(rng.uniform(0.0, 89.0, n))[:, None]
    incoming["direction"] = unit(-np.cos(tilt) * normal + np.sin(tilt) * tangent)
    incoming["origin"] = hits["position"] - incoming["direction"] * F32(3.0)
    return s, hits, incoming
