"""Shared support of the path tests: what include/rt_amd.h states about the path queries — the seed of a bounce, the stream of the
roulette, the layout of rt_path.bounce — read from the header itself, the step restated from the calls it fuses (the CPU forms of the
lobe and environment queries and the oracle's Phong terms), and the roulette and the resolve restated in numpy f32.  No fixtures, no
marks, no GPU."""
import re
from pathlib import Path

import numpy as np

import _lobe_support as S
import _material_support
from homework_18_graphics_raytracer_amd import environment as E, lobes as L, paths as P

F32 = np.float32
HEADER = (Path(__file__).resolve().parent.parent / "include" / "rt_amd.h").read_text()
BLOCK = HEADER[HEADER.index("---- path queries:"):HEADER.index("---- texture queries:")]


def _stated(pattern):
    found = re.search(pattern, BLOCK, flags=re.S)
    assert found, pattern
    return found


# the header says which of the issue's two forms it chose: the hash's sample argument carries s, the seed the bounce alone
BOUNCE_STEP = int(_stated(r"seed_b = seed \+ (0x[0-9a-f]+)u \* b").group(1), 16)
ROULETTE_STREAM = int(_stated(r"u_3 = film_u\(id, film_mix\(seed_h \^\s*(0x[0-9a-f]+)u\), s, 0\)").group(1), 16)
_stated(r"the hash's argument carries s, so the seed carries the bounce")
_stated(r"bits 24-31: the sample index s")
assert ROULETTE_STREAM != int(S.SELECT) and BOUNCE_STEP == 0x9E3779B9


def seed_of(seed, bounce):
    """the seed the header states for a bounce: a u32 wrap"""
    return (int(seed) + BOUNCE_STEP * int(bounce)) & 0xFFFFFFFF


def records(n, spp=1, ids=None, beta=1.0, bounce=0, flags=P.ALIVE):
    """begin_numpy's records with another throughput, bounce count or flags"""
    paths, _ = P.begin_numpy(n, spp, ids)
    paths["beta"] = np.asarray(beta, dtype=F32)
    paths["bounce"] += np.uint32(bounce)
    paths["flags"] = flags
    return paths


def u3(ids, seed, bounce, s):
    """the roulette's uniform of the header"""
    seed_h = S.film_mix(np.uint32(seed_of(seed, bounce)) ^ np.uint32(0x85EBCA6B))
    return S.film_u(ids, S.film_mix(seed_h ^ np.uint32(ROULETTE_STREAM)), s, 0)


def composed_step(surfaces, view, paths, seed, normals=None):
    """One advance without roulette and without `last`, from the calls it replaces, per path (sample 0 of each record): lobes.rays_numpy
    (spp 1, UNIFORM, the bounce's seed) -> the oracle's get_diffuse / get_specular (rt_probe_surfaces' terms) -> mis_weigh_numpy
    (divide_by_own, no other strategy, on beta) -> environment.fold_numpy (spp 1, into zeros).  Every record of ``paths`` has the same
    bounce count.  Returns (dirs, pdf, lobe, asks, beta', moved): ``moved``: the fold wrote the record."""
    surfaces = np.asarray(surfaces).view(L.SURFACE_DTYPE).reshape(-1)
    n = surfaces.shape[0]
    bounce = int(paths["bounce"][0]) & 0xFFFFFF
    assert ((paths["bounce"] & 0xFFFFFF) == bounce).all() and (paths["bounce"] >> 24 == 0).all()
    with np.errstate(all="ignore"):
        dirs, pdf, lobe, asks = L.rays_numpy(surfaces, view, 1, L.UNIFORM, seed_of(seed, bounce), paths["id"], normals)
        diffuse, specular = _material_support.expected_probe(surfaces, view, dirs)
        _, t = L.mis_weigh_numpy(pdf.reshape(-1), 1, None, 0, L.BALANCE, True, rgb=paths["beta"])
        opened, beta = E.fold_numpy(surfaces["valid"] != 0, surfaces["shiness"], asks.reshape(-1), 1, t, diffuse.reshape(-1, 3), specular.reshape(-1, 3),
                                    np.zeros((n, 3), dtype=F32))
    return dirs[0], pdf[0], lobe[0], asks[0], beta, opened != 0


def positive(beta):
    """some channel is > 0 (NaN is not)"""
    with np.errstate(invalid="ignore"):
        return (np.asarray(beta) > 0).any(axis=-1)


def restated_roulette(beta, rr_floor, u):
    """(survives, beta / q) of the header: q = the largest channel with NaN passed over, raised to rr_floor, cut at 1"""
    beta = np.asarray(beta, dtype=F32)
    q = np.zeros(beta.shape[:-1], dtype=F32)
    with np.errstate(invalid="ignore"):
        for c in range(3):
            q = np.where(beta[..., c] > q, beta[..., c], q)
        q = np.where(q < F32(rr_floor), F32(rr_floor), q)
        q = np.where(q > F32(1), F32(1), q).astype(F32)
        return u < q, (beta / q[..., None]).astype(F32)


def restated_resolve(radiance, n, spp, rgb, root=None):
    """the header's association: the first sample as it is, each later one added, / (float)spp, added to the slot"""
    radiance = np.asarray(radiance, dtype=F32).reshape(spp, n, 3)
    acc = radiance[0].copy()
    for s in range(1, spp):
        acc = (acc + radiance[s]).astype(F32)
    mean = (acc / F32(spp)).astype(F32)
    out = np.asarray(rgb, dtype=F32).copy()
    slots = np.arange(n) if root is None else np.asarray(root).astype(np.int64)
    out[slots] = (out[slots] + mean).astype(F32)
    return out


def no_negative_zero(a):
    """-0 as +0: the composed step's fold adds to +0, and the comparison may not depend on that"""
    a = np.asarray(a, dtype=F32).copy()
    a[a == 0] = 0
    return a
