"""Lobe queries (include/rt_amd.h "lobe queries"): directions drawn from a surface's own Phong lobes, the density of a direction under
each sampler, and the weights that combine two of them.

hemisphere.rays draws cosine-distributed directions and environment.rays draws by the sky's brightness; neither looks at the specular
lobe.  ``rays`` draws ``spp`` directions per hit from the mixture of the diffuse lobe about the normal and the specular lobe about the
mirrored view — ``shiness`` chooses between them — with the mixture's density of each; ``pdf`` gives that density for directions of the
caller's own, ``environment_pdf`` the density of directions under an environment's table, and ``mis_weigh`` the balance or power weight
of a sample, multiplied into its radiance on the device.  The fold is environment.fold.

    rays / pdf / environment_pdf / mis_weigh       rt_lobe_rays / rt_lobe_pdf / rt_environment_pdf / rt_mis_weigh
    rays_numpy / pdf_numpy / environment_pdf_numpy / mis_weigh_numpy
                                                    the CPU forms (rt_lobe_samples_cpu, rt_lobe_pdf_cpu, rt_environment_pdf_cpu and
                                                    rt_mis_weigh_cpu of librt_host.so): the device's bits
    glossy_hits                                     rays -> trace_rays -> material_hits + probe_surfaces -> mis_weigh(/ pdf) -> fold
    sky_hits_mis                                    environment.rays and rays, each cast, weighed against the other and folded
                                                    — both written from the public calls alone: to be copied and changed

Arrays are sample-major: entry s * N + i belongs to sample s and hit i.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi
from ._args import (_aligned_bytes, _below_2_32, _count_ptr, _host, _new, _on_stream, _out_tensor, _p, _room, _samples, _stream_ptr, _tensor, _torch, _void,
                    _zeroed_out)
from ._queries import _hit_records, cast_rays, trace_rays
from ._world import Scene
from .environment import TABLE_HEADER_BYTES, Environment, _environment, _environment_rays, _host_environment, fold, lookup, table_bytes
from .materials import SURFACE_DTYPE, material_hits, probe_surfaces

UNIFORM, STRATIFIED = 1, 2  # RT_FILM_UNIFORM / RT_FILM_STRATIFIED (RT_FILM_CENTER, 0, is no pattern of a sampler)
SHADING, GEOMETRIC = 0, 1   # RT_HEMISPHERE_SHADING / RT_HEMISPHERE_GEOMETRIC
BALANCE, POWER = 0, 1       # RT_MIS_BALANCE / RT_MIS_POWER
MAX_SPP = 64


def rays(scene: Scene, hits, incoming, spp: int, pattern: int = STRATIFIED, seed: int = 0, ids=None, normal_kind: int = SHADING, out_rays=None,
         out_asks=None, out_dirs=None, out_pdf=None, out_lobe=None, stream=None):
    """rt_lobe_rays: returns (rays, asks, dirs, pdf, lobe) for ``spp`` directions per hit drawn from the hit's Phong mixture.
    ``incoming`` (N, 11) int32: the rays that produced the hits (Hit.ray); the view is minus their direction.  ``dirs`` (S*N, 3)
    float32: the direction, zeros for a record that is no hit; ``lobe`` (S*N,) uint8: 1 where it came from the specular lobe; ``pdf``
    (S*N,) float32: the mixture's density of the direction; ``asks`` (S*N,) uint8: the record is a hit, the density is finite and
    positive and the direction leaves the surface (about the SHADING or the GEOMETRIC normal); ``rays`` (S*N, 11) int32: the shadow ray
    along the direction, as hemisphere.rays writes it, all-zero words where ``asks`` is 0.  u_0 and u_1 are hemisphere.rays' for the
    same seed: a surface of shiness 0 gets that call's directions."""
    records = _hit_records(hits)
    n = records.shape[0]
    _tensor(incoming, "incoming", "int32", (n, 11))
    spp = _samples(spp)
    _tensor(ids, "ids", "int32", (n,), optional=True)
    entries = spp * n
    dev = records.device
    out_rays = _out_tensor(out_rays, (entries, 11), "int32", dev, "out_rays")
    out_asks = _out_tensor(out_asks, (entries,), "uint8", dev, "out_asks")
    out_dirs = _out_tensor(out_dirs, (entries, 3), "float32", dev, "out_dirs")
    out_pdf = _out_tensor(out_pdf, (entries,), "float32", dev, "out_pdf")
    out_lobe = _out_tensor(out_lobe, (entries,), "uint8", dev, "out_lobe")
    _capi.check(_capi.amd_lib().rt_lobe_rays(scene._h, _p(records), _p(incoming), n, _p(ids), spp, int(pattern), int(seed) & 0xFFFFFFFF, int(normal_kind),
                                             _p(out_rays), _p(out_asks), _p(out_dirs), _p(out_pdf), _p(out_lobe), _stream_ptr(stream)))
    return out_rays, out_asks, out_dirs, out_pdf, out_lobe


_lobe_rays = rays  # the loops have locals of that name


def _probes(dirs, n, name="dirs"):
    """(P, N, 3) or (P*N, 3) -> P"""
    if dirs is not None and hasattr(dirs, "dim") and dirs.dim() == 3:
        _tensor(dirs, name, "float32", (None, n, 3))
        return dirs.shape[0]
    _tensor(dirs, name, "float32", (None, 3))
    if n == 0 or dirs.shape[0] % n:
        raise ValueError(f"{name} must hold a whole number of directions per surface")
    return dirs.shape[0] // n


def pdf(surfaces, view, dirs, normal_kind: int = SHADING, out=None, stream=None):
    """rt_lobe_pdf: the mixture's density of ``dirs`` ((P, N, 3) or (P*N, 3) float32, probe-major as materials.probe_surfaces') on
    ``surfaces`` ((N, 18) int32, materials.material_hits) seen from ``view`` ((N, 3) float32, minus the incoming direction).  Takes no
    scene; GEOMETRIC is refused, a surface carrying the shading normal alone.  Returns ``out``, (P*N,) float32: +0 where valid is 0."""
    n = _tensor(surfaces, "surfaces", "int32", (None, 18)).shape[0]
    _tensor(view, "view", "float32", (n, 3))
    probes = _probes(dirs, n) if n else 0
    out = _out_tensor(out, (probes * n,), "float32", surfaces.device)
    _capi.check(_capi.amd_lib().rt_lobe_pdf(_p(surfaces), n, _p(view), _p(dirs), probes, int(normal_kind), _p(out), _stream_ptr(stream)))
    return out


_lobe_pdf = pdf


def environment_pdf(env: Environment, dirs, table=None, out=None, out_texel=None, want_texel: bool = True, stream=None):
    """rt_environment_pdf: the density per solid angle of ``dirs`` ((K, 3) float32) under the environment's table (``table``; None:
    env.table(stream)) — what environment.rays divides its radiance by.  Returns (pdf (K,) float32, texel (K,) int32: y * W + x);
    +0 for a direction that is zero or not finite, a table of another size and an environment without light.  ``want_texel`` False: no
    texel is written and None is returned in its place."""
    env = _environment(env)
    count = _tensor(dirs, "dirs", "float32", (None, 3)).shape[0]
    if table is None:
        table = env.table(stream)
    _tensor(table, "table", "uint8", (table_bytes(env.width, env.height),))
    out = _out_tensor(out, (count,), "float32", dirs.device)
    out_texel = _out_tensor(out_texel, (count,), "int32", dirs.device, "out_texel") if want_texel else None
    _capi.check(_capi.amd_lib().rt_environment_pdf(C.byref(env.desc), _p(table), _p(dirs), count, _p(out), _p(out_texel), _stream_ptr(stream)))
    return out, out_texel


def _counts(n_own, n_other):
    n_own, n_other = int(n_own), int(n_other)
    if not (0 <= n_own < 1 << 32 and 0 <= n_other < 1 << 32):
        raise ValueError("n_own and n_other are sample counts: 0 .. 2^32 - 1")
    return n_own, n_other


def mis_weigh(pdf_own, n_own: int, pdf_other=None, n_other: int = 0, heuristic: int = BALANCE, divide_by_own: bool = False, weight=None, rgb=None,
              stream=None):
    """rt_mis_weigh: per entry, w = a / (a + b) (BALANCE) or a^2 / (a^2 + b^2) (POWER) with a = n_own * pdf_own and b = n_other *
    pdf_other; ``pdf_other`` None or ``n_other`` 0: w = 1.  An a that is not finite or <= 0 gives 0.  ``weight`` (K,) float32 or None
    receives w; ``rgb`` (K, 3) float32 or None is multiplied by w in place — by w / pdf_own with ``divide_by_own``.  One of the two is
    given.  Returns (weight, rgb) as given."""
    count = _tensor(pdf_own, "pdf_own", "float32", (None,)).shape[0]
    _tensor(pdf_other, "pdf_other", "float32", (count,), optional=True)
    _tensor(weight, "weight", "float32", (count,), optional=True)
    _tensor(rgb, "rgb", "float32", (count, 3), optional=True)
    if weight is None and rgb is None:
        raise ValueError("weight or rgb must be given")
    n_own, n_other = _counts(n_own, n_other)
    _capi.check(_capi.amd_lib().rt_mis_weigh(count, _p(pdf_own), n_own, _p(pdf_other), n_other, int(heuristic), int(bool(divide_by_own)), _p(weight),
                                             _p(rgb), _stream_ptr(stream)))
    return weight, rgb


# ---- the CPU forms ----

def _host_surfaces(surfaces):
    a = np.ascontiguousarray(surfaces)
    if a.dtype == SURFACE_DTYPE:
        return a.reshape(-1)
    if a.ndim == 2 and a.shape[1] == 18 and a.dtype.itemsize == 4:
        return a.view(SURFACE_DTYPE).reshape(-1)
    raise ValueError("surfaces: expected a SURFACE_DTYPE array or an (N, 18) array of 4-byte words")


def rays_numpy(surfaces, view, spp: int, pattern: int = STRATIFIED, seed: int = 0, ids=None, normals=None):
    """rt_lobe_samples_cpu: what rays writes for hits whose material is ``surfaces`` (materials.material_hits; valid 0: zeros) seen
    from ``view`` ((N, 3) float32), bit for bit, on the CPU: (dirs (S, N, 3) float32, pdf (S, N) float32, lobe (S, N) uint8, asks (S, N)
    uint8).  ``normals`` (N, 3) float32 or None: the N to use — None is the record's shading normal (SHADING); pass hit.normal for
    GEOMETRIC.  ``ids``: N record ids or None for 0 .. N - 1."""
    surfaces = _host_surfaces(surfaces)
    n, spp = surfaces.shape[0], _samples(spp)
    view = _host(view, np.float32, (n, 3), "view")
    normals = _host(normals, np.float32, (n, 3), "normals", optional=True)
    ids = _host(ids, np.uint32, (n,), "ids", optional=True)
    dirs, density = np.zeros((spp, n, 3), dtype=np.float32), np.zeros((spp, n), dtype=np.float32)
    lobe, asks = np.zeros((spp, n), dtype=np.uint8), np.zeros((spp, n), dtype=np.uint8)
    _capi.check_host(_capi.host_lib().rt_lobe_samples_cpu(_void(surfaces), _void(normals), _void(view), _void(ids), n, spp, int(pattern),
                                                          int(seed) & 0xFFFFFFFF, _void(dirs), _void(density), _void(lobe), _void(asks)))
    return dirs, density, lobe, asks


def pdf_numpy(surfaces, view, dirs, normal_kind: int = SHADING) -> np.ndarray:
    """rt_lobe_pdf_cpu: pdf on the CPU, bit for bit.  ``dirs`` (P, N, 3) float32; returns (P, N) float32."""
    surfaces = _host_surfaces(surfaces)
    n = surfaces.shape[0]
    view = _host(view, np.float32, (n, 3), "view")
    dirs = np.ascontiguousarray(dirs, dtype=np.float32)
    if dirs.ndim != 3 or dirs.shape[1:] != (n, 3):
        raise ValueError(f"dirs: expected a (P, {n}, 3) float32 array")
    out = np.zeros(dirs.shape[:2], dtype=np.float32)
    _capi.check_host(_capi.host_lib().rt_lobe_pdf_cpu(_void(surfaces), n, _void(view), _void(dirs), dirs.shape[0], int(normal_kind), _void(out)))
    return out


def environment_pdf_numpy(texels, table, dirs, rotation: float = 0.0):
    """rt_environment_pdf_cpu: environment_pdf on the CPU, bit for bit.  ``table``: environment.table_numpy(texels); ``dirs`` (K, 3)
    float32.  Returns (pdf (K,) float32, texel (K,) uint32)."""
    texels, desc = _host_environment(texels, rotation, 1.0, 0)
    size = TABLE_HEADER_BYTES + 8 * texels.shape[0] + 4 * texels.shape[0] * texels.shape[1]
    held = _aligned_bytes(size)
    held[:] = _host(table, np.uint8, (size,), "table")
    dirs = np.ascontiguousarray(dirs, dtype=np.float32)
    if dirs.ndim != 2 or dirs.shape[1] != 3:
        raise ValueError("dirs: expected a (K, 3) float32 array")
    out, texel = np.zeros(dirs.shape[0], dtype=np.float32), np.zeros(dirs.shape[0], dtype=np.uint32)
    _capi.check_host(_capi.host_lib().rt_environment_pdf_cpu(C.byref(desc), _void(held), _void(dirs), dirs.shape[0], _void(out), _void(texel)))
    return out, texel


def mis_weigh_numpy(pdf_own, n_own: int, pdf_other=None, n_other: int = 0, heuristic: int = BALANCE, divide_by_own: bool = False, rgb=None):
    """rt_mis_weigh_cpu: mis_weigh on the CPU, bit for bit.  Returns (weight (K,) float32, rgb — a new (K, 3) array — or None)."""
    pdf_own = np.ascontiguousarray(pdf_own, dtype=np.float32).reshape(-1)
    count = pdf_own.shape[0]
    pdf_other = _host(pdf_other, np.float32, (count,), "pdf_other", optional=True)
    rgb = None if rgb is None else _host(rgb, np.float32, (count, 3), "rgb").copy()
    n_own, n_other = _counts(n_own, n_other)
    weight = np.zeros(count, dtype=np.float32)
    _capi.check_host(_capi.host_lib().rt_mis_weigh_cpu(count, _void(pdf_own), n_own, _void(pdf_other), n_other, int(heuristic), int(bool(divide_by_own)),
                                                       _void(weight), _void(rgb)))
    return weight, rgb


# ---- the two sequences ----

class Workspace:
    """The buffers of glossy_hits and sky_hits_mis, made once by workspace() so that a caller's loop allocates nothing: ``n`` records
    and ``entries`` (sample, hit) entries of room, about 160 B per entry and 72 B per record."""

    def __init__(self, n: int, entries: int, device):
        self.n, self.entries = int(n), int(entries)
        self.rays, self.shadow_hits = _new((entries, 11), "int32", device), _new((entries, 13), "int32", device)
        self.asks, self.lobe = _new((entries,), "uint8", device), _new((entries,), "uint8", device)
        self.dirs, self.radiance = _new((entries, 3), "float32", device), _new((entries, 3), "float32", device)
        self.diffuse, self.specular = _new((entries, 3), "float32", device), _new((entries, 3), "float32", device)
        self.pdf, self.pdf_other = _new((entries,), "float32", device), _new((entries,), "float32", device)
        self.texel = _new((entries,), "int32", device)
        self.surfaces = _new((n, 18), "int32", device)


def workspace(n: int, device, spp: int) -> Workspace:
    """A Workspace for glossy_hits on up to ``n`` hits with ``spp`` samples, and for sky_hits_mis with spp_env + spp_lobe = ``spp``."""
    if n < 0 or spp < 0:
        raise ValueError("n and spp must not be negative")
    return Workspace(int(n), int(n) * int(spp), device)


def _lobe_room(workspace, n, entries, dev, stream):
    return _room(workspace, Workspace, {"n": n, "entries": entries},
                 f"a lobes.Workspace with room for {n} records and {entries} (sample, hit) entries (lobes.workspace)", dev, stream)


def _begin(hits, incoming, ids, out, entries, stream):
    """the arguments the two loops share, checked: -> (records, n, device, out)"""
    records = _hit_records(hits)
    n, dev = records.shape[0], records.device
    _tensor(incoming, "incoming", "int32", (n, 11))
    _tensor(ids, "ids", "int32", (n,), optional=True)
    out = _zeroed_out(out, n, dev, stream)
    _below_2_32(entries, "(sample, hit) entries")
    return records, n, dev, out


def _view_of(incoming, view, n, stream):
    """``view`` as given ((N, 3) float32), or minus the incoming rays' directions, made on ``stream``"""
    if view is not None:
        return _tensor(view, "view", "float32", (n, 3))
    with _on_stream(stream):
        return (-incoming[:, 3:6].view(_torch().float32)).contiguous()


def glossy_hits(scene: Scene, hits, incoming, spp: int, max_depth: int, contribution: float = 1.0, out=None, pattern: int = STRATIFIED, seed: int = 0,
                ids=None, normal_kind: int = SHADING, view=None, ray_count=None, stream=None, workspace=None):
    """One glossy and diffuse bounce of the scene on every hit, ADDED to ``out`` ((N, 3) float32 CUDA; None: a new, zeroed tensor): the
    mean over ``spp`` directions drawn from the hit's own lobes of what ray_trace returns along them (TraceState { depth: max_depth,
    contribution }), times the material's diffuse and specular answer, over the direction's density.  Written from the public calls
    alone — the executable form of the sequence in INTEGRATION.md, to be copied and changed:
    rays -> trace_rays on all S*N rays -> material_hits + probe_surfaces(dirs) -> mis_weigh(pdf, divide_by_own, no other strategy) ->
    environment.fold without shadow hits.  ``view`` (N, 3) float32 or None: minus the incoming directions, made here if not given.  The
    rays of directions that do not ask are all-zero words; trace_rays traces them too and the fold never reads their results.  Every
    buffer is allocated once, up front — or none at all with ``out``, ``view`` and ``workspace``."""
    spp = _samples(spp)
    records, n, dev, out = _begin(hits, incoming, ids, out, spp * _hit_records(hits).shape[0], stream)
    _count_ptr(ray_count)
    if n == 0:
        return out
    m = spp * n
    view = _view_of(incoming, view, n, stream)
    w = _lobe_room(workspace, n, m, dev, stream)
    s = stream
    _lobe_rays(scene, records, incoming, spp, pattern, seed, ids, normal_kind, w.rays[:m], w.asks[:m], w.dirs[:m], w.pdf[:m], w.lobe[:m], stream=s)
    trace_rays(scene, w.rays[:m], max_depth, contribution, out=w.radiance[:m], ray_count=ray_count, stream=s)
    material_hits(scene, records, w.surfaces[:n], stream=s)
    probe_surfaces(w.surfaces[:n], view, w.dirs[:m].view(spp, n, 3), w.diffuse[:m].view(spp, n, 3), w.specular[:m].view(spp, n, 3), stream=s)
    mis_weigh(w.pdf[:m], 1, None, 0, BALANCE, True, rgb=w.radiance[:m], stream=s)
    fold(scene, records, w.asks[:m], spp, w.radiance[:m], w.diffuse[:m], w.specular[:m], out, None, stream=s)
    return out


def sky_hits_mis(scene: Scene, env: Environment, hits, incoming, spp_env: int = 8, spp_lobe: int = 8, heuristic: int = BALANCE, out=None,
                 pattern: int = STRATIFIED, seed: int = 0, ids=None, normal_kind: int = SHADING, view=None, stream=None, workspace=None):
    """The sky's light on every hit from two samplers at once, ADDED to ``out``: ``spp_env`` directions drawn by the sky's brightness
    (environment.rays) and ``spp_lobe`` drawn from the hit's own lobes (rays), each weighed against the other's density.  Written
    from the public calls alone:
      the environment's samples  environment.rays -> cast_rays -> material_hits + probe_surfaces(dirs) -> environment_pdf(dirs) and
                                 pdf(dirs) -> mis_weigh(radiance, which is already over its density) -> environment.fold
      the lobe's samples         rays -> cast_rays -> environment.lookup(the casts' misses, into zeros) -> probe_surfaces(dirs) ->
                                 environment_pdf(dirs) -> mis_weigh(pdf, divide_by_own) -> environment.fold into the same ``out``
    With ``spp_lobe`` 0 the first half alone runs, unweighed: environment.sky_hits' result bit for bit; with ``spp_env`` 0 the second
    alone.  The lobe's samples look the sky up with the environment's filter while the environment's samples carry their own texel: with
    environment.NEAREST the two estimate one integrand.  The casts take every ray, all-zero words included, so the whole sequence may
    be captured at once (the table apart: env.table(stream) is built by the first call).  ``normal_kind`` GEOMETRIC draws about
    hit.normal; the densities the two sets are weighed by are the shading normal's, pdf taking no other."""
    env = _environment(env)
    spp_env, spp_lobe = _samples(spp_env), _samples(spp_lobe)
    total = (spp_env + spp_lobe) * _hit_records(hits).shape[0]
    records, n, dev, out = _begin(hits, incoming, ids, out, total, stream)
    if n == 0 or total == 0:
        return out
    view = _view_of(incoming, view, n, stream)
    w = _lobe_room(workspace, n, total, dev, stream)
    s = stream
    material_hits(scene, records, w.surfaces[:n], stream=s)
    if spp_env:
        m, e = spp_env * n, slice(0, spp_env * n)
        _environment_rays(scene, env, records, spp_env, pattern, seed, ids, normal_kind, env.table(s), w.rays[e], w.asks[e], w.dirs[e], w.radiance[e],
                          w.texel[e], stream=s)
        cast_rays(scene, w.rays[e], out=w.shadow_hits[e], stream=s)
        probe_surfaces(w.surfaces[:n], view, w.dirs[e].view(spp_env, n, 3), w.diffuse[e].view(spp_env, n, 3), w.specular[e].view(spp_env, n, 3), stream=s)
        if spp_lobe:
            environment_pdf(env, w.dirs[e], env.table(s), w.pdf[e], w.texel[e], stream=s)
            _lobe_pdf(w.surfaces[:n], view, w.dirs[e].view(spp_env, n, 3), SHADING, w.pdf_other[e], stream=s)
            mis_weigh(w.pdf[e], spp_env, w.pdf_other[e], spp_lobe, heuristic, False, rgb=w.radiance[e], stream=s)
        fold(scene, records, w.asks[e], spp_env, w.radiance[e], w.diffuse[e], w.specular[e], out, w.shadow_hits[e], stream=s)
    if spp_lobe:
        m = spp_lobe * n
        l = slice(spp_env * n, spp_env * n + m)
        _lobe_rays(scene, records, incoming, spp_lobe, pattern, seed, ids, normal_kind, w.rays[l], w.asks[l], w.dirs[l], w.pdf[l], w.lobe[l], stream=s)
        cast_rays(scene, w.rays[l], out=w.shadow_hits[l], stream=s)
        with _on_stream(s):
            w.radiance[l].zero_()
        lookup(env, w.rays[l], w.shadow_hits[l], out=w.radiance[l], stream=s)
        probe_surfaces(w.surfaces[:n], view, w.dirs[l].view(spp_lobe, n, 3), w.diffuse[l].view(spp_lobe, n, 3), w.specular[l].view(spp_lobe, n, 3), stream=s)
        environment_pdf(env, w.dirs[l], env.table(s), w.pdf_other[l], w.texel[l], stream=s)
        mis_weigh(w.pdf[l], spp_lobe, w.pdf_other[l], spp_env, heuristic, True, rgb=w.radiance[l], stream=s)
        fold(scene, records, w.asks[l], spp_lobe, w.radiance[l], w.diffuse[l], w.specular[l], out, w.shadow_hits[l], stream=s)
    return out
