"""Hemisphere queries (include/rt_amd.h "hemisphere queries"): ambient occlusion and one bounce of diffuse light on caller-supplied hits.

get_shade lights a hit from the stored lights alone.  These calls sample the hemisphere over a hit with ``spp`` cosine-distributed
directions, chosen by the film queries' counter hash, and fold what comes back along them: the share of directions that nothing
blocks (ambient occlusion), and the radiance trace_rays returns along them, weighed by the hit's diffuse colour (one bounce of
inter-reflection) — noisy inputs that film, temporal, svgf and upsample are there to clean.

    rays / fold                rt_hemisphere_rays / rt_hemisphere_fold
    dirs_numpy / fold_numpy    the CPU forms (rt_hemisphere_dirs_cpu / rt_hemisphere_fold_cpu of librt_host.so): the device's bits
    ambient_hits               rays -> select_records -> cast_rays_indexed -> fold, written from the public calls alone
    indirect_hits              rays -> trace_rays -> fold(radiance), likewise: both to be copied and changed

Arrays are sample-major: entry s * N + i belongs to sample s and hit i.
"""
from __future__ import annotations

import numpy as np

from . import _capi
from ._args import _below_2_32, _count_ptr, _host, _new, _on_stream, _out_tensor, _p, _room, _samples, _stream_ptr, _tensor, _void, _zeroed_out
from ._queries import _hit_records, cast_rays_indexed, select_records, trace_rays
from ._world import Scene

UNIFORM, STRATIFIED = 1, 2  # RT_FILM_UNIFORM / RT_FILM_STRATIFIED (RT_FILM_CENTER, 0, is no pattern of a hemisphere)
SHADING, GEOMETRIC = 0, 1   # RT_HEMISPHERE_SHADING / RT_HEMISPHERE_GEOMETRIC
MAX_SPP = 64
INF = float("inf")


def rays(scene: Scene, hits, spp: int, pattern: int = STRATIFIED, seed: int = 0, ids=None, normal_kind: int = SHADING, out_rays=None, out_asks=None,
         out_dirs=None, stream=None):
    """rt_hemisphere_rays: returns (rays, asks, dirs) for ``spp`` cosine-distributed directions about each hit's normal — the shading
    normal get_shade lights with (SHADING) or hit.normal (GEOMETRIC).  ``ids`` (N,) int32 CUDA or None: the record id of the hash (the
    global pixel index, say; None: the record's number).  ``dirs`` (S*N, 3) float32: the direction of every entry of a hit, zeros for a
    record that is no hit; ``asks`` (S*N,) uint8: the direction leaves the surface; ``rays`` (S*N, 11) int32: the shadow ray get_shade
    would cast along it — from the hit, face Back, the hit's primitive excluded — all-zero words where ``asks`` is 0: one batch for
    select_records(asks) + cast_rays_indexed, or for trace_rays."""
    records = _hit_records(hits)
    n = records.shape[0]
    spp = _samples(spp)
    _tensor(ids, "ids", "int32", (n,), optional=True)
    entries = spp * n
    dev = records.device
    out_rays = _out_tensor(out_rays, (entries, 11), "int32", dev, "out_rays")
    out_asks = _out_tensor(out_asks, (entries,), "uint8", dev, "out_asks")
    out_dirs = _out_tensor(out_dirs, (entries, 3), "float32", dev, "out_dirs")
    _capi.check(_capi.amd_lib().rt_hemisphere_rays(scene._h, _p(records), n, _p(ids), spp, int(pattern), int(seed) & 0xFFFFFFFF, int(normal_kind),
                                                   _p(out_rays), _p(out_asks), _p(out_dirs), _stream_ptr(stream)))
    return out_rays, out_asks, out_dirs


_hemisphere_rays = rays  # the loops have locals of that name


def fold(scene: Scene, hits, asks, spp: int, shadow_hits=None, max_distance: float = INF, radiance=None, out=None, open=None, ambient=None, stream=None):
    """rt_hemisphere_fold: a sample is open where ``asks`` is set and its cast — ``shadow_hits`` (S*N, 13) int32, read only where
    ``asks`` is set; None: nothing occludes — found nothing nearer than ``max_distance`` (inf: whatever it found occludes).  ``open``
    (S*N,) uint8 or None: the flag per sample; ``ambient`` (N,) float32 or None: open samples / spp, 0 for a record that is no hit.
    ``radiance`` (S*N, 3) float32 with ``out`` (N, 3) float32, both or neither: out += (diffuse_color * E) * (1 - shiness), E the sum
    over the asked samples' radiance in ascending order divided by spp.  The call ADDS, as light_fold does: zero ``out`` first; a record
    that is no hit is not written.  Returns (open, ambient, out) as given."""
    records = _hit_records(hits)
    n = records.shape[0]
    spp = _samples(spp)
    entries = spp * n
    _tensor(asks, "asks", "uint8", (entries,))
    _tensor(shadow_hits, "shadow_hits", "int32", (entries, 13), optional=True)
    _tensor(radiance, "radiance", "float32", (entries, 3), optional=True)
    _tensor(out, "out", "float32", (n, 3), optional=True)
    if (radiance is None) != (out is None):
        raise ValueError("radiance and out are given together or not at all")
    _tensor(open, "open", "uint8", (entries,), optional=True)
    _tensor(ambient, "ambient", "float32", (n,), optional=True)
    _capi.check(_capi.amd_lib().rt_hemisphere_fold(scene._h, _p(records), n, spp, _p(asks), _p(shadow_hits), float(max_distance), _p(radiance), _p(open),
                                                   _p(ambient), _p(out), _stream_ptr(stream)))
    return open, ambient, out


def dirs_numpy(normals, spp: int, pattern: int = STRATIFIED, seed: int = 0, ids=None) -> np.ndarray:
    """rt_hemisphere_dirs_cpu: what rays writes into ``dirs`` for hits whose normal N is ``normals`` ((N, 3) float32), bit for bit, on
    the CPU: an (S, N, 3) float32 array.  It evaluates no material: for SHADING pass materials.material_hits' shading_normal.  ``ids``:
    N record ids or None for 0 .. N - 1."""
    normals = np.ascontiguousarray(normals, dtype=np.float32)
    if normals.ndim != 2 or normals.shape[1] != 3:
        raise ValueError("normals: expected an (N, 3) float32 array")
    n, spp = normals.shape[0], _samples(spp)
    ids = _host(ids, np.uint32, (n,), "ids", optional=True)
    out = np.zeros((spp, n, 3), dtype=np.float32)
    _capi.check_host(_capi.host_lib().rt_hemisphere_dirs_cpu(_void(normals), _void(ids), n, spp, int(pattern), int(seed) & 0xFFFFFFFF, _void(out)))
    return out


def fold_numpy(hits, valid, diffuse_color, shiness, asks, spp: int, shadow_hits=None, max_distance: float = INF, radiance=None, rgb=None):
    """rt_hemisphere_fold_cpu: fold on the CPU, bit for bit, with what the device reads from the scene as arrays: ``hits`` (N, 13) words
    (the position is read), ``valid`` (N,) the record is a hit, ``diffuse_color`` (N, 3) and ``shiness`` (N,) the material's.  ``rgb``
    (N, 3) float32 or None: the values the call adds to (with ``radiance``).  Returns (open (S*N,) uint8, ambient (N,) float32, rgb — a
    new array — or None)."""
    hits = np.ascontiguousarray(hits)
    if hits.ndim != 2 or hits.shape[1] != 13 or hits.dtype.itemsize != 4:
        raise ValueError("hits: expected an (N, 13) array of 4-byte words")
    n, spp = hits.shape[0], _samples(spp)
    entries = spp * n
    valid = _host(valid, np.uint8, (n,), "valid")
    asks = _host(asks, np.uint8, (entries,), "asks")
    diffuse_color = _host(diffuse_color, np.float32, (n, 3), "diffuse_color")
    shiness = _host(shiness, np.float32, (n,), "shiness")
    if shadow_hits is not None:
        shadow_hits = np.ascontiguousarray(shadow_hits)
        if shadow_hits.shape != (entries, 13) or shadow_hits.dtype.itemsize != 4:
            raise ValueError(f"shadow_hits: expected an ({entries}, 13) array of 4-byte words")
    radiance = _host(radiance, np.float32, (entries, 3), "radiance", optional=True)
    if (radiance is None) != (rgb is None):
        raise ValueError("radiance and rgb are given together or not at all")
    rgb = None if rgb is None else _host(rgb, np.float32, (n, 3), "rgb").copy()
    open_, ambient = np.zeros(entries, dtype=np.uint8), np.zeros(n, dtype=np.float32)
    _capi.check_host(_capi.host_lib().rt_hemisphere_fold_cpu(_void(hits), _void(valid), _void(diffuse_color), _void(shiness), n, spp, _void(asks),
                                                             _void(shadow_hits), float(max_distance), _void(radiance), _void(open_), _void(ambient),
                                                             _void(rgb)))
    return open_, ambient, rgb


class Workspace:
    """The buffers of ambient_hits and indirect_hits, made once by workspace() so that a caller's loop allocates nothing: ``entries``
    (sample, hit) entries of room, about 125 B each."""

    def __init__(self, entries: int, device):
        self.entries = int(entries)
        self.rays, self.shadow_hits = _new((entries, 11), "int32", device), _new((entries, 13), "int32", device)
        self.asks = _new((entries,), "uint8", device)
        self.index, self.count = _new((entries,), "int32", device), _new((1,), "int32", device)
        self.dirs, self.radiance = _new((entries, 3), "float32", device), _new((entries, 3), "float32", device)


def workspace(n: int, device, spp: int) -> Workspace:
    """A Workspace for ambient_hits and indirect_hits on up to ``n`` hits with ``spp`` samples."""
    if n < 0 or spp < 0:
        raise ValueError("n and spp must not be negative")
    return Workspace(int(n) * int(spp), device)


def _hemisphere_room(workspace, entries, dev, stream):
    return _room(workspace, Workspace, {"entries": entries}, f"a hemisphere.Workspace with room for {entries} (sample, hit) entries (hemisphere.workspace)",
                 dev, stream)


def ambient_hits(scene: Scene, hits, spp: int = 16, max_distance: float = INF, pattern: int = STRATIFIED, seed: int = 0, ids=None,
                 normal_kind: int = SHADING, out=None, open=None, ray_count=None, stream=None, workspace=None):
    """Ambient occlusion of every hit: the share of ``spp`` cosine-distributed directions along which nothing lies nearer than
    ``max_distance`` — ``out``, an (N,) float32 CUDA tensor (allocated if None), 0 for a record that is no hit; ``open`` (S*N,) uint8 or
    None: the flag per sample.  Written from the public calls alone — the executable form of the sequence in INTEGRATION.md, to be
    copied and changed: rays -> select_records(asks) -> cast_rays_indexed(rays -> shadow hits, ray_count) -> fold.  The shadow rays
    are Back rays, answered by back faces only: occluders are closed objects, as for every shadow ray of the reference.  Every buffer
    is allocated once, up front — or none at all with ``out`` and ``workspace`` (a Workspace); after that the function only enqueues
    library calls on ``stream`` and reads nothing back.  (Being a sequence of calls it may not be captured before select_records — and,
    on a scene walked breadth-first, cast_rays_indexed — has run once on the stream.)"""
    records = _hit_records(hits)
    n, dev = records.shape[0], records.device
    spp = _samples(spp)
    _tensor(ids, "ids", "int32", (n,), optional=True)
    _tensor(open, "open", "uint8", (spp * n,), optional=True)
    _count_ptr(ray_count)
    with _on_stream(stream):
        out = _out_tensor(out, (n,), "float32", dev)
    m = spp * n
    _below_2_32(m, "(sample, hit) entries")
    if n == 0:
        return out
    w = _hemisphere_room(workspace, m, dev, stream)
    s = stream
    _hemisphere_rays(scene, records, spp, pattern, seed, ids, normal_kind, w.rays[:m], w.asks[:m], w.dirs[:m], stream=s)
    select_records(w.asks[:m], w.index[:m], w.count, stream=s)
    cast_rays_indexed(scene, w.rays[:m], w.index[:m], w.count, w.shadow_hits[:m], ray_count=ray_count, stream=s)
    fold(scene, records, w.asks[:m], spp, w.shadow_hits[:m], max_distance, open=open, ambient=out, stream=s)
    return out


def indirect_hits(scene: Scene, hits, spp: int, max_depth: int, contribution: float = 1.0, out=None, pattern: int = STRATIFIED, seed: int = 0, ids=None,
                  normal_kind: int = SHADING, ray_count=None, stream=None, workspace=None):
    """One bounce of diffuse inter-reflection on every hit, ADDED to ``out`` ((N, 3) float32 CUDA; None: a new, zeroed tensor):
    out += (diffuse_color * E) * (1 - shiness), E the mean over ``spp`` cosine-distributed directions of what ray_trace returns along
    them with TraceState { depth: max_depth, contribution }.  Written from the public calls alone: rays -> trace_rays on all S*N rays ->
    fold(radiance).  The rays of directions that do not ask are all-zero words; trace_rays traces them too, and their results are never
    read, because the fold looks at ``asks``.  A caller who wants them compacted away must read a count back (select_records' count
    sizes the batch): this loop makes no host visit instead.  ``ray_count`` therefore counts the casts of those rays as well.  Every
    buffer is allocated once, up front — or none at all with ``out`` and ``workspace``."""
    records = _hit_records(hits)
    n, dev = records.shape[0], records.device
    spp = _samples(spp)
    _tensor(ids, "ids", "int32", (n,), optional=True)
    _count_ptr(ray_count)
    out = _zeroed_out(out, n, dev, stream)
    m = spp * n
    _below_2_32(m, "(sample, hit) entries")
    if n == 0:
        return out
    w = _hemisphere_room(workspace, m, dev, stream)
    s = stream
    _hemisphere_rays(scene, records, spp, pattern, seed, ids, normal_kind, w.rays[:m], w.asks[:m], w.dirs[:m], stream=s)
    trace_rays(scene, w.rays[:m], max_depth, contribution, out=w.radiance[:m], ray_count=ray_count, stream=s)
    fold(scene, records, w.asks[:m], spp, radiance=w.radiance[:m], out=out, stream=s)
    return out
