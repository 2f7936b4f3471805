"""Environment queries (include/rt_amd.h "environment queries"): a lat-long sky for the rays that found nothing, and sky light on
caller-supplied hits.

A ray that leaves the scene is black, and get_shade lights a hit from the stored lights alone.  An Environment is a caller-owned
(H, W, 3) float32 CUDA image, linear RGB, row 0 at the zenith, y up; ``lookup`` returns its radiance along rays (the records that are
"no hit", or all of them), ``table`` builds the integer sampling table of luma * sin(theta) on the device, ``rays`` draws ``spp``
directions per hit from that table — with the shadow ray along each and the texel's radiance over the density — and ``fold`` adds what
the casts and the material probes answered to a colour per hit.

    lookup / table / table_bytes / rays / fold     rt_environment_lookup / _table / _table_bytes / _rays / _fold
    lookup_numpy / table_numpy / samples_numpy / fold_numpy
                                                    the CPU forms (rt_environment_*_cpu of librt_host.so): the device's bits
    table_fields                                    a table as numpy arrays: width, height, total, w_max, M, C
    sky_hits                                        rays -> select_records -> cast_rays_indexed -> material_hits + probe_surfaces -> fold
    miss_radiance                                   cast_rays -> lookup, both written from the public calls alone: to be copied and changed
    trace_rays_levels                               rt.trace_rays_levels with the keyword ``environment``: the sky behind every level's misses

Arrays are sample-major: entry s * N + i belongs to sample s and hit i.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi
from ._args import (_aligned_bytes, _below_2_32, _count_ptr, _host, _new, _on_stream, _out_tensor, _p, _room, _samples, _stream_ptr, _tensor, _void,
                    _zeroed_out)
from ._loops import _trace_rays_levels
from ._queries import _hit_records, cast_rays, cast_rays_indexed, select_records
from ._world import Scene
from .materials import material_hits, probe_surfaces

NEAREST, BILINEAR = 0, 1    # RT_ENV_NEAREST / RT_ENV_BILINEAR
UNIFORM, STRATIFIED = 1, 2  # RT_FILM_UNIFORM / RT_FILM_STRATIFIED (RT_FILM_CENTER, 0, is no pattern of a sampler)
SHADING, GEOMETRIC = 0, 1   # RT_HEMISPHERE_SHADING / RT_HEMISPHERE_GEOMETRIC
MAX_SPP = 64
MAX_WIDTH, MAX_HEIGHT = 16384, 8192
ROW_TILE = 256              # the columns one workgroup of the row scan takes at a time (csrc/rt_environment_query.hip)
TABLE_HEADER_BYTES = 24


def table_bytes(width: int, height: int) -> int:
    """rt_environment_table_bytes: 24 + 8 H + 4 W H, or 0 for an image over the limits (or with a side of 0)."""
    if not (0 <= int(width) < 1 << 32 and 0 <= int(height) < 1 << 32):
        return 0
    return int(_capi.amd_lib().rt_environment_table_bytes(int(width), int(height)))


class Environment:
    """A lat-long environment: ``texels`` (H, W, 3) float32 CUDA, linear RGB, row 0 at the zenith, held by reference — the caller owns
    it and may write into it (then ``invalidate()`` the table).  ``rotation``: radians about +y, added to phi; ``scale`` multiplies every
    looked-up radiance; ``filter``: NEAREST or BILINEAR (the lookup's; a sample's radiance is its own texel's either way).  ``desc`` is
    the rt_environment passed to the library; ``table(stream)`` the sampling table, built by the first call that asks for it."""

    def __init__(self, texels, rotation: float = 0.0, scale: float = 1.0, filter: int = BILINEAR):
        _tensor(texels, "texels", "float32", (None, None, 3))
        self.texels = texels
        self.height, self.width = int(texels.shape[0]), int(texels.shape[1])
        self.rotation, self.scale, self.filter = float(rotation), float(scale), int(filter)
        self._table = None

    @property
    def desc(self) -> _capi.EnvironmentDesc:
        return _capi.EnvironmentDesc(self.texels.data_ptr(), self.width, self.height, self.rotation, self.scale, self.filter)

    def table(self, stream=None):
        if self._table is None:
            self._table = table(self, stream=stream)
        return self._table

    def invalidate(self) -> None:
        """forget the table: the texels have changed"""
        self._table = None


def _environment(env):
    if not isinstance(env, Environment):
        raise ValueError("env must be an environment.Environment")
    return env


def table(env: Environment, out=None, stream=None):
    """rt_environment_table: the sampling table of ``env`` built on ``stream`` — a max reduction, a scan per row, a scan over the rows —
    into ``out``, a (table_bytes(W, H),) uint8 CUDA tensor (allocated if None).  Returns it; Environment.table() keeps one."""
    env = _environment(env)
    size = table_bytes(env.width, env.height)
    if out is None:
        with _on_stream(stream):
            out = _new((max(size, 1),), "uint8", env.texels.device)[:size]
    else:
        _tensor(out, "out", "uint8", (size,))
    _capi.check(_capi.amd_lib().rt_environment_table(C.byref(env.desc), _p(out), _stream_ptr(stream)))
    return out


def lookup(env: Environment, rays, hits=None, count=None, parent=None, out=None, stream=None):
    """rt_environment_lookup: the environment's radiance along ``rays`` ((N, 11) int32 CUDA; the direction is read).  With ``hits``
    (a Hits or its (N, 13) record tensor) only the records that are "no hit" are written and the others are left as they are; without,
    every record is.  ``count``: a 1-element int32 CUDA tensor, the live records, or None for all N.  ``parent`` (N,) int32 or None:
    record j writes slot parent[j] of ``out`` instead of slot j — tree_fold's addressing; a slot at or beyond out's M writes nothing.
    ``out``: (M, 3) float32 CUDA; None: a new (N, 3) tensor, zeroed when ``hits`` is given.  Returns ``out``."""
    env = _environment(env)
    n, dev = _tensor(rays, "rays", "int32", (None, 11)).shape[0], rays.device
    records = None if hits is None else _hit_records(hits)
    if records is not None and records.shape[0] != n:
        raise ValueError("hits must hold one record per ray")
    _tensor(count, "count", "int32", (1,), optional=True)
    _tensor(parent, "parent", "int32", (n,), optional=True)
    if out is None:
        with _on_stream(stream):
            out = _new((n, 3), "float32", dev)
            if records is not None or count is not None:
                out.zero_()
    else:
        _tensor(out, "out", "float32", (None, 3))
    _capi.check(_capi.amd_lib().rt_environment_lookup(C.byref(env.desc), _p(rays), n, _p(count), _p(records), _p(parent), _p(out), out.shape[0],
                                                      _stream_ptr(stream)))
    return out


def rays(scene: Scene, env: Environment, hits, spp: int, pattern: int = STRATIFIED, seed: int = 0, ids=None, normal_kind: int = SHADING, table=None,
         out_rays=None, out_asks=None, out_dirs=None, out_radiance=None, out_texel=None, stream=None):
    """rt_environment_rays: returns (rays, asks, dirs, radiance, texel) for ``spp`` directions per hit drawn from the environment's
    table (``table``; None: env.table(stream)) in proportion to luma * sin(theta).  ``dirs`` (S*N, 3) float32: the direction, zeros for
    a record that is no hit or an environment without light; ``texel`` (S*N,) int32: y * W + x of the sampled texel; ``asks`` (S*N,)
    uint8: the record is a hit, the density is finite and positive and the direction leaves the surface (about the SHADING or the
    GEOMETRIC normal); ``radiance`` (S*N, 3) float32: texel * scale / pdf where ``asks``, zeros elsewhere; ``rays`` (S*N, 11) int32: the
    shadow ray along the direction, as hemisphere.rays writes it, all-zero words where ``asks`` is 0."""
    env = _environment(env)
    records = _hit_records(hits)
    n = records.shape[0]
    spp = _samples(spp)
    _tensor(ids, "ids", "int32", (n,), optional=True)
    if table is None:
        table = env.table(stream)
    _tensor(table, "table", "uint8", (table_bytes(env.width, env.height),))
    entries = spp * n
    dev = records.device
    out_rays = _out_tensor(out_rays, (entries, 11), "int32", dev, "out_rays")
    out_asks = _out_tensor(out_asks, (entries,), "uint8", dev, "out_asks")
    out_dirs = _out_tensor(out_dirs, (entries, 3), "float32", dev, "out_dirs")
    out_radiance = _out_tensor(out_radiance, (entries, 3), "float32", dev, "out_radiance")
    out_texel = _out_tensor(out_texel, (entries,), "int32", dev, "out_texel")
    _capi.check(_capi.amd_lib().rt_environment_rays(scene._h, C.byref(env.desc), _p(table), _p(records), n, _p(ids), spp, int(pattern),
                                                    int(seed) & 0xFFFFFFFF, int(normal_kind), _p(out_rays), _p(out_asks), _p(out_dirs),
                                                    _p(out_radiance), _p(out_texel), _stream_ptr(stream)))
    return out_rays, out_asks, out_dirs, out_radiance, out_texel


_environment_rays = rays  # the loops have locals of that name


def fold(scene: Scene, hits, asks, spp: int, radiance, diffuse, specular, out, shadow_hits=None, open=None, stream=None):
    """rt_environment_fold: a sample is open where ``asks`` is set and its cast — ``shadow_hits`` (S*N, 13) int32, read only where
    ``asks`` is set; None: nothing occludes — found nothing at all.  ``diffuse`` and ``specular`` ((S, N, 3) or (S*N, 3) float32): what
    materials.probe_surfaces returns for the directions.  out += D * (1 - shiness) + S * shiness with D and S the sums over the open
    samples of diffuse * radiance and specular * radiance, in ascending order, divided by spp.  The call ADDS, as arealights.fold does:
    ``out`` (N, 3) float32 holds what it adds to; a record that is no hit is not written.  ``open`` (S*N,) uint8 or None: the flag per
    sample.  Returns (open, out) as given."""
    records = _hit_records(hits)
    n = records.shape[0]
    spp = _samples(spp)
    entries = spp * n
    _tensor(asks, "asks", "uint8", (entries,))
    _tensor(shadow_hits, "shadow_hits", "int32", (entries, 13), optional=True)
    _tensor(radiance, "radiance", "float32", (entries, 3))
    diffuse = _tensor(diffuse, "diffuse", "float32", (spp, n, 3) if diffuse is not None and diffuse.dim() == 3 else (entries, 3))
    specular = _tensor(specular, "specular", "float32", (spp, n, 3) if specular is not None and specular.dim() == 3 else (entries, 3))
    _tensor(out, "out", "float32", (n, 3))
    _tensor(open, "open", "uint8", (entries,), optional=True)
    _capi.check(_capi.amd_lib().rt_environment_fold(scene._h, _p(records), n, spp, _p(asks), _p(shadow_hits), _p(radiance), _p(diffuse), _p(specular),
                                                    _p(open), _p(out), _stream_ptr(stream)))
    return open, out


# ---- the CPU forms ----

def _host_environment(texels, rotation, scale, filter):
    """-> (the image, held by the caller of this for as long as the descriptor is used; the descriptor)"""
    texels = np.ascontiguousarray(texels, dtype=np.float32)
    if texels.ndim != 3 or texels.shape[2] != 3:
        raise ValueError("texels: expected an (H, W, 3) float32 array")
    if not (texels.shape[0] < 1 << 32 and texels.shape[1] < 1 << 32):
        raise ValueError("texels: a side of 2^32 or more")
    return texels, _capi.EnvironmentDesc(texels.ctypes.data, texels.shape[1], texels.shape[0], float(rotation), float(scale), int(filter))


def table_numpy(texels) -> np.ndarray:
    """rt_environment_table_cpu: the table of an (H, W, 3) float32 image, every word the device's: a (table_bytes(W, H),) uint8 array
    (8-byte aligned; table_fields reads it)."""
    texels, desc = _host_environment(texels, 0.0, 1.0, NEAREST)
    out = _aligned_bytes(TABLE_HEADER_BYTES + 8 * texels.shape[0] + 4 * texels.shape[0] * texels.shape[1])
    _capi.check_host(_capi.host_lib().rt_environment_table_cpu(C.byref(desc), _void(out)))
    return out


def table_fields(table, width: int, height: int) -> dict:
    """A table (a uint8 array, or a CUDA tensor, which is copied to the host) as its parts: ``width``, ``height``, ``total`` (ints),
    ``w_max`` (float32), ``M`` (H,) uint64 — the inclusive marginal — and ``C`` (H, W) uint32 — the inclusive rows."""
    if not isinstance(table, np.ndarray):
        table = table.cpu().numpy()
    raw = np.ascontiguousarray(table).view(np.uint8).reshape(-1)
    size = TABLE_HEADER_BYTES + 8 * height + 4 * width * height
    if raw.size != size:
        raise ValueError(f"table: expected {size} bytes")
    head = raw[:TABLE_HEADER_BYTES].copy()
    return dict(width=int(head[0:4].view(np.uint32)[0]), height=int(head[4:8].view(np.uint32)[0]), total=int(head[8:16].view(np.uint64)[0]),
                w_max=head[16:20].view(np.float32)[0], pad=int(head[20:24].view(np.uint32)[0]),
                M=raw[TABLE_HEADER_BYTES:TABLE_HEADER_BYTES + 8 * height].copy().view(np.uint64),
                C=raw[TABLE_HEADER_BYTES + 8 * height:].copy().view(np.uint32).reshape(height, width))


def lookup_numpy(texels, rays, rotation: float = 0.0, scale: float = 1.0, filter: int = BILINEAR, hits=None, count=None, parent=None, out=None):
    """rt_environment_lookup_cpu: lookup on the CPU, bit for bit.  ``rays``: (N, 11) 4-byte words, or (N, 3) float32 directions.
    ``hits`` (N, 13) words, ``count`` an int, ``parent`` (N,) and ``out`` (M, 3) float32 (copied; None: zeros, (N, 3)) as lookup's.
    Returns the (M, 3) float32 result."""
    texels, desc = _host_environment(texels, rotation, scale, filter)
    rays = np.ascontiguousarray(rays)
    if rays.ndim == 2 and rays.shape[1] == 3:
        words = np.zeros((rays.shape[0], 11), dtype=np.uint32)
        words[:, 3:6] = rays.astype(np.float32).view(np.uint32)
        rays = words
    if rays.ndim != 2 or rays.shape[1] != 11 or rays.dtype.itemsize != 4:
        raise ValueError("rays: expected an (N, 11) array of 4-byte words or an (N, 3) float32 array")
    n = rays.shape[0]
    if hits is not None:
        hits = np.ascontiguousarray(hits)
        if hits.shape != (n, 13) or hits.dtype.itemsize != 4:
            raise ValueError(f"hits: expected an ({n}, 13) array of 4-byte words")
    parent = _host(parent, np.uint32, (n,), "parent", optional=True)
    count = None if count is None else np.array([int(count)], dtype=np.uint32)
    out = np.zeros((n, 3), dtype=np.float32) if out is None else np.array(out, dtype=np.float32, order="C")
    if out.ndim != 2 or out.shape[1] != 3:
        raise ValueError("out: expected an (M, 3) float32 array")
    _capi.check_host(_capi.host_lib().rt_environment_lookup_cpu(C.byref(desc), _void(rays), n, _void(count), _void(hits), _void(parent), _void(out),
                                                                out.shape[0]))
    return out


def samples_numpy(texels, table, normals, spp: int, pattern: int = STRATIFIED, seed: int = 0, ids=None, rotation: float = 0.0, scale: float = 1.0):
    """rt_environment_samples_cpu: what rays writes for hits whose normal N is ``normals`` ((N, 3) float32), bit for bit, on the CPU:
    (dirs (S, N, 3) float32, radiance (S, N, 3) float32, texel (S, N) uint32, asks (S, N) uint8).  ``table``: table_numpy(texels).  It
    evaluates no material: for SHADING pass materials.material_hits' shading_normal.  ``ids``: N record ids or None for 0 .. N - 1."""
    texels, desc = _host_environment(texels, rotation, scale, NEAREST)
    normals = np.ascontiguousarray(normals, dtype=np.float32)
    if normals.ndim != 2 or normals.shape[1] != 3:
        raise ValueError("normals: expected an (N, 3) float32 array")
    n, spp = normals.shape[0], _samples(spp)
    size = TABLE_HEADER_BYTES + 8 * texels.shape[0] + 4 * texels.shape[0] * texels.shape[1]
    held = _aligned_bytes(size)
    held[:] = _host(table, np.uint8, (size,), "table")
    ids = _host(ids, np.uint32, (n,), "ids", optional=True)
    dirs, radiance = np.zeros((spp, n, 3), dtype=np.float32), np.zeros((spp, n, 3), dtype=np.float32)
    texel, asks = np.zeros((spp, n), dtype=np.uint32), np.zeros((spp, n), dtype=np.uint8)
    _capi.check_host(_capi.host_lib().rt_environment_samples_cpu(C.byref(desc), _void(held), _void(normals), _void(ids), n, spp, int(pattern),
                                                                 int(seed) & 0xFFFFFFFF, _void(dirs), _void(radiance), _void(texel), _void(asks)))
    return dirs, radiance, texel, asks


def fold_numpy(valid, shiness, asks, spp: int, radiance, diffuse, specular, rgb, shadow_hits=None):
    """rt_environment_fold_cpu: fold on the CPU, bit for bit, with what the device reads from the scene as arrays: ``valid`` (N,) the
    record is a hit, ``shiness`` (N,) the material's.  ``rgb`` (N, 3) float32: the values the call adds to.  Returns (open (S*N,) uint8,
    rgb — a new array)."""
    valid = np.ascontiguousarray(valid)
    n, spp = valid.shape[0], _samples(spp)
    entries = spp * n
    valid = _host(valid, np.uint8, (n,), "valid")
    shiness = _host(shiness, np.float32, (n,), "shiness")
    asks = _host(np.asarray(asks).reshape(-1), np.uint8, (entries,), "asks")
    radiance = _host(np.asarray(radiance).reshape(-1, 3), np.float32, (entries, 3), "radiance")
    diffuse = _host(np.asarray(diffuse).reshape(-1, 3), np.float32, (entries, 3), "diffuse")
    specular = _host(np.asarray(specular).reshape(-1, 3), np.float32, (entries, 3), "specular")
    if shadow_hits is not None:
        shadow_hits = np.ascontiguousarray(shadow_hits)
        if shadow_hits.shape != (entries, 13) or shadow_hits.dtype.itemsize != 4:
            raise ValueError(f"shadow_hits: expected an ({entries}, 13) array of 4-byte words")
    rgb = _host(rgb, np.float32, (n, 3), "rgb").copy()
    open_ = np.zeros(entries, dtype=np.uint8)
    _capi.check_host(_capi.host_lib().rt_environment_fold_cpu(_void(valid), _void(shiness), n, spp, _void(asks), _void(shadow_hits), _void(radiance),
                                                              _void(diffuse), _void(specular), _void(open_), _void(rgb)))
    return open_, rgb


# ---- the two sequences ----

class Workspace:
    """The buffers of sky_hits and miss_radiance, made once by workspace() so that a caller's loop allocates nothing: ``n`` records and
    ``entries`` (sample, hit) entries of room, about 150 B per entry and 124 B per record."""

    def __init__(self, n: int, entries: int, device):
        self.n, self.entries = int(n), int(entries)
        self.rays, self.shadow_hits = _new((entries, 11), "int32", device), _new((entries, 13), "int32", device)
        self.asks = _new((entries,), "uint8", device)
        self.index, self.count = _new((entries,), "int32", device), _new((1,), "int32", device)
        self.dirs, self.radiance = _new((entries, 3), "float32", device), _new((entries, 3), "float32", device)
        self.diffuse, self.specular = _new((entries, 3), "float32", device), _new((entries, 3), "float32", device)
        self.texel = _new((entries,), "int32", device)
        self.surfaces, self.hits = _new((n, 18), "int32", device), _new((n, 13), "int32", device)


def workspace(n: int, device, spp: int = 0) -> Workspace:
    """A Workspace for sky_hits on up to ``n`` hits with ``spp`` samples, and for miss_radiance on up to ``n`` rays."""
    if n < 0 or spp < 0:
        raise ValueError("n and spp must not be negative")
    return Workspace(int(n), int(n) * int(spp), device)


def _environment_room(workspace, n, entries, dev, stream):
    return _room(workspace, Workspace, {"n": n, "entries": entries},
                 f"an environment.Workspace with room for {n} records and {entries} (sample, hit) entries (environment.workspace)", dev, stream)


def sky_hits(scene: Scene, env: Environment, hits, view, spp: int = 16, out=None, pattern: int = STRATIFIED, seed: int = 0, ids=None,
             normal_kind: int = SHADING, open=None, ray_count=None, stream=None, workspace=None):
    """The sky's light on every hit, ADDED to ``out`` ((N, 3) float32 CUDA; None: a new, zeroed tensor): ``spp`` directions drawn in
    proportion to the environment's brightness, a shadow cast along each, and the material's diffuse and specular answer to the ones
    nothing blocks.  ``view`` (N, 3) float32: what the reference puts into view_direction — minus the incoming ray's direction.  Written
    from the public calls alone — the executable form of the sequence in INTEGRATION.md, to be copied and changed:
    rays -> select_records(asks) -> cast_rays_indexed(rays -> shadow hits) -> material_hits + probe_surfaces(dirs) -> fold.  The table
    is env.table(stream): built by the first call, which therefore enqueues three kernels more.  Every buffer is allocated once, up
    front — or none at all with ``out`` and ``workspace`` (a Workspace); after that the function only enqueues library calls on
    ``stream`` and reads nothing back.  (Being a sequence of calls it may not be captured before select_records — and, on a scene walked
    breadth-first, cast_rays_indexed — has run once on the stream.)"""
    env = _environment(env)
    records = _hit_records(hits)
    n, dev = records.shape[0], records.device
    spp = _samples(spp)
    _tensor(view, "view", "float32", (n, 3))
    _tensor(ids, "ids", "int32", (n,), optional=True)
    _tensor(open, "open", "uint8", (spp * n,), optional=True)
    _count_ptr(ray_count)
    out = _zeroed_out(out, n, dev, stream)
    m = spp * n
    _below_2_32(m, "(sample, hit) entries")
    if n == 0:
        return out
    w = _environment_room(workspace, n, m, dev, stream)
    s = stream
    _environment_rays(scene, env, records, spp, pattern, seed, ids, normal_kind, env.table(s), w.rays[:m], w.asks[:m], w.dirs[:m], w.radiance[:m], w.texel[:m],
                      stream=s)
    select_records(w.asks[:m], w.index[:m], w.count, stream=s)
    cast_rays_indexed(scene, w.rays[:m], w.index[:m], w.count, w.shadow_hits[:m], ray_count=ray_count, stream=s)
    material_hits(scene, records, w.surfaces[:n], stream=s)
    probe_surfaces(w.surfaces[:n], view, w.dirs[:m].view(spp, n, 3), w.diffuse[:m].view(spp, n, 3), w.specular[:m].view(spp, n, 3), stream=s)
    fold(scene, records, w.asks[:m], spp, w.radiance[:m], w.diffuse[:m], w.specular[:m], out, w.shadow_hits[:m], open, stream=s)
    return out


def miss_radiance(scene: Scene, env: Environment, rays, out=None, hits=None, stream=None, workspace=None):
    """What lies behind a batch of rays: cast_rays -> lookup(hits).  ``out`` (N, 3) float32 CUDA (None: a new, zeroed tensor) receives
    the environment's radiance where a ray found nothing and is left as it is where it hit; ``hits`` (N, 13) int32 or None: where the
    cast's records go (for shade_hits or sky_hits afterwards).  Written from the public calls alone; returns ``out``."""
    env = _environment(env)
    n, dev = _tensor(rays, "rays", "int32", (None, 11)).shape[0], rays.device
    out = _zeroed_out(out, n, dev, stream)
    if n == 0:
        return out
    if hits is None:
        hits = _environment_room(workspace, n, 0, dev, stream).hits[:n]
    else:
        _tensor(hits, "hits", "int32", (n, 13))
    cast_rays(scene, rays, out=hits, stream=stream)
    lookup(env, rays, hits, out=out, stream=stream)
    return out


def trace_rays_levels(scene: Scene, rays, max_depth: int, contribution=1.0, out=None, ray_count=None, stream=None, level_capacity=None,
                      check: bool = True, overflow=None, level_counts=None, open_casts: bool = False, environment=None):
    """rt.trace_rays_levels — ray_trace written one level of the recursion tree at a time from the public calls — with one keyword
    more.  ``environment`` (an Environment): each level's tree_fold is followed by ``lookup`` with that level's rays, hits, count and
    parent links (the roots write their own slots), so a ray that leaves the scene, at any depth, returns the sky instead of black and
    the parents fold it with their weights.  A root the entry gate turned away (contribution < 0.001) was never cast and reads as a miss:
    it returns the sky too.  With ``environment=None`` the function enqueues exactly rt.trace_rays_levels' calls.  Every other argument
    is that function's."""
    return _trace_rays_levels(scene, rays, max_depth, contribution, out, ray_count, stream, level_capacity, check, overflow, level_counts, open_casts,
                              environment)
