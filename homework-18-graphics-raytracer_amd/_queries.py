"""The queries on caller-supplied records: rays (cast, trace, the stochastic trace), hits (shade, reflect, refract), scatters, and the
two calls every loop is made of — select_records and cast_rays_indexed."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi
from ._args import _count_ptr, _host_column, _host_records, _new, _out_tensor, _p, _stream_ptr, _tensor, _torch
from ._capi import Camera, Frame
from ._render import Rng
from ._world import Scene

# ---- ray queries: World::cast on caller-supplied rays (include/rt_amd.h rt_cast_rays) ----

FRONT, BACK, BOTH = 0, 1, 2  # FaceDirection, main.rs:52-57
SPHERE, TRIANGLE = 0, 1      # PrimitiveIndex, primitives.rs:31-34
HIT_NONE = -1                # RT_HIT_NONE seen as int32: the cast returned None
RAY_DTYPE = np.dtype([("origin", "<f4", 3), ("direction", "<f4", 3), ("face_direction", "<u4"), ("has_exclude", "<u4"),
                      ("exclude_kind", "<u4"), ("exclude_index", "<u4"), ("exclude_face", "<u4")])  # rt_ray, 44 bytes
HIT_DTYPE = np.dtype([("kind", "<u4"), ("index", "<u4"), ("object_index", "<u4"), ("position", "<f4", 3), ("normal", "<f4", 3),
                      ("uv", "<f4", 2), ("face_direction", "<u4"), ("distance", "<f4")])  # rt_hit, 52 bytes


def make_rays(origins, directions, face=FRONT, exclude_kind=None, exclude_index=None, exclude_face=BOTH):
    """Pack rays into an (N, 11) int32 CUDA tensor of rt_ray records, on the device.

    origins, directions: (N, 3) float32 CUDA tensors (directions are used as given: cast does not normalise them).
    face, exclude_face: FRONT / BACK / BOTH, scalars or (N,) tensors.
    exclude_kind, exclude_index: both None (no exclusion), or scalars / (N,) tensors: SPHERE or TRIANGLE and the index in that
    array; a negative kind means no exclusion for that ray, and an index beyond its array excludes nothing (as in the reference)."""
    torch = _torch()
    for name, t in (("origins", origins), ("directions", directions)):
        _tensor(t, name, "float32", (None, 3), contiguous=False)
    n = origins.shape[0]
    if directions.shape[0] != n:
        raise ValueError("origins and directions differ in length")
    dev = origins.device

    def column(v, name):
        if torch.is_tensor(v):
            if v.shape != (n,):
                raise ValueError(f"{name} must be a scalar or an (N,) tensor")
            return v.to(device=dev, dtype=torch.int64)
        return torch.full((n,), int(v), dtype=torch.int64, device=dev)

    rays = torch.zeros((n, 11), dtype=torch.int32, device=dev)
    rays[:, 0:3] = origins.view(torch.int32)
    rays[:, 3:6] = directions.view(torch.int32)
    rays[:, 6] = column(face, "face").to(torch.int32)
    if (exclude_kind is None) != (exclude_index is None):
        raise ValueError("exclude_kind and exclude_index go together")
    if exclude_kind is not None:
        kind = column(exclude_kind, "exclude_kind")
        some = kind >= 0
        rays[:, 7] = some.to(torch.int32)
        rays[:, 8] = torch.where(some, kind, torch.zeros_like(kind)).to(torch.int32)
        rays[:, 9] = torch.where(some, column(exclude_index, "exclude_index"), torch.zeros_like(kind)).to(torch.int32)
        rays[:, 10] = torch.where(some, column(exclude_face, "exclude_face"), torch.zeros_like(kind)).to(torch.int32)
    return rays


def cast_rays(scene: Scene, rays, out=None, stream=None):
    """World::cast (src/main.rs:180-326) for every ray of an (N, 11) int32 CUDA tensor of rt_ray records (make_rays, camera_rays):
    returns ``out``, an (N, 13) int32 CUDA tensor of rt_hit records (allocated if None; Hits names its fields), bit-identical to the
    reference's cast.  Stream-ordered on ``stream`` (default: torch's current stream)."""
    n = _tensor(rays, "rays", "int32", (None, 11)).shape[0]
    out = _out_tensor(out, (n, 13), "int32", rays.device)
    _capi.check(_capi.amd_lib().rt_cast_rays(scene._h, _p(rays), n, _p(out), _stream_ptr(stream)))
    return out


class Hits:
    """Named views of an (N, 13) int32 tensor of rt_hit records (what cast_rays returns), on the same storage."""

    def __init__(self, records):
        torch = _torch()
        _tensor(records, "records", "int32", (None, 13), cuda=False, contiguous=False)
        self.records = records
        self.kind = records[:, 0]               # SPHERE, TRIANGLE or HIT_NONE
        self.index = records[:, 1]              # in the sphere or the triangle array
        self.object_index = records[:, 2]
        self.position = records[:, 3:6].view(torch.float32)
        self.normal = records[:, 6:9].view(torch.float32)
        self.uv = records[:, 9:11].view(torch.float32)
        self.face = records[:, 11]              # FRONT or BACK
        self.distance = records[:, 12].view(torch.float32)

    @property
    def hit(self):
        """bool mask: the cast returned Some."""
        return self.kind != HIT_NONE

    def __len__(self):
        return self.records.shape[0]


def camera_rays(camera: Camera, frame: Frame, out=None, stream=None):
    """The primary rays Camera::shoot(clip(x, y)) of a frame or tile (src/main.rs:83-99, 1093-1096), as an (rows * cols, 11) int32 CUDA
    tensor of rt_ray records in the tile's compact row order — the rays the Whitted pass casts first, bit for bit."""
    n = frame.rows * frame.cols
    out = _out_tensor(out, (n, 11), "int32", "cuda")
    _capi.check(_capi.amd_lib().rt_camera_rays(C.byref(camera), C.byref(frame), _p(out), _stream_ptr(stream)))
    return out


def cast_rays_numpy(scene: Scene, rays_np) -> np.ndarray:
    """Host-buffer convenience (rt_cast_rays_host, synchronous): rays as a RAY_DTYPE structured array or an (N, 11) array of 4-byte
    words; returns the hits as a HIT_DTYPE structured array."""
    a = _host_records(rays_np, RAY_DTYPE, 11, "rays")
    hits = np.zeros(a.shape[0], dtype=HIT_DTYPE)
    _capi.check(_capi.amd_lib().rt_cast_rays_host(scene._h, a.ctypes.data_as(C.c_void_p), a.shape[0], hits.ctypes.data_as(C.c_void_p)))
    return hits


# ---- radiance queries: World::ray_trace on caller-supplied rays (include/rt_amd.h rt_trace_rays) ----

def trace_rays(scene: Scene, rays, max_depth: int, contribution: float = 1.0, out=None, ray_count=None, stream=None):
    """ray_trace (src/main.rs:466-519) for every ray of an (N, 11) int32 CUDA tensor of rt_ray records (make_rays, camera_rays), with
    TraceState { depth: max_depth, contribution }: returns ``out``, an (N, 3) float32 CUDA tensor (allocated if None) holding
    ray_trace's own value bit for bit — not ``0.0 + value`` as a frame stores it, so ``trace_rays(camera_rays(f)) + 0.0`` is the frame.
    ``ray_count``: a 1-element int64 CUDA tensor that the World::cast count is added to.  Stream-ordered on ``stream`` (default:
    torch's current stream).  Rays that travel together should be neighbours: a wave takes 64 consecutive rays."""
    n = _tensor(rays, "rays", "int32", (None, 11)).shape[0]
    out = _out_tensor(out, (n, 3), "float32", rays.device)
    cnt_ptr = _count_ptr(ray_count)
    _capi.check(_capi.amd_lib().rt_trace_rays(scene._h, _p(rays), n, int(max_depth), float(contribution),
                                              _p(out), cnt_ptr, _stream_ptr(stream)))
    return out


def trace_rays_numpy(scene: Scene, rays_np, max_depth: int, contribution: float = 1.0):
    """Host-buffer convenience (rt_trace_rays_host, synchronous): rays as a RAY_DTYPE structured array or an (N, 11) array of 4-byte
    words; returns (rgb[N, 3] float32, casts)."""
    a = _host_records(rays_np, RAY_DTYPE, 11, "rays")
    rgb = np.zeros((a.shape[0], 3), dtype=np.float32)
    casts = C.c_ulonglong(0)
    _capi.check(_capi.amd_lib().rt_trace_rays_host(scene._h, a.ctypes.data_as(C.c_void_p), a.shape[0], int(max_depth), float(contribution),
                                                   rgb.ctypes.data_as(C.c_void_p), C.byref(casts)))
    return rgb, int(casts.value)


# ---- hit queries: get_shade / get_reflect / get_refract on caller-supplied hits (include/rt_amd.h rt_shade_hits) ----

ESCAPED, INFINITE, TRAPPED = 0, 1, 2  # Refraction, main.rs:149-158 (HIT_NONE: the record was no hit)


def _hit_records(hits, name="hits"):
    return _tensor(hits.records if isinstance(hits, Hits) else hits, name, "int32", (None, 13))


def _hits_and_rays(hits, rays):
    records = _hit_records(hits)
    _tensor(rays, "rays", "int32", (None, 11))
    if rays.shape[0] != records.shape[0]:
        raise ValueError("hits and rays must have one record each per hit: rays[i] is the ray that produced hits[i]")
    return records, records.shape[0]


def shade_hits(scene: Scene, hits, rays, out=None, ray_count=None, stream=None):
    """get_shade (src/main.rs:407-464) for every hit: ``hits`` is a Hits or its (N, 13) int32 CUDA record tensor (what cast_rays
    returns), ``rays`` the (N, 11) rt_ray records that produced them (Hit.ray).  Returns ``out``, an (N, 3) float32 CUDA tensor
    (allocated if None) with get_shade's value bit for bit; a record that is no hit gives black.  ``ray_count``: a 1-element int64 CUDA
    tensor that the shadow casts are added to.  Stream-ordered on ``stream`` (default: torch's current stream)."""
    records, n = _hits_and_rays(hits, rays)
    out = _out_tensor(out, (n, 3), "float32", records.device)
    _capi.check(_capi.amd_lib().rt_shade_hits(scene._h, _p(records), _p(rays), n,
                                              _p(out), _count_ptr(ray_count), _stream_ptr(stream)))
    return out


def reflect_rays(hits, rays, out=None, stream=None):
    """get_reflect (src/main.rs:328-341) for every hit: returns ``out``, an (N, 11) int32 CUDA tensor of rt_ray records (allocated if
    None) that cast_rays / trace_rays take as they are; a record that is no hit gives an all-zero ray.  Needs no scene."""
    records, n = _hits_and_rays(hits, rays)
    out = _out_tensor(out, (n, 11), "int32", records.device)
    _capi.check(_capi.amd_lib().rt_reflect_rays(_p(records), _p(rays), n, _p(out),
                                                _stream_ptr(stream)))
    return out


def _refractions(out, n, device):
    """``out`` if the caller gave one — a Refractions of n records, its three tensors checked — or a new one on ``device``"""
    if out is None:
        return Refractions(_new((n,), "int32", device), _new((n,), "float32", device), _new((n, 11), "int32", device))
    _tensor(out.kind, "out.kind", "int32", (n,))
    _tensor(out.travel, "out.travel", "float32", (n,))
    _tensor(out.rays, "out.rays", "int32", (n, 11))
    return out


class Refractions:
    """What refract_rays returns: ``kind`` (N,) int32 — ESCAPED, INFINITE, TRAPPED, or HIT_NONE for a record that was no hit —,
    ``travel`` (N,) float32 (travel_distance where escaped, else 0) and ``rays`` (N, 11) int32 rt_ray records (escape_ray where
    escaped, else zero words)."""

    def __init__(self, kind, travel, rays):
        self.kind, self.travel, self.rays = kind, travel, rays

    @property
    def escaped(self):
        """bool mask: Refraction::Escaped."""
        return self.kind == ESCAPED

    def __len__(self):
        return self.kind.shape[0]


def refract_rays(scene: Scene, hits, rays, max_distance: float = 100.0, ray_count=None, stream=None, out=None) -> Refractions:
    """get_refract (src/main.rs:343-405) for every hit, the walk through the glass: 1 to 11 casts each.  Returns a Refractions
    (``out``, a Refractions of this size to write into, or a new one); ``ray_count``: a 1-element int64 CUDA tensor that those casts
    are added to."""
    records, n = _hits_and_rays(hits, rays)
    out = _refractions(out, n, records.device)
    _capi.check(_capi.amd_lib().rt_refract_rays(scene._h, _p(records), _p(rays), n, float(max_distance), _p(out.kind), _p(out.travel),
                                                _p(out.rays), _count_ptr(ray_count), _stream_ptr(stream)))
    return out


def shade_hits_numpy(scene: Scene, hits_np, rays_np):
    """Host-buffer convenience (rt_shade_hits_host, synchronous): hits as a HIT_DTYPE array or (N, 13) 4-byte words, rays as a RAY_DTYPE
    array or (N, 11) words; returns (rgb[N, 3] float32, shadow casts)."""
    h, r = _host_records(hits_np, HIT_DTYPE, 13, "hits"), _host_records(rays_np, RAY_DTYPE, 11, "rays")
    if h.shape[0] != r.shape[0]:
        raise ValueError("hits and rays must have one record each per hit")
    rgb = np.zeros((h.shape[0], 3), dtype=np.float32)
    casts = C.c_ulonglong(0)
    _capi.check(_capi.amd_lib().rt_shade_hits_host(scene._h, h.ctypes.data_as(C.c_void_p), r.ctypes.data_as(C.c_void_p), h.shape[0],
                                                   rgb.ctypes.data_as(C.c_void_p), C.byref(casts)))
    return rgb, int(casts.value)


def refract_rays_numpy(scene: Scene, hits_np, rays_np, max_distance: float = 100.0):
    """Host-buffer convenience (rt_refract_rays_host, synchronous): returns (kind[N] int32, travel[N] float32, escape rays as a
    RAY_DTYPE array, casts)."""
    h, r = _host_records(hits_np, HIT_DTYPE, 13, "hits"), _host_records(rays_np, RAY_DTYPE, 11, "rays")
    if h.shape[0] != r.shape[0]:
        raise ValueError("hits and rays must have one record each per hit")
    n = h.shape[0]
    kind = np.zeros(n, dtype=np.int32)
    travel = np.zeros(n, dtype=np.float32)
    escape = np.zeros(n, dtype=RAY_DTYPE)
    casts = C.c_ulonglong(0)
    _capi.check(_capi.amd_lib().rt_refract_rays_host(scene._h, h.ctypes.data_as(C.c_void_p), r.ctypes.data_as(C.c_void_p), n, float(max_distance),
                                                     kind.ctypes.data_as(C.c_void_p), travel.ctypes.data_as(C.c_void_p),
                                                     escape.ctypes.data_as(C.c_void_p), C.byref(casts)))
    return kind, travel, escape, int(casts.value)


def _sample_outputs(accum, samples, valid, n_epochs, n):
    """the three optional outputs of the stochastic queries on n rays: accum (n, 3) f32, samples (n_epochs, n, 3) f32, valid (n_epochs, n) u8"""
    _tensor(accum, "accum", "float32", (n, 3), optional=True)
    _tensor(samples, "samples", "float32", (n_epochs, n, 3), optional=True)
    _tensor(valid, "valid", "uint8", (n_epochs, n), optional=True)


def trace_rays_distributed(scene: Scene, rays, max_depth: int, rng: Rng, n_epochs: int = 1, accum=None, samples=None, valid=None,
                           ray_count=None, stream=None):
    """`n_epochs` samples of distributed_ray_trace (src/main.rs:521-614) per ray of an (N, 11) int32 CUDA tensor of rt_ray records, ray i
    on generator i of ``rng`` (N generators: Rng.seeded, or a frame's Rng of N pixels), whose stream continues (rt_trace_rays_distributed).

    accum   (N, 3) f32 CUDA tensor or None: the samples that pass the filter of main.rs:1157-1160 are added in epoch order.
    samples (n_epochs, N, 3) f32 / valid (n_epochs, N) u8 CUDA tensors or None: raw samples + filter flags.
    ray_count: a 1-element int64 CUDA tensor that the World::cast count is added to.  At least one of accum / samples.
    """
    n = _tensor(rays, "rays", "int32", (None, 11)).shape[0]
    _sample_outputs(accum, samples, valid, n_epochs, n)
    cnt_ptr = _count_ptr(ray_count)
    _capi.check(_capi.amd_lib().rt_trace_rays_distributed(scene._h, _p(rays), n, int(max_depth), rng._h, int(n_epochs),
                                                          _p(accum), _p(samples), _p(valid), cnt_ptr, _stream_ptr(stream)))
    return accum if accum is not None else samples


def trace_rays_distributed_numpy(scene: Scene, rays_np, max_depth: int, rng: Rng, n_epochs: int, img: np.ndarray) -> int:
    """Host-buffer convenience (rt_trace_rays_distributed_host, synchronous): rays as a RAY_DTYPE structured array or an (N, 11) array
    of 4-byte words; `n_epochs` samples per ray are added into ``img`` ((N, 3) f32, in place).  Returns the cast count."""
    a = _host_records(rays_np, RAY_DTYPE, 11, "rays")
    if not (isinstance(img, np.ndarray) and img.dtype == np.float32 and img.flags.c_contiguous and img.shape == (a.shape[0], 3)):
        raise ValueError("expected a contiguous (N, 3) float32 array")
    casts = C.c_ulonglong(0)
    _capi.check(_capi.amd_lib().rt_trace_rays_distributed_host(scene._h, a.ctypes.data_as(C.c_void_p), a.shape[0], int(max_depth), rng._h,
                                                               int(n_epochs), img.ctypes.data_as(C.c_void_p), C.byref(casts)))
    return int(casts.value)


# ---- scatter queries: weighted_select / scatter_hit on caller-supplied hits (include/rt_amd.h rt_scatter_hits) ----

DIFFUSE, REFLECTION, REFRACTION = 0, 1, 2  # ScatterType, main.rs:533-537 (HIT_NONE: the record was no hit)


class Scatters:
    """What scatter_hits returns: ``type`` (N,) int32 — DIFFUSE, REFLECTION, REFRACTION, or HIT_NONE for a record that was no hit —,
    ``rays`` (N, 11) int32 rt_ray records (scattered_hit.ray: with the hits they feed reflect_rays / refract_rays / shade_hits as
    they are) and ``cosine`` (N,) float32 (-hit.normal . new_dir)."""

    def __init__(self, type, rays, cosine):
        self.type, self.rays, self.cosine = type, rays, cosine

    @property
    def alive(self):
        """bool mask: the level goes on — a valid record that does not meet the reference's ``cosine <= 0`` (black).  Spelt as that
        test's negation, so a NaN cosine counts as alive, as in the reference."""
        return (self.type != HIT_NONE) & ~(self.cosine <= 0)

    def __len__(self):
        return self.type.shape[0]


def _rng_of(rng):
    if not isinstance(rng, Rng):
        raise ValueError("rng must be an Rng")
    return rng


def scatter_hits(scene: Scene, hits, rays, rng: Rng, rng_index=None, stream=None, out=None) -> Scatters:
    """The three draws of one level of distributed_ray_trace (src/main.rs:533-554) for every hit: weighted_select, then scatter_hit,
    record i on generator ``rng_index[i]`` of ``rng`` — or generator i when ``rng_index`` is None, and then ``rng`` must hold exactly
    N generators.  ``rng_index``: an (N,) int32 CUDA tensor; an index at or beyond ``rng.count`` (-1, say) makes the record "no hit".
    A record that is no hit draws nothing: its generator does not move.  Returns a Scatters (``out``, a Scatters of this size to write
    into, or a new one).  Calls on one Rng must be serialised."""
    records, n = _hits_and_rays(hits, rays)
    _rng_of(rng)
    if _tensor(rng_index, "rng_index", "int32", (n,), optional=True) is None and n != rng.count:
        raise ValueError("without rng_index the Rng must hold one generator per record")
    if out is None:
        dev = records.device
        out = Scatters(_new((n,), "int32", dev), _new((n, 11), "int32", dev), _new((n,), "float32", dev))
    _tensor(out.type, "out.type", "int32", (n,))
    _tensor(out.rays, "out.rays", "int32", (n, 11))
    _tensor(out.cosine, "out.cosine", "float32", (n,))
    _capi.check(_capi.amd_lib().rt_scatter_hits(scene._h, _p(records), _p(rays), n, rng._h, _p(rng_index), _p(out.type), _p(out.rays),
                                                _p(out.cosine), _stream_ptr(stream)))
    return out


def scatter_factors(scene: Scene, hits, rays, types, next_rays, travel, out=None, stream=None):
    """The factor of one level once its next ray is known (src/main.rs:566-570, 585-589, 605): get_diffuse (DIFFUSE) or get_specular
    (REFLECTION) of the hit's material towards ``next_rays[i]``'s direction seen from ``-rays[i]``'s, or opaque_decay ** travel[i] in all
    three channels (REFRACTION); any other type or a record that is no hit gives 0.  ``types``: (N,) int32, ``next_rays``: (N, 11)
    int32 rt_ray records, ``travel``: (N,) float32, all CUDA.  Returns ``out``, an (N, 3) float32 CUDA tensor (allocated if None)."""
    records, n = _hits_and_rays(hits, rays)
    _tensor(types, "types", "int32", (n,))
    _tensor(next_rays, "next_rays", "int32", (n, 11))
    _tensor(travel, "travel", "float32", (n,))
    out = _out_tensor(out, (n, 3), "float32", records.device)
    _capi.check(_capi.amd_lib().rt_scatter_factors(scene._h, _p(records), _p(rays), _p(types), _p(next_rays), _p(travel), n, _p(out),
                                                   _stream_ptr(stream)))
    return out


def scatter_hits_numpy(scene: Scene, hits_np, rays_np, rng: Rng, rng_index=None):
    """Host-buffer convenience (rt_scatter_hits_host, synchronous; the Rng stays on the device): returns (type[N] int32, scattered rays
    as a RAY_DTYPE array, cosine[N] float32)."""
    h, r = _host_records(hits_np, HIT_DTYPE, 13, "hits"), _host_records(rays_np, RAY_DTYPE, 11, "rays")
    if h.shape[0] != r.shape[0]:
        raise ValueError("hits and rays must have one record each per hit")
    n = h.shape[0]
    _rng_of(rng)
    idx = None
    if rng_index is not None:
        idx = _host_column(rng_index, ("iu", "32-bit integers"), n, "rng_index")
    elif n != rng.count:
        raise ValueError("without rng_index the Rng must hold one generator per record")
    type_ = np.zeros(n, dtype=np.int32)
    out = np.zeros(n, dtype=RAY_DTYPE)
    cosine = np.zeros(n, dtype=np.float32)
    _capi.check(_capi.amd_lib().rt_scatter_hits_host(scene._h, h.ctypes.data_as(C.c_void_p), r.ctypes.data_as(C.c_void_p), n, rng._h,
                                                     None if idx is None else idx.ctypes.data_as(C.c_void_p),
                                                     type_.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p),
                                                     cosine.ctypes.data_as(C.c_void_p)))
    return type_, out, cosine


def scatter_factors_numpy(scene: Scene, hits_np, rays_np, types, next_rays_np, travel):
    """Host-buffer convenience (rt_scatter_factors_host, synchronous): returns rgb[N, 3] float32."""
    h, r = _host_records(hits_np, HIT_DTYPE, 13, "hits"), _host_records(rays_np, RAY_DTYPE, 11, "rays")
    nx = _host_records(next_rays_np, RAY_DTYPE, 11, "next_rays")
    n = h.shape[0]
    if r.shape[0] != n or nx.shape[0] != n:
        raise ValueError("hits, rays and next_rays must have one record each per hit")
    t = _host_column(types, ("iu", "32-bit integers"), n, "types")
    tr = _host_column(travel, ("f", "float32"), n, "travel")
    rgb = np.zeros((n, 3), dtype=np.float32)
    _capi.check(_capi.amd_lib().rt_scatter_factors_host(scene._h, h.ctypes.data_as(C.c_void_p), r.ctypes.data_as(C.c_void_p),
                                                        t.ctypes.data_as(C.c_void_p), nx.ctypes.data_as(C.c_void_p),
                                                        tr.ctypes.data_as(C.c_void_p), n, rgb.ctypes.data_as(C.c_void_p)))
    return rgb


# ---- the two calls every loop is made of: stable selection and indexed casts (include/rt_amd.h rt_select_records, rt_cast_rays_indexed) ----


def select_records(flags, index=None, count=None, stream=None):
    """Stable selection on the device (rt_select_records): ``flags`` is an (N,) uint8 CUDA tensor; returns (index, count) — ``index``
    an (N,) int32 CUDA tensor whose first ``count[0]`` entries are the ascending i with flags[i] != 0 (the rest unspecified), ``count``
    a 1-element int32 CUDA tensor that stays on the device.  The first call on a stream allocates 4 KB of scratch and must not be
    captured into a graph.  N == 0 leaves ``count`` as it was."""
    n = _tensor(flags, "flags", "uint8", (None,)).shape[0]
    index = _out_tensor(index, (n,), "int32", flags.device, "index")
    count = _out_tensor(count, (1,), "int32", flags.device, "count")
    _capi.check(_capi.amd_lib().rt_select_records(_p(flags), n, _p(index), _p(count), _stream_ptr(stream)))
    return index, count


def cast_rays_indexed(scene: Scene, rays, index, count, out, max_count=None, ray_count=None, stream=None):
    """World::cast of the rays an index list names (rt_cast_rays_indexed): for j < min(count[0], max_count), out[index[j]] =
    cast(rays[index[j]]), bit for bit cast_rays' record; records of ``out`` ((N, 13) int32, required) that are not named are not
    written, an index >= N is skipped.  ``index``: an (M,) int32 CUDA tensor, ``count``: a 1-element int32 CUDA tensor (what
    select_records returns), ``max_count``: the host's bound on the list's length (default M).  ``ray_count``: a 1-element int64 CUDA
    tensor that the casts made are added to."""
    n = _tensor(rays, "rays", "int32", (None, 11)).shape[0]
    _tensor(out, "out", "int32", (n, 13))
    _tensor(index, "index", "int32", (None,))
    _tensor(count, "count", "int32", (1,))
    m = index.shape[0] if max_count is None else int(max_count)
    if not 0 <= m <= index.shape[0]:
        raise ValueError("max_count must not exceed the length of index")
    _capi.check(_capi.amd_lib().rt_cast_rays_indexed(scene._h, _p(rays), n, _p(index), _p(count), m, _p(out), _count_ptr(ray_count),
                                                     _stream_ptr(stream)))
    return out
