"""Path queries (include/rt_amd.h "path queries"): the inner step of a path tracer on caller-supplied hits.

lobes.glossy_hits is one stochastic bounce with the Whitted recursion behind it.  Here a path is a 32-byte record that carries its
throughput from bounce to bounce; ``advance`` does between two casts what materials.material_hits, lobes.rays,
materials.probe_surfaces, lobes.mis_weigh and environment.fold do in five launches — one direction from the hit's own lobes, the Phong
terms along it, the throughput over the direction's density — deposits the light the vertex sends back, and ends paths by Russian
roulette on the device; ``begin`` makes the records and ``resolve`` adds the mean of a pixel's paths to its slot.

    begin / advance / resolve                       rt_path_begin / rt_path_advance / rt_path_resolve
    begin_numpy / advance_numpy / resolve_numpy     the CPU forms (rt_path_begin_cpu, rt_path_advance_cpu and rt_path_resolve_cpu of
                                                    librt_host.so): the device's bits
    branch / transmit                               rt_path_branch / rt_path_transmit ("transmission queries"): the choice between a
                                                    vertex's lobes and its glass, and a finished walk folded into the record
    branch_numpy / transmit_numpy                   their CPU forms (rt_path_branch_cpu and rt_path_transmit_cpu): the device's bits
    connect / settle / weigh_escape                 rt_path_connect / rt_path_settle / rt_path_weigh_escape ("connection queries"):
                                                    next-event estimation of the sky — a direction from the environment's table at
                                                    every vertex, weighed against the lobes, its shadow cast settled into the
                                                    radiance, and the sky a lobe ray escaped to weighed the other way round
    connect_numpy / settle_numpy / weigh_escape_numpy
                                                    their CPU forms (rt_path_connect_cpu, rt_path_settle_cpu and
                                                    rt_path_weigh_escape_cpu): the device's bits
    connect_lights / settle_lights                  rt_path_connect_lights / rt_path_settle_lights ("light-connection queries"): next-event
                                                    estimation of the scene's own lights — one light and one point on it per vertex,
                                                    its terms times the throughput over the chance of the choice, its shadow cast
                                                    settled by get_shade's rule; light_seed: the seed arealights.rays draws the same
                                                    points with
    connect_lights_numpy / settle_lights_numpy      their CPU forms (rt_path_connect_lights_cpu and rt_path_settle_lights_cpu): the
                                                    device's bits
    trace_paths                                   begin -> per bounce: shade_hits -> environment.lookup -> advance -> select_records
                                                    -> cast_rays_indexed -> resolve — written from the public calls alone: to be
                                                    copied and changed

Arrays are sample-major: path s * N + i is sample s of root i.  The weighting is environment.fold's: the Phong terms are the
reference's, not normalised, so a white diffuse surface under a constant sky L returns pi * L.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi
from ._args import (_aligned_bytes, _below_2_32, _host, _host_records, _new, _on_stream, _out_tensor, _p, _room, _samples, _stream_ptr, _tensor, _void,
                    _zeroed_out)
from ._capi import Light, SceneDesc
from ._opened import LightWorkspace, _light_range, refract_step, shade_hits_by_light
from ._queries import HIT_DTYPE, HIT_NONE, RAY_DTYPE, _hit_records, cast_rays_indexed, select_records, shade_hits
from ._world import Scene, World
from .environment import TABLE_HEADER_BYTES, Environment, _environment, _host_environment, lookup, table_bytes
from .lobes import BALANCE, POWER, _host_surfaces  # RT_MIS_BALANCE / RT_MIS_POWER: connect's and weigh_escape's heuristic

SHADING, GEOMETRIC = 0, 1  # RT_HEMISPHERE_SHADING / RT_HEMISPHERE_GEOMETRIC
ALIVE, SPECULAR, ESCAPED, ROULETTE, DARK, TRANSMITTED, TRAPPED = 1, 2, 4, 8, 16, 32, 64  # RT_PATH_*
MAX_DISTANCE = 100.0  # what the reference passes to get_refract (main.rs:502): the walk's max_distance in trace_paths
NO_ROULETTE = 0xFFFFFFFF  # an rr_start no bounce reaches
PATH_WORDS = 8
SAMPLE_SHIFT = 24  # rt_path.bounce: the sample index above, the bounces taken below
PATH_DTYPE = np.dtype([("beta", "<f4", (3,)), ("pdf", "<f4"), ("root", "<u4"), ("id", "<u4"), ("bounce", "<u4"), ("flags", "<u4")])
assert PATH_DTYPE.itemsize == 4 * PATH_WORDS


def begin(n: int, spp: int, ids=None, out_paths=None, out_radiance=None, device="cuda", stream=None):
    """rt_path_begin: ``spp`` fresh paths for each of ``n`` roots.  Returns (paths, radiance): ``paths`` (S*N, 8) int32 CUDA, the
    rt_path records (PATH_DTYPE on the host) — beta 1, pdf +0, root i, id ``ids[i]`` ((N,) int32 or None: i), bounce s << 24, flags
    ALIVE; ``radiance`` (S*N, 3) float32, zeroed.  Both are allocated on ``device`` if not given."""
    n, spp = int(n), _samples(spp)
    if n < 0:
        raise ValueError("n must not be negative")
    _tensor(ids, "ids", "int32", (n,), optional=True)
    if ids is not None:
        device = ids.device
    with _on_stream(stream):
        out_paths = _out_tensor(out_paths, (spp * n, PATH_WORDS), "int32", device, "out_paths")
        out_radiance = _out_tensor(out_radiance, (spp * n, 3), "float32", device, "out_radiance")
    _capi.check(_capi.amd_lib().rt_path_begin(n, spp, _p(ids), _p(out_paths), _p(out_radiance), _stream_ptr(stream)))
    return out_paths, out_radiance


def _listed(m, paths, index, count):
    """the record tensor and the list pair of a listed call, checked: (index, count) as the C call takes them"""
    _tensor(paths, "paths", "int32", (m, PATH_WORDS))
    _tensor(index, "index", "int32", (m,), optional=True)  # the call reads up to min(count, M) entries
    _tensor(count, "count", "int32", (1,), optional=index is None)
    return _p(index), (_p(count) if index is not None else None)


def _asks_out(out_asks, m, dev, stream):
    """the asks of a connection: slots that are not listed or not alive are not touched, so a new tensor is zeroed here"""
    if out_asks is None:
        with _on_stream(stream):
            out_asks = _new((m,), "uint8", dev).zero_()
    return _tensor(out_asks, "out_asks", "uint8", (m,))


def advance(scene: Scene, paths, hits, incoming, radiance, emitted=None, index=None, count=None, seed: int = 0, normal_kind: int = SHADING,
            rr_start: int = 3, rr_floor: float = 0.05, last: bool = False, out_rays=None, out_alive=None, stream=None):
    """rt_path_advance: one bounce of the listed paths.  ``paths`` (M, 8) int32, ``hits`` (a Hits or its (M, 13) int32 records: the
    paths' vertices), ``incoming`` (M, 11) int32 (the rays that found them), ``radiance`` (M, 3) float32 and ``emitted`` ((M, 3)
    float32 or None: what each vertex sends back, shade_hits' or the sky's).  ``index`` ((M,) int32) and ``count`` ((1,) int32), what
    select_records returns, list the slots to advance; None: all M.  Per listed live path: radiance += beta * emitted; a "no hit"
    vertex ends it (ESCAPED); ``last`` ends the rest (flags 0); else one direction from the hit's lobes (lobes.rays' for spp 1, UNIFORM,
    the path's id and sample, seed + 0x9e3779b9 * bounce), beta *= (diffuse (1 - shiness) + specular shiness) / pdf, DARK where that
    is not positive, and from bounce ``rr_start`` on Russian roulette with survival max(beta) clamped to [``rr_floor``, 1] (ROULETTE;
    NO_ROULETTE switches it off).  Returns (rays, alive): ``out_rays`` (M, 11) int32, the continuation ray of a survivor — from the
    vertex along the direction drawn, face BOTH, the vertex's own primitive excluded for both faces: its cast finds the path's next
    vertex, the nearest surface whichever way it faces (lobes.rays' ray, face BACK, is an occlusion query) — and zero words for a
    path that ended, and ``out_alive`` (M,) uint8.  ``paths`` and ``radiance`` are updated in place, and so is ``hits``: a path that
    ended leaves a "no hit" record.  Slots that are not listed or not alive are not touched in any of them."""
    records = _hit_records(hits)
    m, dev = records.shape[0], records.device
    index_p, count_p = _listed(m, paths, index, count)
    _tensor(incoming, "incoming", "int32", (m, 11))
    _tensor(radiance, "radiance", "float32", (m, 3))
    _tensor(emitted, "emitted", "float32", (m, 3), optional=True)
    out_rays = _out_tensor(out_rays, (m, 11), "int32", dev, "out_rays")
    out_alive = _out_tensor(out_alive, (m,), "uint8", dev, "out_alive")
    _capi.check(_capi.amd_lib().rt_path_advance(scene._h, _p(paths), m, index_p, count_p, _p(records), _p(incoming),
                                                _p(emitted), int(seed) & 0xFFFFFFFF, int(normal_kind), int(rr_start) & 0xFFFFFFFF, float(rr_floor),
                                                int(bool(last)), _p(radiance), _p(out_rays), _p(out_alive), _stream_ptr(stream)))
    return out_rays, out_alive


def resolve(radiance, n: int, spp: int, out=None, root=None, stream=None):
    """rt_path_resolve: the mean over the ``spp`` samples of each of ``n`` roots of ``radiance`` ((S*N, 3) float32), the samples added
    in ascending order, ADDED to ``out`` ((R, 3) float32; None: a new, zeroed (N, 3) tensor) at slot ``root[i]`` ((N,) int32, distinct
    and below R) or i.  Returns ``out``."""
    n, spp = int(n), _samples(spp)
    _tensor(radiance, "radiance", "float32", (spp * n, 3))
    _tensor(root, "root", "int32", (n,), optional=True)
    if out is None or root is None:
        out = _zeroed_out(out, n, radiance.device, stream)
    else:
        _tensor(out, "out", "float32", (None, 3))
    _capi.check(_capi.amd_lib().rt_path_resolve(_p(radiance), n, spp, _p(root), _p(out), _stream_ptr(stream)))
    return out


# ---- transmission (include/rt_amd.h "transmission queries") ----

def branch(scene: Scene, paths, hits, incoming, index=None, count=None, seed: int = 0, last: bool = False, out_lobe=None, out_transmit=None,
           out_walk_rays=None, out_kind=None, out_travel=None, out_casts=None, out_walk_flags=None, stream=None):
    """rt_path_branch: per listed live path the choice between the vertex's lobes and its glass — it transmits iff the vertex is a hit
    and u_4 < its material's transparency, u_4 from the path's id and sample, seed + 0x9e3779b9 * bounce and a stream of its own — and
    for a path that transmits refract_enter's state of a walk that has cast nothing.  ``paths`` (M, 8) int32, ``hits`` (a Hits or its
    (M, 13) int32 records), ``incoming`` (M, 11) int32; ``index`` / ``count``: advance's list.  Returns (lobe, transmit, walk_rays, kind,
    travel, casts, walk_flags): ``lobe`` and ``transmit`` (M,) uint8, exactly one of them 1 for a listed live path — the operands of
    select_records for advance and for transmit —, and the five arrays of refract_enter, which hold a finished walk (kind HIT_NONE, flag
    0) wherever nothing walks.  ``last``: a transmitting path ends here (flags 0, both bytes 0, its hit "no hit").  Slots that are not
    listed are not touched."""
    records = _hit_records(hits)
    m, dev = records.shape[0], records.device
    index_p, count_p = _listed(m, paths, index, count)
    _tensor(incoming, "incoming", "int32", (m, 11))
    out_lobe = _out_tensor(out_lobe, (m,), "uint8", dev, "out_lobe")
    out_transmit = _out_tensor(out_transmit, (m,), "uint8", dev, "out_transmit")
    out_walk_rays = _out_tensor(out_walk_rays, (m, 11), "int32", dev, "out_walk_rays")
    out_kind = _out_tensor(out_kind, (m,), "int32", dev, "out_kind")
    out_travel = _out_tensor(out_travel, (m,), "float32", dev, "out_travel")
    out_casts = _out_tensor(out_casts, (m,), "int32", dev, "out_casts")
    out_walk_flags = _out_tensor(out_walk_flags, (m,), "uint8", dev, "out_walk_flags")
    _capi.check(_capi.amd_lib().rt_path_branch(scene._h, _p(paths), m, index_p, count_p, _p(records), _p(incoming), int(seed) & 0xFFFFFFFF, int(bool(last)),
                                               _p(out_lobe), _p(out_transmit), _p(out_walk_rays), _p(out_kind), _p(out_travel), _p(out_casts),
                                               _p(out_walk_flags), _stream_ptr(stream)))
    return out_lobe, out_transmit, out_walk_rays, out_kind, out_travel, out_casts, out_walk_flags


def transmit(scene: Scene, paths, hits, kind, travel, escape, walk_flags, index=None, count=None, seed: int = 0, rr_start: int = 3,
             rr_floor: float = 0.05, out_rays=None, out_alive=None, stream=None):
    """rt_path_transmit: the finished walk of each listed live path folded into its record.  ``kind`` (M,) int32, ``travel`` (M,)
    float32 and ``escape`` (M, 11) int32 as refract_step left them, ``hits`` still the vertices the paths entered the glass at.  An
    ESCAPED walk: beta *= opaque_decay ** travel, then advance's own tail (DARK, and from bounce ``rr_start`` on its roulette), and the
    survivor goes on along the escape ray with pdf +0, one bounce more and flags ALIVE | TRANSMITTED; anything else ends the path with
    TRAPPED.  Returns (rays, alive) as advance does; ``paths`` and ``hits`` are updated in place as advance updates them, and ``kind``
    and ``walk_flags`` of every listed slot are left HIT_NONE and 0.  Slots that are not listed are not touched."""
    records = _hit_records(hits)
    m, dev = records.shape[0], records.device
    index_p, count_p = _listed(m, paths, index, count)
    _tensor(kind, "kind", "int32", (m,))
    _tensor(travel, "travel", "float32", (m,))
    _tensor(escape, "escape", "int32", (m, 11))
    _tensor(walk_flags, "walk_flags", "uint8", (m,))
    out_rays = _out_tensor(out_rays, (m, 11), "int32", dev, "out_rays")
    out_alive = _out_tensor(out_alive, (m,), "uint8", dev, "out_alive")
    _capi.check(_capi.amd_lib().rt_path_transmit(scene._h, _p(paths), m, index_p, count_p, _p(records), _p(kind), _p(travel), _p(escape),
                                                 int(seed) & 0xFFFFFFFF, int(rr_start) & 0xFFFFFFFF, float(rr_floor), _p(out_rays), _p(out_alive),
                                                 _p(walk_flags), _stream_ptr(stream)))
    return out_rays, out_alive


# ---- connections (include/rt_amd.h "connection queries") ----

def _table(env, table, stream):
    if table is None:
        table = env.table(stream)
    return _tensor(table, "table", "uint8", (table_bytes(env.width, env.height),))


def connect(scene: Scene, env: Environment, paths, hits, incoming, index=None, count=None, seed: int = 0, normal_kind: int = SHADING,
            heuristic: int = BALANCE, last: bool = False, table=None, out_rays=None, out_asks=None, out_pending=None, stream=None):
    """rt_path_connect: per listed live path one direction drawn from the environment's table (``table``; None: env.table(stream)) at the
    path's vertex — environment.rays' sample for spp 1, UNIFORM, the path's id and sample and seed + 0x9e3779b9 * bounce, a stream apart
    from the lobe's — weighed against the vertex's own lobes (lobes.mis_weigh's weight of environment_pdf against lobes.pdf, one sample
    each) and multiplied by the throughput and the Phong terms.  To be called before advance, on the hits and rays advance will get.
    Returns (rays, asks, pending): ``out_asks`` (M,) uint8, 1 where environment.rays asks and the weight is finite; ``out_rays`` (M, 11)
    int32, the shadow ray where it asks and zero words where it does not; ``out_pending`` (M, 3) float32, what the path's radiance gains
    if that ray finds nothing — written where it asks.  ``last``, a "no hit" vertex and an environment without light ask nothing.  The
    record is read only.  Slots that are not listed or not alive are not touched: ``out_asks`` is zeroed here if not given."""
    env = _environment(env)
    records = _hit_records(hits)
    m, dev = records.shape[0], records.device
    index_p, count_p = _listed(m, paths, index, count)
    _tensor(incoming, "incoming", "int32", (m, 11))
    table = _table(env, table, stream)
    out_rays = _out_tensor(out_rays, (m, 11), "int32", dev, "out_rays")
    out_asks = _asks_out(out_asks, m, dev, stream)
    out_pending = _out_tensor(out_pending, (m, 3), "float32", dev, "out_pending")
    _capi.check(_capi.amd_lib().rt_path_connect(scene._h, C.byref(env.desc), _p(table), _p(paths), m, index_p, count_p, _p(records), _p(incoming),
                                                int(seed) & 0xFFFFFFFF, int(normal_kind), int(heuristic), int(bool(last)), _p(out_rays), _p(out_asks),
                                                _p(out_pending), _stream_ptr(stream)))
    return out_rays, out_asks, out_pending


def settle(paths, asks, pending, radiance, shadow_hits=None, index=None, count=None, stream=None):
    """rt_path_settle: per listed slot, radiance += pending where ``asks`` is set and the slot's record of ``shadow_hits`` ((M, 13) int32:
    what the cast of connect's rays found; None: nothing occludes) is "no hit" at all; the ask is cleared either way.  To be called after
    advance, so that a vertex's deposit is added before its connection.  ``paths`` is not read: a path advance ended still settles.
    Returns ``radiance``."""
    m = _tensor(asks, "asks", "uint8", (None,)).shape[0]
    index_p, count_p = _listed(m, paths, index, count)
    _tensor(shadow_hits, "shadow_hits", "int32", (m, 13), optional=True)
    _tensor(pending, "pending", "float32", (m, 3))
    _tensor(radiance, "radiance", "float32", (m, 3))
    _capi.check(_capi.amd_lib().rt_path_settle(_p(paths), m, index_p, count_p, _p(asks), _p(shadow_hits), _p(pending), _p(radiance), _stream_ptr(stream)))
    return radiance


def weigh_escape(env: Environment, paths, hits, incoming, emitted, index=None, count=None, heuristic: int = BALANCE, table=None, stream=None):
    """rt_path_weigh_escape: per listed live path whose vertex is "no hit" (environment.lookup's rule) and whose record holds the density
    of the direction it was drawn with — pdf finite and > 0 — ``emitted`` ((M, 3) float32: the sky lookup wrote) is multiplied by
    lobes.mis_weigh's weight of that density against environment_pdf of the incoming direction.  A pdf of +0 (a camera ray, a ray that
    left glass), a hit and an environment without light leave it alone.  To be called after lookup and before advance.  Returns
    ``emitted``."""
    env = _environment(env)
    records = _hit_records(hits)
    m, dev = records.shape[0], records.device
    index_p, count_p = _listed(m, paths, index, count)
    _tensor(incoming, "incoming", "int32", (m, 11))
    _tensor(emitted, "emitted", "float32", (m, 3))
    table = _table(env, table, stream)
    _capi.check(_capi.amd_lib().rt_path_weigh_escape(C.byref(env.desc), _p(table), _p(paths), m, index_p, count_p, _p(records), _p(incoming), int(heuristic),
                                                     _p(emitted), _stream_ptr(stream)))
    return emitted


# ---- light connections (include/rt_amd.h "light-connection queries") ----

NO_LIGHT = 0xFFFFFFFF  # ``chosen`` of a path that drew no light
BOUNCE_STEP, LIGHT_POINT_STREAM = 0x9E3779B9, 0x68E31DA4  # RT_PATH_BOUNCE_STEP / RT_LIGHT_CONNECT_POINT_STREAM


def _film_mix(v: int) -> int:
    v &= 0xFFFFFFFF
    v ^= v >> 16
    v = (v * 0x7FEB352D) & 0xFFFFFFFF
    v ^= v >> 15
    v = (v * 0x846CA68B) & 0xFFFFFFFF
    return v ^ (v >> 16)


def light_seed(seed: int, bounce: int) -> int:
    """The seed with which arealights.rays (spp 1, UNIFORM, the paths' ids, sample index s) and arealights.samples_numpy draw the points
    connect_lights draws at bounce ``bounce`` of a loop whose seed is ``seed``: film_mix((seed + 0x9e3779b9 * bounce) ^ 0x68e31da4)."""
    return _film_mix(((int(seed) + BOUNCE_STEP * int(bounce)) & 0xFFFFFFFF) ^ LIGHT_POINT_STREAM)


def connect_lights(scene: Scene, paths, hits, incoming, index=None, count=None, seed: int = 0, radii=None, weights=None, light_first: int = 0,
                   light_count=None, out_rays=None, out_asks=None, out_pending=None, out_reach=None, out_chosen=None, stream=None):
    """rt_path_connect_lights: per listed live path one of the lights light_first .. light_first + light_count - 1 (default: every light
    from light_first on) — uniformly, or by ``weights`` ((L,) float32; one that is not > 0 counts as 0) — and one point on its sphere of
    radius ``radii[l]`` ((L,) float32 or None: points), both from the path's own hash streams for seed + 0x9e3779b9 * bounce; the light's
    Phong terms at the path's vertex times the throughput over the chance of the choice.  To be called before advance, on the hits and
    rays advance will get.  Returns (rays, asks, pending, reach, chosen): ``out_asks`` (M,) uint8, 1 where get_shade would cast towards
    that light; ``out_rays`` (M, 11) int32, the shadow ray where it asks and zero words where it does not; ``out_pending`` (M, 3)
    float32, what the path's radiance gains if the light is not occluded, and ``out_reach`` (M,) float32, the distance to the point
    (-1: a directional light without origin) — both written where it asks; ``out_chosen`` ((M,) int32 or None: not wanted, and None is
    returned) the light drawn, NO_LIGHT where none was.  The record is read only.  Slots that are not listed or not alive are not touched:
    ``out_asks`` is zeroed here if not given."""
    records = _hit_records(hits)
    m, dev = records.shape[0], records.device
    index_p, count_p = _listed(m, paths, index, count)
    _tensor(incoming, "incoming", "int32", (m, 11))
    first, lights = _light_range(scene, light_first, light_count)
    _tensor(radii, "radii", "float32", (lights,), optional=True)
    _tensor(weights, "weights", "float32", (lights,), optional=True)
    out_rays = _out_tensor(out_rays, (m, 11), "int32", dev, "out_rays")
    out_asks = _asks_out(out_asks, m, dev, stream)
    out_pending = _out_tensor(out_pending, (m, 3), "float32", dev, "out_pending")
    out_reach = _out_tensor(out_reach, (m,), "float32", dev, "out_reach")
    _tensor(out_chosen, "out_chosen", "int32", (m,), optional=True)
    _capi.check(_capi.amd_lib().rt_path_connect_lights(scene._h, _p(paths), m, index_p, count_p, _p(records), _p(incoming), first, lights, _p(radii),
                                                       _p(weights), int(seed) & 0xFFFFFFFF, _p(out_rays), _p(out_asks), _p(out_pending), _p(out_reach),
                                                       _p(out_chosen), _stream_ptr(stream)))
    return out_rays, out_asks, out_pending, out_reach, out_chosen


def settle_lights(paths, asks, shadow_rays, reach, pending, radiance, shadow_hits=None, index=None, count=None, stream=None):
    """rt_path_settle_lights: per listed slot, radiance += pending where ``asks`` is set, unless the slot's record of ``shadow_hits``
    ((M, 13) int32: what the cast of connect_lights' rays found; None: nothing occludes) is a hit and either ``reach`` is negative or the
    hit lies nearer to the ray's origin than ``reach`` — get_shade's rule; the ask is cleared either way.  To be called after advance, so
    that a vertex's deposit is added before its connection.  ``paths`` is not read: a path advance ended still settles.  Returns
    ``radiance``."""
    m = _tensor(asks, "asks", "uint8", (None,)).shape[0]
    index_p, count_p = _listed(m, paths, index, count)
    _tensor(shadow_rays, "shadow_rays", "int32", (m, 11))
    _tensor(shadow_hits, "shadow_hits", "int32", (m, 13), optional=True)
    _tensor(reach, "reach", "float32", (m,))
    _tensor(pending, "pending", "float32", (m, 3))
    _tensor(radiance, "radiance", "float32", (m, 3))
    _capi.check(_capi.amd_lib().rt_path_settle_lights(_p(paths), m, index_p, count_p, _p(asks), _p(shadow_rays), _p(shadow_hits), _p(reach), _p(pending),
                                                      _p(radiance), _stream_ptr(stream)))
    return radiance


# ---- the CPU forms ----

def _host_paths(paths, m=None):
    """a copy of the records as a PATH_DTYPE array; ``m``: how many there must be"""
    a = np.ascontiguousarray(paths)
    if a.dtype == PATH_DTYPE:
        a = a.reshape(-1).copy()
    elif a.ndim == 2 and a.shape[1] == PATH_WORDS and a.dtype.itemsize == 4:
        a = a.view(PATH_DTYPE).reshape(-1).copy()
    else:
        raise ValueError("paths: expected a PATH_DTYPE array or an (M, 8) array of 4-byte words")
    if m is not None and a.shape[0] != m:
        raise ValueError(f"paths: expected {m} records")
    return a


def _host_list(index, count, m):
    """(index, count) as the C forms take them: ``index`` padded to M entries that name nothing, ``count`` one u32"""
    if index is None:
        return None, None
    index = np.ascontiguousarray(index).reshape(-1)
    given = _host(index, np.uint32, index.shape, "index")[:m]
    padded = np.full(m, 0xFFFFFFFF, dtype=np.uint32)  # the C form reads up to min(count, M) entries: the rest name nothing
    padded[:given.shape[0]] = given
    return padded, np.array([given.shape[0] if count is None else int(count) & 0xFFFFFFFF], dtype=np.uint32)


def _host_shadow_hits(shadow_hits, m):
    """the shadow hits of a settlement as HIT_DTYPE records, or None: nothing occludes"""
    if shadow_hits is None:
        return None
    shadow_hits = _host_records(shadow_hits, HIT_DTYPE, 13, "shadow_hits")
    if shadow_hits.shape[0] != m:
        raise ValueError(f"shadow_hits: expected {m} records")
    return shadow_hits


def begin_numpy(n: int, spp: int, ids=None):
    """rt_path_begin_cpu: begin on the CPU, bit for bit.  Returns (paths — a PATH_DTYPE array of S*N records —, radiance (S*N, 3))."""
    n, spp = int(n), _samples(spp)
    ids = _host(ids, np.uint32, (n,), "ids", optional=True)
    paths, radiance = np.zeros(spp * n, dtype=PATH_DTYPE), np.full((spp * n, 3), np.nan, dtype=np.float32)
    _capi.check_host(_capi.host_lib().rt_path_begin_cpu(n, spp, _void(ids), _void(paths), _void(radiance)))
    return paths, radiance


def advance_numpy(surfaces, view, paths, radiance, emitted=None, index=None, count=None, seed: int = 0, normals=None, rr_start: int = 3,
                  rr_floor: float = 0.05, last: bool = False, dirs=None, alive=None):
    """rt_path_advance_cpu: what advance writes for paths whose vertices' materials are ``surfaces`` (materials.material_hits; valid 0:
    "no hit") seen from ``view`` ((M, 3) float32), bit for bit, on the CPU.  ``normals`` (M, 3) float32 or None: the N to draw about —
    None is the record's shading normal (SHADING); pass hit.normal for GEOMETRIC.  ``index`` (K,) and ``count`` (an int): the list, or
    None for all M.  Returns new arrays (paths, radiance, dirs (M, 3) float32, alive (M,) uint8): the direction of the next ray in
    place of the ray; ``dirs`` and ``alive`` as given (zeros if None) where a slot is not touched."""
    surfaces = _host_surfaces(surfaces)
    m = surfaces.shape[0]
    view = _host(view, np.float32, (m, 3), "view")
    normals = _host(normals, np.float32, (m, 3), "normals", optional=True)
    paths = _host_paths(paths, m)
    radiance = _host(radiance, np.float32, (m, 3), "radiance").copy()
    emitted = _host(emitted, np.float32, (m, 3), "emitted", optional=True)
    dirs = np.zeros((m, 3), dtype=np.float32) if dirs is None else _host(dirs, np.float32, (m, 3), "dirs").copy()
    alive = np.zeros(m, dtype=np.uint8) if alive is None else _host(alive, np.uint8, (m,), "alive").copy()
    index, count = _host_list(index, count, m)
    _capi.check_host(_capi.host_lib().rt_path_advance_cpu(_void(surfaces), _void(normals), _void(view), _void(paths), m, _void(index), _void(count),
                                                          _void(emitted), int(seed) & 0xFFFFFFFF, int(rr_start) & 0xFFFFFFFF, float(rr_floor),
                                                          int(bool(last)), _void(radiance), _void(dirs), _void(alive)))
    return paths, radiance, dirs, alive


def resolve_numpy(radiance, n: int, spp: int, rgb=None, root=None) -> np.ndarray:
    """rt_path_resolve_cpu: resolve on the CPU, bit for bit.  Returns a new array: ``rgb`` ((R, 3) float32; None: zeros (N, 3)) plus the
    roots' means."""
    n, spp = int(n), _samples(spp)
    radiance = _host(radiance, np.float32, (spp * n, 3), "radiance")
    root = _host(root, np.uint32, (n,), "root", optional=True)
    rgb = np.zeros((n, 3), dtype=np.float32) if rgb is None else np.ascontiguousarray(rgb, dtype=np.float32).copy()
    if rgb.ndim != 2 or rgb.shape[1] != 3 or (root is None and rgb.shape[0] < n) or (root is not None and n and int(root.max()) >= rgb.shape[0]):
        raise ValueError("rgb: expected an (R, 3) float32 array that holds every root's slot")
    _capi.check_host(_capi.host_lib().rt_path_resolve_cpu(_void(radiance), n, spp, _void(root), _void(rgb)))
    return rgb


def _start(a, dtype, shape, name, fill=0):
    return np.full(shape, fill, dtype=dtype) if a is None else _host(a, dtype, shape, name).copy()


def branch_numpy(surfaces, hits, incoming, paths, index=None, count=None, seed: int = 0, last: bool = False, lobe=None, transmit=None,
                 walk_rays=None, kind=None, travel=None, casts=None, walk_flags=None):
    """rt_path_branch_cpu: what branch writes for paths whose vertices are ``hits`` (HIT_DTYPE or (M, 13) words) with the materials
    ``surfaces`` (materials.material_hits; valid 0: "no hit") found by ``incoming`` (RAY_DTYPE or (M, 11) words), bit for bit, on the CPU.
    Returns new arrays (paths, lobe, transmit, walk_rays (M, 11) uint32, kind, travel, casts, walk_flags); the seven outputs as given
    (zeros, kind HIT_NONE, if None) where a slot is not touched.  No hit record is rewritten: the "no hit" of a path ``last`` ends is
    the device's alone."""
    surfaces = _host_surfaces(surfaces)
    m = surfaces.shape[0]
    hits = _host_records(hits, HIT_DTYPE, 13, "hits")
    incoming = _host_records(incoming, RAY_DTYPE, 11, "incoming")
    paths = _host_paths(paths)
    if not hits.shape[0] == incoming.shape[0] == paths.shape[0] == m:
        raise ValueError(f"hits, incoming, paths: expected {m} records each")
    lobe, transmit = _start(lobe, np.uint8, (m,), "lobe"), _start(transmit, np.uint8, (m,), "transmit")
    walk_rays = _start(walk_rays, np.uint32, (m, 11), "walk_rays")
    kind, travel = _start(kind, np.uint32, (m,), "kind", _capi.RT_HIT_NONE), _start(travel, np.float32, (m,), "travel")
    casts, walk_flags = _start(casts, np.uint32, (m,), "casts"), _start(walk_flags, np.uint8, (m,), "walk_flags")
    index, count = _host_list(index, count, m)
    _capi.check_host(_capi.host_lib().rt_path_branch_cpu(_void(surfaces), _void(hits), _void(incoming), _void(paths), m, _void(index), _void(count),
                                                         int(seed) & 0xFFFFFFFF, int(bool(last)), _void(lobe), _void(transmit), _void(walk_rays), _void(kind),
                                                         _void(travel), _void(casts), _void(walk_flags)))
    return paths, lobe, transmit, walk_rays, kind, travel, casts, walk_flags


def transmit_numpy(surfaces, paths, kind, travel, escape, index=None, count=None, seed: int = 0, rr_start: int = 3, rr_floor: float = 0.05,
                   rays=None, alive=None, walk_flags=None):
    """rt_path_transmit_cpu: what transmit writes, bit for bit, on the CPU.  Returns new arrays (paths, kind, rays (M, 11) uint32, alive,
    walk_flags); ``rays``, ``alive`` and ``walk_flags`` as given (zeros if None) where a slot is not touched."""
    surfaces = _host_surfaces(surfaces)
    m = surfaces.shape[0]
    paths = _host_paths(paths, m)
    kind = _host(kind, np.uint32, (m,), "kind").copy()
    travel = _host(travel, np.float32, (m,), "travel")
    escape = _host(escape, np.uint32, (m, 11), "escape")
    rays, alive = _start(rays, np.uint32, (m, 11), "rays"), _start(alive, np.uint8, (m,), "alive")
    walk_flags = _start(walk_flags, np.uint8, (m,), "walk_flags")
    index, count = _host_list(index, count, m)
    _capi.check_host(_capi.host_lib().rt_path_transmit_cpu(_void(surfaces), _void(paths), m, _void(index), _void(count), _void(kind), _void(travel),
                                                           _void(escape), int(seed) & 0xFFFFFFFF, int(rr_start) & 0xFFFFFFFF, float(rr_floor), _void(rays),
                                                           _void(alive), _void(walk_flags)))
    return paths, kind, rays, alive, walk_flags


def _host_table(texels, table):
    """the table in 8-byte-aligned host memory, held by the caller for as long as the call reads it"""
    size = TABLE_HEADER_BYTES + 8 * texels.shape[0] + 4 * texels.shape[0] * texels.shape[1]
    held = _aligned_bytes(size)
    held[:] = _host(table, np.uint8, (size,), "table")
    return held


def connect_numpy(surfaces, view, texels, table, paths, index=None, count=None, seed: int = 0, normals=None, heuristic: int = BALANCE,
                  last: bool = False, rotation: float = 0.0, scale: float = 1.0, dirs=None, asks=None, pending=None):
    """rt_path_connect_cpu: what connect writes for paths whose vertices' materials are ``surfaces`` (materials.material_hits; valid 0:
    "no hit") seen from ``view`` ((M, 3) float32) under the (H, W, 3) float32 image ``texels`` with ``table`` (environment.table_numpy),
    bit for bit, on the CPU.  ``normals`` (M, 3) float32 or None: the N of the lobes' density and of "leaves the surface" — None is the
    record's shading normal (SHADING); pass hit.normal for GEOMETRIC.  Returns new arrays (dirs (M, 3) float32, asks (M,) uint8, pending
    (M, 3) float32): the direction drawn in place of the ray — also where it does not ask, zeros where nothing was drawn —; each as given
    (zeros if None) where a slot is not touched, ``pending`` also where a slot does not ask."""
    surfaces = _host_surfaces(surfaces)
    m = surfaces.shape[0]
    view = _host(view, np.float32, (m, 3), "view")
    normals = _host(normals, np.float32, (m, 3), "normals", optional=True)
    texels, desc = _host_environment(texels, rotation, scale, 0)
    held = _host_table(texels, table)
    paths = _host_paths(paths, m)
    dirs, asks, pending = _start(dirs, np.float32, (m, 3), "dirs"), _start(asks, np.uint8, (m,), "asks"), _start(pending, np.float32, (m, 3), "pending")
    index, count = _host_list(index, count, m)
    _capi.check_host(_capi.host_lib().rt_path_connect_cpu(_void(surfaces), _void(normals), _void(view), C.byref(desc), _void(held), _void(paths), m,
                                                          _void(index), _void(count), int(seed) & 0xFFFFFFFF, int(heuristic), int(bool(last)), _void(dirs),
                                                          _void(asks), _void(pending)))
    return dirs, asks, pending


def settle_numpy(asks, pending, radiance, shadow_hits=None, index=None, count=None):
    """rt_path_settle_cpu: settle on the CPU, bit for bit.  ``shadow_hits``: HIT_DTYPE or (M, 13) words, or None: nothing occludes.
    Returns new arrays (asks, radiance)."""
    asks = np.ascontiguousarray(asks, dtype=np.uint8).reshape(-1).copy()
    m = asks.shape[0]
    pending = _host(pending, np.float32, (m, 3), "pending")
    radiance = _host(radiance, np.float32, (m, 3), "radiance").copy()
    shadow_hits = _host_shadow_hits(shadow_hits, m)
    paths = np.zeros(max(m, 1), dtype=PATH_DTYPE)  # not read
    index, count = _host_list(index, count, m)
    _capi.check_host(_capi.host_lib().rt_path_settle_cpu(_void(paths), m, _void(index), _void(count), _void(asks), _void(shadow_hits), _void(pending),
                                                         _void(radiance)))
    return asks, radiance


def weigh_escape_numpy(texels, table, paths, hits, incoming, emitted, index=None, count=None, heuristic: int = BALANCE, rotation: float = 0.0):
    """rt_path_weigh_escape_cpu: weigh_escape on the CPU, bit for bit.  ``hits``: HIT_DTYPE or (M, 13) words (the kind is read);
    ``incoming``: RAY_DTYPE or (M, 11) words (the direction is read).  Returns a new ``emitted``."""
    texels, desc = _host_environment(texels, rotation, 1.0, 0)
    held = _host_table(texels, table)
    paths = _host_paths(paths)
    m = paths.shape[0]
    hits = _host_records(hits, HIT_DTYPE, 13, "hits")
    incoming = _host_records(incoming, RAY_DTYPE, 11, "incoming")
    if not hits.shape[0] == incoming.shape[0] == m:
        raise ValueError(f"hits, incoming: expected {m} records each")
    emitted = _host(emitted, np.float32, (m, 3), "emitted").copy()
    index, count = _host_list(index, count, m)
    _capi.check_host(_capi.host_lib().rt_path_weigh_escape_cpu(C.byref(desc), _void(held), _void(paths), m, _void(index), _void(count), _void(hits),
                                                               _void(incoming), int(heuristic), _void(emitted)))
    return emitted


def connect_lights_numpy(surfaces, positions, view, lights, paths, index=None, count=None, seed: int = 0, radii=None, weights=None, light_first: int = 0,
                         light_count=None, aux=None, dirs=None, asks=None, pending=None, reach=None, chosen=None):
    """rt_path_connect_lights_cpu: what connect_lights writes for paths whose vertices' materials are ``surfaces`` (materials.material_hits;
    valid 0: "no hit") at ``positions`` ((M, 3) float32) seen from ``view`` ((M, 3) float32, minus the incoming direction), bit for bit,
    on the CPU.  ``lights``: a World, a SceneDesc or a sequence of Light — the scene's lights, indexed as the scene indexes them; ``aux``
    (n_lights, 2) float32 (cos_in, cos_out) or None: computed as the scene's are.  Returns new arrays (dirs (M, 3) float32, asks (M,)
    uint8, pending (M, 3) float32, reach (M,) float32, chosen (M,) uint32): the shadow ray's direction in place of the ray; each as
    given (zeros, ``chosen`` NO_LIGHT, if None) where a slot is not touched, ``pending`` and ``reach`` also where a slot does not ask."""
    if isinstance(lights, World):
        lights = lights.desc()
    if isinstance(lights, SceneDesc):
        desc = lights
        lights = [desc.lights[l] for l in range(desc.n_lights)]
    arr = (Light * max(len(lights), 1))(*lights)
    first = int(light_first)
    n_range = len(lights) - first if light_count is None else int(light_count)
    if first < 0 or n_range < 0 or first + n_range > len(lights):
        raise ValueError(f"lights {first} .. {first + n_range} of {len(lights)}")
    surfaces = _host_surfaces(surfaces)
    m = surfaces.shape[0]
    positions = _host(positions, np.float32, (m, 3), "positions")
    view = _host(view, np.float32, (m, 3), "view")
    radii = _host(radii, np.float32, (n_range,), "radii", optional=True)
    weights = _host(weights, np.float32, (n_range,), "weights", optional=True)
    aux = _host(aux, np.float32, (len(lights), 2), "aux", optional=True)
    paths = _host_paths(paths, m)
    dirs, asks, pending = _start(dirs, np.float32, (m, 3), "dirs"), _start(asks, np.uint8, (m,), "asks"), _start(pending, np.float32, (m, 3), "pending")
    reach, chosen = _start(reach, np.float32, (m,), "reach"), _start(chosen, np.uint32, (m,), "chosen", NO_LIGHT)
    index, count = _host_list(index, count, m)
    _capi.check_host(_capi.host_lib().rt_path_connect_lights_cpu(_void(surfaces), _void(positions), _void(view), C.cast(arr, C.c_void_p), _void(aux),
                                                                 _void(paths), m, _void(index), _void(count), first, n_range, _void(radii), _void(weights),
                                                                 int(seed) & 0xFFFFFFFF, _void(dirs), _void(asks), _void(pending), _void(reach),
                                                                 _void(chosen)))
    return dirs, asks, pending, reach, chosen


def settle_lights_numpy(asks, shadow_rays, reach, pending, radiance, shadow_hits=None, index=None, count=None):
    """rt_path_settle_lights_cpu: settle_lights on the CPU, bit for bit.  ``shadow_rays``: RAY_DTYPE or (M, 11) words; ``shadow_hits``:
    HIT_DTYPE or (M, 13) words, or None: nothing occludes.  Returns new arrays (asks, radiance)."""
    asks = np.ascontiguousarray(asks, dtype=np.uint8).reshape(-1).copy()
    m = asks.shape[0]
    shadow_rays = _host_records(shadow_rays, RAY_DTYPE, 11, "shadow_rays")
    if shadow_rays.shape[0] != m:
        raise ValueError(f"shadow_rays: expected {m} records")
    reach = _host(reach, np.float32, (m,), "reach")
    pending = _host(pending, np.float32, (m, 3), "pending")
    radiance = _host(radiance, np.float32, (m, 3), "radiance").copy()
    shadow_hits = _host_shadow_hits(shadow_hits, m)
    paths = np.zeros(max(m, 1), dtype=PATH_DTYPE)  # not read
    index, count = _host_list(index, count, m)
    _capi.check_host(_capi.host_lib().rt_path_settle_lights_cpu(_void(paths), m, _void(index), _void(count), _void(asks), _void(shadow_rays),
                                                                _void(shadow_hits), _void(reach), _void(pending), _void(radiance)))
    return asks, radiance


# ---- the loop ----

def _connection_buffers(k, device):
    """what a sky connection and a light connection both keep for ``k`` paths: (shadow rays, shadow hits, asks — zeroed —, pending, the
    second index, its count)"""
    return (_new((k, 11), "int32", device), _new((k, 13), "int32", device), _new((k,), "uint8", device).zero_(), _new((k, 3), "float32", device),
            _new((k,), "int32", device), _new((1,), "int32", device))


class Workspace:
    """The buffers of trace_paths, made once by workspace() so that a caller's loop allocates nothing: ``entries`` paths of room, about
    190 B each, ``pairs`` (path, light) pairs for the opened shade step (126 B each; 0: none), and ``walk`` paths of room for
    ``transmission`` (0: none), 159 B each: the lobe and transmit bytes (1 + 1), a second index (4; its count is 4 B once), the walk rays
    (44), the inside hits (52), kind, travel and casts (4 + 4 + 4), the walk flags (1) and the escape rays (44).  ``kind`` is filled with
    HIT_NONE and the walk flags and the escape rays with zeros, once, here.  ``connections`` paths of room for ``nee`` (0: none), 113 B
    each: the shadow rays (44), the shadow hits (52), the asks (1), the pending radiance (12) and a second index (4; its count is 4 B
    once).  The asks are zeroed once, here: settle leaves them so.  ``light_connections`` paths of room for ``light_nee`` (0: none), 117 B
    each and 4 B more with ``chosen``: buffers of their own, since a vertex's sky connection and its light connection are outstanding at
    once — the shadow rays (44), the shadow hits (52), the asks (1, zeroed once, here), the pending radiance (12), the reach (4) and a
    second index (4; its count is 4 B once), and optionally the light chosen (4)."""

    def __init__(self, entries: int, pairs: int, device, walk: int = 0, connections: int = 0, light_connections: int = 0, chosen: bool = False):
        self.entries, self.pairs, self.walk, self.connections = int(entries), int(pairs), int(walk), int(connections)
        self.light_connections = lc = int(light_connections)
        self.light_chosen = None
        if lc:
            (self.light_shadow_rays, self.light_shadow_hits, self.light_asks, self.light_pending, self.light_ask_index,
             self.light_ask_count) = _connection_buffers(lc, device)
            self.light_reach = _new((lc,), "float32", device)
            if chosen:
                self.light_chosen = _new((lc,), "int32", device)
        if connections:
            self.shadow_rays, self.shadow_hits, self.asks, self.pending, self.ask_index, self.ask_count = _connection_buffers(connections, device)
        self.paths, self.radiance = _new((entries, PATH_WORDS), "int32", device), _new((entries, 3), "float32", device)
        self.hits, self.emitted = _new((entries, 13), "int32", device), _new((entries, 3), "float32", device)
        self.rays, self.next_rays = _new((entries, 11), "int32", device), _new((entries, 11), "int32", device)
        self.alive, self.index, self.count = _new((entries,), "uint8", device), _new((entries,), "int32", device), _new((1,), "int32", device)
        self.lights = LightWorkspace(pairs, device) if pairs else None
        if walk:
            self.lobe, self.transmit = _new((walk,), "uint8", device), _new((walk,), "uint8", device)
            self.walk_index, self.walk_count = _new((walk,), "int32", device), _new((1,), "int32", device)
            self.walk_rays, self.inside_hits = _new((walk, 11), "int32", device), _new((walk, 13), "int32", device)
            self.kind = _new((walk,), "int32", device).fill_(HIT_NONE)
            self.travel, self.casts = _new((walk,), "float32", device), _new((walk,), "int32", device)
            self.walk_flags, self.escape = _new((walk,), "uint8", device).zero_(), _new((walk, 11), "int32", device).zero_()


def workspace(n: int, device, spp: int, scene: Scene = None, transmission: bool = False, nee: bool = False, light_nee: bool = False,
              chosen: bool = False) -> Workspace:
    """A Workspace for trace_paths on up to ``n`` roots with ``spp`` samples; with ``scene`` also for ``open_casts`` on its lights, with
    ``transmission`` also the walk buffers of trace_paths(transmission=True), with ``nee`` also the connection buffers of
    trace_paths(nee=True): 113 B per path more — shadow rays 44, shadow hits 52, asks 1, pending 12, a second index 4 — and one count; with ``light_nee`` also the light-connection buffers of
    trace_paths(light_nee=True), separate from the sky's: 117 B per path more — shadow rays 44, shadow hits 52, asks 1, pending 12, reach
    4, a second index 4 — and one count, and with ``chosen`` 4 B per path for the light each vertex drew (Workspace.light_chosen)."""
    if n < 0 or spp < 0:
        raise ValueError("n and spp must not be negative")
    entries = int(n) * int(spp)
    return Workspace(entries, entries * scene.n_lights if scene is not None else 0, device, entries if transmission else 0, entries if nee else 0,
                     entries if light_nee else 0, bool(chosen))


def trace_paths(scene: Scene, hits, incoming, spp: int, max_bounces: int, env=None, rr_start: int = 3, rr_floor: float = 0.05, seed: int = 0, ids=None,
                out=None, open_casts: bool = True, stream=None, workspace=None, transmission: bool = False, walk_rounds: int = 11, nee: bool = False,
                heuristic: int = BALANCE, light_nee: bool = False, light_radii=None, light_weights=None):
    """``spp`` paths of up to ``max_bounces`` bounces from every hit, their mean ADDED to ``out`` ((N, 3) float32 CUDA; None: a new,
    zeroed tensor): at each vertex the light of the scene's lights (shade_hits) — with ``env`` (an environment.Environment) the sky for
    the paths that left the scene — times the throughput, then one direction from the vertex's own lobes.  ``hits`` and ``incoming`` are
    the roots: N hits and the rays that found them.  Written from the public calls alone — the executable form of the sequence in
    INTEGRATION.md, to be copied and changed:
      begin -> the spp copies of the roots' hits and rays
      per bounce b = 0 .. max_bounces:  shade_hits (all slots) -> environment.lookup (the misses; only with env) ->
                  advance(list_b, last = (b == max_bounces)) -> select_records(alive) -> cast_rays_indexed(next rays, list_b+1);
                  the next rays are the next bounce's incoming rays, and what they hit — the nearest surface, front or back: they
                  are cast with face BOTH — the next bounce's vertices
      resolve
    Bounce b draws with seed + 0x9e3779b9 * b; roulette starts at bounce ``rr_start`` (NO_ROULETTE: never).  ``open_casts``:
    shade_hits_by_light in the place of shade_hits, so that every cast of the loop is a cast_rays_indexed (the same bits).  The loop
    visits the host nowhere, and with ``out`` and ``workspace`` (workspace(n, device, spp, scene)) it allocates nothing; after one
    eager call on the stream it may be captured into a graph (select_records and the indexed casts need that first call).
    ``transmission``: paths pass through glass.  At a vertex a path takes the material's refraction with probability transparency and
    the lobes otherwise, and advance(list_b, last) in the sequence above becomes
      branch(list_b, last) -> select_records(lobe) -> advance(that list, last) ->
      ``walk_rounds`` times: select_records(walk flags) -> cast_rays_indexed(walk rays -> inside hits) -> refract_step (all slots) ->
      select_records(transmit) -> transmit(that list)
    (the walk and the transmit are left out of the last bounce: branch ends the paths that would have walked).  Eleven rounds finish
    every walk; fewer end the paths still walking with TRAPPED.  With the default not one call of the sequence changes.  The workspace
    is then workspace(n, device, spp, scene, transmission=True).
    ``nee`` (``env`` is then required): next-event estimation of the sky.  At every vertex but the last bounce's one direction is drawn
    from the environment's table and weighed against the vertex's lobes by ``heuristic`` (BALANCE or POWER), and the sky a lobe-sampled
    ray escapes to is weighed the other way round with the density kept in the record; per bounce the sequence becomes
      shade_hits -> environment.lookup -> weigh_escape(list_b) -> connect(list_b) -> advance(list_b, last) ->
      select_records(asks) -> cast_rays_indexed(shadow rays -> shadow hits) -> settle(that list) ->
      select_records(alive) -> cast_rays_indexed(next rays, list_b+1)
    connect before advance, which moves the throughput and rewrites an ended path's hit; settle after it, so that a vertex's deposit is
    added before its connection.  On the last bounce connect and settle are left out: both estimators integrate the same paths.  With
    ``transmission`` connect takes the lobe list, as advance does — a path that goes through the glass deposits nothing at the vertex and
    connects nothing there — and settle follows transmit.  A sky seen through glass arrives with pdf +0 in the record and keeps its full
    weight, and a connection through glass is occluded by it, so nothing is counted twice.  The connection carries its own texel's
    radiance and the escape the lookup's: with environment.NEAREST the two estimate one integrand.  The workspace is then
    workspace(n, device, spp, scene, nee=True); the table is env.table(stream), built (and allocated) by the first call that asks for it.
    With ``nee`` False not one call of the sequence changes.
    ``light_nee``: next-event estimation of the scene's own lights — one light per vertex, chosen uniformly or by ``light_weights``
    ((n_lights,) float32), and one point on its sphere of radius ``light_radii[l]`` ((n_lights,) float32; None: points), so one shadow
    cast per vertex whatever the number of lights, and soft shadows where the lights have radii.  The shade step is left out (the
    emitted light of the hits is zeros; ``open_casts`` then has nothing to open) and per bounce the sequence becomes
      [zeros] -> environment.lookup (only with env) -> connect_lights(list_b) -> advance(list_b, last) ->
      select_records(light asks) -> cast_rays_indexed(shadow rays -> shadow hits) -> settle_lights(that list) ->
      select_records(alive) -> cast_rays_indexed(next rays, list_b+1)
    The last bounce connects and settles too, as shade_hits lights the last vertex.  With ``nee`` both connections of a vertex are
    outstanding at once, in buffers of their own, and the lights are settled before the sky: a vertex adds deposit, lights, sky, the
    order in which the loop without ``light_nee`` adds them — with one light the two loops give the same bits.  With ``transmission``
    connect_lights takes the lobe list, as advance does, and settle_lights follows transmit.  The workspace is then
    workspace(n, device, spp, scene, light_nee=True) (``chosen``: Workspace.light_chosen receives the light each vertex drew).  With
    ``light_nee`` False not one call of the sequence changes."""
    spp, max_bounces, walk_rounds = _samples(spp), int(max_bounces), int(walk_rounds)
    if max_bounces < 0:
        raise ValueError("max_bounces must not be negative")
    if walk_rounds < 0:
        raise ValueError("walk_rounds must not be negative")
    if nee and env is None:
        raise ValueError("nee needs env: an environment.Environment")
    records = _hit_records(hits)
    n, dev = records.shape[0], records.device
    _tensor(incoming, "incoming", "int32", (n, 11))
    _tensor(ids, "ids", "int32", (n,), optional=True)
    out = _zeroed_out(out, n, dev, stream)
    m = spp * n
    _below_2_32(m, "(sample, hit) entries")
    if m == 0:
        return out
    pairs = m * scene.n_lights if open_casts and not light_nee else 0
    _below_2_32(pairs, "(path, light) pairs")
    sizes = {"entries": m, "pairs": pairs, "walk": m} if transmission else {"entries": m, "pairs": pairs}
    if nee:
        sizes["connections"] = m
    if light_nee:
        sizes["light_connections"] = m
        _tensor(light_radii, "light_radii", "float32", (scene.n_lights,), optional=True)
        _tensor(light_weights, "light_weights", "float32", (scene.n_lights,), optional=True)
    w = _room(workspace, Workspace, sizes,
              f"a paths.Workspace with room for {m} paths and {pairs} (path, light) pairs{' and their walks' if transmission else ''}"
              f"{' and their connections' if nee else ''}{' and their light connections' if light_nee else ''} (paths.workspace)", dev, stream)
    s = stream
    vertices, emitted, radiance, paths, alive, index = w.hits[:m], w.emitted[:m], w.radiance[:m], w.paths[:m], w.alive[:m], w.index[:m]
    rays, next_rays = w.rays[:m], w.next_rays[:m]
    begin(n, spp, ids, paths, radiance, stream=s)
    with _on_stream(s):  # the spp copies of the roots
        vertices.view(spp, n, 13).copy_(records.unsqueeze(0).expand(spp, n, 13))
        rays.view(spp, n, 11).copy_(incoming.unsqueeze(0).expand(spp, n, 11))
    if transmission:
        lobe, through, walk_index, walk_rays, inside_hits = w.lobe[:m], w.transmit[:m], w.walk_index[:m], w.walk_rays[:m], w.inside_hits[:m]
        kind, travel, casts, walk_flags, escape = w.kind[:m], w.travel[:m], w.casts[:m], w.walk_flags[:m], w.escape[:m]
    if nee:
        table = _environment(env).table(s)
        shadow_rays, shadow_hits, asks, pending, ask_index = w.shadow_rays[:m], w.shadow_hits[:m], w.asks[:m], w.pending[:m], w.ask_index[:m]
    if light_nee:
        light_rays, light_hits, light_asks, light_pending = w.light_shadow_rays[:m], w.light_shadow_hits[:m], w.light_asks[:m], w.light_pending[:m]
        light_reach, light_index = w.light_reach[:m], w.light_ask_index[:m]
        light_chosen = w.light_chosen[:m] if w.light_chosen is not None else None

        def connect_to_lights(list_index, list_count):
            connect_lights(scene, paths, vertices, rays, list_index, list_count, seed, light_radii, light_weights, 0, None, light_rays, light_asks,
                           light_pending, light_reach, light_chosen, stream=s)

        def settle_the_lights():
            select_records(light_asks, light_index, w.light_ask_count, stream=s)
            cast_rays_indexed(scene, light_rays, light_index, w.light_ask_count, light_hits, stream=s)
            settle_lights(paths, light_asks, light_rays, light_reach, light_pending, radiance, light_hits, light_index, w.light_ask_count, stream=s)
    listed = counted = None  # bounce 0: every slot
    for b in range(max_bounces + 1):
        if light_nee:
            with _on_stream(s):
                emitted.zero_()  # the shade step is left out
        elif open_casts:
            shade_hits_by_light(scene, vertices, rays, out=emitted, stream=s, workspace=w.lights)
        else:
            shade_hits(scene, vertices, rays, out=emitted, stream=s)
        if env is not None:
            lookup(env, rays, vertices, out=emitted, stream=s)
        last = b == max_bounces
        if nee:
            weigh_escape(env, paths, vertices, rays, emitted, listed, counted, heuristic, table, stream=s)
        if not transmission:
            if nee and not last:
                connect(scene, env, paths, vertices, rays, listed, counted, seed, SHADING, heuristic, False, table, shadow_rays, asks, pending, stream=s)
            if light_nee:
                connect_to_lights(listed, counted)
            advance(scene, paths, vertices, rays, radiance, emitted, listed, counted, seed, SHADING, rr_start, rr_floor, last, next_rays, alive, stream=s)
        else:
            branch(scene, paths, vertices, rays, listed, counted, seed, last, lobe, through, walk_rays, kind, travel, casts, walk_flags, stream=s)
            select_records(lobe, walk_index, w.walk_count, stream=s)
            if nee and not last:
                connect(scene, env, paths, vertices, rays, walk_index, w.walk_count, seed, SHADING, heuristic, False, table, shadow_rays, asks, pending, stream=s)
            if light_nee:
                connect_to_lights(walk_index, w.walk_count)
            advance(scene, paths, vertices, rays, radiance, emitted, walk_index, w.walk_count, seed, SHADING, rr_start, rr_floor, last, next_rays, alive, stream=s)
        if last:
            if light_nee:
                settle_the_lights()
            break
        if transmission:
            for _ in range(walk_rounds):
                select_records(walk_flags, walk_index, w.walk_count, stream=s)
                cast_rays_indexed(scene, walk_rays, walk_index, w.walk_count, inside_hits, stream=s)
                refract_step(scene, vertices, inside_hits, walk_rays, kind, travel, casts, walk_flags, MAX_DISTANCE, escape, stream=s)
            select_records(through, walk_index, w.walk_count, stream=s)
            transmit(scene, paths, vertices, kind, travel, escape, walk_flags, walk_index, w.walk_count, seed, rr_start, rr_floor, next_rays, alive, stream=s)
        if light_nee:
            settle_the_lights()
        if nee:
            select_records(asks, ask_index, w.ask_count, stream=s)
            cast_rays_indexed(scene, shadow_rays, ask_index, w.ask_count, shadow_hits, stream=s)
            settle(paths, asks, pending, radiance, shadow_hits, ask_index, w.ask_count, stream=s)
        listed, counted = select_records(alive, index, w.count, stream=s)
        cast_rays_indexed(scene, next_rays, listed, counted, vertices, stream=s)
        rays, next_rays = next_rays, rays
    return resolve(radiance, n, spp, out, stream=s)
