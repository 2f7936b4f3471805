"""get_shade and get_refract opened into the calls between their casts: the light queries and the refraction queries."""
from __future__ import annotations

from . import _capi
from ._args import _below_2_32, _count_ptr, _new, _on_stream, _out_tensor, _p, _stream_ptr, _tensor, _torch
from ._queries import ESCAPED, Refractions, _hit_records, _hits_and_rays, _refractions, cast_rays_indexed, select_records
from ._world import Scene

# ---- light queries: get_shade light by light (include/rt_amd.h rt_light_rays, rt_light_terms, rt_light_fold) ----


def _light_range(scene: Scene, light_first, light_count):
    first = int(light_first)
    count = scene.n_lights - first if light_count is None else int(light_count)
    if first < 0 or count < 0:
        raise ValueError("light_first and light_count must not be negative (light_count None: every light from light_first on)")
    return first, count


def light_rays(scene: Scene, hits, rays, light_first: int = 0, light_count=None, out_rays=None, out_asks=None, out_distance=None,
               distance: bool = False, stream=None):
    """main.rs:408-433 per hit and light (rt_light_rays): returns (shadow_rays, asks, light_distance) for the lights light_first ..
    light_first + light_count - 1 (default: every light from light_first on), light-major — entry (l - light_first) * N + i belongs to
    light l and hit i.  ``asks`` (L*N,) uint8: 1 where get_shade casts a shadow ray; ``shadow_rays`` (L*N, 11) int32: that ray, bit for
    bit, all-zero words elsewhere — one batch for select_records(asks) + cast_rays_indexed; ``light_distance`` (L*N,) float32, computed
    when ``distance`` is set or ``out_distance`` given (else None): what the reference compares the occluder's distance against."""
    records, n = _hits_and_rays(hits, rays)
    first, count = _light_range(scene, light_first, light_count)
    pairs = count * n
    dev = records.device
    out_rays = _out_tensor(out_rays, (pairs, 11), "int32", dev, "out_rays")
    out_asks = _out_tensor(out_asks, (pairs,), "uint8", dev, "out_asks")
    if out_distance is not None or distance:
        out_distance = _out_tensor(out_distance, (pairs,), "float32", dev, "out_distance")
    _capi.check(_capi.amd_lib().rt_light_rays(scene._h, _p(records), _p(rays), n, first, count, _p(out_rays), _p(out_asks), _p(out_distance),
                                              _stream_ptr(stream)))
    return out_rays, out_asks, out_distance


def light_terms(scene: Scene, hits, rays, asks, shadow_hits, light_first: int = 0, light_count=None, out_lit=None, out_diffuse=None,
                out_specular=None, stream=None):
    """main.rs:435-459 per hit and light (rt_light_terms): returns (lit, diffuse, specular), light-major as light_rays' outputs.
    ``shadow_hits`` (L*N, 13) int32: what a cast of the shadow rays wrote, read only where ``asks`` is set.  ``lit`` (L*N,) uint8: 1
    where the light asks, is Some and is not occluded; there ``diffuse`` and ``specular`` (L*N, 3) float32 are get_diffuse and
    get_specular times the light's colour, not yet weighted by shiness; +0 elsewhere."""
    records, n = _hits_and_rays(hits, rays)
    first, count = _light_range(scene, light_first, light_count)
    pairs = count * n
    dev = records.device
    _tensor(asks, "asks", "uint8", (pairs,))
    _tensor(shadow_hits, "shadow_hits", "int32", (pairs, 13))
    out_lit = _out_tensor(out_lit, (pairs,), "uint8", dev, "out_lit")
    out_diffuse = _out_tensor(out_diffuse, (pairs, 3), "float32", dev, "out_diffuse")
    out_specular = _out_tensor(out_specular, (pairs, 3), "float32", dev, "out_specular")
    _capi.check(_capi.amd_lib().rt_light_terms(scene._h, _p(records), _p(rays), n, first, count, _p(asks), _p(shadow_hits), _p(out_lit),
                                               _p(out_diffuse), _p(out_specular), _stream_ptr(stream)))
    return out_lit, out_diffuse, out_specular


def light_fold(scene: Scene, hits, lit, diffuse, specular, out, stream=None):
    """main.rs:461 (rt_light_fold): for the L = len(lit) / N lights of ``lit``, ``diffuse`` and ``specular`` in order, where lit:
    out = (out + diffuse * (1 - shiness)) + specular * shiness, in place on ``out`` ((N, 3) float32, required).  The call ADDS: zero
    ``out`` before the first range of lights; later ranges continue the sum.  A record that is no hit is not written."""
    records = _hit_records(hits)
    n = records.shape[0]
    _tensor(out, "out", "float32", (n, 3))
    pairs = _tensor(lit, "lit", "uint8", (None,)).shape[0]
    if pairs % n != 0 if n else pairs != 0:
        raise ValueError("lit must have one entry per (light, hit) pair")
    count = pairs // n if n else 0
    _tensor(diffuse, "diffuse", "float32", (pairs, 3))
    _tensor(specular, "specular", "float32", (pairs, 3))
    _capi.check(_capi.amd_lib().rt_light_fold(scene._h, _p(records), n, count, _p(lit), _p(diffuse), _p(specular), _p(out), _stream_ptr(stream)))
    return out


class LightWorkspace:
    """The buffers of one pass of shade_hits_by_light, made once by light_workspace so that a caller's loop allocates nothing:
    ``pairs`` (hit, light) pairs of room."""

    def __init__(self, pairs: int, device):
        self.pairs = int(pairs)
        self.shadow_rays, self.shadow_hits = _new((pairs, 11), "int32", device), _new((pairs, 13), "int32", device)
        self.asks, self.lit = _new((pairs,), "uint8", device), _new((pairs,), "uint8", device)
        self.index, self.count = _new((pairs,), "int32", device), _new((1,), "int32", device)
        self.diffuse, self.specular = _new((pairs, 3), "float32", device), _new((pairs, 3), "float32", device)


def light_workspace(scene: Scene, n: int, device, lights_per_pass=None) -> LightWorkspace:
    """A LightWorkspace for shade_hits_by_light on up to ``n`` hits of ``scene``, ``lights_per_pass`` lights at a time (default: all)."""
    per_pass = scene.n_lights if lights_per_pass is None else min(int(lights_per_pass), scene.n_lights)
    if per_pass < 0 or n < 0:
        raise ValueError("n and lights_per_pass must not be negative")
    return LightWorkspace(int(n) * per_pass, device)


def shade_hits_by_light(scene: Scene, hits, rays, out=None, ray_count=None, stream=None, lights_per_pass=None, workspace=None):
    """shade_hits — the same hits, the same values and cast count, bit for bit — written light by light from the public calls alone:
    the executable form of the sequence in INTEGRATION.md, to be copied and changed (a subset of lights, a shadow rule of one's own,
    per-light output).  Zero ``out``; then per range of ``lights_per_pass`` lights (default: all of them — it bounds the memory, about
    126 B per (hit, light) pair of a pass): light_rays -> select_records(asks) -> cast_rays_indexed(shadow rays -> shadow hits,
    ray_count) -> light_terms -> light_fold.  Every buffer is allocated once, up front; after that the function only enqueues library
    calls on ``stream`` and reads nothing back.  The shadow casts take cast_rays_indexed's routes: on a scene walked breadth-first that
    walk.  (Being a sequence of calls it may not be captured before select_records — and, on such a scene, cast_rays_indexed — has run
    once on the stream.)"""
    records, n = _hits_and_rays(hits, rays)
    dev = records.device
    out = _out_tensor(out, (n, 3), "float32", dev)
    _count_ptr(ray_count)
    lights = scene.n_lights
    per_pass = lights if lights_per_pass is None else int(lights_per_pass)
    if lights_per_pass is not None and per_pass < 1:
        raise ValueError("lights_per_pass must be at least 1")
    per_pass = min(per_pass, lights)
    _below_2_32(n * per_pass, "(hit, light) pairs", " in one pass (lights_per_pass)")
    s = stream
    # allocated (and the fill enqueued) with `stream` as torch's current stream: the caching allocator then ties the blocks to it
    with _on_stream(stream):
        out.zero_()  # `sum` starts black (main.rs:411)
        if n == 0 or lights == 0:
            return out
        pairs = per_pass * n
        if workspace is None:
            workspace = LightWorkspace(pairs, dev)
        elif not isinstance(workspace, LightWorkspace) or workspace.pairs < pairs:
            raise ValueError(f"workspace must be a LightWorkspace with room for {pairs} (hit, light) pairs (light_workspace)")
        shadow_rays, shadow_hits, asks, lit = workspace.shadow_rays, workspace.shadow_hits, workspace.asks, workspace.lit
        index, count, diffuse, specular = workspace.index, workspace.count, workspace.diffuse, workspace.specular
    for first in range(0, lights, per_pass):
        c = min(per_pass, lights - first)
        m = c * n
        light_rays(scene, records, rays, first, c, shadow_rays[:m], asks[:m], stream=s)
        select_records(asks[:m], index[:m], count, stream=s)
        cast_rays_indexed(scene, shadow_rays[:m], index[:m], count, shadow_hits[:m], ray_count=ray_count, stream=s)
        light_terms(scene, records, rays, asks[:m], shadow_hits[:m], first, c, lit[:m], diffuse[:m], specular[:m], stream=s)
        light_fold(scene, records, lit[:m], diffuse[:m], specular[:m], out, stream=s)
    return out


# ---- refraction queries: get_refract bounce by bounce (include/rt_amd.h rt_refract_enter, rt_refract_step) ----

WALKING = 3  # RT_REFR_WALKING: the walk through the glass goes on (beside ESCAPED, INFINITE, TRAPPED and HIT_NONE)


def refract_enter(scene: Scene, hits, rays, out_rays=None, out_kind=None, out_travel=None, out_casts=None, out_flags=None, stream=None):
    """main.rs:354-368 per hit (rt_refract_enter): returns (inside_rays, kind, travel, casts, flags), the state of a walk that has cast
    nothing yet.  ``kind`` (N,) int32: WALKING, TRAPPED where the ray cannot enter, HIT_NONE for a record that is no hit;
    ``inside_rays`` (N, 11) int32: where walking, ray_inside — bit for bit the ray refract_rays casts first —, all-zero words elsewhere;
    ``travel`` (N,) float32 zeros, ``casts`` (N,) int32 zeros, ``flags`` (N,) uint8: 1 where walking — the operand of select_records."""
    records, n = _hits_and_rays(hits, rays)
    dev = records.device
    out_rays = _out_tensor(out_rays, (n, 11), "int32", dev, "out_rays")
    out_kind = _out_tensor(out_kind, (n,), "int32", dev, "out_kind")
    out_travel = _out_tensor(out_travel, (n,), "float32", dev, "out_travel")
    out_casts = _out_tensor(out_casts, (n,), "int32", dev, "out_casts")
    out_flags = _out_tensor(out_flags, (n,), "uint8", dev, "out_flags")
    _capi.check(_capi.amd_lib().rt_refract_enter(scene._h, _p(records), _p(rays), n, _p(out_rays), _p(out_kind), _p(out_travel), _p(out_casts),
                                                 _p(out_flags), _stream_ptr(stream)))
    return out_rays, out_kind, out_travel, out_casts, out_flags


def refract_step(scene: Scene, hits, inside_hits, inside_rays, kind, travel, casts, flags, max_distance: float = 100.0, out_escape=None,
                 stream=None):
    """main.rs:371-402 for one answered cast (rt_refract_step), in place on the state refract_enter made: ``inside_hits`` (N, 13) int32
    is what a cast of ``inside_rays`` wrote, read only where ``kind`` is WALKING.  A walking record counts the cast and becomes INFINITE
    (its ray stays: the one whose cast missed), goes on WALKING with the total-reflection ray and flag 1, becomes ESCAPED with its escape
    ray in ``out_escape``, or TRAPPED; records that were finished get flag 0 and nothing else.  Returns ``out_escape`` ((N, 11) int32;
    zeroed and allocated if None — keep ONE across the rounds: a record's entry is written in the round that finishes it)."""
    records = _hit_records(hits)
    n = records.shape[0]
    _tensor(inside_hits, "inside_hits", "int32", (n, 13))
    _tensor(inside_rays, "inside_rays", "int32", (n, 11))
    _tensor(kind, "kind", "int32", (n,))
    _tensor(travel, "travel", "float32", (n,))
    _tensor(casts, "casts", "int32", (n,))
    _tensor(flags, "flags", "uint8", (n,))
    if out_escape is None:
        with _on_stream(stream):
            out_escape = _new((n, 11), "int32", records.device).zero_()
    _tensor(out_escape, "out_escape", "int32", (n, 11))
    _capi.check(_capi.amd_lib().rt_refract_step(scene._h, _p(records), n, float(max_distance), _p(inside_hits), _p(inside_rays), _p(kind),
                                                _p(travel), _p(casts), _p(flags), _p(out_escape), _stream_ptr(stream)))
    return out_escape


class RefractWorkspace:
    """The state and scratch of refract_rays_by_bounce beside its result, made once by refract_workspace so that a caller's loop
    allocates nothing; ``n`` records of room.  ``rays`` (n, 11): the ray in flight (for an INFINITE record the ray whose cast missed),
    ``inside_hits`` (n, 13), ``casts`` (n,) int32: the casts answered per record, ``flags`` (n,) uint8, ``index`` / ``count``:
    select_records' list."""

    def __init__(self, n: int, device):
        self.n = int(n)
        self.rays, self.inside_hits = _new((n, 11), "int32", device), _new((n, 13), "int32", device)
        self.casts = _new((n,), "int32", device)
        self.flags, self.index, self.count = _new((n,), "uint8", device), _new((n,), "int32", device), _new((1,), "int32", device)
        self._mask = [_new((n,), "bool", device) for _ in range(2)]


def refract_workspace(n: int, device) -> RefractWorkspace:
    """A RefractWorkspace for refract_rays_by_bounce on up to ``n`` hits."""
    if n < 0:
        raise ValueError("n must not be negative")
    return RefractWorkspace(n, device)


def refract_rays_by_bounce(scene: Scene, hits, rays, max_distance: float = 100.0, ray_count=None, stream=None, out=None, rounds: int = 11,
                           workspace=None, resume: bool = False) -> Refractions:
    """refract_rays — the same hits, the same Refractions and cast count, bit for bit — written bounce by bounce from the public calls
    alone: the executable form of the sequence in INTEGRATION.md, to be copied and changed (a bounce limit, an absorption rule per
    segment, a stop at the first interior hit).  refract_enter, then ``rounds`` times select_records(flags) -> cast_rays_indexed(inside
    rays -> inside hits, ray_count) -> refract_step; last, travel is set to 0 where the record ended without escaping, as refract_rays
    reports it.  Eleven rounds finish every walk (main.rs:378); fewer leave the unfinished records WALKING — a caller's own bounce limit —
    with their state in ``out`` and ``workspace``, and a later call with ``resume=True`` and the same ``out`` and ``workspace`` goes on
    from there.  Every buffer is allocated once, up front — or none at all with ``out`` and ``workspace``, a RefractWorkspace
    (refract_workspace); after that the function only enqueues calls on ``stream`` (the library's, and four element-wise fills for the
    travel of the records that did not escape) and reads nothing back.  workspace.casts holds the casts per record.  The casts take
    cast_rays_indexed's routes: on a scene walked breadth-first that walk.  (Being a sequence of calls it may not be captured before
    select_records — and, on such a scene, cast_rays_indexed — has run once on the stream.)"""
    torch = _torch()
    records, n = _hits_and_rays(hits, rays)
    dev = records.device
    rounds = int(rounds)
    if rounds < 0:
        raise ValueError("rounds must not be negative")
    _count_ptr(ray_count)
    if resume and (out is None or workspace is None):
        raise ValueError("resume=True continues the walks held in out and workspace: both are required")
    if workspace is not None and not (isinstance(workspace, RefractWorkspace) and workspace.n >= n):
        raise ValueError(f"workspace must be a RefractWorkspace with room for {n} records (refract_workspace)")
    s = stream
    # allocated (and the fills enqueued) with `stream` as torch's current stream: the caching allocator then ties the blocks to it
    with _on_stream(stream):
        out = _refractions(out, n, dev)
        kind, travel, escape = out.kind, out.travel, out.rays
        if n == 0:
            return out
        if workspace is None:
            workspace = RefractWorkspace(n, dev)
        w = workspace
        w_rays, w_hits, w_casts, w_flags, w_index = w.rays[:n], w.inside_hits[:n], w.casts[:n], w.flags[:n], w.index[:n]
        if not resume:
            escape.zero_()  # refract_step writes a record's escape ray in the round that finishes it; refract_enter finishes some itself
    if not resume:
        refract_enter(scene, records, rays, w_rays, kind, travel, w_casts, w_flags, stream=s)
    for _ in range(rounds):
        select_records(w_flags, w_index, w.count, stream=s)
        cast_rays_indexed(scene, w_rays, w_index, w.count, w_hits, ray_count=ray_count, stream=s)
        refract_step(scene, records, w_hits, w_rays, kind, travel, w_casts, w_flags, max_distance, escape, stream=s)
    with _on_stream(stream):
        ended, not_walking = w._mask[0][:n], w._mask[1][:n]
        torch.ne(kind, ESCAPED, out=ended)
        torch.ne(kind, WALKING, out=not_walking)
        ended.logical_and_(not_walking)
        travel.masked_fill_(ended, 0.0)  # travel_distance belongs to Escaped alone (main.rs:402)
    return out
