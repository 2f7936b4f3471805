"""The level loop and the tree loop: the glue calls of one level, their folds, and the two traces written out level by level."""
from __future__ import annotations

from . import _capi
from ._args import _allocator, _count_ptr, _new, _on_stream, _out_tensor, _p, _stream_ptr, _tensor, _torch
from ._capi import RtError
from ._opened import light_workspace, refract_rays_by_bounce, refract_workspace, shade_hits_by_light
from ._queries import (Refractions, Scatters, _hit_records, _rng_of, _sample_outputs, cast_rays_indexed, reflect_rays, refract_rays,
                       scatter_factors, scatter_hits, select_records, shade_hits)
from ._render import Rng
from ._world import Scene

# ---- level loop: the glue of one level and the fold (include/rt_amd.h rt_level_split ... rt_level_finish) ----

def level_split(hits, types, cosine, out_reflect=None, out_refract=None, stream=None):
    """After scatter_hits (rt_level_split): returns (hits_reflect, hits_refract), (N, 13) int32 rt_hit records — hits[i] where the level
    goes on as a diffuse or reflection scatter, respectively as a refraction, "no hit" elsewhere: the operands of reflect_rays and
    refract_rays.  ``types``, ``cosine``: Scatters.type and Scatters.cosine."""
    records = _hit_records(hits)
    n, dev = records.shape[0], records.device
    _tensor(types, "types", "int32", (n,))
    _tensor(cosine, "cosine", "float32", (n,))
    out_reflect = _out_tensor(out_reflect, (n, 13), "int32", dev, "out_reflect")
    out_refract = _out_tensor(out_refract, (n, 13), "int32", dev, "out_refract")
    _capi.check(_capi.amd_lib().rt_level_split(_p(records), _p(types), _p(cosine), n, _p(out_reflect), _p(out_refract), _stream_ptr(stream)))
    return out_reflect, out_refract


def level_join(types, cosine, reflected, refr_kind, escape, out_rays=None, out_hits=None, out_flags=None, stream=None):
    """After reflect_rays / refract_rays (rt_level_join): returns (next_rays, next_hits, flags) — the ray each record casts next (the
    reflected one, or the escape ray of an Escaped refraction; zero words where there is none), the next hits preset to "no hit", and
    an (N,) uint8 flag where a ray exists: select_records(flags) + cast_rays_indexed(next_rays -> next_hits) follow."""
    n, dev = _tensor(reflected, "reflected", "int32", (None, 11)).shape[0], reflected.device
    _tensor(escape, "escape", "int32", (n, 11))
    _tensor(types, "types", "int32", (n,))
    _tensor(cosine, "cosine", "float32", (n,))
    _tensor(refr_kind, "refr_kind", "int32", (n,))
    out_rays = _out_tensor(out_rays, (n, 11), "int32", dev, "out_rays")
    out_hits = _out_tensor(out_hits, (n, 13), "int32", dev, "out_hits")
    out_flags = _out_tensor(out_flags, (n,), "uint8", dev, "out_flags")
    _capi.check(_capi.amd_lib().rt_level_join(_p(types), _p(cosine), _p(reflected), _p(refr_kind), _p(escape), n, _p(out_rays), _p(out_hits),
                                              _p(out_flags), _stream_ptr(stream)))
    return out_rays, out_hits, out_flags


def level_close(hits, types, cosine, next_hits, out=None, stream=None):
    """After the indexed cast (rt_level_close): returns (N, 13) int32 rt_hit records — hits[i] where a diffuse or reflection scatter
    went on and its next cast missed, "no hit" elsewhere: the operand of get_shade(&scattered_hit), shade_hits(out, Scatters.rays)."""
    records = _hit_records(hits)
    n = records.shape[0]
    nxt = _tensor(_hit_records(next_hits, "next_hits"), "next_hits", "int32", (n, 13))
    _tensor(types, "types", "int32", (n,))
    _tensor(cosine, "cosine", "float32", (n,))
    out = _out_tensor(out, (n, 13), "int32", records.device)
    _capi.check(_capi.amd_lib().rt_level_close(_p(records), _p(types), _p(cosine), _p(nxt), n, _p(out), _stream_ptr(stream)))
    return out


def level_fold(types, cosine, next_hits, factor, shade_next, shade_missed, value, stream=None):
    """One step of the unwind (rt_level_fold), from the deepest level back: ``value`` ((N, 3) float32, in place) holds the value of the
    level below and receives this level's — the mix of main.rs:571 / 590, the sum of main.rs:605, shade_missed or black, in
    trace_rays_distributed's operation order."""
    nxt = _hit_records(next_hits, "next_hits")
    n = nxt.shape[0]
    _tensor(types, "types", "int32", (n,))
    _tensor(cosine, "cosine", "float32", (n,))
    for t, name in ((factor, "factor"), (shade_next, "shade_next"), (shade_missed, "shade_missed"), (value, "value")):
        _tensor(t, name, "float32", (n, 3))
    _capi.check(_capi.amd_lib().rt_level_fold(_p(types), _p(cosine), _p(nxt), _p(factor), _p(shade_next), _p(shade_missed), n, _p(value),
                                              _stream_ptr(stream)))
    return value


def level_finish(value, accum=None, valid=None, stream=None):
    """The sample filter and the accumulation (rt_level_finish, main.rs:1157-1165): valid[i] = all three channels of value[i] are
    is_normal ((N,) uint8 or None); accum[i] += value[i] where valid ((N, 3) float32 or None).  At least one of the two."""
    n = _tensor(value, "value", "float32", (None, 3)).shape[0]
    _tensor(accum, "accum", "float32", (n, 3), optional=True)
    _tensor(valid, "valid", "uint8", (n,), optional=True)
    _capi.check(_capi.amd_lib().rt_level_finish(_p(value), n, _p(accum), _p(valid), _stream_ptr(stream)))
    return accum if accum is not None else valid


def trace_rays_distributed_levels(scene: Scene, rays, max_depth: int, rng: Rng, n_epochs: int = 1, accum=None, samples=None, valid=None,
                                  ray_count=None, stream=None, open_casts: bool = False):
    """trace_rays_distributed — the same arguments, the same samples, flags, accumulated image, cast count and generator records, bit for
    bit — written one level at a time from the public calls alone: the executable form of the loop in INTEGRATION.md, to be copied and
    changed (a stopping rule, a weighting, a re-sort between levels).  Every buffer is allocated once, up front; after that the function
    only enqueues library calls on ``stream``: no tensor arithmetic, nothing read back, no synchronisation.  The cast count is what the
    calls' device counters add up to; the primary casts go through cast_rays_indexed with an identity list so that they are counted too.
    ``open_casts=True`` replaces shade_hits by shade_hits_by_light and refract_rays by refract_rays_by_bounce, each on a workspace made
    up front: every cast of the loop is then a cast_rays_indexed — on a scene walked breadth-first, that walk — with the same bits and
    count (the two add a few element-wise fills to what is enqueued).
    (Being a sequence of calls it may not be captured before select_records has run once on the stream.)"""
    n = _tensor(rays, "rays", "int32", (None, 11)).shape[0]
    n_epochs = int(n_epochs)
    _sample_outputs(accum, samples, valid, n_epochs, n)
    _count_ptr(ray_count)
    _rng_of(rng)
    if n != rng.count:
        raise ValueError("the Rng must hold one generator per ray")
    if accum is None and samples is None:
        raise ValueError("at least one of accum / samples")
    if max_depth > _capi.RT_MAX_DEPTH:
        raise RtError(-5, f"max_depth above RT_MAX_DEPTH ({_capi.RT_MAX_DEPTH})")
    if n == 0 or n_epochs == 0:
        return accum if accum is not None else samples
    depth = max(int(max_depth), 0)
    dev = rays.device
    s = stream
    new = _allocator(dev)
    # allocated (and the one fill enqueued) with `stream` as torch's current stream: the caching allocator then ties the blocks to it
    with _on_stream(stream):
        i32, f32, u8 = "int32", "float32", "uint8"
        # per level: what the fold needs — the scatter (type, cosine, scattered ray), the hits the level ended on, factor and the two shades
        hits = [new((n, 13), i32) for _ in range(depth + 1)]  # hits[k]: what level k scatters; hits[k + 1]: what its next cast found
        scat = [Scatters(new((n,), i32), new((n, 11), i32), new((n,), f32)) for _ in range(depth)]
        factor = [new((n, 3), f32) for _ in range(depth)]
        shade_next = [new((n, 3), f32) for _ in range(depth)]
        shade_missed = [new((n, 3), f32) for _ in range(depth)]
        level_rays = [new((n, 11), i32) for _ in range(2)]  # the rays that produced hits[k], in turn
        h_reflect, h_refract, h_missed = new((n, 13), i32), new((n, 13), i32), new((n, 13), i32)
        reflected = new((n, 11), i32)
        refr = Refractions(new((n,), i32), new((n,), f32), new((n, 11), i32))
        flags, index, count = new((n,), u8), new((n,), i32), new((1,), i32)
        identity, n_all = new((n,), i32), new((1,), i32)
        value = None if samples is not None else new((n, 3), f32)
        flags.fill_(1)
        shade, refract = _level_steps(scene, open_casts, n, depth > 0, dev, ray_count, s)
    select_records(flags, identity, n_all, stream=s)  # 0 .. n-1 and n: the primary casts as an indexed cast, which counts
    for e in range(n_epochs):
        cur_rays = rays
        cast_rays_indexed(scene, cur_rays, identity, n_all, hits[0], ray_count=ray_count, stream=s)  # a miss is written as "no hit"
        for k in range(depth):
            sc = scatter_hits(scene, hits[k], cur_rays, rng, stream=s, out=scat[k])  # the level's three draws; "no hit" draws nothing
            level_split(hits[k], sc.type, sc.cosine, h_reflect, h_refract, stream=s)
            reflect_rays(h_reflect, sc.rays, out=reflected, stream=s)
            refract(h_refract, sc.rays, refr)
            nxt = level_rays[k & 1]
            level_join(sc.type, sc.cosine, reflected, refr.kind, refr.rays, nxt, hits[k + 1], flags, stream=s)
            select_records(flags, index, count, stream=s)
            cast_rays_indexed(scene, nxt, index, count, hits[k + 1], ray_count=ray_count, stream=s)
            scatter_factors(scene, hits[k], cur_rays, sc.type, nxt, refr.travel, out=factor[k], stream=s)
            shade(hits[k + 1], nxt, shade_next[k])  # the mix / sum operand
            level_close(hits[k], sc.type, sc.cosine, hits[k + 1], h_missed, stream=s)
            shade(h_missed, sc.rays, shade_missed[k])  # get_shade(&scattered_hit)
            cur_rays = nxt
        v = samples[e] if samples is not None else value
        shade(hits[depth], cur_rays, v)  # depth <= 0: get_shade(&hit), main.rs:524-527
        for k in reversed(range(depth)):
            level_fold(scat[k].type, scat[k].cosine, hits[k + 1], factor[k], shade_next[k], shade_missed[k], v, stream=s)
        if accum is not None or valid is not None:  # samples alone: the folded value is the sample, nothing to filter into
            level_finish(v, accum, None if valid is None else valid[e], stream=s)
    return accum if accum is not None else samples


# ---- tree loop: ray_trace level by level — gate, split, spawn, gather and fold (include/rt_amd.h rt_tree_gate ... rt_tree_fold) ----


def tree_gate(contribution, count=None, out_flags=None, out_hits=None, stream=None):
    """The entry check of ray_trace on the roots (rt_tree_gate, main.rs:469): returns (flags, hits) — ``flags`` (N,) uint8, 1 where
    j < count and not contribution[j] < 0.001 (NaN passes), ``hits`` (N, 13) int32 preset to "no hit": select_records(flags) +
    cast_rays_indexed(rays -> hits) follow.  ``count``: a 1-element int32 CUDA tensor, or None for N."""
    n, dev = _tensor(contribution, "contribution", "float32", (None,)).shape[0], contribution.device
    _tensor(count, "count", "int32", (1,), optional=True)
    out_flags = _out_tensor(out_flags, (n,), "uint8", dev, "out_flags")
    out_hits = _out_tensor(out_hits, (n, 13), "int32", dev, "out_hits")
    _capi.check(_capi.amd_lib().rt_tree_gate(_p(contribution), n, _p(count), _p(out_flags), _p(out_hits), _stream_ptr(stream)))
    return out_flags, out_hits


def tree_split(scene: Scene, hits, contribution, depth_left: int, count=None, out_shade=None, out_reflect=None, out_refract=None,
               out_weights=None, stream=None):
    """The weights and threshold gates of main.rs:478-504 (rt_tree_split): returns (hits_shade, hits_reflect, hits_refract, weights) —
    the level's hits where get_shade, get_reflect and get_refract are wanted ("no hit" elsewhere), the operands of shade_hits,
    reflect_rays and refract_rays with the level's rays; ``weights`` (N, 4) float32 = (sc, rc, fc, opaque_decay), zeros where the record
    is not live.  ``depth_left``: TraceState.depth of the level."""
    records = _hit_records(hits)
    n, dev = records.shape[0], records.device
    _tensor(contribution, "contribution", "float32", (n,))
    _tensor(count, "count", "int32", (1,), optional=True)
    out_shade = _out_tensor(out_shade, (n, 13), "int32", dev, "out_shade")
    out_reflect = _out_tensor(out_reflect, (n, 13), "int32", dev, "out_reflect")
    out_refract = _out_tensor(out_refract, (n, 13), "int32", dev, "out_refract")
    out_weights = _out_tensor(out_weights, (n, 4), "float32", dev, "out_weights")
    _capi.check(_capi.amd_lib().rt_tree_split(scene._h, _p(records), _p(contribution), n, _p(count), int(depth_left), _p(out_shade),
                                              _p(out_reflect), _p(out_refract), _p(out_weights), _stream_ptr(stream)))
    return out_shade, out_reflect, out_refract, out_weights


def tree_spawn(hits_reflect, refr_kind, out_flags=None, out_child_values=None, stream=None):
    """The child candidates of a level (rt_tree_spawn): returns (flags, child_values) — ``flags`` (2N,) uint8, entry 2j the reflection
    child of record j (hits_reflect[j] is a hit), entry 2j + 1 its refraction child (refr_kind[j] == ESCAPED); ``child_values``
    (2N, 3) float32, zeroed, which the children's tree_fold overwrites.  select_records(flags) + tree_gather follow."""
    records = _hit_records(hits_reflect, "hits_reflect")
    n, dev = records.shape[0], records.device
    _tensor(refr_kind, "refr_kind", "int32", (n,))
    out_flags = _out_tensor(out_flags, (2 * n,), "uint8", dev, "out_flags")
    out_child_values = _out_tensor(out_child_values, (2 * n, 3), "float32", dev, "out_child_values")
    _capi.check(_capi.amd_lib().rt_tree_spawn(_p(records), _p(refr_kind), n, _p(out_flags), _p(out_child_values), _stream_ptr(stream)))
    return out_flags, out_child_values


def tree_gather(index, count, reflected, escape, contribution, weights, overflow, max_count=None, out_rays=None, out_contribution=None,
                out_parent=None, out_count=None, stream=None):
    """The next level from the selected candidates (rt_tree_gather): returns (rays, contribution, parent, count) of the children —
    child j comes from candidate c = index[j]: the reflected ray of record c >> 1 when c is even, its escape ray when odd; its
    contribution is the parent's times rc or fc, its parent slot c.  ``max_count``: the capacity of the child arrays (default: that of
    ``out_rays``, or 2N); candidates beyond it are dropped and their number is ADDED to ``overflow`` (a 1-element int32 CUDA tensor)."""
    n, dev = _tensor(reflected, "reflected", "int32", (None, 11)).shape[0], reflected.device
    _tensor(escape, "escape", "int32", (n, 11))
    _tensor(contribution, "contribution", "float32", (n,))
    _tensor(weights, "weights", "float32", (n, 4))
    _tensor(index, "index", "int32", (None,))
    _tensor(count, "count", "int32", (1,))
    _tensor(overflow, "overflow", "int32", (1,))
    if max_count is None:
        max_count = out_rays.shape[0] if out_rays is not None else 2 * n
    m = int(max_count)
    if not 0 <= min(m, 2 * n) <= index.shape[0]:
        raise ValueError("index must hold every candidate that can be kept")
    if out_rays is None:
        out_rays = _new((m, 11), "int32", dev)
    if out_contribution is None:
        out_contribution = _new((m,), "float32", dev)
    if out_parent is None:
        out_parent = _new((m,), "int32", dev)
    _tensor(out_rays, "out_rays", "int32", (None, 11))
    if out_rays.shape[0] < m or out_contribution.shape[0] < m or out_parent.shape[0] < m:
        raise ValueError("out_rays, out_contribution and out_parent must hold max_count records")
    _tensor(out_contribution, "out_contribution", "float32", (None,))
    _tensor(out_parent, "out_parent", "int32", (None,))
    out_count = _out_tensor(out_count, (1,), "int32", dev, "out_count")
    if out_count.data_ptr() == count.data_ptr():
        raise ValueError("out_count must not alias count")
    _capi.check(_capi.amd_lib().rt_tree_gather(_p(index), _p(count), m, _p(reflected), _p(escape), _p(contribution), _p(weights), n, _p(out_rays),
                                               _p(out_contribution), _p(out_parent), _p(out_count), _p(overflow), _stream_ptr(stream)))
    return out_rays, out_contribution, out_parent, out_count


def tree_fold(hits, depth_left: int, shade, out, count=None, weights=None, refr_kind=None, travel=None, child_values=None, parent=None,
              stream=None):
    """main.rs:516-518 on one level (rt_tree_fold), from the deepest back: the value of every live record j < count — black, the shade
    (depth_left <= 0) or (shade * sc + reflection * rc) + refraction * fc with the children's values of ``child_values`` — is written
    to ``out[parent[j]]``, or to ``out[j]`` when ``parent`` is None (the roots).  ``out``: an (M, 3) float32 CUDA tensor, the parent
    level's child_values or the result; a parent at or beyond M writes nothing."""
    records = _hit_records(hits)
    n = records.shape[0]
    _tensor(shade, "shade", "float32", (n, 3))
    _tensor(count, "count", "int32", (1,), optional=True)
    _tensor(out, "out", "float32", (None, 3))
    if int(depth_left) > 0 and (weights is None or refr_kind is None or travel is None or child_values is None):
        raise ValueError("weights, refr_kind, travel and child_values are required when depth_left > 0")
    _tensor(weights, "weights", "float32", (n, 4), optional=True)
    _tensor(refr_kind, "refr_kind", "int32", (n,), optional=True)
    _tensor(travel, "travel", "float32", (n,), optional=True)
    _tensor(child_values, "child_values", "float32", (2 * n, 3), optional=True)
    _tensor(parent, "parent", "int32", (n,), optional=True)
    _capi.check(_capi.amd_lib().rt_tree_fold(_p(records), _p(count), n, int(depth_left), _p(shade), _p(weights), _p(refr_kind), _p(travel),
                                             _p(child_values), _p(parent), _p(out), out.shape[0], _stream_ptr(stream)))
    return out


# the default capacity of level L is min(n * 2^L, ceil(LEVEL_CAPACITY_FACTOR * n)): DESIGN.md §3.13 has the measured level shares
LEVEL_CAPACITY_FACTOR = 1.5


def default_level_capacity(n: int, level: int) -> int:
    """Records trace_rays_levels provides for level ``level`` (0: the roots) of ``n`` rays when no ``level_capacity`` is given."""
    import math

    return min(n << min(level, 32), int(math.ceil(LEVEL_CAPACITY_FACTOR * n)))


def trace_rays_levels(scene: Scene, rays, max_depth: int, contribution=1.0, out=None, ray_count=None, stream=None, level_capacity=None,
                      check: bool = True, overflow=None, level_counts=None, open_casts: bool = False):
    """trace_rays — the same rays, depth and contribution, the same values and cast count, bit for bit — written one level of the
    recursion tree at a time from the public calls alone: the executable form of the sequence in INTEGRATION.md, to be copied and changed
    (a stopping rule, a weighting, a re-sort between levels).  ``contribution``: a float, or an (N,) float32 CUDA tensor of per-ray root
    contributions.  ``level_capacity``: the records provided for level L >= 1 — an int, a callable L -> int, or None for
    default_level_capacity; children that do not fit are dropped (their parents see black) and counted into the overflow word.
    ``check=True`` reads that word once, after the last call, and raises RtError if it is not zero; ``check=False`` reads nothing back
    and does not synchronise — the form for graph capture.  ``overflow``: a 1-element int32 CUDA tensor the dropped children are ADDED to
    (one is made and zeroed if None); ``level_counts``: a (max(max_depth, 0) + 1,) int32 CUDA tensor that receives the number of records
    cast per level.  Every buffer is allocated once, up front; after that the function only enqueues library calls on ``stream``.
    ``open_casts=True`` replaces shade_hits by shade_hits_by_light and refract_rays by refract_rays_by_bounce, each on a workspace made
    up front: every cast of the loop is then a cast_rays_indexed — on a scene walked breadth-first, that walk — with the same bits and
    count (the two add a few element-wise fills to what is enqueued).
    (Being a sequence of calls it may not be captured before select_records has run once on the stream.)"""
    return _trace_rays_levels(scene, rays, max_depth, contribution, out, ray_count, stream, level_capacity, check, overflow, level_counts, open_casts, None)


def _trace_rays_levels(scene, rays, max_depth, contribution, out, ray_count, stream, level_capacity, check, overflow, level_counts, open_casts, environment,
                       shade_step=None):
    """trace_rays_levels, and environment.trace_rays_levels: with ``environment`` (an environment.Environment) every level's tree_fold is
    followed by environment.lookup on that level's rays, hits, count and parent links, which replaces the +0 the fold wrote for the
    level's misses before the parent level folds; the levels' rays are then kept per level instead of in two buffers used in turn.  With
    None the calls enqueued are trace_rays_levels' as they always were.  ``shade_step`` (textures.trace_rays_levels): a callable
    (records of room, device) -> shade(hits, rays, out), made once, up front, which takes the place of the level's get_shade."""
    torch = _torch()
    n, dev = _tensor(rays, "rays", "int32", (None, 11)).shape[0], rays.device
    out = _out_tensor(out, (n, 3), "float32", dev)
    _count_ptr(ray_count)
    _tensor(overflow, "overflow", "int32", (1,), optional=True)
    if environment is not None:
        from .environment import Environment, lookup as environment_lookup

        if not isinstance(environment, Environment):
            raise ValueError("environment must be an environment.Environment or None")
    if max_depth > _capi.RT_MAX_DEPTH:
        raise RtError(-5, f"max_depth above RT_MAX_DEPTH ({_capi.RT_MAX_DEPTH})")
    depth = max(int(max_depth), 0)
    _tensor(level_counts, "level_counts", "int32", (depth + 1,), optional=True)
    if torch.is_tensor(contribution):
        _tensor(contribution, "contribution", "float32", (n,))
    if n == 0:
        return out
    caps = [n]
    for level in range(1, depth + 1):
        if level_capacity is None:
            cap = default_level_capacity(n, level)
        elif callable(level_capacity):
            cap = int(level_capacity(level))
        else:
            cap = int(level_capacity)
        if cap < 0:
            raise ValueError("level_capacity must not be negative")
        caps.append(min(cap, 2 * caps[-1]))  # a level cannot hold more than two children per parent record
    if 2 * max(caps) >= 1 << 32:
        raise RtError(-5, "a level of 2^31 records or more")
    top = max(caps)
    s = stream
    new = _allocator(dev)
    # allocated (and the fills enqueued) with `stream` as torch's current stream: the caching allocator then ties the blocks to it
    with _on_stream(stream):
        i32, f32, u8 = "int32", "float32", "uint8"
        # per level: what the fold needs
        hits = [new((c, 13), i32) for c in caps]
        shade = [new((c, 3), f32) for c in caps]
        weights = [new((c, 4), f32) for c in caps]
        refr_kind = [new((c,), i32) for c in caps[:depth]]
        travel = [new((c,), f32) for c in caps[:depth]]
        child_values = [new((2 * c, 3), f32) for c in caps[:depth]]
        parent = [None] + [new((c,), i32) for c in caps[1:]]
        counts = level_counts if level_counts is not None else new((depth + 1,), i32)
        count = [counts[k:k + 1] for k in range(depth + 1)]  # count[0]: the roots that passed the gate; the root arrays are full (n)
        # shared by the levels: the fold needs none of it
        h_shade, h_reflect, h_refract = new((top, 13), i32), new((top, 13), i32), new((top, 13), i32)
        reflected, escape = new((top, 11), i32), new((top, 11), i32)
        level_rays = [None, new((top, 11), i32), new((top, 11), i32)]  # children's rays and contributions, in turn
        kept_rays = [rays] + [new((c, 11), i32) for c in caps[1:]] if environment is not None else None  # the lookup wants a level's rays at its fold
        level_contribution = [None, new((top,), f32), new((top,), f32)]
        flags, index, selected = new((2 * top,), u8), new((2 * top,), i32), new((1,), i32)
        identity, n_all = new((top,), i32), new((1,), i32)
        if torch.is_tensor(contribution):
            root_contribution = contribution
        else:
            root_contribution = new((n,), f32)
            root_contribution.fill_(float(contribution))
        if overflow is None:
            overflow = new((1,), i32)
            overflow.zero_()
        counts.zero_()  # a level without room is not visited by any kernel: its count stays 0
        flags[:top].fill_(1)
        shade_level, refract = _level_steps(scene, open_casts, top, depth > 0, dev, ray_count, s)
        if shade_step is not None:
            shade_level = shade_step(top, dev)
    select_records(flags[:top], identity, n_all, stream=s)  # 0 .. top-1: the child levels are cast through it with their own counts
    cur_rays, cur_contribution = rays, root_contribution
    for k in range(depth + 1):
        c, left = caps[k], depth - k
        live = None if k == 0 else count[k]
        if k == 0:
            tree_gate(cur_contribution, None, flags[:c], hits[0], stream=s)
            select_records(flags[:c], index[:c], count[0], stream=s)
            cast_rays_indexed(scene, cur_rays, index[:c], count[0], hits[0], ray_count=ray_count, stream=s)
        else:
            cast_rays_indexed(scene, cur_rays[:c], identity[:c], count[k], hits[k], ray_count=ray_count, stream=s)
        tree_split(scene, hits[k], cur_contribution[:c], left, live, h_shade[:c], h_reflect[:c], h_refract[:c], weights[k], stream=s)
        shade_level(h_shade[:c], cur_rays[:c], shade[k])
        if left > 0:
            reflect_rays(h_reflect[:c], cur_rays[:c], out=reflected[:c], stream=s)
            refract(h_refract[:c], cur_rays[:c], Refractions(refr_kind[k], travel[k], escape[:c]))
            tree_spawn(h_reflect[:c], refr_kind[k], flags[:2 * c], child_values[k], stream=s)
            select_records(flags[:2 * c], index[:2 * c], selected, stream=s)
            nxt = 1 + (k & 1)
            next_rays = level_rays[nxt] if kept_rays is None else kept_rays[k + 1]
            tree_gather(index[:2 * c], selected, reflected[:c], escape[:c], cur_contribution[:c], weights[k], overflow, caps[k + 1],
                        next_rays, level_contribution[nxt], parent[k + 1], count[k + 1], stream=s)
            cur_rays, cur_contribution = next_rays, level_contribution[nxt]
    for k in reversed(range(depth + 1)):
        left = depth - k
        tree_fold(hits[k], left, shade[k], out if k == 0 else child_values[k - 1], None if k == 0 else count[k],
                  weights[k] if left > 0 else None, refr_kind[k] if left > 0 else None, travel[k] if left > 0 else None,
                  child_values[k] if left > 0 else None, parent[k], stream=s)
        if kept_rays is not None:  # the sky behind the level's misses, into the slots the fold just wrote +0 to
            environment_lookup(environment, kept_rays[k][:caps[k]], hits[k], None if k == 0 else count[k], parent[k],
                               out if k == 0 else child_values[k - 1], stream=s)
    if check:
        with _on_stream(stream):
            dropped = int(overflow.item())  # the one readback: it waits for the loop
        if dropped != 0:
            raise RtError(-5, f"trace_rays_levels: {dropped} child records did not fit their level's capacity (level_capacity)")
    return out


def _level_steps(scene, open_casts, n, refract_too, device, ray_count, stream):
    """The ``open_casts`` switch of the two loops: (shade, refract) — get_shade and get_refract(100.0) of (hits, rays) into ``out``, as
    one kernel each, or light by light and bounce by bounce on workspaces made here for ``n`` records (none for refract unless
    ``refract_too``: a loop of depth 0 never refracts)"""
    if not open_casts:
        return (lambda hits, rays, out: shade_hits(scene, hits, rays, out=out, ray_count=ray_count, stream=stream),
                lambda hits, rays, out: refract_rays(scene, hits, rays, 100.0, ray_count=ray_count, stream=stream, out=out))
    lws = light_workspace(scene, n, device)
    rws = refract_workspace(n, device) if refract_too else None
    return (lambda hits, rays, out: shade_hits_by_light(scene, hits, rays, out=out, ray_count=ray_count, stream=stream, workspace=lws),
            lambda hits, rays, out: refract_rays_by_bounce(scene, hits, rays, 100.0, ray_count=ray_count, stream=stream, out=out,
                                                           workspace=rws))
