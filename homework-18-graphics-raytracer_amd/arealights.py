"""Area-light queries (include/rt_amd.h "area-light queries"): soft shadows from lights that have a radius, on caller-supplied hits.

The light queries (rt.light_rays / light_terms / light_fold) evaluated ``spp`` times per (hit, light) pair, each time with the light
moved to a point chosen on the sphere of its radius, and a fold that averages a light's samples — the noisy input that film, temporal,
svgf and upsample are there to clean.  With every radius 0 and one sample it is rt.shade_hits_by_light, and so rt.shade_hits, bit for
bit.

    rays / terms / fold    rt_area_light_rays / rt_area_light_terms / rt_area_light_fold
    samples_numpy          the sampler on the CPU (rt_area_light_samples_cpu of librt_host.so): rays' ``sample``, bit for bit
    shade_hits_soft        the loop, written from the public calls alone: to be copied and changed

Arrays are sample-major, then light-major: entry (s * L + (l - light_first)) * N + i belongs to sample s, light l and hit i.
"""
from __future__ import annotations

import numpy as np

from . import _capi
from ._args import _below_2_32, _count_ptr, _new, _on_stream, _out_tensor, _p, _room, _samples, _stream_ptr, _tensor, _void
from ._capi import Light, SceneDesc
from ._opened import _light_range
from ._queries import _hit_records, _hits_and_rays, cast_rays_indexed, select_records
from ._world import Scene, World

UNIFORM, STRATIFIED = 1, 2  # RT_FILM_UNIFORM / RT_FILM_STRATIFIED (RT_FILM_CENTER, 0, is no pattern of an area light)
MAX_SPP = 64


def rays(scene: Scene, hits, rays, radii, spp: int, pattern: int = STRATIFIED, seed: int = 0, ids=None, light_first: int = 0, light_count=None,
         out_rays=None, out_asks=None, out_sample=None, stream=None):
    """rt_area_light_rays: returns (shadow_rays, asks, sample) for ``spp`` samples of the lights light_first .. light_first + light_count
    - 1 (default: every light from light_first on).  ``radii`` (L,) float32 CUDA: the radius of each light of the range; ``ids`` (N,)
    int32 CUDA or None: the record id of the hash (the global pixel index, say; None: the record's number).  ``sample`` (S*L*N, 3)
    float32: the displaced origin — direction, for a directional light without origin — of every entry; ``asks`` (S*L*N,) uint8 and
    ``shadow_rays`` (S*L*N, 11) int32: what light_rays gives for the displaced light — one batch for select_records(asks) +
    cast_rays_indexed."""
    records, n = _hits_and_rays(hits, rays)
    first, count = _light_range(scene, light_first, light_count)
    spp = _samples(spp)
    _tensor(radii, "radii", "float32", (count,))
    _tensor(ids, "ids", "int32", (n,), optional=True)
    entries = spp * count * n
    dev = records.device
    out_rays = _out_tensor(out_rays, (entries, 11), "int32", dev, "out_rays")
    out_asks = _out_tensor(out_asks, (entries,), "uint8", dev, "out_asks")
    out_sample = _out_tensor(out_sample, (entries, 3), "float32", dev, "out_sample")
    _capi.check(_capi.amd_lib().rt_area_light_rays(scene._h, _p(records), _p(rays), n, first, count, _p(radii), _p(ids), spp, int(pattern),
                                                   int(seed) & 0xFFFFFFFF, _p(out_rays), _p(out_asks), _p(out_sample), _stream_ptr(stream)))
    return out_rays, out_asks, out_sample


_area_rays = rays  # shade_hits_soft has a parameter of that name


def terms(scene: Scene, hits, rays, asks, sample, shadow_hits, spp: int, light_first: int = 0, light_count=None, out_lit=None, out_diffuse=None,
          out_specular=None, stream=None):
    """rt_area_light_terms: returns (lit, diffuse, specular), laid out as rays' outputs: light_terms with each light moved to
    ``sample`` (S*L*N, 3) — the occlusion distance is measured to it, and the Phong terms see that light.  ``sample`` is the caller's:
    what rays wrote, or points of its own (a quad light, another sampling scheme).  ``shadow_hits`` (S*L*N, 13) int32: what a cast of
    the shadow rays wrote, read only where ``asks`` is set."""
    records, n = _hits_and_rays(hits, rays)
    first, count = _light_range(scene, light_first, light_count)
    spp = _samples(spp)
    entries = spp * count * n
    dev = records.device
    _tensor(asks, "asks", "uint8", (entries,))
    _tensor(sample, "sample", "float32", (entries, 3))
    _tensor(shadow_hits, "shadow_hits", "int32", (entries, 13))
    out_lit = _out_tensor(out_lit, (entries,), "uint8", dev, "out_lit")
    out_diffuse = _out_tensor(out_diffuse, (entries, 3), "float32", dev, "out_diffuse")
    out_specular = _out_tensor(out_specular, (entries, 3), "float32", dev, "out_specular")
    _capi.check(_capi.amd_lib().rt_area_light_terms(scene._h, _p(records), _p(rays), n, first, count, spp, _p(asks), _p(sample), _p(shadow_hits),
                                                    _p(out_lit), _p(out_diffuse), _p(out_specular), _stream_ptr(stream)))
    return out_lit, out_diffuse, out_specular


def fold(scene: Scene, hits, lit, diffuse, specular, out, spp: int, visibility=None, stream=None):
    """rt_area_light_fold: for the L = len(lit) / (spp * N) lights in order, the mean over a light's samples — the lit ones summed in
    ascending order, divided by ``spp`` — then out = (out + D * (1 - shiness)) + S * shiness, in place on ``out`` ((N, 3) float32,
    required).  The call ADDS: zero ``out`` before the first range of lights.  ``visibility`` (L*N,) float32 or None: the share of lit
    samples per (light, hit), 0 for a record that is no hit — the shadow mask of each light.  A record that is no hit is not written
    in ``out``."""
    records = _hit_records(hits)
    n = records.shape[0]
    spp = _samples(spp)
    _tensor(out, "out", "float32", (n, 3))
    entries = _tensor(lit, "lit", "uint8", (None,)).shape[0]
    per_light = spp * n
    if entries % per_light != 0 if per_light else entries != 0:
        raise ValueError("lit must have one entry per (sample, light, hit)")
    count = entries // per_light if per_light else 0
    _tensor(diffuse, "diffuse", "float32", (entries, 3))
    _tensor(specular, "specular", "float32", (entries, 3))
    _tensor(visibility, "visibility", "float32", (count * n,), optional=True)
    _capi.check(_capi.amd_lib().rt_area_light_fold(scene._h, _p(records), n, count, spp, _p(lit), _p(diffuse), _p(specular), _p(out), _p(visibility),
                                                   _stream_ptr(stream)))
    return out


def samples_numpy(lights, radii, n: int, spp: int, pattern: int = STRATIFIED, seed: int = 0, ids=None, light_first: int = 0, light_count=None) -> np.ndarray:
    """rt_area_light_samples_cpu: what rays writes into ``sample``, bit for bit, on the CPU: an (S, L, N, 3) float32 array.  ``lights``:
    a World, a SceneDesc or a sequence of Light — the scene's lights, indexed as the scene indexes them; ``radii``: L floats, the range's;
    ``ids``: N record ids or None for 0 .. N - 1."""
    if isinstance(lights, World):
        lights = lights.desc()
    if isinstance(lights, SceneDesc):
        desc = lights
        lights = [desc.lights[l] for l in range(desc.n_lights)]
    arr = (Light * max(len(lights), 1))(*lights)
    first = int(light_first)
    count = len(lights) - first if light_count is None else int(light_count)
    n, spp = int(n), _samples(spp)
    if first < 0 or count < 0 or n < 0 or first + count > len(lights):
        raise ValueError(f"lights {first} .. {first + count} of {len(lights)}")
    radii = np.ascontiguousarray(radii, dtype=np.float32)
    if radii.shape != (count,):
        raise ValueError(f"radii: expected {count} floats, one per light of the range")
    if ids is not None:
        ids = np.ascontiguousarray(ids).astype(np.uint32, copy=False)
        if ids.shape != (n,):
            raise ValueError(f"ids: expected an ({n},) array")
    out = np.zeros((spp, count, n, 3), dtype=np.float32)
    _capi.check_host(_capi.host_lib().rt_area_light_samples_cpu(arr, first, count, _void(radii), _void(ids), n, spp, int(pattern), int(seed) & 0xFFFFFFFF,
                                                                _void(out)))
    return out


class Workspace:
    """The buffers of one pass of shade_hits_soft, made once by workspace() so that a caller's loop allocates nothing: ``entries``
    (sample, light, hit) entries of room, about 138 B each."""

    def __init__(self, entries: int, device):
        self.entries = int(entries)
        self.shadow_rays, self.shadow_hits = _new((entries, 11), "int32", device), _new((entries, 13), "int32", device)
        self.asks, self.lit = _new((entries,), "uint8", device), _new((entries,), "uint8", device)
        self.index, self.count = _new((entries,), "int32", device), _new((1,), "int32", device)
        self.sample = _new((entries, 3), "float32", device)
        self.diffuse, self.specular = _new((entries, 3), "float32", device), _new((entries, 3), "float32", device)


def workspace(scene: Scene, n: int, device, spp: int, lights_per_pass=None) -> Workspace:
    """A Workspace for shade_hits_soft on up to ``n`` hits of ``scene`` with ``spp`` samples, ``lights_per_pass`` lights at a time
    (default: all)."""
    per_pass = scene.n_lights if lights_per_pass is None else min(int(lights_per_pass), scene.n_lights)
    if per_pass < 0 or n < 0 or spp < 0:
        raise ValueError("n, spp and lights_per_pass must not be negative")
    return Workspace(int(n) * per_pass * int(spp), device)


def shade_hits_soft(scene: Scene, hits, rays, radii, spp: int = 16, pattern: int = STRATIFIED, seed: int = 0, ids=None, out=None, visibility=None,
                    ray_count=None, stream=None, lights_per_pass=None, workspace=None):
    """shade_hits with soft shadows: every light l is a sphere of radius ``radii[l]`` ((n_lights,) float32 CUDA), sampled ``spp``
    times per hit.  Written from the public calls alone, as rt.shade_hits_by_light is — the executable form of the sequence in
    INTEGRATION.md, to be copied and changed.  Zero ``out``; then per range of ``lights_per_pass`` lights (default: all of them — it
    bounds the memory): rays -> select_records(asks) -> cast_rays_indexed(shadow rays -> shadow hits, ray_count) -> terms -> fold.
    ``visibility`` ((n_lights * N,) float32 CUDA or None): the share of lit samples per (light, hit), light-major.  With every radius
    0 the values are shade_hits', bit for bit, and the casts ``spp`` times its casts.  Every buffer is allocated once, up front — or
    none at all with ``out`` and ``workspace`` (a Workspace); after that the function only enqueues library calls on ``stream`` and
    reads nothing back.  (Being a sequence of calls it may not be captured before select_records — and, on a scene walked
    breadth-first, cast_rays_indexed — has run once on the stream.)"""
    records, n = _hits_and_rays(hits, rays)
    dev = records.device
    lights = scene.n_lights
    spp = _samples(spp)
    _tensor(radii, "radii", "float32", (lights,))
    _tensor(ids, "ids", "int32", (n,), optional=True)
    _tensor(visibility, "visibility", "float32", (lights * n,), optional=True)
    out = _out_tensor(out, (n, 3), "float32", dev)
    _count_ptr(ray_count)
    per_pass = lights if lights_per_pass is None else int(lights_per_pass)
    if lights_per_pass is not None and per_pass < 1:
        raise ValueError("lights_per_pass must be at least 1")
    per_pass = min(per_pass, lights)
    _below_2_32(n * per_pass * spp, "(sample, light, hit) entries", " in one pass (lights_per_pass)")
    s = stream
    with _on_stream(stream):  # the fill is enqueued with `stream` as torch's current stream
        out.zero_()
    if n == 0 or lights == 0:
        return out
    entries = per_pass * n * spp
    w = _room(workspace, Workspace, {"entries": entries},
              f"an arealights.Workspace with room for {entries} (sample, light, hit) entries (arealights.workspace)", dev, stream)
    for first in range(0, lights, per_pass):
        c = min(per_pass, lights - first)
        m = c * n * spp
        _area_rays(scene, records, rays, radii[first:first + c], spp, pattern, seed, ids, first, c, w.shadow_rays[:m], w.asks[:m], w.sample[:m], stream=s)
        select_records(w.asks[:m], w.index[:m], w.count, stream=s)
        cast_rays_indexed(scene, w.shadow_rays[:m], w.index[:m], w.count, w.shadow_hits[:m], ray_count=ray_count, stream=s)
        terms(scene, records, rays, w.asks[:m], w.sample[:m], w.shadow_hits[:m], spp, first, c, w.lit[:m], w.diffuse[:m], w.specular[:m], stream=s)
        fold(scene, records, w.lit[:m], w.diffuse[:m], w.specular[:m], out, spp, None if visibility is None else visibility[first * n:(first + c) * n],
             stream=s)
    return out
