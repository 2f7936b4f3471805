"""Texture queries (include/rt_amd.h "texture queries"): mip-mapped image textures and normal maps on caller-supplied hits.

The reference's GenerativeMaterial takes two closures of uv; the library enumerates the three main.rs holds.  A Texture is an image
behind such a closure: ``apply`` edits the rt_surface records materials.material_hits wrote — diffuse_color from an image, normal from a
normal map, shading_normal by the reference's own adjust_normal — and ``light_terms_surfaces`` is light_terms on those records, so an
edited surface reaches get_shade's own lights.

    Texture / HostTexture                          a pyramid on the device (built on creation) / in a numpy array
    pyramid / footprint / sample / apply / light_terms_surfaces
                                                    rt_texture_pyramid / _footprint / _sample / _surfaces / rt_light_terms_surfaces
    pyramid_numpy / footprint_numpy / sample_numpy / apply_numpy
                                                    the CPU forms (rt_texture_*_cpu of librt_host.so): the device's bits
    levels / pyramid_floats                         rt_texture_levels / rt_texture_pyramid_floats
    Binding                                         which textures go onto which object's surfaces
    shade_hits_textured                             shade_hits_by_light with material_hits -> apply per binding -> light_terms_surfaces
    trace_rays_levels                               rt.trace_rays_levels with the keywords ``bindings`` and ``spread``
                                                    — both written from the public calls alone: to be copied and changed
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi
from ._args import _below_2_32, _count_ptr, _new, _on_stream, _out_tensor, _p, _stream_ptr, _tensor, _torch, _void
from ._loops import _trace_rays_levels
from ._opened import LightWorkspace, _light_range, light_fold, light_rays, shade_hits_by_light
from ._queries import _hit_records, _hits_and_rays, cast_rays_indexed, select_records
from ._world import Scene, World
from .materials import material_hits

NEAREST, BILINEAR, TRILINEAR = 0, 1, 2  # RT_TEX_NEAREST / RT_TEX_BILINEAR / RT_TEX_TRILINEAR
REPEAT, CLAMP = 0, 1                    # RT_TEX_REPEAT / RT_TEX_CLAMP
MODULATE, NORMALIZE = 1, 2              # RT_TEX_MODULATE / RT_TEX_NORMALIZE
ALL_OBJECTS = 0xFFFFFFFF                # RT_TEX_ALL_OBJECTS
MAX_SIDE = 16384


def levels(width: int, height: int) -> int:
    """rt_texture_levels: 1 + floor(log2(max(width, height))); 0 for a side of 0."""
    if not (0 <= int(width) < 1 << 32 and 0 <= int(height) < 1 << 32):
        return 0
    return int(_capi.amd_lib().rt_texture_levels(int(width), int(height)))


def pyramid_floats(width: int, height: int, n_levels: int) -> int:
    """rt_texture_pyramid_floats: the float32 of levels 0 .. n_levels - 1, or 0 for a texture over the limits."""
    if not all(0 <= int(v) < 1 << 32 for v in (width, height, n_levels)):
        return 0
    return int(_capi.amd_lib().rt_texture_pyramid_floats(int(width), int(height), int(n_levels)))


def level_extent(width: int, height: int, level: int):
    """(width, height) of level ``level``"""
    return max(1, int(width) >> level), max(1, int(height) >> level)


class _Pyramid:
    """what Texture and HostTexture share: the descriptor's fields and the levels as views of ``texels`` (flat float32)"""

    def _describe(self, width, height, n_levels, filter, wrap_u, wrap_v, scale, offset):
        self.width, self.height = int(width), int(height)
        self.n_levels = levels(self.width, self.height) if n_levels is None else int(n_levels)
        self.filter, self.wrap_u, self.wrap_v = int(filter), int(wrap_u), int(wrap_v)
        self.scale, self.offset = (float(scale[0]), float(scale[1])), (float(offset[0]), float(offset[1]))
        self.floats = pyramid_floats(self.width, self.height, self.n_levels)
        if self.floats == 0:
            raise ValueError(f"a texture of 1 .. {MAX_SIDE} texels each way with 1 .. levels(width, height) levels is required")

    def _desc(self, pointer) -> _capi.TextureDesc:
        return _capi.TextureDesc(pointer, self.width, self.height, self.n_levels, self.filter, self.wrap_u, self.wrap_v,
                                 (C.c_float * 2)(*self.scale), (C.c_float * 2)(*self.offset))

    def level(self, l: int):
        """level ``l`` as an (h, w, 3) view of the pyramid"""
        if not 0 <= l < self.n_levels:
            raise ValueError("no such level")
        start = sum(3 * w * h for w, h in (level_extent(self.width, self.height, k) for k in range(l)))
        w, h = level_extent(self.width, self.height, l)
        return self.texels[start:start + 3 * w * h].reshape(h, w, 3)


class Texture(_Pyramid):
    """A texture on the device: ``image`` (H, W, 3) float32 — a numpy array or a tensor, copied — becomes level 0 of a pyramid of
    ``n_levels`` levels (None: all of them) the Texture owns, ``texels`` (a flat float32 CUDA tensor), built on creation by ``pyramid``
    on ``stream``.  ``filter``: NEAREST, BILINEAR or TRILINEAR; ``wrap_u`` / ``wrap_v``: REPEAT or CLAMP; uv maps to uv * scale +
    offset.  The fields may be changed afterwards; ``desc`` is the rt_texture passed to the library.  Texture.over(texels, ...) wraps a
    pyramid tensor of the caller's without building anything."""

    def __init__(self, image, filter: int = TRILINEAR, wrap_u: int = REPEAT, wrap_v: int = REPEAT, scale=(1.0, 1.0), offset=(0.0, 0.0), n_levels=None,
                 device="cuda", stream=None):
        torch = _torch()
        image = torch.as_tensor(image)
        if image.dim() != 3 or image.shape[2] != 3 or image.dtype != torch.float32:
            raise ValueError("image: expected an (H, W, 3) float32 array or tensor")
        self._describe(image.shape[1], image.shape[0], n_levels, filter, wrap_u, wrap_v, scale, offset)
        with _on_stream(stream):
            self.texels = _new((self.floats,), "float32", image.device if image.is_cuda else device)
            self.texels[:3 * self.width * self.height].copy_(image.reshape(-1), non_blocking=False)
        pyramid(self, stream=stream)

    @classmethod
    def over(cls, texels, width: int, height: int, n_levels=None, filter: int = TRILINEAR, wrap_u: int = REPEAT, wrap_v: int = REPEAT,
             scale=(1.0, 1.0), offset=(0.0, 0.0)):
        self = cls.__new__(cls)
        self._describe(width, height, n_levels, filter, wrap_u, wrap_v, scale, offset)
        self.texels = _tensor(texels, "texels", "float32", (self.floats,))
        return self

    @property
    def desc(self) -> _capi.TextureDesc:
        return self._desc(self.texels.data_ptr())


class HostTexture(_Pyramid):
    """The same in a numpy array, for the CPU forms: ``texels`` is a flat float32 array, built by pyramid_numpy on creation."""

    def __init__(self, image, filter: int = TRILINEAR, wrap_u: int = REPEAT, wrap_v: int = REPEAT, scale=(1.0, 1.0), offset=(0.0, 0.0), n_levels=None):
        image = np.ascontiguousarray(image, dtype=np.float32)
        if image.ndim != 3 or image.shape[2] != 3:
            raise ValueError("image: expected an (H, W, 3) float32 array")
        self._describe(image.shape[1], image.shape[0], n_levels, filter, wrap_u, wrap_v, scale, offset)
        self.texels = np.zeros(self.floats, dtype=np.float32)
        self.texels[:image.size] = image.reshape(-1)
        pyramid_numpy(self)

    @classmethod
    def over(cls, texels, width: int, height: int, n_levels=None, filter: int = TRILINEAR, wrap_u: int = REPEAT, wrap_v: int = REPEAT,
             scale=(1.0, 1.0), offset=(0.0, 0.0)):
        self = cls.__new__(cls)
        self._describe(width, height, n_levels, filter, wrap_u, wrap_v, scale, offset)
        if not (isinstance(texels, np.ndarray) and texels.dtype == np.float32 and texels.shape == (self.floats,) and texels.flags.c_contiguous):
            raise ValueError(f"texels: expected a contiguous ({self.floats},) float32 array")
        self.texels = texels
        return self

    @property
    def desc(self) -> _capi.TextureDesc:
        return self._desc(self.texels.ctypes.data)


def _texture(tex, name="tex", optional=False):
    if tex is None and optional:
        return None
    if not isinstance(tex, Texture):
        raise ValueError(f"{name} must be a textures.Texture")
    return tex


def _host_texture(tex, name="tex", optional=False):
    if tex is None and optional:
        return None
    if not isinstance(tex, HostTexture):
        raise ValueError(f"{name} must be a textures.HostTexture")
    return tex


def _ref(desc):
    return None if desc is None else C.byref(desc)


# ---- the device calls ----

def pyramid(tex: Texture, stream=None) -> Texture:
    """rt_texture_pyramid: levels 1 and up of ``tex`` from its level 0, in place — the exact box filter for any extent, one launch per
    level while the source is above 32 texels either way, then one workgroup for all the rest.  Call it again after writing level 0."""
    _capi.check(_capi.amd_lib().rt_texture_pyramid(C.byref(_texture(tex).desc), _stream_ptr(stream)))
    return tex


def footprint(scene: Scene, hits, incoming, spread: float, width0=None, out=None, stream=None):
    """rt_texture_footprint: the uv-space length a ray cone covers at each hit — (width0 + spread * distance) over the cosine, times the
    primitive's uv length per surface length.  ``incoming`` (N, 11) int32: the rays that produced the hits; ``width0`` (N,) float32 or
    None for 0.  Returns ``out``, (N,) float32: +0 for a record that is no hit, a primitive without area and a result that is not
    finite."""
    records, n = _hits_and_rays(hits, incoming)
    _tensor(width0, "width0", "float32", (n,), optional=True)
    out = _out_tensor(out, (n,), "float32", records.device)
    _capi.check(_capi.amd_lib().rt_texture_footprint(scene._h, _p(records), _p(incoming), n, float(spread), _p(width0), _p(out), _stream_ptr(stream)))
    return out


_footprint = footprint  # the sequences have arguments of that name


def _strided(t, name, width):
    """an (N, width) float32 CUDA tensor whose rows may lie inside records: -> (N, the row stride in words)"""
    _tensor(t, name, "float32", (None, width), contiguous=False)
    if t.shape[0] and t.stride(1) != 1:
        raise ValueError(f"{name}: the {width} words of a row must be adjacent")
    return t.shape[0], (t.stride(0) if t.shape[0] > 1 else width)


def sample(tex: Texture, uv, footprint=None, out=None, stream=None):
    """rt_texture_sample: the filtered lookup at ``uv`` ((N, 2) float32, possibly a strided view: hits.view(torch.float32)[:, 9:11]
    reads the uv inside the hit records) with ``footprint`` ((N,) float32 or None for 0; read by TRILINEAR alone).  ``out``: (N, 3)
    float32, possibly a strided view into records of the caller's (allocated if None).  A uv that is not finite gives zeros."""
    tex = _texture(tex)
    n, uv_stride = _strided(uv, "uv", 2)
    _tensor(footprint, "footprint", "float32", (n,), optional=True)
    if out is None:
        with _on_stream(stream):
            out = _new((n, 3), "float32", uv.device)
    rows, out_stride = _strided(out, "out", 3)
    if rows != n:
        raise ValueError("out must hold one row per uv")
    _capi.check(_capi.amd_lib().rt_texture_sample(C.byref(tex.desc), _p(uv), uv_stride, _p(footprint), n, _p(out), out_stride, _stream_ptr(stream)))
    return out


def apply(surfaces, hits, diffuse: Texture = None, normal: Texture = None, footprint=None, object_index: int = ALL_OBJECTS, flags: int = 0, stream=None):
    """rt_texture_surfaces: ``surfaces`` ((N, 18) int32, materials.material_hits) edited in place where valid, the hit's object_index
    is ``object_index`` (ALL_OBJECTS: any) and its uv is finite: diffuse_color from ``diffuse`` (times the old colour with MODULATE),
    normal from ``normal`` (over its length with NORMALIZE) and shading_normal = adjust_normal(normal, hit.normal).  Returns
    ``surfaces``."""
    records = _hit_records(hits)
    n = records.shape[0]
    _tensor(surfaces, "surfaces", "int32", (n, 18))
    _tensor(footprint, "footprint", "float32", (n,), optional=True)
    d, m = _texture(diffuse, "diffuse", True), _texture(normal, "normal", True)
    _capi.check(_capi.amd_lib().rt_texture_surfaces(_ref(d and d.desc), _ref(m and m.desc), _p(records), _p(footprint), n, int(object_index) & 0xFFFFFFFF,
                                                    int(flags), _p(surfaces), _stream_ptr(stream)))
    return surfaces


def light_terms_surfaces(scene: Scene, surfaces, hits, rays, asks, shadow_hits, light_first: int = 0, light_count=None, out_lit=None, out_diffuse=None,
                         out_specular=None, stream=None):
    """rt_light_terms_surfaces: light_terms with the material and the shading normal taken from ``surfaces`` ((N, 18) int32) instead
    of the scene.  On material_hits' records, unedited, it returns light_terms' (lit, diffuse, specular) bit for bit."""
    records, n = _hits_and_rays(hits, rays)
    _tensor(surfaces, "surfaces", "int32", (n, 18))
    first, count = _light_range(scene, light_first, light_count)
    pairs = count * n
    dev = records.device
    _tensor(asks, "asks", "uint8", (pairs,))
    _tensor(shadow_hits, "shadow_hits", "int32", (pairs, 13))
    out_lit = _out_tensor(out_lit, (pairs,), "uint8", dev, "out_lit")
    out_diffuse = _out_tensor(out_diffuse, (pairs, 3), "float32", dev, "out_diffuse")
    out_specular = _out_tensor(out_specular, (pairs, 3), "float32", dev, "out_specular")
    _capi.check(_capi.amd_lib().rt_light_terms_surfaces(scene._h, _p(surfaces), _p(records), _p(rays), n, first, count, _p(asks), _p(shadow_hits),
                                                        _p(out_lit), _p(out_diffuse), _p(out_specular), _stream_ptr(stream)))
    return out_lit, out_diffuse, out_specular


# ---- the CPU forms ----

def _host_words(a, words, name):
    a = np.asarray(a)
    if a.dtype.itemsize != 4 * words and not (a.ndim == 2 and a.shape[1] == words and a.dtype.itemsize == 4):
        raise ValueError(f"{name}: expected records of {words} 4-byte words")
    a = np.ascontiguousarray(a)
    return a, (a.shape[0] if a.ndim else 1)


def _host_strided(a, width):
    """an (N, width) float32 array whose rows may lie inside records, taken as it is: -> (the array, N, the row stride in words)"""
    if not (isinstance(a, np.ndarray) and a.dtype == np.float32 and a.ndim == 2 and a.shape[1] == width):
        a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1, width)
    if a.shape[0] and (a.strides[1] != 4 or a.strides[0] % 4 or a.strides[0] < 4 * width):
        a = np.ascontiguousarray(a)
    return a, a.shape[0], (a.strides[0] // 4 if a.shape[0] > 1 else width)


def _host_plane(a, n, name):
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.shape != (n,):
        raise ValueError(f"{name}: expected an ({n},) float32 array")
    return a


def pyramid_numpy(tex: HostTexture) -> HostTexture:
    """rt_texture_pyramid_cpu: pyramid on the CPU, bit for bit, in place in ``tex.texels``."""
    _capi.check_host(_capi.host_lib().rt_texture_pyramid_cpu(C.byref(_host_texture(tex).desc)))
    return tex


def footprint_numpy(world_or_desc, hits, incoming, spread: float, width0=None) -> np.ndarray:
    """rt_texture_footprint_cpu: footprint on the CPU, bit for bit.  ``world_or_desc``: the World or SceneDesc the hits were cast on, as
    it stands now; ``hits`` (N, 13) and ``incoming`` (N, 11) 4-byte words (or HIT_DTYPE / RAY_DTYPE arrays).  Returns (N,) float32."""
    desc = world_or_desc.desc() if isinstance(world_or_desc, World) else world_or_desc
    hits, n = _host_words(hits, 13, "hits")
    incoming, m = _host_words(incoming, 11, "incoming")
    if m != n:
        raise ValueError("incoming must hold one ray per hit")
    width0 = _host_plane(width0, n, "width0")
    out = np.zeros(n, dtype=np.float32)
    _capi.check_host(_capi.host_lib().rt_texture_footprint_cpu(C.byref(desc), _void(hits), _void(incoming), n, float(spread), _void(width0), _void(out)))
    return out


def sample_numpy(tex: HostTexture, uv, footprint=None, out=None) -> np.ndarray:
    """rt_texture_sample_cpu: sample on the CPU, bit for bit.  ``uv`` (N, 2) float32 and ``out`` (N, 3) float32 (None: a new array) may
    be strided views of record arrays: they are read and written where they lie."""
    tex = _host_texture(tex)
    uv, n, uv_stride = _host_strided(uv, 2)
    footprint = _host_plane(footprint, n, "footprint")
    if out is None:
        out = np.zeros((n, 3), dtype=np.float32)
    given = out
    out, m, out_stride = _host_strided(out, 3)
    if m != n or (out is not given and n):
        raise ValueError("out: expected an (N, 3) float32 array with adjacent words in a row")
    _capi.check_host(_capi.host_lib().rt_texture_sample_cpu(C.byref(tex.desc), _void(uv), uv_stride, _void(footprint), n, _void(out), out_stride))
    return given


def apply_numpy(surfaces, hits, diffuse: HostTexture = None, normal: HostTexture = None, footprint=None, object_index: int = ALL_OBJECTS, flags: int = 0,
                in_place: bool = False) -> np.ndarray:
    """rt_texture_surfaces_cpu: apply on the CPU, bit for bit.  ``surfaces``: a SURFACE_DTYPE array or (N, 18) 4-byte words; a copy is
    edited and returned unless ``in_place`` (then ``surfaces`` must be contiguous)."""
    hits, n = _host_words(hits, 13, "hits")
    given = surfaces
    surfaces, m = _host_words(surfaces, 18, "surfaces")
    if m != n:
        raise ValueError("surfaces must hold one record per hit")
    if in_place and surfaces is not given:
        raise ValueError("surfaces: in_place needs a contiguous array")
    if not in_place:
        surfaces = surfaces.copy()
    footprint = _host_plane(footprint, n, "footprint")
    d, m_ = _host_texture(diffuse, "diffuse", True), _host_texture(normal, "normal", True)
    _capi.check_host(_capi.host_lib().rt_texture_surfaces_cpu(_ref(d and d.desc), _ref(m_ and m_.desc), _void(hits), _void(footprint), n,
                                                              int(object_index) & 0xFFFFFFFF, int(flags), _void(surfaces)))
    return surfaces


# ---- the two sequences ----

class Binding:
    """Which textures go onto which surfaces: ``diffuse`` and ``normal`` (Textures or None) on the hits of object ``object_index``
    (ALL_OBJECTS: every hit), with ``flags`` (MODULATE, NORMALIZE)."""

    def __init__(self, diffuse: Texture = None, normal: Texture = None, object_index: int = ALL_OBJECTS, flags: int = 0):
        self.diffuse, self.normal = _texture(diffuse, "diffuse", True), _texture(normal, "normal", True)
        self.object_index, self.flags = int(object_index), int(flags)

    def wants_footprint(self) -> bool:
        return any(t is not None and t.filter == TRILINEAR and t.n_levels > 1 for t in (self.diffuse, self.normal))


def _bindings(bindings):
    bindings = [] if bindings is None else list(bindings)
    if not all(isinstance(b, Binding) for b in bindings):
        raise ValueError("bindings must be textures.Binding objects")
    return bindings


class Workspace:
    """The buffers of shade_hits_textured, made once by workspace() so that a caller's loop allocates nothing: a LightWorkspace of
    ``pairs`` (hit, light) pairs, and the surfaces and footprints of ``n`` records (76 B each)."""

    def __init__(self, n: int, pairs: int, device):
        self.n = int(n)
        self.light = LightWorkspace(pairs, device)
        self.surfaces, self.footprint = _new((n, 18), "int32", device), _new((n,), "float32", device)


def workspace(scene: Scene, n: int, device, lights_per_pass=None) -> Workspace:
    """A Workspace for shade_hits_textured on up to ``n`` hits of ``scene``, ``lights_per_pass`` lights at a time (default: all)."""
    per_pass = scene.n_lights if lights_per_pass is None else min(int(lights_per_pass), scene.n_lights)
    if per_pass < 0 or n < 0:
        raise ValueError("n and lights_per_pass must not be negative")
    return Workspace(int(n), int(n) * per_pass, device)


def shade_hits_textured(scene: Scene, hits, rays, bindings=None, spread: float = 0.0, width0=None, out=None, ray_count=None, stream=None,
                        lights_per_pass=None, workspace=None):
    """get_shade with textures, written from the public calls alone — the executable form of the sequence in INTEGRATION.md, to be
    copied and changed.  It is shade_hits_by_light with the material taken from surface records: zero ``out``; material_hits ->
    footprint(spread, width0), if a binding holds a TRILINEAR texture with more than one level -> apply per binding, in order -> then per
    range of ``lights_per_pass`` lights: light_rays -> select_records(asks) -> cast_rays_indexed -> light_terms_surfaces -> light_fold.
    The shadow rays are light_rays': which lights ask is decided on the scene's own shading normal, and a normal map then turns the
    terms.  Without ``bindings`` the function enqueues shade_hits_by_light's calls and returns its bits.  ``workspace``: a
    textures.Workspace, or None to allocate up front."""
    bindings = _bindings(bindings)
    if workspace is not None and not isinstance(workspace, Workspace):
        raise ValueError("workspace must be a textures.Workspace (textures.workspace)")
    if not bindings:
        return shade_hits_by_light(scene, hits, rays, out, ray_count, stream, lights_per_pass, None if workspace is None else workspace.light)
    records, n = _hits_and_rays(hits, rays)
    dev = records.device
    out = _out_tensor(out, (n, 3), "float32", dev)
    _count_ptr(ray_count)
    _tensor(width0, "width0", "float32", (n,), optional=True)
    lights = scene.n_lights
    per_pass = lights if lights_per_pass is None else int(lights_per_pass)
    if lights_per_pass is not None and per_pass < 1:
        raise ValueError("lights_per_pass must be at least 1")
    per_pass = min(per_pass, lights)
    _below_2_32(n * per_pass, "(hit, light) pairs", " in one pass (lights_per_pass)")
    s = stream
    with _on_stream(stream):
        out.zero_()  # `sum` starts black (main.rs:411)
        if n == 0 or lights == 0:
            return out
        pairs = per_pass * n
        if workspace is None:
            workspace = Workspace(n, pairs, dev)
        elif workspace.light.pairs < pairs or workspace.n < n:
            raise ValueError(f"workspace must have room for {n} records and {pairs} (hit, light) pairs (textures.workspace)")
    w = workspace.light
    surfaces = workspace.surfaces[:n]
    material_hits(scene, records, surfaces, stream=s)
    cone = None
    if any(b.wants_footprint() for b in bindings):
        cone = _footprint(scene, records, rays, spread, width0, workspace.footprint[:n], stream=s)
    for b in bindings:
        apply(surfaces, records, b.diffuse, b.normal, cone, b.object_index, b.flags, stream=s)
    for first in range(0, lights, per_pass):
        c = min(per_pass, lights - first)
        m = c * n
        light_rays(scene, records, rays, first, c, w.shadow_rays[:m], w.asks[:m], stream=s)
        select_records(w.asks[:m], w.index[:m], w.count, stream=s)
        cast_rays_indexed(scene, w.shadow_rays[:m], w.index[:m], w.count, w.shadow_hits[:m], ray_count=ray_count, stream=s)
        light_terms_surfaces(scene, surfaces, records, rays, w.asks[:m], w.shadow_hits[:m], first, c, w.lit[:m], w.diffuse[:m], w.specular[:m], stream=s)
        light_fold(scene, records, w.lit[:m], w.diffuse[:m], w.specular[:m], out, stream=s)
    return out


def trace_rays_levels(scene: Scene, rays, max_depth: int, contribution=1.0, out=None, ray_count=None, stream=None, level_capacity=None,
                      check: bool = True, overflow=None, level_counts=None, open_casts: bool = False, bindings=None, spread: float = 0.0):
    """rt.trace_rays_levels — ray_trace written one level of the recursion tree at a time from the public calls — with two keywords
    more.  ``bindings``: every level's shade step is shade_hits_textured with these bindings and ``spread`` (a cone that starts at each
    level's own ray origin with width 0), on one textures.Workspace made up front; every other step is unchanged, so reflections show
    the textures too.  Without bindings the function enqueues exactly rt.trace_rays_levels' calls.  Every other argument is that
    function's."""
    bindings = _bindings(bindings)
    if not bindings:
        return _trace_rays_levels(scene, rays, max_depth, contribution, out, ray_count, stream, level_capacity, check, overflow, level_counts, open_casts,
                                  None)

    def shade_step(top, device):
        with _on_stream(stream):
            ws = workspace(scene, top, device)
        return lambda hits, level_rays, shade: shade_hits_textured(scene, hits, level_rays, bindings, spread, out=shade, ray_count=ray_count,
                                                                   stream=stream, workspace=ws)

    return _trace_rays_levels(scene, rays, max_depth, contribution, out, ray_count, stream, level_capacity, check, overflow, level_counts, open_casts,
                              None, shade_step)
