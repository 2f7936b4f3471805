"""MI355X-native render path for the homework-18 raytracer — Python host mirror.

The product is the C-ABI library ``librt_amd.so`` (hand-written HIP for gfx950,
``csrc/rt_kernels.hip``) plus ``librt_host.so`` (scene build / OBJ import /
post_process / PNG, ``csrc/host/rt_host.cpp``).  This package only mirrors the
reference's host-side names on top of them:

    World / ObjectProxy            src/main.rs:130-178, 700-728
    Camera                         src/main.rs:43-49
    render (the Whitted par_iter)  src/main.rs:1087-1104
    cast_rays (World::cast)        src/main.rs:180-326, on caller-supplied rays
    trace_rays (World::ray_trace)  src/main.rs:466-519, on caller-supplied rays
    trace_rays_distributed         src/main.rs:521-614 (distributed_ray_trace), on caller-supplied rays
    shade_hits / reflect_rays / refract_rays   src/main.rs:407-464, 328-341, 343-405 (get_shade, get_reflect, get_refract), on caller-supplied hits
    trace_rays_distributed_levels  src/main.rs:521-614 again, one level at a time from the queries and the level-loop calls
    trace_rays_levels              src/main.rs:466-519 again, one level of the tree at a time from the queries and the tree-loop calls
    light_rays / light_terms / light_fold      src/main.rs:407-464 (get_shade) opened into the calls between its shadow casts
    shade_hits_by_light            src/main.rs:407-464 again, light by light from those calls, select_records and cast_rays_indexed
    refract_enter / refract_step   src/main.rs:343-405 (get_refract) opened into the calls between its casts
    refract_rays_by_bounce         src/main.rs:343-405 again, bounce by bounce from those calls, select_records and cast_rays_indexed
    ray_keys / sort_records / gather_records / scatter_records   the order of a batch: include/rt_amd.h "record ordering"
    cast_rays_ordered / trace_rays_ordered     cast_rays and trace_rays again, on rays the device put into a coherent order first
    triangle_keys / order_triangles / World.ordered   the order of a mesh: include/rt_amd.h "mesh ordering"
    unorder_hits / order_rays      triangle indices between an ordered world and the one it was made from
    post_process / write_to_file   src/main.rs:748-776

PyTorch is used only for device memory, streams and torch.distributed.
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path
from typing import Optional, Sequence

import numpy as np

from . import _capi
from ._capi import Camera, Frame, Light, Material, RtError, SceneDesc, Sphere, Triangle, Vertex

__all__ = [
    "World", "ObjectProxy", "Scene", "Camera", "Frame", "Material", "Light", "RtError", "reference_world",
    "reference_camera", "render_whitted", "render_whitted_numpy", "make_rays", "cast_rays", "Hits", "camera_rays", "cast_rays_numpy", "trace_rays", "trace_rays_numpy", "shade_hits", "reflect_rays", "refract_rays", "Refractions", "ESCAPED", "INFINITE", "TRAPPED", "HIT_NONE", "shade_hits_numpy", "refract_rays_numpy", "scatter_hits", "scatter_factors", "Scatters", "DIFFUSE", "REFLECTION", "REFRACTION", "scatter_hits_numpy", "scatter_factors_numpy", "select_records", "cast_rays_indexed", "level_split", "level_join", "level_close", "level_fold", "level_finish", "trace_rays_distributed_levels", "tree_gate", "tree_split", "tree_spawn", "tree_gather", "tree_fold", "trace_rays_levels", "default_level_capacity", "light_rays", "light_terms", "light_fold", "shade_hits_by_light", "light_workspace", "LightWorkspace", "WALKING", "refract_enter", "refract_step", "refract_rays_by_bounce", "refract_workspace", "RefractWorkspace", "ORDER_DIRECTION_MAJOR", "ray_keys", "sort_temp_bytes", "sort_records", "gather_records", "scatter_records", "order_workspace", "OrderWorkspace", "cast_rays_ordered", "trace_rays_ordered", "triangle_keys", "order_triangles_temp_bytes", "order_triangles", "unorder_hits", "order_rays", "Rng", "focus_rays", "trace_rays_distributed", "trace_rays_distributed_numpy", "render_distributed", "render_distributed_numpy", "set_option", "options", "post_process_device", "encode_srgb8_device", "post_process", "encode_srgb8", "write_to_file",
    "DEFAULT_OBJ",
]

DEFAULT_OBJ = str(_capi.REPO_ROOT / "tests" / "golden" / "dodecahedron.obj")


def _f3(v: Sequence[float]):
    return (C.c_float * 3)(*[float(x) for x in v])


class ObjectProxy:
    """src/main.rs:700-728."""

    def __init__(self, world: "World", object_index: int):
        self.world = world
        self.object_index = object_index

    def push_triangle(self, vertices: Sequence[Vertex]) -> "ObjectProxy":
        arr = (Vertex * 3)(*vertices)
        _capi.check_host(_capi.host_lib().rt_world_push_triangle(self.world._h, self.object_index, arr))
        return self

    def push_triangles(self, triangles: Sequence[Sequence[Vertex]]) -> "ObjectProxy":
        for t in triangles:
            self.push_triangle(t)
        return self

    def push_sphere(self, center: Sequence[float], radius: float) -> "ObjectProxy":
        _capi.check_host(_capi.host_lib().rt_world_push_sphere(self.world._h, self.object_index, _f3(center), float(radius)))
        return self

    def push_flat_triangle(self, positions: Sequence[Sequence[float]], uvs: Sequence[Sequence[float]]) -> "ObjectProxy":
        """triangle(), src/main.rs:730-739."""
        p = (C.c_float * 9)(*[float(x) for v in positions for x in v])
        uv = (C.c_float * 6)(*[float(x) for v in uvs for x in v])
        _capi.check_host(_capi.host_lib().rt_world_push_flat_triangle(self.world._h, self.object_index, p, uv))
        return self

    def push_square(self, positions: Sequence[Sequence[float]], uvs: Sequence[Sequence[float]]) -> "ObjectProxy":
        """square(), src/main.rs:741-746."""
        p = (C.c_float * 12)(*[float(x) for v in positions for x in v])
        uv = (C.c_float * 8)(*[float(x) for v in uvs for x in v])
        _capi.check_host(_capi.host_lib().rt_world_push_square(self.world._h, self.object_index, p, uv))
        return self

    def load_obj(self, path: str, divisor: float = 3.0, offset: Sequence[float] = (0.7, 1.0, -0.5)) -> int:
        """load_obj, src/main.rs:778-807.  Returns the number of triangles pushed."""
        return _capi.check_host(
            _capi.host_lib().rt_world_load_obj(self.world._h, self.object_index, str(path).encode(), float(divisor), _f3(offset))
        )


class World:
    """Host-side scene under construction; src/main.rs:130-178."""

    def __init__(self):
        lib = _capi.host_lib()
        self._free = lib.rt_world_free  # bound now: module globals may be gone at interpreter shutdown
        self._h = lib.rt_world_new()
        if not self._h:
            raise MemoryError("rt_world_new failed")

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._free(h)

    def push_object(self, material: Material) -> ObjectProxy:
        idx = _capi.check_host(_capi.host_lib().rt_world_push_object(self._h, C.byref(material)))
        return ObjectProxy(self, idx)

    def push_light(self, light: Light) -> None:
        _capi.check_host(_capi.host_lib().rt_world_push_light(self._h, C.byref(light)))

    def save_scene(self, path: str, camera: Optional[Camera] = None) -> None:
        """Write the world (and optionally a camera) as a flat scene file: rt_world_save_scene, include/rt_host.h."""
        _capi.check_host(_capi.host_lib().rt_world_save_scene(self._h, C.byref(camera) if camera is not None else None, str(path).encode()))

    @classmethod
    def load_scene(cls, path: str):
        """Read a scene file: returns (World, Camera or None).  rt_world_load_scene, include/rt_host.h."""
        w = cls()
        cam, has = Camera(), C.c_int(0)
        _capi.check_host(_capi.host_lib().rt_world_load_scene(w._h, str(path).encode(), C.byref(cam), C.byref(has)))
        return w, (cam if has.value else None)

    def desc(self) -> SceneDesc:
        d = SceneDesc()
        _capi.host_lib().rt_world_desc(self._h, C.byref(d))
        d._keepalive = self  # the arrays belong to the world
        return d

    def bounds(self):
        """(lo, hi), two float32 arrays of 3: the box of the finite vertex positions and of sphere centre -+ radius (non-finite
        coordinates are left out; an empty world gives zeros).  Host numpy, no device — the box ray_keys measures origins in."""
        return _desc_bounds(self.desc())

    def ordered(self, box=None):
        """(World, perm): a new world with this one's triangles grouped by object and, inside an object, in Z-order of their centroids'
        cells in ``box`` ((lo, hi); None takes bounds()) — the order in which Scene's 16-triangle leaves are patches of the surface
        (rt_order_triangles_host: include/rt_amd.h "mesh ordering"; needs a device).  Materials, spheres and lights are unchanged.
        ``perm`` is a numpy uint32 array: perm[j] is this world's index of the new world's triangle j.  The new world is another
        scene — its casts report its own indices and break ties of equal distance by them: unorder_hits and order_rays map between
        the two."""
        d = self.desc()
        n = int(d.n_triangles)
        lo, hi = self.bounds() if box is None else box
        perm = np.zeros(n, dtype=np.uint32)
        tris = (Triangle * n)()
        _capi.check(_capi.amd_lib().rt_order_triangles_host(d.triangles, n, _box3(lo, "box lo"), _box3(hi, "box hi"), int(d.n_materials),
                                                            perm.ctypes.data_as(C.c_void_p), tris))
        w = World()
        lib = _capi.host_lib()
        for i in range(d.n_materials):
            _capi.check_host(lib.rt_world_push_object(w._h, C.byref(d.materials[i])))
        for j in range(n):
            _capi.check_host(lib.rt_world_push_triangle(w._h, tris[j].object_index, tris[j].vertices))
        for i in range(d.n_spheres):
            sph = d.spheres[i]
            _capi.check_host(lib.rt_world_push_sphere(w._h, sph.object_index, sph.center, sph.radius))
        for i in range(d.n_lights):
            _capi.check_host(lib.rt_world_push_light(w._h, C.byref(d.lights[i])))
        return w, perm


def _desc_bounds(desc: SceneDesc):
    parts = []
    if desc.n_triangles:
        words = C.sizeof(Triangle) // 4  # object_index, then 3 vertices of 8 floats: the position leads each
        tri = np.ctypeslib.as_array(C.cast(desc.triangles, C.POINTER(C.c_float)), shape=(int(desc.n_triangles), words))
        parts.append(tri[:, 1:].reshape(-1, 3, 8)[:, :, 0:3].reshape(-1, 3))
    if desc.n_spheres:
        sph = np.ctypeslib.as_array(C.cast(desc.spheres, C.POINTER(C.c_float)), shape=(int(desc.n_spheres), C.sizeof(Sphere) // 4))
        parts.append(sph[:, 1:4] - sph[:, 4:5])
        parts.append(sph[:, 1:4] + sph[:, 4:5])
    lo, hi = np.zeros(3, dtype=np.float32), np.zeros(3, dtype=np.float32)
    if parts:
        pts = np.concatenate(parts).astype(np.float32)
        for a in range(3):
            col = pts[:, a][np.isfinite(pts[:, a])]
            if col.size:
                lo[a], hi[a] = col.min(), col.max()
    return lo, hi


def reference_world(obj_path: Optional[str] = None) -> World:
    """The literal scene of main(), src/main.rs:810-1075."""
    w = World()
    _capi.check_host(_capi.host_lib().rt_world_build_reference_scene(w._h, str(obj_path or DEFAULT_OBJ).encode()))
    return w


def reference_camera() -> Camera:
    """src/main.rs:1077-1083."""
    cam = Camera()
    _capi.host_lib().rt_reference_camera(C.byref(cam))
    return cam


class Scene:
    """Device-resident scene (rt_scene_create / rt_scene_destroy).  Its counts, object indices and node tree are fixed; the
    update_* methods move triangles, spheres and lights and replace materials in place (include/rt_amd.h "scene updates")."""

    def __init__(self, world_or_desc):
        desc = world_or_desc.desc() if isinstance(world_or_desc, World) else world_or_desc
        self._desc = desc
        self.n_lights = int(desc.n_lights)
        self._h = C.c_void_p()
        _capi.check(_capi.amd_lib().rt_scene_create(C.byref(desc), C.byref(self._h)))

    @staticmethod
    def _device_records(data, record_bytes, name, stream):
        """``data`` as device memory holding whole records of record_bytes: a contiguous CUDA tensor as it is, a numpy array or
        ctypes array uploaded first (on ``stream``, default torch's current one).  Returns (tensor, record count, stream)."""
        import torch

        host = None
        if torch.is_tensor(data):
            if not (data.is_cuda and data.is_contiguous()):
                raise ValueError(f"{name} must be a contiguous CUDA tensor or a numpy array")
            nbytes = data.numel() * data.element_size()
        else:
            host = np.ascontiguousarray(data) if isinstance(data, np.ndarray) else np.frombuffer(data, dtype=np.uint8)
            nbytes = host.nbytes
        if nbytes % record_bytes != 0:
            raise ValueError(f"{name} must hold whole records of {record_bytes} bytes")
        s = stream if stream is not None else torch.cuda.current_stream()
        if host is not None:
            with torch.cuda.stream(s):
                data = torch.from_numpy(host.reshape(-1).view(np.uint8).copy()).to("cuda")
            data.record_stream(s)
        return data, nbytes // record_bytes, s

    def update_vertices(self, first: int, vertices, stream=None) -> None:
        """rt_scene_update_vertices: triangles first .. first + count - 1 get the 3 * count rt_vertex records (8 floats each: position,
        normal, uv) of ``vertices`` — a CUDA tensor, or a numpy / ctypes array of Vertex records that is uploaded first — and the node
        tree is refitted.  Stream-ordered on ``stream`` (default: torch's current stream)."""
        t, n, s = self._device_records(vertices, 3 * C.sizeof(Vertex), "vertices", stream)
        _capi.check(_capi.amd_lib().rt_scene_update_vertices(self._h, int(first), n, C.c_void_p(t.data_ptr()), C.c_void_p(s.cuda_stream)))

    def update_spheres(self, first: int, spheres, stream=None) -> None:
        """rt_scene_update_spheres: spheres first .. get the rt_sphere records (object_index — ignored —, centre, radius: 5 words each)
        of ``spheres``, a CUDA tensor or a numpy / ctypes array of Sphere records."""
        t, n, s = self._device_records(spheres, C.sizeof(Sphere), "spheres", stream)
        _capi.check(_capi.amd_lib().rt_scene_update_spheres(self._h, int(first), n, C.c_void_p(t.data_ptr()), C.c_void_p(s.cuda_stream)))

    def _update_host_records(self, fn, first, records, ctype, stream):
        import torch

        arr = records if isinstance(records, C.Array) and records._type_ is ctype else (ctype * len(records))(*records)
        _capi.check(fn(self._h, int(first), len(arr), arr, _stream_ptr(stream)))

    def update_lights(self, first: int, lights, stream=None) -> None:
        """rt_scene_update_lights: lights first .. are replaced by the Light records of ``lights`` (read at the call)."""
        self._update_host_records(_capi.amd_lib().rt_scene_update_lights, first, lights, Light, stream)

    def update_materials(self, first: int, materials, stream=None) -> None:
        """rt_scene_update_materials: materials (objects) first .. are replaced by the Material records of ``materials``."""
        self._update_host_records(_capi.amd_lib().rt_scene_update_materials, first, materials, Material, stream)

    def close(self) -> None:
        h, self._h = getattr(self, "_h", None), None
        if h:
            _capi.amd_lib().rt_scene_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _stream_ptr(stream):
    """``stream`` (default: torch's current stream) as the void pointer the C entry points take"""
    import torch

    s = stream if stream is not None else torch.cuda.current_stream()
    return C.c_void_p(s.cuda_stream)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _out_tensor(out, shape, dtype, device, name="out"):
    """``out`` if the caller gave one — it must be a contiguous CUDA tensor of this shape and dtype — or a new one on ``device``"""
    import torch

    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if not (torch.is_tensor(out) and out.is_cuda and out.dtype == dtype and out.is_contiguous() and tuple(out.shape) == tuple(shape)):
        raise ValueError(f"{name} must be a contiguous {tuple(shape)} {dtype} CUDA tensor")
    return out


def render_whitted(scene: Scene, camera: Camera, frame: Frame, out=None, ray_count=None, stream=None):
    """Whitted pass over one tile into device memory (src/main.rs:1090-1104).

    ``out``: torch float32 CUDA tensor of shape (rows, cols, 3) (allocated if None).
    ``ray_count``: torch int64 CUDA tensor with one element that the cast count is added to.
    Stream-ordered on ``stream`` (default: torch's current stream); returns ``out``.
    """
    import torch

    rows, cols = frame.rows, frame.cols
    if out is None:
        out = torch.empty((rows, cols, 3), dtype=torch.float32, device="cuda")
    if not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == rows * cols * 3):
        raise ValueError("out must be a contiguous float32 CUDA tensor with rows*cols*3 elements")
    cnt_ptr = _count_ptr(ray_count)
    _capi.check(
        _capi.amd_lib().rt_render_whitted(
            scene._h, C.byref(camera), C.byref(frame), C.c_void_p(out.data_ptr()), cnt_ptr, _stream_ptr(stream)
        )
    )
    return out


def render_whitted_numpy(scene: Scene, camera: Camera, frame: Frame):
    """Host-buffer convenience (rt_render_whitted_host): returns (rgb[rows, cols, 3] float32, casts)."""
    rows, cols = frame.rows, frame.cols
    img = np.empty((rows, cols, 3), dtype=np.float32)
    casts = C.c_ulonglong(0)
    _capi.check(
        _capi.amd_lib().rt_render_whitted_host(scene._h, C.byref(camera), C.byref(frame), img.ctypes.data_as(C.c_void_p), C.byref(casts))
    )
    return img, int(casts.value)


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
    import torch

    for name, t in (("origins", origins), ("directions", directions)):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.shape[1] == 3):
            raise ValueError(f"{name} must be an (N, 3) float32 CUDA tensor")
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


def _records(t, words, name):
    import torch

    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and t.dim() == 2 and t.shape[1] == words):
        raise ValueError(f"{name} must be a contiguous (N, {words}) int32 CUDA tensor")


def cast_rays(scene: Scene, rays, out=None, stream=None):
    """World::cast (src/main.rs:180-326) for every ray of an (N, 11) int32 CUDA tensor of rt_ray records (make_rays, camera_rays):
    returns ``out``, an (N, 13) int32 CUDA tensor of rt_hit records (allocated if None; Hits names its fields), bit-identical to the
    reference's cast.  Stream-ordered on ``stream`` (default: torch's current stream)."""
    import torch

    _records(rays, 11, "rays")
    n = rays.shape[0]
    out = _out_tensor(out, (n, 13), torch.int32, rays.device)
    _capi.check(_capi.amd_lib().rt_cast_rays(scene._h, C.c_void_p(rays.data_ptr()), n, C.c_void_p(out.data_ptr()), _stream_ptr(stream)))
    return out


class Hits:
    """Named views of an (N, 13) int32 tensor of rt_hit records (what cast_rays returns), on the same storage."""

    def __init__(self, records):
        import torch

        if not (torch.is_tensor(records) and records.dtype == torch.int32 and records.dim() == 2 and records.shape[1] == 13):
            raise ValueError("expected an (N, 13) int32 tensor of rt_hit records")
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
    import torch

    n = frame.rows * frame.cols
    out = _out_tensor(out, (n, 11), torch.int32, "cuda")
    _capi.check(_capi.amd_lib().rt_camera_rays(C.byref(camera), C.byref(frame), C.c_void_p(out.data_ptr()), _stream_ptr(stream)))
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
    import torch

    _records(rays, 11, "rays")
    n = rays.shape[0]
    out = _out_tensor(out, (n, 3), torch.float32, rays.device)
    cnt_ptr = _count_ptr(ray_count)
    _capi.check(_capi.amd_lib().rt_trace_rays(scene._h, C.c_void_p(rays.data_ptr()), n, int(max_depth), float(contribution),
                                              C.c_void_p(out.data_ptr()), cnt_ptr, _stream_ptr(stream)))
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


def _hit_records(hits):
    records = hits.records if isinstance(hits, Hits) else hits
    _records(records, 13, "hits")
    return records


def _hits_and_rays(hits, rays):
    records = _hit_records(hits)
    _records(rays, 11, "rays")
    if rays.shape[0] != records.shape[0]:
        raise ValueError("hits and rays must have one record each per hit: rays[i] is the ray that produced hits[i]")
    return records, records.shape[0]


def _column(t, dtype, n, name):
    import torch

    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == dtype and t.is_contiguous() and tuple(t.shape) == (n,)):
        raise ValueError(f"{name} must be a contiguous ({n},) {dtype} CUDA tensor")


def _rgb(t, n, name):
    import torch

    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (n, 3)):
        raise ValueError(f"{name} must be a contiguous ({n}, 3) float32 CUDA tensor")


def _count_ptr(ray_count):
    if ray_count is None:
        return None
    import torch

    if not (torch.is_tensor(ray_count) and ray_count.is_cuda and ray_count.dtype == torch.int64 and ray_count.numel() == 1):
        raise ValueError("ray_count must be a 1-element int64 CUDA tensor")
    return C.c_void_p(ray_count.data_ptr())


def shade_hits(scene: Scene, hits, rays, out=None, ray_count=None, stream=None):
    """get_shade (src/main.rs:407-464) for every hit: ``hits`` is a Hits or its (N, 13) int32 CUDA record tensor (what cast_rays
    returns), ``rays`` the (N, 11) rt_ray records that produced them (Hit.ray).  Returns ``out``, an (N, 3) float32 CUDA tensor
    (allocated if None) with get_shade's value bit for bit; a record that is no hit gives black.  ``ray_count``: a 1-element int64 CUDA
    tensor that the shadow casts are added to.  Stream-ordered on ``stream`` (default: torch's current stream)."""
    import torch

    records, n = _hits_and_rays(hits, rays)
    out = _out_tensor(out, (n, 3), torch.float32, records.device)
    _capi.check(_capi.amd_lib().rt_shade_hits(scene._h, C.c_void_p(records.data_ptr()), C.c_void_p(rays.data_ptr()), n,
                                              C.c_void_p(out.data_ptr()), _count_ptr(ray_count), _stream_ptr(stream)))
    return out


def reflect_rays(hits, rays, out=None, stream=None):
    """get_reflect (src/main.rs:328-341) for every hit: returns ``out``, an (N, 11) int32 CUDA tensor of rt_ray records (allocated if
    None) that cast_rays / trace_rays take as they are; a record that is no hit gives an all-zero ray.  Needs no scene."""
    import torch

    records, n = _hits_and_rays(hits, rays)
    out = _out_tensor(out, (n, 11), torch.int32, records.device)
    _capi.check(_capi.amd_lib().rt_reflect_rays(C.c_void_p(records.data_ptr()), C.c_void_p(rays.data_ptr()), n, C.c_void_p(out.data_ptr()),
                                                _stream_ptr(stream)))
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
    import torch

    records, n = _hits_and_rays(hits, rays)
    if out is None:
        out = Refractions(torch.empty((n,), dtype=torch.int32, device=records.device), torch.empty((n,), dtype=torch.float32, device=records.device),
                          torch.empty((n, 11), dtype=torch.int32, device=records.device))
    kind, travel, escape = out.kind, out.travel, out.rays
    _column(kind, torch.int32, n, "out.kind")
    _column(travel, torch.float32, n, "out.travel")
    _records(escape, 11, "out.rays")
    if escape.shape[0] != n:
        raise ValueError("out must have one record per hit")
    _capi.check(_capi.amd_lib().rt_refract_rays(scene._h, C.c_void_p(records.data_ptr()), C.c_void_p(rays.data_ptr()), n, float(max_distance),
                                                C.c_void_p(kind.data_ptr()), C.c_void_p(travel.data_ptr()), C.c_void_p(escape.data_ptr()),
                                                _count_ptr(ray_count), _stream_ptr(stream)))
    return out


def _host_records(a, dtype, words, name):
    a = np.asarray(a)
    if a.dtype == dtype:
        return np.ascontiguousarray(a).reshape(-1)
    if a.ndim == 2 and a.shape[1] == words and a.dtype.itemsize == 4:
        return np.ascontiguousarray(a).view(dtype).reshape(-1)
    raise ValueError(f"{name}: expected a {'HIT' if words == 13 else 'RAY'}_DTYPE array or an (N, {words}) array of 4-byte words")


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


class Rng:
    """Device-resident per-pixel IsaacRng states of one tile (src/main.rs:1117-1127); rt_rng_create/destroy."""

    def __init__(self, frame: Frame):
        self.frame = frame
        self.count = frame.rows * frame.cols
        self._h = C.c_void_p()
        _capi.check(_capi.amd_lib().rt_rng_create(C.byref(frame), C.byref(self._h)))

    @classmethod
    def seeded(cls, seeds) -> "Rng":
        """Generators that belong to no frame (rt_rng_create_seeded): generator i is IsaacRng::new_from_u64(seeds[i]); ``seeds`` is a
        sequence or array of integers below 2^64.  Rng(frame) is the case seeds[p] = y * 2^33 + x in the tile's row order."""
        a = np.ascontiguousarray(np.asarray(seeds, dtype=np.uint64).reshape(-1))
        self = cls.__new__(cls)
        self.frame = None
        self.count = int(a.shape[0])
        self._h = C.c_void_p()
        _capi.check(_capi.amd_lib().rt_rng_create_seeded(a.ctypes.data_as(C.c_void_p), self.count, C.byref(self._h)))
        return self

    def download(self) -> np.ndarray:
        words = _capi.amd_lib().rt_rng_state_words()
        st = np.empty((self.count, words), dtype=np.uint32)
        _capi.check(_capi.amd_lib().rt_rng_download(self._h, st.ctypes.data_as(C.c_void_p)))
        return st

    def upload(self, states) -> None:
        """The inverse of download (rt_rng_upload): (count, rt_rng_state_words) uint32 records in the reference's layout; the next call
        continues exactly from them.  Synchronises."""
        words = _capi.amd_lib().rt_rng_state_words()
        a = np.asarray(states)
        if not (a.dtype == np.uint32 and a.shape == (self.count, words)):
            raise ValueError(f"expected a ({self.count}, {words}) uint32 array")
        a = np.ascontiguousarray(a)
        _capi.check(_capi.amd_lib().rt_rng_upload(self._h, a.ctypes.data_as(C.c_void_p)))

    def close(self) -> None:
        h, self._h = getattr(self, "_h", None), None
        if h:
            _capi.amd_lib().rt_rng_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def render_distributed(scene: Scene, camera: Camera, frame: Frame, rng: Rng, n_epochs: int = 1, focus: float = 3.0,
                       blur: float = 0.04, accum=None, samples=None, valid=None, ray_count=None, stream=None):
    """`n_epochs` passes of the distributed/DoF closure (src/main.rs:1131-1161) over one tile, on the device.

    accum   (rows, cols, 3) f32 CUDA tensor or None: surviving samples are added in epoch order.
    samples (n_epochs, rows, cols, 3) f32 / valid (n_epochs, rows, cols) u8 CUDA tensors or None: raw samples + filter.
    """
    import torch

    def ptr(t):
        return None if t is None else C.c_void_p(t.data_ptr())

    rows, cols = frame.rows, frame.cols
    for t, shape, dt in ((accum, (rows, cols, 3), torch.float32), (samples, (n_epochs, rows, cols, 3), torch.float32),
                         (valid, (n_epochs, rows, cols), torch.uint8)):
        if t is not None and not (t.is_cuda and t.dtype == dt and t.is_contiguous() and tuple(t.shape) == shape):
            raise ValueError(f"expected a contiguous CUDA {dt} tensor of shape {shape}")
    _capi.check(
        _capi.amd_lib().rt_render_distributed(scene._h, C.byref(camera), C.byref(frame), float(focus), float(blur), rng._h,
                                              int(n_epochs), ptr(accum), ptr(samples), ptr(valid), ptr(ray_count), _stream_ptr(stream))
    )
    return accum if accum is not None else samples


def focus_rays(camera: Camera, frame: Frame, rng: Rng, focus: float = 3.0, blur: float = 0.04, out=None, stream=None):
    """Camera::shoot_focus (src/main.rs:101-127) of every pixel of a frame or tile as an (rows * cols, 11) int32 CUDA tensor of rt_ray
    records in compact row order (rt_focus_rays): the two lens draws come from the pixel's generator in ``rng`` (the frame's Rng, or a
    seeded one of as many generators), which advances — bit for bit the ray render_distributed casts first in that epoch."""
    import torch

    n = frame.rows * frame.cols
    out = _out_tensor(out, (n, 11), torch.int32, "cuda")
    _capi.check(_capi.amd_lib().rt_focus_rays(C.byref(camera), C.byref(frame), float(focus), float(blur), rng._h, C.c_void_p(out.data_ptr()),
                                              _stream_ptr(stream)))
    return out


def trace_rays_distributed(scene: Scene, rays, max_depth: int, rng: Rng, n_epochs: int = 1, accum=None, samples=None, valid=None,
                           ray_count=None, stream=None):
    """`n_epochs` samples of distributed_ray_trace (src/main.rs:521-614) per ray of an (N, 11) int32 CUDA tensor of rt_ray records, ray i
    on generator i of ``rng`` (N generators: Rng.seeded, or a frame's Rng of N pixels), whose stream continues (rt_trace_rays_distributed).

    accum   (N, 3) f32 CUDA tensor or None: the samples that pass the filter of main.rs:1157-1160 are added in epoch order.
    samples (n_epochs, N, 3) f32 / valid (n_epochs, N) u8 CUDA tensors or None: raw samples + filter flags.
    ray_count: a 1-element int64 CUDA tensor that the World::cast count is added to.  At least one of accum / samples.
    """
    import torch

    def ptr(t):
        return None if t is None else C.c_void_p(t.data_ptr())

    _records(rays, 11, "rays")
    n = rays.shape[0]
    for t, shape, dt in ((accum, (n, 3), torch.float32), (samples, (n_epochs, n, 3), torch.float32), (valid, (n_epochs, n), torch.uint8)):
        if t is not None and not (torch.is_tensor(t) and t.is_cuda and t.dtype == dt and t.is_contiguous() and tuple(t.shape) == shape):
            raise ValueError(f"expected a contiguous CUDA {dt} tensor of shape {shape}")
    if ray_count is not None and not (ray_count.is_cuda and ray_count.dtype == torch.int64 and ray_count.numel() == 1):
        raise ValueError("ray_count must be a 1-element int64 CUDA tensor")
    _capi.check(_capi.amd_lib().rt_trace_rays_distributed(scene._h, C.c_void_p(rays.data_ptr()), n, int(max_depth), rng._h, int(n_epochs),
                                                          ptr(accum), ptr(samples), ptr(valid), ptr(ray_count), _stream_ptr(stream)))
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
    import torch

    records, n = _hits_and_rays(hits, rays)
    _rng_of(rng)
    idx_ptr = None
    if rng_index is not None:
        if not (torch.is_tensor(rng_index) and rng_index.is_cuda and rng_index.dtype == torch.int32 and rng_index.is_contiguous()
                and tuple(rng_index.shape) == (n,)):
            raise ValueError("rng_index must be a contiguous (N,) int32 CUDA tensor")
        idx_ptr = C.c_void_p(rng_index.data_ptr())
    elif n != rng.count:
        raise ValueError("without rng_index the Rng must hold one generator per record")
    if out is None:
        out = Scatters(torch.empty((n,), dtype=torch.int32, device=records.device), torch.empty((n, 11), dtype=torch.int32, device=records.device),
                       torch.empty((n,), dtype=torch.float32, device=records.device))
    _column(out.type, torch.int32, n, "out.type")
    _records(out.rays, 11, "out.rays")
    if out.rays.shape[0] != n:
        raise ValueError("out must have one record per hit")
    _column(out.cosine, torch.float32, n, "out.cosine")
    _capi.check(_capi.amd_lib().rt_scatter_hits(scene._h, C.c_void_p(records.data_ptr()), C.c_void_p(rays.data_ptr()), n, rng._h, idx_ptr,
                                                C.c_void_p(out.type.data_ptr()), C.c_void_p(out.rays.data_ptr()), C.c_void_p(out.cosine.data_ptr()),
                                                _stream_ptr(stream)))
    return out


def scatter_factors(scene: Scene, hits, rays, types, next_rays, travel, out=None, stream=None):
    """The factor of one level once its next ray is known (src/main.rs:566-570, 585-589, 605): get_diffuse (DIFFUSE) or get_specular
    (REFLECTION) of the hit's material towards ``next_rays[i]``'s direction seen from ``-rays[i]``'s, or opaque_decay ** travel[i] in all
    three channels (REFRACTION); any other type or a record that is no hit gives 0.  ``types``: (N,) int32, ``next_rays``: (N, 11)
    int32 rt_ray records, ``travel``: (N,) float32, all CUDA.  Returns ``out``, an (N, 3) float32 CUDA tensor (allocated if None)."""
    import torch

    records, n = _hits_and_rays(hits, rays)
    if not (torch.is_tensor(types) and types.is_cuda and types.dtype == torch.int32 and types.is_contiguous() and tuple(types.shape) == (n,)):
        raise ValueError("types must be a contiguous (N,) int32 CUDA tensor")
    _records(next_rays, 11, "next_rays")
    if next_rays.shape[0] != n:
        raise ValueError("next_rays must have one record per hit")
    if not (torch.is_tensor(travel) and travel.is_cuda and travel.dtype == torch.float32 and travel.is_contiguous()
            and tuple(travel.shape) == (n,)):
        raise ValueError("travel must be a contiguous (N,) float32 CUDA tensor")
    out = _out_tensor(out, (n, 3), torch.float32, records.device)
    _capi.check(_capi.amd_lib().rt_scatter_factors(scene._h, C.c_void_p(records.data_ptr()), C.c_void_p(rays.data_ptr()),
                                                   C.c_void_p(types.data_ptr()), C.c_void_p(next_rays.data_ptr()), C.c_void_p(travel.data_ptr()),
                                                   n, C.c_void_p(out.data_ptr()), _stream_ptr(stream)))
    return out


def _host_column(a, dtype, n, name):
    a = np.asarray(a)
    if not (a.dtype.kind in dtype[0] and a.dtype.itemsize == 4 and a.shape == (n,)):
        raise ValueError(f"{name}: expected an ({n},) array of {dtype[1]}")
    return np.ascontiguousarray(a)


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


# ---- level loop: select, indexed casts, the glue of one level and the fold (include/rt_amd.h rt_select_records ... rt_level_finish) ----


def select_records(flags, index=None, count=None, stream=None):
    """Stable selection on the device (rt_select_records): ``flags`` is an (N,) uint8 CUDA tensor; returns (index, count) — ``index``
    an (N,) int32 CUDA tensor whose first ``count[0]`` entries are the ascending i with flags[i] != 0 (the rest unspecified), ``count``
    a 1-element int32 CUDA tensor that stays on the device.  The first call on a stream allocates 4 KB of scratch and must not be
    captured into a graph.  N == 0 leaves ``count`` as it was."""
    import torch

    if not (torch.is_tensor(flags) and flags.is_cuda and flags.dtype == torch.uint8 and flags.is_contiguous() and flags.dim() == 1):
        raise ValueError("flags must be a contiguous (N,) uint8 CUDA tensor")
    n = flags.shape[0]
    if index is None:
        index = torch.empty((n,), dtype=torch.int32, device=flags.device)
    if count is None:
        count = torch.empty((1,), dtype=torch.int32, device=flags.device)
    _column(index, torch.int32, n, "index")
    _column(count, torch.int32, 1, "count")
    _capi.check(_capi.amd_lib().rt_select_records(_p(flags), n, _p(index), _p(count), _stream_ptr(stream)))
    return index, count


def cast_rays_indexed(scene: Scene, rays, index, count, out, max_count=None, ray_count=None, stream=None):
    """World::cast of the rays an index list names (rt_cast_rays_indexed): for j < min(count[0], max_count), out[index[j]] =
    cast(rays[index[j]]), bit for bit cast_rays' record; records of ``out`` ((N, 13) int32, required) that are not named are not
    written, an index >= N is skipped.  ``index``: an (M,) int32 CUDA tensor, ``count``: a 1-element int32 CUDA tensor (what
    select_records returns), ``max_count``: the host's bound on the list's length (default M).  ``ray_count``: a 1-element int64 CUDA
    tensor that the casts made are added to."""
    import torch

    _records(rays, 11, "rays")
    n = rays.shape[0]
    _records(out, 13, "out")
    if out.shape[0] != n:
        raise ValueError("out must have one record per ray")
    if not (torch.is_tensor(index) and index.is_cuda and index.dtype == torch.int32 and index.is_contiguous() and index.dim() == 1):
        raise ValueError("index must be a contiguous (M,) int32 CUDA tensor")
    _column(count, torch.int32, 1, "count")
    m = index.shape[0] if max_count is None else int(max_count)
    if not 0 <= m <= index.shape[0]:
        raise ValueError("max_count must not exceed the length of index")
    _capi.check(_capi.amd_lib().rt_cast_rays_indexed(scene._h, _p(rays), n, _p(index), _p(count), m, _p(out), _count_ptr(ray_count),
                                                     _stream_ptr(stream)))
    return out


def level_split(hits, types, cosine, out_reflect=None, out_refract=None, stream=None):
    """After scatter_hits (rt_level_split): returns (hits_reflect, hits_refract), (N, 13) int32 rt_hit records — hits[i] where the level
    goes on as a diffuse or reflection scatter, respectively as a refraction, "no hit" elsewhere: the operands of reflect_rays and
    refract_rays.  ``types``, ``cosine``: Scatters.type and Scatters.cosine."""
    import torch

    records = _hit_records(hits)
    n = records.shape[0]
    _column(types, torch.int32, n, "types")
    _column(cosine, torch.float32, n, "cosine")
    if out_reflect is None:
        out_reflect = torch.empty((n, 13), dtype=torch.int32, device=records.device)
    if out_refract is None:
        out_refract = torch.empty((n, 13), dtype=torch.int32, device=records.device)
    for t in (out_reflect, out_refract):
        _records(t, 13, "out")
        if t.shape[0] != n:
            raise ValueError("out must have one record per hit")
    _capi.check(_capi.amd_lib().rt_level_split(_p(records), _p(types), _p(cosine), n, _p(out_reflect), _p(out_refract), _stream_ptr(stream)))
    return out_reflect, out_refract


def level_join(types, cosine, reflected, refr_kind, escape, out_rays=None, out_hits=None, out_flags=None, stream=None):
    """After reflect_rays / refract_rays (rt_level_join): returns (next_rays, next_hits, flags) — the ray each record casts next (the
    reflected one, or the escape ray of an Escaped refraction; zero words where there is none), the next hits preset to "no hit", and
    an (N,) uint8 flag where a ray exists: select_records(flags) + cast_rays_indexed(next_rays -> next_hits) follow."""
    import torch

    _records(reflected, 11, "reflected")
    n = reflected.shape[0]
    _records(escape, 11, "escape")
    if escape.shape[0] != n:
        raise ValueError("reflected and escape must have one record each per record")
    _column(types, torch.int32, n, "types")
    _column(cosine, torch.float32, n, "cosine")
    _column(refr_kind, torch.int32, n, "refr_kind")
    if out_rays is None:
        out_rays = torch.empty((n, 11), dtype=torch.int32, device=reflected.device)
    if out_hits is None:
        out_hits = torch.empty((n, 13), dtype=torch.int32, device=reflected.device)
    if out_flags is None:
        out_flags = torch.empty((n,), dtype=torch.uint8, device=reflected.device)
    _records(out_rays, 11, "out_rays")
    _records(out_hits, 13, "out_hits")
    if out_rays.shape[0] != n or out_hits.shape[0] != n:
        raise ValueError("outputs must have one record per record")
    _column(out_flags, torch.uint8, n, "out_flags")
    _capi.check(_capi.amd_lib().rt_level_join(_p(types), _p(cosine), _p(reflected), _p(refr_kind), _p(escape), n, _p(out_rays), _p(out_hits),
                                              _p(out_flags), _stream_ptr(stream)))
    return out_rays, out_hits, out_flags


def level_close(hits, types, cosine, next_hits, out=None, stream=None):
    """After the indexed cast (rt_level_close): returns (N, 13) int32 rt_hit records — hits[i] where a diffuse or reflection scatter
    went on and its next cast missed, "no hit" elsewhere: the operand of get_shade(&scattered_hit), shade_hits(out, Scatters.rays)."""
    import torch

    records = _hit_records(hits)
    n = records.shape[0]
    nxt = _hit_records(next_hits)
    if nxt.shape[0] != n:
        raise ValueError("next_hits must have one record per hit")
    _column(types, torch.int32, n, "types")
    _column(cosine, torch.float32, n, "cosine")
    out = _out_tensor(out, (n, 13), torch.int32, records.device)
    _capi.check(_capi.amd_lib().rt_level_close(_p(records), _p(types), _p(cosine), _p(nxt), n, _p(out), _stream_ptr(stream)))
    return out


def level_fold(types, cosine, next_hits, factor, shade_next, shade_missed, value, stream=None):
    """One step of the unwind (rt_level_fold), from the deepest level back: ``value`` ((N, 3) float32, in place) holds the value of the
    level below and receives this level's — the mix of main.rs:571 / 590, the sum of main.rs:605, shade_missed or black, in
    trace_rays_distributed's operation order."""
    import torch

    nxt = _hit_records(next_hits)
    n = nxt.shape[0]
    _column(types, torch.int32, n, "types")
    _column(cosine, torch.float32, n, "cosine")
    for t, name in ((factor, "factor"), (shade_next, "shade_next"), (shade_missed, "shade_missed"), (value, "value")):
        _rgb(t, n, name)
    _capi.check(_capi.amd_lib().rt_level_fold(_p(types), _p(cosine), _p(nxt), _p(factor), _p(shade_next), _p(shade_missed), n, _p(value),
                                              _stream_ptr(stream)))
    return value


def level_finish(value, accum=None, valid=None, stream=None):
    """The sample filter and the accumulation (rt_level_finish, main.rs:1157-1165): valid[i] = all three channels of value[i] are
    is_normal ((N,) uint8 or None); accum[i] += value[i] where valid ((N, 3) float32 or None).  At least one of the two."""
    import torch

    if not (torch.is_tensor(value) and value.dim() == 2):
        raise ValueError("value must be a contiguous (N, 3) float32 CUDA tensor")
    n = value.shape[0]
    _rgb(value, n, "value")
    if accum is not None:
        _rgb(accum, n, "accum")
    if valid is not None:
        _column(valid, torch.uint8, n, "valid")
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
    import torch

    _records(rays, 11, "rays")
    n = rays.shape[0]
    n_epochs = int(n_epochs)
    for t, shape, dt in ((accum, (n, 3), torch.float32), (samples, (n_epochs, n, 3), torch.float32), (valid, (n_epochs, n), torch.uint8)):
        if t is not None and not (torch.is_tensor(t) and t.is_cuda and t.dtype == dt and t.is_contiguous() and tuple(t.shape) == shape):
            raise ValueError(f"expected a contiguous CUDA {dt} tensor of shape {shape}")
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

    def new(shape, dtype):
        return torch.empty(shape, dtype=dtype, device=dev)

    # allocated (and the one fill enqueued) with `stream` as torch's current stream: the caching allocator then ties the blocks to it
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        i32, f32, u8 = torch.int32, torch.float32, torch.uint8
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
        lws = light_workspace(scene, n, dev) if open_casts else None
        rws = refract_workspace(n, dev) if open_casts and depth > 0 else None
    select_records(flags, identity, n_all, stream=s)  # 0 .. n-1 and n: the primary casts as an indexed cast, which counts

    def shade(level_hits, level_rays, out):  # get_shade, in one kernel or light by light
        if open_casts:
            return shade_hits_by_light(scene, level_hits, level_rays, out=out, ray_count=ray_count, stream=s, workspace=lws)
        return shade_hits(scene, level_hits, level_rays, out=out, ray_count=ray_count, stream=s)

    def refract(level_hits, level_rays, out):  # get_refract(100.0), in one kernel or bounce by bounce
        if open_casts:
            return refract_rays_by_bounce(scene, level_hits, level_rays, 100.0, ray_count=ray_count, stream=s, out=out, workspace=rws)
        return refract_rays(scene, level_hits, level_rays, 100.0, ray_count=ray_count, stream=s, out=out)

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


def _count_word(t, name):
    import torch

    if t is not None:
        _column(t, torch.int32, 1, name)


def _floats(t, shape, name):
    import torch

    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == tuple(shape)):
        raise ValueError(f"{name} must be a contiguous {tuple(shape)} float32 CUDA tensor")


def tree_gate(contribution, count=None, out_flags=None, out_hits=None, stream=None):
    """The entry check of ray_trace on the roots (rt_tree_gate, main.rs:469): returns (flags, hits) — ``flags`` (N,) uint8, 1 where
    j < count and not contribution[j] < 0.001 (NaN passes), ``hits`` (N, 13) int32 preset to "no hit": select_records(flags) +
    cast_rays_indexed(rays -> hits) follow.  ``count``: a 1-element int32 CUDA tensor, or None for N."""
    import torch

    if not (torch.is_tensor(contribution) and contribution.dim() == 1):
        raise ValueError("contribution must be a contiguous (N,) float32 CUDA tensor")
    n = contribution.shape[0]
    _floats(contribution, (n,), "contribution")
    _count_word(count, "count")
    if out_flags is None:
        out_flags = torch.empty((n,), dtype=torch.uint8, device=contribution.device)
    if out_hits is None:
        out_hits = torch.empty((n, 13), dtype=torch.int32, device=contribution.device)
    _column(out_flags, torch.uint8, n, "out_flags")
    _records(out_hits, 13, "out_hits")
    if out_hits.shape[0] != n:
        raise ValueError("out_hits must have one record per root")
    _capi.check(_capi.amd_lib().rt_tree_gate(_p(contribution), n, _p(count), _p(out_flags), _p(out_hits), _stream_ptr(stream)))
    return out_flags, out_hits


def tree_split(scene: Scene, hits, contribution, depth_left: int, count=None, out_shade=None, out_reflect=None, out_refract=None,
               out_weights=None, stream=None):
    """The weights and threshold gates of main.rs:478-504 (rt_tree_split): returns (hits_shade, hits_reflect, hits_refract, weights) —
    the level's hits where get_shade, get_reflect and get_refract are wanted ("no hit" elsewhere), the operands of shade_hits,
    reflect_rays and refract_rays with the level's rays; ``weights`` (N, 4) float32 = (sc, rc, fc, opaque_decay), zeros where the record
    is not live.  ``depth_left``: TraceState.depth of the level."""
    import torch

    records = _hit_records(hits)
    n = records.shape[0]
    _floats(contribution, (n,), "contribution")
    _count_word(count, "count")
    outs = []
    for t in (out_shade, out_reflect, out_refract):
        if t is None:
            t = torch.empty((n, 13), dtype=torch.int32, device=records.device)
        _records(t, 13, "out")
        if t.shape[0] != n:
            raise ValueError("out must have one record per hit")
        outs.append(t)
    if out_weights is None:
        out_weights = torch.empty((n, 4), dtype=torch.float32, device=records.device)
    _floats(out_weights, (n, 4), "out_weights")
    _capi.check(_capi.amd_lib().rt_tree_split(scene._h, _p(records), _p(contribution), n, _p(count), int(depth_left), _p(outs[0]), _p(outs[1]),
                                              _p(outs[2]), _p(out_weights), _stream_ptr(stream)))
    return outs[0], outs[1], outs[2], out_weights


def tree_spawn(hits_reflect, refr_kind, out_flags=None, out_child_values=None, stream=None):
    """The child candidates of a level (rt_tree_spawn): returns (flags, child_values) — ``flags`` (2N,) uint8, entry 2j the reflection
    child of record j (hits_reflect[j] is a hit), entry 2j + 1 its refraction child (refr_kind[j] == ESCAPED); ``child_values``
    (2N, 3) float32, zeroed, which the children's tree_fold overwrites.  select_records(flags) + tree_gather follow."""
    import torch

    records = _hit_records(hits_reflect)
    n = records.shape[0]
    _column(refr_kind, torch.int32, n, "refr_kind")
    if out_flags is None:
        out_flags = torch.empty((2 * n,), dtype=torch.uint8, device=records.device)
    if out_child_values is None:
        out_child_values = torch.empty((2 * n, 3), dtype=torch.float32, device=records.device)
    _column(out_flags, torch.uint8, 2 * n, "out_flags")
    _floats(out_child_values, (2 * n, 3), "out_child_values")
    _capi.check(_capi.amd_lib().rt_tree_spawn(_p(records), _p(refr_kind), n, _p(out_flags), _p(out_child_values), _stream_ptr(stream)))
    return out_flags, out_child_values


def tree_gather(index, count, reflected, escape, contribution, weights, overflow, max_count=None, out_rays=None, out_contribution=None,
                out_parent=None, out_count=None, stream=None):
    """The next level from the selected candidates (rt_tree_gather): returns (rays, contribution, parent, count) of the children —
    child j comes from candidate c = index[j]: the reflected ray of record c >> 1 when c is even, its escape ray when odd; its
    contribution is the parent's times rc or fc, its parent slot c.  ``max_count``: the capacity of the child arrays (default: that of
    ``out_rays``, or 2N); candidates beyond it are dropped and their number is ADDED to ``overflow`` (a 1-element int32 CUDA tensor)."""
    import torch

    _records(reflected, 11, "reflected")
    n = reflected.shape[0]
    _records(escape, 11, "escape")
    if escape.shape[0] != n:
        raise ValueError("reflected and escape must have one record each per record")
    _floats(contribution, (n,), "contribution")
    _floats(weights, (n, 4), "weights")
    if not (torch.is_tensor(index) and index.is_cuda and index.dtype == torch.int32 and index.is_contiguous() and index.dim() == 1):
        raise ValueError("index must be a contiguous (M,) int32 CUDA tensor")
    _count_word(count, "count")
    _count_word(overflow, "overflow")
    if count is None or overflow is None:
        raise ValueError("count and overflow are required")
    if max_count is None:
        max_count = out_rays.shape[0] if out_rays is not None else 2 * n
    m = int(max_count)
    if not 0 <= min(m, 2 * n) <= index.shape[0]:
        raise ValueError("index must hold every candidate that can be kept")
    dev = reflected.device
    if out_rays is None:
        out_rays = torch.empty((m, 11), dtype=torch.int32, device=dev)
    if out_contribution is None:
        out_contribution = torch.empty((m,), dtype=torch.float32, device=dev)
    if out_parent is None:
        out_parent = torch.empty((m,), dtype=torch.int32, device=dev)
    if out_count is None:
        out_count = torch.empty((1,), dtype=torch.int32, device=dev)
    _records(out_rays, 11, "out_rays")
    if out_rays.shape[0] < m or out_contribution.shape[0] < m or out_parent.shape[0] < m:
        raise ValueError("the child arrays must hold max_count records")
    _floats(out_contribution, out_contribution.shape[:1], "out_contribution")
    _column(out_parent, torch.int32, out_parent.shape[0], "out_parent")
    _count_word(out_count, "out_count")
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
    import torch

    records = _hit_records(hits)
    n = records.shape[0]
    _rgb(shade, n, "shade")
    _count_word(count, "count")
    if not (torch.is_tensor(out) and out.dim() == 2):
        raise ValueError("out must be a contiguous (M, 3) float32 CUDA tensor")
    _rgb(out, out.shape[0], "out")
    if int(depth_left) > 0 and (weights is None or refr_kind is None or travel is None or child_values is None):
        raise ValueError("weights, refr_kind, travel and child_values are required when depth_left > 0")
    if weights is not None:
        _floats(weights, (n, 4), "weights")
    if refr_kind is not None:
        _column(refr_kind, torch.int32, n, "refr_kind")
    if travel is not None:
        _column(travel, torch.float32, n, "travel")
    if child_values is not None:
        _floats(child_values, (2 * n, 3), "child_values")
    if parent is not None:
        _column(parent, torch.int32, n, "parent")
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
    import torch

    _records(rays, 11, "rays")
    n = rays.shape[0]
    dev = rays.device
    out = _out_tensor(out, (n, 3), torch.float32, dev)
    _count_ptr(ray_count)
    _count_word(overflow, "overflow")
    if max_depth > _capi.RT_MAX_DEPTH:
        raise RtError(-5, f"max_depth above RT_MAX_DEPTH ({_capi.RT_MAX_DEPTH})")
    depth = max(int(max_depth), 0)
    if level_counts is not None:
        _column(level_counts, torch.int32, depth + 1, "level_counts")
    if torch.is_tensor(contribution):
        _floats(contribution, (n,), "contribution")
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

    def new(shape, dtype):
        return torch.empty(shape, dtype=dtype, device=dev)

    # allocated (and the fills enqueued) with `stream` as torch's current stream: the caching allocator then ties the blocks to it
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        i32, f32, u8 = torch.int32, torch.float32, torch.uint8
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
        lws = light_workspace(scene, top, dev) if open_casts else None
        rws = refract_workspace(top, dev) if open_casts and depth > 0 else None
    select_records(flags[:top], identity, n_all, stream=s)  # 0 .. top-1: the child levels are cast through it with their own counts

    def shade_level(level_hits, level_rays, out):  # get_shade, in one kernel or light by light
        if open_casts:
            return shade_hits_by_light(scene, level_hits, level_rays, out=out, ray_count=ray_count, stream=s, workspace=lws)
        return shade_hits(scene, level_hits, level_rays, out=out, ray_count=ray_count, stream=s)

    def refract(level_hits, level_rays, out):  # get_refract(100.0), in one kernel or bounce by bounce
        if open_casts:
            return refract_rays_by_bounce(scene, level_hits, level_rays, 100.0, ray_count=ray_count, stream=s, out=out, workspace=rws)
        return refract_rays(scene, level_hits, level_rays, 100.0, ray_count=ray_count, stream=s, out=out)

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
            tree_gather(index[:2 * c], selected, reflected[:c], escape[:c], cur_contribution[:c], weights[k], overflow, caps[k + 1],
                        level_rays[nxt], level_contribution[nxt], parent[k + 1], count[k + 1], stream=s)
            cur_rays, cur_contribution = level_rays[nxt], level_contribution[nxt]
    for k in reversed(range(depth + 1)):
        left = depth - k
        tree_fold(hits[k], left, shade[k], out if k == 0 else child_values[k - 1], None if k == 0 else count[k],
                  weights[k] if left > 0 else None, refr_kind[k] if left > 0 else None, travel[k] if left > 0 else None,
                  child_values[k] if left > 0 else None, parent[k], stream=s)
    if check:
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
            dropped = int(overflow.item())  # the one readback: it waits for the loop
        if dropped != 0:
            raise RtError(-5, f"trace_rays_levels: {dropped} child records did not fit their level's capacity (level_capacity)")
    return out

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
    import torch

    records, n = _hits_and_rays(hits, rays)
    first, count = _light_range(scene, light_first, light_count)
    pairs = count * n
    dev = records.device
    if out_rays is None:
        out_rays = torch.empty((pairs, 11), dtype=torch.int32, device=dev)
    if out_asks is None:
        out_asks = torch.empty((pairs,), dtype=torch.uint8, device=dev)
    if out_distance is None and distance:
        out_distance = torch.empty((pairs,), dtype=torch.float32, device=dev)
    _records(out_rays, 11, "out_rays")
    if out_rays.shape[0] != pairs:
        raise ValueError("out_rays must have one record per (light, hit) pair")
    _column(out_asks, torch.uint8, pairs, "out_asks")
    if out_distance is not None:
        _column(out_distance, torch.float32, pairs, "out_distance")
    _capi.check(_capi.amd_lib().rt_light_rays(scene._h, _p(records), _p(rays), n, first, count, _p(out_rays), _p(out_asks), _p(out_distance),
                                              _stream_ptr(stream)))
    return out_rays, out_asks, out_distance


def light_terms(scene: Scene, hits, rays, asks, shadow_hits, light_first: int = 0, light_count=None, out_lit=None, out_diffuse=None,
                out_specular=None, stream=None):
    """main.rs:435-459 per hit and light (rt_light_terms): returns (lit, diffuse, specular), light-major as light_rays' outputs.
    ``shadow_hits`` (L*N, 13) int32: what a cast of the shadow rays wrote, read only where ``asks`` is set.  ``lit`` (L*N,) uint8: 1
    where the light asks, is Some and is not occluded; there ``diffuse`` and ``specular`` (L*N, 3) float32 are get_diffuse and
    get_specular times the light's colour, not yet weighted by shiness; +0 elsewhere."""
    import torch

    records, n = _hits_and_rays(hits, rays)
    first, count = _light_range(scene, light_first, light_count)
    pairs = count * n
    dev = records.device
    _column(asks, torch.uint8, pairs, "asks")
    _records(shadow_hits, 13, "shadow_hits")
    if shadow_hits.shape[0] != pairs:
        raise ValueError("shadow_hits must have one record per (light, hit) pair")
    if out_lit is None:
        out_lit = torch.empty((pairs,), dtype=torch.uint8, device=dev)
    if out_diffuse is None:
        out_diffuse = torch.empty((pairs, 3), dtype=torch.float32, device=dev)
    if out_specular is None:
        out_specular = torch.empty((pairs, 3), dtype=torch.float32, device=dev)
    _column(out_lit, torch.uint8, pairs, "out_lit")
    _rgb(out_diffuse, pairs, "out_diffuse")
    _rgb(out_specular, pairs, "out_specular")
    _capi.check(_capi.amd_lib().rt_light_terms(scene._h, _p(records), _p(rays), n, first, count, _p(asks), _p(shadow_hits), _p(out_lit),
                                               _p(out_diffuse), _p(out_specular), _stream_ptr(stream)))
    return out_lit, out_diffuse, out_specular


def light_fold(scene: Scene, hits, lit, diffuse, specular, out, stream=None):
    """main.rs:461 (rt_light_fold): for the L = len(lit) / N lights of ``lit``, ``diffuse`` and ``specular`` in order, where lit:
    out = (out + diffuse * (1 - shiness)) + specular * shiness, in place on ``out`` ((N, 3) float32, required).  The call ADDS: zero
    ``out`` before the first range of lights; later ranges continue the sum.  A record that is no hit is not written."""
    import torch

    records = _hit_records(hits)
    n = records.shape[0]
    _rgb(out, n, "out")
    if not (torch.is_tensor(lit) and lit.dim() == 1):
        raise ValueError("lit must be a contiguous (L*N,) uint8 CUDA tensor")
    pairs = lit.shape[0]
    if pairs % n != 0 if n else pairs != 0:
        raise ValueError("lit must have one entry per (light, hit) pair")
    count = pairs // n if n else 0
    _column(lit, torch.uint8, pairs, "lit")
    _rgb(diffuse, pairs, "diffuse")
    _rgb(specular, pairs, "specular")
    _capi.check(_capi.amd_lib().rt_light_fold(scene._h, _p(records), n, count, _p(lit), _p(diffuse), _p(specular), _p(out), _stream_ptr(stream)))
    return out


class LightWorkspace:
    """The buffers of one pass of shade_hits_by_light, made once by light_workspace so that a caller's loop allocates nothing:
    ``pairs`` (hit, light) pairs of room."""

    def __init__(self, pairs: int, device):
        import torch

        self.pairs = int(pairs)
        i32, f32, u8 = torch.int32, torch.float32, torch.uint8
        self.shadow_rays = torch.empty((pairs, 11), dtype=i32, device=device)
        self.shadow_hits = torch.empty((pairs, 13), dtype=i32, device=device)
        self.asks, self.lit = torch.empty((pairs,), dtype=u8, device=device), torch.empty((pairs,), dtype=u8, device=device)
        self.index, self.count = torch.empty((pairs,), dtype=i32, device=device), torch.empty((1,), dtype=i32, device=device)
        self.diffuse, self.specular = torch.empty((pairs, 3), dtype=f32, device=device), torch.empty((pairs, 3), dtype=f32, device=device)


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
    import torch

    records, n = _hits_and_rays(hits, rays)
    dev = records.device
    out = _out_tensor(out, (n, 3), torch.float32, dev)
    _count_ptr(ray_count)
    lights = scene.n_lights
    per_pass = lights if lights_per_pass is None else int(lights_per_pass)
    if lights_per_pass is not None and per_pass < 1:
        raise ValueError("lights_per_pass must be at least 1")
    per_pass = min(per_pass, lights)
    if n * per_pass >= 1 << 32:
        raise RtError(-5, "2^32 (hit, light) pairs or more in one pass (lights_per_pass)")
    s = stream
    # allocated (and the fill enqueued) with `stream` as torch's current stream: the caching allocator then ties the blocks to it
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
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
    import torch

    records, n = _hits_and_rays(hits, rays)
    dev = records.device
    if out_rays is None:
        out_rays = torch.empty((n, 11), dtype=torch.int32, device=dev)
    if out_kind is None:
        out_kind = torch.empty((n,), dtype=torch.int32, device=dev)
    if out_travel is None:
        out_travel = torch.empty((n,), dtype=torch.float32, device=dev)
    if out_casts is None:
        out_casts = torch.empty((n,), dtype=torch.int32, device=dev)
    if out_flags is None:
        out_flags = torch.empty((n,), dtype=torch.uint8, device=dev)
    _records(out_rays, 11, "out_rays")
    if out_rays.shape[0] != n:
        raise ValueError("out_rays must have one record per hit")
    _column(out_kind, torch.int32, n, "out_kind")
    _column(out_travel, torch.float32, n, "out_travel")
    _column(out_casts, torch.int32, n, "out_casts")
    _column(out_flags, torch.uint8, n, "out_flags")
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
    import torch

    records = _hit_records(hits)
    n = records.shape[0]
    _records(inside_hits, 13, "inside_hits")
    _records(inside_rays, 11, "inside_rays")
    if inside_hits.shape[0] != n or inside_rays.shape[0] != n:
        raise ValueError("inside_hits and inside_rays must have one record per hit")
    _column(kind, torch.int32, n, "kind")
    _column(travel, torch.float32, n, "travel")
    _column(casts, torch.int32, n, "casts")
    _column(flags, torch.uint8, n, "flags")
    if out_escape is None:
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
            out_escape = torch.zeros((n, 11), dtype=torch.int32, device=records.device)
    _records(out_escape, 11, "out_escape")
    if out_escape.shape[0] != n:
        raise ValueError("out_escape must have one record per hit")
    _capi.check(_capi.amd_lib().rt_refract_step(scene._h, _p(records), n, float(max_distance), _p(inside_hits), _p(inside_rays), _p(kind),
                                                _p(travel), _p(casts), _p(flags), _p(out_escape), _stream_ptr(stream)))
    return out_escape


class RefractWorkspace:
    """The state and scratch of refract_rays_by_bounce beside its result, made once by refract_workspace so that a caller's loop
    allocates nothing; ``n`` records of room.  ``rays`` (n, 11): the ray in flight (for an INFINITE record the ray whose cast missed),
    ``inside_hits`` (n, 13), ``casts`` (n,) int32: the casts answered per record, ``flags`` (n,) uint8, ``index`` / ``count``:
    select_records' list."""

    def __init__(self, n: int, device):
        import torch

        self.n = int(n)
        i32, u8 = torch.int32, torch.uint8
        self.rays = torch.empty((n, 11), dtype=i32, device=device)
        self.inside_hits = torch.empty((n, 13), dtype=i32, device=device)
        self.casts = torch.empty((n,), dtype=i32, device=device)
        self.flags, self.index, self.count = torch.empty((n,), dtype=u8, device=device), torch.empty((n,), dtype=i32, device=device), torch.empty((1,), dtype=i32, device=device)
        self._mask = [torch.empty((n,), dtype=torch.bool, device=device) for _ in range(2)]


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
    import torch

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
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        if out is None:
            out = Refractions(torch.empty((n,), dtype=torch.int32, device=dev), torch.empty((n,), dtype=torch.float32, device=dev),
                              torch.empty((n, 11), dtype=torch.int32, device=dev))
        kind, travel, escape = out.kind, out.travel, out.rays
        _column(kind, torch.int32, n, "out.kind")
        _column(travel, torch.float32, n, "out.travel")
        _records(escape, 11, "out.rays")
        if escape.shape[0] != n:
            raise ValueError("out must have one record per hit")
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
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        ended, not_walking = w._mask[0][:n], w._mask[1][:n]
        torch.ne(kind, ESCAPED, out=ended)
        torch.ne(kind, WALKING, out=not_walking)
        ended.logical_and_(not_walking)
        travel.masked_fill_(ended, 0.0)  # travel_distance belongs to Escaped alone (main.rs:402)
    return out


# ---- record ordering: coherence keys, a stable sort of an index list, gather and scatter (include/rt_amd.h rt_ray_keys ... rt_scatter_records) ----

ORDER_DIRECTION_MAJOR = 1  # RT_ORDER_DIRECTION_MAJOR: the direction code above the origin code


def _words(t, name):
    """a contiguous CUDA tensor of 4-byte elements, one or two dimensional: (records, words per record)"""
    import torch

    if not (torch.is_tensor(t) and t.is_cuda and t.is_contiguous() and t.element_size() == 4 and t.dim() in (1, 2)):
        raise ValueError(f"{name} must be a contiguous CUDA tensor of 4-byte elements, (N,) or (N, words)")
    return t.shape[0], (1 if t.dim() == 1 else t.shape[1])


def _box3(v, name):
    a = np.asarray(v, dtype=np.float32).reshape(-1)
    if a.shape != (3,):
        raise ValueError(f"{name} must hold 3 floats")
    return (C.c_float * 3)(*a.tolist())


def ray_keys(rays, box_lo, box_hi, flags: int = 0, out=None, stream=None):
    """A 30-bit coherence key per ray (rt_ray_keys): the origin's cell in a 64^3 grid over the box ``box_lo`` .. ``box_hi`` (host
    values, e.g. World.bounds()) and the direction's cell in a 64^2 grid over the octahedral map, both in Z-order; origin-major, or
    direction-major with ORDER_DIRECTION_MAJOR.  ``rays``: (N, 11) int32 rt_ray records; returns ``out``, an (N,) int32 CUDA tensor."""
    import torch

    _records(rays, 11, "rays")
    n = rays.shape[0]
    if out is None:
        out = torch.empty((n,), dtype=torch.int32, device=rays.device)
    _column(out, torch.int32, n, "out")
    _capi.check(_capi.amd_lib().rt_ray_keys(_p(rays), n, _box3(box_lo, "box_lo"), _box3(box_hi, "box_hi"), int(flags), _p(out), _stream_ptr(stream)))
    return out


def sort_temp_bytes(n: int) -> int:
    """The workspace sort_records needs for N records (rt_sort_temp_bytes: host arithmetic)."""
    return int(_capi.amd_lib().rt_sort_temp_bytes(int(n)))


def sort_records(keys, first_bit: int = 0, key_bits: int = 32, index=None, count=None, out=None, temp=None, stream=None):
    """Stable radix sort of an index list by bits [first_bit, first_bit + key_bits) of ``keys[index]`` (rt_sort_records), ascending,
    equal keys in input order.  ``keys``: an (N,) int32 CUDA tensor (ray_keys, or any words of the caller's).  ``index``: None for the
    identity list, or an (N,) int32 CUDA tensor whose first min(count[0], N) entries are the list (``count``: a 1-element int32 CUDA
    tensor that stays on the device, None for N); an entry >= N sorts last and keeps its value.  Returns ``out`` ((N,) int32, allocated
    if None, may be ``index`` itself): its first min(count[0], N) entries are the sorted list.  ``temp``: a uint8 CUDA tensor of at
    least sort_temp_bytes(N) bytes (allocated if None).  Nothing is read back: the call may be captured into a graph."""
    import torch

    if not (torch.is_tensor(keys) and keys.is_cuda and keys.dtype == torch.int32 and keys.is_contiguous() and keys.dim() == 1):
        raise ValueError("keys must be a contiguous (N,) int32 CUDA tensor")
    n = keys.shape[0]
    if index is not None:
        _column(index, torch.int32, n, "index")
    if count is not None:
        _column(count, torch.int32, 1, "count")
    if out is None:
        out = torch.empty((n,), dtype=torch.int32, device=keys.device)
    _column(out, torch.int32, n, "out")
    need = sort_temp_bytes(n)
    if temp is None:
        temp = torch.empty((need,), dtype=torch.uint8, device=keys.device)
    if not (torch.is_tensor(temp) and temp.is_cuda and temp.dtype == torch.uint8 and temp.is_contiguous() and temp.dim() == 1):
        raise ValueError("temp must be a contiguous 1-d uint8 CUDA tensor")
    _capi.check(_capi.amd_lib().rt_sort_records(_p(keys), n, int(first_bit), int(key_bits), _p(index), _p(count), _p(out), _p(temp), temp.numel(),
                                                _stream_ptr(stream)))
    return out


def _move_records(src, index, count, out, n_out, max_count):
    import torch

    n_src, words = _words(src, "src")
    if not (torch.is_tensor(index) and index.is_cuda and index.dtype == torch.int32 and index.is_contiguous() and index.dim() == 1):
        raise ValueError("index must be a contiguous (M,) int32 CUDA tensor")
    if count is not None:
        _column(count, torch.int32, 1, "count")
    m = index.shape[0] if max_count is None else int(max_count)
    if not 0 <= m <= index.shape[0]:
        raise ValueError("max_count must not exceed the length of index")
    if out is None:
        out = torch.zeros((n_out,) + tuple(src.shape[1:]), dtype=src.dtype, device=src.device)
    if _words(out, "out")[1] != words or out.dtype != src.dtype:
        raise ValueError("out must hold records of the same words as src")
    return out, n_src, words, m


def gather_records(src, index, count=None, out=None, max_count=None, stream=None):
    """out[j] = src[index[j]] for j < min(count[0], max_count), all-zero words where index[j] >= N (rt_gather_records).  ``src``: a
    contiguous CUDA tensor of 4-byte elements, (N,) or (N, words) with 1 to 64 words per record; ``index``: an (M,) int32 CUDA tensor;
    ``count``: a 1-element int32 CUDA tensor or None (= max_count, default M).  ``out``: (at least max_count, words), allocated if None."""
    out, n, words, m = _move_records(src, index, count, out, index.shape[0] if max_count is None else int(max_count), max_count)
    if out.shape[0] < m:
        raise ValueError("out must hold max_count records")
    _capi.check(_capi.amd_lib().rt_gather_records(_p(src), 4 * words, n, _p(index), _p(count), m, _p(out), _stream_ptr(stream)))
    return out


def scatter_records(src, index, out, count=None, max_count=None, stream=None):
    """out[index[j]] = src[j] for j < min(count[0], max_count); an index >= N, the records of ``out`` (required), is skipped
    (rt_scatter_records).  Records of ``out`` that no entry names are not written; of two entries naming one record either may win."""
    out, n_src, words, m = _move_records(src, index, count, out, 0, max_count)
    if n_src < m:
        raise ValueError("src must hold max_count records")
    _capi.check(_capi.amd_lib().rt_scatter_records(_p(src), 4 * words, out.shape[0], _p(index), _p(count), m, _p(out), _stream_ptr(stream)))
    return out


class OrderWorkspace:
    """The buffers of cast_rays_ordered / trace_rays_ordered for up to ``n`` rays, allocated once: keys, the sorted list, its count
    word (n, written at creation), the sort's workspace and — for trace_rays_ordered — the gathered rays and their values."""

    def __init__(self, n: int, device, trace: bool = False):
        import torch

        self.n = int(n)
        self.keys = torch.empty((self.n,), dtype=torch.int32, device=device)
        self.index = torch.empty((self.n,), dtype=torch.int32, device=device)
        self.count = torch.full((1,), self.n if self.n < 2 ** 31 else self.n - 2 ** 32, dtype=torch.int32, device=device)
        self.temp = torch.empty((sort_temp_bytes(self.n),), dtype=torch.uint8, device=device)
        self.rays = torch.empty((self.n, 11), dtype=torch.int32, device=device) if trace else None
        self.rgb = torch.empty((self.n, 3), dtype=torch.float32, device=device) if trace else None


def order_workspace(n: int, device, trace: bool = False) -> OrderWorkspace:
    return OrderWorkspace(n, device, trace)


def _scene_box(scene: Scene, box):
    if box is not None:
        lo, hi = box
        return lo, hi
    if getattr(scene, "_bounds", None) is None:
        scene._bounds = _desc_bounds(scene._desc)  # of the description the scene was created from
    return scene._bounds


def _order_list(scene, rays, box, flags, workspace, trace, stream):
    n = rays.shape[0]
    w = workspace if workspace is not None else OrderWorkspace(n, rays.device, trace)
    if w.n != n or (trace and w.rays is None):
        raise ValueError("the workspace was made for another number of rays (or without trace=True)")
    lo, hi = _scene_box(scene, box)
    ray_keys(rays, lo, hi, flags, out=w.keys, stream=stream)
    sort_records(w.keys, 0, 30, out=w.index, temp=w.temp, stream=stream)
    return w


def cast_rays_ordered(scene: Scene, rays, box=None, flags: int = 0, out=None, ray_count=None, stream=None, workspace=None):
    """cast_rays with the waves filled in a coherent order: ray_keys, sort_records, then cast_rays_indexed through the sorted list — a
    wave takes 64 consecutive list entries, and each hit goes to its ray's own slot, so ``out`` ((N, 13) int32, allocated if None) is
    cast_rays' record for record, bit for bit.  ``box``: (lo, hi) for the origin cells; None takes the bounds of the description the
    scene was created from.  ``flags``: 0 or ORDER_DIRECTION_MAJOR.  ``workspace``: order_workspace(N, device), made here if None;
    after that the function only enqueues library calls."""
    import torch

    _records(rays, 11, "rays")
    n = rays.shape[0]
    out = _out_tensor(out, (n, 13), torch.int32, rays.device)
    if n == 0:
        return out
    w = _order_list(scene, rays, box, flags, workspace, False, stream)
    cast_rays_indexed(scene, rays, w.index, w.count, out, ray_count=ray_count, stream=stream)
    return out


def trace_rays_ordered(scene: Scene, rays, max_depth: int, contribution: float = 1.0, box=None, flags: int = 0, out=None, ray_count=None,
                       stream=None, workspace=None):
    """trace_rays with the waves filled in a coherent order: ray_keys, sort_records, gather_records of the rays, rt_trace_rays on the
    gathered batch, scatter_records of the values back to the caller's order.  The recursion of a ray does not depend on its
    neighbours, so ``out`` ((N, 3) float32, allocated if None) and the cast count are trace_rays' bit for bit.  ``workspace``:
    order_workspace(N, device, trace=True), made here if None."""
    import torch

    _records(rays, 11, "rays")
    n = rays.shape[0]
    out = _out_tensor(out, (n, 3), torch.float32, rays.device)
    if n == 0:
        return out
    w = _order_list(scene, rays, box, flags, workspace, True, stream)
    gather_records(rays, w.index, out=w.rays, stream=stream)
    trace_rays(scene, w.rays, max_depth, contribution, out=w.rgb, ray_count=ray_count, stream=stream)
    scatter_records(w.rgb, w.index, out, stream=stream)
    return out


# ---- mesh ordering: triangle keys and the permutation that makes the node tree selective (include/rt_amd.h rt_triangle_keys, rt_order_triangles) ----

TRIANGLE_WORDS = C.sizeof(Triangle) // 4  # 25: the object word, then three vertices of eight floats


def triangle_keys(triangles, box_lo, box_hi, out=None, objects=None, stream=None):
    """A 30-bit Z-order key per triangle (rt_triangle_keys): the cell of its centroid in a 1024^3 grid over the box ``box_lo`` ..
    ``box_hi`` (host values, e.g. World.bounds()).  ``triangles``: (N, 25) int32 rt_triangle records; returns ``out``, an (N,) int32
    CUDA tensor.  ``objects``: None, or an (N,) int32 CUDA tensor that receives the object indices."""
    import torch

    _records(triangles, TRIANGLE_WORDS, "triangles")
    n = triangles.shape[0]
    if out is None:
        out = torch.empty((n,), dtype=torch.int32, device=triangles.device)
    _column(out, torch.int32, n, "out")
    if objects is not None:
        _column(objects, torch.int32, n, "objects")
    _capi.check(_capi.amd_lib().rt_triangle_keys(_p(triangles), n, _box3(box_lo, "box_lo"), _box3(box_hi, "box_hi"), _p(out), _p(objects),
                                                 _stream_ptr(stream)))
    return out


def order_triangles_temp_bytes(n: int) -> int:
    """The workspace order_triangles needs for N triangles (rt_order_triangles_temp_bytes: host arithmetic)."""
    return int(_capi.amd_lib().rt_order_triangles_temp_bytes(int(n)))


def order_triangles(triangles, box_lo, box_hi, n_objects: int, out=None, ordered=None, temp=None, stream=None):
    """The permutation that groups triangles by object and, inside an object, by triangle_keys' Z-order, equal pairs in input order
    (rt_order_triangles: the keys, two stable sorts and a gather as one call).  ``triangles``: (N, 25) int32 rt_triangle records;
    ``n_objects``: the world's number of materials.  Returns ``out`` ((N,) int32, allocated if None): out[j] is the old index of the
    triangle at new position j.  ``ordered``: None, or an (N, 25) int32 CUDA tensor that receives triangles[out].  ``temp``: a uint8
    CUDA tensor of at least order_triangles_temp_bytes(N) bytes (allocated if None).  Nothing is read back: the call may be captured."""
    import torch

    _records(triangles, TRIANGLE_WORDS, "triangles")
    n = triangles.shape[0]
    if out is None:
        out = torch.empty((n,), dtype=torch.int32, device=triangles.device)
    _column(out, torch.int32, n, "out")
    if ordered is not None:
        _records(ordered, TRIANGLE_WORDS, "ordered")
        if ordered.shape[0] != n:
            raise ValueError("ordered must have one record per triangle")
    need = order_triangles_temp_bytes(n)
    if temp is None:
        temp = torch.empty((need,), dtype=torch.uint8, device=triangles.device)
    if not (torch.is_tensor(temp) and temp.is_cuda and temp.dtype == torch.uint8 and temp.is_contiguous() and temp.dim() == 1):
        raise ValueError("temp must be a contiguous 1-d uint8 CUDA tensor")
    _capi.check(_capi.amd_lib().rt_order_triangles(_p(triangles), n, _box3(box_lo, "box_lo"), _box3(box_hi, "box_hi"), int(n_objects), _p(out),
                                                   _p(ordered), _p(temp), temp.numel(), _stream_ptr(stream)))
    return out


def _perm(perm):
    p = np.asarray(perm)
    if p.ndim != 1 or p.dtype.kind not in "ui":
        raise ValueError("perm must be a 1-d integer array")
    return p.astype(np.int64)


def unorder_hits(hits_np, perm):
    """Hits cast on an ordered world (World.ordered) in the numbering of the world it was made from: a copy of ``hits_np`` (HIT_DTYPE
    or (N, 13) words) in which ``index`` of every triangle hit is perm[index].  Sphere hits and HIT_NONE records are untouched."""
    h = _host_records(hits_np, HIT_DTYPE, 13, "hits").copy()
    p = _perm(perm)
    index = h["index"].astype(np.int64)
    mine = (h["kind"] == TRIANGLE) & (index < p.size)
    h["index"][mine] = p[index[mine]].astype(np.uint32)
    return h


def order_rays(rays_np, perm):
    """Rays meant for a world in the numbering of its ordered form (World.ordered): a copy of ``rays_np`` (RAY_DTYPE or (N, 11) words) in
    which a triangle ``exclude_index`` i becomes the j with perm[j] == i.  An index outside the array stays as it is (it excludes
    nothing either way); sphere exclusions and rays without one are untouched."""
    r = _host_records(rays_np, RAY_DTYPE, 11, "rays").copy()
    p = _perm(perm)
    inverse = np.empty(p.size, dtype=np.int64)
    inverse[p] = np.arange(p.size)
    index = r["exclude_index"].astype(np.int64)
    mine = (r["has_exclude"] != 0) & (r["exclude_kind"] == TRIANGLE) & (index < p.size)
    r["exclude_index"][mine] = inverse[index[mine]].astype(np.uint32)
    return r


def render_distributed_numpy(scene: Scene, camera: Camera, frame: Frame, rng: Rng, n_epochs: int, img: np.ndarray,
                             focus: float = 3.0, blur: float = 0.04) -> int:
    """`n_epochs` epochs of the stochastic loop added into the host image `img` ((rows, cols, 3) f32, in place):
    rt_render_distributed_host, the form a host-resident `img` binds (src/main.rs:1131-1167).  Returns the cast count."""
    if not (img.dtype == np.float32 and img.flags.c_contiguous and img.shape == (frame.rows, frame.cols, 3)):
        raise ValueError("expected a contiguous (rows, cols, 3) float32 array")
    casts = C.c_ulonglong(0)
    _capi.check(_capi.amd_lib().rt_render_distributed_host(scene._h, C.byref(camera), C.byref(frame), float(focus), float(blur), rng._h,
                                                           int(n_epochs), img.ctypes.data_as(C.c_void_p), C.byref(casts)))
    return int(casts.value)


def set_option(name: str, value=None) -> None:
    """A process-wide switch of librt_amd.so (include/rt_amd.h rt_set_option): an integer named like the environment variable that
    seeds it (the environment is read once per process); None unsets it.  None of them changes a result."""
    _capi.check(_capi.amd_lib().rt_set_option(name.encode(), None if value is None else str(int(value)).encode()))


class options:
    """`with rt.options(RT_AMD_DIST_PIPELINE=0, RT_AMD_DIST_WS_MB=16): ...` — switches set for the block, unset after it."""

    def __init__(self, **switches):
        self._switches = switches

    def __enter__(self):
        for k, v in self._switches.items():
            set_option(k, v)
        return self

    def __exit__(self, *exc):
        for k in self._switches:
            set_option(k, None)
        return False


def post_process_device(img, divisor=None, stream=None):
    """In-place p99-luma normalisation of a (rows, cols, 3) f32 CUDA tensor (src/main.rs:748-762), on the device."""
    import torch

    assert img.is_cuda and img.dtype == torch.float32 and img.is_contiguous() and img.shape[-1] == 3
    _capi.check(_capi.amd_lib().rt_post_process_device(C.c_void_p(img.data_ptr()), img.numel() // 3,
                                                      None if divisor is None else C.c_void_p(divisor.data_ptr()), _stream_ptr(stream)))
    return img


def encode_srgb8_device(img, out=None, stream=None):
    """Linear f32 -> sRGB u8 on the device (src/image.rs:55-66)."""
    import torch

    assert img.is_cuda and img.dtype == torch.float32 and img.is_contiguous()
    if out is None:
        out = torch.empty(img.shape, dtype=torch.uint8, device=img.device)
    _capi.check(_capi.amd_lib().rt_encode_srgb8_device(C.c_void_p(img.data_ptr()), img.numel(), C.c_void_p(out.data_ptr()), _stream_ptr(stream)))
    return out


class PhotonAccumulator:
    """src/photon.rs:9-34 (defined but unused by the reference's main()): per-pixel running sum and weight,
    resolved to sum / weight — a true average over the epochs of the stochastic pass, as the alternative to main()'s
    sum-and-renormalise.  Works on numpy arrays (librt_host.so) or CUDA tensors (librt_amd.so), bit-identically."""

    def __init__(self, rows: int, cols: int, device: str = "cpu"):
        self.rows, self.cols, self.device = rows, cols, device
        if device == "cpu":
            self.sum = np.zeros((rows, cols, 3), dtype=np.float32)
            self.weight = np.zeros((rows, cols), dtype=np.float32)
        else:
            import torch

            self.sum = torch.zeros((rows, cols, 3), dtype=torch.float32, device=device)
            self.weight = torch.zeros((rows, cols), dtype=torch.float32, device=device)

    def accumulate(self, samples, valid, stream=None) -> None:
        """accumulate() for every sample whose filter flag is set: samples (n_epochs, rows, cols, 3) f32, valid
        (n_epochs, rows, cols) u8 — the `samples` / `valid` outputs of render_distributed — in epoch order."""
        n_epochs = int(samples.shape[0])
        assert tuple(samples.shape) == (n_epochs, self.rows, self.cols, 3) and tuple(valid.shape) == (n_epochs, self.rows, self.cols)
        n_pixels = self.rows * self.cols
        if self.device == "cpu":
            assert samples.dtype == np.float32 and valid.dtype == np.uint8 and samples.flags.c_contiguous and valid.flags.c_contiguous
            _capi.host_lib().rt_accumulate(samples.ctypes.data_as(C.c_void_p), valid.ctypes.data_as(C.c_void_p), n_epochs, n_pixels,
                                           self.sum.ctypes.data_as(C.c_void_p), self.weight.ctypes.data_as(C.c_void_p))
        else:
            import torch

            assert samples.is_cuda and samples.dtype == torch.float32 and samples.is_contiguous()
            assert valid.is_cuda and valid.dtype == torch.uint8 and valid.is_contiguous()
            _capi.check(_capi.amd_lib().rt_accumulate_device(C.c_void_p(samples.data_ptr()), C.c_void_p(valid.data_ptr()), n_epochs, n_pixels,
                                                            C.c_void_p(self.sum.data_ptr()), C.c_void_p(self.weight.data_ptr()),
                                                            _stream_ptr(stream)))

    def resolve(self, stream=None):
        """into_rgb_internal: sum / weight, black where nothing was accumulated."""
        n_pixels = self.rows * self.cols
        if self.device == "cpu":
            out = np.empty((self.rows, self.cols, 3), dtype=np.float32)
            _capi.host_lib().rt_accumulator_resolve(self.sum.ctypes.data_as(C.c_void_p), self.weight.ctypes.data_as(C.c_void_p), n_pixels,
                                                    out.ctypes.data_as(C.c_void_p))
            return out
        import torch

        out = torch.empty((self.rows, self.cols, 3), dtype=torch.float32, device=self.device)
        _capi.check(_capi.amd_lib().rt_accumulator_resolve_device(C.c_void_p(self.sum.data_ptr()), C.c_void_p(self.weight.data_ptr()), n_pixels,
                                                                 C.c_void_p(out.data_ptr()), _stream_ptr(stream)))
        return out


def post_process(img: np.ndarray) -> float:
    """In-place p99-luma normalisation, src/main.rs:748-762.  Returns the divisor (0 = untouched)."""
    assert img.dtype == np.float32 and img.flags.c_contiguous and img.shape[-1] == 3
    return float(_capi.host_lib().rt_post_process(img.ctypes.data_as(C.c_void_p), img.size // 3))


def luma_row() -> tuple:
    """The three f32 luma weights of post_process: luma = (w0 * r + w1 * g) + w2 * b."""
    row = (C.c_float * 3)()
    _capi.host_lib().rt_luma_row(row)
    return (float(row[0]), float(row[1]), float(row[2]))


def encode_srgb8(img: np.ndarray) -> np.ndarray:
    """Linear f32 -> sRGB u8, src/image.rs:55-66."""
    assert img.dtype == np.float32 and img.flags.c_contiguous
    out = np.empty(img.shape, dtype=np.uint8)
    _capi.host_lib().rt_encode_srgb8(img.ctypes.data_as(C.c_void_p), img.size, out.ctypes.data_as(C.c_void_p))
    return out


def write_to_file(path: str, rgb8: np.ndarray) -> None:
    """RGB8 PNG via a temporary file + rename, src/main.rs:764-776."""
    assert rgb8.dtype == np.uint8 and rgb8.ndim == 3 and rgb8.shape[2] == 3 and rgb8.flags.c_contiguous
    _capi.check_host(_capi.host_lib().rt_write_png(str(Path(path)).encode(), rgb8.ctypes.data_as(C.c_void_p), rgb8.shape[1], rgb8.shape[0]))
