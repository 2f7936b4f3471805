"""The scene: the host-side World under construction and the device-resident Scene made from it."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np

from . import _capi
from ._args import _box3, _f3, _p, _stream_ptr, _torch
from ._capi import Camera, Light, Material, SceneDesc, Sphere, Triangle, Vertex

DEFAULT_OBJ = str(_capi.REPO_ROOT / "tests" / "golden" / "dodecahedron.obj")


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
        torch = _torch()
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
        _capi.check(_capi.amd_lib().rt_scene_update_vertices(self._h, int(first), n, _p(t), C.c_void_p(s.cuda_stream)))

    def update_spheres(self, first: int, spheres, stream=None) -> None:
        """rt_scene_update_spheres: spheres first .. get the rt_sphere records (object_index — ignored —, centre, radius: 5 words each)
        of ``spheres``, a CUDA tensor or a numpy / ctypes array of Sphere records."""
        t, n, s = self._device_records(spheres, C.sizeof(Sphere), "spheres", stream)
        _capi.check(_capi.amd_lib().rt_scene_update_spheres(self._h, int(first), n, _p(t), C.c_void_p(s.cuda_stream)))

    def _update_host_records(self, fn, first, records, ctype, stream):
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
