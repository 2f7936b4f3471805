"""The order of a batch of records and the order of a mesh: keys, the stable device sort, gather and scatter, the permutations."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi
from ._args import _box3, _host_records, _new, _out_tensor, _p, _stream_ptr, _tensor, _words
from ._capi import Triangle
from ._queries import HIT_DTYPE, RAY_DTYPE, TRIANGLE, cast_rays_indexed, trace_rays
from ._world import Scene, _desc_bounds

# ---- record ordering: coherence keys, a stable sort of an index list, gather and scatter (include/rt_amd.h rt_ray_keys ... rt_scatter_records) ----

ORDER_DIRECTION_MAJOR = 1  # RT_ORDER_DIRECTION_MAJOR: the direction code above the origin code


def _temp(temp, need, device):
    """the byte workspace of a sort: a new one of ``need`` bytes, or the caller's 1-d uint8 tensor (the library checks its length)"""
    return _new((need,), "uint8", device) if temp is None else _tensor(temp, "temp", "uint8", (None,))
def ray_keys(rays, box_lo, box_hi, flags: int = 0, out=None, stream=None):
    """A 30-bit coherence key per ray (rt_ray_keys): the origin's cell in a 64^3 grid over the box ``box_lo`` .. ``box_hi`` (host
    values, e.g. World.bounds()) and the direction's cell in a 64^2 grid over the octahedral map, both in Z-order; origin-major, or
    direction-major with ORDER_DIRECTION_MAJOR.  ``rays``: (N, 11) int32 rt_ray records; returns ``out``, an (N,) int32 CUDA tensor."""
    n = _tensor(rays, "rays", "int32", (None, 11)).shape[0]
    out = _out_tensor(out, (n,), "int32", rays.device)
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
    n = _tensor(keys, "keys", "int32", (None,)).shape[0]
    _tensor(index, "index", "int32", (n,), optional=True)
    _tensor(count, "count", "int32", (1,), optional=True)
    out = _out_tensor(out, (n,), "int32", keys.device)
    temp = _temp(temp, sort_temp_bytes(n), keys.device)
    _capi.check(_capi.amd_lib().rt_sort_records(_p(keys), n, int(first_bit), int(key_bits), _p(index), _p(count), _p(out), _p(temp), temp.numel(),
                                                _stream_ptr(stream)))
    return out


def _move_records(src, index, count, out, n_out, max_count):
    n_src, words = _words(src, "src")
    _tensor(index, "index", "int32", (None,))
    _tensor(count, "count", "int32", (1,), optional=True)
    m = index.shape[0] if max_count is None else int(max_count)
    if not 0 <= m <= index.shape[0]:
        raise ValueError("max_count must not exceed the length of index")
    if out is None:
        out = _new((n_out,) + tuple(src.shape[1:]), src.dtype, src.device).zero_()
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
        self.n = int(n)
        self.keys, self.index = _new((self.n,), "int32", device), _new((self.n,), "int32", device)
        self.count = _new((1,), "int32", device).fill_(self.n if self.n < 2 ** 31 else self.n - 2 ** 32)
        self.temp = _new((sort_temp_bytes(self.n),), "uint8", device)
        self.rays = _new((self.n, 11), "int32", device) if trace else None
        self.rgb = _new((self.n, 3), "float32", device) if trace else None


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
    n = _tensor(rays, "rays", "int32", (None, 11)).shape[0]
    out = _out_tensor(out, (n, 13), "int32", rays.device)
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
    n = _tensor(rays, "rays", "int32", (None, 11)).shape[0]
    out = _out_tensor(out, (n, 3), "float32", rays.device)
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
    n = _tensor(triangles, "triangles", "int32", (None, TRIANGLE_WORDS)).shape[0]
    out = _out_tensor(out, (n,), "int32", triangles.device)
    _tensor(objects, "objects", "int32", (n,), optional=True)
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
    n = _tensor(triangles, "triangles", "int32", (None, TRIANGLE_WORDS)).shape[0]
    out = _out_tensor(out, (n,), "int32", triangles.device)
    _tensor(ordered, "ordered", "int32", (n, TRIANGLE_WORDS), optional=True)
    temp = _temp(temp, order_triangles_temp_bytes(n), triangles.device)
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
