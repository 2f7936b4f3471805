"""Motion of the scene between two frames: where a hit's point was before the scene update (include/rt_amd.h "motion queries").

    keep_positions / positions_kept   the scene keeps its triangles' vertex positions and its spheres' centres and radii as they stand
    previous_positions                for hits on the scene as it stands now, the same surface points on the kept positions
    previous_positions_numpy          the CPU definition (rt_previous_positions_cpu, librt_host.so): no device, no torch
    accumulate_moving_frame           temporal.accumulate_frame for a scene that moves: the history is gathered from where each point was

The loop of an animated sequence is ``scene.update_*`` -> render -> ``accumulate_moving_frame``.  A fixed order of single f32 operations,
so CUDA tensors (librt_amd.so) and numpy arrays (librt_host.so) give the same bits; a primitive that did not move returns the hit position
bit for bit.  A public submodule (``rt.moving`` — ``motion`` is a function of ``rt.temporal``): its names are not re-exported at the top level.  Like the rest of the package it loads
torch on first use only.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi
from ._args import _host_records, _on_stream, _out_tensor, _p, _stream_ptr
from ._capi import Camera, Frame
from ._forms import CUDA
from ._queries import HIT_DTYPE, _hit_records
from ._world import Scene, World
from .materials import primary_surfaces
from .temporal import History

__all__ = ["keep_positions", "positions_kept", "previous_positions", "previous_positions_numpy", "accumulate_moving_frame"]


def keep_positions(scene: Scene, stream=None) -> None:
    """rt_scene_keep_positions: the scene copies its vertex positions, sphere centres and radii as they stand at this point of ``stream``
    (default: torch's current stream) into arrays it owns — what the next ``previous_positions`` answers on.  The first call on a scene
    allocates and cannot be captured into a graph; later calls can."""
    _capi.check(_capi.amd_lib().rt_scene_keep_positions(scene._h, _stream_ptr(stream)))


def positions_kept(scene: Scene) -> bool:
    """has ``keep_positions`` been called on ``scene`` (rt_scene_positions_kept)"""
    return _capi.check(_capi.amd_lib().rt_scene_positions_kept(scene._h)) != 0


def previous_positions(scene: Scene, hits, out=None, stream=None):
    """Where each hit's point was at the last ``keep_positions`` (rt_previous_positions): ``hits`` is a Hits or its (N, 13) int32 CUDA
    record tensor, cast on the scene as it stands now.  Returns ``out``: an (N, 3) float32 CUDA tensor (allocated if None), or any
    float32 view of N x 3 words with one record stride, such as a column range of a record tensor — the other words of a record are
    not written.  A record that is no hit, or names no primitive of the scene, gets three NaNs.  One kernel launch, stream-ordered on
    ``stream`` (default: torch's current stream), capturable when ``out`` is given."""
    records = _hit_records(hits)
    n = records.shape[0]
    if out is None:
        with _on_stream(stream):
            out = _out_tensor(None, (n, 3), "float32", records.device)
    p, stride = CUDA.plane(out, "out", "f", n, 3)
    _capi.check(_capi.amd_lib().rt_previous_positions(scene._h, _p(records), n, p, stride if n else 3, _stream_ptr(stream)))
    return out


def previous_positions_numpy(world_or_desc, was_triangles, was_spheres, hits) -> np.ndarray:
    """The CPU definition (rt_previous_positions_cpu, librt_host.so; no device, no torch).  ``world_or_desc``: the World or SceneDesc as
    it stands NOW — what ``hits`` (a HIT_DTYPE array or an (N, 13) array of 4-byte words) were cast on; ``was_triangles``: the kept vertex
    positions, n_triangles x 9 float32 (x y z of vertices 0, 1, 2), ``was_spheres``: n_spheres x 4 float32 (cx cy cz r); either may be
    None when the scene has none of the kind.  Returns a new (N, 3) float32 array."""
    desc = world_or_desc.desc() if isinstance(world_or_desc, World) else world_or_desc

    def kept(a, count, width, name):
        if a is None:
            return None
        a = np.ascontiguousarray(a)
        if a.dtype != np.float32 or a.size != count * width:
            raise ValueError(f"{name}: expected {count} x {width} float32")
        return a

    wt = kept(was_triangles, int(desc.n_triangles), 9, "was_triangles")
    ws = kept(was_spheres, int(desc.n_spheres), 4, "was_spheres")
    a = _host_records(hits, HIT_DTYPE, 13, "hits")
    n = a.shape[0]
    out = np.zeros((n, 3), dtype=np.float32)
    ptr = lambda x: None if x is None else C.c_void_p(x.ctypes.data)  # noqa: E731
    _capi.check_host(_capi.host_lib().rt_previous_positions_cpu(C.byref(desc), ptr(wt), ptr(ws), ptr(a), n, ptr(out), 3))
    return out


def accumulate_moving_frame(scene: Scene, camera: Camera, frame: Frame, image, history: History, stream=None):
    """``temporal.accumulate_frame`` for a scene that moves between frames: ``materials.primary_surfaces`` of ``camera`` over ``frame``;
    if the scene holds kept positions, ``previous_positions`` of those hits and ``history.push(..., position_was=...)``, otherwise a plain
    push; last ``keep_positions(scene)``, so that the next frame's updates are measured from this frame.  All on ``stream`` (default:
    torch's current stream).  Returns what push returns: (color, variance, length)."""
    with _on_stream(stream):
        s = primary_surfaces(scene, camera, frame, stream=stream)
        if positions_kept(scene):
            was = previous_positions(scene, s.hits, stream=stream).view(frame.rows, frame.cols, 3)
            result = history.push(s, camera, frame, image, stream=stream, position_was=was)
        else:
            result = history.push(s, camera, frame, image, stream=stream)
        keep_positions(scene, stream=stream)
        return result
