"""The material at a hit: approx, adjust_normal and the Phong terms on caller-supplied hits (include/rt_amd.h "material queries").

    material_hits / material_hits_numpy      src/main.rs:408-410 (approx(hit.at), adjust_normal(hit.at.normal)) per hit, as rt_surface records
    probe_surfaces / probe_surfaces_numpy    src/materials.rs:46-66 (get_diffuse, get_specular) of such records for the caller's own directions
    primary_surfaces                         camera_rays -> cast_rays -> material_hits, with the planes a denoiser asks for as views

A public submodule (``rt.materials``): its names are not re-exported at the top level.  Like the rest of the package it loads torch on
first use only.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import numpy as np

from . import _capi
from ._args import _host_records, _out_tensor, _p, _stream_ptr, _tensor, _torch
from ._capi import Camera, Frame
from ._queries import HIT_DTYPE, _hit_records, camera_rays, cast_rays
from ._world import Scene

__all__ = ["SURFACE_DTYPE", "SURFACE_WORDS", "PrimarySurfaces", "material_hits", "material_hits_numpy", "probe_surfaces", "probe_surfaces_numpy",
           "primary_surfaces"]

SURFACE_WORDS = _capi.SURFACE_WORDS  # 18
# rt_surface, 72 bytes: words 0..13 in the order of Material::approx's fields, then the shading normal and the flag
SURFACE_DTYPE = np.dtype([("normal", "<f4", 3), ("diffuse_color", "<f4", 3), ("shiness", "<f4"), ("specular_color", "<f4", 3),
                          ("smoothness", "<f4"), ("transparency", "<f4"), ("refraction_index", "<f4"), ("opaque_decay", "<f4"),
                          ("shading_normal", "<f4", 3), ("valid", "<u4")])


def material_hits(scene: Scene, hits, out=None, stream=None):
    """approx(hit.at) and adjust_normal(hit.at.normal) (src/main.rs:408-410) for every hit (rt_material_hits): ``hits`` is a Hits or its
    (N, 13) int32 CUDA record tensor; returns ``out``, an (N, 18) int32 CUDA tensor of rt_surface records (allocated if None; held as
    the other record tensors are — SURFACE_DTYPE names the fields, ``out.view(torch.float32)`` reads words 0..16).  A record that is no
    hit, or names no material of the scene, is 18 zero words.  The scene's live materials are read.  Stream-ordered on ``stream``."""
    records = _hit_records(hits)
    n = records.shape[0]
    out = _out_tensor(out, (n, SURFACE_WORDS), "int32", records.device)
    _capi.check(_capi.amd_lib().rt_material_hits(scene._h, _p(records), n, _p(out), _stream_ptr(stream)))
    return out


def material_hits_numpy(scene: Scene, hits_np) -> np.ndarray:
    """Host-buffer convenience (rt_material_hits_host, synchronous): hits as a HIT_DTYPE structured array or an (N, 13) array of 4-byte
    words; returns the surfaces as a SURFACE_DTYPE structured array."""
    a = _host_records(hits_np, HIT_DTYPE, 13, "hits")
    surfaces = np.zeros(a.shape[0], dtype=SURFACE_DTYPE)
    _capi.check(_capi.amd_lib().rt_material_hits_host(scene._h, a.ctypes.data_as(C.c_void_p), a.shape[0], surfaces.ctypes.data_as(C.c_void_p)))
    return surfaces


def probe_surfaces(surfaces, view, light_dirs, out_diffuse=None, out_specular=None, stream=None):
    """get_diffuse and get_specular (src/materials.rs:46-66) of every surface for P directions each (rt_probe_surfaces): ``surfaces``
    (N, 18) int32 (material_hits; a caller may have edited it), ``view`` (N, 3) float32 — what the reference puts into
    probe.view_direction: get_shade passes minus the incoming ray's direction —, ``light_dirs`` (P, N, 3) float32, all CUDA.  Returns
    (diffuse, specular), (P, N, 3) float32 each: no light colour applied, not weighted by shiness, +0 where the surface is not valid.
    It takes no scene: the surface record carries what the probe needs."""
    n = _tensor(surfaces, "surfaces", "int32", (None, SURFACE_WORDS)).shape[0]
    _tensor(view, "view", "float32", (n, 3))
    probes = _tensor(light_dirs, "light_dirs", "float32", (None, n, 3)).shape[0]
    dev = surfaces.device
    out_diffuse = _out_tensor(out_diffuse, (probes, n, 3), "float32", dev, "out_diffuse")
    out_specular = _out_tensor(out_specular, (probes, n, 3), "float32", dev, "out_specular")
    _capi.check(_capi.amd_lib().rt_probe_surfaces(_p(surfaces), n, _p(view), _p(light_dirs), probes, _p(out_diffuse), _p(out_specular),
                                                  _stream_ptr(stream)))
    return out_diffuse, out_specular


def _host_surfaces(a):
    a = np.asarray(a)
    if a.dtype == SURFACE_DTYPE:
        return np.ascontiguousarray(a).reshape(-1)
    if a.ndim == 2 and a.shape[1] == SURFACE_WORDS and a.dtype.itemsize == 4:
        return np.ascontiguousarray(a).view(SURFACE_DTYPE).reshape(-1)
    raise ValueError(f"surfaces: expected a SURFACE_DTYPE array or an (N, {SURFACE_WORDS}) array of 4-byte words")


def probe_surfaces_numpy(surfaces_np, view, light_dirs):
    """Host-buffer convenience (rt_probe_surfaces_host, synchronous): surfaces as a SURFACE_DTYPE structured array or an (N, 18) array
    of 4-byte words, ``view`` (N, 3) and ``light_dirs`` (P, N, 3) float32; returns (diffuse, specular), (P, N, 3) float32 each."""
    a = _host_surfaces(surfaces_np)
    n = a.shape[0]
    view, light_dirs = np.asarray(view), np.asarray(light_dirs)
    if view.dtype != np.float32 or view.shape != (n, 3):
        raise ValueError(f"view: expected an ({n}, 3) float32 array")
    if light_dirs.dtype != np.float32 or light_dirs.ndim != 3 or light_dirs.shape[1:] != (n, 3):
        raise ValueError(f"light_dirs: expected a (P, {n}, 3) float32 array")
    view, light_dirs = np.ascontiguousarray(view), np.ascontiguousarray(light_dirs)
    probes = light_dirs.shape[0]
    diffuse, specular = np.zeros((probes, n, 3), dtype=np.float32), np.zeros((probes, n, 3), dtype=np.float32)
    ptr = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    _capi.check(_capi.amd_lib().rt_probe_surfaces_host(ptr(a), n, ptr(view), ptr(light_dirs), probes, ptr(diffuse), ptr(specular)))
    return diffuse, specular


class PrimarySurfaces(NamedTuple):
    """What primary_surfaces returns: the three record tensors, then named views INTO them (no copies), (rows, cols) or (rows, cols, 3)."""
    rays: object              # (rows * cols, 11) int32 rt_ray records
    hits: object              # (rows * cols, 13) int32 rt_hit records
    surfaces: object          # (rows * cols, 18) int32 rt_surface records
    depth: object             # float32: hit.distance
    position: object          # float32 x 3: hit.at.position
    geometric_normal: object  # float32 x 3: hit.at.normal
    shading_normal: object    # float32 x 3: adjust_normal(hit.at.normal)
    albedo: object            # float32 x 3: approx(hit.at).diffuse_color
    object_index: object      # int32
    valid: object             # int32: 1 where the primary ray hit


def primary_surfaces(scene: Scene, camera: Camera, frame: Frame, stream=None) -> PrimarySurfaces:
    """The first hit of every pixel of a frame or tile and the material there: camera_rays -> cast_rays -> material_hits, three calls on
    ``stream``.  Returns a PrimarySurfaces: (rays, hits, surfaces, depth, position, geometric_normal, shading_normal, albedo,
    object_index, valid) — the planes a denoiser or a compositor asks for, as strided views of the records.  Where ``valid`` is 0 the
    hit record is cast's "no hit" record and the surface planes are +0."""
    torch = _torch()
    rows, cols = frame.rows, frame.cols
    rays = camera_rays(camera, frame, stream=stream)
    hits = cast_rays(scene, rays, stream=stream)
    surfaces = material_hits(scene, hits, stream=stream)
    h = hits.view(rows, cols, 13)
    s = surfaces.view(rows, cols, SURFACE_WORDS)
    return PrimarySurfaces(rays, hits, surfaces, h[..., 12].view(torch.float32), h[..., 3:6].view(torch.float32), h[..., 6:9].view(torch.float32),
                           s[..., 14:17].view(torch.float32), s[..., 3:6].view(torch.float32), h[..., 2], s[..., 17])
