"""Shared test support for rt_trace_rays and the wavefront renderer: kernel variants, one traced call, and the parity checks."""
import contextlib

import numpy as np

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import _capi
import _oracle
from _records import torch_device


@contextlib.contextmanager
def variant(v, budget=None):
    lib = _capi.amd_lib()
    _capi.check(lib.rt_set_variant(v))
    if budget is not None:
        _capi.check(lib.rt_set_wavefront_budget(budget))
    try:
        yield
    finally:
        _capi.check(lib.rt_set_variant(_capi.DEFAULT_VARIANT))
        _capi.check(lib.rt_set_wavefront_budget(6))


def trace(scene, rays, depth, contribution=1.0, **kw):
    torch = torch_device()
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    out = rt.trace_rays(scene, rays, depth, contribution, ray_count=count, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy(), int(count.item())


def assert_same(got, want, what=""):
    g, w = np.asarray(got, dtype=np.float32).reshape(-1, 3), np.asarray(want, dtype=np.float32).reshape(-1, 3)
    same = (g.view(np.uint32) == w.view(np.uint32)) | (np.isnan(g) & np.isnan(w))
    bad = np.argwhere(~same)
    assert same.all(), f"{what}: {len(bad)} channels differ, first {bad[:3].tolist()}: got {g[bad[0][0]]} want {w[bad[0][0]]}"


PWF = 16


def _check(world, cam, frame, budget=None, scene=None, variant=PWF | 2):
    lib = _capi.amd_lib()
    scene = scene or rt.Scene(world)
    _capi.check(lib.rt_set_variant(variant))
    if budget is not None:
        _capi.check(lib.rt_set_wavefront_budget(budget))
    try:
        got, casts = rt.render_whitted_numpy(scene, cam, frame)
    finally:
        _capi.check(lib.rt_set_variant(_capi.DEFAULT_VARIANT))
        _capi.check(lib.rt_set_wavefront_budget(6))
    want, wcasts = _oracle.render_whitted(world.desc(), cam, frame)
    g, w = got.view(np.uint32), want.view(np.uint32)
    same = (g == w) | (np.isnan(got) & np.isnan(want))  # NaN payload/sign may differ between x86 and gfx950
    assert same.all(), f"{(~same).sum()} channels differ; first {np.argwhere(~same)[:3].tolist()}"
    assert casts == wcasts
    return got


def _mismatches(got, want):
    same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))  # as in _check
    return int((~same).sum())
