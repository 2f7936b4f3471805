"""The tree-loop ABI (include/rt_amd.h rt_tree_gate, rt_tree_split, rt_tree_spawn, rt_tree_gather, rt_tree_fold) without a GPU: the
symbols exist and are listed, every status of the documented check order is returned with its message before any device work, an
empty level is RT_OK, and the Python wrappers check their arguments."""
import ctypes as C

import numpy as np
import pytest

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import _capi

NAMES = ("rt_tree_gate", "rt_tree_split", "rt_tree_spawn", "rt_tree_gather", "rt_tree_fold")


def test_tree_symbols_are_exported_and_listed():
    lib = _capi.amd_lib()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in _capi.AMD_SYMBOLS, name
    assert lib.rt_abi_version() == 1  # additive: the version stays
    for name in ("tree_gate", "tree_split", "tree_spawn", "tree_gather", "tree_fold", "trace_rays_levels", "default_level_capacity"):
        assert name in rt.__all__ and callable(getattr(rt, name)), name


def test_arguments_are_checked_before_device_work():
    lib = _capi.amd_lib()
    p = C.c_void_p(16)  # never dereferenced: every call below is refused on its arguments first, or has nothing to do
    fake = C.c_void_p(16)

    def gate(n, scene=None, a=p, b=p):
        return lib.rt_tree_gate(a, n, None, b, p, None)

    def split(n, scene=fake, a=p, b=p):
        return lib.rt_tree_split(scene, a, p, n, None, 1, p, p, b, p, None)

    def spawn(n, scene=None, a=p, b=p):
        return lib.rt_tree_spawn(a, p, n, p, b, None)

    def gather(n, scene=None, a=p, b=p, max_count=8):
        return lib.rt_tree_gather(a, p, max_count, p, p, p, p, n, p, p, p, p, b, None)

    def fold(n, scene=None, a=p, b=p, depth_left=1):
        return lib.rt_tree_fold(a, None, n, depth_left, p, p, p, p, p, None, b, 8, None)

    limits = {gate: 32, split: 32, spawn: 31, gather: 31, fold: 32}
    for fn, log2 in limits.items():
        name = fn.__name__
        # 1. the limit on n: unsupported, named as such, and checked first
        assert fn(1 << log2) == -5 and f"2^{log2}".encode() in lib.rt_last_error(), name
        assert fn((1 << log2) + 7, scene=None, a=None, b=None) == -5, name
        assert fn((1 << log2) - 1, a=None) == -1, name  # just below it: the next checks
        # 2. a null scene
        if fn is split:
            assert fn(2, scene=None) == -1 and b"null scene" in lib.rt_last_error()
            assert fn(2, scene=None, a=None) == -1 and b"null scene" in lib.rt_last_error()
            assert fn(0, scene=None) == -1 and b"null scene" in lib.rt_last_error()  # before the empty level
        # 3. nothing to do: status 0 and no device work
        assert fn(0) == 0, name
        assert fn(0, a=None, b=None) == 0, name
        # 4. a null required pointer with records to work on
        for bad in ({"a": None}, {"b": None}):
            assert fn(2, **bad) == -1 and b"null" in lib.rt_last_error() and b"pointer" in lib.rt_last_error(), (name, bad)
    # rt_tree_gather: the capacity of the child level is limited too, and checked first
    assert gather(2, max_count=1 << 32) == -5 and b"2^32" in lib.rt_last_error()
    assert gather(1 << 31, max_count=1 << 32, a=None) == -5
    assert gather(0, max_count=1 << 32) == -5
    # rt_tree_fold at depth_left <= 0 needs neither weights nor the refraction's outputs nor child values
    assert lib.rt_tree_fold(p, None, 0, 0, p, None, None, None, None, None, p, 8, None) == 0
    assert lib.rt_tree_fold(p, None, 2, 1, p, None, p, p, p, None, p, 8, None) == -1 and b"pointer" in lib.rt_last_error()
    assert lib.rt_tree_fold(p, None, 2, 1, p, p, p, p, None, None, p, 8, None) == -1


def test_default_level_capacity():
    """min(n * 2^L, ceil(f * n)) with the factor DESIGN.md §3.13 derives from the measured level shares: never below 1, a multiple of 0.5"""
    f = rt.LEVEL_CAPACITY_FACTOR
    assert f >= 1.0 and (2 * f) == int(2 * f)
    for n in (1, 7, 1000, 2_073_600):
        assert rt.default_level_capacity(n, 0) == n
        for level in (1, 2, 8, 32):
            assert rt.default_level_capacity(n, level) == min(n << level, int(np.ceil(f * n)))


def test_python_wrappers_check_their_arguments():
    hits, rays = np.zeros((3, 13), dtype=np.int32), np.zeros((3, 11), dtype=np.int32)
    with pytest.raises(ValueError):
        rt.tree_gate(np.zeros(3, dtype=np.float32))  # not CUDA tensors
    with pytest.raises(ValueError):
        rt.tree_split(None, hits, np.zeros(3, dtype=np.float32), 1)
    with pytest.raises(ValueError):
        rt.tree_spawn(hits, np.zeros(3, dtype=np.int32))
    with pytest.raises(ValueError):
        rt.tree_gather(np.zeros(6, dtype=np.int32), None, rays, rays, None, None, None)
    with pytest.raises(ValueError):
        rt.tree_fold(hits, 0, np.zeros((3, 3), dtype=np.float32), np.zeros((3, 3), dtype=np.float32))
    with pytest.raises(ValueError):
        rt.trace_rays_levels(None, rays, 5)
