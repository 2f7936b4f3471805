"""The scatter-query ABI (include/rt_amd.h rt_scatter_hits / rt_scatter_factors and their _host forms) without a GPU: the symbols exist
and are listed, every status of the documented check order is returned with its message before any device work, an empty batch is
RT_OK, the Python wrappers refuse wrong dtypes and shapes before calling down, and without a device the host calls fail with a
status and leave their output buffers untouched.  The generators are an empty rt_rng (rt_rng_create_seeded with n = 0), which is
made without a device."""
import ctypes as C

import numpy as np
import pytest

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import _capi

NAMES = ("rt_scatter_hits", "rt_scatter_factors", "rt_scatter_hits_host", "rt_scatter_factors_host")
OK, INVALID, UNSUPPORTED = 0, -1, -5


@pytest.fixture()
def empty_rng():
    lib = _capi.amd_lib()
    h = C.c_void_p()
    assert lib.rt_rng_create_seeded(None, 0, C.byref(h)) == 0 and h.value
    yield h
    assert lib.rt_rng_destroy(h) == 0


def test_scatter_query_symbols_are_exported_and_listed():
    lib = _capi.amd_lib()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in _capi.AMD_SYMBOLS, name
    assert lib.rt_abi_version() == 1  # additive: the version stays
    header = (_capi.REPO_ROOT / "include" / "rt_amd.h").read_text()
    for name in NAMES:
        assert f"int {name}(" in header, name
    assert "Not covered: scatter_hit and weighted_select" not in header


def test_scatter_hits_arguments_are_checked_before_device_work(empty_rng):
    lib = _capi.amd_lib()
    hits = (_capi.Hit * 2)()
    rays = (_capi.Ray * 2)()
    index = (C.c_uint32 * 2)(0, 1)
    kind = (C.c_uint32 * 2)(9, 9)
    out = (_capi.Ray * 2)()
    cosine = (C.c_float * 2)(7.0, 7.0)
    fake = C.c_void_p(16)  # never dereferenced: every call below is refused on its arguments first, or has nothing to do

    def device(n, scene=fake, rng=empty_rng, h=hits, r=rays, i=index, t=kind, o=out, c=cosine):
        return lib.rt_scatter_hits(scene, h, r, n, rng, i, t, o, c, None)

    def host(n, scene=fake, rng=empty_rng, h=hits, r=rays, i=index, t=kind, o=out, c=cosine):
        return lib.rt_scatter_hits_host(scene, h, r, n, rng, i, t, o, c)

    for fn in (device, host):
        # 1. 2^32 records or more: unsupported, named as such, and checked first
        assert fn(1 << 32) == UNSUPPORTED and b"2^32" in lib.rt_last_error(), fn.__name__
        assert fn((1 << 32) + 7, scene=None, rng=None, h=None, r=None, t=None, o=None) == UNSUPPORTED and b"2^32" in lib.rt_last_error()
        # 2. a null scene, then a null rng
        assert fn(2, scene=None) == INVALID and b"null scene" in lib.rt_last_error(), fn.__name__
        assert fn(2, scene=None, rng=None) == INVALID and b"null scene" in lib.rt_last_error()
        assert fn(0, scene=None) == INVALID and b"null scene" in lib.rt_last_error()  # before the empty batch
        assert fn(2, rng=None) == INVALID and b"null rng" in lib.rt_last_error()
        assert fn(0, rng=None) == INVALID and b"null rng" in lib.rt_last_error()
        assert fn(2, rng=None, i=None, h=None) == INVALID and b"null rng" in lib.rt_last_error()
        # 3. without an index array the count must match (the rng holds none): before the pointers are looked at
        assert fn(2, i=None) == INVALID and b"generators" in lib.rt_last_error(), fn.__name__
        assert fn(2, i=None, h=None, t=None) == INVALID and b"generators" in lib.rt_last_error()
        # 4. nothing to do: status 0 and no device work (the fake scene is never read); identity on an empty rng matches n == 0
        assert fn(0) == OK, fn.__name__
        assert fn(0, i=None) == OK
        assert fn(0, h=None, r=None, t=None, o=None, c=None) == OK
        # 5. a null record pointer or a null required output pointer, with an index array so that n is free
        for bad in ({"h": None}, {"r": None}, {"t": None}, {"o": None}):
            assert fn(2, **bad) == INVALID and b"null" in lib.rt_last_error() and b"pointer" in lib.rt_last_error(), (fn.__name__, bad)
        assert fn(0, c=None) == OK  # the cosine output is optional
    assert all(v == 9 for v in kind) and all(v == 7.0 for v in cosine) and bytes(out) == bytes(C.sizeof(out))


def test_scatter_factors_arguments_are_checked_before_device_work():
    lib = _capi.amd_lib()
    hits = (_capi.Hit * 2)()
    rays = (_capi.Ray * 2)()
    nxt = (_capi.Ray * 2)()
    kind = (C.c_uint32 * 2)()
    travel = (C.c_float * 2)()
    rgb = (C.c_float * 6)(*([7.0] * 6))
    fake = C.c_void_p(16)

    def device(n, scene=fake, h=hits, r=rays, t=kind, x=nxt, d=travel, o=rgb):
        return lib.rt_scatter_factors(scene, h, r, t, x, d, n, o, None)

    def host(n, scene=fake, h=hits, r=rays, t=kind, x=nxt, d=travel, o=rgb):
        return lib.rt_scatter_factors_host(scene, h, r, t, x, d, n, o)

    for fn in (device, host):
        assert fn(1 << 32) == UNSUPPORTED and b"2^32" in lib.rt_last_error(), fn.__name__
        assert fn(1 << 32, scene=None, h=None, o=None) == UNSUPPORTED
        assert fn(2, scene=None) == INVALID and b"null scene" in lib.rt_last_error(), fn.__name__
        assert fn(0, scene=None) == INVALID and b"null scene" in lib.rt_last_error()
        assert fn(0) == OK, fn.__name__
        assert fn(0, h=None, r=None, t=None, x=None, d=None, o=None) == OK
        for bad in ({"h": None}, {"r": None}, {"t": None}, {"x": None}, {"d": None}, {"o": None}):
            assert fn(2, **bad) == INVALID and b"null" in lib.rt_last_error() and b"pointer" in lib.rt_last_error(), (fn.__name__, bad)
    assert all(v == 7.0 for v in rgb)


def test_switch_and_names_are_known():
    lib = _capi.amd_lib()
    for value in (b"0", b"1", None):
        assert lib.rt_set_option(b"RT_AMD_SCATTER_PREPARE", value) == 0
    assert (rt.DIFFUSE, rt.REFLECTION, rt.REFRACTION, rt.HIT_NONE) == (0, 1, 2, -1)
    for name in ("DIFFUSE", "REFLECTION", "REFRACTION", "Scatters", "scatter_hits", "scatter_factors", "scatter_hits_numpy",
                 "scatter_factors_numpy"):
        assert name in rt.__all__, name


def test_alive_is_the_negation_of_the_reference_test():
    """`cosine <= 0` is black in the reference, so NaN goes on; a record that is no hit is never alive"""
    torch = pytest.importorskip("torch")
    s = rt.Scatters(torch.tensor([0, 1, 2, 2, rt.HIT_NONE], dtype=torch.int32), None,
                    torch.tensor([0.5, 0.0, -0.25, float("nan"), 0.0], dtype=torch.float32))
    assert s.alive.tolist() == [True, False, False, True, False] and len(s) == 5


def test_python_wrappers_check_their_arguments():
    h13, r11 = np.zeros((3, 13), dtype=np.int32), np.zeros((3, 11), dtype=np.int32)
    rng = rt.Rng.seeded([])
    try:
        with pytest.raises(ValueError):
            rt.scatter_hits(None, h13, r11, rng)  # not CUDA tensors
        with pytest.raises(ValueError):
            rt.scatter_factors(None, h13, r11, np.zeros(3, dtype=np.int32), r11, np.zeros(3, dtype=np.float32))
        with pytest.raises(ValueError):
            rt.scatter_hits_numpy(None, np.zeros((3, 12), dtype=np.int32), r11, rng, rng_index=np.zeros(3, dtype=np.int32))  # 12 words
        with pytest.raises(ValueError):
            rt.scatter_hits_numpy(None, h13, np.zeros((2, 11), dtype=np.int32), rng, rng_index=np.zeros(3, dtype=np.int32))  # one ray per hit
        with pytest.raises(ValueError):
            rt.scatter_hits_numpy(None, h13, r11, rng)  # identity: 3 records on 0 generators
        with pytest.raises(ValueError):
            rt.scatter_hits_numpy(None, h13, r11, rng, rng_index=np.zeros(3, dtype=np.int64))  # 8-byte indices
        with pytest.raises(ValueError):
            rt.scatter_hits_numpy(None, h13, r11, rng, rng_index=np.zeros(2, dtype=np.int32))
        with pytest.raises(ValueError):
            rt.scatter_hits_numpy(None, h13, r11, "rng", rng_index=np.zeros(3, dtype=np.int32))
        with pytest.raises(ValueError):
            rt.scatter_factors_numpy(None, h13, r11, np.zeros(3, dtype=np.float32), r11, np.zeros(3, dtype=np.float32))  # float types
        with pytest.raises(ValueError):
            rt.scatter_factors_numpy(None, h13, r11, np.zeros(3, dtype=np.int32), r11, np.zeros(3, dtype=np.float64))
        with pytest.raises(ValueError):
            rt.scatter_factors_numpy(None, h13, r11, np.zeros(3, dtype=np.int32), np.zeros((3, 13), dtype=np.int32), np.zeros(3, dtype=np.float32))
    finally:
        rng.close()


def test_no_device_fails_loudly_without_fallback(empty_rng):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present (tests/test_gpu_scatter_queries.py covers the device path)")
    lib = _capi.amd_lib()
    hits = np.zeros(4, dtype=rt.HIT_DTYPE)
    hits["kind"] = 1
    hits["normal"] = (0.0, 1.0, 0.0)
    rays = np.zeros(4, dtype=rt.RAY_DTYPE)
    rays["direction"] = (0.0, -1.0, 0.0)
    index = np.arange(4, dtype=np.uint32)
    kind = np.full(4, 9, dtype=np.uint32)
    out = np.full((4, 11), 3, dtype=np.uint32)
    cosine = np.full(4, 7.0, dtype=np.float32)
    travel = np.zeros(4, dtype=np.float32)
    rgb = np.full((4, 3), 7.0, dtype=np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    # the arguments are fine, so the calls go on to the device, which is not there: a status, nothing computed on the host
    rc = lib.rt_scatter_hits_host(C.c_void_p(16), p(hits), p(rays), 4, empty_rng, p(index), p(kind), p(out), p(cosine))
    assert rc in (-2, -3), rc
    assert (kind == 9).all() and (out == 3).all() and (cosine == 7.0).all()
    rc = lib.rt_scatter_factors_host(C.c_void_p(16), p(hits), p(rays), p(kind), p(out), p(travel), 4, p(rgb))
    assert rc in (-2, -3), rc
    assert (rgb == 7.0).all()
