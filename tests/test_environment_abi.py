"""The environment ABI (include/rt_amd.h rt_environment_lookup, rt_environment_table_bytes, rt_environment_table, rt_environment_rays,
rt_environment_fold; include/rt_environment_host.h rt_environment_*_cpu) without a GPU: the symbols exist and are listed, every status of
the documented check order is returned with its message before any device work, spp and pattern are refused in the hemisphere queries'
words, an empty batch is RT_OK, and the Python wrappers check their arguments."""
import ctypes as C
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import _capi, environment

NAMES = ("rt_environment_lookup", "rt_environment_table_bytes", "rt_environment_table", "rt_environment_rays", "rt_environment_fold")
HOST_NAMES = ("rt_environment_lookup_cpu", "rt_environment_table_cpu", "rt_environment_samples_cpu", "rt_environment_fold_cpu")
CENTER, UNIFORM, STRATIFIED = 0, 1, 2
P = C.c_void_p(16)  # never dereferenced: every call below is refused on its arguments first, or has nothing to do


def desc(width=8, height=4, texels=16, filter=0):
    return _capi.EnvironmentDesc(texels, width, height, 0.0, 1.0, filter)


def test_environment_symbols_are_exported_and_listed():
    lib = _capi.amd_lib()
    for name in NAMES:
        assert hasattr(lib, name) and name in _capi.AMD_SYMBOLS, name
    header = (Path(__file__).resolve().parent.parent / "include" / "rt_environment_host.h").read_text()
    declared = sorted(set(re.findall(r"\b(rt_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S))))
    assert declared == sorted(HOST_NAMES) == sorted(_capi.ENVIRONMENT_HOST_SYMBOLS)
    for name in HOST_NAMES:
        assert hasattr(_capi.host_lib(), name), name
    assert lib.rt_abi_version() == 1  # additive: the version stays
    for name in ("Environment", "lookup", "table", "table_bytes", "rays", "fold", "lookup_numpy", "table_numpy", "samples_numpy", "fold_numpy",
                 "workspace", "Workspace", "sky_hits", "miss_radiance", "trace_rays_levels"):
        assert callable(getattr(environment, name)), name
    assert rt.environment is environment and "environment" not in rt.__all__  # a submodule: the top-level surface gains no name
    assert (environment.NEAREST, environment.BILINEAR) == (0, 1)


def test_the_tree_loop_takes_an_environment():
    """the keyword lives on the submodule's form of the loop: rt.trace_rays_levels keeps the signature the package surface pins"""
    parameters = inspect.signature(environment.trace_rays_levels).parameters
    assert "environment" in parameters and parameters["environment"].default is None
    assert list(parameters)[:-1] == list(inspect.signature(rt.trace_rays_levels).parameters)


def test_table_bytes():
    tb = environment.table_bytes
    assert tb(1, 1) == 24 + 8 + 4 and tb(3, 2) == 24 + 16 + 24 and tb(16384, 8191) == 24 + 8 * 8191 + 4 * 16384 * 8191
    assert tb(0, 4) == 0 and tb(4, 0) == 0 and tb(16385, 1) == 0 and tb(1, 8193) == 0 and tb(16384, 8192) == 0  # 2^27 texels


def the_calls():
    lib = _capi.amd_lib()

    def lookup(n, env=desc(), a=P, b=P, **_):
        return lib.rt_environment_lookup(C.byref(env) if env is not None else None, a, n, None, None, None, b, n, None)

    def rays(n, env=desc(), a=P, b=P, spp=1, pattern=UNIFORM, kind=0, scene=P, table=P):
        return lib.rt_environment_rays(scene, C.byref(env) if env is not None else None, table, a, n, None, spp, pattern, 0, kind, b, P, P, P, None, None)

    def fold(n, a=P, b=P, spp=1, scene=P, **_):
        return lib.rt_environment_fold(scene, a, n, spp, b, None, P, P, P, None, P, None)

    return lib, lookup, rays, fold


def test_arguments_are_checked_before_device_work():
    lib, lookup, rays, fold = the_calls()
    err = lib.rt_last_error
    for fn in (lookup, rays, fold):
        name = fn.__name__
        # 1. the count, first
        assert fn(1 << 32) == -5 and b"2^32" in err(), name
        assert fn(1 << 32, env=None, a=None) == -5 and b"2^32" in err(), name
        # 4. nothing to do; 5. a null required pointer
        assert fn(0) == 0 and fn(0, a=None, b=None) == 0, name
        for bad in ({"a": None}, {"b": None}):
            assert fn(2, **bad) == -1 and b"null" in err() and b"pointer" in err(), (name, bad)
    for fn in (rays, fold):
        name = fn.__name__
        assert fn(1 << 26, spp=64) == -5 and b"2^32" in err(), name  # n * spp
        assert fn(2, scene=None) == -1 and b"null scene" in err(), name
        assert fn(0, scene=None) == -1 and b"null scene" in err(), name  # before the empty batch
        assert fn(0, spp=0) == 0 and fn(0, spp=65) == 0, name
        assert fn(2, spp=0, a=None) == -1 and b"pointer" in err(), name  # the pointers before spp
        for spp in (0, 65, 1 << 20):
            assert fn(2, spp=spp) == -1 and b"1 .. 64" in err(), (name, spp)
    # 3. the descriptor, after the scene and before the empty batch
    for fn in (lookup, rays):
        name = fn.__name__
        assert fn(2, env=None) == -1 and b"null environment" in err(), name
        assert fn(0, env=None) == -1 and b"null environment" in err(), name
        assert fn(2, env=desc(texels=None)) == -1 and b"null environment texels" in err(), name
        assert fn(2, env=desc(width=0)) == -1 and b"width or height 0" in err(), name
        assert fn(2, env=desc(height=0)) == -1 and b"width or height 0" in err(), name
        for over in (desc(width=16385, height=1), desc(width=1, height=8193), desc(width=16384, height=8192)):
            assert fn(2, env=over) == -5 and b"16384" in err() and b"8192" in err() and b"2^27" in err(), name
        assert fn(2, env=desc(filter=2)) == -1 and b"unknown filter" in err() and b"RT_ENV_BILINEAR" in err(), name
        assert fn(0, env=desc(filter=2)) == -1, name
        assert fn(2, env=desc(filter=2), a=None) == -1 and b"unknown filter" in err(), name  # before the pointers
    assert rays(2, scene=None, env=None) == -1 and b"null scene" in err()  # the scene before the descriptor
    assert rays(2, table=None) == -1 and b"pointer" in err()
    # the sampler's words are the hemisphere queries'
    hemi = lambda spp, pattern, kind=0: lib.rt_hemisphere_rays(P, P, 2, None, spp, pattern, 0, kind, P, P, P, None)
    for spp, pattern, kind in ((4, CENTER, 0), (4, 3, 0), (5, STRATIFIED, 0), (0, CENTER, 0), (65, UNIFORM, 0), (4, UNIFORM, 2), (4, CENTER, 2)):
        assert rays(2, spp=spp, pattern=pattern, kind=kind) == -1
        mine = err().decode()
        assert hemi(spp, pattern, kind) == -1
        assert mine.split(": ", 1)[1] == err().decode().split(": ", 1)[1] and mine.startswith("rt_environment_rays: ")
    assert rays(0, spp=5, pattern=STRATIFIED) == 0 and rays(0, pattern=CENTER) == 0 and rays(0, kind=7) == 0


def test_the_table_call_checks_its_arguments():
    lib = _capi.amd_lib()
    err = lib.rt_last_error
    table = lambda env=desc(), t=P: lib.rt_environment_table(C.byref(env) if env is not None else None, t, None)
    assert table(env=None) == -1 and b"null environment" in err()
    assert table(desc(texels=None)) == -1 and b"texels" in err()
    assert table(desc(width=0)) == -1 and table(desc(height=0)) == -1
    assert table(desc(width=16385)) == -5 and table(desc(height=8193)) == -5 and b"2^27" in err()
    assert table(desc(filter=5)) == -1 and b"unknown filter" in err()
    assert table(t=None) == -1 and b"null table pointer" in err()
    assert table(t=C.c_void_p(20)) == -1 and b"8-byte aligned" in err()


def test_the_cpu_forms_check_their_arguments():
    lib = _capi.host_lib()
    err = lib.rt_host_last_error
    img = np.ones((4, 8, 3), dtype=np.float32)
    env = desc(texels=img.ctypes.data)
    table = environment.table_numpy(img)
    tp = table.ctypes.data_as(C.c_void_p)
    rays, out = (C.c_uint32 * 44)(), (C.c_float * 12)()
    lookup = lambda n=4, e=env, r=rays, o=out: lib.rt_environment_lookup_cpu(C.byref(e) if e is not None else None, r, n, None, None, None, o, 4)
    assert lookup() == 0
    assert lookup(n=1 << 32) == -5 and b"2^32" in err()
    assert lookup(e=None) == -1 and b"null environment" in err()
    assert lookup(n=0, e=None) == -1 and lookup(n=0, r=None, o=None) == 0
    assert lookup(e=desc(texels=img.ctypes.data, width=0)) == -1 and b"width or height 0" in err()
    assert lookup(e=desc(texels=img.ctypes.data, width=16385)) == -5
    assert lookup(e=desc(texels=img.ctypes.data, filter=2)) == -1 and b"unknown filter" in err()
    assert lookup(r=None) == -1 and lookup(o=None) == -1 and b"pointer" in err()
    assert lib.rt_environment_table_cpu(None, tp) == -1 and lib.rt_environment_table_cpu(C.byref(env), None) == -1 and b"null table pointer" in err()
    assert lib.rt_environment_table_cpu(C.byref(env), C.c_void_p(table.ctypes.data + 4)) == -1 and b"8-byte aligned" in err()
    normals, dirs, radiance = (C.c_float * 12)(*([0.0, 1.0, 0.0] * 4)), (C.c_float * (3 * 64 * 4))(), (C.c_float * (3 * 64 * 4))()
    samples = lambda n=4, spp=1, pattern=UNIFORM, e=env, t=tp, a=normals, d=dirs: lib.rt_environment_samples_cpu(C.byref(e) if e is not None else None, t, a, None,
                                                                                                            n, spp, pattern, 7, d, radiance, None, None)
    assert samples() == 0 and samples(spp=64, pattern=STRATIFIED) == 0
    assert samples(n=1 << 26, spp=64, a=None) == -5 and b"2^32" in err()
    assert samples(e=None) == -1 and samples(n=0, a=None, d=None) == 0
    assert samples(t=None) == -1 and samples(a=None) == -1 and samples(d=None) == -1 and b"pointer" in err()
    for spp in (0, 65):
        assert samples(spp=spp) == -1 and b"1 .. 64" in err()
    assert samples(pattern=CENTER) == -1 and b"RT_FILM_CENTER" in err()
    assert samples(spp=5, pattern=STRATIFIED) == -1 and b"k * k" in err()
    valid, shiness, asks, f24, rgb = (C.c_ubyte * 4)(), (C.c_float * 4)(), (C.c_ubyte * 8)(), (C.c_float * 24)(), (C.c_float * 12)()
    fold = lambda n=4, spp=2, v=valid, a=asks, out=rgb: lib.rt_environment_fold_cpu(v, shiness, n, spp, a, None, f24, f24, f24, None, out)
    assert fold() == 0 and fold(n=0, spp=0, v=None) == 0
    assert fold(n=1 << 31, spp=2, v=None) == -5 and b"2^32" in err()
    assert fold(v=None) == -1 and fold(a=None) == -1 and fold(out=None) == -1 and b"pointer" in err()
    assert fold(spp=0) == -1 and b"1 .. 64" in err()
    with pytest.raises(rt.RtError):
        environment.samples_numpy(img, table, np.zeros((4, 3), dtype=np.float32), 5, STRATIFIED)
    with pytest.raises(rt.RtError):
        environment.lookup_numpy(img, np.zeros((2, 3), dtype=np.float32), filter=7)
    with pytest.raises(ValueError):
        environment.samples_numpy(img, table[:-4], np.zeros((4, 3), dtype=np.float32), 4)
    with pytest.raises(ValueError):
        environment.table_numpy(np.zeros((4, 8), dtype=np.float32))
    with pytest.raises(ValueError):
        environment.fold_numpy(np.ones(4), np.zeros(4), np.zeros(7), 2, np.zeros((8, 3)), np.zeros((8, 3)), np.zeros((8, 3)), np.zeros((4, 3)))


def test_python_wrappers_check_their_arguments():
    hits = np.zeros((3, 13), dtype=np.int32)
    with pytest.raises(ValueError):
        environment.Environment(np.zeros((4, 8, 3), dtype=np.float32))  # not a CUDA tensor
    with pytest.raises(ValueError):
        environment.lookup(None, hits)
    with pytest.raises(ValueError):
        environment.table(None)
    with pytest.raises(ValueError):
        environment.sky_hits(None, None, hits, hits, 4)
    with pytest.raises(ValueError):
        environment.miss_radiance(None, None, hits)
    with pytest.raises(ValueError):
        environment.workspace(-1, "cpu", 4)
    torch = pytest.importorskip("torch")
    with pytest.raises(ValueError):
        environment.Environment(torch.zeros((4, 8, 3), dtype=torch.float32))  # a CPU tensor
    with pytest.raises(ValueError):
        environment.trace_rays_levels(None, torch.zeros((3, 11), dtype=torch.int32), 1, environment="sky")
