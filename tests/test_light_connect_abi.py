"""The light-connection ABI (include/rt_amd.h rt_path_connect_lights, rt_path_settle_lights; include/rt_light_connect_host.h their CPU
forms): exported and listed, declared as ctypes calls them, every documented status with its message in the documented order, an empty
batch RT_OK, and the Python wrappers' own checks.  No GPU: every device call below is refused on its arguments or has nothing to do."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import _capi, paths
import _light_connect_support as LC

ROOT = Path(__file__).resolve().parent.parent
INCLUDE = ROOT / "include"
NAMES = ("rt_path_connect_lights", "rt_path_settle_lights")
HOST_NAMES = ("rt_path_connect_lights_cpu", "rt_path_settle_lights_cpu")
P = C.c_void_p(16)  # never dereferenced: every call below is refused on its arguments first, or has nothing to do
F32 = np.float32


def declaration(header, name):
    text = re.sub(r"/\*.*?\*/", "", (INCLUDE / header).read_text(), flags=re.S)
    found = re.findall(rf"\bint\s+{name}\s*\(([^)]*)\)\s*;", text)
    assert len(found) == 1, name
    return [" ".join(p.split()) for p in found[0].split(",")]


def ctype_of(parameter):
    if "*" in parameter:
        return C.c_void_p
    return {"size_t": C.c_size_t, "uint32_t": C.c_uint32, "int": C.c_int, "float": C.c_float}[parameter.split()[0]]


def test_the_symbols_are_exported_and_listed():
    lib, host = _capi.amd_lib(), _capi.host_lib()
    for name in NAMES:
        assert hasattr(lib, name) and name in _capi.AMD_SYMBOLS and not hasattr(host, name), name
    header = (INCLUDE / "rt_light_connect_host.h").read_text()
    declared = sorted(set(re.findall(r"\b(rt_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S))))
    assert declared == sorted(HOST_NAMES) == sorted(_capi.LIGHT_CONNECT_HOST_SYMBOLS)
    for name in HOST_NAMES:
        assert hasattr(host, name) and not hasattr(lib, name), name
    assert '#include "rt_light_connect_host.h"' in (INCLUDE / "rt_host.h").read_text()
    assert lib.rt_abi_version() == 1  # additive: the version stays
    for name in ("connect_lights", "settle_lights", "connect_lights_numpy", "settle_lights_numpy", "light_seed"):
        assert callable(getattr(paths, name)), name
    text = (INCLUDE / "rt_amd.h").read_text()
    assert text.index("---- connection queries:") < text.index("---- light-connection queries:") < text.index("---- distributed (stochastic")
    block = text[text.index("---- light-connection queries:"):text.index("---- distributed (stochastic")]
    for word in ("rt_path_connect_lights(list_b)", "rt_path_settle_lights(that list)", "0x2545f491u", "0x68e31da4u", "No multiple\n * importance sampling"):
        assert word in block, word
    for word in ("more than one light sample", "geometry", "_host\n * and rt_multi_*", "rt_render_*"):
        assert word in block[block.index("Not covered:"):], word
    # the two new constants are no stream another block draws from
    shared = (ROOT / "homework-18-graphics-raytracer_amd" / "csrc" / "rt_light_connect.h").read_text()
    new = {int(v, 16) for v in re.findall(r"#define RT_LIGHT_CONNECT_(?:CHOICE|POINT)_STREAM (0x[0-9a-f]{8})u", shared)}
    assert new == {0x2545F491, 0x68E31DA4} and not new & {0xC2B2AE35, 0x85EBCA6B, 0x165667B1, 0x27D4EB2F}
    assert paths.light_seed(0, 0) == int(LC.S.film_mix(np.uint32(0x68E31DA4)))
    assert paths.light_seed(5, 2) == int(LC.S.film_mix(np.uint32((5 + 2 * 0x9E3779B9) & 0xFFFFFFFF) ^ np.uint32(0x68E31DA4)))


def test_the_declared_signatures_match_the_ctypes():
    assert declaration("rt_amd.h", "rt_path_connect_lights") == [
        "const rt_scene *scene", "const rt_path *d_paths", "size_t m", "const uint32_t *d_index", "const uint32_t *d_count", "const rt_hit *d_hits",
        "const rt_ray *d_incoming", "uint32_t light_first", "uint32_t light_count", "const float *d_radii", "const float *d_weights", "uint32_t seed",
        "rt_ray *d_shadow_rays", "unsigned char *d_asks", "float *d_pending", "float *d_reach", "uint32_t *d_chosen", "void *hip_stream"]
    assert declaration("rt_amd.h", "rt_path_settle_lights") == [
        "const rt_path *d_paths", "size_t m", "const uint32_t *d_index", "const uint32_t *d_count", "unsigned char *d_asks", "const rt_ray *d_shadow_rays",
        "const rt_hit *d_shadow_hits", "const float *d_reach", "const float *d_pending", "float *d_radiance", "void *hip_stream"]
    lib, host = _capi.amd_lib(), _capi.host_lib()
    for header, library, name in (("rt_amd.h", lib, NAMES[0]), ("rt_amd.h", lib, NAMES[1]), ("rt_light_connect_host.h", host, HOST_NAMES[0]),
                                  ("rt_light_connect_host.h", host, HOST_NAMES[1])):
        assert [ctype_of(p) for p in declaration(header, name)] == list(getattr(library, name).argtypes), name
    assert len(host.rt_path_connect_lights_cpu.argtypes) == 19 and len(host.rt_path_settle_lights_cpu.argtypes) == 10


def test_connect_lights_checks_in_connects_order_then_the_lights():
    lib = _capi.amd_lib()
    err = lib.rt_last_error

    def connect(m, scene=P, paths_=P, index=None, count=None, hits=P, incoming=P, first=0, lights=1, radii=None, weights=None, rays=P, asks=P, pending=P,
                reach=P, chosen=None):
        return lib.rt_path_connect_lights(scene, paths_, m, index, count, hits, incoming, first, lights, radii, weights, 0, rays, asks, pending, reach, chosen, None)

    assert connect(1 << 32) == -5 and b"2^32" in err() and err().startswith(b"rt_path_connect_lights: ")
    assert connect(1 << 32, scene=None, hits=None) == -5 and b"2^32" in err()  # the count, first
    assert connect(2, scene=None) == -1 and b"null scene" in err()
    assert connect(0, scene=None) == -1 and b"null scene" in err()  # before the empty batch
    assert connect(0) == 0 and connect(0, paths_=None, hits=None, rays=None) == 0  # m == 0: RT_OK, nothing launched
    assert connect(2, lights=0) == 0 and connect(2, lights=0, paths_=None, hits=None, first=99) == 0  # no lights: RT_OK, nothing launched
    for bad in ({"paths_": None}, {"hits": None}, {"incoming": None}, {"rays": None}, {"asks": None}, {"pending": None}, {"reach": None}, {"index": P}):
        assert connect(2, **bad) == -1 and b"null" in err() and b"pointer" in err() and b"incoming-ray" in err() and b"reach" in err(), bad
    # rt_path_connect's words for what the two calls share
    mine = err().decode()
    env = _capi.EnvironmentDesc(16, 16, 8, 0.0, 1.0, 0)
    assert lib.rt_path_connect(P, C.byref(env), P, P, 2, P, None, P, P, 0, 0, 0, 0, P, P, P, None) == -1
    assert "path, count (with an index), hit, incoming-ray, ray, flag" in mine and "path, count (with an index), hit, incoming-ray, ray, flag" in err().decode()
    assert connect(2, paths_=C.c_void_p(8)) == -1 and b"16-byte aligned" in err()
    assert connect(2, paths_=None, first=1 << 31, lights=1 << 31) == -1 and b"pointer" in err()  # the pointers before the lights


def test_settle_lights_checks_its_arguments():
    lib = _capi.amd_lib()
    err = lib.rt_last_error

    def settle(m, paths_=P, index=None, count=None, asks=P, rays=P, shadow=P, reach=P, pending=P, radiance=P):
        return lib.rt_path_settle_lights(paths_, m, index, count, asks, rays, shadow, reach, pending, radiance, None)

    assert settle(1 << 32) == -5 and b"2^32" in err() and err().startswith(b"rt_path_settle_lights: ")
    assert settle(0) == 0 and settle(0, paths_=None, asks=None, rays=None, reach=None, pending=None, radiance=None) == 0
    for bad in ({"paths_": None}, {"asks": None}, {"rays": None}, {"reach": None}, {"pending": None}, {"radiance": None}, {"index": P}):
        assert settle(2, **bad) == -1 and b"null" in err() and b"pointer" in err() and b"pending" in err(), bad
    assert settle(2, paths_=C.c_void_p(8)) == -1 and b"16-byte aligned" in err()
    assert settle(2, paths_=C.c_void_p(8), shadow=None) == -1 and b"16-byte aligned" in err()  # d_shadow_hits may be NULL


def test_the_cpu_forms_check_their_arguments():
    lib = _capi.host_lib()
    err = lib.rt_host_last_error
    n = 4
    surfaces, positions, view = LC.floor(n)
    lights = LC.three_lights()
    arr = (_capi.Light * 3)(*lights)
    records = LC.records(n)
    f, b, u = (C.c_float * 64)(), (C.c_ubyte * 8)(), (C.c_uint32 * 8)()
    sp, pp, vp, rp = (a.ctypes.data_as(C.c_void_p) for a in (surfaces, positions, view, records))
    lp = C.cast(arr, C.c_void_p)
    connect = lambda m=n, s=sp, p=pp, v=vp, l=lp, r=rp, count=3, reach=f: lib.rt_path_connect_lights_cpu(s, p, v, l, None, r, m, None, None, 0, count, None, None,
                                                                                                         1, f, b, f, reach, u)
    assert connect(m=1 << 32) == -5 and b"2^32" in err() and err().startswith(b"rt_path_connect_lights_cpu: ")
    assert connect(m=0, s=None, r=None) == 0 and connect(count=0, s=None, l=None) == 0
    for bad in ({"s": None}, {"p": None}, {"v": None}, {"l": None}, {"r": None}, {"reach": None}):
        assert connect(**bad) == -1 and b"pointer" in err(), bad
    assert connect() == 0
    settle = lambda m=n, r=rp, a=b, rays=f, reach=f: lib.rt_path_settle_lights_cpu(r, m, None, None, a, rays, None, reach, f, f)
    assert settle(m=1 << 32) == -5 and settle(m=0, r=None, a=None) == 0
    for bad in ({"r": None}, {"a": None}, {"rays": None}, {"reach": None}):
        assert settle(**bad) == -1 and b"pointer" in err(), bad
    with pytest.raises(ValueError):
        paths.connect_lights_numpy(surfaces, positions, view, lights, records[:3])
    with pytest.raises(ValueError, match="lights"):
        paths.connect_lights_numpy(surfaces, positions, view, lights, records, light_first=2, light_count=2)
    with pytest.raises(ValueError):
        paths.connect_lights_numpy(surfaces, positions, view, lights, records, weights=np.ones(2, F32))
    with pytest.raises(ValueError):
        paths.settle_lights_numpy(np.zeros(n, np.uint8), np.zeros((n, 11), np.uint32), np.zeros(n + 1, F32), np.zeros((n, 3), F32), np.zeros((n, 3), F32))


def test_python_wrappers_check_their_arguments():
    hits = np.zeros((3, 13), dtype=np.int32)
    with pytest.raises(ValueError):
        paths.connect_lights(None, hits, hits, hits)  # not CUDA tensors
    with pytest.raises(ValueError):
        paths.settle_lights(hits, hits, hits, hits, hits, hits)
    with pytest.raises(ValueError):
        paths.trace_paths(None, hits, hits, 4, 2, light_nee=True)
    with pytest.raises(ValueError):
        paths.workspace(-1, "cpu", 4, light_nee=True)
    w = paths.workspace(3, "cpu", 2, light_nee=True, chosen=True)
    assert w.light_connections == 6 and w.light_chosen.shape == (6,) and not w.light_asks.any() and w.connections == 0
    for name, per_path in (("light_shadow_rays", 44), ("light_shadow_hits", 52), ("light_asks", 1), ("light_pending", 12), ("light_reach", 4),
                           ("light_ask_index", 4), ("light_chosen", 4)):
        t = getattr(w, name)
        assert t.numel() * t.element_size() == 6 * per_path, name
    assert paths.workspace(3, "cpu", 2).light_connections == 0
