"""The connection ABI (include/rt_amd.h rt_path_connect, rt_path_settle, rt_path_weigh_escape; include/rt_connect_host.h their CPU forms)
without a GPU: the symbols exist with the declared signatures and are listed, every status of the documented check order is returned
with its message before any device work — rt_path_advance's order and words, the descriptor as rt_environment_rays checks it, then the
heuristic in rt_mis_weigh's words — an empty batch is RT_OK, a table whose header names another size reads as a sky without light, and
the Python wrappers check their arguments."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import _capi, environment as E, lobes, paths
import _connect_support as CS
import _lobe_support as S
import _path_support as PS

ROOT = Path(__file__).resolve().parent.parent
INCLUDE = ROOT / "include"
NAMES = ("rt_path_connect", "rt_path_settle", "rt_path_weigh_escape")
HOST_NAMES = ("rt_path_connect_cpu", "rt_path_settle_cpu", "rt_path_weigh_escape_cpu")
P = C.c_void_p(16)  # never dereferenced: every call below is refused on its arguments first, or has nothing to do
F32 = np.float32


def env_desc(width=16, height=8, texels=16, filter=0):
    return _capi.EnvironmentDesc(texels, width, height, 0.0, 1.0, filter)


def declaration(header, name):
    text = re.sub(r"/\*.*?\*/", "", (INCLUDE / header).read_text(), flags=re.S)
    found = re.findall(rf"\bint\s+{name}\s*\(([^)]*)\)\s*;", text)
    assert len(found) == 1, name
    return [" ".join(p.split()) for p in found[0].split(",")]


def test_connection_symbols_are_exported_and_listed():
    lib, host = _capi.amd_lib(), _capi.host_lib()
    for name in NAMES:
        assert hasattr(lib, name) and name in _capi.AMD_SYMBOLS and not hasattr(host, name), name
    header = (INCLUDE / "rt_connect_host.h").read_text()
    declared = sorted(set(re.findall(r"\b(rt_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S))))
    assert declared == sorted(HOST_NAMES) == sorted(_capi.CONNECT_HOST_SYMBOLS)
    for name in HOST_NAMES:
        assert hasattr(host, name) and not hasattr(lib, name), name
    assert '#include "rt_connect_host.h"' in (INCLUDE / "rt_host.h").read_text()
    assert lib.rt_abi_version() == 1  # additive: the version stays
    for name in ("connect", "settle", "weigh_escape", "connect_numpy", "settle_numpy", "weigh_escape_numpy"):
        assert callable(getattr(paths, name)), name
    assert (paths.BALANCE, paths.POWER) == (lobes.BALANCE, lobes.POWER) == (0, 1)
    text = (INCLUDE / "rt_amd.h").read_text()
    block = text[text.index("---- connection queries:"):text.index("---- distributed (stochastic")]
    assert text.index("---- transmission queries:") < text.index("---- connection queries:")
    for word in ("rt_path_weigh_escape(list_b)", "rt_path_connect(list_b, last)", "rt_path_settle(that list)", "0xc2b2ae35u", "0x85ebca6bu"):
        assert word in block, word
    for word in ("area-light", "more than one", "through glass", "_host and rt_multi_*", "rt_render_*", "rt_path_advance's"):
        assert word in block[block.index("Not covered:"):], word


def test_the_declared_signatures():
    assert declaration("rt_amd.h", "rt_path_connect") == [
        "const rt_scene *scene", "const rt_environment *env", "const void *d_table", "const rt_path *d_paths", "size_t m", "const uint32_t *d_index",
        "const uint32_t *d_count", "const rt_hit *d_hits", "const rt_ray *d_incoming", "uint32_t seed", "uint32_t normal_kind", "uint32_t heuristic", "int last",
        "rt_ray *d_shadow_rays", "unsigned char *d_asks", "float *d_pending", "void *hip_stream"]
    assert declaration("rt_amd.h", "rt_path_settle") == [
        "const rt_path *d_paths", "size_t m", "const uint32_t *d_index", "const uint32_t *d_count", "unsigned char *d_asks", "const rt_hit *d_shadow_hits",
        "const float *d_pending", "float *d_radiance", "void *hip_stream"]
    assert declaration("rt_amd.h", "rt_path_weigh_escape") == [
        "const rt_environment *env", "const void *d_table", "const rt_path *d_paths", "size_t m", "const uint32_t *d_index", "const uint32_t *d_count",
        "const rt_hit *d_hits", "const rt_ray *d_incoming", "uint32_t heuristic", "float *d_emitted", "void *hip_stream"]
    lib, host = _capi.amd_lib(), _capi.host_lib()
    assert len(lib.rt_path_connect.argtypes) == 17 and len(lib.rt_path_settle.argtypes) == 9 and len(lib.rt_path_weigh_escape.argtypes) == 11
    assert len(declaration("rt_connect_host.h", "rt_path_connect_cpu")) == 15 == len(host.rt_path_connect_cpu.argtypes)
    assert len(declaration("rt_connect_host.h", "rt_path_settle_cpu")) == 8 == len(host.rt_path_settle_cpu.argtypes)
    assert len(declaration("rt_connect_host.h", "rt_path_weigh_escape_cpu")) == 10 == len(host.rt_path_weigh_escape_cpu.argtypes)


def test_connect_checks_in_advance_order_then_the_heuristic():
    lib = _capi.amd_lib()
    err = lib.rt_last_error
    good = env_desc()

    def connect(m, scene=P, env=good, table=P, paths_=P, index=None, count=None, hits=P, incoming=P, kind=0, heuristic=0, rays=P, asks=P, pending=P):
        return lib.rt_path_connect(scene, None if env is None else C.byref(env), table, paths_, m, index, count, hits, incoming, 0, kind, heuristic, 0, rays, asks,
                                   pending, None)

    assert connect(1 << 32) == -5 and b"2^32" in err() and err().startswith(b"rt_path_connect: ")
    assert connect(1 << 32, scene=None, env=None, hits=None, heuristic=9) == -5 and b"2^32" in err()  # the count, first
    assert connect(2, scene=None) == -1 and b"null scene" in err()
    assert connect(0, scene=None) == -1 and b"null scene" in err()  # before the empty batch
    assert connect(2, env=None) == -1 and b"null environment" in err()
    assert connect(0, env=env_desc(width=0)) == -1 and b"width or height 0" in err()  # the descriptor before the empty batch
    assert connect(2, env=env_desc(width=1 << 15)) == -5 and b"16384" in err()
    assert connect(2, env=env_desc(filter=5)) == -1 and b"unknown filter" in err()
    assert connect(0) == 0 and connect(0, paths_=None, table=None, hits=None, kind=7, heuristic=7) == 0  # m == 0: RT_OK, nothing launched
    for bad in ({"table": None}, {"paths_": None}, {"hits": None}, {"incoming": None}, {"rays": None}, {"asks": None}, {"pending": None}, {"index": P}):
        assert connect(2, **bad) == -1 and b"null" in err() and b"pointer" in err() and b"incoming-ray" in err(), bad
    assert connect(2, hits=None, kind=2, heuristic=2) == -1 and b"pointer" in err()  # the pointers before the limits
    # the normal_kind in rt_path_advance's words, before the heuristic; the heuristic in rt_mis_weigh's
    assert connect(2, kind=2, heuristic=2) == -1
    mine = err().decode()
    assert lib.rt_path_advance(P, P, 2, None, None, P, P, None, 0, 2, 3, 0.05, 0, P, P, P, None) == -1
    assert mine.split(": ", 1)[1] == err().decode().split(": ", 1)[1] and b"unknown normal_kind" in err()
    assert connect(2, heuristic=2) == -1
    mine = err().decode()
    assert lib.rt_mis_weigh(2, P, 1, P, 1, 2, 0, P, None, None) == -1
    assert mine.split(": ", 1)[1] == err().decode().split(": ", 1)[1] and b"unknown heuristic" in err()
    assert connect(2, paths_=C.c_void_p(8)) == -1 and b"16-byte aligned" in err()  # after everything else
    assert connect(2, table=C.c_void_p(12)) == -1 and b"8-byte aligned" in err()
    assert connect(2, paths_=C.c_void_p(8), heuristic=3) == -1 and b"heuristic" in err()


def test_settle_and_weigh_escape_check_their_arguments():
    lib = _capi.amd_lib()
    err = lib.rt_last_error
    good = env_desc()

    def settle(m, paths_=P, index=None, count=None, asks=P, shadow=P, pending=P, radiance=P):
        return lib.rt_path_settle(paths_, m, index, count, asks, shadow, pending, radiance, None)

    assert settle(1 << 32) == -5 and b"2^32" in err() and err().startswith(b"rt_path_settle: ")
    assert settle(0) == 0 and settle(0, paths_=None, asks=None, pending=None, radiance=None) == 0
    for bad in ({"paths_": None}, {"asks": None}, {"pending": None}, {"radiance": None}, {"index": P}):
        assert settle(2, **bad) == -1 and b"null" in err() and b"pointer" in err() and b"pending" in err(), bad
    assert settle(2, paths_=C.c_void_p(8)) == -1 and b"16-byte aligned" in err()

    def weigh(m, env=good, table=P, paths_=P, index=None, count=None, hits=P, incoming=P, heuristic=0, emitted=P):
        return lib.rt_path_weigh_escape(None if env is None else C.byref(env), table, paths_, m, index, count, hits, incoming, heuristic, emitted, None)

    assert weigh(1 << 32) == -5 and b"2^32" in err() and err().startswith(b"rt_path_weigh_escape: ")
    assert weigh(1 << 32, env=None, heuristic=9) == -5
    assert weigh(2, env=None) == -1 and b"null environment" in err() and weigh(0, env=None) == -1
    assert weigh(2, env=env_desc(texels=None)) == -1 and b"null environment texels" in err()
    assert weigh(0) == 0 and weigh(0, table=None, paths_=None, hits=None, heuristic=9) == 0
    for bad in ({"table": None}, {"paths_": None}, {"hits": None}, {"incoming": None}, {"emitted": None}, {"index": P}):
        assert weigh(2, **bad) == -1 and b"null" in err() and b"pointer" in err() and b"emitted" in err(), bad
    assert weigh(2, emitted=None, heuristic=2) == -1 and b"pointer" in err()  # the pointers before the heuristic
    assert weigh(2, heuristic=2) == -1 and b"unknown heuristic" in err()
    assert weigh(2, paths_=C.c_void_p(8)) == -1 and b"16-byte aligned" in err()
    assert weigh(2, table=C.c_void_p(20)) == -1 and b"8-byte aligned" in err()


def test_the_cpu_forms_check_their_arguments_and_a_table_of_another_size_is_no_table():
    lib = _capi.host_lib()
    err = lib.rt_host_last_error
    n = 4
    surfaces = S.flat_surfaces(n, (0.0, 0.0, 1.0), 0.3, 0.5)
    view = np.tile(np.array([0.3, 0.1, 0.9], dtype=F32), (n, 1))
    img = CS.sun_sky()
    table = E.table_numpy(img)
    records = PS.records(n)
    assert paths.connect_numpy(surfaces, view, img, table, records)[1].any()
    with pytest.raises(rt.RtError, match="unknown heuristic"):
        paths.connect_numpy(surfaces, view, img, table, records, heuristic=2)
    with pytest.raises(rt.RtError, match="unknown heuristic"):
        paths.weigh_escape_numpy(img, table, records, CS.no_hits(n), CS.direction_rays(view), np.ones((n, 3), F32), heuristic=7)
    with pytest.raises(ValueError):
        paths.connect_numpy(surfaces, view, img, table, records[:3])
    with pytest.raises(ValueError):
        paths.connect_numpy(surfaces, view, img, table[:-4], records)
    with pytest.raises(ValueError):
        paths.settle_numpy(np.zeros(n, np.uint8), np.zeros((n + 1, 3), F32), np.zeros((n, 3), F32))
    # a table whose header names another size: a sky without light, as in rt_environment_pdf — nothing asks, nothing is weighed
    other = table.copy()
    other[:4] = np.array([CS.WIDTH + 1], dtype=np.uint32).view(np.uint8)
    dirs, asks, _ = paths.connect_numpy(surfaces, view, img, other, records)
    assert not asks.any() and not dirs.any()
    lobe = PS.records(n)
    lobe["pdf"] = 0.5
    emitted = np.full((n, 3), 2.0, dtype=F32)
    S.assert_same(paths.weigh_escape_numpy(img, other, lobe, CS.no_hits(n), CS.direction_rays(view), emitted), emitted, "another size weighs nothing")
    assert (paths.weigh_escape_numpy(img, table, lobe, CS.no_hits(n), CS.direction_rays(view), emitted) < emitted).all()
    # the raw calls: the count first, the descriptor, the empty batch, the pointers
    desc = env_desc(texels=img.ctypes.data)
    f = (C.c_float * 64)()
    b = (C.c_ubyte * 8)()
    sp, rp, tp = surfaces.ctypes.data_as(C.c_void_p), records.ctypes.data_as(C.c_void_p), table.ctypes.data_as(C.c_void_p)
    connect = lambda m=n, s=sp, t=tp, p=rp, e=desc, h=0: lib.rt_path_connect_cpu(s, None, f, None if e is None else C.byref(e), t, p, m, None, None, 1, h, 0, f, b, f)
    assert connect(m=1 << 32) == -5 and b"2^32" in err() and err().startswith(b"rt_path_connect_cpu: ")
    assert connect(e=None) == -1 and b"null environment" in err()
    assert connect(m=0, s=None, p=None, h=5) == 0
    for bad in ({"s": None}, {"t": None}, {"p": None}):
        assert connect(**bad) == -1 and b"pointer" in err(), bad
    assert connect(h=2) == -1 and b"unknown heuristic" in err()
    assert lib.rt_path_settle_cpu(rp, 1 << 32, None, None, b, None, f, f) == -5 and lib.rt_path_settle_cpu(None, 0, None, None, None, None, None, None) == 0
    assert lib.rt_path_settle_cpu(rp, n, None, None, None, None, f, f) == -1 and b"pointer" in err()
    assert lib.rt_path_weigh_escape_cpu(C.byref(desc), tp, rp, n, None, None, None, f, 0, f) == -1 and b"pointer" in err()
    assert lib.rt_path_weigh_escape_cpu(None, tp, rp, n, None, None, f, f, 0, f) == -1 and b"null environment" in err()


def test_python_wrappers_check_their_arguments():
    hits = np.zeros((3, 13), dtype=np.int32)
    with pytest.raises(ValueError):
        paths.connect(None, None, hits, hits, hits)  # no Environment
    with pytest.raises(ValueError):
        paths.weigh_escape(None, hits, hits, hits, hits)
    with pytest.raises(ValueError):
        paths.settle(hits, hits, hits, hits)  # not CUDA tensors
    with pytest.raises(ValueError, match="nee needs env"):
        paths.trace_paths(None, hits, hits, 4, 2, nee=True)
    with pytest.raises(ValueError):
        paths.workspace(-1, "cpu", 4, nee=True)
