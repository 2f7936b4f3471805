"""The path ABI (include/rt_amd.h rt_path_begin, rt_path_advance, rt_path_resolve; include/rt_path_host.h their CPU forms) without a
GPU: the symbols exist with the declared signatures and are listed, every status of the documented check order is returned with its
message before any device work — the lobe queries' order and words, then rr_floor — an empty batch is RT_OK, the record is 32 bytes,
and the Python wrappers check their arguments."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import _capi, materials, paths

ROOT = Path(__file__).resolve().parent.parent
INCLUDE = ROOT / "include"
NAMES = ("rt_path_begin", "rt_path_advance", "rt_path_resolve")
HOST_NAMES = ("rt_path_begin_cpu", "rt_path_advance_cpu", "rt_path_resolve_cpu")
P = C.c_void_p(16)  # never dereferenced: every call below is refused on its arguments first, or has nothing to do
OFF = 0xFFFFFFFF


def declaration(header, name):
    text = re.sub(r"/\*.*?\*/", "", (INCLUDE / header).read_text(), flags=re.S)
    found = re.findall(rf"\bint\s+{name}\s*\(([^)]*)\)\s*;", text)
    assert len(found) == 1, name
    return [" ".join(p.split()) for p in found[0].split(",")]


def test_path_symbols_are_exported_and_listed():
    lib = _capi.amd_lib()
    for name in NAMES:
        assert hasattr(lib, name) and name in _capi.AMD_SYMBOLS and not hasattr(_capi.host_lib(), name), name
    header = (INCLUDE / "rt_path_host.h").read_text()
    declared = sorted(set(re.findall(r"\b(rt_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S))))
    assert declared == sorted(HOST_NAMES) == sorted(_capi.PATH_HOST_SYMBOLS)
    for name in HOST_NAMES:
        assert hasattr(_capi.host_lib(), name) and not hasattr(lib, name), name
    assert '#include "rt_path_host.h"' in (INCLUDE / "rt_host.h").read_text()
    assert lib.rt_abi_version() == 1  # additive: the version stays
    for name in ("begin", "advance", "resolve", "begin_numpy", "advance_numpy", "resolve_numpy", "workspace", "Workspace", "trace_paths"):
        assert callable(getattr(paths, name)), name
    assert rt.paths is paths and "paths" not in rt.__all__  # a submodule: the top-level surface gains no name
    text = (INCLUDE / "rt_amd.h").read_text()
    for name, value in (("ALIVE", 1), ("SPECULAR", 2), ("ESCAPED", 4), ("ROULETTE", 8), ("DARK", 16)):
        assert getattr(paths, name) == value and re.search(rf"#define RT_PATH_{name} {value}u\b", text), name


def test_the_declared_signatures():
    assert declaration("rt_amd.h", "rt_path_begin") == [
        "size_t n", "uint32_t spp", "const uint32_t *d_ids", "rt_path *d_paths", "float *d_radiance", "void *hip_stream"]
    assert declaration("rt_amd.h", "rt_path_advance") == [
        "const rt_scene *scene", "rt_path *d_paths", "size_t m", "const uint32_t *d_index", "const uint32_t *d_count", "rt_hit *d_hits",
        "const rt_ray *d_incoming", "const float *d_emitted", "uint32_t seed", "uint32_t normal_kind", "uint32_t rr_start", "float rr_floor", "int last",
        "float *d_radiance", "rt_ray *d_next_rays", "unsigned char *d_alive", "void *hip_stream"]
    assert declaration("rt_amd.h", "rt_path_resolve") == [
        "const float *d_radiance", "size_t n", "uint32_t spp", "const uint32_t *d_root", "float *d_rgb", "void *hip_stream"]
    lib, host = _capi.amd_lib(), _capi.host_lib()
    assert len(lib.rt_path_begin.argtypes) == 6 and len(lib.rt_path_advance.argtypes) == 17 and len(lib.rt_path_resolve.argtypes) == 6
    # begin and resolve on the CPU take the device forms' arguments without the stream; advance takes surfaces, normals and views for the scene, the hits and the rays
    assert len(declaration("rt_path_host.h", "rt_path_begin_cpu")) == 5 == len(host.rt_path_begin_cpu.argtypes)
    assert len(declaration("rt_path_host.h", "rt_path_resolve_cpu")) == 5 == len(host.rt_path_resolve_cpu.argtypes)
    assert len(declaration("rt_path_host.h", "rt_path_advance_cpu")) == 15 == len(host.rt_path_advance_cpu.argtypes)


def test_the_record_is_32_bytes(tmp_path):
    assert paths.PATH_DTYPE.itemsize == 32 and paths.PATH_DTYPE.names == ("beta", "pdf", "root", "id", "bounce", "flags")
    assert [paths.PATH_DTYPE.fields[f][1] for f in paths.PATH_DTYPE.names] == [0, 12, 16, 20, 24, 28]
    source = tmp_path / "size.c"
    source.write_text('#include <stddef.h>\n#include "rt_amd.h"\n_Static_assert(sizeof(rt_path) == 32, "size");\n'
                      '_Static_assert(offsetof(rt_path, pdf) == 12 && offsetof(rt_path, root) == 16 && offsetof(rt_path, flags) == 28, "layout");\n')
    done = subprocess.run(["cc", "-std=c11", "-fsyntax-only", "-I", str(INCLUDE), str(source)], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr


def test_advance_checks_as_the_lobe_queries_do_then_rr_floor():
    lib = _capi.amd_lib()
    err = lib.rt_last_error

    def advance(m, scene=P, paths_=P, index=None, count=None, hits=P, incoming=P, emitted=None, kind=0, floor=0.05, radiance=P, rays=P, alive=P):
        return lib.rt_path_advance(scene, paths_, m, index, count, hits, incoming, emitted, 0, kind, 3, floor, 0, radiance, rays, alive, None)

    assert advance(1 << 32) == -5 and b"2^32" in err() and err().startswith(b"rt_path_advance: ")
    assert advance(1 << 32, scene=None, hits=None, floor=0.0) == -5 and b"2^32" in err()  # the count, first
    assert advance(2, scene=None) == -1 and b"null scene" in err()
    assert advance(0, scene=None) == -1 and b"null scene" in err()  # before the empty batch
    assert advance(0) == 0 and advance(0, paths_=None, hits=None, kind=7, floor=0.0) == 0  # m == 0: RT_OK, nothing launched
    for bad in ({"paths_": None}, {"hits": None}, {"incoming": None}, {"radiance": None}, {"rays": None}, {"alive": None}, {"index": P}):
        assert advance(2, **bad) == -1 and b"null" in err() and b"pointer" in err() and b"incoming-ray" in err(), bad
    assert advance(2, hits=None, kind=2, floor=0.0) == -1 and b"pointer" in err()  # the pointers before the limits
    # the normal_kind in the lobe queries' words, before rr_floor
    assert advance(2, kind=2, floor=0.0) == -1
    mine = err().decode()
    assert lib.rt_lobe_rays(P, P, P, 2, None, 1, 1, 0, 2, P, P, P, P, P, None) == -1
    assert mine.split(": ", 1)[1] == err().decode().split(": ", 1)[1] and b"unknown normal_kind" in err()
    for floor in (0.0, 1.5, float("nan"), -0.25, float("inf")):
        assert advance(2, floor=floor) == -1 and b"rr_floor" in err() and b"(0, 1]" in err(), floor
    assert advance(2, paths_=C.c_void_p(8)) == -1 and b"16-byte aligned" in err()  # after everything else
    assert advance(2, paths_=C.c_void_p(8), floor=2.0) == -1 and b"rr_floor" in err()


def test_begin_and_resolve_check_their_arguments():
    lib = _capi.amd_lib()
    err = lib.rt_last_error
    begin = lambda n, spp=4, a=P, b=P: lib.rt_path_begin(n, spp, None, a, b, None)
    resolve = lambda n, spp=4, a=P, b=P: lib.rt_path_resolve(a, n, spp, None, b, None)
    for call, who in ((begin, b"rt_path_begin: "), (resolve, b"rt_path_resolve: ")):
        assert call(1 << 32) == -5 and b"2^32" in err() and err().startswith(who)
        assert call(1 << 26, spp=64) == -5 and b"2^32" in err()  # n * spp
        assert call(0) == 0 and call(0, a=None, b=None, spp=0) == 0
        assert call(2, a=None) == -1 and b"pointer" in err() and call(2, b=None) == -1 and b"pointer" in err()
        assert call(2, a=None, spp=0) == -1 and b"pointer" in err()  # the pointers before spp
        for spp in (0, 65, 1 << 20):
            assert call(2, spp=spp) == -1 and b"1 .. 64" in err()
    assert begin(2, a=C.c_void_p(24)) == -1 and b"16-byte aligned" in err()


def test_the_cpu_forms_check_their_arguments():
    lib = _capi.host_lib()
    err = lib.rt_host_last_error
    surfaces = np.zeros(4, dtype=materials.SURFACE_DTYPE)
    sp = surfaces.ctypes.data_as(C.c_void_p)
    f = (C.c_float * (3 * 64 * 4))()
    records = np.zeros(64 * 4, dtype=paths.PATH_DTYPE)
    rp = records.ctypes.data_as(C.c_void_p)
    alive = (C.c_ubyte * 4)()
    count = (C.c_uint32 * 1)(2)
    begin = lambda n=4, spp=2, a=rp, b=f: lib.rt_path_begin_cpu(n, spp, None, a, b)
    assert begin() == 0 and begin(n=0, a=None, b=None) == 0 and begin(spp=64) == 0
    assert begin(n=1 << 26, spp=64, a=None) == -5 and b"2^32" in err()
    assert begin(a=None) == -1 and begin(b=None) == -1 and b"pointer" in err()
    assert begin(spp=0) == -1 and b"1 .. 64" in err() and begin(spp=65) == -1
    advance = lambda m=4, s=sp, v=f, p=rp, index=None, c=None, floor=0.5, r=f, d=f, a=alive: lib.rt_path_advance_cpu(s, None, v, p, m, index, c, None, 1, OFF, floor, 0,
                                                                                                                    r, d, a)
    assert advance() == 0 and advance(m=0, s=None, p=None, floor=0.0) == 0 and advance(index=f, c=count) == 0
    assert advance(m=1 << 32) == -5 and b"2^32" in err()
    for bad in ({"s": None}, {"v": None}, {"p": None}, {"r": None}, {"d": None}, {"a": None}, {"index": f}):
        assert advance(**bad) == -1 and b"pointer" in err(), bad
    for floor in (0.0, 1.5, float("nan")):
        assert advance(floor=floor) == -1 and b"rr_floor" in err(), floor
    assert advance(floor=0.0, s=None) == -1 and b"pointer" in err()  # the pointers first
    resolve = lambda n=4, spp=2, a=f, b=f: lib.rt_path_resolve_cpu(a, n, spp, None, b)
    assert resolve(n=0, a=None) == 0 and resolve(n=1 << 32) == -5
    assert resolve(a=None) == -1 and resolve(b=None) == -1 and b"pointer" in err() and resolve(spp=0) == -1 and b"1 .. 64" in err()
    with pytest.raises(rt.RtError):
        paths.advance_numpy(surfaces, np.zeros((4, 3), np.float32), records[:4], np.zeros((4, 3), np.float32), rr_floor=0.0)
    with pytest.raises(rt.RtError):
        paths.begin_numpy(4, 65)
    with pytest.raises(ValueError):
        paths.advance_numpy(surfaces, np.zeros((4, 3), np.float32), records[:5], np.zeros((4, 3), np.float32))
    with pytest.raises(ValueError):
        paths.advance_numpy(surfaces, np.zeros((4, 3), np.float32), np.zeros((4, 7), np.uint32), np.zeros((4, 3), np.float32))
    with pytest.raises(ValueError):
        paths.resolve_numpy(np.zeros((8, 3), np.float32), 4, 2, np.zeros((3, 3), np.float32))


def test_python_wrappers_check_their_arguments():
    hits = np.zeros((3, 13), dtype=np.int32)
    with pytest.raises(ValueError):
        paths.begin(-1, 4)
    with pytest.raises(ValueError):
        paths.begin(3, 4, ids=hits)  # not a CUDA tensor
    with pytest.raises(ValueError):
        paths.advance(None, hits, hits, hits, hits)
    with pytest.raises(ValueError):
        paths.resolve(hits, 3, 1)
    with pytest.raises(ValueError):
        paths.trace_paths(None, hits, hits, 4, 2)
    with pytest.raises(ValueError):
        paths.trace_paths(None, hits, hits, 4, -1)
    with pytest.raises(ValueError):
        paths.workspace(-1, "cpu", 4)


def test_the_lobe_block_no_longer_lists_more_than_one_bounce():
    text = (INCLUDE / "rt_amd.h").read_text()
    lobe = text[text.index("---- lobe queries:"):text.index("---- path queries:")]
    covered = lobe[lobe.index("Not covered:"):]
    assert "more than one bounce;" not in covered.lower() and "path queries" in covered
    block = text[text.index("---- path queries:"):text.index("---- texture queries:")]
    for word in ("refraction lobes", "next-event estimation", "_host and rt_multi_*", "rt_render_*"):
        assert word in block[block.index("Not covered:"):], word
