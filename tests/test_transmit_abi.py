"""The transmission ABI (include/rt_amd.h rt_path_branch, rt_path_transmit; include/rt_transmit_host.h their CPU forms) without a GPU:
the symbols exist with the declared signatures and are listed, every status of the documented check order is returned with its message
before any device work, an empty batch is RT_OK, the Python wrappers check their arguments, and without a device the calls fail loudly."""
import ctypes as C
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import _capi, materials, paths

ROOT = Path(__file__).resolve().parent.parent
INCLUDE = ROOT / "include"
NAMES = ("rt_path_branch", "rt_path_transmit")
HOST_NAMES = ("rt_path_branch_cpu", "rt_path_transmit_cpu")
P = C.c_void_p(16)  # never dereferenced: every call below is refused on its arguments first, or has nothing to do


def declaration(header, name):
    text = re.sub(r"/\*.*?\*/", "", (INCLUDE / header).read_text(), flags=re.S)
    found = re.findall(rf"\bint\s+{name}\s*\(([^)]*)\)\s*;", text)
    assert len(found) == 1, name
    return [" ".join(p.split()) for p in found[0].split(",")]


def test_transmit_symbols_are_exported_and_listed():
    lib = _capi.amd_lib()
    for name in NAMES:
        assert hasattr(lib, name) and name in _capi.AMD_SYMBOLS and not hasattr(_capi.host_lib(), name), name
    header = (INCLUDE / "rt_transmit_host.h").read_text()
    declared = sorted(set(re.findall(r"\b(rt_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S))))
    assert declared == sorted(HOST_NAMES) == sorted(_capi.TRANSMIT_HOST_SYMBOLS)
    for name in HOST_NAMES:
        assert hasattr(_capi.host_lib(), name) and not hasattr(lib, name), name
    assert '#include "rt_transmit_host.h"' in (INCLUDE / "rt_path_host.h").read_text()  # and rt_host.h includes that one
    assert lib.rt_abi_version() == 1  # additive: the version stays
    for name in ("branch", "transmit", "branch_numpy", "transmit_numpy"):
        assert callable(getattr(paths, name)), name
    text = (INCLUDE / "rt_amd.h").read_text()
    for name, value in (("TRANSMITTED", 32), ("TRAPPED", 64)):
        assert getattr(paths, name) == value and re.search(rf"#define RT_PATH_{name} {value}u\b", text), name
    block = text[text.index("---- transmission queries:"):text.index("---- distributed (stochastic")]
    for word in ("rough transmission", "_host and rt_multi_*", "rt_render_*"):
        assert word in block[block.index("Not covered:"):], word


def test_the_declared_signatures():
    assert declaration("rt_amd.h", "rt_path_branch") == [
        "const rt_scene *scene", "rt_path *d_paths", "size_t m", "const uint32_t *d_index", "const uint32_t *d_count", "rt_hit *d_hits",
        "const rt_ray *d_incoming", "uint32_t seed", "int last", "unsigned char *d_lobe", "unsigned char *d_transmit", "rt_ray *d_walk_rays",
        "uint32_t *d_kind", "float *d_travel", "uint32_t *d_casts", "unsigned char *d_walk_flags", "void *hip_stream"]
    assert declaration("rt_amd.h", "rt_path_transmit") == [
        "const rt_scene *scene", "rt_path *d_paths", "size_t m", "const uint32_t *d_index", "const uint32_t *d_count", "rt_hit *d_hits",
        "uint32_t *d_kind", "const float *d_travel", "const rt_ray *d_escape", "uint32_t seed", "uint32_t rr_start", "float rr_floor",
        "rt_ray *d_next_rays", "unsigned char *d_alive", "unsigned char *d_walk_flags", "void *hip_stream"]
    lib, host = _capi.amd_lib(), _capi.host_lib()
    assert len(lib.rt_path_branch.argtypes) == 17 and len(lib.rt_path_transmit.argtypes) == 16
    assert len(declaration("rt_transmit_host.h", "rt_path_branch_cpu")) == 16 == len(host.rt_path_branch_cpu.argtypes)
    assert len(declaration("rt_transmit_host.h", "rt_path_transmit_cpu")) == 14 == len(host.rt_path_transmit_cpu.argtypes)


def test_branch_and_transmit_check_in_the_documented_order():
    lib = _capi.amd_lib()
    err = lib.rt_last_error

    def branch(m, scene=P, index=None, count=None, ptrs=None):
        a = [P] * 10 if ptrs is None else ptrs  # paths, hits, incoming, lobe, transmit, walk rays, kind, travel, casts, walk flags
        return lib.rt_path_branch(scene, a[0], m, index, count, a[1], a[2], 0, 0, a[3], a[4], a[5], a[6], a[7], a[8], a[9], None)

    def transmit(m, scene=P, index=None, count=None, ptrs=None, floor=0.05):
        a = [P] * 8 if ptrs is None else ptrs  # paths, hits, kind, travel, escape, next rays, alive, walk flags
        return lib.rt_path_transmit(scene, a[0], m, index, count, a[1], a[2], a[3], a[4], 0, 3, floor, a[5], a[6], a[7], None)

    for fn, n_ptrs, who in ((branch, 10, b"rt_path_branch: "), (transmit, 8, b"rt_path_transmit: ")):
        none = [None] * n_ptrs
        # 1. the limit: unsupported, and checked first — before the null scene, the empty batch and the pointers
        assert fn(1 << 32) == -5 and b"2^32" in err() and err().startswith(who)
        assert fn((1 << 32) + 7, scene=None, ptrs=none) == -5 and b"2^32" in err()
        # 2. a null scene, before the empty batch and the pointers
        assert fn(2, scene=None) == -1 and b"null scene" in err()
        assert fn(0, scene=None, ptrs=none) == -1 and b"null scene" in err()
        # 3. nothing to do: RT_OK, and no pointer is looked at
        assert fn(0) == 0 and fn(0, ptrs=none) == 0
        # 4. every pointer is required; an index needs its count, a count alone is ignored
        for missing in range(n_ptrs):
            ptrs = [P] * n_ptrs
            ptrs[missing] = None
            assert fn(2, ptrs=ptrs) == -1 and b"null" in err() and b"pointer" in err() and err().startswith(who), missing
        assert fn(2, index=P) == -1 and b"pointer" in err() and b"count (with an index)" in err()
        # 6. the record's alignment, after everything else
        unaligned = [C.c_void_p(8)] + [P] * (n_ptrs - 1)
        assert fn(2, ptrs=unaligned) == -1 and b"16-byte aligned" in err()
        assert fn(2, ptrs=[C.c_void_p(8)] + [None] * (n_ptrs - 1)) == -1 and b"pointer" in err()
    # 5. rr_floor, in the path queries' words, after the pointers and before the alignment
    for floor in (0.0, 1.5, float("nan"), -0.25, float("inf")):
        assert transmit(2, floor=floor) == -1 and b"rr_floor" in err() and b"(0, 1]" in err(), floor
    assert transmit(2, floor=0.0, ptrs=[P, None] + [P] * 6) == -1 and b"pointer" in err()
    assert transmit(2, floor=2.0, ptrs=[C.c_void_p(8)] + [P] * 7) == -1 and b"rr_floor" in err()
    assert transmit(0, floor=0.0) == 0  # m == 0 before the limits


def test_the_cpu_forms_check_their_arguments():
    lib = _capi.host_lib()
    err = lib.rt_host_last_error
    m = 4
    surfaces = np.zeros(m, dtype=materials.SURFACE_DTYPE)
    records = np.zeros(m, dtype=paths.PATH_DTYPE)
    words = np.zeros((m, 13), dtype=np.uint32)
    count = (C.c_uint32 * 1)(2)
    v = lambda a: a.ctypes.data_as(C.c_void_p)

    def branch(n=m, index=None, c=None, ptrs=None):
        a = [v(surfaces), v(words), v(words), v(records)] + [v(words)] * 7 if ptrs is None else ptrs
        return lib.rt_path_branch_cpu(a[0], a[1], a[2], a[3], n, index, c, 0, 0, a[4], a[5], a[6], a[7], a[8], a[9], a[10])

    def transmit(n=m, index=None, c=None, ptrs=None, floor=0.5):
        a = [v(surfaces), v(records)] + [v(words)] * 6 if ptrs is None else ptrs
        return lib.rt_path_transmit_cpu(a[0], a[1], n, index, c, a[2], a[3], a[4], 0, 3, floor, a[5], a[6], a[7])

    for fn, n_ptrs in ((branch, 11), (transmit, 8)):
        assert fn() == 0 and fn(n=0, ptrs=[None] * n_ptrs) == 0 and fn(index=v(words), c=count) == 0
        assert fn(n=1 << 32) == -5 and b"2^32" in err()
        for missing in range(n_ptrs):
            ptrs = [v(words)] * n_ptrs
            ptrs[missing] = None
            assert fn(ptrs=ptrs) == -1 and b"pointer" in err(), missing
        assert fn(index=v(words)) == -1 and b"pointer" in err()
    for floor in (0.0, 1.5, float("nan")):
        assert transmit(floor=floor) == -1 and b"rr_floor" in err(), floor
    assert transmit(floor=0.0, ptrs=[None] * 8) == -1 and b"pointer" in err()  # the pointers first
    with pytest.raises(rt.RtError):
        paths.transmit_numpy(surfaces, records, np.zeros(m, np.uint32), np.zeros(m, np.float32), np.zeros((m, 11), np.uint32), rr_floor=0.0)
    with pytest.raises(ValueError):
        paths.transmit_numpy(surfaces, records[:3], np.zeros(m, np.uint32), np.zeros(m, np.float32), np.zeros((m, 11), np.uint32))
    with pytest.raises(ValueError):
        paths.branch_numpy(surfaces, words[:3], np.zeros((m, 11), np.uint32), records)
    with pytest.raises(ValueError):
        paths.branch_numpy(surfaces, words, np.zeros((m, 10), np.uint32), records)


def test_python_wrappers_check_their_arguments():
    hits = np.zeros((3, 13), dtype=np.int32)
    with pytest.raises(ValueError):
        paths.branch(None, hits, hits, hits)  # not CUDA tensors
    with pytest.raises(ValueError):
        paths.transmit(None, hits, hits, hits, hits, hits, hits)
    with pytest.raises(ValueError):
        paths.trace_paths(None, hits, hits, 4, 2, transmission=True)
    with pytest.raises(ValueError):
        paths.trace_paths(None, hits, hits, 4, 2, transmission=True, walk_rounds=-1)
    torch = pytest.importorskip("torch")
    t_hits, t_rays, t_paths = torch.zeros((3, 13), dtype=torch.int32), torch.zeros((3, 11), dtype=torch.int32), torch.zeros((3, 8), dtype=torch.int32)
    with pytest.raises(ValueError):
        paths.branch(None, t_paths, t_hits, t_rays)  # CPU tensors of the right shape are refused as well
    with pytest.raises(ValueError):
        paths.transmit(None, t_paths, t_hits, torch.zeros(3, dtype=torch.int32), torch.zeros(3), t_rays, torch.zeros(3, dtype=torch.uint8))
    p = inspect.signature(paths.trace_paths).parameters
    assert p["transmission"].default is False and p["walk_rounds"].default == 11
    assert inspect.signature(paths.workspace).parameters["transmission"].default is False
    w = paths.workspace(4, "cpu", 2, transmission=True)
    assert w.walk == 8 and w.entries == 8 and (w.kind == -1).all() and not w.walk_flags.any() and not w.escape.any()
    assert paths.workspace(4, "cpu", 2).walk == 0


def test_no_device_fails_loudly_without_fallback():
    torch = pytest.importorskip("torch")
    if torch.cuda.is_available():
        return  # with a device the calls run: tests/test_gpu_transmission.py
    # the calls launch on no device: a status and a message, never a CPU answer
    lib = _capi.amd_lib()
    buf = (C.c_uint32 * 64)()
    paths_ = C.cast(C.c_void_p((C.addressof(buf) + 15) & ~15), C.c_void_p)
    rc = lib.rt_path_transmit(None, paths_, 1, None, None, buf, buf, buf, buf, 0, 3, 0.5, buf, buf, buf, None)
    assert rc == -1 and b"null scene" in lib.rt_last_error()  # without a device no scene exists to pass
    with pytest.raises(rt.RtError) as ei:
        rt.Scene(rt.reference_world())
    assert ei.value.code in (-2, -3)
