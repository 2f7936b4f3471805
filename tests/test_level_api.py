"""The level-loop ABI (include/rt_amd.h rt_select_records, rt_cast_rays_indexed, rt_level_split / join / close / fold / finish) without a
GPU: the symbols exist and are listed, every status of the documented check order is returned before any device work, an empty batch
is RT_OK, and the Python wrappers refuse wrong dtypes and shapes before calling down."""
import ctypes as C

import pytest

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import _capi

NAMES = ("rt_select_records", "rt_cast_rays_indexed", "rt_level_split", "rt_level_join", "rt_level_close", "rt_level_fold", "rt_level_finish")
OK, INVALID, UNSUPPORTED = 0, -1, -5
FAKE = C.c_void_p(16)  # never dereferenced: every call below is refused on its arguments first, or has nothing to do
BIG = 1 << 32


def test_level_symbols_are_exported_listed_and_declared():
    lib = _capi.amd_lib()
    header = (_capi.REPO_ROOT / "include" / "rt_amd.h").read_text()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in _capi.AMD_SYMBOLS, name
        assert f"int {name}(" in header, name
    assert lib.rt_abi_version() == 1  # additive: the version stays
    for name in ("select_records", "cast_rays_indexed", "level_split", "level_join", "level_close", "level_fold", "level_finish",
                 "trace_rays_distributed_levels"):
        assert callable(getattr(rt, name)) and name in rt.__all__, name
    block = header[header.index("level loop: select"):]
    not_covered = block[block.index("Not covered:"):block.index("*/")]
    for what in ("Whitted", "rt_multi_", "indexed forms of the hit and scatter queries"):
        assert what in not_covered, what


def _order(lib, fn, required, scene=False):
    """the documented order for one entry point: fn(n, **pointers) with every pointer fake unless overridden"""
    nothing = {k: None for k in required}
    assert fn(BIG) == UNSUPPORTED and b"2^32" in lib.rt_last_error()
    assert fn(BIG + 7, **nothing) == UNSUPPORTED and b"2^32" in lib.rt_last_error()  # checked first
    if scene:
        assert fn(2, scene=None) == INVALID and b"null scene" in lib.rt_last_error()
        assert fn(0, scene=None) == INVALID and b"null scene" in lib.rt_last_error()  # before the empty batch
        assert fn(BIG, scene=None) == UNSUPPORTED
    assert fn(0) == OK
    assert fn(0, **nothing) == OK  # nothing to do: the pointers are not looked at
    for k in required:
        assert fn(2, **{k: None}) == INVALID and b"null" in lib.rt_last_error() and b"pointer" in lib.rt_last_error(), k


def test_select_records_arguments():
    lib = _capi.amd_lib()

    def fn(n, flags=FAKE, index=FAKE, count=FAKE):
        return lib.rt_select_records(flags, n, index, count, None)

    _order(lib, fn, ("flags", "index", "count"))


def test_cast_rays_indexed_arguments():
    lib = _capi.amd_lib()

    def fn(n, scene=FAKE, rays=FAKE, index=FAKE, count=FAKE, hits=FAKE, max_count=None, ray_count=None):
        return lib.rt_cast_rays_indexed(scene, rays, n, index, count, n if max_count is None else max_count, hits, ray_count, None)

    _order(lib, fn, ("rays", "index", "count", "hits"), scene=True)
    assert fn(2, max_count=BIG) == UNSUPPORTED and b"2^32" in lib.rt_last_error()
    assert fn(2, max_count=BIG, scene=None) == UNSUPPORTED
    assert fn(2, max_count=0, rays=None, hits=None) == OK  # an empty list: nothing to do
    assert fn(2, max_count=0, scene=None) == INVALID


def test_level_glue_arguments():
    lib = _capi.amd_lib()

    def split(n, hits=FAKE, type=FAKE, cosine=FAKE, a=FAKE, b=FAKE):
        return lib.rt_level_split(hits, type, cosine, n, a, b, None)

    def join(n, type=FAKE, cosine=FAKE, reflected=FAKE, kind=FAKE, escape=FAKE, nxt=FAKE, next_hits=FAKE, flags=FAKE):
        return lib.rt_level_join(type, cosine, reflected, kind, escape, n, nxt, next_hits, flags, None)

    def close(n, hits=FAKE, type=FAKE, cosine=FAKE, next_hits=FAKE, out=FAKE):
        return lib.rt_level_close(hits, type, cosine, next_hits, n, out, None)

    def fold(n, type=FAKE, cosine=FAKE, next_hits=FAKE, factor=FAKE, shade_next=FAKE, shade_missed=FAKE, value=FAKE):
        return lib.rt_level_fold(type, cosine, next_hits, factor, shade_next, shade_missed, n, value, None)

    _order(lib, split, ("hits", "type", "cosine", "a", "b"))
    _order(lib, join, ("type", "cosine", "reflected", "kind", "escape", "nxt", "next_hits", "flags"))
    _order(lib, close, ("hits", "type", "cosine", "next_hits", "out"))
    _order(lib, fold, ("type", "cosine", "next_hits", "factor", "shade_next", "shade_missed", "value"))


def test_level_finish_arguments():
    lib = _capi.amd_lib()

    def fn(n, value=FAKE, accum=FAKE, valid=FAKE):
        return lib.rt_level_finish(value, n, accum, valid, None)

    assert fn(BIG) == UNSUPPORTED and b"2^32" in lib.rt_last_error()
    assert fn(BIG, value=None, accum=None, valid=None) == UNSUPPORTED
    assert fn(0) == OK and fn(0, value=None, accum=None, valid=None) == OK
    assert fn(2, value=None) == INVALID and b"pointer" in lib.rt_last_error()
    assert fn(2, accum=None, valid=None) == INVALID and b"neither" in lib.rt_last_error()
    assert fn(2, value=None, accum=None, valid=None) == INVALID and b"pointer" in lib.rt_last_error()  # the value pointer comes first


def test_wrappers_refuse_wrong_tensors_before_calling_down():
    import torch

    cpu = torch.zeros(4, dtype=torch.uint8)
    with pytest.raises(ValueError):
        rt.select_records(cpu)  # not on the device
    with pytest.raises(ValueError):
        rt.level_finish(torch.zeros((4, 3), dtype=torch.float32))
    with pytest.raises(ValueError):
        rt.level_split(torch.zeros((4, 13), dtype=torch.int32), cpu, cpu)
    with pytest.raises(ValueError):
        rt.trace_rays_distributed_levels(None, torch.zeros((4, 11), dtype=torch.int32), 1, None)
