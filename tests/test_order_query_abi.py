"""The record-ordering ABI (include/rt_amd.h rt_ray_keys / rt_sort_temp_bytes / rt_sort_records / rt_gather_records /
rt_scatter_records) without a GPU: the symbols exist and are listed, rt_sort_temp_bytes is host arithmetic, every status of the
documented check order is returned with its message before any device work, World.bounds() is the numpy min / max, and the numpy
restatement of the coherence key — which lives here, and which tests/test_gpu_order_queries.py compares the device's keys with — gives
the hand-computed keys of the documented cases."""
import ctypes as C

import numpy as np
import pytest

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import _capi
from _order_support import box_scale, F32, key_cells, numpy_keys, SORT_BUCKETS, SORT_LARGE, SORT_MAX_TILES, SORT_STEP, sort_tile

NAMES = ("rt_ray_keys", "rt_sort_temp_bytes", "rt_sort_records", "rt_gather_records", "rt_scatter_records")
OK, INVALID, UNSUPPORTED = 0, -1, -5


# ---- the key, restated in numpy: every operation a single f32 operation, in the header's order ----


def _ray(origin, direction):
    r = np.zeros((1, 11), dtype=np.uint32)
    r[0, 0:3] = np.asarray(origin, dtype=F32).view(np.uint32)
    r[0, 3:6] = np.asarray(direction, dtype=F32).view(np.uint32)
    r[0, 6:] = 0xDEADBEEF  # face and exclusion words are not read
    return r


LO, HI = (-2.0, -1.0, 0.0), (2.0, 3.0, 8.0)


def test_key_of_hand_computed_cases():
    cells = lambda o, d: tuple(int(c[0]) for c in key_cells(_ray(o, d), LO, HI))
    assert cells(LO, (0, 0, 1)) == (0, 0, 0, 32, 32)       # at box_lo: origin cells 0; +z is the centre of the map
    assert cells(HI, (0, 0, 1)) == (63, 63, 63, 32, 32)    # at box_hi: 64.0 clamps to 63
    assert cells((0.0, 1.0, 4.0), (0, 0, 1))[:3] == (32, 32, 32)
    assert cells(LO, (0, 0, -1))[3:] == (63, 63)           # -z folds to the corner (1, 1): sg(+0) = +1
    assert cells(LO, (-0.0, -0.0, -1))[3:] == (63, 63)     # sg(-0.0) = +1 as well
    assert cells(LO, (1, 0, 0))[3:] == (63, 32) and cells(LO, (-1, 0, 0))[3:] == (0, 32)
    assert cells(LO, (0, 1, 0))[3:] == (32, 63) and cells(LO, (0, -1, 0))[3:] == (32, 0)
    assert cells(LO, (1, 0, -0.0))[3:] == (63, 32)         # dz = -0.0 does not fold
    assert cells(LO, (0.25, 0.25, -0.5))[3:] == (56, 56)   # p = (.25, .25) folds to (.75, .75): (.75 * .5 + .5) * 64 = 56
    assert cells(LO, (0, 0, 0))[3:] == (0, 0)              # 0 / 0: NaN cells are 0
    assert cells((np.nan, np.nan, np.nan), (0, 0, 1))[:3] == (0, 0, 0)
    assert cells((np.inf, -np.inf, 1e30), (0, 0, 1))[:3] == (63, 0, 63)
    assert cells((-9.0, 9.0, 4.0), (0, 0, 1))[:3] == (0, 63, 32)  # outside the box
    # a degenerate box: hi == lo, hi < lo, NaN -> scale 0 -> cell 0 (inf * 0 is NaN: 0 too)
    assert np.array_equal(box_scale((0, 1, np.nan), (0, 0, 1)), np.zeros(3, dtype=F32))
    assert tuple(int(c[0]) for c in key_cells(_ray((5, np.inf, 5), (0, 0, 1)), (0, 1, np.nan), (0, 0, 1)))[:3] == (0, 0, 0)
    # codes: x = 1 -> bit 0, y = 1 -> bit 1, z = 2 -> bit 5; u = 63 -> even bits, v = 32 -> bit 11
    r = _ray((-2.0 + 1.5 * 4 / 64, -1.0 + 1.5 * 4 / 64, 2.5 * 8 / 64), (1, 0, 0))
    assert tuple(int(c[0]) for c in key_cells(r, LO, HI)) == (1, 1, 2, 63, 32)
    ocode, dcode = 0b100011, 0b010101010101 | (1 << 11)
    assert int(numpy_keys(r, LO, HI, 0)[0]) == (ocode << 12) | dcode
    assert int(numpy_keys(r, LO, HI, 1)[0]) == (dcode << 18) | ocode
    g = np.random.default_rng(1)
    many = np.zeros((1000, 11), dtype=np.uint32)
    many[:, 0:6] = g.normal(0, 3, (1000, 6)).astype(F32).view(np.uint32)
    assert (numpy_keys(many, LO, HI, 0) >> 30).max() == 0 and (numpy_keys(many, LO, HI, 1) >> 30).max() == 0


# ---- the ABI ----

def test_order_symbols_are_exported_and_listed():
    lib = _capi.amd_lib()
    header = (_capi.REPO_ROOT / "include" / "rt_amd.h").read_text()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in _capi.AMD_SYMBOLS, name
        assert f" {name}(" in header, name
    assert "#define RT_ORDER_DIRECTION_MAJOR 1u" in header and rt.ORDER_DIRECTION_MAJOR == 1
    assert lib.rt_abi_version() == 1  # additive: the version stays
    for name in ("ray_keys", "sort_temp_bytes", "sort_records", "gather_records", "scatter_records", "cast_rays_ordered",
                 "trace_rays_ordered", "order_workspace", "ORDER_DIRECTION_MAJOR"):
        assert name in rt.__all__ and hasattr(rt, name), name


def test_sort_temp_bytes_is_host_arithmetic():
    lib = _capi.amd_lib()
    assert lib.rt_sort_temp_bytes(0) == 0
    assert lib.rt_sort_temp_bytes(1 << 32) == 0 and lib.rt_sort_temp_bytes((1 << 32) + 5) == 0
    sizes = sorted({1, 2, 63, 64, 65, 2047, 2048, 2049, 4097, 65537, (1 << 20) + 37, (1 << 21) - 1, 1 << 21, (1 << 21) + 1, (1 << 22) + 1,
                    1 << 24, (1 << 24) + 1, 1 << 31, (1 << 32) - 1} | set(range(2048 * 1023 - 3, 2048 * 1025 + 3, 1)))
    got = [lib.rt_sort_temp_bytes(n) for n in sizes]
    assert all(b > 0 and b % 4 == 0 for b in got)
    assert all(a <= b for a, b in zip(got, got[1:])), "monotone in n"
    assert all(b >= 16 * n for n, b in zip(sizes, got))  # room for two (key, index) pair buffers at least
    assert rt.sort_temp_bytes(4097) == lib.rt_sort_temp_bytes(4097)


def test_sort_tile_restated_and_the_table_it_needs():
    lib = _capi.amd_lib()
    for n, want in SORT_LARGE.items():
        assert sort_tile(n) == want, (n, sort_tile(n))
    assert sort_tile((1 << 20) + 37) == (2048, 513) and sort_tile(2_073_600) == (2048, 1013)  # one step: what the suite had before
    assert sort_tile((1 << 21) + 4099) == (4096, 514)
    for n in sorted(set(SORT_LARGE) | {1, 2048, 2049, (1 << 21) - 1, (1 << 21) + 4099, (1 << 22) + 1, 1 << 24, (1 << 32) - 1}):
        tile, tiles = sort_tile(n)
        assert tile % SORT_STEP == 0 and tiles <= SORT_MAX_TILES and tiles * tile >= n > (tiles - 1) * tile, n
        # the workspace: two (key field, index) pair buffers of n words each, then 257 words per tile of the bucket table — never
        # fewer than the tiles the sort launches (the GPU tests put sentinels behind exactly this many bytes)
        table_words = lib.rt_sort_temp_bytes(n) // 4 - 4 * n
        assert table_words == min(-(-n // SORT_STEP), SORT_MAX_TILES) * SORT_BUCKETS and table_words >= tiles * SORT_BUCKETS, n


def test_ray_keys_arguments_are_checked_before_device_work():
    lib = _capi.amd_lib()
    fake = C.c_void_p(16)  # never dereferenced: every call below is refused on its arguments first, or has nothing to do
    lo, hi = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1)

    def keys(n, r=fake, a=lo, b=hi, flags=0, k=fake):
        return lib.rt_ray_keys(r, n, a, b, flags, k, None)

    assert keys(1 << 32) == UNSUPPORTED and b"2^32" in lib.rt_last_error()
    assert keys((1 << 32) + 1, r=None, a=None, b=None, flags=99, k=None) == UNSUPPORTED  # checked first
    assert keys(0) == OK and keys(0, r=None, a=None, b=None, flags=99, k=None) == OK     # nothing to do
    for bad in ({"r": None}, {"a": None}, {"b": None}, {"k": None}):
        assert keys(2, **bad) == INVALID and b"null" in lib.rt_last_error(), bad
        assert keys(2, flags=2, **bad) == INVALID and b"null" in lib.rt_last_error(), bad   # the pointers before the values
    for flags in (2, 3, 4, 1 << 31):
        assert keys(2, flags=flags) == INVALID and b"flag" in lib.rt_last_error(), flags


def test_sort_records_arguments_are_checked_before_device_work():
    lib = _capi.amd_lib()
    fake = C.c_void_p(16)
    big = 1 << 40

    def sort(n, k=fake, first=0, bits=32, i=fake, c=fake, o=fake, t=fake, size=big):
        return lib.rt_sort_records(k, n, first, bits, i, c, o, t, size, None)

    assert sort(1 << 32) == UNSUPPORTED and b"2^32" in lib.rt_last_error()
    assert sort(1 << 32, k=None, bits=0, i=None, o=None, t=None, size=0) == UNSUPPORTED
    assert sort(0) == OK and sort(0, k=None, bits=0, i=None, o=None, t=None, size=0) == OK
    for bad in ({"k": None}, {"o": None}, {"t": None}):
        assert sort(2, **bad) == INVALID and b"null" in lib.rt_last_error(), bad
        assert sort(2, bits=0, size=0, **bad) == INVALID and b"null" in lib.rt_last_error(), bad
    for first, bits in ((0, 0), (0, 33), (1, 32), (31, 2), (32, 1), (0xFFFFFFFF, 2), (5, 0)):
        assert sort(2, first=first, bits=bits) == INVALID and b"key_bits" in lib.rt_last_error(), (first, bits)
        assert sort(2, first=first, bits=bits, size=0, i=None) == INVALID and b"key_bits" in lib.rt_last_error()  # before the others
    need = lib.rt_sort_temp_bytes(2)
    assert sort(2, size=need - 1) == INVALID and b"rt_sort_temp_bytes" in lib.rt_last_error()
    assert sort(2, size=0, i=None) == INVALID and b"rt_sort_temp_bytes" in lib.rt_last_error()  # before the count without a list
    assert sort(2, i=None) == INVALID and b"count" in lib.rt_last_error()
    assert sort(2, i=None, size=need) == INVALID and b"count" in lib.rt_last_error()


@pytest.mark.parametrize("name", ["rt_gather_records", "rt_scatter_records"])
def test_gather_and_scatter_arguments_are_checked_before_device_work(name):
    lib = _capi.amd_lib()
    fn = getattr(lib, name)
    fake = C.c_void_p(16)

    def move(n, m, s=fake, size=44, i=fake, c=fake, d=fake):
        return fn(s, size, n, i, c, m, d, None)

    assert move(1 << 32, 4) == UNSUPPORTED and b"2^32" in lib.rt_last_error()
    assert move(4, 1 << 32) == UNSUPPORTED and b"2^32" in lib.rt_last_error()
    assert move(1 << 32, 0, s=None, size=5, i=None, d=None) == UNSUPPORTED  # before the empty batch
    assert move(0, 4) == OK and move(4, 0) == OK and move(0, 0, s=None, size=5, i=None, c=None, d=None) == OK
    for bad in ({"s": None}, {"i": None}, {"d": None}):
        assert move(4, 4, **bad) == INVALID and b"null" in lib.rt_last_error(), bad
        assert move(4, 4, size=5, **bad) == INVALID and b"null" in lib.rt_last_error(), bad  # the pointers before the values
    for size in (0, 1, 2, 3, 5, 6, 7, 46, 258, 260, 1 << 20):
        assert move(4, 4, size=size) == INVALID and b"record_bytes" in lib.rt_last_error(), size
        assert move(4, 4, size=size, c=None) == INVALID and b"record_bytes" in lib.rt_last_error(), size


def test_python_wrappers_check_their_arguments():
    r11 = np.zeros((3, 11), dtype=np.int32)
    with pytest.raises(ValueError):
        rt.ray_keys(r11, (0, 0, 0), (1, 1, 1))  # not a CUDA tensor
    with pytest.raises(ValueError):
        rt.sort_records(np.zeros(3, dtype=np.int32))
    with pytest.raises(ValueError):
        rt.gather_records(r11, np.zeros(3, dtype=np.int32))
    with pytest.raises(ValueError):
        rt.scatter_records(r11, np.zeros(3, dtype=np.int32), r11)
    with pytest.raises(ValueError):
        rt.cast_rays_ordered(None, r11)
    with pytest.raises(ValueError):
        rt.trace_rays_ordered(None, r11, 3)


def test_world_bounds_against_numpy():
    world = rt.reference_world()
    d = world.desc()
    pts = [tuple(v.position) for i in range(d.n_triangles) for v in d.triangles[i].vertices]
    for i in range(d.n_spheres):
        s = d.spheres[i]
        c, r = np.asarray(s.center[:], dtype=F32), F32(s.radius)
        pts += [tuple(c - r), tuple(c + r)]
    p = np.asarray(pts, dtype=F32)
    lo, hi = world.bounds()
    assert lo.dtype == F32 and hi.dtype == F32 and lo.shape == (3,) and hi.shape == (3,)
    assert np.array_equal(lo, p.min(axis=0)) and np.array_equal(hi, p.max(axis=0)) and (hi > lo).all()
    # non-finite coordinates are left out, coordinate by coordinate; an empty world is a point at the origin
    w = rt.World()
    assert all(np.array_equal(b, np.zeros(3, dtype=F32)) for b in w.bounds())
    o = w.push_object(d.materials[0])
    o.push_sphere((1.0, 2.0, 3.0), 0.5)
    o.push_flat_triangle([(np.nan, 0.0, 0.0), (0.0, np.inf, 9.0), (-4.0, 1.0, -np.inf)], [(0, 0), (1, 0), (0, 1)])
    lo, hi = w.bounds()
    assert np.array_equal(lo, np.asarray((-4.0, 0.0, 0.0), dtype=F32)) and np.array_equal(hi, np.asarray((1.5, 2.5, 9.0), dtype=F32))
