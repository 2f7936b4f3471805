"""The mesh-ordering ABI (include/rt_amd.h rt_triangle_keys / rt_order_triangles_temp_bytes / rt_order_triangles /
rt_order_triangles_host) without a GPU: the symbols exist and are listed, every status of the documented check order is returned before
any device work, the workspace size is host arithmetic, rt.unorder_hits and rt.order_rays round-trip on hand-made records, and the numpy
restatement of the key and of the two stable sorts — which lives here, and which tests/test_gpu_mesh_order.py compares the device with —
turns the shuffled 2 304-triangle sweep mesh into a description whose leaves rt_scene_create can bound: the node tree of the shuffled,
the ordered and the natural description (rt_scene_describe_nodes, host only) and the median squared radius of their leaves."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import _capi
from _mesh_order_support import _triangle, box_scale, desc_with, F32, HI, LO, numpy_keys, numpy_perm, object_bits, sweep, triangle_cells

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("rt_triangle_keys", "rt_order_triangles_temp_bytes", "rt_order_triangles", "rt_order_triangles_host")
OK, INVALID, UNSUPPORTED = 0, -1, -5
NONE = 0xFFFFFFFF
CONE = 0xFFFFFFFF


def test_key_of_hand_computed_cases():
    cells = lambda *p: tuple(int(c[0]) for c in triangle_cells(_triangle(*p), LO, HI))
    assert cells(LO, LO, LO) == (0, 0, 0)                                      # the centroid on box_lo
    assert cells(HI, HI, HI) == (1023, 1023, 1023)                             # on box_hi: 1024.0 clamps to 1023
    assert cells((0, 1, 4), (0, 1, 4), (0, 1, 4)) == (512, 512, 512)
    assert cells((-3, 0, 0), (3, 0, 0), (0, 3, 12)) == (512, 512, 512)         # the centroid, not a vertex
    assert cells((-9, 9, 4), (-9, 9, 4), (-9, 9, 4)) == (0, 1023, 512)         # beyond both
    assert cells((np.nan, 0, 0), (0, np.inf, 0), (0, 0, -np.inf)) == (0, 1023, 0)
    assert cells((np.inf, 0, 0), (-np.inf, 0, 0), (0, 0, 0))[0] == 0           # inf - inf: NaN cells are 0
    assert cells((-0.0, -0.0, -0.0), (-0.0, -0.0, -0.0), (-0.0, -0.0, -0.0)) == (512, 256, 0)
    assert np.array_equal(box_scale((0, 1, np.nan), (0, 0, 1)), np.zeros(3, dtype=F32))  # hi == lo, hi < lo, NaN: scale 0
    degenerate = _triangle((5, np.inf, 5), (5, 1, 5), (5, 1, 5))
    assert tuple(int(c[0]) for c in triangle_cells(degenerate, (0, 1, np.nan), (0, 0, 1))) == (0, 0, 0)  # inf * 0 is NaN: 0 too
    # x = 1 -> bit 0, y = 1 -> bit 1, z = 2 -> bit 5, x = 1023 -> every third bit
    p = (-2.0 + 1.5 * 4 / 1024, -1.0 + 1.5 * 4 / 1024, 2.5 * 8 / 1024)
    assert cells(p, p, p) == (1, 1, 2) and int(numpy_keys(_triangle(p, p, p), LO, HI)[0]) == 0b100011
    q = (9.0, -9.0, -9.0)
    assert int(numpy_keys(_triangle(q, q, q), LO, HI)[0]) == 0o1111111111
    g = np.random.default_rng(1)
    many = np.zeros((1000, 25), dtype=np.uint32)
    many[:, 1:] = g.normal(0, 3, (1000, 24)).astype(F32).view(np.uint32)
    assert (numpy_keys(many, LO, HI) >> 30).max() == 0
    assert [object_bits(n) for n in (0, 1, 2, 3, 4, 5, 256, 257, 0xFFFFFFFF)] == [1, 1, 1, 2, 2, 3, 8, 9, 32]


# ---- the ABI ----

def test_mesh_order_symbols_are_exported_and_listed():
    lib = _capi.amd_lib()
    header = (_capi.REPO_ROOT / "include" / "rt_amd.h").read_text()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in _capi.AMD_SYMBOLS, name
        assert f" {name}(" in header, name
    assert lib.rt_abi_version() == 1  # additive: the version stays
    for name in ("triangle_keys", "order_triangles_temp_bytes", "order_triangles", "unorder_hits", "order_rays"):
        assert name in rt.__all__ and hasattr(rt, name), name
    assert callable(rt.World.ordered)


def test_order_triangles_temp_bytes_is_host_arithmetic():
    lib = _capi.amd_lib()
    assert lib.rt_order_triangles_temp_bytes(0) == 0
    assert lib.rt_order_triangles_temp_bytes(1 << 32) == 0 and lib.rt_order_triangles_temp_bytes((1 << 32) + 5) == 0
    sizes = sorted({1, 2, 63, 64, 65, 2047, 2048, 2049, 2332, 9244, 147484, (1 << 21) - 1, 1 << 21, (1 << 21) + 1, 1 << 24, 1 << 31, (1 << 32) - 1}
                   | set(range(2048 * 1023 - 3, 2048 * 1025 + 3)))
    got = [lib.rt_order_triangles_temp_bytes(n) for n in sizes]
    assert all(b > 0 and b % 4 == 0 for b in got)
    assert all(a <= b for a, b in zip(got, got[1:])), "monotone in n"
    assert all(b == 8 * n + lib.rt_sort_temp_bytes(n) for n, b in zip(sizes, got))  # the keys, the objects, the sort's own
    assert rt.order_triangles_temp_bytes(2332) == lib.rt_order_triangles_temp_bytes(2332)


def test_triangle_keys_arguments_are_checked_before_device_work():
    lib = _capi.amd_lib()
    fake = C.c_void_p(16)  # never dereferenced: every call below is refused on its arguments first, or has nothing to do
    lo, hi = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1)

    def keys(n, t=fake, a=lo, b=hi, k=fake, o=fake):
        return lib.rt_triangle_keys(t, n, a, b, k, o, None)

    assert keys(1 << 32) == UNSUPPORTED and b"2^32" in lib.rt_last_error()
    assert keys((1 << 32) + 1, t=None, a=None, b=None, k=None, o=None) == UNSUPPORTED  # checked first
    assert keys(0) == OK and keys(0, t=None, a=None, b=None, k=None, o=None) == OK     # nothing to do
    for bad in ({"t": None}, {"a": None}, {"b": None}, {"k": None}):
        assert keys(2, **bad) == INVALID and b"null" in lib.rt_last_error(), bad
        assert keys(2, o=None, **bad) == INVALID and b"null" in lib.rt_last_error(), bad


def test_order_triangles_arguments_are_checked_before_device_work():
    lib = _capi.amd_lib()
    fake = C.c_void_p(16)
    lo, hi = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1)
    big = 1 << 40

    def order(n, t=fake, a=lo, b=hi, objects=3, p=fake, d=fake, w=fake, size=big):
        return lib.rt_order_triangles(t, n, a, b, objects, p, d, w, size, None)

    assert order(1 << 32) == UNSUPPORTED and b"2^32" in lib.rt_last_error()
    assert order(1 << 32, t=None, a=None, b=None, p=None, d=None, w=None, size=0) == UNSUPPORTED  # checked first
    assert order(0) == OK and order(0, t=None, a=None, b=None, p=None, d=None, w=None, size=0) == OK
    for bad in ({"t": None}, {"a": None}, {"b": None}, {"p": None}, {"w": None}):
        assert order(2, **bad) == INVALID and b"null" in lib.rt_last_error(), bad
        assert order(2, size=0, d=None, **bad) == INVALID and b"null" in lib.rt_last_error(), bad  # the pointers before the size
    need = lib.rt_order_triangles_temp_bytes(2)
    for d in (fake, None):
        assert order(2, size=need - 1, d=d) == INVALID and b"rt_order_triangles_temp_bytes" in lib.rt_last_error()
        assert order(2, size=0, d=d) == INVALID and b"rt_order_triangles_temp_bytes" in lib.rt_last_error()


def test_order_triangles_host_checks_and_writes_nothing_without_a_device():
    import torch

    lib = _capi.amd_lib()
    lo, hi = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1)
    tris = (_capi.Triangle * 4)()
    perm = (C.c_uint32 * 4)(*([0xA5A5A5A5] * 4))
    out = (_capi.Triangle * 4)()
    C.memset(out, 0x5A, C.sizeof(out))
    host = lib.rt_order_triangles_host
    assert host(tris, 1 << 32, lo, hi, 1, perm, out) == UNSUPPORTED and b"2^32" in lib.rt_last_error()
    assert host(None, 1 << 32, None, None, 1, None, None) == UNSUPPORTED
    assert host(None, 0, None, None, 1, None, None) == OK
    for bad in ((None, lo, hi, perm), (tris, None, hi, perm), (tris, lo, None, perm), (tris, lo, hi, None)):
        assert host(bad[0], 4, bad[1], bad[2], 1, bad[3], out) == INVALID and b"null" in lib.rt_last_error()
    if torch.cuda.is_available():
        return  # with a device the call runs: tests/test_gpu_mesh_order.py
    assert host(tris, 4, lo, hi, 1, perm, out) < 0  # a status ...
    assert list(perm) == [0xA5A5A5A5] * 4 and bytes(out) == b"\x5a" * C.sizeof(out)  # ... and nothing written
    with pytest.raises(rt.RtError):
        rt.reference_world().ordered()


def test_python_wrappers_check_their_arguments():
    t25 = np.zeros((3, 25), dtype=np.int32)
    with pytest.raises(ValueError):
        rt.triangle_keys(t25, (0, 0, 0), (1, 1, 1))  # not a CUDA tensor
    with pytest.raises(ValueError):
        rt.order_triangles(t25, (0, 0, 0), (1, 1, 1), 1)
    with pytest.raises(ValueError):
        rt.unorder_hits(np.zeros((3, 12), dtype=np.uint32), np.arange(3))
    with pytest.raises(ValueError):
        rt.order_rays(np.zeros((3, 11), dtype=np.uint32), np.zeros((3, 1)))


# ---- the helpers ----

def test_unorder_hits_and_order_rays_round_trip():
    perm = np.asarray([3, 0, 4, 1, 2], dtype=np.uint32)  # new position j holds old triangle perm[j]
    inverse = np.asarray([1, 3, 4, 0, 2], dtype=np.uint32)
    hits = np.zeros(7, dtype=rt.HIT_DTYPE)
    hits["kind"] = [rt.TRIANGLE, rt.TRIANGLE, rt.SPHERE, NONE, rt.TRIANGLE, rt.TRIANGLE, rt.SPHERE]
    hits["index"] = [0, 4, 2, 0, 5, 0xFFFFFFFF, 4]  # two triangle hits, a sphere hit, no hit, two triangle indices outside, a sphere hit
    hits["distance"] = np.arange(7, dtype=F32)
    hits["object_index"] = 9
    back = rt.unorder_hits(hits, perm)
    assert back.dtype == rt.HIT_DTYPE and back is not hits
    assert back["index"].tolist() == [3, 2, 2, 0, 5, 0xFFFFFFFF, 4]
    for field in ("kind", "distance", "object_index", "position", "normal", "uv", "face_direction"):
        assert np.array_equal(back[field], hits[field]), field
    assert hits["index"].tolist() == [0, 4, 2, 0, 5, 0xFFFFFFFF, 4]  # the input is only read
    as_words = rt.unorder_hits(hits.view(np.uint32).reshape(-1, 13), perm)
    assert np.array_equal(as_words.view(np.uint32), back.view(np.uint32))
    # hits in the old numbering, sent forward through the inverse and back
    old = hits.copy()
    assert np.array_equal(rt.unorder_hits(rt.unorder_hits(old, inverse), perm).view(np.uint32), old.view(np.uint32))

    rays = np.zeros(7, dtype=rt.RAY_DTYPE)
    rays["has_exclude"] = [1, 1, 1, 0, 1, 1, 1]
    rays["exclude_kind"] = [rt.TRIANGLE, rt.TRIANGLE, rt.SPHERE, rt.TRIANGLE, rt.TRIANGLE, rt.TRIANGLE, rt.TRIANGLE]
    rays["exclude_index"] = [3, 2, 4, 3, 5, 0xFFFFFFFF, 0]  # the fourth has no exclusion; two are outside the array
    rays["exclude_face"] = [0, 1, 2, 0, 1, 2, 0]
    rays["origin"] = 1.5
    forward = rt.order_rays(rays, perm)
    assert forward["exclude_index"].tolist() == [0, 4, 4, 3, 5, 0xFFFFFFFF, 1]
    for field in ("origin", "direction", "face_direction", "has_exclude", "exclude_kind", "exclude_face"):
        assert np.array_equal(forward[field], rays[field]), field
    assert np.array_equal(rt.order_rays(forward, inverse).view(np.uint32), rays.view(np.uint32))  # and back
    # an excluded triangle and the hit on it name the same primitive on either side
    assert np.array_equal(perm[forward["exclude_index"][[0, 1, 6]]], rays["exclude_index"][[0, 1, 6]])
    identity = np.arange(5, dtype=np.uint32)
    assert np.array_equal(rt.order_rays(rays, identity).view(np.uint32), rays.view(np.uint32))
    assert np.array_equal(rt.unorder_hits(hits, identity).view(np.uint32), hits.view(np.uint32))


# ---- the node table ----


def nodes_of(desc):
    """rt_scene_describe_nodes: rows of (first, count, n_normals, skip_to, dealing word, 0)"""
    lib = _capi.amd_lib()
    n = C.c_uint32(0)
    _capi.check(lib.rt_scene_describe_nodes(C.byref(desc), None, 0, C.byref(n)))
    words = (C.c_uint32 * (6 * n.value))()
    _capi.check(lib.rt_scene_describe_nodes(C.byref(desc), words, n.value, C.byref(n)))
    return np.frombuffer(words, dtype=np.uint32).reshape(-1, 6).copy()


def leaf_r2_hi(raw, nodes):
    """r2_hi — the squared radius, margins included, of the sphere the walkers test — of every leaf of `nodes` that carries one
    (count != 0 and n_normals != 0), restated from layout_scene (csrc/rt_api_layout.hip) in float64: a triangle's own sphere is its
    circumcircle, or the circle over its longest side when it is obtuse, times 1.05 * 1.0001 in the square; a leaf's centre is the middle
    of its vertices' box, its radius the farthest reach of a triangle's sphere, and r2_hi that square times 1.0001.  The rounding to
    binary32 on the way is left out: the figure is compared between descriptions, not with the device's bits."""
    p = np.ascontiguousarray(raw).view(np.uint32).reshape(-1, 25)[:, 1:].copy().view(F32).reshape(-1, 3, 8)[:, :, 0:3].astype(np.float64)
    a, b, c = p[:, 0], p[:, 1], p[:, 2]
    la, lb, lc = ((c - b) ** 2).sum(1), ((c - a) ** 2).sum(1), ((b - a) ** 2).sum(1)
    wa, wb, wc = la * (lb + lc - la), lb * (lc + la - lb), lc * (la + lb - lc)
    with np.errstate(all="ignore"):
        centre = (wa[:, None] * a + wb[:, None] * b + wc[:, None] * c) / (wa + wb + wc)[:, None]
    for obtuse, u, v in ((la >= lb + lc, b, c), (lb >= la + lc, a, c), (lc >= la + lb, a, b)):
        centre[obtuse] = 0.5 * (u[obtuse] + v[obtuse])
    r2 = ((p - centre[:, None, :]) ** 2).sum(2).max(1)  # contains the three vertices
    bq = 1.05 * r2 * 1.0001
    out = []
    for first, count, n_normals in nodes[:, :3]:
        if count == 0 or n_normals == 0:
            continue
        k = slice(int(first), int(first + count))
        v = p[k].reshape(-1, 3)
        mid = 0.5 * (v.min(0) + v.max(0))
        reach = np.sqrt(((centre[k] - mid) ** 2).sum(1)) + np.sqrt(bq[k])
        out.append(reach.max() ** 2 * 1.0001)
    return np.asarray(out)


def test_ordered_leaves_are_patches(tmp_path):
    """the 2 304-triangle flat sweep mesh (k = 3) in the literal scene, shuffled with a fixed seed, then ordered by the numpy
    restatement: a shuffled leaf spans the object, an ordered one spans a patch.  Measured here on the CPU (and written into
    DESIGN.md §3.18): the median r2_hi over the leaves that carry a sphere is 0.1227 shuffled (37 leaves: neighbours that span the
    same sphere are joined up to 64 triangles), 0.01477 ordered (78 leaves), 0.01091 natural (145 leaves) — the ordered median is
    1.35 times the natural order's and 1/8.3 of the shuffled one's.  No factor against the natural order is asserted."""
    world, natural, shuffled, mesh = sweep(3, tmp_path)
    base = world.desc()
    lo, hi = world.bounds()
    perm = numpy_perm(shuffled, lo, hi, base.n_materials)
    assert np.array_equal(np.sort(perm), np.arange(shuffled.shape[0]))
    ordered = shuffled[perm]
    assert (np.diff(ordered[:, 0].astype(np.int64)) >= 0).all()  # grouped by object, ascending
    medians, leaves = {}, {}
    for name, raw in (("shuffled", shuffled), ("ordered", ordered), ("natural", natural)):
        nodes = nodes_of(desc_with(base, raw))
        r2 = leaf_r2_hi(raw, nodes)
        inside = nodes[(nodes[:, 1] != 0) & (nodes[:, 2] != 0)]
        on_mesh = np.isin(inside[:, 0], np.flatnonzero(raw[:, 0] == natural[mesh[0], 0]))
        assert on_mesh.sum() >= 36, (name, "the mesh's leaves carry a sphere", on_mesh.sum())  # 144 leaves of 16; neighbours that span the same sphere are joined up to 64
        medians[name], leaves[name] = float(np.median(r2)), int(r2.size)
    print(f"median r2_hi over leaves with a sphere: shuffled {medians['shuffled']:.6g} ({leaves['shuffled']} leaves), "
          f"ordered {medians['ordered']:.6g} ({leaves['ordered']}), natural {medians['natural']:.6g} ({leaves['natural']}); "
          f"ordered / natural {medians['ordered'] / medians['natural']:.3f}, shuffled / ordered {medians['shuffled'] / medians['ordered']:.1f}")
    assert medians["ordered"] < medians["shuffled"]
