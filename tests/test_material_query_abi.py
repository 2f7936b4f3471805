"""The material-query ABI (include/rt_amd.h rt_material_hits, rt_probe_surfaces and their _host forms; rt.materials) without a GPU: the
record layout in the header, in _capi.py and in SURFACE_DTYPE; the symbols; the documented check order; the submodule's names and
signatures; and the yardstick the GPU tests (tests/test_gpu_material_queries.py) measure with — expected surfaces and Phong terms made
from orc_material_approx, orc_adjust_normal and orc_diffuse_specular alone, pinned here against orc_get_shade.  Every comparison is of
f32 bit patterns: any NaN equals any NaN, -0.0 differs from +0.0."""
import ctypes as C
import inspect
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import _capi
from homework_18_graphics_raytracer_amd._capi import Light, SceneDesc, Sphere
import _oracle
from _material_support import expected_probe, expected_surfaces, F32, handmade_hits, reference_material_roles
from _records import NONE, same_f32, valid_rows

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("rt_material_hits", "rt_material_hits_host", "rt_probe_surfaces", "rt_probe_surfaces_host")
OK, INVALID, UNSUPPORTED = 0, -1, -5


# ---- layout ----

FIELDS = [("normal", 0, 3), ("diffuse_color", 12, 3), ("shiness", 24, 1), ("specular_color", 28, 3), ("smoothness", 40, 1),
          ("transparency", 44, 1), ("refraction_index", 48, 1), ("opaque_decay", 52, 1), ("shading_normal", 56, 3), ("valid", 68, 1)]


def header_fields():
    """(name, offset, words) of rt_surface as include/rt_amd.h declares it: every member is a float, a float array or a uint32_t"""
    text = (ROOT / "include" / "rt_amd.h").read_text()
    body = re.search(r"typedef struct rt_surface \{(.*?)\} rt_surface;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out, offset = [], 0
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        ctype, names = decl.split(None, 1)
        assert ctype in ("float", "uint32_t"), decl
        for name in (x.strip() for x in names.split(",")):
            m = re.fullmatch(r"(\w+)(?:\[(\d+)\])?", name)
            words = int(m.group(2) or 1)
            out.append((m.group(1), offset, words))
            offset += 4 * words
    return out, offset


def test_the_record_is_72_bytes_everywhere():
    fields, size = header_fields()
    assert size == 72 and fields == FIELDS, fields
    assert C.sizeof(_capi.Surface) == 72 and _capi.SURFACE_WORDS == 18
    assert [(n, getattr(_capi.Surface, n).offset, getattr(_capi.Surface, n).size // 4) for n, _ in _capi.Surface._fields_] == FIELDS
    dt = rt.materials.SURFACE_DTYPE
    assert dt.itemsize == 72 and rt.materials.SURFACE_WORDS == 18
    assert [(n, dt.fields[n][1], dt.fields[n][0].itemsize // 4) for n in dt.names] == FIELDS
    assert dt["valid"] == np.uint32 and all(dt[n].base == np.float32 for n in dt.names[:-1])
    # words 0..13 are orc_material_approx's out14, in its order
    m = rt.reference_world().desc().materials[1]
    out14 = (C.c_float * 14)()
    _oracle.lib().orc_material_approx(C.byref(m), (C.c_float * 2)(0, 0), out14)
    want = list(m.normal) + list(m.diffuse_color) + [m.shiness] + list(m.specular_color) + [m.smoothness, m.transparency, m.refraction_index, m.opaque_decay]
    assert list(out14) == want


def test_symbols_are_exported_and_listed():
    lib = _capi.amd_lib()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in _capi.AMD_SYMBOLS, name
    assert lib.rt_abi_version() == 1  # additive: the version stays
    for library in ("librt_amd.so",):
        assert all(hasattr(C.CDLL(str(_capi.PKG_DIR / library)), name) for name in NAMES)
    assert not any(hasattr(_capi.host_lib(), name) for name in NAMES)  # the host library has no HIP: the queries are librt_amd's


# ---- the checks before any device work ----


def test_arguments_are_checked_in_the_documented_order():
    lib = _capi.amd_lib()
    p = C.c_void_p(16)     # never dereferenced: every call below is refused on its arguments first, or has nothing to do
    fake = C.c_void_p(16)  # a scene that is never read

    def hits_dev(n, scene=fake, a=p, b=p):
        return lib.rt_material_hits(scene, a, n, b, None)

    def hits_host(n, scene=fake, a=p, b=p):
        return lib.rt_material_hits_host(scene, a, n, b)

    for fn in (hits_dev, hits_host):
        name = fn.__name__
        assert fn(1 << 32) == UNSUPPORTED and b"2^32" in lib.rt_last_error() and b"rt_material_hits" in lib.rt_last_error(), name
        assert fn((1 << 32) + 7, scene=None, a=None, b=None) == UNSUPPORTED, name  # checked first
        assert fn(2, scene=None) == INVALID and b"null scene" in lib.rt_last_error(), name
        assert fn(0, scene=None) == INVALID and b"null scene" in lib.rt_last_error(), name  # before the empty batch
        assert fn(2, scene=None, a=None) == INVALID and b"null scene" in lib.rt_last_error(), name  # before the pointers
        assert fn(0) == OK and fn(0, a=None, b=None) == OK, name  # nothing to do: the scene is not read
        for bad in ({"a": None}, {"b": None}):
            assert fn((1 << 32) - 1, **bad) == INVALID and b"null" in lib.rt_last_error() and b"pointer" in lib.rt_last_error(), (name, bad)

    def probe_dev(n, probes=1, s=p, v=p, l=p, d=p, sp=p):
        return lib.rt_probe_surfaces(s, n, v, l, probes, d, sp, None)

    def probe_host(n, probes=1, s=p, v=p, l=p, d=p, sp=p):
        return lib.rt_probe_surfaces_host(s, n, v, l, probes, d, sp)

    nothing = dict(s=None, v=None, l=None, d=None, sp=None)
    for fn in (probe_dev, probe_host):
        name = fn.__name__
        assert fn(1 << 32) == UNSUPPORTED and b"2^32" in lib.rt_last_error() and b"rt_probe_surfaces" in lib.rt_last_error(), name
        assert fn(1 << 32, probes=0, **nothing) == UNSUPPORTED, name  # n alone, whatever the probes
        assert fn(1 << 16, probes=1 << 16) == UNSUPPORTED and b"2^32" in lib.rt_last_error() and b"pairs" in lib.rt_last_error(), name
        assert fn(1 << 31, probes=2, **nothing) == UNSUPPORTED, name
        assert fn(3, probes=0xFFFFFFFF) == UNSUPPORTED, name  # formed in 64 bits: does not wrap below the limit
        assert fn(0) == OK and fn(0, **nothing) == OK and fn(5, probes=0) == OK and fn(5, probes=0, **nothing) == OK, name
        assert fn(0, probes=0xFFFFFFFF) == OK, name
        for missing in ("s", "v", "l", "d", "sp"):
            assert fn(65537, probes=65535, **{missing: None}) == INVALID, (name, missing)  # 2^32 - 1 pairs: the next check
            assert b"null" in lib.rt_last_error() and b"pointer" in lib.rt_last_error(), (name, missing)


def test_without_a_device_the_calls_fail_with_a_status_that_names_them():
    import torch

    if torch.cuda.is_available():
        return  # with a device the calls run: tests/test_gpu_material_queries.py
    lib = _capi.amd_lib()
    p = C.c_void_p(16)
    scene = C.create_string_buffer(1 << 16)  # zeros where an rt_scene would be: copied into the launch, which no device takes
    surfaces = np.full((4, 18), 0xA5A5A5A5, dtype=np.uint32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert lib.rt_material_hits(scene, p, 4, p, None) < 0 and b"rt_material_hits" in lib.rt_last_error()
    assert lib.rt_probe_surfaces(p, 4, p, p, 2, p, p, None) < 0 and b"rt_probe_surfaces" in lib.rt_last_error()
    # the host forms: the status, and nothing written
    hits = np.zeros((4, 13), dtype=np.uint32)
    assert lib.rt_material_hits_host(scene, ptr(hits), 4, ptr(surfaces)) < 0 and b"rt_material_hits_host" in lib.rt_last_error()
    view, dirs = np.zeros((4, 3), dtype=F32), np.zeros((2, 4, 3), dtype=F32)
    dif, spe = np.full((2, 4, 3), 7.0, dtype=F32), np.full((2, 4, 3), 7.0, dtype=F32)
    assert lib.rt_probe_surfaces_host(ptr(surfaces), 4, ptr(view), ptr(dirs), 2, ptr(dif), ptr(spe)) < 0
    assert b"rt_probe_surfaces_host" in lib.rt_last_error()
    assert (surfaces == 0xA5A5A5A5).all() and (dif == 7.0).all() and (spe == 7.0).all()
    with pytest.raises(rt.RtError):
        rt.materials.probe_surfaces_numpy(surfaces, view, dirs)


# ---- the submodule ----

MATERIALS_SURFACE = {
    "PrimarySurfaces": "class: rays hits surfaces depth position geometric_normal shading_normal albedo object_index valid",
    "SURFACE_DTYPE": "72 bytes: normal diffuse_color shiness specular_color smoothness transparency refraction_index opaque_decay shading_normal valid",
    "SURFACE_WORDS": "18",
    "material_hits": "(scene: 'Scene', hits, out=None, stream=None)",
    "material_hits_numpy": "(scene: 'Scene', hits_np) -> 'np.ndarray'",
    "primary_surfaces": "(scene: 'Scene', camera: 'Camera', frame: 'Frame', stream=None) -> 'PrimarySurfaces'",
    "probe_surfaces": "(surfaces, view, light_dirs, out_diffuse=None, out_specular=None, stream=None)",
    "probe_surfaces_numpy": "(surfaces_np, view, light_dirs)",
}


def test_the_submodule_is_public_and_its_names_are_pinned():
    m = rt.materials
    assert inspect.ismodule(m) and m.__name__ == "homework_18_graphics_raytracer_amd.materials"
    assert "materials" not in rt.__all__
    assert not any(name in rt.__all__ or hasattr(rt, name) for name in MATERIALS_SURFACE)  # no name-by-name re-export
    assert sorted(m.__all__) == sorted(MATERIALS_SURFACE)
    defined = {name for name, obj in vars(m).items() if not name.startswith("_") and getattr(obj, "__module__", None) == m.__name__}
    assert defined <= set(m.__all__), defined - set(m.__all__)  # nothing public is defined beside the table
    own = {}
    for name in m.__all__:
        obj = getattr(m, name)
        if isinstance(obj, np.dtype):
            own[name] = f"{obj.itemsize} bytes: {' '.join(obj.names)}"
        elif inspect.isclass(obj):
            own[name] = "class: " + " ".join(obj._fields)
        elif callable(obj):
            own[name] = str(inspect.signature(obj))
        else:
            own[name] = repr(obj)
    assert own == MATERIALS_SURFACE, {k: v for k, v in own.items() if MATERIALS_SURFACE.get(k) != v}
    for cls in (rt.Scene, rt.World, rt.Hits):  # no method was added to an existing class
        assert not any("surface" in a or "material_hits" in a for a in vars(cls)), cls


def test_importing_the_submodule_leaves_torch_unloaded():
    code = (f"import sys\nsys.path.insert(0, {str(ROOT)!r})\nimport numpy as np\n"
            "import homework_18_graphics_raytracer_amd as rt\n"
            "from homework_18_graphics_raytracer_amd import materials\n"
            "assert materials is rt.materials and materials.SURFACE_DTYPE.itemsize == 72\n"
            "try:\n"
            "    materials.probe_surfaces_numpy(np.zeros((3, 17), dtype=np.uint32), None, None)\n"  # a numpy-only path
            "except ValueError:\n"
            "    pass\n"
            "print('torch' in sys.modules)\n")
    fresh = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert fresh.returncode == 0 and fresh.stdout.strip() == "False", fresh.stdout + fresh.stderr


def test_python_wrappers_check_their_arguments():
    m = rt.materials
    hits = np.zeros((3, 13), dtype=np.int32)
    with pytest.raises(ValueError):
        m.material_hits(None, hits)  # not a CUDA tensor
    with pytest.raises(ValueError):
        m.probe_surfaces(np.zeros((3, 18), dtype=np.int32), np.zeros((3, 3), dtype=F32), np.zeros((1, 3, 3), dtype=F32))
    with pytest.raises(ValueError):
        m.material_hits_numpy(None, np.zeros((3, 12), dtype=np.uint32))
    with pytest.raises(ValueError):
        m.probe_surfaces_numpy(np.zeros((3, 17), dtype=np.uint32), np.zeros((3, 3), dtype=F32), np.zeros((1, 3, 3), dtype=F32))
    with pytest.raises(ValueError):
        m.probe_surfaces_numpy(np.zeros((3, 18), dtype=np.uint32), np.zeros((2, 3), dtype=F32), np.zeros((1, 3, 3), dtype=F32))
    with pytest.raises(ValueError):
        m.probe_surfaces_numpy(np.zeros((3, 18), dtype=np.uint32), np.zeros((3, 3), dtype=F32), np.zeros((3, 3), dtype=F32))
    torch = pytest.importorskip("torch")
    t_hits = torch.zeros((3, 13), dtype=torch.int32)
    with pytest.raises(ValueError):
        m.material_hits(None, t_hits)  # a CPU tensor
    with pytest.raises(ValueError):
        m.probe_surfaces(torch.zeros((3, 18), dtype=torch.int32), torch.zeros((3, 3)), torch.zeros((1, 3, 3)))


# ---- the yardstick itself ----


def test_expected_surfaces_of_the_handmade_records():
    """what the oracle gives for the records of tests/test_gpu_material_queries.py, against the reference's rules written out by hand"""
    desc = rt.reference_world().desc()
    const, wave, stripes = reference_material_roles(desc)
    hits, labels, invalid = handmade_hits(desc)
    want = expected_surfaces(desc, hits)
    f = want[:, :17].view(F32)
    assert (want[invalid] == 0).all() and (want[np.setdiff1d(np.arange(len(labels)), invalid), 17] == 1).all()
    by = dict(zip(labels, range(len(labels))))
    mc = desc.materials[const]
    for name in ("+z", "z = 1.0 moved by 1 ulps", "z = 1.0 moved by -5 ulps", "z = 1.0, x = 0.0001"):  # the identity rotation
        i = by[f"normal {name}, material {const}"]
        assert f[i, 14:17].tolist() == list(mc.normal) and f[i, 3:6].tolist() == list(mc.diffuse_color), name
    i = by[f"normal -z: the antiparallel branch, material {const}"]  # half a turn about y: (0, 0, 1) -> (0, 0, -1) up to sincosf(pi / 2)
    assert abs(f[i, 16] + 1.0) < 1e-6 and abs(f[i, 14]) < 1e-6 and f[i, 15] == 0.0
    i = by[f"normal z = 1.0, x = 0.002, material {const}"]  # the general branch tilts the normal with the surface
    assert f[i, 14] > 1e-3
    i = by[f"normal NaN, material {wave}"]
    assert np.isnan(f[i, 14:17]).all() and not np.isnan(f[i, 0:14]).any()
    i = by[f"normal +z, material {wave}"]  # sin and cos of u * 10 * 2 pi, flipped to z > 0
    assert f[i, 2] > 0 and abs(float(f[i, 0]) ** 2 + float(f[i, 2]) ** 2 - 1) < 1e-6 and f[i, 1] == 0
    i32 = lambda x: 0 if np.isnan(x) else int(np.clip(np.trunc(np.float64(x)), -2 ** 31, 2 ** 31 - 1))  # Rust's `as i32`  # noqa: E731
    for obj in stripes:
        m = desc.materials[obj]
        for label, i in by.items():
            if not (label.startswith("uv") and label.endswith(f"material {obj}")):
                continue
            u, v = hits[i, 9:11].view(F32)
            arg = v * F32(m.tex_frequency) if m.diffuse_fn == 1 else (u + v) * F32(m.tex_frequency)
            cell = i32(arg)
            even = (abs(cell) % 2) == 0  # Rust's % keeps the dividend's sign: -1 % 2 == -1, which is not 0
            assert f[i, 3:6].tolist() == list(m.tex_color_a if even else m.tex_color_b), (label, cell)
    cells = {i32(hits[by[l], 10:11].view(F32)[0] * F32(20.0)) for l in by if l.startswith("uv") and l.endswith(f"material {wave}")}
    assert {-1, -2, 0, 2 ** 31 - 1, -2 ** 31} <= cells  # a negative odd and even cell, and both saturations


def test_the_oracle_probe_is_get_shade_on_a_white_light():
    """orc_diffuse_specular on the expected surface, weighted by shiness as main.rs:461 does, is orc_get_shade on a scene with one light
    of colour (1, 1, 1) in which nothing can be occluded: one sphere per material of the reference scene, side by side under a
    directional light from above"""
    ref = rt.reference_world().desc()
    n_mat = ref.n_materials
    spheres = (Sphere * n_mat)()
    for k in range(n_mat):
        spheres[k].object_index, spheres[k].center, spheres[k].radius = k, (3.0 * k, 0.0, 0.0), 1.0
    light = Light()
    light.kind, light.has_origin, light.direction, light.color = 0, 0, (0.0, -1.0, 0.0), (1.0, 1.0, 1.0)
    lights = (Light * 1)(light)
    desc = SceneDesc(None, 0, spheres, n_mat, ref.materials, n_mat, lights, 1)
    g = np.random.default_rng(5)
    n = 60 * n_mat
    target = np.repeat(np.arange(n_mat), 60)[:, None] * np.array([3.0, 0, 0]) + g.uniform(-0.9, 0.9, (n, 3))
    origin = target + g.normal(size=(n, 3)) * 4.0 + np.array([0, 6.0, 0])
    direction = target - origin
    direction /= np.linalg.norm(direction, axis=1, keepdims=True)
    rays = np.zeros((n, 11), dtype=np.uint32)
    rays[:, 0:3], rays[:, 3:6] = origin.astype(F32).view(np.uint32), direction.astype(F32).view(np.uint32)
    lib = _oracle.lib()
    orays = (_oracle.OrcRay * n).from_buffer(rays)
    hits = np.zeros((n, 13), dtype=np.uint32)
    hits[:, 0] = NONE
    h = _oracle.OrcHit()
    for i in range(n):
        if lib.orc_cast(C.byref(desc), C.byref(orays[i]), C.byref(h)):
            hits[i] = np.frombuffer(bytes(h), dtype=np.uint32)
    valid = valid_rows(desc, hits)
    assert valid.sum() > n // 2 and set(hits[valid, 2]) == set(range(n_mat))
    surfaces = expected_surfaces(desc, hits)
    view = -rays[:, 3:6].view(F32)
    dirs = np.broadcast_to(-np.array(light.direction[:], dtype=F32), (1, n, 3)).copy()
    diffuse, specular = expected_probe(surfaces, view, dirs)
    shiness = surfaces[:, 6].view(F32)
    with np.errstate(all="ignore"):
        mine = (F32(0.0) + diffuse[0] * (F32(1.0) - shiness)[:, None]) + specular[0] * shiness[:, None]
    ohits = (_oracle.OrcHit * n).from_buffer(hits)
    rgb, casts = (C.c_float * 3)(), C.c_uint64(0)
    lit = 0
    for i in np.flatnonzero(valid):
        lib.orc_get_shade(C.byref(desc), C.byref(ohits[i]), C.byref(orays[i]), rgb, C.byref(casts))
        assert same_f32(mine[i], np.array(rgb[:], dtype=F32)).all(), (i, mine[i], rgb[:])
        lit += casts.value
    assert lit > 100 and (specular[0] != 0).any() and (diffuse[0] != 0).any()
