"""The lobe ABI (include/rt_amd.h rt_lobe_rays, rt_lobe_pdf, rt_environment_pdf, rt_mis_weigh; include/rt_lobe_host.h their CPU forms)
without a GPU: the symbols exist with the declared signatures and are listed, every status of the documented check order is returned
with its message before any device work, spp, pattern and normal_kind are refused in the hemisphere queries' words, an empty batch is
RT_OK, and the Python wrappers check their arguments."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import _capi, environment, lobes, materials

INCLUDE = Path(__file__).resolve().parent.parent / "include"
NAMES = ("rt_lobe_rays", "rt_lobe_pdf", "rt_environment_pdf", "rt_mis_weigh")
HOST_NAMES = ("rt_lobe_samples_cpu", "rt_lobe_pdf_cpu", "rt_environment_pdf_cpu", "rt_mis_weigh_cpu")
CENTER, UNIFORM, STRATIFIED = 0, 1, 2
P = C.c_void_p(16)  # never dereferenced: every call below is refused on its arguments first, or has nothing to do


def desc(width=8, height=4, texels=16, filter=0):
    return _capi.EnvironmentDesc(texels, width, height, 0.0, 1.0, filter)


def declaration(header, name):
    text = re.sub(r"/\*.*?\*/", "", (INCLUDE / header).read_text(), flags=re.S)
    found = re.findall(rf"\bint\s+{name}\s*\(([^)]*)\)\s*;", text)
    assert len(found) == 1, name
    return [" ".join(p.split()) for p in found[0].split(",")]


def test_lobe_symbols_are_exported_and_listed():
    lib = _capi.amd_lib()
    for name in NAMES:
        assert hasattr(lib, name) and name in _capi.AMD_SYMBOLS and not hasattr(_capi.host_lib(), name), name
    header = (INCLUDE / "rt_lobe_host.h").read_text()
    declared = sorted(set(re.findall(r"\b(rt_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S))))
    assert declared == sorted(HOST_NAMES) == sorted(_capi.LOBE_HOST_SYMBOLS)
    for name in HOST_NAMES:
        assert hasattr(_capi.host_lib(), name) and not hasattr(lib, name), name
    assert '#include "rt_lobe_host.h"' in (INCLUDE / "rt_host.h").read_text()
    assert lib.rt_abi_version() == 1  # additive: the version stays
    for name in ("rays", "pdf", "environment_pdf", "mis_weigh", "rays_numpy", "pdf_numpy", "environment_pdf_numpy", "mis_weigh_numpy", "workspace",
                 "Workspace", "glossy_hits", "sky_hits_mis"):
        assert callable(getattr(lobes, name)), name
    assert rt.lobes is lobes and "lobes" not in rt.__all__  # a submodule: the top-level surface gains no name
    assert (lobes.BALANCE, lobes.POWER) == (0, 1)
    assert re.search(r"#define RT_MIS_BALANCE 0u", (INCLUDE / "rt_amd.h").read_text()) and re.search(r"#define RT_MIS_POWER 1u", (INCLUDE / "rt_amd.h").read_text())


def test_the_declared_signatures():
    assert declaration("rt_amd.h", "rt_lobe_rays") == [
        "const rt_scene *scene", "const rt_hit *d_hits", "const rt_ray *d_incoming", "size_t n", "const uint32_t *d_ids", "uint32_t spp", "uint32_t pattern",
        "uint32_t seed", "uint32_t normal_kind", "rt_ray *d_rays", "unsigned char *d_asks", "float *d_dirs", "float *d_pdf", "unsigned char *d_lobe",
        "void *hip_stream"]
    assert declaration("rt_amd.h", "rt_lobe_pdf") == [
        "const rt_surface *d_surfaces", "size_t n", "const float *d_view", "const float *d_dirs", "uint32_t n_probes", "uint32_t normal_kind", "float *d_pdf",
        "void *hip_stream"]
    assert declaration("rt_amd.h", "rt_environment_pdf") == [
        "const rt_environment *env", "const void *d_table", "const float *d_dirs", "size_t count", "float *d_pdf", "uint32_t *d_texel", "void *hip_stream"]
    assert declaration("rt_amd.h", "rt_mis_weigh") == [
        "size_t count", "const float *d_pdf_own", "uint32_t n_own", "const float *d_pdf_other", "uint32_t n_other", "uint32_t heuristic", "int divide_by_own",
        "float *d_weight", "float *d_rgb", "void *hip_stream"]
    lib = _capi.amd_lib()
    assert len(lib.rt_lobe_rays.argtypes) == 15 and len(lib.rt_lobe_pdf.argtypes) == 8
    assert len(lib.rt_environment_pdf.argtypes) == 7 and len(lib.rt_mis_weigh.argtypes) == 10
    # the CPU forms take the device forms' arguments without the stream (the sampler: surfaces and normals for the scene and the hits)
    assert len(declaration("rt_lobe_host.h", "rt_lobe_pdf_cpu")) == 7 and len(declaration("rt_lobe_host.h", "rt_environment_pdf_cpu")) == 6
    assert len(declaration("rt_lobe_host.h", "rt_mis_weigh_cpu")) == 9 and len(declaration("rt_lobe_host.h", "rt_lobe_samples_cpu")) == 12


def test_lobe_rays_checks_as_the_hemisphere_queries_do():
    lib = _capi.amd_lib()
    err = lib.rt_last_error

    def rays(n, a=P, b=P, spp=1, pattern=UNIFORM, kind=0, scene=P, incoming=P):
        return lib.rt_lobe_rays(scene, a, incoming, n, None, spp, pattern, 0, kind, b, P, P, P, P, None)

    assert rays(1 << 32) == -5 and b"2^32" in err()
    assert rays(1 << 32, scene=None, a=None) == -5 and b"2^32" in err()  # the count, first
    assert rays(1 << 26, spp=64) == -5 and b"2^32" in err()  # n * spp
    assert rays(2, scene=None) == -1 and b"null scene" in err()
    assert rays(0, scene=None) == -1 and b"null scene" in err()  # before the empty batch
    assert rays(0) == 0 and rays(0, a=None, b=None, incoming=None) == 0 and rays(0, spp=0) == 0 and rays(0, spp=65, kind=7) == 0
    for bad in ({"a": None}, {"b": None}, {"incoming": None}):
        assert rays(2, **bad) == -1 and b"null" in err() and b"pointer" in err() and b"incoming-ray" in err(), bad
    assert rays(2, spp=0, a=None) == -1 and b"pointer" in err()  # the pointers before spp
    hemi = lambda spp, pattern, kind=0: lib.rt_hemisphere_rays(P, P, 2, None, spp, pattern, 0, kind, P, P, P, None)
    for spp, pattern, kind in ((4, CENTER, 0), (4, 3, 0), (5, STRATIFIED, 0), (0, CENTER, 0), (65, UNIFORM, 0), (4, UNIFORM, 2), (4, CENTER, 2)):
        assert rays(2, spp=spp, pattern=pattern, kind=kind) == -1
        mine = err().decode()
        assert hemi(spp, pattern, kind) == -1
        assert mine.split(": ", 1)[1] == err().decode().split(": ", 1)[1] and mine.startswith("rt_lobe_rays: ")
    for spp in (0, 65, 1 << 20):
        assert rays(2, spp=spp) == -1 and b"1 .. 64" in err()


def test_the_other_three_check_their_arguments():
    lib = _capi.amd_lib()
    err = lib.rt_last_error
    pdf = lambda n, probes=2, kind=0, a=P, b=P, c=P, d=P: lib.rt_lobe_pdf(a, n, b, c, probes, kind, d, None)
    assert pdf(1 << 32) == -5 and b"2^32" in err() and pdf(1 << 32, a=None) == -5
    assert pdf(1 << 20, probes=1 << 12) == -5 and b"2^32" in err() and b"pairs" in err()
    assert pdf(0) == 0 and pdf(0, a=None, kind=1) == 0 and pdf(3, probes=0, a=None) == 0
    for bad in ({"a": None}, {"b": None}, {"c": None}, {"d": None}):
        assert pdf(2, **bad) == -1 and b"null" in err() and b"pointer" in err(), bad
    assert pdf(2, kind=1) == -1 and b"RT_HEMISPHERE_GEOMETRIC" in err() and b"geometric normal" in err()
    assert pdf(2, kind=1, a=None) == -1 and b"pointer" in err()  # the pointers first
    assert pdf(2, kind=2) == -1 and b"unknown normal_kind" in err()

    epdf = lambda n, env=desc(), t=P, a=P, b=P: lib.rt_environment_pdf(C.byref(env) if env is not None else None, t, a, n, b, None, None)
    assert epdf(1 << 32) == -5 and b"2^32" in err() and epdf(1 << 32, env=None) == -5
    assert epdf(2, env=None) == -1 and b"null environment" in err() and epdf(0, env=None) == -1  # the descriptor before the empty batch
    assert epdf(2, env=desc(texels=None)) == -1 and b"null environment texels" in err()
    assert epdf(2, env=desc(width=0)) == -1 and b"width or height 0" in err()
    assert epdf(2, env=desc(width=16385, height=1)) == -5 and b"16384" in err() and b"2^27" in err()
    assert epdf(2, env=desc(filter=2)) == -1 and b"unknown filter" in err() and epdf(2, env=desc(filter=2), a=None) == -1 and b"unknown filter" in err()
    assert epdf(0) == 0 and epdf(0, t=None, a=None, b=None) == 0
    for bad in ({"t": None}, {"a": None}, {"b": None}):
        assert epdf(2, **bad) == -1 and b"null" in err() and b"pointer" in err(), bad

    mis = lambda n, own=P, other=P, h=0, w=P, rgb=P: lib.rt_mis_weigh(n, own, 4, other, 4, h, 0, w, rgb, None)
    assert mis(1 << 32) == -5 and b"2^32" in err() and mis(1 << 32, own=None) == -5
    assert mis(0) == 0 and mis(0, own=None, w=None, rgb=None, h=9) == 0
    assert mis(2, own=None) == -1 and b"pointer" in err()
    assert mis(2, w=None, rgb=None) == -1 and b"pointer" in err() and b"one of the two" in err()
    assert mis(2, h=2) == -1 and b"unknown heuristic" in err() and b"RT_MIS_POWER" in err()
    assert mis(2, h=2, own=None) == -1 and b"pointer" in err()  # the pointers first


def test_the_cpu_forms_check_their_arguments():
    lib = _capi.host_lib()
    err = lib.rt_host_last_error
    surfaces = np.zeros(4, dtype=materials.SURFACE_DTYPE)
    sp = surfaces.ctypes.data_as(C.c_void_p)
    f = (C.c_float * (3 * 64 * 4))()
    samples = lambda n=4, spp=1, pattern=UNIFORM, s=sp, v=f, d=f, p=f: lib.rt_lobe_samples_cpu(s, None, v, None, n, spp, pattern, 7, d, p, None, None)
    assert samples() == 0 and samples(spp=64, pattern=STRATIFIED) == 0 and samples(n=0, s=None, d=None) == 0
    assert samples(n=1 << 26, spp=64, s=None) == -5 and b"2^32" in err()
    assert samples(s=None) == -1 and samples(v=None) == -1 and samples(d=None) == -1 and samples(p=None) == -1 and b"pointer" in err()
    for spp in (0, 65):
        assert samples(spp=spp) == -1 and b"1 .. 64" in err()
    assert samples(pattern=CENTER) == -1 and b"RT_FILM_CENTER" in err()
    assert samples(spp=5, pattern=STRATIFIED) == -1 and b"k * k" in err()
    pdf = lambda n=4, probes=2, kind=0, s=sp, out=f: lib.rt_lobe_pdf_cpu(s, n, f, f, probes, kind, out)
    assert pdf() == 0 and pdf(n=0, s=None) == 0 and pdf(probes=0, s=None) == 0
    assert pdf(n=1 << 32) == -5 and pdf(s=None) == -1 and pdf(out=None) == -1 and b"pointer" in err()
    assert pdf(kind=1) == -1 and b"RT_HEMISPHERE_GEOMETRIC" in err() and pdf(kind=3) == -1 and b"unknown normal_kind" in err()
    img = np.ones((4, 8, 3), dtype=np.float32)
    env, table = desc(texels=img.ctypes.data), environment.table_numpy(img)
    tp = table.ctypes.data_as(C.c_void_p)
    epdf = lambda n=4, e=env, t=tp, d=f, out=f: lib.rt_environment_pdf_cpu(C.byref(e) if e is not None else None, t, d, n, out, None)
    assert epdf() == 0 and epdf(n=0, t=None, d=None) == 0
    assert epdf(n=1 << 32) == -5 and epdf(e=None) == -1 and b"null environment" in err() and epdf(n=0, e=None) == -1
    assert epdf(t=None) == -1 and epdf(d=None) == -1 and epdf(out=None) == -1 and b"pointer" in err()
    mis = lambda n=4, own=f, h=0, w=f, rgb=None: lib.rt_mis_weigh_cpu(n, own, 2, f, 2, h, 0, w, rgb)
    assert mis() == 0 and mis(n=0, own=None, w=None) == 0
    assert mis(n=1 << 32) == -5 and mis(own=None) == -1 and mis(w=None) == -1 and b"pointer" in err()
    assert mis(h=7) == -1 and b"unknown heuristic" in err()
    with pytest.raises(rt.RtError):
        lobes.rays_numpy(surfaces, np.zeros((4, 3), dtype=np.float32), 5, STRATIFIED)
    with pytest.raises(rt.RtError):
        lobes.pdf_numpy(surfaces, np.zeros((4, 3), dtype=np.float32), np.zeros((2, 4, 3), dtype=np.float32), lobes.GEOMETRIC)
    with pytest.raises(ValueError):
        lobes.pdf_numpy(surfaces, np.zeros((4, 3), dtype=np.float32), np.zeros((2, 5, 3), dtype=np.float32))
    with pytest.raises(ValueError):
        lobes.rays_numpy(np.zeros((4, 17), dtype=np.uint32), np.zeros((4, 3), dtype=np.float32), 4)
    with pytest.raises(ValueError):
        lobes.environment_pdf_numpy(img, table[:-4], np.zeros((4, 3), dtype=np.float32))
    with pytest.raises(ValueError):
        lobes.mis_weigh_numpy(np.ones(4), 1, np.ones(5), 1)


def test_python_wrappers_check_their_arguments():
    hits = np.zeros((3, 13), dtype=np.int32)
    with pytest.raises(ValueError):
        lobes.rays(None, hits, hits, 4)  # not CUDA tensors
    with pytest.raises(ValueError):
        lobes.pdf(hits, hits, hits)
    with pytest.raises(ValueError):
        lobes.environment_pdf(None, hits)
    with pytest.raises(ValueError):
        lobes.mis_weigh(hits, 1)
    with pytest.raises(ValueError):
        lobes.glossy_hits(None, hits, hits, 4, 1)
    with pytest.raises(ValueError):
        lobes.sky_hits_mis(None, None, hits, hits)
    with pytest.raises(ValueError):
        lobes.workspace(-1, "cpu", 4)
