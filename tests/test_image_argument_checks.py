"""What the image-space query modules (film, denoise, temporal, svgf, rectify, upsample, adaptive, materials, moving) do with their
array arguments, function by function and form by form, against a table recorded at the commit before the numpy and device forms
of a query were given one body: per case the exception class AND the whole message, or "accepted"; per public name its signature
and docstring.  The table is what says that folding the two forms moved neither the set of accepted arguments nor a wording.

Every single-call query has one valid call on a 2 x 3 image (``upsample``: scale 2 onto 2 x 4; ``svgf``, ``denoise``: two levels, so
that ``temp`` is an operand).  From it the cases are derived per array parameter, outputs included:

    rejected   f64, swap (int32 for float32 and the reverse), trailing (an extent of 2 where 3 is wanted), longer (one pixel too
               many), lastdim (the last dimension not contiguous), transposed (the leading dimensions do not advance by one pixel
               stride), byteoffset (numpy: strides that are no whole words), none (where the plane is required); numpy and cpu (a
               numpy array and a CPU tensor given to the device form), torch (a CPU tensor given to the numpy form)
    accepted   valid (every optional plane None), all (every optional plane and output given), record (a column range of wider
               records: ``records["color"]`` and the views of ``PrimarySurfaces``), field (numpy: a field of a structured array),
               flat and image (the same pixels as (n, width) and as (rows, cols, width)), and the False forms of ``variance``,
               ``variance_out`` and ``clamped``

"rejected" and "accepted" above say what the ways were written for; what a case does is whatever the record holds — a strided
view of a one-word plane is a plane like any other — and the test asserts only that it is still that.  The frame-level compositions
(denoise_frame, the filter_frames, History.push, render_upsampled, render_pass, render_adaptive, ...) are not cases: they hand
their arrays to the functions recorded here.

golden/image_argument_checks.json was written by record() (python tests/test_image_argument_checks.py cpu|gpu FILE) at that
commit, never from the code under test.  A trailing "*" on a result marks a case after which the library's last-error text had
changed: the C side spoke.  It is part of what is compared, so a case that was refused before C must still be refused before C.

The numpy forms need no device, and neither do the device-form cases whose first checked operand is a numpy array, a CPU tensor or
None: those run unmarked, the second kind with CPU tensors standing in for the operands that are never reached ("@cpu").  The
numpy forms of ``materials`` and ``film.camera_rays_offset_numpy`` are host-buffer conveniences of the device library and run with
the device cases.
"""
import ctypes as C
import inspect
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import _capi, adaptive, denoise, film, materials, moving, rectify, svgf, temporal, upsample

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = Path(__file__).resolve().parent / "golden" / "image_argument_checks.json"
MODULES = {m.__name__.rsplit(".", 1)[1]: m for m in (film, denoise, temporal, svgf, rectify, upsample, adaptive, materials, moving)}
ROWS, COLS, N = 2, 3, 6


# ---- operands: (dtype, shape, width, data) — a dtype by name or a numpy record dtype; width: the trailing extent that is one pixel ----
def op(dtype, shape, width=1, data=None):
    return (dtype, tuple(shape), width, data)


F3, F2, F1, I1 = op("float32", (ROWS, COLS, 3), 3), op("float32", (ROWS, COLS, 2), 2), op("float32", (ROWS, COLS)), op("int32", (ROWS, COLS))
HISTORY = {"numpy": op(temporal.HISTORY_DTYPE, (ROWS, COLS)), "cuda": op("int32", (N, 8), 8)}
BOX = {"numpy": op(rectify.BOX_DTYPE, (ROWS, COLS)), "cuda": op("float32", (N, 8), 8)}
LIST = {"sample_list.start": op("int32", (N + 1,), 1, np.arange(N + 1)), "sample_list.pixel": op("int32", (N,), 1, np.arange(N)),
        "sample_list.sample": op("int32", (N,)), "sample_list.total": op("int32", (2,), 1, np.full(2, N))}
LIST_OUT = {"out." + k.split(".")[1]: v for k, v in LIST.items()}


def valid_array(spec):
    dtype, shape, _, data = spec
    a = np.zeros(shape, dtype=dtype)
    if data is not None:
        a[...] = data
    return a


def variant(spec, how, numpy_form):
    """(base array, view of it) of ``spec``'s operand made in one way; None when the way does not apply"""
    dtype, shape, w, _ = spec
    a = valid_array(spec)
    record = not isinstance(dtype, str)
    pixels = shape[:-1] if w > 1 else shape
    tail = (w,) if w > 1 else ()
    same = lambda t: t  # noqa: E731

    def widened(extent, take):
        """``a`` inside an array whose last dimension has ``extent`` elements, as the view ``take`` of it"""
        base = np.zeros(a.shape[:-1] + (extent,), dtype=a.dtype)
        take(base)[...] = a
        return base, take

    if how == "valid":
        return a, same
    if how == "f64":
        return np.zeros(shape, dtype=np.float64), same
    if how == "swap":
        if record:
            return np.zeros(shape + (8,), dtype=np.int32), same
        return a.astype({"float32": "int32", "int32": "float32", "uint8": "int32"}[dtype]), same
    if how == "trailing":
        return (a[..., :w - 1].copy(), same) if w > 1 else None
    if how == "longer":
        return np.concatenate([a.reshape((-1,) + tail), a.reshape((-1,) + tail)[:1]]), same
    if how == "lastdim":
        return None if record else widened(2 * a.shape[-1], lambda t: t[..., ::2])
    if how == "transposed":
        return (np.ascontiguousarray(a.swapaxes(0, 1)), lambda t: t.swapaxes(0, 1)) if a.ndim >= 2 else None
    if how == "byteoffset":
        if not numpy_form:
            return None
        base = np.zeros(pixels, dtype=[("pad", "u1"), ("v", a.dtype, tail)])
        base["v"] = a
        return base, lambda t: t["v"]
    if how == "record":
        if record:
            return None
        if w > 1:
            return widened(w + 5, lambda t: t[..., 2:2 + w])
        base = np.zeros(a.shape + (6,), dtype=a.dtype)
        base[..., 2] = a
        return base, lambda t: t[..., 2]
    if how == "field":
        if not numpy_form or record:
            return None
        base = np.zeros(pixels, dtype=[("a", "<f4", (2,)), ("v", a.dtype, tail), ("b", "<u4", (3,))])
        base["v"] = a
        return base, lambda t: t["v"]
    if how == "flat":
        return (a.reshape((-1,) + tail), same) if len(pixels) > 1 else None
    if how == "image":
        return (a.reshape((ROWS, COLS) + tail), same) if len(pixels) == 1 and pixels[0] == N else None
    raise KeyError(how)


WAYS = ("f64", "swap", "trailing", "longer", "lastdim", "transposed", "byteoffset", "record", "field", "flat", "image")


class Context:
    """The operands every case is built from, made once per device ("cpu": no device, CPU tensors stand in)."""

    def __init__(self, device):
        self.device, self.gpu = device, device == "cuda"
        self.camera, self.frame = rt.reference_camera(), rt.Frame.full(COLS, ROWS, 1)
        self.world = rt.reference_world()
        self.scene = None
        self.torch = None
        if self.gpu:
            self.need_torch()

    def need_torch(self):
        if self.torch is None:
            import torch

            self.torch = torch
            if self.gpu:
                self.scene = rt.Scene(self.world)
                moving.keep_positions(self.scene)
        return self.torch

    def tensor(self, made, device=None):
        """a torch tensor of ``variant``'s (base, view): the base goes to the device whole, the view is taken there"""
        torch = self.need_torch()
        base, view = made
        if base.dtype.names is not None:  # a record array has no tensor: its words
            base = base.view(np.int32).reshape(base.shape + (-1,))
        return view(torch.from_numpy(base).to(device or self.device))

    def film(self, form):
        if form == "numpy":
            return film.Film(ROWS, COLS, device="cpu")
        if self.gpu:
            return film.Film(ROWS, COLS, device="cuda")
        f = film.Film.__new__(film.Film)  # without a device: a stand-in whose planes are never reached
        f.rows, f.cols, f.device, f.filter, f.radius = ROWS, COLS, "cuda", 1, 1.0
        f.sum, f.weight = self.tensor((np.zeros((ROWS, COLS, 3), np.float32), lambda t: t)), self.tensor((np.zeros((ROWS, COLS), np.float32), lambda t: t))
        return f


def _sample_list(start=None, pixel=None, sample=None, total=None):
    return adaptive.SampleList(start, pixel, sample, total, N, N)


def functions(c):
    """name -> per form ("numpy", "cuda"): (callable, fixed keywords, operands in the order they are checked, required, nested
    builders, whether the numpy form needs the device library)"""
    cam, fr = c.camera, c.frame
    tg = {"current": temporal.Guides, "previous": temporal.Guides}
    ug = {"low": upsample.Guides, "full": upsample.Guides}
    sl = {"sample_list": _sample_list, "out": _sample_list}
    planes = dict(normal=F3, position=F3, albedo=F3, valid=I1)
    pairs = lambda prefixes, fields: {f"{p}.{k}": v for p in prefixes for k, v in fields.items()}  # noqa: E731
    tplanes = pairs(("current", "previous"), dict(normal=F3, position=F3, object=I1, valid=I1))
    lo3, lo1 = op("float32", (1, 2, 3), 3), op("int32", (1, 2))
    hi3, hi1 = op("float32", (2, 4, 3), 3), op("int32", (2, 4))
    uplanes = {**pairs(("low",), dict(normal=lo3, position=lo3, albedo=lo3, valid=lo1, object=lo1)),
               **pairs(("full",), dict(normal=hi3, position=hi3, albedo=hi3, valid=hi1, object=hi1))}
    size = dict(rows=ROWS, cols=COLS)
    two = dict(size, levels=2)
    scene = lambda: c.scene  # noqa: E731 — made with the first device case
    nt, ns = int(c.world.desc().n_triangles), int(c.world.desc().n_spheres)
    ones = np.ones(N)

    def both(numpy_fn, cuda_fn, fixed, operands, required, outputs, nested=None, numpy_fixed=None, cuda_fixed=None, numpy_device=False):
        pick = lambda form: {k: (v[form] if isinstance(v, dict) else v) for k, v in operands.items() if not isinstance(v, dict) or form in v}  # noqa: E731
        table = {}
        if numpy_fn is not None:
            table["numpy"] = (numpy_fn, {**fixed, **(numpy_fixed or {})}, pick("numpy"), required, nested or {}, numpy_device)
        if cuda_fn is not None:
            out = {k: (v["cuda"] if isinstance(v, dict) else v) for k, v in outputs.items()}
            table["cuda"] = (cuda_fn, {**fixed, **(cuda_fixed or {})}, {**pick("cuda"), **out}, required, nested or {}, False)
        return table

    return {
        "denoise.atrous": both(denoise.atrous_numpy, denoise.atrous, two, dict(color=F3, **planes), ("color",), dict(out=F3, temp=F3)),
        "temporal.motion": both(temporal.motion_numpy, temporal.motion, dict(camera=cam, frame=fr), dict(position=F3, valid=I1), ("position",), dict(out=F2)),
        "temporal.accumulate": both(temporal.accumulate_numpy, temporal.accumulate, size, dict(color=F3, motion=F2, history=HISTORY, **tplanes),
                                    ("color", "motion", "history"), dict(out=HISTORY["cuda"], variance=F1), tg),
        "svgf.variance": both(svgf.variance_numpy, svgf.variance, size, dict(history=HISTORY, normal=F3, position=F3, valid=I1), ("history",), dict(out=F1)),
        "svgf.atrous": both(svgf.atrous_numpy, svgf.atrous, two, dict(color=F3, variance=F1, **planes), ("color", "variance"),
                            dict(out=F3, variance_out=F1, temp=op("float32", (4 * N,)))),
        "rectify.bounds": both(rectify.bounds_numpy, rectify.bounds, size, dict(color=F3, object=I1, valid=I1), ("color",), dict(out=BOX["cuda"])),
        "rectify.accumulate_bounded": both(rectify.accumulate_bounded_numpy, rectify.accumulate_bounded, size,
                                           dict(color=F3, motion=F2, history=HISTORY, box=BOX, **tplanes), ("color", "motion", "history", "box"),
                                           dict(out=HISTORY["cuda"], variance=F1, clamped=I1), tg),
        "rectify.feedback": both(rectify.feedback_numpy, rectify.feedback, size, dict(color=F3, valid=I1, history=HISTORY), ("color", "history"), {}),
        "upsample.guided": both(upsample.guided_numpy, upsample.guided, dict(rows=2, cols=4, scale=2, demodulate=False), dict(color_lo=lo3, **uplanes),
                                ("color_lo",), dict(out=hi3), ug),
        "adaptive.budget": both(adaptive.budget_numpy, adaptive.budget, {}, dict(mean=F1, variance=F1, count=I1, valid=I1), ("mean", "variance"),
                                dict(out=op("int32", (N,)))),
        "adaptive.sample_list": both(adaptive.sample_list_numpy, adaptive.sample_list, {}, dict(counts=op("int32", (N,), 1, ones), first=op("int32", (N,))),
                                     ("counts",), dict(LIST_OUT, temp=op("uint8", (4096,))), sl, cuda_fixed=dict(capacity=N)),
        "adaptive.offsets_listed": both(adaptive.offsets_listed_numpy, adaptive.offsets_listed, dict(frame=fr), dict(LIST), tuple(LIST),
                                        dict(out=op("float32", (N, 2), 2)), sl),
        "adaptive.camera_rays_listed": both(adaptive.camera_rays_listed_numpy, adaptive.camera_rays_listed, dict(camera=cam, frame=fr),
                                            dict(LIST, offsets=op("float32", (N, 2), 2)), tuple(LIST) + ("offsets",), dict(out=op("int32", (N, 11), 11)), sl),
        "adaptive.splat_listed": both(adaptive.splat_listed_numpy, adaptive.splat_listed, dict(film="film"),
                                      dict(LIST, samples=op("float32", (N, 3), 3), offsets=op("float32", (N, 2), 2), valid=op("uint8", (N,), 1, ones)),
                                      tuple(LIST) + ("samples", "offsets"), {}, sl),
        "film.offsets": both(None, film.offsets, dict(frame=fr, spp=1), {}, (), dict(out=op("float32", (1, N, 2), 2))),
        "film.camera_rays_offset": both(film.camera_rays_offset_numpy, film.camera_rays_offset, dict(camera=cam, frame=fr),
                                        dict(offsets=op("float32", (1, N, 2), 2)), ("offsets",),
                                        dict(out=op("int32", (N, 11), 11)), numpy_device=True),
        "film.Film.splat": both("splat", "splat", {}, dict(samples=op("float32", (1, N, 3), 3), offsets=op("float32", (1, N, 2), 2),
                                                           valid=op("uint8", (1, N), 1, ones)), ("samples", "offsets"), {}),
        "materials.material_hits": both(materials.material_hits_numpy, materials.material_hits, dict(scene=scene), dict(hits=op("int32", (N, 13), 13)), ("hits",),
                                        dict(out=op("int32", (N, 18), 18)), numpy_device=True),
        "materials.probe_surfaces": both(materials.probe_surfaces_numpy, materials.probe_surfaces, {},
                                         dict(surfaces=op("int32", (N, 18), 18), view=op("float32", (N, 3), 3), light_dirs=op("float32", (1, N, 3), 3)),
                                         ("surfaces", "view", "light_dirs"), dict(out_diffuse=op("float32", (1, N, 3), 3), out_specular=op("float32", (1, N, 3), 3)),
                                         numpy_device=True),
        "moving.previous_positions": both(moving.previous_positions_numpy, moving.previous_positions, {},
                                          dict(was_triangles={"numpy": op("float32", (nt, 9), 9)}, was_spheres={"numpy": op("float32", (ns, 4), 4)},
                                               hits=op("int32", (N, 13), 13)), ("was_triangles", "was_spheres", "hits"), dict(out=op("float32", (N, 3), 3)),
                                          numpy_fixed=dict(world_or_desc=c.world), cuda_fixed=dict(scene=scene)),
    }


NUMPY_NAMES = {"film.camera_rays_offset": {"offsets": "offsets_np"}, "materials.material_hits": {"hits": "hits_np"},
               "materials.probe_surfaces": {"surfaces": "surfaces_np"}}
# the False forms of the outputs: case -> (function, form, keywords)
SCALARS = {
    "variance-False": ("temporal.accumulate", dict(variance=False)),
    "variance-False ": ("rectify.accumulate_bounded", dict(variance=False)),
    "clamped-False": ("rectify.accumulate_bounded", dict(clamped=False)),
    "variance_out-False": ("svgf.atrous", dict(variance_out=False)),
}


def cases(c, which):
    """(id, thunk) for every case of one section, in a fixed order: "host" (numpy forms, no device), "first" (device forms, the first
    operand wrong, no device) or "device" (the other device-form cases and the numpy forms that go through the device library)"""
    out = []
    for name, forms in functions(c).items():
        for form, (fn, fixed, operands, required, nested, numpy_device) in forms.items():
            numpy_form = form == "numpy"
            section = ("device" if numpy_device else "host") if numpy_form else "device"
            if which == "first":
                if numpy_form or not operands:
                    continue
            elif section != which:
                continue
            rename = NUMPY_NAMES.get(name, {}) if numpy_form else {}

            def give(spec, how, numpy_form=numpy_form):
                made = variant(spec, how, numpy_form)
                if made is None:
                    return None
                return (lambda: made[1](made[0])) if numpy_form else (lambda: c.tensor(made))

            def call(given, fn=fn, fixed=fixed, nested=nested, form=form, rename=rename, required=required):
                def run():
                    kw = {k: (v() if callable(v) and k == "scene" else v) for k, v in fixed.items()}
                    if kw.get("film") == "film" or isinstance(fn, str):
                        target = c.film(form)
                        if isinstance(fn, str):
                            kw.pop("film", None)
                    groups = {}
                    for k, v in given.items():
                        v = v() if callable(v) else v
                        if "." in k:
                            groups.setdefault(k.split(".")[0], {})[k.split(".")[1]] = v
                        else:
                            kw[rename.get(k, k)] = v
                    for g, parts in groups.items():
                        kw[g] = nested[g](**parts)
                    if isinstance(fn, str):
                        return getattr(target, fn)(**kw)
                    if kw.get("film") == "film":
                        kw["film"] = target
                    return fn(**kw)
                return run

            valid = {k: give(v, "valid") for k, v in operands.items()}
            need = {k: valid[k] for k in required if k in operands}
            label = f"{name}:{form}"
            if which == "first":
                first = next(iter(operands))
                stand_in = lambda spec: (lambda: c.tensor(variant(spec, "valid", False), device="cpu"))  # noqa: E731
                rest = {k: stand_in(operands[k]) for k in required if k in operands}
                made = variant(operands[first], "valid", False)
                ways = [("numpy", lambda made=made: made[0]), ("cpu", rest.get(first, stand_in(operands[first])))] + ([("none", None)] if first in required else [])
                for how, value in ways:
                    out.append((f"{label}-{first}-{how}@cpu", call({**rest, first: value})))
                continue
            out.append((f"{label}-valid", call(need)))
            out.append((f"{label}-all", call(valid)))
            for p, spec in operands.items():
                for how in WAYS:
                    value = give(spec, how)
                    if value is not None:
                        out.append((f"{label}-{p}-{how}", call({**valid, p: value})))
                if p in required:
                    out.append((f"{label}-{p}-none", call({**valid, p: None})))
                made = variant(spec, "valid", False)
                if numpy_form:
                    out.append((f"{label}-{p}-torch", call({**valid, p: lambda made=made: c.tensor(made, device="cpu")})))
                else:
                    out.append((f"{label}-{p}-numpy", call({**valid, p: lambda made=made: made[0]})))
                    out.append((f"{label}-{p}-cpu", call({**valid, p: lambda made=made: c.tensor(made, device="cpu")})))
            for case, (function, keywords) in SCALARS.items():
                if function == name:
                    value = next(iter(keywords.values()))
                    if numpy_form and next(iter(keywords)) == "clamped":
                        continue  # the numpy form has no such keyword
                    out.append((f"{name}:{form}-{case.strip()}", call({**valid, **{k: value for k in keywords}})))
    return out


def outcome(thunk, numpy_form):
    """("accepted" or the exception's class name, with "*" when the library's last-error text changed), the message"""
    if numpy_form:
        lib = _capi.host_lib()
        lib.rt_film_offsets_host(C.byref(rt.Frame.full(1, 1, 1)), 1, 0, 0, None)  # refused: leaves a text that no other call writes
        last = lib.rt_host_last_error
    else:
        lib = _capi.amd_lib()
        lib.rt_set_option(b"RT_AMD_NO_SUCH_SWITCH", None)  # the same for the device library
        last = lib.rt_last_error
    before = last()
    try:
        thunk()
        result, message = "accepted", ""
    except Exception as e:  # noqa: BLE001 — the class is the result
        result, message = type(e).__name__, str(e)
    return result + ("*" if last() != before else ""), message


def host_side(case):
    """does the case call librt_host.so (its last-error text is the one to watch)"""
    return ":numpy" in case and not functions_needing_device(case)


def functions_needing_device(case):
    return case.split(":")[0] in ("film.camera_rays_offset", "materials.material_hits", "materials.probe_surfaces")


def signatures():
    """name -> [signature, docstring] of every public callable of the nine modules and of their classes' public methods"""
    table = {}
    for module_name, module in MODULES.items():
        for name in module.__all__:
            obj = getattr(module, name)
            if not callable(obj):
                continue
            table[f"{module_name}.{name}"] = [str(inspect.signature(obj)), obj.__doc__]
            if inspect.isclass(obj):
                for member, value in sorted(vars(obj).items()):
                    if member.startswith("_") and member != "__init__":
                        continue
                    value = value.__func__ if isinstance(value, (classmethod, staticmethod)) else value
                    if inspect.isfunction(value):
                        table[f"{module_name}.{name}.{member}"] = [str(inspect.signature(value)), value.__doc__]
    return table


def record(device, path):
    """write this device's sections of the table into ``path`` (the other sections of the file are kept)"""
    path = Path(path)
    table = json.loads(path.read_text()) if path.exists() else {}
    c = Context({"gpu": "cuda", "cpu": "cpu"}[device])
    if device == "cpu":
        table["signatures"] = signatures()
    for section in {"cpu": ("host", "first"), "gpu": ("device",)}[device]:
        table[section] = {case: list(outcome(thunk, host_side(case))) for case, thunk in cases(c, section)}
    if c.gpu:
        c.torch.cuda.synchronize()
    path.write_text(json.dumps(table, indent=0, sort_keys=True) + "\n")


EXPECT = json.loads(GOLDEN.read_text()) if GOLDEN.exists() else {"signatures": {}, "host": {}, "first": {}, "device": {}}  # absent only while recording
_contexts = {}


def context(device, section):
    if device not in _contexts:
        _contexts[device] = Context(device)
        _contexts[device].cases = {}
    c = _contexts[device]
    if section not in c.cases:
        c.cases[section] = dict(cases(c, section))
    return c


def check_function(device, section, name):
    """every case of one function, the accepted ones first: one parametrised test per function keeps the file at a few seconds"""
    c = context(device, section)
    want = EXPECT[section]
    mine = [case for case in c.cases[section] if case.split(":")[0] == name]
    assert mine
    failures = []
    for case in sorted(mine, key=lambda case: want[case][0] != "accepted"):
        got = list(outcome(c.cases[section][case], host_side(case)))
        print(f"{case}: recorded {want[case]}, now {got}")
        if got != want[case]:
            failures.append(f"{case}: {got}, recorded {want[case]}")
    if c.gpu:
        c.torch.cuda.synchronize()
    assert not failures, "\n".join(failures)


def names_of(section):
    return sorted({case.split(":")[0] for case in EXPECT.get(section, {})})  # a missing section fails the cover tests


def test_signatures_and_docstrings_are_the_recorded_ones():
    now = signatures()
    assert sorted(now) == sorted(EXPECT["signatures"])
    for name, want in EXPECT["signatures"].items():
        assert now[name] == want, name


@pytest.mark.parametrize("section", ["host", "first"])
def test_the_record_covers_every_case_that_needs_no_device(section):
    assert sorted(context("cpu", section).cases[section]) == sorted(EXPECT[section])


@pytest.mark.parametrize("name", names_of("host"))
def test_numpy_form_of(name):
    check_function("cpu", "host", name)


@pytest.mark.parametrize("name", names_of("first"))
def test_device_form_refuses_its_first_operand_without_a_device(name):
    check_function("cpu", "first", name)


@pytest.mark.gpu
def test_the_record_covers_every_device_case():
    assert sorted(context("cuda", "device").cases["device"]) == sorted(EXPECT["device"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", names_of("device"))
def test_device_form_of(name):
    check_function("cuda", "device", name)


def test_the_numpy_forms_load_neither_torch_nor_the_device_library():
    """one numpy form of each module on a 2 x 3 image, in a fresh interpreter.  ``materials`` has none that is free of the device
    library (its numpy forms are that library's host-buffer conveniences), so importing it is all that is asked of it."""
    code = f"""
import sys
sys.path.insert(0, {str(ROOT)!r})
import numpy as np
import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import adaptive, denoise, film, materials, moving, rectify, svgf, temporal, upsample
f3, f2, f1 = np.zeros((2, 3, 3), np.float32), np.zeros((2, 3, 2), np.float32), np.zeros((2, 3), np.float32)
frame, history = rt.Frame.full(3, 2, 1), np.zeros((2, 3), temporal.HISTORY_DTYPE)
film.offsets_numpy(frame, 1)
film.Film(2, 3).splat(np.zeros((1, 6, 3), np.float32), np.zeros((1, 6, 2), np.float32))
denoise.atrous_numpy(f3, 2, 3, levels=2)
temporal.motion_numpy(f3, rt.reference_camera(), frame)
temporal.accumulate_numpy(f3, f2, 2, 3, history)
svgf.variance_numpy(history, 2, 3)
svgf.atrous_numpy(f3, f1, 2, 3, levels=2)
rectify.bounds_numpy(f3, 2, 3)
rectify.feedback_numpy(f3, history, 2, 3)
upsample.guided_numpy(np.zeros((1, 2, 3), np.float32), 2, 3, demodulate=False)
adaptive.budget_numpy(f1, f1)
adaptive.offsets_listed_numpy(frame, adaptive.sample_list_numpy(np.ones(6, np.uint32)))
world = rt.reference_world()
moving.previous_positions_numpy(world, np.zeros((world.desc().n_triangles, 9), np.float32), np.zeros((world.desc().n_spheres, 4), np.float32),
                                np.zeros((6, 13), np.int32))
assert 'torch' not in sys.modules
assert 'librt_amd' not in open('/proc/self/maps').read()
assert 'librt_host' in open('/proc/self/maps').read()
"""
    done = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr


if __name__ == "__main__":
    record(sys.argv[1], sys.argv[2])
