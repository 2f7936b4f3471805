"""No image query reads or writes outside its operands (tests/_guard_support.py has the harness and why the value tests cannot see it).

One table, ROWS: an entry point, a builder of guarded operands, the call through the Python wrapper with every output and scratch
given, and the expected result from the CPU definition on compact copies.  Every row runs in the numpy form — the ``_cpu`` entry points
of librt_host.so, no GPU — and, marked ``gpu``, on the device: each kernel form, the unit's RT_AMD_DIAG_*_MAX_GROUPS unset and at 1
(one workgroup strides every tile), at the image sizes where the tile logic can go wrong.  A row is run three times with three poisons
around and between its operands; the results must not move.

The case data is the existing suites' (_film_support ... _motion_support).  Where an entry point cannot take what the table's
columns name, the row says so: rt_denoise_atrous takes its colour compact only and refuses out == color (its guides are the record
views); rt_camera_rays_offset has no form in librt_host.so (its expected rays are rt_camera_rays_listed_cpu's on a list that names
every sample); the resolve has no ``out=`` in Python, so its row calls the C entry point."""
import ctypes as C
import functools

import numpy as np
import pytest

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import _capi, adaptive, bloom, denoise, film, moving, rectify, svgf, temporal, upsample
from homework_18_graphics_raytracer_amd._forms import NUMPY
import _adaptive_support as AS
import _bloom_support as BS
import _denoise_support as DS
import _film_support as FS
import _guard_support as G
import _motion_support as MS
import _rectify_support as RS
import _svgf_support as SS
import _temporal_support as TS
import _upsample_support as US

F32, U32 = np.float32, np.uint32
SIZES = [(1, 1), (1, 17), (17, 1), (15, 15), (16, 16), (17, 17), (31, 18), (33, 65)]
LIST_SIZES = [1, 255, 256, 257, 65537]  # 65537: 257 steps, so the scan takes a second round of one entry
SEED = 0x9E3779B9
HIT_WORDS, SURFACE_WORDS, POSITION_AT, OBJECT_AT, NORMAL_AT, ALBEDO_AT, VALID_AT = 13, 18, 3, 2, 14, 3, 17  # primary_surfaces' views
HISTORY, BOX = temporal._HISTORY, rectify._BOX
RECORD_WORDS = 8  # colour inside history records


def ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def frame_of(rows, cols):
    return rt.Frame.full(cols, rows, 0)


def camera():
    return rt.reference_camera()


def shaped(a, *shape):
    """a view of a contiguous array or tensor in another shape"""
    return a.reshape(shape)


def frozen(d):
    for a in d.values():
        a.setflags(write=False)
    return d


class Row:
    """entry: the C entry point the row guards; unit: its RT_AMD_DIAG_<unit>_MAX_GROUPS; form_option: its kernel-form switch or None;
    build(case, size, *variant) -> operands; call(form, operands, size, *variant); want(size, *variant) -> {operand: expected};
    same: {operand: comparison} where a case allows "both NaN"; numpy: False where librt_host.so has no form of the entry"""

    def __init__(self, entry, unit, build, call, want, variants=((),), sizes=SIZES, form_option=None, same=None, numpy=True):
        self.entry, self.cap_option, self.build, self.call, self.want = entry, unit and f"RT_AMD_DIAG_{unit}_MAX_GROUPS", build, call, want
        self.variants, self.sizes, self.form_option, self.same, self.numpy = list(variants), sizes, form_option, same, numpy

    def run(self, form, variant):
        for size in self.sizes:
            G.run_poisoned(lambda case: self.build(case, size, *variant), lambda ops: self.call(form, ops, size, *variant),
                           self.want(size, *variant), form, self.same)


def guide_planes(case, prefix, strided, normal=None, position=None, albedo=None, valid=None, obj=None):
    """the guide planes that are given, compact or as the fields of 13- and 18-word records where primary_surfaces has them"""
    spec = dict(normal=(normal, SURFACE_WORDS, NORMAL_AT, 3), position=(position, HIT_WORDS, POSITION_AT, 3), albedo=(albedo, SURFACE_WORDS, ALBEDO_AT, 3),
                valid=(valid, SURFACE_WORDS, VALID_AT, 1), object=(obj, HIT_WORDS, OBJECT_AT, 1))
    out = {}
    for name, (data, words, at, width) in spec.items():
        if data is None:
            out[name] = None
        elif strided:
            out[name] = case.field(prefix + name, "in", words, at, data=data, width=width)
        else:
            out[name] = case.compact(prefix + name, "in", data=data)
    return out


# ---- film ----

@functools.lru_cache(maxsize=None)
def film_case(rows, cols):
    samples, valid, offsets, total, weight = FS.case_data(rows, cols, 4)
    weight = weight.copy()
    weight[0, 0] = 0.0  # the resolve's black pixel
    weight.setflags(write=False)
    return samples, valid, offsets, total, weight


def b_offsets(case, size):
    return dict(out=case.compact("out", "out", shape=(4, size[0] * size[1], 2)))


def c_offsets(form, o, size):
    frame = frame_of(*size)
    if form == "cuda":
        film.offsets(frame, 4, "stratified", SEED, out=o["out"])
    else:
        _capi.check_host(_capi.host_lib().rt_film_offsets_host(C.byref(frame), 4, film.PATTERNS["stratified"], SEED, ptr(o["out"])))


@functools.lru_cache(maxsize=None)
def w_offsets(size):
    return frozen(dict(out=film.offsets_numpy(frame_of(*size), 4, "stratified", SEED)))


def b_rays_offset(case, size):
    n = size[0] * size[1]
    return dict(offsets=case.compact("offsets", "in", data=film_case(*size)[2]), out=case.compact("out", "out", shape=(4 * n, 11), dtype=np.int32))


def c_rays_offset(form, o, size):
    film.camera_rays_offset(camera(), frame_of(*size), o["offsets"], out=o["out"])


@functools.lru_cache(maxsize=None)
def w_rays_offset(size):
    """rt_camera_rays_listed_cpu on the list that names sample s of pixel i as record s * n + i: "each film.camera_rays_offset's record
    of its pixel" (adaptive.camera_rays_listed_numpy)"""
    n = size[0] * size[1]
    sl = adaptive.SampleList(np.zeros(n + 1, dtype=U32), np.tile(np.arange(n, dtype=U32), 4), np.zeros(4 * n, dtype=U32), np.array([4 * n, 4 * n], dtype=U32),
                             4 * n, n)
    rays = adaptive.camera_rays_listed_numpy(camera(), frame_of(*size), np.array(film_case(*size)[2]).reshape(-1, 2), sl)
    return frozen(dict(out=rays.view(np.int32).reshape(-1, 11)))


FILTER_OF = {0.5: "box", 1.0: "tent", 2.0: "mitchell", 3.0: "mitchell", 4.0: "tent"}  # reach 1 .. 5


def b_splat(case, size, radius):
    samples, valid, offsets, total, weight = film_case(*size)
    return dict(samples=case.compact("samples", "in", data=samples), valid=case.compact("valid", "in", data=valid),
                offsets=case.compact("offsets", "in", data=offsets), sum=case.compact("sum", "inout", data=total),
                weight=case.compact("weight", "inout", data=weight))


def film_on(form, o, size, name, radius):
    f = film.Film(size[0], size[1], name, radius, device="cuda" if form == "cuda" else "cpu")
    f.sum, f.weight = o["sum"], o["weight"]
    return f


def c_splat(form, o, size, radius):
    film_on(form, o, size, FILTER_OF[radius], radius).splat(o["samples"], o["offsets"], o["valid"])


@functools.lru_cache(maxsize=None)
def w_splat(size, radius):
    samples, valid, offsets, total, weight = film_case(*size)
    s, w = FS.host_splat(size[0], size[1], samples, valid, offsets, FILTER_OF[radius], radius, total, weight)
    return frozen(dict(sum=s, weight=w))


def c_accumulate(form, o, size, radius=None):
    acc = rt.PhotonAccumulator(size[0], size[1], "cuda" if form == "cuda" else "cpu")
    acc.sum, acc.weight = o["sum"], o["weight"]
    acc.accumulate(shaped(o["samples"], 4, size[0], size[1], 3), shaped(o["valid"], 4, size[0], size[1]))


@functools.lru_cache(maxsize=None)
def w_accumulate(size, radius=None):
    samples, valid, _, total, weight = film_case(*size)
    acc = rt.PhotonAccumulator(size[0], size[1])
    acc.sum[...], acc.weight[...] = total, weight
    acc.accumulate(np.array(samples).reshape(4, size[0], size[1], 3), np.array(valid).reshape(4, size[0], size[1]))
    return frozen(dict(sum=acc.sum, weight=acc.weight))


def b_resolve(case, size):
    _, _, _, total, weight = film_case(*size)
    return dict(sum=case.compact("sum", "in", data=total), weight=case.compact("weight", "in", data=weight),
                out=case.compact("out", "out", shape=(size[0], size[1], 3)))


def c_resolve(form, o, size):
    n = size[0] * size[1]
    if form == "cuda":
        from homework_18_graphics_raytracer_amd._args import _p, _stream_ptr

        _capi.check(_capi.amd_lib().rt_accumulator_resolve_device(_p(o["sum"]), _p(o["weight"]), n, _p(o["out"]), _stream_ptr(None)))
    else:
        _capi.host_lib().rt_accumulator_resolve(ptr(o["sum"]), ptr(o["weight"]), n, ptr(o["out"]))


@functools.lru_cache(maxsize=None)
def w_resolve(size):
    f = film.Film(size[0], size[1])
    f.sum[...], f.weight[...] = film_case(*size)[3:5]
    return frozen(dict(out=f.resolve()))


# ---- adaptive ----

def b_budget(case, size):
    mean, variance, count, valid = AS.budget_case(size[0] * size[1])
    return dict(mean=case.field("mean", "in", RECORD_WORDS, 3, data=mean), variance=case.field("variance", "in", RECORD_WORDS, 4, data=variance),
                count=case.compact("count", "in", data=count), valid=case.compact("valid", "in", data=valid),
                out=case.compact("out", "out", shape=(size[0] * size[1],), dtype=U32))


def c_budget(form, o, size):
    n = size[0] * size[1]
    if form == "cuda":
        adaptive.budget(o["mean"], o["variance"], o["count"], o["valid"], out=o["out"])
    else:
        adaptive._budget(NUMPY, n, NUMPY.plane(o["mean"], "mean", "f", n, 1), NUMPY.plane(o["variance"], "variance", "f", n, 1), o["count"], o["valid"],
                         adaptive._budget_params(adaptive.GAIN, adaptive.EPSILON, 1, adaptive.SAMPLE_MAX), (n,), "uint32", None, o["out"])


@functools.lru_cache(maxsize=None)
def w_budget(size):
    return frozen(dict(out=adaptive.budget_numpy(*AS.budget_case(size[0] * size[1]))))


@functools.lru_cache(maxsize=None)
def list_case(n, room, with_first):
    counts = AS.counts_case(n, "random")
    total = int(np.minimum(counts, AS.SAMPLE_MAX).sum(dtype=np.uint64))
    capacity = {"total": total, "below": max(total - 1, 0), "zero": 0}[room]
    first = np.random.default_rng(n).integers(0, 1000, n).astype(U32) if with_first else None
    return counts, capacity, first


def b_list(case, n, room, with_first):
    counts, capacity, first = list_case(n, room, with_first)
    o = dict(counts=case.compact("counts", "in", data=counts), first=None if first is None else case.compact("first", "inout", data=first),
             start=case.compact("start", "out", shape=(n + 1,), dtype=U32), pixel=case.compact("pixel", "out", shape=(capacity,), dtype=U32),
             sample=case.compact("sample", "out", shape=(capacity,), dtype=U32), total=case.compact("total", "out", shape=(2,), dtype=U32))
    if case.form == "cuda":
        need = adaptive.list_temp_bytes(n)
        assert need % 4 == 0
        o["temp"] = case.temp("temp", need // 4, dtype=np.uint8)  # exactly list_temp_bytes(n)
    return o


def c_list(form, o, n, room, with_first):
    capacity = list_case(n, room, with_first)[1]
    if form == "cuda":
        adaptive.sample_list(o["counts"], capacity, first=o["first"], out=adaptive.SampleList(o["start"], o["pixel"], o["sample"], o["total"], capacity, n),
                             temp=o["temp"])
    else:
        _capi.check_host(_capi.host_lib().rt_sample_list_cpu(ptr(o["counts"]), n, capacity, ptr(o["first"]), ptr(o["start"]), ptr(o["pixel"]) if capacity else None,
                                                             ptr(o["sample"]) if capacity else None, ptr(o["total"])))


@functools.lru_cache(maxsize=None)
def w_list(n, room, with_first):
    counts, capacity, first = list_case(n, room, with_first)
    first = None if first is None else first.copy()
    sl = adaptive.sample_list_numpy(counts, capacity, first)
    want = dict(start=sl.start, pixel=sl.pixel, sample=sl.sample, total=sl.total)
    if first is not None:
        want["first"] = first
    return frozen(want)


@functools.lru_cache(maxsize=None)
def listed_case(rows, cols, kind):
    """_adaptive_support.splat_case; "last64": its counts with 64 samples in the image's last pixel — the last partial tile"""
    counts, sl, samples, valid, offsets, total, weight = AS.splat_case(rows, cols, 3)
    if kind == "last64":
        counts = counts.copy()
        counts[-1] = AS.SAMPLE_MAX
        sl = adaptive.sample_list_numpy(counts)
        g = np.random.default_rng(rows * 100 + cols)
        samples = g.random((sl.capacity, 3), dtype=F32) * F32(4.0)
        valid = (g.random(sl.capacity) >= 0.25).astype(np.uint8)
        offsets = g.random((sl.capacity, 2), dtype=F32) - F32(0.5)
    return sl, samples, valid, offsets, total, weight


def list_operands(case, sl):
    start, pixel, sample, total = (case.compact(name, "in", data=a) for name, a in (("start", sl.start), ("pixel", sl.pixel), ("sample", sl.sample), ("total", sl.total)))
    return adaptive.SampleList(start, pixel, sample, total, sl.capacity, sl.n)


def b_offsets_listed(case, size):
    sl = listed_case(*size, "random")[0]
    return dict(sl=list_operands(case, sl), out=case.compact("out", "out", shape=(sl.capacity, 2)))


def c_offsets_listed(form, o, size):
    sl, frame = o["sl"], frame_of(*size)
    if form == "cuda":
        adaptive.offsets_listed(frame, sl, "uniform", SEED, out=o["out"])
    else:
        _capi.check_host(_capi.host_lib().rt_film_offsets_listed_cpu(C.byref(frame), film.PATTERNS["uniform"], SEED, ptr(sl.pixel), ptr(sl.sample), ptr(sl.total),
                                                                     sl.capacity, ptr(o["out"])))


@functools.lru_cache(maxsize=None)
def w_offsets_listed(size):
    return frozen(dict(out=adaptive.offsets_listed_numpy(frame_of(*size), listed_case(*size, "random")[0], "uniform", SEED)))


def b_rays_listed(case, size):
    sl, _, _, offsets, _, _ = listed_case(*size, "random")
    return dict(sl=list_operands(case, sl), offsets=case.compact("offsets", "in", data=offsets), out=case.compact("out", "out", shape=(sl.capacity, 11), dtype=np.int32))


def c_rays_listed(form, o, size):
    sl, frame, cam = o["sl"], frame_of(*size), camera()
    if form == "cuda":
        adaptive.camera_rays_listed(cam, frame, o["offsets"], sl, out=o["out"])
    else:
        _capi.check_host(_capi.host_lib().rt_camera_rays_listed_cpu(C.byref(cam), C.byref(frame), ptr(o["offsets"]), ptr(sl.pixel), ptr(sl.total), sl.capacity,
                                                                    ptr(o["out"])))


@functools.lru_cache(maxsize=None)
def w_rays_listed(size):
    sl, _, _, offsets, _, _ = listed_case(*size, "random")
    return frozen(dict(out=adaptive.camera_rays_listed_numpy(camera(), frame_of(*size), offsets, sl).view(np.int32).reshape(-1, 11)))


def b_splat_listed(case, size, kind):
    sl, samples, valid, offsets, total, weight = listed_case(*size, kind)
    return dict(sl=list_operands(case, sl), samples=case.compact("samples", "in", data=samples), valid=case.compact("valid", "in", data=valid),
                offsets=case.compact("offsets", "in", data=offsets), sum=case.compact("sum", "inout", data=total),
                weight=case.compact("weight", "inout", data=weight))


def c_splat_listed(form, o, size, kind):
    adaptive.splat_listed(film_on(form, o, size, "mitchell", 2.0), o["samples"], o["offsets"], o["sl"], o["valid"], AS.SAMPLE_MAX)


@functools.lru_cache(maxsize=None)
def w_splat_listed(size, kind):
    sl, samples, valid, offsets, total, weight = listed_case(*size, kind)
    s, w = AS.host_splat_listed(size[0], size[1], samples, valid, offsets, sl, "mitchell", 2.0, total, weight)
    return frozen(dict(sum=s, weight=w))


# ---- denoise ----

DENOISE_SIGMAS = dict(zip(("sigma_color", "sigma_normal", "sigma_position"), DS.FINITE_SIGMAS))


def b_denoise(case, size, levels, first_level, strided):
    rows, cols = size
    color, normal, position, albedo, valid = DS.case_data(rows, cols)
    o = dict(color=case.compact("color", "in", data=color.reshape(rows, cols, 3)), out=case.compact("out", "out", shape=(rows, cols, 3)),
             temp=shaped(case.temp("temp", rows * cols * 3), rows, cols, 3) if levels >= 2 else None)  # exactly denoise.temp_bytes
    o.update(guide_planes(case, "", strided, normal, position, albedo, valid))
    return o


def c_denoise(form, o, size, levels, first_level, strided):
    guides = {k: o[k] for k in ("normal", "position", "albedo", "valid")}
    if form == "cuda":
        denoise.atrous(o["color"], *size, levels=levels, first_level=first_level, demodulate=True, out=o["out"], temp=o["temp"], **guides, **DENOISE_SIGMAS)
    else:
        denoise._atrous(NUMPY, o["color"], *size, guides["normal"], guides["position"], guides["albedo"], guides["valid"],
                        denoise._params(levels, first_level, *DS.FINITE_SIGMAS, True), o["out"], o["temp"])


@functools.lru_cache(maxsize=None)
def w_denoise(size, levels, first_level, strided):
    color, normal, position, albedo, valid = DS.case_data(*size)
    return frozen(dict(out=denoise.atrous_numpy(color, *size, normal=normal, position=position, albedo=albedo, valid=valid, levels=levels, first_level=first_level,
                                                demodulate=True, **DENOISE_SIGMAS)))


# ---- temporal and rectify ----

@functools.lru_cache(maxsize=None)
def temporal_case(rows, cols):
    color, history, cur, prev = TS.case_data(rows, cols)
    motion = TS.motion_field(rows, cols, "fractional")
    return color, history, cur, prev, motion


def guides_of(planes):
    return dict(normal=planes.normal, position=planes.position, obj=planes.object, valid=planes.valid)


def b_motion(case, size):
    rows, cols = size
    _, _, cur, _, _ = temporal_case(rows, cols)
    position = TS.pixel_positions(camera(), frame_of(rows, cols), np.array([2.0, 7.5, -1.0, 4.0]))
    return dict(position=case.field("position", "in", HIT_WORDS, POSITION_AT, data=position, width=3), valid=case.field("valid", "in", SURFACE_WORDS, VALID_AT, data=cur.valid),
                out=case.compact("out", "out", shape=(rows, cols, 2)))


def c_motion(form, o, size):
    (temporal.motion if form == "cuda" else functools.partial(temporal._motion, NUMPY))(o["position"], camera(), frame_of(*size), o["valid"], out=o["out"])


@functools.lru_cache(maxsize=None)
def w_motion(size):
    position = TS.pixel_positions(camera(), frame_of(*size), np.array([2.0, 7.5, -1.0, 4.0]))
    return frozen(dict(out=temporal.motion_numpy(position, camera(), frame_of(*size), temporal_case(*size)[2].valid)))


def temporal_operands(case, size):
    rows, cols = size
    color, history, cur, prev, motion = temporal_case(rows, cols)
    o = dict(color=case.compact("color", "in", data=color.reshape(rows, cols, 3)), motion=case.compact("motion", "in", data=motion.reshape(rows, cols, 2)),
             history=case.compact("history", "in", data=history.reshape(rows, cols), record=HISTORY), out=case.compact("out", "out", shape=(rows, cols), record=HISTORY),
             variance=case.compact("variance", "out", shape=(rows, cols)))
    g = guide_planes(case, "current.", True, **guides_of(cur))
    o["current"] = temporal.Guides(g["normal"], g["position"], g["object"], g["valid"])
    g = guide_planes(case, "previous.", False, **guides_of(prev))
    o["previous"] = temporal.Guides(g["normal"], g["position"], g["object"], g["valid"])
    return o


def c_accumulate_temporal(form, o, size):
    if form == "cuda":
        temporal.accumulate(o["color"], o["motion"], *size, o["history"], o["current"], o["previous"], out=o["out"], variance=o["variance"], **TS.PARAMS)
    else:
        temporal._accumulate(NUMPY, o["color"], o["motion"], *size, o["history"], o["current"], o["previous"], temporal._params(**TS.PARAMS), o["out"], o["variance"])


def planes_as_guides(p):
    return temporal.Guides(p.normal, p.position, p.object, p.valid)


@functools.lru_cache(maxsize=None)
def w_accumulate_temporal(size):
    color, history, cur, prev, motion = temporal_case(*size)
    out, variance = temporal.accumulate_numpy(color, motion, *size, history, planes_as_guides(cur), planes_as_guides(prev), **TS.PARAMS)
    return frozen(dict(out=out, variance=variance))


BOUNDS_RADII = (1, 3)  # 3: the largest the entry point accepts (_rectify_support.RADII)


def b_bounds(case, size, radius):
    rows, cols = size
    color, obj, valid = RS.case_data(rows, cols)
    return dict(color=case.field("color", "in", RECORD_WORDS, 0, data=color.reshape(rows * cols, 3), width=3), object=case.field("object", "in", HIT_WORDS, OBJECT_AT, data=obj),
                valid=case.compact("valid", "in", data=valid), out=case.compact("out", "out", shape=(rows, cols), record=BOX))


def c_bounds(form, o, size, radius):
    if form == "cuda":
        rectify.bounds(o["color"], *size, object=o["object"], valid=o["valid"], radius=radius, out=o["out"])
    else:
        rectify._bounds(NUMPY, o["color"], *size, o["object"], o["valid"], rectify._bounds_params(rectify.GAMMA, radius), o["out"])


@functools.lru_cache(maxsize=None)
def w_bounds(size, radius):
    color, obj, valid = RS.case_data(*size)
    return frozen(dict(out=rectify.bounds_numpy(color, *size, object=obj, valid=valid, radius=radius)))


def b_bounded(case, size):
    o = temporal_operands(case, size)
    o["box"] = case.compact("box", "in", data=w_bounded_box(size), record=BOX)
    o["clamped"] = case.compact("clamped", "out", shape=size, dtype=U32)
    return o


@functools.lru_cache(maxsize=None)
def w_bounded_box(size):
    return rectify.bounds_numpy(temporal_case(*size)[0], *size, object=temporal_case(*size)[2].object, valid=temporal_case(*size)[2].valid)


def c_bounded(form, o, size):
    if form == "cuda":
        rectify.accumulate_bounded(o["color"], o["motion"], *size, o["history"], o["box"], o["current"], o["previous"], clamped_length=2, out=o["out"],
                                   variance=o["variance"], clamped=o["clamped"], **TS.PARAMS)
    else:
        rectify._accumulate_bounded(NUMPY, o["color"], o["motion"], *size, o["history"], o["box"], o["current"], o["previous"], temporal._params(**TS.PARAMS), 2,
                                    o["out"], o["variance"], o["clamped"], "uint32")


@functools.lru_cache(maxsize=None)
def w_bounded(size):
    color, history, cur, prev, motion = temporal_case(*size)
    out, variance, clamped = rectify.accumulate_bounded_numpy(color, motion, *size, history, w_bounded_box(size), planes_as_guides(cur), planes_as_guides(prev),
                                                              clamped_length=2, **TS.PARAMS)
    return frozen(dict(out=out, variance=variance, clamped=clamped))


def b_feedback(case, size):
    rows, cols = size
    color, history, cur, _, _ = temporal_case(rows, cols)
    return dict(color=case.field("color", "in", RECORD_WORDS, 0, data=color, width=3), valid=case.field("valid", "in", SURFACE_WORDS, VALID_AT, data=cur.valid),
                history=case.compact("history", "inout", data=history.reshape(rows, cols), record=HISTORY))


def c_feedback(form, o, size):
    if form == "cuda":
        rectify.feedback(o["color"], o["history"], *size, valid=o["valid"])
    else:
        rectify._feedback(NUMPY, o["color"], o["history"], *size, o["valid"])


@functools.lru_cache(maxsize=None)
def w_feedback(size):
    color, history, cur, _, _ = temporal_case(*size)
    return frozen(dict(history=rectify.feedback_numpy(color, history, *size, valid=cur.valid)))


# ---- SVGF ----

SVGF_SIGMAS = dict(zip(("sigma_luminance", "sigma_normal", "sigma_position"), SS.FINITE_SIGMAS))


def b_svgf_variance(case, size):
    rows, cols = size
    _, _, history, normal, position, _, valid = SS.case_data(rows, cols)
    o = dict(history=case.compact("history", "in", data=np.asarray(history).reshape(rows, cols), record=HISTORY), out=case.compact("out", "out", shape=(rows, cols)))
    o.update(guide_planes(case, "", True, normal, position, None, valid))
    return o


def c_svgf_variance(form, o, size):
    if form == "cuda":
        svgf.variance(o["history"], *size, normal=o["normal"], position=o["position"], valid=o["valid"], sigma_normal=SS.FINITE_SIGMAS[1],
                      sigma_position=SS.FINITE_SIGMAS[2], out=o["out"])
    else:
        svgf._variance(NUMPY, o["history"], *size, o["normal"], o["position"], o["valid"], svgf._variance_params(SS.FINITE_SIGMAS[1], SS.FINITE_SIGMAS[2], svgf.MIN_LENGTH),
                       o["out"])


@functools.lru_cache(maxsize=None)
def w_svgf_variance(size):
    _, _, history, normal, position, _, valid = SS.case_data(*size)
    return frozen(dict(out=svgf.variance_numpy(history, *size, normal=normal, position=position, valid=valid, sigma_normal=SS.FINITE_SIGMAS[1],
                                               sigma_position=SS.FINITE_SIGMAS[2])))


def b_svgf_atrous(case, size, levels, first_level):
    rows, cols = size
    color, variance, _, normal, position, albedo, valid = SS.case_data(rows, cols)
    words = svgf._temp_words(rows * cols, levels)  # exactly svgf.temp_bytes / 4 (test_temp_formulas_agree holds the two together)
    o = dict(color=case.field("color", "in", RECORD_WORDS, 0, data=np.asarray(color).reshape(rows * cols, 3), width=3),
             variance=case.compact("variance", "in", data=np.asarray(variance).reshape(rows, cols)), out=case.compact("out", "out", shape=(rows, cols, 3)),
             variance_out=case.compact("variance_out", "out", shape=(rows, cols)), temp=case.temp("temp", words) if words else None)
    o.update(guide_planes(case, "", False, normal, position, albedo, valid))
    return o


def c_svgf_atrous(form, o, size, levels, first_level):
    guides = {k: o[k] for k in ("normal", "position", "albedo", "valid")}
    if form == "cuda":
        svgf.atrous(o["color"], o["variance"], *size, levels=levels, first_level=first_level, demodulate=True, out=o["out"], variance_out=o["variance_out"],
                    temp=o["temp"], **guides, **SVGF_SIGMAS)
    else:
        svgf._atrous(NUMPY, o["color"], o["variance"], *size, guides["normal"], guides["position"], guides["albedo"], guides["valid"],
                     svgf._atrous_params(levels, first_level, *SS.FINITE_SIGMAS, True), o["out"], o["variance_out"], o["temp"])


@functools.lru_cache(maxsize=None)
def w_svgf_atrous(size, levels, first_level):
    color, variance, _, normal, position, albedo, valid = SS.case_data(*size)
    out, variance_out = svgf.atrous_numpy(color, variance, *size, normal=normal, position=position, albedo=albedo, valid=valid, levels=levels,
                                          first_level=first_level, demodulate=True, **SVGF_SIGMAS)
    return frozen(dict(out=out, variance_out=variance_out))


# ---- upsample ----

def b_upsample(case, size, scale):
    rows, cols = size
    rl, cl = US.low(rows, scale), US.low(cols, scale)
    color, normal, position, albedo, valid, obj = US.case_data(rl, cl)
    _, hn, hp, ha, hv, ho = US.case_data(rows, cols, seed=12)
    low = guide_planes(case, "low.", True, normal, position, albedo, valid, obj)
    full = guide_planes(case, "full.", False, hn, hp, ha, hv, ho)
    return dict(color=case.field("color", "in", RECORD_WORDS, 0, data=np.asarray(color).reshape(rl * cl, 3), width=3), low=upsample.Guides(**low),
                full=upsample.Guides(**full), out=case.compact("out", "out", shape=(rows, cols, 3)))


def c_upsample(form, o, size, scale):
    sn, sp = US.FINITE_SIGMAS
    if form == "cuda":
        upsample.guided(o["color"], *size, low=o["low"], full=o["full"], scale=scale, radius=scale // 2, sigma_normal=sn, sigma_position=sp, out=o["out"])
    else:
        upsample._guided(NUMPY, o["color"], *size, o["low"], o["full"], scale, upsample._params(scale, scale // 2, sn, sp, True), o["out"])


@functools.lru_cache(maxsize=None)
def w_upsample(size, scale):
    rows, cols = size
    color, normal, position, albedo, valid, obj = US.case_data(US.low(rows, scale), US.low(cols, scale))
    _, hn, hp, ha, hv, ho = US.case_data(rows, cols, seed=12)
    sn, sp = US.FINITE_SIGMAS
    return frozen(dict(out=upsample.guided_numpy(color, rows, cols, upsample.Guides(normal, position, albedo, valid, obj), upsample.Guides(hn, hp, ha, hv, ho),
                                                 scale=scale, radius=scale // 2, sigma_normal=sn, sigma_position=sp)))


# ---- bloom ----

def b_bloom(case, size, levels, how):
    rows, cols = size
    color = BS.case_data(rows, cols)
    temp = case.temp("temp", BS.temp_bytes(rows, cols, levels) // 4)  # exactly bloom.temp_bytes (test_temp_formulas_agree)
    if how == "in place":
        return dict(color=None, out=case.compact("color", "inout", data=color), temp=temp)
    color = case.field("color", "in", RECORD_WORDS, 0, data=color, width=3) if how == "records" else case.compact("color", "in", data=color)
    return dict(color=color, out=case.compact("out", "out", shape=(rows, cols, 3)), temp=temp)


def c_bloom(form, o, size, levels, how):
    color = o["out"] if o["color"] is None else o["color"]
    (bloom.bloom if form == "cuda" else functools.partial(bloom._bloom, NUMPY))(color, bloom.THRESHOLD, bloom.KNEE, bloom.INTENSITY, levels, out=o["out"], temp=o["temp"])


@functools.lru_cache(maxsize=None)
def w_bloom(size, levels, how):
    out = bloom.bloom_numpy(BS.case_data(*size), levels=levels)
    return frozen({"color" if how == "in place" else "out": out})


# ---- motion ----

@functools.lru_cache(maxsize=None)
def device_scene(name):
    """the scene of a _motion_support case on the device: base()'s positions kept, then moved"""
    _, d, verts, sph = MS.base("dome" if name == "dome deformed" else "small")
    _, v, s, _ = MS.moved(name)
    scene = rt.Scene(d)
    moving.keep_positions(scene)
    scene.update_vertices(0, np.ascontiguousarray(v, dtype=F32))
    scene.update_spheres(0, np.ascontiguousarray(s, dtype=F32))
    return scene


def b_previous(case, name, how):
    hits = np.asarray(MS.moved(name)[3]).view(np.int32).reshape(-1, 13)
    n = hits.shape[0]
    out = case.field("out", "out", RECORD_WORDS, 3, shape=(n, 3), width=3) if how == "records" else case.compact("out", "out", shape=(n, 3))
    return dict(hits=case.compact("hits", "in", data=hits), out=out)


def c_previous(form, o, name, how):
    if form == "cuda":
        moving.previous_positions(device_scene(name), o["hits"], out=o["out"])
    else:
        now = MS.moved(name)[0]
        _, _, verts, sph = MS.base("dome" if name == "dome deformed" else "small")
        wt, ws = MS.kept_of(verts, sph)
        stride = RECORD_WORDS if how == "records" else 3
        _capi.check_host(_capi.host_lib().rt_previous_positions_cpu(C.byref(now), ptr(wt), ptr(ws), ptr(o["hits"]), o["hits"].shape[0], ptr(o["out"]), stride))


@functools.lru_cache(maxsize=None)
def w_previous(name, how):
    now, _, _, hits = MS.moved(name)
    _, _, verts, sph = MS.base("dome" if name == "dome deformed" else "small")
    return frozen(dict(out=moving.previous_positions_numpy(now, *MS.kept_of(verts, sph), hits)))


NAN_OK = G.same_or_both_nan
RADII = [(r,) for r in AS.SPLAT_RADII]
ROWS = [
    # the film: three entries older than the rt_X / rt_X_cpu convention, and the two accumulator calls under them
    Row("rt_film_offsets", None, b_offsets, c_offsets, w_offsets),
    Row("rt_camera_rays_offset", None, b_rays_offset, c_rays_offset, w_rays_offset, numpy=False),
    Row("rt_film_splat", "FILM", b_splat, c_splat, w_splat, RADII, form_option="RT_AMD_FILM_SPLAT_FORM"),
    Row("rt_accumulate_device", None, b_splat, c_accumulate, w_accumulate, [(None,)]),
    Row("rt_accumulator_resolve_device", None, b_resolve, c_resolve, w_resolve),
    Row("rt_sample_budget", "ADAPTIVE", b_budget, c_budget, w_budget),
    Row("rt_sample_list", "ADAPTIVE", b_list, c_list, w_list, [(room, first) for room in ("total", "below", "zero") for first in (False, True)], LIST_SIZES),
    Row("rt_film_offsets_listed", "ADAPTIVE", b_offsets_listed, c_offsets_listed, w_offsets_listed, same=dict(out=NAN_OK)),
    Row("rt_camera_rays_listed", "ADAPTIVE", b_rays_listed, c_rays_listed, w_rays_listed),
    Row("rt_film_splat_listed", "ADAPTIVE", b_splat_listed, c_splat_listed, w_splat_listed, [("random",), ("last64",)], form_option="RT_AMD_FILM_SPLAT_FORM"),
    Row("rt_denoise_atrous", "DENOISE", b_denoise, c_denoise, w_denoise, [(1, 0, False), (5, 0, True), (1, 2, True), (4, 2, False)],
        form_option="RT_AMD_DENOISE_FORM"),
    Row("rt_temporal_motion", "TEMPORAL", b_motion, c_motion, w_motion, same=dict(out=NAN_OK)),
    Row("rt_temporal_accumulate", "TEMPORAL", lambda case, size: temporal_operands(case, size), c_accumulate_temporal, w_accumulate_temporal,
        same=dict(out=NAN_OK, variance=NAN_OK)),
    Row("rt_temporal_bounds", "RECTIFY", b_bounds, c_bounds, w_bounds, [(r,) for r in BOUNDS_RADII], same=dict(out=NAN_OK)),
    Row("rt_temporal_accumulate_bounded", "RECTIFY", b_bounded, c_bounded, w_bounded, same=dict(out=NAN_OK, variance=NAN_OK)),
    Row("rt_temporal_feedback", "RECTIFY", b_feedback, c_feedback, w_feedback, same=dict(history=NAN_OK)),
    Row("rt_svgf_variance", "SVGF", b_svgf_variance, c_svgf_variance, w_svgf_variance, same=dict(out=NAN_OK)),
    Row("rt_svgf_atrous", "SVGF", b_svgf_atrous, c_svgf_atrous, w_svgf_atrous, [(1, 0), (5, 0), (2, 2)], form_option="RT_AMD_SVGF_FORM",
        same=dict(out=NAN_OK, variance_out=NAN_OK)),
    Row("rt_upsample_guided", "UPSAMPLE", b_upsample, c_upsample, w_upsample, [(2,), (4,)], form_option="RT_AMD_UPSAMPLE_FORM"),
    Row("rt_bloom", "BLOOM", b_bloom, c_bloom, w_bloom, [(1, "compact"), (5, "records"), (5, "in place")], form_option="RT_AMD_BLOOM_FORM"),
    Row("rt_previous_positions", "MOTION", b_previous, c_previous, w_previous, [("compact",), ("records",)], sizes=MS.CASES, same=dict(out=NAN_OK)),
]


def ident(v):
    return "-".join(str(x).replace(" ", "_") for x in v) or "plain"


NUMPY_CASES = [pytest.param(row, v, id=f"{row.entry}-{ident(v)}") for row in ROWS if row.numpy for v in row.variants]
DEVICE_CASES = [pytest.param(row, v, kernel, cap, id=f"{row.entry}-{ident(v)}-form{kernel}-cap{cap}") for row in ROWS for v in row.variants
                for kernel in ((0, 1) if row.form_option else (None,)) for cap in ((None, 1) if row.cap_option else (None,))]


@pytest.mark.parametrize("row,variant", NUMPY_CASES)
def test_the_cpu_definition_stays_inside_its_operands(row, variant):
    row.run("numpy", variant)


@pytest.mark.gpu
@pytest.mark.parametrize("row,variant,kernel,cap", DEVICE_CASES)
def test_the_device_stays_inside_its_operands(row, variant, kernel, cap):
    switches = {}
    if kernel is not None:
        switches[row.form_option] = kernel
    if cap is not None:
        switches[row.cap_option] = cap
    with rt.options(**switches):
        row.run("cuda", variant)


def test_temp_formulas_agree():
    """the rows size their scratch without the device library's help; these are its formulas (host arithmetic, no device)"""
    for rows, cols in SIZES:
        assert denoise.temp_bytes(rows, cols) == rows * cols * 12
        for levels in (1, 2, 5):
            assert bloom.temp_bytes(rows, cols, levels) == BS.temp_bytes(rows, cols, levels) == bloom._temp_floats(rows, cols, levels) * 4
            assert svgf.temp_bytes(rows, cols, levels) == svgf._temp_words(rows * cols, levels) * 4


# ---- completeness ----

# the hit-side queries that also follow the rt_X / rt_X_cpu convention: they take hit records, not image planes, and their own suites
# hold sentinel-filled outputs (test_gpu_area_lights.py, test_gpu_hemisphere.py)
HIT_QUERIES = {"rt_area_light_samples", "rt_hemisphere_dirs", "rt_hemisphere_fold"}
# the film's entries predate the convention: their CPU definitions are rt_film_offsets_host, rt_film_splat_host, rt_accumulate and
# rt_accumulator_resolve of librt_host.so, and rt_camera_rays_offset has none
BEFORE_THE_CONVENTION = {"rt_film_offsets", "rt_camera_rays_offset", "rt_film_splat", "rt_accumulate_device", "rt_accumulator_resolve_device"}


def test_every_image_query_has_a_guard_row():
    exposed = {name[:-4] for name in _capi.HOST_SYMBOLS if name.endswith("_cpu")} - HIT_QUERIES
    assert exposed and exposed <= set(_capi.AMD_SYMBOLS), exposed - set(_capi.AMD_SYMBOLS)
    exposed |= BEFORE_THE_CONVENTION
    guarded = {row.entry for row in ROWS}
    missing, stale = exposed - guarded, guarded - exposed
    assert not missing, (f"image queries without a guard row: {sorted(missing)} — add a Row to ROWS in tests/test_image_guards.py for each: a builder of guarded "
                         "operands, the call with out= and temp= given, and the expected result from the _numpy form")
    assert not stale, f"guard rows of entry points the libraries do not export: {sorted(stale)}"
    assert len(guarded) == len(ROWS), "two rows name the same entry"


# ---- the harness must be able to fail: wrong stand-ins, numpy only ----

def box_want(a):
    rows, cols = a.shape
    out = np.zeros((rows, cols), dtype=F32)
    for r in range(rows):
        for c in range(cols):
            out[r, c] = a[max(r - 1, 0):r + 2, max(c - 1, 0):c + 2].sum(dtype=F32)
    return out


STAND_IN = np.arange(1, 1 + 5 * 7, dtype=F32).reshape(5, 7)


def stand_in_build(case):
    return dict(case=case, a=case.compact("a", "in", data=STAND_IN), rec=case.field("rec", "in", RECORD_WORDS, 2, data=STAND_IN.reshape(-1)),
                recout=case.field("recout", "out", RECORD_WORDS, 1, shape=(35,)), temp=case.temp("temp", 35), out=case.compact("out", "out", shape=(5, 7)))


def correct(o):
    o["temp"][:] = o["a"].reshape(-1)
    o["out"][...] = box_want(o["a"]) + (o["temp"].sum() - o["a"].sum())
    o["recout"][:] = o["rec"]


def past_the_end(o):
    correct(o)
    op = o["case"]["out"]
    op.whole[op.guard + op.words] = 7


def before_the_start(o):
    correct(o)
    op = o["case"]["out"]
    op.whole[op.guard - 1] = 7


def into_an_input_guard(o):
    correct(o)
    op = o["case"]["a"]
    op.whole[op.guard + op.words + 3] = 7


def unclamped_box(o):
    """a 3 x 3 box filter whose last row reads the row after it: indices into the guarded buffer"""
    correct(o)
    op = o["case"]["a"]
    flat = op.whole.view(F32)
    r = 4
    for c in range(7):
        taps = [flat[op.guard + q * 7 + p] for q in (r - 1, r, r + 1) for p in range(max(c - 1, 0), min(c + 2, 7))]
        o["out"][r, c] = np.sum(np.array(taps, dtype=F32), dtype=F32)


def temp_before_writing(o):
    with np.errstate(all="ignore"):
        stale = o["temp"].sum()
    correct(o)
    with np.errstate(all="ignore"):
        o["out"][0, 0] += stale * F32(0.0) + np.where(np.isnan(stale), F32(1), np.sign(stale))


def last_unwritten(o):
    keep = o["out"][4, 6].copy()
    correct(o)
    o["out"][4, 6] = keep


def between_the_fields(o):
    correct(o)
    op = o["case"]["recout"]
    op.whole[op.guard + 3 * RECORD_WORDS + 5] = 7


WANT = dict(out=box_want(STAND_IN), recout=STAND_IN.reshape(-1))


def test_a_correct_stand_in_passes():
    G.run_poisoned(stand_in_build, correct, WANT)


@pytest.mark.parametrize("wrong,names", [(past_the_end, "output 'out'.*1 words past its last"), (before_the_start, "output 'out'.*1 words before its first"),
                                         (into_an_input_guard, "input 'a'.*4 words past its last"), (unclamped_box, "'out'.*moves with the poison.*input 'a'"),
                                         (temp_before_writing, "'out'.*moves with the poison.*scratch 'temp'"), (last_unwritten, "output 'out'.*left unwritten.*word 34"),
                                         (between_the_fields, "output 'recout'.*between the fields")])
def test_the_harness_catches(wrong, names):
    with pytest.raises(AssertionError, match=names):
        G.run_poisoned(stand_in_build, wrong, WANT)


def device_build(case):
    return dict(case=case, a=case.compact("a", "in", data=STAND_IN), out=case.compact("out", "out", shape=(5, 7)), temp=case.temp("temp", 35))


def device_stand_in(wrong, o):
    """out = 2 a through torch operations on the guarded tensors; every wrong access lies inside a guarded buffer"""
    import torch

    a, out = o["case"]["a"], o["case"]["out"]
    stale, kept = o["temp"][0].clone(), o["out"][4, 6].clone()
    o["temp"].copy_(o["a"].reshape(-1))
    o["out"].copy_(o["temp"].reshape(5, 7) * 2)
    if wrong == "a store past the end":
        out.whole[out.guard + out.words] = 7
    elif wrong == "a load past the end":
        o["out"][4, 6] = a.whole.view(torch.float32)[a.guard + a.words] * 2  # (a copy of the poison would read as "unwritten")
    elif wrong == "scratch read first":
        o["out"][0, 0] = stale * 2
    elif wrong == "an element unwritten":
        o["out"][4, 6] = kept


@pytest.mark.gpu
@pytest.mark.parametrize("wrong,names", [(None, None), ("a store past the end", "output 'out'.*1 words past its last"),
                                         ("a load past the end", "'out'.*moves with the poison.*input 'a'"),
                                         ("scratch read first", "'out'.*moves with the poison.*scratch 'temp'"),
                                         ("an element unwritten", "output 'out'.*left unwritten.*word 34")])
def test_the_harness_catches_on_device_buffers(wrong, names):
    """the same harness on CUDA tensors: uploads, views and downloads are the device rows' own"""
    run = lambda: G.run_poisoned(device_build, functools.partial(device_stand_in, wrong), dict(out=STAND_IN * F32(2)), "cuda")  # noqa: E731
    if wrong is None:
        run()
    else:
        with pytest.raises(AssertionError, match=names):
            run()


def test_guarded_lays_the_buffer_out():
    whole, view = G.guarded(100, G.SENTINEL)
    assert whole.size == 2 * 4096 + 100 and view.size == 100 and view.ctypes.data % 32 == 0 and (whole == G.SENTINEL).all()
    whole, view = G.guarded(5000, 7, align_words=8)
    assert whole.size == 3 * 5000 and view.ctypes.data - whole.ctypes.data == 5000 * 4 and view.ctypes.data % 32 == 0
