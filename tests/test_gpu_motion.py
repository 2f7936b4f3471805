"""The motion queries on the device (include/rt_amd.h "motion queries"): rt_previous_positions, its _host form and the CPU definition
agree bit for bit on every case of tests/test_motion_host.py; batch sizes around the wave and the workgroup, with one workgroup striding
the whole batch; what the snapshot holds after one update, two updates and a second keep; stream order; a captured graph; the scene's
render data untouched; and two frames of the reference scene with the dodecahedron moved between them, through
accumulate_moving_frame, against the CPU path."""
import ctypes as C
import functools

import numpy as np
import pytest

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import _capi, moving, temporal
import _motion_support as ms
from _records import dev, host, torch_device, u32
from _scene_update_support import arrays_of, desc_with
from _temporal_support import HISTORY, NORMAL_AT, OBJECT_AT, POSITION_AT, VALID_AT, bits

pytestmark = pytest.mark.gpu
F32 = np.float32
INVALID, UNSUPPORTED = -1, -5


def update(scene, verts, spheres, first=0, stream=None):
    scene.update_vertices(first, np.ascontiguousarray(verts, dtype=F32), stream=stream)
    if spheres is not None:
        scene.update_spheres(0, np.ascontiguousarray(spheres, dtype=F32), stream=stream)


def device_was(scene, hits):
    out = moving.previous_positions(scene, dev(hits))
    torch_device().cuda.synchronize()
    return u32(out)


def host_form(scene, hits, stride=3, fill=0xDEADBEEF):
    h = np.ascontiguousarray(hits).view(np.uint32).reshape(-1, 13)
    out = np.full((h.shape[0], stride), fill, dtype=np.uint32)
    _capi.check(_capi.amd_lib().rt_previous_positions_host(scene._h, C.c_void_p(h.ctypes.data), h.shape[0], C.c_void_p(out.ctypes.data), stride))
    return out


def cast(scene, rays):
    hits = rt.cast_rays(scene, dev(rays))
    torch_device().cuda.synchronize()
    return u32(hits)


@pytest.mark.parametrize("name", ms.CASES)
def test_device_host_and_cpu_forms_agree(name):
    torch_device()
    _, d, verts, sph = ms.base("dome" if name == "dome deformed" else "small")
    now, v, s, cpu_hits = ms.moved(name)
    scene = rt.Scene(d)
    assert not moving.positions_kept(scene)
    moving.keep_positions(scene)
    assert moving.positions_kept(scene)
    update(scene, v, s)
    # the device's own casts on the updated scene (the oracle's, bit for bit, where neither distance is a NaN), the records that name
    # the degenerate primitives, the records that are no hit of the scene, and positions with a payload
    hits = np.concatenate([cast(scene, ms.case_rays(now, v, s)), cpu_hits[-5:], ms.special_hits(cpu_hits, d.n_triangles, d.n_spheres),
                           ms.payload_hits(cpu_hits)])
    wt, ws = ms.kept_of(verts, sph)
    want = moving.previous_positions_numpy(now, wt, ws, hits).view(np.uint32)
    # Words are compared as words.  The one exception: a NaN that went THROUGH the arithmetic — the payload position on a moved primitive,
    # whatever a degenerate primitive's divides give — carries the payload rule of the hardware that made it (x86 keeps an operand's,
    # gfx950 gives the default NaN), so there "a NaN" is all that is compared; with nothing moved no NaN goes through any arithmetic.
    same = (lambda a, b: a == b) if name == "nothing" else ms.same_words
    assert same(want, ms.restate(v, s, verts, ws, hits)).all()
    got, got_host, got_wide = device_was(scene, hits), host_form(scene, hits), host_form(scene, hits, 5)
    assert same(got, want).all() and same(got_host, want).all() and same(got_wide[:, :3], want).all()
    assert (got_wide[:, 3:] == 0xDEADBEEF).all()
    of_the_scene = ((hits[:, 0] == 1) & (hits[:, 1] < d.n_triangles)) | ((hits[:, 0] == 0) & (hits[:, 1] < d.n_spheres))
    assert ((want != hits[:, 3:6]).any(axis=1) & of_the_scene).any() == (name != "nothing")
    assert (want[~of_the_scene] == ms.NAN_WORD).all() and (got[~of_the_scene] == ms.NAN_WORD).all()
    # a strided view of a record tensor as the output: the other words stay
    torch = torch_device()
    wide = torch.full((hits.shape[0], 7), 5.5, dtype=torch.float32, device="cuda")
    assert moving.previous_positions(scene, dev(hits), out=wide[:, 2:5]) is not None
    torch.cuda.synchronize()
    assert same(u32(wide)[:, 2:5], want).all() and (host(wide)[:, [0, 1, 5, 6]] == 5.5).all()


@functools.lru_cache(maxsize=None)
def deformed_scene():
    _, d, verts, sph = ms.base()
    now, v, s, hits = ms.moved("deformed")
    scene = rt.Scene(d)
    moving.keep_positions(scene)
    update(scene, v, s)
    wt, ws = ms.kept_of(verts, sph)
    return scene, now, wt, ws, hits


@pytest.mark.parametrize("cap", [None, 1])
def test_batch_sizes_around_the_wave_and_the_workgroup(cap):
    """1, a wave and a workgroup plus or minus one, and 4099 records; with RT_AMD_DIAG_MOTION_MAX_GROUPS=1 one workgroup strides them all"""
    scene, now, wt, ws, hits = deformed_scene()
    pool = np.concatenate([hits, ms.special_hits(hits, now.n_triangles, now.n_spheres)])
    with rt.options(RT_AMD_DIAG_MOTION_MAX_GROUPS=cap):
        for n in (1, 63, 64, 65, 255, 256, 257, 4099):
            batch = pool[(np.arange(n) * 7 + n) % pool.shape[0]]
            want = moving.previous_positions_numpy(now, wt, ws, batch).view(np.uint32)
            assert np.array_equal(device_was(scene, batch), want), n
    empty = moving.previous_positions(scene, dev(np.zeros((0, 13), dtype=np.uint32)))
    assert tuple(empty.shape) == (0, 3)


def test_the_keep_of_a_cap_of_one_workgroup_equals_the_default():
    """keep_positions_kernel grid-stride: 216 primitives of the dome scene through one workgroup of 256 lanes is one trip; the 40 + 3 of
    the small scene are less; so the stride is exercised by the large batch above and here by equality of the two keeps' answers"""
    _, d, verts, sph = ms.base("dome")
    now, v, s, hits = ms.moved("dome deformed")
    wt, ws = ms.kept_of(verts, sph)
    want = moving.previous_positions_numpy(now, wt, ws, hits).view(np.uint32)
    for cap in (None, 1):
        scene = rt.Scene(d)
        with rt.options(RT_AMD_DIAG_MOTION_MAX_GROUPS=cap):
            moving.keep_positions(scene)
        update(scene, v, s)
        assert np.array_equal(device_was(scene, hits), want), cap


def test_snapshot_semantics():
    torch = torch_device()
    _, d, verts, sph = ms.base()
    wt, ws = ms.kept_of(verts, sph)
    scene = rt.Scene(d)
    some = np.zeros((1, 13), dtype=np.uint32)
    with pytest.raises(rt.RtError, match="rt_scene_keep_positions") as refused:  # the query before any keep
        moving.previous_positions(scene, dev(some))
    assert refused.value.code == INVALID and not moving.positions_kept(scene)
    moving.keep_positions(scene)
    assert moving.positions_kept(scene)
    # keep -> update of triangles 5 .. 8 -> query: only hits on them differ from their position
    a = ms.jittered(verts, seed=4, which=slice(5, 9))
    scene.update_vertices(5, np.ascontiguousarray(a[5:9]))
    now_a = desc_with(d, verts=a)
    hits = cast(scene, ms.case_rays(now_a, a, sph))
    got = device_was(scene, hits)
    assert np.array_equal(got, moving.previous_positions_numpy(now_a, wt, ws, hits).view(np.uint32))
    differs = (got != hits[:, 3:6]).any(axis=1) & (hits[:, 0] <= 1)
    on_moved = (hits[:, 0] == 1) & (hits[:, 1] >= 5) & (hits[:, 1] < 9)
    assert differs.any() and np.array_equal(differs, on_moved)
    # keep -> update A -> update B -> query: the previous is still the keep's
    b = ms.jittered(verts, seed=6)
    scene.update_vertices(0, np.ascontiguousarray(b))
    now_b = desc_with(d, verts=b)
    hits = cast(scene, ms.case_rays(now_b, b, sph))
    assert np.array_equal(device_was(scene, hits), moving.previous_positions_numpy(now_b, wt, ws, hits).view(np.uint32))
    # keep -> update -> keep -> query: everything is unmoved
    moving.keep_positions(scene)
    valid = hits[:, 0] <= 1
    assert np.array_equal(device_was(scene, hits)[valid], hits[valid, 3:6])
    # a keep on stream s followed by an update, a cast and the query on s, with no synchronisation between them
    s = torch.cuda.Stream()
    c = ms.jittered(verts, seed=8)
    rays, vertices = dev(ms.case_rays(now_b, b, sph)), torch.from_numpy(np.ascontiguousarray(c)).cuda()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        moving.keep_positions(scene, stream=s)
        scene.update_vertices(0, vertices, stream=s)
        hits_s = rt.cast_rays(scene, rays, stream=s)
        was = moving.previous_positions(scene, hits_s, stream=s)
    s.synchronize()
    wt_b = ms.kept_of(b, sph)[0]
    want = moving.previous_positions_numpy(desc_with(d, verts=c), wt_b, ws, u32(hits_s)).view(np.uint32)
    assert np.array_equal(u32(was), want) and (want != u32(hits_s)[:, 3:6]).any()


def test_a_captured_round_replays_on_new_vertices():
    """{keep, update_vertices, cast, previous_positions} captured after one uncaptured round and replayed twice with other vertex data in
    the same buffer: each replay's previous positions are those of the round before it.  The first keep of a scene is refused inside a
    capture."""
    torch = torch_device()
    _, d, verts, sph = ms.base()
    ws = ms.kept_of(verts, sph)[1]
    rounds = [ms.jittered(verts, seed=k) for k in (20, 21, 22)]
    rays_np = ms.case_rays(d, verts, sph)
    scene, fresh = rt.Scene(d), rt.Scene(d)
    s = torch.cuda.Stream()
    rays = dev(rays_np)
    vertices = torch.from_numpy(np.ascontiguousarray(rounds[0])).cuda()
    hits = torch.zeros((rays.shape[0], 13), dtype=torch.int32, device="cuda")
    was = torch.zeros((rays.shape[0], 3), dtype=torch.float32, device="cuda")
    scratch = torch.zeros(4, device="cuda")
    torch.cuda.synchronize()

    def one_round():
        moving.keep_positions(scene, stream=s)
        scene.update_vertices(0, vertices, stream=s)
        rt.cast_rays(scene, rays, out=hits, stream=s)
        moving.previous_positions(scene, hits, out=was, stream=s)

    with torch.cuda.stream(s):
        one_round()  # uncaptured: the first keep and the first update allocate
        s.synchronize()
        refused = torch.cuda.CUDAGraph()
        with torch.cuda.graph(refused, stream=s):
            scratch.fill_(1.0)
            rc = _capi.amd_lib().rt_scene_keep_positions(fresh._h, C.c_void_p(s.cuda_stream))
            text = _capi.amd_lib().rt_last_error().decode()
        assert rc == UNSUPPORTED and "cannot be captured" in text and not moving.positions_kept(fresh)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            one_round()
        before = rounds[0]
        for now_v in rounds[1:]:
            vertices.copy_(torch.from_numpy(np.ascontiguousarray(now_v)))
            was.fill_(7.0)
            graph.replay()
            s.synchronize()
            now = desc_with(d, verts=now_v)
            want = moving.previous_positions_numpy(now, ms.kept_of(before, sph)[0], ws, u32(hits)).view(np.uint32)
            assert np.array_equal(u32(was), want) and (want != u32(hits)[:, 3:6]).any()
            before = now_v


def test_the_scenes_render_data_is_untouched():
    """after keep_positions and the queries a cast of the same rays is bit-identical to before, and so is every node record"""
    scene, now, wt, ws, hits = deformed_scene.__wrapped__()  # a scene of its own: the second keep below replaces its snapshot
    _, v, s, _ = ms.moved("deformed")
    rays = ms.case_rays(now, v, s)
    before, nodes_before = cast(scene, rays), [_nodes(scene, which) for which in (0, 1, 2)]
    moving.keep_positions(scene)
    device_was(scene, hits)
    assert np.array_equal(cast(scene, rays), before)
    for which in (0, 1, 2):
        assert np.array_equal(_nodes(scene, which), nodes_before[which]), which


def _nodes(scene, which):
    lib = _capi.amd_lib()
    n = C.c_size_t(0)
    _capi.check(lib.rt_diag_scene_nodes(scene._h, which, None, 0, C.byref(n)))
    out = np.zeros(n.value, dtype=np.uint32)
    _capi.check(lib.rt_diag_scene_nodes(scene._h, which, C.c_void_p(out.ctypes.data), n.value, C.byref(n)))
    return out


# ---- end to end on the reference scene at 64 x 48: the dodecahedron moved by a third of a pixel's footprint ----


def surfaces_numpy(s):
    hits, surfaces = s.hits.cpu().numpy().view(F32), s.surfaces.cpu().numpy().view(F32)
    return temporal.Guides(surfaces[:, NORMAL_AT:NORMAL_AT + 3], hits[:, POSITION_AT:POSITION_AT + 3], hits.view(np.uint32)[:, OBJECT_AT],
                           surfaces.view(np.uint32)[:, VALID_AT])


def test_two_frames_of_the_reference_scene_with_the_dodecahedron_moved():
    torch = torch_device()
    world = rt.reference_world()
    d = world.desc()
    obj, verts, sph = arrays_of(d)
    dodecahedron = np.flatnonzero(obj == 0)  # object 0, the imported mesh: the first triangles of the scene
    assert dodecahedron.size >= 12 and np.array_equal(dodecahedron, np.arange(dodecahedron.size))
    cam, frame = rt.reference_camera(), rt.Frame.full(64, 48, 3)
    rows, cols = frame.rows, frame.cols
    # a third of a pixel's footprint at the mesh, along the camera's right
    toward, up, eye = (np.array(list(a), dtype=np.float64) for a in (cam.toward, cam.up, cam.center))
    right = np.cross(toward, up)
    right /= np.linalg.norm(right)
    centre = verts[dodecahedron, :, :3].astype(np.float64).reshape(-1, 3).mean(axis=0)
    footprint = float(np.dot(centre - eye, toward / np.linalg.norm(toward))) * np.tan(cam.fovy / 2.0) / rows  # px = clip * rows, clip = x / (z tan)
    moved = verts.copy()
    moved[dodecahedron, :, :3] = (verts[dodecahedron, :, :3].astype(np.float64) + right * footprint / 3.0).astype(F32)
    now = desc_with(d, verts=moved)
    g = np.random.default_rng(21)
    scene = rt.Scene(d)
    clean = rt.render_whitted(scene, cam, frame).cpu().numpy()
    images = [(clean + g.normal(0.0, 0.2, clean.shape).astype(F32)).astype(F32) for _ in range(2)]

    def sequence(step):
        """two frames with the update between them; per frame the records, variance, motion, hits and guides"""
        sc = rt.Scene(d)
        history = temporal.History(rows, cols)
        out = []
        for k, image in enumerate(images):
            if k:
                sc.update_vertices(0, np.ascontiguousarray(moved[dodecahedron]))
            step(sc, cam, frame, dev(image).view(torch.float32), history)
            torch.cuda.synchronize()
            s = history._previous[0]
            out.append(dict(records=history.records.cpu().numpy().view(HISTORY).reshape(-1), variance=history.variance.cpu().numpy().copy(),
                            motion=history.motion.cpu().numpy().copy(), hits=u32(s.hits), guides=surfaces_numpy(s)))
        return sc, out

    scene_with, with_ = sequence(moving.accumulate_moving_frame)
    _, without = sequence(temporal.accumulate_frame)
    assert moving.positions_kept(scene_with)
    first, second = with_
    assert np.array_equal(bits(first["records"]), bits(without[0]["records"]))  # nothing kept yet: a plain push
    # the CPU path fed the same device-produced guides
    wt, ws = ms.kept_of(verts, sph)
    was = moving.previous_positions_numpy(now, wt, ws, second["hits"])
    m = temporal.motion_numpy(was, cam, frame, valid=second["guides"].valid)
    assert np.array_equal(bits(m), bits(second["motion"]))
    want, var = temporal.accumulate_numpy(images[1], m, rows, cols, first["records"], second["guides"]._replace(position=was), first["guides"])
    assert np.array_equal(bits(want.reshape(-1)), bits(second["records"])) and np.array_equal(bits(var), bits(second["variance"]))
    # history length 2 on every pixel whose hit is on the mesh in both frames and was visible in the previous one: the pixel it is
    # gathered from most (its own: the shift is a third of a pixel) showed the same triangle
    h1, h2 = first["hits"], second["hits"]
    on_mesh = (h2[:, 0] == 1) & (h2[:, 1] < dodecahedron.size)
    visible = on_mesh & (h1[:, 0] == 1) & (h1[:, 1] == h2[:, 1])
    assert visible.sum() > 50 and (second["records"]["length"][visible] == 2).all()
    kept_with = int((second["records"]["length"][on_mesh] == 2).sum())
    kept_without = int((without[1]["records"]["length"][on_mesh] == 2).sum())
    print(f"motion: of {int(on_mesh.sum())} pixels on the moved mesh ({int(visible.sum())} on the same triangle in both frames) "
          f"{kept_with} keep their history with the was-positions, {kept_without} without; footprint {footprint:.4g}")
    assert kept_with >= kept_without
    moved_px = np.abs(second["motion"].reshape(-1, 2)[on_mesh] - without[1]["motion"].reshape(-1, 2)[on_mesh]).max()
    assert 0.2 < moved_px < 0.5  # the was-positions project a third of a pixel from where the current ones do

    # History.push without position_was, on the same inputs, is today's accumulate_frame bit for bit
    ha, hb = temporal.History(rows, cols), temporal.History(rows, cols)
    for image in images:
        t = dev(image).view(torch.float32)
        temporal.accumulate_frame(scene, cam, frame, t, ha)
        hb.push(rt.materials.primary_surfaces(scene, cam, frame), cam, frame, t)
        torch.cuda.synchronize()
        assert np.array_equal(u32(ha.records), u32(hb.records)) and np.array_equal(u32(ha.variance), u32(hb.variance))
