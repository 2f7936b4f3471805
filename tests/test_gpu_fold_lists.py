"""GPU parity of the persistent-wavefront kernel's fold lists (csrc/rt_pwf.hip): the NODE step appends every node that has
something below it to the list of its level, in the workgroup's arena, and the closing fold reads the lists, children before
parents.  A node left out of its list keeps its unfolded shade term, a node listed at the wrong level is folded before its
children, a list counter that survives a frame folds stale ids: each shows in the radiance.  So every case compares the f32
frame as u32, and the World::cast count, against the CPU oracle, through test_gpu_wavefront.py's helper.

The cases that are about levels first check, on the oracle's own numbers, that the frame has them: the oracle's cast count
grows with every step of the depth limit up to the one asked, i.e. at least one pixel's ray tree reaches every level — a
node at generation k has an ancestor with something below it at every level above."""
import numpy as np
import pytest

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import _capi
from homework_18_graphics_raytracer_amd._capi import Light, Material
import _oracle
import _scenes
from _records import tile_order
from _trace_support import _check, _mismatches, assert_same, trace, variant

pytestmark = pytest.mark.gpu

PWF = 16 | 2
DEPTH = 8


@pytest.fixture(scope="module")
def ref():
    world = rt.reference_world()
    return world, rt.reference_camera(), rt.Scene(world)


@pytest.fixture(scope="module")
def oracle_casts(ref):
    """the oracle's cast counts of the 64x64 frame at depth limits 0 .. DEPTH"""
    world, cam, _ = ref
    return [_oracle.render_whitted(world.desc(), cam, rt.Frame.full(64, 64, d))[1] for d in range(DEPTH + 1)]


def every_level_is_reached(casts, depth):
    return all(casts[k] > casts[k - 1] for k in range(1, depth + 1))


def test_every_level_populated_several_tiles_per_workgroup(ref, oracle_casts):
    world, cam, scene = ref
    assert every_level_is_reached(oracle_casts, DEPTH)
    _check(world, cam, rt.Frame.full(64, 64, DEPTH), scene=scene, variant=PWF)


@pytest.mark.parametrize("w,h", [(8, 8), (1, 1), (67, 45)])
def test_one_tile_one_lane_and_partial_tiles(ref, w, h):
    """8x8: one tile; 1x1: one lane (its ray misses the scene: a root that is complete as it stands, and empty lists); 67x45:
    partial tiles on both edges"""
    world, cam, scene = ref
    casts = [_oracle.render_whitted(world.desc(), cam, rt.Frame.full(w, h, d))[1] for d in range(DEPTH + 1)]
    assert every_level_is_reached(casts, DEPTH) if w > 1 else casts[DEPTH] == casts[0] > 0
    _check(world, cam, rt.Frame.full(w, h, DEPTH), scene=scene, variant=PWF)


@pytest.mark.parametrize("depth", [0, 1, 2])
def test_no_levels_to_fold_then_one(ref, oracle_casts, depth):
    """depth 0 and 1: roots only (folded by tile); depth 2: the first listed level"""
    world, cam, scene = ref
    assert every_level_is_reached(oracle_casts, depth)
    _check(world, cam, rt.Frame.full(64, 64, depth), scene=scene, variant=PWF)


def test_three_frames_in_a_row_then_another_camera(ref, oracle_casts):
    """The workspace's two header blocks alternate from launch to launch: anything of a list left over from the frame before
    would be folded into this one."""
    import torch

    world, cam, scene = ref
    assert every_level_is_reached(oracle_casts, DEPTH)
    frame = rt.Frame.full(64, 64, DEPTH)
    other = rt.reference_camera()
    other.center[0] += 0.25  # a step to the side: other rays, other trees
    cams = [cam, cam, cam, other]
    wants = {id(c): _oracle.render_whitted(world.desc(), c, frame) for c in (cam, other)}
    assert _mismatches(wants[id(cam)][0], wants[id(other)][0]) != 0  # the other camera sees another frame
    stream = torch.cuda.Stream()
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    with variant(PWF), torch.cuda.stream(stream):
        for step, c in enumerate(cams):
            count.zero_()
            got = rt.render_whitted(scene, c, frame, ray_count=count, stream=stream)
            stream.synchronize()
            want, wcasts = wants[id(c)]
            bad = _mismatches(got.cpu().numpy(), want)
            assert bad == 0, f"step {step}: {bad} channels differ"
            assert int(count.item()) == wcasts, f"step {step}"


def mirror_room(cam, lit=True):
    """A closed room of mirrors (shiness 0.9, opaque) around the camera: every ray hits, every hit above the depth limit reflects
    (0.9^8 is far above the threshold) and nothing refracts, so a pixel's tree is a chain of depth + 1 nodes, each but the last
    with something below it.  Without its light every World::cast is a node's own: the oracle's cast count IS the node count, and
    the light changes no tree."""
    m = Material()
    m.diffuse_fn, m.normal_fn, m.normal = 0, 0, (0.0, 0.0, 1.0)
    m.diffuse_color, m.specular_color = (0.8, 0.6, 0.4), (0.5, 0.5, 0.5)
    m.shiness, m.smoothness, m.transparency, m.refraction_index, m.opaque_decay = 0.9, 0.2, 0.0, 1.0, 0.0
    world = rt.World()
    room = world.push_object(m)
    c = np.array(list(cam.center), dtype=np.float64)
    for tri in _scenes._box(c, (3.0, 2.5, 3.5), np.eye(3)):
        room.push_flat_triangle([tri[0], tri[2], tri[1]], [(0, 0), (0, 1), (1, 0)])  # wound to face inwards
    if lit:
        lamp = Light()
        lamp.kind, lamp.has_origin, lamp.color = 2, 1, (1.0, 0.9, 0.8)
        lamp.origin = tuple(c + np.array([0.5, 1.5, -1.0]))
        world.push_light(lamp)
    return world


def node_cap(pixels, budget, groups):
    """the launcher's rule (rt_api.hip): nodes per arena, for a frame that is one band"""
    assert pixels <= (65536 - 1024) * groups // budget
    want = -(-pixels * budget // groups)
    ring = 8192 if budget >= 4 else 2048
    while ring < want + 1024 and ring < 65536:
        ring *= 2
    return ring - 1024


def test_one_lane_that_reaches_every_level(ref):
    """1x1 in the room of mirrors: one lane, one node listed at every level"""
    _, cam, _ = ref
    world = mirror_room(cam)
    casts = [_oracle.render_whitted(mirror_room(cam, lit=False).desc(), cam, rt.Frame.full(1, 1, d))[1] for d in range(DEPTH + 1)]
    assert casts == list(range(1, DEPTH + 2))  # a chain: one node more per level
    _check(world, cam, rt.Frame.full(1, 1, DEPTH), variant=PWF)


def test_budgets_on_one_workspace(ref):
    """Wave-front budgets 1, 2, 3 and 6 in that order on one scene (one workspace, which grows on the way): at 1, 2 and 3 the frame
    needs more nodes than all arenas together hold, whatever the tiles' distribution, so some arena overflows — with tiles of its
    own left — and the per-pixel kernel renders the frame.  That is asserted on the CPU: the node count is the oracle's cast count
    of the room without its light, the arenas' size is the launcher's rule for every number of workgroups the device can hold (a
    workgroup is 8 waves, a CU holds at most 32).  The lists hold as many ids as the arena has nodes and a node is listed once, so
    they cannot fill up before the arena does: an arena overflow is the only overflow there is."""
    import torch

    _, cam, _ = ref
    frame = rt.Frame.full(832, 480, DEPTH)
    pixels = frame.cols * frame.rows
    nodes = _oracle.render_whitted(mirror_room(cam, lit=False).desc(), cam, frame)[1]
    assert pixels * DEPTH < nodes <= pixels * (DEPTH + 1)  # all but a few pixels (rays into the room's edges) a full chain
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for per_cu in (1, 2, 3, 4):
        groups = min((pixels + 63) // 64, cus * per_cu)
        assert groups * 4 <= (pixels + 63) // 64  # several tiles per workgroup
        caps = [node_cap(pixels, b, groups) for b in (1, 2, 3, 6)]
        assert all(nodes > groups * cap for cap in caps[:3]), (groups, caps)  # overflow is certain at budgets 1, 2 and 3
        assert len(set(caps)) >= 3, (groups, caps)  # and the budgets are not one arena run four times
    world = mirror_room(cam)
    scene = rt.Scene(world)
    want, wcasts = _oracle.render_whitted(world.desc(), cam, frame)
    lib = _capi.amd_lib()
    with variant(PWF):
        for budget in (1, 2, 3, 6):
            _capi.check(lib.rt_set_wavefront_budget(budget))
            try:
                got, casts = rt.render_whitted_numpy(scene, cam, frame)
            finally:
                _capi.check(lib.rt_set_wavefront_budget(6))
            assert _mismatches(got, want) == 0, f"budget {budget}"
            assert casts == wcasts, f"budget {budget}"


def test_ray_batch_in_tile_order(ref, oracle_casts):
    """the RAYS instantiation: the frame's camera rays in the kernel's slot order, against the frame after + 0.0"""
    import torch

    world, cam, scene = ref
    assert every_level_is_reached(oracle_casts, DEPTH)
    frame = rt.Frame.full(64, 64, DEPTH)
    want, wcasts = _oracle.render_whitted(world.desc(), cam, frame)
    perm = torch.from_numpy(tile_order(frame.cols, frame.rows)).cuda()
    with variant(PWF):
        count = torch.zeros(1, dtype=torch.int64, device="cuda")
        frame_gpu = rt.render_whitted(scene, cam, frame, ray_count=count).cpu().numpy()
        got_t, casts = trace(scene, rt.camera_rays(cam, frame)[perm].contiguous(), frame.max_depth)
    got = np.empty_like(got_t)
    got[perm.cpu().numpy()] = got_t
    assert_same(frame_gpu, want, "rt_render_whitted against the oracle")
    assert_same(got + np.float32(0.0), frame_gpu, "rt_trace_rays in tile order")
    assert casts == int(count.item()) == wcasts


def test_breadth_first_walk(ref, oracle_casts):
    """the BFS instantiation, forced on the reference scene"""
    world, cam, _ = ref
    assert every_level_is_reached(oracle_casts, DEPTH)
    with rt.options(RT_AMD_BFS_WALK_TRIANGLES=1):  # read when the scene is created
        scene = rt.Scene(world)
    _check(world, cam, rt.Frame.full(64, 64, DEPTH), scene=scene, variant=PWF)
