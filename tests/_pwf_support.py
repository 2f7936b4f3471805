"""Shared pieces of tests/test_gpu_pwf_instantiations.py: how a small frame is steered onto each of the eight instantiations of
pwf_kernel<PACKED, BFS, RAYS> (csrc/rt_pwf_kernel.h), the scenes, the oracle's frames (computed once each) and the cell runner, which
names the instantiation it ran through homework_18_graphics_raytracer_amd.diagnostics before it compares a pixel.

The steering, derived from pw_plan (csrc/rt_api.hip) and pa_ready_packed (csrc/rt_pwf_common.h) and asserted through the diagnostic
in every cell, so that a change to either moves no cell silently:

  groups     = min(ceil(pixels / 64), workgroups the device holds [/ RT_AMD_WF_SHARE, rounded up]), at least 1
  max_pixels = (65536 - 1024) * groups / budget            more pixels than that: bands of rows (whole 8-row tile bands) or of rays (whole
                                                           64-ray tiles), ceil(pixels / max_pixels) of them, equally long
  want       = ceil(band_pixels * budget / groups)         nodes per arena
  ring_cap   = 8192 (2048 when budget < 4), doubled while ring_cap < want + 1024, up to 65536;  node_cap = ring_cap - 1024
  PACKED     = ((node_cap + 63) / 64 + 2 * (ring_cap / 64)) * 4 > 8192 bytes of page counters
               ring 32768: (496 + 1024) * 4 = 6080, unpacked; ring 65536: (1008 + 2048) * 4 = 12224, packed.  So PACKED <=> ring_cap ==
               65536 <=> want > 32768 - 1024 = 31744 nodes per arena.
  BFS        = the scene was created with at least RT_AMD_BFS_WALK_TRIANGLES triangles (and the stream's workspace holds the lists)
  RAYS       = the call is rt_trace_rays

  UNPACKED    default budget 6 on 67x45 (3015 pixels, 48 tiles -> 48 workgroups): want = ceil(3015 * 6 / 48) = 377 -> ring 8192.
              Budget 32 (the deep frames): want = 2010 -> ring 8192.
  PACKED_MANY budget 512 on 67x45: max_pixels = 64512 * 48 / 512 = 6048 >= 3015, one band; want = ceil(3015 * 512 / 48) = 32160 > 31744
              -> ring 65536.  (64x48, 3072 pixels: want = 32768, the same.)  48 arenas of ~12 MB.
  PACKED_ONE  RT_AMD_WF_SHARE=1000 (one workgroup: ceil(workgroups / 1000) = 1 for any device below 1000 of them) and the default
              budget 6 on 96x64: max_pixels = 64512 / 6 = 10752 >= 6144; want = 36864 > 31744 -> ring 65536.
  BANDS       budget 1100 on 67x45: max_pixels = 64512 * 48 / 1100 = 2815 < 3015 -> 2 bands; rows: ceil(45 / 2) = 23 -> 24 rows (whole
              tile bands) and a ragged last band of 21; rays: ceil(3015 / 2) = 1508 -> 1536 rays and a last band of 1479, no multiple of
              64.  want = ceil(67 * 24 * 1100 / 48) = 36850 (rays: 35200) -> ring 65536.
              A banded call is ALWAYS packed: n bands hold more than (n - 1) * max_pixels pixels, so a band has more than (n - 1) / n >=
              1 / 2 of max_pixels, and want > 64512 / 2 = 32256 > 31744.  The unpacked instantiations therefore have no bands cell;
              test_a_banded_call_is_always_packed sweeps the diagnostic over frames and budgets to show it.
  OVERFLOW    one workgroup (RT_AMD_WF_SHARE=1000), so that the outcome does not depend on how tiles fall to workgroups: the one arena
              must hold every node of the frame, and nodes are not reused within a frame (a tile is only started while node_cap - used
              >= 64 * 10).  The mirror room below at depth 20 has ROOM_NODES_PER_PIXEL ray_trace activations per pixel; 96x64 pixels:
                unpacked  budget 1: want = 6144 -> ring 8192 (from 2048), node_cap 7168 < 6144 * ROOM_NODES_PER_PIXEL
                packed    budget 10 <= ROOM_NODES_PER_PIXEL / 2: pixels * budget = 61440, just under the band limit 64512; want = 61440
                          -> ring 65536, node_cap 64512 < 6144 * ROOM_NODES_PER_PIXEL = 129024
              Many small workgroups need not overflow at budget 1: below budget 4 an arena still has 2048 ring slots, 1024 nodes,
              and a small frame has a workgroup per 64 pixels.  All the numbers above were confirmed on an MI355X through the
              diagnostic (the cells assert them).
"""
import functools

import numpy as np

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import _capi, diagnostics
from homework_18_graphics_raytracer_amd._capi import Camera, Light, Material
import _oracle
import _scenes
from _records import torch_device
from _trace_support import assert_same, trace, variant

PWF = 18  # the persistent wavefront kernel, the per-pixel kernel with scalar fetches behind it

# the plain frame: neither side a multiple of 8; 48 tiles, the last of 7 pixels
W, H = 67, 45
# the one-workgroup frames
W1, H1 = 96, 64

# steer -> (budget, switches); None: the library's default budget of 6
UNPACKED = ("unpacked", None, {})
UNPACKED_32 = ("unpacked", 32, {})
PACKED_MANY = ("packed", 512, {})
PACKED_ONE = ("packed", None, {"RT_AMD_WF_SHARE": 1000})
BANDS = ("packed", 1100, {})
OVERFLOW_UNPACKED = ("unpacked", 1, {"RT_AMD_WF_SHARE": 1000})
OVERFLOW_PACKED = ("packed", 10, {"RT_AMD_WF_SHARE": 1000})

# ray_trace activations (World::cast calls of NODE items) per pixel of the mirror room, 96x64 at depth 20, measured on the oracle as
# the cast count of its twin without lights (no light, no shadow cast; nothing transparent, no refraction cast: every cast is a node's
# own) divided by the pixels.  The room is closed and every surface reflects 0.8 of the light: 0.8^20 = 0.0115 is above ray_trace's
# threshold of 0.001, so every pixel runs to the depth limit: depth + 1 = 21 activations.  measured_room_nodes_per_pixel() recomputes it.
ROOM_NODES_PER_PIXEL = 21.0
ROOM_DEPTH = 20


def _mirror(color, shiness=0.8):
    m = Material()
    m.diffuse_fn = 0
    m.normal_fn = 0
    m.normal = (0.0, 0.0, 1.0)
    m.diffuse_color = color
    m.specular_color = (0.9, 0.9, 0.9)
    m.shiness = shiness
    m.smoothness = 0.2
    m.transparency = 0.0
    m.refraction_index = 1.0
    m.opaque_decay = 0.0
    return m


def room_world(n_lights=2):
    """A closed room of six reflecting walls (two triangles each, seen from inside) around the camera, a reflecting sphere in it, and
    point lights inside: every ray hits something at every depth."""
    w = rt.World()
    uv = [(0, 0), (0, 1), (1, 0), (0, 1)]
    a = 3.0
    walls = [  # corner order as _scenes.random_world's floor: its front faces the room
        [(-a, -a, -a), (-a, -a, a), (a, -a, a), (a, -a, -a)],    # floor, seen from above
        [(-a, a, -a), (a, a, -a), (a, a, a), (-a, a, a)],        # ceiling, seen from below
        [(-a, -a, -a), (a, -a, -a), (a, a, -a), (-a, a, -a)],    # back (z = -a), seen from +z
        [(-a, -a, a), (-a, a, a), (a, a, a), (a, -a, a)],        # front (z = +a), seen from -z
        [(-a, -a, -a), (-a, a, -a), (-a, a, a), (-a, -a, a)],    # left (x = -a), seen from +x
        [(a, -a, -a), (a, -a, a), (a, a, a), (a, a, -a)],        # right (x = +a), seen from -x
    ]
    colors = [(0.9, 0.2, 0.2), (0.2, 0.9, 0.2), (0.2, 0.2, 0.9), (0.9, 0.9, 0.2), (0.2, 0.9, 0.9), (0.9, 0.2, 0.9)]
    for corners, color in zip(walls, colors):
        w.push_object(_mirror(color)).push_square(corners, uv)
    w.push_object(_mirror((0.8, 0.8, 0.8))).push_sphere((0.4, -0.3, -0.8), 0.9)
    for i in range(n_lights):
        l = Light()
        l.kind = 2  # a point light
        l.color = (1.0, 0.9, 0.8) if i == 0 else (0.5, 0.6, 1.0)
        l.has_origin = 1
        l.origin = (1.5 - 2.5 * i, 2.0, 1.0 + 0.7 * i)
        w.push_light(l)
    return w


def room_camera():
    cam = Camera()
    cam.fovy = float(np.float32(np.radians(60.0)))
    cam.center = (-0.7, 0.4, 2.1)
    t = np.array([0.35, -0.25, -1.0])
    cam.toward = tuple(t / np.linalg.norm(t))
    cam.up = (0.0, 1.0, 0.0)
    cam.near = 0.0
    return cam


@functools.lru_cache(maxsize=None)
def measured_room_nodes_per_pixel():
    frame = rt.Frame.full(W1, H1, ROOM_DEPTH)
    _, casts = _oracle.render_whitted(room_world(0).desc(), room_camera(), frame)
    return casts / (W1 * H1)


@functools.lru_cache(maxsize=None)
def world_and_camera(name):
    """the scenes of the matrix, by name (kept alive: a scene's arrays are the world's)"""
    if name == "ref":
        return rt.reference_world(), rt.reference_camera()
    if name == "room":
        return room_world(), room_camera()
    assert name.startswith("lights")
    n = int(name[len("lights"):])
    return _scenes.random_world(40 + n, 30, 3, n_lights=n), _scenes.camera(7)


@functools.lru_cache(maxsize=None)
def scene_of(name, bfs):
    """one rt.Scene per world and walker, so that its workspace (arenas, lists) is allocated once for all its cells.  The walker is
    decided when the scene is created: RT_AMD_BFS_WALK_TRIANGLES=1 makes any mesh a breadth-first one, 0 none."""
    world, _ = world_and_camera(name)
    with rt.options(RT_AMD_BFS_WALK_TRIANGLES=1 if bfs else 0):
        return rt.Scene(world)


@functools.lru_cache(maxsize=None)
def oracle_frame(name, w, h, depth):
    """the oracle's frame and cast count: once per (scene, frame), shared by every cell on it and never written to"""
    world, cam = world_and_camera(name)
    img, casts = _oracle.render_whitted(world.desc(), cam, rt.Frame.full(w, h, depth))
    img.setflags(write=False)
    return img, casts


def run_cell(name, bfs, rays, steer, w, h, depth, stream=None):
    """One cell: render the frame (rays: trace the camera's own rays) on the null stream under `steer`, read the plan and the outcome
    back while the settings still stand, print them, assert the instantiation the cell was written for, then compare radiance as
    uint32 and the cast count with the oracle.  -> (plan, outcome)"""
    torch = torch_device()
    packing, budget, switches = steer
    world, cam = world_and_camera(name)
    scene = scene_of(name, bfs)
    frame = rt.Frame.full(w, h, depth)
    with variant(PWF, budget), rt.options(**switches):
        if rays:
            got, casts = trace(scene, rt.camera_rays(cam, frame), depth)
            got = got.reshape(h, w, 3) + np.float32(0.0)  # a frame is accumulated into zeros: -0.0 + 0.0
            plan = diagnostics.pwf_plan_rays(scene, w * h, depth)
        else:
            count = torch.zeros(1, dtype=torch.int64, device="cuda")
            got = rt.render_whitted(scene, cam, frame, ray_count=count).cpu().numpy()
            casts = int(count.item())
            plan = diagnostics.pwf_plan(scene, frame)
        outcome = diagnostics.pwf_outcome(scene)
    print(f"pwf cell {name} {w}x{h} depth {depth}: (packed, bfs, rays) = {tuple(int(x) for x in plan.instantiation)} groups {plan.groups} "
          f"ring_cap {plan.ring_cap} band_units {plan.band_units} of {plan.units} budget {plan.budget} | launched {int(outcome.launched)} "
          f"overflow {int(outcome.overflow)} tiles_done {outcome.tiles_done}")
    assert plan.persistent and outcome.launched, "the persistent kernel did not run at all"
    assert plan.instantiation == (packing == "packed", bfs, rays), f"the cell was written for another instantiation: {plan}"
    want, wcasts = oracle_frame(name, w, h, depth)
    assert_same(got, want, f"{name} {w}x{h} depth {depth} {plan.instantiation}")
    assert casts == wcasts
    return plan, outcome
