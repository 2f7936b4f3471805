"""Ray queries on the device (include/rt_amd.h rt_cast_rays / rt_camera_rays): every field of every hit equals the oracle's World::cast
(orc_cast) bit for bit, NaN equal to NaN, through the pair-wise kernel, the wave-uniform one (RT_AMD_QUERY_WAVE_UNIFORM) and the
breadth-first walk; camera rays equal orc_shoot(orc_clip(x, y)); stream order and graph capture."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import homework_18_graphics_raytracer_amd as rt
import _oracle
import _scenes
from _hit_support import check
from _records import bounds, oracle_hits, random_rays, same_hits, tessellated_world, torch_device

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def test_reference_scene_random_rays():
    world = rt.reference_world()
    desc = world.desc()
    scene = rt.Scene(world)
    centre, radius = bounds(desc)
    rays = random_rays(1, 10007, desc, centre, radius)
    want = check(scene, desc, rays, "reference scene")
    # the mix did what it was meant to: hits of both kinds, misses, both faces
    assert (want[:, 0] == 1).sum() > 1000 and (want[:, 0] == 0).sum() > 100 and (want[:, 0] == 0xFFFFFFFF).sum() > 1000
    assert (want[want[:, 0] != 0xFFFFFFFF, 11] == 1).sum() > 100
    # the host call and the named views agree with the device tensors
    host = rt.cast_rays_numpy(scene, rays.cpu().numpy())
    assert same_hits(host.view(np.uint32).reshape(-1, 13), want).all()
    hits = rt.Hits(rt.cast_rays(scene, rays))
    torch = torch_device()
    torch.cuda.synchronize()
    mask = hits.hit.cpu().numpy()
    assert (mask == (want[:, 0] != 0xFFFFFFFF)).all()
    assert np.array_equal(hits.distance.cpu().numpy().view(np.uint32)[mask], want[mask, 12])
    assert np.array_equal(hits.position.cpu().numpy().view(np.uint32)[mask], want[mask, 3:6])


def test_edge_rays():
    """rays in a triangle's plane (NaN distances: cast_pairs's whole-wave fallback), zero and non-normalised directions, infinite and
    NaN components, origins on a sphere's surface looking out with Back / Both, face values above 2 (read as Both)"""
    torch = torch_device()
    world = rt.reference_world()
    desc = world.desc()
    scene = rt.Scene(world)
    g = np.random.default_rng(5)
    o, d, face = [], [], []
    for i in range(desc.n_triangles):  # in the plane of an axis-aligned triangle: n.d = 0 and d - n.o = 0, t = 0 / 0
        p = np.array([v.position for v in desc.triangles[i].vertices], dtype=np.float32)
        for k in range(3):
            if p[0, k] == p[1, k] == p[2, k]:
                c = p.mean(axis=0)
                for j in range(3):
                    along = np.zeros(3, np.float32)
                    along[(k + 1 + j % 2) % 3] = 1.0 if j < 2 else -0.5
                    along[(k + 2 - j % 2) % 3] = 0.25 * j
                    origin = c - 3.0 * along
                    origin[k] = p[0, k]
                    o.append(origin)
                    d.append(along)
                    face.append(j % 3)
    for i in range(desc.n_spheres):
        s = desc.spheres[i]
        for k in range(6):
            u = g.normal(size=3)
            u /= np.linalg.norm(u)
            o.append(np.asarray(s.center) + u * s.radius)
            d.append(u if k % 2 else -u)
            face.append([1, 2][k % 2])
    specials = [(0.0, 0.0, 0.0), (0.0, 0.0, -1e-30), (0.0, 0.0, -1e30), (3.0, -7.0, 11.0), (np.inf, 0.0, 0.0), (0.0, -np.inf, 0.0),
                (np.nan, 0.0, -1.0), (0.1, 0.2, np.nan), (np.inf, np.inf, -np.inf)]
    for k, dd in enumerate(specials):
        for origin in ((0.0, 1.0, 3.0), (0.5, 0.5, 0.5), (np.inf, 0.0, 0.0), (np.nan, 1.0, 1.0)):
            o.append(origin)
            d.append(dd)
            face.append(k % 3)
    n = len(o)
    face = np.asarray(face)
    face[::7] = 3 + face[::7]  # above 2: Both
    rays = rt.make_rays(torch.tensor(np.asarray(o, np.float32), device="cuda"), torch.tensor(np.asarray(d, np.float32), device="cuda"),
                        torch.tensor(face, device="cuda"))
    # the oracle reads 3, 4, 5 as Both too (it tests Front and Back only); check it says so on its own records
    want = check(scene, desc, rays, "edge rays")
    assert np.isnan(want[want[:, 0] != 0xFFFFFFFF, 12].view(np.float32)).any(), "no NaN distance among the edge rays"
    assert n > 100


@pytest.mark.parametrize("make", ["random", "clustered", "no_spheres", "no_triangles", "squares"])
def test_scenes(make):
    worlds = {
        "random": [(_scenes.random_world(s, 40, 3), s) for s in (1, 2)],
        "clustered": [(_scenes.clustered_world(s, n_boxes=4), s) for s in (3, 4)] + [(_scenes.clustered_world(5, axis_aligned=True), 5)],
        "no_spheres": [(_scenes.random_world(6, 30, 0), 6)],
        "no_triangles": [(_scenes.random_world(7, 0, 5), 7)],
        "squares": [(_scenes.squares_world(8), 8)],
    }[make]
    for world, seed in worlds:
        desc = world.desc()
        scene = rt.Scene(world)
        centre, radius = bounds(desc)
        check(scene, desc, random_rays(100 + seed, 3000, desc, centre, radius), f"{make} {seed}")


@pytest.mark.parametrize("cap", [0, 96])
def test_breadth_first_walk(tmp_path, cap):
    """a scene walked breadth-first (RT_AMD_BFS_WALK_TRIANGLES low before the scene is created): rt::cast_rays_bfs_kernel, once with
    record lists cut short (RT_AMD_DIAG_BFS_CAP) so that some wave-casts overflow into cast_asm"""
    world = tessellated_world(tmp_path, 2, True)
    desc = world.desc()
    opts = {"RT_AMD_BFS_WALK_TRIANGLES": 1}
    if cap:
        opts["RT_AMD_DIAG_BFS_CAP"] = cap
    with rt.options(**opts):
        scene = rt.Scene(world)
        flat = tessellated_world(tmp_path, 2, False)
        flat_scene = rt.Scene(flat)
        centre, radius = bounds(desc)
        check(scene, desc, random_rays(11, 6000, desc, centre, radius), "bfs spherized")
        check(flat_scene, flat.desc(), random_rays(12, 4000, flat.desc(), centre, radius), "bfs flat")
        torch = torch_device()
        frame = rt.Frame.full(64, 48, 1)
        check(scene, desc, rt.camera_rays(rt.reference_camera(), frame), "bfs camera")


def _orc_primary(camera, frame):
    lib = _oracle.lib()
    out = np.zeros((frame.rows * frame.cols, 11), dtype=np.uint32)
    clip = (C.c_float * 2)()
    r = _oracle.OrcRay()
    k = 0
    for y in range(frame.y0, frame.y1, frame.y_step):
        for x in range(frame.x0, frame.x1):
            lib.orc_clip(frame.width, frame.height, x, y, clip)
            lib.orc_shoot(C.byref(camera), clip, C.byref(r))
            out[k] = np.frombuffer(bytes(r), dtype=np.uint32)
            k += 1
    return out


def test_camera_rays():
    torch = torch_device()
    world = rt.reference_world()
    desc = world.desc()
    scene = rt.Scene(world)
    cam = rt.reference_camera()
    full = rt.Frame.full(160, 120, 5)
    tile = rt.Frame(160, 120, 5, 17, 3, 150, 119, 3)
    for frame in (full, tile):
        rays = rt.camera_rays(cam, frame)
        torch.cuda.synchronize()
        assert np.array_equal(rays.cpu().numpy().view(np.uint32), _orc_primary(cam, frame)), (frame.x0, frame.y_step)
        check(scene, desc, rays, f"camera {frame.y_step}")
    # a primary ray that misses renders black (main.rs:474-477); a hit may be black too, so only this direction
    rays = rt.camera_rays(cam, full)
    hits = rt.Hits(rt.cast_rays(scene, rays))
    img = rt.render_whitted(scene, cam, full)
    torch.cuda.synchronize()
    miss = ~hits.hit.cpu().numpy()
    assert miss.sum() > 100
    assert (img.cpu().numpy().reshape(-1, 3)[miss].view(np.uint32) == 0).all()
    # another camera from the test scenes
    cam2 = _scenes.camera(4)
    rays = rt.camera_rays(cam2, tile)
    torch.cuda.synchronize()
    assert np.array_equal(rays.cpu().numpy().view(np.uint32), _orc_primary(cam2, tile))


def test_streams_capture_and_empty_batches():
    torch = torch_device()
    world = _scenes.random_world(21, 24, 3)
    desc = world.desc()
    scene = rt.Scene(world)
    centre, radius = bounds(desc)
    # two calls on two streams
    ra, rb = random_rays(31, 4099, desc, centre, radius), random_rays(32, 2053, desc, centre, radius)
    torch.cuda.synchronize()
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(sa):
        ha = rt.cast_rays(scene, ra)
    with torch.cuda.stream(sb):
        hb = rt.cast_rays(scene, rb)
    torch.cuda.synchronize()
    assert same_hits(ha.cpu().numpy(), oracle_hits(desc, ra.cpu().numpy())).all()
    assert same_hits(hb.cpu().numpy(), oracle_hits(desc, rb.cpu().numpy())).all()
    # captured into a graph, replayed after the ray buffer is overwritten
    rays = random_rays(33, 1000, desc, centre, radius)
    out = torch.empty((1000, 13), dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        rt.cast_rays(scene, rays, out=out)  # warm-up, uncaptured
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rt.cast_rays(scene, rays, out=out)
    fresh = random_rays(34, 1000, desc, centre, radius)
    rays.copy_(fresh)
    out.fill_(7)
    graph.replay()
    torch.cuda.synchronize()
    assert same_hits(out.cpu().numpy(), oracle_hits(desc, fresh.cpu().numpy())).all()
    # n_rays = 0: status 0, nothing launched, the output untouched
    empty = torch.empty((0, 11), dtype=torch.int32, device="cuda")
    out0 = torch.empty((0, 13), dtype=torch.int32, device="cuda")
    assert rt.cast_rays(scene, empty, out=out0) is out0
    lib = rt._capi.amd_lib()
    sentinel = torch.full((4, 13), 99, dtype=torch.int32, device="cuda")
    some = random_rays(35, 4, desc, centre, radius)
    assert lib.rt_cast_rays(scene._h, C.c_void_p(some.data_ptr()), 0, C.c_void_p(sentinel.data_ptr()), None) == 0
    torch.cuda.synchronize()
    assert (sentinel.cpu().numpy() == 99).all()
