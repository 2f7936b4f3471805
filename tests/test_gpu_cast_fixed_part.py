"""The per-wave-cast fixed part of the intersection loop (csrc/rt_cast.h cast_asm, csrc/rt_cast_asm.h), held to the oracle bit for bit
where it was shortened: a node's normals evaluated by the record's own count (one to eight, or a cone), the lane's own "may use the
rejections" condition in place of a bit shifted out of the wave's mask, and the excluded face read off the ray's exclusion word on the
one triangle a lane excludes.  None of these has a margin — each evaluates what was evaluated before — so the cases aim at what they
touch: every normal count, every (culling mode, excluded face, facing) combination on an excluded triangle and on an excluded sphere,
NaN and infinite components, origins on either side of the neighbourhood bound, waves in which one lane (0 or 63) differs from the rest,
and batches of 1, 63, 64 and 65 rays.  The sphere loop's miss test and the shared camera origin of a tile are unchanged code; their
cases (grazing rays; small frames; a batch whose 65th origin differs in the last bit) are here so that a later change finds them.
Every comparison is of uint32 views against the oracle: hit records of orc_cast, frames and cast counts."""
import numpy as np
import pytest

import homework_18_graphics_raytracer_amd as rt
import _oracle
import _scenes
from _records import dev, host, oracle_hits, ray_records, same_f32, same_hits, torch_device
from _scene_update_support import arrays_of, desc_with
from _trace_support import _check, trace

pytestmark = pytest.mark.gpu
F32 = np.float32
CONE = 0xFFFFFFFF


def cast(scene, rays):
    """rt_cast_rays through the pair-wise walker (cast_pairs) and through the wave-uniform one (cast_asm, the persistent kernel's): both results"""
    torch = torch_device()
    out = {}
    for walker, opts in (("pair-wise", {}), ("wave-uniform", {"RT_AMD_QUERY_WAVE_UNIFORM": 1})):
        with rt.options(**opts):
            got = rt.cast_rays(scene, dev(rays))
        torch.cuda.synchronize()
        out[walker] = host(got).view(np.uint32)
    return out


def assert_hits(got, want, labels, what):
    for walker, g in got.items():
        bad = np.flatnonzero(~same_hits(g, want))
        assert bad.size == 0, f"{what}, {walker}: {bad.size} of {want.shape[0]} differ, first: {labels[bad[0]]}: got {g[bad[0]]} want {want[bad[0]]}"


# ---- a scene with every normal count ----


@pytest.fixture(scope="module")
def counts_world():
    """prismatic patches of one to eight plane directions, two curved ones (cones), a plain run and three spheres; its node array holds
    clustered nodes of many different normal counts and a cone, which the fixture asserts"""
    s = _scenes.Shapes(9100)
    slots = [(0.75 * (i - 2), 0.0, 0.75 * (j - 1)) for j in range(3) for i in range(5)]
    for k, width in enumerate(range(1, 9)):
        s.run(f"prism{width}", "prism", _scenes.patch(16 + 2 * width, "prism", slots[k], s.rng, width=width), glass=(width % 3 == 0))
    s.run("curved40", "curved", _scenes.patch(40, "curved", slots[8], s.rng, width=8), glass=False)
    s.run("curved23", "curved", _scenes.patch(23, "curved", slots[9], s.rng), glass=True)
    s.run("short5", "flat", _scenes.patch(5, "flat", slots[10], s.rng), glass=False)
    s.finish([((0.375, 1.5, 0.375), 0.4), ((-1.125, 1.3, -0.75), 0.35), ((1.1, 1.6, -0.4), 0.45)], (0.2, 3.0, 2.6), (0.0, 0.0, -0.1))
    desc = s.world.desc()
    normals = _scenes.nodes_of(desc)[:, 2]
    print("fixed part: normal counts of the nodes:", sorted(set(int(n) if n != CONE else -1 for n in normals)))
    listed = set(int(n) for n in normals if n != CONE and n != 0)
    assert len(listed) >= 5 and max(listed) >= 7 and min(listed) <= 2 and (normals == CONE).any() and (normals == 0).any()
    return s, desc


def aimed_rays(s, rng, n, spread=0.02):
    """n rays from around the camera towards points on the runs' triangles, with a little spread: coherent waves that skip most nodes"""
    tris = s.tris
    t = tris[rng.integers(0, tris.shape[0], n)]
    w = rng.dirichlet((1.0, 1.0, 1.0), n).astype(F32)
    target = (t * w[:, :, None]).sum(axis=1)
    eye = np.asarray(s.camera.center, dtype=F32) + rng.normal(0, spread, (n, 3)).astype(F32)
    return eye, (target - eye).astype(F32)


def test_every_normal_count(counts_world):
    """waves aimed at one object each (the other nodes' spheres are missed by every lane: their normals decide), and unrelated rays"""
    s, desc = counts_world
    rng = np.random.default_rng(1)
    scene = rt.Scene(s.world)
    rays, labels = [], []
    for name, first, count, _ in s.runs:  # 128 rays per object: two waves whose rays all go to the same few triangles
        t = s.tris[first + rng.integers(0, count, 128)]
        target = t.mean(axis=1) + rng.normal(0, 0.01, (128, 3)).astype(F32)
        eye = np.asarray(s.camera.center, dtype=F32)[None] + rng.normal(0, 0.01, (128, 3)).astype(F32)
        for face in (0, 1, 2):
            rays.append(ray_records(eye, target - eye, face=face)); labels += [f"{name} face {face}"] * 128
    o, d = aimed_rays(s, rng, 1024, spread=0.5)
    rays.append(ray_records(o, d, face=2)); labels += ["scattered"] * 1024
    # rays parallel to a plane of a prism (|n . d| below 1e-3: the node may not be skipped on its sphere alone)
    for name, first, count, kind in s.runs:
        if kind != "prism":
            continue
        t = s.tris[first:first + count]
        e = (t[:, 1] - t[:, 0])[rng.integers(0, count, 64)]
        o = np.asarray(s.camera.center, dtype=F32)[None] + rng.normal(0, 0.3, (64, 3)).astype(F32)
        rays.append(ray_records(o, e, face=2)); labels += [f"{name} in-plane"] * 64
    rays = np.concatenate(rays)
    assert_hits(cast(scene, rays), oracle_hits(desc, rays), labels, "normal counts")


# ---- the excluded face ----


def test_excluded_face_on_triangles_and_spheres(counts_world):
    """every (culling mode, excluded face, facing) on the triangle the ray would hit, the excluded one in a clustered leaf, in the plain
    run, and a sphere; the exclusion in all lanes, in lane 0 alone and in lane 63 alone"""
    s, desc = counts_world
    rng = np.random.default_rng(2)
    scene = rt.Scene(s.world)
    probes, labels = [], []
    for name, first, count, _ in (s.runs[1], s.runs[5], s.runs[8], s.runs[10]):
        tri = first + count // 2
        c = s.tris[tri].mean(axis=0)
        nrm = np.cross(s.tris[tri][1] - s.tris[tri][0], s.tris[tri][2] - s.tris[tri][1])
        nrm = (nrm / np.linalg.norm(nrm)).astype(F32)
        for side in (1.0, -1.0):  # from the front and from the back
            o = (c + side * nrm * F32(0.7))[None] + rng.normal(0, 0.002, (64, 3)).astype(F32)
            d = (c[None] - o).astype(F32)
            for face in (0, 1, 2):
                for ex_face in (0, 1, 2, 7):
                    for who in ("all", "lane0", "lane63", "none", "other"):
                        kind = np.full(64, -1)
                        if who == "all": kind[:] = 1
                        if who == "lane0": kind[0] = 1
                        if who == "lane63": kind[63] = 1
                        if who == "other": kind[:] = 1
                        index = np.full(64, tri + (1 if who == "other" else 0))
                        probes.append(ray_records(o, d, face=face, exclude=(kind, index, np.full(64, ex_face))))
                        labels += [f"{name} tri {tri} side {side} face {face} excluded face {ex_face} {who}"] * 64
    for si in range(desc.n_spheres):  # spheres: from outside and from inside, the sphere excluded
        sph = arrays_of(desc)[2][si]
        c, r = sph[1:4], sph[4]
        for inside in (False, True):
            o = (c + (np.array([0.0, 0.0, 0.0]) if inside else np.array([0.3, 1.7 * r, 0.2])).astype(F32))[None] + rng.normal(0, 0.002, (64, 3)).astype(F32)
            d = rng.normal(0, 1, (64, 3)).astype(F32) if inside else (c[None] - o).astype(F32)
            for face in (0, 1, 2):
                for ex_face in (0, 1, 2):
                    kind = np.where(np.arange(64) % 2 == 0, 0, -1)
                    probes.append(ray_records(o, d, face=face, exclude=(kind, np.full(64, si), np.full(64, ex_face))))
                    labels += [f"sphere {si} inside {inside} face {face} excluded face {ex_face}"] * 64
    rays = np.concatenate(probes)
    want = oracle_hits(desc, rays)
    assert (want[:, 0] == 1).sum() >= 1000 and (want[:, 0] == 0).sum() >= 100
    assert_hits(cast(scene, rays), want, labels, "excluded faces")


# ---- spheres grazed, odd components, the neighbourhood bound, batch sizes ----


@pytest.fixture(scope="module")
def reference():
    world = rt.reference_world()
    return world, world.desc()


def grazing_rays(desc, rng):
    """rays whose line passes a sphere's centre at radius * (1 + e) for e inside, on and outside the miss test's margin of 2^-22"""
    sph = arrays_of(desc)[2]
    rays, labels = [], []
    for si in range(desc.n_spheres):
        c, r = sph[si, 1:4].astype(np.float64), float(sph[si, 4])
        for e in (-1e-3, -2.0 ** -21, -2.0 ** -23, 0.0, 2.0 ** -24, 2.0 ** -23, 2.0 ** -22, 2.0 ** -21, 2.0 ** -20, 1e-3):
            u = rng.normal(0, 1, (64, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
            v = np.cross(u, rng.normal(0, 1, (64, 3))); v /= np.linalg.norm(v, axis=1, keepdims=True)
            o = c[None] + v * r * (1.0 + e) - u * 2.5
            for face in (0, 1, 2):
                rays.append(ray_records(o.astype(F32), u.astype(F32), face=face)); labels += [f"sphere {si} e {e} face {face}"] * 64
    return np.concatenate(rays), labels


def test_spheres_grazed(reference):
    world, desc = reference
    rays, labels = grazing_rays(desc, np.random.default_rng(3))
    want = oracle_hits(desc, rays)
    hit = want[:, 0] == 0
    assert hit.sum() >= 500 and (~hit).sum() >= 500
    assert_hits(cast(rt.Scene(world), rays), want, labels, "grazing rays")


def test_odd_components_and_one_lane_apart(reference):
    """a NaN and an infinity in each component of origin and direction; waves of clear misses with one lane (0, 63) that hits; origins on
    either side of the neighbourhood bound in one wave"""
    world, desc = reference
    rng = np.random.default_rng(4)
    cam = np.array([0.0, 1.0, 3.0], dtype=F32)
    base_o = cam[None] + rng.normal(0, 0.05, (64, 3)).astype(F32)
    base_d = (np.array([0.0, 0.5, 0.0], dtype=F32)[None] - base_o + rng.normal(0, 0.3, (64, 3)).astype(F32)).astype(F32)
    rays, labels = [], []
    for value in (np.nan, np.inf, -np.inf):
        for k in range(6):
            for lanes in (slice(0, 64), slice(0, 1), slice(63, 64)):
                o, d = base_o.copy(), base_d.copy()
                (o if k < 3 else d)[lanes, k % 3] = value
                for face in (0, 1, 2):
                    rays.append(ray_records(o, d, face=face)); labels += [f"{value} in component {k} lanes {lanes} face {face}"] * 64
    away = np.tile(np.array([[0.0, 1.0, 0.0]], dtype=F32), (64, 1))  # straight up from above the scene: nothing there
    up_o = np.tile(np.array([[0.0, 5.0, 0.0]], dtype=F32), (64, 1)) + rng.normal(0, 0.01, (64, 3)).astype(F32)
    for lane in (None, 0, 63):
        o, d = up_o.copy(), away.copy()
        if lane is not None:
            d[lane] = (0.0, -1.0, 0.0)
        rays.append(ray_records(o, d, face=2)); labels += [f"clear misses, lane {lane} aims down"] * 64
    for far in (1e3, 1e6, 1e12, 1e30):  # half the wave starts far outside the scene: those lanes may not use the rejections
        o, d = base_o.copy(), base_d.copy()
        o[::2] = (base_o[::2] - base_d[::2] / np.linalg.norm(base_d[::2], axis=1, keepdims=True) * F32(far)).astype(F32)
        rays.append(ray_records(o, d, face=2)); labels += [f"every other origin {far} away"] * 64
    rays = np.concatenate(rays)
    assert_hits(cast(rt.Scene(world), rays), oracle_hits(desc, rays), labels, "odd components")


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_batch_sizes(reference, n):
    world, desc = reference
    rays = ray_records(*[a[:n] for a in _scenes_rays(desc, n)], face=2)
    assert_hits(cast(rt.Scene(world), rays), oracle_hits(desc, rays), [f"ray {i}" for i in range(n)], f"batch of {n}")


def _scenes_rays(desc, n):
    rng = np.random.default_rng(5)
    o = np.array([0.0, 1.0, 3.0], dtype=F32)[None] + rng.normal(0, 0.05, (n, 3)).astype(F32)
    d = (np.array([0.0, 0.6, 0.0], dtype=F32)[None] - o + rng.normal(0, 0.4, (n, 3)).astype(F32)).astype(F32)
    return o, d


# ---- tiles: one origin per wave ----


@pytest.mark.parametrize("width, height, depth", [(16, 8, 0), (16, 8, 3), (67, 45, 0), (67, 45, 3)])
def test_camera_frames(reference, width, height, depth):
    world, _ = reference
    _check(world, rt.reference_camera(), rt.Frame.full(width, height, depth))


def oracle_trace(desc, rays, depth):
    import ctypes as C

    rays = np.ascontiguousarray(rays).view(np.uint32).reshape(-1, 11).copy()
    n = rays.shape[0]
    orays = (_oracle.OrcRay * n).from_buffer(rays)
    rgb, buf, casts, total = np.zeros((n, 3), dtype=F32), (C.c_float * 3)(), C.c_uint64(0), 0
    lib = _oracle.lib()
    for i in range(n):
        lib.orc_ray_trace(C.byref(desc), C.byref(orays[i]), depth, 1.0, buf, C.byref(casts))
        rgb[i] = buf[:]
        total += casts.value
    return rgb, total


@pytest.mark.parametrize("depth", [0, 3])
def test_batch_whose_65th_origin_differs_in_the_last_bit(reference, depth):
    """rt_trace_rays: the first 64 rays share the camera's origin, the 65th is one ulp off in x; then 63 more with origins of their own"""
    world, desc = reference
    rng = np.random.default_rng(6)
    n = 128
    o = np.tile(np.array([[0.0, 1.0, 3.0]], dtype=F32), (n, 1))
    o[64, 0] = np.nextafter(F32(o[64, 0]), F32(1.0))
    o[65:] += rng.normal(0, 0.05, (n - 65, 3)).astype(F32)
    d = (np.array([0.0, 0.5, 0.0], dtype=F32)[None] - o + rng.normal(0, 0.35, (n, 3)).astype(F32)).astype(F32)
    rays = ray_records(o, d, face=0)
    assert (rays[:64, 0:3] == rays[0, 0:3]).all() and rays[64, 0] != rays[0, 0]
    want, want_casts = oracle_trace(desc, rays, depth)
    got, casts = trace(rt.Scene(world), dev(rays), depth)
    bad = np.flatnonzero(~same_f32(got, want).all(axis=1))
    assert bad.size == 0, f"{bad.size} of {n} differ, first: ray {bad[0]}: got {got[bad[0]]} want {want[bad[0]]}"
    assert casts == want_casts and (want != 0).any()


# ---- updated scenes, and the breadth-first scene ----


def test_updated_scene_equals_a_fresh_one(reference):
    """one sphere, one triangle and one light moved by the update entry points: casts and a frame equal those of a scene created in the
    final state, and the oracle's"""
    world, a = reference
    rng = np.random.default_rng(7)
    _, va, sa = arrays_of(a)
    vb, sb = va.copy(), sa.copy()
    vb[40, :, 0:3] += np.array([0.05, 0.02, -0.03], dtype=F32)  # a triangle of the second clustered leaf
    sb[2, 1:4] += np.array([0.1, 0.05, -0.2], dtype=F32)
    lights = [a.lights[i] for i in range(a.n_lights)]
    lights[1] = _scenes.light(rng, 1)
    b = desc_with(a, verts=vb, spheres=sb, lights=lights)
    scene, fresh = rt.Scene(a), rt.Scene(b)
    scene.update_vertices(40, vb[40:41])
    scene.update_spheres(2, sb[2:3])
    scene.update_lights(1, lights[1:2])
    rays, labels = grazing_rays(b, rng)
    o, d = _scenes_rays(b, 1024)
    rays = np.concatenate([rays[::4], ray_records(o, d, face=2), ray_records(o, d, face=1, exclude=(np.full(1024, 1), np.full(1024, 40), np.full(1024, 1)))])
    labels = labels[::4] + ["towards the scene"] * 1024 + ["triangle 40 excluded"] * 1024
    want = oracle_hits(b, rays)
    got_updated, got_fresh = cast(scene, rays), cast(fresh, rays)
    assert_hits(got_updated, want, labels, "updated scene against the oracle")
    assert_hits(got_fresh, want, labels, "fresh scene against the oracle")
    frame = rt.Frame.full(67, 45, 3)
    img_u, casts_u = rt.render_whitted_numpy(scene, rt.reference_camera(), frame)
    img_f, casts_f = rt.render_whitted_numpy(fresh, rt.reference_camera(), frame)
    want_img, want_casts = _oracle.render_whitted(b, rt.reference_camera(), frame)
    assert same_f32(img_u, want_img).all() and same_f32(img_f, want_img).all() and casts_u == casts_f == want_casts


def test_breadth_first_scene_frame(reference):
    """the records the breadth-first walk shares with the node walk did not change meaning"""
    world, _ = reference
    with rt.options(RT_AMD_BFS_WALK_TRIANGLES=1):
        scene = rt.Scene(world)
    _check(world, rt.reference_camera(), rt.Frame.full(67, 45, 3), scene=scene)
