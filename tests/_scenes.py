"""Random and hand-built scenes for parity tests (through the product's World builder)."""
import numpy as np

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd._capi import Camera, Light, Material


def material(rng, kind="random"):
    m = Material()
    m.diffuse_fn = 0
    m.normal_fn = 0
    m.normal = (0.0, 0.0, 1.0)
    m.diffuse_color = tuple(rng.uniform(0.1, 1.0, 3))
    m.specular_color = tuple(rng.uniform(0.0, 1.0, 3))
    m.shiness = float(rng.choice([0.0, 0.1, 0.5, 1.0]))
    m.smoothness = float(rng.choice([1.0, 0.2, 0.01, 0.00001]))
    m.transparency = float(rng.choice([0.0, 0.0, 0.5, 0.96, 1.0]))
    m.refraction_index = float(rng.choice([1.0, 1.12, 1.6]))
    m.opaque_decay = float(rng.choice([0.0, 0.1, 0.3, 1.0]))
    if kind == "random" and rng.random() < 0.3:
        m.diffuse_fn = int(rng.integers(1, 3))
        m.normal_fn = int(rng.integers(0, 2))
        m.tex_color_a = tuple(rng.uniform(0, 1, 3))
        m.tex_color_b = tuple(rng.uniform(0, 1, 3))
        m.tex_frequency = float(rng.choice([3.0, 10.0, 20.0]))
        m.normal_frequency = float(rng.choice([1.0, 10.0]))
        m.normal = (float(rng.uniform(-0.3, 0.3)), 0.0, 1.0)
    return m


def light(rng, kind):
    l = Light()
    l.kind = kind
    l.color = tuple(rng.uniform(0.3, 1.0, 3))
    if kind == 0:
        d = rng.normal(0, 1, 3)
        d[1] = -abs(d[1]) - 0.2
        l.direction = tuple(d / np.linalg.norm(d))
        l.has_origin = int(rng.random() < 0.3)
        l.origin = tuple(rng.uniform(-3, 3, 3) + np.array([0, 6, 0]))
    elif kind == 1:
        l.has_origin = 1
        l.origin = tuple(rng.uniform(-2, 2, 3) + np.array([0, 8, 0]))
        l.direction = (0.0, -1.0, -0.0)
        l.angle = float(rng.uniform(0.4, 1.2))
        l.softness = float(rng.choice([0.5, 1.0, 2.0]))
    else:
        l.has_origin = 1
        l.origin = tuple(rng.uniform(-2, 2, 3) + np.array([0, 2.5, 0]))
    return l


def random_world(seed, n_triangles, n_spheres, n_materials=5, n_lights=3):
    rng = np.random.default_rng(seed)
    w = rt.World()
    proxies = [w.push_object(material(rng)) for _ in range(max(1, n_materials))]
    # a floor so that most rays hit something, then random triangles
    if n_triangles >= 2:
        proxies[0].push_square([(-4, -0.5, -4), (-4, -0.5, 4), (4, -0.5, 4), (4, -0.5, -4)], [(0, 0), (0, 1), (1, 0), (0, 1)])
    k = 2 if n_triangles >= 2 else 0
    while k < n_triangles:
        c = rng.uniform(-2, 2, 3) + np.array([0, 0.8, 0])
        p = c + rng.normal(0, 0.6, (3, 3))
        uv = rng.uniform(0, 1, (3, 2))
        proxies[int(rng.integers(0, len(proxies)))].push_flat_triangle(p.tolist(), uv.tolist())
        k += 1
    for _ in range(n_spheres):
        proxies[int(rng.integers(0, len(proxies)))].push_sphere(tuple(rng.uniform(-1.5, 1.5, 3) + np.array([0, 0.6, 0])), float(rng.uniform(0.2, 0.6)))
    for i in range(n_lights):
        w.push_light(light(rng, i % 3))
    return w


def camera(seed=0):
    rng = np.random.default_rng(1000 + seed)
    cam = Camera()
    cam.fovy = float(np.float32(np.radians(rng.uniform(40, 75))))
    eye = np.array([rng.uniform(2, 3.5), rng.uniform(1.5, 3.0), rng.uniform(2, 3.5)])
    cam.center = tuple(eye)
    t = -eye + rng.normal(0, 0.2, 3)
    cam.toward = tuple(t / np.linalg.norm(t))
    cam.up = (0.0, 1.0, 0.0)
    cam.near = float(rng.choice([-0.1, 0.0, 0.2]))
    return cam


def _box(center, half, rot):
    """The 12 triangles of a box (outward winding): corners c + rot @ (+-hx, +-hy, +-hz)."""
    c = np.asarray(center, dtype=np.float64)
    h = np.asarray(half, dtype=np.float64)
    corner = lambda sx, sy, sz: (c + rot @ (h * np.array([sx, sy, sz]))).tolist()
    quads = [  # each face as a quad in counter-clockwise order seen from outside
        [(1, -1, -1), (1, 1, -1), (1, 1, 1), (1, -1, 1)], [(-1, -1, 1), (-1, 1, 1), (-1, 1, -1), (-1, -1, -1)],
        [(-1, 1, -1), (-1, 1, 1), (1, 1, 1), (1, 1, -1)], [(-1, -1, 1), (-1, -1, -1), (1, -1, -1), (1, -1, 1)],
        [(-1, -1, 1), (1, -1, 1), (1, 1, 1), (-1, 1, 1)], [(1, -1, -1), (-1, -1, -1), (-1, 1, -1), (1, 1, -1)],
    ]
    tris = []
    for q in quads:
        p = [corner(*v) for v in q]
        tris.append([p[0], p[1], p[2]])
        tris.append([p[0], p[2], p[3]])
    return tris


def _rotation(rng):
    q = rng.normal(0, 1, 4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def clustered_world(seed, n_boxes=4, axis_aligned=False, n_spheres=2):
    """Objects whose triangles are consecutive (so that rt_scene_create clusters them: csrc/rt_device_scene.h "segments"):
    a floor, then boxes of 12 triangles each — randomly rotated, or axis-aligned with round coordinates so that rays
    parallel to faces and origins on face planes occur exactly."""
    rng = np.random.default_rng(seed)
    w = rt.World()
    floor = w.push_object(material(rng, "plain"))
    floor.push_square([(-4, -0.5, -4), (-4, -0.5, 4), (4, -0.5, 4), (4, -0.5, -4)], [(0, 0), (0, 1), (1, 0), (0, 1)])
    for b in range(n_boxes):
        obj = w.push_object(material(rng, "plain"))
        if axis_aligned:
            centre = np.array([float(rng.integers(-3, 4)) * 0.5, float(rng.integers(0, 3)) * 0.5, float(rng.integers(-3, 4)) * 0.5])
            half = np.array([0.25, 0.5, 0.25]) * float(rng.integers(1, 3))
            rot = np.eye(3)
        else:
            centre = rng.uniform(-1.5, 1.5, 3) + np.array([0, 0.6, 0])
            half = rng.uniform(0.15, 0.5, 3)
            rot = _rotation(rng)
        for tri in _box(centre, half, rot):
            obj.push_flat_triangle(tri, rng.uniform(0, 1, (3, 2)).tolist())
    for _ in range(n_spheres):
        w.push_object(material(rng, "plain")).push_sphere(tuple(rng.uniform(-1.5, 1.5, 3) + np.array([0, 0.6, 0])), float(rng.uniform(0.2, 0.5)))
    for i in range(3):
        w.push_light(light(rng, i % 3))
    return w


def axis_camera(eye, toward=(0.0, 0.0, -1.0)):
    """A camera whose centre column / row rays have exact zeros in their directions."""
    cam = Camera()
    cam.fovy = float(np.float32(np.radians(60.0)))
    cam.center = tuple(float(x) for x in eye)
    cam.toward = tuple(float(x) for x in toward)
    cam.up = (0.0, 1.0, 0.0)
    cam.near = 0.0
    return cam


def squares_world(seed, n_squares=10):
    """Axis-aligned square()s with round coordinates, a few per object (so they stay plain runs, not clusters): each is two
    triangles on one plane whose face normals differ at most in the signs of zero components — the pairs the intersection
    loop shares a plane evaluation between (rt_device_scene.h RT_TRI_FOLLOWS / _WEAK) — plus a random triangle between
    some of them, so that followers, non-followers and leaders alternate.  With axis_camera() from a grid point, rays
    parallel to the planes (n.d == +-0: t = +-inf / NaN) and origins on them occur exactly."""
    rng = np.random.default_rng(4000 + seed)
    w = rt.World()
    obj = None
    for k in range(n_squares):
        if k % 3 == 0:
            obj = w.push_object(material(rng, "plain"))
        axis = int(rng.integers(0, 3))
        level = float(rng.integers(-2, 4)) * 0.5
        lo = [float(rng.integers(-4, 2)) * 0.5 for _ in range(2)]
        size = [float(rng.integers(1, 5)) * 0.5 for _ in range(2)]
        u, v = [a for a in range(3) if a != axis]
        corners = []
        for du, dv in ((0, 0), (1, 0), (1, 1), (0, 1)) if rng.integers(0, 2) else ((0, 0), (0, 1), (1, 1), (1, 0)):
            p = [0.0, 0.0, 0.0]
            p[axis] = level
            p[u] = lo[0] + du * size[0]
            p[v] = lo[1] + dv * size[1]
            corners.append(tuple(p))
        obj.push_square(corners, [(0, 0), (0, 1), (1, 1), (1, 0)])
        if rng.integers(0, 3) == 0:
            c = rng.uniform(-1.5, 1.5, 3)
            obj.push_flat_triangle((c + rng.normal(0, 0.5, (3, 3))).tolist(), rng.uniform(0, 1, (3, 2)).tolist())
    w.push_object(material(rng, "plain")).push_sphere((0.3, 0.4, -0.2), 0.35)
    for i in range(3):
        w.push_light(light(rng, i % 3))
    return w


def behind_spot_world(axis=(1.0, 2.0, 3.0), scale=0.37):
    """A square facing a spot light from BEHIND, seen through a very narrow camera aimed at the point where the light's axis,
    extended backwards, meets it: for some of those pixels cgmath's `angle` argument dot / (|a| |b|) rounds to just below -1,
    acos gives NaN, `NaN > spread` is false and the light — pointing the other way — DOES ask, with a NaN colour
    (lights.rs:57-60).  ADVICE r3: the shortcut of rt_shade.h light_asks must not turn those into None."""
    w = rt.World()
    m = Material()
    m.diffuse_fn = 0
    m.normal_fn = 0
    m.normal = (0.0, 0.0, 1.0)
    m.diffuse_color = (0.8, 0.7, 0.6)
    m.specular_color = (0.5, 0.5, 0.5)
    m.shiness, m.smoothness, m.transparency, m.refraction_index, m.opaque_decay = 0.3, 0.2, 0.0, 1.0, 0.0
    ob = w.push_object(m)
    o = np.array([0.3, 1.0, -0.2])
    dn = np.array(axis, float)
    dn /= np.linalg.norm(dn)
    c = o - 1.5 * dn
    a = np.cross(dn, [0, 1, 0])
    a /= np.linalg.norm(a)
    b = np.cross(dn, a)
    corners = [c - 2 * a - 2 * b, c + 2 * a - 2 * b, c + 2 * a + 2 * b, c - 2 * a + 2 * b]
    ob.push_square([tuple(p) for p in corners], [(0, 0), (0, 1), (1, 0), (0, 1)])
    spot = Light()
    spot.kind, spot.has_origin = 1, 1
    spot.origin = tuple(o)
    spot.direction = tuple(np.array(axis, float) * scale)
    spot.angle, spot.softness = 0.9, 1.0
    spot.color = (1.0, 0.9, 0.8)
    w.push_light(spot)
    point = Light()
    point.kind, point.has_origin = 2, 1
    point.origin = tuple(o + np.array([0.5, 0.3, 0.1]))
    point.color = (0.3, 0.3, 0.4)
    w.push_light(point)
    cam = Camera()
    eye = o + 0.4 * a + 0.3 * b + 0.2 * dn
    t = c - eye
    cam.center = tuple(eye)
    cam.toward = tuple(t / np.linalg.norm(t))
    cam.up = tuple(b)
    cam.near = -0.1
    cam.fovy = float(np.float32(2 * np.arctan(2e-3 / np.linalg.norm(t))))
    return w, cam


# ---- scenes that fix the SHAPE of the node array (csrc/rt_api_layout.hip): runs of consecutive triangles of one object ----

def nodes_of(desc):
    """rt_scene_describe_nodes (host only): rows of (first, count, n_normals, skip_to, dealing word, 0), one per node"""
    import ctypes as C

    from homework_18_graphics_raytracer_amd import _capi

    lib = _capi.amd_lib()
    n = C.c_uint32(0)
    _capi.check(lib.rt_scene_describe_nodes(C.byref(desc), None, 0, C.byref(n)))
    words = (C.c_uint32 * (6 * n.value))()
    _capi.check(lib.rt_scene_describe_nodes(C.byref(desc), words, n.value, C.byref(n)))
    return np.frombuffer(words, dtype=np.uint32).reshape(-1, 6).copy()


def patch(n, kind, centre, rng, cell=0.05, width=6, radius=1.5, tilt=0.25):
    """(n, 3, 3) binary32-exact vertex positions of exactly n triangles: a grid of `width` cells per row walked row by row, two
    triangles per cell, cut off after n triangles; normals towards +y before a random tilt of at most `tilt` radians.
    kind "flat": one plane.  "prism": the height is piecewise linear in the column, one slope per column — `width` (<= 8) plane
    directions, the two triangles of a cell coplanar.  "curved": a cap of a sphere of `radius`, slightly twisted — every triangle its own
    direction, all well within 45 degrees of their mean."""
    assert n >= 1 and kind in ("flat", "prism", "curved") and (kind != "prism" or width <= 8)
    t = np.arange(n)
    cell_index = t // 2
    i, j = cell_index % width, cell_index // width
    rows = (n + 2 * width - 1) // (2 * width)
    x0, z0 = (i - width / 2) * cell, (j - rows / 2) * cell
    a, b = np.stack([x0, z0], 1), np.stack([x0 + cell, z0], 1)
    c, d = np.stack([x0 + cell, z0 + cell], 1), np.stack([x0, z0 + cell], 1)
    odd = (t % 2 == 1)[:, None]
    xz = np.stack([a, np.where(odd, d, c), np.where(odd, c, b)], 1)  # (a, c, b) and (a, d, c): face normals towards +y
    x, z = xz[:, :, 0], xz[:, :, 1]
    if kind == "flat":
        y = np.zeros_like(x)
    elif kind == "prism":
        slopes = rng.permutation(np.linspace(-0.4, 0.4, width))  # 0.8 / 7 apart at least: far beyond the 1e-4 within which normals merge
        edge = np.concatenate([[0.0], np.cumsum(slopes * cell)])
        col = np.clip(np.rint(x / cell + width / 2).astype(int), 0, width)  # every vertex lies on a column edge
        y = edge[col]
    else:
        # the twist x z keeps the two triangles of a cell off one plane: on a cap alone they share it to second order (x^2 + z^2 is a sum
        # of a function of x and one of z), and normals within 1e-4 per component count as one direction
        y = np.sqrt(radius * radius - x * x - z * z) - radius + 0.3 * x * z
    p = np.stack([x, y, z], 2)
    yaw, lean, about = rng.uniform(0, 2 * np.pi), rng.uniform(0, tilt), rng.uniform(0, 2 * np.pi)
    cy, sy = np.cos(yaw), np.sin(yaw)
    u = np.array([np.cos(about), 0.0, np.sin(about)])  # a horizontal axis to lean about (Rodrigues)
    k = np.array([[0, -u[2], u[1]], [u[2], 0, -u[0]], [-u[1], u[0], 0]])
    rot = (np.eye(3) + np.sin(lean) * k + (1 - np.cos(lean)) * (k @ k)) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    return (p @ rot.T + np.asarray(centre, dtype=np.float64)).astype(np.float32)


def deck(count, centre, step):
    """(count, 3, 3): one horizontal triangle (normal +y) repeated on the planes y = centre.y + k * step.  Every number is a small
    multiple of a power of two, so a ray with origin.y on a plane and direction.y = 0 lies IN that plane exactly (t = 0 / 0)."""
    cx, cy, cz = centre
    tri = np.array([[cx - 0.25, cy, cz - 0.125], [cx, cy, cz + 0.25], [cx + 0.25, cy, cz - 0.125]])
    out = np.repeat(tri[None], count, 0)
    out[:, :, 1] += (np.arange(count) * step)[:, None]
    assert np.array_equal(out.astype(np.float32).astype(np.float64), out)
    return out.astype(np.float32)


class Shapes:
    """A world made of named runs: .world; .runs, a list of (name, first triangle, count, kind); .tris, the (N, 3, 3) binary32
    positions in index order; .camera, a view of many of the runs."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.world = rt.World()
        self.runs = []
        self._tris = []
        self.camera = None

    @property
    def tris(self):
        return np.concatenate(self._tris)

    def run(self, name, kind, tris, glass=None):
        m = material(self.rng, "plain")
        if glass is not None:  # said outright: the glass walk (get_refract) must start inside some clustered leaves
            m.transparency = 0.96 if glass else 0.0
            m.refraction_index = 1.12 if glass else 1.0
        obj = self.world.push_object(m)
        first = sum(t.shape[0] for t in self._tris)
        for p in tris:
            obj.push_flat_triangle(p.tolist(), self.rng.uniform(0, 1, (3, 2)).tolist())
        self._tris.append(np.asarray(tris, dtype=np.float32))
        self.runs.append((name, first, int(tris.shape[0]), kind))

    def finish(self, spheres, eye, look_at):
        for c, r in spheres:
            self.world.push_object(material(self.rng, "plain")).push_sphere(tuple(c), float(r))
        for k in range(3):
            self.world.push_light(light(self.rng, k))
        cam = Camera()
        cam.fovy = float(np.float32(np.radians(60.0)))
        cam.center = tuple(float(v) for v in eye)
        t = np.asarray(look_at, dtype=np.float64) - np.asarray(eye, dtype=np.float64)
        cam.toward = tuple(t / np.linalg.norm(t))
        cam.up = (0.0, 1.0, 0.0)
        cam.near = 0.0
        self.camera = cam
        return self


DECKS = (("deck64", 64, 2.0 ** -6), ("deck21", 21, 2.0 ** -6), ("deck49", 49, 2.0 ** -6), ("deck0", 24, 0.0))


def leaf_size_world(swap=0):
    """Every clustered-leaf size: one patch object for each count 8 .. 64 (2 052 triangles; count + swap even: flat or prismatic, odd:
    curved), curved objects of 64 + r triangles for r = 1 .. 7 (leaves of 16, 16, 16, 16 and r), and four decks — 64, 21 and 49
    triangles 1/64 apart and 24 identical ones.  The objects sit 0.75 apart on the plane y = 0, each within 0.3 x 0.3 (the neighbour-leaf
    merge of rt_api_layout.hip wants a common sphere within 1.15 of the larger square radius), facing up; three spheres hang
    above the gaps and there are three lights, so that shadow rays meet something."""
    s = Shapes(7100 + swap)
    slots = [(0.75 * (i - 4), 0.0, 0.75 * (j - 3.5)) for j in range(8) for i in range(9)]
    k = 0
    for n in range(8, 65):
        curved = (n + swap) % 2 == 1
        kind = "curved" if curved else ("prism" if (n // 2) % 2 else "flat")
        s.run(f"patch{n}", kind, patch(n, kind, slots[k], s.rng), glass=(n % 3 == 0))
        k += 1
    for r in range(1, 8):
        s.run(f"tree64+{r}", "curved", patch(64 + r, "curved", slots[k], s.rng, width=8), glass=(r % 3 == 0))
        k += 1
    for name, count, step in DECKS:
        s.run(name, "deck", deck(count, (slots[k][0], 0.0 if step else 0.5, slots[k][2]), step), glass=False)
        k += 1
    return s.finish([((0.375, 2.5, 0.375), 0.4), ((-1.125, 2.3, -0.75), 0.35), ((1.875, 2.6, -1.5), 0.45)], (0.2, 3.4, 3.0), (0.0, 0.0, -0.2))


TREE_RUNS = (65, 80, 81, 255, 256, 257, 272, 273)
CRUMPLED = 528       # 33 leaves; leaf 16 is crumpled
DUP_OF = "slab24"    # the clustered object whose triangles 0 .. 6 and 10 .. 16 are repeated, before and after it, as plain runs


def tree_shape_world():
    """The shapes Emit::go (rt_api_layout.hip) gives a run of L leaves around the powers of 16, index-adjacent: curved objects of
    65, 80, 81, 255, 256, 257, 272 and 273 triangles (5, 5, 6, 16, 16, 17, 17, 18 leaves).  Then: a run of 5 triangles and, its own
    object, the 7-triangle copy "dupA" of slab24's triangles 0 .. 6 (two plain runs after a closed tree: ONE plain leaf that must not be
    merged into the tree); slab24, a flat clustered leaf of 24; "dupB", the copy of its triangles 10 .. 16 (equal distances between a
    plain and a pair-wise leaf, the plain one before and after); and a curved object of 528 triangles (33 leaves) whose 17th leaf is
    crumpled — face normals all over the sphere.  A node that fails takes its ancestors with it (they hold the same normals), so
    "a plain leaf inside a tree" is: no root, an inner node over leaves 0 .. 15, the crumpled leaf and leaves 17 .. 32 beside it."""
    s = Shapes(7200)
    slots = [(1.25 * (i - 1.5), 0.0, 1.25 * (j - 1)) for j in range(3) for i in range(4)]
    for k, n in enumerate(TREE_RUNS):
        s.run(f"tree{n}", "curved", patch(n, "curved", slots[k], s.rng, width=8), glass=(k % 3 == 0))
    s.run("short5", "flat", patch(5, "flat", slots[8], s.rng), glass=False)
    slab = patch(24, "flat", slots[9], s.rng)
    s.run("dupA", "flat", slab[0:7], glass=False)
    s.run(DUP_OF, "flat", slab, glass=False)
    s.run("dupB", "flat", slab[10:17], glass=False)
    big = patch(CRUMPLED, "curved", slots[10], s.rng, width=16, radius=2.0)
    leaf = slice(16 * 16, 17 * 16)
    big[leaf, :, 1] += s.rng.uniform(-0.06, 0.06, (16, 3)).astype(np.float32)
    s.run(f"crumpled{CRUMPLED}", "curved", big, glass=False)
    return s.finish([((0.6, 2.4, 0.6), 0.4), ((-0.6, 2.2, -0.6), 0.35)], (0.3, 3.6, 2.9), (0.0, 0.0, -0.2))


BIG_RUNS = (4096, 4112)


def big_tree_world():
    """256 and 257 leaves — a root over 16 inner nodes, and a root over an inner node of 16 inner nodes and one lone leaf — as two
    index-adjacent curved objects: 8 208 triangles, above the default breadth-first switch of 8 192.  They stand
    5 apart: a root's sphere must stay within half the scene's extent to be kept."""
    s = Shapes(7300)
    for k, n in enumerate(BIG_RUNS):
        s.run(f"tree{n}", "curved", patch(n, "curved", (5.0 * k - 2.5, 0.0, 0.0), s.rng, cell=0.03, width=64, radius=3.0, tilt=0.15), glass=(k == 1))
    return s.finish([((0.0, 2.0, 0.3), 0.4)], (0.3, 6.0, 5.5), (0.0, 0.0, 0.0))


def dealing(count):
    """(K, ck, R) of a clustered leaf of `count` triangles: of K = 1 .. 8 chunks of ck = ceil(count / K) triangles (no chunks of fewer
    than 4 once there are two) the first whose pairs per full pass, R * count / K with R = floor(64 / ck), beat the best so far by 5 %"""
    best, best_fill = None, 0.0
    for k in range(1, 9):
        ck = -(-count // k)
        if ck < 4 and k > 1:
            break
        r = 64 // ck
        fill = r * count / k
        if fill > best_fill * 1.05:
            best, best_fill = (k, ck, r), fill
    return best
