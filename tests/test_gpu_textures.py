"""The texture queries on the device (include/rt_amd.h "texture queries"): every call gives the CPU form's bits at every batch size and
pyramid shape; a stripe texture and a normal map filled from rt_material_hits reproduce the enumerated material functions; light terms
on unedited surfaces are rt_light_terms'; the two sequences without bindings are the plain ones, and with a binding the restatement from
the CPU forms; the footprint follows a scene update; and the calls replay from a graph."""
import ctypes as C

import numpy as np
import pytest

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import _capi, materials, textures as T
import _guard_support as G
from _records import dev, host, torch_device, u32

pytestmark = pytest.mark.gpu
F32 = np.float32
WIDTH, HEIGHT = 16, 16
BATCHES = [1, 63, 64, 65, 257]


class Batch:
    pass


@pytest.fixture(scope="module")
def ref():
    torch = torch_device()
    b = Batch()
    b.world = rt.reference_world()
    b.desc = b.world.desc()
    b.scene = rt.Scene(b.world)
    b.rays_t = rt.camera_rays(rt.reference_camera(), rt.Frame.full(WIDTH, HEIGHT, 0))
    b.rays = u32(b.rays_t)
    hits = u32(rt.cast_rays(b.scene, b.rays_t)).copy()
    solid = np.flatnonzero(hits[:, 0] <= 1)
    assert solid.size > 100
    hits[solid[3], 2] = 9999                                                  # names no material: "no hit" to every call
    hits[solid[5], 1] = 0x7FFFFFFF                                            # a primitive index outside its array
    hits[solid[7], 9] = np.array([np.nan], dtype=F32).view(np.uint32)[0]      # a uv that is not finite
    b.hits, b.hits_t, b.n = hits, dev(hits), hits.shape[0]
    b.surfaces_t = materials.material_hits(b.scene, b.hits_t)
    b.surfaces = u32(b.surfaces_t)
    rng = np.random.default_rng(11)
    b.colour_img = rng.random((33, 65, 3), dtype=F32)
    b.normal_img = (rng.random((8, 5, 3), dtype=F32) - F32(0.5)) + F32([0, 0, 1])
    b.materials = [b.desc.materials[i] for i in range(b.desc.n_materials)]
    b.stripe = next(i for i, m in enumerate(b.materials) if m.diffuse_fn == 1)
    b.wave = next(i for i, m in enumerate(b.materials) if m.normal_fn == 1)
    torch.cuda.synchronize()
    return b


def pair(image, **kw):
    return T.Texture(image, **kw), T.HostTexture(image, **kw)


def window(b, n):
    """n records about the middle of the frame, going round it when n is more than it holds"""
    return (np.arange(n) + max(b.n - n, 0) // 2) % b.n


# ---- bits ----

@pytest.mark.parametrize("w,h", [(1, 1), (5, 3), (32, 17), (33, 65), (256, 256)])
def test_the_pyramid_is_the_cpu_form(w, h):
    """1x1: nothing to launch; 5x3 and 32x17: the single-workgroup launch alone; 33x65: one per-level launch, then that launch; 256x256:
    three per-level launches, then that launch"""
    image = np.random.default_rng(w + h).random((h, w, 3), dtype=F32)
    image[h // 2, w // 3, 1] = np.nan
    device, cpu = pair(image)
    torch_device().cuda.synchronize()
    assert device.n_levels == cpu.n_levels == T.levels(w, h)
    assert G.same_or_both_nan(host(device.texels), cpu.texels)


@pytest.mark.parametrize("n", BATCHES)
def test_footprint_sample_and_surfaces_are_the_cpu_forms(ref, n):
    torch = torch_device()
    at = window(ref, n)
    hits, rays = ref.hits[at], ref.rays[at]
    hits_t, rays_t = dev(hits), dev(rays)
    width0 = np.linspace(0, 0.01, n, dtype=F32)
    foot_t = T.footprint(ref.scene, hits_t, rays_t, 0.02, torch.tensor(width0, device="cuda"))
    foot = T.footprint_numpy(ref.world, hits, rays, 0.02, width0)
    assert G.same_bits(host(foot_t), foot) and (n < 64 or foot.any())
    assert G.same_bits(host(T.footprint(ref.scene, hits_t, rays_t, 0.02)), T.footprint_numpy(ref.world, hits, rays, 0.02))
    uv_t = hits_t.view(torch.float32)[:, 9:11]  # inside the records: stride 13
    for filter in (T.NEAREST, T.BILINEAR, T.TRILINEAR):
        for wrap in (T.REPEAT, T.CLAMP):
            kw = dict(filter=filter, wrap_u=wrap, wrap_v=T.REPEAT, scale=(3.0, -2.0), offset=(0.25, 0.5))
            device, cpu = pair(ref.colour_img, **kw)
            out_t = torch.full((n, 18), 7.0, dtype=torch.float32, device="cuda")
            T.sample(device, uv_t, foot_t * 40, out_t[:, 3:6])
            want = np.full((n, 18), 7.0, dtype=F32)
            T.sample_numpy(cpu, hits.view(F32)[:, 9:11], foot * F32(40), want[:, 3:6])
            assert G.same_or_both_nan(host(out_t), want), (filter, wrap)
            normal_t, normal = pair(ref.normal_img, filter=filter, wrap_u=wrap, wrap_v=wrap)
            for flags, index in ((0, T.ALL_OBJECTS), (T.MODULATE | T.NORMALIZE, int(hits[n // 2, 2]))):
                surfaces_t = dev(ref.surfaces[at])
                T.apply(surfaces_t, hits_t, device, normal_t, foot_t * 40, index, flags)
                want = T.apply_numpy(ref.surfaces[at], hits, cpu, normal, foot * F32(40), index, flags)
                assert G.same_or_both_nan(u32(surfaces_t).view(F32), want.view(F32)), (filter, wrap, flags)
    torch.cuda.synchronize()


# ---- the enumerated material functions as textures ----

def made_hits(n, obj, seed):
    rng = np.random.default_rng(seed)
    hits = np.zeros((n, 13), dtype=np.uint32)
    hits[:, 0], hits[:, 2] = 1, obj
    f = hits.view(F32)
    normal = rng.normal(size=(n, 3)).astype(F32)
    f[:, 3:6], f[:, 6:9] = rng.normal(size=(n, 3)), normal / np.linalg.norm(normal, axis=1, keepdims=True).astype(F32)
    f[:, 9:11] = rng.random((n, 2), dtype=F32)
    return hits


def test_a_stripe_texture_gives_material_hits_own_colour(ref):
    m = ref.materials[ref.stripe]
    image = np.empty((20, 1, 3), dtype=F32)
    image[0::2, 0], image[1::2, 0] = F32(list(m.tex_color_a)), F32(list(m.tex_color_b))
    assert m.tex_frequency == 20.0
    hits_t = dev(made_hits(1000, ref.stripe, 1))
    want = materials.material_hits(ref.scene, hits_t)
    got = want.clone()
    got[:, 3:6] = 0
    T.apply(got, hits_t, T.Texture(image, filter=T.NEAREST, n_levels=1))
    colours = np.unique(u32(want)[:, 3:6], axis=0)
    assert len(colours) == 2 and G.same_bits(u32(got), u32(want))


def test_a_normal_map_of_material_hits_own_normals_gives_its_shading_normal(ref):
    w = 64
    hits = made_hits(w, ref.wave, 2)
    hits.view(F32)[:, 9] = (np.arange(w, dtype=F32) + F32(0.5)) / F32(w)  # texel centres
    hits_t = dev(hits)
    want = materials.material_hits(ref.scene, hits_t)
    normals = u32(want)[:, 0:3].view(F32)
    assert len(np.unique(normals, axis=0)) > w // 2  # the wave: the normal depends on u
    tex = T.Texture(normals.reshape(1, w, 3).copy(), filter=T.NEAREST, n_levels=1)
    got = want.clone()
    got[:, 0:3] = 0
    got[:, 14:17] = 0
    T.apply(got, hits_t, None, tex)
    assert G.same_bits(u32(got), u32(want))


# ---- the light terms and the sequences ----

def shadow_casts(ref):
    rays, asks, _ = rt.light_rays(ref.scene, ref.hits_t, ref.rays_t)
    index, count = rt.select_records(asks)
    shadow_hits = torch_device().zeros((asks.shape[0], 13), dtype=torch_device().int32, device="cuda")
    rt.cast_rays_indexed(ref.scene, rays, index, count, shadow_hits)
    return asks, shadow_hits


def test_light_terms_on_unedited_surfaces_are_light_terms(ref):
    asks, shadow_hits = shadow_casts(ref)
    want = rt.light_terms(ref.scene, ref.hits_t, ref.rays_t, asks, shadow_hits)
    got = T.light_terms_surfaces(ref.scene, ref.surfaces_t, ref.hits_t, ref.rays_t, asks, shadow_hits)
    assert host(want[0]).any() and host(want[2]).any()
    assert np.array_equal(host(got[0]), host(want[0]))
    assert G.same_or_both_nan(host(got[1]), host(want[1])) and G.same_or_both_nan(host(got[2]), host(want[2]))
    part = T.light_terms_surfaces(ref.scene, ref.surfaces_t, ref.hits_t, ref.rays_t, asks[ref.n:2 * ref.n], shadow_hits[ref.n:2 * ref.n], 1, 1)
    assert G.same_or_both_nan(host(part[1]), host(want[1])[ref.n:2 * ref.n])


def test_light_terms_on_edited_surfaces_are_probe_surfaces_times_the_light(ref):
    """an independent check on edited records: for a directional light approximate_into_directional returns the light itself, so the
    terms of the pairs nothing occludes are rt_probe_surfaces' answers to (shading_normal, -view, -light.direction) times the light's
    colour — the record's own diffuse_color AND its own shading normal, not the scene's"""
    torch = torch_device()
    first = next(i for i in range(ref.desc.n_lights) if ref.desc.lights[i].kind == 0)
    light = ref.desc.lights[first]
    surfaces_t = ref.surfaces_t.clone()
    T.apply(surfaces_t, ref.hits_t, T.Texture(ref.colour_img, filter=T.BILINEAR, scale=(4.0, 4.0)), T.Texture(ref.normal_img, filter=T.BILINEAR),
            None, T.ALL_OBJECTS, T.NORMALIZE)
    edited, plain = u32(surfaces_t), ref.surfaces
    assert (edited[:, 3:6] != plain[:, 3:6]).any() and (edited[:, 14:17] != plain[:, 14:17]).any()
    asks, shadow_hits = shadow_casts(ref)
    one = slice(first * ref.n, (first + 1) * ref.n)
    lit, diffuse, specular = T.light_terms_surfaces(ref.scene, surfaces_t, ref.hits_t, ref.rays_t, asks[one], shadow_hits[one], first, 1)
    view = (-ref.rays_t[:, 3:6].view(torch.float32)).contiguous()
    towards = torch.tensor(-np.array(list(light.direction), dtype=F32), device="cuda").expand(1, ref.n, 3).contiguous()
    colour = np.array(list(light.color), dtype=F32)
    lit = host(lit) != 0
    assert lit.sum() > 20
    for got, probe, other in zip((diffuse, specular), materials.probe_surfaces(surfaces_t, view, towards),
                                 materials.probe_surfaces(ref.surfaces_t, view, towards)):
        want = host(probe).reshape(ref.n, 3) * colour
        assert G.same_or_both_nan(host(got)[lit], want[lit])
        assert not G.same_or_both_nan(host(got)[lit], (host(other).reshape(ref.n, 3) * colour)[lit])  # the edit reaches the term
        assert not host(got)[~lit].any()


def test_without_bindings_the_sequences_are_the_plain_ones(ref):
    torch = torch_device()
    count, plain = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
    want = rt.shade_hits(ref.scene, ref.hits_t, ref.rays_t, ray_count=plain)
    got = T.shade_hits_textured(ref.scene, ref.hits_t, ref.rays_t, None, ray_count=count)
    assert host(want).any() and G.same_or_both_nan(host(got), host(want)) and int(count.item()) == int(plain.item()) > 0
    count.zero_(), plain.zero_()
    want = rt.trace_rays_levels(ref.scene, ref.rays_t, 3, ray_count=plain)
    got = T.trace_rays_levels(ref.scene, ref.rays_t, 3, ray_count=count, bindings=[])
    assert G.same_or_both_nan(host(got), host(want)) and int(count.item()) == int(plain.item()) > 0


def test_with_a_binding_shade_hits_textured_is_its_restatement(ref):
    torch = torch_device()
    colour_t, colour = pair(ref.colour_img, filter=T.TRILINEAR, scale=(4.0, 4.0))
    normal_t, normal = pair(ref.normal_img, filter=T.BILINEAR)
    objects = np.unique(ref.hits[ref.hits[:, 0] <= 1, 2])
    first = int(objects[0])
    bindings = [T.Binding(colour_t, None, first, T.MODULATE), T.Binding(None, normal_t, T.ALL_OBJECTS, T.NORMALIZE)]
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    got = T.shade_hits_textured(ref.scene, ref.hits_t, ref.rays_t, bindings, spread=0.05, ray_count=count)
    # the restatement: the CPU forms edit the surfaces, the public calls light them
    foot = T.footprint_numpy(ref.world, ref.hits, ref.rays, 0.05)
    surfaces = T.apply_numpy(ref.surfaces, ref.hits, colour, None, foot, first, T.MODULATE)
    surfaces = T.apply_numpy(surfaces, ref.hits, None, normal, foot, T.ALL_OBJECTS, T.NORMALIZE)
    assert (surfaces != ref.surfaces).any()
    asks, shadow_hits = shadow_casts(ref)
    lit, diffuse, specular = T.light_terms_surfaces(ref.scene, dev(surfaces), ref.hits_t, ref.rays_t, asks, shadow_hits)
    want = rt.light_fold(ref.scene, ref.hits_t, lit, diffuse, specular, torch.zeros((ref.n, 3), dtype=torch.float32, device="cuda"))
    plain_count = torch.zeros(1, dtype=torch.int64, device="cuda")
    plain = rt.shade_hits(ref.scene, ref.hits_t, ref.rays_t, ray_count=plain_count)
    assert G.same_or_both_nan(host(got), host(want)) and not G.same_or_both_nan(host(got), host(plain))
    assert int(count.item()) == int(plain_count.item()) > 0  # the shadow rays are light_rays' either way
    levels = T.trace_rays_levels(ref.scene, ref.rays_t, 2, bindings=bindings, spread=0.05)
    assert not G.same_or_both_nan(host(levels), host(rt.trace_rays_levels(ref.scene, ref.rays_t, 2)))


# ---- the footprint reads the live vertices ----

def test_footprint_reads_the_new_vertices():
    world = rt.reference_world()
    d = world.desc()
    scene = rt.Scene(world)
    rays_t = rt.camera_rays(rt.reference_camera(), rt.Frame.full(WIDTH, HEIGHT, 0))
    hits = u32(rt.cast_rays(scene, rays_t))
    on_triangles = hits[hits[:, 0] == 1]
    tri = int(np.bincount(on_triangles[:, 1]).argmax())
    before = host(T.footprint(scene, dev(hits), rays_t, 0.01))
    triangles = (_capi.Triangle * d.n_triangles)()
    C.memmove(triangles, d.triangles, C.sizeof(triangles))
    for k in range(3):  # the same triangle with its uv spread four times as far: sixteen times the uv area
        for c in range(2):
            triangles[tri].vertices[k].uv[c] *= 4.0
    scene.update_vertices(tri, (_capi.Vertex * 3)(*triangles[tri].vertices))
    moved = _capi.SceneDesc(triangles, d.n_triangles, d.spheres, d.n_spheres, d.materials, d.n_materials, d.lights, d.n_lights)
    after = host(T.footprint(scene, dev(hits), rays_t, 0.01))
    mine = (hits[:, 0] == 1) & (hits[:, 1] == tri)
    assert mine.any() and before[mine].all()
    assert G.same_bits(after, T.footprint_numpy(moved, hits, u32(rays_t), 0.01)) and G.same_bits(before, T.footprint_numpy(world, hits, u32(rays_t), 0.01))
    assert np.allclose(after[mine], before[mine] * 4, rtol=1e-6) and G.same_bits(after[~mine], before[~mine])


# ---- capture ----

def test_the_calls_replay_from_a_graph(ref):
    torch = torch_device()
    n = ref.n
    colour = T.Texture(ref.colour_img, filter=T.TRILINEAR, scale=(4.0, 4.0))
    normal = T.Texture(ref.normal_img, filter=T.BILINEAR)
    asks, shadow_hits = shadow_casts(ref)
    pairs = asks.shape[0]

    def run(foot, surfaces, lit, diffuse, specular, stream=None):
        surfaces.copy_(ref.surfaces_t)
        T.footprint(ref.scene, ref.hits_t, ref.rays_t, 0.05, None, foot, stream=stream)
        T.apply(surfaces, ref.hits_t, colour, normal, foot, T.ALL_OBJECTS, T.NORMALIZE, stream=stream)
        T.light_terms_surfaces(ref.scene, surfaces, ref.hits_t, ref.rays_t, asks, shadow_hits, 0, None, lit, diffuse, specular, stream=stream)

    def buffers():
        return (torch.full((n,), 7.0, dtype=torch.float32, device="cuda"), torch.zeros((n, 18), dtype=torch.int32, device="cuda"),
                torch.full((pairs,), 9, dtype=torch.uint8, device="cuda"), torch.full((pairs, 3), 7.0, dtype=torch.float32, device="cuda"),
                torch.full((pairs, 3), 7.0, dtype=torch.float32, device="cuda"))

    want = buffers()
    run(*want)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        got = buffers()
        stream.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):  # no call of the block ran on this stream before: capturable at once
            run(*got, stream=stream)
        for _ in range(2):
            for t in got:
                t.fill_(3)
            graph.replay()
            stream.synchronize()
            for g, w in zip(got, want):
                assert G.same_or_both_nan(host(g).view(np.uint8).view(F32), host(w).view(np.uint8).view(F32))
    assert host(want[2]).any() and host(want[0]).any()
