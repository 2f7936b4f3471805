"""The environment queries on the CPU (include/rt_environment_host.h; the arithmetic is csrc/rt_environment.h's, which the device
shares): the table against an independent numpy model word for word, degenerate images, the two inverse-CDF brackets in exact integers,
the round trip from a sample through the lookup back to its texel, the density against its formula and against a Monte-Carlo integral,
the lookup's centres, seam, poles and rotation, and the fold against a plain loop.  No GPU."""
import math

import numpy as np
import pytest

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import _capi, environment as E

F32 = np.float32
T = E.ROW_TILE
UP = np.array([[0.0, 1.0, 0.0]], dtype=F32)


def words(a):
    a = np.ascontiguousarray(a)
    return a if a.dtype.itemsize == 1 else a.view(np.uint32)


def library_sin(x):
    """rtdm::sinf of f32 angles: rt_math_eval_host(RT_MATH_SIN)"""
    x = np.ascontiguousarray(x, dtype=F32)
    y, out = np.zeros_like(x), np.zeros_like(x)
    _capi.check(_capi.amd_lib().rt_math_eval_host(0, x.ctypes.data, y.ctypes.data, out.ctypes.data, x.size))
    return out


def image(width, height, seed, spoiled=True):
    rng = np.random.default_rng(seed)
    img = rng.random((height, width, 3), dtype=F32) * F32(4)
    if spoiled and width * height >= 6:
        flat = img.reshape(-1, 3)
        k = rng.permutation(flat.shape[0])[:4]
        flat[k[0], 1], flat[k[1], 0], flat[k[2]], flat[k[3]] = np.nan, np.inf, -1.0, 0.0
    return img


def model(img):
    """the table restated: weights in float32 numpy in the documented order, the library's sine, np.cumsum on the integers"""
    height, width, _ = img.shape
    l0, l1, l2 = (F32(v) for v in rt.luma_row())
    sin_row = library_sin(F32(3.1415927) * (np.arange(height, dtype=F32) + F32(0.5)) / F32(height))
    r, g, b = img[..., 0], img[..., 1], img[..., 2]
    with np.errstate(all="ignore"):
        w = ((r * l0 + g * l1) + b * l2) * sin_row[:, None]
        assert w.dtype == F32
        usable = np.isfinite(r) & np.isfinite(g) & np.isfinite(b) & np.isfinite(w) & (w > 0)
        w_max = w[usable].max() if usable.any() else F32(0)
        steps = np.where(usable, w / w_max * F32(65534.0), F32(0))
        assert steps.dtype == F32
    q = np.where(usable, 1 + steps.astype(np.uint32), 0).astype(np.uint64)
    c = np.cumsum(q, axis=1)
    assert c.max(initial=0) < 1 << 32
    return dict(width=width, height=height, total=int(c[:, -1].sum()), w_max=w_max, M=np.cumsum(c[:, -1]), C=c.astype(np.uint32), q=q, usable=usable)


# ---- the table ----

@pytest.mark.parametrize("width,height", [(1, 1), (3, 2), (64, 4), (65, 4), (T, 2), (T + 1, 2), (5, 1), (5, 257)])
def test_the_table_is_the_model(width, height):
    for seed in (1, 2):
        img = image(width, height, seed, spoiled=seed == 1)
        got, want = E.table_fields(E.table_numpy(img), width, height), model(img)
        assert (got["width"], got["height"], got["total"], got["pad"]) == (width, height, want["total"], 0)
        assert words(got["w_max"]) == words(want["w_max"])
        assert (got["M"] == want["M"]).all() and (got["C"] == want["C"]).all()
        assert got["total"] > 0 and got["C"].max() <= 65535 * width


def test_every_texel_that_carries_light_can_be_sampled():
    img = np.full((2, 3, 3), 1e-30, dtype=F32)
    img[0, 0] = 1e30
    m = model(img)
    got = E.table_fields(E.table_numpy(img), 3, 2)
    assert m["usable"].all() and (m["q"].reshape(-1)[1:] == 1).all() and m["q"][0, 0] == 65535
    assert (got["C"] == m["C"]).all()


def samples(img, n, spp=1, pattern=E.UNIFORM, seed=3, rotation=0.0, scale=1.0, normals=None):
    normals = np.tile(UP, (n, 1)) if normals is None else normals
    with np.errstate(all="ignore"):
        return E.samples_numpy(img, E.table_numpy(img), normals, spp, pattern, seed, None, rotation, scale)


def test_degenerate_images():
    # all zero: total 0, nothing asks, every output zero
    dark = np.zeros((4, 8, 3), dtype=F32)
    assert E.table_fields(E.table_numpy(dark), 8, 4)["total"] == 0
    assert all(not a.any() for a in samples(dark, 64, 4))
    # one usable texel: every sample goes there and every direction maps back to it
    one = np.zeros((4, 8, 3), dtype=F32)
    one[2, 5] = (1, 2, 3)
    dirs, radiance, texel, asks = samples(one, 256, 4, normals=np.tile(np.array([[0, -1, 0]], dtype=F32), (256, 1)))
    assert (texel == 2 * 8 + 5).all() and asks.all()  # row 2 lies below the horizon: it asks about the normal -y
    back = E.lookup_numpy(one, dirs.reshape(-1, 3), filter=E.NEAREST)
    assert (back == np.array([1, 2, 3], dtype=F32)).all()
    # NaN, Inf and negative texels get q = 0 and are never sampled; an all-zero row is never chosen
    img = image(8, 6, 7, spoiled=False)
    img[1, 2, 0], img[4, 4, 2], img[0, 7], img[3] = np.nan, np.inf, -2.0, 0.0
    fields = E.table_fields(E.table_numpy(img), 8, 6)
    q = np.diff(np.concatenate([np.zeros((6, 1), dtype=np.int64), fields["C"].astype(np.int64)], axis=1), axis=1)
    assert q[1, 2] == 0 and q[4, 4] == 0 and q[0, 7] == 0 and not q[3].any() and (q > 0).sum() == 48 - 3 - 8
    _, _, texel, _ = samples(img, 4096, 4, E.STRATIFIED)
    seen = np.bincount(texel.reshape(-1), minlength=48).reshape(6, 8)
    assert not seen[q == 0].any() and seen[q > 0].all()


# ---- the brackets ----

def film_mix(v):
    v = np.asarray(v, dtype=np.uint32).copy()
    with np.errstate(over="ignore"):
        v ^= v >> np.uint32(16)
        v *= np.uint32(0x7FEB352D)
        v ^= v >> np.uint32(15)
        v *= np.uint32(0x846CA68B)
        v ^= v >> np.uint32(16)
    return v


def uniform_pair(ids, seed, s):
    """(u_0, u_1) of the documented hash for RT_FILM_UNIFORM, in numpy f32"""
    with np.errstate(over="ignore"):
        seed_e = film_mix(np.uint32(seed) ^ np.uint32(0xC2B2AE35))
        pair = []
        for axis in (0, 1):
            h = film_mix(film_mix(np.asarray(ids, dtype=np.uint32) + seed_e) ^ np.uint32(2 * s + axis))
            pair.append(((h >> np.uint32(8)).astype(F32) * F32(2.0 ** -24) - F32(0.5)) + F32(0.5))
    return pair


def test_the_sample_lies_in_both_brackets():
    """M[y - 1] <= t < M[y] and C[y][x - 1] <= tx < C[y][x], in exact integers"""
    n = 4096
    img = image(16, 8, 11)
    fields = E.table_fields(E.table_numpy(img), 16, 8)
    _, _, texel, _ = samples(img, n, 1, E.UNIFORM, seed=5)
    u0, u1 = uniform_pair(np.arange(n), 5, 0)
    total = fields["total"]
    m = [0] + [int(v) for v in fields["M"]]
    for i in range(n):
        y, x = divmod(int(texel[0, i]), 16)
        t = min(int(float(u0[i]) * float(total)), total - 1)
        assert m[y] <= t < m[y + 1], i
        rowsum = m[y + 1] - m[y]
        tx = min(int(float(u1[i]) * float(rowsum)), rowsum - 1)
        row = [0] + [int(v) for v in fields["C"][y]]
        assert row[x] <= tx < row[x + 1], i
    assert np.unique(texel).size > 100


# ---- the round trip and the density ----

def texel_space(dirs, width, height, rotation):
    d = dirs.astype(np.float64)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    theta = np.arccos(np.clip(d[..., 1], -1, 1))
    phi = np.mod(np.arctan2(d[..., 2], d[..., 0]) - rotation, 2 * math.pi)
    return phi * width / (2 * math.pi), theta * height / math.pi


def test_a_sample_looks_its_own_texel_up():
    """lookup_numpy(NEAREST) of every sampled direction is the sampled texel * scale, but within 1e-4 rad of a texel edge (measured in
    float64 from the direction), where either neighbour may answer; that band holds fewer than 1 % of the samples"""
    width, height, rotation, scale = 8, 4, 0.7, 2.5
    img = image(width, height, 13, spoiled=False)
    dirs, radiance, texel, asks = samples(img, 4096, 4, E.STRATIFIED, 9, rotation, scale)
    flat = dirs.reshape(-1, 3)
    got = E.lookup_numpy(img, flat, rotation, scale, E.NEAREST)
    want = img.reshape(-1, 3)[texel.reshape(-1)] * F32(scale)
    x_f, y_f = texel_space(flat, width, height, rotation)
    near = (np.abs(x_f - np.round(x_f)) * (2 * math.pi / width) < 1e-4) | (np.abs(y_f - np.round(y_f)) * (math.pi / height) < 1e-4)
    same = (words(got) == words(want)).all(axis=1)
    assert same[~near].all(), np.flatnonzero(~same & ~near)[:5]
    assert near.sum() < 0.01 * near.size, near.sum()
    # ... and the radiance is that texel * scale / pdf with the documented density
    fields = E.table_fields(E.table_numpy(img), width, height)
    q = np.diff(np.concatenate([np.zeros((height, 1)), fields["C"].astype(np.float64)], axis=1), axis=1).reshape(-1)[texel.reshape(-1)]
    d = flat.astype(np.float64)
    sin_theta = np.hypot(d[:, 0], d[:, 2]) / np.linalg.norm(d, axis=1)
    pdf = q / fields["total"] * (width * height) / (2 * math.pi ** 2 * sin_theta)
    ask = asks.reshape(-1) == 1
    assert ask.sum() > 0.3 * ask.size and not radiance.reshape(-1, 3)[~ask].any()
    recovered = want[ask].astype(np.float64) / radiance.reshape(-1, 3)[ask].astype(np.float64)
    assert np.abs(recovered / pdf[ask, None] - 1).max() < 1e-5


def test_the_density_integrates_the_cosine_to_pi():
    """a constant sky, 65 536 uniform samples about +y: the mean of max(dir.y, 0) / pdf is the integral of the clamped cosine over the
    sphere, pi; under uniform sphere sampling that estimator has variance 5 pi^2 / 3, and the bound is six standard errors (0.095)"""
    width, height, n = 128, 64, 65536
    img = np.ones((height, width, 3), dtype=F32)
    dirs, radiance, _, asks = samples(img, n, 1, E.UNIFORM, 21)
    pdf = np.where(asks[0] == 1, 1.0 / np.maximum(radiance[0, :, 0].astype(np.float64), 1e-300), np.inf)  # texel * scale = 1
    estimate = (np.maximum(dirs[0, :, 1].astype(np.float64), 0) / pdf).mean()
    bound = 6 * math.sqrt(5 * math.pi ** 2 / 3) / math.sqrt(n)
    assert abs(estimate - math.pi) < bound, (estimate, bound)
    assert abs(np.median(radiance[0][asks[0] == 1].astype(np.float64)) / (4 * math.pi) - 1) < 0.05  # 1 / pdf: close to uniform on the sphere
    print(f"estimate {estimate:.5f}, pi {math.pi:.5f}, bound {bound:.5f}")


# ---- the lookup ----

def centre_dirs(width, height, rotation=0.0):
    x, y = np.meshgrid(np.arange(width) + 0.5, np.arange(height) + 0.5)
    theta, phi = math.pi * y / height, 2 * math.pi * x / width + rotation
    return np.stack([np.sin(theta) * np.cos(phi), np.cos(theta), np.sin(theta) * np.sin(phi)], axis=-1).reshape(-1, 3).astype(F32)


def test_texel_centres_return_the_texel():
    """NEAREST at every centre of an odd-sized image; BILINEAR on 4 x 2, whose centres lie on the diagonals theta, phi = odd multiples of
    pi / 4, where every step of the inverse map is exact and both weights are 0 or 1; on the odd-sized image BILINEAR is the texel to
    the rounding of the inverse map"""
    img = image(7, 5, 17, spoiled=False)
    got = E.lookup_numpy(img, centre_dirs(7, 5), 0.0, 3.0, E.NEAREST)
    assert (words(got) == words(img.reshape(-1, 3) * F32(3))).all()
    small = image(4, 2, 19, spoiled=False)
    for filter in (E.NEAREST, E.BILINEAR):
        got = E.lookup_numpy(small, centre_dirs(4, 2), 0.0, 3.0, filter)
        assert (words(got) == words(small.reshape(-1, 3) * F32(3))).all(), filter
    close = E.lookup_numpy(img, centre_dirs(7, 5), 0.0, 3.0, E.BILINEAR)
    assert np.abs(close - img.reshape(-1, 3) * F32(3)).max() < 1e-4


def test_the_seam_the_poles_and_the_rotation():
    width, height = 8, 4
    img = image(width, height, 23, spoiled=False)
    # half-way across the phi seam, on a row's centre line: the mean of column W - 1 and column 0
    theta = math.pi * 1.5 / height
    seam = np.array([[math.sin(theta), math.cos(theta), 0.0]], dtype=F32)
    got = E.lookup_numpy(img, seam, 0.0, 1.0, E.BILINEAR)[0]
    x_f, y_f = texel_space(seam, width, height, 0.0)
    assert x_f[0] == 0 and abs(y_f[0] - 1.5) < 1e-6
    assert np.abs(got - (img[1, width - 1] * F32(0.5) + img[1, 0] * F32(0.5))).max() < 1e-5
    # the poles clamp: straight up is row 0, straight down row H - 1, in both filters, whatever lies "beyond"
    for filter in (E.NEAREST, E.BILINEAR):
        up, down = E.lookup_numpy(img, np.array([[0, 2, 0], [0, -3, 0]], dtype=F32), 0.0, 1.0, filter)
        row0 = img[0, 0] if filter == E.NEAREST else img[0, width - 1] * F32(0.5) + img[0, 0] * F32(0.5)  # atan2(0, 0) = 0: the seam
        rowl = img[height - 1, 0] if filter == E.NEAREST else img[height - 1, width - 1] * F32(0.5) + img[height - 1, 0] * F32(0.5)
        assert np.abs(up - row0).max() < 1e-6 and np.abs(down - rowl).max() < 1e-6
    # a rotation of 2 pi k / W shifts the columns by k
    for k in (1, 3, -2):
        turned = E.lookup_numpy(img, centre_dirs(width, height), 2 * math.pi * k / width, 1.0, E.NEAREST).reshape(height, width, 3)
        assert (words(turned) == words(np.roll(img, k, axis=1))).all(), k
    # a zero, NaN or Inf direction gives +0
    bad = np.array([[0, 0, 0], [-0.0, 0, 0], [np.nan, 1, 0], [1, np.inf, 0], [0, 1, -np.inf], [3e38, 3e38, 0]], dtype=F32)
    for filter in (E.NEAREST, E.BILINEAR):
        with np.errstate(all="ignore"):
            assert not words(E.lookup_numpy(img, bad, 0.0, 1.0, filter)).any()
    # NaN and Inf texels pass through
    img[2, 3] = (np.nan, np.inf, 1)
    got = E.lookup_numpy(img, centre_dirs(width, height)[2 * width + 3:2 * width + 4], 0.0, 1.0, E.NEAREST)[0]
    assert np.isnan(got[0]) and np.isinf(got[1]) and got[2] == 1


# ---- the fold ----

def test_the_fold_with_unit_radiance_is_its_formula():
    """radiance = 1: the first open sample starts each accumulator, every later one is added, then (rgb + D (1 - shiness)) + S shiness,
    one float32 operation at a time"""
    rng = np.random.default_rng(29)
    n, spp = 37, 4
    valid = (rng.random(n) < 0.8).astype(np.uint8)
    shiness = rng.random(n, dtype=F32)
    asks = (rng.random((spp, n)) < 0.7).astype(np.uint8)
    shadow = np.zeros((spp * n, 13), dtype=np.uint32)
    shadow[:, 0] = rng.choice([0, 1, 0xFFFFFFFF, 7], size=spp * n)
    diffuse, specular = rng.random((spp, n, 3), dtype=F32), rng.random((spp, n, 3), dtype=F32)
    rgb = rng.random((n, 3), dtype=F32)
    open_, got = E.fold_numpy(valid, shiness, asks, spp, np.ones((spp, n, 3), dtype=F32), diffuse, specular, rgb, shadow)
    want_open = (asks == 1) & (valid[None] == 1) & (shadow[:, 0].reshape(spp, n) > 1)
    assert (open_.reshape(spp, n) == want_open).all() and want_open.any(axis=0).sum() > 5 and (~want_open.any(axis=0)).sum() > 2
    want = rgb.copy()
    for i in range(n):
        acc_d = acc_s = None
        for s in range(spp):
            if want_open[s, i]:
                acc_d = diffuse[s, i] if acc_d is None else acc_d + diffuse[s, i]
                acc_s = specular[s, i] if acc_s is None else acc_s + specular[s, i]
        if acc_d is not None:
            d, sp = acc_d / F32(spp), acc_s / F32(spp)
            want[i] = (rgb[i] + d * (F32(1) - shiness[i])) + sp * shiness[i]
    assert want.dtype == F32 and (words(got) == words(want)).all()
    # without shadow hits nothing occludes
    open_all, _ = E.fold_numpy(valid, shiness, asks, spp, np.ones((spp, n, 3), dtype=F32), diffuse, specular, rgb)
    assert (open_all.reshape(spp, n) == ((asks == 1) & (valid[None] == 1))).all()
