"""Shared test support for the post stage (csrc/rt_post.hip: the radix select of post_process, the key map, the sRGB / u8 encode, the
photon accumulator): plain numpy references that share nothing with csrc/ or dist.py, the adversarial key sets of the select tests, and
the tolerance of the encode test with its derivation.

THE SELECT.  The device finds the k-th smallest key by a four-pass radix select; the reference sorts (select_reference).  What state[1]
must hold after the pick of pass p follows from the sort too: the rank of the selected key among the keys that share its top p + 1 bytes
(select_trace).  radix_model() is NOT a reference: it restates the radix select so that test_post_reference.py can switch one step to a
named wrong form and show, on the CPU, that a key set would tell the two apart.

THE ENCODE TOLERANCE (ENCODE_DELTA).  The float64 reference evaluates the sRGB transfer with the decimal constants and the exponent
1 / 2.4; the f32 forms (rt_host.cpp, rt_post.hip) compute r = fl(fl(fl(1.055f * powf(x, EF)) - 0.055f) * 255) with EF = fl(1.0f / 2.4f).
With u = 2^-24 (every rounding, of a constant or of an operation, is relative u at most), for the x in (0.0031308, 1] that matter — the
transfer is 1 at x = 1 and r is clamped above it:
  powf   within 1 ulp of the correctly rounded power (tests/test_detmath_cpu.py), so within 1.5 ulp <= 3u of x^EF; and x^EF = x^(1/2.4) *
         exp((EF - 1/2.4) ln x), a relative |EF - 1/2.4| * |ln x|.  Absolute, on p = x^(1/2.4) <= 1: 3u * p + |EF - 1/2.4| * sup(p |ln x|),
         the supremum at x = e^-2.4, where it is 2.4 / e.
  1.055f relative u (the constant) + u (the product), on 1.055 * p <= 1.055.
  0.055f relative u on 0.055; the subtraction relative u on a result e <= 1.
  * 255  relative u on e <= 1.
  |r_f32 - r_exact| <= 255 * (1.055 * (5u + |EF - 1/2.4| * 2.4 / e) + 0.055u + 2u)          = ENCODE_DELTA, about 1.2e-4.
The linear branch r = fl(fl(12.92f * x) * 255) is within 255 * 12.92 * 0.0031308 * 3u, sixty times less; no float lies between 0.0031308
and its f32 rounding, and at that one float the two branches of the exact transfer differ by less than 1e-5 * 255 (test_post_reference.py
asserts both).  Truncation moves the byte only when r_f32 and r_exact lie on different sides of an integer: never by more than 1, and
only where r_exact is within ENCODE_DELTA of that integer.
MEASURED on the host form (x86-64, the whole input set of encode_inputs(), test_post_reference.py prints it): the largest distance from
an integer at which rt_encode_srgb8 and the float64 reference give different bytes is recorded next to ENCODE_MEASURED below; the bound
used is the derived one.
THE CAP (encode_excused_cap).  ENCODE_DELTA adds six worst cases with one sign.  A byte differs only if the error exceeds the distance to
the integer, so an error of half the bound at most flips the inputs within ENCODE_DELTA / 2 of an integer: their number — a property of
the reference and the input set alone — is the cap on differing bytes.  A systematic error of the size of the bound (a wrong constant in
the last place, a powf 2 ulp off) flips more than that.
"""
import functools

import numpy as np

F32 = np.float32
KEY_INVALID = 0xFFFFFFFF
STATE_WORDS = 260
GRID_CAP = 2048 * 256  # grid_for(): beyond this many elements the kernels of rt_post.hip run grid-stride
EPSILON = F32(2.0 ** -23)  # f32::EPSILON
MIN_NORMAL = F32(2.0 ** -126)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- the select ---------------------------------------------------------------------------------------------------------------------

def rank_wanted(count):
    """(len as f32 * 0.99) as usize (main.rs:754), clamped to the last element"""
    return min(int(F32(count) * F32(0.99)), count - 1)


def select_reference(keys):
    """the key main.rs:754 indexes after its sort, or None without a valid key"""
    valid = np.sort(keys[keys != KEY_INVALID])
    return None if valid.size == 0 else int(valid[rank_wanted(valid.size)])


def select_trace(keys):
    """per pass p: (the histogram the pass must see, the digit it must pick, state[1] after the pick) — all from the sort"""
    valid = np.sort(keys[keys != KEY_INVALID]).astype(np.uint64)
    if valid.size == 0:
        return []
    k = rank_wanted(valid.size)
    target = int(valid[k])
    out = []
    for p in range(4):
        shift = 24 - 8 * p
        group = valid[(valid >> np.uint64(shift + 8)) == np.uint64(target >> (shift + 8))] if p else valid
        hist = np.bincount(((group >> np.uint64(shift)) & np.uint64(0xFF)).astype(np.int64), minlength=256)
        below = int(np.searchsorted(valid >> np.uint64(shift), np.uint64(target >> shift), side="left"))
        out.append((hist, (target >> shift) & 0xFF, k - below))
    return out


def radix_model(keys, pick_le=False, drop_mask_byte=None, count_invalid=False):
    """The four-pass radix select restated, with one step optionally WRONG: pick_le takes `k <= c` for `k < c`; drop_mask_byte = j leaves
    byte j (0 = the top one) out of the prefix comparison of the later passes; count_invalid lets KEY_INVALID into the histograms.
    Returns (the key, the histograms seen).  With no switch set it is the select; test_post_reference.py holds it to the sort."""
    keys = keys.astype(np.uint64)
    count = int((keys != KEY_INVALID).sum())
    if count == 0:
        return None, []
    k, prefix, hists = rank_wanted(count), 0, []
    for p in range(4):
        shift = 24 - 8 * p
        mask = 0 if p == 0 else (0xFFFFFFFF << (shift + 8)) & 0xFFFFFFFF
        if drop_mask_byte is not None and drop_mask_byte < p:
            mask &= ~(0xFF << (24 - 8 * drop_mask_byte)) & 0xFFFFFFFF
        take = (keys & np.uint64(mask)) == np.uint64(prefix & mask)
        if not count_invalid:
            take &= keys != KEY_INVALID
        hist = np.bincount(((keys[take] >> np.uint64(shift)) & np.uint64(0xFF)).astype(np.int64), minlength=256)
        hists.append(hist)
        digit = 255
        for d in range(256):
            c = int(hist[d])
            if (k <= c) if pick_le else (k < c):
                digit = d
                break
            k -= c
        prefix |= digit << shift
    return prefix, hists


def _u32(x):
    return np.asarray(x, dtype=np.uint64).astype(np.uint32)


def _with_byte(base, p, values):
    """`base` with byte p (0 = the top one) replaced by each of `values`"""
    shift = 24 - 8 * p
    return _u32((np.uint64(base) & np.uint64(~(0xFF << shift) & 0xFFFFFFFF)) | (np.asarray(values, dtype=np.uint64) << np.uint64(shift)))


def boundary_sets(p, n=300):
    """Three key sets whose pass p has the bins 0x10, 0x20, 0x30 under one common prefix, the bytes below p distinct per key.  With k the
    rank wanted: the cumulative count through bin 0x10 is k (the rank is the first key of 0x20), k + 1 (the last key of 0x10), and k - 1
    with a bin 0x20 of one key (the rank is the first key of 0x30).  `k < c` against `k <= c` differ on the first and the third."""
    k = rank_wanted(n)
    assert n - k >= 3
    out = []
    for a, b in ((k, n - k - 1), (k + 1, 1), (k - 1, 1)):
        digits = np.repeat([0x10, 0x20, 0x30], [a, b, n - a - b])
        low_bits = 24 - 8 * p  # the bits below byte p
        keys = _with_byte(0x80402010 & ~((1 << low_bits) - 1), p, digits).astype(np.uint64)
        if low_bits:
            keys |= (np.arange(n, dtype=np.uint64) * np.uint64(2654435761)) & np.uint64((1 << low_bits) - 1)
        out.append(_u32(keys)[np.random.default_rng(100 + p).permutation(n)])
    return out


DECOY_TRUE_PREFIX = (0x80, 0x10, 0x20)
DECOY_N, DECOY_REAL, DECOY_RANK = 2000, 5, 2  # of 2000 keys 5 are real, and the rank wanted is the third of them


def decoy_set(p):
    """The prefix decoys of pass p (1, 2 or 3).  The 5 real keys carry the true prefix 0x80 0x10 0x20 in their top p bytes and the digits
    0x40 .. 0x44 in byte p.  For every higher byte j < p there are two classes of decoys that differ from the true prefix in byte j ALONE,
    by -1 (0x7f for j = 0) and by +1 (0x81), each class at least as numerous as the real keys, all with the digit 0x05 in byte p.  The
    classes below hold what is needed for the rank wanted to be the real key with digit 0x42.  A select that leaves byte j out of its mask
    counts both classes of j into pass p's bin 0x05, at least ten keys below 0x40, and ends with a 0x05 key."""
    n, real, r = DECOY_N, DECOY_REAL, DECOY_RANK
    k = rank_wanted(n)
    above_total = n - (k - r) - real
    below_total = k - r
    above = [above_total // p + (1 if j < above_total % p else 0) for j in range(p)]
    below = [below_total // p + (1 if j < below_total % p else 0) for j in range(p)]
    assert min(above) >= real and min(below) >= real
    rng = np.random.default_rng(200 + p)
    true = 0
    for j in range(p):
        true |= DECOY_TRUE_PREFIX[j] << (24 - 8 * j)
    low_bits = 24 - 8 * p  # the bits below byte p
    parts = [_u32(np.uint64(true) | (np.arange(0x40, 0x40 + real, dtype=np.uint64) << np.uint64(low_bits)) | np.uint64(rng.integers(0, 1 << low_bits) if low_bits else 0))]
    for j in range(p):
        for count, delta in ((below[j], -1), (above[j], +1)):
            prefix = (true & ~(0xFF << (24 - 8 * j)) & 0xFFFFFFFF) | ((DECOY_TRUE_PREFIX[j] + delta) << (24 - 8 * j))
            tail = rng.integers(0, 1 << low_bits, count, dtype=np.uint64) if low_bits else np.zeros(count, np.uint64)
            parts.append(_u32(np.uint64(prefix) | (np.uint64(0x05) << np.uint64(low_bits)) | tail))
    keys = np.concatenate(parts)
    assert keys.size == n
    return keys[rng.permutation(n)]


def _spread_keys(rng, n):
    """n distinct keys over every top byte, both halves of the key space (negative and positive lumas)"""
    keys = np.unique(rng.integers(0, KEY_INVALID, 2 * n + 8, dtype=np.uint64))
    return _u32(rng.permutation(keys)[:n])


def grid_stride_set():
    """GRID_CAP + 257 keys: the first GRID_CAP positions — all a capped grid's first stride reaches — hold 20 000 low valid keys among
    invalid ones; the rank wanted, and every key above it, lies in the 257 positions only the second stride reaches."""
    rng = np.random.default_rng(77)
    keys = np.full(GRID_CAP + 257, KEY_INVALID, dtype=np.uint32)
    keys[rng.choice(GRID_CAP, 20000, replace=False)] = rng.integers(0x00000100, 0x40000000, 20000, dtype=np.uint64).astype(np.uint32)
    keys[GRID_CAP:] = _u32(np.uint64(0x80000000) + np.unique(rng.integers(0, 0x7FFFFF00, 400, dtype=np.uint64))[:257])[rng.permutation(257)]
    assert rank_wanted(20257) >= 20000
    return keys


@functools.lru_cache(maxsize=None)
def key_sets():
    """name -> uint32 key array, every adversarial set of the select tests"""
    rng = np.random.default_rng(5)
    sets = {}
    for v in (0x00000000, 0x80000000, 0xFFFFFFFE):
        sets[f"all_equal_{v:08x}"] = np.full(300, v, dtype=np.uint32)
    for j in range(4):
        digits = np.concatenate([[0, 255, 0, 255], rng.integers(0, 256, 296)])
        sets[f"differ_in_byte_{j}"] = _with_byte(0x80102030, j, rng.permutation(digits))
    for p in range(4):
        for name, keys in zip(("at_k", "at_k_plus_1", "at_k_minus_1"), boundary_sets(p)):
            sets[f"boundary_pass{p}_{name}"] = keys
    for p in (1, 2, 3):
        sets[f"decoys_pass{p}"] = decoy_set(p)
    mostly = np.full(1000, KEY_INVALID, dtype=np.uint32)
    mostly[7::100] = _spread_keys(rng, 10)
    sets["invalid_99_percent"] = mostly
    single = np.full(300, KEY_INVALID, dtype=np.uint32)
    single[151] = 0xFFFFFFFE
    sets["invalid_but_one"] = single
    sets["invalid_all"] = np.full(300, KEY_INVALID, dtype=np.uint32)
    for count in (1, 2, 3, 99, 100, 101, 199, 200, 256, 257):
        sets[f"count_{count}"] = _spread_keys(rng, count)
    for length in (1, 63, 64, 65, 255, 256, 257, 1000):
        keys = _spread_keys(rng, length)
        if length > 1:
            keys[rng.random(length) < 0.1] = KEY_INVALID
        sets[f"length_{length}"] = keys
    sets["length_grid_stride"] = grid_stride_set()
    for keys in sets.values():
        keys.setflags(write=False)
    return sets


def bands_of(keys, parts):
    """`keys` over `parts` interleaved bands, then an empty band and a band of invalid keys only"""
    return [np.ascontiguousarray(keys[r::parts]) for r in range(parts)] + [np.zeros(0, np.uint32), np.full(64, KEY_INVALID, np.uint32)]


# ---- the key map and post_process ---------------------------------------------------------------------------------------------------

def luma_reference(img, row):
    """(w0 * r + w1 * g) + w2 * b in float32, three products and two sums, each rounded once"""
    w = [F32(v) for v in row]
    img = img.reshape(-1, 3)
    with np.errstate(all="ignore"):
        return ((w[0] * img[:, 0]).astype(F32) + (w[1] * img[:, 1]).astype(F32)).astype(F32) + (w[2] * img[:, 2]).astype(F32)


def is_normal(x):
    with np.errstate(all="ignore"):
        return np.isfinite(x) & (np.abs(x) >= MIN_NORMAL)


def pixel_with_luma(target, row):
    """an rgb triple with one channel set and the others +0 whose reference luma is exactly `target`, or None"""
    target = F32(target)
    for ch in (1, 0, 2):
        guess = F32(np.float64(target) / np.float64(F32(row[ch])))
        start = int(bits(np.array([np.abs(guess)], F32))[0])
        for step in range(-64, 65):
            if start + step < 0:
                continue
            v = np.array([start + step], np.uint32).view(F32)[0]
            v = -v if target < 0 else v
            px = np.zeros(3, F32)
            px[ch] = v
            if bits(luma_reference(px, row))[0] == bits(np.array([target], F32))[0]:
                return px
    return None


def nan_with_payload(payload, negative=False):
    return np.array([(0xFFC00000 if negative else 0x7FC00000) | (payload & 0x3FFFFF)], np.uint32).view(F32)[0]


def luma_class_values():
    """input values of both signs over every class of float"""
    tiny = np.array([1, 2, 0x7FFFFF, 0x800000, 0x800001], np.uint32).view(F32)  # denormals up to the largest, 2^-126 and the next
    eps = np.array([0x34000000 + d for d in (-2, -1, 0, 1, 2)], np.uint32).view(F32)  # around f32::EPSILON
    pos = np.concatenate([[np.finfo(F32).max, 1.0, 2.0 ** -120, 2.0 ** -124, 2.0 ** -125, 0.0, np.inf, 3.5, 1e-30, 1e30], tiny, eps]).astype(F32)
    nans = np.array([nan_with_payload(0), nan_with_payload(1), nan_with_payload(0x2ABCDE), nan_with_payload(0x3FFFFF, True)], F32)
    return np.concatenate([pos, -pos, nans])


def luma_class_image(row):
    """(n, 3): every value of luma_class_values() in each channel in turn, the other channels +0; then pixels whose LUMA is exactly the
    smallest normal, the largest denormal, f32::EPSILON and its neighbour, of both signs"""
    vals = luma_class_values()
    img = np.zeros((3 * vals.size, 3), F32)
    for ch in range(3):
        img[ch * vals.size:(ch + 1) * vals.size, ch] = vals
    exact = []
    for t in (np.array([0x800000, 0x7FFFFF, 0x800001], np.uint32).view(F32).tolist() + [float(EPSILON), float(np.nextafter(EPSILON, F32(1)))]):
        for sign in (1.0, -1.0):
            px = pixel_with_luma(F32(sign * t), row)
            assert px is not None, t
            exact.append(px)
    return np.concatenate([img, np.array(exact, F32)])


def post_process_reference(img, row):
    """main.rs:748-762 by a sort: returns (image, divisor); the image is a divided copy, or `img` itself when left untouched"""
    luma = luma_reference(img, row)
    normal = np.sort(luma[is_normal(luma)])
    if normal.size == 0:
        return img, F32(0)
    p = normal[rank_wanted(normal.size)]
    if not p > EPSILON:
        return img, F32(0)
    with np.errstate(all="ignore"):
        return (img / p).astype(F32), p


POST_SHAPES = [(1, 1), (1, 2), (10, 10), (1, 101), (7, 37), (725, 724)]  # the last: 524 900 pixels, above GRID_CAP
POST_CONTENTS = ["mixed_signs", "negative_percentile", "selected_is_epsilon", "selected_above_epsilon", "abnormal_30_percent", "abnormal_all"]


@functools.lru_cache(maxsize=None)
def post_image(shape, content, row):
    rows, cols = shape
    n = rows * cols
    rng = np.random.default_rng(1000 * rows + 10 * cols + POST_CONTENTS.index(content))
    k = rank_wanted(n)
    if content == "mixed_signs":
        img = rng.normal(0.2, 1.0, (n, 3)).astype(F32)
    elif content == "negative_percentile":  # n - 1 - k pixels are positive (none fits below 101 pixels), the rank wanted is negative
        img = -rng.uniform(0.1, 3.0, (n, 3)).astype(F32)
        img[rng.choice(n, n - 1 - k, replace=False)] = rng.uniform(0.5, 2.0, (n - 1 - k, 3)).astype(F32)
    elif content in ("selected_is_epsilon", "selected_above_epsilon"):  # every pixel from the rank wanted upwards has the luma in question
        target = EPSILON if content == "selected_is_epsilon" else np.nextafter(EPSILON, F32(1))
        img = rng.uniform(1e-12, 1e-9, (n, 3)).astype(F32)
        img[rng.choice(n, n - k, replace=False)] = pixel_with_luma(target, row)
    else:
        img = rng.uniform(-0.5, 3.0, (n, 3)).astype(F32)
        odd = np.array([np.nan, nan_with_payload(0x1234), np.inf, -np.inf, 1e-40, -1e-42, 0.0, -0.0], F32)
        where = np.arange(n) if content == "abnormal_all" else np.flatnonzero(rng.random(n) < 0.3)
        img[where] = odd[rng.integers(0, odd.size, where.size)][:, None]
    img = img.reshape(rows, cols, 3)
    img.setflags(write=False)
    return img


# ---- the encode ---------------------------------------------------------------------------------------------------------------------

U = 2.0 ** -24
EF = float(F32(1.0) / F32(2.4))  # the exponent the f32 forms use
ENCODE_DELTA = 255.0 * (1.055 * (5 * U + abs(EF - 1 / 2.4) * 2.4 / np.e) + 0.055 * U + 2 * U)
ENCODE_MEASURED = 1.5e-5  # (1.475e-5, on 250 of 132 371 inputs) the host form's largest distance from an integer at a differing byte, x86-64, over encode_inputs()


def transfer_exact(x):
    """r = 255 * sRGB transfer of x, in float64, unclamped (NaN stays NaN)"""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        return 255.0 * np.where(x <= 0.0031308, 12.92 * x, 1.055 * np.power(x, 1 / 2.4) - 0.055)


def encode_reference(x):
    """the byte: clamp to [0, 255], floor, NaN -> 0"""
    r = transfer_exact(x)
    return np.floor(np.where(np.isnan(r), 0.0, np.clip(r, 0.0, 255.0))).astype(np.uint8)


def encode_distance(x):
    """distance of the exact r from the nearest integer; infinite where r is not finite (nothing is excused there)"""
    r = transfer_exact(x)
    with np.errstate(all="ignore"):
        return np.where(np.isfinite(r), np.abs(r - np.rint(r)), np.inf)


def _neighbours(x, n=256):
    """the n floats on either side of the non-negative float x, and x"""
    b = int(bits(np.array([x], F32))[0])
    up = np.arange(b, b + n + 1, dtype=np.int64)
    down = np.arange(1, n + 1, dtype=np.int64)
    below = np.where(b - down >= 0, b - down, 0x80000000 + (down - b))  # below +0 come -0 and the negative denormals
    return np.concatenate([below, up]).astype(np.uint32).view(F32)


def encode_transitions():
    """for each code 1 .. 255 the least float whose reference byte reaches it, by bisection over the bit patterns"""
    lo = np.zeros(255, np.int64)  # reference byte below the code
    hi = np.full(255, int(bits(np.array([2.0], F32))[0]), np.int64)  # at or above it
    codes = np.arange(1, 256)
    assert (encode_reference(hi.astype(np.uint32).view(F32)) >= codes).all() and (encode_reference(lo.astype(np.uint32).view(F32)) < codes).all()
    while (hi - lo > 1).any():
        mid = (lo + hi) // 2
        ge = encode_reference(mid.astype(np.uint32).view(F32)) >= codes
        hi, lo = np.where(ge, mid, hi), np.where(ge, lo, mid)
    return hi.astype(np.uint32).view(F32)


@functools.lru_cache(maxsize=None)
def encode_inputs():
    parts = [_neighbours(t) for t in encode_transitions()]
    parts += [_neighbours(F32(0.0031308)), _neighbours(F32(0.0)), _neighbours(F32(1.0))]
    odd = np.array([1e-45, 1e-40, 1.1754942e-38, -1e-45, -0.0, -1.0, -1e-3, -1e30, np.inf, -np.inf, np.nan, 1e30, 255.0, 256.0, 3.4e38], F32)
    parts.append(np.concatenate([odd, [nan_with_payload(0x155555), nan_with_payload(7, True)]]).astype(F32))
    x = np.concatenate(parts)
    x.setflags(write=False)
    return x


def encode_excused_cap(x):
    return int((encode_distance(x) <= ENCODE_DELTA / 2).sum())


def check_encode(got, x):
    """the assertions of the encode tests on bytes `got` for inputs `x`; returns (differing bytes, their largest distance)"""
    want, dist = encode_reference(x), encode_distance(x)
    off = got.astype(np.int32) - want.astype(np.int32)
    differs = off != 0
    assert np.abs(off).max(initial=0) <= 1, (x[np.abs(off) > 1][:8], got[np.abs(off) > 1][:8], want[np.abs(off) > 1][:8])
    bad = differs & ~(dist <= ENCODE_DELTA)
    assert not bad.any(), (x[bad][:8], got[bad][:8], want[bad][:8], dist[bad][:8])
    return int(differs.sum()), float(dist[differs].max(initial=0.0))


# ---- the accumulator ----------------------------------------------------------------------------------------------------------------

def accumulate_reference(samples, valid, acc, weight):
    """photon.rs:25-28 in numpy float32, epoch by epoch, in place; a sample whose flag is clear is never added (not even as + 0)"""
    with np.errstate(all="ignore"):
        for e in range(samples.shape[0]):
            on = valid[e] != 0
            acc[on] = acc[on] + samples[e][on]
            weight[on] = weight[on] + F32(1)


def resolve_reference(acc, weight):
    """photon.rs:15-23: sum / weight, black while weight < f32::EPSILON"""
    with np.errstate(all="ignore"):
        return np.where((weight < EPSILON)[..., None], F32(0), acc / weight[..., None]).astype(F32)
