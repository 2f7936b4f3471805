"""The generator's tables against their definition, and the oracle's record reader and ziggurat against an independent restatement
(tests/_rng_support.py) on crafted records: generators put at chosen positions with chosen words waiting, so that every branch of
BlockRng::next_u64 and of the ziggurat is taken on purpose and compared value by value.  No GPU; needs mpmath (as
tests/test_detmath_cpu.py does: it is the high-precision judge, and there is no fallback)."""
import collections
import math

import numpy as np
import pytest

import _rng_support as S

MP, mpf = S.MP, S.MP.mpf
R, X, F = S.R, S.X, S.F


@pytest.fixture(scope="module")
def base():
    return S.base_records(4)


# ---- the tables ----

def test_table_ends_and_order():
    assert X[1] == R and X[256] == 0.0 and F[256] == 1.0
    assert all(X[i] > X[i + 1] for i in range(256)) and all(F[i] < F[i + 1] for i in range(256))


def test_f_is_the_density_at_x():
    """F[i] = exp(-X[i]^2 / 2).  The literals are rand's own f64-computed decimals, not correctly rounded values, so the bound is the
    next power of two above twice the measured deviation.  Measured: largest relative deviation 2^-51.10 -> asserted < 2^-50; in ulps
    of the correctly rounded value, 168 of the 257 entries are exact, 46 / 29 are one below / above, 7 / 6 two, 1 three above.  That
    count is asserted as measured: it says which literals the figures belong to (an entry changed in its last digit moves a count)."""
    ref = [MP.exp(-mpf(x) ** 2 / 2) for x in X]
    dev = max(abs(mpf(f) / r - 1) for f, r in zip(F, ref))
    print(f"F against exp(-X^2/2): largest relative deviation 2^{math.log2(dev):.2f}")
    assert dev < 2.0 ** -50
    as_int = lambda v: int(np.array([v], dtype=np.float64).view(np.int64)[0])
    ulps = collections.Counter(as_int(f) - as_int(float(r)) for f, r in zip(F, ref))
    print("F - RN(exp(-X^2/2)) in ulps:", sorted(ulps.items()))
    assert dict(ulps) == {-2: 7, -1: 46, 0: 168, 1: 29, 2: 6, 3: 1}


def test_layers_have_the_area_of_the_base_strip():
    """v = R f(R) + the tail's area beyond R is the area of every layer: X[i] (F[i+1] - F[i]) for i = 1 .. 255, and X[0] = v / f(R).
    Measured, relative to v from mpmath: layers 1 .. 254 within 2^-38.21 and X[0] f(R) within 2^-38.22 (R and the literals carry about
    twelve significant digits of the ideal ziggurat); the top layer i = 255, which ends at X[256] = 0 by construction and takes up
    what is left, 2^-29.91.  Asserted: the next power of two above twice each."""
    f_r = MP.exp(-mpf(R) ** 2 / 2)
    v = mpf(R) * f_r + MP.sqrt(MP.pi / 2) * MP.erfc(mpf(R) / MP.sqrt(2))
    dev = [abs(mpf(X[i]) * (mpf(F[i + 1]) - mpf(F[i])) / v - 1) for i in range(1, 256)]
    inner, top, base_strip = max(dev[:-1]), dev[-1], abs(mpf(X[0]) * f_r / v - 1)
    print(f"layer areas against v: 1..254 2^{math.log2(inner):.2f}, 255 2^{math.log2(top):.2f}; X[0] f(R) 2^{math.log2(base_strip):.2f}")
    assert max(dev) < 2.0 ** -28  # the spread over all 255 layers
    assert inner < 2.0 ** -37 and base_strip < 2.0 ** -37


# ---- the reader ----

POSITIONS = (0, 1, 250, 251, 252, 253, 254, 255, 256)


@pytest.mark.parametrize("position", POSITIONS)
def test_u32_and_range_draws_at_every_edge_position(base, position):
    """eight u32 draws, then eight gen_range(-pi, pi) draws, from a record put at `position` with known words waiting: the same bits
    and the same final record from the oracle and from the restatement"""
    words = [0x9E3779B9 * (k + 1) & S.M32 for k in range(8)]
    for low, high in ((None, None), (-np.float32(np.pi), np.float32(np.pi)), (0.0, 1.0)):
        mine = S.craft(base[position % 4], position, words)
        theirs = mine.copy()
        if low is None:
            want = np.array([S.next_u32(mine) for _ in range(8)], dtype=np.uint32)
            got = S.oracle_u32(theirs, 8)
            crafted = min(8, 256 - position)
            assert list(want[:crafted]) == words[:crafted]
        else:
            want = np.array([S.range_f32(mine, low, high) for _ in range(8)], dtype=np.float32)
            got = S.oracle_range_f32(theirs, low, high, 8)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (position, low)
        assert np.array_equal(theirs, mine), (position, low)
        assert int(mine[S.INDEX]) == (position + 8 if position + 8 <= 256 else position + 8 - 256)


def test_u64_halves_at_the_straddle(base):
    """position 255: the low half is the old block's last word, the high half the new block's first, and one word of the new block is
    used; position 256: both halves from the new block; position 254: both from the old one"""
    for position, used in ((254, 256), (255, 1), (256, 2)):
        rec = S.craft(base[0], position, [0x11111111, 0x22222222])
        nxt = rec.copy()
        S.generate(nxt)
        old, new = rec[S.RESULTS:S.RESULTS + 256].copy(), nxt[S.RESULTS:S.RESULTS + 256]
        v = S.next_u64(rec)
        want = {254: (0x22222222 << 32) | 0x11111111, 255: (int(new[0]) << 32) | 0x11111111, 256: (int(new[1]) << 32) | int(new[0])}[position]
        assert v == want and int(rec[S.INDEX]) == used
        assert np.array_equal(rec[S.RESULTS:S.RESULTS + 256], old if position == 254 else new)


# ---- the ziggurat ----

NORMAL_POSITIONS = (0, 249, 251, 252, 253, 254, 255, 256)


def check_draw(case, position, d, got, what):
    """the restated draw `d` of a crafted case at `position` against a binary64 value `got`"""
    assert min(d.margins) >= S.MARGIN, (what, d.path, d.margins)
    fits = position + len(case.words) <= 256
    if fits:
        assert d.path == case.path and d.tail_turns == case.tail_turns, (what, d.path, d.tail_turns)
    elif position + 2 <= 256:
        first = "wedge" if d.path[0].startswith("wedge") else d.path[0]
        assert first == case.first, (what, d.path)
    if d.exact:
        want = S.to_f64(d.value)
        assert np.float64(got).view(np.uint64) == np.float64(want).view(np.uint64), (what, got, want)
    else:
        assert abs(mpf(float(got)) - d.value) <= S.tail_bound(d), (what, got, float(d.value))


@pytest.mark.parametrize("position", NORMAL_POSITIONS)
def test_every_crafted_ziggurat_case_at_every_edge_position(base, position):
    """orc_rng_draw_normal(0, 1) — whose mean + sd * z is z itself — on every crafted case with the block boundary before, inside and
    after the draw (in the tail cases between the trigger and the Open01 pairs; what lies beyond the boundary is the generator's own
    next block, so there the restatement says which path the draw takes and only the first turn's class is the case's).  Accepts and
    wedge-accepts are x = u X[i], one rounding: the same bits.  Tail values within _rng_support.tail_bound.  The same final record.
    A second draw follows from wherever the first one left the record."""
    seen = collections.Counter()
    for k, case in enumerate(S.CASES):
        mine = S.craft(base[k % 4], position, case.words)
        theirs = mine.copy()
        got = S.oracle_normal(theirs, 2)
        d0, d1 = S.ziggurat(mine), S.ziggurat(mine)
        check_draw(case, position, d0, got[0], (case.name, position))
        assert min(d1.margins) >= S.MARGIN
        if d1.exact:
            assert got[1] == S.to_f64(d1.value)
        else:
            assert abs(mpf(float(got[1])) - d1.value) <= S.tail_bound(d1)
        assert np.array_equal(theirs, mine), (case.name, position)
        seen[tuple(d0.path), d0.tail_turns] += 1
    if position <= 246:  # every case fits: all the paths the cases were built for occur
        assert set(seen) == {(("accept",), 0), (("tail",), 1), (("tail",), 2), (("wedge-accept",), 0), (("wedge-reject", "accept"), 0),
                             (("wedge-reject", "wedge-accept"), 0)}


def test_cases_cover_both_signs_and_every_layer_asked_for():
    names = {c.name for c in S.CASES}
    for sn in "+-":
        for stem in ("accept1", "accept127", "accept254", "tail1", "tail2", "wedge_accept1", "wedge_accept128", "wedge_accept254",
                     "wedge_reject1", "wedge_reject128", "wedge_reject254", "bottom_accept", "bottom_reject"):
            assert stem + sn in names
    rec0 = S.base_records(1)[0]
    for c in S.CASES:
        d = S.ziggurat(S.craft(rec0, 0, c.words))
        assert (float(d.value) < 0) == c.name.endswith("-") and min(d.margins) >= S.MARGIN
        layer = c.words[0] & 0xFF
        want = 0 if c.name.startswith("tail") else 255 if c.name.startswith("bottom") else int("".join(ch for ch in c.name if ch.isdigit()))
        assert layer == want, c.name
