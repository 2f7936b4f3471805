"""The scenes of tests/_scenes.py that fix the SHAPE of the node array are what they claim, without a GPU: rt_scene_describe_nodes
(csrc/rt_api_layout.hip, host only) of leaf_size_world, tree_shape_world and big_tree_world.

The pair-wise dealing (K chunks of ck triangles, R = 64 / ck (ray, chunk) sub-jobs per pass) of a clustered leaf is word 4 of its
node.  DEALINGS below is the table of the 35 dealings the selection rule gives the counts 8 .. 64; `dealing` restates the rule;
the test pins rule, table and the host's words against each other and fails when a dealing, or a remainder leaf of 1 .. 7
triangles, is missing from the scenes.  The tree tests state the nesting of every run literally: a leaf is its triangle count, an
inner node the tuple of its children."""
import numpy as np
import pytest

import _scenes
from _scenes import dealing

CONE = 0xFFFFFFFF

# (K, ck, R): the leaf counts that get it
DEALINGS = {
    (1, 8, 8): [8], (1, 9, 7): [9], (1, 10, 6): [10], (1, 15, 4): [15], (1, 16, 4): [16], (1, 21, 3): [21], (1, 29, 2): [29],
    (1, 30, 2): [30], (1, 31, 2): [31], (1, 32, 2): [32], (1, 57, 1): [57], (1, 58, 1): [58], (1, 59, 1): [59], (1, 60, 1): [60],
    (1, 61, 1): [61], (1, 62, 1): [62], (1, 63, 1): [63], (1, 64, 1): [64], (2, 7, 9): [13, 14], (2, 9, 7): [17, 18],
    (2, 21, 3): [41, 42], (3, 4, 16): [11, 12], (3, 8, 8): [22, 23, 24], (3, 9, 7): [25, 26, 27], (3, 12, 5): [36],
    (3, 15, 4): [43, 44, 45], (3, 16, 4): [46, 47, 48], (4, 7, 9): [28], (5, 4, 16): [19, 20], (5, 7, 9): [33, 34, 35],
    (5, 8, 8): [37, 38, 39, 40], (5, 10, 6): [50], (6, 9, 7): [51, 52, 53, 54], (7, 7, 9): [49], (7, 8, 8): [55, 56],
}


def word(k, ck, r):
    return ck | (k << 8) | (r << 16)


def shape(nodes, k):
    """node k as a nesting: a leaf is its count, an inner node the tuple of its children (the nodes from k + 1 up to its skip_to, each
    followed by the one its own skip_to names)"""
    if nodes[k, 1] != 0:
        return int(nodes[k, 1])
    out, c = [], k + 1
    while c < nodes[k, 3]:
        out.append(shape(nodes, c))
        c = int(nodes[c, 3])
    assert c == nodes[k, 3], f"the children of node {k} do not end on its skip_to"
    return tuple(out)


def check_consistent(nodes, n_triangles):
    """leaves tile [0, n_triangles) in node order; a leaf's skip_to is the next node; an inner node's skip_to is the index after its last
    descendant: inside (k, skip_to) every node's skip_to stays inside, and the node at skip_to is not below it (it starts where the
    subtree's triangles end)"""
    n = nodes.shape[0]
    at = 0
    for k in range(n):
        first, count, _, skip = (int(v) for v in nodes[k, :4])
        assert k < skip <= n, (k, skip)
        if count:
            assert first == at and skip == k + 1, (k, first, at, skip)
            at += count
        else:
            assert skip > k + 1 and first == at and nodes[k + 1, 0] == first, ("an inner node starts with its first descendant", k)
            assert (nodes[k + 1:skip, 3] <= skip).all(), ("a descendant reaches beyond its ancestor", k)
            assert nodes[k + 1:skip, 1].sum() > 0
    assert at == n_triangles


def leaves_of_run(nodes, first, count):
    rows = np.flatnonzero((nodes[:, 1] != 0) & (nodes[:, 0] >= first) & (nodes[:, 0] < first + count))
    return rows


def test_dealing_rule_and_table_agree():
    assert len(DEALINGS) == 35
    counts = sorted(c for v in DEALINGS.values() for c in v)
    assert counts == list(range(8, 65))
    for key, members in DEALINGS.items():
        for c in members:
            assert dealing(c) == key, (c, dealing(c), key)
    assert [dealing(r) for r in range(1, 8)] == [(1, 1, 64), (1, 2, 32), (1, 3, 21), (1, 4, 16), (1, 5, 12), (1, 6, 10), (1, 7, 9)]


@pytest.mark.parametrize("swap", [0, 1])
def test_leaf_size_world_has_every_dealing(swap):
    s = _scenes.leaf_size_world(swap)
    desc = s.world.desc()
    nodes = _scenes.nodes_of(desc)
    assert desc.n_triangles == 2052 + sum(64 + r for r in range(1, 8)) + sum(c for _, c, _ in _scenes.DECKS) < 8192
    check_consistent(nodes, desc.n_triangles)
    seen, remainders, kinds = set(), set(), set()
    for name, first, count, kind in s.runs:
        rows = leaves_of_run(nodes, first, count)
        got = [int(v) for v in nodes[rows, 1]]
        if count <= 64:  # exactly one clustered leaf: nothing split, nothing merged with a neighbour
            assert got == [count] and nodes[rows[0], 0] == first and nodes[rows[0], 2] != 0, (name, got)
            if name.startswith("patch"):
                cone = nodes[rows[0], 2] == CONE
                assert cone == (kind == "curved" and count > 8), (name, kind, int(nodes[rows[0], 2]))
                assert kind == "curved" or 1 <= nodes[rows[0], 2] <= 8
                kinds.add((kind == "curved", dealing(count)))
        else:
            r = count - 64
            assert got == [16, 16, 16, 16, r] and (nodes[rows, 2] != 0).all(), (name, got)
            assert shape(nodes, rows[0] - 1) == (16, 16, 16, 16, r), name  # under one root
            remainders.add(r)
        for k in rows:
            want = dealing(int(nodes[k, 1]))
            assert nodes[k, 4] == word(*want), (name, int(nodes[k, 1]), hex(int(nodes[k, 4])), want)
            seen.add(want)
    assert set(DEALINGS) <= seen, sorted(set(DEALINGS) - seen)
    assert remainders == set(range(1, 8)) and {dealing(r) for r in range(1, 8)} <= seen
    assert {c for c, _ in kinds} == {False, True}  # both kinds (swap exchanges them count by count)


def test_tree_shape_world_nesting():
    s = _scenes.tree_shape_world()
    desc = s.world.desc()
    nodes = _scenes.nodes_of(desc)
    assert desc.n_triangles < 8192
    check_consistent(nodes, desc.n_triangles)
    runs = {name: (first, count) for name, first, count, _ in s.runs}
    top = []  # the top-level nodes, in order
    k = 0
    while k < nodes.shape[0]:
        top.append(k)
        k = int(nodes[k, 3])
    by_first = {int(nodes[k, 0]): k for k in top}
    l16 = (16,) * 16
    want = {65: (16, 16, 16, 16, 1), 80: (16,) * 5, 81: (16,) * 5 + (1,), 255: (16,) * 15 + (15,), 256: l16, 257: (l16, 1),
            272: (l16, 16), 273: (l16, (16, 1))}
    at = 0
    for n in _scenes.TREE_RUNS:  # index-adjacent: each tree starts where the one before ends, as a top-level node
        first, count = runs[f"tree{n}"]
        assert (first, count) == (at, n)
        root = by_first[first]
        assert nodes[root, 1] == 0 and nodes[root, 2] == CONE, n
        assert shape(nodes, root) == want[n], (n, shape(nodes, root))
        at += n
    # two plain runs after the closed tree: ONE plain leaf, a node of its own where the tree's skip_to points
    last_root = by_first[runs["tree273"][0]]
    after = int(nodes[last_root, 3])
    assert after in top
    assert tuple(int(v) for v in nodes[after, :3]) == (runs["short5"][0], 5 + 7, 0)
    assert runs["dupA"] == (runs["short5"][0] + 5, 7)
    slab, dup_b = after + 1, after + 2
    assert tuple(int(v) for v in nodes[slab, :2]) == runs[_scenes.DUP_OF] == (runs["dupA"][0] + 7, 24) and 1 <= nodes[slab, 2] <= 8
    assert nodes[slab, 4] == word(*dealing(24))
    assert tuple(int(v) for v in nodes[dup_b, :3]) == (runs["dupB"][0], 7, 0)
    # the copies are the slab's triangles vertex for vertex
    a, b, c = runs["dupA"][0], runs[_scenes.DUP_OF][0], runs["dupB"][0]
    assert np.array_equal(s.tris[a:a + 7].view(np.uint32), s.tris[b:b + 7].view(np.uint32))
    assert np.array_equal(s.tris[c:c + 7].view(np.uint32), s.tris[b + 10:b + 17].view(np.uint32))
    # the crumpled object: no root; an inner node over leaves 0 .. 15; the crumpled leaf, plain; leaves 17 .. 32 beside it
    first, count = runs[f"crumpled{_scenes.CRUMPLED}"]
    inner = dup_b + 1
    assert inner in top and nodes[inner, 0] == first and shape(nodes, inner) == l16 and nodes[inner, 2] == CONE
    crumpled = int(nodes[inner, 3])
    assert crumpled == inner + 17
    assert tuple(int(v) for v in nodes[crumpled, :3]) == (first + 256, 16, 0)
    rest = nodes[crumpled + 1:]
    assert rest.shape[0] == 16 and (rest[:, 1] == 16).all() and (rest[:, 2] == CONE).all()
    assert all(k in top for k in range(crumpled, nodes.shape[0]))
    # the crumpled leaf's face normals do span more than 60 degrees
    p = s.tris[first + 256:first + 272].astype(np.float64)
    nrm = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 1])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    assert np.abs(nrm @ nrm.T).min() < 0.5
    # every leaf that carries normals also carries a dealing
    tested = nodes[(nodes[:, 1] != 0) & (nodes[:, 2] != 0)]
    assert all(row[4] == word(*dealing(int(row[1]))) for row in tested)


def test_big_tree_world_nesting():
    s = _scenes.big_tree_world()
    desc = s.world.desc()
    nodes = _scenes.nodes_of(desc)
    assert desc.n_triangles == 4096 + 4112 > 8192  # above the default breadth-first switch
    check_consistent(nodes, desc.n_triangles)
    l16 = (16,) * 16
    l256 = (l16,) * 16
    assert nodes[0, 1] == 0 and nodes[0, 0] == 0 and shape(nodes, 0) == l256
    second = int(nodes[0, 3])
    assert second == 1 + 16 + 256 and nodes[second, 0] == 4096 and nodes[second, 1] == 0
    assert shape(nodes, second) == (l256, 16)
    assert nodes[second, 3] == nodes.shape[0]
    assert (nodes[:, 2] == CONE).all()  # every node of both trees can be skipped
