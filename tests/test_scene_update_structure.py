"""What tests/test_gpu_scene_update.py builds for the large dome, checked without a GPU: the description's node tree
(rt_scene_describe_nodes) has a root above RT_REFIT_WAVE_MAX triangles that qualifies with a cone, two levels of inner nodes below
it, and each case's description B has the tree the case is meant to reach."""
import pytest
import _scene_update_support as su


@pytest.fixture(scope="module")
def parts():
    return su.large_dome_parts()


def test_large_dome_has_a_qualifying_root_above_1024_triangles_and_two_inner_levels(parts):
    _, desc, verts = parts
    nodes = su.nodes_of(desc)
    end = su.large_dome_structure(nodes)
    inner = (nodes[:, 1] == 0) & (nodes[:, 0] >= su.LARGE.start) & (end <= su.LARGE.stop)
    assert sorted(end[inner] - nodes[inner, 0])[-2:] == [256, 3200]
    assert su.REFIT_WAVE_MAX == 1024 and su.CONE == 0xFFFFFFFF


def test_the_plain_cap_at_half_angle_0_6_gets_no_root():
    """why the large dome is flattened: with bulge 1 its corner faces are too steep for a cone over all of it"""
    nodes = su.nodes_of(su.dome_world(grid=su.LARGE_GRID).desc())
    su.large_dome_structure(nodes, rooted=False)


@pytest.mark.parametrize("name", su.LARGE_CASES)
def test_large_dome_cases_reach_what_they_are_meant_to(parts, name):
    _, desc, verts = parts
    b, vb, touched, same_tree = su.large_case(name, verts, desc)
    assert same_tree == (name != "leaf crumpled") and su.LARGE.start <= touched.start < touched.stop <= su.LARGE.stop
