"""The motion queries' ABI and Python surface: the symbols in the right library only, the option, rt.moving as a public submodule whose
names stay off the top level and whose numpy path never loads torch, the header's words, and the refusals of the device entry points
in the stated order — those that need no scene without a device, "never kept" on a real scene."""
import ctypes as C
import subprocess
import sys
import types

import numpy as np
import pytest

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import _capi, moving

AMD_NAMES = ("rt_scene_keep_positions", "rt_scene_positions_kept", "rt_previous_positions", "rt_previous_positions_host")
HOST_NAMES = ("rt_previous_positions_cpu",)
HEADER = (_capi.REPO_ROOT / "include" / "rt_amd.h").read_text()
OPTION = "RT_AMD_DIAG_MOTION_MAX_GROUPS"
INVALID, UNSUPPORTED = -1, -5


def test_symbols_are_exported_and_listed_in_the_right_library_only():
    amd, host = _capi.amd_lib(), _capi.host_lib()
    for name in AMD_NAMES:
        assert hasattr(amd, name) and name in _capi.AMD_SYMBOLS and name not in _capi.HOST_SYMBOLS and not hasattr(host, name), name
    for name in HOST_NAMES:
        assert hasattr(host, name) and name in _capi.HOST_SYMBOLS and name not in _capi.AMD_SYMBOLS and not hasattr(amd, name), name
    assert amd.rt_abi_version() == 1  # additive: the version stays


def test_the_option_is_accepted_and_documented():
    amd = _capi.amd_lib()
    assert OPTION in HEADER and OPTION in (_capi.REPO_ROOT / "INTEGRATION.md").read_text()
    assert amd.rt_set_option(OPTION.encode(), b"1") == 0 and amd.rt_set_option(OPTION.encode(), None) == 0


def test_the_header_states_the_block_and_no_longer_leaves_the_plane_to_the_caller():
    block = HEADER[HEADER.index("---- motion queries:"):HEADER.index("---- several GPUs from one process")]
    for name in AMD_NAMES:
        assert name in block, name
    for words in ("no rotation is modelled", "Not covered:", "motion of lights", "rt_multi_*", "0x7fc00000", "was_stride < 3"):
        assert words in block, words
    assert HEADER.index("---- scene updates:") < HEADER.index("---- motion queries:")
    temporal_block = HEADER[HEADER.index("---- temporal queries:"):HEADER.index("---- variance-guided filter queries:")]
    assert "is not provided" not in temporal_block and "rt_previous_positions" in temporal_block
    assert "rt_previous_positions_cpu" in (_capi.REPO_ROOT / "include" / "rt_host.h").read_text()


def test_moving_is_a_public_submodule_off_the_top_level():
    """rt.moving, not rt.motion: temporal.motion is a function, and no name of a submodule's __all__ may be an attribute of the package"""
    assert isinstance(rt.moving, types.ModuleType) and rt.moving is moving
    assert sorted(moving.__all__) == sorted(["keep_positions", "positions_kept", "previous_positions", "previous_positions_numpy",
                                             "accumulate_moving_frame"])
    for name in moving.__all__:
        assert hasattr(moving, name) and name not in rt.__all__ and not hasattr(rt, name), name
    assert "moving" not in rt.__all__ and not hasattr(rt, "motion")


def test_the_numpy_path_leaves_torch_unloaded():
    code = (f"import sys\nsys.path.insert(0, {str(_capi.REPO_ROOT)!r})\nimport numpy as np\n"
            "import homework_18_graphics_raytracer_amd as rt\n"
            "from homework_18_graphics_raytracer_amd import moving\n"
            "w = rt.World()\n"
            "w.push_object(rt.Material()).push_flat_triangle([(0, 0, 0), (1, 0, 0), (0, 1, 0)], [(0, 0), (1, 0), (0, 1)])\n"
            "hit = np.zeros((2, 13), dtype=np.uint32)\n"
            "hit[0, 0] = 1\n"
            "hit[0, 3:6] = np.array([0.25, 0.25, 0.0], dtype=np.float32).view(np.uint32)\n"
            "hit[1, 0] = 0xFFFFFFFF\n"
            "kept = np.array([[0, 0, 1, 1, 0, 1, 0, 1, 1]], dtype=np.float32)\n"
            "was = moving.previous_positions_numpy(w, kept, None, hit)\n"
            "assert was[0].tolist() == [0.25, 0.25, 1.0] and np.isnan(was[1]).all(), was\n"
            "assert 'torch' not in sys.modules\n"
            "print('ok')\n")
    done = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert done.returncode == 0 and done.stdout.strip() == "ok", done.stderr


# ---- refusals of the device entry points, before any device work ----

H, W = C.c_void_p(4096), C.c_void_p(8192)  # never dereferenced: every call below is refused on its arguments


def _query(entry, scene, hits, n, was, stride):
    lib = _capi.amd_lib()
    rc = lib.rt_previous_positions(scene, hits, n, was, stride, None) if entry == "device" else lib.rt_previous_positions_host(scene, hits, n, was, stride)
    return rc, lib.rt_last_error().decode(), "rt_previous_positions" + ("" if entry == "device" else "_host")


@pytest.mark.parametrize("entry", ["device", "host"])
def test_refusals_that_need_no_scene(entry):
    rc, text, who = _query(entry, None, None, 1 << 32, None, 0)  # the count comes before the null scene
    assert rc == UNSUPPORTED and text.startswith(who + ": ") and "2^32 records or more (checked first" in text
    rc, text, who = _query(entry, None, None, 0, None, 0)  # ... and the null scene before "nothing to do"
    assert rc == INVALID and text == who + ": null scene"
    lib = _capi.amd_lib()
    assert lib.rt_scene_keep_positions(None, None) == INVALID and lib.rt_last_error().decode() == "rt_scene_keep_positions: null scene"
    assert lib.rt_scene_positions_kept(None) == INVALID and lib.rt_last_error().decode() == "rt_scene_positions_kept: null scene"


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["device", "host"])
def test_refusals_on_a_scene_in_the_stated_order(entry):
    scene = rt.Scene(rt.reference_world())
    # never kept: after the count and the null scene, before "nothing to do" and the pointers; each case carries the later faults too
    rc, text, who = _query(entry, scene._h, None, 1 << 32, None, 0)
    assert rc == UNSUPPORTED and "2^32 records" in text
    for n in (0, 5):
        rc, text, who = _query(entry, scene._h, None, n, None, 0)
        assert rc == INVALID and text.startswith(who + ": ") and "rt_scene_keep_positions" in text, (n, text)
    assert _capi.amd_lib().rt_scene_positions_kept(scene._h) == 0
    moving.keep_positions(scene)
    assert _capi.amd_lib().rt_scene_positions_kept(scene._h) == 1
    assert _query(entry, scene._h, None, 0, None, 0)[0] == 0  # nothing to do: the pointers are not looked at
    for hits, was in ((None, W), (H, None)):
        rc, text, who = _query(entry, scene._h, hits, 5, was, 0)
        assert rc == INVALID and text == who + ": null hit or was pointer"
    rc, text, who = _query(entry, scene._h, H, 5, W, 2)
    assert rc == INVALID and text == who + ": was_stride must be at least 3 words"


@pytest.mark.gpu
def test_the_wrappers_check_their_tensors():
    import torch

    scene = rt.Scene(rt.reference_world())
    moving.keep_positions(scene)
    hits = torch.zeros((4, 13), dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="hits"):
        moving.previous_positions(scene, hits[:, :12])
    with pytest.raises(ValueError, match="out"):
        moving.previous_positions(scene, hits, out=torch.zeros((4, 3), dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="out"):
        moving.previous_positions(scene, hits, out=torch.zeros((5, 3), dtype=torch.float32, device="cuda"))
    out = moving.previous_positions(scene, hits)  # kind 0, index 0: the reference scene's first sphere, unmoved
    torch.cuda.synchronize()
    assert tuple(out.shape) == (4, 3) and not out.cpu().numpy().any()
