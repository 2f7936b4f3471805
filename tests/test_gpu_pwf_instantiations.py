"""The persistent wavefront kernel by instantiation: pwf_kernel<PACKED, BFS, RAYS> (csrc/rt_pwf_kernel.h) has eight, the launcher
picks one per call, and a frame the arenas cannot finish is rendered by the per-pixel kernel with the same pixels — so parity alone
says neither which code ran nor whether the persistent kernel finished the frame.  Every cell here renders a small frame (RAYS: traces
the camera's own rays), asserts through homework_18_graphics_raytracer_amd.diagnostics the exact (packed, bfs, rays) it was written
for and, unless it is an overflow cell, that the persistent kernel finished the frame itself; then radiance as uint32 and the cast
count against the oracle.  A cell that lands on another instantiation fails.  tests/_pwf_support.py has the steering and its
derivation from pw_plan; run with -s, every cell prints the plan it ran with.

Cells left out, with the reason:
  bands on the four UNPACKED instantiations   a banded call is always packed (_pwf_support.py BANDS has the arithmetic);
                                              test_a_banded_call_is_always_packed shows it through the diagnostic.
Everything else runs on all eight.  tests/test_gpu_wavefront.py is sure of PACKED only in the 3840x2160 test, which now asserts it."""
import numpy as np
import pytest

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import _capi, diagnostics
import _pwf_support as S
from _records import torch_device
from _trace_support import _mismatches

pytestmark = pytest.mark.gpu

WALKERS = [pytest.param(False, id="walk"), pytest.param(True, id="bfs")]
FORMS = [pytest.param(False, id="frame"), pytest.param(True, id="rays")]
PACKINGS = [pytest.param(False, id="unpacked"), pytest.param(True, id="packed")]


def finished(cell, w=S.W, h=S.H):
    """the persistent kernel rendered the w x h frame itself: every workgroup left, every tile written, no overflow flag"""
    plan, outcome = cell
    assert outcome.finished, f"the frame fell back to the per-pixel kernel: {outcome}"
    assert plan.band_units == plan.units and outcome.tiles_done == (w * h + 63) // 64 and outcome.groups_done == plan.groups, outcome
    return cell


@pytest.mark.parametrize("rays", FORMS)
@pytest.mark.parametrize("bfs", WALKERS)
@pytest.mark.parametrize("packed", PACKINGS)
def test_plain_parity(packed, bfs, rays):
    """67x45 at depth 5 on the reference scene: 48 tiles, the last one of 7 pixels, one workgroup each."""
    plan, _ = finished(S.run_cell("ref", bfs, rays, S.PACKED_MANY if packed else S.UNPACKED, S.W, S.H, 5))
    assert plan.groups == 48 and plan.band_units == plan.units
    assert plan.ring_cap == (65536 if packed else 8192) and plan.node_cap == plan.ring_cap - 1024


@pytest.mark.parametrize("rays", FORMS)
@pytest.mark.parametrize("bfs", WALKERS)
def test_packed_with_one_workgroup(bfs, rays):
    """RT_AMD_WF_SHARE=1000 at the default budget on 96x64: one arena for the whole frame, large enough to be packed."""
    plan, _ = finished(S.run_cell("ref", bfs, rays, S.PACKED_ONE, S.W1, S.H1, 5), S.W1, S.H1)
    assert plan.groups == 1 and plan.band_units == plan.units and plan.budget == 6 and plan.ring_cap == 65536


@pytest.mark.parametrize("rays", FORMS)
@pytest.mark.parametrize("bfs", WALKERS)
@pytest.mark.parametrize("packed", PACKINGS)
@pytest.mark.parametrize("depth", [0, 20])
def test_depth_limits(depth, packed, bfs, rays):
    """Depth 0 (roots only: nothing is queued, nothing folded) and depth 20 (ten regions of fold lists per arena); the unpacked deep
    frame at a budget of 32, as tests/test_gpu_wavefront.py's deep frames."""
    steer = S.PACKED_MANY if packed else (S.UNPACKED_32 if depth == 20 else S.UNPACKED)
    finished(S.run_cell("ref", bfs, rays, steer, S.W, S.H, depth))


@pytest.mark.parametrize("rays", FORMS)
@pytest.mark.parametrize("bfs", WALKERS)
@pytest.mark.parametrize("packed", PACKINGS)
@pytest.mark.parametrize("n_lights", [0, 1, 5, 9])
def test_lights(n_lights, packed, bfs, rays):
    """No light, fewer and more lights than the kernel keeps SHADE queues for (the reference scene has three)."""
    finished(S.run_cell(f"lights{n_lights}", bfs, rays, S.PACKED_MANY if packed else S.UNPACKED, S.W, S.H, 5))


@pytest.mark.parametrize("rays", FORMS)
@pytest.mark.parametrize("bfs", WALKERS)
def test_two_bands_with_a_ragged_last_one(bfs, rays):
    """Budget 1100 on 67x45: two launches through one workspace, 24 rows and 21 (1536 rays and 1479, no multiple of 64); the outcome
    read back is the last band's.  Packed only: see the module's docstring."""
    plan, outcome = S.run_cell("ref", bfs, rays, S.BANDS, S.W, S.H, 5)
    assert plan.groups == 48 and plan.ring_cap == 65536
    assert (plan.units, plan.band_units) == ((S.W * S.H, 1536) if rays else (S.H, 24))
    last = (S.W * S.H - 1536) if rays else S.W * (S.H - 24)
    assert outcome.finished and outcome.tiles_done == (last + 63) // 64 and outcome.groups_done == plan.groups


def test_a_banded_call_is_always_packed():
    """Why the unpacked instantiations have no bands cell: over frames up to 128x96 and every budget that bands them, the plan's own
    answer is packed whenever band_units < units — for frames and for batches, for many workgroups and for one."""
    scene = S.scene_of("ref", False)
    lib = _capi.amd_lib()
    banded = 0
    try:
        for share in (None, 1000):
            rt.set_option("RT_AMD_WF_SHARE", share)
            for w, h in ((67, 45), (64, 48), (128, 96), (8, 96), (97, 8), (33, 17)):
                for budget in sorted({b for k in range(1, 8) for b in (k * 64512 * min(48, (w * h + 63) // 64) // (w * h) + d for d in (-1, 0, 1, 2))} |
                                     {7, 64, 700, 1100, 2048, 4096}):
                    if not 1 <= budget <= 4096:
                        continue
                    _capi.check(lib.rt_set_wavefront_budget(budget))
                    for plan in (diagnostics.pwf_plan(scene, rt.Frame.full(w, h, 5)), diagnostics.pwf_plan_rays(scene, w * h, 5)):
                        assert plan.budget == budget
                        if plan.band_units < plan.units:
                            banded += 1
                            assert plan.packed and plan.ring_cap == 65536, (w, h, budget, share, plan)
    finally:
        rt.set_option("RT_AMD_WF_SHARE", None)
        _capi.check(lib.rt_set_wavefront_budget(6))
    assert banded > 100  # the sweep did meet banded plans


def test_the_packing_threshold_is_31744_nodes_per_arena():
    """PACKED <=> ring_cap == 65536 <=> more than 32768 - 1024 nodes wanted per arena: one workgroup, 64 x k pixels at budget 62, so
    that want = 3968 k walks across the threshold (k = 8: 31744, the last unpacked one; k = 9: 35712)."""
    scene = S.scene_of("ref", False)
    lib = _capi.amd_lib()
    seen = {}
    with rt.options(RT_AMD_WF_SHARE=1000):
        try:
            _capi.check(lib.rt_set_wavefront_budget(62))
            for k in range(1, 17):
                plan = diagnostics.pwf_plan(scene, rt.Frame.full(64, k, 5))
                want = 64 * k * 62
                assert plan.groups == 1 and plan.node_cap == plan.ring_cap - 1024 and plan.ring_cap >= min(65536, want + 1024)
                assert plan.packed == (plan.ring_cap == 65536) == (want > 31744), (k, plan)
                seen[k] = plan.packed
        finally:
            _capi.check(lib.rt_set_wavefront_budget(6))
    assert not seen[8] and seen[9]


@pytest.mark.parametrize("rays", FORMS)
@pytest.mark.parametrize("bfs", WALKERS)
@pytest.mark.parametrize("packed", PACKINGS)
def test_overflow_hands_the_frame_to_the_per_pixel_kernel(packed, bfs, rays):
    """One workgroup whose arena cannot hold the frame's nodes (_pwf_support.py OVERFLOW: the mirror room at depth 20 has 21 nodes per
    pixel, measured on the oracle and checked here; the budget is 1, or 10 for the packed arena, at most half of that): the overflow
    flag is raised — asserted, not inferred — and the oracle's frame and cast count come from the per-pixel kernel."""
    assert S.measured_room_nodes_per_pixel() == S.ROOM_NODES_PER_PIXEL
    steer = S.OVERFLOW_PACKED if packed else S.OVERFLOW_UNPACKED
    assert steer[1] * 2 <= S.ROOM_NODES_PER_PIXEL
    plan, outcome = S.run_cell("room", bfs, rays, steer, S.W1, S.H1, S.ROOM_DEPTH)
    assert plan.groups == 1 and plan.band_units == plan.units
    assert plan.node_cap == (64512 if packed else 7168) and plan.node_cap < S.W1 * S.H1 * S.ROOM_NODES_PER_PIXEL
    assert S.W1 * S.H1 * plan.budget <= 64512  # under the band limit
    assert outcome.overflow and outcome.groups_done == 1 and outcome.tiles_done < S.W1 * S.H1 // 64


@pytest.mark.parametrize("rays", FORMS)
@pytest.mark.parametrize("bfs", WALKERS)
def test_the_same_room_fits_a_generous_arena(bfs, rays):
    """... and the room is rendered by the persistent kernel itself once the arenas hold it: the overflow above is the budget's."""
    finished(S.run_cell("room", bfs, rays, S.PACKED_MANY, S.W, S.H, S.ROOM_DEPTH))


@pytest.mark.parametrize("bfs", WALKERS)
def test_state_between_a_packed_and_an_unpacked_instantiation(bfs):
    """As test_state_between_calls_on_one_stream, across instantiations: a packed frame, an unpacked frame, a ray batch of either, and an
    overflowing frame in between, on one stream and one scene — they share the workspace's header (two alternating blocks of
    counters and the frame description) and its arenas.  Every call: the instantiation, whether it finished, the image, the count."""
    torch = torch_device()
    world, cam = S.world_and_camera("room")
    scene = S.scene_of("room", bfs)
    lib = _capi.amd_lib()
    small, big = rt.Frame.full(S.W, S.H, 5), rt.Frame.full(S.W1, S.H1, S.ROOM_DEPTH)
    want = {"small": S.oracle_frame("room", S.W, S.H, 5), "big": S.oracle_frame("room", S.W1, S.H1, S.ROOM_DEPTH)}
    # (frame, rays, budget, share, packed, overflows)
    steps = [("small", False, 512, None, True, False), ("small", False, 6, None, False, False), ("small", False, 6, None, False, False),
             ("small", False, 512, None, True, False), ("big", False, 10, 1000, True, True), ("small", False, 6, None, False, False),
             ("small", True, 512, None, True, False), ("big", False, 1, 1000, False, True), ("small", False, 512, None, True, False),
             ("small", True, 6, None, False, False), ("small", False, 512, None, True, False)]
    stream = torch.cuda.Stream()
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    with torch.cuda.stream(stream):
        for step, (which, rays, budget, share, packed, overflows) in enumerate(steps):
            frame = small if which == "small" else big
            count.zero_()
            _capi.check(lib.rt_set_wavefront_budget(budget))
            rt.set_option("RT_AMD_WF_SHARE", share)
            try:
                if rays:
                    got = rt.trace_rays(scene, rt.camera_rays(cam, frame, stream=stream), frame.max_depth, ray_count=count, stream=stream)
                    plan = diagnostics.pwf_plan_rays(scene, frame.rows * frame.cols, frame.max_depth, stream=stream)
                else:
                    got = rt.render_whitted(scene, cam, frame, ray_count=count, stream=stream)
                    plan = diagnostics.pwf_plan(scene, frame, stream=stream)
                outcome = diagnostics.pwf_outcome(scene, stream=stream)
            finally:
                _capi.check(lib.rt_set_wavefront_budget(6))
                rt.set_option("RT_AMD_WF_SHARE", None)
            stream.synchronize()
            assert plan.persistent and outcome.launched and plan.instantiation == (packed, bfs, rays), f"step {step}: {plan}"
            assert outcome.overflow == overflows, f"step {step}: {outcome}"
            img = got.cpu().numpy().reshape(frame.rows, frame.cols, 3)
            if rays:
                img = img + np.float32(0.0)  # a frame is accumulated into zeros: -0.0 + 0.0
            bad = _mismatches(img, want[which][0])
            assert bad == 0, f"step {step}: {bad} channels differ"
            assert int(count.item()) == want[which][1], f"step {step}"
