"""Which code a Whitted call ran (include/rt_amd.h rt_diag_pwf_plan / rt_diag_pwf_plan_rays / rt_diag_pwf_outcome): the persistent
wavefront kernel has eight instantiations, pwf_kernel<PACKED, BFS, RAYS>, and a frame its arenas cannot finish is rendered by the
per-pixel kernel with the same pixels and cast count — results alone say neither which instantiation a call reached nor whether the
persistent kernel finished the frame.  Read-only: nothing here allocates, launches or changes a setting.

Workspaces are made by the first call that needs them and only grow, so ask AFTER the call in question, with the budget and the
switches as that call had them: the answer is then what that call launched.  ``stream`` is the stream of that call (default: torch's
current stream; the numpy forms run on the null stream, which torch's default stream is).
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

from . import _capi
from ._args import _stream_ptr
from ._capi import Frame
from ._world import Scene

PLAN_WORDS = 10     # RT_DIAG_PWF_PLAN_WORDS
OUTCOME_WORDS = 6   # RT_DIAG_PWF_OUTCOME_WORDS


class PwfPlan(NamedTuple):
    """rt_diag_pwf_plan's words, in their order (RT_DIAG_PWF_PERSISTENT .. RT_DIAG_PWF_BUDGET)"""
    persistent: bool  # the call launches the persistent kernel (else the per-pixel kernel renders the frame)
    groups: int       # workgroups, one arena each
    units: int        # rows of the frame / rays of the batch
    band_units: int   # ... per launch: below `units` the call is several bands
    ring_cap: int
    node_cap: int
    packed: bool      # the three template arguments
    bfs: bool
    rays: bool
    budget: int       # nodes per pixel

    @property
    def instantiation(self):
        return (self.packed, self.bfs, self.rays)


class PwfOutcome(NamedTuple):
    """rt_diag_pwf_outcome's words (of a call of several bands: its last band)"""
    launched: bool    # the call launched the persistent kernel
    overflow: bool    # ... which did not finish the frame within its arenas: the per-pixel kernel rendered it
    tiles_done: int
    groups_done: int
    casts: int        # what the persistent kernel counted

    @property
    def finished(self):
        """the persistent kernel rendered the frame itself"""
        return self.launched and not self.overflow


def _plan(words) -> PwfPlan:
    w = list(words)
    return PwfPlan(bool(w[0]), w[1], w[2], w[3], w[4], w[5], bool(w[6]), bool(w[7]), bool(w[8]), w[9])


def pwf_plan(scene: Scene, frame: Frame, stream=None) -> PwfPlan:
    """The plan of render_whitted(scene, camera, frame) on ``stream``, whatever the camera."""
    words = (C.c_uint32 * PLAN_WORDS)()
    _capi.check(_capi.amd_lib().rt_diag_pwf_plan(scene._h, C.byref(frame), _stream_ptr(stream), words))
    return _plan(words)


def pwf_plan_rays(scene: Scene, n_rays: int, max_depth: int, stream=None) -> PwfPlan:
    """The plan of trace_rays(scene, rays, max_depth) on ``stream`` for a batch of ``n_rays`` rays."""
    words = (C.c_uint32 * PLAN_WORDS)()
    _capi.check(_capi.amd_lib().rt_diag_pwf_plan_rays(scene._h, int(n_rays), int(max_depth), _stream_ptr(stream), words))
    return _plan(words)


def pwf_outcome(scene: Scene, stream=None) -> PwfOutcome:
    """How the last render_whitted / trace_rays call on ``stream`` ended; waits for that stream."""
    words = (C.c_uint32 * OUTCOME_WORDS)()
    _capi.check(_capi.amd_lib().rt_diag_pwf_outcome(scene._h, _stream_ptr(stream), words))
    w = list(words)
    return PwfOutcome(bool(w[0]), bool(w[1]), w[2], w[3], w[4] | (w[5] << 32))
