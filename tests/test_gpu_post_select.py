"""The select of post_process on the device, at its edges (csrc/rt_post.hip; references and key sets: tests/_post_support.py, shown
adversarial on the CPU by tests/test_post_reference.py):
  1. rt_post_hist_device / rt_post_pick_device on keys and state written by the test, against np.sort — one band, and 2 and 3 interleaved
     bands plus an empty band and a band of invalid keys, the states summed between the passes;
  2. rt_post_keys_device on lumas of every class of float;
  3. rt_post_process_device against the sort and the host form, bit for bit, and the divisor of an empty image."""
import ctypes as C

import numpy as np
import pytest

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import _capi
import _post_support as ps

pytestmark = pytest.mark.gpu

SETS = ps.key_sets()


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    import torch

    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _upload_u32(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).cuda()


def _words(t):
    return t.cpu().numpy().view(np.uint32).astype(np.int64)


class _Band:
    """one band's keys and its state: 260 zero words with state[0] = the number of valid keys"""

    def __init__(self, keys):
        self.n = int(keys.size)
        self.keys = _upload_u32(keys if keys.size else np.zeros(1, np.uint32))
        state = np.zeros(ps.STATE_WORDS, np.uint32)
        state[0] = (keys != ps.KEY_INVALID).sum()
        self.state = _upload_u32(state)

    def hist(self, p):
        _capi.check(_capi.amd_lib().rt_post_hist_device(_ptr(self.keys), self.n, p, _ptr(self.state), _stream()))

    def pick(self, p):
        _capi.check(_capi.amd_lib().rt_post_pick_device(p, _ptr(self.state), _stream()))


def _run_select(keys, parts):
    bands = [_Band(keys)] if parts == 1 else [_Band(b) for b in ps.bands_of(keys, parts)]
    total = sum(b.state[0:1] for b in bands)
    for b in bands:
        b.state[0:1].copy_(total)
    trace = ps.select_trace(keys)
    count = int((keys != ps.KEY_INVALID).sum())
    for p in range(4):
        for b in bands:
            b.hist(p)
        hist = sum(b.state[4:260] for b in bands)
        if parts == 1 or p == 0:  # one band sees the whole histogram; so does the sum
            assert np.array_equal(_words(hist), trace[p][0] if trace else np.zeros(256, np.int64)), ("histogram", p)
        for b in bands:
            b.state[4:260].copy_(hist)
            b.pick(p)
        for b in bands:
            state = _words(b.state)
            assert state[0] == count and not state[4:260].any(), ("count kept, histogram cleared", p)
            if trace:
                assert state[1] == trace[p][2], ("rank inside the chosen bin", p, state[1], trace[p][2])
                assert state[2] >> (24 - 8 * p) == ps.select_reference(keys) >> (24 - 8 * p), ("prefix", p, hex(state[2]))
    want = ps.select_reference(keys)
    for b in bands:
        assert _words(b.state)[3] == (ps.KEY_INVALID if want is None else want)


@pytest.mark.parametrize("parts", (1, 2, 3))
@pytest.mark.parametrize("name", sorted(SETS))
def test_select_on_chosen_keys_equals_the_sort(name, parts):
    _run_select(SETS[name], parts)


def test_histograms_of_the_later_passes_over_bands_sum_to_the_reference():
    """what test_select_on_chosen_keys_equals_the_sort checks for one band in every pass, for three bands: the summed histogram of
    each pass is the sort's (the decoys of pass 3 and the set decided beyond the first stride)"""
    for name in ("decoys_pass3", "length_grid_stride", "invalid_99_percent"):
        keys = SETS[name]
        bands = [_Band(b) for b in ps.bands_of(keys, 3)]
        total = sum(b.state[0:1] for b in bands)
        for b in bands:
            b.state[0:1].copy_(total)
        for p, (want, _, _) in enumerate(ps.select_trace(keys)):
            for b in bands:
                b.hist(p)
            hist = sum(b.state[4:260] for b in bands)
            assert np.array_equal(_words(hist), want), (name, p)
            for b in bands:
                b.state[4:260].copy_(hist)
                b.pick(p)


# ---- 2. the key map ---------------------------------------------------------------------------------------------------------------------

def test_keys_of_every_class_of_luma():
    import torch

    row = rt.luma_row()
    img = ps.luma_class_image(row)
    luma = ps.luma_reference(img, row)
    normal = ps.is_normal(luma)
    band = torch.from_numpy(img.copy()).cuda()
    keys = torch.full((img.shape[0],), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    state = torch.full((ps.STATE_WORDS,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    _capi.check(_capi.amd_lib().rt_post_keys_device(_ptr(band), img.shape[0], _ptr(keys), _ptr(state), _stream()))
    got, state = _words(keys), _words(state)
    assert np.array_equal(got != ps.KEY_INVALID, normal), (luma[(got != ps.KEY_INVALID) != normal], got[(got != ps.KEY_INVALID) != normal])
    assert state[0] == normal.sum() and not state[1:].any()
    order = np.argsort(got[normal], kind="stable")
    assert (np.diff(luma[normal][order]) >= 0).all()  # sorting by key is sorting by value
    values, first = np.unique(luma[normal], return_index=True)
    assert (np.diff(got[normal][first]) > 0).all() and values.size > 30  # strictly monotone over the distinct values
    for v in values:  # equal values, equal keys
        assert np.unique(got[normal][luma[normal] == v]).size == 1


# ---- 3. rt_post_process_device ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("content", ps.POST_CONTENTS)
@pytest.mark.parametrize("shape", ps.POST_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_post_process_equals_the_sort_and_the_host(shape, content):
    import torch

    row = rt.luma_row()
    img = ps.post_image(shape, content, row)
    want, wdiv = ps.post_process_reference(img, row)
    t = torch.from_numpy(img.copy()).cuda()
    div = torch.full((1,), -7.0, dtype=torch.float32, device="cuda")
    rt.post_process_device(t, divisor=div)
    got, gdiv = t.cpu().numpy(), div.cpu().numpy()
    host = img.copy()
    hdiv = np.float32(rt.post_process(host))
    assert ps.bits(gdiv)[0] == ps.bits(np.array([wdiv], np.float32))[0] == ps.bits(np.array([hdiv]))[0], (gdiv, wdiv, hdiv)
    assert np.array_equal(ps.bits(got), ps.bits(want)) and np.array_equal(ps.bits(host), ps.bits(want))


def test_empty_image_writes_a_zero_divisor_in_stream_order():
    """n_pixels = 0: *d_divisor receives 0.0 by a write enqueued on the caller's stream (include/rt_amd.h) — also on a side stream, also
    captured into a graph and replayed"""
    import torch

    empty = torch.ones((2, 5, 3), dtype=torch.float32, device="cuda")[:0]  # no pixels, and a pointer that is not null
    div = torch.full((3,), -7.0, dtype=torch.float32, device="cuda")
    rt.post_process_device(empty, divisor=div[1:2])
    assert div.cpu().tolist() == [-7.0, 0.0, -7.0]
    side = torch.cuda.Stream()
    div.fill_(-7.0)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        rt.post_process_device(empty, divisor=div[1:2], stream=side)
    side.synchronize()
    assert div.cpu().tolist() == [-7.0, 0.0, -7.0]
    rt.post_process_device(empty)  # no divisor wanted: nothing to do
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rt.post_process_device(empty, divisor=div[1:2])
    div.fill_(-7.0)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert div.cpu().tolist() == [-7.0, 0.0, -7.0]
