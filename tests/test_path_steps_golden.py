"""The CPU forms of the path loop against words recorded before its plumbing was shared (tests/golden/path_steps.npz, written by
tools/make_path_steps_golden.py from the commit before csrc/rt_path_kernel.h): begin, advance, resolve, branch, transmit, connect,
settle, weigh_escape, connect_lights, settle_lights and light_seed on one crafted batch of 67 slots — dead slots, "no hit" vertices,
glass, a spot light — listed in every way: all slots, an index list with a repeated entry, entries >= M and a count > M, the list
cut short, and a count of 0.  Word equality: the device tests compare against these forms, and the forms share the device's headers;
the fixture shares nothing.  No GPU."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent


def _generator():
    spec = importlib.util.spec_from_file_location("make_path_steps_golden", ROOT / "tools" / "make_path_steps_golden.py")
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


@pytest.fixture(scope="module")
def computed():
    return _generator().steps()


@pytest.fixture(scope="module")
def recorded():
    with np.load(ROOT / "tests" / "golden" / "path_steps.npz") as z:
        return {name: z[name] for name in z.files}


FORMS = ("begin", "advance", "resolve", "branch", "transmit", "connect", "settle", "weigh_escape", "connect_lights", "settle_lights", "light_seed")


def test_the_fixture_holds_every_form_under_every_list(recorded):
    assert {name.split(".")[0] for name in recorded} == set(FORMS)
    for form in FORMS[1:2] + FORMS[3:10]:
        for listing in ("all", "list", "short", "none"):
            assert any(name.startswith(f"{form}.{listing}.") for name in recorded), (form, listing)


def test_the_same_arrays_are_computed(computed, recorded):
    assert sorted(computed) == sorted(recorded)


@pytest.mark.parametrize("form", FORMS)
def test_every_word_is_the_recorded_one(form, computed, recorded):
    names = [name for name in recorded if name.split(".")[0] == form]
    assert names
    for name in names:
        got, want = computed[name], recorded[name]
        assert got.dtype == want.dtype and got.shape == want.shape, name
        differ = np.argwhere(got != want)
        assert differ.size == 0, f"{name}: {len(differ)} words differ, the first at {tuple(differ[0])}: {got[tuple(differ[0])]:#x}, recorded {want[tuple(differ[0])]:#x}"
