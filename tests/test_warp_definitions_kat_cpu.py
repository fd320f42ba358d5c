"""The recorded answers of the warp definition and of the tile model (tests/golden/warp_definitions_kat.npz; what it holds and where it comes
from: tests/golden/make_warp_definitions_golden.py) against tests/warp_def.py and tests/warp_tiles.py as they are now: the file was written by
the layered definitions and the five tile models these two modules replaced, so every array must come out of them bit for bit."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_warp_definitions_golden as gen  # noqa: E402
import warp_tiles as wt  # noqa: E402


@pytest.fixture(scope="module")
def kat():
    return gen.load()


def same(kat, fresh):
    for key, v in fresh.items():
        assert v.dtype == kat[key].dtype and v.shape == kat[key].shape and v.tobytes() == kat[key].tobytes(), key


def test_the_definition_reproduces_the_recorded_remaps(kat):
    fresh = gen.definition_answers()
    assert set(fresh) == {k for k in kat.files if not k.startswith("states_")}
    same(kat, fresh)
    assert sum(k.startswith("constant_") and k.endswith(("cubic", "lanczos4")) for k in fresh) == 6
    assert sum(k.startswith("keep_") and "border" in k for k in fresh) == 6 and sum(k.endswith("_constant") for k in fresh) == 6


def test_the_tile_model_reproduces_the_recorded_states(kat):
    fresh = gen.state_answers()
    assert set(fresh) == {k for k in kat.files if k.startswith("states_")}
    same(kat, fresh)
    sets = sum(len(v) for v in wt.TILE_SETS.values())
    assert sum(k.startswith("states_set_") for k in fresh) == sets + len(wt.TILE_SETS["border"])      # k_warp_border's under both of its rules
    assert {k.rsplit("_", 1)[1] for k in fresh} == set(wt.RULES)


def test_the_file_is_small(kat):
    assert os.path.getsize(os.path.join(os.path.dirname(gen.__file__), "warp_definitions_kat.npz")) < 200 * 1024
