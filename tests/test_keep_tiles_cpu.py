"""CPU model of the keep-edge warp's tiles (tests/warp_tiles.py, rule `written`: k_warp_keep's written samples and box on the oracle's exact map).
It proves that the parameter sets of the GPU tests (test_keep_gpu.py) reach every path of the kernel on BGR, luma and chroma: tiles with no
written sample (copied from prev, or skipped in place), tiles written throughout, mixed tiles staged and gathered, and mixed tiles that the
image's right and bottom edges cut."""
import numpy as np
import pytest

import warp_def as wd
import warp_tiles as wt


@pytest.mark.parametrize("name", sorted(wt.TILE_SETS["keep"]))
def test_set_reaches_its_committed_states(name):
    got = wt.states_of("keep", name)
    for plane, want in wt.TILE_SETS["keep"][name][-1].items():
        for state, least in want.items():
            assert got[plane][state] >= least, (name, plane, state, got[plane])


def test_sets_cover_every_path_of_every_plane():
    total = {p: dict.fromkeys(wt.KEEP_STATES, 0) for p in ("bgr", "luma", "chroma")}
    for name in wt.TILE_SETS["keep"]:
        for plane, counts in wt.states_of("keep", name).items():
            for k in wt.KEEP_STATES:
                total[plane][k] += counts[k]
    for plane, counts in total.items():
        for state in wt.KEEP_STATES:
            assert counts[state] > 0, (plane, state, counts)


def test_boxes_are_over_written_samples_only():
    """One written sample in a tile of NaN and far-away entries: the box is that sample's 2 x 2 footprint (staged), not the stretch to
    -32768 that the border warp's box of every pixel would be; without it the tile is all kept."""
    mx = np.full((16, 64), 1e6, np.float32)
    my = np.full((16, 64), 10.0, np.float32)
    mx[5, 7] = my[5, 7] = np.nan
    assert wt.tile_states(mx, my, 64, 32, "linear", "written")["bgr"]["all_kept"] == 1
    mx[3, 8], my[3, 8] = 20.5, 12.25
    mx[9, 8], my[9, 8] = 63.0, 12.0        # an exact hit on the last column: kept
    s = wt.tile_states(mx, my, 64, 32, "linear", "written")
    assert s["bgr"]["staged_mixed"] == 1 and s["luma"]["staged_mixed"] == 1 and s["bgr"]["gathered"] == 0
    assert s["chroma"]["all_kept"] == 1    # (3, 8) is on an odd row: no chroma sample
    assert abs(1.0 - float(wd.written(mx, my, 64, 32).mean()) - (1 - 1 / 1024)) < 1e-12


def test_budgets_split_staged_from_gathered():
    """Two written samples far apart: 100 x 62 = 6200 positions are over the BGR budget (6144 dwords) and under luma's (12288 bytes)."""
    mx = np.full((16, 64), -5.0, np.float32)
    my = np.full((16, 64), -5.0, np.float32)
    mx[0, 0], my[0, 0] = 0.0, 0.0
    mx[2, 2], my[2, 2] = 98.0, 60.0
    s = wt.tile_states(mx, my, 128, 64, "linear", "written")
    assert s["bgr"]["gathered_mixed"] == 1 and s["luma"]["staged_mixed"] == 1
    assert s["chroma"]["staged_mixed"] == 1   # chroma positions 0 .. 49 x 0 .. 30 of 64 x 32
