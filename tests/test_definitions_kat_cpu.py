"""The recorded answers of the numpy definitions (tests/golden/definitions_kat.npz; golden/make_definitions_golden.py says where they come
from): the file is a fixture of ordinary size, and the definitions there are now -- tests/corner_def.py, tests/lk_def.py and the fetch-ahead
model of tests/lk_segments.py -- reproduce every array in it bit for bit, with none missing and none left over.  The tests that used to hold
two definitions against each other (test_lk_window_cpu.py, test_corner_gradient_cpu.py, test_corner_block_cpu.py) read the same file."""
import glob
import os
import sys

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
import make_definitions_golden as G  # noqa: E402


def test_the_file_is_no_larger_than_the_largest_fixture_there_was():
    others = [p for p in glob.glob(os.path.join(GOLDEN, "*.npz")) if os.path.basename(p) != "definitions_kat.npz"]
    assert os.path.getsize(os.path.join(GOLDEN, "definitions_kat.npz")) <= max(os.path.getsize(p) for p in others) < 1 << 20


def test_the_definitions_reproduce_the_file():
    kat = G.load()
    now = {**G.detector_answers(), **G.tracker_answers()}
    assert sorted(now) == sorted(kat.files) and len(now) == 646
    for k, v in now.items():
        want = kat[k]
        assert want.dtype == v.dtype and want.shape == v.shape and want.tobytes() == np.ascontiguousarray(v).tobytes(), k      # (bytes: the sign of a zero counts)
    for size in G.E.SIZES:                                       # every case of the tests that read the file is in it
        assert "track_edge_" + G.E.size_id(size) + "_options_xy" in now
    assert all(f"block3_{n}_a" in now for n in G.MEASURED) and all(f"products_cut_66x33_B{b}_dxdy" in now for b in (3, 5, 7))
