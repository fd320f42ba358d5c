"""GPU half of the tests of k_corners_fused's ownership seams (tests/corner_seams.py; what the frames reach is asserted without a GPU in
test_corner_seams_cpu.py): on every frame the eigenvalue map bit for bit, the fused detector's raw keys and per-tile counts against the tile
model, and both public detectors against the oracle.  Every comparison is exact."""
import numpy as np
import pytest

import corner_seams as S
import oracle
from test_corner_paths_gpu import check_operators, check_raw, dev, unaligned_view

pytestmark = pytest.mark.gpu


def check_frame(vs, m, gray):
    got = vs.min_eig(gray).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), m.eig.view(np.uint32))
    check_raw(vs, m, gray)
    check_operators(vs, m, gray)


@pytest.mark.parametrize("w,h", S.sizes(), ids=lambda v: str(v))
def test_borders_on_every_ownership_position(vs, cuda, w, h):
    """noise, and noise under rectangles, at every size: the border path everywhere, and from 132 x 66 on the interior path beside it"""
    for kind in ("noise", "rects"):
        m = S.model(kind, w, h)
        check_frame(vs, m, dev(m.img, cuda))


@pytest.mark.parametrize("w,h", [S.BIG, S.RINGED, (67, 33), (4, 5)], ids=lambda v: str(v))
def test_unaligned_views_take_the_border_path_everywhere(vs, cuda, w, h):
    """a base that is not 4-byte aligned and an odd pitch: no tile is interior, and the results are those of the aligned image"""
    assert not S.interior_map(w, h, aligned=False).any()
    for kind in ("noise", "rects"):
        m = S.model(kind, w, h)
        check_frame(vs, m, unaligned_view(m.img, cuda))


def test_interior_and_border_tiles_in_one_launch_run_after_run(vs, cuda):
    """321 x 125 holds six interior tiles among thirty: three runs, one key set, and the tile counts of every run inside the model's range"""
    assert S.interior_map(*S.BIG).sum() == 6
    for kind in ("noise", "rects"):
        m = S.model(kind, *S.BIG)
        g = dev(m.img, cuda)
        runs = [check_raw(vs, m, g) for _ in range(3)]
        assert all(np.array_equal(r[0], runs[0][0]) for r in runs)


def test_good_features_on_a_frame_of_the_largest_size(vs, cuda):
    """640 x 360: eighty interior tiles; the pipeline's parameters and every candidate in order"""
    w, h = 640, 360
    assert S.interior_map(w, h).sum() == 80
    m = S.model("rects", w, h)
    g = dev(m.img, cuda)
    check_frame(vs, m, g)
    exp = oracle.good_features(m.img, 200, 0.01, 30.0)
    assert np.array_equal(vs.good_features(g, 200, 0.01, 30.0), exp) and len(exp) > 50
