"""GPU half of the detector-argument tests: the edge values of `quality` that the contract accepts (tests/test_detect_args_cpu.py has
what it refuses) through every detector of every entry point, against the definitions: oracle.good_features (plain), corner_def (masked,
Harris, Harris with a mask).

    1e-300           the threshold (float)((double)maxVal * quality) rounds to 0: every positive 3 x 3 maximum is a corner
    nextafter(1, 0)  the threshold rounds to maxVal itself
    1.0, 2.0, inf    strict >: nothing lies above the maximum, twice the maximum, infinity -- no corner, no error

The fused detector filters a tile with quality * max(own tile, published maximum), a lower bound of the final threshold for every
quality > 0; these values are where that product leaves the floats it was tuned on.  min_distance at its own edges (0, inf) rides along."""
import numpy as np
import pytest

import corner_def
import oracle
import synth

pytestmark = pytest.mark.gpu

QUALITIES = (1e-300, float(np.nextafter(1.0, 0.0)), 1.0, 2.0, float("inf"))
MAX_CORNERS = 4000


def _frames():
    """name -> (gray, mask): a 322 x 182 luma frame and a 129 x 63 cut of it (on the device a view of the frame: its pitch, an odd base)"""
    big = np.ascontiguousarray(synth.luma(51, 322, 182, rects=60))   # (synth.luma hands back a transposed view)
    out = {}
    for name, (x0, y0, w, h) in {"322x182": (0, 0, 322, 182), "129x63_cut": (37, 21, 129, 63)}.items():
        ys, xs = np.mgrid[0:h, 0:w]
        mask = (((xs // 24 + ys // 16) % 3 != 0) * 255).astype(np.uint8)
        mask[h // 3:h // 2, w // 4:w // 2] = 0
        out[name] = (big, (x0, y0, w, h), mask)
    return out


FRAMES = _frames()


def _device(name, cuda):
    import torch
    big, (x0, y0, w, h), mask = FRAMES[name]
    dbig = torch.from_numpy(big).to(cuda)
    return np.ascontiguousarray(big[y0:y0 + h, x0:x0 + w]), dbig[y0:y0 + h, x0:x0 + w], mask, torch.from_numpy(mask).to(cuda)


@pytest.mark.parametrize("quality", QUALITIES, ids=("q=1e-300", "q=just_under_1", "q=1", "q=2", "q=inf"))
@pytest.mark.parametrize("name", sorted(FRAMES))
def test_accepted_quality_edges(vs, cuda, name, quality):
    g, dg, mask, dmask = _device(name, cuda)
    md = 5.0
    want = {"plain": oracle.good_features(g, MAX_CORNERS, quality, md),
            "masked": corner_def.good_features(g, mask, MAX_CORNERS, quality, md),
            "harris": corner_def.good_features(g, None, MAX_CORNERS, quality, md, harris=True),
            "harris_masked": corner_def.good_features(g, mask, MAX_CORNERS, quality, md, harris=True)}
    # the unmasked definition and the oracle are one definition
    assert np.array_equal(want["plain"], corner_def.good_features(g, np.ones_like(mask), MAX_CORNERS, quality, md))
    print(name, quality, {k: len(v) for k, v in want.items()})
    if quality < 1.0:
        assert quality > 1e-3 or all(len(v) > 20 for v in want.values())
    else:
        assert all(len(v) == 0 for v in want.values())
    got = {"plain": [vs.good_features(dg, MAX_CORNERS, quality, md)]}
    for det in (vs.DETECTOR_AUTO, vs.DETECTOR_TWO_PASS):
        got["plain"].append(vs.good_features(dg, MAX_CORNERS, quality, md, detector=det))
    for det in (vs.DETECTOR_AUTO, vs.DETECTOR_FUSED, vs.DETECTOR_TWO_PASS):
        got["plain"].append(vs.good_features_mask(dg, None, MAX_CORNERS, quality, md, detector=det))
        got.setdefault("masked", []).append(vs.good_features_mask(dg, dmask, MAX_CORNERS, quality, md, detector=det))
        got.setdefault("harris", []).append(vs.good_features_harris(dg, None, MAX_CORNERS, quality, md, detector=det))
        got.setdefault("harris_masked", []).append(vs.good_features_harris(dg, dmask, MAX_CORNERS, quality, md, detector=det))
    for kind, runs in got.items():
        for i, r in enumerate(runs):
            assert r.shape == want[kind].shape and np.array_equal(r, want[kind]), (name, quality, kind, i, r.shape, want[kind].shape)


@pytest.mark.parametrize("name", sorted(FRAMES))
def test_accepted_min_distance_edges(vs, cuda, name):
    """min_distance 0 (no grid), -0.0, beyond the diagonal, just under 2^31, 1e300 and inf: the definitions' corners, one corner from
    the diagonal on, through the three detectors"""
    g, dg, mask, dmask = _device(name, cuda)
    h, w = g.shape
    for md in (0.0, -0.0, float(np.hypot(w, h)) + 1.0, 2147483000.0, 1e300, float("inf")):
        want = oracle.good_features(g, MAX_CORNERS, 0.01, md)
        want_m = corner_def.good_features(g, mask, MAX_CORNERS, 0.01, min(md, 1e6))   # (its grid is python's: any cell beyond the image is one cell)
        assert len(want) == (1 if md > 1 else MAX_CORNERS) or (md <= 1 and len(want) > 20)
        assert np.array_equal(vs.good_features(dg, MAX_CORNERS, 0.01, md), want), md
        for det in (vs.DETECTOR_AUTO, vs.DETECTOR_FUSED, vs.DETECTOR_TWO_PASS):
            assert np.array_equal(vs.good_features_mask(dg, None, MAX_CORNERS, 0.01, md, detector=det), want), (md, det)
            assert np.array_equal(vs.good_features_mask(dg, dmask, MAX_CORNERS, 0.01, md, detector=det), want_m), (md, det)
