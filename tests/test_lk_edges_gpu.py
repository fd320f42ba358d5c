"""GPU half of the LK argument-edge tests (tests/lk_edges.py): start points on both sides of every boundary of the per-level range test,
at every pyramid depth, on both sides of the level-count thresholds and on frames smaller than the window; and non-finite or huge start
points.  vstab_pyr_lk against oracle.pyr_lk, and k_lk_track's multi-pair launches (the same points as pair 0 of a 2-pair launch and of
two chained 1-pair launches, through vstabx_lk_segments) against lk_segments.expected: every status byte and every coordinate bit, the
points with status 0 included; the library's pyramid against the oracle's at every size."""
import numpy as np
import pytest

import lk_edges as E
import lk_segments as S
import oracle

pytestmark = pytest.mark.gpu


def _dev(frames, cuda):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(f)).to(cuda) for f in frames]


def check_pair(got_xy, got_st, exp_xy, exp_st, what):
    bad = np.flatnonzero(got_st != exp_st)
    assert bad.size == 0, (what, "status", bad[:5], got_st[bad[:5]], exp_st[bad[:5]])
    bad = np.argwhere(~E.same_floats(got_xy, exp_xy))
    assert bad.size == 0, (what, "x / y bits", bad[:5], got_xy[bad[0][0]], exp_xy[bad[0][0]], exp_st[bad[0][0]])


def check_records(exp, hrec, drec, what):
    """host copy == device copy; both tags; every status byte; the x / y bits of status 0 and 1 (NaN for NaN); status 2 at (0, 0)"""
    K, n = exp["status"].shape
    assert hrec.shape == (K, n, 4) and np.array_equal(hrec, drec), (what, "host and device records differ")
    seq = np.broadcast_to(np.arange(1, K + 1, dtype=np.uint32)[:, None], (K, n))
    assert np.array_equal(hrec[..., 1], seq) and np.array_equal(hrec[..., 3] >> 2, seq), what
    xy = np.ascontiguousarray(hrec[..., [0, 2]]).view(np.float32)
    for k in range(K):
        check_pair(xy[k], (hrec[k, :, 3] & 3).astype(np.uint8), exp["xy"][k], exp["status"][k], (what, "pair", k))


def run_points(vs, cuda, f, pts, what):
    df = _dev(f, cuda)
    exp_xy, exp_st = oracle.pyr_lk(f[0], f[1], pts)
    got_xy, got_st = vs.pyr_lk(df[0], df[1], pts)
    check_pair(got_xy, got_st, exp_xy, exp_st, (what, "pyr_lk"))
    exp = S.expected(f, pts, [2])
    assert np.array_equal(exp["status"][0], exp_st) and E.same_floats(exp["xy"][0], exp_xy).all()
    recs = []
    for segs in ([2], [1, 1]):
        hrec, drec, pyr = vs.lk_segments(df, pts, segs, want_pyr=True)
        check_records(exp, hrec, drec, (what, segs))
        recs.append(hrec)
    assert np.array_equal(recs[0], recs[1]), (what, "segment invariance")
    return exp, pyr


@pytest.mark.parametrize("size", E.SIZES, ids=E.size_id)
def test_boundary_points(vs, cuda, size):
    """every (level, axis, side, in | out) start point and the corner cases of the size; the library built the pyramid the oracle builds
    (the level count on both sides of its thresholds: a level too many or too few changes the bytes it hands back)"""
    w, h = size
    f = E.frames(w, h)
    pts, tags = E.boundary_cases(w, h)
    exp, pyr = run_points(vs, cuda, f, pts, size)
    # the cases do what the CPU half says: both statuses at pair 0, lost points reported as 2 at pair 1
    assert (exp["status"][0] == 0).any() and ((exp["status"][0] == 1).any() or min(w, h) <= 30)
    assert ((exp["status"][1] == 2) == (exp["status"][0] == 0)).all()
    for i, img in enumerate(f):
        lv = E.pyramid(img)[1:]
        dense = np.concatenate([x.ravel() for x in lv]) if lv else np.zeros(1, np.uint8)
        assert pyr.shape[1] == dense.size and np.array_equal(pyr[i], dense), (size, "pyramid of frame", i)


@pytest.mark.parametrize("size", [(640, 360), (130, 80), (40, 30), (7, 9)], ids=E.size_id)
def test_non_finite_and_huge_points(vs, cuda, size):
    """NaN, +-inf, +-1e30, +-3e9, 2^31 and -(2^31 + 256) in either or both coordinates: status 0 and the point back as it came (NaN for
    NaN), then status 2; -0.0 and the smallest denormal track as 0.0 does.  4-, 2- and 1-level pyramids and a frame below the window."""
    w, h = size
    f = E.frames(w, h)
    pts, n_special, like_zero = E.special_points(w, h)
    df = _dev(f, cuda)
    got_xy, got_st = vs.pyr_lk(df[0], df[1], pts)
    print(size, "status of the special points:", got_st[:n_special].tolist())
    assert not got_st[:n_special].any(), np.flatnonzero(got_st[:n_special])
    assert E.same_floats(got_xy[:n_special], pts[:n_special]).all()
    for i, j in like_zero:
        assert got_st[i] == got_st[j] and np.array_equal(got_xy[i], got_xy[j]), (pts[i], got_xy[i], got_xy[j])
    exp, _ = run_points(vs, cuda, f, pts, size)
    assert (exp["status"][0, :n_special] == 0).all() and (exp["status"][1, :n_special] == 2).all()
