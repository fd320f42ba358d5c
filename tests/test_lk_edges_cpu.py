"""CPU half of the LK argument-edge tests (tests/lk_edges.py): the case set reaches what it claims -- every (level, axis, side, in | out)
boundary per size, every pattern "levels >= L tracked, below skipped" on all four sides --, the reference agrees with the model level by
level, the three statements of the pyramid's level count agree at every size, and the reference refuses every non-finite or huge start
point.  The GPU half (tests/test_lk_edges_gpu.py) runs the same cases through vstab_pyr_lk and k_lk_track's multi-pair launches."""
import numpy as np
import pytest

import lk_edges as E
import lk_segments as S
import oracle

SIDES = {(0, "lo"): "left", (0, "hi"): "right", (1, "lo"): "top", (1, "hi"): "bottom"}


@pytest.mark.parametrize("size", E.SIZES, ids=E.size_id)
def test_level_counts_agree(size):
    """lk_segments.level_sizes, the oracle's vo_pyramid_levels and the table written out in lk_edges.LEVELS: one level count per size, on
    both sides of 42|43, 84|85 and 168|169 on each axis (the library's own lk_levels: the pyramid bytes in test_lk_edges_gpu.py)"""
    w, h = size
    nl, sizes = S.level_sizes(w, h)
    assert nl == E.LEVELS[size] == oracle.lib().vo_pyramid_levels(w, h)
    assert [lv.shape[::-1] for lv in E.pyramid(np.zeros((h, w), np.uint8))] == sizes


@pytest.mark.parametrize("size", E.SIZES, ids=E.size_id)
def test_every_boundary_and_pattern_is_reached(size):
    w, h = size
    nl, sizes = S.level_sizes(w, h)
    pts, tags = E.boundary_cases(w, h)
    trk = E.tracked(pts, w, h)
    # every (level, axis, side, in | out) is present, sits on the origin it names, and decides that level (the other axis is in range)
    seen = {}
    for i, t in enumerate(tags):
        if t[0] != "edge":
            continue
        _, l, axis, side, io = t
        seen[t[1:]] = i
        n_l = sizes[l][axis]
        want = {("lo", "out"): -E.LKW - 1, ("lo", "in"): -E.LKW, ("hi", "in"): n_l - 1, ("hi", "out"): n_l}[(side, io)]
        assert E.origins(pts[i, axis], l) == want, (t, pts[i])
        assert trk[i, l] == (io == "in"), (t, pts[i])
    assert set(seen) == {(l, axis, side, io) for l in range(nl) for axis in (0, 1) for side in ("lo", "hi") for io in ("in", "out")}
    # the pair of a boundary are float32 neighbours
    for (l, axis, side, io), i in seen.items():
        if io == "in":
            j = seen[(l, axis, side, "out")]
            toward = -np.inf if side == "lo" else np.inf
            assert np.nextafter(pts[i, axis], np.float32(toward), dtype=np.float32) == pts[j, axis]
    # every pattern "levels >= L tracked, below skipped", L = 0 .. nl, on every side
    for (axis, side), name in SIDES.items():
        got = {E.pattern(trk[i]) for i, t in enumerate(tags) if t[0] == "edge" and t[2] == axis and t[3] == side}
        assert got == set(range(nl + 1)), (name, got)
    # the corners: both axes on a boundary at once, each decided by its own axis
    corners = [i for i, t in enumerate(tags) if t[0] == "corner"]
    assert len(corners) >= 12
    for i in corners:
        _, (a, sx, iox), (b, sy, ioy) = tags[i]
        assert not trk[i, a] if iox == "out" else True
        assert not trk[i, b] if ioy == "out" else True
        if a == b and iox == ioy == "in":
            assert trk[i, a]
    assert any(trk[i].any() for i in corners) and any(not trk[i].any() for i in corners)


@pytest.mark.parametrize("size", E.SIZES, ids=E.size_id)
def test_oracle_iterates_exactly_where_the_model_says(size):
    """oracle.pyr_lk_iterations: 0 iterations exactly on the levels the model calls skipped or whose matrix is rejected (and on the levels
    the pyramid lacks); status 0 wherever level 0 is one of them; and tracked levels do real work on every size that has texture."""
    w, h = size
    f = E.frames(w, h)
    pts, tags = E.boundary_cases(w, h)
    nl = S.level_sizes(w, h)[0]
    trk = E.tracked(pts, w, h)
    rej = E.matrix_rejected(f[0], pts)
    nxt, st, it = oracle.pyr_lk_iterations(f[0], f[1], pts)
    runs = trk & ~rej
    assert np.array_equal(it[:, :nl] > 0, runs), np.argwhere((it[:, :nl] > 0) != runs)[:5]
    assert not it[:, nl:].any()
    assert not st[~runs[:, 0]].any()
    print(size, "iterating levels", int(runs.sum()), "of", int(trk.sum()), "tracked; status 1:", int(st.sum()))
    if min(w, h) >= 7:   # (1 x 1 has no gradient, 2 x 3 none the 3 x 3 Scharr taps keep: every matrix is rejected)
        assert runs.any(), "no level of any point iterates"
    if min(w, h) > 30:
        assert runs.all(1).any() and (st == 1).any(), "no point is tracked through every level"
    # a skipped point comes back as it went in (every level skipped: the estimate is the start point scaled down and up again)
    none = ~trk.any(1)
    assert none.any() and E.same_floats(nxt[none], pts[none]).all()


@pytest.mark.parametrize("size", [(640, 360), (130, 80), (40, 30), (7, 9)], ids=E.size_id)
def test_oracle_refuses_non_finite_and_huge_points(size):
    """status 0 and the point unchanged (NaN for NaN) for every point with a special coordinate; -0.0 and the smallest denormal track as
    0.0 does; the chained expectation reports 0 in pair 0 and 2 afterwards"""
    w, h = size
    f = E.frames(w, h)
    pts, n_special, like_zero = E.special_points(w, h)
    assert n_special == 9 + 9 + 81
    assert not E.tracked(pts[:n_special], w, h).any() and E.tracked(pts[n_special:], w, h)[:, 0].all()
    nxt, st, it = oracle.pyr_lk_iterations(f[0], f[1], pts)
    assert not st[:n_special].any() and not it[:n_special].any()
    assert E.same_floats(nxt[:n_special], pts[:n_special]).all()
    for i, j in like_zero:
        assert st[i] == st[j] and np.array_equal(nxt[i], nxt[j]) and np.array_equal(it[i], it[j]), (pts[i], nxt[i], nxt[j])
    exp = S.expected(f, pts, [2])
    assert (exp["status"][0, :n_special] == 0).all() and (exp["status"][1, :n_special] == 2).all()
