"""The tracker's options without a GPU (tests/lk_def.py; include/vstab.h, "Tracker options").  (1) At default options the numpy
definition is the oracle bit for bit -- points, status, iteration counts and per-level positions -- over every case of lk_edges and two
lk_segments sets.  (2) Invariants of the new rules.  (3) Every refusal of vstab_pyr_lk_ex and vstab_set_tracker_options that needs no
device, in order, with its message.  (4) The known-answer set reproduces.  (5) What the GPU test's fixtures reach, asserted against the
definition alone."""
import ctypes
import importlib
import os

import numpy as np
import pytest

import lk_edges as E
import lk_def as D
import lk_segments as S
import oracle

vs = importlib.import_module("video-annotator_amd")


# ---- (1) default options: the oracle ---------------------------------------------------------------------------------------------------------
def check_against_oracle(prev, nxt, pts, what):
    r = D.track(prev, nxt, pts)
    xy, st, lv, nl = oracle.pyr_lk_trace(prev, nxt, pts)
    xy2, st2 = oracle.pyr_lk(prev, nxt, pts)
    it = oracle.pyr_lk_iterations(prev, nxt, pts)[2]
    assert r["nl"] == nl, what
    assert np.array_equal(r["status"], st) and np.array_equal(st, st2), what
    assert E.same_floats(r["xy"], xy).all() and E.same_floats(xy, xy2).all(), what
    assert np.array_equal(r["iterations"], it), what
    assert E.same_floats(r["levels"][:, :nl], lv[:, :nl]).all() and np.isnan(r["levels"][:, nl:]).all(), what
    return r


@pytest.mark.parametrize("size", E.SIZES, ids=E.size_id)
def test_default_options_are_the_oracle_on_the_edge_cases(size):
    w, h = size
    f = E.frames(w, h, 2)
    pts = np.concatenate([E.boundary_cases(w, h)[0], E.special_points(w, h)[0]])
    r = check_against_oracle(f[0], f[1], pts, size)
    assert (r["err"][r["status"] == 0] == 0).all()
    assert D.levels_of(w, h) == E.LEVELS[size]


@pytest.mark.parametrize("name,k", [("jump_640", 3), ("leave_200", 0)])
def test_default_options_are_the_oracle_on_segment_sets(name, k):
    frames, pts, _ = S.make_set(name, n=120)
    r = check_against_oracle(frames[k], frames[k + 1], pts, name)
    assert (r["status"] == 1).sum() > 30 and (r["status"] == 0).sum() >= 1


# ---- (2) invariants ------------------------------------------------------------------------------------------------------------------------
def same_result(a, b):
    return (np.array_equal(a["status"], b["status"]) and E.same_floats(a["xy"], b["xy"]).all() and
            np.array_equal(a["err"].view(np.uint32), b["err"].view(np.uint32)) and np.array_equal(a["min_eig"].view(np.uint32), b["min_eig"].view(np.uint32)))


@pytest.mark.parametrize("size", D.GPU_SIZES[21], ids=E.size_id)
def test_a_guess_equal_to_the_previous_point_is_no_guess(size):
    prev, nxt = D.pair(*size)
    pts = np.concatenate([D.points(*size), E.special_points(*size)[0]])
    for opt in ({}, dict(max_level=1, max_iter=5, eps=0.05, min_eig=1e-3)):
        assert same_result(D.track(prev, nxt, pts, **opt), D.track(prev, nxt, pts, guess=pts.copy(), **opt)), (size, opt)


def test_a_threshold_above_every_window_rejects_everything():
    w, h = D.GPU_SIZES[21][0]
    prev, nxt = D.pair(w, h)
    pts = D.points(w, h)
    top = float(D.track(prev, nxt, pts, min_eig=0.0)["min_eig"].max())
    every = D.track(prev, nxt, pts, min_eig=0.0)
    r = D.track(prev, nxt, pts, min_eig=1e3)
    assert 0 < top < 1e3 and not r["status"].any() and not r["err"].any()
    assert E.same_floats(r["xy"], pts).all()          # no level moved it: back as it came (x 2^-L, then x 2 per level: exact)
    assert not r["iterations"].any()
    # the minimum eigenvalue does not care: the finest formed level reports it, rejected or not
    trk = E.tracked(pts, w, h)
    assert np.array_equal(r["min_eig"].view(np.uint32), every["min_eig"].view(np.uint32))
    assert ((r["min_eig"] != 0) <= trk.any(1)).all() and not r["min_eig"][~trk.any(1)].any()


@pytest.mark.parametrize("opt", [{}, dict(max_iter=2), dict(eps=10.0), dict(max_level=0)], ids=str)
def test_the_residual_by_brute_force(opt):
    w, h = D.GPU_SIZES[21][2]
    prev, nxt = D.pair(w, h)
    pts = D.points(w, h)
    r = D.track(prev, nxt, pts, **opt)
    alive = np.flatnonzero(r["status"] == 1)
    assert alive.size >= 20
    for i in alive[::3]:
        want = D.residual_brute_force(prev, nxt, pts[i], r["xy"][i])
        assert want.view(np.uint32) == r["err"][i].view(np.uint32), (i, want, r["err"][i])
    assert (r["err"][r["status"] == 0] == 0).all() and (r["err"][alive] > 0).any()


@pytest.mark.parametrize("thr", [1e-4, 1e-3, 2e-2])
def test_the_minimum_eigenvalue_against_the_threshold(thr):
    """level 0 is the finest level: where its matrix was formed, status 0 by rejection means minEig < threshold (or D < FLT_EPSILON, which these
    frames do not reach without it), and a point that went on to iterate has minEig >= threshold"""
    w, h = D.GPU_SIZES[21][1]
    prev, nxt = D.pair(w, h)
    pts = D.points(w, h)
    r = D.track(prev, nxt, pts, min_eig=thr)
    formed0 = E.tracked(pts, w, h)[:, 0]
    iterated0 = r["iterations"][:, 0] > 0
    assert (r["min_eig"][iterated0] >= np.float32(thr)).all() and iterated0.sum() >= 5
    rejected0 = formed0 & ~iterated0
    assert rejected0.any() and (r["min_eig"][rejected0] < np.float32(thr)).all() and not r["status"][rejected0].any()
    assert (r["status"][r["status"] == 1] <= iterated0[r["status"] == 1]).all()


def test_fewer_levels_is_the_capped_pyramid():
    """rule 1 on its own: max_level = 3 on a 2-level frame changes nothing, and the level count is min(levels, max_level + 1)"""
    for size in D.GPU_SIZES[21]:
        for ml in range(4):
            assert D.levels_of(*size, max_level=ml) == min(E.LEVELS.get(size, S.level_sizes(*size)[0]), ml + 1)
    prev, nxt = D.pair(130, 80)
    pts = D.points(130, 80)
    assert same_result(D.track(prev, nxt, pts, max_level=1), D.track(prev, nxt, pts, max_level=3))


# ---- (3) refusals ----------------------------------------------------------------------------------------------------------------------------
def _ex(**kw):
    """vstab_pyr_lk_ex with pointers nobody dereferences before the refusal: -> (status, message)"""
    L = vs.lib
    a = dict(prev=4096, pp=640, nxt=8192, pn=640, w=640, h=360, n=4, max_level=3, max_iter=30, eps=0.01, min_eig=1e-4, flags=0, err=True)
    a.update(kw)
    xy, out, st, err = np.zeros(8, np.float32), np.zeros(8, np.float32), np.zeros(4, np.uint8), np.zeros(4, np.float32)
    fp = lambda x: x.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    s = L.vstab_pyr_lk_ex(a["prev"], a["pp"], a["nxt"], a["pn"], a["w"], a["h"], fp(xy), a["n"], fp(out), st.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                          fp(err) if a["err"] else None, a["max_level"], a["max_iter"], a["eps"], a["min_eig"], a["flags"], None)
    return s, L.vstab_last_error().decode()


NAN, INF = float("nan"), float("inf")
REFUSALS = [("bad argument", [dict(prev=None), dict(nxt=None), dict(n=-1), dict(w=0), dict(h=-2), dict(pp=639), dict(pn=1)]),
            ("max_level lies in 0 .. 3", [dict(max_level=-1), dict(max_level=4), dict(max_level=1 << 30)]),
            ("max_iter lies in 1 .. 100", [dict(max_iter=0), dict(max_iter=-5), dict(max_iter=101)]),
            ("eps is finite and lies in [0, 10]", [dict(eps=-1e-300), dict(eps=10.000001), dict(eps=NAN), dict(eps=INF), dict(eps=-INF)]),
            ("min_eig_threshold is finite and not negative", [dict(min_eig=-1e-300), dict(min_eig=NAN), dict(min_eig=INF), dict(min_eig=-INF)]),
            ("unknown flag", [dict(flags=1), dict(flags=2), dict(flags=16), dict(flags=4 | 8 | 32), dict(flags=-1)]),
            ("VSTAB_LK_GET_MIN_EIGENVALS needs err", [dict(flags=8, err=False), dict(flags=12, err=False)])]


def test_pyr_lk_ex_refusals_in_order():
    for k, (msg, bads) in enumerate(REFUSALS):
        want = (vs.ERR_INVALID, "vstab_pyr_lk_ex: " + msg)
        for bad in bads:
            assert _ex(**bad) == want, bad
            # everything later in the order is wrong too: the earlier message wins
            for later_msg, later in REFUSALS[k + 1:]:
                assert _ex(**{**later[0], **bad}) == want, (bad, later[0])
    # vstab_pyr_lk's own message keeps its name
    out, st = np.zeros(8, np.float32), np.zeros(4, np.uint8)
    fp = out.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    assert vs.lib.vstab_pyr_lk(None, 640, 8192, 640, 640, 360, fp, 4, fp, st.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), None) == vs.ERR_INVALID
    assert vs.lib.vstab_last_error().decode() == "vstab_pyr_lk: bad argument"


def test_the_binding_knows_the_entry_points():
    assert "vstab_pyr_lk_ex" in vs.SIGNATURES and "vstab_set_tracker_options" in vs.SIGNATURES
    assert (vs.LK_USE_INITIAL_FLOW, vs.LK_GET_MIN_EIGENVALS) == (4, 8) == (D.USE_INITIAL_FLOW, D.GET_MIN_EIGENVALS)


def test_set_tracker_options_refuses_a_null_handle():
    for args in ((3, 30, 0.01, 1e-4), (9, 0, NAN, -1.0)):       # before every option
        assert vs.lib.vstab_set_tracker_options(None, *args) == vs.ERR_INVALID
        assert vs.lib.vstab_last_error().decode() == "vstab_set_tracker_options: null handle"


# ---- (4) the known answers -------------------------------------------------------------------------------------------------------------------
def test_known_answers_reproduce():
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_lk_options_golden as G
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lk_options_kat.npz")
    assert os.path.getsize(path) < 100 * 1024
    kat = np.load(path)
    for name, (prev, nxt, pts, opt, guess) in G.cases().items():
        assert 24 <= len(pts) <= 64
        assert np.array_equal(kat[name + "_pts"].view(np.uint32), pts.view(np.uint32)), name
        if guess is not None:
            assert np.array_equal(kat[name + "_guess"].view(np.uint32), guess.view(np.uint32)), name
        r = D.track(prev, nxt, pts, guess=guess, **opt)
        for k in G.KEYS:
            a, b = kat[f"{name}_{k}"], r[k]
            same = E.same_floats(a, b).all() if a.dtype == np.float32 else np.array_equal(a, b)
            assert same, (name, k)
        assert r["status"].any() and not r["status"].all(), name


# ---- (5) what the GPU test's fixtures reach ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", D.GPU_SIZES[21], ids=E.size_id)
def test_main_cases_have_both_statuses(size):
    prev, nxt = D.pair(*size)
    pts = D.points(*size)
    r = D.track(prev, nxt, pts)
    assert D.levels_of(*size) == {(360, 200): 4, (240, 144): 3, (130, 80): 2, (40, 30): 1}[size]
    assert 3 * int((r["status"] == 1).sum()) >= len(pts) and int((r["status"] == 0).sum()) >= 3, (size, r["status"].sum(), len(pts))


def test_each_option_separates():
    base = {}
    for name, opt in D.OPTION_CASES:
        prev, nxt, pts = D.option_inputs(name)
        key = D.on_moved_pair(name)
        if key not in base:
            base[key] = D.track(prev, nxt, pts)
        r = D.track(prev, nxt, pts, **opt)
        assert not same_result(r, base[key]), name
        assert 3 * int((r["status"] == 1).sum()) >= len(pts) or name in ("min_eig_1",), (name, r["status"].sum())
    # the moved pair needs its pyramid: level 0 alone brings fewer points to where the scene went
    prev, nxt, pts = D.option_inputs("max_level_0")
    on_truth = lambda r: int(((np.abs(r["xy"] - (pts + np.float32(D.MOTION))).max(1) < 0.5) & (r["status"] == 1)).sum())
    assert on_truth(D.track(prev, nxt, pts, max_level=0)) < on_truth(base[True]) and on_truth(base[True]) >= 40


@pytest.mark.parametrize("size", D.GPU_SIZES[21], ids=E.size_id)
def test_initial_flow_cases(size):
    w, h = size
    prev, nxt = D.pair(w, h)
    nl = D.levels_of(w, h)
    cases = D.guesses(w, h, D.points(w, h), nl)
    plain = D.track(prev, nxt, cases["truth_pm3"][0])
    r = D.track(prev, nxt, cases["truth_pm3"][0], guess=cases["truth_pm3"][1])
    assert not same_result(r, plain) and 3 * int(r["status"].sum()) >= len(r["status"])
    # the far side: the search really starts there (the first level's estimate is the guess's), and nearly everything is lost or lands elsewhere
    pts, g = cases["far_side"]
    far = D.track(prev, nxt, pts, guess=g)
    assert not same_result(far, D.track(prev, nxt, pts))
    # both sides of the top level's range: the outer guesses fail the first iteration's range test at every level and come back bit for bit
    pts, g = cases["top_level_edges"]
    e = D.track(prev, nxt, pts, guess=g)
    L = nl - 1
    wl, hl = S.level_sizes(w, h)[1][L]
    org = E.origins(g, L)
    outside = (org[:, 0] < -S.LKW) | (org[:, 0] >= wl) | (org[:, 1] < -S.LKW) | (org[:, 1] >= hl)
    assert outside.sum() == 4 and (~outside).sum() == 4
    assert not e["iterations"][outside, L].any() or (e["iterations"][outside, L] == 1).all()
    assert (e["iterations"][~outside, L] >= 1).all()
    # non-finite and huge guesses: status 0, the guess back (NaN for NaN), no error measure; -0.0 is an ordinary guess
    pts, g = cases["specials"]
    s = D.track(prev, nxt, pts, guess=g)
    wild = ~np.isfinite(g).all(1) | (np.abs(g) > 1e29).any(1)
    assert not s["status"][wild].any() and E.same_floats(s["xy"][wild], g[wild]).all() and not s["err"][wild].any()
    assert (s["iterations"][wild].sum(1) == nl).all()            # one refused iteration per level
    assert (~wild).sum() == 3 and (s["iterations"][~wild].sum(1) > nl).all()   # (-0.0, y), (x, -0.0), (-0.0, -0.0)
    assert (s["min_eig"] > 0).all()                               # the previous point's matrix was formed all the same
    pts, g = cases["block_across_border"]
    c = D.track(prev, nxt, pts, guess=g)
    assert (c["iterations"][:, L] >= 1).all()


def test_the_jump_pair_leaves_the_staged_block():
    """the residual's window lies outside the block the iterations left staged: the kernel's epilogue stages afresh.  At default options
    the last step is at most eps long and the branch is out of reach; a capped or a one-level search ends in mid-flight."""
    prev, nxt, pts = D.jump_pair()
    assert not D.track(prev, nxt, pts)["resid_restaged"].any()
    for opt in D.JUMP_OPTIONS:
        r = D.track(prev, nxt, pts, **opt)
        assert int(r["resid_restaged"].sum()) >= 10 and (r["status"][r["resid_restaged"]] == 1).all(), opt
