"""GPU half of the tracker-window tests: vstab_pyr_lk_win, the vstabx_lk_segments_win hook and a handle with vstab_set_tracker_window
(k_lk_track_win for the windows 15 and 31) against tests/lk_def.py.  Every comparison is bit-exact -- points, status, err in both
modes as float bits, the records of every pair of a segment -- and no point is left out; the pipeline's rotations carry the 1e-9 of
test_lk_options_gpu.py.  What the fixtures reach is asserted without a GPU in test_lk_window_cpu.py."""
import numpy as np
import pytest

import lk_def as W
import lk_edges as E
import lk_segments as S
import oracle

pytestmark = pytest.mark.gpu

CASES = [(win, size) for win in W.NEW_WINDOWS for size in W.GPU_SIZES[win]]
CASE_IDS = ["w%d-%dx%d" % (win, *size) for win, size in CASES]


def dev(img, cuda):
    import torch
    return torch.from_numpy(np.ascontiguousarray(img)).to(cuda)


def check(got, want_xy, want_st, want_err, what):
    xy, st, err = got
    bad = np.flatnonzero(st != want_st)
    assert bad.size == 0, (what, "status", bad[:5], st[bad[:5]], want_st[bad[:5]])
    bad = np.argwhere(~E.same_floats(xy, want_xy))
    assert bad.size == 0, (what, "x / y bits", bad[:5], xy[bad[0][0]], want_xy[bad[0][0]], want_st[bad[0][0]])
    if want_err is not None:
        bad = np.flatnonzero(err.view(np.uint32) != want_err.view(np.uint32))
        assert bad.size == 0, (what, "err bits", bad[:5], err[bad[:5]], want_err[bad[:5]], want_st[bad[:5]])


def both_err_modes(vs, cuda, prev, nxt, pts, win, opt, guess, what):
    """the call with err in its default mode, with VSTAB_LK_GET_MIN_EIGENVALS and without err, each against the definition"""
    want = W.track(prev, nxt, pts, win, guess=guess, **opt)
    kw = dict(max_level=opt.get("max_level", 3), max_iter=opt.get("max_iter", 30), eps=opt.get("eps", 0.01), min_eig_threshold=opt.get("min_eig", 1e-4))
    dp, dn = dev(prev, cuda), dev(nxt, cuda)
    flow = vs.LK_USE_INITIAL_FLOW if guess is not None else 0
    for flags, key in ((flow, "err"), (flow | vs.LK_GET_MIN_EIGENVALS, "min_eig")):
        check(vs.pyr_lk_win(dp, dn, pts, win, flags=flags, guess=guess, **kw), want["xy"], want["status"], want[key], (what, key))
    check(vs.pyr_lk_win(dp, dn, pts, win, flags=flow, guess=guess, want_err=False, **kw), want["xy"], want["status"], None, (what, "no err"))
    return want


# ---- the stateless entry point: every level count, the boundary of the range test at every level, the frame smaller than the window ------------
@pytest.mark.parametrize("win,size", CASES, ids=CASE_IDS)
def test_every_level_count(vs, cuda, win, size):
    w, h = size
    prev, nxt = W.pair(w, h)
    pts = np.concatenate([W.window_points(w, h, win), E.special_points(w, h)[0]])
    want = both_err_modes(vs, cuda, prev, nxt, pts, win, {}, None, (win, size))
    print(win, size, "levels", want["nl"], "status 1:", int(want["status"].sum()), "of", len(pts))


# ---- options on the 4-level frame -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("win", W.NEW_WINDOWS)
def test_combined_options(vs, cuda, win):
    w, h = W.GPU_SIZES[win][0]
    prev, nxt = W.moved_pair(w, h)
    both_err_modes(vs, cuda, prev, nxt, W.window_points(w, h, win), win, W.COMBINED, None, (win, "combined"))


@pytest.mark.parametrize("win", W.NEW_WINDOWS)
def test_initial_flow(vs, cuda, win):
    w, h = W.GPU_SIZES[win][0]
    prev, nxt = W.pair(w, h)
    for name, (pts, guess) in W.window_guesses(w, h, win).items():
        want = both_err_modes(vs, cuda, prev, nxt, pts, win, {}, guess, (win, name))
        print(win, name, "status 1:", int(want["status"].sum()), "of", len(pts))


@pytest.mark.parametrize("win", W.NEW_WINDOWS)
def test_jump_pair_final_window_leaves_the_staged_block(vs, cuda, win):
    prev, nxt, pts = W.jump_pair()
    want = both_err_modes(vs, cuda, prev, nxt, pts, win, dict(max_iter=1), None, (win, "jump"))
    print(win, "residuals behind a re-staged block:", int(want["resid_restaged"].sum()))


# ---- segments and chained launches ------------------------------------------------------------------------------------------------------------
def check_records(exp, hrec, drec, what):
    """test_lk_segments_gpu.check_records, and the position of a status-0 record as well (where the definition dropped the slot)"""
    K, n = exp["status"].shape
    assert hrec.shape == (K, n, 4)
    assert np.array_equal(hrec, drec), (what, "host and device records differ")
    seq = np.arange(1, K + 1, dtype=np.uint32)[:, None]
    assert np.array_equal(hrec[..., 1], np.broadcast_to(seq, (K, n))), what
    assert np.array_equal(hrec[..., 3] >> 2, np.broadcast_to(seq, (K, n))), what
    st = hrec[..., 3] & 3
    bad = np.argwhere(st != exp["status"])
    assert bad.size == 0, (what, "status", bad[:5], st[tuple(bad[0])], exp["status"][tuple(bad[0])])
    tracked = exp["status"] <= 1
    xy = hrec[..., [0, 2]]
    same = E.same_floats(xy.view(np.float32), exp["xy"])
    bad = np.argwhere(tracked[..., None] & ~same)
    assert bad.size == 0, (what, "x / y bits", bad[:5], xy.view(np.float32)[tuple(bad[0][:2])], exp["xy"][tuple(bad[0][:2])])
    assert not (~tracked[..., None] & (xy != 0)).any(), what


@pytest.mark.parametrize("name", S.SEGMENT_CLIPS)
@pytest.mark.parametrize("win", W.NEW_WINDOWS)
def test_segments_and_chains(vs, cuda, win, name):
    frames, pts, exps = S.segment_case(name, win)
    df = [dev(f, cuda) for f in frames]
    recs = []
    for segs, exp in exps.items():
        hrec, drec, _ = vs.lk_segments(df, pts, list(segs), win=win)
        check_records(exp, hrec, drec, (win, name, segs))
        recs.append(hrec)
        assert (exp["status"] == 2).any(), (win, name)      # slots lost earlier are part of the case
    assert np.array_equal(recs[0], recs[1]), (win, name, "segment invariance")
    # a wrong parent tag: status 3 from that launch on
    hrec, drec, _ = vs.lk_segments(df, pts, [3, 3, 2], bad_parent=1, win=win)
    check_records(S.expected(frames[:4], pts, (3,), W=win), hrec[:3], drec[:3], (win, name, "before the bad parent"))
    assert (hrec[3:, :, 3] & 3 == 3).all() and np.array_equal(hrec, drec)


# ---- the pipeline -----------------------------------------------------------------------------------------------------------------------------
def state_machine(frames, K, w, h, r, seed, win):
    """test_lk_options_gpu.state_machine with track = the definition at window `win`"""
    Ko, _ = oracle.get_output_camera(K, w, h)
    rng = oracle.Pcg32(seed)
    counts, warp_rots = [], []

    def track(prev, cur, corners):
        if len(corners) == 0:
            counts.append((0, 0))
            return corners, corners
        res = W.track(prev, cur, corners, win)
        nxt, st = res["xy"], res["status"]
        counts.append((len(corners), int((st > 0).sum())))
        return corners[st > 0], nxt[st > 0]

    sm = oracle.WarpStateMachine(frames, r, lambda g: oracle.good_features(np.ascontiguousarray(g)), track, lambda pp, cp: oracle.estimate_rotation(pp, cp, K, Ko, rng), lambda f, R: (warp_rots.append(R), f)[1])
    exp = []
    while True:
        o = sm.pull_frame()
        if o is None:
            break
        exp.append(o)
    return sm, exp, counts, warp_rots


_key = lambda l: (l["key"], l["n_corners"], l["n_tracked"], l["inliers"], l["R"].tobytes())


@pytest.fixture(scope="module")
def pipe(vs, cuda):
    import corner_tiles as C
    import test_pipeline_gpu as P
    (w, h), frames = C.pipeline_clip("under_spec_cap")
    frames = frames[:10]
    plain, _ = P.run_product(vs, cuda, frames, smooth_radius=2, seed=1)
    return w, h, frames, [_key(l) for l in plain.frame_log()]


@pytest.mark.parametrize("win", W.NEW_WINDOWS)
def test_pipeline_with_tracker_window(vs, cuda, pipe, win):
    """ten frames of corner_tiles' banded 640 x 360 clip: the handle's multi-pair segments and chained launches with the window"""
    import expect
    import test_pipeline_gpu as P
    w, h, frames, plain_log = pipe
    n, r, seed = 10, 2, 1
    K = oracle.get_preset_camera(4, w, h)
    stab, outs = P.run_product(vs, cuda, frames, smooth_radius=r, seed=seed, tracker_window=win)
    log = stab.frame_log()
    assert len(outs) == n - 1 and len(log) == n - 1
    Ko, (cw, ch) = oracle.get_output_camera(K, w, h)
    sm, exp, counts, warp_rots = state_machine(frames, K, w, h, r, seed, win)
    assert [l["key"] for l in log] == [l["key"] for l in sm.log]
    assert [(l["n_corners"], l["n_tracked"]) for l in log] == counts
    assert [l["inliers"] for l in log] == [l["inliers"] for l in sm.log]
    assert all(np.allclose(a["R"], b["R"], atol=1e-9) for a, b in zip(log, sm.log))
    for i in range(len(outs)):
        assert np.allclose(stab.warp_rotation(i), warp_rots[i], atol=1e-9), i
        p = oracle.map_params(K, Ko, stab.warp_rotation(i))
        assert np.array_equal(outs[i], expect.warp(exp[i], p, cw, ch)), i
    assert plain_log != [_key(l) for l in log]


def test_pipeline_window_21_is_the_plain_handle(vs, cuda, pipe):
    import test_pipeline_gpu as P
    w, h, frames, plain_log = pipe
    same, _ = P.run_product(vs, cuda, frames, smooth_radius=2, seed=1, tracker_window=21)
    assert plain_log == [_key(l) for l in same.frame_log()]
    # the default options set explicitly beside the window are the window alone: vstab_set_tracker_options does not reset it
    a, _ = P.run_product(vs, cuda, frames, smooth_radius=2, seed=1, tracker_window=31)
    stab = vs.Stabilizer([dev(f, cuda) for f in frames], total=len(frames), smooth_radius=2, seed=1)
    stab.set_tracker_window(31)
    stab.set_tracker_options(3, 30, 0.01, 1e-4)
    while stab.pull() is not None:
        pass
    assert [_key(l) for l in a.frame_log()] == [_key(l) for l in stab.frame_log()] != plain_log


# ---- the refusals that need a handle, and the routing ----------------------------------------------------------------------------------------------
def test_setter_refusals_that_need_a_handle(vs, cuda):
    import synth
    import torch
    w, h = 322, 182
    K = oracle.get_preset_camera(4, w, h)
    frames, _ = synth.shaky_clip(5, K, w, h, 5, sigma=0.004)
    devf = [torch.from_numpy(f).to(cuda) for f in frames]
    L = vs.lib

    def refused(stab, msg, win):
        assert L.vstab_set_tracker_window(stab._h, win) == vs.ERR_INVALID
        assert L.vstab_last_error().decode() == "vstab_set_tracker_window: " + msg

    def drain(stab):
        k = 0
        while stab.pull() is not None:
            k += 1
        return k

    off = vs.Stabilizer(devf, total=4, smooth_radius=1, tracking=0)
    for win in (31, 16):                                                                 # before the window's own message
        refused(off, "no tracker runs on this handle (tracking = 0)", win)
    off.close()
    stab = vs.Stabilizer(devf, total=4, smooth_radius=1, seed=2)
    for win in (0, -21, 14, 16, 17, 20, 22, 30, 32, 33, 1 << 30):
        refused(stab, "win_size is 15, 21 or 31", win)
    # a refused call leaves the handle unchanged: still the plain handle
    plain = vs.Stabilizer(devf, total=4, smooth_radius=1, seed=2)
    assert drain(plain) == 3 and drain(stab) == 3
    key = lambda l: (l["key"], l["n_corners"], l["n_tracked"], l["R"].tobytes())
    assert [key(l) for l in stab.frame_log()] == [key(l) for l in plain.frame_log()]
    for win in (15, 16):                                                                 # before the window's own message
        refused(stab, "the window must be set before the first pull", win)
    stab.close()
    # in either order with the options, and every offered size
    ok = vs.Stabilizer(devf, total=4, smooth_radius=1, seed=2)
    for win in (15, 21, 31):
        assert L.vstab_set_tracker_window(ok._h, win) == 0, win
    assert L.vstab_set_tracker_options(ok._h, 1, 10, 0.02, 1e-4) == 0 and L.vstab_set_tracker_window(ok._h, 15) == 0
    assert drain(ok) == 3
    ok.close()


@pytest.mark.parametrize("size", [(360, 200), (40, 30)], ids=E.size_id)
def test_window_21_is_pyr_lk_ex(vs, cuda, size):
    w, h = size
    prev, nxt = W.pair(w, h)
    pts = W.points(w, h)
    dp, dn = dev(prev, cuda), dev(nxt, cuda)
    for kw in (dict(), dict(max_level=2, max_iter=8, eps=0.03, min_eig_threshold=1e-3), dict(flags=vs.LK_GET_MIN_EIGENVALS)):
        a, b = vs.pyr_lk_win(dp, dn, pts, 21, **kw), vs.pyr_lk_ex(dp, dn, pts, **kw)
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes(), (size, kw)
    a, b = vs.pyr_lk_win(dp, dn, pts, 21, want_err=False), vs.pyr_lk(dp, dn, pts)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
