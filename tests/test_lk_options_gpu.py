"""GPU half of the tracker-option tests: vstab_pyr_lk_ex (k_lk_track_opt, and k_lk_track where launch_lk routes to it) and a handle with
vstab_set_tracker_options against tests/lk_def.py.  Every comparison is bit-exact -- points, status, err as float bits (a NaN for a
NaN) -- and no point is left out; the pipeline's rotations carry the 1e-9 of test_pipeline_gpu.py.  What the fixtures reach is asserted
without a GPU in test_lk_options_cpu.py."""
import numpy as np
import pytest

import lk_edges as E
import lk_def as D
import oracle

pytestmark = pytest.mark.gpu


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


def both_err_modes(vs, cuda, prev, nxt, pts, opt, guess, what):
    """the call with err in its default mode and with VSTAB_LK_GET_MIN_EIGENVALS, each against the definition; -> the definition's answer"""
    want = D.track(prev, nxt, pts, guess=guess, **opt)
    kw = dict(max_level=opt.get("max_level", 3), max_iter=opt.get("max_iter", 30), eps=opt.get("eps", 0.01), min_eig_threshold=opt.get("min_eig", 1e-4))
    dp, dn = dev(prev, cuda), dev(nxt, cuda)
    flow = vs.LK_USE_INITIAL_FLOW if guess is not None else 0
    for flags, key in ((flow, "err"), (flow | vs.LK_GET_MIN_EIGENVALS, "min_eig")):
        got = vs.pyr_lk_ex(dp, dn, pts, flags=flags, guess=guess, **kw)
        check(got, want["xy"], want["status"], want[key], (what, key))
    return want, (dp, dn, kw)


# ---- default options with err: the OPT instantiation is the default one -------------------------------------------------------------------------
@pytest.mark.parametrize("size", D.GPU_SIZES[21], ids=E.size_id)
def test_default_options_with_err_are_pyr_lk(vs, cuda, size):
    w, h = size
    prev, nxt = D.pair(w, h)
    pts = np.concatenate([D.points(w, h), E.special_points(w, h)[0]])
    want, (dp, dn, kw) = both_err_modes(vs, cuda, prev, nxt, pts, {}, None, size)
    xy, st = vs.pyr_lk(dp, dn, pts)
    check((xy, st, None), want["xy"], want["status"], None, (size, "vstab_pyr_lk"))
    # and without err, at default options, vstab_pyr_lk_ex is vstab_pyr_lk
    check(vs.pyr_lk_ex(dp, dn, pts, want_err=False), xy, st, None, (size, "no err"))
    ox, ost = oracle.pyr_lk(prev, nxt, pts)
    check((xy, st, None), ox, ost, None, (size, "oracle"))


# ---- one option at a time, then combined --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,opt", D.OPTION_CASES, ids=[n for n, _ in D.OPTION_CASES])
def test_options(vs, cuda, name, opt):
    prev, nxt, pts = D.option_inputs(name)
    want, (dp, dn, kw) = both_err_modes(vs, cuda, prev, nxt, pts, opt, None, name)
    # without err: k_lk_track_opt with no error measure -- or, where only the level count differs, k_lk_track on the capped pyramid
    check(vs.pyr_lk_ex(dp, dn, pts, want_err=False, **kw), want["xy"], want["status"], None, (name, "no err"))
    print(name, "status 1:", int(want["status"].sum()), "of", len(pts), "iterations", want["iterations"].sum(0).tolist())


# ---- the initial flow -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", D.GPU_SIZES[21], ids=E.size_id)
def test_initial_flow(vs, cuda, size):
    w, h = size
    prev, nxt = D.pair(w, h)
    nl = D.levels_of(w, h)
    prev_pts = np.concatenate([D.points(w, h), E.special_points(w, h)[0]])
    for name, (pts, guess) in D.guesses(w, h, prev_pts, nl).items():
        for opt in ({}, dict(max_level=1, max_iter=5, eps=0.05, min_eig=1e-3)) if name in ("truth_pm3", "guess_is_prev") else ({},):
            want, (dp, dn, kw) = both_err_modes(vs, cuda, prev, nxt, pts, opt, guess, (size, name, opt))
            if name == "guess_is_prev":   # the bytes of the call without the flag
                check(vs.pyr_lk_ex(dp, dn, pts, **kw), want["xy"], want["status"], want["err"], (size, name, "no flag"))
        print(size, name, "status 1:", int(want["status"].sum()), "of", len(pts))


def test_jump_pair_final_window_leaves_the_staged_block(vs, cuda):
    prev, nxt, pts = D.jump_pair()
    for opt in D.JUMP_OPTIONS + ({},):
        want, _ = both_err_modes(vs, cuda, prev, nxt, pts, opt, None, ("jump", opt))
        print(opt, "residuals behind a re-staged block:", int(want["resid_restaged"].sum()))


# ---- the pipeline ---------------------------------------------------------------------------------------------------------------------------------
PIPE_OPTIONS = (2, 8, 0.03, 1e-3)


def state_machine(frames, K, w, h, r, seed, opt):
    """mask_def.run_state_machine with track = the definition at the options `opt` (max_level, max_iter, eps, min_eig)"""
    Ko, _ = oracle.get_output_camera(K, w, h)
    rng = oracle.Pcg32(seed)
    counts, warp_rots = [], []

    def track(prev, cur, corners):
        if len(corners) == 0:
            counts.append((0, 0))
            return corners, corners
        res = D.track(prev, cur, corners, max_level=opt[0], max_iter=opt[1], eps=opt[2], min_eig=opt[3])
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


def test_pipeline_with_tracker_options(vs, cuda):
    """ten frames of corner_tiles' banded 640 x 360 clip: 200 corners that all stay tracked, no key frame behind the first -- so the handle's
    launches are the multi-pair segments and the chained launches, with options"""
    import corner_tiles as C
    import expect
    import test_pipeline_gpu as P
    (w, h), frames = C.pipeline_clip("under_spec_cap")
    frames, n, r, seed = frames[:10], 10, 2, 1
    K = oracle.get_preset_camera(4, w, h)
    stab, outs = P.run_product(vs, cuda, frames, smooth_radius=r, seed=seed, tracker_options=PIPE_OPTIONS)
    log = stab.frame_log()
    assert len(outs) == n - 1 and len(log) == n - 1
    Ko, (cw, ch) = oracle.get_output_camera(K, w, h)
    sm, exp, counts, warp_rots = state_machine(frames, K, w, h, r, seed, PIPE_OPTIONS)
    assert [l["key"] for l in log] == [l["key"] for l in sm.log]
    assert [(l["n_corners"], l["n_tracked"]) for l in log] == counts
    assert [l["inliers"] for l in log] == [l["inliers"] for l in sm.log]
    assert all(np.allclose(a["R"], b["R"], atol=1e-9) for a, b in zip(log, sm.log))
    for i in range(len(outs)):
        assert np.allclose(stab.warp_rotation(i), warp_rots[i], atol=1e-9), i
        p = oracle.map_params(K, Ko, stab.warp_rotation(i))
        assert np.array_equal(outs[i], expect.warp(exp[i], p, cw, ch)), i
    plain, _ = P.run_product(vs, cuda, frames, smooth_radius=r, seed=seed)
    key = lambda l: (l["key"], l["n_corners"], l["n_tracked"], l["inliers"], l["R"].tobytes())
    assert [key(l) for l in plain.frame_log()] != [key(l) for l in log]
    assert min(l["n_tracked"] for l in log) >= 150 and not any(l["key"] for l in log)
    # the default options, set explicitly, are the handle as it always was
    same, _ = P.run_product(vs, cuda, frames, smooth_radius=r, seed=seed, tracker_options=(3, 30, 0.01, 1e-4))
    assert [key(l) for l in plain.frame_log()] == [key(l) for l in same.frame_log()]


# ---- the refusals that need a handle ----------------------------------------------------------------------------------------------------------------
def test_setter_refusals_that_need_a_handle(vs, cuda):
    import synth
    import torch
    w, h = 322, 182
    K = oracle.get_preset_camera(4, w, h)
    frames, _ = synth.shaky_clip(5, K, w, h, 5, sigma=0.004)
    devf = [torch.from_numpy(f).to(cuda) for f in frames]
    L = vs.lib
    nan, inf = float("nan"), float("inf")

    def refused(stab, msg, *args):
        assert L.vstab_set_tracker_options(stab._h, *args) == vs.ERR_INVALID
        assert L.vstab_last_error().decode() == "vstab_set_tracker_options: " + msg

    def drain(stab):
        k = 0
        while stab.pull() is not None:
            k += 1
        return k

    off = vs.Stabilizer(devf, total=4, smooth_radius=1, tracking=0)
    refused(off, "no tracker runs on this handle (tracking = 0)", 3, 30, 0.01, 1e-4)
    refused(off, "no tracker runs on this handle (tracking = 0)", 7, 0, nan, -1.0)                      # before every option
    off.close()
    stab = vs.Stabilizer(devf, total=4, smooth_radius=1, seed=2)
    for ml in (-1, 4):
        refused(stab, "max_level lies in 0 .. 3", ml, 0, nan, -1.0)                                     # the order: before the later ones
    for mi in (0, 101, -3):
        refused(stab, "max_iter lies in 1 .. 100", 3, mi, nan, -1.0)
    for eps in (-1e-9, 10.5, nan, inf):
        refused(stab, "eps is finite and lies in [0, 10]", 3, 30, eps, nan)
    for me in (-1e-9, nan, inf):
        refused(stab, "min_eig_threshold is finite and not negative", 3, 30, 0.01, me)
    # a refused call leaves the handle unchanged: still the plain handle
    plain = vs.Stabilizer(devf, total=4, smooth_radius=1, seed=2)
    assert drain(plain) == 3 and drain(stab) == 3
    key = lambda l: (l["key"], l["n_corners"], l["n_tracked"], l["R"].tobytes())
    assert [key(l) for l in stab.frame_log()] == [key(l) for l in plain.frame_log()]
    refused(stab, "the options must be set before the first pull", 2, 8, 0.03, 1e-3)
    refused(stab, "the options must be set before the first pull", 9, 0, nan, -1.0)                     # before every option
    stab.close()
    # the edges of what is accepted
    ok = vs.Stabilizer(devf, total=4, smooth_radius=1, seed=2)
    for args in ((0, 1, 0.0, 0.0), (3, 100, 10.0, 1e30)):
        assert L.vstab_set_tracker_options(ok._h, *args) == 0, args
    assert drain(ok) == 3 and all(l["n_tracked"] == 0 for l in ok.frame_log())                          # (a threshold of 1e30 rejects every window)
    assert L.vstab_set_tracker_options(None, 3, 30, 0.01, 1e-4) == vs.ERR_INVALID
    assert L.vstab_last_error().decode() == "vstab_set_tracker_options: null handle"
