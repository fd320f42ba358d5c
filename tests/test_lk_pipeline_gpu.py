"""GPU half of the handle tests of the tracker's window and options (tests/lk_pipeline.py): a handle with vstab_set_tracker_window and / or
vstab_set_tracker_options across the planned key frame (speculative detection, the key segment launched from the speculated corners, adopt,
the chained launches up to it), the unplanned one (dropped launches, the restart from the host's corners), at every pyramid depth on both
ingest routes, as a 10-bit handle, beside a second handle and beside the detector's options -- each against oracle.WarpStateMachine with
track = lk_def.track and find = corner_def.good_features.  Every comparison is the one test_lk_options_gpu.py and test_lk_window_gpu.py make:
key flags, (n_corners, n_tracked) and inliers equal, R and the warp rotations within 1e-9, every emitted frame bit-exact against
expect.warp.  What the fixtures reach is asserted without a GPU in test_lk_pipeline_cpu.py."""
import numpy as np
import pytest

import lk_def as W
import lk_pipeline as P
import oracle

pytestmark = pytest.mark.gpu

LOG_KEY = lambda l: (l["key"], l["n_corners"], l["n_tracked"], l["inliers"], l["fallback"], l["R"].tobytes())
# the launch shapes of test_unplanned_key_frames_drop_the_tracker_launches_enqueued_ahead
ENVS = ({"VSTAB_LK_SEGMENT": "1"}, {"VSTAB_CHAIN_LK": "0"}, {"VSTAB_LK_SEGMENT": "3", "VSTAB_LK_SEG_TARGET": "2"}, {"VSTAB_EPOCH_OVERLAP": "0"},
        {"VSTAB_EPOCH_OVERLAP": "1", "VSTAB_PREFETCH": "16"})


def dev(img, cuda):
    import torch
    return torch.from_numpy(np.ascontiguousarray(img)).to(cuda)


def run(vs, cuda, frames, sync=False, **cfg):
    """test_pipeline_gpu.run_product; sync: a device synchronise behind every pull, so that the next pull finds every frame read ahead
    ingested and every detection enqueued finished"""
    import torch
    stab = vs.Stabilizer([dev(f, cuda) for f in frames], total=len(frames), **cfg)
    outs = []
    while True:
        o = stab.pull()
        if o is None:
            break
        outs.append(o.cpu().numpy())
        if sync:
            torch.cuda.synchronize()
    return stab, outs


def check_against(stab, outs, K, w, h, expected, what):
    """decisions, counts, inliers, rotations and every emitted frame against the state machine's answer"""
    import expect
    sm, exp, counts, warp_rots = expected
    log = stab.frame_log()
    assert len(outs) == len(log) == len(exp) == len(counts), what
    Ko, (cw, ch) = oracle.get_output_camera(K, w, h)
    assert stab.out_size == (cw, ch), what
    assert [l["key"] for l in log] == [bool(l["key"]) for l in sm.log], what
    assert [(l["n_corners"], l["n_tracked"]) for l in log] == counts, what
    assert [l["inliers"] for l in log] == [l["inliers"] for l in sm.log], what
    assert all(np.allclose(a["R"], b["R"], atol=1e-9) for a, b in zip(log, sm.log)), what
    for i in range(len(outs)):
        assert np.allclose(stab.warp_rotation(i), warp_rots[i], atol=1e-9), (what, i)
        p = oracle.map_params(K, Ko, stab.warp_rotation(i))
        assert np.array_equal(outs[i], expect.warp(exp[i], p, cw, ch)), (what, i)
    return log


def check_counters(stab, log, env, what):
    """what holds of the launch bookkeeping by construction, however the launches fell"""
    c = stab.tracker_counters()
    print(what, env, c, "epochs_in_turn", stab.profile()["epochs_in_turn"])
    tracked = sum(1 for l in log if l["n_corners"] > 0)
    assert tracked == len(log), what                                                     # (test_lk_pipeline_cpu.py: every frame has corners)
    assert c["seg_frames_launched"] - c["seg_frames_dropped"] >= tracked, (what, env, c)
    assert c["segs_launched"] <= c["seg_frames_launched"] and c["chained_adopted"] + c["chained_discarded"] <= tracked, (what, env, c)
    assert c["key_prelaunched"] <= sum(l["key"] for l in log), (what, env, c)
    if env.get("VSTAB_CHAIN_LK") == "0":                                                 # no launches ahead: one launch of one frame per frame
        assert c["chained_adopted"] == 0 and c["chained_discarded"] == 0 and c["seg_frames_dropped"] == 0 and c["key_prelaunched"] == 0, (what, c)
        assert c["segs_launched"] == c["seg_frames_launched"] == tracked, (what, c)
    if env.get("VSTAB_LK_SEGMENT") == "1":
        assert c["segs_launched"] == c["seg_frames_launched"], (what, c)
    if env.get("VSTAB_EPOCH_OVERLAP") == "0":
        assert stab.profile()["epochs_in_turn"] == 0, what
    return c


_solo = {}


def solo(vs, cuda, setting, clip="checker"):
    """(frame log keys, emitted frames) of a handle under SETTINGS[setting] alone over a key-frame clip, run once per module"""
    if (clip, setting) not in _solo:
        (w, h), K, frames = P.key_clip(clip)
        stab, outs = run(vs, cuda, frames, smooth_radius=P.R_SMOOTH, seed=P.SEED, **P.handle_cfg(*P.SETTINGS[setting]))
        _solo[clip, setting] = ([LOG_KEY(l) for l in stab.frame_log()], outs)
        stab.close()
    return _solo[clip, setting]


# ---- the key-frame clip -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", list(P.SETTINGS))
@pytest.mark.parametrize("clip", list(P.KEY_CLIPS))
def test_key_frame_clip_against_the_state_machine(vs, cuda, monkeypatch, clip, setting):
    """the counter's key frame at frame 21 and the count's key frames around the fade, under every tracker setting: against the state
    machine, and the same log and the same frames with one frame per launch, with no launches ahead, with short segments, with everything
    on one stream, and with epochs in turn under the deepest read-ahead.  On the checkerboard the planned key frame detects on demand
    (its candidates are over Detector::SPEC_CAP); on the banded clip its corners can come from the speculative detection."""
    (w, h), K, frames = P.key_clip(clip)
    cfg = dict(smooth_radius=P.R_SMOOTH, seed=P.SEED, **P.handle_cfg(*P.SETTINGS[setting]))
    stab, outs = run(vs, cuda, frames, **cfg)
    log = check_against(stab, outs, K, w, h, P.key_clip_expected(setting, clip), (clip, setting))
    keys = [l["key"] for l in log]
    plan = P.planned(keys)
    assert keys[20] and plan[20] and not any(keys[:20]), keys
    assert clip != "checker" or any(keys[i] and not plan[i] for i in range(27, 34)), keys
    check_counters(stab, log, {}, (clip, setting))
    ref = [LOG_KEY(l) for l in log]
    _solo.setdefault((clip, setting), (ref, outs))
    for env in ENVS:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        stab2, outs2 = run(vs, cuda, frames, **cfg)
        for k in env:
            monkeypatch.delenv(k)
        log2 = stab2.frame_log()
        assert [LOG_KEY(l) for l in log2] == ref, (clip, setting, env)
        assert len(outs2) == len(outs) and all(np.array_equal(a, b) for a, b in zip(outs2, outs)), (clip, setting, env)
        assert all(np.array_equal(stab2.warp_rotation(i), stab.warp_rotation(i)) for i in range(len(outs))), (clip, setting, env)
        check_counters(stab2, log2, env, (clip, setting))
        stab2.close()


@pytest.mark.parametrize("env", [{}, {"VSTAB_EPOCH_OVERLAP": "1", "VSTAB_PREFETCH": "16"}, {"VSTAB_EPOCH_OVERLAP": "0"}], ids=["default", "overlap_1_prefetch_16", "overlap_0"])
@pytest.mark.parametrize("setting", list(P.SETTINGS))
@pytest.mark.parametrize("clip", list(P.KEY_CLIPS))
def test_launches_ahead_are_reached_on_purpose(vs, cuda, monkeypatch, clip, setting, env):
    """A device synchronise behind every pull forces the launches ahead; nothing here depends on how fast anything runs.

    track_frame takes `reach` from hipEventQuery of the `ingested` events of the frames read ahead.  Those events were enqueued by earlier
    pulls (the read-ahead is refilled at the end of a pull), so behind a device synchronise every one of them has completed and `reach`
    is the whole read-ahead.  Then (1) a launch covers the frames ahead of the host's whenever there are any (a short segment is
    enqueued when nothing lies beyond the host's frame), so a frame whose predecessor left fewer than 150 survivors -- a key frame nobody
    planned -- finds itself inside a launch that tracked it as an ordinary frame: chained_discarded and seg_frames_dropped count it,
    wherever the state machine has such a key frame (on the checkerboard under every setting; on the banded clip under all but window
    31 alone).  (2) The speculative detection of frame 20 is enqueued when frame 20 is read ahead, eleven pulls before the host gets to
    frame 21, and its event has completed behind the synchronise: Detector::spec_poll_inline selects on the caller's thread unless the
    helper thread has taken the selection, and the chain loop asks again on every pull until the corners are there -- the key segment
    is launched from them, and frame 21 adopts it: key_prelaunched; with epochs in turn that segment goes to the second epoch stream:
    epochs_in_turn.  That is the banded clip.  On the checkerboard the selection finds more candidates than Detector::SPEC_CAP and gives
    up, the chain stops in front of frame 21 and the key frame detects on demand: key_prelaunched and epochs_in_turn are 0 there by
    construction, which is asserted too.

    NOT forced: who selects (caller or helper thread).  A helper thread that took the selection and then was not scheduled for the ten
    pulls that follow would leave key_prelaunched at 0; the selection is host work of microseconds, and nothing here waits for a clock.
    The log and the frames are the state machine's, as in every run."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    (w, h), K, frames = P.key_clip(clip)
    expected = P.key_clip_expected(setting, clip)
    stab, outs = run(vs, cuda, frames, sync=True, smooth_radius=P.R_SMOOTH, seed=P.SEED, **P.handle_cfg(*P.SETTINGS[setting]))
    log = check_against(stab, outs, K, w, h, expected, (clip, setting, env))
    c = check_counters(stab, log, env, (clip, setting, "synchronised"))
    print(stab.detector_counters(), stab.profile()["corner_selections_by_caller"], stab.profile()["corner_selections_by_helper"])
    keys = [bool(l["key"]) for l in expected[0].log]
    plan = P.planned(keys)
    if clip == "banded":
        assert c["key_prelaunched"] >= 1, c                   # the planned key frame adopted the segment launched from the speculated corners
        if env.get("VSTAB_EPOCH_OVERLAP") != "0":             # (a small frame: epochs in turn is the default)
            assert stab.profile()["epochs_in_turn"] >= 1, stab.profile()
    else:
        assert c["key_prelaunched"] == 0 and stab.profile()["epochs_in_turn"] == 0, c
    if any(k and not p for k, p in zip(keys, plan)):          # the unplanned key frame dropped what was enqueued ahead
        assert c["chained_discarded"] >= 1 and c["seg_frames_dropped"] >= 1, c
    else:
        assert (clip, setting) == ("banded", "w31") and c["chained_discarded"] == 0, c
    assert c["chained_adopted"] >= 30 and c["segs_launched"] < c["seg_frames_launched"], c   # multi-pair segments, adopted frame by frame
    ref, ref_outs = solo(vs, cuda, setting, clip)
    assert [LOG_KEY(l) for l in log] == ref and all(np.array_equal(a, b) for a, b in zip(outs, ref_outs))


# ---- every pyramid depth, both ingest routes ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clip,win,opt,nl", P.DEPTH_CASES, ids=P.DEPTH_IDS)
def test_depth_clips_on_both_ingest_routes(vs, cuda, clip, win, opt, nl):
    """handles whose pyramids have 1, 2, 3 and 4 levels -- one level: no pyramid kernel takes the `ingested` event and the fused copy has no
    level 1 to write; 3 and 4 levels at window 15: deeper than Tracker::init allocated -- with frames copied into the ring (ring_hold = 0:
    k_pack_pyr where there is a level 1) and frames used in place, against the state machine; and the first tracked pair against the
    stateless vstab_pyr_lk_win.  On 160 x 80 and 100 x 60 every estimate falls back (a dozen corners at most), so there the counts and
    the inliers are what sees the tracker; on 400 x 160 (window 15 deeper than the default), 400 x 200 (window 31 shallower) and
    480 x 270 no estimate does, and the rotations carry the tracked positions."""
    (w, h), K, frames = P.depth_clip(clip)
    expected = P.depth_expected(clip, win, opt)
    cfg = dict(smooth_radius=P.R_SMOOTH, seed=P.SEED, **P.handle_cfg(win, opt))
    logs = []
    for route, kw in (("copied", dict(ring_hold=0)), ("in place", {})):
        stab, outs = run(vs, cuda, frames, **cfg, **kw)
        log = check_against(stab, outs, K, w, h, expected, (clip, win, opt, route))
        if clip in P.DEPTH_ESTIMATED:
            assert not any(l["fallback"] for l in log), (clip, win, route)
        logs.append([LOG_KEY(l) for l in log])
        stab.close()
    assert logs[0] == logs[1]
    # the stateless call on the first pair: the definition's bits, and the handle's counts
    corners = oracle.good_features(np.ascontiguousarray(frames[0][:h]))
    ml, mi, eps, me = P.DEFAULT_OPTIONS if opt is None else opt
    want = W.track(frames[0][:h], frames[1][:h], corners, win, max_level=ml, max_iter=mi, eps=eps, min_eig=me)
    assert want["nl"] == nl
    xy, st, _ = vs.pyr_lk_win(dev(frames[0][:h], cuda), dev(frames[1][:h], cuda), corners, win, max_level=ml, max_iter=mi, eps=eps, min_eig_threshold=me)
    assert np.array_equal(st, want["status"]) and np.array_equal(xy.view(np.uint32)[st > 0], want["xy"].view(np.uint32)[st > 0])
    assert logs[0][0][1:3] == (len(corners), int((st > 0).sum()))


# ---- a 10-bit handle ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", ["w15", "w21_options"])
def test_ten_bit_handle(vs, cuda, setting):
    """a pixel_depth 10 handle's tracker reads the luma narrowed to 8 bits: over the key-frame clip widened to 16 bits, random low bytes,
    its frame log is the 8-bit handle's on the truncated frames (test_pipeline_ten_bit_handle's pattern), key frames and all"""
    import torch
    (w, h), K, frames = P.key_clip()
    rng = np.random.default_rng(8)
    wide = [((f.astype(np.uint16) << 8) | rng.integers(0, 256, f.shape, dtype=np.uint16)) for f in frames]
    devw = [torch.from_numpy(x.view(np.int16)).to(cuda) for x in wide]
    ten = vs.Stabilizer(devw, total=len(frames), bit_depth=10, smooth_radius=P.R_SMOOTH, seed=P.SEED, pixel_depth=10, blend=vs.BLEND_EXACT,
                        **P.handle_cfg(*P.SETTINGS[setting]))
    cw, ch = ten.out_size
    oy = torch.empty((ch, cw), dtype=torch.int16, device=cuda)
    ouv = torch.empty(((ch + 1) // 2, 2 * ((cw + 1) // 2)), dtype=torch.int16, device=cuda)
    pulls = 0
    while ten.pull_p010_into(oy, ouv):
        pulls += 1
    ref, _ = solo(vs, cuda, setting)
    got = [LOG_KEY(l) for l in ten.frame_log()]
    assert pulls == len(frames) - 1 and got == ref
    keys = [k[0] for k in got]
    assert keys[20] and any(keys[27:34]) and ref != solo(vs, cuda, "w31")[0]
    check_counters(ten, ten.frame_log(), {}, (setting, "10 bit"))


# ---- two handles side by side ---------------------------------------------------------------------------------------------------------------
def test_two_handles_with_different_windows(vs, cuda):
    """a handle at window 15 and one at window 31 with the options, over the key-frame clip, pulled alternately: each gives the log and the
    bytes it gives alone (the window and the options are the handle's, not the process's)"""
    (w, h), K, frames = P.key_clip()
    names = ("w15", "w31_options")
    stabs = [vs.Stabilizer([dev(f, cuda) for f in frames], total=len(frames), smooth_radius=P.R_SMOOTH, seed=P.SEED, **P.handle_cfg(*P.SETTINGS[s])) for s in names]
    outs, done = [[], []], [False, False]
    while not all(done):
        for k, s in enumerate(stabs):
            if not done[k]:
                o = s.pull()
                done[k] = o is None
                if o is not None:
                    outs[k].append(o.cpu().numpy())
    for k, name in enumerate(names):
        ref, ref_outs = solo(vs, cuda, name)
        assert [LOG_KEY(l) for l in stabs[k].frame_log()] == ref, name
        assert len(outs[k]) == len(ref_outs) and all(np.array_equal(a, b) for a, b in zip(outs[k], ref_outs)), name
    assert solo(vs, cuda, names[0])[0] != solo(vs, cuda, names[1])[0]


# ---- tracker and detector options together --------------------------------------------------------------------------------------------------
def test_tracker_and_detector_options_together(vs, cuda):
    """mask_def.overlay_clip() on a handle with window 31 and the options beside block 7, gradient 7, the Harris response and the mask:
    against the state machine with find = corner_def.good_features and track = lk_def.track.  (Block 7 with the Harris response leaves
    about 48 corners outside the mask, so on this handle every frame is a key frame detected on demand; the planned key frame under a
    tracker setting is test_key_frame_clip_against_the_state_machine's.)"""
    K, frames, mask, expected = P.both_expected()
    b = P.BOTH
    stab, outs = run(vs, cuda, frames, smooth_radius=P.BOTH_R, seed=P.BOTH_SEED, corner_block=b["block"], corner_gradient=b["gradient"],
                     corner_response=vs.CORNER_HARRIS, harris_k=b["k"], detection_mask=dev(mask, cuda), **P.handle_cfg(b["win"], b["opt"]))
    log = check_against(stab, outs, K, 640, 360, expected, "tracker and detector options")
    assert not any(l["fallback"] for l in log)
