"""What the fixtures of test_lk_pipeline_gpu.py reach (tests/lk_pipeline.py), asserted against the definitions alone: per tracker setting
the key-frame clip has the counter's key frame and a key frame nobody planned; the depth clips have the level counts they are chosen for and
a tracker that runs on every frame; the clip of the tracker and detector options together tracks on every frame.  And the refusals of the
vstabx_tracker_counters hook that need no device.  No GPU."""
import ctypes
import importlib

import numpy as np
import pytest

import lk_def as W
import lk_pipeline as P

vs = importlib.import_module("video-annotator_amd")


def test_settings_are_the_ones_asked_for():
    assert P.SETTINGS["w15"] == (15, None) and P.SETTINGS["w31"] == (31, None) and P.SETTINGS["w21_options"] == (21, P.PIPE_OPTIONS)
    win, opt = P.SETTINGS["w31_options"]
    assert win in W.NEW_WINDOWS and opt == P.PIPE_OPTIONS == (2, 8, 0.03, 1e-3) and len(P.SETTINGS) == 4
    assert P.handle_cfg(21, None) == {} and P.handle_cfg(31, P.PIPE_OPTIONS) == dict(tracker_window=31, tracker_options=P.PIPE_OPTIONS)


def test_key_clip_is_the_faded_checkerboard():
    (w, h), K, frames = P.key_clip()
    assert (w, h) == (480, 270) and len(frames) == 50 and all(f.shape == (405, 480) for f in frames)
    plain = [k for k in range(50) if set(np.unique(frames[k][:h])) == {50, 150}]
    assert plain == [k for k in range(50) if not 27 <= k <= 30]
    for k in range(27, 31):                                   # 96 + floor((Y - 96) / 12): 50 -> 92, 150 -> 100
        assert set(np.unique(frames[k][:h])) == {92, 100} and np.array_equal(frames[k][h:], frames[0][h:])
        assert np.array_equal(frames[k][:h] == 100, frames[k % 2][:h] == 150)
    assert not np.array_equal(frames[0], frames[1]) and np.array_equal(frames[0], frames[2])
    # eight levels of contrast are under the tracker's default eigenvalue threshold for some windows, not for all: the count's key frames
    assert W.levels_of(w, h, 15) == W.levels_of(w, h, 31) == 4 and W.levels_of(w, h, 21, P.PIPE_OPTIONS[0]) == 3


def test_planned_marks_the_counters_key_frames():
    flags = [False] * 50
    for i in (20, 30, 31):
        flags[i] = True
    assert [i for i, p in enumerate(P.planned(flags)) if p] == [20]
    flags = [False] * 70
    for i in (20, 41, 50):                                    # frame 42 = 21 + 21: the counter's again
        flags[i] = True
    assert [i for i, p in enumerate(P.planned(flags)) if p] == [20, 41]
    assert P.planned([True, False]) == [False, False]


@pytest.mark.parametrize("setting", list(P.SETTINGS))
def test_key_clip_has_a_planned_and_an_unplanned_key_frame(setting):
    sm, exp, counts, _ = P.key_clip_expected(setting)
    keys = [bool(l["key"]) for l in sm.log]
    plan = P.planned(keys)
    assert len(keys) == len(counts) == len(exp) == 49
    assert counts[0][0] >= 150
    assert keys[20] and plan[20] and not any(keys[:20])                                   # the counter's key frame, and none before it
    unplanned = [i for i in range(27, 34) if keys[i] and not plan[i]]
    assert unplanned, (setting, [i for i, k in enumerate(keys) if k])
    # every frame has corners to track (a launch per frame), and the estimate behind an ordinary frame never falls back
    assert all(n > 0 and t > 0 for n, t in counts)
    assert all(l["inliers"] >= 40 for i, l in enumerate(sm.log) if i not in range(26, 32))
    print(setting, "key frames", [i for i, k in enumerate(keys) if k], "unplanned", unplanned, "fewest tracked", min(t for _, t in counts))


def test_which_key_clip_can_be_speculated():
    """the speculative selection of frame 20 (an even frame) gives up over Detector::SPEC_CAP candidates: the checkerboard is over it -- its
    planned key frame always detects on demand -- and the banded clip is under it"""
    import corner_tiles as C
    import oracle
    n = {}
    for name in P.KEY_CLIPS:
        (w, h), K, frames = P.key_clip(name)
        n[name] = len(oracle.good_features(np.ascontiguousarray(frames[20][:h]), 0, 0.01, 0.0))
    assert n["banded"] <= C.SPEC_CAP < n["checker"], n
    (w, h), K, frames = P.key_clip("banded")
    assert (w, h) == (640, 360) and len(frames) == 50 and [W.levels_of(w, h, x) for x in W.WINDOWS] == [4, 4, 4]
    assert all(np.array_equal(frames[k], P.faded(frames[k % 2], h)) == (27 <= k <= 30) for k in range(50))


@pytest.mark.parametrize("setting", list(P.SETTINGS))
def test_banded_key_clip_has_the_planned_key_frame(setting):
    """200 corners, the counter's key frame at frame 21 and none before it; what follows the fade differs by setting (at window 31 nothing
    but the counter's next key frame; with the options a frame on which every corner is lost) and is printed"""
    sm, exp, counts, _ = P.key_clip_expected(setting, "banded")
    keys = [bool(l["key"]) for l in sm.log]
    plan = P.planned(keys)
    assert len(keys) == len(counts) == 49 and counts[0] == (200, 200)
    assert keys[20] and plan[20] and not any(keys[:20]) and all(n >= 150 for n, _ in counts)
    assert all(l["inliers"] >= 40 for l in sm.log[:26])
    print(setting, "key frames", [i for i, k in enumerate(keys) if k], "planned", [i for i, p in enumerate(plan) if p], "fewest tracked", min(t for _, t in counts))


def test_key_clip_settings_differ():
    """the four logs are four different logs: a handle that forgot its window or its options on some path answers another setting's"""
    logs = {s: [(l["key"], c, l["inliers"], l["R"].tobytes()) for l, c in zip(P.key_clip_expected(s)[0].log, P.key_clip_expected(s)[2])] for s in P.SETTINGS}
    names = list(logs)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            assert logs[a] != logs[b], (a, b)
            assert logs[a][:20] != logs[b][:20], (a, b)       # before the first planned key frame already


@pytest.mark.parametrize("clip,win,opt,nl", P.DEPTH_CASES, ids=P.DEPTH_IDS)
def test_depth_clips(clip, win, opt, nl):
    (w, h), K, frames = P.depth_clip(clip)
    assert len(frames) == P.DEPTH_FRAMES and frames[0].shape == (h * 3 // 2, w) and w % 2 == 0 and h % 2 == 0
    assert W.levels_of(w, h, win, 3 if opt is None else opt[0]) == nl
    sm, exp, counts, _ = P.depth_expected(clip, win, opt)
    assert len(counts) == P.DEPTH_FRAMES - 1 and all(n > 0 and t > 0 for n, t in counts), counts
    if clip in P.DEPTH_ESTIMATED:
        assert all(l["inliers"] >= 40 for l in sm.log), [l["inliers"] for l in sm.log]
    first = W.track(frames[0][:h], frames[1][:h], sm_corners(frames[0][:h]), win, **track_kw(opt))
    assert first["nl"] == nl and (len(first["xy"]), int(first["status"].sum())) == counts[0]


def sm_corners(gray):
    import oracle
    return oracle.good_features(np.ascontiguousarray(gray))


def track_kw(opt):
    ml, mi, eps, me = P.DEFAULT_OPTIONS if opt is None else opt
    return dict(max_level=ml, max_iter=mi, eps=eps, min_eig=me)


def test_depth_level_counts():
    """160 x 80: 3 / 2 / 2 levels at 15 / 21 / 31, and 400 x 160: 4 / 3 / 3 -- the window 15 asks for more than Tracker::init allocated;
    100 x 60: 2 / 2 / 1 -- one level at 31 -- and 400 x 200: 4 / 4 / 3 -- the window 31 asks for fewer; and the options' max_level 0 and 1
    at 480 x 270, where every window has four"""
    got = {}
    for clip, win, opt, nl in P.DEPTH_CASES:
        got.setdefault(clip, []).append(nl)
    assert got == {"160x80": [3, 2, 2], "100x60": [2, 2, 1], "400x160": [4, 3, 3], "400x200": [4, 4, 3], "480x270": [1, 2]}
    assert [W.level_sizes(160, 80, x)[0] for x in W.WINDOWS] == [3, 2, 2] and [W.level_sizes(100, 60, x)[0] for x in W.WINDOWS] == [2, 2, 1]
    assert [W.level_sizes(480, 270, x)[0] for x in W.WINDOWS] == [4, 4, 4]
    # the estimated clip sees the window: the three windows give three logs
    for clip in ("400x160", "400x200"):
        logs = [[(c, l["inliers"], l["R"].tobytes()) for l, c in zip(P.depth_expected(clip, x, None)[0].log, P.depth_expected(clip, x, None)[2])] for x in W.WINDOWS]
        assert logs[0] != logs[1] != logs[2] != logs[0], clip
    a, b = (P.depth_expected("480x270", 21, o)[0].log for _, _, o, _ in P.DEPTH_CASES[-2:])
    assert [l["R"].tobytes() for l in a] != [l["R"].tobytes() for l in b]


def test_tracker_and_detector_options_together():
    """mask_def.overlay_clip() under window 31 and the options beside block 7, gradient 7, Harris and the mask: the tracker runs on every
    frame, no corner lies under the mask, and the log is neither the tracker setting's nor the detector setting's alone.  (About 48 corners
    survive block 7 with the Harris response under the mask: every frame of this clip is a key frame detected on demand.)"""
    import corner_def as D
    K, frames, mask, (sm, exp, counts, _) = P.both_expected()
    assert len(frames) == 40 and len(counts) == 39 and all(n > 0 and t > 0 for n, t in counts)
    assert all(l["inliers"] >= 40 for l in sm.log)
    first = D.good_features(frames[0][:360], mask, block=7, gradient=7, harris=True)
    assert len(first) == counts[0][0] and (mask[np.rint(first[:, 1]).astype(int), np.rint(first[:, 0]).astype(int)] != 0).all()
    find = lambda g: D.good_features(g, mask, block=7, gradient=7, harris=True)
    key = lambda run: [(c, l["inliers"], l["R"].tobytes()) for l, c in zip(run[0].log, run[2])]
    detector_only = P.run_state_machine(frames[:6], K, 640, 360, P.BOTH_R, P.BOTH_SEED, 21, None, find)
    tracker_only = P.run_state_machine(frames[:6], K, 640, 360, P.BOTH_R, P.BOTH_SEED, 31, P.PIPE_OPTIONS)
    both = key((sm, exp, counts))[:5]
    assert both != key(detector_only) and both != key(tracker_only)
    print("keys", sum(bool(l["key"]) for l in sm.log), "of", len(sm.log), "corners", min(n for n, _ in counts), "..", max(n for n, _ in counts))


def test_tracker_counters_hook_refuses_null():
    L = vs.lib
    assert L.vstabx_tracker_counters(None, (ctypes.c_long * 6)()) == vs.ERR_INVALID
    assert L.vstab_last_error().decode() == "vstabx_tracker_counters: bad argument"
    assert L.vstabx_tracker_counters(4096, None) == vs.ERR_INVALID
    assert callable(vs.Stabilizer.tracker_counters)
