"""Clips, settings and the state machine of the handle tests of the tracker's window and options (include/vstab.h, "Tracker window" and
"Tracker options"; DESIGN.md sections 29 and 34): what a handle with vstab_set_tracker_window / vstab_set_tracker_options has to do across
planned and unplanned key frames and at every pyramid depth.  The definitions are lk_def.track and corner_def.good_features, plugged into
oracle.WarpStateMachine.  No GPU here; test_lk_pipeline_cpu.py asserts what the fixtures reach.  A plain module, imported by the tests."""
import functools

import numpy as np

import corner_def
import corner_tiles as C
import lk_def as W
import mask_def as M
import oracle
import synth

PIPE_OPTIONS = (2, 8, 0.03, 1e-3)             # (max_level, max_iter, eps, min_eig) of test_lk_options_gpu.py
DEFAULT_OPTIONS = (3, 30, 0.01, 1e-4)
# name -> (window, options or None): the two new windows alone, the options under the default window, and one window with the options
SETTINGS = {"w15": (15, None), "w31": (31, None), "w21_options": (21, PIPE_OPTIONS), "w31_options": (31, PIPE_OPTIONS)}
R_SMOOTH, SEED = 2, 1


def handle_cfg(win, opt):
    """the Stabilizer arguments of a setting"""
    cfg = {}
    if win != 21:
        cfg["tracker_window"] = win
    if opt is not None:
        cfg["tracker_options"] = opt
    return cfg


# ---- the key-frame clip -------------------------------------------------------------------------------------------------------------------
KEY_FRAMES, FADE = 50, (27, 31)               # frames FADE[0] .. FADE[1] - 1 are faded


def faded(frame, h):
    """the frame with its luma at a twelfth of its contrast around 96 (test_unplanned_key_frames_... in test_pipeline_gpu.py)"""
    g = frame.copy()
    g[:h] = (96 + np.floor_divide(g[:h].astype(np.int32) - 96, 12)).astype(np.uint8)
    return g


# "checker": the 480 x 270 checkerboard, 171 corners.  Its candidates are more than Detector::SPEC_CAP, so the speculative selection of frame
# 20 gives up and the planned key frame detects on demand: no launch from speculated corners on this clip, whatever the timing.
# "banded": the 640 x 360 bands, 200 corners, 21,010 candidates -- under SPEC_CAP: the planned key frame's tracker can be launched from the
# speculated corners before the host gets there.
KEY_CLIPS = {"checker": "middle", "banded": "under_spec_cap"}


@functools.lru_cache(maxsize=None)
def key_clip(name="checker"):
    """((w, h), K, frames): corner_tiles.pipeline_clip(KEY_CLIPS[name]) -- moved by a pixel on every odd frame -- over 50 frames, frames
    27 .. 30 faded: the counter's key frame at frame 21, and the count's key frames into the fade or out of it"""
    (w, h), two = C.pipeline_clip(KEY_CLIPS[name])
    frames = [two[k % 2] for k in range(KEY_FRAMES)]
    for k in range(*FADE):
        frames[k] = faded(frames[k], h)
    return (w, h), oracle.get_preset_camera(4, w, h), frames


def planned(keys):
    """per log index: whether the counter half of the key-frame rule (frame - last key > 20) made that frame a key frame.  keys: the key
    flags of a frame log (log index i is frame i + 1; a key frame detects on the frame before it)"""
    last, out = 0, []
    for i, key in enumerate(keys):
        f = i + 1
        out.append(bool(key) and f - last > 20)
        if key:
            last = f - 1
    return out


# ---- the depth clips ------------------------------------------------------------------------------------------------------------------------
DEPTH_FRAMES = 8
# (clip, window, options, levels of the handle's pyramid).  160 x 80 is deeper at 15 (3 levels) than at 21 (2), which init() allocated for;
# 100 x 60 has ONE level at 31; max_level 0 and 1 give the one- and two-level handle at an ordinary size.  The two small frames hold a
# handful of corners 30 px apart (and the preset's lens leaves no room for a frame that low and three times as wide), so every estimate
# there falls back to the identity -- fewer than 40 inliers -- and only the counts see the tracker.  400 x 160 is the smallest frame with 40
# inliers and more on every frame on which the window 15 still asks for a level more (4) than init() allocated (3), and 400 x 200 one on
# which the window 31 has a level fewer (3) than the default's 4: there, and on the max_level handles, the rotations carry the tracked
# positions.  (A tracker that keeps the default window's depth under set_window passes the two small clips and fails these two.)
DEPTH_CASES = [(clip, win, None, nl) for clip, levels in (("160x80", (3, 2, 2)), ("100x60", (2, 2, 1)), ("400x160", (4, 3, 3)), ("400x200", (4, 4, 3)))
               for win, nl in zip(W.WINDOWS, levels)] + [("480x270", 21, (0, 30, 0.01, 1e-4), 1), ("480x270", 21, (1, 30, 0.01, 1e-4), 2)]
DEPTH_IDS = ["%s-w%d%s" % (c, w, "" if o is None else "-max_level_%d" % o[0]) for c, w, o, _ in DEPTH_CASES]
DEPTH_ESTIMATED = ("400x160", "400x200", "480x270")      # the clips whose estimates never fall back


@functools.lru_cache(maxsize=None)
def depth_clip(name):
    """((w, h), K, frames), DEPTH_FRAMES textured, moving frames: of the small sizes a window of synth.luma that moves by (1.3, -0.7) a
    frame under the frame, grey chroma; of the others synth.shaky_clip"""
    w, h = (int(v) for v in name.split("x"))
    K = oracle.get_preset_camera(4, w, h)
    if name in DEPTH_ESTIMATED:
        return (w, h), K, synth.shaky_clip(w + h, K, w, h, DEPTH_FRAMES, sigma=0.004)[0]
    base = synth.luma(w * 7 + h, w + 48, h + 48, rects=max(12, w * h // 1500))
    frames = [C.nv12_of(np.ascontiguousarray(synth.shifted(base, 1.3 * k, -0.7 * k)[24:24 + h, 24:24 + w])) for k in range(DEPTH_FRAMES)]
    return (w, h), K, frames


# ---- the state machine ----------------------------------------------------------------------------------------------------------------------
def run_state_machine(frames, K, w, h, r, seed, win=21, opt=None, find=None):
    """mask_def.run_state_machine with track = lk_def.track at window `win` and the options `opt`: (state machine, frames it emits,
    (n_corners, n_tracked) per frame, rotations handed to the warp).  find: the detector (default: oracle.good_features)"""
    Ko, _ = oracle.get_output_camera(K, w, h)
    rng = oracle.Pcg32(seed)
    counts, warp_rots = [], []
    ml, mi, eps, me = DEFAULT_OPTIONS if opt is None else opt
    find = find or (lambda g: oracle.good_features(np.ascontiguousarray(g)))

    def track(prev, cur, corners):
        if len(corners) == 0:
            counts.append((0, 0))
            return corners, corners
        res = W.track(prev, cur, corners, win, max_level=ml, max_iter=mi, eps=eps, min_eig=me)
        nxt, st = res["xy"], res["status"]
        counts.append((len(corners), int((st > 0).sum())))
        return corners[st > 0], nxt[st > 0]

    sm = oracle.WarpStateMachine(frames, r, find, track, lambda pp, cp: oracle.estimate_rotation(pp, cp, K, Ko, rng), lambda f, R: (warp_rots.append(R), f)[1])
    exp = []
    while True:
        o = sm.pull_frame()
        if o is None:
            break
        exp.append(o)
    return sm, exp, counts, warp_rots


@functools.lru_cache(maxsize=None)
def key_clip_expected(setting, clip="checker"):
    """the state machine over a key-frame clip under SETTINGS[setting] (or "default"), computed once per process and shared"""
    (w, h), K, frames = key_clip(clip)
    win, opt = SETTINGS.get(setting, (21, None))
    return run_state_machine(frames, K, w, h, R_SMOOTH, SEED, win, opt)


@functools.lru_cache(maxsize=None)
def depth_expected(clip, win, opt):
    (w, h), K, frames = depth_clip(clip)
    return run_state_machine(frames, K, w, h, R_SMOOTH, SEED, win, opt)


# ---- tracker and detector options together ------------------------------------------------------------------------------------------------
BOTH = dict(win=31, opt=PIPE_OPTIONS, block=7, gradient=7, harris=True, k=corner_def.K_DEFAULT)
BOTH_R, BOTH_SEED = 5, 5                      # test_pipeline_overlay_clip's


@functools.lru_cache(maxsize=None)
def both_expected():
    """(K, frames, mask, state machine's answer) of mask_def.overlay_clip() under BOTH: window 31 and the options beside block 7, gradient 7,
    the Harris response and the mask"""
    K, _, frames, _, mask = M.overlay_clip()
    find = lambda g: corner_def.good_features(g, mask, block=BOTH["block"], gradient=BOTH["gradient"], harris=True, k=BOTH["k"])
    return K, frames, mask, run_state_machine(frames, K, 640, 360, BOTH_R, BOTH_SEED, BOTH["win"], BOTH["opt"], find)
