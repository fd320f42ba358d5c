"""Generates tests/golden/lk_window_kat.npz, the known-answer vectors of the tracker's window (tests/lk_def.py; include/vstab.h
"Tracker window"): python tests/golden/make_lk_window_golden.py

The frames are lk_edges.frames(130, 80) (three levels at 15, two at 31), lk_def.moved_pair(240, 144) (a 9-pixel motion) and
lk_edges.frames(24, 20) (smaller than the 31-pixel window: several folds); the points a few dozen of lk_def.window_points.  Per case <name>:

  <name>_pts, <name>_guess   the start points and (initial-flow cases) the guesses
  <name>_xy, _status, _err, _min_eig, _iterations   what lk_def.track answers

Fixtures are data only: inputs and expected outputs.  Their purpose is that an edit of the definition shows.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import lk_def as W  # noqa: E402

KEYS = ("xy", "status", "err", "min_eig", "iterations")


def cases():
    """name -> (prev, next, pts, window, options, guess)"""
    out = {}
    a, b, c = W.pair(130, 80), W.moved_pair(240, 144), W.pair(24, 20)
    rng = np.random.default_rng(20261020)
    for win in W.NEW_WINDOWS:
        pa, pb = W.window_points(130, 80, win)[::3], W.window_points(240, 144, win)[::4]
        out["default_130_w%d" % win] = (*a, pa, win, {}, None)
        out["guess_130_w%d" % win] = (*a, pa, win, dict(max_iter=6), (pa + np.float32([1.3, -0.7]) + rng.uniform(-3, 3, pa.shape)).astype(np.float32))
        out["default_240_w%d" % win] = (*b, pb, win, {}, None)
        out["options_240_w%d" % win] = (*b, pb, win, dict(max_level=1, max_iter=5, eps=0.1, min_eig=1e-3), None)
    out["folds_24_w31"] = (*c, W.window_points(24, 20, 31)[::2], 31, {}, None)
    return out


def main():
    out = {}
    for name, (prev, nxt, pts, win, opt, guess) in cases().items():
        r = W.track(prev, nxt, pts, win, guess=guess, **opt)
        out[name + "_pts"] = pts
        if guess is not None:
            out[name + "_guess"] = guess
        for k in KEYS:
            out[f"{name}_{k}"] = r[k].astype(np.int32) if k == "iterations" else r[k]
    path = os.path.join(HERE, "lk_window_kat.npz")
    np.savez_compressed(path, **out)
    print("wrote lk_window_kat.npz:", len(cases()), "cases,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
