"""Generates tests/golden/lk_options_kat.npz, the known-answer vectors of the tracker's options (tests/lk_def.py at window 21; include/vstab.h
"Tracker options"): python tests/golden/make_lk_options_golden.py

The frames are lk_edges.frames(130, 80) (two levels) and lk_def.moved_pair(240, 144) (three levels, a 9-pixel motion); the points a
few dozen of lk_def.points.  Per case <name>:

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
import lk_def as D  # noqa: E402

KEYS = ("xy", "status", "err", "min_eig", "iterations")


def cases():
    """name -> (prev, next, pts, options, guess)"""
    out = {}
    a = D.pair(130, 80)
    pa = D.points(130, 80)[::3]
    b = D.moved_pair(240, 144)
    pb = D.points(240, 144)[::3]
    rng = np.random.default_rng(20261020)
    out["default_130"] = (*a, pa, {}, None)
    out["combined_130"] = (*a, pa, dict(max_level=0, max_iter=4, eps=0.1, min_eig=2e-3), None)
    out["guess_130"] = (*a, pa, dict(max_iter=6), (pa + np.float32([1.3, -0.7]) + rng.uniform(-3, 3, pa.shape)).astype(np.float32))
    out["default_240"] = (*b, pb, {}, None)
    out["max_level_1_240"] = (*b, pb, dict(max_level=1), None)
    out["iter_eps_240"] = (*b, pb, dict(max_iter=3, eps=0.3, min_eig=1e-3), None)
    return out


def main():
    out = {}
    for name, (prev, nxt, pts, opt, guess) in cases().items():
        r = D.track(prev, nxt, pts, guess=guess, **opt)
        out[name + "_pts"] = pts
        if guess is not None:
            out[name + "_guess"] = guess
        for k in KEYS:
            out[f"{name}_{k}"] = r[k].astype(np.int32) if k == "iterations" else r[k]
    path = os.path.join(HERE, "lk_options_kat.npz")
    np.savez_compressed(path, **out)
    print("wrote lk_options_kat.npz:", len(cases()), "cases,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
