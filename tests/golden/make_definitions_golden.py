"""Generates tests/golden/definitions_kat.npz, recorded answers of the numpy definitions themselves (tests/corner_def.py, tests/lk_def.py):
python tests/golden/make_definitions_golden.py

The committed file was produced at commit 7328d61 ("Corner gradient size"), the last one at which the detector was defined in four layers
(mask_def, harris_def, corner_block_def, corner_gradient_def) and the tracker twice (lk_options_def, lk_window_def).  There the tests held
those layers against each other; the answers here are what the OLDER layer of each pair gave on the inputs of those tests -- harris_def and
mask_def for block 3, corner_block_def for gradient 3, lk_options_def for window 21 (lk_window_def for 15 and 31), lk_segments' fetch-ahead
model for window 21 -- computed by this file's cases() through a thin adapter with corner_def's and lk_def's signatures.  Run through the
single definitions there are now it must reproduce the file bit for bit (test_definitions_kat_cpu.py), and the tests that used to compare two
layers compare the one definition with the file.

  products_<frame>_B<B>_<p>      the product planes dx dx, dx dy, dy dy (gradient 3): frames of test_corner_gradient_cpu.py
  response_B<B>_<k>              min_eig, harris (k = 0.06) and corners of luma_322x182 at gradient 3
  block3_<frame>_<k>             the sums a, b, c, harris (k = 0.06), corners_harris and corners_masked (mask_def.overlay_box) at block 3, gradient 3
  track_<case>_<k>               xy, status, err, min_eig, iterations, levels, nl, resid_restaged of track()
  fetch_neigh, fetch_top         lk_segments.fetch_ahead over jump_640 at window 21, as indices into lk_segments.CATS (-1: None)

Frames larger than the stated crops are cut to their top-left corner before the definition runs (CROPS): the planes of the full frames would
make a file of several MiB.  A definition in numpy can go wrong at a border (every crop has its own four), in an interior, and at an axis
shorter than the reach of the reflection ("3x3", "4x5": kept whole); the tile geometry of the kernels plays no part in it.

Fixtures are data only: expected outputs.  Their purpose is that an edit of a definition shows.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import corner_def as D  # noqa: E402
import lk_def as L  # noqa: E402
import lk_edges as E  # noqa: E402
import lk_segments as S  # noqa: E402
import mask_def as M  # noqa: E402

CROPS = {"products": (20, 13), "response": (66, 33), "block3": (40, 24)}       # (w, h)
PLANES = ("dxdx", "dxdy", "dydy")
MEASURED = ("luma_322x182", "tile_257", "cut_66x33", "ramp_2", "stripes_diagonal", "timing")
TRACK_KEYS = ("xy", "status", "err", "min_eig", "iterations", "levels", "nl", "resid_restaged")
PARAMS = (50, 0.01, 3.0)                                                       # max_corners, quality, min_distance: the crops are small
EDGE_OPTIONS = dict(max_level=1, max_iter=4, eps=0.05, min_eig=1e-3)


def crop(g, what):
    w, h = CROPS[what]
    return np.ascontiguousarray(g[:h, :w])


def product_frames():
    """name -> frame: every dense frame of both block sizes' GPU tests and three named frames, cut to CROPS["products"]"""
    out = {f"dense{b}_{name}": g for b in (5, 7) for name, g in D.dense_frames(b).items()}
    out.update({n: D.frame(n) for n in ("luma_322x182", "cut_66x33", "timing")})
    return {name: crop(g, "products") for name, g in out.items()}


def detector_answers():
    out = {}
    for block in D.BLOCKS:
        for name, g in product_frames().items():
            for p, v in zip(PLANES, D.products(g, block, 3)):
                out[f"products_{name}_B{block}_{p}"] = v
        g = crop(D.frame("luma_322x182"), "response")
        out[f"response_B{block}_min_eig"] = D.min_eig(g, block, 3)
        out[f"response_B{block}_harris"] = D.corner_harris(g, block, 3, 0.06)
        out[f"response_B{block}_corners"] = D.good_features(g, None, *PARAMS, block=block, gradient=3)
    for name in MEASURED:
        g = crop(D.frame(name), "block3")
        for p, v in zip("abc", D.covariance_sums(g)):
            out[f"block3_{name}_{p}"] = v
        out[f"block3_{name}_harris"] = D.corner_harris(g, k=0.06)
        out[f"block3_{name}_corners_harris"] = D.good_features(g, None, *PARAMS, harris=True)
        out[f"block3_{name}_corners_masked"] = D.good_features(g, M.overlay_box(*g.shape), *PARAMS)
    return out


def edge_case(size):
    """(prev, next, pts) of a frame size of lk_edges.SIZES: its boundary cases and special points"""
    w, h = size
    f = E.frames(w, h, 2)
    return f[0], f[1], np.concatenate([E.boundary_cases(w, h)[0], E.special_points(w, h)[0]])


def tracker_cases():
    """name -> (prev, next, pts, window, options)"""
    out = {}
    for size in E.SIZES:
        prev, nxt, pts = edge_case(size)
        out["edge_" + E.size_id(size)] = (prev, nxt, pts, 21, {})
        out["edge_" + E.size_id(size) + "_options"] = (prev, nxt, pts, 21, dict(EDGE_OPTIONS, guess=pts + np.float32(0.75)))
    frames, pts, _ = S.make_set("jump_640", n=120)
    out["jump"] = (frames[3], frames[4], pts, 21, {})
    out["jump_one_iteration"] = (frames[3], frames[4], pts, 21, dict(max_iter=1))
    for win in L.WINDOWS:
        out["moved_w%d" % win] = (*L.moved_pair(360, 200), L.grid(360, 200), win, {})
    return out


def stored(k, v):
    """what the file holds of track()'s field k: iteration counts (at most 100) as bytes"""
    return np.asarray(v).astype(np.uint8) if k == "iterations" else np.asarray(v)


def fetch_case():
    frames, pts, _ = S.make_set("jump_640", n=60)
    return S.expected(frames, pts, [8])


def fetch_codes(cats):
    return np.vectorize(lambda c: -1 if c is None else S.CATS.index(c), otypes=[np.int8])(cats)


def tracker_answers():
    out = {}
    for name, (prev, nxt, pts, win, opt) in tracker_cases().items():
        r = L.track(prev, nxt, pts, win, **opt)
        assert set(r) == set(TRACK_KEYS)
        for k in TRACK_KEYS:
            out[f"track_{name}_{k}"] = stored(k, r[k])
    neigh, top = S.fetch_ahead(fetch_case(), 640, 360)
    out["fetch_neigh"], out["fetch_top"] = fetch_codes(neigh), fetch_codes(top)
    return out


def load():
    return np.load(os.path.join(HERE, "definitions_kat.npz"))


def main():
    out = {**detector_answers(), **tracker_answers()}
    path = os.path.join(HERE, "definitions_kat.npz")
    np.savez_compressed(path, **out)
    print("wrote definitions_kat.npz:", len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
