"""Waves of the fused warp kernels at the source edge (vstab_warp_fused.hip, edge_wave): the premise, against the oracle alone, and a
numpy restatement of the kernel's classification of a wave that the GPU tests (test_edge_waves_gpu.py) use to prove that a shape holds
the cases they are about.

The premise.  cv::remap with BORDER_CONSTANT 0 makes a pixel zero when its 2 x 2 footprint lies wholly outside the source -- not
(-1 <= X <= sw - 1 and -1 <= Y <= sh - 1), X, Y = floor(rint(32 * map) / 32) -- whatever the source holds: the kernel zeroes such pixels
without sampling them.  Checked here on the oracle's own map and warps: 8-bit BGR, NV12 out, 10-bit with both blends.

The classification of a wave (64 columns x RW rows of a 64 x 4 RW tile), as the kernel makes it:
    fast      every footprint lies in the tile's staged box
    outside   every footprint is wholly outside the source: zeros
    clamp     the box is staged and every footprint outside it is wholly outside the source: sampled with the others, then zeroed
    gather    a footprint that touches the source is not in the box: pixel by pixel
    dead      the tile is dead by the probe's rule (dead_tiles.rule): nothing is classified"""
import os
import re

import numpy as np
import pytest

import dead_tiles as D
import layouts
import oracle
import synth
from test_p010_cpu import p010_frame

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "video-annotator_amd", "csrc")
PRESET = oracle.GOPRO_H4B_WIDE169_MEASURED
FAST, OUTSIDE, CLAMP, GATHER, DEAD = range(5)
HUGE = 1 << 28      # where the map is no number (cv::remap: cvRound -> INT_MIN; the kernel: an integer >= 2^22 in magnitude)


def taps(mapx, mapy):
    """(X, Y) int64: the upper left tap of every pixel's footprint, floor(rint(32 * map) / 32)."""
    with np.errstate(invalid="ignore", over="ignore"):
        qx, qy = np.rint(32.0 * np.asarray(mapx, np.float64)), np.rint(32.0 * np.asarray(mapy, np.float64))
    bad = ~(np.isfinite(qx) & np.isfinite(qy)) | (np.abs(qx) >= 2.0 ** 22) | (np.abs(qy) >= 2.0 ** 22)
    X, Y = np.floor(np.where(bad, 0.0, qx) / 32.0).astype(np.int64), np.floor(np.where(bad, 0.0, qy) / 32.0).astype(np.int64)
    return np.where(bad, HUGE, X), np.where(bad, HUGE, Y)


def touches(X, Y, sw, sh):
    """One of the four taps is inside the source (the negation of gather_pixel_far's test)."""
    return (X >= -1) & (X <= sw - 1) & (Y >= -1) & (Y <= sh - 1)


def stage_trips(rwb, rw):
    return 3 if rw == 8 else 2 if rw == 4 else (2 if rwb == 8 else 1)


def classify(mapx, mapy, sw, sh, rwb, rw, lds_kb, src_vec_ok=True, dead=None, px=1):
    """Every wave of the 64 x 4 rw tiles of the kernel with tall tiles of 4 rwb rows -> dict of (tile rows, 4, tile columns) arrays:
    kind; n_out / n_in (pixels of the wave wholly outside / touching the source inside the box) and tile-level `staged`, `live`
    (a pixel of the tile touches the source).  dead: the rule's (tile rows, tile columns) verdict or None.  px: LDS dwords per pixel.
    Columns right of the image and rows below it count as the last column / row, as the kernel maps them."""
    dh, dw = mapx.shape
    th = 4 * rw
    rows, cols = -(-dh // th), -(-dw // 64)
    X, Y = taps(mapx, mapy)
    boxes = layouts.tile_boxes(mapx, mapy, sw, sh, th, planar=False, block_w=8)
    pad = ((0, rows * th - dh), (0, cols * 64 - dw))
    X, Y = np.pad(X, pad, mode="edge"), np.pad(Y, pad, mode="edge")
    cap = (lds_kb * 1024 // 4 - 8) // px
    shape = (rows, 4, cols)
    out = dict(kind=np.zeros(shape, np.int64), n_out=np.zeros(shape, np.int64), n_in=np.zeros(shape, np.int64),
               staged=np.zeros((rows, cols), bool), live=np.zeros((rows, cols), bool))
    for (tr, tc), (bx0, by0, wb, hb, have) in boxes.items():
        stageable = have and sw >= 8 and src_vec_ok and (sw % 8 == 0 or bx0 + wb <= (sw & ~7))
        fits = wb * hb <= cap and (wb // 8) * (hb // 2) <= stage_trips(rwb, rw) * 256
        use_lds = bool(stageable and fits)
        out["staged"][tr, tc] = use_lds
        tx, ty = X[tr * th:(tr + 1) * th, tc * 64:(tc + 1) * 64], Y[tr * th:(tr + 1) * th, tc * 64:(tc + 1) * 64]
        t = touches(tx, ty, sw, sh)
        out["live"][tr, tc] = t.any()
        inbox = use_lds & (tx - bx0 >= 0) & (tx - bx0 < wb - 1) & (ty - by0 >= 0) & (ty - by0 < hb - 1)
        for w in range(4):
            s = slice(w * rw, (w + 1) * rw)
            tw, iw = t[s], inbox[s]
            if dead is not None and dead[tr, tc]:
                k = DEAD
            elif iw.all():
                k = FAST
            elif not tw.any():
                k = OUTSIDE
            elif use_lds and not (tw & ~iw).any():
                k = CLAMP
            else:
                k = GATHER
            out["kind"][tr, w, tc] = k
            out["n_out"][tr, w, tc] = int((~tw).sum())
            out["n_in"][tr, w, tc] = int((tw & iw).sum())
    return out


def straddles(mapx, mapy, sw, sh, rw):
    """Which of the four edges and four corners of the source a footprint straddles (X = -1, X = sw - 1, Y = -1, Y = sh - 1 and their
    pairs) in a wave (64 x rw block of the output) that also holds a pixel wholly outside -> set of names."""
    dh, dw = mapx.shape
    X, Y = taps(mapx, mapy)
    t = touches(X, Y, sw, sh)
    L, R, T, B = t & (X == -1), t & (X == sw - 1), t & (Y == -1), t & (Y == sh - 1)
    inner_x, inner_y = (X >= 0) & (X < sw - 1), (Y >= 0) & (Y < sh - 1)
    named = dict(left=L & inner_y, right=R & inner_y, top=T & inner_x, bottom=B & inner_x, top_left=T & L, top_right=T & R, bottom_left=B & L,
                 bottom_right=B & R)
    found = set()
    for y0 in range(0, dh, rw):
        for x0 in range(0, dw, 64):
            s = (slice(y0, y0 + rw), slice(x0, x0 + 64))
            if t[s].all():
                continue
            found |= {k for k, m in named.items() if m[s].any()}
    return found


# ---- the premise ----------------------------------------------------------------------------------------------------------------------
def setup(w, h):
    K = oracle.get_preset_camera(PRESET, w, h)
    Ko, (cw, ch) = oracle.get_output_camera(K, w, h)
    return K, Ko, cw, ch


ROTATIONS = [(0.0, 0.0, 0.0), (0.02, 0.015, 0.01), (0.15, 0.0, 0.1), (0.3, 0.3, 0.3)]


@pytest.mark.parametrize("rv", ROTATIONS)
def test_footprints_wholly_outside_the_source_are_zero_8_bit(rv):
    """BGR and NV12 out: where the oracle's own map puts the footprint wholly outside, BGR is (0, 0, 0), luma what BGR zero converts to,
    and chroma -- taken from the even-row, even-column pixels -- the same."""
    w, h = 256, 144
    K, Ko, cw, ch = setup(w, h)
    f = synth.nv12(11, w, h)
    f[f == 0] = 1                                    # no zero in the source: a zero in the output is the border's
    p = oracle.map_params(K, Ko, oracle.rodrigues(rv))
    X, Y = taps(*oracle.create_map(p, cw, ch))
    far = ~touches(X, Y, w, h)
    assert far.any() and (~far).any()
    bgr = oracle.warp_nv12(f, p, cw, ch)
    assert not bgr[far].any()
    zy, zuv = oracle.cvt_bgr_nv12(np.zeros((2, 2, 3), np.uint8))
    y, uv = oracle.warp_nv12_ex(f, p, cw, ch, 0, 1)
    assert (y[far] == zy[0, 0]).all()
    assert (uv[far[::2, ::2]] == zuv[0, 0]).all()


@pytest.mark.parametrize("blend", [0, 1])
def test_footprints_wholly_outside_the_source_are_zero_10_bit(blend):
    w, h = 256, 144
    K, Ko, cw, ch = setup(w, h)
    y, uv, _, _ = p010_frame(5, w, h)
    for rv in ROTATIONS[1:3]:
        p = oracle.map_params(K, Ko, oracle.rodrigues(rv))
        X, Y = taps(*oracle.create_map(p, cw, ch))
        far = ~touches(X, Y, w, h)
        assert far.any() and (~far).any()
        out = oracle.warp_p010(y, uv, p, cw, ch, None, 0, blend)
        assert not out[far].any()
        zy, zuv = oracle.cvt_bgr10_p010(np.zeros((2, 2, 3), np.uint16))
        oy, ouv = oracle.cvt_bgr10_p010(out)
        assert (oy[far] == zy[0, 0]).all() and (ouv.reshape(-1, (cw + 1) // 2, 2)[far[::2, ::2]] == zuv.reshape(-1, 2)[0]).all()


# ---- the classification ---------------------------------------------------------------------------------------------------------------
def test_the_test_is_the_kernels():
    src = ""
    for name in ("vstab_warp_fused.hip", "vstab_warp_tile.hpp"):
        with open(os.path.join(CSRC, name)) as f:
            src += re.sub(r"\s+", " ", f.read())
    for line in ("const bool touches = (uint32_t)(Xr[j] + fx) < sx && (uint32_t)(Yr[j] + fy) < sy;", "int fx = bx0 + 1, fy = by0 + 1;",
                 "const uint32_t sx = (uint32_t)a.sw + 1u, sy = (uint32_t)a.sh + 1u;",
                 "const bool inbox = (uint32_t)Xr[j] < wlim && (uint32_t)Yr[j] < hlim;",
                 "if (!__builtin_amdgcn_ballot_w64(keep != 0)) return EDGE_OUTSIDE;",
                 "return PATHS == 2 && use_lds && !__builtin_amdgcn_ballot_w64(gather) ? EDGE_CLAMP : EDGE_GATHER;",
                 "static constexpr int value = RW == 8 ? 3 : RW == 4 ? 2 : (RWB == 8 ? 2 : 1);"):
        assert line in src, line


def test_headline_counts():
    """3840 x 2160 -> 3524 x 1999 in 64 x 32 tiles: about a seventh of the waves of the tiles the rule leaves alive hold a pixel wholly
    outside the source, and none of them has anything to gather -- every one is `outside` or `clamp`."""
    w, h = 3840, 2160
    K, Ko, cw, ch = setup(w, h)
    assert (cw, ch) == (3524, 1999)
    p = oracle.map_params(K, Ko, np.eye(3))
    mx, my = oracle.create_map(p, cw, ch)
    c = classify(mx, my, w, h, 8, 8, 40, dead=D.rule(p, cw, ch, w, h, 32))
    kind = c["kind"]
    counts = {n: int((kind == k).sum()) for n, k in (("fast", FAST), ("outside", OUTSIDE), ("clamp", CLAMP), ("gather", GATHER), ("dead", DEAD))}
    print(counts)
    edge = (kind != DEAD) & (kind != FAST)
    assert counts["gather"] == 0
    assert 1000 <= int(edge.sum()) <= 1700 and counts["clamp"] >= 500 and counts["outside"] >= 300
    assert ((c["n_out"] > 0) | ~edge).all()          # a wave leaves the fast path here only through a pixel wholly outside
