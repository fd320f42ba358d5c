"""The corner block size (include/vstab.h, "Corner block size") restated in numpy: OpenCV 4.5's cornerMinEigenVal(gray,
B, 3), cornerHarris(gray, B, 3, k) and goodFeaturesToTrack(gray, corners, max_corners, quality, min_distance, mask, B, useHarris, k) on its
CPU path for B = 3, 5, 7, and the one-pass detector of that block size restated per tile.  No GPU here.

    1  derivatives: the 3 x 3 Sobel pair of harris_def.covariance_sums with scale_B = (float)(1 / (4 B 255))
    2  products dx dx, dx dy, dy dy in binary32
    3  the B x B box sum over the product planes extended by REFLECT_101 (folding as often as it takes), in double and IN THIS ORDER: column
       sums top to bottom, then left to right, then one rounding to float
    4  the minimum-eigenvalue formula (harris_def.min_eig_from_sums) or the Harris formula (harris_def.response_from_sums)
    5  the detector's remaining steps are harris_def's and mask_def's, on this response: they are reused with the response plugged in

The order of step 3 is part of the definition because the double sums of 25 or 49 float products are not always exact (sums_exact)."""
import contextlib
import functools
from unittest import mock

import numpy as np

import corner_tiles as C
import harris_def as H
import mask_def as M
import synth

BLOCKS = (3, 5, 7)
K_DEFAULT = H.K_DEFAULT


def check_block(block):
    if block not in BLOCKS:
        raise ValueError("block_size is 3, 5 or 7")


def reflect_index(i, n):
    """BORDER_REFLECT_101 of the positions i on an axis of n pixels, any overshoot; a 1-pixel axis repeats its pixel"""
    i = np.asarray(i)
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    m = np.mod(i, p)
    return np.where(m >= n, p - m, m)


def products(gray, block):
    """steps 1 and 2: the float32 planes (dx dx, dx dy, dy dy) of the image itself"""
    check_block(block)
    g = np.ascontiguousarray(gray, np.uint8)
    h, w = g.shape
    f32 = np.float32
    scale = f32(1.0 / (4.0 * block * 255.0))
    k0, k1 = f32(2.0) * scale, scale
    p = g.astype(np.int32)[np.ix_(reflect_index(np.arange(-1, h + 1), h), reflect_index(np.arange(-1, w + 1), w))]
    pf = p.astype(f32)
    r = [p[j:j + h] for j in range(3)]                       # rows y - 1, y, y + 1
    d = [(x[:, 2:] - x[:, :-2]).astype(f32) for x in r]      # I(x + 1) - I(x - 1): whole numbers, exact
    dx = (d[0] + d[2]) * k1 + d[1] * k0
    rf = [pf[j:j + h] for j in range(3)]
    s = [x[:, 1:-1] * k0 + (x[:, :-2] + x[:, 2:]) * k1 for x in rf]
    dy = s[2] - s[0]
    assert dx.dtype == f32 and dy.dtype == f32
    return dx * dx, dx * dy, dy * dy


def _extended(q, r):
    """a product plane extended by r pixels of REFLECT_101 on every side: the product AT the mirrored position"""
    h, w = q.shape
    return q[np.ix_(reflect_index(np.arange(-r, h + r), h), reflect_index(np.arange(-r, w + r), w))]


def double_sums(gray, block):
    """step 3 before its rounding: three float64 maps, every addition in the defined order"""
    r = (block - 1) // 2
    h, w = np.asarray(gray).shape
    out = []
    for q in products(gray, block):
        pq = _extended(q, r).astype(np.float64)
        # (both chains start from +0, as harris_def.covariance_sums' does: that changes no sum but one whose terms are all -0, which comes
        #  out +0 -- only dx dy has such terms, and it enters both responses squared, so no response can tell and the kernels need not care)
        col = np.zeros((h, w + 2 * r), np.float64)           # c(y, x') = ((p(y - r) + p(y - r + 1)) + ...) + p(y + r), top to bottom
        for j in range(block):
            col = col + pq[j:j + h]
        acc = np.zeros((h, w), np.float64)                   # S(y, x) = ((c(x - r) + c(x - r + 1)) + ...) + c(x + r), left to right
        for i in range(block):
            acc = acc + col[:, i:i + w]
        out.append(acc)
    return tuple(out)


def covariance_sums(gray, block):
    """steps 1-3: (a, b, c) float32 maps"""
    return tuple(s.astype(np.float32) for s in double_sums(gray, block))


def _as_ints(x, shift=149):
    """the float64 (or float32) array x * 2^shift as Python integers (object array); exact for multiples of 2^-shift"""
    y = np.ldexp(np.asarray(x, np.float64), shift)
    assert np.array_equal(y, np.floor(y))
    return np.frompyfunc(int, 1, 1)(y)


def sums_exact(gray, block):
    """(whether every double sum of step 3 is the exact sum of its products, how many are not): the products times 2^149 are integers,
    and so is a sum that is exact"""
    r = (block - 1) // 2
    h, w = np.asarray(gray).shape
    bad = 0
    for q, s in zip(products(gray, block), double_sums(gray, block)):
        pq = _as_ints(_extended(q, r))
        col = pq[0:h]
        for j in range(1, block):
            col = col + pq[j:j + h]
        acc = col[:, 0:w]
        for i in range(1, block):
            acc = acc + col[:, i:i + w]
        scaled = np.ldexp(s, 149)
        whole = scaled == np.floor(scaled)                   # (a sum with bits below 2^-149 cannot be: the test says so rather than assuming it)
        same = np.frompyfunc(lambda a, b, ok: bool(ok) and int(a) == b, 3, 1)(np.where(whole, scaled, 0.0), acc, whole).astype(bool)
        bad += int((~same).sum())
    return bad == 0, bad


def min_eig(gray, block):
    """cornerMinEigenVal(gray, block, 3): the dense (h, w) float32 map"""
    return H.min_eig_from_sums(*covariance_sums(gray, block))


def corner_harris(gray, block, k=K_DEFAULT):
    """cornerHarris(gray, block, 3, k)"""
    H.check_k(k)
    return H.response_from_sums(*covariance_sums(gray, block), k)


def response(gray, block, harris=False, k=K_DEFAULT):
    return corner_harris(gray, block, k) if harris else min_eig(gray, block)


@contextlib.contextmanager
def _plugged(e):
    """harris_def's detector steps (candidates, good_features, Model) with the response map e in the place of its own"""
    with mock.patch.object(H, "corner_harris", lambda gray, k=K_DEFAULT: e):
        yield


def candidates(gray, mask=None, quality=0.01, block=3, harris=False, k=K_DEFAULT):
    """(response map, boolean map of the candidates, maxVal or None).  The steps are harris_def.candidates': for the minimum eigenvalue its
    rule 4 says nothing new -- with maxVal <= 0 no eigenvalue lies above a threshold of zero or more"""
    with _plugged(response(gray, block, harris, k)):
        return H.candidates(gray, mask, quality, k)


def good_features(gray, mask=None, max_corners=200, quality=0.01, min_distance=30.0, block=3, harris=False, k=K_DEFAULT):
    """goodFeaturesToTrack(gray, max_corners, quality, min_distance, mask, block, harris, k): (n, 2) float32 (x, y) in acceptance order"""
    e, cand, _ = candidates(gray, mask, quality, block, harris, k)
    return M.select(e, cand, max_corners, min_distance)


def Model(img, mask=None, quality=0.01, block=3, harris=False, k=K_DEFAULT):
    """harris_def.Model (final, keys, per tile lo, hi, early, negative; positive, frame_max) over the response of this block size"""
    with _plugged(response(img, block, harris, k)):
        m = H.Model(img, mask, quality, k)
    m.block, m.harris = block, harris
    return m


# ---- frames ---------------------------------------------------------------------------------------------------------------------------------
def dark_noise(seed=3):
    """dark noise beside hard 0 / 255 noise: dy = s2 - s0 can be a rounding residue far below k1, the products of one frame then span up
    to 77 bits and double sums of 25 or 49 of them are not all exact"""
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 10, (64, 64)).astype(np.uint8)
    g[:, 32:] = rng.integers(0, 2, (64, 32)) * 255
    return g


# The one-pass kernel of block B takes its path without reflection arithmetic for a tile whose source box -- columns ox - SX0 .. ox - SX0 +
# SW - 1, rows oy - SY0 .. oy - SY0 + SH - 1 -- lies inside the image (tile_interior over SourceTile<B>, csrc/vstab_corners_tile.hpp).  For tile (1, 1), ox = 64
# and oy = 31, the box ends on the image's last column at w = 64 - SX0 + SW and on its last row at h = 31 - SY0 + SH.
INTERIOR_BOX = {5: dict(SX0=4, SY0=4, SW=72, SH=39), 7: dict(SX0=8, SY0=5, SW=80, SH=41)}


def interior_edge_size(block):
    g = INTERIOR_BOX[block]
    return 64 - g["SX0"] + g["SW"], 31 - g["SY0"] + g["SH"]


def dense_frames(block):
    """name -> frame of the dense-map test at this block size (the byte-path frame is laid out by the test)"""
    cut = lambda seed, w, h: np.ascontiguousarray(synth.luma(seed, max(w, 16), max(h, 16))[:h, :w])
    we, he = interior_edge_size(block)
    return {"3x3": cut(13, 3, 3), "4x5": cut(13, 4, 5), "65x32": cut(13, 65, 32), "66x33": cut(13, 66, 33), "129x63": synth.luma(17, 129, 63),
            "322x182": cut(13, 322, 182), "dark_noise": dark_noise(),
            "interior_edge": cut(19, we, he), "interior_edge_less_w": cut(19, we - 1, he), "interior_edge_less_h": cut(19, we, he - 1)}


STATELESS_FRAMES = ("timing", "luma_322x182") + tuple(f"cut_{w}x{h}" for w, h in C.CUTS)
# The raw-output frames are harris_def's.  With the minimum eigenvalue the frames of pure edges have a maximum of zero or of rounding noise
# below it, which the minimum-eigenvalue definition does not cover ("Detection mask" in vstab.h): they run with the Harris response only.
RAW_FRAMES = H.RAW_FRAMES
RAW_FRAMES_MIN_EIG = tuple(n for n in RAW_FRAMES if n not in ("ramp_0", "ramp_1", "stripes_horizontal", "stripes_vertical"))
# raw-output sets under a mask (mask_def.RAW_SETS): tiles that return early beside tiles that spill or depend on timing
RAW_MASKED = ("timing_top_off", "grid_7x5_tiles_off")


def frame(name):
    return C.timing_frame() if name == "timing" else H.frame(name)


@functools.lru_cache(maxsize=None)
def raw_model(name, block, harris):
    """the model of a named frame (k = 0.04, quality = 0.01, no mask), computed once per process and shared"""
    return Model(frame(name), None, 0.01, block, harris)


@functools.lru_cache(maxsize=None)
def raw_masked_model(name, block, harris):
    g, m = M.RAW_SETS[name]()
    return Model(g, m, 0.01, block, harris)


@functools.lru_cache(maxsize=None)
def rule4_masked_model(block):
    return Model(*H.rule4_masked_frame(), 0.01, block, True)


def textured_frame():
    """the frame on which the three block sizes pick different corners"""
    return np.ascontiguousarray(M.overlay_clip(n=1)[2][0][:360])
