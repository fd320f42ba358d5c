"""The corner gradient size (include/vstab.h, "Corner gradient size") restated in numpy: OpenCV 4.5's
cornerMinEigenVal(gray, B, G), cornerHarris(gray, B, G, k) and goodFeaturesToTrack(gray, corners, max_corners, quality, min_distance, mask, B,
G, useHarris, k) on its CPU path for B, G = 3, 5, 7.  No GPU here.

    1  kernels: getDerivKernels' integer Sobel pair, SMOOTH[G] from the centre outwards and DERIV[G] on the positive side
    2  scale: sigma = 1 / (2^(G - 1) B 255) in double, k_i = (float)((double)s_i sigma)
    3  dx: the row differences D (whole numbers), then the column pass from the outermost pair of rows inwards, the centre last
    4  dy: the smoothed rows S from the centre outwards, then the column pass over ascending i
    5  everything else is corner_block_def's (and through it harris_def's and mask_def's) with these products plugged in

With G = 3 the products are corner_block_def.products bit for bit."""
import contextlib
import functools
from unittest import mock

import numpy as np

import corner_block_def as B
import corner_tiles as C
import harris_def as H
import mask_def as M
import synth

BLOCKS = B.BLOCKS
GRADIENTS = (3, 5, 7)
NEW_PAIRS = tuple((b, g) for g in (5, 7) for b in BLOCKS)            # the pairs no "Corner block size" call serves
K_DEFAULT = B.K_DEFAULT
SMOOTH = {3: (2, 1), 5: (6, 4, 1), 7: (20, 15, 6, 1)}               # s_0 .. s_g
DERIV = {3: (0, 1), 5: (0, 2, 1), 7: (0, 5, 4, 1)}                  # d_0 .. d_g, antisymmetric

dark_noise, textured_frame, frame, reflect_index = B.dark_noise, B.textured_frame, B.frame, B.reflect_index
STATELESS_FRAMES, RAW_FRAMES, RAW_FRAMES_MIN_EIG, RAW_MASKED = B.STATELESS_FRAMES, B.RAW_FRAMES, B.RAW_FRAMES_MIN_EIG, B.RAW_MASKED


def check_gradient(gradient):
    if gradient not in GRADIENTS:
        raise ValueError("gradient_size is 3, 5 or 7")


def coefficients(block, gradient):
    """rule 2: (k_0 .. k_g) as float32"""
    B.check_block(block)
    check_gradient(gradient)
    sigma = 1.0 / (float(1 << (gradient - 1)) * block * 255.0)
    return tuple(np.float32(float(s) * sigma) for s in SMOOTH[gradient])


def row_differences(gray, gradient):
    """rule 3's row pass on the image extended by g rows above and below: D as int32, (h + 2 g, w)"""
    check_gradient(gradient)
    g = (gradient - 1) // 2
    img = np.ascontiguousarray(gray, np.uint8)
    h, w = img.shape
    p = img.astype(np.int32)[np.ix_(reflect_index(np.arange(-g, h + g), h), reflect_index(np.arange(-g, w + g), w))]
    d = np.zeros((h + 2 * g, w), np.int32)
    for i in range(1, g + 1):
        d += DERIV[gradient][i] * (p[:, g + i:g + i + w] - p[:, g - i:g - i + w])
    return d


def products(gray, block, gradient):
    """rules 1 - 4 and the three float products: the float32 planes (dx dx, dx dy, dy dy) of the image itself"""
    k = coefficients(block, gradient)
    g = (gradient - 1) // 2
    f32 = np.float32
    img = np.ascontiguousarray(gray, np.uint8)
    h, w = img.shape
    pf = img[np.ix_(reflect_index(np.arange(-g, h + g), h), reflect_index(np.arange(-g, w + g), w))].astype(f32)
    col = lambda i: pf[:, g + i:g + i + w]                            # I(y', x + i) for every extended row y'
    d = row_differences(img, gradient).astype(f32)                   # whole numbers of magnitude <= 2550: exact
    row = lambda a, i: a[g + i:g + i + h]                             # a(y + i, x)
    dx = (row(d, -g) + row(d, g)) * k[g]
    for m in range(g - 1, 0, -1):
        dx = dx + (row(d, -m) + row(d, m)) * k[m]
    dx = dx + row(d, 0) * k[0]
    s = col(0) * k[0] + (col(-1) + col(1)) * k[1]
    for m in range(2, g + 1):
        s = s + (col(-m) + col(m)) * k[m]
    dy = f32(DERIV[gradient][1]) * (row(s, 1) - row(s, -1))
    for m in range(2, g + 1):
        dy = dy + f32(DERIV[gradient][m]) * (row(s, m) - row(s, -m))
    assert dx.dtype == f32 and dy.dtype == f32 and dx.shape == (h, w) and dy.shape == (h, w)
    return dx * dx, dx * dy, dy * dy


@contextlib.contextmanager
def _plugged(gradient):
    """corner_block_def's steps behind the products (the box sum in its order, the responses, the detector, Model) over these products"""
    check_gradient(gradient)
    with mock.patch.object(B, "products", lambda gray, block: products(gray, block, gradient)):
        yield


def _over(name):
    def f(gray, block, gradient, *a, **kw):
        with _plugged(gradient):
            return getattr(B, name)(gray, block, *a, **kw)
    f.__name__ = name
    f.__doc__ = f"corner_block_def.{name} with the gradient size behind the block size"
    return f


double_sums, covariance_sums, sums_exact, min_eig, corner_harris, response = (_over(n) for n in ("double_sums", "covariance_sums", "sums_exact", "min_eig", "corner_harris",
                                                                                                   "response"))


def candidates(gray, mask=None, quality=0.01, block=3, gradient=3, harris=False, k=K_DEFAULT):
    with _plugged(gradient):
        return B.candidates(gray, mask, quality, block, harris, k)


def good_features(gray, mask=None, max_corners=200, quality=0.01, min_distance=30.0, block=3, gradient=3, harris=False, k=K_DEFAULT):
    """goodFeaturesToTrack(gray, max_corners, quality, min_distance, mask, block, gradient, harris, k): (n, 2) float32 (x, y)"""
    with _plugged(gradient):
        return B.good_features(gray, mask, max_corners, quality, min_distance, block, harris, k)


def Model(img, mask=None, quality=0.01, block=3, gradient=3, harris=False, k=K_DEFAULT):
    with _plugged(gradient):
        m = B.Model(img, mask, quality, block, harris, k)
    m.gradient = gradient
    return m


# ---- frames ---------------------------------------------------------------------------------------------------------------------------------
def source_box(block, gradient):
    """SourceTile<B, G> of csrc/vstab_corners_tile.hpp: the box tile_interior tests"""
    r, g = (block - 1) // 2, (gradient - 1) // 2
    sx0 = (r + 1 + g + 3) & ~3
    return dict(SX0=sx0, SY0=r + 1 + g, SW=(sx0 + 64 + r + 1 + g + 3) & ~3, SH=33 + block - 1 + 2 * g)


def interior_edge_size(block, gradient):
    """(w, h) at which the source box of tile (1, 1) ends on the image's last column and row"""
    b = source_box(block, gradient)
    return 64 - b["SX0"] + b["SW"], 31 - b["SY0"] + b["SH"]


def dense_frames(block, gradient):
    """corner_block_def.dense_frames with the interior-edge frames of this pair"""
    cut = lambda seed, w, h: np.ascontiguousarray(synth.luma(seed, max(w, 16), max(h, 16))[:h, :w])
    we, he = interior_edge_size(block, gradient)
    return {"3x3": cut(13, 3, 3), "4x5": cut(13, 4, 5), "65x32": cut(13, 65, 32), "66x33": cut(13, 66, 33), "129x63": synth.luma(17, 129, 63),
            "322x182": cut(13, 322, 182), "dark_noise": dark_noise(),
            "interior_edge": cut(19, we, he), "interior_edge_less_w": cut(19, we - 1, he), "interior_edge_less_h": cut(19, we, he - 1)}


@functools.lru_cache(maxsize=None)
def raw_model(name, block, gradient, harris):
    return Model(frame(name), None, 0.01, block, gradient, harris)


@functools.lru_cache(maxsize=None)
def raw_masked_model(name, block, gradient, harris):
    g, m = M.RAW_SETS[name]()
    return Model(g, m, 0.01, block, gradient, harris)
