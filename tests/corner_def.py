"""The corner detector (include/vstab.h, "Detection mask", "Harris response", "Corner block size", "Corner gradient size"; DESIGN.md sections
24, 26, 35, 38) restated in numpy, once: OpenCV 4.5's cornerMinEigenVal(gray, B, G), cornerHarris(gray, B, G, k) and goodFeaturesToTrack(gray,
corners, max_corners, quality, min_distance, mask, B, G, useHarris, k) on its CPU path for B, G = 3, 5, 7, and the one-pass detector restated
per tile (Model).  Every option is an argument, in the order DetectSpec has them: mask, quality, block, gradient, harris, k.  No GPU here.

The response
    1  kernels: getDerivKernels' integer Sobel pair, SMOOTH[G] from the centre outwards and DERIV[G] on the positive side
    2  scale: sigma = 1 / (2^(G - 1) B 255) in double, k_i = (float)((double)s_i sigma)
    3  dx: the row differences D (whole numbers), then the column pass from the outermost pair of rows inwards, the centre last
    4  dy: the smoothed rows S from the centre outwards, then the column pass over ascending i
    5  products dx dx, dx dy, dy dy in binary32 (products)
    6  the B x B box sum over the product planes extended by REFLECT_101 (folding as often as it takes), in double and IN THIS ORDER: column
       sums top to bottom, then left to right, both from +0, then one rounding to float (double_sums, covariance_sums).  The order is part of
       the definition because the double sums are not always exact (sums_exact).
    7  minimum eigenvalue: a, c halved, (a + c) - sqrt((a - c)(a - c) + b b) (min_eig_from_sums; at B = G = 3 it is oracle.min_eig bit for
       bit: test_harris_cpu.py); Harris: kf = (float)k, t = a + c, R = (a c - b b) - (kf t) t, 0 <= k < 0.25 (response_from_sums); every
       operation rounded to binary32 in that order -- numpy rounds every float32 operation once and contracts nothing

The detector, on that response (candidates, select)
    1  the response map is that of the whole image: the mask plays no part in it
    2  maxVal = the maximum of the map over the pixels with mask != 0; none: no corner
    3  a (masked) maximum that is not positive gives no corner (for the minimum eigenvalue that says nothing new: with maxVal <= 0 no
       eigenvalue lies above a threshold of zero or more)
    4  threshold (float)((double)maxVal * quality), strict >, for every pixel
    5  the 3 x 3 maximum test runs over all pixels: a masked-out neighbour competes
    6  a candidate is an interior pixel that passes 4 and 5 and has mask != 0
    7  order (value descending, ties: later raster index first), the min_distance grid and max_corners

What a tile's own maximum runs over: the pixels with mask != 0 among the in-image part of the 66 x 33 responses around the tile.  A tile with
no such pixel returns early (`early`): it computes nothing, publishes no maximum and reports a count of 0."""
import functools

import numpy as np

import corner_tiles as C
import mask_def as M
import synth

TW, TH, SLOTS = C.TW, C.TH, C.SLOTS
BLOCKS = (3, 5, 7)
GRADIENTS = (3, 5, 7)
NEW_PAIRS = tuple((b, g) for g in (5, 7) for b in BLOCKS)            # the pairs no "Corner block size" call serves
K_DEFAULT = 0.04
SMOOTH = {3: (2, 1), 5: (6, 4, 1), 7: (20, 15, 6, 1)}               # s_0 .. s_g
DERIV = {3: (0, 1), 5: (0, 2, 1), 7: (0, 5, 4, 1)}                  # d_0 .. d_g, antisymmetric


def check_block(block):
    if block not in BLOCKS:
        raise ValueError("block_size is 3, 5 or 7")


def check_gradient(gradient):
    if gradient not in GRADIENTS:
        raise ValueError("gradient_size is 3, 5 or 7")


def check_k(k):
    if not (np.isfinite(k) and 0.0 <= k < 0.25):
        raise ValueError("k lies in [0, 0.25)")


# ---- the response -----------------------------------------------------------------------------------------------------------------------------
def reflect_index(i, n):
    """BORDER_REFLECT_101 of the positions i on an axis of n pixels, any overshoot; a 1-pixel axis repeats its pixel"""
    i = np.asarray(i)
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    m = np.mod(i, p)
    return np.where(m >= n, p - m, m)


def coefficients(block, gradient):
    """rule 2: (k_0 .. k_g) as float32"""
    check_block(block)
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


def products(gray, block=3, gradient=3):
    """rules 1 - 5: the float32 planes (dx dx, dx dy, dy dy) of the image itself"""
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


def _extended(q, r):
    """a product plane extended by r pixels of REFLECT_101 on every side: the product AT the mirrored position"""
    h, w = q.shape
    return q[np.ix_(reflect_index(np.arange(-r, h + r), h), reflect_index(np.arange(-r, w + r), w))]


def double_sums(gray, block=3, gradient=3):
    """rule 6 before its rounding: three float64 maps, every addition in the defined order"""
    r = (block - 1) // 2
    h, w = np.asarray(gray).shape
    out = []
    for q in products(gray, block, gradient):
        pq = _extended(q, r).astype(np.float64)
        # (both chains start from +0: that changes no sum but one whose terms are all -0, which comes out +0 -- only dx dy has such terms,
        #  and it enters both responses squared, so no response can tell and the kernels need not care)
        col = np.zeros((h, w + 2 * r), np.float64)           # c(y, x') = ((p(y - r) + p(y - r + 1)) + ...) + p(y + r), top to bottom
        for j in range(block):
            col = col + pq[j:j + h]
        acc = np.zeros((h, w), np.float64)                   # S(y, x) = ((c(x - r) + c(x - r + 1)) + ...) + c(x + r), left to right
        for i in range(block):
            acc = acc + col[:, i:i + w]
        out.append(acc)
    return tuple(out)


def covariance_sums(gray, block=3, gradient=3):
    """rules 1 - 6: (a, b, c) float32 maps"""
    return tuple(s.astype(np.float32) for s in double_sums(gray, block, gradient))


def _as_ints(x, shift=149):
    """the float64 (or float32) array x * 2^shift as Python integers (object array); exact for multiples of 2^-shift"""
    y = np.ldexp(np.asarray(x, np.float64), shift)
    assert np.array_equal(y, np.floor(y))
    return np.frompyfunc(int, 1, 1)(y)


def sums_exact(gray, block=3, gradient=3):
    """(whether every double sum of rule 6 is the exact sum of its products, how many are not): the products times 2^149 are integers,
    and so is a sum that is exact"""
    r = (block - 1) // 2
    h, w = np.asarray(gray).shape
    bad = 0
    for q, s in zip(products(gray, block, gradient), double_sums(gray, block, gradient)):
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


def min_eig_from_sums(a, b, c):
    """the minimum-eigenvalue formula of vo_min_eig over the sums of rule 6"""
    half = np.float32(0.5)
    a, c = a * half, c * half
    return (a + c) - np.sqrt((a - c) * (a - c) + b * b)


def response_from_sums(a, b, c, k=K_DEFAULT):
    """the Harris formula over the sums of rule 6"""
    kf = np.float32(k)
    t = a + c
    r = (a * c - b * b) - (kf * t) * t
    assert r.dtype == np.float32
    return r


def min_eig(gray, block=3, gradient=3):
    """cornerMinEigenVal(gray, block, gradient): the dense (h, w) float32 map"""
    return min_eig_from_sums(*covariance_sums(gray, block, gradient))


def corner_harris(gray, block=3, gradient=3, k=K_DEFAULT):
    """cornerHarris(gray, block, gradient, k)"""
    check_k(k)
    return response_from_sums(*covariance_sums(gray, block, gradient), k)


def response(gray, block=3, gradient=3, harris=False, k=K_DEFAULT):
    return corner_harris(gray, block, gradient, k) if harris else min_eig(gray, block, gradient)


# ---- the detector ---------------------------------------------------------------------------------------------------------------------------
def _is_max(e):
    """interior pixels that equal the maximum of their 3 x 3 neighbourhood (every neighbour of an interior pixel is in the image)"""
    h, w = e.shape
    pad = np.full((h + 2, w + 2), -np.inf, np.float32)
    pad[1:-1, 1:-1] = e
    m = e.copy()
    for dy in range(3):
        for dx in range(3):
            m = np.maximum(m, pad[dy:dy + h, dx:dx + w])
    inner = np.zeros((h, w), bool)
    inner[1:h - 1, 1:w - 1] = True
    return inner & (e == m)


def candidates(gray, mask=None, quality=0.01, block=3, gradient=3, harris=False, k=K_DEFAULT):
    """steps 1 - 6: (response map, boolean map of the candidates, maxVal or None)"""
    e = response(np.ascontiguousarray(gray, np.uint8), block, gradient, harris, k)
    sel = np.ones(e.shape, bool) if mask is None else np.asarray(mask) != 0
    assert sel.shape == e.shape
    none = np.zeros(e.shape, bool)
    if not sel.any():
        return e, none, None
    maxv = e[sel].max()
    if not maxv > 0:                                         # step 3
        return e, none, maxv
    thr = np.float32(np.float64(maxv) * quality)
    # (OpenCV sets what fails the threshold to zero and dilates that map: a pixel above a non-negative threshold that equals the maximum of
    #  the thresholded map equals the maximum of the raw one, and the other way round, since zeroed neighbours lie below it either way)
    return e, _is_max(e) & (e > thr) & sel, maxv


def select(e, cand, max_corners, min_distance):
    """step 7, as vo_good_features and select_corners (vstab_hostlogic.hpp) run it: keys descending, the grid of cells of round(min_distance) px"""
    h, w = e.shape
    ys, xs = np.nonzero(cand)
    keys = (e[ys, xs].view(np.uint32).astype(np.uint64) << np.uint64(32)) | (ys * w + xs).astype(np.uint64)
    order = np.argsort(keys)[::-1]
    xs, ys = xs[order], ys[order]
    cell = int(np.rint(min_distance))
    if cell < 1:
        n = len(xs) if max_corners <= 0 else min(len(xs), max_corners)
        return np.stack([xs[:n], ys[:n]], 1).astype(np.float32).reshape(-1, 2)
    gw, gh = -(-w // cell), -(-h // cell)
    grid = [[] for _ in range(gw * gh)]
    md2 = min_distance * min_distance
    out = []
    for x, y in zip(xs.tolist(), ys.tolist()):
        xc, yc = x // cell, y // cell
        good = True
        for yy in range(max(yc - 1, 0), min(yc + 1, gh - 1) + 1):
            for xx in range(max(xc - 1, 0), min(xc + 1, gw - 1) + 1):
                for (a, b) in grid[yy * gw + xx]:
                    if (x - a) * (x - a) + (y - b) * (y - b) < md2:   # (whole numbers below 2^24: exact in the float the detectors use)
                        good = False
                        break
                if not good:
                    break
            if not good:
                break
        if good:
            grid[yc * gw + xc].append((x, y))
            out.append((x, y))
            if max_corners > 0 and len(out) == max_corners:
                break
    return np.array(out, np.float32).reshape(-1, 2)


def good_features(gray, mask=None, max_corners=200, quality=0.01, min_distance=30.0, block=3, gradient=3, harris=False, k=K_DEFAULT):
    """goodFeaturesToTrack(gray, max_corners, quality, min_distance, mask, block, gradient, harris, k): (n, 2) float32 (x, y) in acceptance order"""
    e, cand, _ = candidates(gray, mask, quality, block, gradient, harris, k)
    return select(e, cand, max_corners, min_distance)


class Model:
    """The one-pass detector (k_corners_fused and its variants, then k_filter_keys) per tile, as corner_tiles.Model restates the plain one:
    `final`, `keys`, and per tile `early`, `lo` and `hi` -- the count a tile reports lies between the survivors under the final threshold
    quality * maxVal and those under quality * the tile's own (masked) maximum.  That maximum is taken in the order of the floats' bits read
    as int32 (as the kernel takes it); where it is negative the tile filters with -inf and `hi` is every 3 x 3 maximum it holds
    (`negative`).  `positive` says whether the frame has a (masked) maximum above zero; where it has none, `final` is empty (step 3) and
    what k_filter_keys leaves behind means nothing."""

    def __init__(self, img, mask=None, quality=0.01, block=3, gradient=3, harris=False, k=K_DEFAULT):
        img = np.ascontiguousarray(img, np.uint8)
        h, w = img.shape
        self.img, self.quality, self.block, self.gradient, self.harris, self.k = img, quality, block, gradient, harris, k
        self.mask = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        self.w, self.h = w, h
        e, self.final, maxv = candidates(img, mask, quality, block, gradient, harris, k)
        self.eig = e
        sel = self.sel = np.ones((h, w), bool) if mask is None else self.mask != 0
        bits = e.view(np.int32)
        self.frame_max = maxv
        self.positive = maxv is not None and bool(maxv > 0)
        if maxv is not None:                                  # the sign survives the int order (R is never -0: it ends in a subtraction of a value >= +0)
            assert (int(bits[sel].max()) >= 0) == bool(maxv >= 0)
        is_max = _is_max(e) & sel
        ys, xs = np.nonzero(self.final)
        self.keys = np.sort((e[ys, xs].view(np.uint32).astype(np.uint64) << np.uint64(32)) | (ys * w + xs).astype(np.uint64))
        self.n = len(self.keys)
        self.tiles_x, self.tiles_y = -(-w // TW), -(-h // TH)
        shape = (self.tiles_y, self.tiles_x)
        self.lo, self.hi = np.zeros(shape, np.int64), np.zeros(shape, np.int64)
        self.early, self.negative = np.zeros(shape, bool), np.zeros(shape, bool)
        for ty in range(self.tiles_y):
            for tx in range(self.tiles_x):
                oy, ox = ty * TH, tx * TW
                around = (slice(max(oy - 1, 0), min(oy + TH + 1, h)), slice(max(ox - 1, 0), min(ox + TW + 1, w)))
                if not sel[around].any():
                    self.early[ty, tx] = True
                    continue
                own = int(bits[around][sel[around]].max())
                self.negative[ty, tx] = own < 0
                thr_own = np.float32(np.float64(np.int32(own).view(np.float32)) * quality) if own >= 0 else np.float32(-np.inf)
                sl = (slice(oy, min(oy + TH, h)), slice(ox, min(ox + TW, w)))
                self.lo[ty, tx] = int(self.final[sl].sum())
                self.hi[ty, tx] = int((is_max[sl] & (e[sl] > thr_own)).sum())
        assert (self.lo <= self.hi).all() and int(self.lo.sum()) == self.n
        self.spills = self.lo > SLOTS
        self.timing = (self.lo <= SLOTS) & (self.hi > SLOTS)
        self.keyed = self.hi <= SLOTS
        self.full = (self.lo == SLOTS) & (self.hi == SLOTS)

    def spilled_range(self):
        return int(self.spills.sum()), int((self.hi > SLOTS).sum())

    def corners(self, max_corners, min_distance):
        return select(self.eig, self.final, max_corners, min_distance)


# ---- frames ---------------------------------------------------------------------------------------------------------------------------------
def dark_noise(seed=3):
    """dark noise beside hard 0 / 255 noise: dy = s2 - s0 can be a rounding residue far below k1, the products of one frame then span up
    to 77 bits and double sums of 25 or 49 of them are not all exact"""
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 10, (64, 64)).astype(np.uint8)
    g[:, 32:] = rng.integers(0, 2, (64, 32)) * 255
    return g


def textured_frame():
    """the frame on which the block and gradient sizes pick different corners"""
    return np.ascontiguousarray(M.overlay_clip(n=1)[2][0][:360])


# The one-pass kernel of a pair (B, G) takes its path without reflection arithmetic for a tile whose source box -- columns ox - SX0 .. ox -
# SX0 + SW - 1, rows oy - SY0 .. oy - SY0 + SH - 1 -- lies inside the image (tile_interior over SourceTile<B, G>,
# csrc/vstab_corners_tile.hpp).  INTERIOR_BOX is that box written out by hand for gradient 3 (test_corner_gradient_cpu.py holds source_box
# against it).
INTERIOR_BOX = {5: dict(SX0=4, SY0=4, SW=72, SH=39), 7: dict(SX0=8, SY0=5, SW=80, SH=41)}


def source_box(block, gradient=3):
    """SourceTile<B, G> of csrc/vstab_corners_tile.hpp: the box tile_interior tests"""
    r, g = (block - 1) // 2, (gradient - 1) // 2
    sx0 = (r + 1 + g + 3) & ~3
    return dict(SX0=sx0, SY0=r + 1 + g, SW=(sx0 + 64 + r + 1 + g + 3) & ~3, SH=33 + block - 1 + 2 * g)


def interior_edge_size(block, gradient=3):
    """(w, h) at which the source box of tile (1, 1), ox = 64 and oy = 31, ends on the image's last column and row"""
    b = source_box(block, gradient)
    return 64 - b["SX0"] + b["SW"], 31 - b["SY0"] + b["SH"]


def dense_frames(block, gradient=3):
    """name -> frame of the dense-map test of this pair (the byte-path frame is laid out by the test)"""
    cut = lambda seed, w, h: np.ascontiguousarray(synth.luma(seed, max(w, 16), max(h, 16))[:h, :w])
    we, he = interior_edge_size(block, gradient)
    return {"3x3": cut(13, 3, 3), "4x5": cut(13, 4, 5), "65x32": cut(13, 65, 32), "66x33": cut(13, 66, 33), "129x63": synth.luma(17, 129, 63),
            "322x182": cut(13, 322, 182), "dark_noise": dark_noise(),
            "interior_edge": cut(19, we, he), "interior_edge_less_w": cut(19, we - 1, he), "interior_edge_less_h": cut(19, we, he - 1)}


# the frames of the raw-detector tests (test_harris_cpu.py and test_corner_block_cpu.py assert the state each reaches).  With the minimum
# eigenvalue the frames of pure edges have a maximum of zero or of rounding noise below it, which the minimum-eigenvalue definition does
# not cover ("Detection mask" in vstab.h): they run with the Harris response only.
NON_POSITIVE = ("ramp_0", "ramp_1", "ramp_6", "stripes_horizontal", "stripes_vertical")
RAW_FRAMES = ("tile_255", "tile_256", "tile_257", "tile_258", "grid_5x3", "cut_65x32", "cut_66x33", "timing", "ramp_2", "stripes_diagonal") + NON_POSITIVE + (
    "luma_322x182",)
RAW_FRAMES_MIN_EIG = tuple(n for n in RAW_FRAMES if n not in ("ramp_0", "ramp_1", "stripes_horizontal", "stripes_vertical"))
# raw-output sets under a mask (mask_def.RAW_SETS): tiles that return early beside tiles that spill or depend on timing
RAW_MASKED = ("timing_top_off", "grid_7x5_tiles_off")
STATELESS_FRAMES = ("timing", "luma_322x182") + tuple(f"cut_{w}x{h}" for w, h in C.CUTS)


def frame(name):
    if name == "luma_322x182":
        return synth.luma(11, 322, 182)
    return C.timing_frame() if name == "timing" else C.make(name)


@functools.lru_cache(maxsize=None)
def raw_model(name, block=3, gradient=3, harris=False):
    """the model of a named frame (k = 0.04, quality = 0.01, no mask), computed once per process and shared"""
    return Model(frame(name), None, 0.01, block, gradient, harris)


@functools.lru_cache(maxsize=None)
def raw_masked_model(name, block=3, gradient=3, harris=False):
    """the masked model of a named raw set of mask_def.RAW_SETS"""
    g, m = M.RAW_SETS[name]()
    return Model(g, m, 0.01, block, gradient, harris)


def rule4_masked_frame():
    """(frame, mask): vertical stripes with a patch of texture; the mask is zero on the patch and a margin.  The masked-in responses are
    all <= 0 while the patch holds positive corners: no corner, where the unmasked frame has some"""
    g = C.stripes(200, 95, "vertical").copy()
    g[30:62, 60:124] = synth.luma(5, 64, 32)
    m = M.full(95, 200)
    m[24:68, 52:132] = 0
    return g, m


@functools.lru_cache(maxsize=None)
def rule4_masked_model(block=3, gradient=3):
    return Model(*rule4_masked_frame(), 0.01, block, gradient, True)


def fall_back_frame():
    """the 2-px checkerboard at 640 x 512: more candidates than the key capacity of a fresh Detector"""
    return C.checker(640, 512)
