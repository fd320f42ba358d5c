"""The Harris response (include/vstab.h, "Harris response") restated in numpy: OpenCV 4.5's cornerHarris(gray, 3, 3, k)
and goodFeaturesToTrack(gray, corners, max_corners, quality, min_distance, mask, 3, true, k) on its CPU path, and the one-pass detector
with that response (k_corners_fused_harris / k_corners_fused_harris_masked, then k_filter_keys) restated per tile as mask_def.Model
restates the masked one.  No GPU here.

    1  a, b, c: the box sums of cornerMinEigenVal(3, 3) before its formula halves two of them (covariance_sums; fed through that formula
       they give oracle.min_eig bit for bit: test_harris_cpu.py)
    2  kf = (float)k, t = a + c, R = (a c - b b) - (kf t) t, every operation rounded to binary32 in that order
    3  the detector's steps are mask_def's, on R
    4  a (masked) maximum that is not positive gives no corner
    5  0 <= k < 0.25

numpy rounds every float32 operation once and contracts nothing, which is what the definition asks for."""
import functools

import numpy as np

import corner_tiles as C
import mask_def as M
import synth

TW, TH, SLOTS = C.TW, C.TH, C.SLOTS
K_DEFAULT = 0.04


def covariance_sums(gray):
    """step 1: (a, b, c) float32 maps -- Sobel derivatives scaled by 1 / (4 * 3 * 255) in the documented operation order, float products,
    the un-normalised 3 x 3 box sum under REFLECT_101 in double (exact), one rounding to float"""
    g = np.ascontiguousarray(gray, np.uint8)
    f32 = np.float32
    scale = f32(1.0 / (4.0 * 3.0 * 255.0))
    k0, k1 = f32(2.0) * scale, scale
    p = np.pad(g.astype(np.int32), 1, mode="reflect")
    pf = p.astype(f32)
    h, w = g.shape
    r = [p[j:j + h] for j in range(3)]                       # rows y - 1, y, y + 1
    d = [(x[:, 2:] - x[:, :-2]).astype(f32) for x in r]      # I(x + 1) - I(x - 1): whole numbers, exact
    dx = (d[0] + d[2]) * k1 + d[1] * k0
    rf = [pf[j:j + h] for j in range(3)]
    s = [x[:, 1:-1] * k0 + (x[:, :-2] + x[:, 2:]) * k1 for x in rf]
    dy = s[2] - s[0]
    assert dx.dtype == f32 and dy.dtype == f32
    out = []
    for q in (dx * dx, dx * dy, dy * dy):
        pq = np.pad(q, 1, mode="reflect").astype(np.float64)   # the product AT the mirrored position
        acc = np.zeros((h, w), np.float64)
        for j in range(3):
            for i in range(3):
                acc += pq[j:j + h, i:i + w]
        out.append(acc.astype(f32))
    return tuple(out)


def min_eig_from_sums(a, b, c):
    """the minimum-eigenvalue formula of vo_min_eig over the sums of step 1"""
    half = np.float32(0.5)
    a, c = a * half, c * half
    return (a + c) - np.sqrt((a - c) * (a - c) + b * b)


def response_from_sums(a, b, c, k=K_DEFAULT):
    """step 2"""
    kf = np.float32(k)
    t = a + c
    r = (a * c - b * b) - (kf * t) * t
    assert r.dtype == np.float32
    return r


def check_k(k):
    if not (np.isfinite(k) and 0.0 <= k < 0.25):
        raise ValueError("k lies in [0, 0.25)")


def corner_harris(gray, k=K_DEFAULT):
    """cornerHarris(gray, 3, 3, k): the dense (h, w) float32 map"""
    check_k(k)
    return response_from_sums(*covariance_sums(gray), k)


def candidates(gray, mask=None, quality=0.01, k=K_DEFAULT):
    """steps 1-5 of mask_def on R, with rule 4: (response map, boolean map of the candidates, maxVal or None)"""
    e = corner_harris(gray, k)
    sel = np.ones(e.shape, bool) if mask is None else np.asarray(mask) != 0
    assert sel.shape == e.shape
    none = np.zeros(e.shape, bool)
    if not sel.any():
        return e, none, None
    maxv = e[sel].max()
    if not maxv > 0:                                         # rule 4
        return e, none, maxv
    thr = np.float32(np.float64(maxv) * quality)
    return e, M._is_max(e) & (e > thr) & sel, maxv


def good_features(gray, mask=None, max_corners=200, quality=0.01, min_distance=30.0, k=K_DEFAULT):
    """goodFeaturesToTrack(gray, max_corners, quality, min_distance, mask, 3, true, k): (n, 2) float32 (x, y) in acceptance order"""
    e, cand, _ = candidates(gray, mask, quality, k)
    return M.select(e, cand, max_corners, min_distance)


class Model:
    """mask_def.Model over the Harris response: `final`, `keys`, and per tile `lo`, `hi`, `early`.  A tile's own maximum is taken in the
    order of the floats' bits read as int32 (as the kernel takes it); where that is negative the tile filters with -inf and `hi` is every
    3 x 3 maximum it holds (`negative`).  `positive` says whether the frame has a (masked) maximum above zero; where it has none, `final`
    is empty (rule 4) and what k_filter_keys leaves behind means nothing."""

    def __init__(self, img, mask=None, quality=0.01, k=K_DEFAULT):
        img = np.ascontiguousarray(img, np.uint8)
        h, w = img.shape
        self.img, self.quality, self.k = img, quality, k
        self.mask = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        self.w, self.h = w, h
        e, self.final, maxv = candidates(img, mask, quality, k)
        self.eig = e
        sel = self.sel = np.ones((h, w), bool) if mask is None else self.mask != 0
        bits = e.view(np.int32)
        self.frame_max = maxv
        self.positive = maxv is not None and bool(maxv > 0)
        if maxv is not None:                                  # the sign survives the int order (R is never -0: it ends in a subtraction of a value >= +0)
            assert (int(bits[sel].max()) >= 0) == bool(maxv >= 0)
        is_max = M._is_max(e) & sel
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
        return M.select(self.eig, self.final, max_corners, min_distance)


# ---- the frames of the raw-detector test (test_harris_cpu.py asserts the state each reaches) ----------------------------------------------
NON_POSITIVE = ("ramp_0", "ramp_1", "ramp_6", "stripes_horizontal", "stripes_vertical")
RAW_FRAMES = ("tile_255", "tile_256", "tile_257", "tile_258", "grid_5x3", "cut_65x32", "cut_66x33", "timing", "ramp_2", "stripes_diagonal") + NON_POSITIVE + (
    "luma_322x182",)


def frame(name):
    if name == "luma_322x182":
        return synth.luma(11, 322, 182)
    return C.make(name)


@functools.lru_cache(maxsize=None)
def raw_model(name):
    """the model of a named frame (k = 0.04, quality = 0.01, no mask), computed once per process and shared"""
    return Model(frame(name))


def rule4_masked_frame():
    """(frame, mask): vertical stripes with a patch of texture; the mask is zero on the patch and a margin.  The masked-in responses are
    all <= 0 while the patch holds positive corners: no corner, where the unmasked frame has some"""
    g = C.stripes(200, 95, "vertical").copy()
    g[30:62, 60:124] = synth.luma(5, 64, 32)
    m = M.full(95, 200)
    m[24:68, 52:132] = 0
    return g, m


@functools.lru_cache(maxsize=None)
def rule4_masked_model():
    return Model(*rule4_masked_frame())


def fall_back_frame():
    """the 2-px checkerboard at 640 x 512: more Harris candidates than the key capacity of a fresh Detector"""
    return C.checker(640, 512)
