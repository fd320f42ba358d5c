"""Start points on the argument edges of the LK tracker (vstab_pyr_lk, k_lk_track; video-annotator_amd/csrc/vstab_lk.hip): every
boundary of the per-level range test, the pyramid's level-count thresholds, frames smaller than the window, and non-finite or huge
coordinates.  Test infrastructure only (a plain module, imported by tests/test_lk_edges_cpu.py and tests/test_lk_edges_gpu.py).

The range test.  Level l (w_l x h_l) of a start point (x, y) is tracked iff the window origin floor(x 2^-l - 10) lies in [-21, w_l) and
floor(y 2^-l - 10) in [-21, h_l), all in float32 (origins(), the arithmetic of lk_segments.fetch_ahead).  The kernel evaluates that
test in five places -- the staging, the top level's preparation, a lower level's preparation, the level loop and the fetch-ahead
model of the next pair -- and the reference once.  boundary_cases() puts a start point on both sides of each of the four boundaries

    axis x: origin -22 | -21 (side "lo")   and   w_l - 1 | w_l (side "hi"),      axis y the same with h_l

of every level the pyramid has: the float32 value whose origin is the inner one of the pair, found by walking np.nextafter over the
float32 expression itself, and its float32 neighbour, whose origin is the outer one -- so the rounding of x 2^-l - 10 is part of the
test.  The other coordinate is an ordinary one (the frame's centre), or -- the corner cases -- sits on a boundary of another level.

Non-finite and huge points (SPECIALS): the reference's float-to-int conversion gives INT_MIN for NaN, +-inf and everything outside int,
so no level is tracked: status 0 and the point back as it came.  -0.0 and the smallest denormal are ordinary points."""
import numpy as np

import lk_def as L
import lk_segments as S
import oracle
import synth
from lk_def import FLT_EPSILON, pyramid  # noqa: F401  (pyramid(img): the levels of buildOpticalFlowPyramid at window 21)

LKW = S.LKW
HALF = S.HALF

# (w, h): 4, 4, 3, 2 and 1 levels; both sides of each level-count threshold of the shorter side (42|43, 84|85, 168|169) on each axis
# against a long side of 200; frames smaller than the 21-pixel window (every tap reflected, several folds), and 21 / 22
MAIN_SIZES = [(640, 360), (333, 181), (240, 144), (130, 80), (40, 30)]
THRESHOLD_SIZES = [(s, 200) for s in (42, 43, 84, 85, 168, 169)] + [(200, s) for s in (42, 43, 84, 85, 168, 169)]
TINY_SIZES = [(1, 1), (2, 3), (7, 9), (21, 21), (22, 22)]
SIZES = MAIN_SIZES + THRESHOLD_SIZES + TINY_SIZES
LEVELS = {(640, 360): 4, (333, 181): 4, (240, 144): 3, (130, 80): 2, (40, 30): 1,
          (42, 200): 1, (43, 200): 2, (84, 200): 2, (85, 200): 3, (168, 200): 3, (169, 200): 4,
          (200, 42): 1, (200, 43): 2, (200, 84): 2, (200, 85): 3, (200, 168): 3, (200, 169): 4,
          (1, 1): 1, (2, 3): 1, (7, 9): 1, (21, 21): 1, (22, 22): 1}


def size_id(size):
    return "%dx%d" % size


def frames(w, h, n=3):
    """n frames of one scene moving by about a pixel a frame: synth.luma and synth.shifted where the frame is larger than 30 px, seeded
    noise (the next frame: the noise rolled by a pixel, a tenth of it drawn again) below that.  The content only has to make the
    tracked levels do real work."""
    seed = 7 * w + h
    if min(w, h) > 30:
        base = synth.luma(seed, w, h, rects=max(6, w * h // 6000))
        out = [base] + [synth.shifted(base, 1.3 * k, -0.7 * k) for k in range(1, n)]
    else:
        rng = np.random.default_rng(seed)
        base = rng.integers(0, 256, (h, w), dtype=np.uint8)
        out = [base]
        for k in range(1, n):
            f = np.roll(base, (k % h if h > 1 else 0, k % w if w > 1 else 0), (0, 1)).copy()
            redo = rng.random((h, w)) < 0.1
            f[redo] = rng.integers(0, 256, int(redo.sum()), dtype=np.uint8)
            out.append(f)
    return [np.ascontiguousarray(f, np.uint8) for f in out]


def origins(c, l, W=21):
    """window origin of float32 coordinates c at level l, as lk_segments.fetch_ahead computes it: floor(c * 2^-l - half(W)) in float32,
    int64 (finite coordinates inside int only)"""
    return S._floor_i(np.asarray(c, np.float32) * np.float32(2.0 ** -l) - L.half(W))


def tracked(pts, w, h, W=21):
    """(n, nl) bool: level l of start point i passes the range test.  A non-finite coordinate, or one whose origin lies outside int,
    passes at no level (the reference's conversion gives INT_MIN for it)."""
    pts = np.asarray(pts, np.float32).reshape(-1, 2)
    nl, sizes = S.level_sizes(w, h, W)
    out = np.zeros((pts.shape[0], nl), bool)
    for l in range(nl):
        with np.errstate(invalid="ignore", over="ignore"):
            q = pts * np.float32(2.0 ** -l) - L.half(W)
        ok = np.isfinite(q).all(1) & (np.abs(q) < 2.0 ** 31).all(1)
        ip = S._floor_i(np.where(ok[:, None], q, 0))
        wl, hl = sizes[l]
        out[:, l] = ok & (ip[:, 0] >= -W) & (ip[:, 0] < wl) & (ip[:, 1] >= -W) & (ip[:, 1] < hl)
    return out


def boundary_pair(l, b, W=21):
    """-> (below, at): `at` is the smallest float32 whose level-l origin is >= b, `below` its float32 neighbour towards -inf (origin
    b - 1): walked over the float32 expression, starting from the real-number answer (b + (W - 1) / 2) * 2^l."""
    x = np.float32((b + (W - 1) // 2) * 2.0 ** l)
    lo = np.float32(-np.inf)
    while origins(x, l, W) < b:
        x = np.nextafter(x, np.float32(np.inf), dtype=np.float32)
    while origins(np.nextafter(x, lo, dtype=np.float32), l, W) >= b:
        x = np.nextafter(x, lo, dtype=np.float32)
    below = np.nextafter(x, lo, dtype=np.float32)
    assert origins(x, l, W) == b and origins(below, l, W) == b - 1, (l, b, x, below)
    return below, x


def edge_values(l, n_l, W=21):
    """the four float32 coordinates around the two boundaries of an axis of n_l pixels at level l:
    {("lo", "out"), ("lo", "in"), ("hi", "in"), ("hi", "out")}: value"""
    lo_out, lo_in = boundary_pair(l, -W, W)
    hi_in, hi_out = boundary_pair(l, n_l, W)
    return {("lo", "out"): lo_out, ("lo", "in"): lo_in, ("hi", "in"): hi_in, ("hi", "out"): hi_out}


def edge_cases(w, h, W=21):
    """-> (pts, tags): for every level the window's pyramid has and each axis, the four float32 coordinates around -W (origin -W - 1 | -W)
    and n_l (origin n_l - 1 | n_l), the other coordinate at the frame's centre; tags[i] = (level, axis, "lo" | "hi", "in" | "out")"""
    nl, sizes = S.level_sizes(w, h, W)
    centre = (np.float32(w * 0.5 + 0.25), np.float32(h * 0.5 - 0.25))
    pts, tags = [], []
    for l in range(nl):
        for axis in (0, 1):
            for (side, io), v in edge_values(l, sizes[l][axis], W).items():
                p = list(centre)
                p[axis] = v
                pts.append(p), tags.append((l, axis, side, io))
    return np.asarray(pts, np.float32), tags


def boundary_cases(w, h, W=21):
    """-> (pts (n, 2) float32, tags): edge_cases, tagged ("edge", level, axis, side, "in" | "out") -- axis 0 = x, 1 = y; the other
    coordinate is the frame's centre --, then ("corner", (level_x, side_x, io_x), (level_y, side_y, io_y)) and ("plain",)."""
    nl, sizes = S.level_sizes(w, h, W)
    centre = (np.float32(w * 0.5 + 0.25), np.float32(h * 0.5 - 0.25))
    vals = [[edge_values(l, sizes[l][axis], W) for l in range(nl)] for axis in (0, 1)]
    edges, edge_tags = edge_cases(w, h, W)
    pts, tags = edges.tolist(), [("edge",) + t for t in edge_tags]
    # corners: x on a boundary of level a, y on one of level b -- the finest with the coarsest, both ways, and the coarsest with itself
    for a, b in sorted({(0, nl - 1), (nl - 1, 0), (nl - 1, nl - 1)}):
        for sx in ("lo", "hi"):
            for sy in ("lo", "hi"):
                for iox, ioy in (("in", "in"), ("in", "out"), ("out", "in")):
                    pts.append([vals[0][a][(sx, iox)], vals[1][b][(sy, ioy)]]), tags.append(("corner", (a, sx, iox), (b, sy, ioy)))
    # and three ordinary points (a window on a boundary lies almost wholly outside the image, where the derivatives are zero: most of
    # those are rejected by the matrix): slots that stay alive beside the lost ones in a multi-pair launch
    for p in (centre, (min(3.5, w * 0.5), min(4.25, h * 0.5)), (max(w - 2.25, w * 0.5), max(h - 3.5, h * 0.5))):
        pts.append(list(p)), tags.append(("plain",))
    return np.asarray(pts, np.float32), tags


def pattern(row):
    """the L of "levels >= L tracked, levels below skipped" of one row of tracked(), or None if the row is no such pattern"""
    nl = len(row)
    for L in range(nl + 1):
        if not row[:L].any() and row[L:].all():
            return L
    return None


def matrix_rejected(prev, pts):
    """(n, nl) bool: the 2 x 2 gradient matrix of the window at level l is rejected (minEig < 1e-4 or D < FLT_EPSILON) -- the exact
    integer sums of the interpolated Scharr derivatives (zero outside the image) and the reference's float32 operation order.  Only
    meaningful where tracked() holds (elsewhere the origin is taken as 0)."""
    pts = np.asarray(pts, np.float32).reshape(-1, 2)
    h, w = prev.shape
    trk = tracked(pts, w, h)
    lv = pyramid(prev)
    out = np.zeros(trk.shape, bool)
    pad = LKW + 2
    wy, wx = np.mgrid[0:LKW, 0:LKW]
    for l, img in enumerate(lv):
        der = np.pad(oracle.scharr(img).astype(np.int64), ((pad, pad), (pad, pad), (0, 0)))
        q = np.where(trk[:, l, None], pts, 0) * np.float32(2.0 ** -l) - HALF
        ip = S._floor_i(q)
        a, b = q[:, 0] - ip[:, 0].astype(np.float32), q[:, 1] - ip[:, 1].astype(np.float32)
        one, sc = np.float32(1.0), np.float32(16384.0)
        iw00 = np.rint((one - a) * (one - b) * sc).astype(np.int64)
        iw01 = np.rint(a * (one - b) * sc).astype(np.int64)
        iw10 = np.rint((one - a) * b * sc).astype(np.int64)
        iw11 = 16384 - iw00 - iw01 - iw10
        for i in np.flatnonzero(trk[:, l]):
            Y, X = ip[i, 1] + pad + wy, ip[i, 0] + pad + wx
            d = (der[Y, X] * iw00[i] + der[Y, X + 1] * iw01[i] + der[Y + 1, X] * iw10[i] + der[Y + 1, X + 1] * iw11[i] + (1 << 13)) >> 14
            ix, iy = d[..., 0], d[..., 1]
            fs = np.float32(1.0 / (1 << 20))
            A11, A12, A22 = (np.float32((ix * ix).sum()) * fs, np.float32((ix * iy).sum()) * fs, np.float32((iy * iy).sum()) * fs)
            D = A11 * A22 - A12 * A12
            min_eig = ((A22 + A11) - np.sqrt((A11 - A22) * (A11 - A22) + (np.float32(4.0) * A12) * A12)) / np.float32(2 * LKW * LKW)
            out[i, l] = bool(min_eig < np.float32(1e-4) or D < FLT_EPSILON)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# non-finite and huge start points
# ---------------------------------------------------------------------------------------------------------------------------------
SPECIALS = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 3e9, -3e9, 2147483648.0, -2147483904.0], np.float32)
DENORMAL = np.float32(1.401298464324817e-45)   # the smallest positive float32


def special_points(w, h):
    """-> (pts, n_special, like_zero): the first n_special points have a SPECIALS coordinate (each with an ordinary one on either axis,
    and every pair of them); then, four to a group, (v, y0), (0.0, y0), (x0, v), (x0, 0.0) for v = -0.0 and the smallest denormal:
    like_zero lists (index of the point with v, index of its twin with 0.0)."""
    x0, y0 = np.float32(w * 0.5 + 0.25), np.float32(h * 0.5 - 0.25)
    pts = [(s, y0) for s in SPECIALS] + [(x0, s) for s in SPECIALS] + [(a, b) for a in SPECIALS for b in SPECIALS]
    n_special = len(pts)
    like_zero = []
    for v in (np.float32(-0.0), DENORMAL):
        k = len(pts)
        pts += [(v, y0), (np.float32(0.0), y0), (x0, v), (x0, np.float32(0.0))]
        like_zero += [(k, k + 1), (k + 2, k + 3)]
    return np.asarray(pts, np.float32), n_special, like_zero


def same_floats(a, b):
    """element-wise: equal bits, or both NaN (whatever the payload)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
