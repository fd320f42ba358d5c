"""The tracker (include/vstab.h, "Tracker options" and "Tracker window"; DESIGN.md sections 29 and 34) restated in numpy, once: OpenCV 4.5's
CPU LKTrackerInvoker with winSize (W, W), maxLevel, the criteria's count and epsilon, minEigThreshold, OPTFLOW_USE_INITIAL_FLOW, err and
OPTFLOW_LK_GET_MIN_EIGENVALS, in this project's arithmetic -- exact integer sums converted once, the float32 operations in the order of
oracle/vstab_oracle.c (vo_lk_point).  No GPU here, and no call of oracle.pyr_lk: test_lk_options_cpu.py holds this file against it at the
default window and options.  A plain module, imported by the tests, by lk_segments and by lk_edges (so the case helpers at its end import
those two where they run, not at the top).

    1  levels      min(levels_W(w, h), max_level + 1); levels_W halves with (n + 1) // 2 and stops before the first level with w_l <= W or
                   h_l <= W; at most 4.  A level is what it always was (oracle.pyr_down, oracle.scharr)
    2  start       with USE_INITIAL_FLOW the top level L starts the next-image estimate at guess * float32(2^-L); the previous image's side
                   (window, derivatives, matrix, the previous point's range test) does not see the guess
    3  iterations  at most max_iter; a level ends on (double)dx dx + (double)dy dy <= (double)eps (double)eps; the oscillation rule keeps 0.01
    4  rejection   minEig < float32(min_eig_threshold) or D < FLT_EPSILON; minEig is divided by float32(2 W W)
    5  err         level 0, status still 1 behind the final range test: f = next - half, origin floor(f), weights of its fraction,
                   S = sum over the window of |DESCALE(J interpolated, 9) - Iw|, an integer <= W W 8160 < 2^24 (asserted),
                   err = float32(S) / float32(32 W W); status 0: err 0
    6  min eig     with GET_MIN_EIGENVALS err is minEig of the finest level whose matrix was formed, rejected or not; none: 0

    half      float32((W - 1) / 2)
    origin    floor(p 2^-l - half), float32
    range     origin in [-W, w_l) x [-W, h_l); NaN, infinities and values outside int fail (the reference's conversion gives INT_MIN)
    padding   REFLECT_101 of both images, folded as often as it takes; derivatives outside the image are zero

All points of a call advance together, level by level and iteration by iteration (arrays of n x W x W); a point's arithmetic never reads
another point's.  track() returns both err modes at once and, beside the definition, what the tests want to reach on purpose in the KERNEL's
bookkeeping (video-annotator_amd/csrc/vstab_lk_window.hpp): the block geometry (geometry()) and whether the residual's window lies outside
the next-image block the iterations left staged (`resid_restaged`).  Where a block sits never changes a value."""
import numpy as np

import oracle

WINDOWS = (15, 21, 31)          # what the library offers
NEW_WINDOWS = (15, 31)          # ... beyond calcOpticalFlowPyrLK's default
USE_INITIAL_FLOW, GET_MIN_EIGENVALS = 4, 8
F32 = np.float32
ONE, SC, FLT_SCALE = F32(1.0), F32(16384.0), F32(1.0 / (1 << 20))
FLT_EPSILON = F32(1.1920928955078125e-7)


def _roundup4(n):
    return (n + 3) & ~3


def geometry(W):
    """the kernel's blocks for window W: tap block, previous-image neighbourhood, next-image slack and block, fetch-ahead slack, window
    pixels per lane"""
    lkt, lkr, lkjm = W + 1, _roundup4(W + 3), 5
    lkjr = _roundup4(lkt + 2 * lkjm)
    return {"LKT": lkt, "LKR": lkr, "LKJM": lkjm, "LKJR": lkjr, "SLACK": (lkjr - lkr) // 2, "PPL": (W * W + 63) // 64}


def half(W):
    return F32((W - 1) // 2)


def level_sizes(w, h, W=21):
    """(levels_W, [(w_l, h_l)]): buildOpticalFlowPyramid with maxLevel 3 and winSize W"""
    sizes = [(w, h)]
    for _ in range(3):
        w, h = (w + 1) // 2, (h + 1) // 2
        if w <= W or h <= W:
            break
        sizes.append((w, h))
    return len(sizes), sizes


def levels_of(w, h, W=21, max_level=3):
    return min(level_sizes(w, h, W)[0], max_level + 1)


def pyramid(img, nl=None, W=21):
    """nl levels (default: all the window's pyramid has) of buildOpticalFlowPyramid: oracle.pyr_down chained"""
    if nl is None:
        nl = level_sizes(img.shape[1], img.shape[0], W)[0]
    out = [np.ascontiguousarray(img, np.uint8)]
    for _ in range(1, nl):
        out.append(oracle.pyr_down(out[-1]))
    return out


def _floor_i(v):
    return np.floor(v).astype(np.int64)


def _reflect101(i, n):
    i = np.asarray(i, np.int64).copy()
    if n == 1:
        return np.zeros_like(i)
    while True:
        bad = (i < 0) | (i >= n)
        if not bad.any():
            return i
        i = np.where(i < 0, -i, np.where(i >= n, 2 * n - 2 - i, i))


def _padded(img, pad):
    """the image under BORDER_REFLECT_101, pad pixels to every side, int64"""
    h, w = img.shape
    return img[np.ix_(_reflect101(np.arange(-pad, h + pad), h), _reflect101(np.arange(-pad, w + pad), w))].astype(np.int64)


def _in_range(q, w, h, W):
    """the reference's range test of a window origin floor(q) -> (ok, origin int64 (0 where not ok))"""
    with np.errstate(invalid="ignore"):
        fin = np.isfinite(q).all(1) & (np.abs(q) < 2.0 ** 31).all(1)
    ip = _floor_i(np.where(fin[:, None], q, 0))
    ok = fin & (ip[:, 0] >= -W) & (ip[:, 0] < w) & (ip[:, 1] >= -W) & (ip[:, 1] < h)
    return ok, np.where(ok[:, None], ip, 0)


def _weights(q, ip):
    a, b = q[:, 0] - ip[:, 0].astype(F32), q[:, 1] - ip[:, 1].astype(F32)
    w00 = np.rint((ONE - a) * (ONE - b) * SC).astype(np.int64)
    w01 = np.rint(a * (ONE - b) * SC).astype(np.int64)
    w10 = np.rint((ONE - a) * b * SC).astype(np.int64)
    return [x[:, None, None] for x in (w00, w01, w10, 16384 - w00 - w01 - w10)]


def _interp(P, ip, wts, shift, W, pad):
    """DESCALE(bilinear taps of the padded plane P at the windows of origin ip, shift): (n, W, W) int64"""
    wy, wx = np.mgrid[0:W, 0:W]
    Y, X = ip[:, 1, None, None] + pad + wy, ip[:, 0, None, None] + pad + wx
    return (P[Y, X] * wts[0] + P[Y, X + 1] * wts[1] + P[Y + 1, X] * wts[2] + P[Y + 1, X + 1] * wts[3] + (1 << (shift - 1))) >> shift


def _block(c, w, h, W):
    """the kernel's lk_block_origin for a next-image block around the window corner c: origin floor(c) - LKJM where c lies in
    (-(W + 1), w) x (-(W + 1), h), else none (a huge negative origin, for which "window outside the block" holds)"""
    with np.errstate(invalid="ignore"):
        ok = (c[:, 0] > -(W + 1)) & (c[:, 0] < w) & (c[:, 1] > -(W + 1)) & (c[:, 1] < h)
    return np.where(ok[:, None], _floor_i(np.where(ok[:, None], c, 0)) - 5, -(1 << 30))


def _outside(ip, blk, W):
    jr = geometry(W)["LKJR"]
    return (ip[:, 0] < blk[:, 0]) | (ip[:, 1] < blk[:, 1]) | (ip[:, 0] + W + 1 > blk[:, 0] + jr) | (ip[:, 1] + W + 1 > blk[:, 1] + jr)


def track(prev, nxt, pts, W=21, max_level=3, max_iter=30, eps=0.01, min_eig=1e-4, guess=None):
    """-> dict: xy (n, 2) float32, status (n,) uint8, err (n,) float32 (rule 5), min_eig (n,) float32 (rule 6), iterations (n, 4) int,
    levels (n, 4, 2) float32 (where each point stood after level l, as oracle.pyr_lk_trace: NaN for absent levels), nl, and
    resid_restaged (n,) bool.  guess: (n, 2) float32 -- USE_INITIAL_FLOW."""
    assert W % 2 == 1
    HALF, PAD, LKJM = half(W), W + 3, 5            # a window origin lies in [-W, n): taps reach from -W to n + W
    prev, nxt = np.ascontiguousarray(prev, np.uint8), np.ascontiguousarray(nxt, np.uint8)
    pts = np.ascontiguousarray(pts, F32).reshape(-1, 2)
    n = pts.shape[0]
    h0, w0 = prev.shape
    nl = levels_of(w0, h0, W, max_level)
    pI, pJ = pyramid(prev, nl), pyramid(nxt, nl)
    thr, eps2 = F32(min_eig), np.float64(eps) * np.float64(eps)
    start = pts if guess is None else np.ascontiguousarray(guess, F32).reshape(-1, 2)
    assert start.shape == pts.shape
    xy = np.zeros((n, 2), F32)
    status = np.ones(n, np.uint8)
    err, meig = np.zeros(n, F32), np.zeros(n, F32)
    iters = np.zeros((n, 4), np.int64)
    lv = np.full((n, 4, 2), np.nan, F32)
    blk0 = np.full((n, 2), -(1 << 30), np.int64)      # (kernel bookkeeping) the level-0 block the iterations leave staged
    restaged = np.zeros(n, bool)
    Iw0 = np.zeros((n, W, W), np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for l in range(nl - 1, -1, -1):
            h, w = pI[l].shape
            ls = F32(2.0 ** -l)
            xy = start * ls if l == nl - 1 else xy * F32(2.0)                                   # rule 2
            if l == 1:
                blk0 = _block(xy * F32(2.0) - HALF, w0, h0, W)
            q = pts * ls - HALF
            ok, ip = _in_range(q, w, h, W)
            if l == 0:
                status[~ok] = 0
                if nl == 1:
                    blk0 = np.where(ok[:, None], ip - LKJM, blk0) if guess is None else _block(xy - HALF, w, h, W)
            idx = np.flatnonzero(ok)
            if idx.size:
                PI, PJ = _padded(pI[l], PAD), _padded(pJ[l], PAD)
                der = np.pad(oracle.scharr(pI[l]).astype(np.int64), ((PAD, PAD), (PAD, PAD), (0, 0)))
                wts = _weights(q[idx], ip[idx])
                Iw = _interp(PI, ip[idx], wts, 9, W, PAD)
                Ix, Iy = _interp(der[..., 0], ip[idx], wts, 14, W, PAD), _interp(der[..., 1], ip[idx], wts, 14, W, PAD)
                if l == 0:
                    Iw0[idx] = Iw
                A11 = (Ix * Ix).sum((1, 2)).astype(F32) * FLT_SCALE
                A12 = (Ix * Iy).sum((1, 2)).astype(F32) * FLT_SCALE
                A22 = (Iy * Iy).sum((1, 2)).astype(F32) * FLT_SCALE
                Dt = A11 * A22 - A12 * A12
                me = ((A22 + A11) - np.sqrt((A11 - A22) * (A11 - A22) + (F32(4.0) * A12) * A12)) / F32(2 * W * W)
                meig[idx] = me                                                                   # rule 6: before the rejection test
                rej = (me < thr) | (Dt < FLT_EPSILON)                                            # rule 4
                if l == 0:
                    status[idx[rej]] = 0
                keep = ~rej
                idx, Iw, Ix, Iy, A11, A12, A22 = idx[keep], Iw[keep], Ix[keep], Iy[keep], A11[keep], A12[keep], A22[keep]
                Dt = ONE / Dt[keep]
                npos = xy[idx] - HALF
                pd = np.zeros((idx.size, 2), F32)
                live = np.arange(idx.size)
                for j in range(max_iter):                                                        # rule 3
                    if live.size == 0:
                        break
                    g = idx[live]
                    iters[g, l] += 1
                    okj, inj = _in_range(npos[live], w, h, W)
                    if l == 0:
                        status[g[~okj]] = 0
                    live, g, inj = live[okj], g[okj], inj[okj]
                    if live.size == 0:
                        break
                    if l == 0:
                        out = _outside(inj, blk0[g], W)
                        blk0[g[out]] = inj[out] - LKJM
                    diff = _interp(PJ, inj, _weights(npos[live], inj), 9, W, PAD) - Iw[live]
                    b1 = (diff * Ix[live]).sum((1, 2)).astype(F32) * FLT_SCALE
                    b2 = (diff * Iy[live]).sum((1, 2)).astype(F32) * FLT_SCALE
                    dx = (A12[live] * b2 - A22[live] * b1) * Dt[live]
                    dy = (A12[live] * b1 - A11[live] * b2) * Dt[live]
                    d = np.stack([dx, dy], 1)
                    npos[live] = npos[live] + d
                    xy[g] = npos[live] + HALF
                    conv = dx.astype(np.float64) * dx + dy.astype(np.float64) * dy <= eps2
                    osc = ~conv & (j > 0) & (np.abs((dx + pd[live, 0]).astype(np.float64)) < 0.01) & (np.abs((dy + pd[live, 1]).astype(np.float64)) < 0.01)
                    xy[g[osc]] = xy[g[osc]] - d[osc] * F32(0.5)
                    pd[live] = d
                    live = live[~(conv | osc)]
            lv[:, l] = xy
            if l == 0:
                # OpenCV's test of the final position behind the loop, then rule 5
                alive = np.flatnonzero(status == 1)
                f = xy[alive] - HALF
                okf, ipf = _in_range(f, w, h, W)
                status[alive[~okf]] = 0
                alive, f, ipf = alive[okf], f[okf], ipf[okf]
                if alive.size:
                    resid = np.abs(_interp(_padded(pJ[0], PAD), ipf, _weights(f, ipf), 9, W, PAD) - Iw0[alive]).sum((1, 2))
                    assert resid.max() <= W * W * 8160 < 1 << 24
                    err[alive] = resid.astype(F32) / F32(32 * W * W)
                    restaged[alive] = _outside(ipf, blk0[alive], W)
    return {"xy": xy, "status": status, "err": err, "min_eig": meig, "iterations": iters, "levels": lv, "nl": nl, "resid_restaged": restaged}


def err_of(res, flags):
    return res["min_eig"] if flags & GET_MIN_EIGENVALS else res["err"]


def residual_brute_force(prev, nxt, p, q, W=21):
    """rule 5 once more for window W, by plain Python loops with scalar arithmetic and a reflection written out again (a loop per
    index): the residual of start point p (level-0 window of `prev`) at the returned point q in `nxt`.  Shares nothing with track() but
    numpy's float32."""
    h, w = prev.shape

    def fold(i, n):
        if n == 1:
            return 0
        while i < 0 or i >= n:
            i = -i if i < 0 else 2 * n - 2 - i
        return i

    def at(img, x, y):
        return int(img[fold(y, h), fold(x, w)])

    def corner(c):
        f = F32(c) - F32((W - 1) // 2)
        i = int(np.floor(f))
        return i, f - F32(i)

    def wts(a, b):
        w00, w01, w10 = (int(np.rint((ONE - a) * (ONE - b) * SC)), int(np.rint(a * (ONE - b) * SC)), int(np.rint((ONE - a) * b * SC)))
        return w00, w01, w10, 16384 - w00 - w01 - w10

    (ix, a), (iy, b) = corner(p[0]), corner(p[1])
    (jx, c), (jy, d) = corner(q[0]), corner(q[1])
    wi, wj = wts(a, b), wts(c, d)
    total = 0
    for y in range(W):
        for x in range(W):
            iv = (at(prev, ix + x, iy + y) * wi[0] + at(prev, ix + x + 1, iy + y) * wi[1] + at(prev, ix + x, iy + y + 1) * wi[2] +
                  at(prev, ix + x + 1, iy + y + 1) * wi[3] + 256) >> 9
            jv = (at(nxt, jx + x, jy + y) * wj[0] + at(nxt, jx + x + 1, jy + y) * wj[1] + at(nxt, jx + x, jy + y + 1) * wj[2] +
                  at(nxt, jx + x + 1, jy + y + 1) * wj[3] + 256) >> 9
            total += abs(jv - iv)
    return F32(total) / F32(32 * W * W)


# ---- the cases of the GPU tests (test_lk_options_cpu.py and test_lk_window_cpu.py assert what they reach) ----------------------------------
# per window the smallest frames with each level count; at 15 one frame at most 16 pixels high, and at 31 one smaller than the window (every
# tap reflected, more than one fold).  40 x 30 has ONE level at 15 -- its second level would be 20 x 15, and 15 <= 15 stops the pyramid -- so
# 40 x 32 (20 x 16) stands for the two-level pyramid there.
GPU_SIZES = {21: [(360, 200), (240, 144), (130, 80), (40, 30)], 31: [(360, 256), (240, 144), (130, 80), (40, 30), (24, 20)],
             15: [(360, 200), (240, 144), (130, 80), (40, 32), (40, 30), (40, 16)]}
GPU_LEVELS = {21: [4, 3, 2, 1], 31: [4, 3, 2, 1, 1], 15: [4, 4, 3, 2, 1, 1]}
MOTION = (9.0, -4.0)                                          # the "9-pixel motion" of the option cases (content moves by this)
COMBINED = dict(max_level=2, max_iter=8, eps=0.03, min_eig=1e-3)
OPTION_CASES = ([("max_level_%d" % v, dict(max_level=v)) for v in (0, 1, 2)] + [("max_iter_%d" % v, dict(max_iter=v)) for v in (1, 2, 100)] +
                [("eps_%g" % v, dict(eps=v)) for v in (0.0, 0.3, 10.0)] + [("min_eig_%g" % v, dict(min_eig=v)) for v in (0.0, 1e-3, 1.0)] +
                [("combined", COMBINED)])
JUMP_OPTIONS = (dict(max_iter=1), dict(max_level=0), dict(max_level=1, max_iter=3))   # what reaches resid_restaged on jump_pair() at 21
# start points 8 px above the 4-level frame: most of the window lies outside the image, where the derivatives are zero, and what is left gives
# 0 < minEig < 1e-4 with D >= FLT_EPSILON -- the windows the default threshold rejects and min_eig_threshold = 0 tracks (window 21)
WEAK_POINTS = np.asarray([(x, -7.75) for x in (238.25, 241.25, 244.25, 268.25, 271.25, 274.25)], F32)


def pair(w, h):
    """(prev, next) of lk_edges.frames(w, h): the scene moves by about (1.3, -0.7)"""
    import lk_edges as E
    f = E.frames(w, h, 2)
    return f[0], f[1]


def moved_pair(w=360, h=200):
    """a pair whose content moves by MOTION: too far for level 0 alone, so max_level separates"""
    import lk_edges as E
    import synth
    base = E.frames(w, h, 1)[0]
    return base, np.ascontiguousarray(synth.shifted(base, *MOTION), np.uint8)


def grid(w, h, n=64):
    """about n points on a jittered grid, 2 px inside the frame"""
    k = max(int(round(np.sqrt(n * w / h))), 1)
    m = max(n // k, 1)
    rng = np.random.default_rng(w * 31 + h)
    xs, ys = np.meshgrid(np.linspace(2, w - 3, k), np.linspace(2, h - 3, m))
    p = np.stack([xs.ravel(), ys.ravel()], 1) + rng.uniform(-0.5, 0.5, (k * m, 2))
    return p.astype(F32)


def points(w, h):
    """the points of a main case at window 21: the grid and lk_edges.boundary_cases (edges, corners and plain points)"""
    import lk_edges as E
    return np.concatenate([grid(w, h), E.boundary_cases(w, h)[0]]).astype(F32)


def window_points(w, h, W):
    """the points of a main case at window W: the grid and lk_edges.edge_cases"""
    import lk_edges as E
    return np.concatenate([grid(w, h), E.edge_cases(w, h, W)[0]]).astype(F32)


def on_moved_pair(name):
    """max_level, max_iter and the combined case run on the moved pair: it needs its pyramid, and a few of its points run into the cap of 30"""
    return name.startswith(("max_level", "max_iter")) or name == "combined"


def option_inputs(name):
    """(prev, next, pts) of an option case on the 4-level frame of window 21: the moved pair (on_moved_pair) or the ordinary one"""
    w, h = GPU_SIZES[21][0]
    prev, nxt = moved_pair(w, h) if on_moved_pair(name) else pair(w, h)
    return prev, nxt, np.concatenate([points(w, h), WEAK_POINTS]) if name.startswith("min_eig") else points(w, h)


def _special_guesses(centre):
    sp = np.asarray([np.nan, np.inf, -np.inf, 1e30, -1e30, -0.0], F32)
    spec = np.asarray([(v, centre[1]) for v in sp] + [(centre[0], v) for v in sp] + [(a, b) for a in sp for b in sp], F32)
    return np.tile(np.asarray([centre], F32), (len(spec), 1)), spec


def guesses(w, h, prev_pts, nl):
    """-> {name: (pts, guess)} of the initial-flow cases at window 21 on a w x h frame with nl levels (truth: the scene moves by (1.3, -0.7))"""
    import lk_edges as E
    rng = np.random.default_rng(5 * w + h)
    g = grid(w, h)
    truth = g + F32([1.3, -0.7])
    out = {"truth_pm3": (g, (truth + rng.uniform(-3, 3, g.shape)).astype(F32)), "guess_is_prev": (prev_pts, prev_pts.copy())}
    # the far side of the frame: the block has to follow the guess, not the previous point
    out["far_side"] = (g, np.stack([F32(w - 1) - g[:, 0], F32(h - 1) - g[:, 1]], 1).astype(F32))
    # both sides of each boundary of the top level's range [-21, w_L) x [-21, h_L), the other coordinate at the centre
    L = nl - 1
    wl, hl = level_sizes(w, h)[1][L]
    centre = (F32(w * 0.5 + 0.25), F32(h * 0.5 - 0.25))
    edge = []
    for axis, n_l in ((0, wl), (1, hl)):
        for v in E.edge_values(L, n_l).values():
            p = list(centre)
            p[axis] = v
            edge.append(p)
    edge = np.asarray(edge, F32)
    out["top_level_edges"] = (np.tile(np.asarray([centre], F32), (len(edge), 1)), edge)
    # a guess whose top-level block (origin floor(guess 2^-L - 10) - 5, 32 x 32) crosses the image border on each side, the window inside the range
    s = F32(2.0 ** L)
    cross = np.asarray([[F32(6.5) * s, centre[1]], [F32(wl - 8.25) * s, centre[1]], [centre[0], F32(5.75) * s], [centre[0], F32(hl - 7.5) * s],
                        [F32(-3.5) * s, F32(-2.25) * s], [F32(wl + 4.5) * s, F32(hl + 3.25) * s]], F32)
    out["block_across_border"] = (np.tile(np.asarray([centre], F32), (len(cross), 1)), cross)
    out["specials"] = _special_guesses(centre)
    return out


def window_guesses(w, h, W):
    """-> {name: (pts, guess)} of the initial-flow cases on window W's 4-level frame (truth: the scene moves by (1.3, -0.7)): the truth
    +- 3, the far side of the frame, top-level blocks across the image border, and special values"""
    nl, sizes = level_sizes(w, h, W)
    rng = np.random.default_rng(5 * w + h + W)
    g = grid(w, h)
    truth = g + F32([1.3, -0.7])
    out = {"truth_pm3": (g, (truth + rng.uniform(-3, 3, g.shape)).astype(F32))}
    out["far_side"] = (g, np.stack([F32(w - 1) - g[:, 0], F32(h - 1) - g[:, 1]], 1).astype(F32))
    L = nl - 1
    wl, hl = sizes[L]
    s, hf = F32(2.0 ** L), float(half(W))
    centre = (F32(w * 0.5 + 0.25), F32(h * 0.5 - 0.25))
    # the top-level block has origin floor(c) - 5 for the window corner c = guess 2^-L - half, and side LKJR: c chosen so that the block
    # crosses each border (left, right, top, bottom, two corners), the window inside the range
    jr = geometry(W)["LKJR"]
    corners = [(1.5, None), (wl - jr + 8.75, None), (None, 2.25), (None, hl - jr + 7.5), (-8.5, -7.25), (wl - 3.5, hl - 2.75)]
    cross = np.asarray([[centre[0] if cx is None else F32(cx + hf) * s, centre[1] if cy is None else F32(cy + hf) * s] for cx, cy in corners], F32)
    out["block_across_border"] = (np.tile(np.asarray([centre], F32), (len(cross), 1)), cross)
    out["specials"] = _special_guesses(centre)
    return out


def jump_pair():
    """a frame pair of lk_segments' JUMP clip and points whose final window leaves the staged block (resid_restaged): pair 3 -> 4, where the
    motion reverses by 41 pixels"""
    import lk_segments as S
    frames, pts, _ = S.make_set("jump_640", n=120)
    return frames[3], frames[4], pts
