"""The tracker's options (include/vstab.h, "Tracker options") restated in numpy: OpenCV 4.5's CPU LKTrackerInvoker with
maxLevel, the criteria's count and epsilon, minEigThreshold, OPTFLOW_USE_INITIAL_FLOW, err and OPTFLOW_LK_GET_MIN_EIGENVALS, in this project's
arithmetic -- exact integer sums converted once, the float32 operations in the order of oracle/vstab_oracle.c (vo_lk_point).  No GPU here, and
no call of oracle.pyr_lk: test_lk_options_cpu.py holds this file against it at default options.  A plain module, imported by the tests.

    1  levels      min(levels of the frame, max_level + 1); a level is what it always was (oracle.pyr_down, oracle.scharr)
    2  start       with USE_INITIAL_FLOW the top level L starts the next-image estimate at guess * float32(2^-L); the previous image's side
                   (window, derivatives, matrix, the previous point's range test) does not see the guess
    3  iterations  at most max_iter; a level ends on (double)dx dx + (double)dy dy <= (double)eps (double)eps; the oscillation rule keeps 0.01
    4  rejection   minEig < float32(min_eig_threshold) or D < FLT_EPSILON
    5  err         level 0, status still 1 behind the final range test: f = next - 10, origin floor(f), weights of its fraction,
                   S = sum over the window of |DESCALE(J interpolated, 9) - Iw|, err = float32(S) / float32(14112); status 0: err 0
    6  min eig     with GET_MIN_EIGENVALS err is minEig of the finest level whose matrix was formed, rejected or not; none: 0

All points of a call advance together, level by level and iteration by iteration (arrays of n x 21 x 21); a point's arithmetic never reads
another point's.  track() returns both err modes at once and, beside the definition, one fact about the KERNEL's bookkeeping that a test wants
to reach on purpose: whether the residual's window lies outside the 32 x 32 next-image block the iterations left staged (`resid_restaged`)."""
import numpy as np

import lk_edges as E
import lk_segments as S
import oracle

LKW, HALF = S.LKW, S.HALF
LKJR, LKJM = S.LKJR, S.LKJM
USE_INITIAL_FLOW, GET_MIN_EIGENVALS = 4, 8
F32 = np.float32
ONE, SC, FLT_SCALE = F32(1.0), F32(16384.0), F32(1.0 / (1 << 20))
PAD = LKW + 3          # a window origin lies in [-21, n): taps reach from -21 to n + 21
_WY, _WX = np.mgrid[0:LKW, 0:LKW]


def _reflect101(i, n):
    i = np.asarray(i, np.int64).copy()
    if n == 1:
        return np.zeros_like(i)
    while True:
        bad = (i < 0) | (i >= n)
        if not bad.any():
            return i
        i = np.where(i < 0, -i, np.where(i >= n, 2 * n - 2 - i, i))


def _padded(img):
    """the image under BORDER_REFLECT_101, PAD pixels to every side, int64"""
    h, w = img.shape
    return img[np.ix_(_reflect101(np.arange(-PAD, h + PAD), h), _reflect101(np.arange(-PAD, w + PAD), w))].astype(np.int64)


def _in_range(q, w, h):
    """the reference's range test of a window origin floor(q): NaN, infinities and everything outside int fail (its conversion gives INT_MIN);
    -> (ok, origin int64 (0 where not ok))"""
    with np.errstate(invalid="ignore"):
        fin = np.isfinite(q).all(1) & (np.abs(q) < 2.0 ** 31).all(1)
    ip = S._floor_i(np.where(fin[:, None], q, 0))
    ok = fin & (ip[:, 0] >= -LKW) & (ip[:, 0] < w) & (ip[:, 1] >= -LKW) & (ip[:, 1] < h)
    return ok, np.where(ok[:, None], ip, 0)


def _weights(q, ip):
    a, b = q[:, 0] - ip[:, 0].astype(F32), q[:, 1] - ip[:, 1].astype(F32)
    w00 = np.rint((ONE - a) * (ONE - b) * SC).astype(np.int64)
    w01 = np.rint(a * (ONE - b) * SC).astype(np.int64)
    w10 = np.rint((ONE - a) * b * SC).astype(np.int64)
    return [x[:, None, None] for x in (w00, w01, w10, 16384 - w00 - w01 - w10)]


def _interp(P, ip, wts, shift):
    """DESCALE(bilinear taps of the padded plane P at the windows of origin ip, shift): (n, 21, 21) int64"""
    Y, X = ip[:, 1, None, None] + PAD + _WY, ip[:, 0, None, None] + PAD + _WX
    return (P[Y, X] * wts[0] + P[Y, X + 1] * wts[1] + P[Y + 1, X] * wts[2] + P[Y + 1, X + 1] * wts[3] + (1 << (shift - 1))) >> shift


def levels_of(w, h, max_level=3):
    return min(S.level_sizes(w, h)[0], max_level + 1)


def _block(c, w, h):
    """the kernel's lk_block_origin for a next-image block around the window corner c (n, 2): origin floor(c) - 5 where c lies in
    (-22, w) x (-22, h), else None (as a huge negative origin, for which "window outside the block" holds)"""
    with np.errstate(invalid="ignore"):
        ok = (c[:, 0] > -(LKW + 1)) & (c[:, 0] < w) & (c[:, 1] > -(LKW + 1)) & (c[:, 1] < h)
    return np.where(ok[:, None], S._floor_i(np.where(ok[:, None], c, 0)) - LKJM, -(1 << 30))


def _outside(ip, blk):
    return (ip[:, 0] < blk[:, 0]) | (ip[:, 1] < blk[:, 1]) | (ip[:, 0] + LKW + 1 > blk[:, 0] + LKJR) | (ip[:, 1] + LKW + 1 > blk[:, 1] + LKJR)


def track(prev, nxt, pts, max_level=3, max_iter=30, eps=0.01, min_eig=1e-4, guess=None):
    """-> dict: xy (n, 2) float32, status (n,) uint8, err (n,) float32 (rule 5), min_eig (n,) float32 (rule 6), iterations (n, 4) int,
    levels (n, 4, 2) float32 (where each point stood after level l, as oracle.pyr_lk_trace: NaN for absent levels), nl, and
    resid_restaged (n,) bool.  guess: (n, 2) float32 -- USE_INITIAL_FLOW."""
    prev, nxt = np.ascontiguousarray(prev, np.uint8), np.ascontiguousarray(nxt, np.uint8)
    pts = np.ascontiguousarray(pts, F32).reshape(-1, 2)
    n = pts.shape[0]
    h0, w0 = prev.shape
    nl = levels_of(w0, h0, max_level)
    pI, pJ = E.pyramid(prev)[:nl], E.pyramid(nxt)[:nl]
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
    Iw0 = np.zeros((n, LKW, LKW), np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for l in range(nl - 1, -1, -1):
            h, w = pI[l].shape
            ls = F32(2.0 ** -l)
            xy = start * ls if l == nl - 1 else xy * F32(2.0)                                   # rule 2
            if l == 1:
                blk0 = _block(xy * F32(2.0) - HALF, w0, h0)
            q = pts * ls - HALF
            ok, ip = _in_range(q, w, h)
            if l == 0:
                status[~ok] = 0
                if nl == 1:
                    blk0 = np.where(ok[:, None], ip - LKJM, blk0) if guess is None else _block(xy - HALF, w, h)
            idx = np.flatnonzero(ok)
            if idx.size:
                PI, PJ = _padded(pI[l]), _padded(pJ[l])
                der = np.pad(oracle.scharr(pI[l]).astype(np.int64), ((PAD, PAD), (PAD, PAD), (0, 0)))
                wts = _weights(q[idx], ip[idx])
                Iw = _interp(PI, ip[idx], wts, 9)
                Ix, Iy = _interp(der[..., 0], ip[idx], wts, 14), _interp(der[..., 1], ip[idx], wts, 14)
                if l == 0:
                    Iw0[idx] = Iw
                A11 = (Ix * Ix).sum((1, 2)).astype(F32) * FLT_SCALE
                A12 = (Ix * Iy).sum((1, 2)).astype(F32) * FLT_SCALE
                A22 = (Iy * Iy).sum((1, 2)).astype(F32) * FLT_SCALE
                D = A11 * A22 - A12 * A12
                me = ((A22 + A11) - np.sqrt((A11 - A22) * (A11 - A22) + (F32(4.0) * A12) * A12)) / F32(2 * LKW * LKW)
                meig[idx] = me                                                                   # rule 6: before the rejection test
                rej = (me < thr) | (D < E.FLT_EPSILON)                                           # rule 4
                if l == 0:
                    status[idx[rej]] = 0
                keep = ~rej
                idx, Iw, Ix, Iy, A11, A12, A22 = idx[keep], Iw[keep], Ix[keep], Iy[keep], A11[keep], A12[keep], A22[keep]
                D = ONE / D[keep]
                npos = xy[idx] - HALF
                pd = np.zeros((idx.size, 2), F32)
                live = np.arange(idx.size)
                for j in range(max_iter):                                                        # rule 3
                    if live.size == 0:
                        break
                    g = idx[live]
                    iters[g, l] += 1
                    okj, inj = _in_range(npos[live], w, h)
                    if l == 0:
                        status[g[~okj]] = 0
                    live, g, inj = live[okj], g[okj], inj[okj]
                    if live.size == 0:
                        break
                    if l == 0:
                        out = _outside(inj, blk0[g])
                        blk0[g[out]] = inj[out] - LKJM
                    diff = _interp(PJ, inj, _weights(npos[live], inj), 9) - Iw[live]
                    b1 = (diff * Ix[live]).sum((1, 2)).astype(F32) * FLT_SCALE
                    b2 = (diff * Iy[live]).sum((1, 2)).astype(F32) * FLT_SCALE
                    dx = (A12[live] * b2 - A22[live] * b1) * D[live]
                    dy = (A12[live] * b1 - A11[live] * b2) * D[live]
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
                okf, ipf = _in_range(f, w, h)
                status[alive[~okf]] = 0
                alive, f, ipf = alive[okf], f[okf], ipf[okf]
                if alive.size:
                    resid = np.abs(_interp(_padded(pJ[0]), ipf, _weights(f, ipf), 9) - Iw0[alive]).sum((1, 2))
                    assert resid.max() < 1 << 24
                    err[alive] = resid.astype(F32) / F32(32 * LKW * LKW)
                    restaged[alive] = _outside(ipf, blk0[alive])
    return {"xy": xy, "status": status, "err": err, "min_eig": meig, "iterations": iters, "levels": lv, "nl": nl, "resid_restaged": restaged}


def err_of(res, flags):
    return res["min_eig"] if flags & GET_MIN_EIGENVALS else res["err"]


def residual_brute_force(prev, nxt, p, q):
    """rule 5 once more, by plain Python loops over the 441 pixels with scalar arithmetic: the residual of start point p (level-0 window of
    `prev`) at the returned point q in `nxt`.  Shares nothing with track() but numpy's float32."""
    h, w = prev.shape

    def at(img, x, y):
        return int(img[int(_reflect101([y], h)[0]), int(_reflect101([x], w)[0])])

    def corner(c):
        f = F32(c) - HALF
        i = int(np.floor(f))
        return i, f - F32(i)

    def wts(a, b):
        w00, w01, w10 = (int(np.rint((ONE - a) * (ONE - b) * SC)), int(np.rint(a * (ONE - b) * SC)), int(np.rint((ONE - a) * b * SC)))
        return w00, w01, w10, 16384 - w00 - w01 - w10

    (ix, a), (iy, b) = corner(p[0]), corner(p[1])
    (jx, c), (jy, d) = corner(q[0]), corner(q[1])
    wi, wj = wts(a, b), wts(c, d)
    total = 0
    for y in range(LKW):
        for x in range(LKW):
            iv = (at(prev, ix + x, iy + y) * wi[0] + at(prev, ix + x + 1, iy + y) * wi[1] + at(prev, ix + x, iy + y + 1) * wi[2] +
                  at(prev, ix + x + 1, iy + y + 1) * wi[3] + 256) >> 9
            jv = (at(nxt, jx + x, jy + y) * wj[0] + at(nxt, jx + x + 1, jy + y) * wj[1] + at(nxt, jx + x, jy + y + 1) * wj[2] +
                  at(nxt, jx + x + 1, jy + y + 1) * wj[3] + 256) >> 9
            total += abs(jv - iv)
    return F32(total) / F32(14112.0)


# ---- the cases of the GPU test (test_lk_options_cpu.py asserts what they reach) -----------------------------------------------------------
GPU_SIZES = [(360, 200), (240, 144), (130, 80), (40, 30)]    # 4, 3, 2 and 1 levels: the smallest frames with each level count
MOTION = (9.0, -4.0)                                          # the "9-pixel motion" of the option cases (content moves by this)


def pair(w, h):
    """(prev, next) of lk_edges.frames(w, h): the scene moves by about (1.3, -0.7)"""
    f = E.frames(w, h, 2)
    return f[0], f[1]


def moved_pair(w=360, h=200):
    """a pair whose content moves by MOTION: too far for level 0 alone, so max_level separates"""
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
    """the points of a main case: the grid and lk_edges.boundary_cases"""
    return np.concatenate([grid(w, h), E.boundary_cases(w, h)[0]]).astype(F32)


OPTION_CASES = ([("max_level_%d" % v, dict(max_level=v)) for v in (0, 1, 2)] + [("max_iter_%d" % v, dict(max_iter=v)) for v in (1, 2, 100)] +
                [("eps_%g" % v, dict(eps=v)) for v in (0.0, 0.3, 10.0)] + [("min_eig_%g" % v, dict(min_eig=v)) for v in (0.0, 1e-3, 1.0)] +
                [("combined", dict(max_level=2, max_iter=8, eps=0.03, min_eig=1e-3))])


# start points 8 px above the 4-level frame: most of the window lies outside the image, where the derivatives are zero, and what is left gives
# 0 < minEig < 1e-4 with D >= FLT_EPSILON -- the windows the default threshold rejects and min_eig_threshold = 0 tracks
WEAK_POINTS = np.asarray([(x, -7.75) for x in (238.25, 241.25, 244.25, 268.25, 271.25, 274.25)], F32)


def on_moved_pair(name):
    """max_level, max_iter and the combined case run on the moved pair: it needs its pyramid, and a few of its points run into the cap of 30"""
    return name.startswith(("max_level", "max_iter")) or name == "combined"


def option_inputs(name):
    """(prev, next, pts) of an option case on the 4-level frame: the moved pair (on_moved_pair) or the ordinary one"""
    w, h = GPU_SIZES[0]
    prev, nxt = moved_pair(w, h) if on_moved_pair(name) else pair(w, h)
    return prev, nxt, np.concatenate([points(w, h), WEAK_POINTS]) if name.startswith("min_eig") else points(w, h)


def guesses(w, h, prev_pts, nl):
    """-> {name: (pts, guess)} of the initial-flow cases on a w x h frame with nl levels (truth: the scene moves by (1.3, -0.7))"""
    rng = np.random.default_rng(5 * w + h)
    g = grid(w, h)
    truth = g + F32([1.3, -0.7])
    out = {"truth_pm3": (g, (truth + rng.uniform(-3, 3, g.shape)).astype(F32)), "guess_is_prev": (prev_pts, prev_pts.copy())}
    # the far side of the frame: the block has to follow the guess, not the previous point
    out["far_side"] = (g, np.stack([F32(w - 1) - g[:, 0], F32(h - 1) - g[:, 1]], 1).astype(F32))
    # both sides of each boundary of the top level's range [-21, w_L) x [-21, h_L), the other coordinate at the centre
    L = nl - 1
    wl, hl = S.level_sizes(w, h)[1][L]
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
    sp = np.asarray([np.nan, np.inf, -np.inf, 1e30, -1e30, -0.0], F32)
    spec = np.asarray([(v, centre[1]) for v in sp] + [(centre[0], v) for v in sp] + [(a, b) for a in sp for b in sp], F32)
    out["specials"] = (np.tile(np.asarray([centre], F32), (len(spec), 1)), spec)
    return out


def jump_pair():
    """a frame pair of lk_segments' JUMP clip and points whose final window leaves the staged block (resid_restaged): pair 3 -> 4, where the
    motion reverses by 41 pixels"""
    frames, pts, _ = S.make_set("jump_640", n=120)
    return frames[3], frames[4], pts


JUMP_OPTIONS = (dict(max_iter=1), dict(max_level=0), dict(max_level=1, max_iter=3))   # what reaches resid_restaged on jump_pair()
