"""Full-range content for the 10-bit warps and maximum-contrast content for the tracker (test infrastructure only, a plain module).

The 10-bit kernels carry value-range arguments in their comments (video-annotator_amd/csrc/vstab_device10.hpp, vstab_warp_planar.hip):
  saturating add   the luma + chroma sum of a conversion needs 33 bits; __builtin_elementwise_add_sat stands in for the oracle's
                   64-bit sum.  It engages only for bright luma on a chroma site with U near the top (luma 938 needs U = 1023);
  dark luma        max(y - 64, 0), folded into the chroma term as max(y, 64);
  fp16 clamp       a binary16 accumulator can end at 1023.5 or 1024 from taps of 1023; it must come out as 1023, not 0.
The synthetic frames of the older tests (8-bit limited range x 4) never reach any of them.  p010_extreme_frame does, and reach()
counts -- exactly, on the oracle's map -- how often a parameter set makes each branch decide, so that a test can commit to it.

The tracker keeps its LK sums in int32 pieces whose bounds are argued in vstab_lk.hip.  contrast_* build 0 / 255 content
(checkerboards, hard steps, saturated rectangles) whose window sums pass 2^31, which the smooth synthetic frames never do."""
import numpy as np

import oracle
import synth
from test_p010_cpu import CY, CUB, CUG, CVG, CVR

INT_MAX = 2 ** 31 - 1


# ---- 10-bit content ----------------------------------------------------------------------------------------------------------
KINDS = ("noise", "dark", "white", "near_white", "blue_bright", "corner_00", "corner_0f", "corner_f0", "corner_ff", "sat_white", "dark_blue")


def p010_extreme_frame(seed, w, h, block=16, junk=True):
    """Full-range P010 planes: 10-bit noise over 0..1023 in luma and chroma, overlaid with flat blocks (block x block luma
    pixels, block / 2 chroma sites square) of every kind in KINDS -- luma 0..63, luma 1023 and just below, luma >= 950 on chroma
    sites with U >= 980, the four (U, V) corners flat in both channels, luma 1023 on U = 1023 and dark luma on U = 1023.  Each kind
    takes at least one block when the frame has len(KINDS) blocks.  -> (y16, uv16, y10, uv10) like test_p010_cpu.p010_frame."""
    rng = np.random.default_rng(seed)
    y10 = rng.integers(0, 1024, (h, w), dtype=np.uint16)
    uv10 = rng.integers(0, 1024, (h // 2, w), dtype=np.uint16)
    U, V = uv10[:, 0::2], uv10[:, 1::2]
    bx, by = -(-w // block), -(-h // block)
    kinds = np.concatenate([np.arange(len(KINDS)), rng.integers(0, len(KINDS), max(0, bx * by - len(KINDS)))])[:bx * by]
    rng.shuffle(kinds)
    cb = block // 2
    for k, kind in enumerate(kinds):
        name = KINDS[kind]
        ys, xs = slice((k // bx) * block, (k // bx + 1) * block), slice((k % bx) * block, (k % bx + 1) * block)
        cs, cx = slice((k // bx) * cb, (k // bx + 1) * cb), slice((k % bx) * cb, (k % bx + 1) * cb)
        if name == "dark":
            y10[ys, xs] = rng.integers(0, 64)
        elif name == "white":
            y10[ys, xs] = 1023
        elif name == "near_white":
            y10[ys, xs] = rng.choice([1021, 1022])
        elif name == "blue_bright":
            y10[ys, xs] = rng.integers(950, 1024, y10[ys, xs].shape)
            U[cs, cx] = rng.integers(980, 1024, U[cs, cx].shape)
        elif name.startswith("corner"):
            U[cs, cx] = 1023 if name[-2] == "f" else 0
            V[cs, cx] = 1023 if name[-1] == "f" else 0
        elif name == "sat_white":
            y10[ys, xs], U[cs, cx] = 1023, 1023
        elif name == "dark_blue":
            y10[ys, xs], U[cs, cx] = rng.integers(0, 64), 1023
    uv10[:, 0::2], uv10[:, 1::2] = U, V
    lo = rng.integers(0, 64, (h, w), dtype=np.uint16) if junk else 0
    lo2 = rng.integers(0, 64, (h // 2, w), dtype=np.uint16) if junk else 0
    return (y10 << 6) | lo, (uv10 << 6) | lo2, y10, uv10


def stretched_clip(seed, K, w, h, n, sigma=0.004):
    """synth.shaky_clip with its luma stretched over the whole 10-bit range (30 -> 0, 225 -> 1023: the rectangles' levels end at
    black and white), full-range chroma that moves with the frame, two bits of detail and junk below: -> (P010 frames (1.5 h, w)
    uint16, rotations).  The tracker sees the top 8 bits, a contrast-stretched copy of the clip: it still finds its corners."""
    frames8, rots = synth.shaky_clip(seed, K, w, h, n, sigma)
    rng = np.random.default_rng(seed + 77)
    out = []
    xx = np.arange(w // 2)[None, :]
    yy = np.arange(h // 2)[:, None]
    for k, f in enumerate(frames8):
        y10 = np.clip(np.rint((f[:h].astype(np.float64) - 30.0) * (1023.0 / 195.0)) + rng.integers(-2, 3, (h, w)), 0, 1023).astype(np.uint16)
        uv10 = np.empty((h // 2, w), np.uint16)
        uv10[:, 0::2] = np.clip(np.rint(512 + 620 * np.sin(xx / 23.0 + k * 0.3) * np.cos(yy / 31.0)), 0, 1023)
        uv10[:, 1::2] = np.clip(np.rint(512 + 620 * np.cos(xx / 37.0 - yy / 19.0 + k * 0.2)), 0, 1023)
        wide = np.concatenate([y10, uv10]) << 6
        out.append(wide | rng.integers(0, 64, wide.shape, dtype=np.uint16))
    return out, rots


# ---- the exact reach of a parameter set ----------------------------------------------------------------------------------------
def _quantise(mx, my):
    """rint(32 * map) as cv::remap's fixed point: -> (X, Y, fx, fy, ok)."""
    ax = np.asarray(mx, np.float32).astype(np.float64) * 32.0
    ay = np.asarray(my, np.float32).astype(np.float64) * 32.0
    ok = (np.abs(ax) < 2 ** 31) & (np.abs(ay) < 2 ** 31)
    sx = np.where(ok, np.rint(np.where(ok, ax, 0)), 0).astype(np.int64)
    sy = np.where(ok, np.rint(np.where(ok, ay, 0)), 0).astype(np.int64)
    return sx >> 5, sy >> 5, sx & 31, sy & 31, ok


def _fp16_acc(taps, fx, fy):
    """The binary16 blend's accumulator before rounding and clamping: four fused multiply-adds, taps 00, 01, 10, 11 (float64 of the
    product and sum is exact; one rounding to binary16 = the fused multiply-add)."""
    ws = ((32 - fx) * (32 - fy), fx * (32 - fy), (32 - fx) * fy, fx * fy)
    acc = np.zeros(fx.shape, np.float16)
    for t, k in zip(taps, ws):
        acc = (t.astype(np.float64) * (k / 1024.0) + acc.astype(np.float64)).astype(np.float16)
    return acc


def _taps(plane, X, Y, inside, border):
    """The four taps (values) of every footprint of a (h, w) plane; outside the plane = border."""
    h, w = plane.shape
    out = []
    for dy in (0, 1):
        for dx in (0, 1):
            xx, yy = X + dx, Y + dy
            ok = inside & (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
            out.append((np.where(ok, plane[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)], border), ok))
    return out


def reach_bgr(y10, uv10, mx, my):
    """BGR16 output (vstab_warp_p010, vstab_warp_p010_planes): over every tap inside the source of every output pixel --
    sat: conversions whose luma + chroma sum exceeds INT_MAX in some channel (where the saturating add decides);
    dark: taps with luma < 64;  clamp: binary16 accumulators (pixel x channel) >= 1023.5 before the clamp."""
    h, w = y10.shape
    X, Y, fx, fy, ok = _quantise(mx, my)
    inside = ok & (X < w) & (X + 1 >= 0) & (Y < h) & (Y + 1 >= 0)
    Yv = y10.astype(np.int64)
    U = np.repeat(np.repeat(uv10[:, 0::2].astype(np.int64) - 512, 2, 0), 2, 1)[:h, :w]
    V = np.repeat(np.repeat(uv10[:, 1::2].astype(np.int64) - 512, 2, 0), 2, 1)[:h, :w]
    yy = np.maximum(Yv - 64, 0) * CY
    sums = np.stack([yy + (1 << 19) + CUB * U, yy + (1 << 19) + CVG * V + CUG * U, yy + (1 << 19) + CVR * V])
    sat_px = (sums > INT_MAX).any(0)
    bgr = np.clip(sums >> 20, 0, 1023)
    sat = dark = 0
    taps = {c: [] for c in range(3)}
    for (yv, tok), dy, dx in zip(_taps(Yv, X, Y, inside, 0), (0, 0, 1, 1), (0, 1, 0, 1)):
        cy, cx = np.clip(Y + dy, 0, h - 1), np.clip(X + dx, 0, w - 1)
        sat += int((tok & sat_px[cy, cx]).sum())
        dark += int((tok & (yv < 64)).sum())
        for c in range(3):
            taps[c].append(np.where(tok, bgr[c][cy, cx], 0))
    clamp = sum(int((inside & (_fp16_acc(taps[c], fx, fy) >= 1023.5)).sum()) for c in range(3))
    return {"sat": sat, "dark": dark, "clamp": clamp}


def reach_planar(y10, uv10, mx, my):
    """Plane-wise output (vstab_warp_p010_planar): binary16 accumulators >= 1023.5 before the clamp, luma and chroma (U and V)."""
    X, Y, fx, fy, ok = _quantise(mx, my)
    h, w = y10.shape
    inside = ok & (X < w) & (X + 1 >= 0) & (Y < h) & (Y + 1 >= 0)
    luma = int((inside & (_fp16_acc([t for t, _ in _taps(y10.astype(np.int64), X, Y, inside, 64)], fx, fy) >= 1023.5)).sum())
    cmx, cmy = oracle.chroma_maps(mx, my)
    X, Y, fx, fy, ok = _quantise(cmx, cmy)
    ch, cw = uv10.shape[0], uv10.shape[1] // 2
    inside = ok & (X < cw) & (X + 1 >= 0) & (Y < ch) & (Y + 1 >= 0)
    chroma = 0
    for c in (0, 1):
        plane = uv10[:, c::2].astype(np.int64)
        chroma += int((inside & (_fp16_acc([t for t, _ in _taps(plane, X, Y, inside, 512)], fx, fy) >= 1023.5)).sum())
    return {"clamp_y": luma, "clamp_c": chroma}


# ---- the GPU tests' parameter sets -----------------------------------------------------------------------------------------------
# name: (source w, h, map mode, rotation, rotation of the last row or None, output camera scale and size (None: the default), frame seed).  Mode 0 / 1 / 5 on aligned
# planes take the LDS-tiled kernel of vstab_warp_p010 (scale 0.25: boxes over the LDS budget, gather_pixel10); modes 2 - 4 the direct
# kernel.  The same sets serve vstab_warp_p010_planes and vstab_warp_p010_planar where those take the mode.
SETS = {
    "m0_640": (640, 360, 0, (0.02, -0.03, 0.01), None, None, 41),
    "m0_640_rs": (640, 360, 0, (0.01, -0.02, 0.005), (0.05, -0.01, -0.03), None, 42),
    "m1_320": (320, 180, 1, (0.05, -0.1, 0.2), None, None, 43),
    "m1_320_rs": (320, 180, 1, (0.05, -0.1, 0.2), (0.07, -0.09, 0.18), None, 44),
    "split_1280": (1280, 720, 0, (0.0, 0.0, 0.0), None, (0.25, 448, 252), 45),
    "split_roll_1280": (1280, 720, 0, (0.0, 0.0, 1.5708), None, (1.0, 1100, 700), 46),
    "m2_320": (320, 180, 2, (0.05, -0.1, 0.2), None, None, 47),
    "m3_320": (320, 180, 3, (0.05, -0.1, 0.2), (0.02, 0.03, -0.1), None, 48),
    "m4_320": (320, 180, 4, (0.05, -0.1, 0.2), None, None, 49),
}
LENS = {1: ((1, 150.0), (0, 110.0)), 2: ((1, 150.0), (1, 165.0)), 3: ((0, 100.0), (0, 80.0)), 4: ((0, 100.0), (1, 300.0))}


def set_params(name):
    """-> (y16, uv16, y10, uv10, params, rot_bottom or None, dw, dh, mode) of a SETS entry (mode 5 sets reuse the mode 0 cameras)."""
    w, h, mode, rv, rvb, scale, seed = SETS[name]
    y16, uv16, y10, uv10 = p010_extreme_frame(seed, w, h)
    if mode in LENS:
        (ip, ifov), (op, ofov) = LENS[mode]
        dw, dh = 301, 171
        Ki, Ko = oracle.lens_camera(ip, ifov, w, h), oracle.lens_camera(op, ofov, dw, dh)
    else:
        Ki = oracle.get_preset_camera(4, w, h)
        Ko, (dw, dh) = oracle.get_output_camera(Ki, w, h) if scale is None else oracle.get_output_camera(Ki, w, h, scale=scale[0])
        if scale is not None:
            dw, dh = scale[1:]
    p = oracle.map_params(Ki, Ko, oracle.rodrigues(rv))
    rb = None if rvb is None else oracle.map_params(Ki, Ko, oracle.rodrigues(rvb))[8:]
    return y16, uv16, y10, uv10, p, rb, dw, dh, mode


def set_map(name):
    y16, uv16, y10, uv10, p, rb, dw, dh, mode = set_params(name)
    return oracle.create_map_rs(p, rb, dw, dh, mode) if rb is not None else oracle.create_map_ex(p, dw, dh, mode)


# ---- maximum-contrast luma for the tracker ---------------------------------------------------------------------------------------
def checkerboard(w, h, cell, phase=(0, 0)):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.where((((xx + phase[0]) // cell) + ((yy + phase[1]) // cell)) % 2 == 0, 255, 0).astype(np.uint8)


def steps(w, h, seed):
    """Hard 0 <-> 255 steps: vertical and horizontal bands of random widths (2..9 px) xor'ed, and a diagonal half-plane."""
    rng = np.random.default_rng(seed)
    cuts = np.cumsum(rng.integers(2, 10, w))
    band_x = (np.searchsorted(cuts, np.arange(w), side="right") % 2).astype(bool)
    cuts = np.cumsum(rng.integers(2, 10, h))
    band_y = (np.searchsorted(cuts, np.arange(h), side="right") % 2).astype(bool)
    img = band_x[None, :] ^ band_y[:, None]
    yy, xx = np.mgrid[0:h, 0:w]
    img[(xx + 2 * yy) > (w + h) * 0.9] ^= True
    return np.where(img, 255, 0).astype(np.uint8)


def saturated_rects(w, h, seed, n=None):
    """0 / 255 rectangles (3..24 px) on a 0 / 255 background, each drawn in the opposite level of what lies under its corner."""
    rng = np.random.default_rng(seed)
    img = np.where(rng.random() < 0.5, 0, 255) * np.ones((h, w), np.uint8)
    for _ in range(n or max(20, w * h // 300)):
        rw, rh = rng.integers(3, 25, 2)
        x, y = rng.integers(-4, w - 2), rng.integers(-4, h - 2)
        x0, y0 = max(x, 0), max(y, 0)
        img[y0:y + rh, x0:x + rw] = 255 - img[min(y0, h - 1), min(x0, w - 1)]
    return img.astype(np.uint8)


def contrast_image(kind, w, h, seed=0):
    if kind.startswith("checker"):
        return checkerboard(w, h, int(kind[-1]), (seed % 3, seed % 2))
    if kind == "steps":
        return steps(w, h, seed)
    return saturated_rects(w, h, seed)


CONTRAST = ("checker1", "checker2", "checker3", "checker4", "steps", "rects")


def contrast_pair(kind, w, h, seed, shift):
    """(prev, next, points): next = prev moved by a sub-pixel `shift` (bilinear, synth.shifted); points on corners of prev (the oracle's
    detector, minimum distance 3), on grid positions, and within 2 px of every image edge -- some just outside."""
    prev = contrast_image(kind, w, h, seed)
    nxt = synth.shifted(prev, *shift)
    rng = np.random.default_rng(seed + 5)
    c = oracle.good_features(prev, max_corners=60, quality=0.01, min_distance=3.0)
    m = 24
    edge = np.concatenate([np.stack([rng.uniform(-1.5, 2.0, m), rng.uniform(0, h - 1, m)], 1),
                           np.stack([rng.uniform(w - 3.0, w + 0.5, m), rng.uniform(0, h - 1, m)], 1),
                           np.stack([rng.uniform(0, w - 1, m), rng.uniform(-1.5, 2.0, m)], 1),
                           np.stack([rng.uniform(0, w - 1, m), rng.uniform(h - 3.0, h + 0.5, m)], 1)])
    grid = np.stack([rng.uniform(3, w - 4, 40), rng.uniform(3, h - 4, 40)], 1)
    return prev, nxt, np.concatenate([c, edge, grid]).astype(np.float32)
