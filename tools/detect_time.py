"""Run the corner detectors at 4K and 1080p a few times (for rocprofv3 --kernel-trace --stats).
usage: detect_time.py [--lib LIB.so] [--n N] [--fused-only] [--mask {full,overlay,roi}] [--harris [--k K]] [--alternations K] [--block B] [--gradient G]
   LIB: another build of the library (tools/devlib.py), for parent / branch runs
   --mask: K alternations of N unmasked detections (k_corners_fused) and N detections under the mask (k_corners_fused_masked,
           vstab_good_features_mask) per size, in one process: `full` is non-zero everywhere, `overlay` is zero on a box over 9 % of the frame
           grown by 16 px (the lower left), `roi` leaves a window of a tenth of the fused detector's tiles.
   --harris: K alternations (rounds) of N detections with the minimum eigenvalue and N with the Harris response (vstab_good_features_harris,
           k_corners_fused_harris) per size, in one process; with --mask both run under the mask (k_corners_fused_masked and
           k_corners_fused_harris_masked).  tools/kernel_medians.py <dir> k_corners rounds gives the figures per round.
   --block B: N one-pass detections and N dense maps with goodFeaturesToTrack's blockSize B per size (5, 7: vstab_good_features_block and
           vstab_min_eig_block, k_corners_fused_block<B> and k_corner_response_block<B>; 3: the entry points and kernels without a
           block, so that the figures of one session stand beside each other); with --harris the Harris response, with --mask under the mask.
           One block size per run; a trace names the kernels with their sizes (k_corners_fused_block<5, 3>), and so does tools/kernel_medians.py.
   --gradient G: with --block B, goodFeaturesToTrack's gradientSize G beside it (5, 7: vstab_good_features_grad and vstab_min_eig_grad or
           vstab_corner_harris_grad, k_corners_fused_block<B, G> and k_corner_response_block<B, G>; 3 or none: what --block B alone runs).
   tools/kernel_medians.py <dir> turns the kernel trace into medians per kernel and grid."""
import argparse, hashlib, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import importlib
import numpy as np
import torch
import synth
ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=None)
ap.add_argument("--n", type=int, default=20)
ap.add_argument("--fused-only", action="store_true")
ap.add_argument("--mask", choices=("full", "overlay", "roi"), default=None)
ap.add_argument("--harris", action="store_true")
ap.add_argument("--k", type=float, default=0.04)
ap.add_argument("--alternations", type=int, default=3)
ap.add_argument("--block", type=int, default=None)
ap.add_argument("--gradient", type=int, default=None)
a = ap.parse_args()
if a.gradient is not None and a.block is None:
    ap.error("--gradient goes with --block")
grad = a.gradient not in (None, 3)
if a.lib:
    import devlib
    vs = devlib.load(a.lib)
else:
    vs = importlib.import_module("video-annotator_amd")


def make_mask(kind, w, h):
    m = np.full((h, w), 255, np.uint8)
    if kind == "overlay":     # the box of the 640 x 360 clip (rows 250..339, columns 20..259: 9.4 % of the frame) scaled, grown by 16 px
        s = w / 640.0
        m[max(int(250 * s) - 16, 0):min(int(340 * s) + 16, h), max(int(20 * s) - 16, 0):min(int(260 * s) + 16, w)] = 0
    if kind == "roi":         # a centred window of sqrt(1/10) of either side: a tenth of the 64 x 31 tiles
        m[:] = 0
        rw, rh = int(w * 0.1 ** 0.5), int(h * 0.1 ** 0.5)
        m[(h - rh) // 2:(h - rh) // 2 + rh, (w - rw) // 2:(w - rw) // 2 + rw] = 255
    return m


for w, h in ((3840, 2160), (1920, 1080)):
    g = torch.from_numpy(np.ascontiguousarray(synth.luma(41, w, h, rects=400))).cuda()
    if a.block is not None:
        m = torch.from_numpy(make_mask(a.mask, w, h)).cuda() if a.mask else None
        info = {}
        for _ in range(a.n):
            if grad:
                c = vs.good_features_grad(g, m, block_size=a.block, gradient_size=a.gradient, use_harris=a.harris, k=a.k, detector=vs.DETECTOR_FUSED, info=info)
                e = vs.corner_harris_grad(g, a.block, a.gradient, a.k) if a.harris else vs.min_eig_grad(g, a.block, a.gradient)
            elif a.block != 3:
                c = vs.good_features_block(g, m, block_size=a.block, use_harris=a.harris, k=a.k, detector=vs.DETECTOR_FUSED, info=info)
                e = vs.corner_harris_block(g, a.block, a.k) if a.harris else vs.min_eig_block(g, a.block)
            elif a.harris:
                c = vs.good_features_harris(g, m, k=a.k, detector=vs.DETECTOR_FUSED, info=info)
                e = vs.corner_harris(g, a.k)
            else:
                c = vs.good_features_mask(g, m, detector=vs.DETECTOR_FUSED, info=info)
                e = vs.min_eig(g)
        torch.cuda.synchronize()
        print(w, h, "block", a.block, "gradient", a.gradient or 3, "mask", a.mask, "harris k %g" % a.k if a.harris else "minimum eigenvalue", "detector", info["detector_used"], "corners", len(c),
              hashlib.sha1(np.ascontiguousarray(c).tobytes()).hexdigest()[:12], "map", hashlib.sha1(e.cpu().numpy().tobytes()).hexdigest()[:12], flush=True)
        continue
    if a.harris:
        m = torch.from_numpy(make_mask(a.mask, w, h)).cuda() if a.mask else None
        for _ in range(a.alternations):
            for harris in (False, True):
                info = {}
                for _ in range(a.n):
                    if harris:
                        c = vs.good_features_harris(g, m, k=a.k, detector=vs.DETECTOR_FUSED, info=info)
                    else:
                        c = vs.good_features_mask(g, m, detector=vs.DETECTOR_FUSED, info=info)
                torch.cuda.synchronize()
                print(w, h, "mask", a.mask, "harris k %g" % a.k if harris else "minimum eigenvalue", "detector", info["detector_used"], "corners", len(c),
                      hashlib.sha1(np.ascontiguousarray(c).tobytes()).hexdigest()[:12], flush=True)
        continue
    if a.mask:
        mh = make_mask(a.mask, w, h)
        m = torch.from_numpy(mh).cuda()
        tiles = [(ty, tx) for ty in range(0, h, 31) for tx in range(0, w, 64)]
        live = sum(bool(mh[max(ty - 1, 0):ty + 32, max(tx - 1, 0):tx + 65].any()) for ty, tx in tiles)
        for _ in range(a.alternations):
            for masked in (False, True):
                info = {}
                for _ in range(a.n):
                    c = vs.good_features_mask(g, m, detector=vs.DETECTOR_FUSED, info=info) if masked else vs.good_features(g, detector=vs.DETECTOR_AUTO, info=info)
                torch.cuda.synchronize()
        print(w, h, "mask", a.mask, "masked-in %.1f %%" % (100.0 * (mh != 0).mean()), "tiles that do not return early", live, "of", len(tiles),
              "detector", info["detector_used"], "corners", len(c), hashlib.sha1(np.ascontiguousarray(c).tobytes()).hexdigest()[:12], flush=True)
        continue
    for det in (vs.DETECTOR_AUTO,) if a.fused_only else (vs.DETECTOR_AUTO, vs.DETECTOR_TWO_PASS):
        info = {}
        for _ in range(a.n):
            c = vs.good_features(g, detector=det, info=info)
        torch.cuda.synchronize()
        print(w, h, "detector", info["detector_used"], "corners", len(c), hashlib.sha1(np.ascontiguousarray(c).tobytes()).hexdigest()[:12], flush=True)
