"""Isolated timing of the LK tracker at 4K (development helper): run under rocprofv3 --kernel-trace --stats and
read k_lk_track's (or, with options, k_lk_track_opt's) average; also prints the wall time of the stateless call (which includes the
pyramids).  Options: --max-level, --max-iter, --eps, --min-eig, --err (ask for the error measure), --points N, --calls N."""
import argparse, importlib, os, sys, time
import numpy as np, torch
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R); sys.path.insert(0, os.path.join(R, "tests"))
vs = importlib.import_module("video-annotator_amd")
import bench
ap = argparse.ArgumentParser()
ap.add_argument("--max-level", type=int, default=3)
ap.add_argument("--max-iter", type=int, default=30)
ap.add_argument("--eps", type=float, default=0.01)
ap.add_argument("--min-eig", type=float, default=1e-4)
ap.add_argument("--err", action="store_true")
ap.add_argument("--points", type=int, default=200)
ap.add_argument("--calls", type=int, default=30)
ap.add_argument("--win", type=int, default=21, help="the tracker's window: 15 and 31 run k_lk_track_win (vstab_pyr_lk_win)")
a = ap.parse_args()
plain = (a.max_level, a.max_iter, a.eps, a.min_eig) == (3, 30, 0.01, 1e-4) and not a.err and a.win == 21
w, h = 3840, 2160
K = vs.get_preset_camera(4, w, h)
frames, _ = bench.shaky_ring(torch, torch.device("cuda"), w, h, K, 6, seed=0)
grays = [f[:h] for f in frames]
pts = vs.good_features(grays[0], a.points)
print("features", len(pts), "kernel", "k_lk_track_win (window %d)" % a.win if a.win != 21 else
      "k_lk_track" if plain or (not a.err and (a.max_iter, a.eps, a.min_eig) == (30, 0.01, 1e-4)) else "k_lk_track_opt")


def call():
    if plain:
        return vs.pyr_lk(grays[0], grays[1], pts)
    if a.win != 21:
        return vs.pyr_lk_win(grays[0], grays[1], pts, a.win, a.max_level, a.max_iter, a.eps, a.min_eig, want_err=a.err)[:2]
    return vs.pyr_lk_ex(grays[0], grays[1], pts, a.max_level, a.max_iter, a.eps, a.min_eig, want_err=a.err)[:2]


for i in range(3):
    call()
torch.cuda.synchronize()
t0 = time.perf_counter()
for i in range(a.calls):
    out, st = call()
torch.cuda.synchronize()
print("pyr_lk call %.1f us, tracked %d" % ((time.perf_counter() - t0) / a.calls * 1e6, int(st.sum())))
