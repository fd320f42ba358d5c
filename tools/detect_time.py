"""Run the corner detectors at 4K and 1080p a few times (for rocprofv3 --kernel-trace --stats).
usage: detect_time.py [--lib LIB.so] [--n N] [--fused-only]   -- LIB: another build of the library (tools/devlib.py), for parent / branch runs"""
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
a = ap.parse_args()
if a.lib:
    import devlib
    vs = devlib.load(a.lib)
else:
    vs = importlib.import_module("video-annotator_amd")
for w, h in ((3840, 2160), (1920, 1080)):
    g = torch.from_numpy(np.ascontiguousarray(synth.luma(41, w, h, rects=400))).cuda()
    for det in (vs.DETECTOR_AUTO,) if a.fused_only else (vs.DETECTOR_AUTO, vs.DETECTOR_TWO_PASS):
        info = {}
        for _ in range(a.n):
            c = vs.good_features(g, detector=det, info=info)
        torch.cuda.synchronize()
        print(w, h, "detector", info["detector_used"], "corners", len(c), hashlib.sha1(np.ascontiguousarray(c).tobytes()).hexdigest()[:12], flush=True)
