"""Driver for profiles/colour_warp_4k.txt (development helper): the COLOUR instantiation of k_warp_fused (vstab_warp_nv12_colour with
(BT709, LIMITED)) beside the default kernel (vstab_warp_nv12_ex), at the 4K config-3 size (3840 x 2160 NV12 -> 3524 x 1999) with the
preset fisheye camera and its output camera, rotation rodrigues(0.01, -0.02, 0.015), random frames, map modes 0 and 5, BGR8 and NV12
through BGR.
usage: python tools/colour_time.py <root of a built tree> [launches] [rounds]
In one process, `rounds` (default 3) times in turn: the default kernel, the colour kernel with (CVTCOLOR, LIMITED) -- which must launch
the default kernel and reproduce its bytes --, the colour kernel with (BT709, LIMITED).  Each `launches` (default 20) launches after 3
warm-up ones, each launch's own start / end stamps through vstab_time_next_launch.  Prints the median, min and max of every repeat in
microseconds and one checksum per variant (the first two must agree).  The default kernel's instruction stream is the parent commit's
(tools/asm_kernel_diff.py), so its repeats stand for the parent's kernel."""
import importlib
import os
import sys
import zlib

import numpy as np
import torch

root = os.path.abspath(sys.argv[1])
launches = int(sys.argv[2]) if len(sys.argv) > 2 else 20
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
sys.path.insert(0, root)
vs = importlib.import_module("video-annotator_amd")
assert os.path.dirname(os.path.dirname(vs.LIB_PATH)) == os.path.join(root, "video-annotator_amd"), vs.LIB_PATH
w, h = 3840, 2160
K = vs.get_preset_camera(4, w, h)
Ko, (cw, ch) = vs.get_output_camera(K, w, h)
assert (cw, ch) == (3524, 1999)
a, b, c = 0.01, -0.02, 0.015
th = float(np.sqrt(a * a + b * b + c * c))
Kx = np.array([[0, -c, b], [c, 0, -a], [-b, a, 0]]) / th
R = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
p = vs.map_params(K, Ko, R)
nf = 4
torch.manual_seed(0)
frames = [torch.randint(0, 256, (h * 3 // 2, w), dtype=torch.uint8, device="cuda") for _ in range(nf)]


def timed(run, n):
    t = []
    for i in range(3 + n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        vs.time_next_launch(e0, e1)
        run(i)
        torch.cuda.synchronize()
        if i >= 3:
            t.append(e0.elapsed_time(e1) * 1000.0)
    return t


def checksum(out):
    crc = 0
    for t in (out,) if torch.is_tensor(out) else out:
        crc = zlib.crc32(t.cpu().numpy().tobytes(), crc)
    return crc


for mode in (vs.MAP_CREATEMAP_CL, vs.MAP_CREATEMAP_CL_OPENCL):
    for fmt, tag in ((vs.OUT_BGR8, "bgr8"), (vs.OUT_NV12, "nv12")):
        out = torch.zeros((ch, cw, 3), dtype=torch.uint8, device="cuda") if fmt == vs.OUT_BGR8 else vs.nv12_out_planes(cw, ch)
        runs = (("default (vstab_warp_nv12_ex)", lambda i: vs.warp_nv12(frames[i % nf], p, cw, ch, mode, fmt, out=out)),
                ("colour CVTCOLOR limited", lambda i: vs.warp_nv12_colour(frames[i % nf], p, cw, ch, vs.COLOUR_CVTCOLOR, vs.RANGE_LIMITED, mode, fmt, out=out)),
                ("colour BT709 limited", lambda i: vs.warp_nv12_colour(frames[i % nf], p, cw, ch, vs.COLOUR_BT709, vs.RANGE_LIMITED, mode, fmt, out=out)))
        crcs, meds = [], {}
        for rep in range(rounds):
            for name, run in runs:
                t = timed(run, launches)
                meds.setdefault(name, []).append(float(np.median(t)))
                print(f"mode {mode} {tag} round {rep} {name:30s} n={len(t):3d} median {np.median(t):8.1f} us  min {min(t):8.1f}  max {max(t):8.1f}", flush=True)
                if rep == 0:
                    run(0)
                    torch.cuda.synchronize()
                    crcs.append(checksum(out))
        print(f"mode {mode} {tag} checksums default {crcs[0]:08x} CVTCOLOR {crcs[1]:08x} BT709 {crcs[2]:08x}", flush=True)
        assert crcs[0] == crcs[1], "(CVTCOLOR, LIMITED) must reproduce the default kernel's bytes"
        print(f"mode {mode} {tag} medians of the rounds: " + "; ".join(f"{n}: {np.median(m):.1f} us (rounds {min(m):.1f} .. {max(m):.1f})" for n, m in meds.items()), flush=True)
print(f"{root}: {launches} launches per repeat, {rounds} rounds, {w}x{h} -> {cw}x{ch}")
