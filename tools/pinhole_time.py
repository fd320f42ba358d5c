"""Driver for profiles/pinhole_warp_4k.txt (development helper): the pinhole-lens warp (vstab_warp_nv12_pinhole: k_warp_border, k_warp_cubic_rs
and k_warp_lanczos4_rs with the MAP_RECTD_TO_RECT map) beside the kernels that serve map mode 3 without distortion (vstab_warp_nv12_border,
vstab_warp_nv12_cubic[_border], vstab_warp_nv12_lanczos4[_border]), at the 4K config-3 size (3840 x 2160 NV12 -> 3524 x 1999) with a
rect 100 -> rect 80 lens, rotation rodrigues(0.01, -0.02, 0.015), random frames: three resamplers, BORDER_CONSTANT and BORDER_REFLECT_101,
BGR and plane-wise.
usage: python tools/pinhole_time.py <root of a built tree> [launches] [rounds]
In one process, `rounds` (default 3) times in turn per kernel: the sibling; the pinhole kernel with D = (1e-30, 0, 0, 0, 0), whose map is
the sibling's bit for bit (1 + 1e-30 r2 rounds to 1), so the difference is the added instructions alone; the pinhole kernel with D_M
(tests/pinhole_def.py).  Each `launches` (default 20) launches after 3 warm-up ones, each launch's own start / end stamps through
vstab_time_next_launch.  Prints the median, min and max of every repeat in microseconds and one checksum per variant (the first two must
agree).  Under `rocprofv3 --kernel-trace --stats` the profiler's own file has the per-kernel times; under `rocprofv3 --pmc` pass a small
`launches` and one round."""
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
w, h, cw, ch = 3840, 2160, 3524, 1999
K, Ko = vs.lens_camera(vs.PROJ_RECT, 100.0, w, h), vs.lens_camera(vs.PROJ_RECT, 80.0, cw, ch)
a, b, c = 0.01, -0.02, 0.015
th = float(np.sqrt(a * a + b * b + c * c))
Kx = np.array([[0, -c, b], [c, 0, -a], [-b, a, 0]]) / th
R = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
p = vs.map_params(K, Ko, R)
D_EPS, D_M = (1e-30, 0.0, 0.0, 0.0, 0.0), (-0.12, 0.02, 0.0005, -0.0004, 0.0)
MODE = vs.MAP_RECT_TO_RECT
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


def line(name, t):
    print(f"{name:58s} n={len(t):3d} median {np.median(t):9.1f} us  min {min(t):9.1f}  max {max(t):9.1f}", flush=True)


def sibling(resample, border, fmt, out):
    if resample == vs.RESAMPLE_DEFAULT:
        return lambda i: vs.warp_nv12_border(frames[i % nf], p, cw, ch, MODE, fmt, border, out=out)
    if border == vs.BORDER_CONSTANT:
        fn = vs.warp_nv12_cubic if resample == vs.RESAMPLE_CUBIC else vs.warp_nv12_lanczos4
        return lambda i: fn(frames[i % nf], p, cw, ch, MODE, fmt, out=out)
    fn = vs.warp_nv12_cubic_border if resample == vs.RESAMPLE_CUBIC else vs.warp_nv12_lanczos4_border
    return lambda i: fn(frames[i % nf], p, cw, ch, MODE, fmt, border, out=out)


def checksum(out):
    crc = 0
    for t in (out,) if torch.is_tensor(out) else out:
        crc = zlib.crc32(t.cpu().numpy().tobytes(), crc)
    return crc


for resample, rname in ((vs.RESAMPLE_DEFAULT, "linear"), (vs.RESAMPLE_CUBIC, "cubic"), (vs.RESAMPLE_LANCZOS4, "lanczos4")):
    for border, bname in ((vs.BORDER_CONSTANT, "CONSTANT"), (vs.BORDER_REFLECT_101, "REFLECT_101")):
        for fmt, tag in ((vs.OUT_BGR8, "bgr"), (vs.OUT_NV12_PLANAR, "planar")):
            out = torch.zeros((ch, cw, 3), dtype=torch.uint8, device="cuda") if fmt == vs.OUT_BGR8 else vs.nv12_out_planes(cw, ch)
            runs = (("sibling (mode 3)", sibling(resample, border, fmt, out)),
                    ("pinhole D_eps", lambda i: vs.warp_nv12_pinhole(frames[i % nf], p, D_EPS, cw, ch, MODE, resample, border, fmt, out=out)),
                    ("pinhole D_M", lambda i: vs.warp_nv12_pinhole(frames[i % nf], p, D_M, cw, ch, MODE, resample, border, fmt, out=out)))
            crcs = []
            for rep in range(rounds):
                for name, run in runs:
                    line(f"{rname:8s} {bname:11s} {tag:6s} round {rep} {name}", timed(run, launches))
                    if rep == 0:
                        run(0)
                        torch.cuda.synchronize()
                        crcs.append(checksum(out))
            print(f"{rname:8s} {bname:11s} {tag:6s} checksums sibling {crcs[0]:08x} D_eps {crcs[1]:08x} D_M {crcs[2]:08x}", flush=True)
            assert crcs[0] == crcs[1], "D_eps must reproduce the sibling's bytes"
print(f"{root}: {launches} launches per repeat, {rounds} rounds, {w}x{h} -> {cw}x{ch}")
