"""Driver for profiles/rs_resample_4k.txt (development helper): the cubic and Lanczos tile kernels with a rotation per output row
(vstab_warp_nv12_rs_ex) and their siblings without one, at the 4K config-3 shape (3840 x 2160 NV12 -> 3524 x 1999, preset camera 4 and its
output camera, map mode 1, identity rotation, random frames).
usage: python tools/rs_resample_time.py <root of a built tree> sib | rs | rsd [launches]
  sib   vstab_warp_nv12_cubic / _cubic_border / _lanczos4 / _lanczos4_border: one rotation (runs on a tree without the per-row kernels)
  rs    vstab_warp_nv12_rs_ex with the last row's rotation rodrigues(0.002, -0.003, 0.001): k_warp_cubic_rs / k_warp_lanczos4_rs<1, ...>
  rsd   the same through a calibrated lens, D = (-0.02, 0.004, -0.001, 0.0002), and INTER_LINEAR too: ...<11, ...>, k_warp_border<11, ...>
Each kernel (CONSTANT and REFLECT_101; BGR and plane-wise) is launched 5 + `launches` (default 30) times, the kernels in turn; each
launch's own start / end stamps through vstab_time_next_launch.  Prints the median, min and max per kernel in microseconds, and one checksum
over all outputs.  Under `rocprofv3 --pmc` pass a small `launches`: the counters come from the profiler's own file."""
import importlib
import os
import sys
import zlib

import numpy as np
import torch

root, what = os.path.abspath(sys.argv[1]), sys.argv[2]
launches = int(sys.argv[3]) if len(sys.argv) > 3 else 30
sys.path.insert(0, root)
vs = importlib.import_module("video-annotator_amd")
assert os.path.dirname(os.path.dirname(vs.LIB_PATH)) == os.path.join(root, "video-annotator_amd"), vs.LIB_PATH
w, h, mode = 3840, 2160, 1
K = vs.get_preset_camera(4, w, h)
Ko, (cw, ch) = vs.get_output_camera(K, w, h)
p = vs.map_params(K, Ko, np.eye(3))
a, b, c = 0.002, -0.003, 0.001       # the read-out rotation, first order is all a timing needs
rb = vs.map_params(K, Ko, np.array([[1, -c, b], [c, 1, -a], [-b, a, 1]], np.float64))[8:]
D = (-0.02, 0.004, -0.001, 0.0002)
nf = 4
torch.manual_seed(0)
frames = [torch.randint(0, 256, (h * 3 // 2, w), dtype=torch.uint8, device="cuda") for _ in range(nf)]
bgr = torch.zeros((ch, cw, 3), dtype=torch.uint8, device="cuda")
planes = vs.nv12_out_planes(cw, ch)
CONSTANT, REFLECT_101 = vs.BORDER_CONSTANT, vs.BORDER_REFLECT_101
NAMES = {vs.RESAMPLE_DEFAULT: "linear", vs.RESAMPLE_CUBIC: "cubic", vs.RESAMPLE_LANCZOS4: "lanczos4"}
runs = []
for fmt, out in ((vs.OUT_BGR8, bgr), (vs.OUT_NV12_PLANAR, planes)):
    for resample in (vs.RESAMPLE_CUBIC, vs.RESAMPLE_LANCZOS4) + ((vs.RESAMPLE_DEFAULT,) if what == "rsd" else ()):
        for border in (CONSTANT, REFLECT_101):
            name = f"{what:3s} {NAMES[resample]:8s} {'bgr' if fmt == vs.OUT_BGR8 else 'planar':6s} {'CONSTANT' if border == CONSTANT else 'REFLECT_101'}"
            if what != "sib":
                runs.append((name, lambda i, r=resample, b=border, f=fmt, o=out: vs.warp_nv12_rs_ex(frames[i % nf], p, cw, ch, rb, D if what == "rsd" else None,
                                                                                                     mode, r, b, f, out=o)))
            elif border == CONSTANT:
                fn = vs.warp_nv12_cubic if resample == vs.RESAMPLE_CUBIC else vs.warp_nv12_lanczos4
                runs.append((name, lambda i, fn=fn, f=fmt, o=out: fn(frames[i % nf], p, cw, ch, mode, f, out=o)))
            else:
                fn = vs.warp_nv12_cubic_border if resample == vs.RESAMPLE_CUBIC else vs.warp_nv12_lanczos4_border
                runs.append((name, lambda i, fn=fn, b=border, f=fmt, o=out: fn(frames[i % nf], p, cw, ch, mode, f, b, out=o)))
times = {name: [] for name, _ in runs}
crc = 0
for i in range(5 + launches):
    for name, run in runs:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        vs.time_next_launch(e0, e1)
        run(i)
        torch.cuda.synchronize()
        if i >= 5:
            times[name].append(e0.elapsed_time(e1) * 1000.0)
        if i == 4 + launches:
            for t in (bgr,) + tuple(planes):
                crc = zlib.crc32(t.cpu().numpy().tobytes(), crc)
for name, t in times.items():
    print(f"{name:40s} n={len(t):3d} median {np.median(t):9.1f} us  min {min(t):9.1f}  max {max(t):9.1f}")
print(f"{what} {root}: {len(runs)} kernels x {5 + launches} launches, {w}x{h} -> {cw}x{ch}, checksum {crc:08x}")
