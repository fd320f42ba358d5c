"""Driver for profiles/distort_resample_4k.txt (development helper): the cubic, Lanczos and bilinear-border tile kernels at the 4K config-3
shape (3840 x 2160 NV12 -> 3524 x 1999, preset camera 4 and its output camera, map mode 1, identity rotation, random frames), one launch
sequence per process, meant to run under `rocprofv3 --kernel-trace --stats`.
usage: python tools/distort_resample_time.py <root of a built tree> sib | dist | dist0
  sib    the undistorted entry points (vstab_warp_nv12_cubic / _cubic_border / _lanczos4 / _lanczos4_border / _border): kernel mode 1
  dist   vstab_warp_nv12_dist_ex with D = (-0.02, 0.004, -0.001, 0.0002): kernel mode 9
  dist0  vstab_warp_nv12_dist_ex with D = 0: kernel mode 9 on the map, boxes, taps and bytes of mode 1 (the instructions' cost alone)
Each of the ten kernels (cubic and Lanczos: CONSTANT and REFLECT_101; bilinear: REFLECT_101; BGR and plane-wise) is launched 5 + 50 times,
the kernels in turn.  Prints one checksum over all outputs."""
import importlib
import os
import sys
import zlib

import numpy as np
import torch

root, what = os.path.abspath(sys.argv[1]), sys.argv[2]
sys.path.insert(0, root)
vs = importlib.import_module("video-annotator_amd")
assert os.path.dirname(os.path.dirname(vs.LIB_PATH)) == os.path.join(root, "video-annotator_amd"), vs.LIB_PATH
w, h, mode, D = 3840, 2160, 1, (0.0, 0.0, 0.0, 0.0) if what == "dist0" else (-0.02, 0.004, -0.001, 0.0002)
K = vs.get_preset_camera(4, w, h)
Ko, (cw, ch) = vs.get_output_camera(K, w, h)
p = vs.map_params(K, Ko, np.eye(3))
nf = 4
torch.manual_seed(0)
frames = [torch.randint(0, 256, (h * 3 // 2, w), dtype=torch.uint8, device="cuda") for _ in range(nf)]
bgr = torch.zeros((ch, cw, 3), dtype=torch.uint8, device="cuda")
planes = vs.nv12_out_planes(cw, ch)
CONSTANT, REFLECT_101 = vs.BORDER_CONSTANT, vs.BORDER_REFLECT_101
runs = []
for fmt, out in ((vs.OUT_BGR8, bgr), (vs.OUT_NV12_PLANAR, planes)):
    for resample, border in ((vs.RESAMPLE_CUBIC, CONSTANT), (vs.RESAMPLE_CUBIC, REFLECT_101), (vs.RESAMPLE_LANCZOS4, CONSTANT),
                             (vs.RESAMPLE_LANCZOS4, REFLECT_101), (vs.RESAMPLE_DEFAULT, REFLECT_101)):
        if what != "sib":
            runs.append(lambda i, r=resample, b=border, f=fmt, o=out: vs.warp_nv12_dist_ex(frames[i % nf], p, D, cw, ch, mode, r, b, f, out=o))
        elif resample == vs.RESAMPLE_DEFAULT:
            runs.append(lambda i, b=border, f=fmt, o=out: vs.warp_nv12_border(frames[i % nf], p, cw, ch, mode, f, b, out=o))
        elif border == CONSTANT:
            fn = vs.warp_nv12_cubic if resample == vs.RESAMPLE_CUBIC else vs.warp_nv12_lanczos4
            runs.append(lambda i, fn=fn, f=fmt, o=out: fn(frames[i % nf], p, cw, ch, mode, f, out=o))
        else:
            fn = vs.warp_nv12_cubic_border if resample == vs.RESAMPLE_CUBIC else vs.warp_nv12_lanczos4_border
            runs.append(lambda i, fn=fn, b=border, f=fmt, o=out: fn(frames[i % nf], p, cw, ch, mode, f, b, out=o))
crc = 0
for i in range(55):
    for run in runs:
        run(i)
        if i == 54:
            torch.cuda.synchronize()
            for t in (bgr,) + tuple(planes):
                crc = zlib.crc32(t.cpu().numpy().tobytes(), crc)
torch.cuda.synchronize()
print(f"{what} {root}: {len(runs)} kernels x 55 launches, {w}x{h} -> {cw}x{ch}, checksum {crc:08x}")
