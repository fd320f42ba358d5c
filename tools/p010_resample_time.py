"""Driver for profiles/p010_resample_4k.txt (development helper): the cubic and Lanczos kernels of the plane-wise 10-bit warp
(vstab_warp_p010_planar_ex) beside their 8-bit plane-wise twins (vstab_warp_nv12_rs_ex, VSTAB_OUT_NV12_PLANAR) and beside the bilinear
10-bit warp (vstab_warp_p010_planar), at the 4K shape: 3840 x 2160 -> 3524 x 1999, preset camera 4 and its output camera, map mode 5,
identity rotation, random frames.
usage: python tools/p010_resample_time.py <root of a built tree> [launches]
Sources come from rings of distinct frames larger than the 256 MiB Infinity Cache (12 P010 frames of 23.7 MiB, 24 NV12 frames of 11.9 MiB),
so no launch finds its source in cache from the launch before.  Every kernel (both resamplers x CONSTANT and REFLECT_101 x one rotation and a
rotation per row, at 10 and at 8 bits; the bilinear 10-bit warp with and without a rotation per row) is launched 5 + `launches` (default
30) times, the kernels in turn; each launch's own start / end stamps through vstab_time_next_launch.  Prints the median, min and max per
kernel in microseconds, the ratio of each 10-bit median to its 8-bit twin's, and one checksum over the last outputs."""
import importlib
import os
import sys
import zlib

import numpy as np
import torch

root = os.path.abspath(sys.argv[1])
launches = int(sys.argv[2]) if len(sys.argv) > 2 else 30
sys.path.insert(0, root)
vs = importlib.import_module("video-annotator_amd")
assert os.path.dirname(os.path.dirname(vs.LIB_PATH)) == os.path.join(root, "video-annotator_amd"), vs.LIB_PATH
w, h, mode = 3840, 2160, vs.MAP_CREATEMAP_CL_OPENCL
K = vs.get_preset_camera(4, w, h)
Ko, (cw, ch) = vs.get_output_camera(K, w, h)
p = vs.map_params(K, Ko, np.eye(3))
a, b, c = 0.002, -0.003, 0.001       # the read-out rotation, first order is all a timing needs
rb = vs.map_params(K, Ko, np.array([[1, -c, b], [c, 1, -a], [-b, a, 1]], np.float64))[8:]
N10, N8 = 12, 24
torch.manual_seed(0)
frames10 = [torch.randint(-32768, 32768, (h * 3 // 2, w), dtype=torch.int16, device="cuda") for _ in range(N10)]
frames8 = [torch.randint(0, 256, (h * 3 // 2, w), dtype=torch.uint8, device="cuda") for _ in range(N8)]
assert N10 * frames10[0].numel() * 2 > 256 << 20 and N8 * frames8[0].numel() > 256 << 20
out10 = (torch.zeros((ch, cw), dtype=torch.int16, device="cuda"), torch.zeros(((ch + 1) // 2, 2 * ((cw + 1) // 2)), dtype=torch.int16, device="cuda"))
out8 = vs.nv12_out_planes(cw, ch)
CONSTANT, REFLECT_101 = vs.BORDER_CONSTANT, vs.BORDER_REFLECT_101
NAMES = {vs.RESAMPLE_CUBIC: "cubic", vs.RESAMPLE_LANCZOS4: "lanczos4"}
runs = []
for rot in (None, rb):
    how = "per row" if rot is not None else "one rot"
    runs.append((f"10 linear   CONSTANT    {how}", lambda i, r=rot: vs.warp_p010_planar(frames10[i % N10][:h], frames10[i % N10][h:], p, cw, ch, r, mode,
                                                                                       vs.BLEND_EXACT, out_y=out10[0], out_uv=out10[1])))
    for resample in (vs.RESAMPLE_CUBIC, vs.RESAMPLE_LANCZOS4):
        for border in (CONSTANT, REFLECT_101):
            tail = f"{NAMES[resample]:8s} {'CONSTANT   ' if border == CONSTANT else 'REFLECT_101'} {how}"
            runs.append(("10 " + tail, lambda i, r=rot, s=resample, m=border: vs.warp_p010_planar_ex(frames10[i % N10][:h], frames10[i % N10][h:], p, cw, ch, r,
                                                                                                     mode, s, m, out_y=out10[0], out_uv=out10[1])))
            runs.append((" 8 " + tail, lambda i, r=rot, s=resample, m=border: vs.warp_nv12_rs_ex(frames8[i % N8], p, cw, ch, r, None, mode, s, m,
                                                                                                 vs.OUT_NV12_PLANAR, out=out8)))
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
for t in tuple(out10) + tuple(out8):
    crc = zlib.crc32(t.cpu().numpy().tobytes(), crc)
for name, t in times.items():
    line = f"{name:44s} n={len(t):3d} median {np.median(t):9.1f} us  min {min(t):9.1f}  max {max(t):9.1f}"
    if name.startswith("10 ") and " 8 " + name[3:] in times:
        line += f"  x{np.median(t) / np.median(times[' 8 ' + name[3:]]):.2f} of its 8-bit twin"
    print(line)
print(f"{root}: {len(runs)} kernels x {5 + launches} launches, {w}x{h} -> {cw}x{ch}, checksum {crc:08x}")
