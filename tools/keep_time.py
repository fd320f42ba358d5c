"""Driver for profiles/keep_edges_4k.txt (development helper): the keep-edge warp (vstab_warp_nv12_keep, k_warp_keep) beside its sibling, the
border warp's tile under BORDER_CONSTANT (vstab_warp_nv12_border, k_warp_border<..., 0>: the same tile and the same map, and it stores every
pixel), at the 4K config-3 shape (3840 x 2160 NV12 -> 3524 x 1999, preset camera 4 and its output camera, rotation
rodrigues(0.01, -0.02, 0.015), random frames), map modes 0 and 5, BGR and plane-wise.
usage: python tools/keep_time.py <root of a built tree> [launches]
In one process, three times in turn: the sibling, the keep warp in place, the keep warp with a separate prev -- each `launches` (default
20) launches after 3 warm-up ones, each launch's own start / end stamps through vstab_time_next_launch.  vstab_warp_nv12_ex (k_warp_fused /
k_warp_planar) is timed once per shape for orientation.  Prints the median, min and max of every repeat in microseconds, the kept share of
each plane, and one checksum over the outputs.  Under `rocprofv3 --kernel-trace --stats` the profiler's own file has the per-kernel times
(in-place and separate launches are one kernel there); under `rocprofv3 --pmc` pass a small `launches`."""
import importlib
import os
import sys
import zlib

import numpy as np
import torch

root = os.path.abspath(sys.argv[1])
launches = int(sys.argv[2]) if len(sys.argv) > 2 else 20
sys.path.insert(0, root)
vs = importlib.import_module("video-annotator_amd")
assert os.path.dirname(os.path.dirname(vs.LIB_PATH)) == os.path.join(root, "video-annotator_amd"), vs.LIB_PATH
w, h = 3840, 2160
K = vs.get_preset_camera(4, w, h)
Ko, (cw, ch) = vs.get_output_camera(K, w, h)
a, b, c = 0.01, -0.02, 0.015
th = float(np.sqrt(a * a + b * b + c * c))
Kx = np.array([[0, -c, b], [c, 0, -a], [-b, a, 0]]) / th
R = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
p = vs.map_params(K, Ko, R)
nf = 4
torch.manual_seed(0)
frames = [torch.randint(0, 256, (h * 3 // 2, w), dtype=torch.uint8, device="cuda") for _ in range(nf)]


def kept(mx, my, sw, sh):
    """Share of kept samples of float map planes over a sw x sh plane (the quantisation of include/vstab.h, finite maps)."""
    X, Y = torch.round(mx * 32).to(torch.int64) >> 5, torch.round(my * 32).to(torch.int64) >> 5
    return 1.0 - float(((X >= 0) & (X <= sw - 2) & (Y >= 0) & (Y <= sh - 2)).float().mean())


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
    print(f"{name:44s} n={len(t):3d} median {np.median(t):9.1f} us  min {min(t):9.1f}  max {max(t):9.1f}")


crc = 0
for mode in (vs.MAP_CREATEMAP_CL, vs.MAP_CREATEMAP_CL_OPENCL):
    mx, my = vs.create_map(p, cw, ch, "cuda", mode)
    mx, my = torch.nan_to_num(mx, nan=-1e6), torch.nan_to_num(my, nan=-1e6)
    print(f"mode {mode}: kept share luma / BGR {kept(mx, my, w, h):.4f}, chroma {kept(mx[::2, ::2] * 0.5, my[::2, ::2] * 0.5, w // 2, h // 2):.4f}")
    for fmt, tag in ((vs.OUT_BGR8, "bgr"), (vs.OUT_NV12_PLANAR, "planar")):
        mk = (lambda: torch.randint(0, 256, (ch, cw, 3), dtype=torch.uint8, device="cuda")) if fmt == vs.OUT_BGR8 else \
             (lambda: tuple(torch.randint(0, 256, t.shape, dtype=torch.uint8, device="cuda") for t in vs.nv12_out_planes(cw, ch)))
        out, prev = mk(), mk()
        line(f"mode {mode} {tag:6s} vstab_warp_nv12_ex (orientation)", timed(lambda i: vs.warp_nv12(frames[i % nf], p, cw, ch, mode, fmt, out=out), launches))
        for rep in range(3):
            line(f"mode {mode} {tag:6s} rep {rep} border CONSTANT (sibling)",
                 timed(lambda i: vs.warp_nv12_border(frames[i % nf], p, cw, ch, mode, fmt, vs.BORDER_CONSTANT, out=out), launches))
            line(f"mode {mode} {tag:6s} rep {rep} keep in place", timed(lambda i: vs.warp_nv12_keep(frames[i % nf], p, cw, ch, out, mode, fmt, out=out), launches))
            line(f"mode {mode} {tag:6s} rep {rep} keep separate prev", timed(lambda i: vs.warp_nv12_keep(frames[i % nf], p, cw, ch, prev, mode, fmt, out=out), launches))
        for t in (out,) if fmt == vs.OUT_BGR8 else out:
            crc = zlib.crc32(t.cpu().numpy().tobytes(), crc)
print(f"{root}: {launches} launches per repeat, {w}x{h} -> {cw}x{ch}, checksum {crc:08x}")
