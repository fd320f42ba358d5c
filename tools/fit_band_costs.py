"""Development helper: least-squares fit of the per-tile cost model of the weighted XCD bands (csrc/vstab_warp_bands.hpp) to the
per-workgroup durations tools/wg_timeline.py saved (QDUMP=file.npz), and the per-XCD table of such a dump.
usage: python tools/fit_band_costs.py <dump.npz> even|weighted [library]     (4K headline geometry, identity rotation, as wg_timeline.py
runs it; weighted: the bands of the build that made the dump -- lib/libvstab.so, or the library named, whose cost constants may differ)
Every workgroup is one tile of the schedule: a tall 64 x 32 tile (done whole, or as two half-height tiles when its box is over the LDS
budget) or a half-height 64 x 16 tile of a band's tail; dead or live by the kernel's rule (tests/dead_tiles.py); a live tile's staged box
from the exact map (tests/layouts.py tile_boxes).  Model: duration = dead | live constant per tile kind + slope * staged 8 x 2 blocks."""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dead_tiles as D
import layouts
import oracle

dump, kind = np.load(sys.argv[1]), sys.argv[2]
w, h, rwb, lds_kb, tail = 3840, 2160, 8, 40, 0.5
K = oracle.get_preset_camera(4, w, h)
Ko, (cw, ch) = oracle.get_output_camera(K, w, h)
p = oracle.map_params(K, Ko, np.eye(3))
s = layouts.tile_schedule(cw, ch, rwb, lds_kb, tail)
if kind == "weighted":
    import importlib
    if len(sys.argv) > 3:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import devlib
        lib = devlib.load(sys.argv[3]).lib
    else:
        lib = importlib.import_module("video-annotator_amd").lib
    u32p, ip, fp = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_float)
    lib.vstabx_band_costs.argtypes = [fp, ctypes.c_int] + [ctypes.c_int] * 5 + [u32p, ctypes.c_int]
    lib.vstabx_weighted_bands.argtypes = [ctypes.c_int] * 4 + [ctypes.c_double, u32p, ctypes.c_int, ip]
    n = -(-ch // 16)
    cost, out, pf = np.zeros(n, np.uint32), np.zeros(19, np.int32), np.ascontiguousarray(p, np.float32)
    assert lib.vstabx_band_costs(pf.ctypes.data_as(fp), 0, w, h, cw, ch, 16, cost.ctypes.data_as(u32p), n) == 0
    assert lib.vstabx_weighted_bands(cw, ch, rwb, lds_kb, tail, cost.ctypes.data_as(u32p), n, out.ctypes.data_as(ip)) == 0
    s = dict(tiles_x=int(out[17]), band_y=[int(v) for v in out[:9]], split_y=[int(v) for v in out[9:17]], grid=int(out[18]))
live, _ = layouts.block_tiles(s, rwb)
tile_of = {b: (x0, ys, rows) for b, x0, ys, rows in live}
mx, my, _, _ = D.exact_map(p, np.arange(cw)[None, :], np.arange(ch)[:, None])
boxes = {th: layouts.tile_boxes(mx, my, w, h, th, planar=False, block_w=8) for th in (32, 16)}
dead = {th: D.rule(p, cw, ch, w, h, th) for th in (32, 16)}
cap = lds_kb * 256 - 8
blk, dur = dump["blk"], dump["end"] - dump["start"]
rows_, feats = [], []   # features: dead tall, dead half, live tall, live tall done as two halves, live half, blocks
for b, d in zip(blk, dur):
    x0, ys, th = tile_of[int(b)]
    f = np.zeros(6)
    if th == 32 and ys % 32 == 0 and dead[32][ys // 32, x0 // 64]:
        f[0] = 1
    elif th == 16 and dead[16][ys // 16, x0 // 64]:
        f[1] = 1
    elif th == 32:
        # a tall tile of a band that starts on an odd half-row is not on the 32-row grid of `boxes`: use its two halves' boxes
        if ys % 32 == 0:
            bx = boxes[32][(ys // 32, x0 // 64)]
            split = bx[2] * bx[3] > cap
        else:
            split = False
        halves = [boxes[16][(r, x0 // 64)] for r in (ys // 16, ys // 16 + 1) if (r, x0 // 64) in boxes[16]]
        if split:
            f[3] = 1
            f[5] = sum(v[2] * v[3] for v in halves) / 16.0
        else:
            f[2] = 1
            f[5] = (boxes[32][(ys // 32, x0 // 64)][2] * boxes[32][(ys // 32, x0 // 64)][3] if ys % 32 == 0 else sum(v[2] * v[3] for v in halves)) / 16.0
    else:
        f[4] = 1
        bx = boxes[16][(ys // 16, x0 // 64)]
        f[5] = bx[2] * bx[3] / 16.0
    feats.append(f)
A, y = np.array(feats), np.array(dur)
coef, *_ = np.linalg.lstsq(A, y, rcond=None)
res = y - A @ coef
names = ["dead tall", "dead half", "live tall", "live tall as two halves", "live half", "per staged 8x2 block"]
print(f"{len(y)} workgroups; tiles by kind: " + ", ".join(f"{n} {int(c)}" for n, c in zip(names[:5], A[:, :5].sum(axis=0))))
for n, c in zip(names, coef):
    print(f"  {n:28s} {c:8.4f} us")
print(f"  residual rms {np.sqrt((res ** 2).mean()):.3f} us; mean measured: " + ", ".join(f"{n} {y[A[:, i] > 0].mean():.2f}" for i, n in enumerate(names[:5]) if (A[:, i] > 0).any()))
print("per XCD: workgroups, last end (us), sum of workgroup durations (us), modelled sum")
for k in range(8):
    m = (blk & 7) == k
    print(f"  xcd {k}: {int(m.sum()):5d}  {dump['end'][m].max():6.2f}  {dur[m].sum():8.1f}  {(A[m] @ coef).sum():8.1f}")
ends = np.array([dump["end"][(blk & 7) == k].max() for k in range(8)])
print(f"XCD end times: min {ends.min():.2f} max {ends.max():.2f} spread {ends.max() - ends.min():.2f} us")
