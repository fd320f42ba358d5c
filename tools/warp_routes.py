#!/usr/bin/env python3
"""Which kernel serves which 8-bit NV12 warp: every servable combination called once through the public binding, one process, one line per
call.  Under `rocprofv3 --kernel-trace --output-format csv -d <dir> -- python3 tools/warp_routes.py` the profiler's trace holds the kernels
in launch order; `python3 tools/warp_routes.py --kernels <dir>` prints that ordered list (template arguments included, the torch kernels of
the set-up dropped).  Two builds route alike when their lists are the same: profiles/warp_request_routes.txt.

The combinations: 6 map modes x {ideal, fisheye coefficients, pinhole coefficients, pinhole coefficients all zero} x {one rotation, a
rotation per row} x 3 resamplers x 4 border modes x {BGR8, plane-wise NV12}, where served (a rotation per row: map modes 0, 1 and 5; fisheye
coefficients: 1 and 2; pinhole coefficients: 3 and 4) -- warp_nv12_rs_ex, or warp_nv12_pinhole for a rectilinear lens.  Then every older
entry point once per output format it has, the keep-edge warp and the quantised map.  64 x 32 source, 32 x 16 output: the smallest shape the
plane-wise warp takes, with room to spare.  Calls only what the binding had before the routing was made one function."""
import csv
import glob
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SW, SH, DW, DH = 64, 32, 32, 16
LENSES = ("ideal", "fisheye", "pinhole", "pinhole0")
D_FISH, D_RECT, D_ZERO = (0.02, -0.004, 0.001, 0.0), (-0.05, 0.01, 0.001, -0.002, 0.0), (0.0,) * 5


def served(mode, lens, rs):
    if rs and mode not in (0, 1, 5):
        return False
    return {"ideal": True, "fisheye": mode in (1, 2), "pinhole": mode in (3, 4) and not rs, "pinhole0": mode in (3, 4) and not rs}[lens]


def rotation_z(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([c, -s, 0, s, c, 0, 0, 0, 1], np.float32)


def calls(vs, nv12, p, rb, qmap):
    """(label, thunk) of every call, in the order they are made"""
    fmts = (("bgr8", vs.OUT_BGR8), ("planar", vs.OUT_NV12_PLANAR))
    borders = (vs.BORDER_CONSTANT, vs.BORDER_REPLICATE, vs.BORDER_REFLECT, vs.BORDER_REFLECT_101)
    resamplers = (vs.RESAMPLE_DEFAULT, vs.RESAMPLE_CUBIC, vs.RESAMPLE_LANCZOS4)
    for mode in range(6):
        for lens in LENSES:
            for rs in (0, 1):
                if not served(mode, lens, rs):
                    continue
                for rsm in resamplers:
                    for b in borders:
                        for fname, fmt in fmts:
                            label = f"mode={mode} lens={lens} rs={rs} resample={rsm} border={b} out={fname}"
                            if lens in ("pinhole", "pinhole0"):
                                d = D_RECT if lens == "pinhole" else D_ZERO
                                yield "warp_nv12_pinhole " + label, lambda d=d, mode=mode, rsm=rsm, b=b, fmt=fmt: vs.warp_nv12_pinhole(nv12, p, d, DW, DH, mode, rsm, b, fmt)
                            else:
                                kw = dict(rot_bottom=rb if rs else None, dist=D_FISH if lens == "fisheye" else None, mode=mode, resample=rsm, border_mode=b, out_format=fmt)
                                yield "warp_nv12_rs_ex " + label, lambda kw=kw: vs.warp_nv12_rs_ex(nv12, p, DW, DH, **kw)
    # the older entry points, each once per output format (map mode 1: the one every lens and the rotation per row admit)
    for fname, fmt in fmts + (("nv12", vs.OUT_NV12),):
        yield f"warp_nv12 out={fname}", lambda fmt=fmt: vs.warp_nv12(nv12, p, DW, DH, 1, fmt)
        yield f"warp_nv12_rs out={fname}", lambda fmt=fmt: vs.warp_nv12_rs(nv12, p, rb, DW, DH, 1, fmt)
    yield "warp_nv12_bgr", lambda: vs.warp_nv12_bgr(nv12, p, DW, DH)
    yield "warp_nv12_mapped out=bgr8", lambda: vs.warp_nv12_mapped(nv12, qmap, DW, DH, vs.OUT_BGR8)
    yield "warp_nv12_mapped out=nv12", lambda: vs.warp_nv12_mapped(nv12, qmap, DW, DH, vs.OUT_NV12)
    for fname, fmt in fmts:
        yield f"warp_nv12_dist out={fname}", lambda fmt=fmt: vs.warp_nv12_dist(nv12, p, D_FISH, DW, DH, 1, fmt)
        yield f"warp_nv12_dist_ex cubic reflect out={fname}", lambda fmt=fmt: vs.warp_nv12_dist_ex(nv12, p, D_FISH, DW, DH, 1, vs.RESAMPLE_CUBIC, vs.BORDER_REFLECT, fmt)
        yield f"warp_nv12_cubic out={fname}", lambda fmt=fmt: vs.warp_nv12_cubic(nv12, p, DW, DH, 1, fmt)
        yield f"warp_nv12_lanczos4 out={fname}", lambda fmt=fmt: vs.warp_nv12_lanczos4(nv12, p, DW, DH, 1, fmt)
        for b in borders:
            yield f"warp_nv12_cubic_border border={b} out={fname}", lambda fmt=fmt, b=b: vs.warp_nv12_cubic_border(nv12, p, DW, DH, 1, fmt, b)
            yield f"warp_nv12_lanczos4_border border={b} out={fname}", lambda fmt=fmt, b=b: vs.warp_nv12_lanczos4_border(nv12, p, DW, DH, 1, fmt, b)
            for rs in (0, 1):
                yield (f"warp_nv12_border border={b} rs={rs} out={fname}",
                       lambda fmt=fmt, b=b, rs=rs: vs.warp_nv12_border(nv12, p, DW, DH, 1, fmt, b, rb if rs else None))
        for rs in (0, 1):
            yield f"warp_nv12_keep rs={rs} out={fname}", lambda fmt=fmt, rs=rs: keep(vs, nv12, p, rb if rs else None, fmt)


def keep(vs, nv12, p, rb, fmt):
    import torch
    if fmt == vs.OUT_BGR8:
        prev = torch.zeros((DH, DW, 3), dtype=torch.uint8, device=nv12.device)
    else:
        prev = tuple(torch.zeros_like(t) for t in vs.nv12_out_planes(DW, DH, nv12.device))
    return vs.warp_nv12_keep(nv12, p, DW, DH, prev, 1, fmt, rb)


def run():
    import torch
    vs = importlib.import_module("video-annotator_amd")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(7)
    nv12 = torch.from_numpy(rng.integers(16, 236, (SH * 3 // 2, SW), dtype=np.uint8)).to(dev)
    p = np.concatenate([np.array([SW / 2, SH / 2, 24, 24, DW / 2, DH / 2, 20, 20], np.float32), rotation_z(0.02)])
    rb = rotation_z(0.05)
    qmap = vs.quantised_map(p, DW, DH, 1)
    torch.cuda.synchronize()
    n = 0
    for label, call in calls(vs, nv12, p, rb, qmap):
        call()
        print(label, flush=True)
        n += 1
    torch.cuda.synchronize()
    print(f"{n} calls ({vs.version()})")


def kernels(trace_dir):
    f = glob.glob(trace_dir + "/**/*kernel_trace.csv", recursive=True)[0]
    rows = [r for r in csv.DictReader(open(f)) if "vstab" in r["Kernel_Name"]]
    for r in sorted(rows, key=lambda r: int(r["Start_Timestamp"])):
        print(r["Kernel_Name"])


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--kernels":
        kernels(sys.argv[2])
    else:
        run()
