"""Driver for profiles/colour10_warp_4k.txt (development helper): the COLOUR instantiations of the 10-bit k_warp_fused
(vstab_warp_p010_colour / vstab_warp_p010_planes_colour with (BT2020, LIMITED)) beside the default kernels (vstab_warp_p010 /
vstab_warp_p010_planes), at the 4K config-5 shape: 3840 x 2160 P010 -> 3524 x 1999 with the preset fisheye camera and its output camera,
a rotation per output row (rodrigues(0.01, -0.02, 0.015) at the top, (0.012, -0.018, 0.013) at the bottom), random frames, map mode 0,
both blends, 16-bit BGR and P010 planes out.
usage: python tools/colour10_time.py <root of a built tree> [launches] [rounds]
In one process, `rounds` (default 3) times in turn: the default kernel, the colour entry point with (CVTCOLOR, LIMITED) -- which must
launch the default kernel and reproduce its bytes --, the colour kernel with (BT2020, LIMITED).  Each `launches` (default 20) launches
after 3 warm-up ones, each launch's own start / end stamps through vstab_time_next_launch.  Prints the median, min and max of every
repeat in microseconds and one checksum per variant (the first two must agree).  The default kernels' instruction streams are the parent
commit's (tools/asm_kernel_diff.py), so their repeats stand for the parent's kernels."""
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


def rodrigues(a, b, c):
    th = float(np.sqrt(a * a + b * b + c * c))
    Kx = np.array([[0, -c, b], [c, 0, -a], [-b, a, 0]]) / th
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


p = vs.map_params(K, Ko, rodrigues(0.01, -0.02, 0.015))
rb = vs.map_params(K, Ko, rodrigues(0.012, -0.018, 0.013))[8:]
nf = 4
torch.manual_seed(0)
# P010 words: ten random bits at the top of every 16-bit sample
frames = [(torch.randint(0, 1024, (h * 3 // 2, w), dtype=torch.int32, device="cuda") << 6).to(torch.int16) for _ in range(nf)]
DEFAULT, BT2020L = (vs.COLOUR_CVTCOLOR, vs.RANGE_LIMITED), (vs.COLOUR_BT2020, vs.RANGE_LIMITED)


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


for blend, btag in ((vs.BLEND_EXACT, "exact"), (vs.BLEND_FP16, "fp16")):
    for planes, tag in ((False, "bgr16"), (True, "p010")):
        if planes:
            out = (torch.zeros((ch, cw), dtype=torch.int16, device="cuda"), torch.zeros(((ch + 1) // 2, 2 * ((cw + 1) // 2)), dtype=torch.int16, device="cuda"))

            def warp(i, colour):
                f = frames[i % nf]
                vs.warp_p010_planes(f[:h], f[h:], p, cw, ch, rb, vs.MAP_CREATEMAP_CL, blend, out_y=out[0], out_uv=out[1], colour=colour)
        else:
            out = torch.zeros((ch, cw, 3), dtype=torch.int16, device="cuda")

            def warp(i, colour):
                f = frames[i % nf]
                vs.warp_p010(f[:h], f[h:], p, cw, ch, rb, vs.MAP_CREATEMAP_CL, blend, out=out, colour=colour)
        runs = (("default", lambda i: warp(i, None)), ("colour CVTCOLOR limited", lambda i: warp(i, DEFAULT)), ("colour BT2020 limited", lambda i: warp(i, BT2020L)))
        crcs, meds = [], {}
        for rep in range(rounds):
            for name, run in runs:
                t = timed(run, launches)
                meds.setdefault(name, []).append(float(np.median(t)))
                print(f"{btag} {tag} round {rep} {name:26s} n={len(t):3d} median {np.median(t):8.1f} us  min {min(t):8.1f}  max {max(t):8.1f}", flush=True)
                if rep == 0:
                    run(0)
                    torch.cuda.synchronize()
                    crcs.append(checksum(out))
        print(f"{btag} {tag} checksums default {crcs[0]:08x} CVTCOLOR {crcs[1]:08x} BT2020 {crcs[2]:08x}", flush=True)
        assert crcs[0] == crcs[1], "(CVTCOLOR, LIMITED) must reproduce the default kernel's bytes"
        assert crcs[2] != crcs[0], "(BT2020, LIMITED) must not"
        print(f"{btag} {tag} medians of the rounds: " + "; ".join(f"{n}: {np.median(m):.1f} us (rounds {min(m):.1f} .. {max(m):.1f})" for n, m in meds.items()), flush=True)
print(f"{root}: {launches} launches per repeat, {rounds} rounds, {w}x{h} P010 -> {cw}x{ch}, a rotation per row")
