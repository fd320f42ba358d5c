"""Development helper (tools/dev/libvstab_dev.so, `make -C video-annotator_amd dev`): eight wall-clock stamps per wave of
one launch of the fused warp kernel -> how long each phase of a tile takes, workgroup durations, residency over time.
usage: python tools/wg_timeline.py [development library]; env: QW, QH, QMODE as tools/quick_warp_time.py; QDUMP=file.npz also saves
blockIdx, start and end (us) of every workgroup that ran a tile, for fits of the per-tile cost (profiles/dead_tiles_bands_4k.txt), and
every stamp (us).  QDEAD=1 (the 4K headline geometry, modes 0 / 5): phase medians of the dead workgroups alone -- dead by the kernel's rule
(tests/dead_tiles.py) as tools/fit_band_costs.py classifies them, tall and half-height, the all-dead stretch at the start of XCD 0's band
and dead tiles that run among live ones apart (profiles/dead_store_4k.txt).  QLOAD=file.npz prints everything from a dump saved with the
stamps instead of running a launch (no GPU and no torch; the library that made the dump is still loaded and must be named: the cameras
and, with QDEAD, the bands come from its host code)."""
import ctypes, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import devlib
vs = devlib.load(sys.argv[1] if len(sys.argv) > 1 else None)
w, h = int(os.environ.get("QW", 3840)), int(os.environ.get("QH", 2160))
mode = int(os.environ.get("QMODE", 0))
K = vs.get_preset_camera(4, w, h); Ko, (cw, ch) = vs.get_output_camera(K, w, h)
p = vs.map_params(K, Ko, np.eye(3))
if os.environ.get("QLOAD"):
    dump = np.load(os.environ["QLOAD"])
    if "stamps" not in dump: sys.exit(f"{os.environ['QLOAD']} holds no stamps (saved by an earlier wg_timeline.py: blk, start and end only); tools/fit_band_costs.py reads such a dump")
    blk, t = dump["blk"], dump["stamps"]
else:
    import torch
    frames = [torch.randint(0, 256, (h * 3 // 2, w), dtype=torch.uint8, device="cuda") for _ in range(4)]
    outs = [torch.empty((ch, cw, 3), dtype=torch.uint8, device="cuda") for _ in range(4)]
    for i in range(8): vs.warp_nv12(frames[i % 4], p, cw, ch, mode, 0, out=outs[i % 4])
    torch.cuda.synchronize()
    nwg = 16384
    buf = torch.zeros((nwg, 4, 8), dtype=torch.int64, device="cuda")
    vs._L.vstab_dev_set_timing.argtypes = [ctypes.c_void_p]
    vs._L.vstab_dev_set_timing(ctypes.c_void_p(buf.data_ptr()))
    for i in range(3): vs.warp_nv12(frames[i % 4], p, cw, ch, mode, 0, out=outs[i % 4])   # the last launch's stamps survive
    torch.cuda.synchronize()
    vs._L.vstab_dev_set_timing(ctypes.c_void_p(0))
    t = buf.cpu().numpy().astype(np.float64)
    live = t[:, 0, 7] != 0
    blk = np.nonzero(live)[0]  # blockIdx.x of every workgroup that ran a tile
    t = t[live] / 100.0  # microseconds
    t[t == 0] = np.nan   # a stamp a wave never took
    t0 = t[:, :, 0].min()
    t -= t0
start, end = t[:, :, 0].min(axis=1), t[:, :, 7].max(axis=1)
dur = end - start
print(f"workgroups {len(t)}  span {end.max():.2f} us")
if os.environ.get("QDUMP"): np.savez(os.environ["QDUMP"], blk=blk, start=start, end=end, stamps=t)
print(f"workgroup duration us: median {np.median(dur):.2f} p10 {np.percentile(dur,10):.2f} p90 {np.percentile(dur,90):.2f} max {dur.max():.2f}; "
      f"sum {dur.sum():.0f} us -> mean residency {dur.sum()/end.max():.0f} workgroups")
names = ["probe + barrier", "load issue", "map", "convert", "barrier", "sample + blend", "store"]
for wv, label in ((0, "wave 0 (probes)"), (1, "wave 1"), (3, "wave 3")):
    d = np.diff(t[:, wv, :], axis=1)
    print(f"  {label}: " + "  ".join(f"{n} {np.nanmedian(d[:, k]):.2f} (p90 {np.nanpercentile(d[:, k], 90):.2f})" for k, n in enumerate(names)))
edges = np.linspace(0, end.max(), 25)
for a, b in zip(edges[:-1], edges[1:]):
    m = (a + b) / 2
    print(f"  t={m:6.1f} us  resident {int(((start <= m) & (end > m)).sum()):5d}  started {int(((start >= a) & (start < b)).sum()):5d}")
# per XCD (blockIdx.x % 8: one band of output rows each): when its first / last workgroup ran, and how much work it had
print("per XCD: workgroups, first start, last end, sum of workgroup durations (us)")
for k in range(8):
    m = (blk & 7) == k
    print(f"  xcd {k}: {int(m.sum()):5d}  {start[m].min():6.2f}  {end[m].max():6.2f}  {dur[m].sum():8.1f}   median tile {np.median(dur[m]):.2f}")
print("residency per XCD over time (128 workgroup slots each):")
for m_ in np.linspace(0, end.max(), 13)[1:-1]:
    print(f"  t={m_:5.1f} us  " + " ".join(f"{int((((blk & 7) == k) & (start <= m_) & (end > m_)).sum()):4d}" for k in range(8)))
# dispatch order: is workgroup b ever started before workgroup b - 8 * 128 ... (in-order dispatch across the XCDs?)
order = np.argsort(blk)
st_sorted = start[order]
print(f"start times in blockIdx order: non-decreasing steps {int((np.diff(st_sorted) >= -0.02).sum())} of {len(st_sorted) - 1}; largest step back {(-np.diff(st_sorted)).max():.2f} us")
if os.environ.get("QDEAD") == "1":
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import dead_tiles as D, layouts
    rwb, lds_kb, tail = layouts.fused_launch(cw, ch)
    assert (rwb, lds_kb, tail) == (8, 40, 0.5) and mode in (0, 5)
    # the bands of the library that ran (its own cost constants), through its hooks
    u32p, ip, fp = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_float)
    vs.lib.vstabx_band_costs.argtypes = [fp, ctypes.c_int] + [ctypes.c_int] * 5 + [u32p, ctypes.c_int]
    vs.lib.vstabx_weighted_bands.argtypes = [ctypes.c_int] * 4 + [ctypes.c_double, u32p, ctypes.c_int, ip]
    n = -(-ch // 16)
    cost, out, pf = np.zeros(n, np.uint32), np.zeros(19, np.int32), np.ascontiguousarray(p, np.float32)
    assert vs.lib.vstabx_band_costs(pf.ctypes.data_as(fp), 0, w, h, cw, ch, 16, cost.ctypes.data_as(u32p), n) == 0
    if os.environ.get("VSTAB_BANDS") == "0": cost[:] = 1   # even bands
    assert vs.lib.vstabx_weighted_bands(cw, ch, rwb, lds_kb, tail, cost.ctypes.data_as(u32p), n, out.ctypes.data_as(ip)) == 0
    s = dict(tiles_x=int(out[17]), band_y=[int(v) for v in out[:9]], split_y=[int(v) for v in out[9:17]], grid=int(out[18]))
    print("bands (rows): " + " ".join(str(b - a) for a, b in zip(s["band_y"], s["band_y"][1:])) + f"  grid {s['grid']}")
    tile_of = {b: (x0, ys, rows) for b, x0, ys, rows in layouts.block_tiles(s, rwb)[0]}
    assert set(tile_of) == set(int(b) for b in blk), "the workgroups that ran are not the schedule's"
    rule = {th: D.rule(p, cw, ch, w, h, th) for th in (32, 16)}
    kind = np.zeros(len(blk), int)   # 0 live, 32 dead tall, 16 dead half
    for i, b in enumerate(blk):
        x0, ys, th = tile_of[int(b)]
        if ys % th == 0 and rule[th][ys // th, x0 // 64]: kind[i] = th
    # the all-dead stretch of XCD 0: the dead tiles of the leading tile rows of its band of which the rule finds two thirds or more dead
    # (no row of the headline output is dead from end to end: its first has 50 dead tiles of 56)
    x0m, row_y = (blk & 7) == 0, np.array([tile_of[int(b)][1] for b in blk])
    stretch_end = s["band_y"][0]
    for y in sorted(set(row_y[x0m].tolist())):
        if (kind[x0m & (row_y == y)] != 0).mean() < 2.0 / 3.0: break
        stretch_end = y + 1
    stretch = x0m & (row_y < stretch_end) & (kind != 0)
    print(f"dead workgroups: tall {int((kind == 32).sum())}, half {int((kind == 16).sum())}; dead stretch of XCD 0 (rows two thirds dead or more): rows below {stretch_end}, "
          f"{int(stretch.sum())} dead workgroups, over at {end[stretch].max() if stretch.any() else 0.0:.2f} us")
    print("  dead tiles, medians (us)            n   whole   w0 0>1  w0 1>6  w0 6>7 | w3 0>1  w3 1>6  w3 6>7   (0>1 probe + barrier, 1>6 the skipped phases and their barrier, 6>7 store)")
    for th, label in ((32, "tall"), (16, "half")):
        for sel, where in ((stretch, "XCD 0 dead stretch"), (~stretch, "among live tiles")):
            m = (kind == th) & sel
            if not m.any(): continue
            f = lambda wv, a, b: np.nanmedian(t[m, wv, b] - t[m, wv, a])
            print(f"  {label} {where:24s} {int(m.sum()):5d}  {np.median(dur[m]):6.2f}  " + "  ".join(f"{f(0, a, b):6.2f}" for a, b in ((0, 1), (1, 6), (6, 7))) +
                  " | " + "  ".join(f"{f(3, a, b):6.2f}" for a, b in ((0, 1), (1, 6), (6, 7))))
    m = kind == 0
    print(f"  live tiles: tall {int((m & np.array([tile_of[int(b)][2] == 32 for b in blk])).sum())} median {np.median(dur[m & np.array([tile_of[int(b)][2] == 32 for b in blk])]):.2f} us, "
          f"half median {np.median(dur[m & np.array([tile_of[int(b)][2] == 16 for b in blk])]):.2f} us; wave 3 store 6>7 median {np.median(t[m, 3, 7] - t[m, 3, 6]):.2f}")
