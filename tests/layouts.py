"""Source frames in the device layouts decoders hand over, the C ABI called with separate planes, output planes guarded by
canaries, and a CPU model of the tiled kernels' source boxes.  Test infrastructure only (a plain module, imported by the tests).

Every NV12 / P010 entry point takes two independent planes (a base pointer and a pitch each); the binding's convenience
functions always pass one packed buffer.  Here the planes are placed as decoders place them -- chroma in its own allocation,
before luma, at an aligned-height offset, at another pitch -- and every buffer byte outside the planes is a fill pattern, so a
read with the wrong pitch or plane is visibly wrong.  Outputs get canary bands above, below and right of each plane."""
import ctypes

import numpy as np

FILL = 0xA7      # source bytes outside the planes
CANARY = 0xC5    # output bytes outside the planes
GUARD_ROWS = 3

# layout_spec(name, ...) -> (luma pitch, chroma pitch, placement, luma offset, chroma offset); placement "one": both planes in one
# buffer at their offsets, "two": two allocations
LAYOUTS = ("packed", "separate", "chroma_first", "decoder", "uv_wider", "uv_narrower", "unaligned")


def _al(v, a):
    return (v + a - 1) // a * a


def layout_spec(name, rb, h):
    """-> (pitch_y, pitch_uv, how, luma offset, chroma offset) for a plane of rb bytes per row and h luma rows."""
    if name == "packed":
        return rb, rb, "one", 0, rb * h
    if name == "separate":
        return rb, rb, "two", 0, 0
    if name == "chroma_first":
        p = _al(rb, 16)
        return p, p, "one", _al(p * (h // 2), 256) + 256, 0
    if name == "decoder":            # pitch > width, chroma at y + pitch * align(h, 32)
        p = _al(rb + 1, 256)
        return p, p, "one", 0, p * _al(h, 32)
    if name == "uv_wider":           # both 16-byte aligned: the staged paths are taken
        py = _al(rb, 16)
        return py, py + 96, "two", 0, 0
    if name == "uv_narrower":
        pu = _al(rb, 16)
        return pu + 160, pu, "one", 0, (pu + 160) * h + 64
    if name == "unaligned":          # 4-byte aligned bases and pitches only: the global-memory gather path
        py, pu = _al(rb, 16) + 4, _al(rb, 16) + 36
        return py, pu, "two", 4, 4
    raise ValueError(name)


class Src:
    """One source frame placed in device memory: y / uv pointers, pitches, the (w, h) of the frame and the buffers kept alive."""

    def __init__(self, y, uv, pitch_y, pitch_uv, w, h, keep):
        self.y, self.uv, self.pitch_y, self.pitch_uv, self.w, self.h, self.keep = y, uv, pitch_y, pitch_uv, w, h, keep


def _rows_into(buf, off, pitch, plane_bytes):
    """Copy the rows of a (rows, rb) uint8 host array into a flat device uint8 tensor at byte `off` with `pitch`."""
    import torch
    rows, rb = plane_bytes.shape
    view = torch.as_strided(buf, (rows, rb), (pitch, 1), off)
    view.copy_(torch.from_numpy(np.ascontiguousarray(plane_bytes)))


def place(y, uv, name, cuda, host=False, spec=None):
    """y (h, w) / uv (h / 2, w) host planes, uint8 (NV12) or uint16 (P010 words) -> Src in layout `name` (or `spec`, a layout_spec
    tuple), in device memory or (host) in host memory."""
    import torch
    yb, ub = np.ascontiguousarray(y).view(np.uint8), np.ascontiguousarray(uv).view(np.uint8)
    h, rb = yb.shape
    w = y.shape[1]
    py, pu, how, oy, ou = spec or layout_spec(name, rb, h)
    dev = "cpu" if host else cuda
    if how == "two":
        by = torch.full((oy + py * h + 64,), FILL, dtype=torch.uint8, device=dev)
        bu = torch.full((ou + pu * (h // 2) + 64,), FILL, dtype=torch.uint8, device=dev)
    else:
        n = max(oy + py * h, ou + pu * (h // 2)) + 64
        by = bu = torch.full((n,), FILL, dtype=torch.uint8, device=dev)
    _rows_into(by, oy, py, yb)
    _rows_into(bu, ou, pu, ub)
    return Src(by.data_ptr() + oy, bu.data_ptr() + ou, py, pu, w, h, (by, bu))


class Plane:
    """An output plane of `rows` x `rb` bytes inside a buffer with GUARD_ROWS canary rows above and below and `pad` canary bytes
    right of every row (pad keeps 16-byte alignment, so the vector stores are taken)."""

    def __init__(self, rows, rb, cuda, pad=48):
        import torch
        self.rows, self.rb, self.pitch = rows, rb, _al(rb, 16) + pad
        self.buf = torch.full(((rows + 2 * GUARD_ROWS) * self.pitch,), CANARY, dtype=torch.uint8, device=cuda)
        self.ptr = self.buf.data_ptr() + GUARD_ROWS * self.pitch

    def host(self, dtype=np.uint8, shape=None):
        """-> the plane's bytes as `dtype` (shape (rows, rb / itemsize) or `shape`), after checking every canary byte (of a pitch wider
        than the row plus 64 bytes -- a plane past 4 GiB --, the first 64 canary bytes right of each row)."""
        import torch
        cols = min(self.pitch, _al(self.rb, 16) + 64)
        a = torch.as_strided(self.buf, (self.rows + 2 * GUARD_ROWS, cols), (self.pitch, 1)).cpu().numpy()
        g = GUARD_ROWS
        bad = int((a[:g] != CANARY).sum() + (a[g + self.rows:] != CANARY).sum() + (a[g:g + self.rows, self.rb:] != CANARY).sum())
        assert bad == 0, f"{bad} bytes written outside the plane"
        p = np.ascontiguousarray(a[g:g + self.rows, :self.rb]).view(dtype)
        return p if shape is None else p.reshape(shape)


def out_nv12(dw, dh, cuda):
    return Plane(dh, dw, cuda), Plane((dh + 1) // 2, 2 * ((dw + 1) // 2), cuda)


def out_p010(dw, dh, cuda):
    return Plane(dh, 2 * dw, cuda), Plane((dh + 1) // 2, 4 * ((dw + 1) // 2), cuda)


# ---- the C ABI with separate planes ---------------------------------------------------------------------------------------------
def _f(a):
    a = np.ascontiguousarray(a, np.float32)
    return a, a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _call(vs, fn, *args):
    st = getattr(vs.lib, fn)(*args)
    if st != vs.OK:
        raise vs.VstabError(st, fn)


def warp_nv12(vs, s, params, dw, dh, mode, out_format, cuda, rot_bottom=None):
    """vstab_warp_nv12_ex (or _rs with rot_bottom) -> BGR (dh, dw, 3), or (y, uv) NV12 planes."""
    p, pp = _f(params)
    if out_format == vs.OUT_BGR8:
        o = Plane(dh, 3 * dw, cuda)
        d, dp, du, dpu = o.ptr, o.pitch, None, 0
    else:
        oy, ou = out_nv12(dw, dh, cuda)
        d, dp, du, dpu = oy.ptr, oy.pitch, ou.ptr, ou.pitch
    if rot_bottom is None:
        _call(vs, "vstab_warp_nv12_ex", s.y, s.pitch_y, s.uv, s.pitch_uv, s.w, s.h, pp, int(mode), int(out_format), d, dp, du, dpu, dw, dh, vs._stream())
    else:
        rb, rbp = _f(np.asarray(rot_bottom).reshape(9))
        _call(vs, "vstab_warp_nv12_rs", s.y, s.pitch_y, s.uv, s.pitch_uv, s.w, s.h, pp, rbp, int(mode), int(out_format), d, dp, du, dpu, dw, dh,
              vs._stream())
    if out_format == vs.OUT_BGR8:
        return o.host(shape=(dh, dw, 3))
    return oy.host(), ou.host()


def warp_nv12_mapped(vs, s, qmap, dw, dh, out_format, cuda):
    if out_format == vs.OUT_BGR8:
        o = Plane(dh, 3 * dw, cuda)
        _call(vs, "vstab_warp_nv12_mapped", s.y, s.pitch_y, s.uv, s.pitch_uv, s.w, s.h, qmap.data_ptr(), int(out_format), o.ptr, o.pitch, None, 0,
              dw, dh, vs._stream())
        return o.host(shape=(dh, dw, 3))
    oy, ou = out_nv12(dw, dh, cuda)
    _call(vs, "vstab_warp_nv12_mapped", s.y, s.pitch_y, s.uv, s.pitch_uv, s.w, s.h, qmap.data_ptr(), int(out_format), oy.ptr, oy.pitch, ou.ptr,
          ou.pitch, dw, dh, vs._stream())
    return oy.host(), ou.host()


def warp_nv12_cubic(vs, s, params, dw, dh, mode, out_format, cuda, out=None):
    """vstab_warp_nv12_cubic -> BGR (dh, dw, 3), or (y, uv) plane-wise NV12.  out: the output Plane (BGR) or (luma, chroma) Planes,
    for callers that place the output themselves; default canaried planes of the natural size."""
    p, pp = _f(params)
    if out_format == vs.OUT_BGR8:
        o = out or Plane(dh, 3 * dw, cuda)
        _call(vs, "vstab_warp_nv12_cubic", s.y, s.pitch_y, s.uv, s.pitch_uv, s.w, s.h, pp, int(mode), int(out_format), o.ptr, o.pitch, None, 0,
              dw, dh, vs._stream())
        return o.host(shape=(dh, dw, 3))
    oy, ou = out or out_nv12(dw, dh, cuda)
    _call(vs, "vstab_warp_nv12_cubic", s.y, s.pitch_y, s.uv, s.pitch_uv, s.w, s.h, pp, int(mode), int(out_format), oy.ptr, oy.pitch, ou.ptr,
          ou.pitch, dw, dh, vs._stream())
    return oy.host(), ou.host()


def warp_nv12_nearest(vs, s, params, dw, dh, mode, cuda):
    p, pp = _f(params)
    o = Plane(dh, 3 * dw, cuda)
    _call(vs, "vstab_warp_nv12_nearest_ex", s.y, s.pitch_y, s.uv, s.pitch_uv, s.w, s.h, pp, int(mode), o.ptr, o.pitch, dw, dh, vs._stream())
    return o.host(shape=(dh, dw, 3))


def cvt_nv12_bgr(vs, s, cuda):
    o = Plane(s.h, 3 * s.w, cuda)
    _call(vs, "vstab_cvt_nv12_bgr", s.y, s.pitch_y, s.uv, s.pitch_uv, s.w, s.h, o.ptr, o.pitch, vs._stream())
    return o.host(shape=(s.h, s.w, 3))


def pack(vs, s, cuda, p010=False):
    """vstab_pack_nv12 / vstab_pack_p010 -> the packed 8-bit NV12 frame (h * 3 / 2, w); writes w * h * 3 / 2 bytes from its dst."""
    o = Plane(s.h * 3 // 2, s.w, cuda, pad=0)
    _call(vs, "vstab_pack_p010" if p010 else "vstab_pack_nv12", s.y, s.pitch_y, s.uv, s.pitch_uv, s.w, s.h, o.ptr, vs._stream())
    return o.host()


def warp_p010(vs, s, params, dw, dh, mode, blend, cuda, rot_bottom=None):
    """vstab_warp_p010 -> (dh, dw, 3) uint16 BGR."""
    p, pp = _f(params)
    rb, rbp = _f(np.asarray(rot_bottom).reshape(9)) if rot_bottom is not None else (None, None)
    o = Plane(dh, 6 * dw, cuda)
    _call(vs, "vstab_warp_p010", s.y, s.pitch_y, s.uv, s.pitch_uv, s.w, s.h, pp, rbp, int(mode), int(blend), o.ptr, o.pitch, dw, dh, vs._stream())
    return o.host(np.uint16, (dh, dw, 3))


def warp_p010_planes(vs, s, params, dw, dh, mode, blend, cuda, rot_bottom=None, planar=False):
    """vstab_warp_p010_planes (planar: vstab_warp_p010_planar) -> (y, uv) uint16 P010 words."""
    p, pp = _f(params)
    rb, rbp = _f(np.asarray(rot_bottom).reshape(9)) if rot_bottom is not None else (None, None)
    oy, ou = out_p010(dw, dh, cuda)
    _call(vs, "vstab_warp_p010_planar" if planar else "vstab_warp_p010_planes", s.y, s.pitch_y, s.uv, s.pitch_uv, s.w, s.h, pp, rbp, int(mode), int(blend),
          oy.ptr, oy.pitch, ou.ptr, ou.pitch, dw, dh, vs._stream())
    return oy.host(np.uint16), ou.host(np.uint16)


# ---- the tiled kernels' source boxes, restated (vstab_warp_tile.hpp probe_tile, launch_warp_planar / launch_warp_fused) ---------------
def _rint(v):
    return np.rint(v)   # round half to even, as cvRound


def planar_launch(dw, dh, depth):
    """(rwb, lds_kb, capacity in pixels) launch_warp_planar picks."""
    bps = 2 if depth == 10 else 1
    tiles32 = -(-dw // 64) * -(-dh // 32)
    rwb = 4 if tiles32 < 1536 else 8
    lds_kb = (40 if bps == 2 else 24) if rwb == 8 else 14 * bps
    cap = (lds_kb * 1024 - 32 - 4 * 768 * bps) * 2 // (3 * bps)
    return rwb, lds_kb, cap


def tile_boxes(mapx, mapy, sw, sh, th, planar=True, block_w=16):
    """Source boxes of the 64 x th output tiles from exact map planes (dh, dw): perimeter extremes of the quantised map, clamped to
    [-1, sw] / [-1, sh], the probe's margins, BLOCK_W alignment and even height.  -> dict (tile row, tile column) -> (bx0, by0, wb, hb, have)."""
    dh, dw = mapx.shape
    lo_m, hi_m, cap = (2, 5, 1) if planar else (1, 2, 0)
    qx = np.floor(_rint(32.0 * mapx.astype(np.float64)) / 32.0)
    qy = np.floor(_rint(32.0 * mapy.astype(np.float64)) / 32.0)
    qx = np.nan_to_num(qx, nan=1e9)
    qy = np.nan_to_num(qy, nan=1e9)
    X, Y = np.clip(qx, -1, sw), np.clip(qy, -1, sh)
    out = {}
    for y0 in range(0, dh, th):
        for x0 in range(0, dw, 64):
            ys, xs = slice(y0, min(dh, y0 + th)), slice(x0, min(dw, x0 + 64))
            bx, by = X[ys, xs], Y[ys, xs]
            per = np.zeros(bx.shape, bool)
            per[0, :], per[-1, :], per[:, 0], per[:, -1] = True, True, True, True
            mnx, mxx, mny, mxy = int(bx[per].min()), int(bx[per].max()), int(by[per].min()), int(by[per].max())
            lox, hix = max(mnx - lo_m, -lo_m), min(mxx + hi_m, sw + cap)
            loy, hiy = max(mny - lo_m, -lo_m), min(mxy + hi_m, sh + cap)
            bx0, by0 = lox & ~(block_w - 1), loy & ~1
            wb = (hix + 1 - bx0 + block_w - 1) & ~(block_w - 1)
            hb = (hiy + 1 - by0 + 1) & ~1
            have = mnx < sw and mxx >= -1 and mny < sh and mxy >= -1
            out[(y0 // th, x0 // 64)] = (bx0, by0, wb, hb, have)
    return out


def planar_tile_states(mapx, mapy, sw, sh, depth, margin=0):
    """What the plane-wise kernel does with each tall tile of a launch, before the fix of `fits`: counts of
    'wide' (staged although a box row has more than 64 chunks, with `margin` pixels to spare), 'split' (over the LDS budget),
    'staged' (the rest that have a box).  -> (counts, rwb, capacity)."""
    dh, dw = mapx.shape
    rwb, _, cap = planar_launch(dw, dh, depth)
    bw = 16 // (2 if depth == 10 else 1)
    counts = {"wide": 0, "split": 0, "staged": 0, "outside": 0}
    for (bx0, by0, wb, hb, have) in tile_boxes(mapx, mapy, sw, sh, 4 * rwb, True, bw).values():
        if not have:
            counts["outside"] += 1
        elif (wb + margin) * (hb + margin) > cap or wb * hb > cap:
            counts["split"] += 1
        elif (wb - margin) // bw > 64 and (wb + margin) * (hb + margin) <= cap:
            counts["wide"] += 1
        else:
            counts["staged"] += 1
    return counts, rwb, cap


# ---- the XCD band / tile schedule, restated (vstab_warp_tile.hpp tile_schedule, the three launchers, the block -> tile prologue of
# k_warp_fused / k_warp_planar).  The constants are the launchers' own; test_tile_schedule_cpu.py pins them against the sources. ------------
TILES32_RWB8 = 1536          # launch_warp_fused / launch_warp_planar: 64 x 32 tiles (rwb 8) from this many 64 x 32 tiles on
FUSED_LDS_KB = {4: 20, 8: 40}
FUSED10_LDS_KB, FUSED10_RWB, FUSED10_TAIL_TILES = 40, 8, 1024
TAIL_SLOTS_PER_RESIDENT = 256.0   # tail on when the launch has more tiles than 256 x (workgroups a CU holds): more than one round
SLOTS_PER_WG_PER_CU = 32          # tile_schedule: 32 CUs per XCD
LDS_BUDGET_KB = 160


def fused_launch(dw, dh):
    """(rwb, lds_kb, tail_rounds) launch_warp_fused picks."""
    tiles32 = -(-dw // 64) * -(-dh // 32)
    rwb = 4 if tiles32 < TILES32_RWB8 else 8
    lds_kb = FUSED_LDS_KB[rwb]
    tail = 0.5 if -(-dw // 64) * -(-dh // (4 * rwb)) > TAIL_SLOTS_PER_RESIDENT * (LDS_BUDGET_KB // lds_kb) else 0.0
    return rwb, lds_kb, tail


def fused10_launch(dw, dh):
    """(rwb, lds_kb, tail_rounds) launch_warp_fused10 picks."""
    tiles = -(-dw // 64) * -(-dh // (4 * FUSED10_RWB))
    return FUSED10_RWB, FUSED10_LDS_KB, (0.5 if tiles > FUSED10_TAIL_TILES else 0.0)


def planar_resident(rwb, lds_kb):
    return min(LDS_BUDGET_KB // lds_kb, 7 if rwb == 8 else 8, 8)


def planar_schedule_launch(dw, dh, depth):
    """(rwb, lds_kb, tail_rounds) launch_warp_planar picks."""
    rwb, lds_kb, _ = planar_launch(dw, dh, depth)
    tail = 0.25 if -(-dw // 64) * -(-dh // (4 * rwb)) > TAIL_SLOTS_PER_RESIDENT * planar_resident(rwb, lds_kb) else 0.0
    return rwb, lds_kb, tail


def _lround(v):
    return int(np.floor(v + 0.5)) if v >= 0 else -int(np.floor(-v + 0.5))


def tile_schedule(dw, dh, rwb, lds_kb, tail_rounds):
    """-> dict(tiles_x, band_y (9), split_y (8), shares (8), grid) as tile_schedule fills FusedArgs and sizes the grid."""
    tiles_x = -(-dw // 64)
    th = 4 * rwb
    ts = th // 2
    half_rows = -(-dh // ts)
    slots = SLOTS_PER_WG_PER_CU * max(1, min(8, LDS_BUDGET_KB // lds_kb))
    band_y = [min(dh, (k * half_rows // 8) * ts) for k in range(9)]
    band_y[8] = dh
    split_y, shares = [], []
    for k in range(8):
        rows = band_y[k + 1] - band_y[k]
        tall_rows_max = rows // th
        tail_tall_rows = min(tall_rows_max, _lround(tail_rounds * slots / tiles_x))
        tall_rows = tall_rows_max - tail_tall_rows
        split_y.append(band_y[k] + tall_rows * th)
        shares.append(tall_rows * tiles_x + -(-(band_y[k + 1] - split_y[k]) // ts) * tiles_x)
    return dict(tiles_x=tiles_x, band_y=band_y, split_y=split_y, shares=shares, grid=8 * max(shares))


def block_tiles(s, rwb):
    """The prologue of k_warp_fused / k_warp_planar for every block of the grid of schedule `s`: -> list of (block, x0, ys, rows) of the
    live blocks -- rows 4 rwb for a tall tile (done whole, or as two half-height tiles), 2 rwb for a half-height one -- and the number
    of blocks that return at once."""
    th = 4 * rwb
    ts = th // 2
    tx = s["tiles_x"]
    live, idle = [], 0
    for b in range(s["grid"]):
        k, idx = b & 7, b >> 3
        y_lo, y_sp, y_hi = s["band_y"][k], s["split_y"][k], s["band_y"][k + 1]
        n_tall = ((y_sp - y_lo) // th) * tx
        if idx < n_tall:
            row = idx // tx
            live.append((b, (idx - row * tx) * 64, y_lo + row * th, th))
        else:
            i2 = idx - n_tall
            row = i2 // tx
            ys = y_sp + row * ts
            if ys >= y_hi:
                idle += 1
                continue
            live.append((b, (i2 - row * tx) * 64, ys, ts))
    return live, idle
