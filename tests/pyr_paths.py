"""The image pyramid (csrc/vstab_pyramid.hip: k_pyr_down, k_pyr_down_x2, k_pack_pyr) restated for the tests: the definition of a level,
the host's choices per call, the paths those choices send every group and tile down, and the calls that reach each path on purpose.
No GPU here, apart from the two helpers at the end (Fenced, place) that put planes where a Call says.

THE DEFINITION.  pyr_down_ref: dst(y, x) = (sum_{j,i} k_j k_i src(fold(2y - 2 + j), fold(2x - 2 + i)) + 128) >> 8 with k = 1 4 6 4 1 in int64,
dst = ((w + 1) / 2, (h + 1) / 2), fold = BORDER_REFLECT_101 in closed form (fold101: i mod (2n - 2), upper half mirrored, n == 1 -> 0) --
not the `while` loop the kernel and the oracle share.  Every expected byte of test_pyr_paths_gpu.py comes from it.

THE HOST'S CHOICES.  A Call gives sw, sh and for each plane (base % 16, pitch); that is all launch_pyr_down, pyr_grid, pack_pyr_ok,
launch_pack_pyr, pyr_down_x2_ok and launch_pyr_down_x2 look at.  down_host / x2_host / pack_host return what they derive: vec_ok,
dst_vec_ok, near, the PyrGrid, uv_vec with the causes that deny it, nb_uv, and whether vstab_pyr_down_x2 falls back to two launches.

THE PATHS.  down_paths / x2_paths / pack_paths walk the modelled grid -- every (block, thread) decoded as pyr_down_dispatch does, every tile
item as pyr_down_x2_tile does -- and count how often each named path is taken.  DOWN_PATHS, X2_PATHS, PACK_PATHS are the full name sets.

  k_pyr_down, per group of 4 outputs (g, y):
    int_fast          interior group, y >= 1 and 2y + 2 < sh: five rows from one address, 16-byte loads
    int_top           interior group of row 0 (rows -2, -1 reflected)
    int_bottom_even   interior, 2y + 2 == sh (row sh reflected)        int_bottom_odd   interior, 2y + 1 == sh (rows sh, sh + 1 reflected)
    edge_dword        an edge group's dword column loaded whole          edge_all_bytes   an edge group's dword column by bytes because !vec_ok
    edge_left         a dword column with gx < 0                         edge_right       a dword column with gx + 4 > sw
    far               !near (sw < 16 or sh < 4): reflect101's loop       far_multi_fold   a tap of a stored output folds more than once
    store_partial     dw % 4 != 0: the last group stores 1 .. 3 bytes
    edge_blocks_many  nb_edge >= 2: e / n_edge crosses workgroups        int_blocks_many_x  nbx >= 2: more than 64 interior groups a row
  far_multi_fold is exactly sw <= 2 or sh <= 2 (asserted): the taps of stored outputs span -2 .. n + 1 at most, -2 leaves a 1- or 2-wide image
  twice, and n + 1 -> n - 3 is inside from n = 3 on.  (At sw = 3 .. 9 only bytes with weight 0 or of outputs past dw fold twice.)

  k_pyr_down_x2, per 16 x 10 tile of the second level:
    tile_interior_dst_dword / tile_interior_dst_bytes   interior tile, second level stored as dwords (dst_vec_ok) or bytes
    tile_border       every other tile, with
      mid_dword / mid_bytes          the first-level store of an owned group (vec_ok && mx + 4 <= mw, or byte-wise and clipped at mw)
      region_skipped                 a group of the region outside the first level: not computed, never read
      second_reflect_left / _right / _top / _bottom   a second-level tap reflected in first-level coordinates
      second_clipped                 an output of the tile with x >= dw or y >= dh
    far               !near: only at sw == 15 (pyr_down_x2_ok needs sw >= 15, sh >= 15)
    fallback_two_launches            !pyr_down_x2_ok: vstab_pyr_down_x2 runs k_pyr_down twice

  k_pack_pyr:
    copy_int_fast / copy_int_rows    the 8 x 2 source bytes an interior group owns, stored as two uint2 (fast rows / top and bottom rows)
    copy_edge                        an edge group's, byte by byte under `2 x0 + b < sw` -- which never clips while pack_pyr_ok holds
                                     (w % 8 == 0: the last group ends at w), asserted as copy_edge_clipped == 0
    uv_vec                           chroma copied 16 bytes a thread
    uv_bytes_chroma_base / _chroma_pitch / _width / _ring_base   chroma byte by byte, by cause (uv % 16, pitch_uv % 16, sw % 16 == 8, ring % 16 == 8)
    refused                          pack_pyr_ok is false: nothing launched

THE CASES.  DOWN_CASES, X2_CASES, PACK_CASES: each the smallest shape that reaches what its `what` names (test_pyr_paths_cpu.py asserts that
it does, and that each table reaches every name)."""
import collections
import dataclasses

import numpy as np

G4 = 1 << 32
P2_TW, P2_TH = 16, 10                       # k_pyr_down_x2: second-level outputs per workgroup
P2_MG = (2 * P2_TW + 5 + 3) // 4
P2_MW, P2_MH = 4 * P2_MG, 2 * P2_TH + 3    # the first-level region of a tile
P2_ITEMS = P2_MG * P2_MH
OK, ERR_INVALID = 0, -2

MSG_DOWN_ARG = "vstab_pyr_down: bad argument"
MSG_X2_ARG = "vstab_pyr_down_x2: bad argument"
MSG_DOWN_4G = "pyr_down: planes of 4 GiB or more are not supported"
MSG_X2_4G = "pyr_down_x2: planes of 4 GiB or more are not supported"
MSG_X2_SMALL = "pyr_down_x2: image too small"
MSG_PACK = "pack_pyr: planes not aligned for the fused copy"


def div_up(a, b):
    return -(-a // b)


def al(v, a):
    return div_up(v, a) * a


# ---- a. the definition ---------------------------------------------------------------------------------------------------------------
def fold101(i, n):
    """BORDER_REFLECT_101 of index (array) i into [0, n), closed form."""
    i = np.asarray(i, np.int64)
    if n == 1:
        return np.zeros_like(i)
    p = 2 * n - 2
    m = np.mod(i, p)
    return np.where(m >= n, p - m, m)


def folds(i, n):
    """How often reflect101's loop (`while (i < 0 || i >= n) i = i < 0 ? -i : 2n - 2 - i`) turns for index i.  n == 1, where the loop would
    never end and reflect101 returns 0 before it, counts as 2 for any i outside: more than one fold, by the special case."""
    if n == 1:
        return 2 * (i != 0)
    k = 0
    while i < 0 or i >= n:
        i = -i if i < 0 else 2 * n - 2 - i
        k += 1
    return k


def pyr_down_ref(img):
    a = np.asarray(img)
    assert a.dtype == np.uint8 and a.ndim == 2 and a.size > 0
    h, w = a.shape
    dh, dw = (h + 1) // 2, (w + 1) // 2
    a = a.astype(np.int64)
    k = (1, 4, 6, 4, 1)
    ys, xs = 2 * np.arange(dh) - 2, 2 * np.arange(dw) - 2
    acc = np.zeros((dh, dw), np.int64)
    for j in range(5):
        rows = a[fold101(ys + j, h)]
        for i in range(5):
            acc += k[j] * k[i] * rows[:, fold101(xs + i, w)]
    assert acc.max() <= 255 * 256
    return ((acc + 128) >> 8).astype(np.uint8)


# ---- b. the host's choices ---------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Call:
    """One call: kind "down" (vstab_pyr_down), "x2" (vstab_pyr_down_x2) or "pack" (launch_pack_pyr).  A plane is (base % 16, pitch).
    src: the source / the luma plane.  dst: the level written (x2: the second one; pack: level 1).  mid: x2's first level.
    uv: pack's chroma plane.  ring: pack's ring base % 16 (its pitch is sw).  what: the paths the case is there for."""
    kind: str
    sw: int
    sh: int
    src: tuple
    dst: tuple
    mid: tuple = None
    uv: tuple = None
    ring: int = 0
    what: tuple = ()

    @property
    def id(self):
        s = f"{self.kind}-{self.sw}x{self.sh}-s{self.src[0]}.{self.src[1]}"
        if self.mid:
            s += f"-m{self.mid[0]}.{self.mid[1]}"
        s += f"-d{self.dst[0]}.{self.dst[1]}"
        if self.uv:
            s += f"-u{self.uv[0]}.{self.uv[1]}-r{self.ring}"
        return s


def a4(plane):
    return plane[0] % 4 == 0 and plane[1] % 4 == 0


PyrGrid = collections.namedtuple("PyrGrid", "n_groups g_lo g_hi nbx nb_int nb_edge")


def pyr_grid(sw, dw, dh, wide):
    n_groups, g_lo = div_up(dw, 4), 1
    g_hi = max(g_lo, min((sw - 12) // 8 + 1 if sw >= 12 else 0, dw // 4)) if wide else g_lo
    nbx = div_up(g_hi - g_lo, 64)
    return PyrGrid(n_groups, g_lo, g_hi, nbx, nbx * div_up(dh, 4), div_up(dh * (n_groups - (g_hi - g_lo)), 256))


def down_refusal(sw, sh, src, dst):
    """-> (status, message) of vstab_pyr_down for non-null planes; (OK, None) if it launches."""
    if sw <= 0 or sh <= 0 or src[1] < sw or dst[1] < (sw + 1) // 2:
        return ERR_INVALID, MSG_DOWN_ARG
    if src[1] * sh >= G4 or dst[1] * ((sh + 1) // 2) >= G4:
        return ERR_INVALID, MSG_DOWN_4G
    return OK, None


def down_host(sw, sh, src, dst):
    dw, dh = (sw + 1) // 2, (sh + 1) // 2
    vec_ok = a4(src) and a4(dst)
    near = sw >= 16 and sh >= 4
    return dict(sw=sw, sh=sh, dw=dw, dh=dh, vec_ok=vec_ok, near=near, grid=pyr_grid(sw, dw, dh, vec_ok and near))


def x2_ok(sw, sh):
    return (sw + 1) // 2 >= 8 and (sh + 1) // 2 >= 8


def x2_refusal(sw, sh, src, mid, dst):
    """-> (status, message) of vstab_pyr_down_x2 for non-null planes."""
    mw, mh = (sw + 1) // 2, (sh + 1) // 2
    if sw <= 0 or sh <= 0 or src[1] < sw or mid[1] < mw or dst[1] < (mw + 1) // 2:
        return ERR_INVALID, MSG_X2_ARG
    if not x2_ok(sw, sh):
        st = down_refusal(sw, sh, src, mid)
        return st if st[0] != OK else down_refusal(mw, mh, mid, dst)
    if src[1] * sh >= G4 or mid[1] * mh >= G4 or dst[1] * ((mh + 1) // 2) >= G4:
        return ERR_INVALID, MSG_X2_4G
    return OK, None


def x2_host(c):
    mw, mh = (c.sw + 1) // 2, (c.sh + 1) // 2
    dw, dh = (mw + 1) // 2, (mh + 1) // 2
    return dict(sw=c.sw, sh=c.sh, mw=mw, mh=mh, dw=dw, dh=dh, fallback=not x2_ok(c.sw, c.sh), vec_ok=a4(c.src) and a4(c.mid), dst_vec_ok=a4(c.dst),
                near=c.sw >= 16 and c.sh >= 4, tiles_x=div_up(dw, P2_TW), tiles_y=div_up(dh, P2_TH))


def pack_ok(c):
    """pack_pyr_ok from the Call's (base % 16, pitch) pairs."""
    w, h = c.sw, c.sh
    return (w >= 16 and h >= 4 and w % 8 == 0 and h % 2 == 0 and a4(c.src) and c.ring % 8 == 0 and a4(c.dst) and c.src[1] < (1 << 24) and c.uv[1] < (1 << 24)
            and c.src[1] * h < G4 and c.uv[1] * (h // 2) < G4 and c.dst[1] * ((h + 1) // 2) < G4 and w * h * 3 // 2 < G4)


def pack_host(c):
    dw, dh = (c.sw + 1) // 2, (c.sh + 1) // 2
    causes = [n for n, bad in (("chroma_base", c.uv[0] % 16 != 0), ("chroma_pitch", c.uv[1] % 16 != 0), ("width", c.sw % 16 != 0), ("ring_base", c.ring % 16 != 0))
              if bad]
    return dict(sw=c.sw, sh=c.sh, dw=dw, dh=dh, ok=pack_ok(c), grid=pyr_grid(c.sw, dw, dh, True), uv_vec=not causes, uv_causes=causes,
                nb_uv=max(1, min(256, div_up(c.sw * (c.sh // 2), 256 * 16))))


# ---- c. the paths --------------------------------------------------------------------------------------------------------------------
DOWN_PATHS = frozenset("int_fast int_top int_bottom_even int_bottom_odd edge_dword edge_left edge_right edge_all_bytes far far_multi_fold store_partial "
                       "edge_blocks_many int_blocks_many_x".split())
X2_PATHS = frozenset("tile_interior_dst_dword tile_interior_dst_bytes tile_border mid_dword mid_bytes region_skipped second_reflect_left second_reflect_right "
                     "second_reflect_top second_reflect_bottom second_clipped far fallback_two_launches".split())
PACK_PATHS = frozenset("copy_int_fast copy_int_rows copy_edge uv_vec uv_bytes_chroma_base uv_bytes_chroma_pitch uv_bytes_width uv_bytes_ring_base refused".split())


def decode_grid(G, dh):
    """Every (block, thread) of the grid of k_pyr_down / k_pack_pyr's pyramid part, decoded as pyr_down_dispatch does.
    -> (g, y) of the live edge threads and (g, y) of the live interior threads, four int arrays in grid order."""
    n_edge = G.n_groups - (G.g_hi - G.g_lo)
    e = np.arange(G.nb_edge * 256)                       # e = blockIdx.x * 256 + threadIdx.x
    y = e // n_edge
    i = e - y * n_edge
    g = np.where(i < G.g_lo, i, G.g_hi + (i - G.g_lo))
    live = y < dh
    eg, ey = g[live], y[live]
    b = np.arange(G.nb_int)                              # b = blockIdx.x - nb_edge
    by = b // max(G.nbx, 1)
    bx = b - by * G.nbx
    t = np.arange(256)
    g = (G.g_lo + bx[:, None] * 64 + (t & 63)[None, :]).ravel()
    y = (by[:, None] * 4 + (t >> 6)[None, :]).ravel()
    live = (g < G.g_hi) & (y < dh)
    return eg, ey, g[live], y[live]


def _interior_rows(P, ys, sh, names):
    """Count the interior groups of rows ys under names = (fast, top, bottom_even, bottom_odd)."""
    for y in ys.tolist():
        if y >= 1 and 2 * y + 2 < sh:
            P[names[0]] += 1
        elif y < 1:
            P[names[1]] += 1
        elif 2 * y + 2 == sh:
            P[names[2]] += 1
        else:
            assert 2 * y + 1 == sh, (y, sh)
            P[names[3]] += 1


def multi_fold_taps(sw, sh):
    """Taps of stored outputs whose index folds more than once (columns, rows)."""
    dw, dh = (sw + 1) // 2, (sh + 1) // 2
    cols = sum(folds(2 * x - 2 + i, sw) > 1 for x in range(dw) for i in range(5))
    rows = sum(folds(2 * y - 2 + j, sh) > 1 for y in range(dh) for j in range(5))
    return cols, rows


def down_paths(sw, sh, src, dst):
    """-> Counter: path name -> how many groups (dword columns for the edge_* names; 1 for the names of the whole launch) take it."""
    H = down_host(sw, sh, src, dst)
    G, dw, dh = H["grid"], H["dw"], H["dh"]
    P = collections.Counter()
    eg, ey, ig, iy = decode_grid(G, dh)
    _interior_rows(P, iy, sh, ("int_fast", "int_top", "int_bottom_even", "int_bottom_odd"))
    for g, n in zip(*np.unique(eg, return_counts=True)):
        for q in range(4):
            gx = 8 * int(g) - 4 + 4 * q
            if H["vec_ok"] and gx >= 0 and gx + 4 <= sw:
                P["edge_dword"] += int(n)
                continue
            P["edge_left"] += int(n) * (gx < 0)
            P["edge_right"] += int(n) * (gx + 4 > sw)
            P["edge_all_bytes"] += int(n) * (not H["vec_ok"])
    if not H["near"]:
        P["far"] = len(eg)
        P["far_multi_fold"] = sum(multi_fold_taps(sw, sh))
    P["store_partial"] = dh * (dw % 4 != 0)
    P["edge_blocks_many"] = int(G.nb_edge >= 2)
    P["int_blocks_many_x"] = int(G.nbx >= 2)
    return +P


@dataclasses.dataclass
class Tile:
    """One workgroup of k_pyr_down_x2: what it computes, stores and reads."""
    bx: int
    by: int
    interior: bool
    written: np.ndarray          # (P2_MH, P2_MW) bool: region bytes written to LDS
    mid: list                    # (my, mx, n bytes, "dword" | "bytes") first-level stores
    out: list                    # (y, x, n bytes, "dword" | "bytes") second-level stores
    reads: list                  # per output of a border tile: (5 region rows, 5 region columns) its taps read
    paths: collections.Counter


def x2_tile(H, bx, by):
    sw, sh, mw, mh, dw, dh = (H[k] for k in ("sw", "sh", "mw", "mh", "dw", "dh"))
    x0, y0 = bx * P2_TW, by * P2_TH
    mx0, my0 = 2 * x0 - 4, 2 * y0 - 2
    interior = (H["vec_ok"] and mx0 >= 2 and my0 >= 1 and mx0 + P2_MW <= mw and my0 + P2_MH <= mh and 2 * (mx0 + P2_MW) + 4 <= sw
                and 2 * (my0 + P2_MH) + 1 <= sh)
    T = Tile(bx, by, interior, np.zeros((P2_MH, P2_MW), bool), [], [], [], collections.Counter())
    P = T.paths
    for it in range(P2_ITEMS):               # one item per thread: tid = it
        ry, g = divmod(it, P2_MG)
        my, mx = my0 + ry, mx0 + 4 * g
        owns = 1 <= g <= P2_TW // 2 and 2 <= ry < 2 + 2 * P2_TH
        if interior:
            T.written[ry, 4 * g:4 * g + 4] = True
            if owns:
                T.mid.append((my, mx, 4, "dword"))
            continue
        if my < 0 or my >= mh or mx < 0 or mx >= mw:
            P["region_skipped"] += 1
            continue
        T.written[ry, 4 * g:4 * g + 4] = True
        if owns:
            if H["vec_ok"] and mx + 4 <= mw:
                T.mid.append((my, mx, 4, "dword"))
                P["mid_dword"] += 1
            else:
                T.mid.append((my, mx, min(4, mw - mx), "bytes"))
                P["mid_bytes"] += 1
    if interior:
        kind = "dword" if H["dst_vec_ok"] else "bytes"
        P["tile_interior_dst_" + kind] += 1
        for tid in range((P2_TW // 4) * P2_TH):
            ty, g = divmod(tid, P2_TW // 4)
            T.out.append((y0 + ty, x0 + 4 * g, 4, kind))
        return T
    P["tile_border"] += 1
    for e in range(P2_TW * P2_TH):
        ty, tx = divmod(e, P2_TW)
        x, y = x0 + tx, y0 + ty
        if x >= dw or y >= dh:
            P["second_clipped"] += 1
            continue
        cx, cy = 2 * x - 2 + np.arange(5), 2 * y - 2 + np.arange(5)
        P["second_reflect_left"] += int((cx < 0).any())
        P["second_reflect_right"] += int((cx >= mw).any())
        P["second_reflect_top"] += int((cy < 0).any())
        P["second_reflect_bottom"] += int((cy >= mh).any())
        T.reads.append((fold101(cy, mh) - my0, fold101(cx, mw) - mx0))
        T.out.append((y, x, 1, "bytes"))
    return T


def x2_tiles(c):
    H = x2_host(c)
    assert not H["fallback"]
    return H, [x2_tile(H, bx, by) for by in range(H["tiles_y"]) for bx in range(H["tiles_x"])]


def x2_paths(c):
    H = x2_host(c)
    if H["fallback"]:
        return collections.Counter(fallback_two_launches=1)
    P = collections.Counter()
    tiles = [x2_tile(H, bx, by) for by in range(H["tiles_y"]) for bx in range(H["tiles_x"])]
    for T in tiles:
        P += T.paths
    if not H["near"]:
        P["far"] = sum(not T.interior for T in tiles)
    return +P


def pack_paths(c):
    H = pack_host(c)
    if not H["ok"]:
        return collections.Counter(refused=1)
    P = collections.Counter()
    eg, ey, ig, iy = decode_grid(H["grid"], H["dh"])
    _interior_rows(P, iy, c.sh, ("copy_int_fast", "copy_int_rows", "copy_int_rows", "copy_int_rows"))
    P["copy_edge"] = len(eg)
    P["copy_edge_clipped"] = int(sum(8 * int(g) + b >= c.sw for g in eg for b in range(8)))
    if H["uv_vec"]:
        P["uv_vec"] = 1
    for cause in H["uv_causes"]:
        P["uv_bytes_" + cause] = 1
    return +P


def paths(c):
    return down_paths(c.sw, c.sh, c.src, c.dst) if c.kind == "down" else x2_paths(c) if c.kind == "x2" else pack_paths(c)


# ---- d. the cases --------------------------------------------------------------------------------------------------------------------
def _tight(w):
    return (0, w)


def _down(sw, sh, src=None, dst=None, what=()):
    dw = (sw + 1) // 2
    return Call("down", sw, sh, src or _tight(sw), dst or _tight(dw), what=tuple(what))


def _down_cases():
    cases = []
    # every width 1 .. 24 at heights 1 .. 6, dense planes: widths 1 .. 4 (a tap leaves the image twice), the far / near thresholds sw = 16
    # and sh = 4, every residue of dw mod 4, odd and even heights.  Odd widths have an odd pitch, so vec_ok is off there.
    named = {
        (1, 1): ("far", "far_multi_fold"), (2, 2): ("far_multi_fold",), (2, 5): ("far_multi_fold",), (5, 2): ("far_multi_fold",),
        (15, 6): ("far", "edge_right"), (16, 3): ("far", "edge_dword"), (16, 4): ("edge_dword", "edge_left", "edge_right"),
        (24, 4): ("int_top", "int_bottom_even"),                 # dense and aligned (sw % 8 == 0): the interior group g = 1, no fast row
        (24, 5): ("int_top", "int_fast", "int_bottom_odd"),
        (24, 6): ("int_top", "int_fast", "int_bottom_even"),
        (18, 5): ("store_partial",), (23, 5): ("edge_all_bytes",),
    }
    for sh in range(1, 7):
        for sw in range(1, 25):
            what = named.get((sw, sh), ("far",) if sw < 16 or sh < 4 else ("edge_left",))
            if (sw <= 2 or sh <= 2) and "far_multi_fold" not in what:
                what += ("far_multi_fold",)
            cases.append(_down(sw, sh, what=what))
    # 20 x 5 is the first image with an interior group (g = 1: 8 + 12 <= sw) and one fast row between a top and a bottom row; its level is 10
    # wide, so the output pitch is 12.  20 x 4 has no fast row, 20 x 6 an even bottom.
    cases.append(_down(20, 4, dst=(0, 12), what=("int_top", "int_bottom_even")))
    cases.append(_down(20, 5, dst=(0, 12), what=("int_top", "int_fast", "int_bottom_odd", "store_partial")))
    cases.append(_down(20, 6, dst=(0, 12), what=("int_top", "int_fast", "int_bottom_even")))
    # source layouts at 44 x 9 (dw = 22, dh = 5: two row blocks, a partial last group; interior groups 1 .. 4 where aligned) into a 4-aligned
    # output: base 0 .. 3 past a 16-byte boundary x pitch = width, 4-aligned and wider, odd and wider
    for off in range(4):
        for pitch in (44, 52, 47):
            ok = off == 0 and pitch % 4 == 0
            cases.append(_down(44, 9, (off, pitch), (0, 24), ("int_fast", "int_bottom_odd", "store_partial") if ok else ("edge_all_bytes", "store_partial")))
    cases.append(_down(45, 9, (0, 45), (0, 24), ("edge_all_bytes",)))          # an odd pitch that is the width
    # output layouts, the source dense and aligned: dense (22 is no multiple of 4, 24 is), 4-aligned and wider, odd, base + 1, base + 2
    for sw in (44, 48):
        dw = sw // 2
        for dst in ((0, dw), (0, al(dw, 4) + 4), (0, al(dw, 4) + 5), (1, al(dw, 4) + 4), (2, al(dw, 4) + 4), (4, al(dw, 4) + 8), (12, al(dw, 4) + 4)):
            cases.append(_down(sw, 9, (0, sw), dst, ("int_fast",) if a4(dst) else ("edge_all_bytes",)))
    # both planes pitched and offset by a multiple of 4: still the dword paths
    cases.append(_down(44, 9, (8, 60), (4, 28), ("int_fast", "edge_dword")))
    # more than 256 edge groups: 13 groups a row x 21 rows, unaligned; and 2 edge groups a row x 130 rows, aligned
    cases.append(_down(100, 41, (1, 101), (0, 52), ("edge_blocks_many", "edge_all_bytes")))
    cases.append(_down(24, 260, what=("edge_blocks_many", "int_fast")))
    # more than 64 interior groups a row: sw = 532 is the first (g_hi = 66), three rows
    cases.append(_down(532, 5, dst=(0, 268), what=("int_blocks_many_x", "int_top", "int_fast", "int_bottom_odd")))
    cases.append(_down(600, 18, (0, 608), (0, 304), ("int_blocks_many_x", "int_bottom_even")))
    return cases


def _x2(sw, sh, src=None, mid=None, dst=None, what=()):
    mw = (sw + 1) // 2
    return Call("x2", sw, sh, src or _tight(sw), dst or _tight((mw + 1) // 2), mid=mid or _tight(mw), what=tuple(what))


def _x2_cases():
    cases = []
    # 140 x 83 is the smallest source with an interior tile (tile (1, 1) of 3 x 3); 144 x 84 has dense planes that are all 4-aligned.
    # All eight combinations of source, middle and destination being 4-aligned: the unaligned ones by an odd pitch or a base of 1 / 2 / 3.
    for sw, sh in ((140, 83), (144, 84)):
        mw = (sw + 1) // 2
        dw = (mw + 1) // 2
        for sa in (True, False):
            for ma in (True, False):
                for da in (True, False):
                    src = (0, al(sw, 4) + 4) if sa else ((0, sw + 3) if sh == 83 else (2, al(sw, 4)))
                    mid = (4, al(mw, 4) + 4) if ma else ((1, al(mw, 4)) if sh == 83 else (0, al(mw, 4) + 1))
                    dst = (8, al(dw, 4)) if da else ((0, al(dw, 4) + 3) if sh == 83 else (3, al(dw, 4) + 4))
                    what = ("tile_border",)
                    if sa and ma:
                        what += ("tile_interior_dst_dword" if da else "tile_interior_dst_bytes", "mid_dword")
                    else:
                        what += ("mid_bytes",)
                    cases.append(_x2(sw, sh, src, mid, dst, what))
    cases.append(_x2(144, 84, what=("tile_interior_dst_dword", "second_clipped", "region_skipped")))   # dense planes: every pitch is the width
    cases.append(_x2(140, 83, what=("mid_bytes", "second_reflect_right", "second_reflect_bottom")))    # dense: mw = 70, so vec_ok is off
    # the smallest two-level images: one tile, everything reflected and clipped
    cases.append(_x2(15, 15, what=("far", "second_reflect_left", "second_reflect_right", "second_reflect_top", "second_reflect_bottom", "second_clipped")))
    cases.append(_x2(15, 40, (0, 16), (0, 8), (0, 4), what=("far", "mid_dword")))
    cases.append(_x2(16, 16, what=("mid_dword", "region_skipped")))
    cases.append(_x2(16, 15, (1, 16), what=("mid_bytes",)))
    # two tiles a row and a column with ragged ends: mw = 35 (a clipped byte store at the right end of the first level), dw = 18, dh = 11
    cases.append(_x2(70, 43, (0, 72), (0, 36), (0, 20), what=("mid_bytes", "mid_dword", "second_clipped")))
    cases.append(_x2(65, 41, what=("tile_border",)))
    # the fallback: vstab_pyr_down_x2 on an image under 15 x 15 runs k_pyr_down twice
    for sw, sh in ((14, 30), (30, 14), (9, 9), (1, 1), (3, 2)):
        cases.append(_x2(sw, sh, what=("fallback_two_launches",)))
    cases.append(_x2(14, 15, (1, 17), (2, 9), (3, 5), what=("fallback_two_launches",)))
    return cases


def _pack(sw, sh, src=None, uv=None, ring=0, dst=None, what=()):
    dw = (sw + 1) // 2
    return Call("pack", sw, sh, src or _tight(sw), dst or _tight(dw), uv=uv or _tight(sw), ring=ring, what=tuple(what))


def _pack_cases():
    return [
        _pack(16, 4, what=("copy_edge", "uv_vec")),                          # the smallest legal frame: no interior group, every group copies by bytes
        _pack(24, 4, what=("copy_int_rows", "uv_bytes_width")),              # one interior group, rows 0 (top) and 1 (bottom) only
        _pack(32, 6, what=("copy_int_fast", "copy_int_rows", "uv_vec")),     # interior groups 1 and 2 with one fast row
        _pack(40, 8, what=("copy_int_fast", "uv_bytes_width")),              # sw % 16 == 8
        _pack(32, 6, src=(0, 48), what=("copy_int_fast", "uv_vec")),         # a luma pitch wider than the row
        _pack(32, 6, src=(4, 36), what=("copy_int_fast",)),                  # luma only 4-aligned
        _pack(32, 6, dst=(0, 20), what=("copy_int_fast",)),                  # a level-1 pitch wider than dw
        _pack(32, 6, dst=(4, 24), what=("copy_int_fast",)),
        _pack(32, 6, uv=(4, 32), what=("uv_bytes_chroma_base",)),
        _pack(32, 6, uv=(0, 36), what=("uv_bytes_chroma_pitch",)),
        _pack(32, 6, uv=(0, 48), what=("uv_vec",)),                          # a chroma pitch wider than the row, still 16-aligned
        _pack(32, 6, ring=8, what=("uv_bytes_ring_base",)),
        _pack(40, 8, uv=(0, 48), what=("uv_bytes_width",)),                  # sw % 16 == 8 alone: the chroma pitch is 16-aligned
        _pack(48, 10, uv=(1, 49), ring=8, what=("uv_bytes_chroma_base", "uv_bytes_chroma_pitch", "uv_bytes_ring_base")),
        # what pack_pyr_ok refuses
        _pack(20, 4, what=("refused",)),                                     # w % 8 != 0
        _pack(8, 4, what=("refused",)),                                      # w < 16
        _pack(32, 5, what=("refused",)),                                     # odd h
        _pack(32, 2, what=("refused",)),                                     # h < 4
        _pack(32, 6, src=(2, 32), what=("refused",)),                        # luma base 2 past alignment
        _pack(32, 6, src=(0, 34), what=("refused",)),                        # luma pitch
        _pack(32, 6, ring=4, what=("refused",)),                             # ring 4 past alignment
        _pack(32, 6, dst=(0, 18), what=("refused",)),                        # dpitch % 4 != 0
        _pack(32, 6, dst=(2, 16), what=("refused",)),                        # level-1 base
    ]


DOWN_CASES, X2_CASES, PACK_CASES = _down_cases(), _x2_cases(), _pack_cases()
TABLES = {"down": (DOWN_CASES, DOWN_PATHS), "x2": (X2_CASES, X2_PATHS), "pack": (PACK_CASES, PACK_PATHS)}

# The planes just under 4 GiB: a 144 x 84 source whose pitch is the largest multiple of 4 with pitch * 84 < 2^32 -- its last rows start near 2^32.
BIG_W, BIG_H = 144, 84
BIG_PITCH = (G4 - 1) // BIG_H // 4 * 4


def content(kind, seed, w, h):
    """The planes the GPU tests run on: "random" bytes, or "extreme" -- every byte 0 or 255 at random (no two neighbours tied together, so a
    swapped or dropped byte shows), with a solid 255 block at the top left, border included, and a solid 0 block at the bottom right: sums
    of exactly 255 * 256 + 128 and of 128 at the dot-product accumulators and the byte extraction, and everything between."""
    rng = np.random.default_rng(seed)
    if kind == "random":
        return rng.integers(0, 256, (h, w), dtype=np.uint8)
    a = (rng.integers(0, 2, (h, w)) * 255).astype(np.uint8)
    a[: max(3, (h + 2) // 3), : max(3, (w + 2) // 3)] = 255     # (three rows and columns: with the reflection, all 25 taps of output (0, 0))
    a[h - h // 4:, w - w // 4:] = 0
    return a


# ---- e. planes on the device -----------------------------------------------------------------------------------------------------------
FENCE, GUARD_ROWS = 0xC5, 3


class Fenced:
    """A device plane of rows x rb bytes at base % 16 == off with pitch `pitch`, inside a buffer filled with FENCE: GUARD_ROWS rows of pitch
    bytes (and the offset) above, as many below, and the pitch padding right of every row.  view(): the (rows, rb) strided tensor a kernel
    writes through; ptr: its address.  host(): the plane's bytes, after asserting that every other byte of the buffer still holds FENCE."""

    def __init__(self, rows, rb, cuda, off=0, pitch=None, fill=FENCE):
        import torch
        pitch = rb if pitch is None else pitch
        assert pitch >= rb and 0 <= off < 16
        self.rows, self.rb, self.pitch, self.fill = rows, rb, pitch, fill
        self.lead = al(GUARD_ROWS * pitch + 16, 16) + off
        self.buf = torch.full((self.lead + rows * pitch + GUARD_ROWS * pitch + 32,), fill, dtype=torch.uint8, device=cuda)
        assert self.buf.data_ptr() % 16 == 0
        self.ptr = self.buf.data_ptr() + self.lead

    def view(self):
        import torch
        return torch.as_strided(self.buf, (self.rows, self.rb), (self.pitch, 1), self.lead)

    def host(self):
        a = self.buf.cpu().numpy()
        inside = np.zeros(a.shape, bool)
        idx = self.lead + np.arange(self.rows)[:, None] * self.pitch + np.arange(self.rb)[None, :]
        inside[idx] = True
        bad = np.flatnonzero(~inside & (a != self.fill))
        assert bad.size == 0, (f"{bad.size} bytes written outside the {self.rows} x {self.rb} plane (pitch {self.pitch}); the first at byte "
                               f"{int(bad[0]) - self.lead} from the plane's base (row {(int(bad[0]) - self.lead) // self.pitch}, "
                               f"column {(int(bad[0]) - self.lead) % self.pitch})")
        return a[idx]

    def untouched(self):
        """Nothing at all was written: plane and fences."""
        return bool((self.buf == self.fill).all().item())


def place(img, cuda, off=0, pitch=None, seed=0):
    """The (h, w) host plane at base % 16 == off with pitch `pitch` in a device buffer of junk bytes -> (buffer, strided (h, w) view)."""
    import torch
    h, w = img.shape
    pitch = w if pitch is None else pitch
    assert pitch >= w and 0 <= off < 16
    lead = 16 + off
    junk = np.random.default_rng(1000 + seed).integers(0, 256, lead + h * pitch + 48, dtype=np.uint8)
    buf = torch.from_numpy(junk).to(cuda)
    assert buf.data_ptr() % 16 == 0
    v = torch.as_strided(buf, (h, w), (pitch, 1), lead)
    v.copy_(torch.from_numpy(np.array(img)))      # (a copy: the shared references are read-only)
    return buf, v
