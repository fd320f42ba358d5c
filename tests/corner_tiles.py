"""The one-pass corner detector (k_corners_fused, then k_filter_keys; csrc/vstab_corners_fused.hip) restated per tile on the oracle's
eigenvalue map, and the frames that put its tiles, its k_filter_keys workgroups and its key buffer into a chosen state.  No GPU here.

A tile is 64 x 31 output pixels (TW x TH).  k_corners_fused takes the tile's own maximum over the in-image part of the 66 x 33
eigenvalues around it -- in the order of the floats' bits read as int32, which is the float order only while the maximum is not negative --
and keeps the tile's interior 3 x 3 maxima above quality * max(own maximum, frame maximum published so far): a count between

    lo  the survivors under the final threshold quality * max(frame), and
    hi  the survivors under quality * own maximum (every 3 x 3 maximum when the own maximum is negative: the threshold is -inf then),

depending on which tiles ran first.  With more than SLOTS survivors the tile hands over a dense map instead of keys.  k_filter_keys packs
FK_TILES tiles into a workgroup, FK_TILES / 4 consecutive ones per wave, applies the final threshold and appends: the keys of keyed tiles
through `kept` in LDS with one atomic per workgroup, those of spilled tiles row by row with one atomic per wave and row.

States of a tile:  keys (hi <= SLOTS), full (lo == hi == SLOTS), spills (lo > SLOTS), timing (lo <= SLOTS < hi: it spills in one run and
not in another), and negative_max beside them."""
import functools

import numpy as np

import oracle
import synth

TW, TH, SLOTS, FK_TILES = 64, 31, 256, 16
SPEC_CAP, KEY_CAP = 1 << 15, 1 << 18          # Detector::SPEC_CAP; the key capacity a Detector starts with
GROUND = 50


# ---- the model ---------------------------------------------------------------------------------------------------------------------
class Model:
    """Everything the tests compare with, for one luma frame and quality level."""

    def __init__(self, img, quality=0.01):
        img = np.ascontiguousarray(img, np.uint8)
        self.img, self.quality = img, quality
        h, w = img.shape
        self.w, self.h = w, h
        e = self.eig = oracle.min_eig(img)
        bits = e.view(np.int32)
        fmax = int(bits.max())
        assert fmax >= 0, "a frame whose maximum is negative: both kernels' int-ordered maximum means nothing there"
        self.frame_max = np.int32(fmax).view(np.float32)
        assert self.frame_max == e.max()
        self.thr = np.float32(np.float64(self.frame_max) * quality)
        pad = np.full((h + 2, w + 2), -np.inf, np.float32)
        pad[1:-1, 1:-1] = e
        m = e.copy()
        for dy in range(3):
            for dx in range(3):
                m = np.maximum(m, pad[dy:dy + h, dx:dx + w])
        inner = np.zeros((h, w), bool)
        inner[1:h - 1, 1:w - 1] = True
        self.is_max = inner & (e == m)
        self.final = self.is_max & (e > self.thr)
        ys, xs = np.nonzero(self.final)
        # what the detector hands to the host, sorted ascending: float bits << 32 | raster index
        self.keys = np.sort((e[ys, xs].view(np.uint32).astype(np.uint64) << np.uint64(32)) | (ys * w + xs).astype(np.uint64))
        self.n = len(self.keys)
        self.tiles_x, self.tiles_y = -(-w // TW), -(-h // TH)
        self.n_tiles = self.tiles_x * self.tiles_y
        shape = (self.tiles_y, self.tiles_x)
        self.own_bits = np.zeros(shape, np.int32)
        self.lo, self.hi = np.zeros(shape, np.int64), np.zeros(shape, np.int64)
        for ty in range(self.tiles_y):
            for tx in range(self.tiles_x):
                oy, ox = ty * TH, tx * TW
                own = int(bits[max(oy - 1, 0):min(oy + TH + 1, h), max(ox - 1, 0):min(ox + TW + 1, w)].max())
                thr_own = np.float32(np.float64(np.int32(own).view(np.float32)) * quality) if own >= 0 else np.float32(-np.inf)
                sl = (slice(oy, min(oy + TH, h)), slice(ox, min(ox + TW, w)))
                self.own_bits[ty, tx] = own
                self.lo[ty, tx] = int(self.final[sl].sum())
                self.hi[ty, tx] = int((self.is_max[sl] & (e[sl] > thr_own)).sum())
        assert (self.lo <= self.hi).all() and int(self.lo.sum()) == self.n
        self.negative_max = self.own_bits < 0
        self.spills = self.lo > SLOTS
        self.timing = (self.lo <= SLOTS) & (self.hi > SLOTS)
        self.keyed = self.hi <= SLOTS
        self.full = (self.lo == SLOTS) & (self.hi == SLOTS)

    def state(self, t):
        """the state of tile t (tile rows first)"""
        ty, tx = divmod(t, self.tiles_x)
        return "spills" if self.spills[ty, tx] else "timing" if self.timing[ty, tx] else "full" if self.full[ty, tx] else "keys"

    def spilled_range(self):
        """(fewest, most) tiles that hand over a dense map in a run"""
        return int(self.spills.sum()), int((self.hi > SLOTS).sum())

    def workgroups(self):
        """per k_filter_keys workgroup: its tiles, the tile rows they lie in, the keys it gathers in LDS (fewest, most: a timing tile's keys
        go through LDS only when it did not spill) and the waves (0..3) that hold both a tile that spills and a tile that hands over keys"""
        out = []
        lo, sp, tm, kd = self.lo.ravel(), self.spills.ravel(), self.timing.ravel(), self.keyed.ravel()
        for g in range(-(-self.n_tiles // FK_TILES)):
            tiles = list(range(g * FK_TILES, min((g + 1) * FK_TILES, self.n_tiles)))
            mixed = []
            for wv in range(4):
                mine = [t for t in tiles if (t - g * FK_TILES) // (FK_TILES // 4) == wv]
                if any(sp[t] for t in mine) and any(kd[t] and lo[t] > 0 for t in mine):
                    mixed.append(wv)
            out.append(dict(tiles=tiles, rows=sorted({t // self.tiles_x for t in tiles}), mixed_waves=mixed,
                            kept=(int(sum(lo[t] for t in tiles if kd[t])), int(sum(lo[t] for t in tiles if kd[t] or tm[t])))))
        return out

    def corners(self, max_corners, min_distance):
        return oracle.good_features(self.img, max_corners, self.quality, min_distance)


@functools.lru_cache(maxsize=None)
def model(name):
    """the model of a named set (SETS), computed once per process and shared"""
    return Model(make(name))


# ---- image builders ------------------------------------------------------------------------------------------------------------------
def checker(w, h, phase=0):
    """the 2-px checkerboard of 50 / 150, moved by `phase` px along both axes: its eigenvalue map is one plateau at the frame maximum"""
    return ((np.add.outer((np.arange(h) + phase) // 2, (np.arange(w) + phase) // 2) % 2) * 100 + GROUND).astype(np.uint8)


# Patches of checkerboard on a flat ground, (y0, y1, x0, x1) inside a 64 x 31 cell.  Every survivor sits at the frame maximum or within 1 %
# of it (the patch's rim), so lo == hi: the count does not depend on timing.  The numbered cells keep 4 px of ground to the cell's edge, so
# a tile's count is the cell's wherever the cell lies in a frame; "P" is a plateau (far over SLOTS), 0 is flat.  The E cells touch the
# image corner of a single-tile frame.  test_corner_tiles_cpu.py asserts every count.
CELLS = {
    0: [],
    255: [(4, 24, 4, 18), (4, 16, 24, 45)],
    256: [(4, 24, 4, 18), (4, 14, 24, 52)],
    257: [(4, 24, 4, 19), (4, 14, 24, 48)],
    258: [(4, 24, 4, 18), (4, 18, 24, 42)],
    "P": [(2, 29, 2, 62)],
    "E255": [(0, 21, 0, 19)],
    "E256": [(0, 29, 0, 13), (0, 8, 17, 30)],
    "E257": [(0, 23, 0, 18)],
    "E258": [(0, 23, 0, 18), (0, 3, 22, 25)],
}


def cell(patches):
    c = np.full((TH, TW), GROUND, np.uint8)
    ck = checker(TW, TH)
    for y0, y1, x0, x1 in patches:
        c[y0:y1, x0:x1] = ck[y0:y1, x0:x1]
    return c


def cells_frame(grid, w=None, h=None):
    """a frame of len(grid) x len(grid[0]) cells, each named by its survivor count in CELLS, cut to w x h"""
    img = np.vstack([np.hstack([cell(CELLS[c]) for c in row]) for row in grid])
    return np.ascontiguousarray(img[:h, :w])


def patched_checker(w, h, flat):
    """the checkerboard of w x h with the rectangles `flat` (y0, y1, x0, x1) set to the ground value: fewer survivors"""
    g = checker(w, h)
    for y0, y1, x0, x1 in flat:
        g[y0:y1, x0:x1] = GROUND
    return g


@functools.lru_cache(maxsize=None)
def _flat_deltas():
    """survivors that a flat rectangle of r x c at (10, 10) takes from a checkerboard (a local effect, measured on 120 x 120)"""
    full = Model(checker(120, 120)).n
    return {full - Model(patched_checker(120, 120, [(10, 10 + r, 10, 10 + c)])).n: (r, c) for r in range(2, 40) for c in range(2, 40)}


def tuned_checker(w, h, target):
    """the checkerboard of w x h, (w - 4)(h - 4) survivors, with one flat rectangle that leaves exactly `target`"""
    surplus = (w - 4) * (h - 4) - target
    assert surplus >= 0
    if surplus == 0:
        return checker(w, h)
    r, c = _flat_deltas()[surplus]       # KeyError: no single rectangle removes that many
    return patched_checker(w, h, [(10, 10 + r, 10, 10 + c)])


def ramp(w, h, a, b, c=0):
    """the linear ramp a x + b y + c (clipped to a byte): its eigenvalues are rounding noise around zero"""
    yy, xx = np.mgrid[0:h, 0:w]
    return np.clip(a * xx + b * yy + c, 0, 255).astype(np.uint8)


def stripes(w, h, kind, period=4):
    yy, xx = np.mgrid[0:h, 0:w]
    t = {"vertical": xx, "horizontal": yy, "diagonal": xx + yy}[kind]
    return np.where((t // (period // 2)) % 2 == 0, 200, 30).astype(np.uint8)


def timing_frame(w=320, h=124, seed=7):
    """Two tile rows of texture (synth.luma) over two flat ones that carry checkerboard patches of LOW contrast across the tile seams:
    their plateau lies above 1 % of such a tile's own maximum and below 1 % of the frame's, so those tiles spill or not by timing.  Two of
    them hold a rectangle of medium contrast as well, whose corners pass the final threshold: lo > 0."""
    g = synth.luma(seed, w, h).copy()
    lowc = ((np.add.outer(np.arange(h) // 2, np.arange(w) // 2) % 2) * 6 + 100).astype(np.uint8)
    g[2 * TH:] = 100
    for (y0, y1, x0, x1) in [(2 * TH + 6, 4 * TH - 6, 40, 90), (2 * TH + 6, 4 * TH - 6, 168, 216), (3 * TH - 12, 3 * TH + 12, 236, 300)]:
        g[y0:y1, x0:x1] = lowc[y0:y1, x0:x1]
    g[100:112, 100:120] = 120
    g[108:118, 222:232] = 120
    return g


# ---- the named sets --------------------------------------------------------------------------------------------------------------------
def _grid(tx, ty, fill, **at):
    """ty x tx cells of `fill`, with tile numbers (tile rows first) given as t<number>=<cell>"""
    g = [[fill] * tx for _ in range(ty)]
    for k, v in at.items():
        t = int(k[1:])
        g[t // tx][t % tx] = v
    return g


def _sets():
    s = {}
    for n in (255, 256, 257, 258):
        s[f"tile_{n}"] = lambda n=n: cells_frame([[f"E{n}"]])
        s[f"inset_{n}"] = lambda n=n: cells_frame([[n]])
    s["full_16"] = lambda: cells_frame(_grid(4, 4, 256))                                          # one workgroup, `kept` filled exactly
    s["mixed_wave"] = lambda: cells_frame(_grid(4, 2, 255, t1=257, t2="P", t6=256))                 # spills and keys in wave 0
    s["spill_last"] = lambda: cells_frame(_grid(3, 2, 255, t5=257))                                 # tile 5 of 6 spills: last of the grid
    # tile counts with every residue mod 4 and 1, 15, 16, 17 mod 16; tiles_x of 3, 5 and 7 make workgroups wrap over tile rows
    for tx, ty in GRIDS:
        s[f"grid_{tx}x{ty}"] = lambda tx=tx, ty=ty: cells_frame([[GRID_CELLS[(x * 5 + y * 3) % 6] for x in range(tx)] for y in range(ty)])
    # plateau tiles cut by the right and the bottom image edge: w mod 64 and h mod 31 in {1, 2, 63 / 30}
    for w, h in CUTS:
        s[f"cut_{w}x{h}"] = lambda w=w, h=h: checker(w, h)
    s["timing"] = timing_frame
    for k, (a, b, c) in enumerate(RAMPS):
        s[f"ramp_{k}"] = lambda a=a, b=b, c=c: ramp(RAMP_W, RAMP_H, a, b, c)
    for kind in ("vertical", "horizontal", "diagonal"):
        s[f"stripes_{kind}"] = lambda kind=kind: stripes(200, 95, kind)
    return s


GRIDS = ((1, 1), (2, 1), (3, 1), (5, 3), (4, 4), (17, 1), (3, 6), (7, 5), (5, 7))
GRID_CELLS = (255, 256, 257, 0, "P", 258)
CUTS = ((65, 32), (66, 33), (127, 61), (129, 63), (191, 92), (194, 95))
RAMP_W, RAMP_H = 150, 70
RAMPS = ((1, 0, 0), (0, 1, 0), (1, 1, 0), (1, 2, 3), (0.5, 0.25, 10), (0.3, 0.7, 0), (1.5, 0.1, 5))
SETS = _sets()


def make(name):
    return SETS[name]()


# the frames around the key capacity 2^18 of a fresh Detector (stateless operator)
def cap_frame(which):
    # 570 x 468 (570 x 464, whose plain checkerboard has 260,360, is under the capacity): 262,624 survivors, and a flat patch of 21 x 14
    # takes 480 of them, one of 23 x 13 takes 479 -- the same frame but for the patch on either side of the capacity
    return {"2^18": lambda: tuned_checker(570, 468, KEY_CAP), "2^18+1": lambda: tuned_checker(570, 468, KEY_CAP + 1)}[which]()


def banded(kind="at", phase=0, w=640, h=360):
    """Bands of checkerboard 30 rows apart on flat ground: 200 corners 30 px apart (a handle re-detects on EVERY frame while it has fewer
    than 150, and then never speculates).  kind "under": eleven bands of 8 rows, 21,010 candidates.  "at": exactly SPEC_CAP -- bands of 8,
    10 and 16 rows and a band of one candidate row cut at column 316 for the last few hundred.  "over": a 5 x 5 patch adds one.
    phase moves the checkerboard inside the bands, not the bands.  The counts above are those of phase 0 ONLY: at phase 1 the three
    kinds have 27,984, 40,048 and 40,050 candidates -- "at" is over SPEC_CAP there.  The pipeline's SPEC_CAP cases hold because the
    speculative detection reads frame 20, an even frame (phase 0); test_corner_tiles_cpu.py pins both phases."""
    ck = checker(w, h, phase)
    g = np.full((h, w), GROUND, np.uint8)
    for k, rows in enumerate((8,) * 11 if kind == "under" else (8, 8, 8, 8, 8, 8, 8, 8, 10, 16, 16)):
        g[10 + 30 * k:10 + 30 * k + rows] = ck[10 + 30 * k:10 + 30 * k + rows]
    if kind != "under":
        g[342:348, 4:316] = ck[342:348, 4:316]
    if kind == "over":
        g[341:346, 500:505] = ck[341:346, 500:505]
    return g


def pipeline_clip(which):
    """(luma size, packed NV12 frames) of the pipeline's clips.  The checkerboard of every odd frame is moved by one pixel along both axes
    (a clip that stands still has the rotation estimate at the identity, where the product and the oracle agree to 1.3e-9 only); the even
    frames, the detected ones among them, are the frame the counts are given for.  `under_spec_cap`, `at_spec_cap` and `over_spec_cap`
    (640 x 360, banded) have 21,010, exactly SPEC_CAP and SPEC_CAP + 1 candidates.  `middle_320` (the 320 x 180 checkerboard: 78 corners,
    so every frame is a key frame detected synchronously) and `middle` (480 x 270: 171 corners, a planned key frame at frame 21) lie
    between SPEC_CAP and the key capacity.  `large` is over the key capacity (3 frames: the seed detection overflows the fused detector)
    with 5 textured, moving frames behind it for the same handle: the tracker loses corners on the way into the texture, so the frames after
    it are key frames detected on textured frames."""
    if which == "large":
        K = oracle.get_preset_camera(4, 640, 480)
        return (640, 480), [nv12_of(checker(640, 480, k % 2)) for k in range(3)] + synth.shaky_clip(4, K, 640, 480, 5, sigma=0.004)[0]
    luma = {"middle_320": lambda p: checker(320, 180, p), "middle": lambda p: checker(480, 270, p), "under_spec_cap": lambda p: banded("under", p),
            "at_spec_cap": lambda p: banded("at", p), "over_spec_cap": lambda p: banded("over", p)}[which]
    two = [nv12_of(luma(0)), nv12_of(luma(1))]
    return (two[0].shape[1], two[0].shape[0] * 2 // 3), [two[k % 2] for k in range(25)]


def nv12_of(luma):
    """packed NV12 with grey chroma"""
    h, w = luma.shape
    out = np.full((h * 3 // 2, w), 128, np.uint8)
    out[:h] = luma
    return out
