"""The zero stores of dead tiles in the 8-bit fused kernels' BGR output against the oracle, bit for bit, at every destination alignment and
every strip height: mode 5 against the reference's createMap kernel, mode 0 against the IEEE map.  The destination is a canaried buffer
compared WHOLE -- guard rows, pitch padding and the bytes before an offset base included -- so a store that leaves its strip shows up.
Every case first asserts with the CPU model of the rule (dead_tiles.py) that some dead tiles are full (all 64 columns and all rows inside
the output: the store phase's fast path), that others are ragged (last tile column, rows cut by the output's height) and that some tile
is cut by the source edge.  Strip heights: RW 4 (64 x 16 tiles of the small outputs, and the half-height tail of the 64 x 32 kernel),
RW 2 (the half-height tail of the 64 x 16 kernel), RW 8 (64 x 32 tiles).  Destination pitch and base at every multiple of 4 mod 16, and an
odd pitch (byte stores).  Written for a 16-byte-per-lane store of a dead strip at 4-byte alignment, which was measured and not kept
(profiles/dead_store_4k.txt); the cases are the ones such a store has to pass, and they hold the present store code to the same."""
import ctypes

import numpy as np
import pytest

import dead_tiles as D
import layouts
import oracle
import synth

pytestmark = pytest.mark.gpu

PRESET = oracle.GOPRO_H4B_WIDE169_MEASURED
G = layouts.GUARD_ROWS
RV_BIG = [(0.01, -0.02, 0.005), (0.12, 0.2, -0.1)]


class Canvas:
    """A BGR destination of `rows` x `rb` bytes at `pitch`, its first byte at residue `base16` mod 16, in a buffer of canary bytes."""

    def __init__(self, rows, rb, cuda, pitch, base16=0):
        import torch
        self.rows, self.rb, self.pitch = rows, rb, pitch
        self.off = (base16 - G * pitch) % 16 + 16
        self.n = self.off + (rows + 2 * G) * pitch + 32
        self.buf = torch.full((self.n,), layouts.CANARY, dtype=torch.uint8, device=cuda)
        assert self.buf.data_ptr() % 16 == 0
        self.ptr = self.buf.data_ptr() + self.off + G * pitch
        assert self.ptr % 16 == base16

    def differs(self, exp):
        """Bytes of the whole buffer that are not `exp` inside the plane and the canary everywhere else."""
        want = np.full(self.n, layouts.CANARY, np.uint8)
        first = self.off + G * self.pitch
        rows = np.lib.stride_tricks.as_strided(want[first:], (self.rows, self.rb), (self.pitch, 1))
        rows[:] = np.ascontiguousarray(exp).reshape(self.rows, self.rb)
        return int((self.buf.cpu().numpy() != want).sum())


def run(vs, src, p, dw, dh, mode, canvas):
    pp = np.ascontiguousarray(p, np.float32)
    layouts._call(vs, "vstab_warp_nv12_ex", src.y, src.pitch_y, src.uv, src.pitch_uv, src.w, src.h, layouts._f(pp)[1], int(mode), int(vs.OUT_BGR8),
                  canvas.ptr, canvas.pitch, None, 0, dw, dh, vs._stream())


def expected(frame, p, dw, dh, mode):
    return oracle.warp_nv12_ref_gfx950(frame, p, dw, dh) if mode == 5 else oracle.warp_nv12_ex(frame, p, dw, dh, mode, 0)


def dead_census(p, dw, dh, sw, sh, th):
    """-> (dead tiles that are full, dead tiles that are ragged, tiles cut by the source edge, (the rule's grid of dead tiles, that of the full ones)) at tile height th."""
    r = D.rule(p, dw, dh, sw, sh, th)
    full = np.zeros_like(r)
    full[:dh // th, :dw // 64] = True
    live = D.live_pixels(p, dw, dh, sw, sh)
    cut = int((D.tiles_any(live, th) & D.tiles_any(~live, th)).sum())
    return int((r & full).sum()), int((r & ~full).sum()), cut, (r, r & full)


def reaches_both_paths(p, dw, dh, sw, sh, th, want=None):
    full, ragged, cut, grid = dead_census(p, dw, dh, sw, sh, th)
    assert full >= 1 and ragged >= 1 and cut >= 1, (dw, dh, th, full, ragged, cut)
    if want is not None:
        assert (full, ragged) == want, (dw, dh, th, full, ragged)
    return grid


def launcher_bands(vs, p, sw, sh, dw, dh):
    """The bands launch_warp_fused gives this launch (several rounds of tiles: weighed by cost), through the library's hooks."""
    rwb, lds_kb, tail = layouts.fused_launch(dw, dh)
    assert tail > 0
    u32p, ip, fp = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_float)
    lib = vs.lib
    lib.vstabx_band_costs.restype = lib.vstabx_weighted_bands.restype = ctypes.c_int
    lib.vstabx_band_costs.argtypes = [fp, ctypes.c_int] + [ctypes.c_int] * 5 + [u32p, ctypes.c_int]
    lib.vstabx_weighted_bands.argtypes = [ctypes.c_int] * 4 + [ctypes.c_double, u32p, ctypes.c_int, ip]
    n = -(-dh // (2 * rwb))
    cost, out, pf = np.zeros(n, np.uint32), np.zeros(19, np.int32), np.ascontiguousarray(p, np.float32)
    assert lib.vstabx_band_costs(pf.ctypes.data_as(fp), 0, sw, sh, dw, dh, 2 * rwb, cost.ctypes.data_as(u32p), n) == 0
    assert lib.vstabx_weighted_bands(dw, dh, rwb, lds_kb, tail, cost.ctypes.data_as(u32p), n, out.ctypes.data_as(ip)) == 0
    return [int(v) for v in out[:9]], [int(v) for v in out[9:17]]


def dead_in_tails(vs, p, sw, sh, dw, dh, grid_half):
    """Tiles of grid_half (half-height tiles, (rows, cols) bool) inside the bands' tails [split_y, band end)."""
    ts = 2 * layouts.fused_launch(dw, dh)[0]
    band_y, split_y = launcher_bands(vs, p, sw, sh, dw, dh)
    return sum(int(grid_half[sp // ts:-(-hi // ts)].sum()) for sp, hi in zip(split_y, band_y[1:]))


# pitch residues 0, 4, 8, 12 mod 16 at base 0, base residues 4, 8, 12 at pitch residue 0, two mixed ones, and the odd pitch (byte stores)
def alignments(rb):
    p16 = layouts._al(rb, 16) + 48
    return [(p16 + dp, b) for dp, b in ((0, 0), (4, 0), (8, 0), (12, 0), (0, 4), (0, 8), (0, 12), (4, 12), (12, 4), (8, 8))] + [(p16 + 1, 0)]


SMALL = {(256, 144): ((-0.2, -0.15, 0.05), (230, 131), (2, 3)), (250, 142): ((0.3, 0.3, 0.3), (273, 157), (5, 4))}


@pytest.fixture(scope="module")
def small_cases():
    """(w, h) -> frame, params, output size, expected BGR per mode: computed once, shared by the alignments."""
    out = {}
    for (w, h), (rv, size, _) in SMALL.items():
        f = synth.nv12(70 + w, w, h)
        K = oracle.get_preset_camera(PRESET, w, h)
        Ko, (cw, ch) = oracle.get_output_camera(K, w, h)
        assert (cw, ch) == size
        p = oracle.map_params(K, Ko, oracle.rodrigues(rv))
        out[(w, h)] = (f, p, cw, ch, {mode: expected(f, p, cw, ch, mode) for mode in (0, 5)})
    return out


@pytest.mark.parametrize("w,h", list(SMALL))
def test_rw4_every_alignment(vs, cuda, small_cases, w, h):
    """64 x 16 tiles (RW 4), all resident at once."""
    f, p, cw, ch, exp = small_cases[(w, h)]
    assert layouts.fused_launch(cw, ch) == (4, 20, 0.0)
    reaches_both_paths(p, cw, ch, w, h, 16, SMALL[(w, h)][2])
    src = layouts.place(f[:h], f[h:], "decoder", cuda)
    for pitch, base in alignments(3 * cw):
        for mode in (0, 5):
            c = Canvas(ch, 3 * cw, cuda, pitch, base)
            run(vs, src, p, cw, ch, mode, c)
            assert c.differs(exp[mode]) == 0, (w, h, mode, pitch % 16, base, c.differs(exp[mode]))


@pytest.fixture(scope="module")
def frame_720():
    return synth.nv12(78, 1280, 720)


@pytest.mark.parametrize("rv,want", list(zip(RV_BIG, [(1364, 97), (985, 42)])))
def test_rw2_half_height_tail_of_the_64x16_kernel(vs, cuda, frame_720, rv, want):
    """A stateless 2040 x 1050 output of a 1280 x 720 source: 64 x 16 tiles in several rounds, so every band ends in 64 x 8 tiles
    (RW 2); more than 1,000 dead ones lie inside the bands' tails, more than 900 of them full."""
    w, h, dw, dh = 1280, 720, 2040, 1050
    K = oracle.get_preset_camera(PRESET, w, h)
    Ko, _ = oracle.get_output_camera(K, w, h)
    Ko = Ko.copy()
    Ko[0, 2], Ko[1, 2] = (dw - 1) / 2, (dh - 1) / 2
    assert layouts.fused_launch(dw, dh) == (4, 20, 0.5)
    p = oracle.map_params(K, Ko, oracle.rodrigues(rv))
    reaches_both_paths(p, dw, dh, w, h, 16, want)
    dead8, full8 = reaches_both_paths(p, dw, dh, w, h, 8)
    assert dead_in_tails(vs, p, w, h, dw, dh, dead8) > 1000 and dead_in_tails(vs, p, w, h, dw, dh, full8) > 900
    src = layouts.place(frame_720[:h], frame_720[h:], "packed", cuda)
    for mode in (0, 5):
        exp = expected(frame_720, p, dw, dh, mode)
        c = Canvas(dh, 3 * dw, cuda, layouts._al(3 * dw, 16) + 52, 8)
        run(vs, src, p, dw, dh, mode, c)
        assert c.differs(exp) == 0, (rv, mode, c.differs(exp))


@pytest.fixture(scope="module")
def frame_1080():
    return synth.nv12(77, 1920, 1080)


@pytest.mark.parametrize("rv,want", list(zip(RV_BIG, [((905, 75), (1879, 109)), ((533, 28), (1126, 29))])))
def test_rw8_and_its_half_height_rw4(vs, cuda, frame_1080, rv, want):
    """A stateless 3050 x 1010 output (64 x 32 tiles with a half-height tail; the last tile column 42 pixels wide, the last tile row 18
    rows high) of a 1920 x 1080 source at 0.9 of the output camera's focal length.
    Every alignment for the first rotation, one for the second."""
    w, h, dw, dh = 1920, 1080, 3050, 1010
    K = oracle.get_preset_camera(PRESET, w, h)
    Ko, _ = oracle.get_output_camera(K, w, h)
    Ko = Ko.copy()
    Ko[0, 0], Ko[1, 1] = 0.9 * Ko[0, 0], 0.9 * Ko[1, 1]
    Ko[0, 2], Ko[1, 2] = (dw - 1) / 2, (dh - 1) / 2
    assert layouts.fused_launch(dw, dh) == (8, 40, 0.5)
    p = oracle.map_params(K, Ko, oracle.rodrigues(rv))
    reaches_both_paths(p, dw, dh, w, h, 32, want[0])
    _, full16 = reaches_both_paths(p, dw, dh, w, h, 16, want[1])
    assert dead_in_tails(vs, p, w, h, dw, dh, full16) >= 1
    src = layouts.place(frame_1080[:h], frame_1080[h:], "packed", cuda)
    every = alignments(3 * dw)
    for mode in (0, 5):
        exp = expected(frame_1080, p, dw, dh, mode)
        for pitch, base in (every if rv == RV_BIG[0] else every[7:8] + every[-1:]):
            c = Canvas(dh, 3 * dw, cuda, pitch, base)
            run(vs, src, p, dw, dh, mode, c)
            assert c.differs(exp) == 0, (rv, mode, pitch % 16, base, c.differs(exp))
