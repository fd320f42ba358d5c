"""Waves of the fused warp kernels at the source edge (vstab_warp_fused.hip: edge_wave's EDGE_OUTSIDE and EDGE_CLAMP beside the
pixel-by-pixel path) against the oracle, bit for bit, into canaried planes.  Small sources (640 x 360, 256 x 144, 250 x 142) behind the
preset camera, so that the pincushion's edge crosses the tiles; the 64 x 16 kernels at the cameras' own outputs, the 64 x 32 kernels
with their half-height tail at a stateless 3100 x 1010 output (1,568 tiles of 64 x 32; neither size a multiple of the tile).
Before anything is compared, the CPU classifier (test_edge_waves_cpu.classify) must find in the shape the waves the case is about:
  mixed     a `clamp` wave with pixels wholly outside the source and pixels in the box
  outside   a wave wholly outside inside a tile that touches the source
  missed    a tile that is dead in truth and that the probe's rule leaves alive
  far+gather  a `gather` wave that also holds pixels wholly outside
and the rotations of the 64 x 16 cases between them put a footprint across each of the four edges and four corners of the source, in a
wave that also holds a pixel wholly outside.  Map mode 5 is held to the reference kernel's own map, as tests/expect.py does it."""
import numpy as np
import pytest

import dead_tiles as D
import distort_def as dd
import layouts
import oracle
import synth
from test_edge_waves_cpu import CLAMP, GATHER, OUTSIDE, PRESET, classify, straddles
from test_p010_cpu import p010_frame

pytestmark = pytest.mark.gpu

TOP, BOTTOM, STEEP = (0.026, -0.007, 0.004), (-0.037, 0.002, -0.003), (0.3, 0.3, 0.3)   # corners of the source: top pair, bottom pair; 30 degrees
BIG = (3100, 1010)


def camera(w, h, big=False):
    K = oracle.get_preset_camera(PRESET, w, h)
    Ko, (cw, ch) = oracle.get_output_camera(K, w, h)
    if big:       # the source seen four times enlarged in the middle of the stateless output
        cw, ch = BIG
        Ko = Ko.copy()
        Ko[0, 0], Ko[1, 1] = 4.0 * Ko[0, 0], 4.0 * Ko[1, 1]
        Ko[0, 2], Ko[1, 2] = (cw - 1) / 2, (ch - 1) / 2
    return K, Ko, cw, ch


def cases(mx, my, sw, sh, launch, p=None, dw=0, dh=0, vec=True, nan_behind=False, px=1):
    """-> {tile height: {case: count}} from the classifier, for the launch's tall and half-height tiles.  p: the rule's parameters where
    the kernel knows dead tiles."""
    rwb, lds_kb, _ = launch
    out = {}
    for rw in (rwb, rwb // 2):
        dead = D.rule(p, dw, dh, sw, sh, 4 * rw, nan_behind) if p is not None else None
        c = classify(mx, my, sw, sh, rwb, rw, lds_kb, vec, dead, px)
        k = c["kind"]
        out[4 * rw] = dict(mixed=int(((k == CLAMP) & (c["n_out"] > 0) & (c["n_in"] > 0)).sum()),
                           outside=int(((k == OUTSIDE) & c["live"][:, None, :]).sum()),
                           missed=int((~c["live"] & ~dead).sum()) if dead is not None else 0,
                           far_gather=int(((k == GATHER) & (c["n_out"] > 0)).sum()), clamp=int((k == CLAMP).sum()), kind=k)
    return out


def ieee_map(p, dw, dh, mode):
    return oracle.create_map_ex(p, dw, dh, 1) if mode == 1 else oracle.create_map(p, dw, dh)   # (mode 5: the same map to a fraction of a pixel)


def expected8(frame, p, dw, dh, mode, nv12):
    if mode == 5:
        bgr = oracle.warp_nv12_ref_gfx950(frame, p, dw, dh)
        return oracle.cvt_bgr_nv12(bgr) if nv12 else bgr
    return oracle.warp_nv12_ex(frame, p, dw, dh, mode, 1 if nv12 else 0)


def check8(vs, cuda, src, frame, p, dw, dh, mode, what):
    exp = expected8(frame, p, dw, dh, mode, False)
    got = layouts.warp_nv12(vs, src, p, dw, dh, mode, vs.OUT_BGR8, cuda)
    assert np.array_equal(got, exp), (what, "bgr", int((got != exp).any(axis=2).sum()))
    ey, euv = expected8(frame, p, dw, dh, mode, True)
    gy, guv = layouts.warp_nv12(vs, src, p, dw, dh, mode, vs.OUT_NV12, cuda)
    assert np.array_equal(gy, ey) and np.array_equal(guv, euv.reshape(guv.shape)), (what, "nv12")


@pytest.fixture(scope="module")
def frames():
    return {(w, h): synth.nv12(90 + w, w, h) for w, h in ((640, 360), (256, 144), (250, 142))}


@pytest.mark.parametrize("mode", [0, 1, 5])
@pytest.mark.parametrize("w,h", [(640, 360), (250, 142)])
def test_64x16_kernels(vs, cuda, frames, w, h, mode):
    """The cameras' own outputs (583 x 331 and 273 x 157: no multiple of 64 or 16).  250 is no multiple of the 8-pixel staging block: the
    tiles that reach the last block column are not staged, and their waves at the right edge gather beside pixels wholly outside."""
    f = frames[(w, h)]
    K, Ko, cw, ch = camera(w, h)
    launch = layouts.fused_launch(cw, ch)
    assert launch[0] == 4 and cw % 64 and ch % 16
    src = layouts.place(f[:h], f[h:], "decoder", cuda)
    found = set()
    for rv in (TOP, BOTTOM, STEEP):
        p = oracle.map_params(K, Ko, oracle.rodrigues(rv))
        mx, my = ieee_map(p, cw, ch, mode)
        found |= straddles(mx, my, w, h, 4)
        for th, c in cases(mx, my, w, h, launch, p, cw, ch, nan_behind=mode == 1).items():
            assert c["mixed"] >= 5 and c["outside"] >= 1 and c["missed"] >= 1, (w, h, mode, rv, th, c)
            assert c["far_gather"] >= 1 or (w % 8 == 0 and rv != STEEP), (w, h, mode, rv, th, "nothing to gather beside pixels wholly outside")
        check8(vs, cuda, src, f, p, cw, ch, mode, (w, h, mode, rv))
    assert found == {"left", "right", "top", "bottom", "top_left", "top_right", "bottom_left", "bottom_right"} or w != 640, found


@pytest.mark.parametrize("mode", [0, 5])
def test_64x32_kernels_and_their_tail(vs, cuda, frames, mode):
    w, h = 640, 360
    f = frames[(w, h)]
    K, Ko, dw, dh = camera(w, h, big=True)
    launch = layouts.fused_launch(dw, dh)
    assert launch == (8, 40, 0.5) and dw % 64 and dh % 32 and dh % 16
    s = layouts.tile_schedule(dw, dh, *launch)
    src = layouts.place(f[:h], f[h:], "packed", cuda)
    for rv in ((0.02, 0.015, 0.01), (0.1, -0.05, 0.5)):
        p = oracle.map_params(K, Ko, oracle.rodrigues(rv))
        c = cases(*ieee_map(p, dw, dh, mode), w, h, launch, p, dw, dh)
        for th in (32, 16):
            assert c[th]["mixed"] >= 20 and c[th]["outside"] >= 5 and c[th]["missed"] >= 5, (mode, rv, th, c[th])
        # both tile heights really meet such waves: the tall tiles of some band, the half-height tail of some band
        tall = any((c[32]["kind"][lo // 32:sp // 32] == CLAMP).any() for lo, sp in zip(s["band_y"], s["split_y"]))
        tail = any((c[16]["kind"][sp // 16:-(-hi // 16)] == CLAMP).any() for sp, hi in zip(s["split_y"], s["band_y"][1:]))
        assert tall and tail, (mode, rv, tall, tail)
        check8(vs, cuda, src, f, p, dw, dh, mode, ("big", mode, rv))


@pytest.mark.parametrize("mode", [0, 5])
def test_unaligned_planes_nothing_staged(vs, cuda, frames, mode):
    """4-byte aligned bases and pitches: no tile has a box in LDS.  Waves wholly outside are zeroed, every other wave is gathered."""
    w, h = 256, 144
    f = frames[(w, h)]
    K, Ko, cw, ch = camera(w, h)
    launch = layouts.fused_launch(cw, ch)
    src = layouts.place(f[:h], f[h:], "unaligned", cuda)
    for rv in (TOP, STEEP):
        p = oracle.map_params(K, Ko, oracle.rodrigues(rv))
        for th, c in cases(*ieee_map(p, cw, ch, mode), w, h, launch, p, cw, ch, vec=False).items():
            assert c["clamp"] == 0 and c["outside"] >= 1 and c["far_gather"] >= 5, (mode, rv, th, c)
        check8(vs, cuda, src, f, p, cw, ch, mode, ("unaligned", mode, rv))


@pytest.mark.parametrize("big", [False, True])
def test_rotation_per_row(vs, cuda, frames, big):
    """MAP_RS_*: map modes 0 and 1 with the last row turned by 0.4 degrees about y (no dead tiles in these kernels)."""
    w, h = 640, 360
    f = frames[(w, h)]
    K, Ko, dw, dh = camera(w, h, big)
    launch = layouts.fused_launch(dw, dh)
    src = layouts.place(f[:h], f[h:], "packed", cuda)
    a = np.deg2rad(0.4)
    turn = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    for mode in (1,) if big else (0, 1):
        p = oracle.map_params(K, Ko, oracle.rodrigues(TOP))
        rb = (turn @ np.asarray(p[8:17], np.float64).reshape(3, 3)).astype(np.float32)
        for th, c in cases(*oracle.create_map_rs(p, rb, dw, dh, mode), w, h, launch).items():
            assert c["mixed"] >= 5 and c["outside"] >= 1, (big, mode, th, c)
        exp = oracle.warp_nv12_rs(f, p, rb, dw, dh, mode, 0)
        got = layouts.warp_nv12(vs, src, p, dw, dh, mode, vs.OUT_BGR8, cuda, rot_bottom=rb)
        assert np.array_equal(got, exp), (big, mode, "bgr")
        if not big:
            ey, euv = oracle.warp_nv12_rs(f, p, rb, dw, dh, mode, 1)
            gy, guv = layouts.warp_nv12(vs, src, p, dw, dh, mode, vs.OUT_NV12, cuda, rot_bottom=rb)
            assert np.array_equal(gy, ey) and np.array_equal(guv, euv.reshape(guv.shape)), (big, mode, "nv12")


@pytest.mark.parametrize("big", [False, True])
def test_quantised_map_of_the_caller(vs, cuda, frames, big):
    """CACHED: the kernel reads the map's integers.  (The 64 x 32 kernel to BGR has EDGE_OUTSIDE only: edge_paths.)"""
    w, h = 640, 360
    f = frames[(w, h)]
    K, Ko, dw, dh = camera(w, h, big)
    launch = layouts.fused_launch(dw, dh)
    src = layouts.place(f[:h], f[h:], "packed", cuda)
    p = oracle.map_params(K, Ko, oracle.rodrigues(BOTTOM))
    for th, c in cases(*oracle.create_map(p, dw, dh), w, h, launch).items():
        assert c["mixed"] >= 5 and c["outside"] >= 1, (big, th, c)
    q = vs.quantised_map(p, dw, dh, mode=0)
    exp = oracle.warp_nv12_ex(f, p, dw, dh, 0, 0)
    got = layouts.warp_nv12_mapped(vs, src, q, dw, dh, vs.OUT_BGR8, cuda)
    assert np.array_equal(got, exp), (big, "bgr", int((got != exp).any(axis=2).sum()))
    ey, euv = oracle.warp_nv12_ex(f, p, dw, dh, 0, 1)
    gy, guv = layouts.warp_nv12_mapped(vs, src, q, dw, dh, vs.OUT_NV12, cuda)
    assert np.array_equal(gy, ey) and np.array_equal(guv, euv.reshape(guv.shape)), (big, "nv12")


@pytest.mark.parametrize("big", [False, True])
def test_distorted_lens(vs, cuda, frames, big):
    import torch
    w, h = 640, 360
    f = frames[(w, h)]
    K, Ko, dw, dh = camera(w, h, big)
    launch = layouts.fused_launch(dw, dh)
    fd = torch.from_numpy(f).to(cuda)
    for rv in (TOP, BOTTOM):
        p = oracle.map_params(K, Ko, oracle.rodrigues(rv))
        for th, c in cases(*dd.maps(p, dw, dh, 1, dd.D_A), w, h, launch).items():
            assert c["mixed"] >= 5 and c["outside"] >= 1, (big, rv, th, c)
        got = vs.warp_nv12_dist(fd, p, dd.D_A, dw, dh, 1, vs.OUT_BGR8).cpu().numpy()
        exp = dd.warp_bgr(f, p, dw, dh, 1, dd.D_A)
        assert np.array_equal(got, exp), (big, rv, int((got != exp).any(axis=2).sum()))


@pytest.mark.parametrize("blend", [0, 1])
@pytest.mark.parametrize("big", [False, True])
def test_10_bit_both_blends_both_outputs(vs, cuda, blend, big):
    """DEPTH 10: 64 x 32 tiles always; the stateless output adds the half-height tail.  The fp16 blend stages 8-byte pixels."""
    w, h = 640, 360
    K, Ko, dw, dh = camera(w, h, big)
    launch = layouts.fused10_launch(dw, dh)
    assert launch[2] == (0.5 if big else 0.0)
    y, uv, _, _ = p010_frame(33, w, h)
    src = layouts.place(y, uv, "packed", cuda)
    for rv, mode in ((TOP, 0),) if big else ((TOP, 0), (BOTTOM, 5)):
        p = oracle.map_params(K, Ko, oracle.rodrigues(rv))
        c = cases(*oracle.create_map(p, dw, dh), w, h, launch, p, dw, dh, px=2 if blend else 1)
        for th in (32, 16) if big else (32,):
            assert c[th]["mixed"] >= 5 and c[th]["outside"] >= 1 and c[th]["missed"] >= 1, (blend, big, th, c[th])
        exp = oracle.warp_p010_ref_gfx950(y, uv, p, dw, dh, None, blend) if mode == 5 else oracle.warp_p010(y, uv, p, dw, dh, None, 0, blend)
        got = layouts.warp_p010(vs, src, p, dw, dh, mode, blend, cuda)
        assert np.array_equal(got, exp), (blend, big, mode, "bgr16", int((got != exp).any(axis=2).sum()))
        ey, euv = oracle.cvt_bgr10_p010(exp)
        gy, guv = layouts.warp_p010_planes(vs, src, p, dw, dh, mode, blend, cuda)
        assert np.array_equal(gy, ey) and np.array_equal(guv, euv.reshape(guv.shape)), (blend, big, mode, "p010")


def test_pipeline_pull_1080p(vs, cuda):
    """Sixteen frames at 1080p through pull_into, every emitted frame against the oracle's warp of its input under the rotation the
    pipeline chose for it (the clip: one rendered frame rolled by a random walk of even pixel offsets)."""
    import torch
    w, h, n = 1920, 1080, 17
    K, Ko, cw, ch = camera(w, h)
    launch = layouts.fused_launch(cw, ch)
    base = synth.shaky_clip(23, K, w, h, 1)[0][0]
    rng = np.random.default_rng(9)
    pos = np.cumsum(2 * rng.integers(-4, 5, (n, 2)), axis=0)
    frames = []
    for dx, dy in pos:
        f = np.empty_like(base)
        f[:h] = np.roll(base[:h], (int(dy), int(dx)), axis=(0, 1))
        f[h:] = np.roll(base[h:], (int(dy) // 2, int(dx)), axis=(0, 1))
        frames.append(f)
    stab = vs.Stabilizer([torch.from_numpy(f).to(cuda) for f in frames], total=n, smooth_radius=2, seed=4)
    out = torch.empty((ch, cw, 3), dtype=torch.uint8, device=cuda)
    for i in range(n - 1):
        assert stab.pull_into(out)
        p = oracle.map_params(K, Ko, stab.warp_rotation(i))
        if i == 0:
            for th, c in cases(*oracle.create_map(p, cw, ch), w, h, launch, p, cw, ch).items():
                assert c["mixed"] >= 20 and c["outside"] >= 5, (th, c)
        exp = oracle.warp_nv12_ref_gfx950(frames[i + 1], p, cw, ch)
        assert np.array_equal(out.cpu().numpy(), exp), i
    assert not stab.pull_into(out)
