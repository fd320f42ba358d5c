"""The Lanczos resampler's definition (tests/warp_def.py) and its ABI, without a GPU: the integer weight table's properties and its
independence of the libm, the table the library's kernels embed, the numpy remap's behaviour, the committed known answers, vstab_create's
handling of `resample = 4`, and the stateless functions' argument checks."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import warp_def as wd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KAT = os.path.join(ROOT, "tests", "golden", "lanczos4_kat.npz")
HEADER = os.path.join(ROOT, "video-annotator_amd", "csrc", "vstab_lanczos4.hpp")


@pytest.fixture(scope="module")
def tab():
    return wd.lanczos4_table()


def header_literals(name):
    text = open(HEADER).read()
    body = re.search(r"LANCZOS4_%s\[32\] = \{(.*?)\};" % name, text, re.S).group(1)
    return [float.fromhex(v.strip()) for v in body.split(",")]


def test_every_entry_sums_to_one(tab):
    assert tab.shape == (1024, 8, 8)
    assert (tab.sum(axis=(1, 2)) == 32768).all()


def test_entry_zero_is_not_the_identity(tab):
    """fx = fy = 0: the centre weight saturates to 32767 at tap (3, 3), outside the correction window, which gives the missing 1 to
    tap (4, 4)."""
    e = np.zeros((8, 8), np.int32)
    e[3, 3], e[4, 4] = 32767, 1
    assert np.array_equal(tab[0], e)


def test_both_forms_of_the_x0_special_case_give_the_same_table(tab):
    """OpenCV has returned the unit row early at x = 0, and has put a 1e30f sentinel in tap 3 and normalised: the float rows differ (the
    sentinel leaves ~1e-30 in the other taps), the integer table does not."""
    early, sentinel = wd.lanczos4_coeffs(variant="early"), wd.lanczos4_coeffs(variant="sentinel")
    assert np.array_equal(early[1:], sentinel[1:])
    assert not np.array_equal(early[0], sentinel[0]) and sentinel[0, 3] == 1.0
    assert np.array_equal(wd.lanczos4_table(variant="sentinel"), tab)


def test_correction_stays_in_its_window(tab):
    """The correction moves at most one weight of an entry, inside rows and columns 4, 5."""
    _, prod = wd.lanczos4_table(products=True)
    raw = np.clip(np.rint(prod).astype(np.int64), -32768, 32767)
    moved = tab != raw
    assert moved.sum(axis=(1, 2)).max() == 1
    assert not moved[:, :4, :].any() and not moved[:, 6:, :].any() and not moved[:, :, :4].any() and not moved[:, :, 6:].any()
    assert moved.any()


def test_table_does_not_depend_on_the_libm(tab):
    """Every s0 / c0 moved by one double ulp, up or down, all at once and in random mixtures: no entry changes.  (The table does depend
    on fp32 operation order and on cvRound's ties: a few products are exact ties, ~120 lie within 1e-3 of one.)"""
    s0, c0 = wd.sincos()
    for d in (np.inf, -np.inf):
        assert np.array_equal(wd.lanczos4_table([np.nextafter(v, d) for v in s0], [np.nextafter(v, d) for v in c0]), tab)
        assert np.array_equal(wd.lanczos4_table([np.nextafter(v, d) for v in s0], [np.nextafter(v, -d) for v in c0]), tab)
    rng = np.random.default_rng(7)
    for _ in range(4):
        ds, dc = rng.choice([np.inf, -np.inf, 0.0], 32), rng.choice([np.inf, -np.inf, 0.0], 32)
        ps = [np.nextafter(v, d) if d else v for v, d in zip(s0, ds)]
        pc = [np.nextafter(v, d) if d else v for v, d in zip(c0, dc)]
        assert np.array_equal(wd.lanczos4_table(ps, pc), tab)
    _, prod = wd.lanczos4_table(products=True)
    frac = np.abs(prod - np.floor(prod) - 0.5)
    assert (frac == 0).sum() == 4 and (frac < 1e-3).sum() == 120


def test_committed_literals(tab):
    """The header's sin / cos literals are the KAT's, within one ulp of this host's libm, and the table built from them is the KAT's."""
    kat = np.load(KAT)
    s0, c0 = header_literals("S0"), header_literals("C0")
    assert np.array_equal(np.array(s0), kat["s0"]) and np.array_equal(np.array(c0), kat["c0"])
    here_s, here_c = wd.sincos()
    for a, b in zip(s0 + c0, here_s + here_c):
        assert abs(a - b) <= math.ulp(b)
    assert np.array_equal(wd.lanczos4_table(s0, c0), tab)


def test_table_matches_golden_and_library(tab, vs):
    kat = np.load(KAT)
    assert np.array_equal(tab, kat["table"].astype(np.int32))
    assert np.array_equal(vs.lanczos4_weights().astype(np.int32), tab)   # the table compiled into the kernels' code object


def test_golden_remaps():
    n = 0
    for k, src, mx, my, border, out in wd.golden_cases("lanczos4_kat", "src", "mapx", "mapy", "border", "out"):
        assert np.array_equal(wd.remap(src, mx, my, "lanczos4", wd.CONSTANT, border), out), k
        n += 1
    assert n >= 6


def test_integer_translation_copies():
    rng = np.random.default_rng(1)
    src = rng.integers(0, 256, (40, 50, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:30, 0:40].astype(np.float32)
    out = wd.remap(src, xx + 5, yy + 3, "lanczos4")
    assert np.array_equal(out, src[3:33, 5:45])


def test_fractional_positions_within_a_level_of_float_lanczos():
    rng = np.random.default_rng(2)
    src = rng.integers(0, 256, (30, 30), dtype=np.uint8)
    mx = rng.uniform(4, 24, (40, 40)).astype(np.float32)
    my = rng.uniform(4, 24, (40, 40)).astype(np.float32)
    got = wd.remap(src, mx, my, "lanczos4").astype(np.int64)
    ref = wd.remap_float(src, mx, my, "lanczos4")
    assert np.abs(got - ref).max() <= 1
    # Lanczos overshoots: a step edge saturates instead of wrapping
    step = np.zeros((12, 12), np.uint8)
    step[:, 6:] = 255
    yy, xx = np.mgrid[0:12, 0:96].astype(np.float32)
    out = wd.remap(step, xx / 8.0, yy * 0 + 6, "lanczos4")
    assert out.min() == 0 and out.max() == 255


def test_border_rule_per_tap():
    """A tap outside the source enters the blend as the border value; a footprint wholly outside gives the border value."""
    src = np.full((10, 10), 100, np.uint8)
    one = lambda x, y, b: wd.remap(src, np.array([[x]], np.float32), np.array([[y]], np.float32), "lanczos4", wd.CONSTANT, b)[0, 0]
    # fx = fy = 0: tap (X, Y) alone (32767) plus tap (X + 1, Y + 1) (1)
    assert one(-1.0, 4.0, 20) == 20 and one(0.0, 4.0, 20) == 100
    # half a pixel left of the source: the blend of border and source per the table's weights
    w = wd.lanczos4_table()[16].sum(axis=0)   # fx = 16, fy = 0: column weights
    exp = (int(sum(w[k] * (20 if k < 4 else 100) for k in range(8))) + (1 << 14)) >> 15   # X = -1: columns -4 .. 3
    assert one(-0.5, 4.0, 20) == exp
    for far in (-5.0, 14.0, 40.0):
        assert one(far, 4.0, 20) == 20
    # X = -4: tap columns -7 .. 0, one inside, weight 0 at fx = 0 -- the footprint touches, the border wins
    assert one(-4.0, 4.0, 20) == 20


def test_nan_and_huge_entries_give_the_border():
    src = np.full((9, 9, 2), 9, np.uint8)
    vals = np.array([[np.nan, np.inf, -np.inf, 1e9, -1e9, 3e9, -3e9]], np.float32)
    out = wd.remap(src, vals, np.full_like(vals, 4.0), "lanczos4", wd.CONSTANT, (128, 77))
    assert (out[..., 0] == 128).all() and (out[..., 1] == 77).all()
    out = wd.remap(src, np.full_like(vals, 4.0), vals, "lanczos4", wd.CONSTANT, (128, 77))
    assert (out[..., 0] == 128).all() and (out[..., 1] == 77).all()


def test_lanczos4_matches_opencv_when_present():
    """The restatement against OpenCV itself -- the check that confirms (or corrects) the correction window and the x = 0 rule."""
    cv2 = pytest.importorskip("cv2")
    rng = np.random.default_rng(3)
    for cn, border in ((1, 16), (2, (128, 128)), (3, (0, 0, 0))):
        src = rng.integers(0, 256, (37, 53, cn) if cn > 1 else (37, 53), dtype=np.uint8)
        mx = rng.uniform(-6, 59, (41, 43)).astype(np.float32)
        my = rng.uniform(-6, 43, (41, 43)).astype(np.float32)
        mx[::7, ::5] = np.floor(mx[::7, ::5] * 32 + 0.5) / 32 + 1.0 / 64   # ties
        my[::3, ::4] = np.floor(my[::3, ::4])                              # fy = 0
        bv = (border,) * 4 if np.isscalar(border) else tuple(border) + (0,) * (4 - len(border))
        exp = cv2.remap(src, mx, my, cv2.INTER_LANCZOS4, borderMode=cv2.BORDER_CONSTANT, borderValue=bv)
        assert np.array_equal(wd.remap(src, mx, my, "lanczos4", wd.CONSTANT, border), exp), cn


# ---------------------------------------------------------------------------------------------
# ABI
# ---------------------------------------------------------------------------------------------
def test_abi_keeps_version_6_and_names_lanczos4(vs):
    assert vs.lib.vstab_abi_version() == 0x56534206 == vs.ABI_VERSION   # no struct changed
    assert vs.RESAMPLE_LANCZOS4 == 4
    text = open(os.path.join(ROOT, "include", "vstab.h")).read()
    assert "VSTAB_RESAMPLE_LANCZOS4 = 4" in text and "vstab_lanczos4_weights(int16_t out[65536])" in text
    adapter = open(os.path.join(ROOT, "include", "vstab_frame_source.hpp")).read()
    assert "if (interpolation == 4) cfg.interpolation = 1, cfg.resample = VSTAB_RESAMPLE_LANCZOS4;" in adapter


def _create(vs, cfg):
    calls = []
    cb = vs.PULL_FN(lambda user, out: calls.append(1) or vs.EOF)
    src = vs.Source(cb, cb, None)
    h = ctypes.c_void_p()
    rc = vs.lib.vstab_create(ctypes.byref(cfg), ctypes.byref(src), ctypes.byref(h))
    return rc, vs.lib.vstab_last_error(), calls, h


def test_create_refuses_bad_lanczos4_configs_before_device_work(vs):
    for bad in (vs.default_config(resample=vs.RESAMPLE_LANCZOS4, interpolation=0), vs.default_config(resample=vs.RESAMPLE_LANCZOS4, pixel_depth=10),
                vs.default_config(resample=5), vs.default_config(resample=3)):
        rc, err, calls, h = _create(vs, bad)
        assert rc == vs.ERR_INVALID and (b"resample" in err or b"RESAMPLE_LANCZOS4" in err), err
        assert not h.value and not calls   # refused before upstream was touched
    rc, err, calls, h = _create(vs, vs.default_config(interpolation=4))   # INTER_LANCZOS4 goes through `resample`, not `interpolation`
    assert rc == vs.ERR_INVALID and b"interpolation" in err and not calls and not h.value


def test_create_accepts_lanczos4(vs):
    """resample = 4 with INTER_LINEAR and 8-bit pixels passes every argument check: create goes on to the device (no GPU: a device
    error) or to upstream (a GPU: this empty source's EOF)."""
    for cfg in (vs.default_config(resample=vs.RESAMPLE_LANCZOS4), vs.default_config(resample=vs.RESAMPLE_LANCZOS4, pixel_depth=8, lens_mode=1),
                vs.default_config(resample=vs.RESAMPLE_LANCZOS4, tracking=0, map_precision=0)):
        rc, err, calls, h = _create(vs, cfg)
        assert rc in (vs.EOF, vs.ERR_DEVICE), (rc, err)
        assert b"resample" not in err and b"RESAMPLE" not in err and not h.value


def test_stateless_lanczos4_refuses_bad_arguments_without_a_device(vs):
    """Argument checks come before any launch: null pointers, channel counts, sizes, borders, output formats, map modes."""
    b = (ctypes.c_int * 3)(0, 0, 0)
    bad_border = (ctypes.c_int * 3)(0, 256, 0)
    P = 4096   # a non-null dummy address: never dereferenced, every call below is refused first
    L = vs.lib
    R = L.vstab_remap_lanczos4
    assert R(None, 64, 8, 8, 1, P, 32, P, 32, b, P, 8, 8, 8, None) == vs.ERR_INVALID
    assert R(P, 64, 8, 8, 4, P, 32, P, 32, b, P, 32, 8, 8, None) == vs.ERR_INVALID
    assert R(P, 64, 8, 8, 0, P, 32, P, 32, b, P, 32, 8, 8, None) == vs.ERR_INVALID
    assert R(P, 64, 0, 8, 1, P, 32, P, 32, b, P, 32, 8, 8, None) == vs.ERR_INVALID
    assert R(P, 1 << 16, 32768, 8, 1, P, 32, P, 32, b, P, 32, 8, 8, None) == vs.ERR_INVALID     # 32768 wide
    assert R(P, 64, 8, 8, 1, P, 1 << 18, P, 1 << 18, b, P, 1 << 16, 32768, 8, None) == vs.ERR_INVALID
    assert b"32767" in L.vstab_last_error()
    assert R(P, 64, 8, 8, 2, P, 32, P, 32, bad_border, P, 32, 8, 8, None) == vs.ERR_INVALID
    assert b"border" in L.vstab_last_error()
    assert R(P, 64, 8, 8, 1, P, 16, P, 32, b, P, 32, 8, 8, None) == vs.ERR_INVALID   # map pitch < 4 * width
    assert R(P + 2, 64, 8, 8, 1, P + 2, 32, P, 32, b, P, 32, 8, 8, None) == vs.ERR_INVALID   # map plane not 4-byte aligned
    assert R(P, 64, 8, 8, 1, P, 32, P, 32, None, P, 32, 8, 8, None) == vs.ERR_INVALID
    assert b"vstab_remap_lanczos4" in L.vstab_last_error()
    p = np.zeros(17, np.float32)
    fp = p.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    W = L.vstab_warp_nv12_lanczos4
    assert W(P, 64, P, 64, 64, 32, fp, 0, vs.OUT_NV12, P, 64, P, 64, 32, 16, None) == vs.ERR_INVALID
    assert b"VSTAB_OUT_BGR8 or VSTAB_OUT_NV12_PLANAR" in L.vstab_last_error()
    assert W(P, 64, P, 64, 64, 32, fp, 0, 7, P, 192, None, 0, 32, 16, None) == vs.ERR_INVALID
    assert W(P, 64, P, 64, 64, 32, fp, 6, vs.OUT_BGR8, P, 192, None, 0, 32, 16, None) == vs.ERR_INVALID
    assert W(P, 64, P, 64, 64, 32, fp, -1, vs.OUT_BGR8, P, 192, None, 0, 32, 16, None) == vs.ERR_INVALID
    assert W(P, 64, P, 64, 63, 32, fp, 0, vs.OUT_BGR8, P, 192, None, 0, 32, 16, None) == vs.ERR_INVALID   # odd source
    assert W(P, 1 << 16, P, 1 << 16, 32768, 32, fp, 0, vs.OUT_BGR8, P, 192, None, 0, 32, 16, None) == vs.ERR_INVALID   # source 32768 wide
    assert W(P, 64, P, 64, 64, 32, fp, 0, vs.OUT_BGR8, P, 1 << 17, None, 0, 32768, 16, None) == vs.ERR_INVALID   # output 32768 wide
    assert W(P, 64, P, 64, 64, 32, fp, 0, vs.OUT_BGR8, P, 64, None, 0, 32, 16, None) == vs.ERR_INVALID   # pitch < 3 * width
    assert W(P, 64, P, 64, 64, 32, fp, 0, vs.OUT_NV12_PLANAR, P, 64, None, 0, 32, 16, None) == vs.ERR_INVALID   # no chroma plane
    assert W(P, 64, P, 64, 64, 32, fp, 0, vs.OUT_NV12_PLANAR, P, 64, P, 30, 31, 16, None) == vs.ERR_INVALID   # chroma pitch < 2 ceil(31 / 2)
    assert W(P, 64, P + 1, 64, 64, 32, fp, 0, vs.OUT_BGR8, P, 192, None, 0, 32, 16, None) == vs.ERR_INVALID   # odd chroma address
    assert W(None, 64, P, 64, 64, 32, fp, 0, vs.OUT_BGR8, P, 192, None, 0, 32, 16, None) == vs.ERR_INVALID
    assert W(P, 64, P, 64, 64, 32, fp, 0, vs.OUT_BGR8, P, 192, None, 0, 0, 16, None) == vs.ERR_INVALID
    assert b"vstab_warp_nv12_lanczos4" in L.vstab_last_error()
    assert L.vstab_lanczos4_weights(None) == vs.ERR_INVALID
