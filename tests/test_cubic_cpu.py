"""The bicubic resampler's definition (tests/warp_def.py) and its ABI, without a GPU: the integer weight table's properties, the table the
library's kernels embed, the numpy remap's behaviour, the committed known answers, and vstab_create's refusals of bad `resample` values."""
import ctypes
import os

import numpy as np
import pytest

import warp_def as wd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KAT = os.path.join(ROOT, "tests", "golden", "cubic_kat.npz")


@pytest.fixture(scope="module")
def tab():
    return wd.cubic_table()


def test_every_entry_sums_to_one(tab):
    assert tab.shape == (1024, 4, 4)
    assert (tab.sum(axis=(1, 2)) == 32768).all()


def test_integer_position_entry(tab):
    """fx = fy = 0: the centre weight saturates to 32767 and the correction gives the missing 1 to tap (+1, +1)."""
    e = np.zeros((4, 4), np.int32)
    e[1, 1], e[2, 2] = 32767, 1
    assert np.array_equal(tab[0], e)


def test_entries_mirror_within_one(tab):
    """The rounded products for fx mirror those for 32 - fx about the centre (columns 0..3 -> 3..0) within 1 per weight -- c3 is a
    remainder, so exact symmetry is not promised -- and likewise for fy.  The sum correction then moves at most one weight of an entry, inside
    the window (rows and columns 2, 3), by the entry's rounding excess: it is not mirrored, so corrected entries can differ by a few more."""
    c = wd.cubic_coeffs()
    raw = np.clip(np.rint(((c[:, None, :, None] * c[None, :, None, :]).astype(np.float32) * np.float32(32768)).astype(np.float32)), -32768, 32767)
    raw = raw.astype(np.int64)                      # [fy, fx, k1, k2] before the correction
    for f in range(1, 32):
        for g in range(32):
            assert np.abs(raw[g, f] - raw[g, 32 - f][:, ::-1]).max() <= 1, (g, f)
            assert np.abs(raw[f, g] - raw[32 - f, g][::-1, :]).max() <= 1, (f, g)
    moved = tab.reshape(32, 32, 4, 4) != raw
    assert moved.sum(axis=(2, 3)).max() == 1
    assert not moved[:, :, :2, :].any() and not moved[:, :, :, :2].any()


def test_table_matches_golden_and_library(tab, vs):
    kat = np.load(KAT)
    assert np.array_equal(tab, kat["table"].astype(np.int32))
    assert np.array_equal(vs.cubic_weights().astype(np.int32), tab)   # the table compiled into the kernels' code object


def test_golden_remaps():
    n = 0
    for k, src, mx, my, border, out in wd.golden_cases("cubic_kat", "src", "mapx", "mapy", "border", "out"):
        assert np.array_equal(wd.remap(src, mx, my, "cubic", wd.CONSTANT, border), out), k
        n += 1
    assert n >= 6


def test_integer_translation_copies(tab):
    rng = np.random.default_rng(1)
    src = rng.integers(0, 256, (40, 50, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:30, 0:40].astype(np.float32)
    out = wd.remap(src, xx + 5, yy + 3, "cubic")
    assert np.array_equal(out, src[3:33, 5:45])


def test_fractional_positions_within_a_level_of_float_bicubic():
    rng = np.random.default_rng(2)
    src = rng.integers(0, 256, (30, 30), dtype=np.uint8)
    mx = rng.uniform(2, 26, (40, 40)).astype(np.float32)
    my = rng.uniform(2, 26, (40, 40)).astype(np.float32)
    got = wd.remap(src, mx, my, "cubic").astype(np.int64)
    ref = wd.remap_float(src, mx, my, "cubic")
    assert np.abs(got - ref).max() <= 1
    # cubic overshoots: a step edge saturates instead of wrapping
    step = np.zeros((8, 8), np.uint8)
    step[:, 4:] = 255
    yy, xx = np.mgrid[0:8, 0:64].astype(np.float32)
    out = wd.remap(step, xx / 8.0, yy * 0 + 4, "cubic")
    assert out.min() == 0 and out.max() == 255


def test_border_rule_per_tap():
    """A tap outside the source enters the blend as the border value; a footprint wholly outside gives the border value."""
    src = np.full((6, 6), 100, np.uint8)
    # footprint X - 1 .. X + 2 at X = -1: two columns outside (border 20), two inside (100); fx = fy = 0 -> the centre tap (column -1) alone
    assert wd.remap(src, np.array([[-1.0]], np.float32), np.array([[2.0]], np.float32), "cubic", wd.CONSTANT, 20)[0, 0] == 20
    assert wd.remap(src, np.array([[0.0]], np.float32), np.array([[2.0]], np.float32), "cubic", wd.CONSTANT, 20)[0, 0] == 100
    # half a pixel left of the source: the blend of border and source per the table's weights
    w = wd.cubic_table()[16].sum(axis=0)   # fx = 16, fy = 0: column weights
    exp = (int(w[0] * 20 + w[1] * 20 + w[2] * 100 + w[3] * 100) + (1 << 14)) >> 15
    assert wd.remap(src, np.array([[-0.5]], np.float32), np.array([[2.0]], np.float32), "cubic", wd.CONSTANT, 20)[0, 0] == exp
    for far in (-3.0, 8.0, 40.0):
        assert wd.remap(src, np.array([[far]], np.float32), np.array([[2.0]], np.float32), "cubic", wd.CONSTANT, 20)[0, 0] == 20


def test_nan_and_huge_entries_give_the_border():
    src = np.full((5, 5, 2), 9, np.uint8)
    vals = np.array([[np.nan, np.inf, -np.inf, 1e9, -1e9, 3e9, -3e9]], np.float32)
    out = wd.remap(src, vals, np.full_like(vals, 2.0), "cubic", wd.CONSTANT, (128, 77))
    assert (out[..., 0] == 128).all() and (out[..., 1] == 77).all()
    out = wd.remap(src, np.full_like(vals, 2.0), vals, "cubic", wd.CONSTANT, (128, 77))
    assert (out[..., 0] == 128).all() and (out[..., 1] == 77).all()


def test_cubic_matches_opencv_when_present():
    """The restatement against OpenCV itself -- the check that confirms (or corrects) the correction window of the table."""
    cv2 = pytest.importorskip("cv2")
    rng = np.random.default_rng(3)
    for cn, border in ((1, 16), (2, (128, 128)), (3, (0, 0, 0))):
        src = rng.integers(0, 256, (37, 53, cn) if cn > 1 else (37, 53), dtype=np.uint8)
        mx = rng.uniform(-4, 57, (41, 43)).astype(np.float32)
        my = rng.uniform(-4, 41, (41, 43)).astype(np.float32)
        mx[::7, ::5] = np.floor(mx[::7, ::5] * 32 + 0.5) / 32 + 1.0 / 64   # ties
        bv = (border,) * 4 if np.isscalar(border) else tuple(border) + (0,) * (4 - len(border))
        exp = cv2.remap(src, mx, my, cv2.INTER_CUBIC, borderMode=cv2.BORDER_CONSTANT, borderValue=bv)
        assert np.array_equal(wd.remap(src, mx, my, "cubic", wd.CONSTANT, border), exp), cn


# ---------------------------------------------------------------------------------------------
# ABI
# ---------------------------------------------------------------------------------------------
def test_abi_version_6_and_config_mirror(vs):
    assert vs.lib.vstab_abi_version() == 0x56534206 == vs.ABI_VERSION
    assert vs.lib.vstab_struct_size(2) == ctypes.sizeof(vs.Config)
    cfg = vs.default_config()
    assert cfg.resample == vs.RESAMPLE_DEFAULT == 0 and vs.RESAMPLE_CUBIC == 2
    text = open(os.path.join(ROOT, "include", "vstab.h")).read()
    assert "int resample;" in text and "VSTAB_RESAMPLE_CUBIC = 2" in text


def test_create_refuses_bad_resample_before_device_work(vs):
    calls = []
    cb = vs.PULL_FN(lambda user, out: calls.append(1) or vs.EOF)
    src = vs.Source(cb, cb, None)
    h = ctypes.c_void_p()
    for bad in (vs.default_config(resample=7), vs.default_config(resample=1), vs.default_config(resample=-1),
                vs.default_config(resample=vs.RESAMPLE_CUBIC, interpolation=0), vs.default_config(resample=vs.RESAMPLE_CUBIC, pixel_depth=10)):
        assert vs.lib.vstab_create(ctypes.byref(bad), ctypes.byref(src), ctypes.byref(h)) == vs.ERR_INVALID
        assert b"resample" in vs.lib.vstab_last_error() or b"RESAMPLE_CUBIC" in vs.lib.vstab_last_error()
        assert not h.value
    assert not calls   # refused before upstream was touched


def test_stateless_cubic_refuses_bad_arguments_without_a_device(vs):
    """Argument checks come before any launch: null pointers, channel counts, sizes, borders, output formats, map modes."""
    b = (ctypes.c_int * 3)(0, 0, 0)
    bad_border = (ctypes.c_int * 3)(0, 256, 0)
    P = 4096   # a non-null dummy address: never dereferenced, every call below is refused first
    L = vs.lib
    assert L.vstab_remap_cubic(None, 64, 8, 8, 1, P, 32, P, 32, b, P, 8, 8, 8, None) == vs.ERR_INVALID
    assert L.vstab_remap_cubic(P, 64, 8, 8, 4, P, 32, P, 32, b, P, 32, 8, 8, None) == vs.ERR_INVALID
    assert L.vstab_remap_cubic(P, 64, 8, 8, 0, P, 32, P, 32, b, P, 32, 8, 8, None) == vs.ERR_INVALID
    assert L.vstab_remap_cubic(P, 64, 0, 8, 1, P, 32, P, 32, b, P, 32, 8, 8, None) == vs.ERR_INVALID
    assert L.vstab_remap_cubic(P, 64, 8, 8, 2, P, 32, P, 32, bad_border, P, 32, 8, 8, None) == vs.ERR_INVALID
    assert b"border" in L.vstab_last_error()
    assert L.vstab_remap_cubic(P, 64, 8, 8, 1, P, 16, P, 32, b, P, 32, 8, 8, None) == vs.ERR_INVALID   # map pitch < 4 * width
    assert L.vstab_remap_cubic(P, 64, 8, 8, 1, P, 32, P, 32, None, P, 32, 8, 8, None) == vs.ERR_INVALID
    p = np.zeros(17, np.float32)
    fp = p.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    W = L.vstab_warp_nv12_cubic
    assert W(P, 64, P, 64, 64, 32, fp, 0, vs.OUT_NV12, P, 64, P, 64, 32, 16, None) == vs.ERR_INVALID
    assert b"VSTAB_OUT_BGR8 or VSTAB_OUT_NV12_PLANAR" in L.vstab_last_error()
    assert W(P, 64, P, 64, 64, 32, fp, 0, 7, P, 192, None, 0, 32, 16, None) == vs.ERR_INVALID
    assert W(P, 64, P, 64, 64, 32, fp, 6, vs.OUT_BGR8, P, 192, None, 0, 32, 16, None) == vs.ERR_INVALID
    assert W(P, 64, P, 64, 63, 32, fp, 0, vs.OUT_BGR8, P, 192, None, 0, 32, 16, None) == vs.ERR_INVALID   # odd source
    assert W(P, 64, P, 64, 64, 32, fp, 0, vs.OUT_BGR8, P, 64, None, 0, 32, 16, None) == vs.ERR_INVALID   # pitch < 3 * width
    assert W(P, 64, P, 64, 64, 32, fp, 0, vs.OUT_NV12_PLANAR, P, 64, None, 0, 32, 16, None) == vs.ERR_INVALID   # no chroma plane
    assert W(P, 64, P + 1, 64, 64, 32, fp, 0, vs.OUT_BGR8, P, 192, None, 0, 32, 16, None) == vs.ERR_INVALID   # odd chroma address
    assert W(None, 64, P, 64, 64, 32, fp, 0, vs.OUT_BGR8, P, 192, None, 0, 32, 16, None) == vs.ERR_INVALID
    assert W(P, 64, P, 64, 64, 32, fp, 0, vs.OUT_BGR8, P, 192, None, 0, 0, 16, None) == vs.ERR_INVALID
