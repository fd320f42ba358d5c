"""Border modes of the cubic and Lanczos resamplers without a GPU: the numpy statement (tests/warp_def.py) against a literal
per-pixel restatement of OpenCV's non-constant branch, its golden vectors and OpenCV itself where installed; the constant border against the
constant-border definitions; the closed-form borderInterpolate over every position a footprint reaches; the tile-box model of the kernels
(tests/warp_tiles.py, rule `every`); and the argument checks of the new entry points."""
import ctypes
import os

import numpy as np
import pytest

import warp_def as wd
import warp_tiles as wt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESAMPLERS = ("cubic", "lanczos4")


def golden_cases():
    for k, r, *rest in wd.golden_cases("resample_border_kat", "resampler", "src", "mapx", "mapy", "mode", "out"):
        yield (k, RESAMPLERS[r], *rest)


def opencv_literal(resampler, src, mapx, mapy, mode):
    """OpenCV's remapBicubic / remapLanczos4 for one pixel at a time, on the branch of a non-constant borderMode: every tap's column and row
    through borderInterpolate (OpenCV's loop), cval * ONE + sum((S - cval) * w) with cval = 0, then (+ 2^14) >> 15 saturated."""
    K, LO = wd.FOOTPRINT[resampler]
    tab = wd.table(resampler)
    s = np.asarray(src, np.uint8)
    flat = s.ndim == 2
    if flat:
        s = s[:, :, None]
    sh, sw, cn = s.shape
    X, Y, f = wd.quantise(mapx, mapy)
    out = np.zeros(X.shape + (cn,), np.uint8)
    for (i, j), _ in np.ndenumerate(X):
        xs = wd.border_interpolate_loop(np.arange(K) + X[i, j] - LO, sw, mode)
        ys = wd.border_interpolate_loop(np.arange(K) + Y[i, j] - LO, sh, mode)
        w = tab[f[i, j]]
        for c in range(cn):
            acc = 0
            for k1 in range(K):
                for k2 in range(K):
                    acc += int(s[ys[k1], xs[k2], c]) * int(w[k1, k2])
            out[i, j, c] = min(max((acc + (1 << 14)) >> 15, 0), 255)
    return out[:, :, 0] if flat else out


@pytest.mark.parametrize("resampler", RESAMPLERS)
def test_definition_equals_opencv_literal(resampler):
    rng = np.random.default_rng(11)
    for sw, sh, cn in ((1, 1, 1), (2, 3, 3), (3, 2, 2), (9, 7, 3)):
        src = rng.integers(0, 256, (sh, sw, cn) if cn > 1 else (sh, sw), dtype=np.uint8)
        mx = rng.uniform(-3 * sw - 4, 4 * sw + 4, (5, 7)).astype(np.float32)
        my = rng.uniform(-3 * sh - 4, 4 * sh + 4, (5, 7)).astype(np.float32)
        mx[0, :3], my[0, :3] = [np.nan, 1e30, -32768.0], [np.nan, -1e30, 32768.0]
        for mode in wd.MODES:
            assert np.array_equal(wd.remap(src, mx, my, resampler, mode), opencv_literal(resampler, src, mx, my, mode)), \
                (resampler, sw, sh, mode)


def test_tables_sum_to_one():
    """cval * ONE + sum((S - cval) * w) == sum(S * w) needs every entry to sum to 32768."""
    assert (wd.table("cubic").sum(axis=(1, 2)) == 32768).all()
    assert (wd.table("lanczos4").sum(axis=(1, 2)) == 32768).all()


def test_constant_equals_constant_definitions():
    """The constant border of the one remap against what the constant-border definitions of the cubic and Lanczos resamplers answered while
    they were layers of their own (tests/golden/warp_definitions_kat.npz, constant_c<cn>_*)."""
    kat = wd.golden("warp_definitions_kat")
    for cn in (1, 2, 3):
        src, mx, my, bd = (kat[f"constant_c{cn}_{k}"] for k in ("src", "mapx", "mapy", "border"))
        assert src.shape[:2] == (13, 17) and mx.shape == (11, 15) and len(bd) == cn
        for r in RESAMPLERS:
            assert np.array_equal(wd.remap(src, mx, my, r, wd.CONSTANT, bd), kat[f"constant_c{cn}_{r}"]), (cn, r)


def test_golden_remaps():
    seen = set()
    n = 0
    for k, resampler, src, mx, my, mode, out in golden_cases():
        assert np.array_equal(wd.remap(src, mx, my, resampler, mode), out), k
        cn = 1 if src.ndim == 2 else src.shape[2]
        seen |= {(resampler, mode, cn), (resampler, "w", src.shape[1]), (resampler, "h", src.shape[0])}
        n += 1
    assert n >= 54
    for r in RESAMPLERS:
        assert {(r, m, c) for m in wd.MODES for c in (1, 2, 3)} <= seen
        assert {(r, a, v) for a in ("w", "h") for v in (1, 2, 3)} <= seen


def test_golden_maps_hold_the_special_entries():
    specials = dict.fromkeys(("nan", "inf", "-inf", "1e30", "-1e30", "32768", "-32768", "tie", "far"), False)
    for _, _, src, mx, my, _, _ in golden_cases():
        sh, sw = src.shape[:2]
        for m, n in ((mx, sw), (my, sh)):
            specials["nan"] |= bool(np.isnan(m).any())
            specials["inf"] |= bool(np.isposinf(m).any())
            specials["-inf"] |= bool(np.isneginf(m).any())
            specials["1e30"] |= bool((m == np.float32(1e30)).any())
            specials["-1e30"] |= bool((m == np.float32(-1e30)).any())
            specials["32768"] |= bool((m == 32768.0).any())
            specials["-32768"] |= bool((m == -32768.0).any())
            with np.errstate(invalid="ignore"):
                fin = m[np.isfinite(m) & (np.abs(m) < 1e6)]
                specials["tie"] |= bool(((fin * 64) % 2 == 1).any())
                specials["far"] |= bool(((fin < -3 * n) | (fin > 4 * n)).any())
    assert all(specials.values()), specials


def test_resample_border_matches_opencv_when_present():
    """cv2.remap with INTER_CUBIC / INTER_LANCZOS4 and each border mode, where OpenCV is installed (skipped otherwise)."""
    cv2 = pytest.importorskip("cv2")
    interp = {"cubic": cv2.INTER_CUBIC, "lanczos4": cv2.INTER_LANCZOS4}
    for k, resampler, src, mx, my, mode, out in golden_cases():
        if not (np.isfinite(mx).all() and np.isfinite(my).all()):
            continue   # cv2's SIMD path may treat NaN / inf differently from its scalar one
        assert np.array_equal(cv2.remap(src, mx, my, interp[resampler], borderMode=mode), out), k


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 1919, 1920, 32767])
@pytest.mark.parametrize("mode", wd.MODES)
def test_closed_form_equals_opencv_loop_over_footprints(n, mode):
    """Footprints reach X - 3 .. X + 4 with X in [-32768, 32767]: the closed form equals OpenCV's loop over [-32772, 32772]."""
    p = np.arange(-32772, 32773, dtype=np.int64)
    loop = wd.border_interpolate_loop(p, n, mode)
    assert ((loop >= 0) & (loop < n)).all()
    assert np.array_equal(wd.border_interpolate(p, n, mode), loop)


TILE_KEYS = sorted((r, name) for r in RESAMPLERS for name in wt.TILE_SETS[r + "_border"])


@pytest.mark.parametrize("key", TILE_KEYS)
def test_tile_set_reaches_its_committed_states(key):
    got = wt.states_of(key[0] + "_border", key[1])
    for plane, want in wt.TILE_SETS[key[0] + "_border"][key[1]][-1].items():
        for state, least in want.items():
            assert got[plane][state] >= least, (key, plane, state, got[plane])


@pytest.mark.parametrize("resampler", RESAMPLERS)
def test_tile_sets_cover_every_path_of_every_plane(resampler):
    total = {p: dict.fromkeys(wt.BORDER_STATES, 0) for p in ("bgr", "luma", "chroma")}
    for name in wt.TILE_SETS[resampler + "_border"]:
        for plane, counts in wt.states_of(resampler + "_border", name).items():
            for k in wt.BORDER_STATES:
                total[plane][k] += counts[k]
    for plane, counts in total.items():
        for state in wt.BORDER_STATES:
            assert counts[state] > 0, (resampler, plane, state, counts)


def test_axis_pixel_gathers_its_tile():
    """Map mode 0's 0/0 axis pixel quantises to X = Y = -32768: its footprint reaches -32771 and the tile holding it is gathered."""
    mx = np.full((16, 64), 10.0, np.float32)
    my = np.full((16, 64), 10.0, np.float32)
    mx[5, 7] = my[5, 7] = np.nan
    for r, lo in (("cubic", 1), ("lanczos4", 3)):
        x0, y0, bw, bh, _ = wt.tile_boxes(mx, my, 64, 32, r, "every")["bgr"]
        assert x0[0, 0] == -32768 - lo and bw[0, 0] * bh[0, 0] > wt.BUDGET["bgr"]


def test_header_and_binding(vs):
    text = open(os.path.join(ROOT, "include", "vstab.h")).read()
    assert "#define VSTAB_ABI_VERSION 0x56534206" in text
    for name in ("vstab_remap_cubic_border", "vstab_remap_lanczos4_border", "vstab_warp_nv12_cubic_border", "vstab_warp_nv12_lanczos4_border",
                 "vstab_set_border_mode_ex"):
        assert name in text and name in vs.SIGNATURES and hasattr(vs.lib, name)
    for name in ("remap_cubic_border", "remap_lanczos4_border", "warp_nv12_cubic_border", "warp_nv12_lanczos4_border"):
        assert callable(getattr(vs, name))
    assert hasattr(vs.Stabilizer, "set_border_mode_ex")


@pytest.mark.parametrize("name", ["cubic", "lanczos4"])
def test_resample_border_entry_points_refuse_bad_arguments_without_a_device(vs, name):
    """Argument checks come before any launch: null pointers, channel counts, sizes, pitches, border modes (WRAP, TRANSPARENT and others),
    output formats, map modes, odd sources and misaligned chroma.  The setter refuses a NULL handle."""
    P = 4096   # a non-null dummy address: never dereferenced, every call below is refused first
    L = vs.lib
    R = getattr(L, f"vstab_remap_{name}_border")
    bd = (ctypes.c_int * 3)(0, 0, 0)
    for bad in (3, 5, -1, 16, 6):
        assert R(P, 64, 8, 8, 1, P, 32, P, 32, bad, bd, P, 8, 8, 8, None) == vs.ERR_INVALID
        assert b"border_mode" in L.vstab_last_error()
    assert R(None, 64, 8, 8, 1, P, 32, P, 32, 1, bd, P, 8, 8, 8, None) == vs.ERR_INVALID
    assert R(P, 64, 8, 8, 4, P, 32, P, 32, 1, bd, P, 32, 8, 8, None) == vs.ERR_INVALID
    assert R(P, 64, 8, 8, 0, P, 32, P, 32, 1, bd, P, 32, 8, 8, None) == vs.ERR_INVALID
    assert R(P, 64, 0, 8, 1, P, 32, P, 32, 1, bd, P, 32, 8, 8, None) == vs.ERR_INVALID
    assert R(P, 64, 32768, 8, 1, P, 32, P, 32, 1, bd, P, 32, 8, 8, None) == vs.ERR_INVALID
    assert R(P, 64, 8, 8, 1, P, 16, P, 32, 1, bd, P, 32, 8, 8, None) == vs.ERR_INVALID   # map pitch < 4 * width
    assert R(P, 64, 8, 8, 1, P + 2, 32, P, 32, 1, bd, P, 32, 8, 8, None) == vs.ERR_INVALID   # map plane not 4-byte aligned
    assert R(P, 64, 8, 8, 3, P, 32, P, 32, 1, bd, P, 16, 8, 8, None) == vs.ERR_INVALID   # dst pitch < 3 * width
    assert R(P, 64, 8, 8, 1, P, 32, P, 32, 0, None, P, 8, 8, 8, None) == vs.ERR_INVALID   # CONSTANT needs border[]
    assert R(P, 64, 8, 8, 1, P, 32, P, 32, 0, (ctypes.c_int * 3)(256, 0, 0), P, 8, 8, 8, None) == vs.ERR_INVALID
    p = np.zeros(17, np.float32)
    fp = p.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    W = getattr(L, f"vstab_warp_nv12_{name}_border")
    B = vs.BORDER_REFLECT_101
    assert W(P, 64, P, 64, 64, 32, fp, 0, vs.OUT_NV12, B, P, 64, P, 64, 32, 16, None) == vs.ERR_INVALID
    assert b"VSTAB_OUT_BGR8 or VSTAB_OUT_NV12_PLANAR" in L.vstab_last_error()
    assert W(P, 64, P, 64, 64, 32, fp, 0, 7, B, P, 192, None, 0, 32, 16, None) == vs.ERR_INVALID
    for bad in (3, 5, -1, 8):
        assert W(P, 64, P, 64, 64, 32, fp, 0, vs.OUT_BGR8, bad, P, 192, None, 0, 32, 16, None) == vs.ERR_INVALID
        assert b"border_mode" in L.vstab_last_error()
    assert W(P, 64, P, 64, 64, 32, fp, 6, vs.OUT_BGR8, B, P, 192, None, 0, 32, 16, None) == vs.ERR_INVALID
    assert W(P, 64, P, 64, 64, 32, fp, -1, vs.OUT_BGR8, B, P, 192, None, 0, 32, 16, None) == vs.ERR_INVALID
    assert W(P, 64, P, 64, 63, 32, fp, 0, vs.OUT_BGR8, B, P, 192, None, 0, 32, 16, None) == vs.ERR_INVALID   # odd source
    assert W(P, 64, P, 64, 64, 31, fp, 0, vs.OUT_BGR8, B, P, 192, None, 0, 32, 16, None) == vs.ERR_INVALID
    assert W(P, 65536, P, 65536, 32768, 32, fp, 0, vs.OUT_BGR8, B, P, 192, None, 0, 32, 16, None) == vs.ERR_INVALID   # > 32767
    assert W(P, 64, P, 64, 64, 32, fp, 0, vs.OUT_BGR8, B, P, 64, None, 0, 32, 16, None) == vs.ERR_INVALID   # pitch < 3 * width
    assert W(P, 64, P, 64, 64, 32, fp, 0, vs.OUT_NV12_PLANAR, B, P, 64, None, 0, 32, 16, None) == vs.ERR_INVALID   # no chroma plane
    assert W(P, 64, P + 1, 64, 64, 32, fp, 0, vs.OUT_BGR8, B, P, 192, None, 0, 32, 16, None) == vs.ERR_INVALID   # odd chroma address
    assert W(P, 64, P, 63, 64, 32, fp, 0, vs.OUT_BGR8, B, P, 192, None, 0, 32, 16, None) == vs.ERR_INVALID   # pitch < width
    assert W(None, 64, P, 64, 64, 32, fp, 0, vs.OUT_BGR8, B, P, 192, None, 0, 32, 16, None) == vs.ERR_INVALID
    assert W(P, 64, P, 64, 64, 32, None, 0, vs.OUT_BGR8, B, P, 192, None, 0, 32, 16, None) == vs.ERR_INVALID
    assert W(P, 64, P, 64, 64, 32, fp, 0, vs.OUT_BGR8, B, P, 192, None, 0, 0, 16, None) == vs.ERR_INVALID
    assert L.vstab_set_border_mode_ex(None, B) == vs.ERR_INVALID
    assert L.vstab_set_border_mode_ex(None, 0) == vs.ERR_INVALID
