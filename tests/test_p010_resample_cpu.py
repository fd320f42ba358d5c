"""CPU tests of the plane-wise 10-bit warp with the cubic and Lanczos resamplers (include/vstab.h, "Cubic and Lanczos resampling at 10
bits"): the numpy definition (tests/warp10_def.py) against the 8-bit one, its identity, accumulator bound and float cross-check, the
known-answer file, the refusal tables of vstab_warp_p010_planar_ex and vstab_set_resample10 (no device: every row is refused before a
launch, a handle that is "not null" is a dummy address a refused call never reads), and the tile states the GPU tests
(tests/test_p010_resample_gpu.py) rely on, from warp_tiles' model with the 10-bit budgets."""
import ctypes

import numpy as np
import pytest

import warp10_def as w10
import warp_def as wd
import warp_tiles as wt

RESAMPLERS = w10.RESAMPLERS
P = 4096  # a non-null dummy address


def zoomed_out(mode=1, rot=True):
    sw, sh, dw, dh, fi, fo = wd.ZOOMED_OUT
    p, rb = wd.case_params(sw, sh, dw, dh, fi, fo)
    return sw, sh, wd.maps(p, dw, dh, mode, rb if rot else None)


# ---------------------------------------------------------------------------------------------------------------------
# 1 - 5: the definition
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("border_mode", wd.ALL_BORDERS)
@pytest.mark.parametrize("resampler", RESAMPLERS)
def test_samples_of_eight_bits_give_the_8_bit_definition(resampler, border_mode):
    """Sources with samples <= 255 and border values <= 255: the 10-bit blend clamped at 255 is cv::remap's 8-bit one, one and three channels."""
    sw, sh, (mx, my) = zoomed_out()
    rng = np.random.default_rng(11)
    for cn, border in ((1, 16), (2, (128, 77)), (3, (0, 255, 31))):
        src = rng.integers(0, 256, (sh, sw, cn), dtype=np.uint8)
        src[::7, ::5] = 255
        src[3::7, 2::5] = 0
        s = src[:, :, 0] if cn == 1 else src
        got = np.minimum(w10.remap10(s, mx, my, resampler, border_mode, border), 255)
        assert np.array_equal(got, wd.remap(s, mx, my, resampler, border_mode, border)), (cn, border)


@pytest.mark.parametrize("resampler", RESAMPLERS)
def test_identity_map_returns_the_source(resampler):
    rng = np.random.default_rng(12)
    src = rng.integers(0, 1024, (20, 33)).astype(np.uint16)
    yy, xx = np.mgrid[0:20, 0:33].astype(np.float32)
    for border_mode in wd.ALL_BORDERS:
        assert np.array_equal(w10.remap10(src, xx, yy, resampler, border_mode, 64), src), border_mode
    y16 = (src << 6) | rng.integers(0, 64, src.shape).astype(np.uint16)                     # junk below the ten bits
    uv16 = (rng.integers(0, 1024, (10, 34)).astype(np.uint16) << 6) | 63
    oy, ouv = w10.planar10(y16, uv16[:, :32], xx[:, :32], yy[:, :32], resampler, wd.REFLECT)
    assert np.array_equal(oy, y16[:, :32] & 0xFFC0) and np.array_equal(ouv, uv16[:, :32] & 0xFFC0)


def test_accumulator_fits_int32():
    """From the committed tables: the largest sum of |w| of an entry, times 1023, plus the rounding term."""
    assert w10.accumulator_bound("cubic") == (61952, 61952 * 1023 + (1 << 14))
    assert w10.accumulator_bound("lanczos4") == (96336, 98568112)
    assert w10.accumulator_bound("lanczos4")[1] < 2 ** 31
    for r in RESAMPLERS:
        assert (wd.table(r).sum((1, 2)) == 32768).all() and np.abs(wd.table(r)).max() <= 32767


CONTENT = ("random", "extreme", "smooth")


def content(kind, sw, sh):
    rng = np.random.default_rng(13)
    if kind == "random":
        return rng.integers(0, 1024, (sh, sw))
    if kind == "extreme":
        return rng.choice([0, 1023], (sh, sw))
    yy, xx = np.mgrid[0:sh, 0:sw]
    return np.rint(511.5 + 511.5 * np.sin(xx / 9.0) * np.cos(yy / 7.0)).astype(np.int64)


@pytest.mark.parametrize("kind", CONTENT)
@pytest.mark.parametrize("resampler", RESAMPLERS)
def test_within_one_level_of_a_float_statement(resampler, kind):
    """ZOOMED_OUT, map mode 1 with a rotation per row: the integer tables against exact float coefficients of the same quantised position.
    On the 0 / 1023 content the blend overshoots at both ends: both clamps occur, in more than 1800 of the 20000 samples each."""
    sw, sh, (mx, my) = zoomed_out()
    src = content(kind, sw, sh)
    got = w10.remap10(src, mx, my, resampler, wd.CONSTANT, w10.BORDER_Y)
    assert np.abs(got - w10.remap10_float(src, mx, my, resampler, w10.BORDER_Y)).max() <= 1
    if kind == "extreme":
        raw = w10.remap10(src, mx, my, resampler, wd.CONSTANT, w10.BORDER_Y, clamp=False)
        low, high = int((raw < 0).sum()), int((raw > 1023).sum())
        print(resampler, "clamped low", low, "high", high, "of", raw.size)
        assert low > 1800 and high > 1800, (low, high)
        assert got.min() == 0 and got.max() == 1023


def test_known_answers_reproduce():
    n = 0
    for k, y16, uv16, params, mode, resample, border, size, luma, chroma in wd.golden_cases(
            "p010_resample_kat", "y16", "uv16", "params", "mode", "resample", "border", "size", "luma", "chroma"):
        g = wd.golden("p010_resample_kat")
        rb = g[f"case{k}_rot_bottom"] if f"case{k}_rot_bottom" in g else None
        resampler = {v: r for r, v in wd.RESAMPLE.items()}[resample]
        oy, ouv = w10.planar10(y16, uv16, *wd.maps(params, int(size[0]), int(size[1]), mode, rb), resampler, border)
        assert np.array_equal(oy, luma) and np.array_equal(ouv, chroma), k
        assert oy.shape == (size[1], size[0]) and ouv.shape == ((size[1] + 1) // 2, 2 * ((size[0] + 1) // 2))
        assert not (oy & 63).any() and not (ouv & 63).any()
        n += 1
    assert n == 8


# ---------------------------------------------------------------------------------------------------------------------
# 6: refusals
# ---------------------------------------------------------------------------------------------------------------------
EX = "vstab_warp_p010_planar_ex: "
NULL, SIZES = EX + "null pointer", EX + "sizes must be in [1, 32767], source even and at least 8 x 2"
SRC_BAD = EX + "bad source pitch or alignment (16-bit samples; chroma pairs 4-byte aligned)"
DST_BAD = EX + "bad output pitch or alignment (16-bit samples; chroma pairs 4-byte aligned)"
MAP_MODE, PER_ROW = EX + "unknown map mode", EX + "the per-row warp exists for the fisheye -> pinhole modes (0, 1, 5) only"
DEFAULT = EX + "VSTAB_RESAMPLE_DEFAULT (the bilinear warp) is served by vstab_warp_p010_planar"
RESAMPLE = EX + "resample must be VSTAB_RESAMPLE_CUBIC (2) or VSTAB_RESAMPLE_LANCZOS4 (4)"
BORDER = "border_mode must be VSTAB_BORDER_CONSTANT (0), _REPLICATE (1), _REFLECT (2) or _REFLECT_101 (4)"
INVALID, UNSUPPORTED = "ERR_INVALID", "ERR_UNSUPPORTED"
ROT = "rot"
# a call that would be served: 64 x 36 -> 20 x 10
GOOD = dict(y=P, pitch_y=128, uv=2 * P, pitch_uv=128, sw=64, sh=36, params="params", rot_bottom=None, map_mode=0, resample=2, border_mode=0,
            dst_y=3 * P, pitch_dst_y=40, dst_uv=4 * P, pitch_dst_uv=40, dw=20, dh=10, stream=None)
# what differs from GOOD -> status, the whole message; rows that break two checks carry the message of the earlier one
EX_ROWS = [
    (dict(y=None), INVALID, NULL), (dict(uv=None), INVALID, NULL), (dict(dst_y=None), INVALID, NULL), (dict(dst_uv=None), INVALID, NULL),
    (dict(params=None), INVALID, NULL), (dict(y=None, sw=7), INVALID, NULL),
    (dict(sw=6), INVALID, SIZES), (dict(sw=65), INVALID, SIZES), (dict(sh=0), INVALID, SIZES), (dict(sh=37), INVALID, SIZES), (dict(dw=0), INVALID, SIZES),
    (dict(dh=32768), INVALID, SIZES), (dict(sw=32768), INVALID, SIZES), (dict(dw=-1, pitch_y=2), INVALID, SIZES),
    (dict(pitch_y=126), INVALID, SRC_BAD), (dict(pitch_uv=126), INVALID, SRC_BAD), (dict(pitch_y=129), INVALID, SRC_BAD), (dict(pitch_uv=130), INVALID, SRC_BAD),
    (dict(y=P + 1), INVALID, SRC_BAD), (dict(uv=2 * P + 2), INVALID, SRC_BAD), (dict(pitch_y=126, pitch_dst_y=2), INVALID, SRC_BAD),
    (dict(pitch_dst_y=38), INVALID, DST_BAD), (dict(pitch_dst_y=41), INVALID, DST_BAD), (dict(pitch_dst_uv=36), INVALID, DST_BAD),
    (dict(pitch_dst_uv=42), INVALID, DST_BAD), (dict(dst_y=3 * P + 1), INVALID, DST_BAD), (dict(dst_uv=4 * P + 2), INVALID, DST_BAD),
    (dict(dw=21, pitch_dst_y=42), INVALID, DST_BAD),                      # ceil(21 / 2) chroma pairs need 44 bytes
    (dict(pitch_dst_y=38, map_mode=9), INVALID, DST_BAD),
    (dict(map_mode=-1), INVALID, MAP_MODE), (dict(map_mode=6), INVALID, MAP_MODE), (dict(map_mode=6, rot_bottom=ROT), INVALID, MAP_MODE),
    (dict(map_mode=9, resample=0), INVALID, MAP_MODE),
    (dict(map_mode=2, rot_bottom=ROT), INVALID, PER_ROW), (dict(map_mode=3, rot_bottom=ROT), INVALID, PER_ROW),
    (dict(map_mode=4, rot_bottom=ROT, resample=0), INVALID, PER_ROW),
    (dict(resample=0), UNSUPPORTED, DEFAULT), (dict(resample=0, border_mode=3), UNSUPPORTED, DEFAULT),
    (dict(resample=1), INVALID, RESAMPLE), (dict(resample=3), INVALID, RESAMPLE), (dict(resample=-2), INVALID, RESAMPLE), (dict(resample=5, border_mode=3), INVALID, RESAMPLE),
    (dict(border_mode=3), INVALID, EX + BORDER), (dict(border_mode=5), INVALID, EX + BORDER), (dict(border_mode=-1, resample=4), INVALID, EX + BORDER),
    # (the bilinear kernel's "source pitch too large" limit does not exist here: such a pitch passes on to the next check)
    (dict(pitch_y=1 << 24, pitch_uv=1 << 24, border_mode=3), INVALID, EX + BORDER),
]


@pytest.mark.parametrize("row", range(len(EX_ROWS)))
def test_warp_p010_planar_ex_refuses_before_any_launch(vs, row):
    bad, status, text = EX_ROWS[row]
    params = np.zeros(17, np.float32).ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    rot = np.zeros(9, np.float32).ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    args = [{"params": params, ROT: rot}.get(v, v) if isinstance(v, str) else v for v in dict(GOOD, **bad).values()]
    got = vs.lib.vstab_warp_p010_planar_ex(*args)
    assert got == getattr(vs, status), (bad, got, vs.lib.vstab_last_error())
    assert vs.lib.vstab_last_error() == text.encode(), bad


SET = "vstab_set_resample10: "
SET_ROWS = [
    ((None, 2, 0), INVALID, SET + "null handle"), ((None, 9, 9), INVALID, SET + "null handle"), ((None, 0, 1), INVALID, SET + "null handle"),
    ((P, 1, 0), INVALID, SET + "resample must be VSTAB_RESAMPLE_DEFAULT (0), _CUBIC (2) or _LANCZOS4 (4)"),
    ((P, 3, 7), INVALID, SET + "resample must be VSTAB_RESAMPLE_DEFAULT (0), _CUBIC (2) or _LANCZOS4 (4)"),
    ((P, -1, 1), INVALID, SET + "resample must be VSTAB_RESAMPLE_DEFAULT (0), _CUBIC (2) or _LANCZOS4 (4)"),
    ((P, 2, 3), INVALID, SET + BORDER), ((P, 4, 5), INVALID, SET + BORDER), ((P, 0, 3), INVALID, SET + BORDER), ((P, 4, -1), INVALID, SET + BORDER),
    ((P, 0, 1), UNSUPPORTED, SET + "VSTAB_RESAMPLE_DEFAULT (the bilinear warp) has the constant border at 10 bits; border modes are served with _CUBIC and _LANCZOS4"),
    ((P, 0, 4), UNSUPPORTED, SET + "VSTAB_RESAMPLE_DEFAULT (the bilinear warp) has the constant border at 10 bits; border modes are served with _CUBIC and _LANCZOS4"),
]


@pytest.mark.parametrize("row", range(len(SET_ROWS)))
def test_set_resample10_refuses_bad_values_before_reading_the_handle(vs, row):
    args, status, text = SET_ROWS[row]
    got = vs.lib.vstab_set_resample10(*args)
    assert got == getattr(vs, status), (args, got, vs.lib.vstab_last_error())
    assert vs.lib.vstab_last_error() == text.encode(), args


def test_the_binding_declares_both_entry_points(vs):
    assert "vstab_warp_p010_planar_ex" in vs.SIGNATURES and "vstab_set_resample10" in vs.SIGNATURES
    assert callable(vs.warp_p010_planar_ex) and callable(vs.Stabilizer.set_resample10)


# ---------------------------------------------------------------------------------------------------------------------
# 7: tile states (map modes 0 and 1: the oracle's maps need no GPU)
# ---------------------------------------------------------------------------------------------------------------------
def test_budgets_are_the_lds_halves():
    assert w10.BUDGET == {"luma": 24 * 1024 // 2 // 2, "chroma": 24 * 1024 // 2 // 4} and w10.BUDGET["luma"] == wt.BUDGET["bgr"]


@pytest.mark.parametrize("resampler", RESAMPLERS)
@pytest.mark.parametrize("rot", [False, True])
@pytest.mark.parametrize("mode", [0, 1])
def test_zoomed_out_stages_every_box(mode, rot, resampler):
    sw, sh, (mx, my) = zoomed_out(mode, rot)
    largest = {"luma": 0, "chroma": 0}
    for border_mode in (wd.CONSTANT, wd.REFLECT_101):
        s = w10.tile_states(mx, my, sw, sh, resampler, border_mode)
        for plane in ("luma", "chroma"):
            assert s[plane]["gathered"] == 0 and s[plane]["staged"] + s[plane]["none"] == 28, (plane, s[plane])
            largest[plane] = max(largest[plane], s[plane]["largest_staged"])
        if border_mode == wd.CONSTANT:
            assert 2 <= s["luma"]["none"] <= 5, s["luma"]
        else:
            assert s["luma"]["none"] == 0 and s["chroma"]["none"] == 0
    assert largest["luma"] <= 2904 and largest["chroma"] <= 920
    if (resampler, rot) == ("lanczos4", True):
        assert largest == {"luma": 2904, "chroma": 920}


@pytest.mark.parametrize("resampler", RESAMPLERS)
@pytest.mark.parametrize("mode", [0, 1])
def test_gathers_gathers_every_tile(mode, resampler):
    sw, sh, dw, dh, fi, fo = wd.GATHERS
    p, rb = wd.case_params(sw, sh, dw, dh, fi, fo, wd.GATHERS_R0, wd.GATHERS_R_BOTTOM)
    least = {"luma": [], "chroma": []}
    for rot in (None, rb):
        for border_mode in (wd.CONSTANT, wd.REFLECT_101):
            s = w10.tile_states(*wd.maps(p, dw, dh, mode, rot), sw, sh, resampler, border_mode)
            for plane in ("luma", "chroma"):
                assert s[plane]["gathered"] == 4 and s[plane]["staged"] == 0 and s[plane]["none"] == 0
                least[plane].append(s[plane]["least_gathered"])
    assert min(least["luma"]) >= 205755 and min(least["chroma"]) >= 38454
    if resampler == "cubic":
        assert (min(least["luma"]), min(least["chroma"])) == (205755, 38454)


@pytest.mark.parametrize("kernel", ["cubic", "lanczos4"])
def test_all_states_holds_every_state_on_both_planes(kernel):
    s = w10.set_states(kernel, "all_states")
    assert {k: s["luma"][k] for k in ("none", "staged", "gathered", "partial_staged")} == {"none": 12, "staged": 18, "gathered": 18, "partial_staged": 6}
    assert {k: s["chroma"][k] for k in ("none", "staged", "gathered")} == {"none": 12, "staged": 24, "gathered": 12}


# kernel, set -> luma boxes of exactly 6144 words (luma's budget is the 8-bit BGR budget: the committed BGR sets carry over)
LUMA_AT_BUDGET = {("cubic", "bgr_at_budget"): 5, ("cubic", "bgr_at_budget_m0"): 1, ("lanczos4", "bgr_at_budget"): 2, ("cubic_border", "bgr_at_budget"): 2,
                  ("lanczos4_border", "bgr_at_budget"): 1}


@pytest.mark.parametrize("kernel,name", sorted(LUMA_AT_BUDGET))
def test_luma_boxes_of_exactly_the_budget(kernel, name):
    s = w10.set_states(kernel, name)
    assert s["luma"]["at_budget"] == LUMA_AT_BUDGET[kernel, name] and s["luma"]["largest_staged"] == 6144, s["luma"]


def test_a_luma_box_one_over_the_budget():
    s = w10.set_states("cubic", "bgr_over_by_one")["luma"]
    assert s["over_by_one"] == 1 and s["least_gathered"] == 6145 and s["staged"] == 1, s


@pytest.mark.parametrize("kernel", ["cubic_border", "lanczos4_border"])
def test_border_sets(kernel):
    """zoomed_out: 128 tiles, all staged on both planes, with tiles wholly outside, boxes across all four edges, odd and even widths (what
    warp_tiles commits the set to, whatever the budget); gathers: all gathered."""
    s = w10.set_states(kernel, "zoomed_out")
    for plane in ("luma", "chroma"):
        assert s[plane]["staged"] == 128 and s[plane]["gathered"] == 0 and s[plane]["none"] == 0
    full = wt.states_of(kernel, "zoomed_out")
    for plane in ("luma", "chroma"):
        assert full[plane]["staged"] == 128       # (small boxes: staged under the 8-bit budgets as well, so these counts are the 10-bit kernels' too)
        for state, least in wt._EDGES.items():
            assert full[plane][state] >= least, (plane, state)
    g = w10.set_states(kernel, "gathers")
    for plane in ("luma", "chroma"):
        assert g[plane]["gathered"] == 9 and g[plane]["staged"] == 0


@pytest.mark.parametrize("resampler", RESAMPLERS)
def test_a_chroma_box_of_exactly_the_budget(resampler):
    params, sw, sh, dw, dh, mode = w10.chroma_set_params(resampler)
    m = wd.maps(params, dw, dh, mode)
    c = w10.tile_states(*m, sw, sh, resampler, wd.CONSTANT)
    assert c["chroma"]["at_budget"] == 1 and c["chroma"]["staged"] == 2 and c["chroma"]["largest_staged"] == 3072 and c["luma"]["gathered"] == 2, c
    r = w10.tile_states(*m, sw, sh, resampler, wd.REFLECT_101)
    assert r["chroma"]["at_budget"] == 1 and r["chroma"]["staged"] == 1 and r["chroma"]["gathered"] == 1, r
