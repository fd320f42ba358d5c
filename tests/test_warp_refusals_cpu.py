"""The refusals of the bilinear and 10-bit warp entry points, as a table: every distinct message of every entry point, calls that break two
checks at once (the earlier check's message wins: that pins the order), and for vstab_warp_p010_planes one VSTAB_ERR_UNSUPPORTED call
per term of its tiled_ok.  Every call is refused before any device work: the pointers are a dummy non-null address that is never
dereferenced, so the table runs without a GPU.  Each row: entry point, the arguments that differ from a good call, status, and the whole
vstab_last_error() text."""
import ctypes

import numpy as np
import pytest

P = 4096                       # a non-null dummy address, 16-byte aligned
_params = np.zeros(17, np.float32)
_rot = np.zeros(9, np.float32)
FP = _params.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
RB = _rot.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
BGR8, NV12, PLANAR = 0, 1, 2   # VSTAB_OUT_*
INVALID, UNSUPPORTED = "ERR_INVALID", "ERR_UNSUPPORTED"
M16, G4 = 1 << 24, 1 << 32

# a good call of every entry point, arguments in the order of include/vstab.h
_NV12 = dict(y=P, pitch_y=64, uv=P, pitch_uv=64, sw=64, sh=32, params=FP)
_OUT = dict(dst=P, pitch_dst=192, dst_uv=None, pitch_dst_uv=0, dw=32, dh=16, stream=None)
_P010 = dict(y=P, pitch_y=128, uv=P, pitch_uv=128, sw=64, sh=32, params=FP, rot_bottom=None, map_mode=0, blend=0)
_P010_OUT = dict(dst_y=P, pitch_dst_y=64, dst_uv=P, pitch_dst_uv=64, dw=32, dh=16, stream=None)
GOOD = {
    "vstab_warp_nv12_ex": dict(_NV12, map_mode=0, out_format=BGR8, **_OUT),
    "vstab_warp_nv12_rs": dict(_NV12, rot_bottom=RB, map_mode=0, out_format=BGR8, **_OUT),
    "vstab_warp_nv12_mapped": dict(y=P, pitch_y=64, uv=P, pitch_uv=64, sw=64, sh=32, qmap=P, out_format=BGR8, **_OUT),
    "vstab_warp_nv12_nearest_ex": dict(_NV12, map_mode=0, dst=P, pitch_dst=96, dw=32, dh=16, stream=None),
    "vstab_quantised_map": dict(qmap=P, dw=32, dh=16, params=FP, map_mode=0, stream=None),
    "vstab_warp_p010": dict(_P010, dst=P, pitch_dst=192, dw=32, dh=16, stream=None),
    "vstab_warp_p010_planes": dict(_P010, **_P010_OUT),
    "vstab_warp_p010_planar": dict(_P010, **_P010_OUT),
    "vstab_cvt_bgr16_p010": dict(src=P, pitch_src=192, width=32, height=16, dst_y=P, pitch_y=64, dst_uv=P, pitch_uv=64, stream=None),
    "vstab_create_map_ex": dict(map_x=P, pitch_x=128, map_y=P, pitch_y=128, cols=32, rows=16, params=FP, map_mode=0, stream=None),
    "vstab_remap_bilinear": dict(src=P, pitch_src=64, sw=64, sh=32, channels=1, map_x=P, pitch_x=128, map_y=P, pitch_y=128, dst=P, pitch_dst=32,
                                 dw=32, dh=16, stream=None),
}

_PLANAR_OUT = dict(out_format=PLANAR, pitch_dst=32, dst_uv=P, pitch_dst_uv=32)
_NEED_TILED = "vstab_warp_p010_planes: needs 16-byte aligned source planes and a fisheye -> pinhole map"
_P010_SIZES = ": sizes must be in [1, 32767], source even and at least "
_P010_OUTPUT = ": bad output pitch or alignment (16-bit samples; chroma pairs 4-byte aligned)"


def _warp_impl_rows(fn):
    """The checks vstab_warp_nv12_ex, _rs and _mapped share (their messages stand under vstab_warp_nv12), in their order."""
    n = "vstab_warp_nv12: "
    rows = [
        (fn, dict(y=None), INVALID, n + "null pointer"),
        (fn, dict(uv=None), INVALID, n + "null pointer"),
        (fn, dict(dst=None), INVALID, n + "null pointer"),
        (fn, dict(dst=None, sw=63), INVALID, n + "null pointer"),
        (fn, dict(sw=0), INVALID, n + "source must be even-sized and <= 32767"),
        (fn, dict(sw=63), INVALID, n + "source must be even-sized and <= 32767"),
        (fn, dict(sh=31), INVALID, n + "source must be even-sized and <= 32767"),
        (fn, dict(sw=32768, pitch_y=32768, pitch_uv=32768), INVALID, n + "source must be even-sized and <= 32767"),
        (fn, dict(sh=32768), INVALID, n + "source must be even-sized and <= 32767"),
        (fn, dict(sh=-2, dw=0), INVALID, n + "source must be even-sized and <= 32767"),
        (fn, dict(dw=0), INVALID, n + "output size must be in [1, 32767]"),
        (fn, dict(dh=0), INVALID, n + "output size must be in [1, 32767]"),
        (fn, dict(dw=32768, pitch_dst=98304), INVALID, n + "output size must be in [1, 32767]"),
        (fn, dict(dh=32768, out_format=7), INVALID, n + "output size must be in [1, 32767]"),
        (fn, dict(out_format=3), INVALID, n + "unknown output format"),
        (fn, dict(out_format=-1, pitch_y=63), INVALID, n + "unknown output format"),
        (fn, dict(pitch_y=63), INVALID, n + "pitch smaller than row"),
        (fn, dict(pitch_uv=62), INVALID, n + "pitch smaller than row"),
        (fn, dict(pitch_dst=95), INVALID, n + "pitch smaller than row"),
        (fn, dict(out_format=NV12, pitch_dst=31, dst_uv=P, pitch_dst_uv=32), INVALID, n + "pitch smaller than row"),
        (fn, dict(out_format=NV12, pitch_dst=31), INVALID, n + "pitch smaller than row"),
        (fn, dict(out_format=NV12, pitch_dst=32), INVALID, n + "NV12 output needs a chroma plane of 2*ceil(width/2) bytes per row"),
        (fn, dict(out_format=NV12, pitch_dst=32, dst_uv=P, pitch_dst_uv=31), INVALID,
         n + "NV12 output needs a chroma plane of 2*ceil(width/2) bytes per row"),
        (fn, dict(out_format=PLANAR, pitch_dst=32, dst_uv=P, pitch_dst_uv=30, uv=P + 1), INVALID,
         n + "NV12 output needs a chroma plane of 2*ceil(width/2) bytes per row"),
        (fn, dict(uv=P + 1), INVALID, n + "chroma plane must be 2-B aligned"),
        (fn, dict(pitch_uv=65), INVALID, n + "chroma plane must be 2-B aligned"),
        (fn, dict(_PLANAR_OUT, sw=14, pitch_uv=65), INVALID, n + "chroma plane must be 2-B aligned"),
        (fn, dict(_PLANAR_OUT, pitch_y=M16), INVALID, n + "source pitch too large for this mode"),
        (fn, dict(out_format=NV12, pitch_dst=32, dst_uv=P, pitch_dst_uv=32, pitch_uv=M16), INVALID, n + "source pitch too large for this mode"),
        (fn, dict(_PLANAR_OUT, sw=14, pitch_y=65536, sh=32766 * 2), INVALID, n + "source must be even-sized and <= 32767"),
    ]
    return rows


def _rows():
    rows = []
    # ---- vstab_warp_nv12_ex -------------------------------------------------------------------------------------------------------
    fn, n = "vstab_warp_nv12_ex", "vstab_warp_nv12: "
    rows += _warp_impl_rows(fn)
    rows += [
        (fn, dict(params=None), INVALID, n + "null pointer"),
        (fn, dict(map_mode=-1), INVALID, n + "unknown map mode"),
        (fn, dict(map_mode=6), INVALID, n + "unknown map mode"),
        (fn, dict(map_mode=6, out_format=3), INVALID, n + "unknown map mode"),
        (fn, dict(dw=0, map_mode=6), INVALID, n + "output size must be in [1, 32767]"),
        (fn, dict(map_mode=1, pitch_y=M16), INVALID, n + "source pitch too large for this mode"),
        (fn, dict(map_mode=5, pitch_uv=M16), INVALID, n + "source pitch too large for this mode"),
        (fn, dict(map_mode=1, pitch_y=M16 - 16, sh=258), INVALID, n + "source pitch too large for this mode"),
        (fn, dict(map_mode=1, pitch_y=M16, uv=P + 1), INVALID, n + "chroma plane must be 2-B aligned"),
        (fn, dict(_PLANAR_OUT, sw=14), INVALID, n + "the plane-wise warp needs a source of at least 16 x 2"),
        (fn, dict(_PLANAR_OUT, sw=14, pitch_y=M16), INVALID, n + "source pitch too large for this mode"),
    ]
    # ---- vstab_warp_nv12_rs -------------------------------------------------------------------------------------------------------
    fn = "vstab_warp_nv12_rs"
    per_row = "vstab_warp_nv12_rs: the per-row warp exists for the fisheye -> pinhole modes (0, 1, 5) only"
    rows += _warp_impl_rows(fn)
    rows += [
        (fn, dict(rot_bottom=None), INVALID, "vstab_warp_nv12_rs: null pointer"),
        (fn, dict(rot_bottom=None, y=None, sw=63), INVALID, "vstab_warp_nv12_rs: null pointer"),
        (fn, dict(params=None), INVALID, n + "null pointer"),
        (fn, dict(map_mode=6), INVALID, n + "unknown map mode"),
        (fn, dict(map_mode=2), INVALID, per_row),
        (fn, dict(map_mode=3), INVALID, per_row),
        (fn, dict(map_mode=4), INVALID, per_row),
        (fn, dict(map_mode=2, uv=P + 1), INVALID, n + "chroma plane must be 2-B aligned"),
        (fn, dict(map_mode=2, pitch_y=M16), INVALID, per_row),
        (fn, dict(map_mode=0, pitch_y=M16), INVALID, n + "source pitch too large for this mode"),
        (fn, dict(_PLANAR_OUT, map_mode=5, sh=0), INVALID, n + "source must be even-sized and <= 32767"),
        (fn, dict(_PLANAR_OUT, map_mode=5, sw=8, pitch_y=M16), INVALID, n + "source pitch too large for this mode"),
        (fn, dict(_PLANAR_OUT, map_mode=5, sw=8), INVALID, n + "the plane-wise warp needs a source of at least 16 x 2"),
    ]
    # ---- vstab_warp_nv12_mapped ---------------------------------------------------------------------------------------------------
    fn = "vstab_warp_nv12_mapped"
    qm = "vstab_warp_nv12_mapped: the quantised map must be a 16-byte aligned device buffer"
    rows += _warp_impl_rows(fn)
    rows += [
        (fn, dict(qmap=None), INVALID, qm),
        (fn, dict(qmap=P + 8), INVALID, qm),
        (fn, dict(qmap=P + 8, y=None), INVALID, qm),
        (fn, dict(pitch_y=M16), INVALID, n + "source pitch too large for this mode"),
        (fn, dict(_PLANAR_OUT), UNSUPPORTED,
         "vstab_warp_nv12_mapped: the quantised map holds no chroma positions -- VSTAB_OUT_NV12_PLANAR goes through vstab_warp_nv12_ex"),
        (fn, dict(_PLANAR_OUT, sw=14), UNSUPPORTED,
         "vstab_warp_nv12_mapped: the quantised map holds no chroma positions -- VSTAB_OUT_NV12_PLANAR goes through vstab_warp_nv12_ex"),
        (fn, dict(_PLANAR_OUT, pitch_uv=M16), INVALID, n + "source pitch too large for this mode"),
    ]
    # ---- vstab_warp_nv12_nearest_ex -----------------------------------------------------------------------------------------------
    fn, n = "vstab_warp_nv12_nearest_ex", "vstab_warp_nv12_nearest: "
    sizes, pitch = n + "sizes must be in [1, 32767], source even", n + "bad pitch or chroma alignment"
    modes = n + "the nearest-neighbour warp exists for the reference's own map (modes 0 and 5)"
    rows += [(fn, {k: None}, INVALID, n + "null pointer") for k in ("y", "uv", "dst", "params")]
    rows += [(fn, dict(y=None, sw=0), INVALID, n + "null pointer")]
    rows += [(fn, d, INVALID, sizes) for d in (dict(sw=0), dict(sh=0), dict(sw=63), dict(sh=31), dict(sw=32768), dict(sh=32768), dict(dw=0), dict(dh=0),
                                               dict(dw=32768), dict(dh=32768), dict(dw=0, pitch_y=1), dict(sw=63, map_mode=1, uv=P + 1))]
    rows += [(fn, d, INVALID, pitch) for d in (dict(pitch_y=63), dict(pitch_uv=62), dict(pitch_dst=95), dict(uv=P + 1), dict(pitch_uv=65),
                                               dict(pitch_uv=65, map_mode=1))]
    rows += [(fn, dict(map_mode=m), INVALID, modes) for m in (1, 2, 3, 4, 6, -1)]
    # ---- vstab_quantised_map ------------------------------------------------------------------------------------------------------
    fn, n = "vstab_quantised_map", "vstab_quantised_map: "
    rows += [(fn, d, INVALID, n + "bad argument") for d in (dict(qmap=None), dict(params=None), dict(dw=0), dict(dh=0), dict(dw=32768), dict(dh=32768),
                                                            dict(dw=0, map_mode=6), dict(qmap=None, map_mode=-1))]
    rows += [(fn, d, INVALID, n + "unknown map mode") for d in (dict(map_mode=-1), dict(map_mode=6), dict(map_mode=6, qmap=P + 4))]
    rows += [(fn, d, INVALID, n + "the buffer must be 16-byte aligned") for d in (dict(qmap=P + 4), dict(qmap=P + 8, map_mode=5))]
    # ---- vstab_warp_p010 ----------------------------------------------------------------------------------------------------------
    fn, n = "vstab_warp_p010", "vstab_warp_p010"
    pitch = n + ": bad pitch or alignment (16-bit samples; chroma pairs 4-byte aligned)"
    rows += [(fn, {k: None}, INVALID, n + ": null pointer") for k in ("y", "uv", "dst", "params")]
    rows += [(fn, dict(dst=None, sw=2), INVALID, n + ": null pointer")]
    rows += [(fn, d, INVALID, n + _P010_SIZES + "4 x 2") for d in (dict(sw=2), dict(sh=0), dict(sw=5), dict(sh=3), dict(dw=0), dict(dh=0), dict(sw=32768),
                                                                   dict(sh=32768), dict(dw=32768), dict(dh=32768), dict(sw=2, pitch_y=2), dict(dh=0, blend=2))]
    rows += [(fn, d, INVALID, pitch) for d in (dict(pitch_y=126), dict(pitch_uv=124), dict(pitch_dst=190), dict(pitch_y=129), dict(pitch_uv=130),
                                               dict(pitch_dst=193), dict(y=P + 1), dict(uv=P + 2), dict(dst=P + 1), dict(uv=P + 2, map_mode=6))]
    rows += [(fn, d, INVALID, n + ": unknown map mode") for d in (dict(map_mode=-1), dict(map_mode=6), dict(map_mode=6, blend=2))]
    rows += [(fn, d, INVALID, n + ": unknown blend") for d in (dict(blend=2), dict(blend=-1), dict(blend=2, map_mode=3, rot_bottom=RB))]
    # ---- vstab_warp_p010_planes ---------------------------------------------------------------------------------------------------
    fn, n = "vstab_warp_p010_planes", "vstab_warp_p010_planes"
    rows += [(fn, {k: None}, INVALID, n + ": null pointer") for k in ("y", "uv", "dst_y", "dst_uv", "params")]
    rows += [(fn, dict(dst_uv=None, sw=4), INVALID, n + ": null pointer")]
    rows += [(fn, d, INVALID, n + _P010_SIZES + "8 x 2") for d in (dict(sw=4), dict(sw=6), dict(sh=0), dict(sw=9), dict(sh=3), dict(dw=0), dict(dh=0),
                                                                   dict(sw=32768), dict(sh=32768), dict(dw=32768), dict(dh=32768), dict(sw=6, pitch_dst_y=62))]
    rows += [(fn, d, INVALID, n + _P010_OUTPUT) for d in (dict(pitch_dst_y=62), dict(pitch_dst_y=65), dict(pitch_dst_uv=60), dict(pitch_dst_uv=66),
                                                          dict(dst_y=P + 1), dict(dst_uv=P + 2), dict(dst_uv=P + 2, blend=2))]
    rows += [(fn, d, INVALID, n + ": unknown blend") for d in (dict(blend=2), dict(blend=-1), dict(blend=2, map_mode=2), dict(blend=2, y=P + 8))]
    rows += [(fn, d, UNSUPPORTED, _NEED_TILED) for d in (            # one per term of tiled_ok, in its order
        dict(map_mode=2), dict(map_mode=3), dict(map_mode=4), dict(map_mode=6), dict(map_mode=-1), dict(map_mode=2, rot_bottom=RB),
        dict(y=P + 8), dict(uv=P + 8), dict(pitch_y=136), dict(pitch_uv=136), dict(pitch_y=112), dict(pitch_uv=112),
        dict(pitch_y=M16), dict(pitch_uv=M16), dict(pitch_y=M16 - 16, sh=258), dict(pitch_dst_y=M16, dh=256),
        dict(y=P + 2), dict(uv=P + 4), dict(pitch_y=126), dict(pitch_uv=124))]
    # ---- vstab_warp_p010_planar ---------------------------------------------------------------------------------------------------
    fn, n = "vstab_warp_p010_planar", "vstab_warp_p010_planar"
    source = n + ": bad source pitch or alignment (16-bit samples; chroma pairs 4-byte aligned)"
    per_row = n + ": the per-row warp exists for the fisheye -> pinhole modes (0, 1, 5) only"
    rows += [(fn, {k: None}, INVALID, n + ": null pointer") for k in ("y", "uv", "dst_y", "dst_uv", "params")]
    rows += [(fn, dict(y=None, sw=4), INVALID, n + ": null pointer")]
    rows += [(fn, d, INVALID, n + _P010_SIZES + "8 x 2") for d in (dict(sw=4), dict(sw=6), dict(sh=0), dict(sw=9), dict(sh=3), dict(dw=0), dict(dh=0),
                                                                   dict(sw=32768), dict(sh=32768), dict(dw=32768), dict(dh=32768), dict(sw=6, pitch_y=2))]
    rows += [(fn, d, INVALID, source) for d in (dict(pitch_y=126), dict(pitch_uv=124), dict(pitch_y=129), dict(pitch_uv=130), dict(y=P + 1), dict(uv=P + 2),
                                                dict(uv=P + 2, pitch_dst_y=62))]
    rows += [(fn, d, INVALID, n + _P010_OUTPUT) for d in (dict(pitch_dst_y=62), dict(pitch_dst_y=65), dict(pitch_dst_uv=60), dict(pitch_dst_uv=66),
                                                          dict(dst_y=P + 1), dict(dst_uv=P + 2), dict(dst_uv=P + 2, map_mode=6))]
    rows += [(fn, d, INVALID, n + ": unknown map mode") for d in (dict(map_mode=-1), dict(map_mode=6), dict(map_mode=6, blend=2))]
    rows += [(fn, d, INVALID, n + ": unknown blend") for d in (dict(blend=2), dict(blend=-1), dict(blend=2, map_mode=2, rot_bottom=RB))]
    rows += [(fn, d, INVALID, per_row) for d in (dict(map_mode=2, rot_bottom=RB), dict(map_mode=3, rot_bottom=RB), dict(map_mode=4, rot_bottom=RB),
                                                 dict(map_mode=4, rot_bottom=RB, pitch_y=M16))]
    rows += [(fn, d, INVALID, n + ": source pitch too large") for d in (dict(pitch_y=M16), dict(pitch_uv=M16), dict(pitch_y=M16 - 16, sh=258),
                                                                        dict(pitch_y=M16, rot_bottom=RB, map_mode=5))]
    # ---- vstab_cvt_bgr16_p010 -----------------------------------------------------------------------------------------------------
    fn, n = "vstab_cvt_bgr16_p010", "vstab_cvt_bgr16_p010: "
    rows += [(fn, {k: None}, INVALID, n + "null pointer") for k in ("src", "dst_y", "dst_uv")]
    rows += [(fn, dict(src=None, width=0), INVALID, n + "null pointer")]
    rows += [(fn, d, INVALID, n + "sizes must be in [1, 32767]") for d in (dict(width=0), dict(height=0), dict(width=32768), dict(height=32768),
                                                                            dict(width=0, pitch_src=1))]
    rows += [(fn, d, INVALID, n + "bad pitch or alignment (16-bit samples; chroma pairs 4-byte aligned)")
             for d in (dict(pitch_src=190), dict(pitch_src=193), dict(pitch_y=62), dict(pitch_y=65), dict(pitch_uv=60), dict(pitch_uv=66), dict(src=P + 1),
                       dict(dst_y=P + 1), dict(dst_uv=P + 2), dict(width=31, pitch_uv=62))]
    # ---- vstab_create_map_ex ------------------------------------------------------------------------------------------------------
    fn, n = "vstab_create_map_ex", "vstab_create_map: "
    rows += [(fn, {k: None}, INVALID, n + "null pointer") for k in ("map_x", "map_y", "params")]
    rows += [(fn, dict(map_x=None, cols=0), INVALID, n + "null pointer")]
    rows += [(fn, d, INVALID, n + "size must be in [1, 32767] (createMap.cl:10-11)") for d in (dict(cols=0), dict(rows=0), dict(cols=32768), dict(rows=32768),
                                                                                                dict(cols=0, pitch_x=2))]
    rows += [(fn, d, INVALID, n + "bad pitch") for d in (dict(pitch_x=124), dict(pitch_y=124), dict(pitch_x=130), dict(pitch_y=130),
                                                         dict(pitch_x=130, map_mode=6))]
    rows += [(fn, dict(map_mode=m), INVALID, n + "unknown map mode") for m in (-1, 6)]
    # ---- vstab_remap_bilinear -----------------------------------------------------------------------------------------------------
    fn, n = "vstab_remap_bilinear", "vstab_remap_bilinear: "
    rows += [(fn, {k: None}, INVALID, n + "null pointer") for k in ("src", "map_x", "map_y", "dst")]
    rows += [(fn, dict(dst=None, channels=2), INVALID, n + "null pointer")]
    rows += [(fn, d, INVALID, n + "channels must be 1 or 3") for d in (dict(channels=0), dict(channels=2), dict(channels=4), dict(channels=2, sw=0))]
    rows += [(fn, d, INVALID, n + "bad size") for d in (dict(sw=0), dict(sh=0), dict(dw=0), dict(dh=0), dict(sw=32768), dict(sh=32768),
                                                        dict(sw=0, pitch_x=4))]
    rows += [(fn, d, INVALID, n + "pitch smaller than row") for d in (dict(pitch_src=63), dict(pitch_dst=31), dict(pitch_x=124), dict(pitch_y=124),
                                                                      dict(channels=3, pitch_src=191, pitch_dst=96), dict(channels=3, pitch_src=192, pitch_dst=95))]
    return rows


ROWS = _rows()


def test_the_table_names_every_entry_point():
    assert {fn for fn, _, _, _ in ROWS} == set(GOOD)
    for fn, bad, _, _ in ROWS:
        assert bad and set(bad) <= set(GOOD[fn]), (fn, bad)


@pytest.mark.parametrize("fn", sorted(GOOD))
def test_warp_entry_points_refuse_bad_arguments_without_a_device(vs, fn):
    L = vs.lib
    for name, bad, status, text in ROWS:
        if name != fn:
            continue
        got = getattr(L, fn)(*dict(GOOD[fn], **bad).values())
        assert got == getattr(vs, status), (fn, bad, got, L.vstab_last_error())
        assert L.vstab_last_error() == text.encode(), (fn, bad)
