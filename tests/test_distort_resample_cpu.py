"""CPU tests of the calibrated lens in the cubic, Lanczos and border warps (include/vstab.h, vstab_warp_nv12_dist_ex and
vstab_set_input_calibration_ex): the refusals as a table in the style of test_distort_refusals_cpu.py (every distinct message, calls that
break two checks at once -- the earlier check's message wins, which pins the documented order --, every call refused before any device
work: the device pointers are a dummy address), the unchanged ABI, the tile states the GPU tests' shapes are there for (from the committed
CPU model of the kernels' boxes, tests/warp_tiles.py, over the distorted maps), the golden file against the definition, and the new
kernels' private segments against their siblings' (from the built library's kernel metadata)."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import distort_def as dd
import oracle
import warp_def as wd
import warp_tiles as wt
from test_distort_gpu import cameras
from test_distort_refusals_cpu import BGR8, D_BAD, DD, DF, FISH, FOLD, FP, INVALID, K9, M16, NV12, OTHER_MODES, P, PLANAR, f32, f64
from test_lens_gpu import ROTS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(os.path.dirname(__file__), "golden")
DEFAULT, CUBIC, LANCZOS4 = 0, 2, 4       # VSTAB_RESAMPLE_*

GOOD = {
    "vstab_warp_nv12_dist_ex": dict(y=P, pitch_y=64, uv=P, pitch_uv=64, sw=64, sh=32, params=FP, dist=DF, map_mode=1, resample=CUBIC, border_mode=4,
                                    out_format=BGR8, dst=P, pitch_dst=192, dst_uv=None, pitch_dst_uv=0, dw=32, dh=16, stream=None),
    "vstab_set_input_calibration_ex": dict(h=None, K=K9, D=DD),
}
_PLANAR_OUT = dict(out_format=PLANAR, pitch_dst=32, dst_uv=P, pitch_dst_uv=32)
_LINEAR = dict(resample=DEFAULT, border_mode=0)      # delegates to vstab_warp_nv12_dist once every check of the new entry point has passed


def _rows():
    rows = []
    fn, n = "vstab_warp_nv12_dist_ex", "vstab_warp_nv12_dist_ex: "
    fmt = n + "the distorted-lens warp emits VSTAB_OUT_BGR8 or VSTAB_OUT_NV12_PLANAR (NV12 through BGR is not served)"
    bm = n + "border_mode must be VSTAB_BORDER_CONSTANT (0), _REPLICATE (1), _REFLECT (2) or _REFLECT_101 (4)"
    rs = n + "resample must be VSTAB_RESAMPLE_DEFAULT (0), _CUBIC (2) or _LANCZOS4 (4)"
    # 1. dist null, before everything; 2. check_warp_nv12's checks in its order
    rows += [(fn, {k: None}, INVALID, n + "null pointer") for k in ("y", "uv", "dst", "params", "dist")]
    rows += [(fn, d, INVALID, n + "null pointer") for d in (dict(dst=None, sw=63), dict(dist=None, map_mode=0), dict(dist=None, sw=63),
                                                            dict(dist=None, resample=1), dict(dist=None, border_mode=3), dict(_LINEAR, dist=None))]
    rows += [(fn, d, INVALID, n + "source must be even-sized and <= 32767") for d in (
        dict(sw=0), dict(sw=63), dict(sh=31), dict(sw=32768, pitch_y=32768, pitch_uv=32768), dict(sh=32768), dict(sh=-2, dw=0), dict(sw=63, resample=1))]
    rows += [(fn, d, INVALID, n + "output size must be in [1, 32767]") for d in (
        dict(dw=0), dict(dh=0), dict(dw=32768, pitch_dst=98304), dict(dh=32768, out_format=7), dict(dw=0, map_mode=6), dict(dw=0, resample=1),
        dict(dh=0, border_mode=3))]
    rows += [(fn, d, INVALID, fmt) for d in (dict(out_format=NV12, pitch_dst=32, dst_uv=P, pitch_dst_uv=32), dict(out_format=3), dict(out_format=-1, pitch_y=63),
                                             dict(out_format=NV12, map_mode=0), dict(out_format=3, border_mode=3), dict(_LINEAR, out_format=NV12))]
    rows += [(fn, dict(border_mode=b), INVALID, bm) for b in (3, 5, -1, 8, 16)]
    rows += [(fn, d, INVALID, bm) for d in (dict(border_mode=3, pitch_y=63), dict(border_mode=3, resample=1), dict(border_mode=3, map_mode=0),
                                            dict(border_mode=3, resample=DEFAULT), dict(border_mode=5, dist=f32(D_BAD[4])))]
    rows += [(fn, d, INVALID, n + "pitch smaller than row") for d in (dict(pitch_y=63), dict(pitch_uv=62), dict(pitch_dst=95), dict(_PLANAR_OUT, pitch_dst=31),
                                                                      dict(pitch_dst=95, dist=f32(D_BAD[4])), dict(pitch_dst=95, resample=1))]
    rows += [(fn, d, INVALID, n + "plane-wise output needs a chroma plane of 2*ceil(width/2) bytes per row") for d in (
        dict(_PLANAR_OUT, dst_uv=None), dict(_PLANAR_OUT, pitch_dst_uv=31), dict(_PLANAR_OUT, pitch_dst_uv=30, uv=P + 1))]
    rows += [(fn, d, INVALID, n + "chroma plane must be 2-B aligned") for d in (dict(uv=P + 1), dict(pitch_uv=65), dict(uv=P + 1, map_mode=3),
                                                                                dict(uv=P + 1, resample=3))]
    # 3. the resampler, before the map mode and the coefficients
    rows += [(fn, dict(resample=r), INVALID, rs) for r in (1, 3, 5, -1)]
    rows += [(fn, d, INVALID, rs) for d in (dict(resample=1, map_mode=0), dict(resample=3, dist=f32(D_BAD[0])), dict(resample=5, map_mode=6, dist=f32(D_BAD[4])),
                                            dict(_PLANAR_OUT, resample=-1), dict(resample=1, border_mode=0))]
    # 4. the map mode, before the coefficients
    rows += [(fn, dict(map_mode=m, resample=r), INVALID, n + FISH) for m in OTHER_MODES for r in (DEFAULT, CUBIC, LANCZOS4)]
    rows += [(fn, d, INVALID, n + FISH) for d in (dict(map_mode=4, dist=f32(D_BAD[0])), dict(_PLANAR_OUT, map_mode=5), dict(_LINEAR, map_mode=0),
                                                  dict(_LINEAR, map_mode=3, dist=f32(D_BAD[5])))]
    # 5. the coefficients
    rows += [(fn, dict(dist=f32(d), map_mode=m), INVALID, n + FOLD) for d in D_BAD for m in (1, 2)]
    rows += [(fn, dict(dist=f32(D_BAD[5]), resample=r, border_mode=b), INVALID, n + FOLD) for r in (DEFAULT, CUBIC, LANCZOS4) for b in (0, 1, 2, 4)]
    rows += [(fn, dict(_PLANAR_OUT, dist=f32(D_BAD[5])), INVALID, n + FOLD), (fn, dict(_LINEAR, dist=f32(D_BAD[5]), pitch_y=M16), INVALID, n + FOLD)]
    # (INTER_LINEAR with the constant border is vstab_warp_nv12_dist: what that refuses behind its argument checks, under its own name)
    rows += [(fn, dict(_LINEAR, pitch_y=M16), INVALID, "vstab_warp_nv12: source pitch too large for this mode"),
             (fn, dict(_LINEAR, **_PLANAR_OUT, sw=14), INVALID, "vstab_warp_nv12: the plane-wise warp needs a source of at least 16 x 2")]
    # ---- vstab_set_input_calibration_ex (everything else needs a live handle: test_distort_resample_gpu.py) ------------------------
    fn, n = "vstab_set_input_calibration_ex", "vstab_set_input_calibration_ex: "
    rows += [(fn, d, INVALID, n + "null argument") for d in (dict(h=None), dict(h=None, D=None), dict(h=None, K=None), dict(h=None, D=f64(D_BAD[4])))]
    return rows


ROWS = _rows()


def test_the_table_names_both_entry_points_and_every_message():
    assert {fn for fn, _, _, _ in ROWS} == set(GOOD)
    for fn, bad, _, _ in ROWS:
        assert bad and set(bad) <= set(GOOD[fn]), (fn, bad)
    # every message include/vstab.h states for vstab_warp_nv12_dist_ex is in the table
    text = " ".join(open(os.path.join(ROOT, "include", "vstab.h")).read().replace(" *", " ").split())
    doc = text[text.index("vstab_warp_nv12_dist for every 8-bit resampler"):text.index("VSTAB_API vstab_status vstab_warp_nv12_dist_ex")]
    stated = set(re.findall(r'"([^"]+)"', doc)) - {"Lens distortion", "vstab_warp_nv12_dist_ex: "}
    tabled = {t.split(": ", 1)[1] for fn, _, _, t in ROWS if t.startswith("vstab_warp_nv12_dist_ex: ")}
    assert len(stated) == 11 and stated == tabled, (stated ^ tabled)


@pytest.mark.parametrize("fn", sorted(GOOD))
def test_new_entry_points_refuse_bad_arguments_without_a_device(vs, fn):
    L = vs.lib
    n = 0
    for name, bad, status, text in ROWS:
        if name != fn:
            continue
        got = getattr(L, fn)(*dict(GOOD[fn], **bad).values())
        assert got == getattr(vs, status), (fn, bad, got, L.vstab_last_error())
        assert L.vstab_last_error() == text.encode(), (fn, bad, L.vstab_last_error())
        n += 1
    assert n >= 4


def test_abi_version_and_struct_sizes_are_unchanged(vs):
    """No struct changed: the layout version and the five struct sizes are the parent's."""
    assert vs.lib.vstab_abi_version() == 0x56534206 == vs.ABI_VERSION
    assert [vs.lib.vstab_struct_size(k) for k in range(6)] == [104, 24, 144, 168, 160, -1]
    assert vs.RESAMPLE_DEFAULT == DEFAULT and vs.RESAMPLE_CUBIC == CUBIC and vs.RESAMPLE_LANCZOS4 == LANCZOS4


# ---------------------------------------------------------------------------------------------------------------------
# tile states of the shapes test_distort_resample_gpu.py runs
# ---------------------------------------------------------------------------------------------------------------------
def shape_maps(w, h, dw, dh, mode, rv, D=dd.D_A):
    Kin, Kout = cameras(w, h, dw, dh, mode)
    return dd.maps(oracle.map_params(Kin, Kout, oracle.rodrigues(rv)), dw, dh, mode, D)


KERNELS = [(r, b) for r in wd.RESAMPLERS for b in (wd.CONSTANT, wd.REFLECT_101) if (r, b) != ("linear", wd.CONSTANT)]
PLANES = ("bgr", "luma", "chroma")


def test_tile_states_640x360_every_tile_staged_partial_tiles_and_crossings():
    w, h, dw, dh = 640, 360, 333, 201
    mx, my = shape_maps(w, h, dw, dh, 1, ROTS[1])
    for r, b in KERNELS:
        st = wt.tile_states(mx, my, w, h, r, wt.kernel_rule(r, b))
        for pl in PLANES:
            s = st[pl]
            assert s["staged"] == 78 and s["gathered"] == 0 and s["odd_w"] > 0 and s["even_w"] > 0, (r, b, pl, s)
            if b == wd.CONSTANT:
                assert s["none"] == 0 and s["partial_staged"] == 18, (r, b, pl, s)
    mx, my = shape_maps(w, h, dw, dh, 2, ROTS[1])
    for r, b in KERNELS:
        st = wt.tile_states(mx, my, w, h, r, wt.kernel_rule(r, b))
        s = st["bgr"]
        assert s["gathered"] == 0
        if b == wd.CONSTANT:
            assert s["none"] > 0 and s["staged"] > 0 and s["partial_staged"] > 0, (r, s)       # tiles with no box beside staged ones
        else:
            assert s["outside_staged"] > 0 and min(s["cross_l"], s["cross_r"], s["cross_t"], s["cross_b"]) > 0, (r, s)
            c = st["chroma"]
            assert min(c["cross_l"], c["cross_r"], c["cross_t"], c["cross_b"]) > 0, (r, c)


def test_tile_states_1024x576_staged_and_gathered_in_one_launch():
    w, h, dw, dh = 1024, 576, 200, 72
    mx, my = shape_maps(w, h, dw, dh, 1, ROTS[1])
    for r, b in KERNELS:
        st = wt.tile_states(mx, my, w, h, r, wt.kernel_rule(r, b))
        for pl in PLANES:
            assert st[pl]["staged"] > 0 and st[pl]["gathered"] > 0, (r, b, pl, st[pl])
        assert st["bgr"]["staged"] + st["bgr"]["gathered"] == 20
    mx, my = shape_maps(w, h, dw, dh, 2, ROTS[1])
    for r, b in KERNELS:
        st = wt.tile_states(mx, my, w, h, r, wt.kernel_rule(r, b))
        for pl in PLANES:
            assert st[pl]["gathered"] > 0, (r, b, pl, st[pl])
            if b == wd.CONSTANT:
                assert st[pl]["none"] > 0, (r, pl, st[pl])         # mode 2 adds tiles with no box
            else:
                assert st[pl]["staged"] > 0 and st[pl]["outside_staged"] > 0, (r, pl, st[pl])
        assert st["chroma"]["staged"] > 0


def test_tile_states_2048x1152_every_tile_gathers():
    w, h, dw, dh = 2048, 1152, 256, 128
    for mode in (1, 2):
        mx, my = shape_maps(w, h, dw, dh, mode, ROTS[1])
        for r, b in KERNELS:
            st = wt.tile_states(mx, my, w, h, r, wt.kernel_rule(r, b))
            for pl in PLANES:
                assert st[pl]["staged"] == 0 and st[pl]["gathered"] == 32 and st[pl].get("none", 0) == 0, (mode, r, b, pl, st[pl])


def test_tile_states_nan_third_of_the_map():
    w, h, dw, dh = 128, 72, 130, 70
    for mode in (1, 2):
        mx, my = shape_maps(w, h, dw, dh, mode, ROTS[3])
        nan = np.isnan(mx)
        assert 0.3 < nan.mean() < 0.4 and np.array_equal(nan, np.isnan(my))
        tiles = [nan[y:y + 16, x:x + 64] for y in range(0, dh, 16) for x in range(0, dw, 64)]
        mixed, all_nan = sum(bool(t.any() and not t.all()) for t in tiles), sum(bool(t.all()) for t in tiles)
        assert mixed > 0 and all_nan > 0
        for r, b in KERNELS:
            st = wt.tile_states(mx, my, w, h, r, wt.kernel_rule(r, b))
            for pl in PLANES:
                s = st[pl]
                if b == wd.CONSTANT:       # a NaN entry quantises to (-32768, -32768): it touches nothing and stays out of the box
                    assert s["gathered"] == 0 and s["none"] > 0 and s["staged"] > 0, (mode, r, pl, s)
                else:                       # every footprint counts: the box of a tile that holds a NaN entry beside a number reaches -32768
                    assert s["gathered"] > 0 and s["staged"] > 0, (mode, r, pl, s)
            if b != wd.CONSTANT:           # (a tile of NaN entries alone has a small box at -32768: staged, wholly outside)
                assert st["bgr"]["gathered"] == mixed and st["bgr"]["outside_staged"] == all_nan, (mode, r, st["bgr"])


# ---------------------------------------------------------------------------------------------------------------------
# golden vectors
# ---------------------------------------------------------------------------------------------------------------------
def golden_cases():
    kat = np.load(os.path.join(GOLD, "distort_resample_kat.npz"))
    k = 0
    while f"case{k}_src" in kat.files:
        yield k, {key[len(f"case{k}_"):]: kat[key] for key in kat.files if key.startswith(f"case{k}_")}
        k += 1


def test_golden_file_reproduces_from_the_definition():
    sys.path.insert(0, GOLD)
    import make_distort_resample_golden as gen
    kat = np.load(os.path.join(GOLD, "distort_resample_kat.npz"))
    fresh = gen.build()
    assert sorted(kat.files) == sorted(fresh)
    for key in kat.files:
        assert np.array_equal(kat[key], fresh[key]) and kat[key].dtype == fresh[key].dtype, key
    cases = list(golden_cases())
    assert len(cases) == len(gen.CASES) == 5
    assert {int(c["mode"]) for _, c in cases} == {1, 2}
    fam = {("border" if int(c["resample"]) == 0 else "constant" if int(c["border"]) == 0 else "resample_border") for _, c in cases}
    assert fam == {"border", "constant", "resample_border"}                     # each kernel family appears
    assert {int(c["resample"]) for _, c in cases} == {0, 2, 4}
    for _, c in cases:
        assert c["src"].shape[1] <= 64 and c["src"].shape[0] * 2 // 3 <= 36
        assert (c["bgr"] != 0).mean() > 0.1 and c["luma"].shape == c["bgr"].shape[:2]


# ---------------------------------------------------------------------------------------------------------------------
# the new kernels' resources
# ---------------------------------------------------------------------------------------------------------------------
def test_new_kernels_have_no_larger_private_segment_than_their_siblings(tmp_path):
    """The 44 MAP_FISHD_* instantiations of the resamplers' tile kernels (map modes 9 / 10 of the kernel templates) against the kernel of
    map mode 1 / 2 with the same remaining template arguments, from the kernel metadata of the library as built."""
    lib = shutil.copy(os.path.join(ROOT, "video-annotator_amd", "lib", "libvstab.so"), tmp_path / "libvstab.so")
    subprocess.run(["/opt/rocm/llvm/bin/llvm-objdump", "--offloading", str(lib)], check=True, capture_output=True)     # code objects beside the copy
    sizes = {}
    for obj in sorted(tmp_path.glob("libvstab.so.*gfx950")):
        notes = subprocess.run(["/opt/rocm/llvm/bin/llvm-readelf", "--notes", str(obj)], check=True, capture_output=True, text=True).stdout
        for block in notes.split("- .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", block).group(1)
            sizes[name] = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1))
    new = [n for n in sizes if re.match(r"_ZN5vstab\d+k_warp_(cubic|lanczos4|border|cubic_border|lanczos4_border)ILi(9|10)E", n)]
    count = {}
    for n in new:
        fam = re.match(r"_ZN5vstab\d+(k_warp_\w+?)ILi", n).group(1)
        count[fam] = count.get(fam, 0) + 1
        sibling = n.replace("ILi9E", "ILi1E", 1).replace("ILi10E", "ILi2E", 1)
        assert sibling in sizes and sibling != n, n
        assert sizes[n] <= sizes[sibling], (n, sizes[n], sizes[sibling])
    assert count == {"k_warp_cubic": 4, "k_warp_lanczos4": 4, "k_warp_cubic_border": 12, "k_warp_lanczos4_border": 12, "k_warp_border": 12}, count
