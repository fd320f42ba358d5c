"""CPU half of the corner-block tests (include/vstab.h, "Corner block size"): the definition tests/corner_def.py at block 3 against the
recorded answers of the definitions it replaced and the oracle, at blocks 5 and 7 against its golden file, the exactness of its double sums, what the frames of the GPU test reach at each block
size, and every refusal that needs no device, in order, with its message."""
import ctypes
import importlib
import os

import numpy as np
import pytest

import corner_def as D
import corner_tiles as C
import mask_def as M
import oracle

NEW = (5, 7)
MEASURED = ("luma_322x182", "tile_257", "cut_66x33", "ramp_2", "stripes_diagonal", "timing")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def definitions_kat():
    """(make_definitions_golden, its file): the answers of the definitions there were before tests/corner_def.py"""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_definitions_golden as G
    return G, G.load()


# ---- the definition -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MEASURED)
def test_block_3_is_the_definition_there_was(name):
    """against the oracle on the whole frame; against what harris_def and mask_def answered (golden/definitions_kat.npz) on the frame CROPPED
    to its top-left 40 x 24 pixels -- the planes of the whole frames would not fit a fixture"""
    g = D.frame(name)
    assert np.array_equal(bits(D.min_eig(g, 3)), bits(oracle.min_eig(g)))
    assert np.array_equal(D.good_features(g), oracle.good_features(g))
    G, kat = definitions_kat()
    g = G.crop(g, "block3")
    assert g.shape == (24, 40)
    for p, mine in zip("abc", D.covariance_sums(g, 3)):
        assert np.array_equal(bits(mine), bits(kat[f"block3_{name}_{p}"])), p
    assert np.array_equal(bits(D.corner_harris(g, 3, 3, 0.06)), bits(kat[f"block3_{name}_harris"]))
    assert np.array_equal(bits(D.good_features(g, None, *G.PARAMS, harris=True)), bits(kat[f"block3_{name}_corners_harris"]))
    assert np.array_equal(bits(D.good_features(g, M.overlay_box(*g.shape), *G.PARAMS)), bits(kat[f"block3_{name}_corners_masked"]))


def test_golden_file():
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_corner_block_golden as G
    kat = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "corner_block_kat.npz"))
    n = 0
    for name, g in G.frames().items():
        assert np.array_equal(kat[name + "_gray"], g)
        for block in NEW:
            for k, v in G.answers(g, block).items():
                want = kat[f"{name}_b{block}_{k}"]
                assert want.dtype == v.dtype and want.shape == v.shape and np.array_equal(bits(want), bits(v)), (name, block, k)
                n += 1
    assert n == len(kat.files) - len(G.frames()) == 40
    assert len(kat["luma_40x24_b5_corners"]) > 5 and len(kat["luma_40x24_b7_corners_masked"]) > 2


def test_reflection_folds_as_often_as_it_takes():
    assert D.reflect_index(np.arange(-7, 10), 3).tolist() == [1, 2, 1, 0, 1, 2, 1, 0, 1, 2, 1, 0, 1, 2, 1, 0, 1]
    assert D.reflect_index(np.arange(-3, 4), 1).tolist() == [0] * 7
    g = np.array([[7], [9], [200]], np.uint8)                  # a 1-pixel axis repeats its pixel: no derivative along it
    a, b, c = D.covariance_sums(g, 7)
    assert not a.any() and not b.any() and c.any()


@pytest.mark.parametrize("block", NEW)
def test_sums_are_exact_on_the_frames_of_the_gpu_test(block):
    names = sorted(set(D.STATELESS_FRAMES) | set(D.RAW_FRAMES) | set(MEASURED))
    for name in names:
        assert D.sums_exact(D.frame(name), block) == (True, 0), name
    for name, g in D.dense_frames(block).items():
        if name != "dark_noise":
            assert D.sums_exact(g, block) == (True, 0), name
    assert D.sums_exact(D.textured_frame(), block) == (True, 0)


def test_sums_are_not_exact_on_dark_noise():
    """seed 3 of the recipe, under the defined order: block 3 is exact, 5 and 7 are not"""
    g = D.dark_noise(3)
    assert D.sums_exact(g, 3) == (True, 0)
    counts = {b: D.sums_exact(g, b) for b in NEW}
    print("inexact double sums on the dark-noise frame:", counts)
    for b in NEW:
        ok, n = counts[b]
        assert not ok and n > 0


# ---- what the frames of the GPU test reach -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", NEW)
def test_states_of_the_raw_frames(block):
    for harris, names in ((False, D.RAW_FRAMES_MIN_EIG), (True, D.RAW_FRAMES)):
        models = {n: D.raw_model(n, block, 3, harris) for n in names}
        assert any(m.spills.any() for m in models.values()), "no tile that always spills"
        assert any(m.timing.any() for m in models.values()), "no tile that spills by timing"
        assert any(m.positive and m.lo.any() and m.keyed.any() for m in models.values())
        if harris:
            assert any(m.negative.any() and m.positive for m in models.values()), "no tile with a negative maximum in a frame with corners"
            for n in D.NON_POSITIVE:
                assert not models[n].positive and models[n].negative.all(), n
        else:
            assert all(m.positive for m in models.values())     # the minimum-eigenvalue definition covers every frame it is given
    for harris in (False, True):
        for n in D.RAW_MASKED:
            m = D.raw_masked_model(n, block, 3, harris)
            assert m.early.any() and m.positive and m.n > 0 and not m.final[m.mask == 0].any(), n
        assert any(D.raw_masked_model(n, block, 3, harris).timing.any() or D.raw_masked_model(n, block, 3, harris).spills.any() for n in D.RAW_MASKED)
    r4 = D.rule4_masked_model(block)
    assert not r4.positive and r4.frame_max < 0 and r4.early.any()
    assert len(D.good_features(r4.img, None, 4000, 0.01, 0.0, block, 3, True)) > 0


@pytest.mark.parametrize("block", NEW)
def test_fall_back_frame_is_over_the_key_capacity(block):
    """the 2-px checkerboard at 640 x 512 keeps its plateau under a 5 x 5 and a 7 x 7 box"""
    for harris in (False, True):
        _, cand, maxv = D.candidates(D.fall_back_frame(), None, 0.01, block, 3, harris)
        assert maxv > 0 and int(cand.sum()) > C.KEY_CAP


def test_block_sizes_separate():
    g = D.textured_frame()
    a, b, c = (D.good_features(g, block=blk) for blk in D.BLOCKS)
    assert min(len(a), len(b), len(c)) >= 40
    assert not np.array_equal(a, b) and not np.array_equal(a, c) and not np.array_equal(b, c)
    for blk in (1, 2, 4, 6, 8, 9, 0, -3):
        with pytest.raises(ValueError):
            D.min_eig(g, blk)


def test_interior_edge_sizes():
    """tile (1, 1) of the edge frames has its source box end on the image's last column and row"""
    assert D.interior_edge_size(5) == (132, 66) and D.interior_edge_size(7) == (136, 67)
    for block in NEW:
        w, h = D.interior_edge_size(block)
        assert w % 4 == 0 and w > 64 + 4 and h > 31                       # dword-aligned rows; tile (1, 1) exists
        fr = D.dense_frames(block)
        assert fr["interior_edge"].shape == (h, w) and fr["interior_edge_less_w"].shape == (h, w - 1) and fr["interior_edge_less_h"].shape == (h - 1, w)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
BAD_BLOCKS = (0, 1, 2, 4, 6, 8, 9, 11, -3)


def test_refusals_without_a_device():
    vs = importlib.import_module("video-annotator_amd")
    L, c = vs.lib, ctypes
    xy, n, used = np.zeros(16, np.float32), c.c_int(), c.c_int()
    fp = xy.ctypes.data_as(c.POINTER(c.c_float))

    def gfb(gray=4096, pitch=640, w=640, h=360, mask=8192, pm=640, mc=4, q=0.01, md=3.0, block=5, harris=1, k=0.04, det=0, xyp=fp, cnt=None):
        st = L.vstab_good_features_block(gray, pitch, w, h, mask, pm, mc, q, md, block, harris, k, det, xyp, c.byref(n) if cnt is None else cnt, c.byref(used), None)
        return st, L.vstab_last_error().decode()

    name = "vstab_good_features_block: "
    bad, bad_block = (vs.ERR_INVALID, name + "bad argument"), (vs.ERR_INVALID, name + "block_size is 3, 5 or 7")
    for kw in (dict(gray=None), dict(xyp=None), dict(cnt=c.POINTER(c.c_int)()), dict(w=2), dict(h=2), dict(pitch=639), dict(mc=0), dict(det=3), dict(det=-1),
               dict(harris=2), dict(harris=-1)):
        assert gfb(**kw) == bad, kw
    for blk in BAD_BLOCKS:
        assert gfb(block=blk) == bad_block, blk
        assert gfb(block=blk, mask=None, pm=0, harris=0) == bad_block, blk
    assert gfb(q=0.0) == (vs.ERR_INVALID, name + "quality must be > 0 and min_distance >= 0")
    assert gfb(md=-1.0) == (vs.ERR_INVALID, name + "quality must be > 0 and min_distance >= 0")
    assert gfb(pm=639) == (vs.ERR_INVALID, name + "the mask's pitch is smaller than the image's width")
    assert gfb(pm=1 << 24, h=256) == (vs.ERR_INVALID, name + "mask planes of 4 GiB or more are not supported")
    for k in (0.25, -1e-12, float("nan"), float("inf")):
        assert gfb(k=k) == (vs.ERR_INVALID, name + "k lies in [0, 0.25)"), k
    # the order, two broken arguments at once: bad argument, block, quality and min_distance, the mask's pitch, its size, k
    assert gfb(harris=2, block=4) == bad and gfb(w=2, block=9) == bad and gfb(det=7, q=0.0) == bad
    assert gfb(block=4, q=0.0) == bad_block and gfb(block=6, pm=1) == bad_block and gfb(block=1, k=1.0) == bad_block
    assert gfb(q=float("nan"), pm=1)[1].endswith("min_distance >= 0") and gfb(md=float("nan"), k=1.0)[1].endswith("min_distance >= 0")
    assert gfb(pm=639, h=1 << 23, k=1.0)[1].endswith("smaller than the image's width")
    assert gfb(pm=1 << 24, h=256, k=1.0)[1].endswith("4 GiB or more are not supported")

    def dense(fn, gray=4096, pitch=640, w=640, h=360, block=5, k=0.04, out=8192):
        args = (gray, pitch, w, h, block) + ((k,) if fn == "vstab_corner_harris_block" else ()) + (out, None)
        return getattr(L, fn)(*args), L.vstab_last_error().decode()

    for fn in ("vstab_min_eig_block", "vstab_corner_harris_block"):
        for kw in (dict(gray=None), dict(out=None), dict(w=0), dict(h=0), dict(pitch=639), dict(gray=None, block=4), dict(pitch=1, block=9, k=1.0)):
            assert dense(fn, **kw) == (vs.ERR_INVALID, fn + ": bad argument"), (fn, kw)
        for blk in BAD_BLOCKS:
            assert dense(fn, block=blk) == (vs.ERR_INVALID, fn + ": block_size is 3, 5 or 7"), (fn, blk)
        assert dense(fn, block=4, k=1.0) == (vs.ERR_INVALID, fn + ": block_size is 3, 5 or 7")
    for k in (0.25, -0.04, float("nan")):
        for blk in D.BLOCKS:
            assert dense("vstab_corner_harris_block", block=blk, k=k) == (vs.ERR_INVALID, "vstab_corner_harris_block: k lies in [0, 0.25)"), k

    for blk in (5, 4):
        assert L.vstab_set_corner_block(None, blk) == vs.ERR_INVALID
        assert L.vstab_last_error().decode() == "vstab_set_corner_block: null handle"

    class Fake:   # a "device" plane: only its pointer and pitch reach the library, which refuses before using them
        def __init__(self, ptr, pitch, shape):
            self.ptr, self.pitch, self.shape = ptr, pitch, shape

        def data_ptr(self):
            return self.ptr

        def stride(self, d):
            return self.pitch

    def hook(msg, gray=None, mask=None, **kw):
        with pytest.raises(vs.VstabError) as e:
            vs.corners_fused_block(Fake(4096, 640, (360, 640)) if gray is None else gray, mask, stream=c.c_void_p(), **kw)
        assert e.value.status == vs.ERR_INVALID and str(e.value).endswith("vstabx_corners_fused_block: " + msg), str(e.value)

    hook("response is 0 or 1", response=2, block_size=4)
    hook("bad argument", gray=Fake(0, 640, (360, 640)), block_size=4)
    hook("an image is at least 3 x 3 and its pitch at least its width", w=2, block_size=5)
    hook("quality lies in (0, 1]", quality=0.0, block_size=4)
    hook("cap is 1 .. 2^24 keys", cap=0, block_size=4)
    for blk in BAD_BLOCKS:
        hook("block_size is 3, 5 or 7", block_size=blk)
    hook("block_size is 3, 5 or 7", block_size=4, mask=Fake(8192, 639, (360, 640)), response=vs.CORNER_HARRIS, k=0.3)
    hook("the mask's pitch is smaller than the image's width", mask=Fake(8192, 639, (360, 640)), block_size=7, response=vs.CORNER_HARRIS, k=0.3)
    hook("k lies in [0, 0.25)", block_size=7, response=vs.CORNER_HARRIS, k=0.25)


def test_header_declares_what_the_library_and_the_binding_have():
    import test_abi_cpu as A
    vs = importlib.import_module("video-annotator_amd")
    names = A.declared_symbols()
    new = {"vstab_min_eig_block", "vstab_corner_harris_block", "vstab_good_features_block", "vstab_set_corner_block"}
    assert new <= set(names) and new <= set(vs.SIGNATURES)
    A.test_library_exports_every_declared_symbol(vs)
    assert hasattr(ctypes.CDLL(vs.LIB_PATH), "vstabx_corners_fused_block")
    assert all(callable(f) for f in (vs.min_eig_block, vs.corner_harris_block, vs.good_features_block, vs.corners_fused_block, vs.Stabilizer.set_corner_block))
    assert vs.lib.vstab_abi_version() == vs.ABI_VERSION == 0x56534206                    # no struct changed: the version the tracker window left
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "vstab.h")).read()
    assert "Corner block size" in header and "blockSize and gradientSize" not in header and "blockSize other than" not in header
