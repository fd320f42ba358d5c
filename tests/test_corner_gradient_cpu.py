"""CPU half of the corner-gradient tests (include/vstab.h, "Corner gradient size"): the definition tests/corner_def.py at gradient 3 against the
recorded answers of the definition it replaced, at gradients 5 and 7 against its golden file, its coefficients, the inexact double sums that bind the box order for block 3, and every
refusal that needs no device, in order, with its message."""
import ctypes
import importlib
import os

import numpy as np
import pytest

import corner_def as D

BAD_GRADIENTS = (-1, 0, 1, 2, 4, 6, 8, 9, 11, -3)
BAD_BLOCKS = (0, 1, 2, 4, 6, 8, 9, 11, -3)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def definitions_kat():
    """(make_definitions_golden, its file): the answers of the definitions there were before tests/corner_def.py"""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_definitions_golden as G
    return G, G.load()


# ---- the definition -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", D.BLOCKS)
def test_gradient_3_is_the_definition_there_was(block):
    """every dense frame of both block sizes' GPU tests (ten names, the interior-edge ones at both sizes), and the named frames, against what
    corner_block_def answered (golden/definitions_kat.npz).  The frames are CROPPED to their top-left corner, 20 x 13 pixels for the products
    and 66 x 33 for the responses ("3x3" and "4x5" stay whole): the planes of the whole frames would not fit a fixture"""
    G, kat = definitions_kat()
    frames = G.product_frames()
    assert len(frames) == 23 and all(g.shape == (min(13, g.shape[0]), min(20, g.shape[1])) for g in frames.values())
    for name, g in frames.items():
        for p, mine in zip(G.PLANES, D.products(g, block, 3)):
            assert np.array_equal(bits(mine), bits(kat[f"products_{name}_B{block}_{p}"])), (name, p)
    g = G.crop(D.frame("luma_322x182"), "response")
    assert g.shape == (33, 66)
    assert np.array_equal(bits(D.min_eig(g, block, 3)), bits(kat[f"response_B{block}_min_eig"]))
    assert np.array_equal(bits(D.corner_harris(g, block, 3, 0.06)), bits(kat[f"response_B{block}_harris"]))
    assert np.array_equal(bits(D.good_features(g, None, *G.PARAMS, block=block, gradient=3)), bits(kat[f"response_B{block}_corners"]))


def test_row_differences_are_whole_and_coefficients_are_the_stated_casts():
    g = D.dark_noise()
    g[0, :] = 255                                                     # the largest differences there are
    g[1, ::2] = 0
    for G, bound in ((3, 255), (5, 4 * 255), (7, 10 * 255)):
        d = D.row_differences(g, G)
        assert d.dtype == np.int32 and int(np.abs(d).max()) <= bound <= 2550
        assert np.array_equal(d.astype(np.float32).astype(np.int32), d)           # exact as floats
        for blk in D.BLOCKS:
            k = D.coefficients(blk, G)
            sigma = 1.0 / (float(1 << (G - 1)) * blk * 255.0)
            assert len(k) == (G + 1) // 2 and all(x.dtype == np.float32 for x in k)
            assert [x.tobytes() for x in k] == [np.float32(float(s) * sigma).tobytes() for s in D.SMOOTH[G]]
    for blk in D.BLOCKS:                                              # G = 3: the k1 = scale_B, k0 = 2.0f * scale_B of the block definition
        scale = np.float32(1.0 / (4.0 * blk * 255.0))
        assert D.coefficients(blk, 3) == (np.float32(2.0) * scale, scale)
    assert D.SMOOTH == {3: (2, 1), 5: (6, 4, 1), 7: (20, 15, 6, 1)} and D.DERIV == {3: (0, 1), 5: (0, 2, 1), 7: (0, 5, 4, 1)}
    for G in D.GRADIENTS:                                             # the Sobel pair of aperture G: binomial smoothing, its difference
        full = D.SMOOTH[G][:0:-1] + D.SMOOTH[G]
        assert sum(full) == 1 << (G - 1)


def test_a_constant_axis_has_no_derivative():
    g = np.array([[7], [9], [200], [3], [90]], np.uint8)             # a 1-pixel axis repeats its pixel
    for G in D.GRADIENTS:
        a, b, c = D.covariance_sums(g, 3, G)
        assert not a.any() and not b.any() and c.any()


def test_golden_file():
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_corner_gradient_golden as G
    kat = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "corner_gradient_kat.npz"))
    g = G.gray()
    assert g.shape == (33, 66) and np.array_equal(kat["gray"], g)
    n = 0
    for block, gradient in D.NEW_PAIRS:
        for k, v in G.answers(g, block, gradient).items():
            want = kat[f"b{block}_g{gradient}_{k}"]
            assert want.dtype == v.dtype and want.shape == v.shape and np.array_equal(bits(want), bits(v)), (block, gradient, k)
            n += 1
    assert n == len(kat.files) - 1 == 12


def test_block_3_sums_are_not_exact_on_dark_noise():
    """why the order of the box sum binds block 3 once G is not 3: seed 3 of the recipe"""
    g = D.dark_noise(3)
    assert D.sums_exact(g, 3, 3) == (True, 0)
    counts = {G: D.sums_exact(g, 3, G) for G in (5, 7)}
    print("inexact block-3 double sums on the dark-noise frame:", counts)
    assert counts == {5: (False, 15), 7: (False, 11)}


def test_gradient_sizes_separate():
    g = D.textured_frame()
    got = {(b, G): D.good_features(g, block=b, gradient=G) for G in D.GRADIENTS for b in (3, 7)}
    assert [len(got[(b, G)]) for G in D.GRADIENTS for b in (3, 7)] == [69, 68, 74, 83, 78, 90]
    keys = list(got)
    for i, a in enumerate(keys):
        for b in keys[i + 1:]:
            assert not np.array_equal(got[a], got[b]), (a, b)
    for G in BAD_GRADIENTS:
        with pytest.raises(ValueError):
            D.min_eig(g, 3, G)


def test_interior_edge_sizes():
    """tile (1, 1) of the edge frames has its source box end on the image's last column and row"""
    want = {(3, 5): (132, 66), (3, 7): (136, 67), (5, 5): (136, 67), (5, 7): (136, 68), (7, 5): (136, 68), (7, 7): (136, 69)}
    assert {p: D.interior_edge_size(*p) for p in D.NEW_PAIRS} == want
    for b in (5, 7):
        assert D.interior_edge_size(b, 3) == D.interior_edge_size(b) and D.source_box(b, 3) == D.INTERIOR_BOX[b]
    for b, G in D.NEW_PAIRS:
        w, h = D.interior_edge_size(b, G)
        assert w % 4 == 0 and w > 64 + 4 and h > 31
        fr = D.dense_frames(b, G)
        assert fr["interior_edge"].shape == (h, w) and fr["interior_edge_less_w"].shape == (h, w - 1) and fr["interior_edge_less_h"].shape == (h - 1, w)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
def test_refusals_without_a_device():
    vs = importlib.import_module("video-annotator_amd")
    L, c = vs.lib, ctypes
    xy, n, used = np.zeros(16, np.float32), c.c_int(), c.c_int()
    fp = xy.ctypes.data_as(c.POINTER(c.c_float))

    def gfg(gray=4096, pitch=640, w=640, h=360, mask=8192, pm=640, mc=4, q=0.01, md=3.0, block=5, grad=5, harris=1, k=0.04, det=0, xyp=fp, cnt=None):
        st = L.vstab_good_features_grad(gray, pitch, w, h, mask, pm, mc, q, md, block, grad, harris, k, det, xyp, c.byref(n) if cnt is None else cnt, c.byref(used), None)
        return st, L.vstab_last_error().decode()

    name = "vstab_good_features_grad: "
    bad, bad_block, bad_grad = (vs.ERR_INVALID, name + "bad argument"), (vs.ERR_INVALID, name + "block_size is 3, 5 or 7"), (vs.ERR_INVALID, name + "gradient_size is 3, 5 or 7")
    for kw in (dict(gray=None), dict(xyp=None), dict(cnt=c.POINTER(c.c_int)()), dict(w=2), dict(h=2), dict(pitch=639), dict(mc=0), dict(det=3), dict(det=-1),
               dict(harris=2), dict(harris=-1)):
        assert gfg(**kw) == bad, kw
    for blk in BAD_BLOCKS:
        assert gfg(block=blk) == bad_block, blk
    for G in BAD_GRADIENTS:
        assert gfg(grad=G) == bad_grad, G
        assert gfg(grad=G, block=3, mask=None, pm=0, harris=0) == bad_grad, G
    assert gfg(q=0.0) == (vs.ERR_INVALID, name + "quality must be > 0 and min_distance >= 0")
    assert gfg(md=-1.0) == (vs.ERR_INVALID, name + "quality must be > 0 and min_distance >= 0")
    assert gfg(pm=639) == (vs.ERR_INVALID, name + "the mask's pitch is smaller than the image's width")
    assert gfg(pm=1 << 24, h=256) == (vs.ERR_INVALID, name + "mask planes of 4 GiB or more are not supported")
    for k in (0.25, -1e-12, float("nan"), float("inf")):
        assert gfg(k=k) == (vs.ERR_INVALID, name + "k lies in [0, 0.25)"), k
    # the order, two broken arguments at once: bad argument, block, gradient, quality and min_distance, the mask's pitch, its size, k
    assert gfg(harris=2, grad=4) == bad and gfg(w=2, grad=9) == bad and gfg(det=7, block=4, grad=4) == bad
    assert gfg(block=4, grad=4) == bad_block and gfg(block=9, grad=-1, q=0.0) == bad_block
    assert gfg(grad=4, q=0.0) == bad_grad and gfg(grad=6, pm=1) == bad_grad and gfg(grad=1, k=1.0) == bad_grad and gfg(grad=-1, md=-1.0) == bad_grad
    assert gfg(q=float("nan"), pm=1)[1].endswith("min_distance >= 0") and gfg(pm=639, k=1.0)[1].endswith("smaller than the image's width")

    def dense(fn, gray=4096, pitch=640, w=640, h=360, block=5, grad=5, k=0.04, out=8192):
        args = (gray, pitch, w, h, block, grad) + ((k,) if fn == "vstab_corner_harris_grad" else ()) + (out, None)
        return getattr(L, fn)(*args), L.vstab_last_error().decode()

    for fn in ("vstab_min_eig_grad", "vstab_corner_harris_grad"):
        for kw in (dict(gray=None), dict(out=None), dict(w=0), dict(h=0), dict(pitch=639), dict(gray=None, grad=4), dict(pitch=1, block=9, grad=9, k=1.0)):
            assert dense(fn, **kw) == (vs.ERR_INVALID, fn + ": bad argument"), (fn, kw)
        for blk in BAD_BLOCKS:
            assert dense(fn, block=blk) == (vs.ERR_INVALID, fn + ": block_size is 3, 5 or 7"), (fn, blk)
            assert dense(fn, block=blk, grad=4) == (vs.ERR_INVALID, fn + ": block_size is 3, 5 or 7"), (fn, blk)
        for G in BAD_GRADIENTS:
            for blk in D.BLOCKS:
                assert dense(fn, block=blk, grad=G, k=1.0) == (vs.ERR_INVALID, fn + ": gradient_size is 3, 5 or 7"), (fn, blk, G)
    for k in (0.25, -0.04, float("nan")):
        for G in D.GRADIENTS:
            assert dense("vstab_corner_harris_grad", grad=G, k=k) == (vs.ERR_INVALID, "vstab_corner_harris_grad: k lies in [0, 0.25)"), k

    for G in (5, 4):
        assert L.vstab_set_corner_gradient(None, G) == vs.ERR_INVALID
        assert L.vstab_last_error().decode() == "vstab_set_corner_gradient: null handle"

    class Fake:   # a "device" plane: only its pointer and pitch reach the library, which refuses before using them
        def __init__(self, ptr, pitch, shape):
            self.ptr, self.pitch, self.shape = ptr, pitch, shape

        def data_ptr(self):
            return self.ptr

        def stride(self, d):
            return self.pitch

    def hook(msg, gray=None, mask=None, **kw):
        with pytest.raises(vs.VstabError) as e:
            vs.corners_fused_grad(Fake(4096, 640, (360, 640)) if gray is None else gray, mask, stream=c.c_void_p(), **kw)
        assert e.value.status == vs.ERR_INVALID and str(e.value).endswith("vstabx_corners_fused_grad: " + msg), str(e.value)

    hook("response is 0 or 1", response=2, gradient_size=4)
    hook("bad argument", gray=Fake(0, 640, (360, 640)), gradient_size=4)
    hook("an image is at least 3 x 3 and its pitch at least its width", w=2, gradient_size=4)
    hook("quality lies in (0, 1]", quality=0.0, gradient_size=4)
    hook("cap is 1 .. 2^24 keys", cap=0, gradient_size=4)
    for G in BAD_GRADIENTS:
        hook("gradient_size is 3, 5 or 7", gradient_size=G)
        hook("gradient_size is 3, 5 or 7", gradient_size=G, block_size=7)
    hook("block_size is 3, 5 or 7", block_size=4, gradient_size=4)
    hook("gradient_size is 3, 5 or 7", gradient_size=4, mask=Fake(8192, 639, (360, 640)), response=vs.CORNER_HARRIS, k=0.3)
    hook("the mask's pitch is smaller than the image's width", mask=Fake(8192, 639, (360, 640)), gradient_size=7, response=vs.CORNER_HARRIS, k=0.3)
    hook("k lies in [0, 0.25)", gradient_size=7, block_size=7, response=vs.CORNER_HARRIS, k=0.25)


def test_header_declares_what_the_library_and_the_binding_have():
    import test_abi_cpu as A
    vs = importlib.import_module("video-annotator_amd")
    names = A.declared_symbols()
    new = {"vstab_min_eig_grad", "vstab_corner_harris_grad", "vstab_good_features_grad", "vstab_set_corner_gradient"}
    assert new <= set(names) and new <= set(vs.SIGNATURES)
    A.test_library_exports_every_declared_symbol(vs)
    assert hasattr(ctypes.CDLL(vs.LIB_PATH), "vstabx_corners_fused_grad")
    assert all(callable(f) for f in (vs.min_eig_grad, vs.corner_harris_grad, vs.good_features_grad, vs.corners_fused_grad, vs.Stabilizer.set_corner_gradient))
    assert vs.lib.vstab_abi_version() == vs.ABI_VERSION == 0x56534206                    # no struct changed
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "vstab.h")).read()
    assert "Corner gradient size" in header
    flat = " ".join(header.replace(" * ", " ").split())
    for gone in ("gradientSize other than 3 is not offered", "gradientSize stays 3", "3 is still not offered for the detector"):
        assert gone not in flat, gone
