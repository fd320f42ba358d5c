"""CPU half of the Harris tests: the restatement (tests/corner_def.py with harris=True) pinned to the oracle where the two responses share their sums,
closed-form values of the response, the tile states the GPU test's frames reach under it, rule 4 with and without a mask, the clips the
GPU test needs, and the refusals that need no device."""
import ctypes
import importlib

import numpy as np
import pytest

import corner_tiles as C
import corner_def as H
import mask_def as M
import oracle
import synth


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", ["luma_7", "timing", "grid_5x3", "cut_65x32"])
def test_shared_sums_give_the_oracles_eigenvalues(name):
    """a, b, c through the minimum-eigenvalue formula are oracle.min_eig bit for bit: only the Harris formula is new"""
    g = synth.luma(7, 320, 124) if name == "luma_7" else C.timing_frame() if name == "timing" else C.make(name)
    assert np.array_equal(bits(H.min_eig_from_sums(*H.covariance_sums(g))), bits(oracle.min_eig(g)))


def test_closed_forms_of_the_response():
    flat = np.full((40, 70), 93, np.uint8)
    assert not bits(H.corner_harris(flat)).any()                            # +0 everywhere
    assert len(H.good_features(flat, harris=True)) == 0
    step = np.full((40, 70), 30, np.uint8)
    step[:, 35:] = 200
    a, b, c = H.covariance_sums(step)
    assert not b.any() and not c.any() and a.max() > 0
    for k in (0.04, 0.06, 0.2):
        kf = np.float32(k)
        assert np.array_equal(bits(H.response_from_sums(a, b, c, k)), bits(np.float32(0) - (kf * a) * a))   # R = -kf a a exactly
        assert H.corner_harris(step, k=k).max() == 0 and len(H.good_features(step, harris=True, k=k)) == 0                   # an edge is no corner
    g = synth.luma(7, 320, 124)
    a, b, c = H.covariance_sums(g)
    assert np.array_equal(bits(H.response_from_sums(a, b, c, 0.0)), bits(a * c - b * b))                      # k = 0: the determinant
    for k in (-0.01, 0.25, 1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            H.corner_harris(g, k=k)


def test_states_the_raw_frames_reach():
    """what test_harris_gpu.py's raw frames put the one-pass detector into (k = 0.04, quality = 0.01)"""
    for n in (255, 256, 257, 258):                                          # both sides of the slot count, in one tile
        m = H.raw_model(f"tile_{n}", harris=True)
        assert m.lo.shape == (1, 1) and (int(m.lo[0, 0]), int(m.hi[0, 0]), m.n) == (n, n, n) and m.positive
        assert bool(m.spills[0, 0]) == (n > C.SLOTS) and bool(m.full[0, 0]) == (n == C.SLOTS)
    m = H.raw_model("grid_5x3", harris=True)
    assert (int(m.spills.sum()), int(m.keyed.sum()), int(m.timing.sum())) == (12, 3, 0)
    for name in ("cut_65x32", "cut_66x33"):
        m = H.raw_model(name, harris=True)
        assert int(m.spills.sum()) == 1 and bool(m.spills[0, 0]) and int(m.timing.sum()) == 0
    m = H.raw_model("timing", harris=True)
    assert (int(m.timing.sum()), int(m.keyed.sum()), int(m.spills.sum())) == (5, 15, 0) and m.n > 0
    # a tile whose own maximum is negative beside positive ones: it filters with -inf, and hi is every 3 x 3 maximum it holds
    for name in ("ramp_2", "stripes_diagonal"):
        m = H.raw_model(name, harris=True)
        assert m.positive and m.n > 0 and m.negative.any() and not m.negative.all() and m.timing.any(), name
        is_max = H._is_max(m.eig)
        for ty, tx in zip(*np.nonzero(m.negative)):
            assert m.lo[ty, tx] == 0 and m.hi[ty, tx] == int(is_max[ty * C.TH:(ty + 1) * C.TH, tx * C.TW:(tx + 1) * C.TW].sum()) > C.SLOTS, name
    for name in H.NON_POSITIVE:                                             # rule 4: ordinary inputs, no corner
        m = H.raw_model(name, harris=True)
        assert m.frame_max < 0 and not m.positive and m.n == 0 and m.negative.all() and not m.final.any(), name
        assert (m.hi > C.SLOTS).any(), name                                 # and tiles that hand over dense maps all the same
        assert len(H.good_features(m.img, None, 0, 0.01, 0.0, harris=True)) == 0
    m = H.raw_model("luma_322x182", harris=True)
    assert m.keyed.all() and 100 <= m.n <= 200 and 0.45 < float((m.eig < 0).mean()) < 0.6
    for name in H.RAW_FRAMES:
        m = H.raw_model(name, harris=True)
        assert not m.early.any() and (m.lo <= m.hi).all() and int(m.lo.sum()) == m.n, name


def test_the_int_order_keeps_the_sign_of_the_maximum():
    """the kernels' maximum (bits read as int32) is wrong among negative values and right about the sign"""
    for name in ("stripes_vertical", "ramp_2", "luma_322x182"):
        e = H.raw_model(name, harris=True).eig
        imax = np.int32(e.view(np.int32).max()).view(np.float32)
        assert (imax >= 0) == (e.max() >= 0), name
        if e.max() >= 0:
            assert imax == e.max()
    e = H.raw_model("stripes_vertical", harris=True).eig
    assert np.int32(e.view(np.int32).max()).view(np.float32) == e.min() < e.max() < 0       # among negatives the int order is the reverse


def test_rule_4_under_a_mask():
    g, mask = H.rule4_masked_frame()
    e = H.corner_harris(g)
    assert e[mask != 0].max() <= 0 < e[mask == 0].max()
    assert len(H.good_features(g, mask, 0, 0.01, 0.0, harris=True)) == 0 and len(H.good_features(g, None, 0, 0.01, 0.0, harris=True)) > 0
    m = H.rule4_masked_model()
    assert not m.positive and m.n == 0 and (m.hi > C.SLOTS).any() and not m.early.all()
    # and masks as the detector knows them: an all-zero mask has no corner, a full one changes nothing
    g = synth.luma(7, 320, 124)
    assert len(H.good_features(g, np.zeros(g.shape, np.uint8), harris=True)) == 0
    assert np.array_equal(H.good_features(g, M.full(*g.shape, 3), harris=True), H.good_features(g, harris=True))
    assert not np.array_equal(H.good_features(g, M.overlay_box(*g.shape), 0, 0.01, 0.0, harris=True), H.good_features(g, None, 0, 0.01, 0.0, harris=True))


def test_k_separates_and_both_separate_from_the_minimum_eigenvalue():
    g = np.ascontiguousarray(M.overlay_clip(n=1)[1][0][:360])
    a, b, c = H.good_features(g, harris=True, k=0.04), H.good_features(g, harris=True, k=0.15), oracle.good_features(g)
    print(len(a), len(b), len(c))
    assert min(len(a), len(b), len(c)) >= 40
    assert not np.array_equal(a, b) and not np.array_equal(a, c) and not np.array_equal(b, c)


def test_fall_back_frame_is_over_the_key_capacity():
    _, cand, maxv = H.candidates(H.fall_back_frame(), harris=True)
    assert maxv > 0 and int(cand.sum()) > C.KEY_CAP


def test_planned_key_clip_under_harris():
    (w, h), frames = C.pipeline_clip("under_spec_cap")
    K = oracle.get_preset_camera(4, w, h)
    sm, _, counts, _ = M.run_state_machine(frames, K, w, h, 2, 1, lambda g: H.good_features(g, harris=True))
    assert [k for k, lg in enumerate(sm.log) if lg["key"]] == [20]
    assert counts[0][0] == 200 and min(min(c) for c in counts) >= 150
    assert len(H.good_features(frames[0][:h], None, 0, 0.01, 0.0, harris=True)) <= C.SPEC_CAP


def test_refusals_without_a_device():
    """the message order of the two stateless entry points, pinned by breaking two checks at once, and of the hook"""
    vs = importlib.import_module("video-annotator_amd")
    L, c = vs.lib, ctypes
    xy, n, used = np.zeros(16, np.float32), c.c_int(), c.c_int()
    fp = xy.ctypes.data_as(c.POINTER(c.c_float))

    def gfh(gray=4096, pitch=640, w=640, h=360, mask=8192, pm=640, mc=4, k=0.04, det=0, xyp=fp, cnt=None):
        st = L.vstab_good_features_harris(gray, pitch, w, h, mask, pm, mc, 0.01, 3.0, k, det, xyp, c.byref(n) if cnt is None else cnt, c.byref(used), None)
        return st, L.vstab_last_error().decode()

    name = "vstab_good_features_harris: "
    bad, bad_k = name + "bad argument", name + "k lies in [0, 0.25)"
    for kw in (dict(gray=None), dict(xyp=None), dict(cnt=c.POINTER(c.c_int)()), dict(w=2), dict(h=2), dict(pitch=639), dict(mc=0), dict(det=3), dict(det=-1)):
        assert gfh(**kw) == (vs.ERR_INVALID, bad), kw
    assert gfh(pm=639) == (vs.ERR_INVALID, name + "the mask's pitch is smaller than the image's width")
    assert gfh(pm=1 << 24, h=256) == (vs.ERR_INVALID, name + "mask planes of 4 GiB or more are not supported")
    for k in (0.25, 0.5, -1e-12, float("nan"), float("inf"), -float("inf")):
        assert gfh(k=k) == (vs.ERR_INVALID, bad_k), k
        assert gfh(k=k, mask=None, pm=0) == (vs.ERR_INVALID, bad_k), k
    # the order: vstab_good_features_ex's arguments, the mask's pitch, its size, then k
    assert gfh(w=2, pm=1, k=1.0) == (vs.ERR_INVALID, bad)
    assert gfh(pm=639, h=1 << 23, k=1.0)[1].endswith("smaller than the image's width")
    assert gfh(pm=1 << 24, h=256, k=1.0)[1].endswith("4 GiB or more are not supported")
    assert gfh(det=7, k=1.0) == (vs.ERR_INVALID, bad)

    def dense(gray=4096, pitch=640, w=640, h=360, k=0.04, out=8192):
        return L.vstab_corner_harris(gray, pitch, w, h, k, out, None), L.vstab_last_error().decode()

    for kw in (dict(gray=None), dict(out=None), dict(w=0), dict(h=0), dict(pitch=639), dict(gray=None, k=1.0), dict(pitch=1, k=float("nan"))):
        assert dense(**kw) == (vs.ERR_INVALID, "vstab_corner_harris: bad argument"), kw
    for k in (0.25, -0.04, float("nan")):
        assert dense(k=k) == (vs.ERR_INVALID, "vstab_corner_harris: k lies in [0, 0.25)"), k

    class Fake:   # a "device" plane: only its pointer and pitch reach the library, which refuses before using them
        def __init__(self, ptr, pitch, shape):
            self.ptr, self.pitch, self.shape = ptr, pitch, shape

        def data_ptr(self):
            return self.ptr

        def stride(self, d):
            return self.pitch

    def hook(msg, gray=None, mask=None, **kw):
        with pytest.raises(vs.VstabError) as e:
            vs.corners_fused_harris(Fake(4096, 640, (360, 640)) if gray is None else gray, mask, stream=c.c_void_p(), **kw)
        assert e.value.status == vs.ERR_INVALID and str(e.value).endswith("vstabx_corners_fused_harris: " + msg), str(e.value)

    hook("bad argument", gray=Fake(0, 640, (360, 640)))
    hook("an image is at least 3 x 3 and its pitch at least its width", w=2)
    hook("quality lies in (0, 1]", quality=0.0, k=0.3)
    hook("cap is 1 .. 2^24 keys", cap=0, k=0.3)
    hook("the mask's pitch is smaller than the image's width", mask=Fake(8192, 639, (360, 640)), k=0.3)
    hook("k lies in [0, 0.25)", k=0.25)
    hook("k lies in [0, 0.25)", mask=Fake(8192, 640, (360, 640)), k=float("nan"))
    assert L.vstab_set_corner_response(None, 1, 0.04) == vs.ERR_INVALID
    assert L.vstab_last_error().decode() == "vstab_set_corner_response: null handle"


def test_header_declares_what_the_library_and_the_binding_have():
    import test_abi_cpu as A
    vs = importlib.import_module("video-annotator_amd")
    names = A.declared_symbols()
    assert {"vstab_corner_harris", "vstab_good_features_harris", "vstab_set_corner_response"} <= set(names)
    A.test_library_exports_every_declared_symbol(vs)
    assert hasattr(ctypes.CDLL(vs.LIB_PATH), "vstabx_corners_fused_harris")
    assert (vs.CORNER_MIN_EIGENVAL, vs.CORNER_HARRIS) == (0, 1)
