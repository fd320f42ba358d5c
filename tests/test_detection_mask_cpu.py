"""CPU half of the detection-mask tests: the definition (tests/corner_def.py under the masks of tests/mask_def.py) against the oracle's detector and against the two wrong
versions it has to separate from, what the masked tile model reaches, the property that motivates the feature on the oracle alone, the
clip the GPU test needs, and the refusals that need no device."""
import ctypes
import importlib

import numpy as np
import pytest

import corner_def as D
import corner_tiles as C
import mask_def as M
import oracle
import synth

PARAMS = ((0, 0.01, 0.0), (200, 0.01, 30.0))


@pytest.mark.parametrize("name", ["luma_1", "luma_7", "luma_23", "timing", "banded_under"])
def test_full_mask_is_the_unmasked_detector(name):
    g = {"timing": C.timing_frame, "banded_under": lambda: C.banded("under")}.get(name, lambda: synth.luma(int(name[5:]), 320, 124))()
    for value in (1, 255):
        for mc, q, md in PARAMS:
            assert np.array_equal(D.good_features(g, M.full(*g.shape, value), mc, q, md), oracle.good_features(g, mc, q, md)), (name, mc)


def test_filtering_afterwards_is_another_detector():
    g, m = M.case_filter_afterwards()
    e = oracle.min_eig(g)
    assert 0.0137 < e[m != 0].max() / e.max() < 0.0139
    assert len(D.good_features(g, m, 0, 0.01, 0.0)) == 5154 and len(D.good_features(g, m, 200, 0.01, 30.0)) == 13
    unmasked = oracle.good_features(g, 0, 0.01, 0.0)
    assert len(unmasked) == 89 and int((m[unmasked[:, 1].astype(int), unmasked[:, 0].astype(int)] != 0).sum()) == 8


def test_masked_out_neighbours_compete():
    g, m = M.case_neighbours_compete()
    assert int((m == 0).sum()) == 156
    e = oracle.min_eig(g)
    assert 0.888 < e[m != 0].max() / e.max() < 0.890
    assert len(D.good_features(g, m, 0, 0.01, 0.0)) == 3


def test_all_zero_mask_has_no_corner():
    g = synth.luma(7, 320, 124)
    assert D.good_features(g, np.zeros(g.shape, np.uint8)).shape == (0, 2)
    m = D.Model(g, np.zeros(g.shape, np.uint8))
    assert m.n == 0 and m.early.all() and not m.lo.any() and not m.hi.any()


def test_masked_model_invariants_and_what_the_gpu_sets_reach():
    states = set()
    for name in M.RAW_SETS:
        m = D.raw_masked_model(name)
        assert (m.lo <= m.hi).all() and int(m.lo.sum()) == m.n, name
        assert not m.lo[m.early].any() and not m.hi[m.early].any(), name
        assert (m.mask == 0).any() and (m.mask != 0).any(), name                       # a mask is in force
        assert m.positive and not m.negative.any(), name                               # no negative masked maximum: inside the definition
        states |= {s for s, a in (("keys", m.keyed & (m.lo > 0)), ("full", m.full), ("spills", m.spills), ("timing", m.timing), ("early", m.early)) if a.any()}
    assert states == {"keys", "full", "spills", "timing", "early"}
    assert all(D.raw_masked_model(n).early.any() and not D.raw_masked_model(n).early.all() for n in ("grid_7x5_tiles_off", "full_16_tiles_off", "timing_top_off", "timing_rows"))
    # whole tiles switched off, with their ring (early) and without it (a count of 0, yet computed)
    m = D.raw_masked_model("grid_5x3_tiles_off")
    assert not m.early.any() and [int(m.hi.ravel()[t]) for t in (0, 4, 7, 11)] == [0, 0, 0, 0] and m.spills.any()
    assert int(D.raw_masked_model("grid_7x5_tiles_off").early.sum()) == 7 and int(D.raw_masked_model("full_16_tiles_off").early.sum()) == 4
    # plateau tiles cut in half still spill; exactly 256 and 257 survivors in what was a plateau tile
    for name in ("mixed_wave_half", "grid_7x5_half"):
        m, whole = D.raw_masked_model(name), C.model(name[:-5])
        plateau = whole.lo > 1000
        assert plateau.any() and m.spills[plateau].all() and (m.lo[plateau] < whole.lo[plateau]).all()
    m = D.raw_masked_model("mixed_wave_256")
    assert (m.lo.ravel()[2], m.hi.ravel()[2]) == (256, 256) and C.model("mixed_wave").spills.ravel()[2]
    m = D.raw_masked_model("grid_5x3_257")
    assert (m.lo.ravel()[2], m.hi.ravel()[2]) == (257, 257)
    assert D.raw_masked_model("timing_top_off").timing.any()


@pytest.fixture(scope="module")
def overlay_runs():
    K, clean, over, rots, mask = M.overlay_clip()
    w, h = 640, 360
    out = {}
    for name, frames, find in (("clean", clean, lambda g: oracle.good_features(np.ascontiguousarray(g))),
                               ("overlay", over, lambda g: oracle.good_features(np.ascontiguousarray(g))),
                               ("masked", over, lambda g: D.good_features(g, mask))):
        sm, _, _, _ = M.run_state_machine(frames, K, w, h, 5, 5, find)
        errs = [oracle.rotation_angle(lg["R"] @ (rots[k] @ rots[k - 1].T).T) for k, lg in enumerate(sm.log, start=1)]
        out[name] = (float(np.median(errs)), float(max(errs)), min(lg["inliers"] for lg in sm.log))
    return out


def test_the_mask_brings_the_rotation_error_back(overlay_runs):
    """an unmoved overlay over 9 % of the frame votes for "the camera did not move"; the mask (the overlay grown by 16 px) removes the vote"""
    print({k: "median %.2e max %.2e min inliers %d" % v for k, v in overlay_runs.items()})
    clean, over, masked = (overlay_runs[k] for k in ("clean", "overlay", "masked"))
    assert masked[0] <= over[0] / 3
    assert masked[0] <= 2 * clean[0]
    assert masked[2] >= 40


def test_planned_key_clip_under_the_mask():
    (w, h), frames, mask = M.planned_key_clip()
    K = oracle.get_preset_camera(4, w, h)
    sm, _, counts, _ = M.run_state_machine(frames, K, w, h, 2, 1, lambda g: D.good_features(g, mask))
    assert [k for k, lg in enumerate(sm.log) if lg["key"]] == [20]
    assert min(min(c) for c in counts) >= 150
    assert len(D.good_features(frames[0][:h], mask, 0, 0.01, 0.0)) <= C.SPEC_CAP


class Fake:   # a "device" plane: only its pointer and pitch reach the library, which refuses before using them
    def __init__(self, ptr, pitch, shape):
        self.ptr, self.pitch, self.shape = ptr, pitch, shape

    def data_ptr(self):
        return self.ptr

    def stride(self, d):
        return self.pitch


def test_refusals_without_a_device():
    vs = importlib.import_module("video-annotator_amd")
    L, c = vs.lib, ctypes
    xy, n, used = np.zeros(16, np.float32), c.c_int(), c.c_int()
    fp = xy.ctypes.data_as(c.POINTER(c.c_float))

    def gfm(gray=4096, pitch=640, w=640, h=360, mask=8192, pm=640, mc=4, det=0, xyp=fp, cnt=None):
        st = L.vstab_good_features_mask(gray, pitch, w, h, mask, pm, mc, 0.01, 3.0, det, xyp, c.byref(n) if cnt is None else cnt, c.byref(used), None)
        return st, L.vstab_last_error().decode()

    bad = "vstab_good_features_mask: bad argument"
    for kw in (dict(gray=None), dict(xyp=None), dict(cnt=c.POINTER(c.c_int)()), dict(w=2), dict(h=2), dict(pitch=639), dict(mc=0), dict(det=3), dict(det=-1)):
        assert gfm(**kw) == (vs.ERR_INVALID, bad), kw
    assert gfm(pm=639) == (vs.ERR_INVALID, "vstab_good_features_mask: the mask's pitch is smaller than the image's width")
    assert gfm(pm=1 << 24, h=256) == (vs.ERR_INVALID, "vstab_good_features_mask: mask planes of 4 GiB or more are not supported")
    # the order: the arguments of vstab_good_features_ex first, then the mask's pitch, then its size; without a mask its pitch is not looked at
    assert gfm(w=2, pm=1) == (vs.ERR_INVALID, bad)
    assert gfm(pm=639, h=1 << 23, pitch=640)[1].endswith("smaller than the image's width")
    assert gfm(gray=None, mask=None, pm=0) == (vs.ERR_INVALID, bad)
    # the unmasked call keeps its name and keeps refusing VSTAB_DETECTOR_FUSED
    assert L.vstab_good_features_ex(4096, 640, 640, 360, 4, 0.01, 3.0, vs.DETECTOR_FUSED, fp, c.byref(n), None, None) == vs.ERR_INVALID
    assert L.vstab_last_error().decode() == "vstab_good_features: bad argument"

    def hook(msg, gray=None, mask=None, **kw):
        with pytest.raises(vs.VstabError) as e:
            vs.corners_fused_mask(Fake(4096, 640, (360, 640)) if gray is None else gray, Fake(8192, 640, (360, 640)) if mask is None else mask,
                                  stream=c.c_void_p(), **kw)
        assert e.value.status == vs.ERR_INVALID and str(e.value).endswith("vstabx_corners_fused_mask: " + msg), str(e.value)

    hook("bad argument", gray=Fake(0, 640, (360, 640)))
    hook("bad argument", mask=Fake(0, 640, (360, 640)))
    size = "an image is at least 3 x 3 and its pitch at least its width"
    hook(size, gray=Fake(4096, 639, (360, 640)))
    hook(size, w=2)
    hook(size, h=-1)
    big = "planes of 4 GiB or more and images of 2^31 pixels or more are not supported"
    hook(big, gray=Fake(4096, 1 << 20, (4096, 640)))
    hook(big, gray=Fake(4096, 1 << 16, (1 << 15, 1 << 16)), mask=Fake(8192, 1 << 16, (1 << 15, 1 << 16)))
    hook("quality lies in (0, 1]", quality=0.0)
    hook("quality lies in (0, 1]", quality=float("nan"))
    hook("cap is 1 .. 2^24 keys", cap=0)
    hook("canary is 1 .. 2^16 keys", canary=(1 << 16) + 1)
    hook("the mask's pitch is smaller than the image's width", mask=Fake(8192, 639, (360, 640)))
    hook("mask planes of 4 GiB or more are not supported", gray=Fake(4096, 640, (4096, 640)), mask=Fake(8192, 1 << 20, (4096, 640)))
    # the order: the image's checks, quality, cap, canary, then the mask's
    hook("cap is 1 .. 2^24 keys", cap=0, mask=Fake(8192, 1, (360, 640)))
    hook("quality lies in (0, 1]", quality=2.0, cap=0, canary=0)
    # the handle's setter: everything but the null handle needs a handle, hence a device (test_detection_mask_gpu.py)
    assert L.vstab_set_detection_mask(None, 4096, 640, vs.MEM_DEVICE if hasattr(vs, "MEM_DEVICE") else 0) == vs.ERR_INVALID
    assert L.vstab_last_error().decode() == "vstab_set_detection_mask: null handle"


def test_header_declares_what_the_library_and_the_binding_have():
    """the symbol test of test_abi_cpu.py with the new declarations in the header"""
    import test_abi_cpu as A
    vs = importlib.import_module("video-annotator_amd")
    names = A.declared_symbols()
    assert "vstab_good_features_mask" in names and "vstab_set_detection_mask" in names
    A.test_library_exports_every_declared_symbol(vs)
    assert hasattr(ctypes.CDLL(vs.LIB_PATH), "vstabx_corners_fused_mask")
