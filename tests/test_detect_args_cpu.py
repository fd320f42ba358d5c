"""The detector's scalar arguments, no device needed.  (1) goodFeaturesToTrack's contract -- quality > 0, min_distance >= 0, NaN fails
either -- as vstab_good_features, _ex, _mask and _harris refuse it: message and order pinned.  (2) The host half of the detector
(select_corners, csrc/vstab_hostlogic.hpp, through vstabx_select_corners) and the oracle's vo_good_features against a brute-force
definition of the minimum-distance rule at every min_distance where the grid's cell meets a rounding or an int conversion: 0.4 .. 2.5, the
image's longer side, beyond its diagonal, just under 2^31, beyond it, 1e300 and inf.  The grid itself is not the judge: both
implementations share it.

The definition: visit the keys by value descending, ties later raster index first; accept a key unless an accepted corner lies at squared
distance < min_distance^2; stop at max_corners."""
import ctypes
import importlib

import numpy as np
import pytest

import corner_def
import oracle
import synth

vs = importlib.import_module("video-annotator_amd")

BAD_QUALITY = (0.0, -0.0, -1e-300, -0.01, -1.0, float("-inf"), float("nan"))
BAD_DISTANCE = (-1e-300, -0.5, -30.0, float("-inf"), float("nan"))
MESSAGE = ": quality must be > 0 and min_distance >= 0"


def _calls():
    """name -> (name in the messages, call(quality, min_distance, **kw) -> (status, message)); kw: mc (max_corners), pm (mask pitch), k"""
    L, c = vs.lib, ctypes
    xy, n, used = np.zeros(16, np.float32), c.c_int(), c.c_int()
    fp = xy.ctypes.data_as(c.POINTER(c.c_float))

    def done(st):
        return st, L.vstab_last_error().decode()

    def plain(q, md, mc=4, **kw):
        return done(L.vstab_good_features(4096, 640, 640, 360, mc, q, md, fp, c.byref(n), None))

    def ex(q, md, mc=4, det=0, **kw):
        return done(L.vstab_good_features_ex(4096, 640, 640, 360, mc, q, md, det, fp, c.byref(n), c.byref(used), None))

    def mask(q, md, mc=4, pm=640, det=0, **kw):
        return done(L.vstab_good_features_mask(4096, 640, 640, 360, 8192, pm, mc, q, md, det, fp, c.byref(n), c.byref(used), None))

    def harris(q, md, mc=4, pm=640, k=0.04, det=0, **kw):
        return done(L.vstab_good_features_harris(4096, 640, 640, 360, 8192, pm, mc, q, md, k, det, fp, c.byref(n), c.byref(used), None))

    return {"vstab_good_features": ("vstab_good_features", plain), "vstab_good_features_ex": ("vstab_good_features", ex),
            "vstab_good_features_mask": ("vstab_good_features_mask", mask), "vstab_good_features_harris": ("vstab_good_features_harris", harris)}


@pytest.mark.parametrize("entry", ["vstab_good_features", "vstab_good_features_ex", "vstab_good_features_mask", "vstab_good_features_harris"])
def test_quality_and_min_distance_are_refused(entry):
    name, call = _calls()[entry]
    want = (vs.ERR_INVALID, name + MESSAGE)
    for q in BAD_QUALITY:
        assert call(q, 30.0) == want, q
    for md in BAD_DISTANCE:
        assert call(0.01, md) == want, md
    assert call(float("nan"), float("nan")) == want and call(-1.0, -1.0) == want
    # the order: behind "bad argument" (max_corners <= 0 stays one of those, an unknown detector too) ...
    assert call(-1.0, 30.0, mc=0) == (vs.ERR_INVALID, name + ": bad argument")
    assert call(0.01, float("nan"), mc=-3) == (vs.ERR_INVALID, name + ": bad argument")
    if entry != "vstab_good_features":
        assert call(-1.0, 30.0, det=7) == (vs.ERR_INVALID, name + ": bad argument")
    # ... and before the mask's checks and k's
    assert call(-1.0, 30.0, pm=639) == want and call(0.01, -1.0, pm=1 << 24) == want
    assert call(float("nan"), 30.0, k=0.3) == want and call(0.01, float("nan"), k=float("nan")) == want
    # what passes the contract reaches the checks behind it (a device is needed only behind those)
    if entry in ("vstab_good_features_mask", "vstab_good_features_harris"):
        for q, md in ((1e-300, 0.0), (float("inf"), float("inf")), (2.0, 1e300), (0.01, -0.0)):
            assert call(q, md, pm=639) == (vs.ERR_INVALID, name + ": the mask's pitch is smaller than the image's width"), (q, md)
    if entry == "vstab_good_features_harris":
        assert call(float("inf"), float("inf"), k=0.3) == (vs.ERR_INVALID, name + ": k lies in [0, 0.25)")


def test_the_fused_hooks_keep_refusing_what_the_contract_refuses():
    """vstabx_corners_fused* take no min_distance and keep their own, narrower rule and message (quality in (0, 1]: pinned by
    test_detection_mask_cpu.py and test_harris_cpu.py); every quality the contract refuses is refused there"""
    class Fake:
        shape = (360, 640)

        def __init__(self, ptr):
            self.ptr = ptr

        def data_ptr(self):
            return self.ptr

        def stride(self, d):
            return 640

    for q in BAD_QUALITY:
        for fn, args in ((vs.corners_fused, ()), (vs.corners_fused_mask, (Fake(8192),)), (vs.corners_fused_harris, (Fake(8192),))):
            with pytest.raises(vs.VstabError) as e:
                fn(Fake(4096), *args, quality=q, stream=ctypes.c_void_p())
            assert e.value.status == vs.ERR_INVALID and str(e.value).endswith(": quality lies in (0, 1]"), (q, str(e.value))


# ---------------------------------------------------------------------------------------------------------------------------------
# the minimum-distance rule
# ---------------------------------------------------------------------------------------------------------------------------------
def brute_force(keys, w, max_corners, min_distance):
    """the definition in the module's docstring: (n, 2) float32 corners in the order they are accepted"""
    order = np.sort(np.asarray(keys, np.uint64))[::-1]           # value, then raster index, both descending
    idx = (order & np.uint64(0xFFFFFFFF)).astype(np.int64)
    xs, ys = idx % w, idx // w
    md2 = float(min_distance) * float(min_distance)               # (+inf for 1e300 and inf)
    ax, ay = np.zeros(len(idx), np.int64), np.zeros(len(idx), np.int64)
    n = 0
    for x, y in zip(xs.tolist(), ys.tolist()):
        if n and ((ax[:n] - x) ** 2 + (ay[:n] - y) ** 2 < md2).any():
            continue
        ax[n], ay[n] = x, y
        n += 1
        if max_corners > 0 and n == max_corners:
            break
    return np.stack([ax[:n], ay[:n]], 1).astype(np.float32)


def distances(w, h):
    return (0.0, 0.4, 0.5, 0.6, 1.0, 1.4, 1.5, 2.5, 30.0, float(max(w, h)), float(np.hypot(w, h)) + 1.0, 1e6, 2147483000.0, 4e9, 1e300, float("inf"))


FRAMES = {"luma_160x90": (31, 160, 90), "luma_97x61": (32, 97, 61)}


def frame_keys(name):
    """the candidate keys (float bits << 32 | raster index) of a frame at quality 0.01: oracle.min_eig, thresholded, 3 x 3 maxima"""
    seed, w, h = FRAMES[name]
    g = synth.luma(seed, w, h, rects=24)
    e, cand, _ = corner_def.candidates(g, np.ones((h, w), np.uint8), 0.01)
    ys, xs = np.nonzero(cand)
    keys = (e[ys, xs].view(np.uint32).astype(np.uint64) << np.uint64(32)) | (ys * w + xs).astype(np.uint64)
    assert len(keys) > 60
    return g, keys, w, h


def plateau_keys():
    """a plateau of ties -- every pixel of a 40 x 30 block of a 57 x 41 image, one value -- under a handful of stronger keys: the order
    among equal values (later raster index first) decides every acceptance"""
    w, h = 57, 41
    ys, xs = np.mgrid[5:35, 9:49]
    one = np.uint64(np.float32(0.25).view(np.uint32))
    keys = (one << np.uint64(32)) | (ys * w + xs).astype(np.uint64).ravel()
    top = np.uint64(np.float32(0.5).view(np.uint32))
    strong = np.array([(top << np.uint64(32)) | np.uint64(y * w + x) for x, y in ((0, 0), (56, 40), (7, 20), (8, 20))], np.uint64)
    assert len(np.unique(np.concatenate([keys, strong]) & np.uint64(0xFFFFFFFF))) == len(keys) + 4   # (a pixel has one key)
    return np.concatenate([keys, strong]), w, h


@pytest.mark.parametrize("max_corners", (0, 25), ids=("no_limit", "max_25"))
@pytest.mark.parametrize("name", sorted(FRAMES) + ["plateau"])
def test_select_corners_against_the_brute_force_definition(name, max_corners):
    if name == "plateau":
        keys, w, h = plateau_keys()
        g = None
    else:
        g, keys, w, h = frame_keys(name)
    rng = np.random.default_rng(3)
    counts = []
    for md in distances(w, h):
        want = brute_force(keys, w, max_corners, md)
        shuffled = keys.copy()
        rng.shuffle(shuffled)
        got = vs.select_corners(shuffled, w, h, max_corners, md)
        assert got.shape == want.shape and np.array_equal(got, want), (name, md, got.shape, want.shape)
        if g is not None:
            ref = oracle.good_features(g, max_corners, 0.01, md)
            assert ref.shape == want.shape and np.array_equal(ref, want), (name, "oracle", md, ref.shape, want.shape)
        counts.append(len(want))
    # the distances do what they are there for: nothing rejected up to 1.0 (two pixels are never closer than 1), some at 30 -- on the
    # plateau of neighbours from 1.4 on --, and one corner from beyond the diagonal on
    full = len(keys) if max_corners <= 0 else min(len(keys), max_corners)
    assert counts[:5] == [full] * 5
    assert counts[-6:] == [1] * 6
    if max_corners <= 0:
        assert full > counts[8] > 1
        if name == "plateau":
            assert full > counts[5] > counts[7] > counts[8]
