"""CPU half of the multi-pair LK tests (tests/lk_segments.py): the scripted clips mean what they claim, they reach every fetch-ahead
branch of k_lk_track with fi > 0, what the pipeline's own clip reaches is pinned, and the test hook refuses bad arguments without a
device."""
import ctypes
import importlib

import numpy as np
import pytest

import lk_segments as M
import oracle
import synth


@pytest.fixture(scope="module")
def runs():
    """every scripted set tracked by the oracle as one chain, with the model's decisions"""
    out = {}
    for name in M.SETS:
        frames, pts, off = M.make_set(name)
        K = len(frames) - 1
        exp = M.expected(frames, pts, [K])
        h, w = frames[0].shape
        neigh, top = M.fetch_ahead(exp, w, h)
        out[name] = (frames, pts, off, exp, neigh, top)
    return out


def test_translation_scripts_move_by_their_shift(runs):
    """Ground truth: the oracle's median flow over the slots it keeps equals the scripted shift within 0.05 px, pair by pair."""
    for name in M.TRANSLATION:
        frames, pts, off, exp, _, _ = runs[name]
        for k in range(len(frames) - 1):
            ok = exp["status"][k] == 1
            assert ok.sum() >= 10, (name, k)
            flow = np.median(exp["xy"][k][ok] - exp["start"][k][ok], 0)
            assert np.abs(flow + (off[k + 1] - off[k])).max() < 0.05, (name, k, flow, off[k + 1] - off[k])


def test_every_fetch_ahead_branch_is_reached(runs):
    """With fi > 0: on the 4-level pyramid every level's neighbourhood is served ahead, missed (level 0 carried the feature more
    than the slack at that level: blind_640) and not fetched (a block across the border); the top level's predicted block is served,
    missed (the motion jumps: jump_640, blind_640) and not fetched.  The 2- and 3-level pyramids serve and skip fetching at every
    level, the 1-level one fetches nothing.  `skipped` is reached by start points of a first pair only (the model's docstring says
    why it cannot happen later) -- and never with fi > 0."""
    total = {}
    per_levels = {}
    for name, (frames, _, _, exp, neigh, top) in runs.items():
        r = M.reached(neigh, top, exp["fi"], exp["nl"])
        for key, v in r.items():
            total[key] = total.get(key, 0) + v
            per_levels.setdefault(exp["nl"], {})[key] = per_levels.setdefault(exp["nl"], {}).get(key, 0) + v
    for l in range(4):
        for c in ("served", "missed", "not_fetched"):
            assert per_levels[4].get(("neigh", l, c), 0) > 0, (l, c)
        assert total.get(("neigh", l, "skipped"), 0) == 0
        assert per_levels[4].get(("first", l, "skipped"), 0) > 0, l
    for c in ("served", "missed", "not_fetched"):
        assert per_levels[4].get(("top", c), 0) > 0, c
    for nl in (2, 3):
        for l in range(nl):
            assert per_levels[nl].get(("neigh", l, "served"), 0) > 0 and per_levels[nl].get(("neigh", l, "not_fetched"), 0) > 0, (nl, l)
        assert per_levels[nl].get(("top", "served"), 0) > 0, nl
    assert set(k for k in per_levels[1] if k[0] in ("neigh", "top")) == {("neigh", 0, "not_fetched"), ("top", "not_fetched")}
    assert total.get(("top", "skipped"), 0) == 0


def test_scripts_lose_slots_mid_segment(runs):
    """A slot lost in the middle of a segment, three ways: its window slid wholly into the flat patch (eigenvalue test: minEig 0),
    drifted across the border, or was carried out of the image by the last Gauss-Newton step (the final-position rule: the oracle
    without that rule keeps it)."""
    frames, pts, off, exp, _, _ = runs["flat_200"]
    x0, y0, x1, y1, k0 = M.SETS["flat_200"][5]
    k, s = np.nonzero((exp["status"] == 0) & (exp["fi"][:, None] > 0) & (np.arange(len(frames) - 1)[:, None] >= k0))
    st = exp["start"][k, s]
    inside = (st[:, 0] - 11 >= x0) & (st[:, 0] + 12 <= x1) & (st[:, 1] - 11 >= y0) & (st[:, 1] + 12 <= y1)   # the 21 x 21 window and its taps
    assert inside.any()
    for name in ("drift_240", "drift_y_333", "leave_200"):
        exp = runs[name][3]
        assert ((exp["status"] == 0) & (exp["fi"][:, None] > 0)).any(), name
    frames, pts, off, exp, _, _ = runs["leave_200"]
    rule = 0
    for k in range(1, len(frames) - 1):
        lost = np.flatnonzero(exp["status"][k] == 0)
        oracle.set_lk_final_check(False)
        try:
            _, st = oracle.pyr_lk(frames[k], frames[k + 1], exp["start"][k][lost])
        finally:
            oracle.set_lk_final_check(True)
        rule += int((st == 1).sum())
    assert rule > 0


def test_pipeline_clip_reaches_only_served_and_unfetched():
    """Pinned fact: the pipeline's smoke clip (640 x 360, sigma 0.004 rad, oracle corners, seven pairs as one segment) never misses a
    block fetched ahead -- what the scripted sets are for."""
    K = oracle.get_preset_camera(oracle.GOPRO_H4B_WIDE169_MEASURED, 640, 360)
    frames, _ = synth.shaky_clip(2, K, 640, 360, 8, sigma=0.004)
    ys = [f[:360] for f in frames]
    pts = oracle.good_features(ys[0], 200, 0.01, 30.0)
    exp = M.expected(ys, pts, [7])
    neigh, top = M.fetch_ahead(exp, 640, 360)
    r = M.reached(neigh, top, exp["fi"], exp["nl"])
    assert {k: v for k, v in r.items() if k[0] in ("neigh", "top")} == {
        ("neigh", 0, "not_fetched"): 34, ("neigh", 0, "served"): 382, ("neigh", 1, "not_fetched"): 91, ("neigh", 1, "served"): 325,
        ("neigh", 2, "not_fetched"): 182, ("neigh", 2, "served"): 234, ("neigh", 3, "not_fetched"): 330, ("neigh", 3, "served"): 86,
        ("top", "not_fetched"): 330, ("top", "served"): 86}


def test_model_restates_the_kernel_tests():
    """Hand-made cases of the model's integer tests: the +-4 px slack of a neighbourhood, the 2-px margin of the top block, the
    interior test of a block fetched ahead."""
    w, h = 640, 360
    nl = M.level_sizes(w, h)[0]
    assert nl == 4
    # pair 1 starts where level 0 put it; level 1 said e0 / 2.  Neighbourhood origin floor(e0 - 10) - 5; served iff ipx - 1 - origin in 0..8
    for shift, cat0 in ((0.0, "served"), (4.0, "served"), (4.499, "served"), (4.5, "missed"), (-4.0, "served"), (-4.501, "missed")):
        e0 = np.float32(300.5)
        exp = {"status": np.ones((2, 1), np.uint8), "fi": np.array([0, 1]), "start": np.array([[[290.0, 180.0]], [[e0 + shift, 180.0]]], np.float32),
               "levels": np.full((2, 1, 4, 2), np.nan, np.float32)}
        exp["levels"][0, 0, 1] = (e0 / 2, 90.0)
        neigh, top = M.fetch_ahead(exp, w, h)
        assert neigh[1, 0, 0] == cat0, (shift, neigh[1, 0, 0])
    # a neighbourhood block across the border is not fetched
    exp["start"][1, 0] = (12.0, 180.0)
    exp["levels"][0, 0, 1] = (6.0, 90.0)
    neigh, top = M.fetch_ahead(exp, w, h)
    assert neigh[1, 0, 0] == "not_fetched" and neigh[1, 0, 3] == "not_fetched"
    # the top block (level 3, 80 x 45) around p0 = (320, 180): origin (25, 7); served iff the window keeps 2 px inside it, i.e.
    # ipx - floor(p0 / 8 - 10) in -3 .. 3
    exp["start"][0, 0] = (320.0, 180.0)
    exp["levels"][0, 0, 1] = (160.0, 90.0)
    for s, cat in ((0, "served"), (3, "served"), (4, "missed"), (-3, "served"), (-4, "missed")):
        exp["start"][1, 0] = (320.0 + 8 * s, 180.0)
        neigh, top = M.fetch_ahead(exp, w, h)
        assert top[1, 0] == cat, (s, top[1, 0])


def test_hook_refuses_bad_arguments_without_a_device():
    """vstabx_lk_segments checks everything before it touches the device: null frames / points / outputs, sizes, a segment of 0 or 9
    pairs, more pairs than record buffers, a bad_parent that is not a chained launch, a pitch below the width, half the pack-mode
    planes, pack mode on a one-level pyramid, planes that pack_pyr_ok refuses."""
    vs = importlib.import_module("video-annotator_amd")
    L = vs.lib
    c = ctypes

    class Fake:   # a "device" plane: only its pointer and pitch reach the library, which refuses before using them
        def __init__(self, ptr, pitch, shape):
            self.ptr, self.pitch, self.shape = ptr, pitch, shape

        def data_ptr(self):
            return self.ptr

        def stride(self, d):
            return self.pitch

    def call(frames, pts, segs, **kw):
        with pytest.raises(vs.VstabError) as e:
            vs.lk_segments(frames, pts, segs, stream=ctypes.c_void_p(), **kw)
        assert e.value.status == vs.ERR_INVALID, str(e.value)

    w, h = 640, 360
    fr = [Fake(4096 * (i + 1), 640, (h, w)) for i in range(9)]
    pts = np.array([[100.0, 100.0]], np.float32)
    call(fr, pts, [0])
    call(fr, pts, [9])
    call(fr, pts, [-1, 9])
    call(fr, np.zeros((0, 2), np.float32), [8])
    call(fr, pts, [])
    call(fr[:1] * 34, pts, [8, 8, 8, 8, 1])          # 33 pairs > 32 record buffers
    call(fr, pts, [4, 4], bad_parent=0)             # the first launch has no parent
    call(fr, pts, [4, 4], bad_parent=2)
    call(fr, pts, [8], w=0)
    call(fr, pts, [8], h=-1)
    call([Fake(4096, 639, (h, w))] + fr[1:], pts, [8])                    # pitch < width
    call([Fake(0, 640, (h, w))] + fr[1:], pts, [8])                       # null frame
    call(fr, pts, [8], uv=fr)                                              # uv without rings
    call(fr, pts, [8], rings=fr)
    small = [Fake(4096, 64, (30, 40))] * 9
    call(small, pts, [8], uv=small, rings=small)                            # one level: no level 1 to pack
    call([Fake(4098, 640, (h, w))] + fr[1:], pts, [8], uv=fr, rings=fr)    # luma base not 4-byte aligned: pack_pyr_ok refuses
    call(fr, pts, [8], uv=fr, rings=[Fake(4100, 0, (h, w))] + fr[1:])      # ring not 8-byte aligned
    hrec = np.zeros(4, np.uint32)
    f = (c.c_void_p * 9)(*[x.ptr for x in fr])
    p = (c.c_size_t * 9)(*([640] * 9))
    sg = np.array([8], np.int32)
    u32 = c.POINTER(c.c_uint32)
    for args in ((None, p, pts, hrec, hrec), (f, None, pts, hrec, hrec), (f, p, None, hrec, hrec), (f, p, pts, None, hrec), (f, p, pts, hrec, None)):
        fa, pa, pt, hr, dr = args
        rc = L.vstabx_lk_segments(fa, pa, w, h, None if pt is None else pt.ctypes.data_as(c.POINTER(c.c_float)), 1, sg.ctypes.data_as(c.POINTER(c.c_int)), 1,
                                  None, None, None, -1, None if hr is None else hr.ctypes.data_as(u32), None if dr is None else dr.ctypes.data_as(u32), None, None)
        assert rc == vs.ERR_INVALID
