"""GPU half of the Harris tests: vstab_corner_harris against the definition bit for bit, vstab_good_features_harris with its three
detectors, the raw output of k_corners_fused_harris(_masked) + k_filter_keys (test hook vstabx_corners_fused_harris), the two-pass
fall-back and a handle with vstab_set_corner_response, against tests/corner_def.py.  What the named frames reach is asserted without a
GPU in test_harris_cpu.py.  Every comparison is exact (rotations: the 1e-9 of test_pipeline_gpu.py)."""
import numpy as np
import pytest

import corner_tiles as C
import corner_def as H
import mask_def as M
import oracle
import synth
from test_detection_mask_gpu import FILL, LAYOUTS, PARAMS, dev, mask_view

pytestmark = pytest.mark.gpu

KS = (0.0, 0.04, 0.06, 0.2)


# ---- the dense map -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(3, 3), (65, 32), (66, 33), (322, 182)])
def test_dense_map_is_the_definition(vs, cuda, w, h):
    g = synth.luma(13, max(w, 16), max(h, 16))[:h, :w]
    gd = dev(g, cuda)
    sums = H.covariance_sums(g)
    for k in KS:
        got = vs.corner_harris(gd, k).cpu().numpy()
        assert np.array_equal(got.view(np.uint32), H.response_from_sums(*sums, k).view(np.uint32)), (w, h, k)


def test_dense_map_byte_path(vs, cuda):
    """129 x 63 with a pitch above the width from an odd base address: no dword loads"""
    import torch
    w, h, pitch = 129, 63, 141
    g = synth.luma(17, w, h)
    buf = torch.zeros(pitch * h + 8, dtype=torch.uint8, device=cuda)
    v = buf[1:1 + pitch * h].view(h, pitch)[:, :w]
    v.copy_(torch.from_numpy(np.ascontiguousarray(g)).to(cuda))
    assert v.data_ptr() % 2 == 1 and v.stride(0) == pitch
    sums = H.covariance_sums(g)
    for k in KS:
        assert np.array_equal(vs.corner_harris(v, k).cpu().numpy().view(np.uint32), H.response_from_sums(*sums, k).view(np.uint32)), k


# ---- the stateless detectors ----------------------------------------------------------------------------------------------------------------
def frame(name):
    return C.timing_frame() if name == "timing" else H.frame(name)


def masks_for(g):
    h, w = g.shape
    return {"none": None, "full": M.full(h, w), "zero": np.zeros((h, w), np.uint8), "overlay": M.overlay_box(h, w), "roi": M.roi(h, w),
            "checker_1": M.checkerboard(h, w, 1, 1), "checker_64x31": M.checkerboard(h, w, 31, 64, 1, 1)}


def check_stateless(vs, cuda, g, mask, what, k=H.K_DEFAULT):
    gd = dev(g, cuda)
    e, cand, _ = H.candidates(g, mask, 0.01, harris=True, k=k)
    exp = [H.select(e, cand, mc, md) for mc, _, md in PARAMS]
    for layout in LAYOUTS if mask is not None else ("none",):
        md_ = None if mask is None else mask_view(mask, cuda, layout)
        for det in (vs.DETECTOR_AUTO, vs.DETECTOR_FUSED, vs.DETECTOR_TWO_PASS):
            for (mc, q, md), want in zip(PARAMS, exp):
                info = {}
                got = vs.good_features_harris(gd, md_, mc, q, md, k, detector=det, info=info)
                assert np.array_equal(got, want), (what, layout, det, mc, len(got), len(want))
                assert info["detector_used"] == (vs.DETECTOR_TWO_PASS if det == vs.DETECTOR_TWO_PASS else vs.DETECTOR_FUSED)
    return [len(x) for x in exp]


@pytest.mark.parametrize("name", ["timing", "luma_322x182"] + [f"cut_{w}x{h}" for w, h in C.CUTS])
def test_stateless_all_detectors_against_the_definition(vs, cuda, name):
    g = frame(name)
    for what, mask in masks_for(g).items():
        n = check_stateless(vs, cuda, g, mask, what)
        print(name, what, "corners", n)
        if what == "zero":
            assert n == [0, 0]
    # the minimum-eigenvalue entry points are where they were
    assert np.array_equal(vs.good_features_mask(dev(g, cuda), None, 200, 0.01, 30.0, detector=vs.DETECTOR_FUSED), oracle.good_features(g))
    assert np.array_equal(vs.good_features_mask(dev(g, cuda), mask_view(M.full(*g.shape), cuda, "aligned"), 200, 0.01, 30.0), oracle.good_features(g))


def test_k_separates(vs, cuda):
    g = np.ascontiguousarray(M.overlay_clip(n=1)[2][0][:360])
    lists = [check_stateless(vs, cuda, g, None, f"k {k}", k) for k in (0.04, 0.15)]
    a, b = (vs.good_features_harris(dev(g, cuda), None, k=k) for k in (0.04, 0.15))
    assert not np.array_equal(a, b) and not np.array_equal(a, oracle.good_features(g)) and not np.array_equal(b, oracle.good_features(g)), lists


# ---- the raw hook ---------------------------------------------------------------------------------------------------------------------------
def host_half(vs, m, keys, kept, max_bits, mc, md):
    """what Detector::good_features does behind the kernels: rule 4 from the sign of the published maximum, then the selection"""
    if max_bits < 0:
        return np.zeros((0, 2), np.float32)
    k = np.sort(keys[:kept])
    cand = np.zeros((m.h, m.w), bool)
    idx = (k & np.uint64(0xffffffff)).astype(np.int64)
    cand[idx // m.w, idx % m.w] = True
    return H.select(m.eig, cand, mc, md)


def check_raw(vs, cuda, m, mask_dev=None):
    g = dev(m.img, cuda)
    if not m.positive:
        # rule 4: nothing of what the kernels leave counts; a key buffer of a modest size must still be respected
        keys, kept, spilled, tiles, max_bits = vs.corners_fused_harris(g, mask_dev, m.k, m.quality, cap=1024, canary=64)
        print(f"{m.w} x {m.h}: no positive response, published maximum bits {max_bits}, kept {kept}, spilled {spilled}")
        assert max_bits < 0
        assert (keys[min(kept, 1024):] == FILL).all()
        assert m.frame_max < 0 and np.array_equal(tiles, m.hi)          # every tile filters with -inf: all of its masked-in 3 x 3 maxima
        assert len(host_half(vs, m, keys, kept, max_bits, 200, 30.0)) == 0
        return
    keys, kept, spilled, tiles, max_bits = vs.corners_fused_harris(g, mask_dev, m.k, m.quality, cap=m.n + 7, canary=64)
    print(f"{m.w} x {m.h}: kept {kept} (model {m.n}), spilled {spilled} (model {m.spilled_range()}), negative tiles {int(m.negative.sum())}, "
          f"tile counts {tiles.ravel().tolist()[:12]}")
    assert max_bits >= 0 and np.int32(max_bits).view(np.float32) == m.frame_max
    assert kept == m.n
    assert (keys[kept:] == FILL).all()                               # nothing written past the keys: the tail of the buffer and the canary
    assert np.array_equal(np.sort(keys[:kept]), m.keys)
    assert tiles.shape == m.lo.shape and (tiles >= m.lo).all() and (tiles <= m.hi).all()
    assert not tiles[m.early].any()
    lo, hi = m.spilled_range()
    assert lo <= spilled <= hi and spilled == int((tiles > C.SLOTS).sum())
    for mc, q, md in PARAMS:
        assert np.array_equal(host_half(vs, m, keys, kept, max_bits, mc, md), m.corners(mc, md))


@pytest.mark.parametrize("name", H.RAW_FRAMES)
def test_raw_output_against_the_model(vs, cuda, name):
    m = H.raw_model(name, harris=True)
    check_raw(vs, cuda, m)
    g = dev(m.img, cuda)
    for det in (vs.DETECTOR_AUTO, vs.DETECTOR_FUSED, vs.DETECTOR_TWO_PASS):
        for mc, q, md in PARAMS:
            got = vs.good_features_harris(g, None, mc, q, md, m.k, detector=det)
            assert np.array_equal(got, m.corners(mc, md)), (name, det, mc)
            assert m.positive or len(got) == 0


def test_rule_4_under_a_mask(vs, cuda):
    """the masked-in responses are all <= 0 while a masked-out patch holds positive corners: no corner, from any detector"""
    m = H.rule4_masked_model()
    assert not m.positive
    for layout in LAYOUTS:
        md_ = mask_view(m.mask, cuda, layout)
        check_raw(vs, cuda, m, md_)
        for det in (vs.DETECTOR_AUTO, vs.DETECTOR_FUSED, vs.DETECTOR_TWO_PASS):
            assert len(vs.good_features_harris(dev(m.img, cuda), md_, 4000, 0.01, 0.0, detector=det)) == 0
    assert len(vs.good_features_harris(dev(m.img, cuda), None, 4000, 0.01, 0.0)) > 0


def test_two_pass_fall_back(vs, cuda):
    g = H.fall_back_frame()
    e, cand, _ = H.candidates(g, harris=True)
    assert int(cand.sum()) > C.KEY_CAP
    for mc, q, md in PARAMS:
        info = {}
        got = vs.good_features_harris(dev(g, cuda), None, mc, q, md, detector=vs.DETECTOR_AUTO, info=info)
        assert info["detector_used"] == vs.DETECTOR_TWO_PASS
        assert np.array_equal(got, H.select(e, cand, mc, md)), mc


# ---- the pipeline -----------------------------------------------------------------------------------------------------------------------
def run_product(vs, cuda, frames, mask=None, k=H.K_DEFAULT, **cfg):
    import test_pipeline_gpu as P
    return P.run_product(vs, cuda, frames, detection_mask=mask, corner_response=vs.CORNER_HARRIS, harris_k=k, **cfg)


def check_against_state_machine(vs, cuda, frames, K, w, h, r, seed, mask, mask_arg, k=H.K_DEFAULT):
    """test_detection_mask_gpu.check_against_state_machine with find = corner_def.good_features with the Harris response"""
    import expect
    stab, outs = run_product(vs, cuda, frames, mask_arg, k, smooth_radius=r, seed=seed)
    log = stab.frame_log()
    n = len(frames)
    assert len(outs) == max(n - 1, 0) and len(log) == max(n - 1, 0)
    Ko, (cw, ch) = oracle.get_output_camera(K, w, h)
    sm, exp, counts, warp_rots = M.run_state_machine(frames, K, w, h, r, seed, lambda g: H.good_features(g, mask, harris=True, k=k))
    assert [l["key"] for l in log] == [l["key"] for l in sm.log]
    assert [(l["n_corners"], l["n_tracked"]) for l in log] == counts
    assert [l["inliers"] for l in log] == [l["inliers"] for l in sm.log]
    assert all(np.allclose(a["R"], b["R"], atol=1e-9) for a, b in zip(log, sm.log))
    for i in range(len(outs)):
        assert np.allclose(stab.warp_rotation(i), warp_rots[i], atol=1e-9), i
        p = oracle.map_params(K, Ko, stab.warp_rotation(i))
        assert np.array_equal(outs[i], expect.warp(exp[i], p, cw, ch)), i
    return stab, log


@pytest.mark.parametrize("masked", [False, True])
def test_pipeline_overlay_clip(vs, cuda, masked):
    import test_pipeline_gpu as P
    K, _, frames, _, mask = M.overlay_clip()
    w, h = 640, 360
    _, log = check_against_state_machine(vs, cuda, frames, K, w, h, 5, 5, mask if masked else None, dev(mask, cuda) if masked else None)
    plain, _ = P.run_product(vs, cuda, frames, smooth_radius=5, seed=5, detection_mask=dev(mask, cuda) if masked else None)
    assert not all(np.array_equal(a["R"], b["R"]) for a, b in zip(plain.frame_log(), log))


def test_pipeline_planned_key_frame_is_detected_ahead(vs, cuda):
    (w, h), frames = C.pipeline_clip("under_spec_cap")
    K = oracle.get_preset_camera(4, w, h)
    stab, log = check_against_state_machine(vs, cuda, frames, K, w, h, 2, 1, None, None)
    c, prof = stab.detector_counters(), stab.profile()
    selections = prof["corner_selections_by_caller"] + prof["corner_selections_by_helper"]
    assert [k for k, l in enumerate(log) if l["key"]] == [20] and selections == 1           # the counter's key frame, detected ahead of time
    assert c["spec_over_cap"] == 0 and c["fused_overflows"] == 0
    assert min(l["n_tracked"] for l in log) >= 150


def test_pipeline_ten_bit_handle(vs, cuda):
    """a pixel_depth 10 handle's detector reads the luma narrowed to 8 bits: with Harris its frame log is that of the 8-bit handle on the
    truncated frames"""
    import torch
    K, _, frames8, _, mask = M.overlay_clip(n=8)
    n, r = len(frames8), 2
    rng = np.random.default_rng(8)
    wide = [((f.astype(np.uint16) << 8) | rng.integers(0, 256, f.shape, dtype=np.uint16)) for f in frames8]
    devw = [torch.from_numpy(x.view(np.int16)).to(cuda) for x in wide]
    ten = vs.Stabilizer(devw, total=n, bit_depth=10, smooth_radius=r, seed=3, pixel_depth=10, blend=vs.BLEND_EXACT, corner_response=vs.CORNER_HARRIS, harris_k=0.06)
    cw, ch = ten.out_size
    pulls = 0
    while True:
        oy = torch.empty((ch, cw), dtype=torch.int16, device=cuda)
        ouv = torch.empty(((ch + 1) // 2, 2 * ((cw + 1) // 2)), dtype=torch.int16, device=cuda)
        if not ten.pull_p010_into(oy, ouv):
            break
        pulls += 1
    import test_pipeline_gpu as P
    eight, _ = run_product(vs, cuda, frames8, None, 0.06, smooth_radius=r, seed=3)
    plain, _ = P.run_product(vs, cuda, frames8, smooth_radius=r, seed=3)
    key = lambda l: (l["key"], l["n_corners"], l["n_tracked"], l["inliers"], l["R"].tobytes())
    assert pulls == n - 1 and [key(l) for l in ten.frame_log()] == [key(l) for l in eight.frame_log()]
    assert [key(l) for l in plain.frame_log()] != [key(l) for l in eight.frame_log()]


def _short_clip(cuda):
    import torch
    w, h = 322, 182
    K = oracle.get_preset_camera(4, w, h)
    frames, _ = synth.shaky_clip(5, K, w, h, 5, sigma=0.004)
    return w, h, frames, [torch.from_numpy(f).to(cuda) for f in frames]


def _drain(stab):
    outs = []
    while True:
        o = stab.pull()
        if o is None:
            return outs
        outs.append(o.cpu().numpy())


def test_reset_to_the_minimum_eigenvalue(vs, cuda):
    """Harris, then VSTAB_CORNER_MIN_EIGENVAL (k not looked at) before the first pull: the plain handle's log and output bytes"""
    w, h, frames, devf = _short_clip(cuda)
    plain = vs.Stabilizer(devf, total=len(devf), smooth_radius=1, seed=2)
    outs0 = _drain(plain)
    stab = vs.Stabilizer(devf, total=len(devf), smooth_radius=1, seed=2, corner_response=vs.CORNER_HARRIS, harris_k=0.1)
    stab.set_corner_response(vs.CORNER_MIN_EIGENVAL, 99.0)
    outs = _drain(stab)
    harris = vs.Stabilizer(devf, total=len(devf), smooth_radius=1, seed=2, corner_response=vs.CORNER_HARRIS, harris_k=0.1)
    _drain(harris)
    key = lambda l: (l["key"], l["n_corners"], l["n_tracked"], l["inliers"], l["fallback"], l["R"].tobytes())
    assert [key(l) for l in plain.frame_log()] == [key(l) for l in stab.frame_log()] and any(l["n_corners"] > 0 for l in plain.frame_log())
    assert len(outs) == len(outs0) == len(devf) - 1 and all(np.array_equal(a, b) for a, b in zip(outs, outs0))
    assert [key(l) for l in plain.frame_log()] != [key(l) for l in harris.frame_log()]


def test_setter_refusals_that_need_a_handle(vs, cuda):
    w, h, frames, devf = _short_clip(cuda)
    L = vs.lib

    def refused(stab, msg, response, k):
        assert L.vstab_set_corner_response(stab._h, response, k) == vs.ERR_INVALID
        assert L.vstab_last_error().decode() == "vstab_set_corner_response: " + msg

    off = vs.Stabilizer(devf, total=4, smooth_radius=1, tracking=0)
    refused(off, "no detector runs on this handle (tracking = 0)", vs.CORNER_HARRIS, 0.04)
    refused(off, "no detector runs on this handle (tracking = 0)", 7, 0.5)                          # before the response and k
    off.close()
    stab = vs.Stabilizer(devf, total=4, smooth_radius=1, seed=2)
    bad_response = "response must be VSTAB_CORNER_MIN_EIGENVAL (0) or VSTAB_CORNER_HARRIS (1)"
    refused(stab, bad_response, 2, 0.04)
    refused(stab, bad_response, -1, 0.5)                                                            # the response before k
    for k in (0.25, -1e-9, float("nan"), float("inf")):
        refused(stab, "k lies in [0, 0.25)", vs.CORNER_HARRIS, k)
    assert L.vstab_set_corner_response(stab._h, vs.CORNER_MIN_EIGENVAL, float("nan")) == 0          # k is not looked at
    # a refused call leaves the handle unchanged: still the plain handle
    plain = vs.Stabilizer(devf, total=4, smooth_radius=1, seed=2)
    _drain(plain)
    assert len(_drain(stab)) == 3
    key = lambda l: (l["key"], l["n_corners"], l["n_tracked"], l["R"].tobytes())
    assert [key(l) for l in stab.frame_log()] == [key(l) for l in plain.frame_log()]
    refused(stab, "the response must be set before the first pull", vs.CORNER_HARRIS, 0.04)
    refused(stab, "the response must be set before the first pull", 5, 0.5)                         # before the response and k
    stab.close()
    assert L.vstab_set_corner_response(None, vs.CORNER_HARRIS, 0.04) == vs.ERR_INVALID
    assert L.vstab_last_error().decode() == "vstab_set_corner_response: null handle"
