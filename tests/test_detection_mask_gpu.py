"""GPU half of the detection-mask tests: vstab_good_features_mask with its three detectors, the raw output of k_corners_fused_masked +
k_filter_keys (test hook vstabx_corners_fused_mask), the two-pass fall-back and a handle with vstab_set_detection_mask, against the
definition and the masked tile model of tests/mask_def.py.  What the named sets reach is asserted without a GPU in
test_detection_mask_cpu.py.  Every comparison is exact (rotations: the 1e-9 of test_pipeline_gpu.py)."""

import numpy as np
import pytest

import corner_tiles as C
import expect
import corner_def as D
import mask_def as M
import oracle
import synth

pytestmark = pytest.mark.gpu

FILL = np.uint64(0xA5A5A5A5A5A5A5A5)
PARAMS = ((4000, 0.01, 0.0), (200, 0.01, 30.0))
LAYOUTS = ("aligned", "pitch_w1", "odd_base")


def dev(img, cuda):
    import torch
    return torch.from_numpy(np.ascontiguousarray(img)).to(cuda)


def mask_view(mask, cuda, layout):
    """the mask as a device view: base and pitch 4-byte aligned (the dword loads), pitch w + 1 on an aligned base, or an odd base address"""
    import torch
    h, w = mask.shape
    pitch, off = {"aligned": ((w + 3) // 4 * 4 + 4, 0), "pitch_w1": (w + 1, 0), "odd_base": ((w + 3) // 4 * 4, 1)}[layout]
    buf = torch.full((pitch * h + 8,), 255, dtype=torch.uint8, device=cuda)      # the padding reads "masked in": a byte taken from it would show
    v = buf[off:off + pitch * h].view(h, pitch)[:, :w]
    v.copy_(torch.from_numpy(np.ascontiguousarray(mask)).to(cuda))
    assert v.stride(0) == pitch and (v.data_ptr() % 4 == 0) == (off == 0) and (layout != "aligned" or pitch % 4 == 0)
    return v


def frame(name):
    if name == "timing":
        return C.timing_frame()
    if name == "luma_322x182":
        return synth.luma(11, 322, 182)
    return C.make(name)


def masks_for(g):
    h, w = g.shape
    m = C.Model(g)
    y, x = divmod(int(m.keys[-1] & np.uint64(0xffffffff)), w)            # the strongest corner (the last of the tie on a plateau)
    on, beside = np.zeros((h, w), np.uint8), np.zeros((h, w), np.uint8)
    on[y, x] = 1
    beside[y, x + 1 if x + 2 < w else x - 1] = 255
    return {"full": M.full(h, w), "overlay": M.overlay_box(h, w), "roi": M.roi(h, w), "checker_1": M.checkerboard(h, w, 1, 1),
            "checker_64x31": M.checkerboard(h, w, 31, 64, 1, 1), "on_a_corner": on, "beside_a_corner": beside, "zero": np.zeros((h, w), np.uint8)}


def check_stateless(vs, cuda, g, mask, what):
    gd = dev(g, cuda)
    e, cand, _ = D.candidates(g, mask)
    exp = [D.select(e, cand, mc, md) for mc, _, md in PARAMS]
    for layout in LAYOUTS:
        md_ = mask_view(mask, cuda, layout)
        for det in (vs.DETECTOR_AUTO, vs.DETECTOR_FUSED, vs.DETECTOR_TWO_PASS):
            for (mc, q, md), want in zip(PARAMS, exp):
                info = {}
                got = vs.good_features_mask(gd, md_, mc, q, md, detector=det, info=info)
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
        if what == "full":
            assert np.array_equal(vs.good_features_mask(dev(g, cuda), mask_view(mask, cuda, "aligned"), 200, 0.01, 30.0), vs.good_features(dev(g, cuda), detector=vs.DETECTOR_AUTO))
            assert np.array_equal(vs.good_features_mask(dev(g, cuda), None, 200, 0.01, 30.0, detector=vs.DETECTOR_FUSED), oracle.good_features(g))


def test_stateless_separating_cases(vs, cuda):
    g, m = M.case_filter_afterwards()
    assert check_stateless(vs, cuda, g, m, "filter afterwards") == [4000, 13]
    got = vs.good_features_mask(dev(g, cuda), dev(m, cuda), 6000, 0.01, 0.0)
    assert len(got) == 5154
    g, m = M.case_neighbours_compete()
    assert check_stateless(vs, cuda, g, m, "neighbours compete")[0] == 3


def check_raw(vs, m, gray, mask, cap=None):
    """one run of the hook against the masked model m"""
    cap = m.n + 7 if cap is None else cap
    keys, kept, spilled, tiles = vs.corners_fused_mask(gray, mask, m.quality, cap=cap, canary=64)
    print(f"{m.w} x {m.h}: kept {kept} (model {m.n}), spilled {spilled} (model {m.spilled_range()}), early {int(m.early.sum())}, tile counts {tiles.ravel().tolist()[:12]}")
    assert kept == m.n
    assert (keys[kept:] == FILL).all()                               # nothing written past the keys: the tail of the buffer and the canary
    assert np.array_equal(np.sort(keys[:kept]), m.keys)
    assert tiles.shape == m.lo.shape and (tiles >= m.lo).all() and (tiles <= m.hi).all()
    assert not tiles[m.early].any()
    lo, hi = m.spilled_range()
    assert lo <= spilled <= hi and spilled == int((tiles > C.SLOTS).sum())


@pytest.mark.parametrize("name", list(M.RAW_SETS))
def test_raw_output_against_the_masked_model(vs, cuda, name):
    m = D.raw_masked_model(name)
    g = dev(m.img, cuda)
    for layout in LAYOUTS:
        check_raw(vs, m, g, mask_view(m.mask, cuda, layout))
    for mc, q, md in PARAMS:
        assert np.array_equal(vs.good_features_mask(g, dev(m.mask, cuda), mc, q, md), m.corners(mc, md))


def test_two_pass_fall_back_under_a_mask(vs, cuda):
    """2^18 + 1 candidates with a mask that removes none of them (one flat pixel masked out): over the key capacity, the two-pass detector
    with its masked maximum and gate.  With a mask that removes a block of them: under the capacity, the fused detector."""
    img = C.cap_frame("2^18+1")
    h, w = img.shape
    base = C.Model(img)
    assert base.n == C.KEY_CAP + 1
    g = dev(img, cuda)
    keep, drop = M.full(h, w), M.full(h, w)
    assert not base.final[15, 15]                                   # inside the flat patch
    keep[15, 15] = 0
    drop[100:108, 100:140] = 0
    for mask, used in ((keep, vs.DETECTOR_TWO_PASS), (drop, vs.DETECTOR_FUSED)):
        e, cand, _ = D.candidates(img, mask)
        n = int(cand.sum())
        assert (n > C.KEY_CAP) == (used == vs.DETECTOR_TWO_PASS) and n >= C.KEY_CAP - 400, n
        md_ = mask_view(mask, cuda, "aligned")
        for mc, q, md in PARAMS:
            info = {}
            got = vs.good_features_mask(g, md_, mc, q, md, detector=vs.DETECTOR_AUTO, info=info)
            assert info["detector_used"] == used
            assert np.array_equal(got, D.select(e, cand, mc, md)), (used, mc)


# ---- the pipeline -----------------------------------------------------------------------------------------------------------------------
def run_product(vs, cuda, frames, mask, **cfg):
    import test_pipeline_gpu as P
    return P.run_product(vs, cuda, frames, detection_mask=mask, **cfg)


def check_against_state_machine(vs, cuda, frames, K, w, h, r, seed, mask, mask_arg, reference=None):
    """test_pipeline_gpu._check_against_oracle_state_machine with find_corners = the definition under `mask`; mask_arg is what the handle
    is given (a device tensor or a host array)"""
    stab, outs = run_product(vs, cuda, frames, mask_arg, smooth_radius=r, seed=seed)
    log = stab.frame_log()
    n = len(frames)
    assert len(outs) == max(n - 1, 0) and len(log) == max(n - 1, 0)
    Ko, (cw, ch) = oracle.get_output_camera(K, w, h)
    sm, exp, counts, warp_rots = reference or M.run_state_machine(frames, K, w, h, r, seed, lambda g: D.good_features(g, mask))
    assert [l["key"] for l in log] == [l["key"] for l in sm.log]
    assert [(l["n_corners"], l["n_tracked"]) for l in log] == counts
    assert [l["inliers"] for l in log] == [l["inliers"] for l in sm.log]
    assert all(np.allclose(a["R"], b["R"], atol=1e-9) for a, b in zip(log, sm.log))
    for i in range(len(outs)):
        assert np.allclose(stab.warp_rotation(i), warp_rots[i], atol=1e-9), i
        p = oracle.map_params(K, Ko, stab.warp_rotation(i))
        assert np.array_equal(outs[i], expect.warp(exp[i], p, cw, ch)), i
    return stab, log


def test_pipeline_overlay_clip_device_and_host_mask(vs, cuda):
    K, _, frames, _, mask = M.overlay_clip()
    w, h = 640, 360
    ref = M.run_state_machine(frames, K, w, h, 5, 5, lambda g: D.good_features(g, mask))
    _, log = check_against_state_machine(vs, cuda, frames, K, w, h, 5, 5, mask, dev(mask, cuda), ref)
    assert min(l["inliers"] for l in log) >= 40
    padded = np.full((h, w + 13), 255, np.uint8)
    padded[:, :w] = mask
    _, log2 = check_against_state_machine(vs, cuda, frames, K, w, h, 5, 5, mask, padded[:, :w], ref)
    assert [(l["key"], l["n_corners"], l["n_tracked"]) for l in log] == [(l["key"], l["n_corners"], l["n_tracked"]) for l in log2]
    # and the mask matters on this clip: a handle without it takes other corners
    import test_pipeline_gpu as P
    plain, _ = P.run_product(vs, cuda, frames, smooth_radius=5, seed=5)
    assert not all(np.array_equal(a["R"], b["R"]) for a, b in zip(plain.frame_log(), log))


def test_pipeline_planned_key_frame_is_detected_ahead_under_the_mask(vs, cuda):
    (w, h), frames, mask = M.planned_key_clip()
    K = oracle.get_preset_camera(4, w, h)
    stab, log = check_against_state_machine(vs, cuda, frames, K, w, h, 2, 1, mask, mask_view(mask, cuda, "odd_base"))
    c, prof = stab.detector_counters(), stab.profile()
    selections = prof["corner_selections_by_caller"] + prof["corner_selections_by_helper"]
    assert [k for k, l in enumerate(log) if l["key"]] == [20] and selections == 1           # the counter's key frame, detected ahead of time
    assert c["spec_over_cap"] == 0 and c["fused_overflows"] == 0
    assert min(l["n_tracked"] for l in log) >= 150
    # the corners of the planned key frame lie inside the mask: the speculative detection read it
    assert (D.good_features(frames[20][:h], mask)[:, 1] >= 70).all()


def test_pipeline_all_zero_and_full_masks(vs, cuda):
    w, h = 322, 182
    K = oracle.get_preset_camera(4, w, h)
    frames, _ = synth.shaky_clip(5, K, w, h, 9, sigma=0.004)
    zero = np.zeros((h, w), np.uint8)
    _, log = check_against_state_machine(vs, cuda, frames[:7], K, w, h, 2, 1, zero, dev(zero, cuda))
    assert len(log) == 6 and all(l["key"] and l["n_corners"] == 0 and l["fallback"] for l in log)
    import test_pipeline_gpu as P
    plain, outs0 = P.run_product(vs, cuda, frames, smooth_radius=3, seed=3)
    masked, outs = run_product(vs, cuda, frames, M.full(h, w, 3), smooth_radius=3, seed=3)
    key = lambda l: (l["key"], l["n_corners"], l["n_tracked"], l["inliers"], l["fallback"], l["R"].tobytes())
    assert [key(l) for l in plain.frame_log()] == [key(l) for l in masked.frame_log()] and any(l["n_corners"] > 0 for l in plain.frame_log())
    assert len(outs) == len(outs0) == 8 and all(np.array_equal(a, b) for a, b in zip(outs, outs0))


def test_pipeline_ten_bit_handle_takes_the_mask(vs, cuda):
    """a pixel_depth 10 handle's detector reads the luma narrowed to 8 bits: under the mask its rotations are those of the 8-bit handle on
    the truncated frames"""
    import torch
    K, _, frames8, _, mask = M.overlay_clip(n=8)
    n, r = len(frames8), 2
    rng = np.random.default_rng(8)
    wide = [((f.astype(np.uint16) << 8) | rng.integers(0, 256, f.shape, dtype=np.uint16)) for f in frames8]
    devw = [torch.from_numpy(x.view(np.int16)).to(cuda) for x in wide]
    ten = vs.Stabilizer(devw, total=n, bit_depth=10, smooth_radius=r, seed=3, pixel_depth=10, blend=vs.BLEND_EXACT, detection_mask=mask)
    cw, ch = ten.out_size
    pulls = 0
    while True:
        oy = torch.empty((ch, cw), dtype=torch.int16, device=cuda)
        ouv = torch.empty(((ch + 1) // 2, 2 * ((cw + 1) // 2)), dtype=torch.int16, device=cuda)
        if not ten.pull_p010_into(oy, ouv):
            break
        pulls += 1
    eight, _ = run_product(vs, cuda, frames8, mask, smooth_radius=r, seed=3)
    plain, _ = run_product(vs, cuda, frames8, None, smooth_radius=r, seed=3)
    key = lambda l: (l["key"], l["n_corners"], l["n_tracked"], l["inliers"], l["R"].tobytes())
    assert pulls == n - 1 and [key(l) for l in ten.frame_log()] == [key(l) for l in eight.frame_log()]
    assert [key(l) for l in plain.frame_log()] != [key(l) for l in eight.frame_log()]


def test_setter_refusals_that_need_a_handle(vs, cuda):
    import ctypes
    import torch
    w, h = 322, 182
    K = oracle.get_preset_camera(4, w, h)
    frames, _ = synth.shaky_clip(5, K, w, h, 4, sigma=0.004)
    devf = [torch.from_numpy(f).to(cuda) for f in frames]
    mask = dev(M.full(h, w), cuda)
    L = vs.lib

    def refused(stab, msg, ptr, pitch, mem):
        assert L.vstab_set_detection_mask(stab._h, ptr, pitch, mem) == vs.ERR_INVALID
        assert L.vstab_last_error().decode() == "vstab_set_detection_mask: " + msg

    off = vs.Stabilizer(devf, total=4, smooth_radius=1, tracking=0)
    refused(off, "no detector runs on this handle (tracking = 0)", mask.data_ptr(), w, 0)
    refused(off, "no detector runs on this handle (tracking = 0)", None, 0, 0)
    off.close()
    stab = vs.Stabilizer(devf, total=4, smooth_radius=1, seed=2)
    refused(stab, "the mask's pitch is smaller than the frame's width", mask.data_ptr(), w - 1, 0)
    refused(stab, "mem must be VSTAB_MEM_DEVICE (0) or VSTAB_MEM_HOST (1)", mask.data_ptr(), w, 2)
    refused(stab, "the mask's pitch is smaller than the frame's width", mask.data_ptr(), w - 1, 7)      # the pitch before mem
    # set, then clear with NULL (pitch and mem are not looked at): the handle is one without a mask again
    zero = np.zeros((h, w), np.uint8)
    stab.set_detection_mask(zero)
    assert L.vstab_set_detection_mask(stab._h, None, 0, 99) == 0
    outs = []
    while True:
        o = stab.pull()
        if o is None:
            break
        outs.append(o)
    assert len(outs) == 3 and all(l["n_corners"] > 0 for l in stab.frame_log())
    refused(stab, "the mask must be set before the first pull", mask.data_ptr(), w, 0)
    refused(stab, "the mask must be set before the first pull", None, 0, 0)
    stab.close()
    assert L.vstab_set_detection_mask(None, mask.data_ptr(), w, 0) == vs.ERR_INVALID
