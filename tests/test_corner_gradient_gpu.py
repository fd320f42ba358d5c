"""GPU half of the corner-gradient tests (include/vstab.h, "Corner gradient size"): vstab_min_eig_grad / vstab_corner_harris_grad against the
definition bit for bit for the six new pairs of block and gradient size, vstab_good_features_grad with its three detectors, the raw output
of k_corners_fused_block<B, G> + k_filter_keys (test hook vstabx_corners_fused_grad), the two-pass fall-back and a handle with
vstab_set_corner_gradient, against tests/corner_def.py.  Every comparison is exact (rotations: the 1e-9 of test_pipeline_gpu.py)."""
import numpy as np
import pytest

import corner_def as D
import corner_tiles as C
import mask_def as M
import oracle
from test_detection_mask_gpu import FILL, LAYOUTS, PARAMS, dev, mask_view
from test_harris_gpu import host_half, masks_for

pytestmark = pytest.mark.gpu

KS = (0.0, 0.04, 0.2)
RESPONSES = (False, True)
FULL_PAIRS = ((3, 5), (7, 7))                                         # the whole matrix of masks, layouts and detectors; the raw hook
LEAN_PAIRS = tuple(p for p in D.NEW_PAIRS if p not in FULL_PAIRS)     # DETECTOR_AUTO, no mask
pair_id = lambda p: f"b{p[0]}g{p[1]}"


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def check_dense(vs, gd, g, block, gradient, what):
    sums = D.covariance_sums(g, block, gradient)
    got = vs.min_eig_grad(gd, block, gradient).cpu().numpy()
    assert np.array_equal(bits(got), bits(D.min_eig_from_sums(*sums))), (what, block, gradient, "min_eig")
    for k in KS:
        got = vs.corner_harris_grad(gd, block, gradient, k).cpu().numpy()
        assert np.array_equal(bits(got), bits(D.response_from_sums(*sums, k))), (what, block, gradient, k)


# ---- the dense maps ---------------------------------------------------------------------------------------------------------------------
# 3 x 3 and 4 x 5: a reach of up to 7 folds a 3-pixel axis several times; 65 x 32 and 66 x 33 are the tile seams; 322 x 182 has interior
# tiles; dark_noise has double sums that are not exact (for block 3 too).  interior_edge: tile (1, 1)'s source box ends exactly on the
# image's last byte (the kernel's interior path, tile_interior); interior_edge_less_h: one row less, that tile takes the border path on
# dword-aligned rows; interior_edge_less_w: one column less (rows that are no longer dword aligned: every tile takes its byte loads).
@pytest.mark.parametrize("pair", D.NEW_PAIRS, ids=pair_id)
@pytest.mark.parametrize("name", ["3x3", "4x5", "65x32", "66x33", "322x182", "dark_noise", "interior_edge", "interior_edge_less_w", "interior_edge_less_h"])
def test_dense_maps_are_the_definition(vs, cuda, name, pair):
    g = D.dense_frames(*pair)[name]
    check_dense(vs, dev(g, cuda), g, *pair, name)


@pytest.mark.parametrize("pair", D.NEW_PAIRS, ids=pair_id)
def test_dense_maps_byte_path(vs, cuda, pair):
    """129 x 63 with a pitch above the width from an odd base address: no dword loads"""
    import torch
    w, h, pitch = 129, 63, 141
    g = D.dense_frames(*pair)["129x63"]
    buf = torch.zeros(pitch * h + 8, dtype=torch.uint8, device=cuda)
    v = buf[1:1 + pitch * h].view(h, pitch)[:, :w]
    v.copy_(torch.from_numpy(np.ascontiguousarray(g)).to(cuda))
    assert v.data_ptr() % 2 == 1 and v.stride(0) == pitch
    check_dense(vs, v, g, *pair, "byte path")


@pytest.mark.parametrize("block", D.BLOCKS)
def test_gradient_3_through_the_new_names(vs, cuda, block):
    """gradient_size 3: the bytes of the _block twins, through all three stateless names"""
    for name in ("66x33", "322x182"):
        g = D.dense_frames(block, 5)[name]
        gd = dev(g, cuda)
        assert np.array_equal(bits(vs.min_eig_grad(gd, block, 3).cpu().numpy()), bits(vs.min_eig_block(gd, block).cpu().numpy()))
        for k in KS:
            assert np.array_equal(bits(vs.corner_harris_grad(gd, block, 3, k).cpu().numpy()), bits(vs.corner_harris_block(gd, block, k).cpu().numpy()))
        assert np.array_equal(bits(vs.min_eig_grad(gd, block, 3).cpu().numpy()), bits(D.min_eig(g, block, 3)))
    g = D.frame("luma_322x182")
    gd = dev(g, cuda)
    full = mask_view(M.full(*g.shape), cuda, "aligned")
    for det in (vs.DETECTOR_AUTO, vs.DETECTOR_FUSED, vs.DETECTOR_TWO_PASS):
        for mask, harris in ((None, False), (full, True)):
            got = vs.good_features_grad(gd, mask, 200, 0.01, 30.0, block, 3, harris, 0.04 if harris else float("nan"), detector=det)    # k is not looked at
            assert len(got) > 0 and np.array_equal(got, vs.good_features_block(gd, mask, 200, 0.01, 30.0, block, harris, 0.04, detector=det))


# ---- the stateless detector ----------------------------------------------------------------------------------------------------------------
def check_stateless(vs, cuda, g, mask, what, block, gradient, harris, detectors, k=D.K_DEFAULT):
    gd = dev(g, cuda)
    e, cand, _ = D.candidates(g, mask, 0.01, block, gradient, harris, k)
    exp = [D.select(e, cand, mc, md) for mc, _, md in PARAMS]
    for layout in LAYOUTS if mask is not None else ("none",):
        md_ = None if mask is None else mask_view(mask, cuda, layout)
        for det in detectors:
            for (mc, q, md), want in zip(PARAMS, exp):
                info = {}
                got = vs.good_features_grad(gd, md_, mc, q, md, block, gradient, harris, k, detector=det, info=info)
                assert np.array_equal(got, want), (what, block, gradient, harris, layout, det, mc, len(got), len(want))
                assert info["detector_used"] == (vs.DETECTOR_TWO_PASS if det == vs.DETECTOR_TWO_PASS else vs.DETECTOR_FUSED)
    return [len(x) for x in exp]


@pytest.mark.parametrize("harris", RESPONSES)
@pytest.mark.parametrize("pair", FULL_PAIRS, ids=pair_id)
@pytest.mark.parametrize("name", D.STATELESS_FRAMES)
def test_stateless_all_detectors_against_the_definition(vs, cuda, name, pair, harris):
    g = D.frame(name)
    total = 0
    for what, mask in masks_for(g).items():
        n = check_stateless(vs, cuda, g, mask, what, *pair, harris, (vs.DETECTOR_AUTO, vs.DETECTOR_FUSED, vs.DETECTOR_TWO_PASS))
        print(name, pair, harris, what, "corners", n)
        total += n[0]
        if what == "zero":
            assert n == [0, 0]
    assert total > 0


@pytest.mark.parametrize("pair", LEAN_PAIRS, ids=pair_id)
def test_stateless_other_pairs(vs, cuda, pair):
    for name in D.STATELESS_FRAMES:
        for harris in RESPONSES:
            n = check_stateless(vs, cuda, D.frame(name), None, "none", *pair, harris, (vs.DETECTOR_AUTO,))
            print(name, pair, harris, "corners", n)


def test_gradient_sizes_separate(vs, cuda):
    g = D.textured_frame()
    pairs = [(b, G) for G in D.GRADIENTS for b in (3, 7)]
    got = [vs.good_features_grad(dev(g, cuda), None, block_size=b, gradient_size=G) for b, G in pairs]
    for (b, G), x in zip(pairs, got):
        assert np.array_equal(x, D.good_features(g, block=b, gradient=G)), (b, G)
    assert all(not np.array_equal(got[i], got[j]) for i in range(len(got)) for j in range(i + 1, len(got)))


# ---- the raw hook ---------------------------------------------------------------------------------------------------------------------------
def check_raw(vs, cuda, m, mask_dev=None):
    """test_corner_block_gpu.check_raw through vstabx_corners_fused_grad"""
    g = dev(m.img, cuda)
    response = vs.CORNER_HARRIS if m.harris else vs.CORNER_MIN_EIGENVAL
    if not m.positive:
        # rule 4: nothing of what the kernels leave counts; a key buffer of a modest size must still be respected
        assert m.harris
        keys, kept, spilled, tiles, max_bits = vs.corners_fused_grad(g, mask_dev, m.block, m.gradient, response, m.k, m.quality, cap=1024, canary=64)
        assert max_bits < 0
        assert (keys[min(kept, 1024):] == FILL).all()
        assert m.frame_max < 0 and np.array_equal(tiles, m.hi)          # every tile filters with -inf: all of its masked-in 3 x 3 maxima
        assert len(host_half(vs, m, keys, kept, max_bits, 200, 30.0)) == 0
        return
    keys, kept, spilled, tiles, max_bits = vs.corners_fused_grad(g, mask_dev, m.block, m.gradient, response, m.k, m.quality, cap=m.n + 7, canary=64)
    print(f"{m.w} x {m.h} block {m.block} gradient {m.gradient} harris {m.harris}: kept {kept} (model {m.n}), spilled {spilled} (model {m.spilled_range()}), "
          f"negative tiles {int(m.negative.sum())}, early tiles {int(m.early.sum())}")
    assert max_bits >= 0 and np.int32(max_bits).view(np.float32) == m.frame_max
    assert kept == m.n
    assert (keys[kept:] == FILL).all()                               # nothing written past the keys: the tail of the buffer and the canary
    assert np.array_equal(np.sort(keys[:kept]), m.keys)
    assert tiles.shape == m.lo.shape and (tiles >= m.lo).all() and (tiles <= m.hi).all()
    assert not tiles[m.early].any()                                  # an early tile wrote its count of zero over the fill
    lo, hi = m.spilled_range()
    assert lo <= spilled <= hi and spilled == int((tiles > C.SLOTS).sum())
    for mc, q, md in PARAMS:
        assert np.array_equal(host_half(vs, m, keys, kept, max_bits, mc, md), m.corners(mc, md))


@pytest.mark.parametrize("pair", FULL_PAIRS, ids=pair_id)
@pytest.mark.parametrize("name", D.RAW_FRAMES)
def test_raw_output_against_the_model(vs, cuda, name, pair):
    for harris in RESPONSES:
        if harris or name in D.RAW_FRAMES_MIN_EIG:
            m = D.raw_model(name, *pair, harris)
            if harris and name in D.NON_POSITIVE:
                assert not m.positive                                 # the Harris frames whose maximum is not positive
            check_raw(vs, cuda, m)


@pytest.mark.parametrize("pair", FULL_PAIRS, ids=pair_id)
def test_raw_output_under_a_mask(vs, cuda, pair):
    """tiles that return early beside tiles that keep keys"""
    for harris in RESPONSES:
        m = D.raw_masked_model("grid_7x5_tiles_off", *pair, harris)
        assert m.early.any() and m.positive and m.n > 0
        for layout in LAYOUTS:
            check_raw(vs, cuda, m, mask_view(m.mask, cuda, layout))


@pytest.mark.parametrize("pair,harris", [((3, 5), True), ((5, 7), False)], ids=lambda p: str(p))
def test_two_pass_fall_back(vs, cuda, pair, harris):
    """more candidates than the key buffer holds: the one-pass detector hands over to the new dense kernels"""
    g = D.fall_back_frame()
    e, cand, _ = D.candidates(g, None, 0.01, *pair, harris)
    assert int(cand.sum()) > C.KEY_CAP
    for mc, q, md in PARAMS:
        info = {}
        got = vs.good_features_grad(dev(g, cuda), None, mc, q, md, *pair, harris, detector=vs.DETECTOR_AUTO, info=info)
        assert info["detector_used"] == vs.DETECTOR_TWO_PASS
        assert np.array_equal(got, D.select(e, cand, mc, md)), mc


# ---- the pipeline -----------------------------------------------------------------------------------------------------------------------
def check_against_state_machine(vs, cuda, frames, K, w, h, r, seed, block, gradient, mask=None, harris=False, k=D.K_DEFAULT):
    """test_corner_block_gpu.check_against_state_machine with find = corner_def.good_features at a pair of sizes"""
    import expect
    import test_pipeline_gpu as P
    cfg = dict(smooth_radius=r, seed=seed, corner_gradient=gradient)
    if block is not None:
        cfg["corner_block"] = block
    if mask is not None:
        cfg["detection_mask"] = dev(mask, cuda)
    if harris:
        cfg.update(corner_response=vs.CORNER_HARRIS, harris_k=k)
    stab, outs = P.run_product(vs, cuda, frames, **cfg)
    log = stab.frame_log()
    n = len(frames)
    assert len(outs) == max(n - 1, 0) and len(log) == max(n - 1, 0)
    Ko, (cw, ch) = oracle.get_output_camera(K, w, h)
    find = lambda g: D.good_features(g, mask, block=3 if block is None else block, gradient=gradient, harris=harris, k=k)
    sm, exp, counts, warp_rots = M.run_state_machine(frames, K, w, h, r, seed, find)
    assert [l["key"] for l in log] == [l["key"] for l in sm.log]
    assert [(l["n_corners"], l["n_tracked"]) for l in log] == counts
    assert [l["inliers"] for l in log] == [l["inliers"] for l in sm.log]
    assert all(np.allclose(a["R"], b["R"], atol=1e-9) for a, b in zip(log, sm.log))
    for i in range(len(outs)):
        assert np.allclose(stab.warp_rotation(i), warp_rots[i], atol=1e-9), i
        p = oracle.map_params(K, Ko, stab.warp_rotation(i))
        assert np.array_equal(outs[i], expect.warp(exp[i], p, cw, ch)), i
    return stab, log


LOG_KEY = lambda l: (l["key"], l["n_corners"], l["n_tracked"], l["inliers"], l["fallback"], l["R"].tobytes())


@pytest.mark.parametrize("block,gradient,masked_harris", [(None, 5, False), (7, 7, True)])
def test_pipeline_overlay_clip(vs, cuda, block, gradient, masked_harris):
    """the overlay clip with gradient 5 alone and with gradient 7 beside block 7, the latter under the mask with the Harris response"""
    import test_pipeline_gpu as P
    K, _, frames, _, mask = M.overlay_clip()
    _, log = check_against_state_machine(vs, cuda, frames, K, 640, 360, 5, 5, block, gradient, mask if masked_harris else None, masked_harris)
    if not masked_harris:
        plain, _ = P.run_product(vs, cuda, frames, smooth_radius=5, seed=5)
        assert [LOG_KEY(l) for l in plain.frame_log()] != [LOG_KEY(l) for l in log]          # a log at gradient 5 differs from the plain one


def test_pipeline_ten_bit_handle(vs, cuda):
    """a pixel_depth 10 handle's detector reads the luma narrowed to 8 bits: at gradient 5 its frame log is that of the 8-bit handle on the
    truncated frames"""
    import torch
    import test_pipeline_gpu as P
    K, _, frames8, _, mask = M.overlay_clip(n=8)
    n, r = len(frames8), 2
    rng = np.random.default_rng(8)
    wide = [((f.astype(np.uint16) << 8) | rng.integers(0, 256, f.shape, dtype=np.uint16)) for f in frames8]
    devw = [torch.from_numpy(x.view(np.int16)).to(cuda) for x in wide]
    ten = vs.Stabilizer(devw, total=n, bit_depth=10, smooth_radius=r, seed=3, pixel_depth=10, blend=vs.BLEND_EXACT, corner_gradient=5)
    cw, ch = ten.out_size
    pulls = 0
    while True:
        oy = torch.empty((ch, cw), dtype=torch.int16, device=cuda)
        ouv = torch.empty(((ch + 1) // 2, 2 * ((cw + 1) // 2)), dtype=torch.int16, device=cuda)
        if not ten.pull_p010_into(oy, ouv):
            break
        pulls += 1
    eight, _ = P.run_product(vs, cuda, frames8, smooth_radius=r, seed=3, corner_gradient=5)
    plain, _ = P.run_product(vs, cuda, frames8, smooth_radius=r, seed=3)
    key = lambda l: (l["key"], l["n_corners"], l["n_tracked"], l["inliers"], l["R"].tobytes())
    assert pulls == n - 1 and [key(l) for l in ten.frame_log()] == [key(l) for l in eight.frame_log()]
    assert [key(l) for l in plain.frame_log()] != [key(l) for l in eight.frame_log()]


def _short_clip(cuda):
    import synth
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


def test_reset_to_gradient_3(vs, cuda):
    """7, then 3 before the first pull: the plain handle's log and output bytes"""
    w, h, frames, devf = _short_clip(cuda)
    plain = vs.Stabilizer(devf, total=len(devf), smooth_radius=1, seed=2)
    outs0 = _drain(plain)
    stab = vs.Stabilizer(devf, total=len(devf), smooth_radius=1, seed=2, corner_gradient=7)
    stab.set_corner_gradient(3)
    outs = _drain(stab)
    seven = vs.Stabilizer(devf, total=len(devf), smooth_radius=1, seed=2, corner_gradient=7)
    _drain(seven)
    assert [LOG_KEY(l) for l in plain.frame_log()] == [LOG_KEY(l) for l in stab.frame_log()] and any(l["n_corners"] > 0 for l in plain.frame_log())
    assert len(outs) == len(outs0) == len(devf) - 1 and all(np.array_equal(a, b) for a, b in zip(outs, outs0))
    assert [LOG_KEY(l) for l in plain.frame_log()] != [LOG_KEY(l) for l in seven.frame_log()]


def test_setter_in_any_order_with_block_response_and_mask(vs, cuda):
    """gradient, block, response and mask are independent: every order of the four setters gives the same log"""
    w, h, frames, devf = _short_clip(cuda)
    mask = M.overlay_box(h, w)
    logs = []
    for order in ("gbmr", "rbmg", "mgrb"):
        stab = vs.Stabilizer(devf, total=len(devf), smooth_radius=1, seed=2)
        for s in order:
            {"g": lambda: stab.set_corner_gradient(5), "b": lambda: stab.set_corner_block(7), "m": lambda: stab.set_detection_mask(dev(mask, cuda)),
             "r": lambda: stab.set_corner_response(vs.CORNER_HARRIS, 0.06)}[s]()
        _drain(stab)
        logs.append([LOG_KEY(l) for l in stab.frame_log()])
    assert logs[0] == logs[1] == logs[2]
    want = D.good_features(frames[0][:h], mask, block=7, gradient=5, harris=True, k=0.06)
    assert stab.frame_log()[0]["n_corners"] == len(want) > 0


def test_setter_refusals_that_need_a_handle(vs, cuda):
    w, h, frames, devf = _short_clip(cuda)
    L = vs.lib

    def refused(stab, msg, gradient):
        assert L.vstab_set_corner_gradient(stab._h, gradient) == vs.ERR_INVALID
        assert L.vstab_last_error().decode() == "vstab_set_corner_gradient: " + msg

    off = vs.Stabilizer(devf, total=4, smooth_radius=1, tracking=0)
    refused(off, "no detector runs on this handle (tracking = 0)", 5)
    refused(off, "no detector runs on this handle (tracking = 0)", 4)                               # before the gradient size
    off.close()
    stab = vs.Stabilizer(devf, total=4, smooth_radius=1, seed=2)
    for gradient in (-1, 0, 1, 2, 4, 6, 8, 9, -5):
        refused(stab, "gradient_size is 3, 5 or 7", gradient)
    # a refused call leaves the handle unchanged: still the plain handle
    plain = vs.Stabilizer(devf, total=4, smooth_radius=1, seed=2)
    _drain(plain)
    assert len(_drain(stab)) == 3
    assert [LOG_KEY(l) for l in stab.frame_log()] == [LOG_KEY(l) for l in plain.frame_log()]
    refused(stab, "the gradient size must be set before the first pull", 5)
    refused(stab, "the gradient size must be set before the first pull", 4)                         # before the gradient size
    stab.close()
    assert L.vstab_set_corner_gradient(None, 5) == vs.ERR_INVALID
    assert L.vstab_last_error().decode() == "vstab_set_corner_gradient: null handle"
