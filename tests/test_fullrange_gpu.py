"""GPU parity of the 10-bit warps on full-range content and of the tracking kernels on maximum-contrast content (tests/fullrange.py).
The parameter sets are those whose reach test_fullrange_cpu.py commits to: saturating conversions, luma below 64 and binary16
accumulators at 1023.5 and above in every 10-bit kernel.  Bar: every word / byte / coordinate bit equals the oracle; nothing is
written around the output planes."""
import numpy as np
import pytest

import expect
import fullrange as F
import lk_segments as M
import oracle
from test_lk_segments_gpu import check_records

pytestmark = pytest.mark.gpu
CANARY = -21846   # 0xaaaa


def dev(a, cuda):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(cuda)


def host(t):
    return t.cpu().numpy().view(np.uint16)


def boxed(cuda, rows, cols, ch=None):
    """An output plane inside a canary frame (one row above and below, 2 samples left, 4 right): -> (frame, view)."""
    import torch
    shape = (rows + 2, cols + 6) + (() if ch is None else (ch,))
    b = torch.full(shape, CANARY, dtype=torch.int16, device=cuda)
    return b, b[1:rows + 1, 2:cols + 2]


def untouched(b, v):
    import torch
    m = torch.ones(b.shape[:2], dtype=torch.bool, device=b.device)
    m[1:v.shape[0] + 1, 2:v.shape[1] + 2] = False
    return bool((b[m] == CANARY).all())


def bgr16(vs, cuda, yd, ud, p, dw, dh, rb, mode, blend):
    b, v = boxed(cuda, dh, dw, 3)
    vs.warp_p010(yd, ud, p, dw, dh, rb, mode, blend, out=v)
    assert untouched(b, v)
    return host(v)


@pytest.mark.parametrize("name", list(F.SETS))
def test_warp_p010_full_range(vs, cuda, name):
    """vstab_warp_p010: the LDS-tiled kernel (modes 0 / 1 / 5, aligned planes; split_1280 / split_roll_1280 send boxes over the LDS
    budget to gather_pixel10), the direct kernel (modes 2 - 4; and the mode 0 sets again on planes that are not 16-byte aligned),
    both blends, the rotation per row where the set has one."""
    import torch
    y, uv, _, _, p, rb, dw, dh, mode = F.set_params(name)
    yd, ud = dev(y, cuda), dev(uv, cuda)
    for blend in (vs.BLEND_EXACT, vs.BLEND_FP16):
        exp = oracle.warp_p010(y, uv, p, dw, dh, rb, mode, blend)
        got = bgr16(vs, cuda, yd, ud, p, dw, dh, rb, mode, blend)
        assert np.array_equal(got, exp), (name, blend, int((got != exp).any(-1).sum()))
        if mode == 0 and y.shape[1] <= 640:
            # mode 5: the reference kernel's map arithmetic (tests/expect.py)
            got = bgr16(vs, cuda, yd, ud, p, dw, dh, rb, vs.MAP_CREATEMAP_CL_OPENCL, blend)
            assert np.array_equal(got, expect.warp_p010(y, uv, p, dw, dh, rb, blend, expect.OPENCL)), (name, "opencl", blend)
            # planes 8 bytes off a 16-byte boundary, padded pitches: the direct kernel
            h, w = y.shape
            Y = torch.zeros((h, w + 12), dtype=torch.int16, device=cuda)
            U = torch.zeros((h // 2, w + 8), dtype=torch.int16, device=cuda)
            Y[:, 4:w + 4], U[:, 4:w + 4] = yd, ud
            got = bgr16(vs, cuda, Y[:, 4:w + 4], U[:, 4:w + 4], p, dw, dh, rb, mode, blend)
            assert np.array_equal(got, exp), (name, "direct", blend)


@pytest.mark.parametrize("name", ["m0_640", "m0_640_rs", "m1_320_rs", "split_1280"])
def test_warp_p010_planes_full_range(vs, cuda, name):
    """vstab_warp_p010_planes (P010 out of the tiled kernel) = the oracle's warp, then its BGR -> P010; both blends."""
    y, uv, _, _, p, rb, dw, dh, mode = F.set_params(name)
    yd, ud = dev(y, cuda), dev(uv, cuda)
    cw = (dw + 1) // 2
    for blend in (vs.BLEND_EXACT, vs.BLEND_FP16):
        ey, euv = oracle.cvt_bgr10_p010(oracle.warp_p010(y, uv, p, dw, dh, rb, mode, blend))
        by, vy = boxed(cuda, dh, dw)
        bc, vc = boxed(cuda, (dh + 1) // 2, 2 * cw)
        vs.warp_p010_planes(yd, ud, p, dw, dh, rb, mode, blend, out_y=vy, out_uv=vc)
        assert np.array_equal(host(vy), ey) and np.array_equal(host(vc), euv), (name, blend)
        assert untouched(by, vy) and untouched(bc, vc)


def planar(vs, cuda, yd, ud, p, dw, dh, rb, blend):
    cw = (dw + 1) // 2
    by, vy = boxed(cuda, dh, dw)
    bc, vc = boxed(cuda, (dh + 1) // 2, 2 * cw)
    vs.warp_p010_planar(yd, ud, p, dw, dh, rb, vs.MAP_CREATEMAP_CL, blend, out_y=vy, out_uv=vc)
    assert untouched(by, vy) and untouched(bc, vc)
    return host(vy), host(vc)


@pytest.mark.parametrize("name", ["m0_640", "m0_640_rs", "split_1280", "split_roll_1280"])
def test_warp_p010_planar_full_range(vs, cuda, name):
    """vstab_warp_p010_planar: LDS-DMA tiles (m0_640*), split boxes and samples from global memory (split_*), both blends, the rotation
    per row; and the same frame on planes the 16-byte LDS-DMA cannot take."""
    import torch
    y, uv, _, _, p, rb, dw, dh, _ = F.set_params(name)
    yd, ud = dev(y, cuda), dev(uv, cuda)
    for blend in (0, 1):
        ey, euv = oracle.warp_p010_planar(y, uv, p, dw, dh, 0, rb, blend)
        gy, guv = planar(vs, cuda, yd, ud, p, dw, dh, rb, blend)
        assert np.array_equal(gy, ey) and np.array_equal(guv, euv), (name, blend, int((gy != ey).sum()), int((guv != euv).sum()))
        if name == "m0_640":
            h, w = y.shape
            rows, pitch = h * 3 // 2, w + 2
            buf = torch.zeros(rows * pitch + 64, dtype=torch.int16, device=cuda)
            view = buf[2:2 + rows * pitch].view(rows, pitch)[:, :w]
            view.copy_(dev(np.concatenate([y, uv]), cuda))
            gy, guv = planar(vs, cuda, view[:h], view[h:], p, dw, dh, rb, blend)
            assert np.array_equal(gy, ey) and np.array_equal(guv, euv), (name, "unaligned", blend)


def test_warp_p010_planar_full_range_4k(vs, cuda):
    w, h = 3840, 2160
    y, uv, y10, uv10 = F.p010_extreme_frame(51, w, h, block=32)
    K = oracle.get_preset_camera(4, w, h)
    Ko, (dw, dh) = oracle.get_output_camera(K, w, h)
    p = oracle.map_params(K, Ko, oracle.rodrigues((0.004, -0.002, 0.001)))
    rb = oracle.map_params(K, Ko, oracle.rodrigues((0.006, -0.001, 0.002)))[8:]
    gy, guv = planar(vs, cuda, dev(y, cuda), dev(uv, cuda), p, dw, dh, rb, 1)
    ey, euv = oracle.warp_p010_planar(y, uv, p, dw, dh, 0, rb, 1)
    assert np.array_equal(gy, ey) and np.array_equal(guv, euv), (int((gy != ey).sum()), int((guv != euv).sum()))
    q = F.reach_planar(y10, uv10, *oracle.create_map_rs(p, rb, dw, dh))
    assert q["clamp_y"] > 1000 and q["clamp_c"] > 1000, q


@pytest.mark.parametrize("pull", ["bgr16", "p010", "p010_planar"])
def test_pipeline_pulls_on_the_stretched_clip(vs, cuda, pull):
    """pixel_depth = 10 handles on the contrast-stretched clip (full-range luma and chroma): every frame of vstab_pull_frame_bgr16 /
    _p010 / _p010_planar against the oracle under the handle's rotation, both blends."""
    import torch
    W, H, n = 640, 360, 6
    K = oracle.get_preset_camera(4, W, H)
    Ko, (cw, ch) = oracle.get_output_camera(K, W, H)
    wide, _ = F.stretched_clip(3, K, W, H, n)
    frames = [dev(f, cuda) for f in wide]
    for blend in (vs.BLEND_EXACT, vs.BLEND_FP16):
        stab = vs.Stabilizer(frames, total=n, bit_depth=10, smooth_radius=2, seed=3, pixel_depth=10, blend=blend)
        for i in range(n - 1):
            y16, uv16 = wide[i + 1][:H], wide[i + 1][H:]
            if pull == "bgr16":
                o = torch.empty((ch, cw, 3), dtype=torch.int16, device=cuda)
                assert stab.pull_bgr16_into(o), i
                p = oracle.map_params(K, Ko, stab.warp_rotation(i))
                assert np.array_equal(host(o), expect.warp_p010(y16, uv16, p, cw, ch, None, blend)), (blend, i)
                continue
            oy = torch.empty((ch, cw), dtype=torch.int16, device=cuda)
            ouv = torch.empty(((ch + 1) // 2, 2 * ((cw + 1) // 2)), dtype=torch.int16, device=cuda)
            assert (stab.pull_p010_into if pull == "p010" else stab.pull_p010_planar_into)(oy, ouv), i
            p = oracle.map_params(K, Ko, stab.warp_rotation(i))
            if pull == "p010":
                ey, euv = oracle.cvt_bgr10_p010(expect.warp_p010(y16, uv16, p, cw, ch, None, blend))
            else:
                ey, euv = expect.warp_p010_planar(y16, uv16, p, cw, ch, None, blend)
            assert np.array_equal(host(oy), ey) and np.array_equal(host(ouv), euv), (pull, blend, i)
        assert len(stab.frame_log()) == n - 1 and min(l["inliers"] for l in stab.frame_log()) >= 20
        stab.close()


# ---- maximum-contrast tracking ---------------------------------------------------------------------------------------------------
SIZES = [(160, 120), (97, 71), (1920, 1080)]


def u8(a, cuda):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def test_pyramid_min_eig_and_detectors_on_contrast_images(vs, cuda):
    for kind in F.CONTRAST:
        for k, (w, h) in enumerate(SIZES):
            if w > 1000 and kind not in ("checker2", "steps"):
                continue
            img = F.contrast_image(kind, w, h, seed=k)
            d = u8(img, cuda)
            e1 = oracle.pyr_down(img)
            assert np.array_equal(vs.pyr_down(d).cpu().numpy(), e1), (kind, w)
            mid, dst = vs.pyr_down_x2(d)
            assert np.array_equal(mid.cpu().numpy(), e1) and np.array_equal(dst.cpu().numpy(), oracle.pyr_down(e1)), (kind, w)
            got, exp = vs.min_eig(d).cpu().numpy(), oracle.min_eig(img)
            assert np.array_equal(got.view(np.uint32), exp.view(np.uint32)), (kind, w)
            for mc, q, md in ((4000, 0.01, 0.0), (200, 0.01, 30.0)) if w < 1000 else ():   # (1080p plateaus: test_track_gpu)
                exp = oracle.good_features(img, mc, q, md)
                for det in (vs.DETECTOR_AUTO, vs.DETECTOR_TWO_PASS):
                    info = {}
                    got = vs.good_features(d, mc, q, md, detector=det, info=info)
                    assert np.array_equal(got, exp), (kind, w, mc, det, len(got), len(exp))
                    assert info["detector_used"] == (vs.DETECTOR_FUSED if det == vs.DETECTOR_AUTO else vs.DETECTOR_TWO_PASS), (kind, w, det)


def test_pyr_lk_on_contrast_pairs(vs, cuda):
    """Windows whose sum Ix^2 / sum diff Ix pass 2^31 (test_fullrange_cpu.py): statuses and every coordinate bit as the oracle's."""
    from test_fullrange_cpu import CONTRAST_PAIRS
    big = 0
    for kind in F.CONTRAST:
        for w, h, seed, shift in CONTRAST_PAIRS:
            prev, nxt, pts = F.contrast_pair(kind, w, h, seed, shift)
            exp, est, sums = oracle.pyr_lk_sums(prev, nxt, pts)
            got, gst = vs.pyr_lk(u8(prev, cuda), u8(nxt, cuda), pts)
            assert np.array_equal(gst, est), (kind, w, np.nonzero(gst != est)[0])
            ok = est > 0
            assert np.array_equal(got[ok].view(np.uint32), exp[ok].view(np.uint32)), (kind, w, np.nonzero((got != exp).any(1) & ok)[0])
            assert np.array_equal(got.view(np.uint32), exp.view(np.uint32)), (kind, w, "status 0")
            big += int(((sums >= 2 ** 31).any(1) & ok).sum())
    assert big >= 50


@pytest.mark.parametrize("kind", ["checker3", "checker4", "steps", "rects"])
def test_lk_segments_on_contrast_clips(vs, cuda, kind):
    """Multi-pair launches (k_lk_track with fi > 0) and chained launches on a clip of a contrast image moving by sub-pixel steps."""
    w, h, K = 160, 120, 4
    prev, _, pts = F.contrast_pair(kind, w, h, 3, (0.0, 0.0))
    import synth
    frames = [prev] + [synth.shifted(prev, 0.43 * k, -0.29 * k) for k in range(1, K + 1)]
    exp = M.expected(frames, pts, [K])
    df = [u8(f, cuda) for f in frames]
    recs = []
    for segs in ([K], [1] * K, [1, 3]):
        hrec, drec, _ = vs.lk_segments(df, pts, segs)
        check_records(exp, hrec, drec, (kind, segs))
        recs.append(hrec)
    assert all(np.array_equal(r, recs[0]) for r in recs[1:]), kind
    assert (exp["status"] == 1).sum() >= 20
