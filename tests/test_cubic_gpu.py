"""GPU parity of the bicubic resampler (cv::remap INTER_CUBIC; include/vstab.h "Bicubic resampling") through the C ABI and the pipeline
object: vstab_remap_cubic, vstab_warp_nv12_cubic (BGR8 and plane-wise NV12) and vstab_config.resample.  Bar: every byte equals the numpy
definition (tests/warp_def.py) fed by the oracle's maps -- the reference kernel's own map, run on this GPU, for VSTAB_MAP_CREATEMAP_CL_OPENCL."""
import numpy as np
import pytest

import expect
import oracle
import synth
import warp_def as wd

pytestmark = pytest.mark.gpu

ROTS = [(0.0, 0.0, 0.0), (0.02, -0.03, 0.01), (-0.15, 0.1, 0.3)]
PAST = (0.6, -0.4, 0.2)   # looks past the source: large border areas, footprints straddling every edge


def dev(a, cuda):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def cams(w, h, rvec, preset=4):
    K = oracle.get_preset_camera(preset, w, h)
    Ko, (dw, dh) = oracle.get_output_camera(K, w, h)
    return oracle.map_params(K, Ko, oracle.rodrigues(rvec)), dw, dh


def special_maps(rng, sw, sh, dw, dh):
    mx = rng.uniform(-4.0, sw + 3.0, (dh, dw)).astype(np.float32)
    my = rng.uniform(-4.0, sh + 3.0, (dh, dw)).astype(np.float32)
    sel = rng.random((dh, dw)) < 0.2   # exact 1/64-pixel ties of the 1/32 quantisation
    mx[sel] = ((rng.integers(-128, 32 * sw + 128, int(sel.sum())) + 0.5) / 32.0).astype(np.float32)
    my[sel] = ((rng.integers(-128, 32 * sh + 128, int(sel.sum())) + 0.5) / 32.0).astype(np.float32)
    special = np.array([np.nan, np.inf, -np.inf, 1e9, -1e9, 2147483520.0, -2147483648.0, 5e9, -0.0], np.float32)
    for m in (mx, my):
        pick = rng.random((dh, dw)) < 0.05
        m[pick] = rng.choice(special, int(pick.sum()))
    return mx, my


def gpu_remap(vs, cuda, src, mx, my, border):
    return vs.remap_cubic(dev(src, cuda), dev(mx, cuda), dev(my, cuda), border).cpu().numpy()


def test_remap_cubic_matches_definition(vs, cuda):
    rng = np.random.default_rng(5)
    for (sw, sh) in [(1, 1), (3, 3), (2, 7), (37, 21), (300, 170)]:
        for cn, border in ((1, (16,)), (2, (128, 128)), (3, (0, 9, 255))):
            src = rng.integers(0, 256, (sh, sw, cn) if cn > 1 else (sh, sw), dtype=np.uint8)
            dw, dh = (71, 33) if sw < 100 else (333, 190)
            mx, my = special_maps(rng, sw, sh, dw, dh)
            got = gpu_remap(vs, cuda, src, mx, my, border)
            exp = wd.remap(src, mx, my, "cubic", wd.CONSTANT, border)
            assert np.array_equal(got, exp), (sw, sh, cn, int((got != exp).sum()))


def test_remap_cubic_golden_vectors(vs, cuda):
    import os
    kat = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cubic_kat.npz"))
    k = 0
    while f"case{k}_src" in kat:
        got = gpu_remap(vs, cuda, kat[f"case{k}_src"], kat[f"case{k}_mapx"], kat[f"case{k}_mapy"], tuple(int(b) for b in kat[f"case{k}_border"]))
        assert np.array_equal(got, kat[f"case{k}_out"]), k
        k += 1


def test_remap_cubic_refuses_bad_arguments(vs, cuda):
    import torch
    src = torch.zeros((8, 8), dtype=torch.uint8, device=cuda)
    m = torch.zeros((4, 4), dtype=torch.float32, device=cuda)
    with pytest.raises(vs.VstabError):
        vs.remap_cubic(src, m, m, (300,))
    with pytest.raises(vs.VstabError):
        vs.remap_cubic(torch.zeros((8, 8, 4), dtype=torch.uint8, device=cuda), m, m)


def run_bgr(vs, cuda, f, p, dw, dh, mode, pad=0):
    import torch
    buf = torch.full((dh, dw * 3 + pad), 7, dtype=torch.uint8, device=cuda)
    out = buf[:, : dw * 3].view(dh, dw, 3)
    vs.warp_nv12_cubic(dev(f, cuda), p, dw, dh, mode, vs.OUT_BGR8, out=out)
    if pad:
        assert bool((buf[:, dw * 3:] == 7).all())   # nothing written past a row
    return out.cpu().numpy()


def run_planar(vs, cuda, f, p, dw, dh, mode, pad=0):
    import torch
    cw = (dw + 1) // 2
    yb = torch.full((dh, dw + pad), 7, dtype=torch.uint8, device=cuda)
    cb = torch.full(((dh + 1) // 2, 2 * cw + pad), 7, dtype=torch.uint8, device=cuda)
    yv, cv = yb[:, :dw], cb[:, : 2 * cw]
    vs.warp_nv12_cubic(dev(f, cuda), p, dw, dh, mode, vs.OUT_NV12_PLANAR, out=(yv, cv))
    if pad:
        assert bool((yb[:, dw:] == 7).all()) and bool((cb[:, 2 * cw:] == 7).all())
    return yv.cpu().numpy(), cv.cpu().numpy()


def check(vs, cuda, f, p, dw, dh, mode, pad=0, planar=True):
    got = run_bgr(vs, cuda, f, p, dw, dh, mode, pad)
    exp = wd.bgr(f, *wd.maps(p, dw, dh, mode), "cubic")
    assert np.array_equal(got, exp), ("bgr", mode, dw, dh, int((got != exp).sum()))
    if planar:
        gy, guv = run_planar(vs, cuda, f, p, dw, dh, mode, pad)
        ey, euv = wd.planar(f, *wd.maps(p, dw, dh, mode), "cubic")
        assert np.array_equal(gy, ey), ("luma", mode, dw, dh, int((gy != ey).sum()))
        assert np.array_equal(guv, euv), ("chroma", mode, dw, dh, int((guv != euv).sum()))


def test_warp_cubic_sizes_and_rotations(vs, cuda):
    for (w, h) in [(128, 72), (320, 180), (640, 368), (1920, 1080)]:
        f = synth.nv12(w + 3 * h, w, h, full_range=(w < 1000))
        for rv in (ROTS + [PAST] if w < 1000 else ROTS[1:2]):
            p, dw, dh = cams(w, h, rv)
            sizes = [(dw, dh), (dw - 1, dh - 3)] if w < 1000 else [(dw, dh)]
            for (ow, oh) in sizes:
                check(vs, cuda, f, p, ow, oh, vs.MAP_CREATEMAP_CL, pad=(16 if w == 320 else 0))


def test_warp_cubic_4k_config3_shape(vs, cuda):
    w, h = 3840, 2160
    f = synth.nv12(77, w, h)
    p, dw, dh = cams(w, h, (0.01, -0.02, 0.015))
    assert (dw, dh) == (3524, 1999)
    check(vs, cuda, f, p, dw, dh, vs.MAP_CREATEMAP_CL)


def test_warp_cubic_every_projection_pair(vs, cuda):
    w, h, dw, dh = 640, 360, 481, 271
    f = synth.nv12(9, w, h, full_range=True)
    lenses = [(oracle.PROJ_FISH, 150.0, oracle.PROJ_RECT, 110.0), (oracle.PROJ_FISH, 150.0, oracle.PROJ_FISH, 165.0),
              (oracle.PROJ_RECT, 100.0, oracle.PROJ_RECT, 80.0), (oracle.PROJ_RECT, 100.0, oracle.PROJ_FISH, 300.0)]
    for ip, ifov, op, ofov in lenses:
        Kin, Kout = oracle.lens_camera(ip, ifov, w, h), oracle.lens_camera(op, ofov, dw, dh)
        mode = oracle.map_mode(ip, op)
        for rv in ROTS[1:] + [(0.0, 1.2, 0.0)]:
            check(vs, cuda, f, oracle.map_params(Kin, Kout, oracle.rodrigues(rv)), dw, dh, mode)


def test_warp_cubic_reference_kernel_map(vs, cuda):
    if not oracle.ref_gfx950_available():
        pytest.skip("oracle/_ref/createMap.gfx950.co not built")
    for (w, h) in [(640, 360), (1920, 1080)]:
        f = synth.nv12(w, w, h)
        for rv in ROTS[1:]:
            p, dw, dh = cams(w, h, rv)
            check(vs, cuda, f, p, dw, dh, vs.MAP_CREATEMAP_CL_OPENCL)


def test_warp_cubic_unaligned_and_pitched_planes(vs, cuda):
    """A luma plane at an odd address with an odd pitch, a chroma plane of its own at an even address with another pitch, and a packed
    frame at a 2-byte offset: the kernels read the planes byte by byte (chroma as aligned pairs) whatever their alignment."""
    import ctypes
    import torch
    w, h = 320, 180
    f = synth.nv12(31, w, h)
    p, dw, dh = cams(w, h, ROTS[1])
    exp_bgr = wd.bgr(f, *wd.maps(p, dw, dh, 0), "cubic")
    ey, euv = wd.planar(f, *wd.maps(p, dw, dh, 0), "cubic")
    # separate planes through the C ABI: luma at offset 1, pitch w + 37; chroma at offset 6, pitch w + 14
    py, puv = w + 37, w + 14
    ybuf = torch.zeros(h * py + 64, dtype=torch.uint8, device=cuda)
    cbuf = torch.zeros((h // 2) * puv + 64, dtype=torch.uint8, device=cuda)
    yv = ybuf[1: 1 + h * py].view(h, py)[:, :w]
    cv = cbuf[6: 6 + (h // 2) * puv].view(h // 2, puv)[:, :w]
    yv.copy_(dev(f[:h], cuda))
    cv.copy_(dev(f[h:], cuda))
    assert yv.data_ptr() % 2 == 1 and cv.data_ptr() % 2 == 0
    pa = np.ascontiguousarray(p, np.float32)
    fp = pa.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    out = torch.empty((dh, dw, 3), dtype=torch.uint8, device=cuda)
    assert vs.lib.vstab_warp_nv12_cubic(yv.data_ptr(), py, cv.data_ptr(), puv, w, h, fp, 0, vs.OUT_BGR8, out.data_ptr(), out.stride(0), None, 0,
                                        dw, dh, vs._stream()) == vs.OK
    oy, ouv = vs.nv12_out_planes(dw, dh, cuda)
    assert vs.lib.vstab_warp_nv12_cubic(yv.data_ptr(), py, cv.data_ptr(), puv, w, h, fp, 0, vs.OUT_NV12_PLANAR, oy.data_ptr(), oy.stride(0),
                                        ouv.data_ptr(), ouv.stride(0), dw, dh, vs._stream()) == vs.OK
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), exp_bgr)
    assert np.array_equal(oy.cpu().numpy(), ey) and np.array_equal(ouv.cpu().numpy(), euv)
    # a packed frame at a 2-byte offset with a pitch that is no multiple of 4
    pitch2 = w + 38
    buf2 = torch.zeros((h * 3 // 2) * pitch2 + 64, dtype=torch.uint8, device=cuda)
    view2 = buf2[2: 2 + (h * 3 // 2) * pitch2].view(h * 3 // 2, pitch2)[:, :w]
    view2.copy_(dev(f, cuda))
    assert np.array_equal(vs.warp_nv12_cubic(view2, p, dw, dh, vs.MAP_CREATEMAP_CL, vs.OUT_BGR8).cpu().numpy(), exp_bgr)
    gy, guv = vs.warp_nv12_cubic(view2, p, dw, dh, vs.MAP_CREATEMAP_CL, vs.OUT_NV12_PLANAR)
    assert np.array_equal(gy.cpu().numpy(), ey) and np.array_equal(guv.cpu().numpy(), euv)
    # a packed frame with an odd pitch puts the chroma plane at an odd address: refused, not misread
    pitch = w + 37
    buf = torch.zeros((h * 3 // 2) * pitch + 64, dtype=torch.uint8, device=cuda)
    view = buf[1: 1 + (h * 3 // 2) * pitch].view(h * 3 // 2, pitch)[:, :w]
    view.copy_(dev(f, cuda))
    with pytest.raises(vs.VstabError):
        vs.warp_nv12_cubic(view, p, dw, dh, vs.MAP_CREATEMAP_CL, vs.OUT_BGR8)


def test_warp_cubic_extreme_box_shapes(vs, cuda):
    """Wide flat and tall narrow source boxes (anisotropic cameras).  The BGR tiles of the 2048 x 32 and 4096 x 64 sets are over the
    LDS budget and sampled from global memory; every luma and chroma tile, and every tile of the 64 x 1024 set, is staged
    (tests/test_cubic_tiles_cpu.py counts them; test_cubic_paths_gpu.py has the sets that gather luma and chroma)."""
    for sw, sh, dw, dh, sx, sy in [(2048, 32, 128, 64, 15.0, 0.25), (64, 1024, 128, 64, 0.125, 15.0), (4096, 64, 200, 70, 15.5, 0.3)]:
        f = synth.nv12(61, sw, sh)
        Ki = np.array([[100.0 * sx, 0, sw / 2], [0, 100.0 * sy, sh / 2], [0, 0, 1]])
        Ko = np.array([[100.0, 0, dw / 2], [0, 100.0, dh / 2], [0, 0, 1]])
        for rot in [(0.0, 0.0, 0.0), (0.0, 0.0, 0.002)]:
            check(vs, cuda, f, oracle.map_params(Ki, Ko, oracle.rodrigues(rot)), dw, dh, vs.MAP_RECT_TO_RECT)


def test_warp_cubic_refuses_other_formats(vs, cuda):
    w, h = 128, 72
    f = dev(synth.nv12(1, w, h), cuda)
    p, dw, dh = cams(w, h, ROTS[0])
    for fmt in (vs.OUT_NV12, 5):
        with pytest.raises(vs.VstabError):
            vs.warp_nv12_cubic(f, p, dw, dh, vs.MAP_CREATEMAP_CL, fmt)
    with pytest.raises(vs.VstabError):
        vs.warp_nv12_cubic(f, p, dw, dh, 6, vs.OUT_BGR8)


# ---------------------------------------------------------------------------------------------
# the pipeline object
# ---------------------------------------------------------------------------------------------
W, H = 640, 360


@pytest.fixture(scope="module")
def clip():
    K = oracle.get_preset_camera(4, W, H)
    frames, rots = synth.shaky_clip(3, K, W, H, 12, sigma=0.004)
    return K, frames, rots


def pulls(vs, cuda, frames, how, **cfg):
    import torch
    stab = vs.Stabilizer([torch.from_numpy(f).to(cuda) for f in frames], total=len(frames), **cfg)
    outs = []
    if how == "frames":
        cw, ch = stab.out_size
        ring = [torch.zeros((ch, cw, 3), dtype=torch.uint8, device=cuda) for _ in range(3)]
        while True:
            n = stab.pull_frames_into(ring, len(outs), 3)
            outs += [ring[(len(outs) + i) % 3].cpu().numpy() for i in range(n)]
            if n < 3:
                break
    else:
        while True:
            o = stab.pull_nv12(planar=True) if how == "planar" else stab.pull()
            if o is None:
                break
            outs.append(tuple(x.cpu().numpy() for x in o) if how == "planar" else o.cpu().numpy())
    return stab, outs


@pytest.mark.parametrize("tracking", [1, 0])
def test_pipeline_cubic_frames(vs, cuda, clip, tracking):
    K, frames, _ = clip
    Ko, (cw, ch) = oracle.get_output_camera(K, W, H)
    ref, _ = pulls(vs, cuda, frames, "pull", smooth_radius=2, tracking=tracking, map_precision=expect.IEEE)
    for how in ("pull", "frames", "planar"):
        stab, outs = pulls(vs, cuda, frames, how, smooth_radius=2, tracking=tracking, map_precision=expect.IEEE, resample=vs.RESAMPLE_CUBIC)
        assert len(outs) == len(frames) - 1
        for i, o in enumerate(outs):
            assert np.array_equal(stab.warp_rotation(i), ref.warp_rotation(i)), (how, i)   # rotations are the bilinear handle's
            p = oracle.map_params(K, Ko, stab.warp_rotation(i))
            if how == "planar":
                ey, euv = wd.planar(frames[i + 1], *wd.maps(p, cw, ch, 0), "cubic")
                assert np.array_equal(o[0], ey) and np.array_equal(o[1], euv), (how, tracking, i)
            else:
                assert np.array_equal(o, wd.bgr(frames[i + 1], *wd.maps(p, cw, ch, 0), "cubic")), (how, tracking, i)


def test_pipeline_cubic_default_precision(vs, cuda, clip):
    if not oracle.ref_gfx950_available():
        pytest.skip("oracle/_ref/createMap.gfx950.co not built")
    K, frames, _ = clip
    Ko, (cw, ch) = oracle.get_output_camera(K, W, H)
    stab, outs = pulls(vs, cuda, frames[:6], "pull", smooth_radius=2, tracking=0, resample=vs.RESAMPLE_CUBIC)
    for i in (0, len(outs) - 1):
        p = oracle.map_params(K, Ko, stab.warp_rotation(i))
        assert np.array_equal(outs[i], wd.bgr(frames[i + 1], *wd.maps(p, cw, ch, 5), "cubic")), i


def test_pipeline_cubic_lens_mode(vs, cuda, clip):
    K, frames, _ = clip
    cfg = dict(lens_mode=1, in_projection=1, out_projection=0, in_dfov=150.0, out_dfov=110.0, out_width=480, out_height=270, smooth_radius=2)
    stab, outs = pulls(vs, cuda, frames[:8], "pull", resample=vs.RESAMPLE_CUBIC, **cfg)
    Kout = oracle.lens_camera(oracle.PROJ_RECT, 110.0, 480, 270)
    for i in (0, len(outs) - 1):
        p = oracle.map_params(stab.K_in, Kout, stab.warp_rotation(i))
        assert np.array_equal(outs[i], wd.bgr(frames[i + 1], *wd.maps(p, 480, 270, oracle.MAP_FISH_TO_RECT), "cubic")), i


def test_pipeline_cubic_refusals(vs, cuda, clip):
    import torch
    K, frames, _ = clip
    fr = [torch.from_numpy(f).to(cuda) for f in frames[:5]]
    stab = vs.Stabilizer(fr, total=5, smooth_radius=1, resample=vs.RESAMPLE_CUBIC)
    with pytest.raises(vs.VstabError, match="RESAMPLE_CUBIC"):
        stab.pull_nv12(planar=False)                  # NV12 through BGR: refused before a frame is taken
    n = 0
    while stab.pull() is not None:                     # the handle keeps working and no frame was lost
        n += 1
    assert n == 4
    stab.close()
    ro = [oracle.rodrigues((0.0, 0.0, 0.001))] * 5
    stab = vs.Stabilizer(fr, total=5, smooth_radius=1, resample=vs.RESAMPLE_CUBIC, readouts=ro)
    with pytest.raises(vs.VstabError, match="read-out"):
        stab.pull()
    stab.close()
    for bad in (dict(pixel_depth=10), dict(interpolation=0), dict(resample=3)):
        with pytest.raises(vs.VstabError):
            vs.Stabilizer(fr, total=5, smooth_radius=1, **dict(dict(resample=vs.RESAMPLE_CUBIC), **bad))
