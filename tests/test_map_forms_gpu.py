"""The lens map is stated once (csrc/vstab_map.hpp) and reached by many kernels: the map planes, the quantised map, the fused BGR warp, the
10-bit warp, the bilinear warp with a border mode and the cubic warp.  This test pins them to each other and to the oracle at the pixels
where the chain branches: the axis pixel, both sides of the arc tangent's argument reduction, rays behind the camera, pixels outside the
source -- each class asserted non-empty on the oracle's map before any GPU call.  Every float and every sample must be equal.

96 x 40 output (one and a half tile columns, more than one tile row of either height: whole and clipped tiles), 64 x 48 source, the output
camera's principal point at the integer pixel (48, 20).  Map modes 0 (createMap.cl), 1 (fisheye -> pinhole, guarded) and 1 with k1..k4;
a rotation of about 100 degrees about the vertical axis for the rays behind the camera; one case with a rotation per output row."""
import numpy as np
import pytest

import distort_def as dd
import oracle
import warp_def as wd

pytestmark = pytest.mark.gpu

W, H, DW, DH = 64, 48, 96, 40
INT_MIN = -(2 ** 31)
F = np.float32
ROT_ID, ROT_SMALL, ROT_BEHIND = (0.0, 0.0, 0.0), (0.05, -0.1, 0.2), (0.0, 1.75, 0.0)      # 1.75 rad = 100.3 degrees about the vertical axis
ROT_LAST_ROW = (0.07, -0.09, 0.18)
MODES = {"createmap": (0, None), "fish_to_rect": (1, None), "fish_to_rect_k1k4": (1, dd.D_A)}


def cameras():
    Kin = oracle.lens_camera(oracle.PROJ_FISH, 120.0, W, H)
    Kout = oracle.lens_camera(oracle.PROJ_RECT, 130.0, DW, DH)
    assert Kout[0, 2] == DW // 2 and Kout[1, 2] == DH // 2
    return Kin, Kout


def params(rv):
    Kin, Kout = cameras()
    return oracle.map_params(Kin, Kout, oracle.rodrigues(rv))


def oracle_maps(p, mode, D, rot_bottom=None):
    if rot_bottom is not None:
        assert D is None
        return oracle.create_map_rs(p, rot_bottom, DW, DH, mode)
    if D is not None:
        return dd.maps(p, DW, DH, mode, D)
    return oracle.create_map(p, DW, DH) if mode == 0 else oracle.create_map_ex(p, DW, DH, mode)


def ray(p):
    """(px, py, wz) of every output pixel, fp32 as the map has them (one rotation)."""
    p = np.asarray(p, F)
    with np.errstate(all="ignore"):
        vx = ((np.arange(DW, dtype=F) - p[4]) / p[6])[None, :]
        vy = ((np.arange(DH, dtype=F) - p[5]) / p[7])[:, None]
        wx, wy, wz = ((p[8 + 3 * i] * vx + p[9 + 3 * i] * vy) + p[10 + 3 * i] for i in range(3))
        return wx / wz, wy / wz, wz


def frames():
    """NV12 and P010 frames whose samples differ between any two neighbours, so a tap one pixel off changes the result."""
    c, r = np.meshgrid(np.arange(W), np.arange(H))
    y = ((37 * c + 101 * r + 3 * c * r) & 255).astype(np.uint8)
    assert (y[:, 1:] != y[:, :-1]).all() and (y[1:] != y[:-1]).all()
    cc, cr = np.meshgrid(np.arange(W), np.arange(H // 2))
    uv = ((53 * cc + 89 * cr + 4 * cc * cr + 17) & 255).astype(np.uint8)
    assert (uv[:, 2:] != uv[:, :-2]).all() and (uv[1:] != uv[:-1]).all()
    y16 = ((y.astype(np.uint16) * 4 + ((c + r) & 3).astype(np.uint16)) << 6)
    uv16 = ((uv.astype(np.uint16) * 4 + ((cc + 2 * cr) & 3).astype(np.uint16)) << 6)
    return np.vstack([y, uv]), y16, uv16


def dev(a, cuda):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_map(got_x, got_y, ex, ey, what):
    """Bit equality; where the oracle's entry is not a number (mode 0's 0/0 axis pixel, the guarded modes' rays behind the camera) the
    kernel's must not be one either, and its bits are left open."""
    nan = np.isnan(ex) | np.isnan(ey)
    assert np.array_equal(np.isnan(got_x) | np.isnan(got_y), nan), what
    assert np.array_equal(bits(got_x)[~nan], bits(ex)[~nan]) and np.array_equal(bits(got_y)[~nan], bits(ey)[~nan]), what


def check_classes(p, mode, mx, my, rot):
    """The classes of pixels this case is there for, on the oracle's map."""
    px, py, wz = ray(p)
    rad = np.sqrt(px * px + py * py)
    front = wz > 0
    with np.errstate(invalid="ignore"):
        outside = (mx < -1) | (mx > W) | (my < -1) | (my > H)
        inside = (mx >= 0) & (mx <= W - 1) & (my >= 0) & (my <= H - 1)
    assert inside.any() and outside.any(), "pixels inside and outside the source"
    assert (front & (rad < 1)).any() and (front & (rad > 1)).any(), "both sides of the argument reduction"
    if rot == ROT_ID:
        assert px[DH // 2, DW // 2] == 0 and py[DH // 2, DW // 2] == 0, "the axis pixel"
        if mode == 0:
            assert np.isnan(mx[DH // 2, DW // 2])                              # createMap.cl: 0 / 0
        else:
            assert mx[DH // 2, DW // 2] == p[0] and my[DH // 2, DW // 2] == p[1]   # factor 1: the input centre exactly
    if rot == ROT_BEHIND:
        assert (wz <= 0).any() and front.any(), "rays behind the camera"
        if mode != 0:
            assert np.array_equal(np.isnan(mx), wz <= 0)


def check_kernels(vs, cuda, p, mode, D, mx, my, what, rot_bottom=None):
    """Every kernel that evaluates the map, against the oracle's remaps of the oracle's map (mx, my)."""
    nv12, y16, uv16 = frames()
    fd = dev(nv12, cuda)
    bgr = oracle.cvt_nv12_bgr(nv12)
    if rot_bottom is not None:
        fused = vs.warp_nv12_rs(fd, p, rot_bottom, DW, DH, mode)
        border = vs.warp_nv12_border(fd, p, DW, DH, mode, vs.OUT_BGR8, vs.BORDER_REFLECT_101, rot_bottom)
        cubic = vs.warp_nv12_rs_ex(fd, p, DW, DH, rot_bottom, None, mode, vs.RESAMPLE_CUBIC, vs.BORDER_CONSTANT)
    elif D is not None:
        fused = vs.warp_nv12_dist(fd, p, D, DW, DH, mode)
        border = vs.warp_nv12_dist_ex(fd, p, D, DW, DH, mode, vs.RESAMPLE_DEFAULT, vs.BORDER_REFLECT_101)
        cubic = vs.warp_nv12_dist_ex(fd, p, D, DW, DH, mode, vs.RESAMPLE_CUBIC, vs.BORDER_CONSTANT)
    else:
        fused = vs.warp_nv12(fd, p, DW, DH, mode)
        border = vs.warp_nv12_border(fd, p, DW, DH, mode, vs.OUT_BGR8, vs.BORDER_REFLECT_101)
        cubic = vs.warp_nv12_cubic(fd, p, DW, DH, mode)
    assert np.array_equal(fused.cpu().numpy(), oracle.remap_bilinear(bgr, mx, my)), (what, "fused")
    assert np.array_equal(border.cpu().numpy(), wd.remap(bgr, mx, my, "linear", wd.REFLECT_101)), (what, "border")
    assert np.array_equal(cubic.cpu().numpy(), wd.remap(bgr, mx, my, "cubic", wd.CONSTANT, 0)), (what, "cubic")
    if D is None:   # the 10-bit warp has no lens coefficients
        import torch
        exp = oracle.remap_bilinear10(oracle.cvt_p010_bgr10(y16, uv16), mx, my, 0)
        # planes at 16-byte aligned addresses take the tiled 10-bit kernel, planes four bytes off them k_warp_p010 (two pixels a thread)
        for off in (0, 2):
            yb = torch.zeros((H, W + 8), dtype=torch.int16, device=cuda)
            ub = torch.zeros((H // 2, W + 8), dtype=torch.int16, device=cuda)
            yv, uvv = yb[:, off:off + W], ub[:, off:off + W]
            yv.copy_(dev(y16.view(np.int16), cuda)), uvv.copy_(dev(uv16.view(np.int16), cuda))
            assert yv.data_ptr() % 16 == 2 * off and uvv.data_ptr() % 16 == 2 * off
            got = vs.warp_p010(yv, uvv, p, DW, DH, rot_bottom, mode, vs.BLEND_EXACT)
            assert np.array_equal(got.cpu().numpy().view(np.uint16), exp), (what, "p010", off)


@pytest.mark.parametrize("name", list(MODES))
@pytest.mark.parametrize("rot", [ROT_ID, ROT_SMALL, ROT_BEHIND])
def test_every_kernel_has_the_oracles_map(vs, cuda, name, rot):
    mode, D = MODES[name]
    p = params(rot)
    mx, my = oracle_maps(p, mode, D)
    check_classes(p, mode, mx, my, rot)                    # before any GPU call
    # the map planes
    gx, gy = vs.create_map(p, DW, DH, mode=mode) if D is None else vs.create_map_dist(p, D, DW, DH, mode)
    same_map(gx.cpu().numpy(), gy.cpu().numpy(), mx, my, (name, rot, "planes"))
    # the quantised map: cvRound(32 * map) of the same planes
    q = vs.quantised_map(p, DW, DH, mode) if D is None else vs.quantised_map_dist(p, D, DW, DH, mode)
    q = q.cpu().numpy().view(np.int32).reshape(DH, -1, 2)[:, :DW]
    qx, qy, ok = dd.quantised(mx, my)
    inr = ok & (np.abs(qx) < 2 ** 30) & (np.abs(qy) < 2 ** 30)
    assert np.array_equal(q[..., 0][inr], qx[inr]) and np.array_equal(q[..., 1][inr], qy[inr]), (name, rot, "quantised")
    assert (q[..., 0][~ok] == INT_MIN).all(), (name, rot, "quantised: not a number")
    check_kernels(vs, cuda, p, mode, D, mx, my, (name, rot))


@pytest.mark.parametrize("mode", [0, 1])
def test_every_kernel_has_the_oracles_map_with_a_rotation_per_row(vs, cuda, mode):
    p = params(ROT_SMALL)
    rb = params(ROT_LAST_ROW)[8:]
    mx, my = oracle_maps(p, mode, None, rb)
    one_x, _ = oracle_maps(p, mode, None)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(bits(mx[0]), bits(one_x[0])) and (mx[1:] != one_x[1:]).any(axis=1).all(), "every row but the first has its own rotation"
        assert ((mx >= 0) & (mx <= W - 1) & (my >= 0) & (my <= H - 1)).any() and ((mx < -1) | (mx > W) | (my < -1) | (my > H)).any()
    check_kernels(vs, cuda, p, mode, None, mx, my, ("rs", mode), rot_bottom=rb)
