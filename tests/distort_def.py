"""numpy statement of the lens distortion the *_dist entry points and a calibrated handle are held to (include/vstab.h, "Lens distortion";
DESIGN.md section 18): OpenCV's fisheye (Kannala-Brandt) model on the INPUT camera,

  theta_d = theta (1 + k1 theta^2 + k2 theta^4 + k3 theta^6 + k4 theta^8),   image radius = f theta_d.

  map     (fp32, per output pixel) map modes 1 / 2 (oracle.create_map_ex) up to theta = atan(rad), then -- every operation an IEEE binary32
          operation of its own --
              s2 = theta * theta;  g = k4;  g = g * s2 + k3;  g = g * s2 + k2;  g = g * s2 + k1;  theta_d = theta * (1 + g * s2)
          k = theta_d / rad (1 on the axis), map = centre + (p * k) * focal; NaN exactly where modes 1 / 2 are.  D = 0: theta_d == theta
          bit for bit, so maps(..., D=0) IS oracle.create_map_ex (test_distort_cpu.py pins that).
  points  (fp64) OpenCV 4.5's fisheye::undistortPoints: theta_d clipped to pi/2, Newton from theta = theta_d, at most 10 steps, stop at
          |fix| < 1e-8, scale = tan(theta) / theta_d; no theta found -> (-1e6, -1e6).

atan and sin / cos are the oracle's (oracle.atanf, oracle.sincosf); colour conversion, bilinear remap and the plane-wise warp are the
oracle's too: the distorted warp differs from modes 1 / 2 in the map alone."""
import numpy as np

import oracle

F = np.float32
PI_F = F(3.1415927410125732421875)
D_0 = (0.0, 0.0, 0.0, 0.0)
D_A = (-0.02, 0.004, -0.001, 0.0002)
D_B = (0.05, 0.01, 0.0, 0.0)
D_C = (-0.05, 0.0, 0.0, 0.0)
INT_MIN = -(2 ** 31)


def maps(p, dw, dh, mode, D=D_0):
    """(mapx, mapy) float32 (dh, dw) of map mode 1 (fisheye -> pinhole) or 2 (fisheye -> fisheye) with the input lens's D."""
    assert mode in (1, 2)
    p = np.asarray(p, F)
    k1, k2, k3, k4 = (F(v) for v in D)
    one = F(1)
    with np.errstate(all="ignore"):
        vx = np.broadcast_to(((np.arange(dw, dtype=F) - p[4]) / p[6])[None, :], (dh, dw))
        vy = np.broadcast_to(((np.arange(dh, dtype=F) - p[5]) / p[7])[:, None], (dh, dw))
        ok = np.ones((dh, dw), bool)
        if mode == 2:
            rho = np.sqrt(vx * vx + vy * vy)
            ok = rho < PI_F
            sn, cs = oracle.sincosf(rho)
            s = np.where(rho == 0, one, sn / rho)
            rx, ry, rz = vx * s, vy * s, cs
            wx = (p[8] * rx + p[9] * ry) + p[10] * rz
            wy = (p[11] * rx + p[12] * ry) + p[13] * rz
            wz = (p[14] * rx + p[15] * ry) + p[16] * rz
        else:
            wx = (p[8] * vx + p[9] * vy) + p[10]
            wy = (p[11] * vx + p[12] * vy) + p[13]
            wz = (p[14] * vx + p[15] * vy) + p[16]
        ok = ok & (wz > 0)
        cx, cy = wx / wz, wy / wz
        rad = np.sqrt(cx * cx + cy * cy)
        at = oracle.atanf(rad).reshape(dh, dw)
        s2 = at * at
        g = np.full((dh, dw), k4, F)
        g = g * s2 + k3
        g = g * s2 + k2
        g = g * s2 + k1
        td = at * (one + g * s2)
        k = np.where(rad == 0, one, td / rad)
        mx = p[0] + (cx * k) * p[2]
        my = p[1] + (cy * k) * p[3]
    assert mx.dtype == F and my.dtype == F and td.dtype == F
    return np.where(ok, mx, F(np.nan)), np.where(ok, my, F(np.nan))


def quantised(mx, my):
    """cv::remap's integers of a map: (qx, qy) int64 = rint(32 * map), and `ok` where the entry is a number (elsewhere qx is INT_MIN)."""
    ok = ~(np.isnan(mx) | np.isnan(my))
    with np.errstate(invalid="ignore"):
        qx, qy = np.rint(mx * F(32)), np.rint(my * F(32))
    return np.where(ok, qx, INT_MIN).astype(np.int64), np.where(ok, qy, 0).astype(np.int64), ok


def warp_bgr(nv12, p, dw, dh, mode, D=D_0):
    """cvtColor(NV12 -> BGR), then cv::remap(INTER_LINEAR, BORDER_CONSTANT 0) with the distorted map -> (dh, dw, 3) uint8."""
    mx, my = maps(p, dw, dh, mode, D)
    return oracle.remap_bilinear(oracle.cvt_nv12_bgr(nv12), mx, my)


def warp_planar(nv12, p, dw, dh, mode, D=D_0):
    """The plane-wise warp (VSTAB_OUT_NV12_PLANAR) with the distorted map -> (luma (dh, dw), chroma (ceil(dh/2), 2 ceil(dw/2)))."""
    nv12 = np.asarray(nv12)
    h = nv12.shape[0] * 2 // 3
    mx, my = maps(p, dw, dh, mode, D)
    return oracle.warp_planar_mapped(nv12[:h], nv12[h:], mx, my)


# ---------------------------------------------------------------------------------------------------------------------
# points (fp64)
# ---------------------------------------------------------------------------------------------------------------------
def distort_theta(theta, D):
    t2 = theta * theta
    return theta * (1 + D[0] * t2 + D[1] * t2 ** 2 + D[2] * t2 ** 3 + D[3] * t2 ** 4)


def min_derivative(D):
    """min of d theta_d / d theta over the 1025 points theta = i (pi/2) / 1024: the accepted coefficients have it > 0."""
    t = np.arange(1025) * (np.pi / 2) / 1024
    t2 = t * t
    return float((1 + 3 * D[0] * t2 + 5 * D[1] * t2 ** 2 + 7 * D[2] * t2 ** 3 + 9 * D[3] * t2 ** 4).min())


def undistort_theta(theta_d, D):
    """OpenCV 4.5's Newton iteration for one theta_d -> (theta, converged and not flipped, steps taken)."""
    theta = theta_d
    for j in range(10):
        t2 = theta * theta
        t4 = t2 * t2
        t6 = t4 * t2
        t8 = t6 * t2
        a, b, c, d = D[0] * t2, D[1] * t4, D[2] * t6, D[3] * t8
        fix = (theta * (1 + a + b + c + d) - theta_d) / (1 + 3 * a + 5 * b + 7 * c + 9 * d)
        theta = theta - fix
        if abs(fix) < 1e-8:
            return theta, not (theta_d > 0 and theta < 0), j + 1
    return theta, False, 10


def undistort_points(pts, K, D, R=None, P=None):
    """fisheye::undistortPoints(pts, K, D, R, P) -> (n, 2) float64."""
    pts = np.asarray(pts, np.float64).reshape(-1, 2)
    RR = np.eye(3) if R is None else np.asarray(R, np.float64)
    if P is not None:
        RR = np.asarray(P, np.float64) @ RR
    out = np.empty_like(pts)
    for i, (x, y) in enumerate(pts):
        pwx, pwy = (x - K[0, 2]) / K[0, 0], (y - K[1, 2]) / K[1, 1]
        theta_d = min(max(-np.pi / 2, float(np.sqrt(pwx * pwx + pwy * pwy))), np.pi / 2)
        scale = 0.0
        if abs(theta_d) > 1e-8:
            theta, ok, _ = undistort_theta(theta_d, D)
            if not ok:
                out[i] = -1000000.0
                continue
            scale = np.tan(theta) / theta_d
        u = np.array([pwx * scale, pwy * scale, 1.0])
        v = RR @ u
        out[i] = v[0] / v[2], v[1] / v[2]
    return out


def project(K, D, rays):
    """Rays (n, 3) -> pixels (n, 2) of the distorted fisheye camera (K, D): the forward model, fp64."""
    rays = np.asarray(rays, np.float64)
    x, y, z = rays[:, 0], rays[:, 1], rays[:, 2]
    r = np.hypot(x, y)
    td = distort_theta(np.arctan2(r, z), D)
    s = np.where(r > 1e-12, td / np.maximum(r, 1e-12), 1.0)
    return np.stack([K[0, 2] + K[0, 0] * x * s, K[1, 2] + K[1, 1] * y * s], axis=-1)


def lens_rays(K, D, w, h):
    """Unit rays of every pixel of the distorted fisheye camera (K, D), through the Newton inverse: (h, w, 3) float64."""
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    px, py = (xs - K[0, 2]) / K[0, 0], (ys - K[1, 2]) / K[1, 1]
    td = np.hypot(px, py)
    th = td.copy()
    for _ in range(10):       # the same Newton steps, vectorised: every pixel converges within a few
        t2 = th * th
        a, b, c, d = D[0] * t2, D[1] * t2 ** 2, D[2] * t2 ** 3, D[3] * t2 ** 4
        th = th - (th * (1 + a + b + c + d) - td) / (1 + 3 * a + 5 * b + 7 * c + 9 * d)
    assert np.abs(distort_theta(th, D) - td).max() < 1e-12
    s = np.where(td > 1e-12, np.sin(th) / np.maximum(td, 1e-12), 1.0)
    return np.stack([px * s, py * s, np.cos(th)], axis=-1)


def shaky_clip(seed, K, D, w, h, n, sigma=0.004):
    """synth.shaky_clip seen through the distorted lens (K, D): the same texture, orientations and chroma, the luma re-rendered through
    lens_rays -> n packed NV12 frames + the camera orientations."""
    import synth
    ideal, rots = synth.shaky_clip(seed, K, w, h, n, sigma=sigma)      # the orientations and the chroma planes are that clip's
    tex = synth.sphere_texture(seed)
    rays = lens_rays(K, D, w, h)
    frames = []
    for f, R in zip(ideal, rots):
        f = f.copy()
        f[:h] = synth.render_frame(tex, rays, R)
        frames.append(f)
    return frames, rots
