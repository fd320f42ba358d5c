"""numpy statement of the pinhole lens distortion the *_pinhole entry points are held to (include/vstab.h, "Pinhole lens distortion"; DESIGN.md
section 23): OpenCV's Brown-Conrady model on a RECTILINEAR input camera, D = (k1, k2, p1, p2, k3) in cv::calibrateCamera's order.

  map     (fp32, per output pixel) map modes 3 / 4 (oracle.create_map_ex) up to x = wx / wz, y = wy / wz, then -- every operation an IEEE
          binary32 operation of its own --
              xx = x*x;  yy = y*y;  xy = x*y;  r2 = xx + yy
              g = k3;  g = g*r2 + k2;  g = g*r2 + k1;  rad = 1 + g*r2
              a = 2*xy;  dx = p1*a + p2*(r2 + 2*xx);  dy = p1*(r2 + 2*yy) + p2*a
              xd = x*rad + dx;  yd = y*rad + dy
          map = centre + (xd, yd) * focal; NaN exactly where modes 3 / 4 are (wz <= 0; mode 4: rho >= pi).  D = 0: maps(..., D_0) IS
          oracle.create_map_ex (test_pinhole_cpu.py pins that).
  points  (fp64) OpenCV 4.5's cv::undistortPoints with its default criteria: five fixed-point steps from (x0, y0), no epsilon test; a
          negative 1 / (radial factor) gives the point back as it came.

sin / cos are the oracle's (oracle.sincosf); colour conversion and every resampler behind the map are the existing definitions
(warp_def.bgr / planar): the distorted warp differs from modes 3 / 4 in the map alone."""
import numpy as np

import oracle

F = np.float32
PI_F = F(3.1415927410125732421875)
D_0 = (0.0, 0.0, 0.0, 0.0, 0.0)
D_P = (-0.28, 0.09, 0.001, -0.0008, -0.012)
D_Q = (0.12, 0.03, -0.002, 0.0015, 0.0)
D_M = (-0.12, 0.02, 0.0005, -0.0004, 0.0)


def maps(p, dw, dh, mode, D=D_0):
    """(mapx, mapy) float32 (dh, dw) of map mode 3 (pinhole -> pinhole) or 4 (pinhole -> fisheye) with the input lens's D."""
    assert mode in (3, 4)
    p = np.asarray(p, F)
    k1, k2, p1, p2, k3 = (F(v) for v in D)
    one, two = F(1), F(2)
    with np.errstate(all="ignore"):
        vx = np.broadcast_to(((np.arange(dw, dtype=F) - p[4]) / p[6])[None, :], (dh, dw))
        vy = np.broadcast_to(((np.arange(dh, dtype=F) - p[5]) / p[7])[:, None], (dh, dw))
        ok = np.ones((dh, dw), bool)
        if mode == 4:
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
        x, y = wx / wz, wy / wz
        xx, yy, xy = x * x, y * y, x * y
        r2 = xx + yy
        g = np.full((dh, dw), k3, F)
        g = g * r2 + k2
        g = g * r2 + k1
        rad = one + g * r2
        a = two * xy
        dx = p1 * a + p2 * (r2 + two * xx)
        dy = p1 * (r2 + two * yy) + p2 * a
        xd, yd = x * rad + dx, y * rad + dy
        mx = p[0] + xd * p[2]
        my = p[1] + yd * p[3]
    assert mx.dtype == F and my.dtype == F and rad.dtype == F and dx.dtype == F
    return np.where(ok, mx, F(np.nan)), np.where(ok, my, F(np.nan))


# ---------------------------------------------------------------------------------------------------------------------
# points (fp64)
# ---------------------------------------------------------------------------------------------------------------------
def distort_normalised(x, y, D):
    """The forward model on normalised coordinates (arrays or scalars), fp64."""
    k1, k2, p1, p2, k3 = D
    r2 = x * x + y * y
    rad = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
    return x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x), y * rad + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y


def undistort_normalised(x0, y0, D):
    """cv::undistortPoints' iteration for one normalised point: exactly five steps, no epsilon test."""
    k1, k2, p1, p2, k3 = D
    x, y = x0, y0
    for _ in range(5):
        r2 = x * x + y * y
        icdist = 1 / (1 + ((k3 * r2 + k2) * r2 + k1) * r2)
        if icdist < 0:
            return x0, y0
        dX = 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        dY = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        x, y = (x0 - dX) * icdist, (y0 - dY) * icdist
    return x, y


def undistort_points(pts, K, D, R=None, P=None):
    """cv::undistortPoints(pts, K, D, R, P) -> (n, 2) float64."""
    pts = np.asarray(pts, np.float64).reshape(-1, 2)
    K = np.asarray(K, np.float64)
    D = tuple(float(v) for v in D)
    RR = np.eye(3) if R is None else np.asarray(R, np.float64)
    if P is not None:
        RR = np.asarray(P, np.float64) @ RR
    out = np.empty_like(pts)
    for i, (u, v) in enumerate(pts):
        x, y = undistort_normalised((u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], D)
        q = RR @ np.array([x, y, 1.0])
        out[i] = q[0] / q[2], q[1] / q[2]
    return out


def project(K, D, rays):
    """Rays (n, 3), z > 0 -> pixels (n, 2) of the distorted pinhole camera (K, D): the forward model, fp64."""
    rays = np.asarray(rays, np.float64)
    xd, yd = distort_normalised(rays[:, 0] / rays[:, 2], rays[:, 1] / rays[:, 2], D)
    return np.stack([K[0, 2] + K[0, 0] * xd, K[1, 2] + K[1, 1] * yd], axis=-1)


def round_trip_residual(K, D, pts):
    """Largest |undistort(pixel) - the normalised point that projects to it| over pts (n, 2) normalised points, in normalised coordinates:
    what five steps of cv::undistortPoints leave of the distortion."""
    pts = np.asarray(pts, np.float64).reshape(-1, 2)
    xd, yd = distort_normalised(pts[:, 0], pts[:, 1], D)
    back = np.array([undistort_normalised(a, b, D) for a, b in zip(xd, yd)])
    return float(np.hypot(back[:, 0] - pts[:, 0], back[:, 1] - pts[:, 1]).max())


def lens_rays(K, D, w, h):
    """Rays (z = 1) of every pixel of the distorted pinhole camera (K, D): the fixed-point iteration run until it stands still (the
    renderer wants the lens's true inverse, not what five steps leave of it): (h, w, 3) float64."""
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    x0, y0 = (xs - K[0, 2]) / K[0, 0], (ys - K[1, 2]) / K[1, 1]
    k1, k2, p1, p2, k3 = D
    x, y = x0.copy(), y0.copy()
    for _ in range(60):
        r2 = x * x + y * y
        icdist = 1 / (1 + ((k3 * r2 + k2) * r2 + k1) * r2)
        x, y = (x0 - (2 * p1 * x * y + p2 * (r2 + 2 * x * x))) * icdist, (y0 - (p1 * (r2 + 2 * y * y) + 2 * p2 * x * y)) * icdist
    xd, yd = distort_normalised(x, y, D)
    assert max(np.abs(xd - x0).max(), np.abs(yd - y0).max()) < 1e-10
    return np.stack([x, y, np.ones_like(x)], axis=-1)


def shaky_clip(seed, K, D, w, h, n, sigma=0.004):
    """synth.shaky_clip seen through the distorted pinhole lens (K, D): the same texture, orientations and chroma, the luma re-rendered
    through lens_rays -> n packed NV12 frames + the camera orientations (modelled on distort_def.shaky_clip)."""
    import synth
    ideal, rots = synth.shaky_clip(seed, K, w, h, n, sigma=sigma, projection="rect")      # the orientations and the chroma planes are that clip's
    tex = synth.sphere_texture(seed)
    rays = lens_rays(K, D, w, h)
    rays = rays / np.linalg.norm(rays, axis=-1, keepdims=True)
    frames = []
    for f, R in zip(ideal, rots):
        f = f.copy()
        f[:h] = synth.render_frame(tex, rays, R)
        frames.append(f)
    return frames, rots
