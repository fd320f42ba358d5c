// vstab_geometry.cpp -- host-side camera geometry (fp64) behind the C ABI.
// Replaces get_preset_camera / get_output_camera (FrameSourceWarp.cpp:27-165) and the
// cv::fisheye::undistortPoints calls (:93, :322, :333) for the zero-distortion case the
// reference uses.  These run once per clip / on <= 200 points per frame, so they stay on the
// host exactly as in the reference.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "vstab_geometry.hpp"
#include "vstab_internal.hpp"

namespace vstab {

static thread_local std::string g_last_error;
void set_error(const std::string &msg) { g_last_error = msg; }

static thread_local LaunchEvents g_launch_events;
void set_launch_events(hipEvent_t start, hipEvent_t stop) { g_launch_events = {start, stop}; }
LaunchEvents take_launch_events() {
    const LaunchEvents e = g_launch_events;
    g_launch_events = LaunchEvents();
    return e;
}
bool launch_events_pending() { return g_launch_events.start != nullptr; }

// FrameSourceWarp.cpp:22-25: the published FOVs are stored in `const int`, dropping the fraction.
static const int FOV_H_43W = (int)122.6, FOV_V_43W = (int)94.4, FOV_H_169W = (int)118.2, FOV_V_169W = (int)69.5;

bool preset_camera(int preset, int w, int h, Mat3 &K) {
    K = Mat3::identity();
    K(0, 2) = (w - 1.) / 2;  // :31-32 principal point at the centre by default
    K(1, 2) = (h - 1.) / 2;
    switch (preset) {
        case VSTAB_GOPRO_H4B_WIDE43_PUBLISHED:
            K(0, 0) = w / (FOV_H_43W * M_PI / 180);
            K(1, 1) = h / (FOV_V_43W * M_PI / 180);
            break;
        case VSTAB_GOPRO_H4B_WIDE169_PUBLISHED:
            K(0, 0) = w / (FOV_H_169W * M_PI / 180);
            K(1, 1) = h / (FOV_V_169W * M_PI / 180);
            break;
        case VSTAB_GOPRO_H4B_WIDE43_MEASURED:  // :50-56 (fx AND fy scale with height)
            K(0, 2) = 967.37 * w / 1920, K(1, 2) = 711.07 * h / 1440;
            K(0, 0) = 942.96 * h / 1440, K(1, 1) = 942.53 * h / 1440;
            break;
        case VSTAB_GOPRO_H4B_WIDE43_MEASURED_STABILISATION:
            K(0, 2) = 965.90 * w / 1920, K(1, 2) = 712.94 * h / 1440;
            K(0, 0) = 1045.58 * h / 1440, K(1, 1) = 1045.64 * h / 1440;
            break;
        case VSTAB_GOPRO_H4B_WIDE169_MEASURED:
            K(0, 2) = 1361.80 * w / 2704, K(1, 2) = 745.19 * h / 1520;
            K(0, 0) = 1392.49 * h / 1520, K(1, 1) = 1383.47 * h / 1520;
            break;
        case VSTAB_GOPRO_H4B_WIDE169_MEASURED_STABILISATION:
            K(0, 2) = 1357.49 * w / 2704, K(1, 2) = 736.74 * h / 1520;
            K(0, 0) = 1626.67 * h / 1520, K(1, 1) = 1619.46 * h / 1520;
            break;
        default:
            return false;
    }
    return true;
}

vstab_status check_distortion(const char *n, const double D[4]) {
    bool ok = D && std::isfinite(D[0]) && std::isfinite(D[1]) && std::isfinite(D[2]) && std::isfinite(D[3]);
    for (int i = 0; ok && i <= 1024; i++) {  // d theta_d / d theta on a grid of [0, pi/2]
        const double t = i * (M_PI / 2.) / 1024, t2 = t * t, t4 = t2 * t2, t6 = t4 * t2, t8 = t6 * t2;
        ok = 1 + 3 * D[0] * t2 + 5 * D[1] * t4 + 7 * D[2] * t6 + 9 * D[3] * t8 > 0;
    }
    return ok ? VSTAB_OK : fail(VSTAB_ERR_INVALID, std::string(n) + ": the distortion must keep theta_d increasing on [0, pi/2]");
}

// theta_d -> theta as OpenCV 4.5's fisheye::undistortPoints inverts the polynomial: Newton from theta = theta_d, at most 10 steps, stop at
// |fix| < 1e-8.  False when it did not converge or theta changed sign.  k = 0: the first step is zero and theta = theta_d.
bool fisheye_theta(double theta_d, const double k[4], double &theta) {
    bool converged = false;
    theta = theta_d;
    for (int j = 0; j < 10 && !converged; j++) {
        const double t2 = theta * theta, t4 = t2 * t2, t6 = t4 * t2, t8 = t6 * t2;
        const double a = k[0] * t2, b = k[1] * t4, c = k[2] * t6, d = k[3] * t8;
        const double fix = (theta * (1 + a + b + c + d) - theta_d) / (1 + 3 * a + 5 * b + 7 * c + 9 * d);
        theta -= fix;
        converged = std::fabs(fix) < 1e-8;
    }
    return converged && !((theta_d < 0 && theta > 0) || (theta_d > 0 && theta < 0));
}

// OpenCV 4.5 cv::undistortPoints with its default criteria for one normalised point of a rectilinear lens with D = (k1, k2, p1, p2, k3): five
// fixed-point steps from (x0, y0), no epsilon test; a negative 1 / (radial factor) gives the point back as it came
void pinhole_undistort_normalised(double x0, double y0, const double D[5], double &x, double &y) {
    const double k1 = D[0], k2 = D[1], p1 = D[2], p2 = D[3], k3 = D[4];
    x = x0, y = y0;
    for (int j = 0; j < 5; j++) {
        const double r2 = x * x + y * y;
        const double icdist = 1 / (1 + ((k3 * r2 + k2) * r2 + k1) * r2);
        if (icdist < 0) {
            x = x0, y = y0;
            break;
        }
        const double dX = 2 * p1 * x * y + p2 * (r2 + 2 * x * x), dY = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y;
        x = (x0 - dX) * icdist, y = (y0 - dY) * icdist;
    }
}

// OpenCV 4.5 fisheye::undistortPoints: theta_d clipped to pi/2, theta from fisheye_theta, scale = tan(theta)/theta_d; a point whose theta
// was not found is (-1e6, -1e6).  D null = zero: today's ideal lens, bit for bit.  fish false: a rectilinear lens, D its (k1, k2, p1, p2, k3)
// (five; pinhole_undistort_normalised) or null for the ideal pinhole.
void fisheye_undistort(const double *pts, int n, const Mat3 &K, const Mat3 &RR, double *out, bool fish, const double *D) {
    static const double zero[4] = {0, 0, 0, 0};
    const double *k = D ? D : zero;
    for (int i = 0; i < n; i++) {
        const double pwx = (pts[2 * i] - K(0, 2)) / K(0, 0), pwy = (pts[2 * i + 1] - K(1, 2)) / K(1, 1);
        double theta_d = std::sqrt(pwx * pwx + pwy * pwy);
        theta_d = std::min(std::max(-M_PI / 2., theta_d), M_PI / 2.);
        double scale = 0.0;
        if (fish && std::fabs(theta_d) > 1e-8) {
            double theta;
            if (!fisheye_theta(theta_d, k, theta)) {
                out[2 * i] = out[2 * i + 1] = -1000000.0;
                continue;
            }
            scale = std::tan(theta) / theta_d;
        }
        if (!fish) scale = 1.0;
        double ux = pwx * scale, uy = pwy * scale;
        if (!fish && D) pinhole_undistort_normalised(pwx, pwy, D, ux, uy);
        const double x = RR(0, 0) * ux + RR(0, 1) * uy + RR(0, 2);
        const double y = RR(1, 0) * ux + RR(1, 1) * uy + RR(1, 2);
        const double z = RR(2, 0) * ux + RR(2, 1) * uy + RR(2, 2);
        out[2 * i] = x / z, out[2 * i + 1] = y / z;
    }
}

bool lens_camera(int projection, double dfov_deg, int w, int h, double cx, double cy, Mat3 &K) {
    if (w <= 0 || h <= 0 || !(dfov_deg > 0)) return false;
    const double half_diag = 0.5 * std::sqrt((double)w * w + (double)h * h), half_fov = 0.5 * dfov_deg * M_PI / 180.0;
    double f;
    if (projection == VSTAB_PROJ_RECT) {
        if (!(dfov_deg < 180)) return false;
        f = half_diag / std::tan(half_fov);
    } else if (projection == VSTAB_PROJ_FISH) {
        if (!(dfov_deg < 360)) return false;
        f = half_diag / half_fov;
    } else {
        return false;
    }
    K = Mat3::identity();
    K(0, 0) = K(1, 1) = f;
    K(0, 2) = cx < 0 ? 0.5 * w : cx, K(1, 2) = cy < 0 ? 0.5 * h : cy;
    return true;
}

static int cv_round(double v) { return (int)std::nearbyint(v); }  // round half to even

void output_camera(const Mat3 &Kin, int w, int h, double scale, bool crop, double zoom, Mat3 &Kout, int &ow,
                   int &oh) {
    const double probes[16] = {0, 0, 0, h - 1., w - 1., 0, w - 1., h - 1.,                  // corners :96-99
                               Kin(0, 2), 0, w - 1., Kin(1, 2), Kin(0, 2), h - 1., 0, Kin(1, 2)};  // edge mid-points
    double ext[16];
    fisheye_undistort(probes, 8, Kin, Mat3::identity(), ext);
    const int start = crop ? 4 : 0;  // :119
    double max_x = ext[2 * start], min_x = max_x, max_y = ext[2 * start + 1], min_y = max_y;
    for (int i = start; i < 8; i++) {
        max_x = std::max(max_x, ext[2 * i]), min_x = std::min(min_x, ext[2 * i]);
        max_y = std::max(max_y, ext[2 * i + 1]), min_y = std::min(min_y, ext[2 * i + 1]);
    }
    const int idx = cv_round(w - 1.), idy = cv_round(h - 1.);  // :142 cv::Point (int)
    const double in_len = std::sqrt(1. * idx * idx + idy * idy);
    const int odx = cv_round(ext[6] - ext[0]), ody = cv_round(ext[7] - ext[1]);  // :146 cv::Point (int)
    const double out_len = std::sqrt(1. * odx * odx + ody * ody);
    scale *= in_len / out_len;  // :150
    Kout = Mat3::identity();
    Kout(0, 0) = scale, Kout(1, 1) = scale;
    Kout(0, 2) = scale * -min_x / zoom, Kout(1, 2) = scale * -min_y / zoom;
    ow = (int)(scale * (max_x - min_x) / zoom);  // :163 cv::Size(double,double) truncates
    oh = (int)(scale * (max_y - min_y) / zoom);
}

void map_params(const Mat3 &Kin, const Mat3 &Kout, const Mat3 &R, float p[17]) {
    p[0] = (float)Kin(0, 2), p[1] = (float)Kin(1, 2), p[2] = (float)Kin(0, 0), p[3] = (float)Kin(1, 1);
    p[4] = (float)Kout(0, 2), p[5] = (float)Kout(1, 2), p[6] = (float)Kout(0, 0), p[7] = (float)Kout(1, 1);
    for (int i = 0; i < 9; i++) p[8 + i] = (float)R.m[i];
}

}  // namespace vstab

using namespace vstab;

extern "C" {

const char *vstab_last_error(void) { return g_last_error.c_str(); }

const char *vstab_version(void) { return "vstab 0.1 gfx950"; }

int vstab_device_count(void) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        set_error(std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
        return e == hipErrorNoDevice ? 0 : (int)VSTAB_ERR_DEVICE;
    }
    return n;
}

vstab_status vstab_get_preset_camera(int preset, int width, int height, double K[9]) {
    if (!K || width <= 0 || height <= 0) return fail(VSTAB_ERR_INVALID, "vstab_get_preset_camera: bad argument");
    Mat3 m;
    if (!preset_camera(preset, width, height, m)) return fail(VSTAB_ERR_INVALID, "vstab_get_preset_camera: unknown preset");
    std::memcpy(K, m.m, sizeof(m.m));
    return VSTAB_OK;
}

vstab_status vstab_get_output_camera(const double K_in[9], int width, int height, double scale, int crop_borders,
                                     double zoom, double K_out[9], int *out_width, int *out_height) {
    if (!K_in || !K_out || !out_width || !out_height || width <= 0 || height <= 0 || !(scale > 0) || !(zoom > 0))
        return fail(VSTAB_ERR_INVALID, "vstab_get_output_camera: bad argument");
    Mat3 ki, ko;
    std::memcpy(ki.m, K_in, sizeof(ki.m));
    output_camera(ki, width, height, scale, crop_borders != 0, zoom, ko, *out_width, *out_height);
    std::memcpy(K_out, ko.m, sizeof(ko.m));
    return VSTAB_OK;
}

vstab_status vstab_lens_camera(int projection, double dfov_deg, int width, int height, double cx, double cy, double K[9]) {
    Mat3 k;
    if (!K || !lens_camera(projection, dfov_deg, width, height, cx, cy, k))
        return fail(VSTAB_ERR_INVALID, "vstab_lens_camera: bad projection, field of view or size");
    std::memcpy(K, k.m, sizeof(k.m));
    return VSTAB_OK;
}

static vstab_status undistort_points(const std::string &name, const double *pts, int n, const double K[9], const double *D, const double *R, const double *P,
                                     double *out) {
    if (!pts || !K || !out || n < 0) return fail(VSTAB_ERR_INVALID, name + ": bad argument");
    if (D) VSTAB_TRY(check_distortion(name.c_str(), D));
    Mat3 k, rr = Mat3::identity();
    std::memcpy(k.m, K, sizeof(k.m));
    if (R) std::memcpy(rr.m, R, sizeof(rr.m));
    if (P) {
        Mat3 p;
        std::memcpy(p.m, P, sizeof(p.m));
        rr = p * rr;
    }
    fisheye_undistort(pts, n, k, rr, out, true, D);
    return VSTAB_OK;
}

vstab_status vstab_fisheye_undistort_points(const double *pts, int n, const double K[9], const double *R, const double *P, double *out) {
    return undistort_points("vstab_fisheye_undistort_points", pts, n, K, nullptr, R, P, out);
}

vstab_status vstab_fisheye_undistort_points_d(const double *pts, int n, const double K[9], const double D[4], const double *R, const double *P,
                                              double *out) {
    if (!D) return fail(VSTAB_ERR_INVALID, "vstab_fisheye_undistort_points_d: bad argument");
    return undistort_points("vstab_fisheye_undistort_points_d", pts, n, K, D, R, P, out);
}

vstab_status vstab_undistort_points_pinhole(const double *pts, int n, const double K[9], const double D[5], const double *R, const double *P,
                                            double *out) {
    const std::string name = "vstab_undistort_points_pinhole";
    if (!pts || !K || !D || !out || n < 0) return fail(VSTAB_ERR_INVALID, name + ": bad argument");
    VSTAB_TRY(check_pinhole_distortion(name.c_str(), D));
    Mat3 k, rr = Mat3::identity();
    std::memcpy(k.m, K, sizeof(k.m));
    if (R) std::memcpy(rr.m, R, sizeof(rr.m));
    if (P) {
        Mat3 p;
        std::memcpy(p.m, P, sizeof(p.m));
        rr = p * rr;
    }
    fisheye_undistort(pts, n, k, rr, out, false, D);
    return VSTAB_OK;
}

void vstab_map_params(const double K_in[9], const double K_out[9], const double R[9], float params[17]) {
    Mat3 a, b, c;
    std::memcpy(a.m, K_in, sizeof(a.m));
    std::memcpy(b.m, K_out, sizeof(b.m));
    std::memcpy(c.m, R, sizeof(c.m));
    map_params(a, b, c, params);
}

}  // extern "C"

extern "C" void vstab_time_next_launch(void *start_event, void *stop_event) {
    vstab::set_launch_events(static_cast<hipEvent_t>(start_event), static_cast<hipEvent_t>(stop_event));
}
