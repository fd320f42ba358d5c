/*
 * vstab_oracle.c -- CPU restatement of the reference hot path (TEST INFRASTRUCTURE ONLY).
 *
 * This file is the parity oracle for the HIP implementation in video-annotator_amd/csrc/.
 * It is NOT part of the product: only tests/, __graft_entry__.smoke() and bench.py's
 * cpu_baseline leg may load it.  The product library never links or calls it.
 *
 * Each function restates one step of the reference pipeline
 * (/root/reference/opencv/FrameSourceWarp.cpp, createMap.cl, FrameSourceFfmpegOpenCl.cpp).
 * Where the arithmetic lives in a third-party dependency that is absent from the reference
 * tree (OpenCV >= 4.5, meson.build:33; gram_savitzky_golay, meson.build:37) the published
 * algorithm of that dependency is restated and the function says so.
 *
 * PARITY PINNING
 *   - vo_create_map is pinned against the reference's own createMap.cl compiled for x86-64
 *     (oracle/_ref, see oracle/Makefile) -- identical except for the atan implementation
 *     (see vo_atanf) -- and against golden vectors generated from that build (tests/golden).
 *   - every OpenCV-derived function below is "parity unpinned": the reference holds no tests,
 *     fixtures or golden vectors and OpenCV is not installed in the build image.
 *
 * Floating point: compile with -ffp-contract=off and without -ffast-math.  Every fused
 * multiply-add below is an explicit fmaf(); every other operation is a single IEEE-754
 * binary32 operation, so the HIP kernels can reproduce the results bit for bit.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <limits.h>
#include <float.h>

#ifdef _OPENMP
#include <omp.h>
#endif

#define VO_API __attribute__((visibility("default")))

VO_API int vo_num_threads(void) {
#ifdef _OPENMP
    return omp_get_max_threads();
#else
    return 1;
#endif
}

VO_API void vo_set_num_threads(int n) {
#ifdef _OPENMP
    omp_set_num_threads(n);
#else
    (void)n;
#endif
}

/* ------------------------------------------------------------------------------------------
 * a1: NV12 plane packing.  FrameSourceFfmpegOpenCl.cpp:58-85 -- two image->buffer copies:
 * luma (w x h bytes) at offset 0, chroma (w/2 x h/2 two-byte texels) at offset w*h.
 * ------------------------------------------------------------------------------------------ */
VO_API int vo_pack_nv12(const uint8_t *y, size_t pitch_y, const uint8_t *uv, size_t pitch_uv,
                        int w, int h, uint8_t *dst) {
    if ((w & 1) || (h & 1) || w <= 0 || h <= 0) return 1; /* "Mismatched image dimensions", :53 */
    for (int r = 0; r < h; r++) memcpy(dst + (size_t)r * w, y + (size_t)r * pitch_y, (size_t)w);
    uint8_t *d = dst + (size_t)w * h;
    for (int r = 0; r < h / 2; r++) memcpy(d + (size_t)r * w, uv + (size_t)r * pitch_uv, (size_t)w);
    return 0;
}

/* ------------------------------------------------------------------------------------------
 * a2: cvtColor(COLOR_YUV2BGR_NV12), call site FrameSourceWarp.cpp:401.
 * Third-party arithmetic (OpenCV 4.5 imgproc color_yuv, CPU path): integer
 * BT.601 limited range, 20-bit fixed point.  nv12 = packed (h*3/2) x w bytes.
 * ------------------------------------------------------------------------------------------ */
#define VO_CY 1220542
#define VO_CUB 2116026
#define VO_CUG (-409993)
#define VO_CVG (-852492)
#define VO_CVR 1673527
#define VO_YUV_SHIFT 20

static inline uint8_t vo_sat8(int v) { return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v); }

static inline void vo_yuv_to_bgr(int Y, int U, int V, uint8_t *bgr) {
    int u = U - 128, v = V - 128;
    int ruv = (1 << (VO_YUV_SHIFT - 1)) + VO_CVR * v;
    int guv = (1 << (VO_YUV_SHIFT - 1)) + VO_CVG * v + VO_CUG * u;
    int buv = (1 << (VO_YUV_SHIFT - 1)) + VO_CUB * u;
    int y = (Y - 16 > 0 ? Y - 16 : 0) * VO_CY;
    bgr[0] = vo_sat8((y + buv) >> VO_YUV_SHIFT);
    bgr[1] = vo_sat8((y + guv) >> VO_YUV_SHIFT);
    bgr[2] = vo_sat8((y + ruv) >> VO_YUV_SHIFT);
}

VO_API void vo_cvt_nv12_bgr(const uint8_t *nv12, int w, int h, uint8_t *bgr) {
    const uint8_t *yp = nv12, *uvp = nv12 + (size_t)w * h;
#pragma omp parallel for schedule(static)
    for (int r = 0; r < h; r++) {
        const uint8_t *yrow = yp + (size_t)r * w;
        const uint8_t *uvrow = uvp + (size_t)(r >> 1) * w;
        uint8_t *o = bgr + (size_t)r * w * 3;
        for (int c = 0; c < w; c++)
            vo_yuv_to_bgr(yrow[c], uvrow[c & ~1], uvrow[(c & ~1) + 1], o + 3 * c);
    }
}

/* 10-bit input (BASELINE config 5, no reference counterpart): P010 / P016 planes -- 16-bit little-endian
 * samples with the significant bits at the top, pitches in bytes -- narrowed to packed 8-bit NV12 by
 * truncation (sample >> 8).  DEFINED here; the rest of the path is the reference's 8-bit path. */
VO_API int vo_pack_p010(const uint8_t *y, size_t pitch_y, const uint8_t *uv, size_t pitch_uv, int w, int h, uint8_t *dst) {
    if (w <= 0 || h <= 0 || (w & 1) || (h & 1)) return -1;
    for (int r = 0; r < h + h / 2; r++) {
        const uint8_t *s = r < h ? y + (size_t)r * pitch_y : uv + (size_t)(r - h) * pitch_uv;
        for (int c = 0; c < w; c++) dst[(size_t)r * w + c] = (uint8_t)(((unsigned)s[2 * c] | ((unsigned)s[2 * c + 1] << 8)) >> 8);
    }
    return 0;
}

/* ------------------------------------------------------------------------------------------
 * atan used by the map.  OpenCL leaves atan() implementation defined (<= 5 ulp); the x86
 * build of the reference kernel (oracle/_ref) uses libm atanf.  To let a GPU kernel match
 * this restatement bit for bit the restatement fixes ONE algorithm built only from IEEE
 * operations and fmaf: x > 1 -> pi/2 - atan(1/x); atan(t) = t + t*s*q(s), s = t*t, q a
 * degree-7 minimax polynomial (max error < 1 ulp on [0, inf), verified exhaustively in
 * tests).  Argument must be >= 0 or NaN (it is a vector length).
 * ------------------------------------------------------------------------------------------ */
static const float VO_ATAN_Q[8] = {
    -0.33333125710487366f, 0.19993145763874054f,  -0.14205896854400635f, 0.1064559817314148f,
    -0.07508683204650879f, 0.04269874095916748f,  -0.016053270548582077f, 0.0028423243202269077f};
#define VO_PIO2_HI 1.57079637050628662109375f
#define VO_PIO2_LO (-4.37113900018624283e-8f)

VO_API float vo_atanf(float x) {
    int inv = x > 1.0f;
    float t = inv ? 1.0f / x : x;
    float s = t * t;
    float q = VO_ATAN_Q[7];
    for (int i = 6; i >= 0; i--) q = fmaf(q, s, VO_ATAN_Q[i]);
    float r = fmaf(t * s, q, t);
    if (inv) r = (VO_PIO2_HI - r) + VO_PIO2_LO;
    return r;
}

VO_API void vo_atanf_array(const float *x, float *y, long n) {
    for (long i = 0; i < n; i++) y[i] = vo_atanf(x[i]);
}

/* max ulp error of vo_atanf over every binary32 in [lo_bits, hi_bits) vs double atan */
VO_API double vo_atanf_max_ulp(uint32_t lo_bits, uint32_t hi_bits, uint32_t stride) {
    double worst = 0;
#pragma omp parallel for reduction(max : worst) schedule(static)
    for (int64_t b = lo_bits; b < (int64_t)hi_bits; b += stride) {
        uint32_t u = (uint32_t)b;
        float x;
        memcpy(&x, &u, 4);
        float a = vo_atanf(x);
        double ref = atan((double)x);
        float rf = (float)ref;
        double ulp = (double)nextafterf(rf, INFINITY) - (double)rf;
        double e = fabs((double)a - ref) / ulp;
        if (e > worst) worst = e;
    }
    return worst;
}

/* ------------------------------------------------------------------------------------------
 * a9: createMap.cl:1-51 restated.  p[17] = the 17 cl_float scalars in kernel-argument order
 * (FrameSourceWarp.cpp:283-299): src cx,cy,fx,fy ; map(out) cx,cy,fx,fy ; rot00..rot22.
 * dot() = products summed left to right, unfused (createMap.cl:27-31); length() =
 * sqrtf(x*x+y*y) (createMap.cl:38); map planes are dense cols-wide float arrays.
 * ------------------------------------------------------------------------------------------ */
static inline void vo_map_pixel(int x, int y, const float *p, float *mx, float *my) {
    float vx = ((float)x - p[4]) / p[6];
    float vy = ((float)y - p[5]) / p[7];
    float wx = (p[8] * vx + p[9] * vy) + p[10];
    float wy = (p[11] * vx + p[12] * vy) + p[13];
    float wz = (p[14] * vx + p[15] * vy) + p[16];
    float cx = wx / wz, cy = wy / wz;
    float r = sqrtf(cx * cx + cy * cy);
    float k = vo_atanf(r) / r;
    *mx = p[0] + (cx * k) * p[2];
    *my = p[1] + (cy * k) * p[3];
}

VO_API void vo_create_map(float *mapx, float *mapy, int cols, int rows, const float *p) {
#pragma omp parallel for schedule(static)
    for (int y = 0; y < rows; y++)
        for (int x = 0; x < cols; x++)
            vo_map_pixel(x, y, p, mapx + (size_t)y * cols + x, mapy + (size_t)y * cols + x);
}

/* ------------------------------------------------------------------------------------------
 * a10: cv::remap(src, dst, mapx, mapy, INTER_LINEAR), BORDER_CONSTANT 0; call site
 * FrameSourceWarp.cpp:306-312.  Third-party arithmetic (OpenCV 4.5 imgproc remap, CPU path;
 * SURVEY.md A.6): coordinates quantised to 1/32 px, 15-bit weights, round half up.
 * ------------------------------------------------------------------------------------------ */
static inline int vo_cvround(float v) {
    /* cvRound = SSE cvtss2si: round half even; NaN / out of int range -> INT_MIN */
    if (!(v >= -2147483648.0f && v < 2147483648.0f)) return INT_MIN;
    return (int)lrintf(v);
}

static inline int vo_sat16(int v) { return v < -32768 ? -32768 : v > 32767 ? 32767 : v; }

static inline void vo_remap_pixel(const uint8_t *src, int sw, int sh, int cn, float mx, float my,
                                  uint8_t *out) {
    int sx = vo_cvround(mx * 32.0f), sy = vo_cvround(my * 32.0f);
    int X = vo_sat16(sx >> 5), Y = vo_sat16(sy >> 5);
    int fx = sx & 31, fy = sy & 31;
    if (X >= sw || X + 1 < 0 || Y >= sh || Y + 1 < 0) {
        for (int c = 0; c < cn; c++) out[c] = 0;
        return;
    }
    int w00 = (32 - fx) * (32 - fy), w01 = fx * (32 - fy), w10 = (32 - fx) * fy, w11 = fx * fy;
    int in00 = X >= 0 && Y >= 0, in01 = X + 1 < sw && Y >= 0;
    int in10 = X >= 0 && Y + 1 < sh, in11 = X + 1 < sw && Y + 1 < sh;
    for (int c = 0; c < cn; c++) {
        int p00 = in00 ? src[((size_t)Y * sw + X) * cn + c] : 0;
        int p01 = in01 ? src[((size_t)Y * sw + X + 1) * cn + c] : 0;
        int p10 = in10 ? src[((size_t)(Y + 1) * sw + X) * cn + c] : 0;
        int p11 = in11 ? src[((size_t)(Y + 1) * sw + X + 1) * cn + c] : 0;
        /* weights*32 sum to 1<<15; (v + (1<<14)) >> 15 == (v' + 512) >> 10 */
        out[c] = vo_sat8((p00 * w00 + p01 * w01 + p10 * w10 + p11 * w11 + 512) >> 10);
    }
}

VO_API void vo_remap_bilinear(const uint8_t *src, int sw, int sh, int cn, const float *mapx,
                              const float *mapy, uint8_t *dst, int dw, int dh) {
#pragma omp parallel for schedule(static)
    for (int y = 0; y < dh; y++)
        for (int x = 0; x < dw; x++)
            vo_remap_pixel(src, sw, sh, cn, mapx[(size_t)y * dw + x], mapy[(size_t)y * dw + x],
                           dst + ((size_t)y * dw + x) * cn);
}

/* cv::remap(INTER_NEAREST, BORDER_CONSTANT 0) -- FrameSourceWarp.hpp:90 lets the caller choose the interpolation and
 * :311 passes it on; the reference itself only ever passes INTER_LINEAR.  OpenCV 4.5 CPU path: the float maps are
 * converted with cvRound (round half to even) and saturate_cast<short>, a pixel outside the source is the border value. */
VO_API void vo_remap_nearest(const uint8_t *src, int sw, int sh, int cn, const float *mapx, const float *mapy, uint8_t *dst, int dw, int dh) {
#pragma omp parallel for schedule(static)
    for (int y = 0; y < dh; y++)
        for (int x = 0; x < dw; x++) {
            const int sx = vo_sat16(vo_cvround(mapx[(size_t)y * dw + x])), sy = vo_sat16(vo_cvround(mapy[(size_t)y * dw + x]));
            uint8_t *o = dst + ((size_t)y * dw + x) * cn;
            for (int c = 0; c < cn; c++) o[c] = (unsigned)sx < (unsigned)sw && (unsigned)sy < (unsigned)sh ? src[((size_t)sy * sw + sx) * cn + c] : 0;
        }
}

/* a2+a9+a10 as the reference runs them (FrameSourceWarp.cpp:401 then :272-314): full-frame
 * colour conversion, map planes written to memory, remap reading them back.  `work` must
 * hold w*h*3 + 2*dw*dh*4 bytes.  Used as the CPU baseline in bench.py. */
VO_API void vo_warp_nv12_reference_path(const uint8_t *nv12, int w, int h, const float *p,
                                        uint8_t *dst, int dw, int dh, uint8_t *work) {
    uint8_t *bgr = work;
    float *mapx = (float *)(work + (((size_t)w * h * 3 + 15) & ~(size_t)15));
    float *mapy = mapx + (size_t)dw * dh;
    vo_cvt_nv12_bgr(nv12, w, h, bgr);
    vo_create_map(mapx, mapy, dw, dh, p);
    vo_remap_bilinear(bgr, w, h, 3, mapx, mapy, dst, dw, dh);
}

/* ------------------------------------------------------------------------------------------
 * f1: the libdewobble-style camera surface the CLI drives
 * (render.ts:611-617, 669-683, 711-717): in_p / out_p in {fish, rect}.  libdewobble itself is
 * NOT in the reference tree (third-party ffmpeg filter, unpinned), so this map has no reference
 * output to pin against -- "parity unpinned": the arithmetic is DEFINED here, chosen so that
 * mode fish->rect performs exactly the createMap.cl operations wherever those are well defined,
 * and differs from createMap.cl only in the two degenerate cases it mishandles:
 *   - the ray that hits the optical axis (radius 0): createMap.cl divides 0/0 and blacks the
 *     pixel out; here the correction factor is 1 (its limit);
 *   - rays behind the camera (w.z <= 0): createMap.cl mirrors them; here they are outside.
 * Modes: 1 fish->rect, 2 fish->fish, 3 rect->rect, 4 rect->fish (input -> output projection);
 * fish = equidistant (r = f*theta), rect = pinhole (r = f*tan(theta)).
 * ------------------------------------------------------------------------------------------ */
#define VO_PI_F 3.1415927410125732421875f
#define VO_TWO_OVER_PI 0.636619746685028076171875f

/* sin and cos of t in [0, pi]: quadrant k = rint(t*2/pi), r = t - k*pi/2 (two-constant Cody-Waite
 * with fmaf), degree-7 / degree-8 polynomials on |r| <= pi/4 (Cephes single-precision
 * coefficients), then the quadrant symmetry.  Built from IEEE operations and fmaf only, so a GPU
 * kernel can match it bit for bit. */
VO_API void vo_sincosf_pos(float t, float *sn, float *cs) {
    float k = rintf(t * VO_TWO_OVER_PI);
    float r = fmaf(k, -VO_PIO2_HI, t);
    r = fmaf(k, -VO_PIO2_LO, r);
    float z = r * r;
    float ps = fmaf(fmaf(-1.9515295891e-4f, z, 8.3321608736e-3f), z, -1.6666654611e-1f);
    float pc = fmaf(fmaf(2.443315711809948e-5f, z, -1.388731625493765e-3f), z, 4.166664568298827e-2f);
    float s = fmaf(r * z, ps, r);
    float c = fmaf(z * z, pc, fmaf(-0.5f, z, 1.0f));
    if (k == 1.0f) *sn = c, *cs = -s;
    else if (k == 2.0f) *sn = -s, *cs = -c;
    else *sn = s, *cs = c;
}

VO_API void vo_sincosf_array(const float *t, float *sn, float *cs, long n) {
    for (long i = 0; i < n; i++) vo_sincosf_pos(t[i], sn + i, cs + i);
}

static inline void vo_map_pixel_ex(int x, int y, const float *p, int mode, float *mx, float *my) {
    const int out_fish = mode == 2 || mode == 4, in_fish = mode == 1 || mode == 2;
    float vx = ((float)x - p[4]) / p[6];
    float vy = ((float)y - p[5]) / p[7];
    float rx = vx, ry = vy, rz = 1.0f;
    *mx = *my = NAN;
    if (out_fish) {
        float rho = sqrtf(vx * vx + vy * vy); /* = theta of the output ray */
        if (!(rho < VO_PI_F)) return;
        float sn, cs;
        vo_sincosf_pos(rho, &sn, &cs);
        float s = rho == 0.0f ? 1.0f : sn / rho;
        rx = vx * s, ry = vy * s, rz = cs;
    }
    float wx = (p[8] * rx + p[9] * ry) + p[10] * rz;
    float wy = (p[11] * rx + p[12] * ry) + p[13] * rz;
    float wz = (p[14] * rx + p[15] * ry) + p[16] * rz;
    if (!(wz > 0.0f)) return;
    float cx = wx / wz, cy = wy / wz;
    if (in_fish) {
        float r = sqrtf(cx * cx + cy * cy);
        float k = r == 0.0f ? 1.0f : vo_atanf(r) / r;
        *mx = p[0] + (cx * k) * p[2];
        *my = p[1] + (cy * k) * p[3];
    } else {
        *mx = p[0] + cx * p[2];
        *my = p[1] + cy * p[3];
    }
}

/* mode 0 = createMap.cl (vo_create_map); 1..4 as above */
VO_API void vo_create_map_ex(float *mapx, float *mapy, int cols, int rows, const float *p, int mode) {
    if (mode == 0) {
        vo_create_map(mapx, mapy, cols, rows, p);
        return;
    }
#pragma omp parallel for schedule(static)
    for (int y = 0; y < rows; y++)
        for (int x = 0; x < cols; x++)
            vo_map_pixel_ex(x, y, p, mode, mapx + (size_t)y * cols + x, mapy + (size_t)y * cols + x);
}

/* ------------------------------------------------------------------------------------------
 * BASELINE config 5 (no reference counterpart; arithmetic defined by this project): rolling-shutter warp.  Output row y
 * is mapped with its own matrix, the nine entries interpolated in fp32 between the rotation of the first row (p[8..16])
 * and the rotation of the last row (rot_bottom):  t = (float)y / (float)max(rows - 1, 1)  (IEEE division),
 * d_k = rot_bottom[k] - p[8 + k],  m_k = fmaf(t, d_k, p[8 + k]);  then the map arithmetic of `mode` (0 = createMap.cl,
 * 1 = fish -> rect) with m in place of the rotation.  No re-orthonormalisation: the two rotations are a frame apart.
 * ------------------------------------------------------------------------------------------ */
VO_API void vo_create_map_rs(float *mapx, float *mapy, int cols, int rows, const float *p, const float *rot_bottom, int mode) {
    float d[9];
    for (int k = 0; k < 9; k++) d[k] = rot_bottom[k] - p[8 + k];
    const float den = (float)(rows > 1 ? rows - 1 : 1);
#pragma omp parallel for schedule(static)
    for (int y = 0; y < rows; y++) {
        float q[17];
        memcpy(q, p, sizeof q);
        const float t = (float)y / den;
        for (int k = 0; k < 9; k++) q[8 + k] = fmaf(t, d[k], p[8 + k]);
        for (int x = 0; x < cols; x++) {
            if (mode == 0)
                vo_map_pixel(x, y, q, mapx + (size_t)y * cols + x, mapy + (size_t)y * cols + x);
            else
                vo_map_pixel_ex(x, y, q, mode, mapx + (size_t)y * cols + x, mapy + (size_t)y * cols + x);
        }
    }
}

/* ------------------------------------------------------------------------------------------
 * f2: NV12 output for the encoder hand-off (render.ts:275-281).
 * The reference's C++ path stops at BGR; the conversion is DEFINED as OpenCV 4.5's
 * cvtColor(COLOR_BGR2YUV_I420) arithmetic (imgproc color_yuv, RGB8toYUV420pInvoker: BT.601
 * limited range, 20-bit fixed point, chroma taken from the top-left pixel of each 2x2 block, no
 * averaging) with U and V interleaved as NV12.  Odd sizes: chroma planes are ceil(w/2) x
 * ceil(h/2) (every 2x2 block's top-left pixel exists).  y: w x h, uv: 2*ceil(w/2) x ceil(h/2).
 * ------------------------------------------------------------------------------------------ */
#define VO_CRY 269484
#define VO_CGY 528482
#define VO_CBY 102760
#define VO_CRU (-155188)
#define VO_CGU (-305135)
#define VO_CBU 460324
#define VO_CGV (-385875)
#define VO_CBV (-74448)

VO_API void vo_cvt_bgr_nv12(const uint8_t *bgr, int w, int h, uint8_t *yp, uint8_t *uvp) {
    const int half = 1 << 19, s16 = 16 << 20, s128 = 128 << 20;
    const int cw = (w + 1) / 2;
#pragma omp parallel for schedule(static)
    for (int r = 0; r < h; r++) {
        const uint8_t *row = bgr + (size_t)r * w * 3;
        for (int c = 0; c < w; c++) {
            int B = row[3 * c], G = row[3 * c + 1], R = row[3 * c + 2];
            yp[(size_t)r * w + c] = vo_sat8((VO_CRY * R + VO_CGY * G + VO_CBY * B + half + s16) >> 20);
            if (!(r & 1) && !(c & 1)) {
                uint8_t *o = uvp + ((size_t)(r >> 1) * cw + (c >> 1)) * 2;
                o[0] = vo_sat8((VO_CRU * R + VO_CGU * G + VO_CBU * B + half + s128) >> 20);
                o[1] = vo_sat8((VO_CBU * R + VO_CGV * G + VO_CBV * B + half + s128) >> 20);
            }
        }
    }
}

/* 10-bit BGR (values 0..1023 in 16-bit containers) -> P010 (16-bit samples, the 10 significant bits at the top; chroma interleaved
 * U, V at half resolution from the top-left pixel of each 2 x 2 block): vo_cvt_bgr_nv12's arithmetic at 10 bits -- the same
 * BT.601 constants and 20-bit shift, offsets 64 / 512, saturation to [0, 1023].  DEFINED here (config 5's encoder hand-off has no
 * reference counterpart).  All sums fit int32: 1023 * (CRY + CGY + CBY) + (64 << 20) + (1 << 19) < 2^30. */
static inline int vo_sat10i(int v) { return v < 0 ? 0 : v > 1023 ? 1023 : v; }
VO_API void vo_cvt_bgr10_p010(const uint16_t *bgr, int w, int h, uint16_t *yp, uint16_t *uvp) {
    const int half = 1 << 19, s64 = 64 << 20, s512 = 512 << 20;
    const int cw = (w + 1) / 2;
#pragma omp parallel for schedule(static)
    for (int r = 0; r < h; r++) {
        const uint16_t *row = bgr + (size_t)r * w * 3;
        for (int c = 0; c < w; c++) {
            const int B = row[3 * c], G = row[3 * c + 1], R = row[3 * c + 2];
            yp[(size_t)r * w + c] = (uint16_t)(vo_sat10i((VO_CRY * R + VO_CGY * G + VO_CBY * B + half + s64) >> 20) << 6);
            if (!(r & 1) && !(c & 1)) {
                uint16_t *o = uvp + ((size_t)(r >> 1) * cw + (c >> 1)) * 2;
                o[0] = (uint16_t)(vo_sat10i((VO_CRU * R + VO_CGU * G + VO_CBU * B + half + s512) >> 20) << 6);
                o[1] = (uint16_t)(vo_sat10i((VO_CBU * R + VO_CGV * G + VO_CBV * B + half + s512) >> 20) << 6);
            }
        }
    }
}

/* the generalised warp as a reference-style chain: cvtColor, map planes (mode), remap,
 * optional BGR -> NV12.  out_format 0: dst = BGR (dw*dh*3); 1: dst = Y plane then the
 * interleaved chroma plane (dw*dh + 2*ceil(dw/2)*ceil(dh/2) bytes).  work as for
 * vo_warp_nv12_reference_path plus dw*dh*3 bytes when out_format = 1. */
VO_API void vo_warp_nv12_ex(const uint8_t *nv12, int w, int h, const float *p, int mode, int out_format,
                            uint8_t *dst, int dw, int dh, uint8_t *work) {
    uint8_t *bgr = work;
    float *mapx = (float *)(work + (((size_t)w * h * 3 + 15) & ~(size_t)15));
    float *mapy = mapx + (size_t)dw * dh;
    uint8_t *tmp = (uint8_t *)(mapy + (size_t)dw * dh);
    vo_cvt_nv12_bgr(nv12, w, h, bgr);
    vo_create_map_ex(mapx, mapy, dw, dh, p, mode);
    if (out_format == 0) {
        vo_remap_bilinear(bgr, w, h, 3, mapx, mapy, dst, dw, dh);
    } else {
        vo_remap_bilinear(bgr, w, h, 3, mapx, mapy, tmp, dw, dh);
        vo_cvt_bgr_nv12(tmp, dw, dh, dst, dst + (size_t)dw * dh);
    }
}

/* the rolling-shutter warp as a reference-style chain (cvtColor, per-row map planes, remap, optional BGR -> NV12);
 * buffers as vo_warp_nv12_ex */
VO_API void vo_warp_nv12_rs(const uint8_t *nv12, int w, int h, const float *p, const float *rot_bottom, int mode, int out_format,
                            uint8_t *dst, int dw, int dh, uint8_t *work) {
    uint8_t *bgr = work;
    float *mapx = (float *)(work + (((size_t)w * h * 3 + 15) & ~(size_t)15));
    float *mapy = mapx + (size_t)dw * dh;
    uint8_t *tmp = (uint8_t *)(mapy + (size_t)dw * dh);
    vo_cvt_nv12_bgr(nv12, w, h, bgr);
    vo_create_map_rs(mapx, mapy, dw, dh, p, rot_bottom, mode);
    if (out_format == 0) {
        vo_remap_bilinear(bgr, w, h, 3, mapx, mapy, dst, dw, dh);
    } else {
        vo_remap_bilinear(bgr, w, h, 3, mapx, mapy, tmp, dw, dh);
        vo_cvt_bgr_nv12(tmp, dw, dh, dst, dst + (size_t)dw * dh);
    }
}

/* ------------------------------------------------------------------------------------------
 * BASELINE.json config 5: the 10-bit pixel path ("4K P010, fp16 blend, rolling-shutter per-row warp").  The reference
 * is 8-bit throughout, so there is nothing to pin against: the arithmetic is DEFINED here ("parity unpinned") and the
 * HIP operator vstab_warp_p010 reproduces it bit for bit.
 *   samples   P010: 16-bit little-endian, significant bits at the top -> s >> 6 in [0, 1023]
 *   colour    cvtColor's BT.601 constants and shift at 10 bits: offsets 64 (luma) and 512 (chroma), 64-bit sums
 *   map       vo_create_map_ex / vo_create_map_rs
 *   remap     cv::remap's quantisation; blend 0: (sum p*w + 512) >> 10 as the 8-bit path; blend 1 ("fp16 blend"):
 *             acc = fma16(p00, w00/1024, 0), fma16(p01, w01/1024, acc), fma16(p10, ..), fma16(p11, ..) -- each one
 *             fused multiply-add rounded once to binary16, ties to even -- then rint (ties to even), clamp to 1023
 *   output    BGR, 16-bit containers, values 0..1023
 * ------------------------------------------------------------------------------------------ */
static inline uint16_t vo_sat10(long long v) { return (uint16_t)(v < 0 ? 0 : v > 1023 ? 1023 : v); }

static inline void vo_yuv10_to_bgr10(int Y, int U, int V, uint16_t *bgr) {
    long long u = U - 512, v = V - 512;
    long long ruv = (1 << (VO_YUV_SHIFT - 1)) + VO_CVR * v;
    long long guv = (1 << (VO_YUV_SHIFT - 1)) + VO_CVG * v + VO_CUG * u;
    long long buv = (1 << (VO_YUV_SHIFT - 1)) + VO_CUB * u;
    long long y = (long long)(Y - 64 > 0 ? Y - 64 : 0) * VO_CY;
    bgr[0] = vo_sat10((y + buv) >> VO_YUV_SHIFT);
    bgr[1] = vo_sat10((y + guv) >> VO_YUV_SHIFT);
    bgr[2] = vo_sat10((y + ruv) >> VO_YUV_SHIFT);
}

static inline int vo_p010_sample(const uint8_t *row, int i) { return (int)(((unsigned)row[2 * i] | ((unsigned)row[2 * i + 1] << 8)) >> 6); }

VO_API void vo_cvt_p010_bgr10(const uint8_t *y, size_t pitch_y, const uint8_t *uv, size_t pitch_uv, int w, int h, uint16_t *bgr) {
#pragma omp parallel for schedule(static)
    for (int r = 0; r < h; r++) {
        const uint8_t *yrow = y + (size_t)r * pitch_y, *crow = uv + (size_t)(r >> 1) * pitch_uv;
        for (int c = 0; c < w; c++)
            vo_yuv10_to_bgr10(vo_p010_sample(yrow, c), vo_p010_sample(crow, c & ~1), vo_p010_sample(crow, (c & ~1) + 1), bgr + ((size_t)r * w + c) * 3);
    }
}

/* round an exactly known real (held in a double) to IEEE binary16, ties to even; returned as a double */
static inline double vo_round_f16(double v) {
    if (v == 0.0) return v;
    int e;
    frexp(v, &e);                 /* |v| = m * 2^e, m in [0.5, 1) -> binary exponent e - 1 */
    int ex = e - 1 < -14 ? -14 : e - 1;
    double q = ldexp(1.0, ex - 10);
    return nearbyint(v / q) * q;  /* default rounding mode: ties to even */
}

static inline uint16_t vo_blend_f16(int p00, int p01, int p10, int p11, int w00, int w01, int w10, int w11) {
    double acc = 0.0;
    acc = vo_round_f16((double)p00 * ((double)w00 / 1024.0) + acc);  /* operands are exact binary16 values; the sum is exact in double */
    acc = vo_round_f16((double)p01 * ((double)w01 / 1024.0) + acc);
    acc = vo_round_f16((double)p10 * ((double)w10 / 1024.0) + acc);
    acc = vo_round_f16((double)p11 * ((double)w11 / 1024.0) + acc);
    long v = lrint(acc);
    return (uint16_t)(v > 1023 ? 1023 : v);
}

static inline void vo_remap_pixel10(const uint16_t *src, int sw, int sh, float mx, float my, int blend, uint16_t *out) {
    int sx = vo_cvround(mx * 32.0f), sy = vo_cvround(my * 32.0f);
    int X = vo_sat16(sx >> 5), Y = vo_sat16(sy >> 5);
    int fx = sx & 31, fy = sy & 31;
    if (X >= sw || X + 1 < 0 || Y >= sh || Y + 1 < 0) {
        out[0] = out[1] = out[2] = 0;
        return;
    }
    int w00 = (32 - fx) * (32 - fy), w01 = fx * (32 - fy), w10 = (32 - fx) * fy, w11 = fx * fy;
    int in00 = X >= 0 && Y >= 0, in01 = X + 1 < sw && Y >= 0;
    int in10 = X >= 0 && Y + 1 < sh, in11 = X + 1 < sw && Y + 1 < sh;
    for (int c = 0; c < 3; c++) {
        int p00 = in00 ? src[((size_t)Y * sw + X) * 3 + c] : 0;
        int p01 = in01 ? src[((size_t)Y * sw + X + 1) * 3 + c] : 0;
        int p10 = in10 ? src[((size_t)(Y + 1) * sw + X) * 3 + c] : 0;
        int p11 = in11 ? src[((size_t)(Y + 1) * sw + X + 1) * 3 + c] : 0;
        out[c] = blend ? vo_blend_f16(p00, p01, p10, p11, w00, w01, w10, w11)
                       : (uint16_t)((p00 * w00 + p01 * w01 + p10 * w10 + p11 * w11 + 512) >> 10);
    }
}

/* The 10-bit remap on its own: 10-bit BGR frame (vo_cvt_p010_bgr10) + map planes -> 10-bit BGR.  Lets a test feed map planes
 * that did not come from this file -- the reference's own createMap kernel run on the GPU (oracle/_ref/createMap.gfx950.co). */
VO_API void vo_remap_bilinear10(const uint16_t *bgr, int w, int h, const float *mapx, const float *mapy, int blend, uint16_t *dst, int dw, int dh) {
#pragma omp parallel for schedule(static)
    for (int yy = 0; yy < dh; yy++)
        for (int x = 0; x < dw; x++)
            vo_remap_pixel10(bgr, w, h, mapx[(size_t)yy * dw + x], mapy[(size_t)yy * dw + x], blend, dst + ((size_t)yy * dw + x) * 3);
}

/* work: w*h*6 + 16 + 2*dw*dh*4 bytes.  rot_bottom may be NULL (one rotation for the frame). */
VO_API void vo_warp_p010(const uint8_t *y, size_t pitch_y, const uint8_t *uv, size_t pitch_uv, int w, int h, const float *p,
                         const float *rot_bottom, int mode, int blend, uint16_t *dst, int dw, int dh, uint8_t *work) {
    uint16_t *bgr = (uint16_t *)work;
    float *mapx = (float *)(work + (((size_t)w * h * 6 + 15) & ~(size_t)15));
    float *mapy = mapx + (size_t)dw * dh;
    vo_cvt_p010_bgr10(y, pitch_y, uv, pitch_uv, w, h, bgr);
    if (rot_bottom)
        vo_create_map_rs(mapx, mapy, dw, dh, p, rot_bottom, mode);
    else if (mode == 0)
        vo_create_map(mapx, mapy, dw, dh, p);
    else
        vo_create_map_ex(mapx, mapy, dw, dh, p, mode);
#pragma omp parallel for schedule(static)
    for (int yy = 0; yy < dh; yy++)
        for (int x = 0; x < dw; x++)
            vo_remap_pixel10(bgr, w, h, mapx[(size_t)yy * dw + x], mapy[(size_t)yy * dw + x], blend, dst + ((size_t)yy * dw + x) * 3);
}

/* ------------------------------------------------------------------------------------------
 * f2 as SURVEY.md 8(f) row 2 states it: the PLANE-WISE warp, "without a colour round trip" -- what an ffmpeg filter that
 * takes and returns NV12 / P010 surfaces does (render.ts:606-607, 664-665, 688; encoders render.ts:275-281).  The C++
 * prototype stops at BGR and libdewobble is not in the reference tree, so this operator is DEFINED here ("parity unpinned")
 * as what an OpenCV caller would write with the reference's own map:
 *     remap(Y,  Y',  mapx,  mapy,  INTER_LINEAR, BORDER_CONSTANT, Scalar(16))            -- luma, 1 channel
 *     remap(UV, UV', cmapx, cmapy, INTER_LINEAR, BORDER_CONSTANT, Scalar(128, 128))      -- chroma, 2 interleaved channels
 *     cmap(cx, cy) = map(2 cx, 2 cy) * 0.5f,   ceil(dw / 2) x ceil(dh / 2) entries
 *   - luma uses the map and cv::remap's quantisation of the BGR path (vo_remap_pixel): same coordinates, same weights;
 *   - chroma: sample (cx, cy) of either chroma plane sits on luma pixel (2 cx, 2 cy) -- the siting vo_cvt_bgr_nv12 uses when
 *     it takes chroma from the top-left pixel of a 2 x 2 block, and the one cvtColor(NV12 -> BGR) implies when it replicates
 *     a chroma sample over its block.  Source and destination share the convention, so a sample offset common to both
 *     (MPEG-2's half-pixel vertical shift) cancels to first order.  The map entry of that luma pixel, halved (exact in
 *     fp32), is the position in the chroma plane; cv::remap then quantises it like any other map: cvRound(32 * cmap);
 *   - border: limited-range black (Y 16, U = V 128; 64 / 512 at 10 bits) -- what the BGR path's border, cv::remap's
 *     Scalar(0) = black, is in this colour space (vo_cvt_bgr_nv12 of (0, 0, 0)).  A border of 0 would be green.
 *     As in cv::remap, a footprint entirely outside the source gives the border value, and a tap outside it contributes the
 *     border value with its weight;
 *   - 10 bits (P010 words, significant bits at the top): sample = word >> 6, same coordinates and weights, blend 0 exact
 *     ((sum + 512) >> 10), blend 1 the binary16 chain of vo_blend_f16; output word = value << 6.
 * ------------------------------------------------------------------------------------------ */
VO_API void vo_chroma_maps(const float *mapx, const float *mapy, int dw, int dh, float *cmx, float *cmy) {
    const int cw = (dw + 1) / 2, ch = (dh + 1) / 2;
    for (int cy = 0; cy < ch; cy++)
        for (int cx = 0; cx < cw; cx++) {
            cmx[(size_t)cy * cw + cx] = mapx[(size_t)(2 * cy) * dw + 2 * cx] * 0.5f;
            cmy[(size_t)cy * cw + cx] = mapy[(size_t)(2 * cy) * dw + 2 * cx] * 0.5f;
        }
}

/* cv::remap(INTER_LINEAR, BORDER_CONSTANT, border) of one plane: cn interleaved channels (1 or 2), depth 8 (bytes) or 10
 * (16-bit words, sample = word >> 6, stored back << 6).  Pitches in bytes.  border[c]: the constant, as a sample value. */
VO_API void vo_remap_plane(const uint8_t *src, size_t spitch, int sw, int sh, int cn, int depth, const float *mapx, const float *mapy,
                           const int *border, int blend, uint8_t *dst, size_t dpitch, int dw, int dh) {
#pragma omp parallel for schedule(static)
    for (int y = 0; y < dh; y++)
        for (int x = 0; x < dw; x++) {
            const float mx = mapx[(size_t)y * dw + x], my = mapy[(size_t)y * dw + x];
            const int sx = vo_cvround(mx * 32.0f), sy = vo_cvround(my * 32.0f);
            const int X = vo_sat16(sx >> 5), Y = vo_sat16(sy >> 5), fx = sx & 31, fy = sy & 31;
            const int outside = X >= sw || X + 1 < 0 || Y >= sh || Y + 1 < 0;
            const int w00 = (32 - fx) * (32 - fy), w01 = fx * (32 - fy), w10 = (32 - fx) * fy, w11 = fx * fy;
            const int in00 = X >= 0 && Y >= 0, in01 = X + 1 < sw && Y >= 0, in10 = X >= 0 && Y + 1 < sh, in11 = X + 1 < sw && Y + 1 < sh;
            for (int c = 0; c < cn; c++) {
                int v;
                if (outside) {
                    v = border[c];
                } else {
#define VO_TAP(XX, YY, IN) ((IN) ? (depth == 8 ? (int)src[(size_t)(YY) * spitch + (size_t)(XX) * cn + c]                                         \
                                               : vo_p010_sample(src + (size_t)(YY) * spitch, (XX) * cn + c))                                      \
                                 : border[c])
                    const int p00 = VO_TAP(X, Y, in00), p01 = VO_TAP(X + 1, Y, in01), p10 = VO_TAP(X, Y + 1, in10), p11 = VO_TAP(X + 1, Y + 1, in11);
#undef VO_TAP
                    v = blend ? (int)vo_blend_f16(p00, p01, p10, p11, w00, w01, w10, w11) : (p00 * w00 + p01 * w01 + p10 * w10 + p11 * w11 + 512) >> 10;
                }
                if (depth == 8) {
                    dst[(size_t)y * dpitch + (size_t)x * cn + c] = (uint8_t)v;
                } else {
                    uint8_t *o = dst + (size_t)y * dpitch + ((size_t)x * cn + c) * 2;
                    o[0] = (uint8_t)((v << 6) & 255), o[1] = (uint8_t)((v << 6) >> 8);
                }
            }
        }
}

/* The plane-wise warp given luma map planes (from vo_create_map*, or from anywhere else: the reference's own kernel run on the GPU).
 * y / uv: source planes (w x h luma, w/2 x h/2 chroma pairs), dst_y: dw x dh, dst_uv: ceil(dw/2) x ceil(dh/2) pairs, all dense
 * (pitch = row bytes).  work: 2 * ceil(dw/2) * ceil(dh/2) floats. */
VO_API void vo_warp_planar_mapped(const uint8_t *y, size_t pitch_y, const uint8_t *uv, size_t pitch_uv, int w, int h, int depth, const float *mapx,
                                  const float *mapy, int blend, uint8_t *dst_y, uint8_t *dst_uv, int dw, int dh, float *work) {
    const int cw = (dw + 1) / 2, ch = (dh + 1) / 2, bps = depth == 8 ? 1 : 2;
    const int black_y[1] = {depth == 8 ? 16 : 64}, black_uv[2] = {depth == 8 ? 128 : 512, depth == 8 ? 128 : 512};
    float *cmx = work, *cmy = work + (size_t)cw * ch;
    vo_remap_plane(y, pitch_y, w, h, 1, depth, mapx, mapy, black_y, blend, dst_y, (size_t)dw * bps, dw, dh);
    vo_chroma_maps(mapx, mapy, dw, dh, cmx, cmy);
    vo_remap_plane(uv, pitch_uv, w / 2, h / 2, 2, depth, cmx, cmy, black_uv, blend, dst_uv, (size_t)cw * 2 * bps, cw, ch);
}

/* ------------------------------------------------------------------------------------------
 * a3: goodFeaturesToTrack(gray, 200, 0.01, 30), call site FrameSourceWarp.cpp:230.
 * Third-party arithmetic (OpenCV 4.5 imgproc featureselect/corner, CPU path).
 * ------------------------------------------------------------------------------------------ */
static inline int vo_reflect101(int i, int n) {
    if (n == 1) return 0;
    while (i < 0 || i >= n) i = i < 0 ? -i : 2 * n - 2 - i;
    return i;
}

/* cornerMinEigenVal(blockSize 3, ksize 3): Sobel derivatives scaled by 1/(4*3*255), products,
 * un-normalised 3x3 box sum (double accumulator, as OpenCV's boxFilter uses for 32F input),
 * min eigenvalue in float.  gray has row pitch `pitch`.  eig is dense w x h float. */
VO_API void vo_min_eig(const uint8_t *gray, size_t pitch, int w, int h, float *eig) {
    const float scale = (float)(1.0 / (4.0 * 3.0 * 255.0));
    const float k0 = 2.0f * scale, k1 = scale;
    float *dx = (float *)malloc(sizeof(float) * (size_t)w * h);
    float *dy = (float *)malloc(sizeof(float) * (size_t)w * h);
#pragma omp parallel for schedule(static)
    for (int y = 0; y < h; y++) {
        int ym = vo_reflect101(y - 1, h), yp = vo_reflect101(y + 1, h);
        for (int x = 0; x < w; x++) {
            int xm = vo_reflect101(x - 1, w), xp = vo_reflect101(x + 1, w);
            const uint8_t *r0 = gray + (size_t)ym * pitch, *r1 = gray + (size_t)y * pitch,
                          *r2 = gray + (size_t)yp * pitch;
            /* Dx: row [-1 0 1] (exact), column [1 2 1]*scale as (a+c)*k1 + b*k0 */
            float d0 = (float)(r0[xp] - r0[xm]), d1 = (float)(r1[xp] - r1[xm]),
                  d2 = (float)(r2[xp] - r2[xm]);
            dx[(size_t)y * w + x] = (d0 + d2) * k1 + d1 * k0;
            /* Dy: row [1 2 1]*scale as b*k0 + (a+c)*k1, column [-1 0 1] */
            float s0 = (float)r0[x] * k0 + ((float)r0[xm] + (float)r0[xp]) * k1;
            float s2 = (float)r2[x] * k0 + ((float)r2[xm] + (float)r2[xp]) * k1;
            dy[(size_t)y * w + x] = s2 - s0;
        }
    }
#pragma omp parallel for schedule(static)
    for (int y = 0; y < h; y++) {
        for (int x = 0; x < w; x++) {
            double sxx = 0, sxy = 0, syy = 0;
            for (int j = -1; j <= 1; j++) {
                int yy = vo_reflect101(y + j, h);
                for (int i = -1; i <= 1; i++) {
                    int xx = vo_reflect101(x + i, w);
                    float a = dx[(size_t)yy * w + xx], b = dy[(size_t)yy * w + xx];
                    sxx += (double)(a * a);
                    sxy += (double)(a * b);
                    syy += (double)(b * b);
                }
            }
            float a = (float)sxx * 0.5f, b = (float)sxy, c = (float)syy * 0.5f;
            eig[(size_t)y * w + x] = (a + c) - sqrtf((a - c) * (a - c) + b * b);
        }
    }
    free(dx);
    free(dy);
}

typedef struct {
    float v;
    int idx;
} vo_cand;

static int vo_cand_cmp(const void *pa, const void *pb) {
    const vo_cand *a = (const vo_cand *)pa, *b = (const vo_cand *)pb;
    if (a->v > b->v) return -1;
    if (a->v < b->v) return 1;
    return a->idx > b->idx ? -1 : a->idx < b->idx ? 1 : 0; /* ties: later raster position first */
}

/* Full detector.  Returns corner count; xy receives (x,y) pairs in acceptance order.
 * If eig_out != NULL it receives the raw (un-thresholded) response map. */
VO_API int vo_good_features(const uint8_t *gray, size_t pitch, int w, int h, int max_corners,
                            double quality, double min_distance, float *xy, float *eig_out) {
    float *eig = (float *)malloc(sizeof(float) * (size_t)w * h);
    vo_min_eig(gray, pitch, w, h, eig);
    if (eig_out) memcpy(eig_out, eig, sizeof(float) * (size_t)w * h);
    float maxv = 0;
    int any = 0;
    for (size_t i = 0; i < (size_t)w * h; i++)
        if (!any || eig[i] > maxv) maxv = eig[i], any = 1;
    float thr = (float)((double)maxv * quality);
    for (size_t i = 0; i < (size_t)w * h; i++)
        if (!(eig[i] > thr)) eig[i] = 0;
    vo_cand *cand = (vo_cand *)malloc(sizeof(vo_cand) * (size_t)w * h);
    size_t nc = 0;
    for (int y = 1; y < h - 1; y++)
        for (int x = 1; x < w - 1; x++) {
            float v = eig[(size_t)y * w + x];
            if (v == 0) continue;
            float m = v;
            for (int j = -1; j <= 1; j++)
                for (int i = -1; i <= 1; i++) {
                    float n = eig[(size_t)(y + j) * w + (x + i)];
                    if (n > m) m = n;
                }
            if (v == m) cand[nc].v = v, cand[nc].idx = y * w + x, nc++;
        }
    qsort(cand, nc, sizeof(vo_cand), vo_cand_cmp);
    /* the cell is clamped to the longer side before it becomes an int: any larger cell is the same 1 x 1 grid, and lrint of a
     * double beyond long (or of inf) is undefined.  The distance test below runs on min_distance as given. */
    double longer = (double)(w > h ? w : h);
    int cell = (int)lrint(min_distance < longer ? min_distance : longer);
    int n = 0;
    if (cell < 1) {
        for (size_t i = 0; i < nc && (max_corners <= 0 || n < max_corners); i++) {
            xy[2 * n] = (float)(cand[i].idx % w), xy[2 * n + 1] = (float)(cand[i].idx / w);
            n++;
        }
    } else {
        int gw = (w + cell - 1) / cell, gh = (h + cell - 1) / cell;
        /* per-cell singly linked lists of accepted corners */
        int *head = (int *)malloc(sizeof(int) * (size_t)gw * gh);
        int cap = max_corners > 0 ? max_corners : (int)nc + 1;
        int *next = (int *)malloc(sizeof(int) * (size_t)cap);
        for (int i = 0; i < gw * gh; i++) head[i] = -1;
        double md2 = min_distance * min_distance;
        for (size_t i = 0; i < nc; i++) {
            int x = cand[i].idx % w, y = cand[i].idx / w;
            int xc = x / cell, yc = y / cell;
            int x1 = xc - 1 < 0 ? 0 : xc - 1, y1 = yc - 1 < 0 ? 0 : yc - 1;
            int x2 = xc + 1 > gw - 1 ? gw - 1 : xc + 1, y2 = yc + 1 > gh - 1 ? gh - 1 : yc + 1;
            int good = 1;
            for (int yy = y1; yy <= y2 && good; yy++)
                for (int xx = x1; xx <= x2 && good; xx++)
                    for (int j = head[yy * gw + xx]; j >= 0; j = next[j]) {
                        float ddx = (float)x - xy[2 * j], ddy = (float)y - xy[2 * j + 1];
                        if ((double)(ddx * ddx + ddy * ddy) < md2) {
                            good = 0;
                            break;
                        }
                    }
            if (good) {
                xy[2 * n] = (float)x, xy[2 * n + 1] = (float)y;
                next[n] = head[yc * gw + xc];
                head[yc * gw + xc] = n;
                n++;
                if (max_corners > 0 && n == max_corners) break;
            }
        }
        free(head);
        free(next);
    }
    free(cand);
    free(eig);
    return n;
}

/* ------------------------------------------------------------------------------------------
 * a4: calcOpticalFlowPyrLK defaults (win 21x21, maxLevel 3, 30 iterations, eps 0.01,
 * minEigThreshold 1e-4), call site FrameSourceWarp.cpp:252.  Third-party arithmetic
 * (OpenCV 4.5 video/lkpyramid + imgproc/pyramids, CPU path).
 * One documented deviation: OpenCV accumulates A11/A12/A22/b1/b2 in float in a build-specific
 * SIMD lane order; this restatement accumulates the (integer) products exactly in int64 and
 * converts once, which is order free and within OpenCV's own rounding noise.
 * ------------------------------------------------------------------------------------------ */
VO_API void vo_pyr_down(const uint8_t *src, size_t spitch, int sw, int sh, uint8_t *dst,
                        size_t dpitch) {
    int dw = (sw + 1) / 2, dh = (sh + 1) / 2;
    static const int k[5] = {1, 4, 6, 4, 1};
#pragma omp parallel for schedule(static)
    for (int y = 0; y < dh; y++)
        for (int x = 0; x < dw; x++) {
            int sum = 0;
            for (int j = 0; j < 5; j++) {
                int yy = vo_reflect101(2 * y + j - 2, sh);
                int rs = 0;
                for (int i = 0; i < 5; i++) rs += k[i] * src[(size_t)yy * spitch + vo_reflect101(2 * x + i - 2, sw)];
                sum += k[j] * rs;
            }
            dst[(size_t)y * dpitch + x] = (uint8_t)((sum + 128) >> 8);
        }
}

/* calcSharrDeriv: interleaved (dx,dy) int16, dense w x h, computed with REFLECT_101 borders */
VO_API void vo_scharr(const uint8_t *src, size_t pitch, int w, int h, int16_t *deriv) {
#pragma omp parallel for schedule(static)
    for (int y = 0; y < h; y++) {
        const uint8_t *r0 = src + (size_t)vo_reflect101(y - 1, h) * pitch;
        const uint8_t *r1 = src + (size_t)y * pitch;
        const uint8_t *r2 = src + (size_t)vo_reflect101(y + 1, h) * pitch;
        for (int x = 0; x < w; x++) {
            int xm = vo_reflect101(x - 1, w), xp = vo_reflect101(x + 1, w);
            int t0m = (r0[xm] + r2[xm]) * 3 + r1[xm] * 10, t0p = (r0[xp] + r2[xp]) * 3 + r1[xp] * 10;
            int t1m = r2[xm] - r0[xm], t1c = r2[x] - r0[x], t1p = r2[xp] - r0[xp];
            deriv[((size_t)y * w + x) * 2] = (int16_t)(t0p - t0m);
            deriv[((size_t)y * w + x) * 2 + 1] = (int16_t)((t1p + t1m) * 3 + t1c * 10);
        }
    }
}

#define VO_LK_WIN 21
#define VO_LK_MAXLEVEL 3
#define VO_DESCALE(x, n) (((x) + (1 << ((n)-1))) >> (n))

typedef struct {
    int w, h;
    uint8_t *img;   /* dense w x h */
    int16_t *deriv; /* dense w x h x 2, only for the previous image */
} vo_level;

static inline int vo_img_at(const vo_level *L, int x, int y) { /* REFLECT_101 padded read */
    return L->img[(size_t)vo_reflect101(y, L->h) * L->w + vo_reflect101(x, L->w)];
}
static inline int vo_der_at(const vo_level *L, int x, int y, int c) { /* zero padded read */
    if (x < 0 || y < 0 || x >= L->w || y >= L->h) return 0;
    return L->deriv[((size_t)y * L->w + x) * 2 + c];
}

static int vo_build_pyramid(const uint8_t *img, size_t pitch, int w, int h, vo_level *lv,
                            int with_deriv) {
    int nl = 0;
    lv[0].w = w, lv[0].h = h;
    lv[0].img = (uint8_t *)malloc((size_t)w * h);
    for (int r = 0; r < h; r++) memcpy(lv[0].img + (size_t)r * w, img + (size_t)r * pitch, (size_t)w);
    for (int l = 0; l <= VO_LK_MAXLEVEL; l++) {
        if (l > 0) {
            int pw = lv[l - 1].w, ph = lv[l - 1].h;
            int nw = (pw + 1) / 2, nh = (ph + 1) / 2;
            if (nw <= VO_LK_WIN || nh <= VO_LK_WIN) break;
            lv[l].w = nw, lv[l].h = nh;
            lv[l].img = (uint8_t *)malloc((size_t)nw * nh);
            vo_pyr_down(lv[l - 1].img, (size_t)pw, pw, ph, lv[l].img, (size_t)nw);
        }
        lv[l].deriv = NULL;
        if (with_deriv) {
            lv[l].deriv = (int16_t *)malloc(sizeof(int16_t) * 2 * (size_t)lv[l].w * lv[l].h);
            vo_scharr(lv[l].img, (size_t)lv[l].w, lv[l].w, lv[l].h, lv[l].deriv);
        }
        nl = l + 1;
    }
    return nl;
}

static void vo_free_pyramid(vo_level *lv, int nl) {
    for (int l = 0; l < nl; l++) {
        free(lv[l].img);
        free(lv[l].deriv);
    }
}

VO_API int vo_pyramid_levels(int w, int h) {
    int nl = 1;
    for (int l = 1; l <= VO_LK_MAXLEVEL; l++) {
        w = (w + 1) / 2, h = (h + 1) / 2;
        if (w <= VO_LK_WIN || h <= VO_LK_WIN) break;
        nl++;
    }
    return nl;
}

/* cvFloor = SSE cvtss2si and a correction: NaN / out of int range -> INT_MIN (as vo_cvround), which every range test below refuses */
static inline int vo_cvfloor(float v) {
    if (!(v >= -2147483648.0f && v < 2147483648.0f)) return INT_MIN;
    return (int)floorf(v);
}

/* Accumulation of the LK sums.  0 (normative for this project): exact int64 sums converted once.  1: fp32 accumulation in
 * raster order, the literal reading of OpenCV's scalar loop -- only used to MEASURE what the documented
 * deviation is worth (tests/test_oracle_cpu.py); OpenCV's SIMD builds use yet another, lane-wise order. */
static int vo_lk_float_acc = 0;
VO_API void vo_set_lk_accumulation(int mode) { vo_lk_float_acc = mode != 0; }
/* 1 (normative): OpenCV's test of the final position behind the iteration loop.  0: without it -- only to let a test
 * find and show inputs on which the rule decides (tests/test_oracle_cpu.py). */
static int vo_lk_final_check = 1;
VO_API void vo_set_lk_final_check(int on) { vo_lk_final_check = on != 0; }

static inline void vo_lk_sum_max(int64_t *m, int64_t v) {
    if (v < 0) v = -v;
    if (v > *m) *m = v;
}

/* iters (may be NULL): incremented once per Gauss-Newton iteration this call starts (vo_pyr_lk_iterations)
 * sums (may be NULL): 5 int64, raised to the largest |sum A11|, |A12|, |A22| (this level's window) and |b1|, |b2| (every iteration) */
static void vo_lk_point(const vo_level *I, const vo_level *J, int level, int max_level,
                        const float *prev_pt, float *next_pt, uint8_t *status, int *iters, int64_t *sums) {
    const float half = (VO_LK_WIN - 1) * 0.5f;
    const float lscale = (float)(1.0 / (1 << level));
    float ppx = prev_pt[0] * lscale, ppy = prev_pt[1] * lscale;
    float npx, npy;
    if (level == max_level)
        npx = ppx, npy = ppy;
    else
        npx = next_pt[0] * 2.0f, npy = next_pt[1] * 2.0f;
    next_pt[0] = npx, next_pt[1] = npy;
    ppx -= half, ppy -= half;
    int ipx = vo_cvfloor(ppx), ipy = vo_cvfloor(ppy);
    if (ipx < -VO_LK_WIN || ipx >= I->w || ipy < -VO_LK_WIN || ipy >= I->h) {
        if (level == 0) *status = 0;
        return;
    }
    float a = ppx - (float)ipx, b = ppy - (float)ipy;
    const int W_BITS = 14;
    const float FLT_SCALE = 1.0f / (1 << 20);
    int iw00 = (int)lrintf((1.f - a) * (1.f - b) * (1 << W_BITS));
    int iw01 = (int)lrintf(a * (1.f - b) * (1 << W_BITS));
    int iw10 = (int)lrintf((1.f - a) * b * (1 << W_BITS));
    int iw11 = (1 << W_BITS) - iw00 - iw01 - iw10;
    int16_t Iw[VO_LK_WIN * VO_LK_WIN], Ixw[VO_LK_WIN * VO_LK_WIN], Iyw[VO_LK_WIN * VO_LK_WIN];
    int64_t sA11 = 0, sA12 = 0, sA22 = 0;
    float fA11 = 0, fA12 = 0, fA22 = 0;
    for (int y = 0; y < VO_LK_WIN; y++)
        for (int x = 0; x < VO_LK_WIN; x++) {
            int X = ipx + x, Y = ipy + y;
            int ival = VO_DESCALE(vo_img_at(I, X, Y) * iw00 + vo_img_at(I, X + 1, Y) * iw01 +
                                      vo_img_at(I, X, Y + 1) * iw10 + vo_img_at(I, X + 1, Y + 1) * iw11,
                                  W_BITS - 5);
            int ixval = VO_DESCALE(vo_der_at(I, X, Y, 0) * iw00 + vo_der_at(I, X + 1, Y, 0) * iw01 +
                                       vo_der_at(I, X, Y + 1, 0) * iw10 + vo_der_at(I, X + 1, Y + 1, 0) * iw11,
                                   W_BITS);
            int iyval = VO_DESCALE(vo_der_at(I, X, Y, 1) * iw00 + vo_der_at(I, X + 1, Y, 1) * iw01 +
                                       vo_der_at(I, X, Y + 1, 1) * iw10 + vo_der_at(I, X + 1, Y + 1, 1) * iw11,
                                   W_BITS);
            Iw[y * VO_LK_WIN + x] = (int16_t)ival;
            Ixw[y * VO_LK_WIN + x] = (int16_t)ixval;
            Iyw[y * VO_LK_WIN + x] = (int16_t)iyval;
            sA11 += (int64_t)ixval * ixval;
            sA12 += (int64_t)ixval * iyval;
            sA22 += (int64_t)iyval * iyval;
            fA11 += (float)(ixval * ixval), fA12 += (float)(ixval * iyval), fA22 += (float)(iyval * iyval);
        }
    if (sums) vo_lk_sum_max(sums, sA11), vo_lk_sum_max(sums + 1, sA12), vo_lk_sum_max(sums + 2, sA22);
    float A11 = (float)sA11 * FLT_SCALE, A12 = (float)sA12 * FLT_SCALE, A22 = (float)sA22 * FLT_SCALE;
    if (vo_lk_float_acc) A11 = fA11 * FLT_SCALE, A12 = fA12 * FLT_SCALE, A22 = fA22 * FLT_SCALE;
    float D = A11 * A22 - A12 * A12;
    float minEig = ((A22 + A11) - sqrtf((A11 - A22) * (A11 - A22) + (4.f * A12) * A12)) /
                   (float)(2 * VO_LK_WIN * VO_LK_WIN);
    if (minEig < 1e-4f || D < FLT_EPSILON) {
        if (level == 0) *status = 0;
        return;
    }
    D = 1.f / D;
    npx -= half, npy -= half;
    float pdx = 0, pdy = 0;
    const double eps2 = 0.01 * 0.01;
    for (int j = 0; j < 30; j++) {
        if (iters) ++*iters;
        int inx = vo_cvfloor(npx), iny = vo_cvfloor(npy);
        if (inx < -VO_LK_WIN || inx >= J->w || iny < -VO_LK_WIN || iny >= J->h) {
            if (level == 0) *status = 0;
            break;
        }
        a = npx - (float)inx, b = npy - (float)iny;
        iw00 = (int)lrintf((1.f - a) * (1.f - b) * (1 << W_BITS));
        iw01 = (int)lrintf(a * (1.f - b) * (1 << W_BITS));
        iw10 = (int)lrintf((1.f - a) * b * (1 << W_BITS));
        iw11 = (1 << W_BITS) - iw00 - iw01 - iw10;
        int64_t sb1 = 0, sb2 = 0;
        float fb1 = 0, fb2 = 0;
        for (int y = 0; y < VO_LK_WIN; y++)
            for (int x = 0; x < VO_LK_WIN; x++) {
                int X = inx + x, Y = iny + y;
                int diff = VO_DESCALE(vo_img_at(J, X, Y) * iw00 + vo_img_at(J, X + 1, Y) * iw01 +
                                          vo_img_at(J, X, Y + 1) * iw10 + vo_img_at(J, X + 1, Y + 1) * iw11,
                                      W_BITS - 5) -
                           Iw[y * VO_LK_WIN + x];
                sb1 += (int64_t)diff * Ixw[y * VO_LK_WIN + x];
                sb2 += (int64_t)diff * Iyw[y * VO_LK_WIN + x];
                fb1 += (float)(diff * Ixw[y * VO_LK_WIN + x]), fb2 += (float)(diff * Iyw[y * VO_LK_WIN + x]);
            }
        if (sums) vo_lk_sum_max(sums + 3, sb1), vo_lk_sum_max(sums + 4, sb2);
        float b1 = (float)sb1 * FLT_SCALE, b2 = (float)sb2 * FLT_SCALE;
        if (vo_lk_float_acc) b1 = fb1 * FLT_SCALE, b2 = fb2 * FLT_SCALE;
        float dx = (A12 * b2 - A22 * b1) * D, dy = (A12 * b1 - A11 * b2) * D;
        npx += dx, npy += dy;
        next_pt[0] = npx + half, next_pt[1] = npy + half;
        if ((double)dx * dx + (double)dy * dy <= eps2) break;
        if (j > 0 && fabs((double)(dx + pdx)) < 0.01 && fabs((double)(dy + pdy)) < 0.01) {
            next_pt[0] -= dx * 0.5f, next_pt[1] -= dy * 0.5f;
            break;
        }
        pdx = dx, pdy = dy;
    }
    /* OpenCV 4.x LKTrackerInvoker, behind the iteration loop, when the caller asks for `err` -- the reference does
     * (FrameSourceWarp.cpp:250-259) -- and the level is 0: the FINAL position (the stored next point minus the half
     * window, recomputed in float) is tested against [-win, cols) x [-win, rows) once more and the feature is
     * dropped when its window has left the image, e.g. through the last Gauss-Newton step or the half-step
     * correction above.  (The error measure itself is computed there and never used by the reference.) */
    if (level == 0 && *status && vo_lk_final_check) {
        const float fx = next_pt[0] - half, fy = next_pt[1] - half;
        const int inx = vo_cvfloor(fx), iny = vo_cvfloor(fy);
        if (inx < -VO_LK_WIN || inx >= J->w || iny < -VO_LK_WIN || iny >= J->h) *status = 0;
    }
}

/* prev_pts/next_pts: n (x,y) pairs; status: n bytes.  Returns number of pyramid levels used. */
/* iterations (may be NULL): n x 4 ints, the Gauss-Newton iterations each feature ran on pyramid levels 0..3 -- what
 * decides how long the slowest workgroup of the GPU tracker runs.
 * level_pts (may be NULL): n x 4 (x, y) floats, where each feature stood in the next image after pyramid level 0..3 -- the
 * point that level's iterations ended on, in that level's coordinates (a skipped level: the point it started from; levels the
 * pyramid does not have are left alone).  The GPU tracker fetches the next frame pair's blocks ahead around these
 * (tests/lk_segments.py).
 * sums (may be NULL): n x 5 int64, per feature the largest |sum A11|, |sum A12|, |sum A22|, |sum b1|, |sum b2| over its levels and
 * Gauss-Newton iterations -- the magnitudes the GPU tracker's int32 pieces must hold (vo_pyr_lk_sums). */
VO_API int vo_pyr_lk_trace_sums(const uint8_t *prev, size_t ppitch, const uint8_t *next, size_t npitch, int w, int h,
                                const float *prev_pts, int n, float *next_pts, uint8_t *status, int *iterations, float *level_pts,
                                int64_t *sums) {
    vo_level I[VO_LK_MAXLEVEL + 1], J[VO_LK_MAXLEVEL + 1];
    int nl = vo_build_pyramid(prev, ppitch, w, h, I, 1);
    vo_build_pyramid(next, npitch, w, h, J, 0);
    for (int i = 0; i < n; i++) status[i] = 1;
    if (iterations) memset(iterations, 0, sizeof(int) * 4 * (size_t)n);
    if (sums) memset(sums, 0, sizeof(int64_t) * 5 * (size_t)n);
    for (int level = nl - 1; level >= 0; level--) {
#pragma omp parallel for schedule(dynamic, 4)
        for (int i = 0; i < n; i++) {
            vo_lk_point(&I[level], &J[level], level, nl - 1, prev_pts + 2 * i, next_pts + 2 * i,
                        status + i, iterations ? iterations + 4 * i + level : NULL, sums ? sums + 5 * i : NULL);
            if (level_pts) level_pts[8 * i + 2 * level] = next_pts[2 * i], level_pts[8 * i + 2 * level + 1] = next_pts[2 * i + 1];
        }
    }
    vo_free_pyramid(I, nl);
    vo_free_pyramid(J, nl);
    return nl;
}

VO_API int vo_pyr_lk_trace(const uint8_t *prev, size_t ppitch, const uint8_t *next, size_t npitch, int w, int h,
                           const float *prev_pts, int n, float *next_pts, uint8_t *status, int *iterations, float *level_pts) {
    return vo_pyr_lk_trace_sums(prev, ppitch, next, npitch, w, h, prev_pts, n, next_pts, status, iterations, level_pts, NULL);
}

VO_API int vo_pyr_lk_sums(const uint8_t *prev, size_t ppitch, const uint8_t *next, size_t npitch, int w, int h,
                          const float *prev_pts, int n, float *next_pts, uint8_t *status, int64_t *sums) {
    return vo_pyr_lk_trace_sums(prev, ppitch, next, npitch, w, h, prev_pts, n, next_pts, status, NULL, NULL, sums);
}

VO_API int vo_pyr_lk_iterations(const uint8_t *prev, size_t ppitch, const uint8_t *next, size_t npitch, int w,
                                int h, const float *prev_pts, int n, float *next_pts, uint8_t *status, int *iterations) {
    return vo_pyr_lk_trace(prev, ppitch, next, npitch, w, h, prev_pts, n, next_pts, status, iterations, NULL);
}

VO_API int vo_pyr_lk(const uint8_t *prev, size_t ppitch, const uint8_t *next, size_t npitch, int w,
                     int h, const float *prev_pts, int n, float *next_pts, uint8_t *status) {
    return vo_pyr_lk_trace(prev, ppitch, next, npitch, w, h, prev_pts, n, next_pts, status, NULL, NULL);
}
