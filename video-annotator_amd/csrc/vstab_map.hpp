// vstab_map.hpp -- the lens map (createMap.cl:13-50 and this project's extensions of it): the one piece of arithmetic every warp kernel
// reproduces bit for bit, each formula stated once over the value type T -- float, or f32x2 for two pixels at once.  DESIGN.md section 37
// says what is stated where, and why two interleaved forms (vstab_warp_tile.hpp) keep their own operation order.
// Everything here must reproduce the reference arithmetic bit for bit, so the translation units are compiled with -ffp-contract=off: a*b+c is
// two roundings unless written as a fused multiply-add.  hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt keeps `/` and sqrtf IEEE-correct.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vstab {

// ---------------------------------------------------------------------------------------------
// createMap.cl:13-50 arithmetic.  The 17 kernel arguments in argument order.
// ---------------------------------------------------------------------------------------------
struct MapParams {
    float icx, icy, ifx, ify;  // src_center_x/y, src_focal_x/y     (createMap.cl:4)
    float ocx, ocy, ofx, ofy;  // map_center_x/y, map_focal_x/y     (createMap.cl:5)
    float r[9];                // rot00..rot22                      (createMap.cl:6-8)
};
// k1..k4 of the input lens (OpenCV's fisheye model: theta_d = theta (1 + k1 theta^2 + k2 theta^4 + k3 theta^6 + k4 theta^8)); read by
// the MAP_FISHD_* modes only, zero everywhere else
struct Distortion {
    float k1, k2, k3, k4;
};
// The input camera as the exact chain reads it: centre and focal length (scaled by 32 where the caller wants 32 * map, the value
// cv::remap rounds -- an exact power-of-two scaling folded into the constants), the third column of the rotation, the lens.
struct MapParams32 {
    float icx32, icy32, ifx32, ify32;
    float r02, r12, r22;
    Distortion d;
};

// Column / row terms of the rotated ray: dot(row_i, v) = (r_i0*vx + r_i1*vy) + r_i2*1
// (createMap.cl:27-31, left-to-right unfused).  r_i0*vx depends only on the column and
// r_i1*vy only on the row, so they are hoisted out of the per-pixel work.
struct ColTerm {
    float a0, a1, a2;
};
struct RowTerm {
    float b0, b1, b2;
};

// ---------------------------------------------------------------------------------------------
// The value type.  Two pixels at once: ext_vector_type(2) -> v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32, which issue two fp32 operations
// in 4.8 cycles where two v_fma_f32 take 8 (tools/probe_rate.hip).  Every component goes through exactly the scalar instantiation's operation
// sequence, so the results are bit-identical to it.  By type: the fused multiply-add and the two hardware seeds.
// ---------------------------------------------------------------------------------------------
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef int i32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2 splat2(float v) { return (f32x2){v, v}; }
__device__ __forceinline__ float vfma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ f32x2 vfma(f32x2 a, f32x2 b, f32x2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ float rcp_seed(float d) { return __builtin_amdgcn_rcpf(d); }  // v_rcp_f32, 1 ulp
__device__ __forceinline__ f32x2 rcp_seed(f32x2 d) { return (f32x2){__builtin_amdgcn_rcpf(d.x), __builtin_amdgcn_rcpf(d.y)}; }
__device__ __forceinline__ float rsq_seed(float x) { return __builtin_amdgcn_rsqf(x); }  // v_rsq_f32, 1 ulp
__device__ __forceinline__ f32x2 rsq_seed(f32x2 x) { return (f32x2){__builtin_amdgcn_rsqf(x.x), __builtin_amdgcn_rsqf(x.y)}; }

// ---------------------------------------------------------------------------------------------
// Hand-scheduled IEEE-754 binary32 primitives for the hot kernel.  Each returns exactly what the
// correctly rounded operation returns for every finite, non-denormal-scaled input the map can
// produce (they are the LLVM AMDGPU expansions of fdiv / fsqrt minus the denormal pre-scaling;
// degenerate inputs -- 0, inf, NaN -- end in NaN or a huge value and the pixel is black either
// way).  tools/probe_isa.hip checks them against `/` and sqrtf on the GPU.
// ---------------------------------------------------------------------------------------------
// refined reciprocal: v_rcp_f32 (1 ulp) + one Newton step
template <typename T>
__device__ __forceinline__ T rcp_refined(T d) {
    const T r = rcp_seed(d);
    const T e = vfma(-d, r, T(1.0f));
    return vfma(e, r, r);
}
// n / d given r = rcp_refined(d): two residual corrections (Markstein), correctly rounded
template <typename T>
__device__ __forceinline__ T div_with_rcp(T n, T d, T r) {
    T q = n * r;
    T e = vfma(-d, q, n);
    q = vfma(e, r, q);
    e = vfma(-d, q, n);
    return vfma(e, r, q);
}
// correctly rounded sqrt: v_rsq_f32 seed, one coupled Newton step for sqrt and 1/(2 sqrt), one residual
// correction (LLVM's AMDGPU expansion of fsqrt for normal inputs; all plain FMAs).  x = 0 or inf give
// NaN here instead of 0 / inf -- both can only occur on a degenerate ray whose pixel is black either way.
template <typename T>
__device__ __forceinline__ T sqrt_rn(T x) {
    const T y = rsq_seed(x);
    T g = x * y, h = T(0.5f) * y;
    const T e = vfma(-h, g, T(0.5f));
    h = vfma(h, e, h);
    g = vfma(g, e, g);
    const T d = vfma(-g, g, x);
    return vfma(d, h, g);
}

// ---------------------------------------------------------------------------------------------
// The arc tangent.  atan for x >= 0 (or NaN): x > 1 -> pi/2 - atan(1/x); atan(t) = t + t*s*q(s), s = t*t.
// OpenCL leaves atan implementation defined; the algorithm is fixed here (and, independently,
// in the CPU oracle) so results are reproducible.  < 1.5 ulp.
// The coefficients of q, highest power first, and pi/2 in two parts are stated here once; the probe and the interleaved pair form
// (vstab_warp_tile.hpp) read them from here and keep their own operation order.
// ---------------------------------------------------------------------------------------------
constexpr float ATAN_Q[8] = {0.0028423243202269077f, -0.016053270548582077f, 0.04269874095916748f, -0.07508683204650879f,
                             0.1064559817314148f,    -0.14205896854400635f,  0.19993145763874054f, -0.33333125710487366f};
constexpr float PIO2_HI = 1.57079637050628662109375f, PIO2_LO = -4.37113900018624283e-8f;  // pi/2 = PIO2_HI + PIO2_LO
// T at = atan(rad), given rr = rcp_refined(rad), which the user shares with its division by the radius: the reduction, the eight
// fused multiply-adds, the two-part pi/2.  The one exact statement, and a text, not a function: a call between the radius and the guarded
// division of fish_chain is opaque to the passes that run before inlining, and every kernel of the guarded modes then comes out another
// (k_quantised_map<MAP_FISH_TO_RECT> 426 -> 359 lines, 32 -> 39 registers; as much with only the polynomial behind the call, or with the
// reduction outside it).  profiles/map_one_form.txt has the forms that were tried.
#define VSTAB_ATAN_WITH_RCP(T, at, rad, rr)                                            \
    T at;                                                                              \
    {                                                                                  \
        const auto inv_ = rad > T(1.0f);                                               \
        const T t_ = inv_ ? div_with_rcp(T(1.0f), rad, rr) : rad;                      \
        const T s_ = t_ * t_;                                                          \
        T q_ = T(ATAN_Q[0]);                                                           \
        q_ = vfma(q_, s_, T(ATAN_Q[1]));                                               \
        q_ = vfma(q_, s_, T(ATAN_Q[2]));                                               \
        q_ = vfma(q_, s_, T(ATAN_Q[3]));                                               \
        q_ = vfma(q_, s_, T(ATAN_Q[4]));                                               \
        q_ = vfma(q_, s_, T(ATAN_Q[5]));                                               \
        q_ = vfma(q_, s_, T(ATAN_Q[6]));                                               \
        q_ = vfma(q_, s_, T(ATAN_Q[7]));                                               \
        at = vfma(t_ * s_, q_, t_);                                                    \
        at = inv_ ? (T(PIO2_HI) - at) + T(PIO2_LO) : at;                               \
    }
__device__ __forceinline__ float atan_pos(float x) {
    const float rr = rcp_refined(x);
    VSTAB_ATAN_WITH_RCP(float, at, x, rr)
    return at;
}

// theta -> theta_d, every operation rounded on its own (the translation units are built with -ffp-contract=off): DESIGN.md section 18.
// d = 0 returns `at` bit for bit.
template <typename T>
__device__ __forceinline__ T distort_theta(T at, const Distortion &d) {
    const T s2 = at * at;
    T g = T(d.k4);
    g = g * s2 + T(d.k3);
    g = g * s2 + T(d.k2);
    g = g * s2 + T(d.k1);
    return at * (T(1.0f) + g * s2);
}
// normalised pinhole coordinates -> distorted ones through OpenCV's (k1, k2, p1, p2, k3), every operation rounded on its own: DESIGN.md
// section 23.  d = 0 returns (x, y) bit for bit wherever x * x + y * y is finite.
__device__ __forceinline__ void distort_pinhole(float x, float y, const float *d, float &xd, float &yd) {
    const float k1 = d[0], k2 = d[1], p1 = d[2], p2 = d[3], k3 = d[4];
    const float xx = x * x, yy = y * y, xy = x * y, r2 = xx + yy;
    float g = k3;
    g = g * r2 + k2;
    g = g * r2 + k1;
    const float rad = 1.0f + g * r2;
    const float a = 2.0f * xy;
    const float dx = p1 * a + p2 * (r2 + 2.0f * xx);
    const float dy = p1 * (r2 + 2.0f * yy) + p2 * a;
    xd = x * rad + dx, yd = y * rad + dy;
}

// ---------------------------------------------------------------------------------------------
// The fisheye-input chain, createMap.cl:33-49 with the primitives above: ray (wx, wy, wz) -> two divisions, radius, arc tangent,
// division by the radius, scaling into the source.  p: the input camera -- members icx32, icy32, ifx32, ify32 (centre and focal length,
// scaled by 32 or not) and, for DIST, d -- in the caller's own struct: a MapParams32 for one pixel; for two, a struct whose members are
// pairs already (from a MapParams32 the four `* 32` of k_warp_p010 became two packed multiplies and its eight kernels of modes 0 and 1
// came out another, 903 -> 904 lines; as four arguments of the value type the k_warp_fused and k_warp_planar kernels of modes 2 and 10 did).
//   GUARD  the generalised map (below) where createMap.cl degenerates: the axis pixel (px = py = 0) gets the factor 1 instead of 0/0.
//          Its other departure -- a ray behind the camera (wz <= 0) is outside (NaN), not mirrored -- stands after the call at the two
//          guarded users: inside this function it changed the kernels of the distorted and the fisheye-output modes.
//   DIST   distort_theta with d between the arc tangent and the division.
// ---------------------------------------------------------------------------------------------
template <bool GUARD, bool DIST, typename T, typename Cam>
__device__ __forceinline__ void fish_chain(const Cam &p, T wx, T wy, T wz, T &ax, T &ay) {
    const T rz = rcp_refined(wz);
    const T px = div_with_rcp(wx, wz, rz), py = div_with_rcp(wy, wz, rz);  // createMap.cl:33-36
    const T q = px * px + py * py;
    const T rad = sqrt_rn(q);                                              // createMap.cl:38 length()
    const T rr = rcp_refined(rad);
    VSTAB_ATAN_WITH_RCP(T, at, rad, rr)
    if constexpr (DIST) at = distort_theta(at, p.d);
    T k;                                                                   // createMap.cl:39
    if constexpr (GUARD) k = (q == T(0.0f)) ? T(1.0f) : div_with_rcp(at, rad, rr);
    else k = div_with_rcp(at, rad, rr);
    ax = T(p.icx32) + (px * k) * T(p.ifx32);                               // createMap.cl:48
    ay = T(p.icy32) + (py * k) * T(p.ify32);                               // createMap.cl:49
}
// createMap.cl:13-50 itself (MAP_CREATEMAP_CL), from the hoisted column / row terms
__device__ __forceinline__ void map_pixel32(const MapParams32 &p, const ColTerm &c, const RowTerm &r, float &ax, float &ay) {
    fish_chain<false, false>(p, (c.a0 + r.b0) + p.r02, (c.a1 + r.b1) + p.r12, (c.a2 + r.b2) + p.r22, ax, ay);
}
// and unscaled, with the compiler's own division and square root: the stand-alone map and the un-tiled warp (k_create_map, vstab_warp.hip)
__device__ __forceinline__ ColTerm col_term(const MapParams &p, int x) {
    const float vx = ((float)x - p.ocx) / p.ofx;  // createMap.cl:16
    return {p.r[0] * vx, p.r[3] * vx, p.r[6] * vx};
}
__device__ __forceinline__ RowTerm row_term(const MapParams &p, int y) {
    const float vy = ((float)y - p.ocy) / p.ofy;  // createMap.cl:17
    return {p.r[1] * vy, p.r[4] * vy, p.r[7] * vy};
}
__device__ __forceinline__ void map_pixel(const MapParams &p, const ColTerm &c, const RowTerm &r, float &mx, float &my) {
    const float wx = (c.a0 + r.b0) + p.r[2];
    const float wy = (c.a1 + r.b1) + p.r[5];
    const float wz = (c.a2 + r.b2) + p.r[8];
    const float px = wx / wz, py = wy / wz;             // createMap.cl:33-36
    const float rad = sqrtf(px * px + py * py);         // createMap.cl:38 length()
    const float k = atan_pos(rad) / rad;                // createMap.cl:39
    mx = p.icx + (px * k) * p.ifx;                      // createMap.cl:48
    my = p.icy + (py * k) * p.ify;                      // createMap.cl:49
}

// ---------------------------------------------------------------------------------------------
// Generalised map (the libdewobble option surface in_p / out_p in {fish, rect},
// render.ts:611-617,669-683,711-717).  libdewobble is not part of the reference tree, so the arithmetic
// is defined by this project (the test suite holds a plain-C statement of it): mode
// FISH_TO_RECT performs createMap.cl's operations and differs only where createMap.cl degenerates
// (axis ray: correction factor 1 instead of 0/0; rays behind the camera: outside instead of mirrored).
// ---------------------------------------------------------------------------------------------
enum MapMode { MAP_CREATEMAP_CL = 0, MAP_FISH_TO_RECT = 1, MAP_FISH_TO_FISH = 2, MAP_RECT_TO_RECT = 3, MAP_RECT_TO_FISH = 4,
               // createMap.cl with the arithmetic ROCm's OpenCL compiler gives it on gfx950 (below)
               MAP_CREATEMAP_CL_OPENCL = 5,
               // internal: modes 0 / 1 / 5 with a per-row rotation (rolling shutter, BASELINE config 5)
               MAP_RS_CREATEMAP_CL = 6, MAP_RS_FISH_TO_RECT = 7, MAP_RS_CREATEMAP_CL_OPENCL = 8,
               // internal: modes 1 / 2 with the input lens's distortion polynomial (vstab_*_dist)
               MAP_FISHD_TO_RECT = 9, MAP_FISHD_TO_FISH = 10,
               // internal: mode 9 with a per-row rotation (vstab_warp_nv12_rs_ex: k_warp_border, k_warp_cubic_rs, k_warp_lanczos4_rs)
               MAP_RS_FISHD_TO_RECT = 11,
               // internal: modes 3 / 4 with the input lens's Brown-Conrady polynomial (vstab_*_pinhole)
               MAP_RECTD_TO_RECT = 12, MAP_RECTD_TO_FISH = 13 };
// the projection pair (and arithmetic) of a mode: the rolling-shutter modes share their base mode's
constexpr bool map_mode_is_rs(int mode) { return (mode >= MAP_RS_CREATEMAP_CL && mode <= MAP_RS_CREATEMAP_CL_OPENCL) || mode == MAP_RS_FISHD_TO_RECT; }
constexpr int map_mode_base(int mode) {
    return mode == MAP_RS_CREATEMAP_CL ? MAP_CREATEMAP_CL : mode == MAP_RS_FISH_TO_RECT ? MAP_FISH_TO_RECT : mode == MAP_RS_CREATEMAP_CL_OPENCL ? MAP_CREATEMAP_CL_OPENCL :
           mode == MAP_RS_FISHD_TO_RECT ? MAP_FISHD_TO_RECT : mode;
}
template <int MODE>
struct ModeTraits {
    static constexpr bool dist = MODE == MAP_FISHD_TO_RECT || MODE == MAP_FISHD_TO_FISH || MODE == MAP_RS_FISHD_TO_RECT;  // theta -> theta_d on the way into the input lens
    static constexpr bool rectd = MODE == MAP_RECTD_TO_RECT || MODE == MAP_RECTD_TO_FISH;  // (k1, k2, p1, p2, k3) on the way into a rectilinear input lens
    static constexpr bool out_fish = MODE == MAP_FISH_TO_FISH || MODE == MAP_RECT_TO_FISH || MODE == MAP_FISHD_TO_FISH || MODE == MAP_RECTD_TO_FISH;
    static constexpr bool in_fish = MODE == MAP_FISH_TO_RECT || MODE == MAP_FISH_TO_FISH || MODE == MAP_CREATEMAP_CL || MODE == MAP_CREATEMAP_CL_OPENCL || dist;
};

// ---------------------------------------------------------------------------------------------
// createMap.cl:13-50 AS THE REFERENCE'S OWN KERNEL COMPUTES IT ON THIS GPU.  The reference hands createMap.cl to the
// OpenCL runtime (FrameSourceWarp.cpp:224,301), whose compiler is free to contract a*b+c (FP_CONTRACT is ON in OpenCL
// C), to divide within 2.5 ulp, to take length() within 3 and atan() within 5.  The test infrastructure holds
// that file built by ROCm's OpenCL front end for gfx950 (createMap.gfx950.co); its instruction stream is (llvm-objdump -d):
//   a / b      = ldexp(frexp_mant(a) * v_rcp_f32(frexp_mant(b)), frexp_exp(a) - frexp_exp(b))
//   dot(r, v)  = fma(r1, vy, r0 * vx) + r2           (the * 1 of the third component folded away)
//   length(p)  = v_sqrt_f32(fma(py, py, px * px))      with ocml's rescaling outside [2^-126, inf)
//   atan(x)    = ocml's: t = x > 1 ? v_rcp_f32(x) : x, odd polynomial of degree 17 in t, pi/2 - . when reciprocated
//   map        = fma(focal, p * k, centre)
// The functions below are that stream, operation for operation; tests/test_refcl_gpu.py compares them bit for bit with
// the code object run on the same device.  v_rcp_f32 / v_sqrt_f32 are hardware approximations (1 ulp), so this mode
// has no CPU restatement: its checker is the reference's own kernel.
// ---------------------------------------------------------------------------------------------
constexpr float f32_bits(uint32_t u) { return __builtin_bit_cast(float, u); }
__device__ __forceinline__ float ocl_div(float a, float b) {
    const float r = __builtin_amdgcn_rcpf(__builtin_amdgcn_frexp_mantf(b));
    const float m = __builtin_amdgcn_frexp_mantf(a) * r;
    return __builtin_ldexpf(m, __builtin_amdgcn_frexp_expf(a) - __builtin_amdgcn_frexp_expf(b));
}
__device__ __forceinline__ float ocl_sqrt_scaled(float x) {  // ocml's native-precision sqrt: denormal inputs rescaled
    const bool small = 0x1p-126f > x;
    const float y = __builtin_amdgcn_sqrtf(__builtin_ldexpf(x, small ? 32 : 0));
    return __builtin_ldexpf(y, small ? -16 : 0);
}
__device__ __forceinline__ float ocl_length2(float px, float py) {
    const float q = __builtin_fmaf(py, py, px * px);
    if (!(0x1p-126f > q)) {  // also NaN
        if (q != __builtin_inff()) return __builtin_amdgcn_sqrtf(q);
        const float a = px * 0x1p-65f, b = py * 0x1p-65f;
        return 0x1p65f * ocl_sqrt_scaled(__builtin_fmaf(b, b, a * a));
    }
    const float a = px * 0x1p86f, b = py * 0x1p86f;
    return 0x1p-86f * ocl_sqrt_scaled(__builtin_fmaf(b, b, a * a));
}
// ocml's atan: the coefficients of its polynomial in s = t * t, highest power first, and its pi/2; stated here once and read by the
// interleaved pair form (vstab_warp_tile.hpp, map_pairs_ocl)
constexpr float OCML_ATAN[8] = {f32_bits(0x3b2d2a58u), f32_bits(0xbc7a590cu), f32_bits(0x3d29fb3fu), f32_bits(0xbd97d4d7u),
                                f32_bits(0x3dd931b2u), f32_bits(0xbe1160e6u), f32_bits(0x3e4cb8bfu), f32_bits(0xbeaaaa62u)};
constexpr float OCML_PIO2 = f32_bits(0x3fc90fdbu);
// given t = |x| > 1 ? 1 / |x| : |x| (the reciprocal is a raw v_rcp_f32 there)
__device__ __forceinline__ float ocl_atan_poly(float t, bool inv) {
    const float s = t * t;
    float p = __builtin_fmaf(OCML_ATAN[0], s, OCML_ATAN[1]);
    p = __builtin_fmaf(s, p, OCML_ATAN[2]);
    p = __builtin_fmaf(s, p, OCML_ATAN[3]);
    p = __builtin_fmaf(s, p, OCML_ATAN[4]);
    p = __builtin_fmaf(s, p, OCML_ATAN[5]);
    p = __builtin_fmaf(s, p, OCML_ATAN[6]);
    p = __builtin_fmaf(s, p, OCML_ATAN[7]);
    const float r = __builtin_fmaf(t, s * p, t);
    return inv ? OCML_PIO2 - r : r;
}
__device__ __forceinline__ float ocl_atan(float x) {
    const float a = __builtin_fabsf(x);
    const bool inv = a > 1.0f;
    return __builtin_copysignf(ocl_atan_poly(inv ? __builtin_amdgcn_rcpf(a) : a, inv), x);
}
// One pixel, the code object's stream literally.  vx, vy = ocl_div(x - ocx, ofx), ocl_div(y - ocy, ofy); a = r_i0 * vx.
// c = centre, f = focal length of the input camera (both may carry cv::remap's exact factor 32).
// r = the nine rotation entries (the frame's, or one output row's in the rolling-shutter warp).
__device__ __forceinline__ void map_pixel_ocl_literal(float icx, float icy, float ifx, float ify, const float (&r)[9], float a0, float a1, float a2,
                                                      float vy, float &ax, float &ay) {
    const float wz = __builtin_fmaf(r[7], vy, a2) + r[8];
    const float wx = __builtin_fmaf(r[1], vy, a0) + r[2];
    const float wy = __builtin_fmaf(r[4], vy, a1) + r[5];
    const float px = ocl_div(wx, wz), py = ocl_div(wy, wz);
    const float rad = ocl_length2(px, py);
    const float k = ocl_div(ocl_atan(rad), rad);
    ax = __builtin_fmaf(ifx, px * k, icx);
    ay = __builtin_fmaf(ify, py * k, icy);
}
// The same results from fewer instructions wherever no intermediate leaves the normal range: a multiplication's
// rounding does not depend on its operands' exponents and v_rcp_f32 works on the significand alone, so
// frexp / ldexp around `a * rcp(b)` change nothing, and the reciprocal of the radius serves both atan's argument
// reduction and the final division.  `regular` says whether that holds for this pixel (else: the literal stream).
__device__ __forceinline__ bool map_pixel_ocl_fast(float icx, float icy, float ifx, float ify, const float (&r)[9], float a0, float a1, float a2,
                                                   float vy, float &ax, float &ay) {
    const float wz = __builtin_fmaf(r[7], vy, a2) + r[8];
    const float wx = __builtin_fmaf(r[1], vy, a0) + r[2];
    const float wy = __builtin_fmaf(r[4], vy, a1) + r[5];
    const float rz = __builtin_amdgcn_rcpf(wz);
    const float px = wx * rz, py = wy * rz;
    const float q = __builtin_fmaf(py, py, px * px);
    const float rad = __builtin_amdgcn_sqrtf(q), rr = __builtin_amdgcn_rcpf(rad);
    const bool inv = rad > 1.0f;
    const float k = ocl_atan_poly(inv ? rr : rad, inv) * rr;
    ax = __builtin_fmaf(ifx, px * k, icx);
    ay = __builtin_fmaf(ify, py * k, icy);
    const float az = __builtin_fabsf(wz);
    return az >= 0x1p-40f && az <= 0x1p40f && q >= 0x1p-80f && q <= 0x1p80f;  // false for NaN
}

// sin, cos on [0, pi]: quadrant reduction with a two-constant pi/2, Cephes single-precision polynomials
__device__ __forceinline__ void sincos_pos(float t, float &sn, float &cs) {
    const float k = __builtin_rintf(t * 0.636619746685028076171875f);
    float r = __builtin_fmaf(k, -PIO2_HI, t);
    r = __builtin_fmaf(k, -PIO2_LO, r);
    const float z = r * r;
    const float ps = __builtin_fmaf(__builtin_fmaf(-1.9515295891e-4f, z, 8.3321608736e-3f), z, -1.6666654611e-1f);
    const float pc = __builtin_fmaf(__builtin_fmaf(2.443315711809948e-5f, z, -1.388731625493765e-3f), z, 4.166664568298827e-2f);
    const float s = __builtin_fmaf(r * z, ps, r);
    const float c = __builtin_fmaf(z * z, pc, __builtin_fmaf(-0.5f, z, 1.0f));
    sn = k == 1.0f ? c : k == 2.0f ? -s : s;
    cs = k == 1.0f ? -s : k == 2.0f ? -c : c;
}

// Normalised output coordinate (createMap.cl:16-17) as the mode divides: IEEE, or the OpenCL build's reciprocal form.
template <int MODE>
__device__ __forceinline__ float norm_coord(float n, float d, float rcp_refined_d) {
    if constexpr (MODE == MAP_CREATEMAP_CL_OPENCL) return ocl_div(n, d);
    else return div_with_rcp(n, d, rcp_refined_d);
}

// One pixel of the generalised map.  p holds the input camera (scaled by 32 in the fused kernel, unscaled in
// the map-plane kernel -- the scaling is an exact power of two either way), P the output camera and rotation.
// c / r are the hoisted column / row products for pinhole output; vx, vy the normalised output coordinates for
// fisheye output.  Outside (NaN) when the output ray is beyond 180 degrees or lands behind the input camera.
// pd: the five coefficients of the MAP_RECTD_* modes (MapParams32 has room for four), read by no other mode.
template <int MODE>
__device__ __forceinline__ void map_pixel_ex(const MapParams32 &p, const MapParams &P, const ColTerm &c, const RowTerm &r,
                                             float vx, float vy, float &ax, float &ay, const float *pd = nullptr) {
    if constexpr (MODE == MAP_CREATEMAP_CL) {
        map_pixel32(p, c, r, ax, ay);
    } else if constexpr (MODE == MAP_CREATEMAP_CL_OPENCL) {
        if (!map_pixel_ocl_fast(p.icx32, p.icy32, p.ifx32, p.ify32, P.r, c.a0, c.a1, c.a2, vy, ax, ay))
            map_pixel_ocl_literal(p.icx32, p.icy32, p.ifx32, p.ify32, P.r, c.a0, c.a1, c.a2, vy, ax, ay);
    } else {
        float wx, wy, wz;
        bool ok = true;
        if constexpr (ModeTraits<MODE>::out_fish) {
            const float q = vx * vx + vy * vy;
            const bool zero = q == 0.0f;
            const float rho = sqrt_rn(q);  // NaN when q == 0
            ok = zero || rho < 3.1415927410125732421875f;
            float sn, cs;
            sincos_pos(zero ? 0.0f : rho, sn, cs);
            const float s = zero ? 1.0f : div_with_rcp(sn, rho, rcp_refined(rho));
            const float rx = vx * s, ry = vy * s;
            wx = (P.r[0] * rx + P.r[1] * ry) + P.r[2] * cs;
            wy = (P.r[3] * rx + P.r[4] * ry) + P.r[5] * cs;
            wz = (P.r[6] * rx + P.r[7] * ry) + P.r[8] * cs;
        } else {
            wx = (c.a0 + r.b0) + p.r02;
            wy = (c.a1 + r.b1) + p.r12;
            wz = (c.a2 + r.b2) + p.r22;
        }
        ok = ok && wz > 0.0f;
        if constexpr (ModeTraits<MODE>::in_fish) {
            fish_chain<true, ModeTraits<MODE>::dist>(p, wx, wy, wz, ax, ay);
        } else {
            const float rz = rcp_refined(wz);
            const float px = div_with_rcp(wx, wz, rz), py = div_with_rcp(wy, wz, rz);
            if constexpr (ModeTraits<MODE>::rectd) {
                float xd, yd;
                distort_pinhole(px, py, pd, xd, yd);
                ax = p.icx32 + xd * p.ifx32;
                ay = p.icy32 + yd * p.ify32;
            } else {
                ax = p.icx32 + px * p.ifx32;
                ay = p.icy32 + py * p.ify32;
            }
        }
        if (!ok) ax = ay = __builtin_nanf("");
    }
}

// The preamble of map_pixel_ex: from a column's vx and a row's vy (the normalised output coordinates, divided as the caller's mode divides) to
// 32 * map or the map, by p's scaling.  Four sites keep the preamble in place, each with a note of the listing that changed through this layer:
// the probe and the map phase of the tiled kernels, the per-row rotation of border_map and k_warp_p010.
template <int MODE>
__device__ __forceinline__ void map_at(const MapParams32 &p, const MapParams &P, float vx, float vy, float &ax, float &ay, const float *pd = nullptr) {
    const ColTerm ct = {P.r[0] * vx, P.r[3] * vx, P.r[6] * vx};
    const RowTerm rt = {P.r[1] * vy, P.r[4] * vy, P.r[7] * vy};
    map_pixel_ex<MODE>(p, P, ct, rt, vx, vy, ax, ay, pd);
}
// The same from an output pixel (x, y), k_quantised_map's arithmetic (the fused kernels' map, bit for bit, in every mode); rfx, rfy = rcp_refined(ofx, ofy)
template <int MODE>
__device__ __forceinline__ void map_at(const MapParams32 &p, const MapParams &P, int x, int y, float rfx, float rfy, float &ax, float &ay,
                                       const float *pd = nullptr) {
    const float vy = norm_coord<MODE>((float)y - P.ocy, P.ofy, rfy);
    const float vx = norm_coord<MODE>((float)x - P.ocx, P.ofx, rfx);
    map_at<MODE>(p, P, vx, vy, ax, ay, pd);
}

// ---------------------------------------------------------------------------------------------
// cv::remap coordinate quantisation (OpenCV 4.5 CPU path): sx = cvRound(map*32),
// X = sx >> 5, f = sx & 31.  cvRound of NaN / out-of-int-range is INT_MIN on x86, which always
// lands outside the source; `far` reports those cases so the caller writes 0.
// ---------------------------------------------------------------------------------------------
struct Tap {
    int X, Y, fx, fy;
    bool far;
};

__device__ __forceinline__ Tap quantise(float mx, float my) {
    const float ax = mx * 32.0f, ay = my * 32.0f;
    Tap t;
    t.far = !(fabsf(ax) < 1073741824.0f) || !(fabsf(ay) < 1073741824.0f);
    const int sx = (int)__builtin_rintf(ax), sy = (int)__builtin_rintf(ay);
    t.X = sx >> 5, t.Y = sy >> 5, t.fx = sx & 31, t.fy = sy & 31;
    return t;
}

}  // namespace vstab
