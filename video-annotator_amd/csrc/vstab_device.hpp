// vstab_device.hpp -- device-side arithmetic shared by the HIP kernels (gfx950 only): the colour conversion and the bilinear blend
// here, the lens map in vstab_map.hpp, which this header includes.  Everything must reproduce the reference arithmetic bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "vstab_map.hpp"

namespace vstab {

// ---------------------------------------------------------------------------------------------
// Colour conversion: cvtColor(COLOR_YUV2BGR_NV12) / cvtColor(COLOR_BGR2YUV_I420) arithmetic (OpenCV 4.5 CPU path, SURVEY.md A.1: BT.601
// limited range, 20-bit fixed point) and, in the same forms, a colour spec's (include/vstab.h, "Colour matrix and range").  Each function is
// stated once, over the source K of its coefficients:
//   CvtColor8 / CvtColor10   cvtColor's constants as a type: every product folds;
//   ColourCoef               a spec's row in a block of kernel arguments, so that one kernel serves every spec.  The block is what
//                            vstab_colour_coefficients[10] writes: five forward coefficients, yoff, eight inverse ones.
// Every coefficient is below 2^23 (24-bit multiplies hold) and every forward sum of the 8-bit path below 5.8e8 in magnitude (int32 holds).
// ---------------------------------------------------------------------------------------------
// cvtColor's numbers, forward and inverse: stated here once (tests/test_colour_cpu.py reads these two lines) and used through the types below
constexpr int CY = 1220542, CUB = 2116026, CUG = -409993, CVG = -852492, CVR = 1673527;
constexpr int CRY = 269484, CGY = 528482, CBY = 102760, CRU = -155188, CGU = -305135, CBU = 460324, CGV = -385875, CBV = -74448;
template <int YOFF>  // the luma offset: 16 at 8 bits, 64 at 10
struct CvtColor {
    static constexpr int cy = CY, cub = CUB, cug = CUG, cvg = CVG, cvr = CVR, yoff = YOFF;
    static constexpr int cry = CRY, cgy = CGY, cby = CBY, cru = CRU, cgu = CGU, cbu = CBU, cgv = CGV, cbv = CBV;
};
using CvtColor8 = CvtColor<16>;
using CvtColor10 = CvtColor<64>;
struct ColourCoef {
    int cy, cub, cug, cvg, cvr, yoff;
    int cry, cgy, cby, cru, cgu, cbu, cgv, cbv;
};
template <typename K>
constexpr bool coef_at_run_time = std::is_same<K, ColourCoef>::value;
// coefficient * value: 24 bits wide where the coefficient arrives at run time, a plain product the compiler folds as it likes where it is
// a constant.  The multiply belongs to the source: __mul24 of a constant made every default k_warp_fused kernel 40 to 85 lines longer and
// gave two of them a private segment.  And it is written in place, not called: a product inside a helper function is out of sight of the
// value-range passes that run before inlining, which then no longer see that U | V << 8 of cvtColor's inverse has no common bits (six
// instructions more per store loop of every default NV12 kernel).  DESIGN.md section 32, "The coefficient source".
#define VSTAB_CMUL(k, c, v) (coef_at_run_time<std::decay_t<decltype(k)>> ? __mul24(c, v) : (c) * (v))

struct ChromaTerm {
    int ruv, guv, buv;
};
template <typename K>
__device__ __forceinline__ ChromaTerm chroma_term(const K &k, int U, int V) {
    const int u = U - 128, v = V - 128;
    return {(1 << 19) + k.cvr * v, (1 << 19) + k.cvg * v + k.cug * u, (1 << 19) + k.cub * u};
}
__device__ __forceinline__ ChromaTerm chroma_term(int U, int V) { return chroma_term(CvtColor8{}, U, V); }
__device__ __forceinline__ int sat8(int v) { return min(max(v, 0), 255); }

// gfx950's v_ashr_pk_u8_i32 D, S0, S1, n writes {sat_u8(S0 >> n), sat_u8(S1 >> n)} into ONE 16-bit
// half of D (low half; high half with op_sel:[0,0,0,1]) and PRESERVES the other half (measured:
// tools/probe_isa.hip).  ROCm 7.2 hipcc pattern-matches `sat8(a >> 20) | sat8(b >> 20) << 8` into
// it but then assumes the other half is zero -> wrong bytes 2,3.  The empty asm below makes the
// shifted value opaque so the generic path keeps a plain v_med3_i32; the tiled kernel uses the
// instruction deliberately (pack_bgrx).
__device__ __forceinline__ int ashr20(int v) {
    v >>= 20;
    asm volatile("" : "+v"(v));
    return v;
}

template <typename K>
__device__ __forceinline__ void yuv_to_bgr(const K &k, int Y, const ChromaTerm &c, int &b, int &g, int &r) {
    const int y = max(Y - k.yoff, 0) * k.cy;
    b = sat8(ashr20(y + c.buv));
    g = sat8(ashr20(y + c.guv));
    r = sat8(ashr20(y + c.ruv));
}
__device__ __forceinline__ void yuv_to_bgr(int Y, const ChromaTerm &c, int &b, int &g, int &r) { yuv_to_bgr(CvtColor8{}, Y, c, b, g, r); }

// Chroma terms with the luma offset folded in: channel = sat8((max(Y, yoff) * CY + term) >> 20), which is
// the same integer as sat8((max(Y - yoff, 0) * CY + (1 << 19) + C * uv) >> 20).
template <typename K>
__device__ __forceinline__ ChromaTerm chroma_term_folded(const K &k, int U, int V) {
    const int u = U - 128, v = V - 128;
    const int K0 = (1 << 19) - k.yoff * k.cy;  // a constant, or uniform
    return {K0 + VSTAB_CMUL(k, k.cvr, v), K0 + VSTAB_CMUL(k, k.cvg, v) + VSTAB_CMUL(k, k.cug, u), K0 + VSTAB_CMUL(k, k.cub, u)};
}

// One BGRx pixel (byte 3 = 0) from a luma byte and folded chroma terms: 1 max + 3 mad + 2 pack.
template <typename K>
__device__ __forceinline__ uint32_t pack_bgrx(const K &k, int Y, const ChromaTerm &c) {
    const int y = max(Y, k.yoff);
    const int b = __mul24(y, k.cy) + c.buv, g = __mul24(y, k.cy) + c.guv, r = __mul24(y, k.cy) + c.ruv;
    uint32_t d;
    asm("v_ashr_pk_u8_i32 %0, %1, %2, 20" : "=v"(d) : "v"(b), "v"(g));
    asm("v_ashr_pk_u8_i32 %0, %1, 0, 20 op_sel:[0,0,0,1]" : "+v"(d) : "v"(r));
    return d;
}

// The inverse, cvtColor(COLOR_BGR2YUV_I420)'s form (RGB8toYUV420pInvoker): v = B | G << 8 | R << 16; chroma from the top-left pixel of each
// 2 x 2 block.  No sum leaves int32 (|coefficient| < 2^20, three bytes, 129 << 20).  The saturation is part of the definition: full range
// reaches an unsaturated U or V of 256 (pure blue, pure red).  ashr20: see above -- the compiler must not fuse the shift and the saturation
// of two bytes that are then packed.
template <typename K>
__device__ __forceinline__ uint32_t inverse_byte(const K &, int sum) {
    // cvtColor's constants keep Y in [16, 235] and U, V in [16, 240] for every 8-bit BGR: the saturation never acts and is left out
    if constexpr (coef_at_run_time<K>) return (uint32_t)sat8(ashr20(sum));
    else return (uint32_t)sum >> 20;
}
template <typename K>
__device__ __forceinline__ uint32_t bgr_to_y(const K &k, uint32_t v) {
    const int B = v & 255, G = (v >> 8) & 255, R = (v >> 16) & 255;
    return inverse_byte(k, VSTAB_CMUL(k, k.cry, R) + VSTAB_CMUL(k, k.cgy, G) + VSTAB_CMUL(k, k.cby, B) + (1 << 19) + (k.yoff << 20));
}
template <typename K>
__device__ __forceinline__ uint32_t bgr_to_uv(const K &k, uint32_t v) {  // U | V << 8
    const int B = v & 255, G = (v >> 8) & 255, R = (v >> 16) & 255;
    const uint32_t U = inverse_byte(k, VSTAB_CMUL(k, k.cru, R) + VSTAB_CMUL(k, k.cgu, G) + VSTAB_CMUL(k, k.cbu, B) + (1 << 19) + (128 << 20));
    const uint32_t V = inverse_byte(k, VSTAB_CMUL(k, k.cbu, R) + VSTAB_CMUL(k, k.cgv, G) + VSTAB_CMUL(k, k.cbv, B) + (1 << 19) + (128 << 20));
    return U | (V << 8);
}

// cv::remap fixed-point bilinear blend of four BGRx taps:
//   out_c = (p00*(32-fx)(32-fy) + p01*fx(32-fy) + p10*(32-fx)fy + p11*fx*fy + 512) >> 10
// evaluated as an exact two-stage integer lerp (vertical per column with v_dot4_u32_u8 on byte pairs gathered by
// v_perm_b32, then horizontal per channel).  Integer arithmetic is distributive, so this equals the four-product
// sum bit for bit.  Returns 0x00RRGGBB.
__device__ __forceinline__ uint32_t blend_bgrx(uint32_t t00, uint32_t t01, uint32_t t10, uint32_t t11,
                                               uint32_t fx, uint32_t fy) {
    // vertical lerp per column and channel as byte dot products: v = top * (32 - fy) + bottom * fy  (<= 255 * 32)
    const uint32_t gy = 32u - fy;
    const uint32_t w_lo = gy | (fy << 8), w_hi = w_lo << 16;  // weights against bytes (0,1) / bytes (2,3)
    const uint32_t bg_l = __builtin_amdgcn_perm(t10, t00, 0x05010400u);  // [top.B, bottom.B, top.G, bottom.G]
    const uint32_t r_l = __builtin_amdgcn_perm(t10, t00, 0x0c0c0602u);   // [top.R, bottom.R, 0, 0]
    const uint32_t bg_r = __builtin_amdgcn_perm(t11, t01, 0x05010400u);
    const uint32_t r_r = __builtin_amdgcn_perm(t11, t01, 0x0c0c0602u);
    // horizontal lerp with the weights scaled by 64: (l * gx + r * fx + 512) << 6 has the result byte at bits 16..23.
    // The six dot products and six multiply-adds are ONE hand-ordered block: gfx950 needs three independent
    // instructions between a v_dot4 and the VALU instruction that reads its result (the compiler pads its own dot4s with
    // s_nop, cannot see into inline assembly, and left to itself emits two multiplies and a three-operand add per channel
    // where two multiply-adds do) -- here every dot product is read five instructions after it was issued.
    const uint32_t fx6 = fx << 6, gx6 = 2048u - fx6, half = 32768u;
    uint32_t vb_r, vg_r, vr_r, vb_l, vg_l, vr_l, sb, sg, sr;
    asm("v_dot4_u32_u8 %0, %9, %13, 0\n\t"
        "v_dot4_u32_u8 %1, %9, %14, 0\n\t"
        "v_dot4_u32_u8 %2, %10, %13, 0\n\t"
        "v_dot4_u32_u8 %3, %11, %13, 0\n\t"
        "v_dot4_u32_u8 %4, %11, %14, 0\n\t"
        "v_dot4_u32_u8 %5, %12, %13, 0\n\t"
        "v_mad_u32_u24 %6, %0, %15, %17\n\t"
        "v_mad_u32_u24 %7, %1, %15, %17\n\t"
        "v_mad_u32_u24 %8, %2, %15, %17\n\t"
        "v_mad_u32_u24 %6, %3, %16, %6\n\t"
        "v_mad_u32_u24 %7, %4, %16, %7\n\t"
        "v_mad_u32_u24 %8, %5, %16, %8"
        : "=&v"(vb_r), "=&v"(vg_r), "=&v"(vr_r), "=&v"(vb_l), "=&v"(vg_l), "=&v"(vr_l), "=&v"(sb), "=&v"(sg), "=&v"(sr)
        : "v"(bg_r), "v"(r_r), "v"(bg_l), "v"(r_l), "v"(w_lo), "v"(w_hi), "v"(fx6), "v"(gx6), "v"(half));
    const uint32_t bg = __builtin_amdgcn_perm(sg, sb, 0x0c0c0602u);  // [B, G, 0, 0]
    return __builtin_amdgcn_perm(sr, bg, 0x0c060100u);               // [B, G, R, 0]
}

}  // namespace vstab
