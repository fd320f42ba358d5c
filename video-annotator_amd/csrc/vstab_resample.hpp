// vstab_resample.hpp -- what the cv::remap kernels of the cubic and Lanczos warps (vstab_warp_cubic.hip, vstab_warp_lanczos4.hip,
// vstab_warp_resample_border.hip) share: the launch arguments, the quantisation of a map position (the same for INTER_LINEAR, INTER_CUBIC and
// INTER_LANCZOS4), the sources a tap reads, the blends, and the map of an output pixel.
#pragma once
#include <climits>

#include "vstab_device.hpp"
#include "vstab_warp_args.hpp"

namespace vstab {

struct CubicArgs {  // the warp kernels' one argument (both resamplers)
    WarpArgs w;
    MapParams32 p32;
};

// cvRound (NaN / outside the int range -> INT_MIN), then cv::remap's split: X = saturate_cast<short>(sx >> 5), f = sx & 31
struct CubicTap {
    int X, Y, f;  // f = fy * 32 + fx: the table entry
};
__device__ __forceinline__ int cv_round_f32(float a) { return (a >= -2147483648.0f && a < 2147483648.0f) ? (int)__builtin_rintf(a) : INT_MIN; }
__device__ __forceinline__ CubicTap cubic_tap(float ax32, float ay32) {  // ax32, ay32 = 32 * map
    const int sx = cv_round_f32(ax32), sy = cv_round_f32(ay32);
    return {min(max(sx >> 5, -32768), 32767), min(max(sy >> 5, -32768), 32767), (sy & 31) * 32 + (sx & 31)};
}

// ---------------------------------------------------------------------------------------------------------------------
// Sources: a tap (X, Y) of a plane as a dword with one channel per byte, the border value where it lies outside.
// ---------------------------------------------------------------------------------------------------------------------
struct SrcNv12Bgr {  // NV12 planes converted with the cvtColor arithmetic (BGRx); border 0 (cv::remap's Scalar(0))
    const uint8_t *y, *uv;
    size_t pitch_y, pitch_uv;
    int w, h;
    __device__ __forceinline__ uint32_t operator()(int X, int Y) const {
        if ((unsigned)X < (unsigned)w && (unsigned)Y < (unsigned)h) {
            const int yv = y[(size_t)Y * pitch_y + X];
            const uint16_t c = *reinterpret_cast<const uint16_t *>(uv + (size_t)(Y >> 1) * pitch_uv + (X & ~1));
            int b, g, r;
            yuv_to_bgr(yv, chroma_term(c & 255, c >> 8), b, g, r);
            return (uint32_t)b | ((uint32_t)g << 8) | ((uint32_t)r << 16);
        }
        return 0;
    }
};
template <int CN>
struct SrcBytes {  // CN interleaved 8-bit channels per pixel
    const uint8_t *p;
    size_t pitch;
    int w, h;
    uint32_t border;  // one byte per channel
    __device__ __forceinline__ uint32_t operator()(int X, int Y) const {
        if ((unsigned)X < (unsigned)w && (unsigned)Y < (unsigned)h) {
            const uint8_t *s = p + (size_t)Y * pitch + (size_t)X * CN;
            uint32_t v = s[0];
            if constexpr (CN > 1) v |= (uint32_t)s[1] << 8;
            if constexpr (CN > 2) v |= (uint32_t)s[2] << 16;
            return v;
        }
        return border;
    }
};

// ---------------------------------------------------------------------------------------------------------------------
// The blends: (sum + 2^14) >> 15 from the fixed-point tables (vstab_cubic.hpp, vstab_lanczos4.hpp).
// ---------------------------------------------------------------------------------------------------------------------
// One channel (byte CH of every tap dword) of the blend: channel pairs of horizontally adjacent taps gathered into int16 pairs by
// v_perm_b32, eight v_dot2_i32_i16 against the weight pairs.  |sum| < 16 * 32767 * 255: no overflow.
template <int CH>
__device__ __forceinline__ uint32_t cubic_channel(const uint32_t (&t)[16], const uint32_t (&w)[8]) {
    constexpr uint32_t sel = CH | 0x0c00u | ((4u + CH) << 16) | 0x0c000000u;  // [left.CH, 0, right.CH, 0]
    typedef short short2v __attribute__((ext_vector_type(2)));
    int acc = 1 << 14;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        acc = __builtin_amdgcn_sdot2(__builtin_bit_cast(short2v, __builtin_amdgcn_perm(t[4 * r + 1], t[4 * r], sel)), __builtin_bit_cast(short2v, w[2 * r]),
                                     acc, false);
        acc = __builtin_amdgcn_sdot2(__builtin_bit_cast(short2v, __builtin_amdgcn_perm(t[4 * r + 3], t[4 * r + 2], sel)),
                                     __builtin_bit_cast(short2v, w[2 * r + 1]), acc, false);
    }
    return (uint32_t)sat8(acc >> 15);
}

// One footprint row of one channel (byte CH of every tap dword): channel pairs of horizontally adjacent taps gathered into int16 pairs by
// v_perm_b32, four v_dot2_i32_i16 against the row's weight pairs.  |sum| over the 64 taps < 64 * 32767 * 255: no overflow.
template <int CH>
__device__ __forceinline__ int lz_row(int acc, const uint32_t (&t)[8], const uint4 &w) {
    constexpr uint32_t sel = CH | 0x0c00u | ((4u + CH) << 16) | 0x0c000000u;  // [left.CH, 0, right.CH, 0]
    typedef short short2v __attribute__((ext_vector_type(2)));
    acc = __builtin_amdgcn_sdot2(__builtin_bit_cast(short2v, __builtin_amdgcn_perm(t[1], t[0], sel)), __builtin_bit_cast(short2v, w.x), acc, false);
    acc = __builtin_amdgcn_sdot2(__builtin_bit_cast(short2v, __builtin_amdgcn_perm(t[3], t[2], sel)), __builtin_bit_cast(short2v, w.y), acc, false);
    acc = __builtin_amdgcn_sdot2(__builtin_bit_cast(short2v, __builtin_amdgcn_perm(t[5], t[4], sel)), __builtin_bit_cast(short2v, w.z), acc, false);
    acc = __builtin_amdgcn_sdot2(__builtin_bit_cast(short2v, __builtin_amdgcn_perm(t[7], t[6], sel)), __builtin_bit_cast(short2v, w.w), acc, false);
    return acc;
}

// 32 * map of output pixel (x, y): k_quantised_map's arithmetic (the fused kernels' map, bit for bit, in every mode)
template <int MODE>
__device__ __forceinline__ void cubic_map(const CubicArgs &c, int x, int y, float rfx, float rfy, float &ax, float &ay) {
    const MapParams &p = c.w.p;
    const float vy = norm_coord<MODE>((float)y - p.ocy, p.ofy, rfy);
    const RowTerm rt = {p.r[1] * vy, p.r[4] * vy, p.r[7] * vy};
    const float vx = norm_coord<MODE>((float)x - p.ocx, p.ofx, rfx);
    const ColTerm ct = {p.r[0] * vx, p.r[3] * vx, p.r[6] * vx};
    map_pixel_ex<MODE>(c.p32, p, ct, rt, vx, vy, ax, ay);
}

}  // namespace vstab
