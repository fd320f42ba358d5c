// vstab_resample.hpp -- what the cv::remap kernels of the cubic and Lanczos warps (vstab_warp_cubic.hip, vstab_warp_lanczos4.hip) share:
// the launch arguments, the quantisation of a map position (the same for INTER_LINEAR, INTER_CUBIC and INTER_LANCZOS4), the sources a tap
// reads, and the map of an output pixel.
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
