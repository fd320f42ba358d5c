// vstab_border.hpp -- what the border-mode kernels (vstab_warp_border.hip, vstab_warp_resample_border.hip) share: OpenCV's borderInterpolate
// in closed form, the sources a virtual position reads, the tile's box in virtual coordinates and its staging into LDS.
#pragma once
#include <climits>

#include "../../include/vstab.h"
#include "vstab_device.hpp"

namespace vstab {

// OpenCV's borderInterpolate in closed form: REPLICATE clamps; REFLECT folds by the period 2 len, REFLECT_101 by 2 len - 2 (len 1 -> 0).
// Equal to OpenCV's loop for every p in [-32768, 32768] and len in [1, 32767] (tests/test_border_cpu.py restates it).  CONSTANT: p itself.
template <int BORDER>
__device__ __forceinline__ int border_index(int p, int len) {
    if constexpr (BORDER == VSTAB_BORDER_CONSTANT) {
        return p;
    } else {
        if ((unsigned)p < (unsigned)len) return p;
        if constexpr (BORDER == VSTAB_BORDER_REPLICATE) {
            return p < 0 ? 0 : len - 1;
        } else {
            constexpr int D = BORDER == VSTAB_BORDER_REFLECT_101 ? 1 : 0;
            if (D && len == 1) return 0;
            const int per = 2 * len - 2 * D;
            int q = p % per;
            q += q < 0 ? per : 0;
            return q < len ? q : per - 1 + D - q;  // REFLECT: 2 len - 1 - q; REFLECT_101: 2 len - 2 - q
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Sources: a virtual position (X, Y) as a dword with one channel per byte -- read at its border-interpolated position, or the border value
// (CONSTANT) where it lies outside.
// ---------------------------------------------------------------------------------------------------------------------
template <int BORDER>
struct BorderNv12Bgr {  // NV12 planes converted with the cvtColor arithmetic (BGRx); CONSTANT border 0
    const uint8_t *y, *uv;
    size_t pitch_y, pitch_uv;
    int w, h;
    __device__ __forceinline__ uint32_t at(int X, int Y) const {  // X, Y inside
        const int yv = y[(size_t)Y * pitch_y + X];
        const uint16_t c = *reinterpret_cast<const uint16_t *>(uv + (size_t)(Y >> 1) * pitch_uv + (X & ~1));
        int b, g, r;
        yuv_to_bgr(yv, chroma_term(c & 255, c >> 8), b, g, r);
        return (uint32_t)b | ((uint32_t)g << 8) | ((uint32_t)r << 16);
    }
    __device__ __forceinline__ uint32_t row_col(int X, int Y) const {  // X, Y already border-interpolated
        if constexpr (BORDER == VSTAB_BORDER_CONSTANT) {
            if (!((unsigned)X < (unsigned)w && (unsigned)Y < (unsigned)h)) return 0;
        }
        return at(X, Y);
    }
};
template <int CN, int BORDER>
struct BorderBytes {  // CN interleaved 8-bit channels per pixel
    const uint8_t *p;
    size_t pitch;
    int w, h;
    uint32_t border;  // CONSTANT: one byte per channel
    __device__ __forceinline__ uint32_t at(int X, int Y) const {  // X, Y inside
        const uint8_t *s = p + (size_t)Y * pitch + (size_t)X * CN;
        uint32_t v = s[0];
        if constexpr (CN > 1) v |= (uint32_t)s[1] << 8;
        if constexpr (CN > 2) v |= (uint32_t)s[2] << 16;
        return v;
    }
    __device__ __forceinline__ uint32_t row_col(int X, int Y) const {  // X, Y already border-interpolated
        if constexpr (BORDER == VSTAB_BORDER_CONSTANT) {
            if (!((unsigned)X < (unsigned)w && (unsigned)Y < (unsigned)h)) return border;
        }
        return at(X, Y);
    }
};

// ---------------------------------------------------------------------------------------------------------------------
// The tile's box and its staging.
// ---------------------------------------------------------------------------------------------------------------------
struct BorderBox {
    int x0, y0, w, h;
    bool lds;  // staged (uniform over the workgroup)
};

// min / max of the top-left tap positions a thread passes in, reduced over the workgroup through red[16] in LDS; the box covers X .. X + 1,
// Y .. Y + 1 of all of them (a wider footprint passes its first column / row and the one before its last)
__device__ __forceinline__ BorderBox border_box(int mnx, int mxx, int mny, int mxy, int *red, int cap_elems) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        mnx = min(mnx, __shfl_xor(mnx, m)), mxx = max(mxx, __shfl_xor(mxx, m));
        mny = min(mny, __shfl_xor(mny, m)), mxy = max(mxy, __shfl_xor(mxy, m));
    }
    const int wave = threadIdx.x >> 6;
    __syncthreads();  // red[] may still be read by a previous box
    if ((threadIdx.x & 63) == 0) red[4 * wave] = mnx, red[4 * wave + 1] = mxx, red[4 * wave + 2] = mny, red[4 * wave + 3] = mxy;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; k++) mnx = min(mnx, red[4 * k]), mxx = max(mxx, red[4 * k + 1]), mny = min(mny, red[4 * k + 2]), mxy = max(mxy, red[4 * k + 3]);
    const bool have = mnx <= mxx;  // else the tile has no pixel (cannot happen: every thread evaluates a clamped pixel)
    BorderBox b;  // the same in every lane: scalar registers
    b.x0 = __builtin_amdgcn_readfirstlane(mnx), b.y0 = __builtin_amdgcn_readfirstlane(mny);
    b.w = __builtin_amdgcn_readfirstlane(have ? mxx - mnx + 2 : 0), b.h = __builtin_amdgcn_readfirstlane(have ? mxy - mny + 2 : 0);
    b.lds = have && (long)b.w * b.h <= cap_elems;
    return b;
}

// every virtual position of the box read once (rows by wave, columns by lane).  A box inside the source -- most tiles -- reads it as it
// is; any other goes through borderInterpolate, each column's position once for all its rows (the fold's integer remainder is ~20 vector
// instructions: evaluated per staged element it made the kernel VALU-bound at twice the cost of this form)
template <int BORDER, typename T, typename Src>
__device__ __forceinline__ void border_stage(const Src &s, const BorderBox &b, T *lds) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (b.x0 >= 0 && b.x0 + b.w <= s.w && b.y0 >= 0 && b.y0 + b.h <= s.h) {  // uniform
        for (int r = wave; r < b.h; r += 4)
            for (int c = lane; c < b.w; c += 64) lds[r * b.w + c] = (T)s.at(b.x0 + c, b.y0 + r);
    } else {
        for (int c = lane; c < b.w; c += 64) {
            const int sx = border_index<BORDER>(b.x0 + c, s.w);
            for (int r = wave; r < b.h; r += 4) lds[r * b.w + c] = (T)s.row_col(sx, border_index<BORDER>(b.y0 + r, s.h));
        }
    }
}

}  // namespace vstab
