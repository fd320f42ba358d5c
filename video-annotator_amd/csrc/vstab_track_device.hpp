// vstab_track_device.hpp -- device-side helpers shared by the tracking kernels: vstab_pyramid.hip, vstab_lk.hip and vstab_lk_win.hip
// (vstab_lk_window.hpp) and, through vstab_corners_tile.hpp, the corner units (vstab_corners.hip, vstab_corners_fused.hip, vstab_corners_block.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vstab {

__device__ __forceinline__ int reflect101(int i, int n) {  // BORDER_REFLECT_101, any overshoot
    if (n == 1) return 0;
    while (i < 0 || i >= n) i = i < 0 ? -i : 2 * n - 2 - i;
    return i;
}

// One dword of a REFLECT_101-padded u8 image at (gx .. gx+3, gy), gx a multiple of 4.  Dwords that lie
// inside the row are one aligned load (also on border tiles); only dwords straddling the left /
// right image edge are assembled from bytes.
__device__ __forceinline__ uint32_t load4_reflect(const uint8_t *__restrict__ src, uint32_t pitch, int w, int h, int gx,
                                                  int gy, bool vec_ok) {
    const uint8_t *row = src + (uint32_t)reflect101(gy, h) * pitch;
    if (vec_ok && gx >= 0 && gx + 4 <= w) return *reinterpret_cast<const uint32_t *>(row + gx);
    uint32_t v = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) v |= (uint32_t)row[reflect101(gx + i, w)] << (8 * i);
    return v;
}

// e / d for 0 <= e < n as one 24-bit multiply and a shift: (e * magic) >> 16 (the compiler's division by a constant is a 64-bit
// multiply-high)
constexpr bool div_magic_ok(int d, int magic, int n) {
    for (int e = 0; e < n; e++)
        if (((e * magic) >> 16) != e / d) return false;
    return true;
}

}  // namespace vstab
