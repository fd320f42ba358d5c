// vstab_cubic.hpp -- the integer weight table of cv::remap's INTER_CUBIC (OpenCV 4.5 CPU path, 8-bit data), built at compile time.
// Shared by the cubic kernels (vstab_warp_cubic.hip, which embed it in their code object) and the host (vstab_cubic_weights).
//
// Entry (fy, fx) (index fy * 32 + fx, fx / fy = the 1/32-pixel fractions of the quantised map) holds 16 weights w[k1][k2] for the taps
// (X - 1 + k2, Y - 1 + k1):
//   c(x)       interpolateCubic(x) in fp32, A = -0.75, x = k * (1 / 32)  -- the operation order of OpenCV's imgwarp.cpp, no contraction;
//   w[k1][k2]  saturate_cast<short>(cvRound(c_fy[k1] * c_fx[k2] * 32768.f)), the product in fp32;
//   then initInterTab2D's correction when the 16 weights do not sum to 32768 (CUBIC_FIX_LO below).
// Every entry then sums to 32768, so a blend with the border value substituted for each tap outside the source equals OpenCV's
// cval * ONE + sum((S - cval) * w).  The same definition is restated in numpy by tests/warp_def.py and pinned by tests/golden/cubic_kat.npz.
#pragma once
#include <stdint.h>

namespace vstab {

constexpr int CUBIC_TAB = 32 * 32;  // entries
// initInterTab2D's correction window: rows and columns {ksize / 2, ksize / 2 + 1} = {2, 3} of the 4 x 4 entry, i.e. the taps at
// +1 and +2 from (X, Y).  The one detail of the definition no test here can hold against OpenCV itself (tests/test_cubic_cpu.py
// compares with cv2 where it is installed).
constexpr int CUBIC_FIX_LO = 2;

struct alignas(16) CubicTable {  // the kernels read an entry as two 16-byte loads
    int16_t w[CUBIC_TAB * 16];
};

// cvRound of a finite float well inside the int range: round half to even
constexpr int cubic_round(float v) {
    const double d = v;
    long long t = (long long)d;  // toward zero
    const double fr = d - (double)t;
    if (fr > 0.5 || (fr == 0.5 && (t & 1))) t += 1;
    else if (fr < -0.5 || (fr == -0.5 && (t & 1))) t -= 1;
    return (int)t;
}

constexpr void cubic_coeffs(float x, float *c) {  // interpolateCubic, imgwarp.cpp
    const float A = -0.75f;
    c[0] = ((A * (x + 1) - 5 * A) * (x + 1) + 8 * A) * (x + 1) - 4 * A;
    c[1] = ((A + 2) * x - (A + 3)) * x * x + 1;
    c[2] = ((A + 2) * (1 - x) - (A + 3)) * (1 - x) * (1 - x) + 1;
    c[3] = 1.f - c[0] - c[1] - c[2];
}

constexpr CubicTable make_cubic_table() {
    CubicTable t{};
    float c[32][4] = {};
    for (int k = 0; k < 32; k++) cubic_coeffs(k * (1.f / 32), c[k]);
    for (int fy = 0; fy < 32; fy++)
        for (int fx = 0; fx < 32; fx++) {
            int16_t *w = t.w + (fy * 32 + fx) * 16;
            int sum = 0;
            for (int k1 = 0; k1 < 4; k1++)
                for (int k2 = 0; k2 < 4; k2++) {
                    const int v = cubic_round(c[fy][k1] * c[fx][k2] * 32768.f);
                    w[k1 * 4 + k2] = (int16_t)(v < -32768 ? -32768 : v > 32767 ? 32767 : v);
                    sum += w[k1 * 4 + k2];
                }
            if (sum != 32768) {
                const int diff = sum - 32768;
                int mk1 = CUBIC_FIX_LO, mk2 = CUBIC_FIX_LO, Mk1 = CUBIC_FIX_LO, Mk2 = CUBIC_FIX_LO;
                for (int k1 = CUBIC_FIX_LO; k1 < CUBIC_FIX_LO + 2; k1++)
                    for (int k2 = CUBIC_FIX_LO; k2 < CUBIC_FIX_LO + 2; k2++) {
                        if (w[k1 * 4 + k2] < w[mk1 * 4 + mk2]) mk1 = k1, mk2 = k2;
                        else if (w[k1 * 4 + k2] > w[Mk1 * 4 + Mk2]) Mk1 = k1, Mk2 = k2;
                    }
                if (diff < 0) w[Mk1 * 4 + Mk2] = (int16_t)(w[Mk1 * 4 + Mk2] - diff);
                else w[mk1 * 4 + mk2] = (int16_t)(w[mk1 * 4 + mk2] - diff);
            }
        }
    return t;
}

}  // namespace vstab
