// vstab_lanczos4.hpp -- the integer weight table of cv::remap's INTER_LANCZOS4 (OpenCV 4.5 CPU path, 8-bit data), built at compile time.
// Shared by the Lanczos kernels (vstab_warp_lanczos4.hip, which embed it in their code object) and the host (vstab_lanczos4_weights).
//
// Entry (fy, fx) (index fy * 32 + fx, fx / fy = the 1/32-pixel fractions of the quantised map) holds 64 weights w[k1][k2] for the taps
// (X - 3 + k2, Y - 3 + k1):
//   c(x)       interpolateLanczos4(x), x = k * (1 / 32): s0 = sin(y0), c0 = cos(y0), y0 = -(x + 3) * pi / 4 (the committed literals below),
//              c[i] = (float)((cs[i][0] * s0 + cs[i][1] * c0) / (y * y)), y = -(x + 3 - i) * pi / 4, in double; summed in fp32 in order
//              i = 0..7 and each multiplied by 1.f / sum in fp32.  x = 0 is the unit row [0, 0, 0, 1, 0, 0, 0, 0] (OpenCV's early return; its
//              1e30f sentinel for tap 3 gives the same table, tests/test_lanczos4_cpu.py).  No contraction anywhere.
//   w[k1][k2]  saturate_cast<short>(cvRound(c_fy[k1] * c_fx[k2] * 32768.f)), the product in fp32;
//   then initInterTab2D's correction when the 64 weights do not sum to 32768 (LANCZOS4_FIX_LO below).
// Every entry then sums to 32768, so a blend with the border value substituted for each tap outside the source equals OpenCV's
// cval * ONE + sum((S - cval) * w).  Entry 0 is not the identity: 32768 saturates to 32767 at tap (3, 3), outside the correction window, and
// the correction adds 1 at tap (4, 4).  The same definition is restated in numpy by tests/warp_def.py and pinned by
// tests/golden/lanczos4_kat.npz.
#pragma once
#include <stdint.h>

#include "vstab_cubic.hpp"  // cubic_round: cvRound of a float

namespace vstab {

constexpr int LANCZOS4_TAB = 32 * 32;  // entries
// initInterTab2D's correction window: rows and columns {ksize / 2, ksize / 2 + 1} = {4, 5} of the 8 x 8 entry, i.e. the taps at +1 and +2
// from (X, Y)
constexpr int LANCZOS4_FIX_LO = 4;

// sin(y0) and cos(y0), y0 = -(k / 32 + 3) * pi / 4, k = 0..31, in double: the only inputs that cannot be constexpr.  Printed by
// tests/golden/make_lanczos4_golden.py; the table does not move when any of them moves by one ulp (tests/test_lanczos4_cpu.py).
constexpr double LANCZOS4_S0[32] = {
    -0x1.6a09e667f3bcdp-1, -0x1.610b7551d2ce0p-1, -0x1.57d69348ceca1p-1, -0x1.4e6cabbe3e5e8p-1,
    -0x1.44cf325091dd6p-1, -0x1.3affa292050bap-1, -0x1.30ff7fce17036p-1, -0x1.26d054cdd12e0p-1,
    -0x1.1c73b39ae68c8p-1, -0x1.11eb3541b4b22p-1, -0x1.073879922ffeep-1, -0x1.f8ba4dbf89abcp-2,
    -0x1.e2b5d3806f63fp-2, -0x1.cc66e9931c463p-2, -0x1.b5d1009e15cbfp-2, -0x1.9ef7943a8ed8bp-2,
    -0x1.87de2a6aea965p-2, -0x1.7088530fa45a2p-2, -0x1.58f9a75ab1fe2p-2, -0x1.4135c94176600p-2,
    -0x1.294062ed59f06p-2, -0x1.111d262b1f679p-2, -0x1.f19f97b215f21p-3, -0x1.c0b826a7e4f6cp-3,
    -0x1.8f8b83c69a617p-3, -0x1.5e214448b3fc6p-3, -0x1.2c8106e8e613cp-3, -0x1.f564e56a97319p-4,
    -0x1.917a6bc29b43cp-4, -0x1.2d52092ce1a0cp-4, -0x1.91f65f10dd80dp-5, -0x1.92155f7a36689p-6};
constexpr double LANCZOS4_C0[32] = {
    -0x1.6a09e667f3bccp-1, -0x1.72d0837efff95p-1, -0x1.7b5df226aafadp-1, -0x1.83b0e0bff976ep-1,
    -0x1.8bc806b151741p-1, -0x1.93a22499263fbp-1, -0x1.9b3e047f38740p-1, -0x1.a29a7a0462781p-1,
    -0x1.a9b66290ea1a4p-1, -0x1.b090a58150200p-1, -0x1.b728345196e3dp-1, -0x1.bd7c0ac6f9529p-1,
    -0x1.c38b2f180bdb0p-1, -0x1.c954b213411f4p-1, -0x1.ced7af43cc773p-1, -0x1.d4134d14dc93ap-1,
    -0x1.d906bcf328d46p-1, -0x1.ddb13b6ccc23cp-1, -0x1.e212104f686e4p-1, -0x1.e6288ec48e112p-1,
    -0x1.e9f4156c62ddap-1, -0x1.ed740e7684963p-1, -0x1.f0a7efb9230d7p-1, -0x1.f38f3ac64e588p-1,
    -0x1.f6297cff75cb0p-1, -0x1.f8764fa714ba9p-1, -0x1.fa7557f08a517p-1, -0x1.fc26470e19fd3p-1,
    -0x1.fd88da3d12525p-1, -0x1.fe9cdad01883ap-1, -0x1.ff621e3796d7ep-1, -0x1.ffd886084cd0dp-1};

struct alignas(16) Lanczos4Table {  // the kernels read a row of an entry as one 16-byte load
    int16_t w[LANCZOS4_TAB * 64];
};

constexpr void lanczos4_coeffs(int k, float *c) {  // interpolateLanczos4, imgwarp.cpp
    constexpr double s45 = 0.70710678118654752440084436210485, pi = 3.1415926535897932384626433832795;
    constexpr double cs[8][2] = {{1, 0}, {-s45, -s45}, {0, 1}, {s45, -s45}, {-1, 0}, {s45, s45}, {0, -1}, {-s45, s45}};
    const float x = k * (1.f / 32);
    if (k == 0) {
        for (int i = 0; i < 8; i++) c[i] = i == 3 ? 1.f : 0.f;
        return;
    }
    float sum = 0;
    for (int i = 0; i < 8; i++) {
        const double y = -(double)(x + 3 - i) * pi * 0.25;
        c[i] = (float)((cs[i][0] * LANCZOS4_S0[k] + cs[i][1] * LANCZOS4_C0[k]) / (y * y));
        sum += c[i];
    }
    sum = 1.f / sum;
    for (int i = 0; i < 8; i++) c[i] *= sum;
}

constexpr Lanczos4Table make_lanczos4_table() {
    Lanczos4Table t{};
    float c[32][8] = {};
    for (int k = 0; k < 32; k++) lanczos4_coeffs(k, c[k]);
    for (int fy = 0; fy < 32; fy++)
        for (int fx = 0; fx < 32; fx++) {
            int16_t *w = t.w + (fy * 32 + fx) * 64;
            int sum = 0;
            for (int k1 = 0; k1 < 8; k1++)
                for (int k2 = 0; k2 < 8; k2++) {
                    const int v = cubic_round(c[fy][k1] * c[fx][k2] * 32768.f);
                    w[k1 * 8 + k2] = (int16_t)(v < -32768 ? -32768 : v > 32767 ? 32767 : v);
                    sum += w[k1 * 8 + k2];
                }
            if (sum != 32768) {
                const int diff = sum - 32768;
                int mk1 = LANCZOS4_FIX_LO, mk2 = LANCZOS4_FIX_LO, Mk1 = LANCZOS4_FIX_LO, Mk2 = LANCZOS4_FIX_LO;
                for (int k1 = LANCZOS4_FIX_LO; k1 < LANCZOS4_FIX_LO + 2; k1++)
                    for (int k2 = LANCZOS4_FIX_LO; k2 < LANCZOS4_FIX_LO + 2; k2++) {
                        if (w[k1 * 8 + k2] < w[mk1 * 8 + mk2]) mk1 = k1, mk2 = k2;
                        else if (w[k1 * 8 + k2] > w[Mk1 * 8 + Mk2]) Mk1 = k1, Mk2 = k2;
                    }
                if (diff < 0) w[Mk1 * 8 + Mk2] = (int16_t)(w[Mk1 * 8 + Mk2] - diff);
                else w[mk1 * 8 + mk2] = (int16_t)(w[mk1 * 8 + mk2] - diff);
            }
        }
    return t;
}

}  // namespace vstab
