// vstab_pyramid.hip -- the image pyramid of the camera-motion front-end for gfx950: cv::pyrDown as buildOpticalFlowPyramid uses it, one
// level per launch (k_pyr_down), fused with the copy of an upstream frame (k_pack_pyr), or two levels per launch (k_pyr_down_x2).
// Compiled with -ffp-contract=off; everything here is integer arithmetic.
#include <algorithm>

#include <hip/hip_ext.h>

#include "vstab_internal.hpp"
#include "vstab_track.hpp"
#include "vstab_track_device.hpp"

namespace vstab {

// =============================================================================================
// k_pyr_down -- cv::pyrDown as used by buildOpticalFlowPyramid: 5x5 binomial
// [1 4 6 4 1]^2, integer, (sum + 128) >> 8, REFLECT_101, dst = ((w+1)/2, (h+1)/2).
// Register-only: one thread produces 4 adjacent outputs of one row from five 16-byte row segments
// (aligned dword loads; the overlap between neighbouring threads is served by L1/L2).  The 25 taps of
// an output are accumulated with v_dot4_u32_u8 straight on the packed source dwords: the weight
// dword of row j holds k_j * (1 4 6 4 1) at the byte positions of the taps (<= 36, a byte), two
// dot products per output and row, so no byte is ever unpacked.  One dword store.  No LDS, no
// barriers: the kernel is a pure stream and overlaps with the LK kernel of the previous frame.
// (That is the one-row body: the edge groups, k_pack_pyr and k_pyr_down_x2.  The interior workgroups of k_pyr_down
// run pyr_down_rows below: PYR_ROWS output rows a thread, every source row loaded and summed horizontally once.)
// =============================================================================================
__device__ __forceinline__ uint32_t udot4(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_udot4(a, b, c, false); }

// Four adjacent outputs from the five 16-byte row segments that hold their taps (output c uses bytes 2c+2 .. 2c+6 of a segment), packed into
// one dword: the weight dword of row j holds k_j * (1 4 6 4 1) at the byte positions of the taps, two dot products per output and row.
__device__ __forceinline__ uint32_t pyr_down_dot4x4(const uint32_t (&d)[5][4]) {
    uint32_t acc[4] = {128u, 128u, 128u, 128u};
#pragma unroll
    for (int j = 0; j < 5; j++) {
        const uint32_t k = j == 0 || j == 4 ? 1u : j == 2 ? 6u : 4u;
        // weight dwords (byte 0 = lowest address): taps 1 4 | 6 4 1 split over two dwords, or 1 4 6 4 | 1
        const uint32_t w_hi2 = (k << 16) | (4 * k << 24);          // (0, 0, k, 4k)
        const uint32_t w_lo3 = 6 * k | (4 * k << 8) | (k << 16);   // (6k, 4k, k, 0)
        const uint32_t w_all = k | (4 * k << 8) | (6 * k << 16) | (4 * k << 24);  // (k, 4k, 6k, 4k)
        acc[0] = udot4(d[j][1], w_lo3, udot4(d[j][0], w_hi2, acc[0]));
        acc[1] = udot4(d[j][2], k, udot4(d[j][1], w_all, acc[1]));
        acc[2] = udot4(d[j][2], w_lo3, udot4(d[j][1], w_hi2, acc[2]));
        acc[3] = udot4(d[j][3], k, udot4(d[j][2], w_all, acc[3]));
    }
    // result byte c = bits 8..15 of acc[c] (sum + 128 <= 255 * 256 + 128 < 2^16)
    const uint32_t p01 = __builtin_amdgcn_perm(acc[1], acc[0], 0x0c0c0501u), p23 = __builtin_amdgcn_perm(acc[3], acc[2], 0x0c0c0501u);
    return __builtin_amdgcn_perm(p23, p01, 0x05040100u);
}

// outputs x0 .. x0+3 of row y, packed.  EDGE = false: the 16-byte window lies inside the row and everything is dword aligned.
// NEAR: sw >= 16 and sh >= 4, so that every tap is within one reflection of the image.
// COPY: the group also copies the source bytes it owns -- columns 2 x0 .. 2 x0 + 7 of rows 2 y and 2 y + 1, which it has loaded anyway
// (dwords 1 and 2 of window rows 2 and 3) -- to `cp` (pitch cpitch, 8-byte aligned rows when !EDGE): k_pack_pyr, the copy of an
// upstream frame into the ring and the first pyramid level in one pass over the luma plane.
template <bool EDGE, bool NEAR, bool COPY = false>
__device__ __forceinline__ uint32_t pyr_down_group4(const uint8_t *__restrict__ src, uint32_t spitch, int sw, int sh, int x0, int y, bool vec_ok,
                                                    uint8_t *__restrict__ cp = nullptr, uint32_t cpitch = 0) {
    const int sx0 = 2 * x0 - 4;  // the 16 bytes [sx0, sx0+16) hold the taps of outputs x0..x0+3: output c uses bytes 2c+2 .. 2c+6
    const uint8_t *row[5];
#pragma unroll
    for (int j = 0; j < 5; j++) {
        const int ry = 2 * y - 2 + j;
        row[j] = src + (uint32_t)(NEAR ? min(abs(ry), 2 * sh - 2 - abs(ry)) : reflect101(ry, sh)) * spitch;
    }
    uint32_t d[5][4];
    if (!EDGE) {
        if (y >= 1 && 2 * y + 2 < sh) {
            // wave-uniform (a wave is one output row): the five source rows 2y - 2 .. 2y + 2 are inside the image, so their
            // addresses are one multiply and four pitch steps -- the reflection of every row (five quarter-rate 32-bit
            // multiplies, ten 64-bit adds, twenty min / max / sub) was a third of the kernel's vector instructions
            const uint8_t *r0 = src + (size_t)(uint32_t)(2 * y - 2) * spitch + sx0;
#pragma unroll
            for (int j = 0; j < 5; j++) {
                const uint4 v = *reinterpret_cast<const uint4 *>(r0 + (size_t)j * spitch);  // one 16-byte load (4-byte aligned: global loads take any alignment)
                d[j][0] = v.x, d[j][1] = v.y, d[j][2] = v.z, d[j][3] = v.w;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 5; j++) {
                const uint32_t *p = reinterpret_cast<const uint32_t *>(row[j] + sx0);
                d[j][0] = p[0], d[j][1] = p[1], d[j][2] = p[2], d[j][3] = p[3];
            }
        }
    } else {
        // Whether a dword lies inside the row is the same for the five rows: one branch per dword column, the five (or
        // twenty byte) loads under it in flight together -- a branch per load would cost a memory latency per load.
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int gx = sx0 + 4 * q;
            if (vec_ok && gx >= 0 && gx + 4 <= sw) {
#pragma unroll
                for (int j = 0; j < 5; j++) d[j][q] = *reinterpret_cast<const uint32_t *>(row[j] + gx);
            } else {
                int col[4];
#pragma unroll
                for (int i = 0; i < 4; i++) col[i] = NEAR ? min(abs(gx + i), 2 * sw - 2 - abs(gx + i)) : reflect101(gx + i, sw);
#pragma unroll
                for (int j = 0; j < 5; j++)
                    d[j][q] = (uint32_t)row[j][col[0]] | ((uint32_t)row[j][col[1]] << 8) | ((uint32_t)row[j][col[2]] << 16) | ((uint32_t)row[j][col[3]] << 24);
            }
        }
    }
    if (COPY) {
#pragma unroll
        for (int jj = 2; jj <= 3; jj++) {
            const int r = 2 * y + jj - 2;
            if (r >= sh) break;  // (an odd height's last output row has no second source row)
            uint8_t *o = cp + (uint32_t)r * cpitch + (uint32_t)(2 * x0);
            if (!EDGE) {
                *reinterpret_cast<uint2 *>(o) = make_uint2(d[jj][1], d[jj][2]);
            } else {
#pragma unroll
                for (int b = 0; b < 8; b++)
                    if (2 * x0 + b < sw) o[b] = (uint8_t)((b < 4 ? d[jj][1] : d[jj][2]) >> (8 * (b & 3)));
            }
        }
    }
    return pyr_down_dot4x4(d);
}

template <bool EDGE, bool NEAR, bool COPY = false>
__device__ __forceinline__ void pyr_down_group(const uint8_t *__restrict__ src, uint32_t spitch, int sw, int sh, uint8_t *__restrict__ dst, size_t dpitch,
                                               int dw, int x0, int y, bool vec_ok, uint8_t *__restrict__ cp = nullptr, uint32_t cpitch = 0) {
    const uint32_t out = pyr_down_group4<EDGE, NEAR, COPY>(src, spitch, sw, sh, x0, y, vec_ok, cp, cpitch);
    uint8_t *o = dst + (size_t)((uint32_t)y * (uint32_t)dpitch) + x0;  // one 32-bit multiply (the launchers refuse dpitch * dh >= 2^32)
    if (!EDGE) {
        *reinterpret_cast<uint32_t *>(o) = out;
    } else {
        for (int c = 0; c < 4 && x0 + c < dw; c++) o[c] = (uint8_t)(out >> (8 * c));
    }
}

// The interior body of k_pyr_down: one thread produces outputs 4g .. 4g+3 of the R rows y0 .. y0+R-1 from 2R + 3 source rows, each loaded
// once (16 bytes at 8g - 4) and summed horizontally once.  The filter is separable and everything is an integer, so the order is free:
//   horizontal, per source row: h_c = (1 4 6 4 1) . bytes 2c+2 .. 2c+6, two dot products per output against the unscaled weights
//     (h <= 16 * 255 = 4080), and the four sums paired into 16-bit halves of two dwords (h0 | h1 << 16, h2 | h3 << 16);
//   vertical, per output row and pair: h[0] + h[4] + 4 (h[1] + h[2] + h[3]) + 2 h[2] + 128 in plain 32-bit adds on the pairs -- the
//     largest half is 255 * 256 + 128 = 65408 < 2^16, so nothing carries from the low half into the high one;
//   the result bytes are bits 8 .. 15 of the four halves: one v_perm, one dword store per row.
// A wave is 64 groups of ONE row group (y0 is made a scalar), so the row addresses, REFLECT_101 of the row index at the top and bottom
// of the image, and the test that drops the rows past dh of the last row group are scalar instructions; a load's address is the thread's
// column address plus a scalar row offset (one 64-bit add).  A row index still negative after the fold -- only dropped rows tap it --
// is clamped to row 0: read, never used.
// All 2R + 3 loads are issued before the first dependent instruction: one memory latency per thread, as before.
template <int R>
__device__ __forceinline__ void pyr_down_rows(const uint8_t *__restrict__ src, uint32_t spitch, int sh, uint8_t *__restrict__ dst, uint32_t dpitch, int dh, int g,
                                              int y0) {
    constexpr int NS = 2 * R + 3;
    const uint32_t sx0 = 8u * (uint32_t)g - 4u;  // (g >= 1)
    uint4 v[NS];
#pragma unroll
    for (int j = 0; j < NS; j++) {
        const int a = abs(2 * y0 - 2 + j), ry = max(min(a, 2 * sh - 2 - a), 0);
        v[j] = *reinterpret_cast<const uint4 *>(src + (size_t)((uint32_t)ry * spitch) + sx0);  // (16 bytes at a 4-byte aligned address: global loads take any alignment)
    }
    uint32_t p[NS][2];
#pragma unroll
    for (int j = 0; j < NS; j++) {
        // weight dwords (byte 0 = lowest address), as in pyr_down_dot4x4 with k = 1
        const uint32_t w_hi2 = 0x04010000u, w_lo3 = 0x00010406u, w_all = 0x04060401u;
        const uint32_t h0 = udot4(v[j].y, w_lo3, udot4(v[j].x, w_hi2, 0u)), h1 = udot4(v[j].z, 1u, udot4(v[j].y, w_all, 0u));
        const uint32_t h2 = udot4(v[j].z, w_lo3, udot4(v[j].y, w_hi2, 0u)), h3 = udot4(v[j].w, 1u, udot4(v[j].z, w_all, 0u));
        p[j][0] = (h1 << 16) | h0, p[j][1] = (h3 << 16) | h2;
    }
#pragma unroll
    for (int r = 0; r < R; r++) {
        uint32_t s[2];
#pragma unroll
        for (int q = 0; q < 2; q++) {
            const uint32_t mid = p[2 * r + 1][q] + p[2 * r + 3][q] + p[2 * r + 2][q];
            const uint32_t out = p[2 * r][q] + p[2 * r + 4][q] + 0x00800080u;
            s[q] = (mid << 2) + ((p[2 * r + 2][q] << 1) + out);
        }
        if (y0 + r < dh) *reinterpret_cast<uint32_t *>(dst + (size_t)((uint32_t)(y0 + r) * dpitch) + 4u * (uint32_t)g) = __builtin_amdgcn_perm(s[1], s[0], 0x07050301u);
    }
}

// Output rows a thread of k_pyr_down's interior workgroups produces (R above).  4 and 2 were built and measured (DESIGN section 31,
// profiles/pyr_rows_4k.txt): 4 is kept for every height; -DVSTAB_PYR_ROWS=2 rebuilds the other for a comparison.
#ifndef VSTAB_PYR_ROWS
#define VSTAB_PYR_ROWS 4
#endif
constexpr int PYR_ROWS = VSTAB_PYR_ROWS;

// Groups of 4 outputs [g_lo, g_hi) of every row are interior (64 groups x 4 rows per workgroup; in k_pyr_down, R > 1, 64 groups x
// 4 row groups of R rows, a wave being one row group); the remaining groups --
// the first of a row, the last one to three, or all of them for an unaligned or tiny image -- are gathered in workgroups
// of their own, so that no wavefront of the bulk ever runs the byte path.  Those come first in the grid: they are the
// slow ones.  (pyr_grid on the host side.)
template <bool COPY, int R = 1>
__device__ __forceinline__ void pyr_down_dispatch(const uint8_t *__restrict__ src, uint32_t spitch, int sw, int sh, uint8_t *__restrict__ dst, size_t dpitch, int dw,
                                                  int dh, int vec_ok, int g_lo, int g_hi, int nbx, int nb_edge, int n_groups, int near,
                                                  uint8_t *__restrict__ cp = nullptr, uint32_t cpitch = 0) {
    if ((int)blockIdx.x >= nb_edge) {
        const int b = blockIdx.x - nb_edge, by = b / nbx, bx = b - by * nbx;
        if constexpr (R > 1) {
            static_assert(!COPY, "the fused copy keeps the one-row body");
            const int g = g_lo + bx * 64 + (threadIdx.x & 63);
            const int y0 = R * __builtin_amdgcn_readfirstlane(by * 4 + (threadIdx.x >> 6));  // (a wave is one row group)
            if (g >= g_hi || y0 >= dh) return;
            pyr_down_rows<R>(src, spitch, sh, dst, (uint32_t)dpitch, dh, g, y0);
            return;
        }
        const int g = g_lo + bx * 64 + (threadIdx.x & 63), y = by * 4 + (threadIdx.x >> 6);
        if (g >= g_hi || y >= dh) return;
        pyr_down_group<false, true, COPY>(src, spitch, sw, sh, dst, dpitch, dw, 4 * g, y, true, cp, cpitch);
    } else {
        const int n_edge = n_groups - (g_hi - g_lo);  // edge groups per row
        const int e = blockIdx.x * 256 + threadIdx.x;
        const int y = e / n_edge, i = e - y * n_edge;
        if (y >= dh) return;
        const int g = i < g_lo ? i : g_hi + (i - g_lo);
        if (near)
            pyr_down_group<true, true, COPY>(src, spitch, sw, sh, dst, dpitch, dw, 4 * g, y, vec_ok != 0, cp, cpitch);
        else
            pyr_down_group<true, false, COPY>(src, spitch, sw, sh, dst, dpitch, dw, 4 * g, y, vec_ok != 0, cp, cpitch);
    }
}

__global__ void __launch_bounds__(256) k_pyr_down(const uint8_t *__restrict__ src, size_t spitch, int sw, int sh,
                                                  uint8_t *__restrict__ dst, size_t dpitch, int dw, int dh, int vec_ok, int g_lo, int g_hi,
                                                  int nbx, int nb_edge, int n_groups, int near) {
    pyr_down_dispatch<false, PYR_ROWS>(src, (uint32_t)spitch, sw, sh, dst, dpitch, dw, dh, vec_ok, g_lo, g_hi, nbx, nb_edge, n_groups, near);
}

// k_pack_pyr -- the copy of an upstream NV12 frame into the library's ring AND the first pyramid level of its luma plane in one launch
// (vstab_frame.hold = 0: a decoder that recycles its surfaces): every group of k_pyr_down also stores the 8 x 2 source bytes it owns,
// and workgroups behind the pyramid's copy the chroma plane.  One pass over the luma instead of two, one kernel less on the read-ahead
// stream.  Same arithmetic, same bytes.
__global__ void __launch_bounds__(256) k_pack_pyr(const uint8_t *__restrict__ src, uint32_t spitch, int sw, int sh, uint8_t *__restrict__ dst, uint32_t dpitch,
                                                  int dw, int dh, int vec_ok, int g_lo, int g_hi, int nbx, int nb_edge, int n_groups, int near, int nb_pyr,
                                                  const uint8_t *__restrict__ uv, uint32_t uvpitch, uint8_t *__restrict__ ring, uint32_t rpitch, int uv_vec) {
    if ((int)blockIdx.x >= nb_pyr) {
        // chroma: sh / 2 rows of sw bytes behind the luma rows of the ring, 16 bytes per thread where everything is aligned
        uint8_t *cdst = ring + (uint32_t)sh * rpitch;
        const int rows = sh / 2;
        if (uv_vec) {
            const int vecs = sw / 16;
            for (int e = ((int)blockIdx.x - nb_pyr) * 256 + threadIdx.x; e < rows * vecs; e += ((int)gridDim.x - nb_pyr) * 256) {
                const int r = e / vecs, c = e - r * vecs;
                reinterpret_cast<uint4 *>(cdst + (uint32_t)r * rpitch)[c] = reinterpret_cast<const uint4 *>(uv + (uint32_t)r * uvpitch)[c];
            }
        } else {
            for (int e = ((int)blockIdx.x - nb_pyr) * 256 + threadIdx.x; e < rows * sw; e += ((int)gridDim.x - nb_pyr) * 256) {
                const int r = e / sw, c = e - r * sw;
                cdst[(uint32_t)r * rpitch + c] = uv[(uint32_t)r * uvpitch + c];
            }
        }
        return;
    }
    pyr_down_dispatch<true>(src, spitch, sw, sh, dst, dpitch, dw, dh, vec_ok, g_lo, g_hi, nbx, nb_edge, n_groups, near, ring, rpitch);
}

// =============================================================================================
// k_pyr_down_x2 -- TWO pyramid levels in one launch (levels 2 and 3 of the LK pyramid from level 1): the small levels are
// launch- and latency-bound as kernels of their own (a 4K frame's level 3 is 480 x 270), and the prefetch stream paid three
// launches per frame.  A workgroup owns 16 x 10 outputs of the SECOND level: it computes the 40 x 23 first-level outputs around
// them straight from global memory with the arithmetic of k_pyr_down (four outputs per thread: 230 of the 256 threads, all
// loads of the workgroup in flight at once; into LDS, and to global memory for the 32 x 20 of them it owns), then the second
// level from those, four outputs per thread with the same dot products on the LDS dwords -- reflecting FIRST-LEVEL coordinates,
// as pyrDown of the stored first level does.  Integer sums: exact in any order.
// (The first version staged the 80 x 57 source bytes of a 14 x 12 tile in LDS, index arithmetic included, and produced one
// second-level output per thread: 0.58 M vector instructions per 4K frame and 6.3 us alone; this one 5.2 us (4.1 at 1080p).
// Tiles of 28 x 22 with three groups per thread need fewer instructions still but leave a 1080p frame 63 workgroups: 9 us.)
// =============================================================================================
constexpr int P2_TW = 16, P2_TH = 10;                   // second-level outputs per workgroup
constexpr int P2_MG = (2 * P2_TW + 5 + 3) / 4, P2_MW = 4 * P2_MG;  // first-level region: groups of 4 columns from 2 x0 - 4 on (taps of the tile: 2 x0 - 2 .. 2 x0 + 2 P2_TW)
constexpr int P2_MH = 2 * P2_TH + 3;                    // rows 2 y0 - 2 .. 2 y0 + 2 P2_TH
constexpr int P2_ITEMS = P2_MG * P2_MH, P2_ROUNDS = (P2_ITEMS + 255) / 256;
static_assert(P2_TW % 4 == 0 && 2 * P2_TW + 5 <= P2_MW, "the region holds the taps of the tile's last output");

template <bool NEAR>
__device__ __forceinline__ void pyr_down_x2_tile(const uint8_t *__restrict__ src, uint32_t spitch, int sw, int sh, uint8_t *__restrict__ mid, uint32_t mpitch, int mw,
                                                 int mh, uint8_t *__restrict__ dst, uint32_t dpitch, int dw, int dh, bool vec_ok, bool dst_vec_ok,
                                                 uint8_t (&smid)[P2_MH][P2_MW]) {
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * P2_TW, y0 = blockIdx.y * P2_TH;  // second-level origin of the tile
    const int mx0 = 2 * x0 - 4, my0 = 2 * y0 - 2;                 // first-level origin of the region
    // an interior workgroup: every first-level output of its region exists, and all their taps (source columns 2 mx0 - 4 .. 2 mx0 + 2 P2_MW + 3,
    // rows 2 my0 - 2 .. 2 my0 + 2 P2_MH) lie inside the source -- aligned dword loads, no reflection in either level, whole tile inside dst
    const bool interior = vec_ok && mx0 >= 2 && my0 >= 1 && mx0 + P2_MW <= mw && my0 + P2_MH <= mh && 2 * (mx0 + P2_MW) + 4 <= sw && 2 * (my0 + P2_MH) + 1 <= sh;  // uniform
    // ---- first level: P2_MG groups of 4 outputs x P2_MH rows, one group per thread (P2_ROUNDS = 1 with the 16 x 10 tile) --------------------------
    if (interior) {
        // every load of the thread's groups first (one memory latency however many rounds), then the arithmetic
        uint32_t d[P2_ROUNDS][5][4];
#pragma unroll
        for (int k = 0; k < P2_ROUNDS; k++) {
            const int it = min(tid + 256 * k, P2_ITEMS - 1);  // (a thread past the end loads the last group again and drops it)
            const int ry = it / P2_MG, g = it - ry * P2_MG;
            const uint8_t *r0 = src + (uint32_t)(2 * (my0 + ry) - 2) * spitch + (uint32_t)(2 * (mx0 + 4 * g) - 4);
#pragma unroll
            for (int j = 0; j < 5; j++) {
                const uint4 v = *reinterpret_cast<const uint4 *>(r0 + (uint32_t)j * spitch);  // (16 bytes at a 4-byte aligned address: global loads take any alignment)
                d[k][j][0] = v.x, d[k][j][1] = v.y, d[k][j][2] = v.z, d[k][j][3] = v.w;
            }
        }
#pragma unroll
        for (int k = 0; k < P2_ROUNDS; k++) {
            const int it = tid + 256 * k;
            if (it >= P2_ITEMS) break;
            const int ry = it / P2_MG, g = it - ry * P2_MG;
            const uint32_t out = pyr_down_dot4x4(d[k]);
            *reinterpret_cast<uint32_t *>(&smid[ry][4 * g]) = out;
            // the tile owns first-level columns 2 x0 .. 2 x0 + 2 P2_TW - 1 (groups 1 .. P2_TW / 2) and rows 2 y0 .. 2 y0 + 2 P2_TH - 1
            if (g >= 1 && g <= P2_TW / 2 && ry >= 2 && ry < 2 + 2 * P2_TH) *reinterpret_cast<uint32_t *>(mid + (uint32_t)(my0 + ry) * mpitch + (mx0 + 4 * g)) = out;
        }
    } else {
#pragma unroll 1
        for (int k = 0; k < P2_ROUNDS; k++) {
            const int it = tid + 256 * k;
            if (it >= P2_ITEMS) break;
            const int ry = it / P2_MG, g = it - ry * P2_MG;
            const int my = my0 + ry, mx = mx0 + 4 * g;
            if (my < 0 || my >= mh || mx < 0 || mx >= mw) continue;  // (outside the first level: never read -- the second level reflects its coordinates into the image)
            const uint32_t out = pyr_down_group4<true, NEAR>(src, spitch, sw, sh, mx, my, vec_ok);
            *reinterpret_cast<uint32_t *>(&smid[ry][4 * g]) = out;
            if (g >= 1 && g <= P2_TW / 2 && ry >= 2 && ry < 2 + 2 * P2_TH) {
                uint8_t *o = mid + (uint32_t)my * mpitch + mx;
                if (vec_ok && mx + 4 <= mw) *reinterpret_cast<uint32_t *>(o) = out;
                else
                    for (int c = 0; c < 4 && mx + c < mw; c++) o[c] = (uint8_t)(out >> (8 * c));
            }
        }
    }
    __syncthreads();
    // ---- second level from the first-level region ----------------------------------------------------------------------------------------------
    if (interior) {
        // four outputs per item: their taps are bytes 8 g + 2 c + 2 .. + 6 of region rows 2 ty .. 2 ty + 4 -- the layout of pyr_down_dot4x4
        if (tid < (P2_TW / 4) * P2_TH) {
            const int ty = tid / (P2_TW / 4), g = tid - ty * (P2_TW / 4);
            uint32_t d[5][4];
#pragma unroll
            for (int j = 0; j < 5; j++) {
                const uint2 lo = *reinterpret_cast<const uint2 *>(&smid[2 * ty + j][8 * g]), hi = *reinterpret_cast<const uint2 *>(&smid[2 * ty + j][8 * g + 8]);
                d[j][0] = lo.x, d[j][1] = lo.y, d[j][2] = hi.x, d[j][3] = hi.y;
            }
            const uint32_t out = pyr_down_dot4x4(d);
            uint8_t *o = dst + (uint32_t)(y0 + ty) * dpitch + (x0 + 4 * g);
            if (dst_vec_ok) *reinterpret_cast<uint32_t *>(o) = out;
            else
                for (int c = 0; c < 4; c++) o[c] = (uint8_t)(out >> (8 * c));
        }
    } else {
        // border workgroups: output by output, REFLECT_101 in first-level coordinates
        for (int e = tid; e < P2_TW * P2_TH; e += 256) {
            const int ty = e / P2_TW, tx = e - ty * P2_TW;
            const int x = x0 + tx, y = y0 + ty;
            if (x >= dw || y >= dh) continue;
            int col[5];
#pragma unroll
            for (int i = 0; i < 5; i++) col[i] = reflect101(2 * x - 2 + i, mw) - mx0;
            uint32_t acc = 128u;
#pragma unroll
            for (int j = 0; j < 5; j++) {
                const uint8_t *r = smid[reflect101(2 * y - 2 + j, mh) - my0];
                const uint32_t k = j == 0 || j == 4 ? 1u : j == 2 ? 6u : 4u;
                acc += k * ((uint32_t)r[col[0]] + 4u * r[col[1]] + 6u * r[col[2]] + 4u * r[col[3]] + r[col[4]]);
            }
            dst[(uint32_t)y * dpitch + x] = (uint8_t)(acc >> 8);
        }
    }
}

__global__ void __launch_bounds__(256) k_pyr_down_x2(const uint8_t *__restrict__ src, uint32_t spitch, int sw, int sh, uint8_t *__restrict__ mid,
                                                     uint32_t mpitch, int mw, int mh, uint8_t *__restrict__ dst, uint32_t dpitch, int dw, int dh, int vec_ok,
                                                     int dst_vec_ok, int near) {
    __shared__ __attribute__((aligned(16))) uint8_t smid[P2_MH][P2_MW];
    if (near) pyr_down_x2_tile<true>(src, spitch, sw, sh, mid, mpitch, mw, mh, dst, dpitch, dw, dh, vec_ok != 0, dst_vec_ok != 0, smid);
    else pyr_down_x2_tile<false>(src, spitch, sw, sh, mid, mpitch, mw, mh, dst, dpitch, dw, dh, vec_ok != 0, dst_vec_ok != 0, smid);
}

// ---------------------------------------------------------------------------------------------
// host launchers
// ---------------------------------------------------------------------------------------------
// The grid of k_pyr_down / k_pack_pyr: group g = outputs 4g .. 4g+3 reads source bytes [8g - 4, 8g + 12), so it is interior iff g >= 1,
// 8g + 12 <= sw and 4g + 4 <= dw -- and only where rows are dword aligned and every tap within one reflection (`wide` = vec_ok && near).
// nb_edge workgroups of 256 edge groups come first, then nb_int = nbx x div_up(dh, 4 rows) workgroups of 64 interior groups x 4 row groups
// of `rows` rows each (k_pack_pyr: 1; k_pyr_down: PYR_ROWS).
struct PyrGrid {
    int n_groups, g_lo, g_hi, nbx, nb_int, nb_edge;
};
static PyrGrid pyr_grid(int sw, int dw, int dh, bool wide, int rows = 1) {
    const int n_groups = div_up(dw, 4), g_lo = 1, g_hi = wide ? std::max(g_lo, std::min(sw >= 12 ? (sw - 12) / 8 + 1 : 0, dw / 4)) : g_lo;
    const int nbx = div_up(g_hi - g_lo, 64);
    return {n_groups, g_lo, g_hi, nbx, nbx * (int)div_up(dh, 4 * rows), (int)div_up(dh * (n_groups - (g_hi - g_lo)), 256)};
}

// `done` (optional): an event that completes with this kernel -- bound to the launch itself (hipExtLaunchKernelGGL's stop event), so that the
// stream carries no marker packet of its own behind the kernel: a hipEventRecord after every frame's pyramid cost the prefetch stream ~6 us
// per frame (rocprofv3 kernel trace: the next frame's first kernel started 6.5 us after this frame's last one ended, 0.0 us between two kernels)
vstab_status check_pyr_down(size_t spitch, int /*sw*/, int sh, size_t dpitch) {
    // the kernel forms row offsets as 32-bit products
    if ((uint64_t)spitch * (uint64_t)sh >= (1ull << 32) || (uint64_t)dpitch * (uint64_t)((sh + 1) / 2) >= (1ull << 32))
        return fail(VSTAB_ERR_INVALID, "pyr_down: planes of 4 GiB or more are not supported");
    return VSTAB_OK;
}
vstab_status launch_pyr_down(const uint8_t *src, size_t spitch, int sw, int sh, uint8_t *dst, size_t dpitch,
                             hipStream_t s, hipEvent_t done) {
    const int dw = (sw + 1) / 2, dh = (sh + 1) / 2;
    VSTAB_TRY(check_pyr_down(spitch, sw, sh, dpitch));
    const int vec_ok = reinterpret_cast<uintptr_t>(src) % 4 == 0 && spitch % 4 == 0 && reinterpret_cast<uintptr_t>(dst) % 4 == 0 && dpitch % 4 == 0;
    const int near = sw >= 16 && sh >= 4;
    const PyrGrid g = pyr_grid(sw, dw, dh, vec_ok && near, PYR_ROWS);
    hipExtLaunchKernelGGL(k_pyr_down, dim3(g.nb_edge + g.nb_int), dim3(256), 0, s, nullptr, done, 0, src, spitch, sw, sh, dst, dpitch, dw, dh, vec_ok, g.g_lo, g.g_hi, g.nbx,
                          g.nb_edge, g.n_groups, near);
    VSTAB_HIP_TRY(hipGetLastError());
    return VSTAB_OK;
}

// Copy + first level in one launch (k_pack_pyr): ring = the NV12 frame (y, uv) packed (luma rows of pitch w, chroma rows behind them: what
// vstab_pack_nv12 writes), dst = pyrDown(luma).  Only where pack_pyr_ok says so; `copied` (optional) completes with the launch.
bool pack_pyr_ok(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int w, int h, const void *ring, const void *dst, size_t dpitch) {
    return w >= 16 && h >= 4 && !(w & 7) && !(h & 1) && reinterpret_cast<uintptr_t>(y) % 4 == 0 && pitch_y % 4 == 0 && reinterpret_cast<uintptr_t>(ring) % 8 == 0 &&
           reinterpret_cast<uintptr_t>(dst) % 4 == 0 && dpitch % 4 == 0 && pitch_y < (1u << 24) && pitch_uv < (1u << 24) && (uint64_t)pitch_y * (uint64_t)h < (1ull << 32) &&
           (uint64_t)pitch_uv * (uint64_t)(h / 2) < (1ull << 32) &&  // (k_pack_pyr forms row * pitch_uv in 32 bits)
           (uint64_t)dpitch * (uint64_t)((h + 1) / 2) < (1ull << 32) &&  // (and row * dpitch, as k_pyr_down does)
           (uint64_t)w * (uint64_t)h * 3 / 2 < (1ull << 32);
}
vstab_status launch_pack_pyr(const uint8_t *y, size_t pitch_y, const uint8_t *uv, size_t pitch_uv, int sw, int sh, uint8_t *ring, uint8_t *dst, size_t dpitch,
                             hipStream_t s, hipEvent_t copied) {
    const int dw = (sw + 1) / 2, dh = (sh + 1) / 2;
    if (!pack_pyr_ok(y, pitch_y, uv, pitch_uv, sw, sh, ring, dst, dpitch)) return fail(VSTAB_ERR_INVALID, "pack_pyr: planes not aligned for the fused copy");
    const PyrGrid g = pyr_grid(sw, dw, dh, true);  // (pack_pyr_ok: aligned rows, sw >= 16, sh >= 4)
    const int uv_vec = reinterpret_cast<uintptr_t>(uv) % 16 == 0 && pitch_uv % 16 == 0 && sw % 16 == 0 && reinterpret_cast<uintptr_t>(ring) % 16 == 0;
    const int nb_uv = std::max(1, std::min(256, (int)div_up((unsigned)(sw * (sh / 2)), 256u * 16u)));
    hipExtLaunchKernelGGL(k_pack_pyr, dim3(g.nb_edge + g.nb_int + nb_uv), dim3(256), 0, s, nullptr, copied, 0, y, (uint32_t)pitch_y, sw, sh, dst, (uint32_t)dpitch, dw, dh, 1,
                          g.g_lo, g.g_hi, g.nbx, g.nb_edge, g.n_groups, 1, g.nb_edge + g.nb_int, uv, (uint32_t)pitch_uv, ring, (uint32_t)sw, uv_vec);
    VSTAB_HIP_TRY(hipGetLastError());
    return VSTAB_OK;
}

// Two levels in one launch (k_pyr_down_x2): mid = pyrDown(src), dst = pyrDown(mid).  Needs an image a reflected tap never leaves
// twice (>= 4 x 4 at the middle level); the caller falls back to two single-level launches otherwise.
bool pyr_down_x2_ok(int sw, int sh) { return (sw + 1) / 2 >= 8 && (sh + 1) / 2 >= 8; }
vstab_status check_pyr_down_x2(size_t spitch, int sw, int sh, size_t mpitch, size_t dpitch) {
    const int mh = (sh + 1) / 2, dh = (mh + 1) / 2;
    if (!pyr_down_x2_ok(sw, sh)) return fail(VSTAB_ERR_INVALID, "pyr_down_x2: image too small");
    if ((uint64_t)spitch * (uint64_t)sh >= (1ull << 32) || (uint64_t)mpitch * (uint64_t)mh >= (1ull << 32) || (uint64_t)dpitch * (uint64_t)dh >= (1ull << 32))
        return fail(VSTAB_ERR_INVALID, "pyr_down_x2: planes of 4 GiB or more are not supported");
    return VSTAB_OK;
}
vstab_status launch_pyr_down_x2(const uint8_t *src, size_t spitch, int sw, int sh, uint8_t *mid, size_t mpitch, uint8_t *dst, size_t dpitch, hipStream_t s,
                                hipEvent_t done) {
    const int mw = (sw + 1) / 2, mh = (sh + 1) / 2, dw = (mw + 1) / 2, dh = (mh + 1) / 2;
    VSTAB_TRY(check_pyr_down_x2(spitch, sw, sh, mpitch, dpitch));
    const int vec_ok = reinterpret_cast<uintptr_t>(src) % 4 == 0 && spitch % 4 == 0 && reinterpret_cast<uintptr_t>(mid) % 4 == 0 && mpitch % 4 == 0;
    const int dst_vec_ok = reinterpret_cast<uintptr_t>(dst) % 4 == 0 && dpitch % 4 == 0;
    const int near = sw >= 16 && sh >= 4;
    hipExtLaunchKernelGGL(k_pyr_down_x2, dim3(div_up(dw, P2_TW), div_up(dh, P2_TH)), dim3(256), 0, s, nullptr, done, 0, src, (uint32_t)spitch, sw, sh, mid,
                          (uint32_t)mpitch, mw, mh, dst, (uint32_t)dpitch, dw, dh, vec_ok, dst_vec_ok, near);
    VSTAB_HIP_TRY(hipGetLastError());
    return VSTAB_OK;
}

// Kernels of this translation unit are one code object, loaded by the runtime at the first launch of any of them.  Touching one of them
// here (vstab_preload_kernels) moves that load to a moment the caller chooses.
vstab_status preload_pyramid_kernels() {
    hipFuncAttributes at;
    VSTAB_HIP_TRY(hipFuncGetAttributes(&at, reinterpret_cast<const void *>(&k_pyr_down)));
    return VSTAB_OK;
}

}  // namespace vstab
