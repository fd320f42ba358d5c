// vstab_corners_fused.hip -- the one-pass corner detector for gfx950: response, threshold and 3x3 non-maximum test in one kernel
// (k_corners_fused; under a detection mask k_corners_fused_masked; with the Harris response k_corners_fused_harris and
// k_corners_fused_harris_masked), then k_filter_keys with the final threshold.  The two-pass detector behind it is vstab_corners.hip.
// Replaces the OpenCV call at FrameSourceWarp.cpp:230 (goodFeaturesToTrack).  Compiled with -ffp-contract=off: float results are
// bit-reproducible.
#include "vstab_corners_tile.hpp"
#include "vstab_internal.hpp"

namespace vstab {

// =============================================================================================
// k_corners_fused -- cornerMinEigenVal + the threshold / 3x3 non-maximum test of goodFeaturesToTrack in ONE pass
// over the image: the eigenvalue map never goes to HBM.  A workgroup owns 64 x 31 output
// pixels and evaluates the eigenvalue on the 66 x 33 pixels around them (the halo ring is recomputed, 1.11x), so the
// 3x3 maximum test needs nothing from a neighbour.
//   load    72 x 38 source bytes -> LDS, one dword per thread and round (row = index / 18 by multiply and shift)
//   prod    68 x 35 Sobel pairs and their float products dx dx, dx dy, dy dy, each formed ONCE per derivative pixel:
//           119 threads (two waves, the other two wait at the barrier: an idle wave issues nothing) own 4 columns x
//           5 rows each and share the per-row terms D = I(x+1) - I(x-1), S = I(x) k0 + (I(x-1) + I(x+1)) k1 between
//           them (7 source rows for 5 output rows); same float operation order as k_min_eig -> identical bits.  The
//           derivative at a position mirrored across the image border has the sign of the mirrored axis flipped
//           (k_min_eig): that leaves dx dx and dy dy as they are and flips dx dy when exactly one axis is mirrored.
//           Three float planes -> LDS
//   box     242 threads own 3 x 3 pixels: per quantity the 5 x 5 products are widened once and added in double (box
//           sums of float products are exact in double in any order: <= 48 significant bits), the middle pair of a
//           column or row is shared by the sums around it: 40 additions per quantity for 9 box sums; ONE
//           double -> float conversion per box sum
//   eig     behind a barrier, since the eigenvalues take the storage of the dx dx plane: eigenvalue in float as
//           k_min_eig -> LDS, tile maximum
//   nms     3x3 maximum with v_max3, threshold, append of 64-bit keys with one LDS atomic per wave
// A tile whose 72 x 38 source bytes all lie inside an image of dword-aligned rows (one workgroup-uniform test) takes
// a path without reflection arithmetic, sign flips and image-bounds tests.
// The threshold quality * max(frame) is not known until every tile is done, so a tile filters with a LOWER bound of
// it -- quality * max(own tile, frame maximum published so far) -- and k_filter_keys applies the final threshold to
// the survivors.  Which candidates survive the first filter depends on timing; the set that survives the second
// does not (lower bound <= final threshold, monotone rounding), and the host sorts the keys.
// =============================================================================================
// (CF_TW x CF_TH = 64 x 31 output pixels per tile and CF_SLOTS = 256 key slots per tile -- a tile holds at most 1984 / 4 strict 3x3
// maxima; fine noise reaches ~220 -- are part of the scratch layout: vstab_track.hpp)
constexpr int CF_EH = CF_TH + 2;                      // eigenvalue region: 66 x 33, image (oy - 1 .., ox - 1 ..)
constexpr int CF_DH = 35, CF_DP = 68;                 // derivative-product region: 68 x 35, image (oy - 2 .., ox - 2 ..)
using CfSource = SourceTile3;                           // source tile: 72 x 38 from image (oy - 3 .., ox - 4 ..); 37 rows used
constexpr int CF_SW = CfSource::SW, CF_SH = CfSource::SH;
constexpr int CF_EP = 67;
constexpr int CF_PC = CF_DP / 4, CF_PR = 5, CF_PG = CF_DH / CF_PR;  // prod: 17 column groups of 4, 7 row groups of 5
constexpr int CF_BX = 22, CF_BY = 11;                  // box / eig: 22 x 11 blocks of 3 x 3
static_assert(CF_PC * 4 == CF_DP && CF_PG * CF_PR == CF_DH && CF_DH + 2 <= CF_SH && CF_PC * CF_PG <= 256, "prod ownership covers the region");
static_assert(CF_BX * 3 == CF_TW + 2 && CF_BY * 3 == CF_EH && CF_EH + 2 == CF_DH && CF_BX * CF_BY <= 256, "box ownership covers the region");
static_assert(CF_EH * CF_EP <= CF_DH * CF_DP, "the eigenvalues fit the plane they take over");

// row and column of a product group and a box block as one 24-bit multiply and a shift (div_magic_ok)
static_assert(div_magic_ok(CF_PC, 3856, 256) && div_magic_ok(CF_BX, 2979, 256), "division constants");
// the kernel a helper is instantiated for (vstab_corners_tile.hpp has the reason).  In the helpers of this unit MASKED and HARRIS are such
// tags too wherever the text does not use them: HARRIS changes the code in cf_eigenvalues alone.
template <bool MASKED, bool HARRIS>
struct CfTag {};

// byte B of v as a float.  Written as the instruction: from (float)((v >> 8 B) & 255) the compiler builds the differences and sums of two
// bytes in integers (an SDWA operation and a conversion apiece) where the six floats of a row, converted once, serve all of them.
// Static VALU instructions of the prod phase per wave with the plain C++ form / with this one: 329 / 272 on the interior path, 410 / 348
// on the border path (hipcc of ROCm 7.2, -O3; count the instructions between the second and third barrier of a path to see whether a
// later compiler still needs it -- results are the same bits either way).
template <int B>
__device__ __forceinline__ float ubyte_f32(uint32_t v) {
    float f;
    if (B == 0) asm("v_cvt_f32_ubyte0 %0, %1" : "=v"(f) : "v"(v));
    if (B == 1) asm("v_cvt_f32_ubyte1 %0, %1" : "=v"(f) : "v"(v));
    if (B == 2) asm("v_cvt_f32_ubyte2 %0, %1" : "=v"(f) : "v"(v));
    if (B == 3) asm("v_cvt_f32_ubyte3 %0, %1" : "=v"(f) : "v"(v));
    return f;
}

// prod: product entry (r, q) <-> image (oy - 2 + r, ox - 2 + q) <-> tile[r + 1][q + 2]; a thread owns q = 4c .. 4c+3, r = 5g .. 5g+4
template <bool INTERIOR, bool MASKED = false, bool HARRIS = false>
__device__ __forceinline__ void cf_products(const uint8_t (&tile)[CF_SH][CF_SW], float (&prod)[3][CF_DH][CF_DP], int ox, int oy, int w, int h, int tid) {
    if (tid >= CF_PC * CF_PG) return;
    const float scale = (float)(1.0 / (4.0 * 3.0 * 255.0));
    const float k0 = 2.0f * scale, k1 = scale;
    const int g = __mul24(tid, 3856) >> 16, c = tid - g * CF_PC;
    uint32_t flip_x[4];  // the sign bit where the column lies outside the image
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int gx = ox - 2 + 4 * c + i;
        flip_x[i] = !INTERIOR && (gx < 0 || gx >= w) ? 0x80000000u : 0u;
    }
    float D[CF_PR + 2][4], S[CF_PR + 2][4];
#pragma unroll
    for (int j = 0; j < CF_PR + 2; j++) {
        const uint32_t *row = reinterpret_cast<const uint32_t *>(&tile[CF_PR * g + j][4 * c]);
        const uint32_t lo = row[0], hi = row[1];  // bytes 4c .. 4c+7; columns q-1 .. q+4 are bytes 1 .. 6
        const float f[6] = {ubyte_f32<1>(lo), ubyte_f32<2>(lo), ubyte_f32<3>(lo), ubyte_f32<0>(hi), ubyte_f32<1>(hi), ubyte_f32<2>(hi)};
#pragma unroll
        for (int i = 0; i < 4; i++) {
            D[j][i] = f[i + 2] - f[i];
            S[j][i] = f[i + 1] * k0 + (f[i] + f[i + 2]) * k1;
        }
    }
#pragma unroll
    for (int r = 0; r < CF_PR; r++) {
        const int gy = oy - 2 + CF_PR * g + r;
        const uint32_t flip_y = !INTERIOR && (gy < 0 || gy >= h) ? 0x80000000u : 0u;
        float xx[4], xy[4], yy[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const float dx = (D[r][i] + D[r + 2][i]) * k1 + D[r + 1][i] * k0;
            const float dy = S[r + 2][i] - S[r][i];
            xx[i] = dx * dx, yy[i] = dy * dy;
            xy[i] = INTERIOR ? dx * dy : __uint_as_float(__float_as_uint(dx * dy) ^ flip_x[i] ^ flip_y);
        }
        *reinterpret_cast<float4 *>(&prod[0][CF_PR * g + r][4 * c]) = make_float4(xx[0], xx[1], xx[2], xx[3]);
        *reinterpret_cast<float4 *>(&prod[1][CF_PR * g + r][4 * c]) = make_float4(xy[0], xy[1], xy[2], xy[3]);
        *reinterpret_cast<float4 *>(&prod[2][CF_PR * g + r][4 * c]) = make_float4(yy[0], yy[1], yy[2], yy[3]);
    }
}

// the three sums of three consecutive terms out of five, exact in double: the middle pair is shared by the first two
__device__ __forceinline__ void cf_sum3of5(double p0, double p1, double p2, double p3, double p4, double &s0, double &s1, double &s2) {
    const double m = p1 + p2;
    s0 = p0 + m, s1 = m + p3, s2 = (p2 + p3) + p4;
}

// box + eig: eigenvalue entry (ey, ex) <-> image (oy - 1 + ey, ox - 1 + ex) <-> product rows ey .. ey+2, columns ex .. ex+2; a thread owns
// ex = 3bx .. 3bx+2, ey = 3by .. 3by+2.  `es` is the storage of prod[0]: every thread has its box sums in registers before any
// eigenvalue is stored.  Returns the thread's maximum over the in-image eigenvalues (int-bit order, as k_min_eig).
// MASKED: the maximum runs over the eigenvalues with a non-zero mask byte instead (entry (ey, ex) <-> mtile[ey + 2][ex + 3]; a byte outside
// the image is zero there).  The mask bytes must be in `mtile` before the call: the barrier in here orders them before their readers.
// HARRIS: the response is R = (a c - b b) - (kf t) t with t = a + c over the box sums as they are (vstab.h, "Harris response"; no
// contraction in this unit); it is negative over much of an ordinary frame, and the int-bit maximum of a tile without a value >= +0 is
// negative: tile_select filters such a tile with -inf, and whether the FRAME's maximum is positive the host reads from its sign.
template <bool INTERIOR, bool MASKED = false, bool HARRIS = false>
__device__ __forceinline__ int cf_eigenvalues(const float (&prod)[3][CF_DH][CF_DP], float (&es)[CF_EH][CF_EP], int ox, int oy, int w, int h, int tid,
                                              const uint8_t (*mtile)[CF_SW] = nullptr, float kf = 0.0f) {
    const bool active = tid < CF_BX * CF_BY;
    const int t = min(tid, CF_BX * CF_BY - 1);  // the 14 threads without a block add up the last one's sums and store nothing
    const int by = __mul24(t, 2979) >> 16, bx = t - by * CF_BX;
    float sum[3][3][3];  // [quantity][row][column] box sums rounded to float
    {
#pragma unroll
        for (int q = 0; q < 3; q++) {
            double col[3][5];
#pragma unroll
            for (int i = 0; i < 5; i++) {
                double p[5];
#pragma unroll
                for (int j = 0; j < 5; j++) p[j] = (double)prod[q][3 * by + j][3 * bx + i];
                cf_sum3of5(p[0], p[1], p[2], p[3], p[4], col[0][i], col[1][i], col[2][i]);
            }
#pragma unroll
            for (int e = 0; e < 3; e++) {
                double s[3];
                cf_sum3of5(col[e][0], col[e][1], col[e][2], col[e][3], col[e][4], s[0], s[1], s[2]);
#pragma unroll
                for (int i = 0; i < 3; i++) sum[q][e][i] = (float)s[i];
            }
        }
    }
    __syncthreads();
    int best = INT_MIN;
    if (active) {
#pragma unroll
        for (int e = 0; e < 3; e++)
#pragma unroll
            for (int i = 0; i < 3; i++) {
                float ev;
                if (HARRIS) {
                    const float a = sum[0][e][i], b = sum[1][e][i], cc = sum[2][e][i], t = a + cc;
                    ev = (a * cc - b * b) - (kf * t) * t;
                } else {
                    const float a = sum[0][e][i] * 0.5f, b = sum[1][e][i], cc = sum[2][e][i] * 0.5f;
                    ev = (a + cc) - sqrtf((a - cc) * (a - cc) + b * b);
                }
                es[3 * by + e][3 * bx + i] = ev;
                const int gx = ox - 1 + 3 * bx + i, gy = oy - 1 + 3 * by + e;
                if (MASKED) {
                    if (mtile[3 * by + e + 2][3 * bx + i + 3] != 0) best = max(best, __float_as_int(ev));
                } else if (INTERIOR || (gx >= 0 && gx < w && gy >= 0 && gy < h)) best = max(best, __float_as_int(ev));
            }
    }
    return best;
}

// One tile, source to keys: the toolkit of vstab_corners_tile.hpp around cf_products and cf_eigenvalues.
// MASKED (k_corners_fused_masked; `mask`: a w x h plane of bytes, non-zero = "a corner may be reported here"):
//   - a tile without a non-zero mask byte among the in-image pixels of its 66 x 33 eigenvalues writes a count of 0 and returns before it
//     loads the source (tile_masked_out; its flags lie in prod, which is first written behind the barrier that follows tile_store);
//   - the tile maximum, and with it the published frame maximum, runs over the eigenvalues with a non-zero mask byte;
//   - a survivor has a non-zero mask byte (tile_nonmax), while the 3 x 3 maximum it is compared with knows no mask.
// The mask bytes wait in three registers while the source tile is in use and take its place in LDS behind the products.
template <bool INTERIOR, bool MASKED = false, bool HARRIS = false>
__device__ __forceinline__ void cf_tile(uint8_t (&tile)[CF_SH][CF_SW], float (&prod)[3][CF_DH][CF_DP], int &bmax, unsigned int &bcount, unsigned int &bseen,
                                        const uint8_t *__restrict__ src, uint32_t pitch, int w, int h, double quality, unsigned int *__restrict__ max_key,
                                        unsigned long long *__restrict__ slots, unsigned int *__restrict__ tile_counts, float *__restrict__ spill, bool vec_ok,
                                        const uint8_t *__restrict__ mask = nullptr, uint32_t mpitch = 0, bool mvec_ok = false, float kf = 0.0f) {
    using G = CfSource;
    using TAG = CfTag<MASKED, HARRIS>;
    float (&es)[CF_EH][CF_EP] = *reinterpret_cast<float (*)[CF_EH][CF_EP]>(&prod[0][0][0]);
    const int tid = threadIdx.x;
    const int ox = blockIdx.x * CF_TW, oy = blockIdx.y * CF_TH;
    uint32_t mv[G::LOADS];
    if (MASKED) {
        tile_load_mask<G, INTERIOR, TAG>(mv, mask, mpitch, w, h, ox, oy, mvec_ok, tid);
        if (tile_masked_out<G, TAG>(mv, reinterpret_cast<uint32_t *>(&prod[2][0][0]), tid)) {
            if (tid == 0) tile_counts[blockIdx.y * gridDim.x + blockIdx.x] = 0;
            return;
        }
    }
    uint32_t v[G::LOADS];
    tile_load<G, INTERIOR, TAG>(v, src, pitch, w, h, ox, oy, vec_ok, tid);
    if (tid == 0) bmax = INT_MIN, bcount = 0;
    tile_store<G, TAG>(tile, v, tid);
    const unsigned int seen = tile_seen<TAG>(max_key, tid);
    __syncthreads();
    cf_products<INTERIOR, MASKED, HARRIS>(tile, prod, ox, oy, w, h, tid);
    __syncthreads();
    if (MASKED) tile_store<G, TAG>(tile, mv, tid);  // the source bytes are dead; cf_eigenvalues' barrier stands between this and the first reader
    const int best = cf_eigenvalues<INTERIOR, MASKED, HARRIS>(prod, es, ox, oy, w, h, tid, tile, kf);
    tile_select<G, INTERIOR, TAG>(best, seen, es, tile, std::bool_constant<MASKED>(), bmax, bcount, bseen, w, h, quality, max_key, slots, tile_counts, spill);
}

// what each of the four kernels is: the tile's LDS, and cf_tile on the interior path or on the other
template <bool MASKED, bool HARRIS>
__device__ __forceinline__ void cf_kernel(const uint8_t *__restrict__ src, size_t pitch, int w, int h, double quality, unsigned int *__restrict__ max_key,
                                          unsigned long long *__restrict__ slots, unsigned int *__restrict__ tile_counts, float *__restrict__ spill, int vec_ok,
                                          const uint8_t *__restrict__ mask = nullptr, size_t mpitch = 0, int mvec_ok = 0, float kf = 0.0f) {
    __shared__ __attribute__((aligned(16))) uint8_t tile[CF_SH][CF_SW];   // the source bytes; MASKED: behind the products, the mask bytes
    __shared__ __attribute__((aligned(16))) float prod[3][CF_DH][CF_DP];  // dx dx, dx dy, dy dy; then the eigenvalues in place of dx dx
    __shared__ int bmax;
    __shared__ unsigned int bcount, bseen;
    if (tile_interior<CfSource, CfTag<MASKED, HARRIS>>(blockIdx.x * CF_TW, blockIdx.y * CF_TH, w, h, vec_ok))
        cf_tile<true, MASKED, HARRIS>(tile, prod, bmax, bcount, bseen, src, (uint32_t)pitch, w, h, quality, max_key, slots, tile_counts, spill, true, mask, (uint32_t)mpitch,
                                      mvec_ok != 0, kf);
    else
        cf_tile<false, MASKED, HARRIS>(tile, prod, bmax, bcount, bseen, src, (uint32_t)pitch, w, h, quality, max_key, slots, tile_counts, spill, vec_ok != 0, mask,
                                       (uint32_t)mpitch, mvec_ok != 0, kf);
}

__global__ void __launch_bounds__(256) k_corners_fused(const uint8_t *__restrict__ src, size_t pitch, int w, int h, double quality,
                                                       unsigned int *__restrict__ max_key, unsigned long long *__restrict__ slots,
                                                       unsigned int *__restrict__ tile_counts, float *__restrict__ spill, int vec_ok) {
    cf_kernel<false, false>(src, pitch, w, h, quality, max_key, slots, tile_counts, spill, vec_ok);
}

// k_corners_fused_masked -- k_corners_fused under a detection mask (goodFeaturesToTrack's `mask`; vstab.h, "Detection mask"): the same
// phases over the same LDS, cf_tile<., MASKED = true>.  The frame maximum it publishes is the maximum over the masked-in pixels, so
// quality * max(own, seen) is still a lower bound of the final threshold and k_filter_keys serves it unchanged.
// (amdgpu_waves_per_eu: left alone the compiler takes 130 VGPRs here -- three workgroups per CU where k_corners_fused has four; asked for
//  four waves per SIMD it fits 128 without a spill.  DESIGN.md section 24 has the table.)
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) k_corners_fused_masked(const uint8_t *__restrict__ src, size_t pitch, int w, int h, double quality,
                                                              unsigned int *__restrict__ max_key, unsigned long long *__restrict__ slots,
                                                              unsigned int *__restrict__ tile_counts, float *__restrict__ spill, int vec_ok,
                                                              const uint8_t *__restrict__ mask, size_t mpitch, int mvec_ok) {
    cf_kernel<true, false>(src, pitch, w, h, quality, max_key, slots, tile_counts, spill, vec_ok, mask, mpitch, mvec_ok);
}

// k_corners_fused_harris, k_corners_fused_harris_masked -- the two kernels above with the Harris response (goodFeaturesToTrack's
// useHarrisDetector and k; vstab.h, "Harris response"): cf_tile<., ., HARRIS = true>, kf = (float)k.  Everything behind the response is
// shared: a candidate lies above a non-negative threshold wherever the frame has a positive maximum, so its bits order as its value and
// k_filter_keys serves both.  A frame (under a mask: its masked-in part) without a positive response publishes a maximum with the sign
// bit set; the host reports no corner then (no_positive_response: Detector::good_features, Detector::spec_select).
// (The masked kernel does not need the amdgpu_waves_per_eu(4, 4) of its sibling: left alone the compiler takes 100 VGPRs for it, under
//  the 128 of four workgroups per CU, and 119 for the unmasked one.  DESIGN.md section 26 has the table.)
__global__ void __launch_bounds__(256) k_corners_fused_harris(const uint8_t *__restrict__ src, size_t pitch, int w, int h, double quality,
                                                              unsigned int *__restrict__ max_key, unsigned long long *__restrict__ slots,
                                                              unsigned int *__restrict__ tile_counts, float *__restrict__ spill, int vec_ok, float kf) {
    cf_kernel<false, true>(src, pitch, w, h, quality, max_key, slots, tile_counts, spill, vec_ok, nullptr, 0, 0, kf);
}

__global__ void __launch_bounds__(256) k_corners_fused_harris_masked(
    const uint8_t *__restrict__ src, size_t pitch, int w, int h, double quality, unsigned int *__restrict__ max_key, unsigned long long *__restrict__ slots,
    unsigned int *__restrict__ tile_counts, float *__restrict__ spill, int vec_ok, const uint8_t *__restrict__ mask, size_t mpitch, int mvec_ok, float kf) {
    cf_kernel<true, true>(src, pitch, w, h, quality, max_key, slots, tile_counts, spill, vec_ok, mask, mpitch, mvec_ok, kf);
}

// k_filter_keys -- the final threshold quality * max(frame) over the survivors of k_corners_fused.  A workgroup
// gathers the keys of FK_TILES tiles in LDS and appends them with ONE global atomic; a tile that spilled (dense map) is
// scanned row by row and appended per wavefront.  counts[0] = keys kept (may exceed cap_out: the caller then re-runs
// with the two-pass detector, whose key buffer grows), counts[1] = number of spilled tiles (statistics).
constexpr int FK_TILES = 16;
__global__ void __launch_bounds__(256) k_filter_keys(const unsigned long long *__restrict__ slots, const unsigned int *__restrict__ tile_counts,
                                                     const float *__restrict__ spill, int n_tiles, int tiles_x, int w,
                                                     const unsigned int *__restrict__ max_key, double quality,
                                                     unsigned long long *__restrict__ out, unsigned int *__restrict__ counts, unsigned int cap_out) {
    __shared__ unsigned long long kept[FK_TILES * CF_SLOTS];
    __shared__ unsigned int n_kept, base, n_spilled;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    if (tid == 0) n_kept = 0, n_spilled = 0;
    __syncthreads();
    const float thr = (float)((double)__int_as_float((int)(*max_key ^ 0x80000000u)) * quality);
    for (int k = 0; k < FK_TILES / 4; k++) {
        const int t = blockIdx.x * FK_TILES + wave * (FK_TILES / 4) + k;
        if (t >= n_tiles) break;
        const unsigned int n = tile_counts[t];
        if (n > CF_SLOTS) {
            if (lane == 0) atomicAdd(&n_spilled, 1u);
            const int ty0 = t / tiles_x, ox = (t - ty0 * tiles_x) * CF_TW, oy = ty0 * CF_TH;
            float v[CF_TH];  // all 31 rows in flight at once: one memory latency, not 31
#pragma unroll
            for (int r = 0; r < CF_TH; r++) v[r] = spill[(size_t)t * (CF_TW * CF_TH) + r * CF_TW + lane];
#pragma unroll
            for (int r = 0; r < CF_TH; r++) {
                const bool keep = v[r] > thr;
                const unsigned long long ballot = __ballot(keep);
                if (ballot) {
                    unsigned int b = 0;
                    if (lane == 0) b = atomicAdd(&counts[0], (unsigned int)__popcll(ballot));
                    b = __builtin_amdgcn_readfirstlane(b);
                    const unsigned int slot = b + __builtin_amdgcn_mbcnt_hi((uint32_t)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ballot, 0));
                    if (keep && slot < cap_out) out[slot] = ((unsigned long long)__float_as_uint(v[r]) << 32) | (unsigned int)((oy + r) * w + ox + lane);
                }
            }
            continue;
        }
        for (unsigned int i = lane; i < ((n + 63) & ~63u); i += 64) {
            unsigned long long key = 0;
            bool keep = false;
            if (i < n) {
                key = slots[(size_t)t * CF_SLOTS + i];
                keep = __uint_as_float((unsigned int)(key >> 32)) > thr;
            }
            const unsigned long long ballot = __ballot(keep);
            if (ballot) {
                unsigned int b = 0;
                if (lane == 0) b = atomicAdd(&n_kept, (unsigned int)__popcll(ballot));
                b = __builtin_amdgcn_readfirstlane(b);
                if (keep) kept[b + __builtin_amdgcn_mbcnt_hi((uint32_t)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ballot, 0))] = key;
            }
        }
    }
    __syncthreads();
    const unsigned int n = n_kept;
    if (tid == 0) {
        if (n) base = atomicAdd(&counts[0], n);
        if (n_spilled) atomicAdd(&counts[1], n_spilled);
    }
    __syncthreads();
    for (unsigned int i = tid; i < n; i += 256)
        if (base + i < cap_out) out[base + i] = kept[i];
}

// Fused detector.  spec.mask (optional: (uint64_t)mask_pitch * h < 2^32): k_corners_fused_masked takes the place of k_corners_fused,
// everything else is the same; spec.harris: the Harris response in place of the minimum eigenvalue, k_corners_fused_harris /
// k_corners_fused_harris_masked -- words->max then says whether the frame has a positive response at all (no_positive_response);
// spec.block or spec.gradient other than 3: k_corners_fused_block of that pair in their place.
// scratch: corners_fused_scratch_bytes(w, h) (per tile: 256 key slots, a count, and room for a dense 64 x 31 map that only a tile with
// more survivors than slots writes).  On return (stream order) keys holds min(words->kept, cap) keys; the result is complete iff
// words->kept <= cap.
size_t corners_fused_scratch_bytes(int w, int h) { return CornersFusedScratch(w, h).bytes; }

vstab_status launch_corners_fused(const uint8_t *src, size_t pitch, int w, int h, double quality, void *scratch, unsigned long long *keys,
                                  unsigned int cap, DetectorWords *words, hipStream_t s, const DetectSpec &spec) {
    VSTAB_HIP_TRY(hipMemsetAsync(words, 0, sizeof(DetectorWords), s));
    const int vec_ok = reinterpret_cast<uintptr_t>(src) % 4 == 0 && pitch % 4 == 0;
    const int mvec_ok = reinterpret_cast<uintptr_t>(spec.mask) % 4 == 0 && spec.mask_pitch % 4 == 0;
    const CornersFusedScratch lay(w, h);
    uint8_t *base = static_cast<uint8_t *>(scratch);
    unsigned long long *slots = reinterpret_cast<unsigned long long *>(base + lay.slots_off);
    float *spill = reinterpret_cast<float *>(base + lay.spill_off);
    unsigned int *tile_counts = reinterpret_cast<unsigned int *>(base + lay.counts_off);
    const dim3 grid(lay.tiles_x, lay.tiles_y);
    if (spec.block != 3 || spec.gradient != 3)  // one kernel per pair of sizes, mask and response as its arguments (vstab_corners_block.hip)
        VSTAB_TRY(launch_corners_fused_block(src, pitch, w, h, quality, &words->max, slots, tile_counts, spill, grid, s, spec, vec_ok, mvec_ok));
    else if (spec.harris && spec.mask)
        hipLaunchKernelGGL(k_corners_fused_harris_masked, grid, dim3(256), 0, s, src, pitch, w, h, quality, &words->max, slots, tile_counts, spill, vec_ok, spec.mask,
                           spec.mask_pitch, mvec_ok, spec.kf);
    else if (spec.harris)
        hipLaunchKernelGGL(k_corners_fused_harris, grid, dim3(256), 0, s, src, pitch, w, h, quality, &words->max, slots, tile_counts, spill, vec_ok, spec.kf);
    else if (spec.mask)
        hipLaunchKernelGGL(k_corners_fused_masked, grid, dim3(256), 0, s, src, pitch, w, h, quality, &words->max, slots, tile_counts, spill, vec_ok, spec.mask,
                           spec.mask_pitch, mvec_ok);
    else
        hipLaunchKernelGGL(k_corners_fused, grid, dim3(256), 0, s, src, pitch, w, h, quality, &words->max, slots, tile_counts, spill, vec_ok);
    hipLaunchKernelGGL(k_filter_keys, dim3(div_up(lay.tiles, FK_TILES)), dim3(256), 0, s, slots, tile_counts, spill, lay.tiles, lay.tiles_x, w, &words->max, quality, keys,
                       &words->kept, cap);  // counts[0], counts[1] of the kernel: kept, spilled
    VSTAB_HIP_TRY(hipGetLastError());
    return VSTAB_OK;
}

// Kernels of this translation unit are one code object of their own, loaded by the runtime at the first launch of any of them.  Touching
// one of them here (vstab_preload_kernels) moves that load to a moment the caller chooses.
vstab_status preload_corners_fused_kernels() {
    hipFuncAttributes at;
    VSTAB_HIP_TRY(hipFuncGetAttributes(&at, reinterpret_cast<const void *>(&k_corners_fused)));
    // (the masked and Harris kernels and k_filter_keys are kernels of this unit: the same code object, loaded with it)
    return VSTAB_OK;
}

}  // namespace vstab
