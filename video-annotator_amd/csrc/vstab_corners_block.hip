// vstab_corners_block.hip -- the corner detector's kernels for every pair of block size and gradient size other than (3, 3) (vstab.h,
// "Corner block size" and "Corner gradient size": goodFeaturesToTrack's blockSize and gradientSize, 3, 5 or 7 each): templates over the
// block size B and the gradient size G, one one-pass detector kernel k_corners_fused_block<B, G> and one dense-map kernel
// k_corner_response_block<B, G> per pair.  A further pair is one more entry of CB_KERNELS.  The mask pointer (NULL: none) and
// the response (minimum eigenvalue or Harris) are workgroup-uniform kernel arguments.  The pair (3, 3) is not built from these templates:
// k_corners_fused and its siblings (vstab_corners_fused.hip) and k_min_eig / k_corner_harris (vstab_corners.hip) stay as they are.
// launch_corners_fused (vstab_corners_fused.hip) and launch_corner_response (vstab_corners.hip) come here for every other pair;
// k_filter_keys, k_masked_max and the candidate kernels behind them serve every pair.  Compiled with -ffp-contract=off.
//
// Both kernels work on the tile of the one-pass detector: CF_TW x CF_TH = 64 x 31 output pixels, the response on the 66 x 33 pixels around
// them.  What follows from B and G, r = (B - 1) / 2 and g = (G - 1) / 2:
//   response  66 x 33, image (oy - 1 .., ox - 1 ..)
//   products  (66 + B - 1) x (33 + B - 1), image (oy - 1 - r .., ox - 1 - r ..): 68 x 35, 70 x 37 and 72 x 39
//   source    a ring of g more, from a dword-aligned column (SourceTile<B, G>, vstab_corners_tile.hpp)
// Phases (256 threads, a barrier between any two):
//   load      the source bytes under REFLECT_101 -> LDS, dwords (tile_load, tile_store)
//   prod      the G x G Sobel pair (vstab.h, "Corner gradient size", rules 1 - 4; for G = 3 that of k_min_eig in its operation order, scale
//             1 / (4 B 255)) and the float products dx dx, dx dy, dy dy, each formed once: a thread owns 2 columns x 6 rows (2 + 2 g columns
//             of 6 + 2 g source rows; the last strip of rows overlaps the one before it instead of testing bounds -- two threads then store
//             the same floats).  The derivative at a position mirrored across the image border has the sign of the mirrored axis flipped
//             once per fold: dx dy is flipped where the folds in x and in y differ in parity (an image narrower than r + g + 1 folds more
//             than once).  That holds for every aperture: the REFLECT_101 extension is even about every border pixel and periodic, so the
//             source around a position folded an odd number of times along an axis is the source around its image, mirrored along that
//             axis.  The row differences D are whole numbers and negate exactly where x is mirrored, the smoothed rows S are sums of
//             symmetric pairs and keep their bits; where y is mirrored the pairs of D merely swap and every S(y + i) - S(y - i) negates
//             exactly.  So dx dx and dy dy have the bits of the products at the image position and dx dy differs in its sign only
//   box       the un-normalised B x B sum IN THE ORDER THE DEFINITION FIXES, all in double: the column sum of a product column top to
//             bottom, formed afresh for every output row (no sliding update), then B column sums left to right, ONE rounding to float.
//             The double sums of 5 x 5 and 7 x 7 float products are not always exact (the products of one frame span up to 77 bits), so
//             another order may round another way.  A thread owns 11 columns of one response row: it walks down its B product rows, adds
//             each to its 11 + B - 1 column sums, then adds B column sums across for every output -- a column sum is a pure function of
//             its pixel, so sharing it between horizontally adjacent outputs is the same arithmetic.  One quantity at a time, in a loop
//             that is NOT unrolled, each behind a barrier of its own: the float sums go back into the plane they came from, entry (ey,
//             ex) of the 66 x 33 in place of product (ey, ex).  (Unrolled, with the 33 sums of a thread kept in registers, the compiler
//             moves the loads of all three quantities to the front: 320 VGPRs at B = 5, spills at B = 7.)
//   response  the formula of k_min_eig or of k_corner_harris on the thread's own sums, into the dx dx plane in place
// and then, in k_corners_fused_block, the tile's tail as block 3 has it (tile_select), byte for byte in CornersFusedScratch's layout, so that
// k_filter_keys and the host serve every block size.  A tile whose source box lies inside an image of dword-aligned rows takes a path without
// reflection arithmetic, sign flips and bounds tests (tile_interior, one workgroup-uniform test).
#include "vstab_corners_tile.hpp"
#include "vstab_internal.hpp"

namespace vstab {

constexpr int CB_EW = CF_TW + 2, CB_EH = CF_TH + 2;                        // responses: 66 x 33
constexpr int CB_PR_ROWS = 6;                                               // prod: column groups of 2, row strips of 6
constexpr int CB_BX_NC = 11, CB_BX_CG = CB_EW / CB_BX_NC, CB_BX_RS = CB_EH;  // box: column groups of 11, one row each
static_assert(CB_BX_CG * CB_BX_NC == CB_EW && CB_BX_CG * CB_BX_RS <= 256, "box ownership covers the region");

// the source tile of block B under gradient G and the regions inside it
template <int B, int G>
struct BlockTile : SourceTile<B, G> {
    using S = SourceTile<B, G>;
    static constexpr int PW = CB_EW + B - 1, PH = CB_EH + B - 1;  // products
    static constexpr int PX = S::SX0 - 1 - S::R;                   // product (pr, pq) <-> tile[pr + GR][pq + PX]
    static constexpr int PR_CG = PW / 2, PR_RS = (PH + CB_PR_ROWS - 1) / CB_PR_ROWS;
    static_assert((B == 3 || B == 5 || B == 7) && (G == 3 || G == 5 || G == 7), "block and gradient sizes built from these templates");
    static_assert(S::SH == PH + 2 * S::GR, "the source tile is the products and a ring of g");
    static_assert(PW % 2 == 0 && PR_CG * PR_RS <= 256 && PH >= CB_PR_ROWS && PH - CB_PR_ROWS + (CB_PR_ROWS - 1 + 2 * S::GR) < S::SH, "prod ownership covers the region, its source rows lie in the tile");
    static_assert(PX >= S::GR && PW - 1 + PX + S::GR < S::SW, "every product's source columns lie in the tile");
};

// getDerivKernels' integer Sobel pair of aperture G, from the centre outwards: smoothing s_0 .. s_g, derivative d_0 .. d_g (antisymmetric,
// d_0 = 0).  coef(i): k_i = (float)((double)s_i sigma) with sigma = 1 / (2^(G - 1) B 255) in double -- for G = 3 the k1 = scale_B,
// k0 = 2 scale_B of k_min_eig bit for bit.
template <int G>
struct SobelPair {
    static constexpr int GR = (G - 1) / 2;
    static constexpr int SMOOTH[3][4] = {{2, 1, 0, 0}, {6, 4, 1, 0}, {20, 15, 6, 1}};
    static constexpr int DERIV[3][4] = {{0, 1, 0, 0}, {0, 2, 1, 0}, {0, 5, 4, 1}};
    static constexpr float d(int i) { return (float)DERIV[GR - 1][i]; }
    template <int B>
    static constexpr float coef(int i) {
        return (float)((double)SMOOTH[GR - 1][i] * (1.0 / ((double)(1 << (G - 1)) * B * 255.0)));
    }
};

// whether BORDER_REFLECT_101 folds position i of an axis of n pixels an odd number of times (the sign of a derivative taken there)
__device__ __forceinline__ uint32_t fold_parity(int i, int n) {
    if (n == 1) return 0;
    uint32_t p = 0;
    while (i < 0 || i >= n) i = i < 0 ? -i : 2 * n - 2 - i, p ^= 1u;
    return p;
}

// prod: a thread owns product columns 2 cg, 2 cg + 1 and rows r0 .. r0 + 5, r0 = min(6 rs, PH - 6)
template <int B, int G, bool INTERIOR, class T = BlockTile<B, G>>
__device__ __forceinline__ void cb_products(const uint8_t (&tile)[T::SH][T::SW], float (&prod)[3][T::PH][T::PW], int ox, int oy, int w, int h, int tid) {
    if (tid >= T::PR_CG * T::PR_RS) return;
    using K = SobelPair<G>;
    constexpr int g = T::GR;
    constexpr float k[4] = {K::template coef<B>(0), K::template coef<B>(1), K::template coef<B>(2), K::template coef<B>(3)};  // k_0 .. k_g
    constexpr float d[4] = {K::d(0), K::d(1), K::d(2), K::d(3)};                                                              // d_0 .. d_g
    const int rs = tid / T::PR_CG, cg = tid - rs * T::PR_CG;
    const int r0 = min(CB_PR_ROWS * rs, T::PH - CB_PR_ROWS), q0 = 2 * cg;
    uint32_t flip_x[2];  // the sign bit where the column is folded an odd number of times
#pragma unroll
    for (int i = 0; i < 2; i++) flip_x[i] = INTERIOR ? 0u : fold_parity(ox - 1 - T::R + q0 + i, w) << 31;
    // the row passes, once per source row: D = sum of d_m (I(x + m) - I(x - m)), whole numbers; S = I(x) k_0 + (I(x - 1) + I(x + 1)) k_1 + ..
    float D[CB_PR_ROWS + 2 * g][2], S[CB_PR_ROWS + 2 * g][2];
#pragma unroll
    for (int j = 0; j < CB_PR_ROWS + 2 * g; j++) {
        const uint8_t *row = &tile[r0 + j][q0 + T::PX - g];  // columns q0 - g .. q0 + 1 + g of the product grid
        float f[2 + 2 * g];
#pragma unroll
        for (int c = 0; c < 2 + 2 * g; c++) f[c] = (float)row[c];
#pragma unroll
        for (int i = 0; i < 2; i++) {
            float dsum = f[i + g + 1] - f[i + g - 1], ssum = f[i + g] * k[0] + (f[i + g - 1] + f[i + g + 1]) * k[1];
            if (g > 1) dsum = d[1] * dsum;
#pragma unroll
            for (int m = 2; m <= g; m++) {
                dsum = dsum + d[m] * (f[i + g + m] - f[i + g - m]);
                ssum = ssum + (f[i + g - m] + f[i + g + m]) * k[m];
            }
            D[j][i] = dsum;
            S[j][i] = ssum;
        }
        // G = 7: 12 rows of 8 bytes.  Left alone the optimiser forms every D first and keeps the 96 converted bytes alive for the S that
        // follow: 23 spilled VGPRs.  An empty asm that names the row's four sums has them formed here, row by row.
        if (g == 3) asm volatile("" : "+v"(D[j][0]), "+v"(D[j][1]), "+v"(S[j][0]), "+v"(S[j][1]));
    }
    // the column passes: dx from the outermost pair of rows inwards, the centre last; dy from the innermost pair outwards
#pragma unroll
    for (int r = 0; r < CB_PR_ROWS; r++) {
        const uint32_t flip_y = INTERIOR ? 0u : fold_parity(oy - 1 - T::R + r0 + r, h) << 31;
#pragma unroll
        for (int i = 0; i < 2; i++) {
            float dx = (D[r][i] + D[r + 2 * g][i]) * k[g];
#pragma unroll
            for (int m = g - 1; m >= 1; m--) dx = dx + (D[r + g - m][i] + D[r + g + m][i]) * k[m];
            dx = dx + D[r + g][i] * k[0];
            float dy = S[r + g + 1][i] - S[r + g - 1][i];
            if (g > 1) dy = d[1] * dy;
#pragma unroll
            for (int m = 2; m <= g; m++) dy = dy + d[m] * (S[r + g + m][i] - S[r + g - m][i]);
            prod[0][r0 + r][q0 + i] = dx * dx;
            prod[1][r0 + r][q0 + i] = INTERIOR ? dx * dy : __uint_as_float(__float_as_uint(dx * dy) ^ flip_x[i] ^ flip_y);
            prod[2][r0 + r][q0 + i] = dy * dy;
        }
    }
}

// box: the sums of one quantity for response row e0, columns x0 .. x0 + 10 (products: rows e0 .., columns x0 ..), in the defined order --
// column sums top to bottom, then left to right, in double; one rounding to float
template <int B, int PW>
__device__ __forceinline__ void cb_box(const float (*pl)[PW], int e0, int x0, float (&out)[CB_BX_NC]) {
    constexpr int NCOL = CB_BX_NC + B - 1;
    double col[NCOL];
#pragma unroll
    for (int j = 0; j < B; j++) {
        float f[NCOL];
#pragma unroll
        for (int c = 0; c < NCOL; c++) f[c] = pl[e0 + j][x0 + c];
#pragma unroll
        for (int c = 0; c < NCOL; c++) col[c] = j == 0 ? (double)f[c] : col[c] + (double)f[c];
    }
#pragma unroll
    for (int i = 0; i < CB_BX_NC; i++) {
        double sum = col[i];
#pragma unroll
        for (int k = 1; k < B; k++) sum = sum + col[i + k];
        out[i] = (float)sum;
    }
}

// box + response: entry (ey, ex) <-> image (oy - 1 + ey, ox - 1 + ex) <-> prod[.][ey][ex] once the sums are in place; a thread owns row
// ey = t / 6 and ex = 11 (t % 6) .. + 10.  The threads without a block take the last one's: they add up its sums and store the same floats.
// Returns the thread's maximum (int-bit order, as k_min_eig) over the in-image responses or, under a mask, over those with a non-zero mask
// byte (entry (ey, ex) <-> mtile[ey + SY0 - 1][ex + SX0 - 1]; a byte outside the image is zero there; the barriers in here order the mask
// bytes before their readers).
template <int B, int G, bool INTERIOR, class T = BlockTile<B, G>>
__device__ __forceinline__ int cb_responses(float (&prod)[3][T::PH][T::PW], int ox, int oy, int w, int h, int tid, const uint8_t (*mtile)[T::SW], bool masked, bool harris,
                                            float kf) {
    // (the copies run in the wave of their original, in lockstep with it: none reads back a sum the original has replaced by its response)
    static_assert((CB_BX_CG * CB_BX_RS - 1) / 64 == 255 / 64, "the threads without a block share a wave with the thread they copy");
    const int t = min(tid, CB_BX_CG * CB_BX_RS - 1);
    const int e0 = t / CB_BX_CG, x0 = CB_BX_NC * (t - e0 * CB_BX_CG);
#pragma unroll 1
    for (int q = 0; q < 3; q++) {
        float sum[CB_BX_NC];
        cb_box<B>(prod[q], e0, x0, sum);
        __syncthreads();  // every product of this plane has been read
#pragma unroll
        for (int i = 0; i < CB_BX_NC; i++) prod[q][e0][x0 + i] = sum[i];
    }
    // (what a thread reads back below it wrote itself)
    int best = INT_MIN;
#pragma unroll
    for (int i = 0; i < CB_BX_NC; i++) {
        float ev;
        if (harris) {
            const float a = prod[0][e0][x0 + i], b = prod[1][e0][x0 + i], cc = prod[2][e0][x0 + i], tr = a + cc;
            ev = (a * cc - b * b) - (kf * tr) * tr;
        } else {
            const float a = prod[0][e0][x0 + i] * 0.5f, b = prod[1][e0][x0 + i], cc = prod[2][e0][x0 + i] * 0.5f;
            ev = (a + cc) - sqrtf((a - cc) * (a - cc) + b * b);
        }
        prod[0][e0][x0 + i] = ev;
        const int gx = ox - 1 + x0 + i, gy = oy - 1 + e0;
        if (masked) {
            if (mtile[e0 + T::SY0 - 1][x0 + i + T::SX0 - 1] != 0) best = max(best, __float_as_int(ev));
        } else if (INTERIOR || (gx >= 0 && gx < w && gy >= 0 && gy < h)) best = max(best, __float_as_int(ev));
    }
    return best;
}

// the shared front of both kernels: source -> products -> responses in prod[0] (entry (ey, ex) of the 66 x 33); returns the thread's maximum.
// Under a mask the mask bytes (mv, loaded by the caller) take the source tile's place in LDS behind the products.
template <int B, int G, bool INTERIOR, class T = BlockTile<B, G>>
__device__ __forceinline__ int cb_response_tile(uint8_t (&tile)[T::SH][T::SW], float (&prod)[3][T::PH][T::PW], const uint32_t (&v)[T::LOADS], const uint32_t (&mv)[T::LOADS],
                                                int ox, int oy, int w, int h, bool masked, bool harris, float kf) {
    const int tid = threadIdx.x;
    tile_store<T>(tile, v, tid);
    __syncthreads();
    cb_products<B, G, INTERIOR>(tile, prod, ox, oy, w, h, tid);
    __syncthreads();
    if (masked) tile_store<T>(tile, mv, tid);  // the source bytes are dead; cb_responses' barriers stand between this and the first reader
    return cb_responses<B, G, INTERIOR>(prod, ox, oy, w, h, tid, tile, masked, harris, kf);
}

// One tile of k_corners_fused_block, source to keys.  mask (NULL: none): a tile without a non-zero mask byte among the in-image pixels of its
// 66 x 33 responses writes a count of 0 and returns before it loads the source (tile_masked_out; its flags lie in prod, which is first written
// behind the barriers of cb_response_tile); the tile maximum runs over the responses with a non-zero mask byte; a survivor has a non-zero
// mask byte.
template <int B, int G, bool INTERIOR, class T = BlockTile<B, G>>
__device__ __forceinline__ void cb_tile(uint8_t (&tile)[T::SH][T::SW], float (&prod)[3][T::PH][T::PW], int &bmax, unsigned int &bcount, unsigned int &bseen,
                                        const uint8_t *__restrict__ src, uint32_t pitch, int w, int h, double quality, unsigned int *__restrict__ max_key,
                                        unsigned long long *__restrict__ slots, unsigned int *__restrict__ tile_counts, float *__restrict__ spill, bool vec_ok,
                                        const uint8_t *__restrict__ mask, uint32_t mpitch, bool mvec_ok, bool harris, float kf) {
    const int tid = threadIdx.x;
    const int ox = blockIdx.x * CF_TW, oy = blockIdx.y * CF_TH;
    const int tile_idx = blockIdx.y * gridDim.x + blockIdx.x;
    const bool masked = mask != nullptr;
    uint32_t mv[T::LOADS] = {};
    if (masked) {
        tile_load_mask<T, INTERIOR>(mv, mask, mpitch, w, h, ox, oy, mvec_ok, tid);
        if (tile_masked_out<T>(mv, reinterpret_cast<uint32_t *>(&prod[2][0][0]), tid)) {
            if (tid == 0) tile_counts[tile_idx] = 0;
            return;
        }
    }
    uint32_t v[T::LOADS];
    tile_load<T, INTERIOR>(v, src, pitch, w, h, ox, oy, vec_ok, tid);
    if (tid == 0) bmax = INT_MIN, bcount = 0;
    const unsigned int seen = tile_seen(max_key, tid);
    const int best = cb_response_tile<B, G, INTERIOR>(tile, prod, v, mv, ox, oy, w, h, masked, harris, kf);
    tile_select<T, INTERIOR>(best, seen, prod[0], tile, masked, bmax, bcount, bseen, w, h, quality, max_key, slots, tile_counts, spill);
}

// k_corners_fused_block -- k_corners_fused and its three siblings for block B and gradient G in one kernel: mask (NULL: none) and harris are the same for
// every workgroup of a launch.
template <int B, int G>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) k_corners_fused_block(const uint8_t *__restrict__ src, size_t pitch, int w, int h, double quality, unsigned int *__restrict__ max_key,
                                                             unsigned long long *__restrict__ slots, unsigned int *__restrict__ tile_counts, float *__restrict__ spill,
                                                             int vec_ok, const uint8_t *__restrict__ mask, size_t mpitch, int mvec_ok, int harris, float kf) {
    using T = BlockTile<B, G>;
    __shared__ __attribute__((aligned(16))) uint8_t tile[T::SH][T::SW];  // the source bytes; behind the products, the mask bytes
    __shared__ __attribute__((aligned(16))) float prod[3][T::PH][T::PW];  // dx dx, dx dy, dy dy; then their box sums, then the responses in place of dx dx
    __shared__ int bmax;
    __shared__ unsigned int bcount, bseen;
    if (tile_interior<T>(blockIdx.x * CF_TW, blockIdx.y * CF_TH, w, h, vec_ok))
        cb_tile<B, G, true>(tile, prod, bmax, bcount, bseen, src, (uint32_t)pitch, w, h, quality, max_key, slots, tile_counts, spill, true, mask, (uint32_t)mpitch, mvec_ok != 0,
                         harris != 0, kf);
    else
        cb_tile<B, G, false>(tile, prod, bmax, bcount, bseen, src, (uint32_t)pitch, w, h, quality, max_key, slots, tile_counts, spill, vec_ok != 0, mask, (uint32_t)mpitch,
                          mvec_ok != 0, harris != 0, kf);
}

// k_corner_response_block -- cornerMinEigenVal(B, G) or, harris, cornerHarris(B, G, k) as a dense w x h map, and its int-bit maximum
// (*max_bits, initialised as launch_corner_response does): the front of the kernel above, then the tile's 64 x 31 responses to memory, a
// wave per 8 rows, a lane per column.
template <int B, int G, bool INTERIOR, class T = BlockTile<B, G>>
__device__ __forceinline__ void cb_dense_tile(uint8_t (&tile)[T::SH][T::SW], float (&prod)[3][T::PH][T::PW], int &bmax, const uint8_t *__restrict__ src, uint32_t pitch, int w,
                                              int h, float *__restrict__ resp, int *__restrict__ max_bits, bool vec_ok, bool harris, float kf) {
    const float(&es)[T::PH][T::PW] = prod[0];
    const int tid = threadIdx.x;
    const int ox = blockIdx.x * CF_TW, oy = blockIdx.y * CF_TH;
    uint32_t v[T::LOADS];
    const uint32_t mv[T::LOADS] = {};
    tile_load<T, INTERIOR>(v, src, pitch, w, h, ox, oy, vec_ok, tid);
    if (tid == 0) bmax = INT_MIN;
    int best = cb_response_tile<B, G, INTERIOR>(tile, prod, v, mv, ox, oy, w, h, false, harris, kf);
    best = wave_max_i32(best);
    if ((tid & 63) == 63) atomicMax(&bmax, best);
    __syncthreads();
    if (tid == 0) atomicMax(max_bits, bmax);
    const int tx = tid & 63, x = ox + tx;
    for (int ty = tid >> 6; ty < CF_TH; ty += 4) {
        const int y = oy + ty;
        if (x < w && y < h) resp[(size_t)y * w + x] = es[ty + 1][tx + 1];
    }
}

template <int B, int G>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) k_corner_response_block(const uint8_t *__restrict__ src, size_t pitch, int w, int h, float *__restrict__ resp,
                                                               int *__restrict__ max_bits, int vec_ok, int harris, float kf) {
    using T = BlockTile<B, G>;
    __shared__ __attribute__((aligned(16))) uint8_t tile[T::SH][T::SW];
    __shared__ __attribute__((aligned(16))) float prod[3][T::PH][T::PW];
    __shared__ int bmax;
    if (tile_interior<T>(blockIdx.x * CF_TW, blockIdx.y * CF_TH, w, h, vec_ok))
        cb_dense_tile<B, G, true>(tile, prod, bmax, src, (uint32_t)pitch, w, h, resp, max_bits, true, harris != 0, kf);
    else
        cb_dense_tile<B, G, false>(tile, prod, bmax, src, (uint32_t)pitch, w, h, resp, max_bits, vec_ok != 0, harris != 0, kf);
}

namespace {
// one entry per pair of block and gradient size; naming the kernels here is what instantiates them
struct CornerBlockKernels {
    int block, gradient;
    void (*fused)(const uint8_t *, size_t, int, int, double, unsigned int *, unsigned long long *, unsigned int *, float *, int, const uint8_t *, size_t, int, int, float);
    void (*dense)(const uint8_t *, size_t, int, int, float *, int *, int, int, float);
};
template <int B, int G>
constexpr CornerBlockKernels cb_kernels{B, G, k_corners_fused_block<B, G>, k_corner_response_block<B, G>};
constexpr CornerBlockKernels CB_KERNELS[] = {cb_kernels<5, 3>, cb_kernels<7, 3>, cb_kernels<3, 5>, cb_kernels<5, 5>, cb_kernels<7, 5>,
                                             cb_kernels<3, 7>, cb_kernels<5, 7>, cb_kernels<7, 7>};

const CornerBlockKernels *kernels_for(int block, int gradient) {
    for (const CornerBlockKernels &k : CB_KERNELS)
        if (k.block == block && k.gradient == gradient) return &k;
    return nullptr;
}
}  // namespace

bool corner_block_offered(int block) { return block == 3 || kernels_for(block, 3) != nullptr; }
bool corner_gradient_offered(int gradient) { return gradient == 3 || kernels_for(3, gradient) != nullptr; }

// the first kernel of launch_corners_fused for a spec whose (block, gradient) is not (3, 3): same grid, same scratch, same words
vstab_status launch_corners_fused_block(const uint8_t *src, size_t pitch, int w, int h, double quality, unsigned int *max_key, unsigned long long *slots,
                                        unsigned int *tile_counts, float *spill, dim3 grid, hipStream_t s, const DetectSpec &spec, int vec_ok, int mvec_ok) {
    const CornerBlockKernels *k = kernels_for(spec.block, spec.gradient);
    if (!k) return fail(VSTAB_ERR_INVALID, "launch_corners_fused: no kernel for this block and gradient size");
    hipLaunchKernelGGL(k->fused, grid, dim3(256), 0, s, src, pitch, w, h, quality, max_key, slots, tile_counts, spill, vec_ok, spec.mask, spec.mask_pitch, mvec_ok,
                       (int)spec.harris, spec.kf);
    VSTAB_HIP_TRY(hipGetLastError());
    return VSTAB_OK;
}

// launch_corner_response's kernel for a (block, gradient) other than (3, 3) (max_bits is initialised there)
vstab_status launch_corner_response_block(const uint8_t *src, size_t pitch, int w, int h, int block, bool harris, float kf, float *resp, int *max_bits, hipStream_t s,
                                          int gradient) {
    const CornerBlockKernels *k = kernels_for(block, gradient);
    if (!k) return fail(VSTAB_ERR_INVALID, "launch_corner_response: no kernel for this block and gradient size");
    const int vec_ok = reinterpret_cast<uintptr_t>(src) % 4 == 0 && pitch % 4 == 0;
    hipLaunchKernelGGL(k->dense, dim3(div_up(w, CF_TW), div_up(h, CF_TH)), dim3(256), 0, s, src, pitch, w, h, resp, max_bits, vec_ok, (int)harris, kf);
    VSTAB_HIP_TRY(hipGetLastError());
    return VSTAB_OK;
}

// this unit's code object (vstab_preload_kernels)
vstab_status preload_corner_block_kernels() {
    hipFuncAttributes at;
    VSTAB_HIP_TRY(hipFuncGetAttributes(&at, reinterpret_cast<const void *>(CB_KERNELS[0].fused)));
    return VSTAB_OK;
}

}  // namespace vstab
