// vstab_corners_block.hpp -- the corner response over a B x B block (vstab.h, "Corner block size"; goodFeaturesToTrack's blockSize), as a
// TEXT: vstab_corners_block.hip includes it once per block size with VSTAB_CB_B defined (5, 7), and every inclusion yields, in a namespace
// of its own (cb5, cb7), one one-pass detector kernel k_corners_fused_block and one dense-map kernel k_corner_response_block.  The mask
// pointer (NULL: none) and the response (minimum eigenvalue or Harris) are workgroup-uniform kernel arguments.  Block 3 is not built from
// this text: k_corners_fused and its siblings (vstab_corners_fused.hip) and k_min_eig / k_corner_harris (vstab_corners.hip) stay as they are.
//
// Both kernels work on the tile of the one-pass detector: CF_TW x CF_TH = 64 x 31 output pixels, the response on the 66 x 33 pixels around
// them.  What follows from B, r = (B - 1) / 2:
//   response  66 x 33, image (oy - 1 .., ox - 1 ..)
//   products  (66 + B - 1) x (33 + B - 1), image (oy - 1 - r .., ox - 1 - r ..): 70 x 37 and 72 x 39
//   source    one ring more, from a dword-aligned column: 72 x 39 bytes from (oy - 4, ox - 4) and 80 x 41 bytes from (oy - 5, ox - 8)
// Phases (256 threads, a barrier between any two):
//   load      the source bytes under REFLECT_101 -> LDS, dwords
//   prod      the Sobel pair of k_min_eig (same operation order, scale 1 / (4 B 255)) and the float products dx dx, dx dy, dy dy, each
//             formed once: a thread owns 2 columns x 6 rows (8 source rows; the last strip of rows overlaps the one before it instead of
//             testing bounds -- two threads then store the same floats).  The derivative at a position mirrored across the image border
//             has the sign of the mirrored axis flipped once per fold: dx dy is flipped where the folds in x and in y differ in parity
//             (an image narrower than r + 2 folds more than once)
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
// and then, in k_corners_fused_block, what cf_tile does behind its eigenvalues (tile maximum, lower bound of the threshold, 3 x 3 maximum
// test, keys or a dense spill), byte for byte in CornersFusedScratch's layout, so that k_filter_keys and the host serve every block size.
// A tile whose source box lies inside an image of dword-aligned rows takes a path without reflection arithmetic, sign flips and bounds
// tests (cb_interior, one workgroup-uniform test).
#ifndef VSTAB_CB_B
#error "define VSTAB_CB_B (5 or 7) before including vstab_corners_block.hpp"
#endif
#define VSTAB_CB_CAT_(a, b) a##b
#define VSTAB_CB_CAT(a, b) VSTAB_CB_CAT_(a, b)

namespace vstab {
namespace VSTAB_CB_CAT(cb, VSTAB_CB_B) {

constexpr int B = VSTAB_CB_B, R = (B - 1) / 2;
static_assert(B == 5 || B == 7, "block sizes built from this text");
constexpr int EW = CF_TW + 2, EH = CF_TH + 2;            // responses: 66 x 33
constexpr int PW = EW + B - 1, PH = EH + B - 1;          // products
constexpr int SY0 = R + 2, SX0 = (R + 2 + 3) & ~3;       // the source tile starts at image (oy - SY0, ox - SX0)
constexpr int SW = (SX0 + CF_TW + R + 2 + 3) & ~3, SH = PH + 2;
constexpr int PX = SX0 - 1 - R;                           // product (pr, pq) <-> tile[pr + 1][pq + PX]
constexpr int LOADS = (SH * (SW / 4) + 255) / 256;
constexpr int PR_ROWS = 6, PR_CG = PW / 2, PR_RS = (PH + PR_ROWS - 1) / PR_ROWS;  // prod: column groups of 2, row strips of 6
constexpr int BX_NC = 11, BX_CG = EW / BX_NC, BX_RS = EH;  // box: column groups of 11, one row each
static_assert(PW % 2 == 0 && PR_CG * PR_RS <= 256 && PH >= PR_ROWS && PH - PR_ROWS + (PR_ROWS + 1) < SH, "prod ownership covers the region, its source rows lie in the tile");
static_assert(PX >= 1 && PW - 1 + PX + 1 < SW, "every product's source columns lie in the tile");
static_assert(BX_CG * BX_NC == EW && BX_CG * BX_RS <= 256, "box ownership covers the region");
static_assert(SX0 % 4 == 0 && SW % 4 == 0 && SX0 >= R + 2 && SW - SX0 >= CF_TW + R + 2, "the source tile is dword aligned and holds the ring");

// whether BORDER_REFLECT_101 folds position i of an axis of n pixels an odd number of times (the sign of a derivative taken there)
__device__ __forceinline__ uint32_t fold_parity(int i, int n) {
    if (n == 1) return 0;
    uint32_t p = 0;
    while (i < 0 || i >= n) i = i < 0 ? -i : 2 * n - 2 - i, p ^= 1u;
    return p;
}

// the tile's source box lies inside the image, and its rows are dword aligned
__device__ __forceinline__ bool cb_interior(int ox, int oy, int w, int h, int vec_ok) {
    return vec_ok && ox >= SX0 && ox - SX0 + SW <= w && oy >= SY0 && oy - SY0 + SH <= h;
}

// load: dword e of the source tile <-> row e / (SW / 4), bytes 4 (e % (SW / 4)) ..
template <bool INTERIOR>
__device__ __forceinline__ void cb_load(uint32_t (&v)[LOADS], const uint8_t *__restrict__ src, uint32_t pitch, int w, int h, int ox, int oy, bool vec_ok, int tid) {
#pragma unroll
    for (int k = 0; k < LOADS; k++) {
        const int e = tid + 256 * k;
        const int ry = e / (SW / 4), rd = e - ry * (SW / 4);
        v[k] = 0;
        if (e >= SH * (SW / 4)) continue;
        if (INTERIOR) v[k] = *reinterpret_cast<const uint32_t *>(src + ((uint32_t)(oy - SY0 + ry) * pitch + (uint32_t)(ox - SX0 + 4 * rd)));
        else v[k] = load4_reflect(src, pitch, w, h, ox - SX0 + 4 * rd, oy - SY0 + ry, vec_ok);
    }
}
__device__ __forceinline__ void cb_store(uint8_t (&tile)[SH][SW], const uint32_t (&v)[LOADS], int tid) {
#pragma unroll
    for (int k = 0; k < LOADS; k++)
        if (tid + 256 * k < SH * (SW / 4)) reinterpret_cast<uint32_t *>(&tile[0][0])[tid + 256 * k] = v[k];
}
// The mask bytes of the tile in the layout of the source tile; nothing is mirrored: a byte outside the image is never read and counts as
// zero.  vec_ok: the MASK's base and pitch are 4-byte aligned.
template <bool INTERIOR>
__device__ __forceinline__ void cb_load_mask(uint32_t (&v)[LOADS], const uint8_t *__restrict__ mask, uint32_t pitch, int w, int h, int ox, int oy, bool vec_ok, int tid) {
#pragma unroll
    for (int k = 0; k < LOADS; k++) {
        const int e = tid + 256 * k;
        const int ry = e / (SW / 4), rd = e - ry * (SW / 4);
        v[k] = 0;
        if (e >= SH * (SW / 4)) continue;
        const int gx = ox - SX0 + 4 * rd, gy = oy - SY0 + ry;
        if (!INTERIOR && (gy < 0 || gy >= h)) continue;
        const uint8_t *row = mask + (uint32_t)gy * pitch;
        if (vec_ok && (INTERIOR || (gx >= 0 && gx + 4 <= w))) {
            v[k] = *reinterpret_cast<const uint32_t *>(row + gx);
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++)
                if (INTERIOR || (gx + i >= 0 && gx + i < w)) v[k] |= (uint32_t)row[gx + i] << (8 * i);
        }
    }
}
// whether one of the thread's mask dwords holds a non-zero byte of the 66 x 33 pixels the tile takes its maximum over: rows SY0 - 1 ..
// SY0 + 31 and bytes SX0 - 1 .. SX0 + 64 of the tile
__device__ __forceinline__ bool cb_mask_any(const uint32_t (&v)[LOADS], int tid) {
    bool any = false;
#pragma unroll
    for (int k = 0; k < LOADS; k++) {
        const int e = tid + 256 * k;
        const int ry = e / (SW / 4), rd = e - ry * (SW / 4);
        uint32_t sel = 0;
#pragma unroll
        for (int i = 0; i < 4; i++)
            if (4 * rd + i >= SX0 - 1 && 4 * rd + i <= SX0 + CF_TW) sel |= 0xffu << (8 * i);
        any = any || (ry >= SY0 - 1 && ry <= SY0 + CF_TH && (v[k] & sel) != 0);  // (a dword past the tile is zero: cb_load_mask)
    }
    return any;
}

// prod: a thread owns product columns 2 cg, 2 cg + 1 and rows r0 .. r0 + 5, r0 = min(6 rs, PH - 6)
template <bool INTERIOR>
__device__ __forceinline__ void cb_products(const uint8_t (&tile)[SH][SW], float (&prod)[3][PH][PW], int ox, int oy, int w, int h, int tid) {
    if (tid >= PR_CG * PR_RS) return;
    const float scale = (float)(1.0 / (4.0 * B * 255.0));
    const float k0 = 2.0f * scale, k1 = scale;
    const int rs = tid / PR_CG, cg = tid - rs * PR_CG;
    const int r0 = min(PR_ROWS * rs, PH - PR_ROWS), q0 = 2 * cg;
    uint32_t flip_x[2];  // the sign bit where the column is folded an odd number of times
#pragma unroll
    for (int i = 0; i < 2; i++) flip_x[i] = INTERIOR ? 0u : fold_parity(ox - 1 - R + q0 + i, w) << 31;
    float D[PR_ROWS + 2][2], S[PR_ROWS + 2][2];
#pragma unroll
    for (int j = 0; j < PR_ROWS + 2; j++) {
        const uint8_t *row = &tile[r0 + j][q0 + PX - 1];  // columns q0 - 1 .. q0 + 2 of the product grid
        const float f[4] = {(float)row[0], (float)row[1], (float)row[2], (float)row[3]};
#pragma unroll
        for (int i = 0; i < 2; i++) {
            D[j][i] = f[i + 2] - f[i];
            S[j][i] = f[i + 1] * k0 + (f[i] + f[i + 2]) * k1;
        }
    }
#pragma unroll
    for (int r = 0; r < PR_ROWS; r++) {
        const uint32_t flip_y = INTERIOR ? 0u : fold_parity(oy - 1 - R + r0 + r, h) << 31;
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const float dx = (D[r][i] + D[r + 2][i]) * k1 + D[r + 1][i] * k0;
            const float dy = S[r + 2][i] - S[r][i];
            prod[0][r0 + r][q0 + i] = dx * dx;
            prod[1][r0 + r][q0 + i] = INTERIOR ? dx * dy : __uint_as_float(__float_as_uint(dx * dy) ^ flip_x[i] ^ flip_y);
            prod[2][r0 + r][q0 + i] = dy * dy;
        }
    }
}

// box: the sums of one quantity for response row e0, columns x0 .. x0 + 10 (products: rows e0 .., columns x0 ..), in the defined order --
// column sums top to bottom, then left to right, in double; one rounding to float
__device__ __forceinline__ void cb_box(const float (*pl)[PW], int e0, int x0, float (&out)[BX_NC]) {
    constexpr int NCOL = BX_NC + B - 1;
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
    for (int i = 0; i < BX_NC; i++) {
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
template <bool INTERIOR>
__device__ __forceinline__ int cb_responses(float (&prod)[3][PH][PW], int ox, int oy, int w, int h, int tid, const uint8_t (*mtile)[SW], bool masked, bool harris,
                                            float kf) {
    // (the copies run in the wave of their original, in lockstep with it: none reads back a sum the original has replaced by its response)
    static_assert((BX_CG * BX_RS - 1) / 64 == 255 / 64, "the threads without a block share a wave with the thread they copy");
    const int t = min(tid, BX_CG * BX_RS - 1);
    const int e0 = t / BX_CG, x0 = BX_NC * (t - e0 * BX_CG);
#pragma unroll 1
    for (int q = 0; q < 3; q++) {
        float sum[BX_NC];
        cb_box(prod[q], e0, x0, sum);
        __syncthreads();  // every product of this plane has been read
#pragma unroll
        for (int i = 0; i < BX_NC; i++) prod[q][e0][x0 + i] = sum[i];
    }
    // (what a thread reads back below it wrote itself)
    int best = INT_MIN;
#pragma unroll
    for (int i = 0; i < BX_NC; i++) {
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
            if (mtile[e0 + SY0 - 1][x0 + i + SX0 - 1] != 0) best = max(best, __float_as_int(ev));
        } else if (INTERIOR || (gx >= 0 && gx < w && gy >= 0 && gy < h)) best = max(best, __float_as_int(ev));
    }
    return best;
}

// the maximum of `best` over the wave in its lane 63 (DPP, as cf_tile)
__device__ __forceinline__ int cb_wave_max(int best) {
    best = max(best, __builtin_amdgcn_update_dpp(INT_MIN, best, 0x111, 0xf, 0xf, false));
    best = max(best, __builtin_amdgcn_update_dpp(INT_MIN, best, 0x112, 0xf, 0xf, false));
    best = max(best, __builtin_amdgcn_update_dpp(INT_MIN, best, 0x114, 0xf, 0xf, false));
    best = max(best, __builtin_amdgcn_update_dpp(INT_MIN, best, 0x118, 0xf, 0xf, false));
    best = max(best, __builtin_amdgcn_update_dpp(INT_MIN, best, 0x142, 0xa, 0xf, false));
    best = max(best, __builtin_amdgcn_update_dpp(INT_MIN, best, 0x143, 0xc, 0xf, false));
    return best;
}

// cf_nonmax over this text's tile: threshold + 3 x 3 maximum test, lane = column, a wave walks its 8 rows (the last wave 7).  DENSE =
// false: survivors are appended to the tile's slots (*bcount counts all of them, also those past the last slot); DENSE = true: every pixel
// of the tile is written, the response for a survivor and -inf otherwise.  masked: a survivor also has a non-zero mask byte (pixel (ty,
// tx) of the tile <-> mtile[ty + SY0][tx + SX0]); its neighbours compete in the maximum whatever their mask bytes say.
template <bool DENSE, bool INTERIOR>
__device__ __forceinline__ void cb_nonmax(const float (&es)[PH][PW], int tid, int ox, int oy, int w, int h, float thr_lb, unsigned long long *__restrict__ my_slots,
                                          unsigned int *bcount, float *__restrict__ dense, const uint8_t (*mtile)[SW], bool masked) {
    const int tx = tid & 63, r0 = __builtin_amdgcn_readfirstlane(tid >> 6) * 8;
    const int x = ox + tx;
    const bool x_in = INTERIOR || (x >= 1 && x < w - 1);
    float rm0 = fmaxf(fmaxf(es[r0][tx], es[r0][tx + 1]), es[r0][tx + 2]);
    float c1 = es[r0 + 1][tx + 1];
    float rm1 = fmaxf(fmaxf(es[r0 + 1][tx], c1), es[r0 + 1][tx + 2]);
    float v[8];
    bool cand[8];
    unsigned long long ballot[8];
    unsigned int total = 0;
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const int ty = r0 + r;
        const bool row = r < 7 || ty < CF_TH;  // false only for the last wave's eighth row
        const int below = r < 7 ? ty + 2 : min(ty + 2, EH - 1);
        const float c2 = es[below][tx + 1];
        const float rm2 = fmaxf(fmaxf(es[below][tx], c2), es[below][tx + 2]);
        const float m = fmaxf(fmaxf(rm0, rm1), rm2);
        const int y = oy + ty;
        cand[r] = row && x_in && (INTERIOR || (y >= 1 && y < h - 1)) && c1 > thr_lb && c1 == m;
        if (masked) cand[r] = cand[r] && mtile[ty + SY0][tx + SX0] != 0;  // (ty + SY0 < SH also for the last wave's eighth row)
        if (DENSE) {
            if (row) dense[ty * CF_TW + tx] = cand[r] ? c1 : -__builtin_inff();
        } else {
            v[r] = c1;
            ballot[r] = __builtin_amdgcn_ballot_w64(cand[r]);
            total += (unsigned int)__popcll(ballot[r]);
        }
        rm0 = rm1, rm1 = rm2, c1 = c2;
    }
    if (!DENSE && total) {
        unsigned int base = 0;
        if (tx == 0) base = atomicAdd(bcount, total);  // LDS
        base = __builtin_amdgcn_readfirstlane(base);
#pragma unroll
        for (int r = 0; r < 8; r++) {
            if (!ballot[r]) continue;
            const unsigned int slot = base + __builtin_amdgcn_mbcnt_hi((uint32_t)(ballot[r] >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ballot[r], 0));
            if (cand[r] && slot < CF_SLOTS) my_slots[slot] = ((unsigned long long)__float_as_uint(v[r]) << 32) | (unsigned int)((oy + r0 + r) * w + x);
            base += (unsigned int)__popcll(ballot[r]);
        }
    }
}

// the shared front of both kernels: source -> products -> responses in prod[0] (entry (ey, ex) of the 66 x 33); returns the thread's maximum.
// Under a mask the mask bytes (mv, loaded by the caller) take the source tile's place in LDS behind the products.
template <bool INTERIOR>
__device__ __forceinline__ int cb_response_tile(uint8_t (&tile)[SH][SW], float (&prod)[3][PH][PW], const uint32_t (&v)[LOADS], const uint32_t (&mv)[LOADS], int ox, int oy,
                                                int w, int h, bool masked, bool harris, float kf) {
    const int tid = threadIdx.x;
    cb_store(tile, v, tid);
    __syncthreads();
    cb_products<INTERIOR>(tile, prod, ox, oy, w, h, tid);
    __syncthreads();
    if (masked) cb_store(tile, mv, tid);  // the source bytes are dead; cb_responses' barriers stand between this and the first reader
    return cb_responses<INTERIOR>(prod, ox, oy, w, h, tid, tile, masked, harris, kf);
}

// cf_tile for block B.  mask (NULL: none): a tile without a non-zero mask byte among the in-image pixels of its 66 x 33 responses writes a
// count of 0 and returns before it loads the source -- one value for the workgroup, so every barrier below is reached by all of its
// threads or by none; the tile maximum runs over the responses with a non-zero mask byte; a survivor has a non-zero mask byte.
// harris: a tile without a response >= +0 has a negative int-bit maximum and filters with -inf; the host reads the sign of the frame's.
template <bool INTERIOR>
__device__ __forceinline__ void cb_tile(uint8_t (&tile)[SH][SW], float (&prod)[3][PH][PW], int &bmax, unsigned int &bcount, unsigned int &bseen,
                                        const uint8_t *__restrict__ src, uint32_t pitch, int w, int h, double quality, unsigned int *__restrict__ max_key,
                                        unsigned long long *__restrict__ slots, unsigned int *__restrict__ tile_counts, float *__restrict__ spill, bool vec_ok,
                                        const uint8_t *__restrict__ mask, uint32_t mpitch, bool mvec_ok, bool harris, float kf) {
    const float(&es)[PH][PW] = prod[0];
    const int tid = threadIdx.x;
    const int ox = blockIdx.x * CF_TW, oy = blockIdx.y * CF_TH;
    const int tile_idx = blockIdx.y * gridDim.x + blockIdx.x;
    const bool masked = mask != nullptr;
    uint32_t mv[LOADS] = {};
    if (masked) {
        cb_load_mask<INTERIOR>(mv, mask, mpitch, w, h, ox, oy, mvec_ok, tid);
        // one flag per wave in LDS nobody uses yet (prod is first written behind the barriers of cb_response_tile), one barrier, the same
        // answer in every thread
        uint32_t *flags = reinterpret_cast<uint32_t *>(&prod[2][0][0]);
        const bool mine = __builtin_amdgcn_ballot_w64(cb_mask_any(mv, tid)) != 0;
        if ((tid & 63) == 0) flags[tid >> 6] = mine;
        __syncthreads();
        if ((flags[0] | flags[1] | flags[2] | flags[3]) == 0) {
            if (tid == 0) tile_counts[tile_idx] = 0;
            return;
        }
    }
    uint32_t v[LOADS];
    cb_load<INTERIOR>(v, src, pitch, w, h, ox, oy, vec_ok, tid);
    if (tid == 0) bmax = INT_MIN, bcount = 0;
    // the frame maximum published so far (biased bits), a lower bound of the final one: ONE lane asks, device scope, behind the tile's
    // loads, and nothing needs the answer before the responses are done (cf_tile has the reasons)
    unsigned int seen = 0;
    if (tid == 255) seen = __hip_atomic_load(max_key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    int best = cb_response_tile<INTERIOR>(tile, prod, v, mv, ox, oy, w, h, masked, harris, kf);
    best = cb_wave_max(best);
    if ((tid & 63) == 63) atomicMax(&bmax, best);
    if (tid == 255) bseen = seen;
    __syncthreads();
    const int tile_max = bmax;
    seen = bseen;
    // only a tile that raises the maximum it saw publishes
    if (tid == 0 && ((unsigned int)tile_max ^ 0x80000000u) > seen) atomicMax(max_key, (unsigned int)tile_max ^ 0x80000000u);
    // lower bound of the frame threshold; only meaningful for a non-negative maximum (float order == int order)
    const int lb_bits = max(tile_max, (int)(seen ^ 0x80000000u));
    const float thr_lb = lb_bits >= 0 ? (float)((double)__int_as_float(lb_bits) * quality) : -__builtin_inff();
    cb_nonmax<false, INTERIOR>(es, tid, ox, oy, w, h, thr_lb, slots + (size_t)tile_idx * CF_SLOTS, &bcount, nullptr, tile, masked);
    __syncthreads();
    const unsigned int n = bcount;
    if (tid == 0) tile_counts[tile_idx] = n;
    // more survivors than slots: a dense 64 x 31 map instead (-inf = not a survivor), which k_filter_keys scans with the final threshold
    if (n > CF_SLOTS) cb_nonmax<true, INTERIOR>(es, tid, ox, oy, w, h, thr_lb, nullptr, nullptr, spill + (size_t)tile_idx * (CF_TW * CF_TH), tile, masked);
}

// k_corners_fused_block -- k_corners_fused and its three siblings for block B in one kernel: mask (NULL: none) and harris are the same for
// every workgroup of a launch.
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) k_corners_fused_block(const uint8_t *__restrict__ src, size_t pitch, int w, int h, double quality, unsigned int *__restrict__ max_key,
                                                             unsigned long long *__restrict__ slots, unsigned int *__restrict__ tile_counts, float *__restrict__ spill,
                                                             int vec_ok, const uint8_t *__restrict__ mask, size_t mpitch, int mvec_ok, int harris, float kf) {
    __shared__ __attribute__((aligned(16))) uint8_t tile[SH][SW];  // the source bytes; behind the products, the mask bytes
    __shared__ __attribute__((aligned(16))) float prod[3][PH][PW];  // dx dx, dx dy, dy dy; then their box sums, then the responses in place of dx dx
    __shared__ int bmax;
    __shared__ unsigned int bcount, bseen;
    if (cb_interior(blockIdx.x * CF_TW, blockIdx.y * CF_TH, w, h, vec_ok))
        cb_tile<true>(tile, prod, bmax, bcount, bseen, src, (uint32_t)pitch, w, h, quality, max_key, slots, tile_counts, spill, true, mask, (uint32_t)mpitch, mvec_ok != 0,
                      harris != 0, kf);
    else
        cb_tile<false>(tile, prod, bmax, bcount, bseen, src, (uint32_t)pitch, w, h, quality, max_key, slots, tile_counts, spill, vec_ok != 0, mask, (uint32_t)mpitch,
                       mvec_ok != 0, harris != 0, kf);
}

// k_corner_response_block -- cornerMinEigenVal(B, 3) or, harris, cornerHarris(B, 3, k) as a dense w x h map, and its int-bit maximum
// (*max_bits, initialised as launch_corner_response does): the front of the kernel above, then the tile's 64 x 31 responses to memory, a
// wave per 8 rows, a lane per column.
template <bool INTERIOR>
__device__ __forceinline__ void cb_dense_tile(uint8_t (&tile)[SH][SW], float (&prod)[3][PH][PW], int &bmax, const uint8_t *__restrict__ src, uint32_t pitch, int w, int h,
                                              float *__restrict__ resp, int *__restrict__ max_bits, bool vec_ok, bool harris, float kf) {
    const float(&es)[PH][PW] = prod[0];
    const int tid = threadIdx.x;
    const int ox = blockIdx.x * CF_TW, oy = blockIdx.y * CF_TH;
    uint32_t v[LOADS];
    const uint32_t mv[LOADS] = {};
    cb_load<INTERIOR>(v, src, pitch, w, h, ox, oy, vec_ok, tid);
    if (tid == 0) bmax = INT_MIN;
    int best = cb_response_tile<INTERIOR>(tile, prod, v, mv, ox, oy, w, h, false, harris, kf);
    best = cb_wave_max(best);
    if ((tid & 63) == 63) atomicMax(&bmax, best);
    __syncthreads();
    if (tid == 0) atomicMax(max_bits, bmax);
    const int tx = tid & 63, x = ox + tx;
    for (int ty = tid >> 6; ty < CF_TH; ty += 4) {
        const int y = oy + ty;
        if (x < w && y < h) resp[(size_t)y * w + x] = es[ty + 1][tx + 1];
    }
}

__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) k_corner_response_block(const uint8_t *__restrict__ src, size_t pitch, int w, int h, float *__restrict__ resp,
                                                               int *__restrict__ max_bits, int vec_ok, int harris, float kf) {
    __shared__ __attribute__((aligned(16))) uint8_t tile[SH][SW];
    __shared__ __attribute__((aligned(16))) float prod[3][PH][PW];
    __shared__ int bmax;
    if (cb_interior(blockIdx.x * CF_TW, blockIdx.y * CF_TH, w, h, vec_ok))
        cb_dense_tile<true>(tile, prod, bmax, src, (uint32_t)pitch, w, h, resp, max_bits, true, harris != 0, kf);
    else
        cb_dense_tile<false>(tile, prod, bmax, src, (uint32_t)pitch, w, h, resp, max_bits, vec_ok != 0, harris != 0, kf);
}

}  // namespace cb<B>
}  // namespace vstab
#undef VSTAB_CB_CAT
#undef VSTAB_CB_CAT_
