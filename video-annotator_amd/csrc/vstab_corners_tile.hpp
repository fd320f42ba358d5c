// vstab_corners_tile.hpp -- what the one-pass corner detector does with a tile whatever the block size of its response: the geometry of the
// source tile, its load (image and mask), the masked tile's early return, and everything behind the responses (tile maximum, lower bound of
// the threshold, 3 x 3 maximum test, keys or a dense spill).  k_corners_fused and its siblings (vstab_corners_fused.hip, block 3 with
// gradient 3) and k_corners_fused_block / k_corner_response_block (vstab_corners_block.hip, every other pair of block and gradient size)
// are built from it; what they keep for themselves is how the responses of a tile are formed.  The wave maximum also serves
// vstab_corners.hip.
//
// Every tile_ function is a template over the geometry G of the source tile (a type; the gradient size is SourceTile's second argument)
// and over a TAG that changes nothing in the function: it
// gives the kernel that names it instantiations of its own.  An instantiation that two kernels of a unit inlined would be cloned where a
// single kernel has it moved into its only caller, and the optimiser's choices behind that differ: with a tag per kernel the instructions of
// k_corners_fused stay exactly what they were before it had siblings (k_corners_fused_masked, then the Harris pair; CfTag in
// vstab_corners_fused.hip).  The block kernels take their mask and response as arguments and need none.
#pragma once
#include <climits>
#include <type_traits>

#include "vstab_track.hpp"
#include "vstab_track_device.hpp"

namespace vstab {

// the maximum of `best` over each row of 16 lanes in the row's last lane (DPP), and over the wave in lane 63
__device__ __forceinline__ int row_max_i32(int best) {
    best = max(best, __builtin_amdgcn_update_dpp(INT_MIN, best, 0x111, 0xf, 0xf, false));
    best = max(best, __builtin_amdgcn_update_dpp(INT_MIN, best, 0x112, 0xf, 0xf, false));
    best = max(best, __builtin_amdgcn_update_dpp(INT_MIN, best, 0x114, 0xf, 0xf, false));
    return max(best, __builtin_amdgcn_update_dpp(INT_MIN, best, 0x118, 0xf, 0xf, false));
}
__device__ __forceinline__ int wave_max_i32(int best) {
    best = row_max_i32(best);
    best = max(best, __builtin_amdgcn_update_dpp(INT_MIN, best, 0x142, 0xa, 0xf, false));
    return max(best, __builtin_amdgcn_update_dpp(INT_MIN, best, 0x143, 0xc, 0xf, false));
}

// The source tile of a CF_TW x CF_TH = 64 x 31 tile whose responses sum a B x B block of products of a G x G derivative, r = (B - 1) / 2 and
// g = (G - 1) / 2: the 66 x 33 responses around the tile need products r further out and those a ring of g source pixels more, from a
// dword-aligned column: SW x SH bytes from image (oy - SY0, ox - SX0).  (B, G) -> SW x SH from (oy - SY0, ox - SX0):
//   (3, 3) 72 x 37 (3, 4)   (3, 5) 72 x 39 (4, 4)   (3, 7) 80 x 41 (5, 8)
//   (5, 3) 72 x 39 (4, 4)   (5, 5) 80 x 41 (5, 8)   (5, 7) 80 x 43 (6, 8)
//   (7, 3) 80 x 41 (5, 8)   (7, 5) 80 x 43 (6, 8)   (7, 7) 80 x 45 (7, 8)
// A thread holds LOADS dwords of it, dword e <-> row row(e), bytes 4 (e - row(e) SW / 4) ..; sel(rd) selects, of dword rd of a row, the
// bytes that belong to the 66 columns of the responses: bytes SX0 - 1 .. SX0 + 64 of the row.
template <int B, int G = 3>
struct SourceTile {
    static constexpr int R = (B - 1) / 2, GR = (G - 1) / 2;
    static constexpr int SY0 = R + 1 + GR, SX0 = (R + 1 + GR + 3) & ~3;
    static constexpr int SW = (SX0 + CF_TW + R + 1 + GR + 3) & ~3, SH = CF_TH + 2 + B - 1 + 2 * GR;
    static constexpr int LOADS = (SH * (SW / 4) + 255) / 256;
    static_assert(SX0 % 4 == 0 && SW % 4 == 0 && SX0 >= R + 1 + GR && SW - SX0 >= CF_TW + R + 1 + GR, "the source tile is dword aligned and holds the ring");
    static __device__ __forceinline__ int row(int e) { return e / (SW / 4); }
    static __device__ __forceinline__ uint32_t sel(int rd) {
        uint32_t s = 0;
#pragma unroll
        for (int i = 0; i < 4; i++)
            if (4 * rd + i >= SX0 - 1 && 4 * rd + i <= SX0 + CF_TW) s |= 0xffu << (8 * i);
        return s;
    }
};
static_assert(SourceTile<5>::SW == 72 && SourceTile<5>::SH == 39 && SourceTile<5>::SY0 == 4 && SourceTile<5>::SX0 == 4, "gradient 3: the tile block 5 has always had");
static_assert(SourceTile<7>::SW == 80 && SourceTile<7>::SH == 41 && SourceTile<7>::SY0 == 5 && SourceTile<7>::SX0 == 8, "gradient 3: the tile block 7 has always had");
static_assert(SourceTile<7, 7>::SW == 80 && SourceTile<7, 7>::SH == 45, "the largest tile");
// Block 3's, as k_corners_fused has always had it: 72 x 38 bytes from (oy - 3, ox - 4), one row more than the formula (37 are used); the
// row of a dword as one 24-bit multiply and a shift (div_magic_ok); and of a row's 18 dwords the last byte of the first, the first byte of
// the last, every byte of those between, said in that form: the generic loop costs both masked block-3 kernels 60 to 160 instructions.
struct SourceTile3 {
    static constexpr int SY0 = 3, SX0 = 4, SW = 72, SH = 38;
    static constexpr int LOADS = (SH * (SW / 4) + 255) / 256;
    static_assert(SY0 == SourceTile<3>::SY0 && SX0 == SourceTile<3>::SX0 && SW == SourceTile<3>::SW && SH >= SourceTile<3>::SH, "block 3's tile is the formulas' tile");
    static_assert(div_magic_ok(SW / 4, 3641, SH * (SW / 4) + 256), "division constant");
    static __device__ __forceinline__ int row(int e) { return __mul24(e, 3641) >> 16; }
    static __device__ __forceinline__ uint32_t sel(int rd) { return rd == 0 ? 0xff000000u : rd == SW / 4 - 1 ? 0x000000ffu : 0xffffffffu; }
};

// the tile's source bytes lie inside the image, and its rows are dword aligned: the path without reflection arithmetic, sign flips and bounds tests
template <class G, class TAG = void>
__device__ __forceinline__ bool tile_interior(int ox, int oy, int w, int h, int vec_ok) {
    return vec_ok && ox >= G::SX0 && ox - G::SX0 + G::SW <= w && oy >= G::SY0 && oy - G::SY0 + G::SH <= h;
}

// load: the source tile under REFLECT_101; a thread's loads are in flight together
template <class G, bool INTERIOR, class TAG = void>
__device__ __forceinline__ void tile_load(uint32_t (&v)[G::LOADS], const uint8_t *__restrict__ src, uint32_t pitch, int w, int h, int ox, int oy, bool vec_ok, int tid) {
#pragma unroll
    for (int k = 0; k < G::LOADS; k++) {
        const int e = tid + 256 * k;
        const int ry = G::row(e), rd = e - ry * (G::SW / 4);
        v[k] = 0;
        if (e >= G::SH * (G::SW / 4)) continue;
        if (INTERIOR) v[k] = *reinterpret_cast<const uint32_t *>(src + ((uint32_t)(oy - G::SY0 + ry) * pitch + (uint32_t)(ox - G::SX0 + 4 * rd)));
        else v[k] = load4_reflect(src, pitch, w, h, ox - G::SX0 + 4 * rd, oy - G::SY0 + ry, vec_ok);
    }
}
template <class G, class TAG = void>
__device__ __forceinline__ void tile_store(uint8_t (&tile)[G::SH][G::SW], const uint32_t (&v)[G::LOADS], int tid) {
#pragma unroll
    for (int k = 0; k < G::LOADS; k++)
        if (tid + 256 * k < G::SH * (G::SW / 4)) reinterpret_cast<uint32_t *>(&tile[0][0])[tid + 256 * k] = v[k];
}

// The mask bytes of the tile in the layout and with the addressing of tile_load: dwords where the mask's rows are dword aligned, bytes
// otherwise -- but nothing is mirrored: a byte outside the image is never read and counts as zero ("masked out").  INTERIOR says that
// the source tile lies inside the image (the mask has the image's size), vec_ok that the MASK's base and pitch are 4-byte aligned.
template <class G, bool INTERIOR, class TAG = void>
__device__ __forceinline__ void tile_load_mask(uint32_t (&v)[G::LOADS], const uint8_t *__restrict__ mask, uint32_t pitch, int w, int h, int ox, int oy, bool vec_ok, int tid) {
#pragma unroll
    for (int k = 0; k < G::LOADS; k++) {
        const int e = tid + 256 * k;
        const int ry = G::row(e), rd = e - ry * (G::SW / 4);
        v[k] = 0;
        if (e >= G::SH * (G::SW / 4)) continue;
        const int gx = ox - G::SX0 + 4 * rd, gy = oy - G::SY0 + ry;
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
// SY0 + 31 of the tile, and G::sel's bytes of them
template <class G, class TAG = void>
__device__ __forceinline__ bool tile_mask_any(const uint32_t (&v)[G::LOADS], int tid) {
    bool any = false;
#pragma unroll
    for (int k = 0; k < G::LOADS; k++) {
        const int e = tid + 256 * k;
        const int ry = G::row(e), rd = e - ry * (G::SW / 4);
        const uint32_t sel = G::sel(rd);
        any = any || (ry >= G::SY0 - 1 && ry <= G::SY0 + CF_TH && (v[k] & sel) != 0);  // (a dword past the tile is zero: tile_load_mask)
    }
    return any;
}
// The masked tile's early return: whether none of the tile's mask bytes (mv: tile_load_mask) under its 66 x 33 responses is non-zero.
// Such a tile writes a count of 0 and returns before it loads the source; it publishes no maximum and no key.  The answer is one value for
// the workgroup -- a flag per wave in `flags`, 4 dwords of LDS nobody uses yet, behind one barrier -- so every later barrier is reached by
// all of its threads or by none.
template <class G, class TAG = void>
__device__ __forceinline__ bool tile_masked_out(const uint32_t (&mv)[G::LOADS], uint32_t *flags, int tid) {
    const bool mine = __builtin_amdgcn_ballot_w64(tile_mask_any<G, TAG>(mv, tid)) != 0;
    if ((tid & 63) == 0) flags[tid >> 6] = mine;
    __syncthreads();
    return (flags[0] | flags[1] | flags[2] | flags[3]) == 0;
}

// threshold + 3x3 maximum test over the 66 x 33 responses in LDS (`es`, rows of any pitch): lane = column, a wave walks its 8 rows (the
// last wave 7) with a rolling row maximum.  DENSE = false: survivors are appended to the tile's slots, one LDS atomic per wave for the
// rows' survivors together (*bcount counts all of them, also those past the last slot); DENSE = true: every pixel of the tile is written,
// the response for a survivor and -inf otherwise.  INTERIOR: every pixel of the tile is an interior pixel of the image.
// masked (a bool, or a std::bool_constant where the kernel knows): a survivor also has a non-zero mask byte; `mtile` holds the tile's mask
// bytes in the layout of the source tile (pixel (ty, tx) of the tile <-> mtile[ty + SY0][tx + SX0]).  Its neighbours compete in the maximum
// whatever their mask bytes say.
template <class G, bool DENSE, bool INTERIOR, class TAG = void, class MASKED, int EROWS, int EP>
__device__ __forceinline__ void tile_nonmax(const float (&es)[EROWS][EP], int tid, int ox, int oy, int w, int h, float thr_lb, unsigned long long *__restrict__ my_slots,
                                            unsigned int *bcount, float *__restrict__ dense, const uint8_t (*mtile)[G::SW], MASKED masked) {
    const int tx = tid & 63, r0 = __builtin_amdgcn_readfirstlane(tid >> 6) * 8;  // the rows are the wave's: scalar
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
        const bool row = r < 7 || ty < CF_TH;            // scalar; false only for the last wave's eighth row
        const int below = r < 7 ? ty + 2 : min(ty + 2, CF_TH + 1);
        const float c2 = es[below][tx + 1];
        const float rm2 = fmaxf(fmaxf(es[below][tx], c2), es[below][tx + 2]);
        const float m = fmaxf(fmaxf(rm0, rm1), rm2);
        const int y = oy + ty;
        cand[r] = row && x_in && (INTERIOR || (y >= 1 && y < h - 1)) && c1 > thr_lb && c1 == m;
        if (masked) cand[r] = cand[r] && mtile[ty + G::SY0][tx + G::SX0] != 0;  // (ty + SY0 <= 31 + SY0 < SH also for the last wave's eighth row)
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

// The frame maximum published so far (biased bits), in thread 255 (0 elsewhere): a lower bound of the final one.  Device-scope load: the
// atomics of other XCDs do not pass through this XCD's L2.  Every workgroup reads this one address, and the memory side serves such reads
// one after the other: ONE lane asks -- in the last wave, which has no part in block 3's products, and behind the tile's loads, so that no
// wait for those waits for this -- and nothing needs the answer before the responses are done.
template <class TAG = void>
__device__ __forceinline__ unsigned int tile_seen(const unsigned int *__restrict__ max_key, int tid) {
    unsigned int seen = 0;
    if (tid == 255) seen = __hip_atomic_load(max_key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return seen;
}

// Everything behind the responses.  `best` is the thread's maximum over the responses that count (in the image; under a mask, with a
// non-zero mask byte) in the int-bit order of k_min_eig, `seen` what tile_seen returned, `es` the 66 x 33 responses, `mtile` and `masked`
// as in tile_nonmax; bmax and bcount are the tile's words of LDS, reset by thread 0 before the barrier that precedes the responses.  The
// threshold quality * max(frame) is not known until every tile is done, so the tile filters with a LOWER bound of it -- quality * max(own
// tile, frame maximum seen) -- and k_filter_keys applies the final threshold to the survivors.  A tile without a response >= +0 (Harris) has
// a negative int-bit maximum and filters with -inf; whether the FRAME's maximum is positive the host reads from its sign.
template <class G, bool INTERIOR, class TAG = void, class MASKED, int EROWS, int EP>
__device__ __forceinline__ void tile_select(int best, unsigned int seen, const float (&es)[EROWS][EP], const uint8_t (*mtile)[G::SW], MASKED masked, int &bmax,
                                            unsigned int &bcount, unsigned int &bseen, int w, int h, double quality, unsigned int *__restrict__ max_key,
                                            unsigned long long *__restrict__ slots, unsigned int *__restrict__ tile_counts, float *__restrict__ spill) {
    const int tid = threadIdx.x;
    const int ox = blockIdx.x * CF_TW, oy = blockIdx.y * CF_TH;
    best = wave_max_i32(best);
    if ((tid & 63) == 63) atomicMax(&bmax, best);
    if (tid == 255) bseen = seen;
    __syncthreads();
    const int tile_max = bmax;
    seen = bseen;
    // Every workgroup hitting one address costs ~11 ns apiece on this part (all XCDs meet at the memory side):
    // only a tile that raises the maximum it saw publishes.
    if (tid == 0 && ((unsigned int)tile_max ^ 0x80000000u) > seen) atomicMax(max_key, (unsigned int)tile_max ^ 0x80000000u);
    // lower bound of the frame threshold; only meaningful for a non-negative maximum (float order == int order)
    const int lb_bits = max(tile_max, (int)(seen ^ 0x80000000u));
    const float thr_lb = lb_bits >= 0 ? (float)((double)__int_as_float(lb_bits) * quality) : -__builtin_inff();
    const int tile_idx = blockIdx.y * gridDim.x + blockIdx.x;
    tile_nonmax<G, false, INTERIOR, TAG>(es, tid, ox, oy, w, h, thr_lb, slots + (size_t)tile_idx * CF_SLOTS, &bcount, nullptr, mtile, masked);
    __syncthreads();
    const unsigned int n = bcount;
    if (tid == 0) tile_counts[tile_idx] = n;
    // A tile with more survivors than slots (a response plateau: a smooth ramp, a periodic texture) leaves them as a
    // dense 64 x 31 map instead (-inf = not a survivor); k_filter_keys scans that with the final threshold.
    if (n > CF_SLOTS) tile_nonmax<G, true, INTERIOR, TAG>(es, tid, ox, oy, w, h, thr_lb, nullptr, nullptr, spill + (size_t)tile_idx * (CF_TW * CF_TH), mtile, masked);
}

}  // namespace vstab
