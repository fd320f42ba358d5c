// vstab_warp_p010_resample.hip -- INTER_CUBIC and INTER_LANCZOS4 with every border mode for the plane-wise 10-bit warp: P010 planes in
// and out, no colour conversion (vstab_warp_p010_planar_ex, vstab_set_resample10).  Definition (include/vstab.h, "Cubic and Lanczos
// resampling at 10 bits"; tests/warp10_def.py): the 8-bit definition on the ten significant bits -- sample = word >> 6, the map quantised to
// 1/32 pixel, the 4 x 4 / 8 x 8 footprint, the int16 weight tables of the 8-bit resamplers, each tap outside the plane the border value (64
// luma, 512 chroma; BORDER_CONSTANT) or read at its borderInterpolate position, (sum + 2^14) >> 15 clamped to 0..1023, word = value << 6.
// Chroma as VSTAB_OUT_NV12_PLANAR has it: at the even pixels of even rows, the map halved and quantised again, the border decided over the
// chroma plane's own size, U and V blended separately.
//
// The tile's phases, the box, the staging and the footprint rows are the resamplers' common ones (vstab_resample.hpp).  This unit holds the
// 16-bit sources, the 16-bit channel blends, the one tile of the 10-bit kernels and both weight tables (in its own code object).
// |sum| <= 96336 * 1023 + 2^14 < 2^27 (96336: the largest sum of |w| of a Lanczos entry; cubic 61952): int32 holds it.
#include "vstab_cubic.hpp"
#include "vstab_lanczos4.hpp"
#include "vstab_warp_host.hpp"

namespace vstab {

__device__ const CubicTable g_cubic10 = make_cubic_table();           // in the code object's read-only data: loaded with the kernels
__device__ const Lanczos4Table g_lanczos4_10 = make_lanczos4_table();

// ---------------------------------------------------------------------------------------------------------------------
// Sources: a position (X, Y) of a P010 plane as a dword of ten-bit samples -- luma: the sample; chroma: U | V << 16 -- read at its
// border-interpolated position, or the border value (CONSTANT) where it lies outside.  Addresses in 64 bits, as BorderBytes forms them.
// ---------------------------------------------------------------------------------------------------------------------
template <int BORDER>
struct BorderWords {  // one 16-bit sample per position
    const uint8_t *p;
    size_t pitch;
    int w, h;
    uint32_t border;  // CONSTANT: the ten-bit border value
    __device__ __forceinline__ uint32_t at(int X, int Y) const {  // X, Y inside
        return (uint32_t)*reinterpret_cast<const uint16_t *>(p + (size_t)Y * pitch + (size_t)X * 2) >> 6;
    }
    __device__ __forceinline__ uint32_t row_col(int X, int Y) const {  // X, Y already border-interpolated
        if constexpr (BORDER == VSTAB_BORDER_CONSTANT) {
            if ((unsigned)X < (unsigned)w && (unsigned)Y < (unsigned)h) return at(X, Y);
            return border;
        } else {
            return at(X, Y);
        }
    }
};
template <int BORDER>
struct BorderWordPairs {  // one (U, V) pair of 16-bit samples per position, 4-byte aligned
    const uint8_t *p;
    size_t pitch;
    int w, h;
    uint32_t border;  // CONSTANT: U | V << 16
    __device__ __forceinline__ uint32_t at(int X, int Y) const {  // X, Y inside
        return (*reinterpret_cast<const uint32_t *>(p + (size_t)Y * pitch + (size_t)X * 4) >> 6) & 0x03ff03ffu;
    }
    __device__ __forceinline__ uint32_t row_col(int X, int Y) const {  // X, Y already border-interpolated
        if constexpr (BORDER == VSTAB_BORDER_CONSTANT) {
            if ((unsigned)X < (unsigned)w && (unsigned)Y < (unsigned)h) return at(X, Y);
            return border;
        } else {
            return at(X, Y);
        }
    }
};

// ---------------------------------------------------------------------------------------------------------------------
// The 16-bit channel blends.  Ten-bit samples are int16 operands of v_dot2_i32_i16 as they stand: a horizontally adjacent luma pair is
// packed by v_lshl_or_b32, a pair of U or of V picked from the halves of two chroma dwords by v_perm_b32.
// ---------------------------------------------------------------------------------------------------------------------
typedef short short2v10 __attribute__((ext_vector_type(2)));
// channel CH of the taps lo (low half of the pair) and hi; CN 1: the taps are the samples themselves
template <int CN, int CH>
__device__ __forceinline__ short2v10 pair10(uint32_t lo, uint32_t hi) {
    if constexpr (CN == 1) return __builtin_bit_cast(short2v10, lo | (hi << 16));
    else return __builtin_bit_cast(short2v10, __builtin_amdgcn_perm(hi, lo, CH ? 0x07060302u : 0x05040100u));
}
__device__ __forceinline__ uint32_t clamp10(int v) { return (uint32_t)min(max(v, 0), 1023); }
// K taps of one footprint row against the row's K / 2 weight pairs
template <int CN, int CH, int K>
__device__ __forceinline__ int row10(int acc, const uint32_t (&t)[K], const uint32_t *w) {
#pragma unroll
    for (int c = 0; c < K / 2; c++) acc = __builtin_amdgcn_sdot2(pair10<CN, CH>(t[2 * c], t[2 * c + 1]), __builtin_bit_cast(short2v10, w[c]), acc, false);
    return acc;
}

struct Cubic10 {
    static constexpr int K = 4, LO = 1;
    // some tap of the footprint inside a w x h plane
    __device__ __forceinline__ static bool touches(const CubicTap &t, int w, int h) { return t.X + 2 >= 0 && t.X - 1 < w && t.Y + 2 >= 0 && t.Y - 1 < h; }
    // the channels 0 .. CN - 1 of the output, ten bits in each 16-bit half
    template <int CN, typename Rows>
    __device__ __forceinline__ static uint32_t blend(const Rows &rows, int f) {
        const uint4 *p = reinterpret_cast<const uint4 *>(g_cubic10.w) + 2 * f;
        const uint4 a = p[0], b = p[1];
        const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        int acc0 = 1 << 14, acc1 = 1 << 14;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            uint32_t v[4];
            rows(r, v);
            acc0 = row10<CN, 0>(acc0, v, w + 2 * r);
            if constexpr (CN > 1) acc1 = row10<CN, 1>(acc1, v, w + 2 * r);
        }
        uint32_t out = clamp10(acc0 >> 15);
        if constexpr (CN > 1) out |= clamp10(acc1 >> 15) << 16;
        return out;
    }
};

struct Lanczos4_10 {
    static constexpr int K = 8, LO = 3;
    __device__ __forceinline__ static bool touches(const CubicTap &t, int w, int h) { return t.X + 4 >= 0 && t.X - 3 < w && t.Y + 4 >= 0 && t.Y - 3 < h; }
    // row by row, the row's 8 weights in one 16-byte load
    template <int CN, typename Rows>
    __device__ __forceinline__ static uint32_t blend(const Rows &rows, int f) {
        int acc0 = 1 << 14, acc1 = 1 << 14;
#pragma unroll
        for (int r = 0; r < 8; r++) {
            uint32_t v[8];
            const uint4 q = reinterpret_cast<const uint4 *>(g_lanczos4_10.w)[8 * f + r];
            const uint32_t w[4] = {q.x, q.y, q.z, q.w};
            rows(r, v);
            acc0 = row10<CN, 0>(acc0, v, w);
            if constexpr (CN > 1) acc1 = row10<CN, 1>(acc1, v, w);
        }
        uint32_t out = clamp10(acc0 >> 15);
        if constexpr (CN > 1) out |= clamp10(acc1 >> 15) << 16;
        return out;
    }
};

// ---------------------------------------------------------------------------------------------------------------------
// The warp of one tile: resample_tile_rs's phases (vstab_resample.hpp) over 16-bit planes.  RS: a rotation per output row (map modes 0, 1
// and 5).  BORDER_CONSTANT: only the footprints that touch the plane enter the box, a tile with none has no box, a pixel whose footprint
// does not touch is the border value; the other modes: every footprint, in virtual coordinates.
// stage: RESAMPLE_LDS_BYTES, 16-byte aligned -- luma words in one half (6144), chroma pair dwords in the other (3072); red: 16 ints.
// ---------------------------------------------------------------------------------------------------------------------
constexpr uint32_t P010_BORDER_Y = 64u, P010_BORDER_UV = 512u | (512u << 16);  // vstab_warp_p010_planar's border values

template <typename R, int MODE, int BORDER, bool RS>
__device__ __forceinline__ void resample10_tile(const BorderArgs &ba, uint8_t *stage, int *red) {
    const WarpArgs &a = ba.c.w;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = blockIdx.x * RESAMPLE_TW + lane, y0 = blockIdx.y * RESAMPLE_TH + wave * RESAMPLE_RW;
    const float rfx = rcp_refined(a.p.ofx), rfy = rcp_refined(a.p.ofy);
    // 1. map (pixels right of / below the image are evaluated as the last column / row: never stored, inside the box)
    CubicTap t[RESAMPLE_RW];
    float ax[RESAMPLE_RW], ay[RESAMPLE_RW];
#pragma unroll
    for (int j = 0; j < RESAMPLE_RW; j++) {
        border_map<MODE, RS>(ba, min(x, a.dw - 1), min(y0 + j, a.dh - 1), rfx, rfy, ax[j], ay[j]);
        t[j] = cubic_tap(ax[j], ay[j]);
    }
    // 2. the boxes: luma footprints; chroma footprints of the even lanes' even rows, the map halved (exact) and quantised again
    const int cw = a.sw >> 1, ch = a.sh >> 1;
    const bool cact = !(lane & 1);
    int mnx = INT_MAX, mxx = INT_MIN, mny = INT_MAX, mxy = INT_MIN;
#pragma unroll
    for (int j = 0; j < RESAMPLE_RW; j++)
        if (resample_blends<R, BORDER>(t[j], a.sw, a.sh)) footprint_extent<R>(t[j], mnx, mxx, mny, mxy);
    CubicTap tc[RESAMPLE_RW / 2];
    int cmnx = INT_MAX, cmxx = INT_MIN, cmny = INT_MAX, cmxy = INT_MIN;
#pragma unroll
    for (int k = 0; k < RESAMPLE_RW / 2; k++) {
        tc[k] = cubic_tap(ax[2 * k] * 0.5f, ay[2 * k] * 0.5f);
        if (cact && resample_blends<R, BORDER>(tc[k], cw, ch)) footprint_extent<R>(tc[k], cmnx, cmxx, cmny, cmxy);
    }
    const BorderWords<BORDER> sy = {a.y, a.pitch_y, a.sw, a.sh, P010_BORDER_Y};  // (the border values: read by BORDER_CONSTANT alone)
    const BorderWordPairs<BORDER> suv = {a.uv, a.pitch_uv, cw, ch, P010_BORDER_UV};
    uint16_t *lds_y = reinterpret_cast<uint16_t *>(stage);
    uint32_t *lds_c = reinterpret_cast<uint32_t *>(stage + RESAMPLE_LDS_BYTES / 2);
    const TileBox by = tile_box<0, 2, true>(mnx, mxx, mny, mxy, red, RESAMPLE_LDS_BYTES / 4);
    const TileBox bc = tile_box<0, 2, true>(cmnx, cmxx, cmny, cmxy, red, RESAMPLE_LDS_BYTES / 8);
    // 3. stage
    if (by.lds) stage_box<BORDER, true>(sy, by, lds_y);
    if (bc.lds) stage_box<BORDER, true>(suv, bc, lds_c);
    __syncthreads();
    // 4. blend
#pragma unroll
    for (int j = 0; j < RESAMPLE_RW; j++) {
        const int y = y0 + j;
        if (x >= a.dw || y >= a.dh) continue;
        const CubicTap q = pick_tap(t, j);
        const uint32_t Y = resample_blends<R, BORDER>(q, a.sw, a.sh) ? resample_pixel<R, 1, BORDER>(sy, by, (const uint16_t *)lds_y, q) : P010_BORDER_Y;
        *reinterpret_cast<uint16_t *>(a.dst + (size_t)y * a.pitch_dst + (size_t)x * 2) = (uint16_t)(Y << 6);
        if (cact && !(j & 1)) {
            const CubicTap qc = pick_tap(tc, j / 2);
            const uint32_t UV = resample_blends<R, BORDER>(qc, cw, ch) ? resample_pixel<R, 2, BORDER>(suv, bc, (const uint32_t *)lds_c, qc) : P010_BORDER_UV;
            *reinterpret_cast<uint32_t *>(a.dst_uv + (size_t)(y >> 1) * a.pitch_dst_uv + (size_t)x * 2) = UV << 6;  // chroma sample x / 2: one dword
        }
    }
}

template <typename R, int MODE, int BORDER, bool RS>
__global__ void __launch_bounds__(256) k_warp_p010_resample(BorderArgs ba) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[RESAMPLE_LDS_BYTES];
    __shared__ __attribute__((aligned(16))) int red[16];  // read back as ds_read_b96 / ds_read2_b32: 16-byte aligned
    resample10_tile<R, MODE, BORDER, RS>(ba, stage, red);
}

// Kernels of this translation unit (and the two weight tables with them) are one code object: see preload_warp_kernels
vstab_status preload_p010_resample_kernels() {
    hipFuncAttributes at;
    VSTAB_HIP_TRY(hipFuncGetAttributes(&at, reinterpret_cast<const void *>(&k_warp_p010_resample<Cubic10, MAP_CREATEMAP_CL, VSTAB_BORDER_CONSTANT, false>)));
    return VSTAB_OK;
}

// ba checked and filled (vstab_warp_p010_planar_ex); map_mode 0 .. 5, rs with 0, 1 and 5 alone; resample CUBIC or LANCZOS4
vstab_status launch_warp_resample10(const BorderArgs &ba, int map_mode, bool rs, int resample, int border_mode, void *stream) {
    with_kernel_mode(map_mode, [&](auto mode) {
        with_border_mode(border_mode, [&](auto border) {
            with_bool(rs, [&](auto rs_c) {
                constexpr int MODE = decltype(mode)::value, BORDER = decltype(border)::value;
                constexpr bool RS = decltype(rs_c)::value;
                if constexpr (MODE <= MAP_CREATEMAP_CL_OPENCL && (!RS || map_mode_fish_to_pinhole(MODE))) {
                    if (resample == VSTAB_RESAMPLE_CUBIC) launch_tiles(k_warp_p010_resample<Cubic10, MODE, BORDER, RS>, ba, ba.c.w.dw, ba.c.w.dh, stream);
                    else launch_tiles(k_warp_p010_resample<Lanczos4_10, MODE, BORDER, RS>, ba, ba.c.w.dw, ba.c.w.dh, stream);
                }
            });
        });
    });
    VSTAB_HIP_TRY(hipGetLastError());
    return VSTAB_OK;
}

}  // namespace vstab
