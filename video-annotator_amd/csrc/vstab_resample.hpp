// vstab_resample.hpp -- the device side of the cv::remap kernels beside the headline warp: INTER_CUBIC (vstab_warp_cubic.hip), INTER_LANCZOS4
// (vstab_warp_lanczos4.hip) and INTER_LINEAR with a border mode (vstab_warp_border.hip), each with BORDER_CONSTANT, _REPLICATE, _REFLECT and
// _REFLECT_101.  One statement of each thing: the quantisation of a map position (the same for all three resamplers), OpenCV's
// borderInterpolate, the sources a tap reads, the tile's box, its staging into LDS, the read of a footprint row, the blends' channel
// arithmetic, the map of an output pixel, and -- for cubic and Lanczos with a non-constant border -- the tile and the stateless remap
// themselves, over a resampler trait.  The bilinear tap is here too: the keep-edge kernels (vstab_warp_keep.hip) blend with it.
//
// The tile (resample_tile; k_warp_cubic, k_warp_lanczos4 and k_warp_border run the same phases from the same pieces in their own units,
// for the reasons given there and in DESIGN.md §16): 64 x 16 output pixels, one workgroup of 256 threads, four rows per thread:
//   1. map      the exact map of the thread's four pixels in registers (k_quantised_map's arithmetic for every mode), quantised;
//   2. box      min / max of the footprints over the tile, reduced over the workgroup: exact, not probed.  BORDER_CONSTANT: the footprints
//               that touch the source (a tile with none has no box).  Other modes: every footprint, in VIRTUAL coordinates -- a reflected
//               border has no pixel "wholly outside", so a tile far outside the source still reads (mirrored) picture;
//   3. stage    each position of the box read once and converted (BGRx dwords; luma bytes / chroma pairs plane-wise): the border value in
//               every position outside (CONSTANT), or the source at the border-interpolated position;
//   4. blend    K LDS reads per footprint row, each at its natural alignment, v_dot2_i32_i16 on channel pairs gathered by v_perm_b32.
// A box over the LDS budget (strong minification, degenerate rotations, the axis pixel of map mode 0 at -32768) is sampled from global
// memory with the same arithmetic; so is every pixel of the stateless remap.  The map is never written to memory.
#pragma once
#include <climits>

#include "../../include/vstab.h"
#include "vstab_device.hpp"
#include "vstab_warp_args.hpp"

namespace vstab {

constexpr int RESAMPLE_TW = 64, RESAMPLE_TH = 16, RESAMPLE_RW = 4;  // tile; rows per thread (4 waves x 4 rows)
constexpr int RESAMPLE_LDS_BYTES = 24 * 1024;                       // stage budget per workgroup: six workgroups per CU by LDS

struct CubicArgs {  // the warp kernels' one argument (all resamplers)
    WarpArgs w;
    MapParams32 p32;
};
struct BorderArgs {  // the kernels that take a rotation per output row (k_warp_border, k_warp_cubic_rs, k_warp_lanczos4_rs)
    CubicArgs c;
    float rs_d[9];  // RS: rotation of the last output row minus the first's (c.w.p.r), fp32
    float rs_den;   // and (float)max(dh - 1, 1)
    float pd[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};  // MAP_RECTD_*: k1, k2, p1, p2, k3 of a rectilinear input lens (vstab_warp_nv12_pinhole); no other mode reads them
};

// cvRound (NaN / outside the int range -> INT_MIN), then cv::remap's split: X = saturate_cast<short>(sx >> 5), f = sx & 31
struct CubicTap {
    int X, Y, f;  // f = fy * 32 + fx: the table entry
};
__device__ __forceinline__ int cv_round_f32(float a) { return (a >= -2147483648.0f && a < 2147483648.0f) ? (int)__builtin_rintf(a) : INT_MIN; }
__device__ __forceinline__ CubicTap cubic_tap(float ax32, float ay32) {  // ax32, ay32 = 32 * map
    const int sx = cv_round_f32(ax32), sy = cv_round_f32(ay32);
    return {min(max(sx >> 5, -32768), 32767), min(max(sy >> 5, -32768), 32767), (sy & 31) * 32 + (sx & 31)};
}

// 32 * map of output pixel (x, y) for the kernels that take BorderArgs: map_at (vstab_map.hpp), with BorderArgs::pd for the MAP_RECTD_* modes.
// RS: the row's own rotation, m_k = fmaf(t, rs_d[k], r[k]) with t = (float)y / rs_den, fed to the mode's arithmetic as the per-row warp
// (vstab_warp_tile.hpp, map_phase) does.  Its preamble stands in place: through map_at, with the rotation a per-thread value, the four
// k_warp_keep kernels with a rotation per row came out another (modes 0 and 1: 2015 -> 2007, 2586 -> 2587, 2031 -> 2034, 2627 -> 2612
// lines), and so did every such k_warp_border, k_warp_cubic_rs and k_warp_lanczos4_rs kernel of modes 0, 1 and 11.
template <int MODE, bool RS>
__device__ __forceinline__ void border_map(const BorderArgs &ba, int x, int y, float rfx, float rfy, float &ax, float &ay) {
    if constexpr (RS) {
        const MapParams &p0 = ba.c.w.p;
        MapParams P = p0;
        const float t = div_with_rcp((float)y, ba.rs_den, rcp_refined(ba.rs_den));
#pragma unroll
        for (int k = 0; k < 9; k++) P.r[k] = __builtin_fmaf(t, ba.rs_d[k], p0.r[k]);
        MapParams32 p32 = ba.c.p32;
        p32.r02 = P.r[2], p32.r12 = P.r[5], p32.r22 = P.r[8];
        const float vy = norm_coord<MODE>((float)y - P.ocy, P.ofy, rfy);
        const RowTerm rt = {P.r[1] * vy, P.r[4] * vy, P.r[7] * vy};
        const float vx = norm_coord<MODE>((float)x - P.ocx, P.ofx, rfx);
        const ColTerm ct = {P.r[0] * vx, P.r[3] * vx, P.r[6] * vx};
        map_pixel_ex<MODE>(p32, P, ct, rt, vx, vy, ax, ay);
    } else {
        map_at<MODE>(ba.c.p32, ba.c.w.p, x, y, rfx, rfy, ax, ay, ba.pd);
    }
}

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
// Sources: a position (X, Y) as a dword with one channel per byte -- read at its border-interpolated position, or the border value
// (CONSTANT) where it lies outside.
// ---------------------------------------------------------------------------------------------------------------------
template <int BORDER>
struct BorderNv12Bgr {  // NV12 planes converted with the cvtColor arithmetic (BGRx); CONSTANT border 0 (cv::remap's Scalar(0))
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
            if ((unsigned)X < (unsigned)w && (unsigned)Y < (unsigned)h) return at(X, Y);
            return 0;
        } else {
            return at(X, Y);
        }
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
            if ((unsigned)X < (unsigned)w && (unsigned)Y < (unsigned)h) return at(X, Y);
            return border;
        } else {
            return at(X, Y);
        }
    }
};

// ---------------------------------------------------------------------------------------------------------------------
// The tile's box, its staging and the read of a footprint row.
// ---------------------------------------------------------------------------------------------------------------------
struct TileBox {
    int x0, y0, w, h;
    bool lds;  // staged (uniform over the workgroup)
};

// min / max of the tap anchors (X, Y) a thread passes in, reduced over the workgroup through red[16] in LDS.  The box covers the K x K
// footprint X - LO .. X - LO + K - 1 of all of them (<1, 4> cubic, <3, 8> Lanczos, <0, 2> bilinear).  No anchor from any thread: no box.
// SCALAR: the box, the same in every lane, in scalar registers.  The kernels whose box is in virtual coordinates were measured with it, the
// cubic and Lanczos kernels of the constant border without; each keeps its form ("After the consolidation").
template <int LO, int K, bool SCALAR>
__device__ __forceinline__ TileBox tile_box(int mnx, int mxx, int mny, int mxy, int *red, int cap_elems) {
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
    const bool have = mnx <= mxx;
    TileBox b;
    if constexpr (SCALAR) {
        b.x0 = __builtin_amdgcn_readfirstlane(mnx - LO), b.y0 = __builtin_amdgcn_readfirstlane(mny - LO);
        b.w = __builtin_amdgcn_readfirstlane(have ? mxx - mnx + K : 0), b.h = __builtin_amdgcn_readfirstlane(have ? mxy - mny + K : 0);
    } else {
        b.x0 = mnx - LO, b.y0 = mny - LO, b.w = have ? mxx - mnx + K : 0, b.h = have ? mxy - mny + K : 0;
    }
    b.lds = have && (long)b.w * b.h <= cap_elems;
    return b;
}

// every position of the box read once (rows by wave, columns by lane).  FOLD false (the cubic and Lanczos kernels of the constant border,
// whose box hugs the source): position by position, the border value outside.  FOLD true (virtual coordinates): a box inside the source --
// most tiles -- reads it as it is; any other goes through borderInterpolate, each column's position once for all its rows (the fold's
// integer remainder is ~20 vector instructions: evaluated per staged element it made the kernel VALU-bound at twice the cost of this form)
template <int BORDER, bool FOLD, typename T, typename Src>
__device__ __forceinline__ void stage_box(const Src &s, const TileBox &b, T *lds) {
    if constexpr (!FOLD) {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        for (int r = wave; r < b.h; r += 4)
            for (int c = lane; c < b.w; c += 64) lds[r * b.w + c] = (T)s.row_col(b.x0 + c, b.y0 + r);
    } else {
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
}

// K horizontally adjacent taps of the staged box, each read at its natural alignment.  BGRx dwords are 4-byte aligned whatever the tap, so
// the compiler's ds_read2_b32 pairs are aligned too.  Luma bytes / chroma pairs: one ds_read_u8 / ds_read_u16 per tap -- volatile, because
// the compiler otherwise merges the adjacent taps into ds_read_b32 / ds_read_b64 at a 1- or 2-byte boundary, which gfx950 executes lane by
// lane: 64 cycles instead of 2.3 (profiles/r05_lds_access_cost.txt)
template <int K, typename T>
__device__ __forceinline__ void lds_row(const T *p, uint32_t *v) {
    if constexpr (sizeof(T) < 4) {
        typedef __attribute__((address_space(3))) T LdsT;
        const volatile LdsT *q = (const volatile LdsT *)p;
#pragma unroll
        for (int c = 0; c < K; c++) v[c] = q[c];
    } else {
#pragma unroll
        for (int c = 0; c < K; c++) v[c] = p[c];
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// The bilinear tap, its read and its blend (k_warp_border, k_remap_border; k_warp_keep, k_remap_keep in vstab_warp_keep.hip).
// ---------------------------------------------------------------------------------------------------------------------
// bilinear tap: the top-left virtual position and the two weight pairs {w00, w01}, {w10, w11} as int16 halves
struct BorderTap {
    int X, Y;
    uint32_t w0, w1;
};
template <int BORDER>
__device__ __forceinline__ BorderTap border_tap(float ax32, float ay32, int w, int h) {
    const CubicTap t = cubic_tap(ax32, ay32);  // cvRound, sat16(s >> 5), s & 31: INTER_LINEAR's quantisation
    const uint32_t fx = t.f & 31, fy = t.f >> 5;
    BorderTap b;
    b.X = t.X, b.Y = t.Y;
    if constexpr (BORDER == VSTAB_BORDER_CONSTANT) {
        // every position outside is the border value: a pair of taps wholly outside may move to (-2, -1) / (len, len + 1), which keeps the box
        // inside [-2, len + 1] (the axis pixel of map mode 0 would stretch it to -32768 otherwise)
        b.X = min(max(b.X, -2), w), b.Y = min(max(b.Y, -2), h);
    }
    b.w0 = ((32 - fx) * (32 - fy)) | ((fx * (32 - fy)) << 16);
    b.w1 = ((32 - fx) * fy) | ((fx * fy) << 16);
    return b;
}

// One channel (byte CH of every tap dword): the horizontally adjacent taps' channel gathered into an int16 pair by v_perm_b32, two
// v_dot2_i32_i16 against the weight pairs.  Weights sum to 1024: no overflow, no saturation needed.
template <int CH>
__device__ __forceinline__ uint32_t border_channel(uint32_t t00, uint32_t t01, uint32_t t10, uint32_t t11, const BorderTap &t) {
    constexpr uint32_t sel = CH | 0x0c00u | ((4u + CH) << 16) | 0x0c000000u;  // [left.CH, 0, right.CH, 0]
    typedef short short2v __attribute__((ext_vector_type(2)));
    int acc = __builtin_amdgcn_sdot2(__builtin_bit_cast(short2v, __builtin_amdgcn_perm(t01, t00, sel)), __builtin_bit_cast(short2v, t.w0), 512, false);
    acc = __builtin_amdgcn_sdot2(__builtin_bit_cast(short2v, __builtin_amdgcn_perm(t11, t10, sel)), __builtin_bit_cast(short2v, t.w1), acc, false);
    return (uint32_t)acc >> 10;
}

// the four taps of t: from the staged box, or from the source itself when the box was not staged (uniform over the workgroup)
template <int BORDER, typename T, typename Src>
__device__ __forceinline__ void border_taps(const Src &s, const TileBox &b, const T *lds, const BorderTap &t, uint32_t (&v)[4]) {
    if (b.lds) {
        const int at = (t.Y - b.y0) * b.w + (t.X - b.x0);
        const T *q = lds + at;
        lds_row<2>(q, v), lds_row<2>(q + b.w, v + 2);
    } else {
        const int x0 = border_index<BORDER>(t.X, s.w), x1 = border_index<BORDER>(t.X + 1, s.w);
        const int y0 = border_index<BORDER>(t.Y, s.h), y1 = border_index<BORDER>(t.Y + 1, s.h);
        v[0] = s.row_col(x0, y0), v[1] = s.row_col(x1, y0), v[2] = s.row_col(x0, y1), v[3] = s.row_col(x1, y1);
    }
}

// Footprint rows: rows(r, v) fills v[0 .. K - 1] with the taps of footprint row r -- from the staged box, or from the source itself when the
// box was not staged (uniform over the workgroup), each tap border-interpolated.
template <int BORDER, int K, int LO, typename T, typename Src>
struct TapRows {
    const Src &s;
    TileBox b;
    const T *lds;
    int X, Y;  // the tap (by value: a reference into the thread's tap array kept that array in scratch)
    __device__ __forceinline__ void operator()(int r, uint32_t (&v)[K]) const {
        if (b.lds) {
            const int at = (Y - LO + r - b.y0) * b.w + (X - LO - b.x0);
            lds_row<K>(lds + at, v);
        } else {
            const int sy = border_index<BORDER>(Y - LO + r, s.h);
#pragma unroll
            for (int c = 0; c < K; c++) v[c] = s.row_col(border_index<BORDER>(X - LO + c, s.w), sy);
        }
    }
};

// ---------------------------------------------------------------------------------------------------------------------
// The blends' channel arithmetic: (sum + 2^14) >> 15 from the fixed-point tables (vstab_cubic.hpp, vstab_lanczos4.hpp).
// ---------------------------------------------------------------------------------------------------------------------
// One channel (byte CH of every tap dword) of the cubic blend: channel pairs of horizontally adjacent taps gathered into int16 pairs by
// v_perm_b32, eight v_dot2_i32_i16 against the weight pairs.  |sum| < 16 * 32767 * 255: no overflow.
template <int CH>
__device__ __forceinline__ uint32_t cubic_channel(const uint32_t (&t)[16], const uint32_t (&w)[8]) {
    constexpr uint32_t sel = CH | 0x0c00u | ((4u + CH) << 16) | 0x0c000000u;  // [left.CH, 0, right.CH, 0]
    typedef short short2v __attribute__((ext_vector_type(2)));
    int acc = 1 << 14;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        acc = __builtin_amdgcn_sdot2(__builtin_bit_cast(short2v, __builtin_amdgcn_perm(t[4 * r + 1], t[4 * r], sel)), __builtin_bit_cast(short2v, w[2 * r]),
                                     acc, false);
        acc = __builtin_amdgcn_sdot2(__builtin_bit_cast(short2v, __builtin_amdgcn_perm(t[4 * r + 3], t[4 * r + 2], sel)),
                                     __builtin_bit_cast(short2v, w[2 * r + 1]), acc, false);
    }
    return (uint32_t)sat8(acc >> 15);
}

// One footprint row of one channel of the Lanczos blend: channel pairs of horizontally adjacent taps gathered into int16 pairs by
// v_perm_b32, four v_dot2_i32_i16 against the row's weight pairs.  |sum| over the 64 taps < 64 * 32767 * 255: no overflow.
template <int CH>
__device__ __forceinline__ int lz_row(int acc, const uint32_t (&t)[8], const uint4 &w) {
    constexpr uint32_t sel = CH | 0x0c00u | ((4u + CH) << 16) | 0x0c000000u;  // [left.CH, 0, right.CH, 0]
    typedef short short2v __attribute__((ext_vector_type(2)));
    acc = __builtin_amdgcn_sdot2(__builtin_bit_cast(short2v, __builtin_amdgcn_perm(t[1], t[0], sel)), __builtin_bit_cast(short2v, w.x), acc, false);
    acc = __builtin_amdgcn_sdot2(__builtin_bit_cast(short2v, __builtin_amdgcn_perm(t[3], t[2], sel)), __builtin_bit_cast(short2v, w.y), acc, false);
    acc = __builtin_amdgcn_sdot2(__builtin_bit_cast(short2v, __builtin_amdgcn_perm(t[5], t[4], sel)), __builtin_bit_cast(short2v, w.z), acc, false);
    acc = __builtin_amdgcn_sdot2(__builtin_bit_cast(short2v, __builtin_amdgcn_perm(t[7], t[6], sel)), __builtin_bit_cast(short2v, w.w), acc, false);
    return acc;
}

// ---------------------------------------------------------------------------------------------------------------------
// Cubic and Lanczos with BORDER_REPLICATE, _REFLECT or _REFLECT_101, over a resampler trait R: the footprint R::K, R::LO and
// R::blend<CN>(rows, f), the channels 0 .. CN - 1 of the output as one byte each, from the footprint's rows and the table entry f (the
// trait lives beside its weight table, in the resampler's unit).  The constant border's kernels keep a tile of their own there, from the
// same pieces: only the footprints that touch the source enter their box, and a pixel whose footprint does not touch is the border value.
// ---------------------------------------------------------------------------------------------------------------------
// the footprint's first column / row and the one before its last: anchors for tile_box<0, 2>.  (Passing X, Y to tile_box<LO, K> is the same
// box, but not the same code: the compiler's output for the border kernels was measured in this form and is kept to the instruction.)
template <typename R>
__device__ __forceinline__ void footprint_extent(const CubicTap &t, int &mnx, int &mxx, int &mny, int &mxy) {
    mnx = min(mnx, t.X - R::LO), mxx = max(mxx, t.X - R::LO + R::K - 2);
    mny = min(mny, t.Y - R::LO), mxy = max(mxy, t.Y - R::LO + R::K - 2);
}

// one output sample
template <typename R, int CN, int BORDER, typename T, typename Src>
__device__ __forceinline__ uint32_t resample_pixel(const Src &s, const TileBox &b, const T *lds, const CubicTap &t) {
    const TapRows<BORDER, R::K, R::LO, T, Src> rows = {s, b, lds, t.X, t.Y};
    return R::template blend<CN>(rows, t.f);
}

// The warp of one tile.  PLANAR false: BGR8 out (cvtColor then cv::remap with the resampler and border mode BORDER); PLANAR true: the
// plane-wise warp (luma; chroma at the even pixels' positions halved, folded over the chroma plane's own size).
// stage: RESAMPLE_LDS_BYTES, 16-byte aligned; red: 16 ints, 16-byte aligned (read back as ds_read_b96 / ds_read2_b32).
template <typename R, int MODE, bool PLANAR, int BORDER>
__device__ __forceinline__ void resample_tile(const CubicArgs &c, uint8_t *stage, int *red) {
    static_assert(BORDER != VSTAB_BORDER_CONSTANT, "BORDER_CONSTANT is served by k_warp_cubic / k_warp_lanczos4");
    const WarpArgs &a = c.w;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = blockIdx.x * RESAMPLE_TW + lane, y0 = blockIdx.y * RESAMPLE_TH + wave * RESAMPLE_RW;
    const float rfx = rcp_refined(a.p.ofx), rfy = rcp_refined(a.p.ofy);
    // 1. map (pixels right of / below the image are evaluated as the last column / row: never stored, inside the box)
    CubicTap t[RESAMPLE_RW];
    float ax[RESAMPLE_RW], ay[RESAMPLE_RW];
#pragma unroll
    for (int j = 0; j < RESAMPLE_RW; j++) {
        map_at<MODE>(c.p32, c.w.p, min(x, a.dw - 1), min(y0 + j, a.dh - 1), rfx, rfy, ax[j], ay[j]);
        t[j] = cubic_tap(ax[j], ay[j]);
    }
    // 2. box of the luma / BGR footprints: every pixel, no "touches the source" filter
    int mnx = INT_MAX, mxx = INT_MIN, mny = INT_MAX, mxy = INT_MIN;
#pragma unroll
    for (int j = 0; j < RESAMPLE_RW; j++) footprint_extent<R>(t[j], mnx, mxx, mny, mxy);
    if constexpr (!PLANAR) {
        const BorderNv12Bgr<BORDER> src = {a.y, a.uv, a.pitch_y, a.pitch_uv, a.sw, a.sh};
        uint32_t *lds = reinterpret_cast<uint32_t *>(stage);
        const TileBox b = tile_box<0, 2, true>(mnx, mxx, mny, mxy, red, RESAMPLE_LDS_BYTES / 4);
        // 3. stage
        if (b.lds) stage_box<BORDER, true>(src, b, lds);
        __syncthreads();
        // 4. blend
#pragma unroll
        for (int j = 0; j < RESAMPLE_RW; j++) {
            const int y = y0 + j;
            if (x >= a.dw || y >= a.dh) continue;
            const uint32_t bgr = resample_pixel<R, 3, BORDER>(src, b, (const uint32_t *)lds, t[j]);
            uint8_t *o = a.dst + (size_t)y * a.pitch_dst + (size_t)x * 3;
            o[0] = (uint8_t)bgr, o[1] = (uint8_t)(bgr >> 8), o[2] = (uint8_t)(bgr >> 16);
        }
    } else {
        // chroma sample (x / 2, y / 2) of every even output pixel: the map halved (exact) and quantised again, over the chroma plane's size
        const int cw = a.sw >> 1, ch = a.sh >> 1;
        const bool cact = !(lane & 1);
        CubicTap tc[RESAMPLE_RW / 2];
        int cmnx = INT_MAX, cmxx = INT_MIN, cmny = INT_MAX, cmxy = INT_MIN;
#pragma unroll
        for (int k = 0; k < RESAMPLE_RW / 2; k++) {
            tc[k] = cubic_tap(ax[2 * k] * 0.5f, ay[2 * k] * 0.5f);
            if (cact) footprint_extent<R>(tc[k], cmnx, cmxx, cmny, cmxy);
        }
        const BorderBytes<1, BORDER> sy = {a.y, a.pitch_y, a.sw, a.sh, 0u};
        const BorderBytes<2, BORDER> suv = {a.uv, a.pitch_uv, cw, ch, 0u};
        uint8_t *lds_y = stage;                                                         // luma bytes: half the budget
        uint16_t *lds_c = reinterpret_cast<uint16_t *>(stage + RESAMPLE_LDS_BYTES / 2);  // chroma pairs: the other half
        const TileBox by = tile_box<0, 2, true>(mnx, mxx, mny, mxy, red, RESAMPLE_LDS_BYTES / 2);
        const TileBox bc = tile_box<0, 2, true>(cmnx, cmxx, cmny, cmxy, red, RESAMPLE_LDS_BYTES / 4);
        if (by.lds) stage_box<BORDER, true>(sy, by, lds_y);
        if (bc.lds) stage_box<BORDER, true>(suv, bc, lds_c);
        __syncthreads();
#pragma unroll
        for (int j = 0; j < RESAMPLE_RW; j++) {
            const int y = y0 + j;
            if (x >= a.dw || y >= a.dh) continue;
            a.dst[(size_t)y * a.pitch_dst + x] = (uint8_t)resample_pixel<R, 1, BORDER>(sy, by, (const uint8_t *)lds_y, t[j]);
            if (cact && !(j & 1)) {
                const uint32_t UV = resample_pixel<R, 2, BORDER>(suv, bc, (const uint16_t *)lds_c, tc[j / 2]);
                uint8_t *o = a.dst_uv + (size_t)(y >> 1) * a.pitch_dst_uv + (size_t)x;  // chroma sample x / 2: bytes x, x + 1
                o[0] = (uint8_t)UV, o[1] = (uint8_t)(UV >> 8);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Cubic and Lanczos with a rotation per output row (k_warp_cubic_rs, k_warp_lanczos4_rs; map modes 0, 1 and 5, and MAP_RS_FISHD_TO_RECT: the
// calibrated lens), every border mode: resample_tile's phases with border_map<MODE, true> as the map.  The MAP_RECTD_* modes (a rectilinear
// lens's five coefficients, which travel in BorderArgs) ride the same tile with one rotation: border_map<MODE, false>.  BORDER_CONSTANT goes through the
// same tile with the constant border's touch filter (R::touches, as k_warp_cubic / k_warp_lanczos4 have it): only the footprints that
// touch the source enter the box, a tile with none has no box, a pixel whose footprint does not touch is the border value.
// ---------------------------------------------------------------------------------------------------------------------
// whether the pixel of tap t is blended (any other is the border value): every pixel, but for the constant border
template <typename R, int BORDER>
__device__ __forceinline__ bool resample_blends(const CubicTap &t, int w, int h) {
    if constexpr (BORDER == VSTAB_BORDER_CONSTANT) return R::touches(t, w, h);
    else return true;
}
// tap j of the thread's taps without an index into the array: where the compiler keeps the blend loop rolled (the Lanczos BGR kernels) an
// indexed read puts the array into scratch memory; a chain of selects keeps it in registers, and folds to t[j] where the loop is unrolled
template <int N>
__device__ __forceinline__ CubicTap pick_tap(const CubicTap (&t)[N], int j) {
    CubicTap r = t[0];
#pragma unroll
    for (int k = 1; k < N; k++)
        if (j == k) r = t[k];
    return r;
}
// stage, red: as for resample_tile
template <typename R, int MODE, bool PLANAR, int BORDER>
__device__ __forceinline__ void resample_tile_rs(const BorderArgs &ba, uint8_t *stage, int *red) {
    const WarpArgs &a = ba.c.w;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = blockIdx.x * RESAMPLE_TW + lane, y0 = blockIdx.y * RESAMPLE_TH + wave * RESAMPLE_RW;
    const float rfx = rcp_refined(a.p.ofx), rfy = rcp_refined(a.p.ofy);
    // 1. map, each row's matrix formed where it is consumed (pixels right of / below the image are evaluated as the last column / row)
    CubicTap t[RESAMPLE_RW];
    float ax[RESAMPLE_RW], ay[RESAMPLE_RW];
#pragma unroll
    for (int j = 0; j < RESAMPLE_RW; j++) {
        border_map<MODE, !ModeTraits<MODE>::rectd>(ba, min(x, a.dw - 1), min(y0 + j, a.dh - 1), rfx, rfy, ax[j], ay[j]);
        t[j] = cubic_tap(ax[j], ay[j]);
    }
    // 2. box of the luma / BGR footprints, in virtual coordinates: every pixel (CONSTANT: those that touch the source)
    int mnx = INT_MAX, mxx = INT_MIN, mny = INT_MAX, mxy = INT_MIN;
#pragma unroll
    for (int j = 0; j < RESAMPLE_RW; j++)
        if (resample_blends<R, BORDER>(t[j], a.sw, a.sh)) footprint_extent<R>(t[j], mnx, mxx, mny, mxy);
    if constexpr (!PLANAR) {
        const BorderNv12Bgr<BORDER> src = {a.y, a.uv, a.pitch_y, a.pitch_uv, a.sw, a.sh};
        uint32_t *lds = reinterpret_cast<uint32_t *>(stage);
        const TileBox b = tile_box<0, 2, true>(mnx, mxx, mny, mxy, red, RESAMPLE_LDS_BYTES / 4);
        // 3. stage
        if (b.lds) stage_box<BORDER, true>(src, b, lds);
        __syncthreads();
        // 4. blend
#pragma unroll
        for (int j = 0; j < RESAMPLE_RW; j++) {
            const int y = y0 + j;
            if (x >= a.dw || y >= a.dh) continue;
            const CubicTap q = pick_tap(t, j);
            const uint32_t bgr = resample_blends<R, BORDER>(q, a.sw, a.sh) ? resample_pixel<R, 3, BORDER>(src, b, (const uint32_t *)lds, q) : 0u;
            uint8_t *o = a.dst + (size_t)y * a.pitch_dst + (size_t)x * 3;
            o[0] = (uint8_t)bgr, o[1] = (uint8_t)(bgr >> 8), o[2] = (uint8_t)(bgr >> 16);
        }
    } else {
        // chroma sample (x / 2, y / 2) of every even output pixel: the map halved (exact) and quantised again, over the chroma plane's size
        const int cw = a.sw >> 1, ch = a.sh >> 1;
        const bool cact = !(lane & 1);
        CubicTap tc[RESAMPLE_RW / 2];
        int cmnx = INT_MAX, cmxx = INT_MIN, cmny = INT_MAX, cmxy = INT_MIN;
#pragma unroll
        for (int k = 0; k < RESAMPLE_RW / 2; k++) {
            tc[k] = cubic_tap(ax[2 * k] * 0.5f, ay[2 * k] * 0.5f);
            if (cact && resample_blends<R, BORDER>(tc[k], cw, ch)) footprint_extent<R>(tc[k], cmnx, cmxx, cmny, cmxy);
        }
        const BorderBytes<1, BORDER> sy = {a.y, a.pitch_y, a.sw, a.sh, 16u};  // (the border values: read by BORDER_CONSTANT alone)
        const BorderBytes<2, BORDER> suv = {a.uv, a.pitch_uv, cw, ch, 0x8080u};
        uint8_t *lds_y = stage;                                                         // luma bytes: half the budget
        uint16_t *lds_c = reinterpret_cast<uint16_t *>(stage + RESAMPLE_LDS_BYTES / 2);  // chroma pairs: the other half
        const TileBox by = tile_box<0, 2, true>(mnx, mxx, mny, mxy, red, RESAMPLE_LDS_BYTES / 2);
        const TileBox bc = tile_box<0, 2, true>(cmnx, cmxx, cmny, cmxy, red, RESAMPLE_LDS_BYTES / 4);
        if (by.lds) stage_box<BORDER, true>(sy, by, lds_y);
        if (bc.lds) stage_box<BORDER, true>(suv, bc, lds_c);
        __syncthreads();
#pragma unroll
        for (int j = 0; j < RESAMPLE_RW; j++) {
            const int y = y0 + j;
            if (x >= a.dw || y >= a.dh) continue;
            const CubicTap q = pick_tap(t, j);
            a.dst[(size_t)y * a.pitch_dst + x] = (uint8_t)(resample_blends<R, BORDER>(q, a.sw, a.sh) ? resample_pixel<R, 1, BORDER>(sy, by, (const uint8_t *)lds_y, q) : 16u);
            if (cact && !(j & 1)) {
                const CubicTap qc = pick_tap(tc, j / 2);
                const uint32_t UV = resample_blends<R, BORDER>(qc, cw, ch) ? resample_pixel<R, 2, BORDER>(suv, bc, (const uint16_t *)lds_c, qc) : 0x8080u;
                uint8_t *o = a.dst_uv + (size_t)(y >> 1) * a.pitch_dst_uv + (size_t)x;  // chroma sample x / 2: bytes x, x + 1
                o[0] = (uint8_t)UV, o[1] = (uint8_t)(UV >> 8);
            }
        }
    }
}

// The stateless remap's pixel: cv::remap(resampler, BORDER) of CN interleaved 8-bit channels with float map planes (any map, NaN / huge /
// tie entries included).  One thread per output pixel, taps from global memory.
#define VSTAB_REMAP_PARAMS                                                                                                                             \
    const uint8_t *__restrict__ src, size_t pitch_src, int sw, int sh, const float *__restrict__ mapx, size_t pitch_x, const float *__restrict__ mapy, \
        size_t pitch_y
#define VSTAB_REMAP_DST uint8_t *__restrict__ dst, size_t pitch_dst, int dw, int dh
template <typename R, int CN, int BORDER>
__device__ __forceinline__ void remap_pixel(VSTAB_REMAP_PARAMS, VSTAB_REMAP_DST) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= dw || y >= dh) return;
    const float mx = reinterpret_cast<const float *>(reinterpret_cast<const uint8_t *>(mapx) + (size_t)y * pitch_x)[x];
    const float my = reinterpret_cast<const float *>(reinterpret_cast<const uint8_t *>(mapy) + (size_t)y * pitch_y)[x];
    const CubicTap t = cubic_tap(mx * 32.0f, my * 32.0f);
    const BorderBytes<CN, BORDER> s = {src, pitch_src, sw, sh, 0u};
    const TileBox none = {0, 0, 0, 0, false};
    const uint32_t out = resample_pixel<R, CN, BORDER>(s, none, (const uint32_t *)nullptr, t);
    uint8_t *o = dst + (size_t)y * pitch_dst + (size_t)x * CN;
    o[0] = (uint8_t)out;
    if constexpr (CN > 1) o[1] = (uint8_t)(out >> 8);
    if constexpr (CN > 2) o[2] = (uint8_t)(out >> 16);
}

}  // namespace vstab
