// vstab_warp_lanczos4.hip -- cv::remap's INTER_LANCZOS4 for gfx950, with every border mode: the fused NV12 -> BGR8 warp, the plane-wise
// NV12 -> NV12 warp and the stateless remap of map planes.  Definition (include/vstab.h, vstab_warp_nv12_lanczos4 and "Border modes of the
// cubic and Lanczos resamplers"; tests/warp_def.py): the map quantised to 1/32 pixel as for INTER_LINEAR,
// an 8 x 8 footprint at (X - 3 .. X + 4, Y - 3 .. Y + 4), 64 integer weights from OpenCV's fixed-point table (vstab_lanczos4.hpp), each tap
// outside the source the border value (BORDER_CONSTANT) or read at its borderInterpolate position, (sum + 2^14) >> 15 saturated to 0..255.
//
// The tile's phases, the remap and the entry points are the resamplers' common ones (vstab_resample.hpp, vstab_warp_host.hpp).  This
// unit holds the Lanczos table, the Lanczos blend, the constant border's tile (k_warp_lanczos4) and the kernels under their names.  The table is 128 KiB, four times the L1: the rows of an entry a
// pixel reads depend on its fractions only, and neighbouring pixels share fy.
#include "vstab_lanczos4.hpp"
#include "vstab_warp_host.hpp"

namespace vstab {

__device__ const Lanczos4Table g_lanczos4 = make_lanczos4_table();  // in the code object's read-only data: loaded with the kernels

// row r of an entry's weights: 8 int16 as 4 packed pairs (one 16-byte load), pair h = columns 2 h (low half) and 2 h + 1
__device__ __forceinline__ uint4 lz_weights(int f, int r) { return reinterpret_cast<const uint4 *>(g_lanczos4.w)[8 * f + r]; }

struct Lanczos4 {
    static constexpr int K = 8, LO = 3;
    // some tap of the footprint inside a w x h source
    __device__ __forceinline__ static bool touches(const CubicTap &t, int w, int h) { return t.X + 4 >= 0 && t.X - 3 < w && t.Y + 4 >= 0 && t.Y - 3 < h; }
    // row by row, the row's 8 weights at once: channels 0 .. CN - 1 of the output, one byte each
    template <int CN, typename Rows>
    __device__ __forceinline__ static uint32_t blend(const Rows &rows, int f) {
        int acc0 = 1 << 14, acc1 = 1 << 14, acc2 = 1 << 14;
#pragma unroll
        for (int r = 0; r < 8; r++) {
            uint32_t v[8];
            const uint4 w = lz_weights(f, r);
            rows(r, v);
            acc0 = lz_row<0>(acc0, v, w);
            if constexpr (CN > 1) acc1 = lz_row<1>(acc1, v, w);
            if constexpr (CN > 2) acc2 = lz_row<2>(acc2, v, w);
        }
        uint32_t out = (uint32_t)sat8(acc0 >> 15);
        if constexpr (CN > 1) out |= (uint32_t)sat8(acc1 >> 15) << 8;
        if constexpr (CN > 2) out |= (uint32_t)sat8(acc2 >> 15) << 16;
        return out;
    }
};

// ---------------------------------------------------------------------------------------------------------------------
// The constant border: footprint rows and blend with the tap as it stands (no border interpolation), the tile and the remap.
// ---------------------------------------------------------------------------------------------------------------------
// the 8 taps of footprint row r: from the staged box, or from the source itself when the box was not staged
template <typename T, typename Src>
__device__ __forceinline__ void lz_taps(const Src &s, const TileBox &b, const T *lds, const CubicTap &t, int r, uint32_t (&v)[8]) {
    if (b.lds) {
        const int at = (t.Y - 3 + r - b.y0) * b.w + (t.X - 3 - b.x0);
        lds_row<8>(lds + at, v);
    } else {
#pragma unroll
        for (int c = 0; c < 8; c++) v[c] = s.row_col(t.X - 3 + c, t.Y - 3 + r);
    }
}

// The blend of one footprint: channels 0 .. CN - 1 of the output, one byte each
template <int CN, typename T, typename Src>
__device__ __forceinline__ uint32_t lz_blend(const Src &s, const TileBox &b, const T *lds, const CubicTap &t) {
    int acc0 = 1 << 14, acc1 = 1 << 14, acc2 = 1 << 14;
#pragma unroll
    for (int r = 0; r < 8; r++) {
        uint32_t v[8];
        const uint4 w = lz_weights(t.f, r);
        lz_taps(s, b, lds, t, r, v);
        acc0 = lz_row<0>(acc0, v, w);
        if constexpr (CN > 1) acc1 = lz_row<1>(acc1, v, w);
        if constexpr (CN > 2) acc2 = lz_row<2>(acc2, v, w);
    }
    uint32_t out = (uint32_t)sat8(acc0 >> 15);
    if constexpr (CN > 1) out |= (uint32_t)sat8(acc1 >> 15) << 8;
    if constexpr (CN > 2) out |= (uint32_t)sat8(acc2 >> 15) << 16;
    return out;
}

// k_warp_lanczos4 -- NV12 in; PLANAR false: BGR8 out (cvtColor then cv::remap INTER_LANCZOS4, border 0); PLANAR true: the plane-wise warp
// (luma border 16; chroma at the even pixels' positions halved, border (128, 128)).
// The tile's phases with the constant border's touch filter, kept apart from resample_tile as k_warp_cubic's is (vstab_warp_cubic.hip).
template <int MODE, bool PLANAR>
__global__ void __launch_bounds__(256) k_warp_lanczos4(CubicArgs c) {
    const WarpArgs &a = c.w;
    __shared__ __attribute__((aligned(16))) uint8_t stage[RESAMPLE_LDS_BYTES];
    __shared__ __attribute__((aligned(16))) int red[16];  // read back as ds_read_b96 / ds_read2_b32: 16-byte aligned
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = blockIdx.x * RESAMPLE_TW + lane, y0 = blockIdx.y * RESAMPLE_TH + wave * RESAMPLE_RW;
    const float rfx = rcp_refined(a.p.ofx), rfy = rcp_refined(a.p.ofy);
    // 1. map (pixels right of / below the image are evaluated as the last column / row: never stored, inside the box)
    CubicTap t[RESAMPLE_RW], tc[RESAMPLE_RW / 2];
    float ax[RESAMPLE_RW], ay[RESAMPLE_RW];
#pragma unroll
    for (int j = 0; j < RESAMPLE_RW; j++) {
        map_at<MODE>(c.p32, c.w.p, min(x, a.dw - 1), min(y0 + j, a.dh - 1), rfx, rfy, ax[j], ay[j]);
        t[j] = cubic_tap(ax[j], ay[j]);
    }
    // 2. box of the luma / BGR taps
    int mnx = INT_MAX, mxx = INT_MIN, mny = INT_MAX, mxy = INT_MIN;
#pragma unroll
    for (int j = 0; j < RESAMPLE_RW; j++)
        if (Lanczos4::touches(t[j], a.sw, a.sh)) mnx = min(mnx, t[j].X), mxx = max(mxx, t[j].X), mny = min(mny, t[j].Y), mxy = max(mxy, t[j].Y);
    if constexpr (!PLANAR) {
        const BorderNv12Bgr<VSTAB_BORDER_CONSTANT> src = {a.y, a.uv, a.pitch_y, a.pitch_uv, a.sw, a.sh};
        uint32_t *lds = reinterpret_cast<uint32_t *>(stage);
        const TileBox b = tile_box<3, 8, false>(mnx, mxx, mny, mxy, red, RESAMPLE_LDS_BYTES / 4);
        // 3. stage
        if (b.lds) stage_box<VSTAB_BORDER_CONSTANT, false>(src, b, lds);
        __syncthreads();
        // 4. blend
#pragma unroll
        for (int j = 0; j < RESAMPLE_RW; j++) {
            const int y = y0 + j;
            if (x >= a.dw || y >= a.dh) continue;
            const uint32_t bgr = Lanczos4::touches(t[j], a.sw, a.sh) ? lz_blend<3>(src, b, (const uint32_t *)lds, t[j]) : 0u;
            uint8_t *o = a.dst + (size_t)y * a.pitch_dst + (size_t)x * 3;
            o[0] = (uint8_t)bgr, o[1] = (uint8_t)(bgr >> 8), o[2] = (uint8_t)(bgr >> 16);
        }
    } else {
        // chroma sample (x / 2, y / 2) of every even output pixel: the map halved (exact) and quantised again
        const int cw = a.sw >> 1, ch = a.sh >> 1;
        const bool cact = !(lane & 1);
        int cmnx = INT_MAX, cmxx = INT_MIN, cmny = INT_MAX, cmxy = INT_MIN;
#pragma unroll
        for (int k = 0; k < RESAMPLE_RW / 2; k++) {
            tc[k] = cubic_tap(ax[2 * k] * 0.5f, ay[2 * k] * 0.5f);
            if (cact && Lanczos4::touches(tc[k], cw, ch))
                cmnx = min(cmnx, tc[k].X), cmxx = max(cmxx, tc[k].X), cmny = min(cmny, tc[k].Y), cmxy = max(cmxy, tc[k].Y);
        }
        const BorderBytes<1, VSTAB_BORDER_CONSTANT> sy = {a.y, a.pitch_y, a.sw, a.sh, 16u};
        const BorderBytes<2, VSTAB_BORDER_CONSTANT> suv = {a.uv, a.pitch_uv, cw, ch, 0x8080u};
        uint8_t *lds_y = stage;                                                  // luma bytes: half the budget
        uint16_t *lds_c = reinterpret_cast<uint16_t *>(stage + RESAMPLE_LDS_BYTES / 2);  // chroma pairs: the other half
        const TileBox by = tile_box<3, 8, false>(mnx, mxx, mny, mxy, red, RESAMPLE_LDS_BYTES / 2);
        const TileBox bc = tile_box<3, 8, false>(cmnx, cmxx, cmny, cmxy, red, RESAMPLE_LDS_BYTES / 4);
        if (by.lds) stage_box<VSTAB_BORDER_CONSTANT, false>(sy, by, lds_y);
        if (bc.lds) stage_box<VSTAB_BORDER_CONSTANT, false>(suv, bc, lds_c);
        __syncthreads();
#pragma unroll
        for (int j = 0; j < RESAMPLE_RW; j++) {
            const int y = y0 + j;
            if (x >= a.dw || y >= a.dh) continue;
            const uint32_t Y = Lanczos4::touches(t[j], a.sw, a.sh) ? lz_blend<1>(sy, by, (const uint8_t *)lds_y, t[j]) : 16u;
            a.dst[(size_t)y * a.pitch_dst + x] = (uint8_t)Y;
            if (cact && !(j & 1)) {
                const CubicTap &q = tc[j / 2];
                const uint32_t UV = Lanczos4::touches(q, cw, ch) ? lz_blend<2>(suv, bc, (const uint16_t *)lds_c, q) : 0x8080u;
                uint8_t *o = a.dst_uv + (size_t)(y >> 1) * a.pitch_dst_uv + (size_t)x;  // chroma sample x / 2: bytes x, x + 1
                o[0] = (uint8_t)UV, o[1] = (uint8_t)(UV >> 8);
            }
        }
    }
}

// k_remap_lanczos4 -- cv::remap(INTER_LANCZOS4, BORDER_CONSTANT border) of CN interleaved 8-bit channels with float map planes: the
// stateless building block (any map, NaN / huge / tie entries included).  One thread per output pixel, taps from global memory.
template <int CN>
__global__ void __launch_bounds__(256) k_remap_lanczos4(VSTAB_REMAP_PARAMS, uint32_t border, VSTAB_REMAP_DST) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= dw || y >= dh) return;
    const float mx = reinterpret_cast<const float *>(reinterpret_cast<const uint8_t *>(mapx) + (size_t)y * pitch_x)[x];
    const float my = reinterpret_cast<const float *>(reinterpret_cast<const uint8_t *>(mapy) + (size_t)y * pitch_y)[x];
    const CubicTap t = cubic_tap(mx * 32.0f, my * 32.0f);
    uint32_t out = border;
    if (Lanczos4::touches(t, sw, sh)) {
        const BorderBytes<CN, VSTAB_BORDER_CONSTANT> s = {src, pitch_src, sw, sh, border};
        const TileBox none = {0, 0, 0, 0, false};
        out = lz_blend<CN>(s, none, (const uint32_t *)nullptr, t);
    }
    uint8_t *o = dst + (size_t)y * pitch_dst + (size_t)x * CN;
    o[0] = (uint8_t)out;
    if constexpr (CN > 1) o[1] = (uint8_t)(out >> 8);
    if constexpr (CN > 2) o[2] = (uint8_t)(out >> 16);
}

// k_warp_lanczos4_border / k_remap_lanczos4_border -- the warp / the stateless remap with border mode BORDER (REPLICATE, REFLECT, REFLECT_101)
template <int MODE, bool PLANAR, int BORDER>
__global__ void __launch_bounds__(256) k_warp_lanczos4_border(CubicArgs c) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[RESAMPLE_LDS_BYTES];
    __shared__ __attribute__((aligned(16))) int red[16];
    resample_tile<Lanczos4, MODE, PLANAR, BORDER>(c, stage, red);
}
template <int CN, int BORDER>
__global__ void __launch_bounds__(256) k_remap_lanczos4_border(VSTAB_REMAP_PARAMS, VSTAB_REMAP_DST) {
    remap_pixel<Lanczos4, CN, BORDER>(src, pitch_src, sw, sh, mapx, pitch_x, mapy, pitch_y, dst, pitch_dst, dw, dh);
}

// k_warp_lanczos4_rs -- the warp with a rotation per output row (vstab_warp_nv12_rs_ex; map modes 0, 1, 5 and MAP_RS_FISHD_TO_RECT), every
// border mode, BORDER_CONSTANT included: resample_tile_rs (vstab_resample.hpp).  MAP_RECTD_TO_RECT / _FISH (vstab_warp_nv12_pinhole): the
// same tile with one rotation and the rectilinear lens's five coefficients, which travel in BorderArgs
template <int MODE, bool PLANAR, int BORDER>
__global__ void __launch_bounds__(256) k_warp_lanczos4_rs(BorderArgs ba) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[RESAMPLE_LDS_BYTES];
    __shared__ __attribute__((aligned(16))) int red[16];
    resample_tile_rs<Lanczos4, MODE, PLANAR, BORDER>(ba, stage, red);
}

struct Lanczos4Kernels {
    template <int MODE, bool PLANAR, int BORDER>
    static auto warp() {
        if constexpr (BORDER == VSTAB_BORDER_CONSTANT) return k_warp_lanczos4<MODE, PLANAR>;
        else return k_warp_lanczos4_border<MODE, PLANAR, BORDER>;
    }
    template <int MODE, bool PLANAR, int BORDER>
    static auto warp_rs() {
        return k_warp_lanczos4_rs<MODE, PLANAR, BORDER>;
    }
    template <int CN, int BORDER>
    static auto remap() {
        if constexpr (BORDER == VSTAB_BORDER_CONSTANT) return k_remap_lanczos4<CN>;
        else return k_remap_lanczos4_border<CN, BORDER>;
    }
};

// Kernels of this translation unit (and the weight table with them) are one code object: see preload_warp_kernels
vstab_status preload_lanczos4_kernels() {
    hipFuncAttributes at;
    VSTAB_HIP_TRY(hipFuncGetAttributes(&at, reinterpret_cast<const void *>(&k_remap_lanczos4<1>)));
    return VSTAB_OK;
}

vstab_status launch_warp_lanczos4(const BorderArgs &ba, const WarpRoute &r, int out_format, int border_mode, void *stream) {
    return launch_warp_resample<Lanczos4Kernels>(ba, r, out_format, border_mode, stream);
}

}  // namespace vstab

using namespace vstab;

extern "C" {

vstab_status vstab_lanczos4_weights(int16_t *out) {
    static constexpr Lanczos4Table tab = make_lanczos4_table();
    if (!out) return fail(VSTAB_ERR_INVALID, "vstab_lanczos4_weights: null pointer");
    for (int i = 0; i < LANCZOS4_TAB * 64; i++) out[i] = tab.w[i];
    return VSTAB_OK;
}

vstab_status vstab_remap_lanczos4(const void *src, size_t pitch_src, int sw, int sh, int channels, const void *map_x, size_t pitch_x, const void *map_y,
                                  size_t pitch_y, const int border[3], void *dst, size_t pitch_dst, int dw, int dh, void *stream) {
    return remap_resample<Lanczos4Kernels>("vstab_remap_lanczos4", src, pitch_src, sw, sh, channels, map_x, pitch_x, map_y, pitch_y, nullptr, border, dst,
                                           pitch_dst, dw, dh, stream);
}

vstab_status vstab_remap_lanczos4_border(const void *src, size_t pitch_src, int sw, int sh, int channels, const void *map_x, size_t pitch_x,
                                         const void *map_y, size_t pitch_y, int border_mode, const int border[3], void *dst, size_t pitch_dst, int dw,
                                         int dh, void *stream) {
    return remap_resample<Lanczos4Kernels>("vstab_remap_lanczos4_border", src, pitch_src, sw, sh, channels, map_x, pitch_x, map_y, pitch_y, &border_mode,
                                           border, dst, pitch_dst, dw, dh, stream);
}

vstab_status vstab_warp_nv12_lanczos4(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int sw, int sh, const float params[17], int map_mode,
                                      int out_format, void *dst, size_t pitch_dst, void *dst_uv, size_t pitch_dst_uv, int dw, int dh, void *stream) {
    return warp_nv12({.e = ENTRY_LANCZOS4, .y = y, .pitch_y = pitch_y, .uv = uv, .pitch_uv = pitch_uv, .sw = sw, .sh = sh, .params = params, .map_mode = map_mode,
                      .resample = VSTAB_RESAMPLE_LANCZOS4, .out_format = out_format, .dst = dst, .pitch_dst = pitch_dst, .dst_uv = dst_uv, .pitch_dst_uv = pitch_dst_uv,
                      .dw = dw, .dh = dh, .stream = stream});
}

vstab_status vstab_warp_nv12_lanczos4_border(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int sw, int sh, const float params[17],
                                             int map_mode, int out_format, int border_mode, void *dst, size_t pitch_dst, void *dst_uv, size_t pitch_dst_uv, int dw, int dh,
                                             void *stream) {
    return warp_nv12({.e = ENTRY_LANCZOS4_BORDER, .y = y, .pitch_y = pitch_y, .uv = uv, .pitch_uv = pitch_uv, .sw = sw, .sh = sh, .params = params,
                      .map_mode = map_mode, .resample = VSTAB_RESAMPLE_LANCZOS4, .border_mode = border_mode, .out_format = out_format, .dst = dst,
                      .pitch_dst = pitch_dst, .dst_uv = dst_uv, .pitch_dst_uv = pitch_dst_uv, .dw = dw, .dh = dh, .stream = stream});
}

}  // extern "C"
