// vstab_warp_cubic.hip -- cv::remap's INTER_CUBIC for gfx950, with every border mode: the fused NV12 -> BGR8 warp, the plane-wise
// NV12 -> NV12 warp and the stateless remap of map planes.  Definition (include/vstab.h, vstab_warp_nv12_cubic and "Border modes of the cubic
// and Lanczos resamplers"; tests/warp_def.py): the map quantised to 1/32 pixel as for INTER_LINEAR, a 4 x 4
// footprint at (X - 1 .. X + 2, Y - 1 .. Y + 2), 16 integer weights from OpenCV's fixed-point table (vstab_cubic.hpp), each tap outside the
// source the border value (BORDER_CONSTANT) or read at its borderInterpolate position, (sum + 2^14) >> 15 saturated to 0..255.
//
// The tile's phases, the remap and the entry points are the resamplers' common ones (vstab_resample.hpp, vstab_warp_host.hpp).  This
// unit holds the cubic table, the cubic blend, the constant border's tile (k_warp_cubic) and the kernels under their names.
#include "vstab_cubic.hpp"
#include "vstab_warp_host.hpp"

namespace vstab {

__device__ const CubicTable g_cubic = make_cubic_table();  // in the code object's read-only data: loaded with the kernels

// the 16 weights of an entry as 8 packed int16 pairs (two 16-byte loads, cache-resident): pair 2 r + h = row r, columns 2 h (low half) and
// 2 h + 1
__device__ __forceinline__ void cubic_weights(int f, uint32_t (&w)[8]) {
    const uint4 *p = reinterpret_cast<const uint4 *>(g_cubic.w) + 2 * f;
    const uint4 a = p[0], b = p[1];
    w[0] = a.x, w[1] = a.y, w[2] = a.z, w[3] = a.w, w[4] = b.x, w[5] = b.y, w[6] = b.z, w[7] = b.w;
}

// the constant border's 16 taps: from the staged box (16 LDS reads), or from the source itself when the box was not staged
template <typename T, typename Src>
__device__ __forceinline__ void cubic_taps(const Src &s, const TileBox &b, const T *lds, const CubicTap &t, uint32_t (&v)[16]) {
    if (b.lds) {
        const int at = (t.Y - 1 - b.y0) * b.w + (t.X - 1 - b.x0);
        const T *q = lds + at;
#pragma unroll
        for (int r = 0; r < 4; r++) lds_row<4>(q + r * b.w, v + 4 * r);
    } else {
#pragma unroll
        for (int r = 0; r < 4; r++)
#pragma unroll
            for (int c = 0; c < 4; c++) v[4 * r + c] = s.row_col(t.X - 1 + c, t.Y - 1 + r);
    }
}

struct Cubic {
    static constexpr int K = 4, LO = 1;
    // some tap of the footprint inside a w x h source
    __device__ __forceinline__ static bool touches(const CubicTap &t, int w, int h) { return t.X + 2 >= 0 && t.X - 1 < w && t.Y + 2 >= 0 && t.Y - 1 < h; }
    // all 16 taps, then channel by channel
    template <int CN, typename Rows>
    __device__ __forceinline__ static uint32_t blend(const Rows &rows, int f) {
        uint32_t w[8], v[16];
        cubic_weights(f, w);
#pragma unroll
        for (int r = 0; r < 4; r++) {
            uint32_t row[4];
            rows(r, row);
#pragma unroll
            for (int c = 0; c < 4; c++) v[4 * r + c] = row[c];
        }
        return channels<CN>(v, w);
    }
    template <int CN>
    __device__ __forceinline__ static uint32_t channels(const uint32_t (&v)[16], const uint32_t (&w)[8]) {
        uint32_t out = cubic_channel<0>(v, w);
        if constexpr (CN > 1) out |= cubic_channel<1>(v, w) << 8;
        if constexpr (CN > 2) out |= cubic_channel<2>(v, w) << 16;
        return out;
    }
};

// k_warp_cubic -- NV12 in; PLANAR false: BGR8 out (cvtColor then cv::remap INTER_CUBIC, border 0); PLANAR true: the plane-wise warp
// (luma border 16; chroma at the even pixels' positions halved, border (128, 128)).
// The tile's phases (vstab_resample.hpp) with what the constant border alone has: only footprints that touch the source enter the box, a
// tile with none has no box, a pixel whose footprint does not touch is the border value.  Kept apart from resample_tile because through it
// and the trait's row functor the compiler's instruction counts for these kernels rose ("After the consolidation").
template <int MODE, bool PLANAR>
__global__ void __launch_bounds__(256) k_warp_cubic(CubicArgs c) {
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
        if (Cubic::touches(t[j], a.sw, a.sh)) mnx = min(mnx, t[j].X), mxx = max(mxx, t[j].X), mny = min(mny, t[j].Y), mxy = max(mxy, t[j].Y);
    if constexpr (!PLANAR) {
        const BorderNv12Bgr<VSTAB_BORDER_CONSTANT> src = {a.y, a.uv, a.pitch_y, a.pitch_uv, a.sw, a.sh};
        uint32_t *lds = reinterpret_cast<uint32_t *>(stage);
        const TileBox b = tile_box<1, 4, false>(mnx, mxx, mny, mxy, red, RESAMPLE_LDS_BYTES / 4);
        // 3. stage
        if (b.lds) stage_box<VSTAB_BORDER_CONSTANT, false>(src, b, lds);
        __syncthreads();
        // 4. blend
#pragma unroll
        for (int j = 0; j < RESAMPLE_RW; j++) {
            const int y = y0 + j;
            if (x >= a.dw || y >= a.dh) continue;
            uint32_t B = 0, G = 0, R = 0;
            if (Cubic::touches(t[j], a.sw, a.sh)) {
                uint32_t v[16], w[8];
                cubic_weights(t[j].f, w);
                cubic_taps(src, b, lds, t[j], v);
                B = cubic_channel<0>(v, w), G = cubic_channel<1>(v, w), R = cubic_channel<2>(v, w);
            }
            uint8_t *o = a.dst + (size_t)y * a.pitch_dst + (size_t)x * 3;
            o[0] = (uint8_t)B, o[1] = (uint8_t)G, o[2] = (uint8_t)R;
        }
    } else {
        // chroma sample (x / 2, y / 2) of every even output pixel: the map halved (exact) and quantised again
        const int cw = a.sw >> 1, ch = a.sh >> 1;
        const bool cact = !(lane & 1);
        int cmnx = INT_MAX, cmxx = INT_MIN, cmny = INT_MAX, cmxy = INT_MIN;
#pragma unroll
        for (int k = 0; k < RESAMPLE_RW / 2; k++) {
            tc[k] = cubic_tap(ax[2 * k] * 0.5f, ay[2 * k] * 0.5f);
            if (cact && Cubic::touches(tc[k], cw, ch))
                cmnx = min(cmnx, tc[k].X), cmxx = max(cmxx, tc[k].X), cmny = min(cmny, tc[k].Y), cmxy = max(cmxy, tc[k].Y);
        }
        const BorderBytes<1, VSTAB_BORDER_CONSTANT> sy = {a.y, a.pitch_y, a.sw, a.sh, 16u};
        const BorderBytes<2, VSTAB_BORDER_CONSTANT> suv = {a.uv, a.pitch_uv, cw, ch, 0x8080u};
        uint8_t *lds_y = stage;                                                     // luma bytes: half the budget
        uint16_t *lds_c = reinterpret_cast<uint16_t *>(stage + RESAMPLE_LDS_BYTES / 2);  // chroma pairs: the other half
        const TileBox by = tile_box<1, 4, false>(mnx, mxx, mny, mxy, red, RESAMPLE_LDS_BYTES / 2);
        const TileBox bc = tile_box<1, 4, false>(cmnx, cmxx, cmny, cmxy, red, RESAMPLE_LDS_BYTES / 4);
        if (by.lds) stage_box<VSTAB_BORDER_CONSTANT, false>(sy, by, lds_y);
        if (bc.lds) stage_box<VSTAB_BORDER_CONSTANT, false>(suv, bc, lds_c);
        __syncthreads();
#pragma unroll
        for (int j = 0; j < RESAMPLE_RW; j++) {
            const int y = y0 + j;
            if (x >= a.dw || y >= a.dh) continue;
            uint32_t Y = 16;
            if (Cubic::touches(t[j], a.sw, a.sh)) {
                uint32_t v[16], w[8];
                cubic_weights(t[j].f, w);
                cubic_taps(sy, by, lds_y, t[j], v);
                Y = cubic_channel<0>(v, w);
            }
            a.dst[(size_t)y * a.pitch_dst + x] = (uint8_t)Y;
            if (cact && !(j & 1)) {
                const CubicTap &q = tc[j / 2];
                uint32_t U = 128, V = 128;
                if (Cubic::touches(q, cw, ch)) {
                    uint32_t v[16], w[8];
                    cubic_weights(q.f, w);
                    cubic_taps(suv, bc, lds_c, q, v);
                    U = cubic_channel<0>(v, w), V = cubic_channel<1>(v, w);
                }
                uint8_t *o = a.dst_uv + (size_t)(y >> 1) * a.pitch_dst_uv + (size_t)x;  // chroma sample x / 2: bytes x, x + 1
                o[0] = (uint8_t)U, o[1] = (uint8_t)V;
            }
        }
    }
}

// k_warp_cubic_border -- the warp with border mode BORDER (REPLICATE, REFLECT, REFLECT_101); k_remap_cubic / k_remap_cubic_border -- the
// stateless remap, constant border (value border) / border mode BORDER
template <int MODE, bool PLANAR, int BORDER>
__global__ void __launch_bounds__(256) k_warp_cubic_border(CubicArgs c) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[RESAMPLE_LDS_BYTES];
    __shared__ __attribute__((aligned(16))) int red[16];
    resample_tile<Cubic, MODE, PLANAR, BORDER>(c, stage, red);
}
template <int CN>
__global__ void __launch_bounds__(256) k_remap_cubic(VSTAB_REMAP_PARAMS, uint32_t border, VSTAB_REMAP_DST) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= dw || y >= dh) return;
    const float mx = reinterpret_cast<const float *>(reinterpret_cast<const uint8_t *>(mapx) + (size_t)y * pitch_x)[x];
    const float my = reinterpret_cast<const float *>(reinterpret_cast<const uint8_t *>(mapy) + (size_t)y * pitch_y)[x];
    const CubicTap t = cubic_tap(mx * 32.0f, my * 32.0f);
    uint32_t out = border;
    if (Cubic::touches(t, sw, sh)) {
        const BorderBytes<CN, VSTAB_BORDER_CONSTANT> s = {src, pitch_src, sw, sh, border};
        const TileBox none = {0, 0, 0, 0, false};
        uint32_t v[16], w[8];
        cubic_weights(t.f, w);
        cubic_taps(s, none, (const uint32_t *)nullptr, t, v);
        out = Cubic::channels<CN>(v, w);
    }
    uint8_t *o = dst + (size_t)y * pitch_dst + (size_t)x * CN;
    o[0] = (uint8_t)out;
    if constexpr (CN > 1) o[1] = (uint8_t)(out >> 8);
    if constexpr (CN > 2) o[2] = (uint8_t)(out >> 16);
}
template <int CN, int BORDER>
__global__ void __launch_bounds__(256) k_remap_cubic_border(VSTAB_REMAP_PARAMS, VSTAB_REMAP_DST) {
    remap_pixel<Cubic, CN, BORDER>(src, pitch_src, sw, sh, mapx, pitch_x, mapy, pitch_y, dst, pitch_dst, dw, dh);
}

// k_warp_cubic_rs -- the warp with a rotation per output row (vstab_warp_nv12_rs_ex; map modes 0, 1, 5 and MAP_RS_FISHD_TO_RECT), every
// border mode, BORDER_CONSTANT included: resample_tile_rs (vstab_resample.hpp).  MAP_RECTD_TO_RECT / _FISH (vstab_warp_nv12_pinhole): the
// same tile with one rotation and the rectilinear lens's five coefficients, which travel in BorderArgs
template <int MODE, bool PLANAR, int BORDER>
__global__ void __launch_bounds__(256) k_warp_cubic_rs(BorderArgs ba) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[RESAMPLE_LDS_BYTES];
    __shared__ __attribute__((aligned(16))) int red[16];
    resample_tile_rs<Cubic, MODE, PLANAR, BORDER>(ba, stage, red);
}

struct CubicKernels {
    template <int MODE, bool PLANAR, int BORDER>
    static auto warp() {
        if constexpr (BORDER == VSTAB_BORDER_CONSTANT) return k_warp_cubic<MODE, PLANAR>;
        else return k_warp_cubic_border<MODE, PLANAR, BORDER>;
    }
    template <int MODE, bool PLANAR, int BORDER>
    static auto warp_rs() {
        return k_warp_cubic_rs<MODE, PLANAR, BORDER>;
    }
    template <int CN, int BORDER>
    static auto remap() {
        if constexpr (BORDER == VSTAB_BORDER_CONSTANT) return k_remap_cubic<CN>;
        else return k_remap_cubic_border<CN, BORDER>;
    }
};

// Kernels of this translation unit (and the weight table with them) are one code object: see preload_warp_kernels
vstab_status preload_cubic_kernels() {
    hipFuncAttributes at;
    VSTAB_HIP_TRY(hipFuncGetAttributes(&at, reinterpret_cast<const void *>(&k_remap_cubic<1>)));
    return VSTAB_OK;
}

vstab_status launch_warp_cubic(const BorderArgs &ba, const WarpRoute &r, int out_format, int border_mode, void *stream) {
    return launch_warp_resample<CubicKernels>(ba, r, out_format, border_mode, stream);
}

}  // namespace vstab

using namespace vstab;

extern "C" {

vstab_status vstab_cubic_weights(int16_t *out) {
    static constexpr CubicTable tab = make_cubic_table();
    if (!out) return fail(VSTAB_ERR_INVALID, "vstab_cubic_weights: null pointer");
    for (int i = 0; i < CUBIC_TAB * 16; i++) out[i] = tab.w[i];
    return VSTAB_OK;
}

vstab_status vstab_remap_cubic(const void *src, size_t pitch_src, int sw, int sh, int channels, const void *map_x, size_t pitch_x, const void *map_y,
                               size_t pitch_y, const int border[3], void *dst, size_t pitch_dst, int dw, int dh, void *stream) {
    return remap_resample<CubicKernels>("vstab_remap_cubic", src, pitch_src, sw, sh, channels, map_x, pitch_x, map_y, pitch_y, nullptr, border, dst,
                                        pitch_dst, dw, dh, stream);
}

vstab_status vstab_remap_cubic_border(const void *src, size_t pitch_src, int sw, int sh, int channels, const void *map_x, size_t pitch_x,
                                      const void *map_y, size_t pitch_y, int border_mode, const int border[3], void *dst, size_t pitch_dst, int dw,
                                      int dh, void *stream) {
    return remap_resample<CubicKernels>("vstab_remap_cubic_border", src, pitch_src, sw, sh, channels, map_x, pitch_x, map_y, pitch_y, &border_mode, border,
                                        dst, pitch_dst, dw, dh, stream);
}

vstab_status vstab_warp_nv12_cubic(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int sw, int sh, const float params[17], int map_mode,
                                   int out_format, void *dst, size_t pitch_dst, void *dst_uv, size_t pitch_dst_uv, int dw, int dh, void *stream) {
    return warp_nv12({.e = ENTRY_CUBIC, .y = y, .pitch_y = pitch_y, .uv = uv, .pitch_uv = pitch_uv, .sw = sw, .sh = sh, .params = params, .map_mode = map_mode,
                      .resample = VSTAB_RESAMPLE_CUBIC, .out_format = out_format, .dst = dst, .pitch_dst = pitch_dst, .dst_uv = dst_uv, .pitch_dst_uv = pitch_dst_uv,
                      .dw = dw, .dh = dh, .stream = stream});
}

vstab_status vstab_warp_nv12_cubic_border(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int sw, int sh, const float params[17],
                                          int map_mode, int out_format, int border_mode, void *dst, size_t pitch_dst, void *dst_uv, size_t pitch_dst_uv, int dw, int dh,
                                          void *stream) {
    return warp_nv12({.e = ENTRY_CUBIC_BORDER, .y = y, .pitch_y = pitch_y, .uv = uv, .pitch_uv = pitch_uv, .sw = sw, .sh = sh, .params = params,
                      .map_mode = map_mode, .resample = VSTAB_RESAMPLE_CUBIC, .border_mode = border_mode, .out_format = out_format, .dst = dst,
                      .pitch_dst = pitch_dst, .dst_uv = dst_uv, .pitch_dst_uv = pitch_dst_uv, .dw = dw, .dh = dh, .stream = stream});
}

}  // extern "C"
