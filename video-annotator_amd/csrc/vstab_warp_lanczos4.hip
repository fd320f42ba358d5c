// vstab_warp_lanczos4.hip -- cv::remap's INTER_LANCZOS4 for gfx950: the fused NV12 -> BGR8 warp, the plane-wise NV12 -> NV12 warp and the
// stateless remap of map planes.  Definition (include/vstab.h, vstab_warp_nv12_lanczos4; tests/lanczos4_def.py): the map quantised to 1/32
// pixel as for INTER_LINEAR, an 8 x 8 footprint at (X - 3 .. X + 4, Y - 3 .. Y + 4), 64 integer weights from OpenCV's fixed-point table
// (vstab_lanczos4.hpp), border value substituted for each tap outside the source, (sum + 2^14) >> 15 saturated to 0..255.
//
// The warp kernels (k_warp_lanczos4) follow k_warp_cubic (vstab_warp_cubic.hip) phase for phase, on 64 x 16 output tiles, one workgroup of
// 256 threads each, four rows per thread:
//   1. map      the exact map of the thread's four pixels in registers (k_quantised_map's arithmetic for every mode), quantised;
//   2. box      the tile's source box: min / max of the footprints that touch the source, reduced over the workgroup -- exact, not probed;
//   3. stage    the box read into LDS once per source pixel, converted (BGRx dwords; luma bytes / chroma pairs in the plane-wise
//               kernel), the border value in every position outside the source;
//   4. blend    row by row, 8 LDS reads per footprint row, each at its natural alignment (ds_read2_b32 pairs of BGRx dwords; one
//               ds_read_u8 per luma tap, one ds_read_u16 per chroma pair), the row's 8 weights as one 16-byte load from the table,
//               v_dot2_i32_i16 on channel pairs gathered by v_perm_b32: four per row, 32 per channel.
// A box over the LDS budget is sampled from global memory instead; so is every pixel of the stateless remap.  The table is 128 KiB, four
// times the L1: the rows of an entry a pixel reads depend on its fractions only, and neighbouring pixels share fy.
#include <hip/hip_ext.h>

#include "vstab_internal.hpp"
#include "vstab_lanczos4.hpp"
#include "vstab_resample.hpp"

namespace vstab {

__device__ const Lanczos4Table g_lanczos4 = make_lanczos4_table();  // in the code object's read-only data: loaded with the kernels

constexpr int LZ_TW = 64, LZ_TH = 16, LZ_RW = 4;  // tile; rows per thread (4 waves x 4 rows)
constexpr int LZ_LDS_BYTES = 24 * 1024;           // stage budget per workgroup: six workgroups per CU by LDS

// some tap of the footprint inside a w x h source
__device__ __forceinline__ bool lz_touches(const CubicTap &t, int w, int h) { return t.X + 4 >= 0 && t.X - 3 < w && t.Y + 4 >= 0 && t.Y - 3 < h; }

// row r of an entry's weights: 8 int16 as 4 packed pairs, pair h = columns 2 h (low half) and 2 h + 1
__device__ __forceinline__ uint4 lz_weights(int f, int r) { return reinterpret_cast<const uint4 *>(g_lanczos4.w)[8 * f + r]; }

// ---------------------------------------------------------------------------------------------------------------------
// The tile's phases.
// ---------------------------------------------------------------------------------------------------------------------
struct Lanczos4Box {
    int x0, y0, w, h;
    bool lds;  // staged (uniform over the workgroup)
};

// min / max of the tap columns and rows over the footprints a thread passes in (any that touch the source), reduced over the workgroup
// through red[16] in LDS.  The box covers X - 3 .. X + 4 of all of them; it lies inside [-7, w + 6] x [-7, h + 6].
__device__ __forceinline__ Lanczos4Box lz_box(int mnx, int mxx, int mny, int mxy, int *red, int cap_elems) {
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
    const bool have = mnx <= mxx;  // else no footprint of the tile touches the source
    Lanczos4Box b;
    b.x0 = mnx - 3, b.y0 = mny - 3, b.w = have ? mxx - mnx + 8 : 0, b.h = have ? mxy - mny + 8 : 0;
    b.lds = have && (long)b.w * b.h <= cap_elems;
    return b;
}

template <typename T, typename Src>
__device__ __forceinline__ void lz_stage(const Src &s, const Lanczos4Box &b, T *lds) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int r = wave; r < b.h; r += 4)
        for (int c = lane; c < b.w; c += 64) lds[r * b.w + c] = (T)s(b.x0 + c, b.y0 + r);
}

// the 8 taps of footprint row r: from the staged box, or from the source itself when the box was not staged
template <typename T, typename Src>
__device__ __forceinline__ void lz_taps(const Src &s, const Lanczos4Box &b, const T *lds, const CubicTap &t, int r, uint32_t (&v)[8]) {
    if (b.lds) {
        const int at = (t.Y - 3 + r - b.y0) * b.w + (t.X - 3 - b.x0);
        if constexpr (sizeof(T) < 4) {
            // luma bytes / chroma pairs: one ds_read_u8 / ds_read_u16 per tap, at its natural alignment.  Volatile, because the compiler
            // otherwise merges the adjacent taps of a row into ds_read_b32 / ds_read_b64 at a 1- or 2-byte boundary, which gfx950 executes
            // lane by lane: 64 cycles instead of 2.3 (profiles/r05_lds_access_cost.txt)
            typedef __attribute__((address_space(3))) T LdsT;
            const volatile LdsT *q = (const volatile LdsT *)(lds + at);
#pragma unroll
            for (int c = 0; c < 8; c++) v[c] = q[c];
        } else {  // BGRx dwords: 4-byte aligned whatever the tap, so the compiler's ds_read2_b32 pairs are aligned too
            const T *q = lds + at;
#pragma unroll
            for (int c = 0; c < 8; c++) v[c] = q[c];
        }
    } else {
#pragma unroll
        for (int c = 0; c < 8; c++) v[c] = s(t.X - 3 + c, t.Y - 3 + r);
    }
}

// The blend of one footprint: channels 0 .. CN - 1 of the output, one byte each
template <int CN, typename T, typename Src>
__device__ __forceinline__ uint32_t lz_blend(const Src &s, const Lanczos4Box &b, const T *lds, const CubicTap &t) {
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
template <int MODE, bool PLANAR>
__global__ void __launch_bounds__(256) k_warp_lanczos4(CubicArgs c) {
    const WarpArgs &a = c.w;
    __shared__ __attribute__((aligned(16))) uint8_t stage[LZ_LDS_BYTES];
    __shared__ __attribute__((aligned(16))) int red[16];  // read back as ds_read_b96 / ds_read2_b32: 16-byte aligned
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = blockIdx.x * LZ_TW + lane, y0 = blockIdx.y * LZ_TH + wave * LZ_RW;
    const float rfx = rcp_refined(a.p.ofx), rfy = rcp_refined(a.p.ofy);
    // 1. map (pixels right of / below the image are evaluated as the last column / row: never stored, inside the box)
    CubicTap t[LZ_RW], tc[LZ_RW / 2];
    float ax[LZ_RW], ay[LZ_RW];
#pragma unroll
    for (int j = 0; j < LZ_RW; j++) {
        cubic_map<MODE>(c, min(x, a.dw - 1), min(y0 + j, a.dh - 1), rfx, rfy, ax[j], ay[j]);
        t[j] = cubic_tap(ax[j], ay[j]);
    }
    // 2. box of the luma / BGR taps
    int mnx = INT_MAX, mxx = INT_MIN, mny = INT_MAX, mxy = INT_MIN;
#pragma unroll
    for (int j = 0; j < LZ_RW; j++)
        if (lz_touches(t[j], a.sw, a.sh)) mnx = min(mnx, t[j].X), mxx = max(mxx, t[j].X), mny = min(mny, t[j].Y), mxy = max(mxy, t[j].Y);
    if constexpr (!PLANAR) {
        const SrcNv12Bgr src = {a.y, a.uv, a.pitch_y, a.pitch_uv, a.sw, a.sh};
        uint32_t *lds = reinterpret_cast<uint32_t *>(stage);
        const Lanczos4Box b = lz_box(mnx, mxx, mny, mxy, red, LZ_LDS_BYTES / 4);
        // 3. stage
        if (b.lds) lz_stage(src, b, lds);
        __syncthreads();
        // 4. blend
#pragma unroll
        for (int j = 0; j < LZ_RW; j++) {
            const int y = y0 + j;
            if (x >= a.dw || y >= a.dh) continue;
            const uint32_t bgr = lz_touches(t[j], a.sw, a.sh) ? lz_blend<3>(src, b, (const uint32_t *)lds, t[j]) : 0u;
            uint8_t *o = a.dst + (size_t)y * a.pitch_dst + (size_t)x * 3;
            o[0] = (uint8_t)bgr, o[1] = (uint8_t)(bgr >> 8), o[2] = (uint8_t)(bgr >> 16);
        }
    } else {
        // chroma sample (x / 2, y / 2) of every even output pixel: the map halved (exact) and quantised again
        const int cw = a.sw >> 1, ch = a.sh >> 1;
        const bool cact = !(lane & 1);
        int cmnx = INT_MAX, cmxx = INT_MIN, cmny = INT_MAX, cmxy = INT_MIN;
#pragma unroll
        for (int k = 0; k < LZ_RW / 2; k++) {
            tc[k] = cubic_tap(ax[2 * k] * 0.5f, ay[2 * k] * 0.5f);
            if (cact && lz_touches(tc[k], cw, ch))
                cmnx = min(cmnx, tc[k].X), cmxx = max(cmxx, tc[k].X), cmny = min(cmny, tc[k].Y), cmxy = max(cmxy, tc[k].Y);
        }
        const SrcBytes<1> sy = {a.y, a.pitch_y, a.sw, a.sh, 16u};
        const SrcBytes<2> suv = {a.uv, a.pitch_uv, cw, ch, 0x8080u};
        uint8_t *lds_y = stage;                                                  // luma bytes: half the budget
        uint16_t *lds_c = reinterpret_cast<uint16_t *>(stage + LZ_LDS_BYTES / 2);  // chroma pairs: the other half
        const Lanczos4Box by = lz_box(mnx, mxx, mny, mxy, red, LZ_LDS_BYTES / 2);
        const Lanczos4Box bc = lz_box(cmnx, cmxx, cmny, cmxy, red, LZ_LDS_BYTES / 4);
        if (by.lds) lz_stage(sy, by, lds_y);
        if (bc.lds) lz_stage(suv, bc, lds_c);
        __syncthreads();
#pragma unroll
        for (int j = 0; j < LZ_RW; j++) {
            const int y = y0 + j;
            if (x >= a.dw || y >= a.dh) continue;
            const uint32_t Y = lz_touches(t[j], a.sw, a.sh) ? lz_blend<1>(sy, by, (const uint8_t *)lds_y, t[j]) : 16u;
            a.dst[(size_t)y * a.pitch_dst + x] = (uint8_t)Y;
            if (cact && !(j & 1)) {
                const CubicTap &q = tc[j / 2];
                const uint32_t UV = lz_touches(q, cw, ch) ? lz_blend<2>(suv, bc, (const uint16_t *)lds_c, q) : 0x8080u;
                uint8_t *o = a.dst_uv + (size_t)(y >> 1) * a.pitch_dst_uv + (size_t)x;  // chroma sample x / 2: bytes x, x + 1
                o[0] = (uint8_t)UV, o[1] = (uint8_t)(UV >> 8);
            }
        }
    }
}

// k_remap_lanczos4 -- cv::remap(INTER_LANCZOS4, BORDER_CONSTANT border) of CN interleaved 8-bit channels with float map planes: the
// stateless building block (any map, NaN / huge / tie entries included).  One thread per output pixel, taps from global memory.
template <int CN>
__global__ void __launch_bounds__(256) k_remap_lanczos4(const uint8_t *__restrict__ src, size_t pitch_src, int sw, int sh, const float *__restrict__ mapx,
                                                        size_t pitch_x, const float *__restrict__ mapy, size_t pitch_y, uint32_t border,
                                                        uint8_t *__restrict__ dst, size_t pitch_dst, int dw, int dh) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= dw || y >= dh) return;
    const float mx = reinterpret_cast<const float *>(reinterpret_cast<const uint8_t *>(mapx) + (size_t)y * pitch_x)[x];
    const float my = reinterpret_cast<const float *>(reinterpret_cast<const uint8_t *>(mapy) + (size_t)y * pitch_y)[x];
    const CubicTap t = cubic_tap(mx * 32.0f, my * 32.0f);
    uint32_t out = border;
    if (lz_touches(t, sw, sh)) {
        const SrcBytes<CN> s = {src, pitch_src, sw, sh, border};
        const Lanczos4Box none = {0, 0, 0, 0, false};
        out = lz_blend<CN>(s, none, (const uint32_t *)nullptr, t);
    }
    uint8_t *o = dst + (size_t)y * pitch_dst + (size_t)x * CN;
    o[0] = (uint8_t)out;
    if constexpr (CN > 1) o[1] = (uint8_t)(out >> 8);
    if constexpr (CN > 2) o[2] = (uint8_t)(out >> 16);
}

// Kernels of this translation unit (and the weight table with them) are one code object: see preload_warp_kernels
vstab_status preload_lanczos4_kernels() {
    hipFuncAttributes at;
    VSTAB_HIP_TRY(hipFuncGetAttributes(&at, reinterpret_cast<const void *>(&k_remap_lanczos4<1>)));
    return VSTAB_OK;
}

template <int MODE, bool PLANAR>
static void launch_warp_lanczos4(const CubicArgs &c, dim3 grid, const LaunchEvents &ev, hipStream_t st) {
    auto kernel = k_warp_lanczos4<MODE, PLANAR>;
    if (ev.start) hipExtLaunchKernelGGL(kernel, grid, dim3(256), 0, st, ev.start, ev.stop, 0, c);
    else hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, c);
}

static inline bool lz_aligned(const void *p, size_t a) { return (reinterpret_cast<uintptr_t>(p) % a) == 0; }

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
    if (!src || !map_x || !map_y || !dst || !border) return fail(VSTAB_ERR_INVALID, "vstab_remap_lanczos4: null pointer");
    if (channels < 1 || channels > 3) return fail(VSTAB_ERR_INVALID, "vstab_remap_lanczos4: channels must be 1, 2 or 3");
    if (sw <= 0 || sh <= 0 || dw <= 0 || dh <= 0 || sw > 32767 || sh > 32767 || dw > 32767 || dh > 32767)
        return fail(VSTAB_ERR_INVALID, "vstab_remap_lanczos4: sizes must be in [1, 32767]");
    if (pitch_src < (size_t)sw * channels || pitch_dst < (size_t)dw * channels || pitch_x < (size_t)dw * 4 || pitch_y < (size_t)dw * 4 || pitch_x % 4 ||
        pitch_y % 4 || !lz_aligned(map_x, 4) || !lz_aligned(map_y, 4))
        return fail(VSTAB_ERR_INVALID, "vstab_remap_lanczos4: pitch smaller than a row, or map planes not 4-byte aligned");
    uint32_t b = 0;
    for (int k = 0; k < channels; k++) {
        if (border[k] < 0 || border[k] > 255) return fail(VSTAB_ERR_INVALID, "vstab_remap_lanczos4: border values must be in [0, 255]");
        b |= (uint32_t)border[k] << (8 * k);
    }
    const dim3 grid(div_up(dw, 64), div_up(dh, 4));
    hipStream_t s = static_cast<hipStream_t>(stream);
#define VSTAB_LAUNCH(CN)                                                                                                                      \
    hipLaunchKernelGGL(k_remap_lanczos4<CN>, grid, dim3(256), 0, s, (const uint8_t *)src, pitch_src, sw, sh, (const float *)map_x, pitch_x, \
                       (const float *)map_y, pitch_y, b, (uint8_t *)dst, pitch_dst, dw, dh)
    if (channels == 1) VSTAB_LAUNCH(1);
    else if (channels == 2) VSTAB_LAUNCH(2);
    else VSTAB_LAUNCH(3);
#undef VSTAB_LAUNCH
    VSTAB_HIP_TRY(hipGetLastError());
    return VSTAB_OK;
}

vstab_status vstab_warp_nv12_lanczos4(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int sw, int sh, const float params[17],
                                      int map_mode, int out_format, void *dst, size_t pitch_dst, void *dst_uv, size_t pitch_dst_uv, int dw, int dh,
                                      void *stream) {
    if (!y || !uv || !dst || !params) return fail(VSTAB_ERR_INVALID, "vstab_warp_nv12_lanczos4: null pointer");
    if (sw <= 0 || sh <= 0 || (sw & 1) || (sh & 1) || sw > 32767 || sh > 32767)
        return fail(VSTAB_ERR_INVALID, "vstab_warp_nv12_lanczos4: source must be even-sized and <= 32767");
    if (dw <= 0 || dh <= 0 || dw > 32767 || dh > 32767) return fail(VSTAB_ERR_INVALID, "vstab_warp_nv12_lanczos4: output size must be in [1, 32767]");
    if (map_mode < VSTAB_MAP_CREATEMAP_CL || map_mode > VSTAB_MAP_CREATEMAP_CL_OPENCL)
        return fail(VSTAB_ERR_INVALID, "vstab_warp_nv12_lanczos4: unknown map mode");
    if (out_format != VSTAB_OUT_BGR8 && out_format != VSTAB_OUT_NV12_PLANAR)
        return fail(VSTAB_ERR_INVALID,
                    "vstab_warp_nv12_lanczos4: the Lanczos warp emits VSTAB_OUT_BGR8 or VSTAB_OUT_NV12_PLANAR (NV12 through BGR is not served)");
    const bool planar = out_format == VSTAB_OUT_NV12_PLANAR;
    if (pitch_y < (size_t)sw || pitch_uv < (size_t)sw || pitch_dst < (size_t)dw * (planar ? 1 : 3))
        return fail(VSTAB_ERR_INVALID, "vstab_warp_nv12_lanczos4: pitch smaller than row");
    if (planar && (!dst_uv || pitch_dst_uv < (size_t)((dw + 1) / 2) * 2))
        return fail(VSTAB_ERR_INVALID, "vstab_warp_nv12_lanczos4: plane-wise output needs a chroma plane of 2*ceil(width/2) bytes per row");
    if (!lz_aligned(uv, 2) || pitch_uv % 2) return fail(VSTAB_ERR_INVALID, "vstab_warp_nv12_lanczos4: chroma plane must be 2-B aligned");
    CubicArgs c;
    WarpArgs &a = c.w;
    a.y = (const uint8_t *)y, a.uv = (const uint8_t *)uv, a.dst = (uint8_t *)dst, a.dst_uv = planar ? (uint8_t *)dst_uv : nullptr;
    a.pitch_y = pitch_y, a.pitch_uv = pitch_uv, a.pitch_dst = pitch_dst, a.pitch_dst_uv = planar ? pitch_dst_uv : 0;
    a.sw = sw, a.sh = sh, a.dw = dw, a.dh = dh;
    MapParams &p = a.p;
    p.icx = params[0], p.icy = params[1], p.ifx = params[2], p.ify = params[3];
    p.ocx = params[4], p.ocy = params[5], p.ofx = params[6], p.ofy = params[7];
    for (int i = 0; i < 9; i++) p.r[i] = params[8 + i];
    c.p32 = {params[0] * 32.0f, params[1] * 32.0f, params[2] * 32.0f, params[3] * 32.0f, params[10], params[13], params[16]};
    const dim3 grid(div_up(dw, LZ_TW), div_up(dh, LZ_TH));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const LaunchEvents ev = take_launch_events();  // a profiling caller's pair: the kernel's own start / end stamps
#define VSTAB_MODES(P)                                                                                    \
    switch (map_mode) {                                                                                   \
        case VSTAB_MAP_CREATEMAP_CL: launch_warp_lanczos4<MAP_CREATEMAP_CL, P>(c, grid, ev, st); break;   \
        case VSTAB_MAP_FISH_TO_RECT: launch_warp_lanczos4<MAP_FISH_TO_RECT, P>(c, grid, ev, st); break;   \
        case VSTAB_MAP_FISH_TO_FISH: launch_warp_lanczos4<MAP_FISH_TO_FISH, P>(c, grid, ev, st); break;   \
        case VSTAB_MAP_RECT_TO_RECT: launch_warp_lanczos4<MAP_RECT_TO_RECT, P>(c, grid, ev, st); break;   \
        case VSTAB_MAP_RECT_TO_FISH: launch_warp_lanczos4<MAP_RECT_TO_FISH, P>(c, grid, ev, st); break;   \
        default: launch_warp_lanczos4<MAP_CREATEMAP_CL_OPENCL, P>(c, grid, ev, st); break;                \
    }
    if (planar) VSTAB_MODES(true)
    else VSTAB_MODES(false)
#undef VSTAB_MODES
    VSTAB_HIP_TRY(hipGetLastError());
    return VSTAB_OK;
}

}  // extern "C"
