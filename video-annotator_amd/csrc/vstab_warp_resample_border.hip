// vstab_warp_resample_border.hip -- cv::remap's INTER_CUBIC and INTER_LANCZOS4 with a border mode for gfx950: the fused NV12 -> BGR8 warp,
// the plane-wise NV12 -> NV12 warp and the stateless remap of map planes.  Definition (include/vstab.h, "Border modes of the cubic and Lanczos
// resamplers"; tests/resample_border_def.py): the map quantised to 1/32 pixel, the K x K footprint (X - LO + i, Y - LO + j) -- K = 4, LO = 1
// for cubic; K = 8, LO = 3 for Lanczos -- each tap read at (borderInterpolate(x, w), borderInterpolate(y, h)), BORDER_REPLICATE,
// BORDER_REFLECT or BORDER_REFLECT_101, the weights of the resampler's table, (sum + 2^14) >> 15 saturated.  BORDER_CONSTANT is not served
// here: the entry points hand it to the constant-border kernels (vstab_warp_cubic.hip, vstab_warp_lanczos4.hip), whose bytes it is.
//
// The warp kernels (k_warp_cubic_border, k_warp_lanczos4_border) follow k_warp_border's scheme (vstab_warp_border.hip) on 64 x 16 output
// tiles, one workgroup of 256 threads, four rows per thread:
//   1. map      the exact map of the thread's four pixels in registers (k_quantised_map's arithmetic for every mode), quantised;
//   2. box      min / max of the whole footprint over every pixel of the tile, reduced over the workgroup, in virtual coordinates;
//   3. stage    each virtual position of the box read once: as it is where the box lies inside the source, else through borderInterpolate
//               once per column for all its rows (vstab_border.hpp, border_stage);
//   4. blend    the constant-border kernels' blend from LDS: K reads per footprint row at their natural alignment (volatile narrow reads of
//               luma bytes and chroma pairs), v_dot2_i32_i16 against the table's weight pairs.
// A box over the LDS budget is sampled from global memory, each tap folded; so is every pixel of the stateless remap.  This code object
// carries its own copies of the two weight tables.
#include <climits>

#include <hip/hip_ext.h>

#include "vstab_border.hpp"
#include "vstab_cubic.hpp"
#include "vstab_internal.hpp"
#include "vstab_lanczos4.hpp"
#include "vstab_resample.hpp"

namespace vstab {

__device__ const CubicTable g_rb_cubic = make_cubic_table();           // in this code object's read-only data: loaded with its kernels
__device__ const Lanczos4Table g_rb_lanczos4 = make_lanczos4_table();

constexpr int RB_TW = 64, RB_TH = 16, RB_RW = 4;  // tile; rows per thread (4 waves x 4 rows)
constexpr int RB_LDS_BYTES = 24 * 1024;           // stage budget per workgroup, as the constant-border kernels'

// ---------------------------------------------------------------------------------------------------------------------
// Footprint rows: rows(r, v) fills v[0 .. K - 1] with the taps of footprint row r -- from the staged box, or from the source itself when the
// box was not staged (uniform over the workgroup), each tap folded.
// ---------------------------------------------------------------------------------------------------------------------
template <int BORDER, int K, int LO, typename T, typename Src>
struct RbRows {
    const Src &s;
    BorderBox b;
    const T *lds;
    int X, Y;  // the tap (by value: a reference into the thread's tap array kept that array in scratch)
    __device__ __forceinline__ void operator()(int r, uint32_t (&v)[K]) const {
        if (b.lds) {
            const int at = (Y - LO + r - b.y0) * b.w + (X - LO - b.x0);
            if constexpr (sizeof(T) < 4) {
                // luma bytes / chroma pairs: one ds_read_u8 / ds_read_u16 per tap at its natural alignment (volatile: the compiler otherwise
                // merges adjacent taps into misaligned wide reads, executed lane by lane -- profiles/r05_lds_access_cost.txt)
                typedef __attribute__((address_space(3))) T LdsT;
                const volatile LdsT *q = (const volatile LdsT *)(lds + at);
#pragma unroll
                for (int c = 0; c < K; c++) v[c] = q[c];
            } else {  // BGRx dwords
                const T *q = lds + at;
#pragma unroll
                for (int c = 0; c < K; c++) v[c] = q[c];
            }
        } else {
            const int sy = border_index<BORDER>(Y - LO + r, s.h);
#pragma unroll
            for (int c = 0; c < K; c++) v[c] = s.at(border_index<BORDER>(X - LO + c, s.w), sy);
        }
    }
};

// ---------------------------------------------------------------------------------------------------------------------
// The resamplers: footprint and blend (channels 0 .. CN - 1 of the output, one byte each).
// ---------------------------------------------------------------------------------------------------------------------
struct RbCubic {
    static constexpr int K = 4, LO = 1;
    template <int CN, typename Rows>
    __device__ __forceinline__ static uint32_t blend(const Rows &rows, int f) {  // k_warp_cubic's: all 16 taps, then channel by channel
        const uint4 *p = reinterpret_cast<const uint4 *>(g_rb_cubic.w) + 2 * f;
        const uint4 a = p[0], b = p[1];
        const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        uint32_t v[16];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            uint32_t row[4];
            rows(r, row);
#pragma unroll
            for (int c = 0; c < 4; c++) v[4 * r + c] = row[c];
        }
        uint32_t out = cubic_channel<0>(v, w);
        if constexpr (CN > 1) out |= cubic_channel<1>(v, w) << 8;
        if constexpr (CN > 2) out |= cubic_channel<2>(v, w) << 16;
        return out;
    }
};
struct RbLanczos4 {
    static constexpr int K = 8, LO = 3;
    template <int CN, typename Rows>
    __device__ __forceinline__ static uint32_t blend(const Rows &rows, int f) {  // k_warp_lanczos4's: row by row, the row's 8 weights at once
        int acc0 = 1 << 14, acc1 = 1 << 14, acc2 = 1 << 14;
#pragma unroll
        for (int r = 0; r < 8; r++) {
            uint32_t v[8];
            const uint4 w = reinterpret_cast<const uint4 *>(g_rb_lanczos4.w)[8 * f + r];
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

// one output sample
template <typename R, int CN, int BORDER, typename T, typename Src>
__device__ __forceinline__ uint32_t rb_sample(const Src &s, const BorderBox &b, const T *lds, const CubicTap &t) {
    const RbRows<BORDER, R::K, R::LO, T, Src> rows = {s, b, lds, t.X, t.Y};
    return R::template blend<CN>(rows, t.f);
}

// the footprint's first column / row and the one before its last, for border_box (which adds 2)
template <typename R>
__device__ __forceinline__ void rb_extent(const CubicTap &t, int &mnx, int &mxx, int &mny, int &mxy) {
    mnx = min(mnx, t.X - R::LO), mxx = max(mxx, t.X - R::LO + R::K - 2);
    mny = min(mny, t.Y - R::LO), mxy = max(mxy, t.Y - R::LO + R::K - 2);
}

// The warp of one tile.  PLANAR false: BGR8 out (cvtColor then cv::remap with the resampler and border mode BORDER); PLANAR true: the
// plane-wise warp (luma; chroma at the even pixels' positions halved, folded over the chroma plane's own size).
template <typename R, int MODE, bool PLANAR, int BORDER>
__device__ __forceinline__ void rb_warp(const CubicArgs &c, uint8_t *stage, int *red) {
    static_assert(BORDER != VSTAB_BORDER_CONSTANT, "BORDER_CONSTANT is served by k_warp_cubic / k_warp_lanczos4");
    const WarpArgs &a = c.w;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = blockIdx.x * RB_TW + lane, y0 = blockIdx.y * RB_TH + wave * RB_RW;
    const float rfx = rcp_refined(a.p.ofx), rfy = rcp_refined(a.p.ofy);
    // 1. map (pixels right of / below the image are evaluated as the last column / row: never stored, inside the box)
    CubicTap t[RB_RW];
    float ax[RB_RW], ay[RB_RW];
#pragma unroll
    for (int j = 0; j < RB_RW; j++) {
        cubic_map<MODE>(c, min(x, a.dw - 1), min(y0 + j, a.dh - 1), rfx, rfy, ax[j], ay[j]);
        t[j] = cubic_tap(ax[j], ay[j]);
    }
    // 2. box of the luma / BGR footprints: every pixel, no "touches the source" filter
    int mnx = INT_MAX, mxx = INT_MIN, mny = INT_MAX, mxy = INT_MIN;
#pragma unroll
    for (int j = 0; j < RB_RW; j++) rb_extent<R>(t[j], mnx, mxx, mny, mxy);
    if constexpr (!PLANAR) {
        const BorderNv12Bgr<BORDER> src = {a.y, a.uv, a.pitch_y, a.pitch_uv, a.sw, a.sh};
        uint32_t *lds = reinterpret_cast<uint32_t *>(stage);
        const BorderBox b = border_box(mnx, mxx, mny, mxy, red, RB_LDS_BYTES / 4);
        // 3. stage
        if (b.lds) border_stage<BORDER>(src, b, lds);
        __syncthreads();
        // 4. blend
#pragma unroll
        for (int j = 0; j < RB_RW; j++) {
            const int y = y0 + j;
            if (x >= a.dw || y >= a.dh) continue;
            const uint32_t bgr = rb_sample<R, 3, BORDER>(src, b, (const uint32_t *)lds, t[j]);
            uint8_t *o = a.dst + (size_t)y * a.pitch_dst + (size_t)x * 3;
            o[0] = (uint8_t)bgr, o[1] = (uint8_t)(bgr >> 8), o[2] = (uint8_t)(bgr >> 16);
        }
    } else {
        // chroma sample (x / 2, y / 2) of every even output pixel: the map halved (exact) and quantised again, over the chroma plane's size
        const int cw = a.sw >> 1, ch = a.sh >> 1;
        const bool cact = !(lane & 1);
        CubicTap tc[RB_RW / 2];
        int cmnx = INT_MAX, cmxx = INT_MIN, cmny = INT_MAX, cmxy = INT_MIN;
#pragma unroll
        for (int k = 0; k < RB_RW / 2; k++) {
            tc[k] = cubic_tap(ax[2 * k] * 0.5f, ay[2 * k] * 0.5f);
            if (cact) rb_extent<R>(tc[k], cmnx, cmxx, cmny, cmxy);
        }
        const BorderBytes<1, BORDER> sy = {a.y, a.pitch_y, a.sw, a.sh, 0u};
        const BorderBytes<2, BORDER> suv = {a.uv, a.pitch_uv, cw, ch, 0u};
        uint8_t *lds_y = stage;                                                   // luma bytes: half the budget
        uint16_t *lds_c = reinterpret_cast<uint16_t *>(stage + RB_LDS_BYTES / 2);  // chroma pairs: the other half
        const BorderBox by = border_box(mnx, mxx, mny, mxy, red, RB_LDS_BYTES / 2);
        const BorderBox bc = border_box(cmnx, cmxx, cmny, cmxy, red, RB_LDS_BYTES / 4);
        if (by.lds) border_stage<BORDER>(sy, by, lds_y);
        if (bc.lds) border_stage<BORDER>(suv, bc, lds_c);
        __syncthreads();
#pragma unroll
        for (int j = 0; j < RB_RW; j++) {
            const int y = y0 + j;
            if (x >= a.dw || y >= a.dh) continue;
            a.dst[(size_t)y * a.pitch_dst + x] = (uint8_t)rb_sample<R, 1, BORDER>(sy, by, (const uint8_t *)lds_y, t[j]);
            if (cact && !(j & 1)) {
                const uint32_t UV = rb_sample<R, 2, BORDER>(suv, bc, (const uint16_t *)lds_c, tc[j / 2]);
                uint8_t *o = a.dst_uv + (size_t)(y >> 1) * a.pitch_dst_uv + (size_t)x;  // chroma sample x / 2: bytes x, x + 1
                o[0] = (uint8_t)UV, o[1] = (uint8_t)(UV >> 8);
            }
        }
    }
}

// k_warp_cubic_border / k_warp_lanczos4_border -- NV12 in, the warp with border mode BORDER (REPLICATE, REFLECT, REFLECT_101); MODE: map
// modes 0 .. 5
template <int MODE, bool PLANAR, int BORDER>
__global__ void __launch_bounds__(256) k_warp_cubic_border(CubicArgs c) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[RB_LDS_BYTES];
    __shared__ __attribute__((aligned(16))) int red[16];
    rb_warp<RbCubic, MODE, PLANAR, BORDER>(c, stage, red);
}
template <int MODE, bool PLANAR, int BORDER>
__global__ void __launch_bounds__(256) k_warp_lanczos4_border(CubicArgs c) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[RB_LDS_BYTES];
    __shared__ __attribute__((aligned(16))) int red[16];
    rb_warp<RbLanczos4, MODE, PLANAR, BORDER>(c, stage, red);
}

// k_remap_cubic_border / k_remap_lanczos4_border -- cv::remap(resampler, BORDER) of CN interleaved 8-bit channels with float map planes: the
// stateless building block (any map, NaN / huge / tie entries included).  One thread per output pixel, taps from global memory.
template <typename R, int CN, int BORDER>
__device__ __forceinline__ void rb_remap(const uint8_t *__restrict__ src, size_t pitch_src, int sw, int sh, const float *__restrict__ mapx, size_t pitch_x,
                                         const float *__restrict__ mapy, size_t pitch_y, uint8_t *__restrict__ dst, size_t pitch_dst, int dw, int dh) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= dw || y >= dh) return;
    const float mx = reinterpret_cast<const float *>(reinterpret_cast<const uint8_t *>(mapx) + (size_t)y * pitch_x)[x];
    const float my = reinterpret_cast<const float *>(reinterpret_cast<const uint8_t *>(mapy) + (size_t)y * pitch_y)[x];
    const CubicTap t = cubic_tap(mx * 32.0f, my * 32.0f);
    const BorderBytes<CN, BORDER> s = {src, pitch_src, sw, sh, 0u};
    const BorderBox none = {0, 0, 0, 0, false};
    const uint32_t out = rb_sample<R, CN, BORDER>(s, none, (const uint32_t *)nullptr, t);
    uint8_t *o = dst + (size_t)y * pitch_dst + (size_t)x * CN;
    o[0] = (uint8_t)out;
    if constexpr (CN > 1) o[1] = (uint8_t)(out >> 8);
    if constexpr (CN > 2) o[2] = (uint8_t)(out >> 16);
}
#define VSTAB_RB_REMAP_ARGS                                                                                                                   \
    const uint8_t *__restrict__ src, size_t pitch_src, int sw, int sh, const float *__restrict__ mapx, size_t pitch_x, const float *__restrict__ mapy, \
        size_t pitch_y, uint8_t *__restrict__ dst, size_t pitch_dst, int dw, int dh
template <int CN, int BORDER>
__global__ void __launch_bounds__(256) k_remap_cubic_border(VSTAB_RB_REMAP_ARGS) {
    rb_remap<RbCubic, CN, BORDER>(src, pitch_src, sw, sh, mapx, pitch_x, mapy, pitch_y, dst, pitch_dst, dw, dh);
}
template <int CN, int BORDER>
__global__ void __launch_bounds__(256) k_remap_lanczos4_border(VSTAB_RB_REMAP_ARGS) {
    rb_remap<RbLanczos4, CN, BORDER>(src, pitch_src, sw, sh, mapx, pitch_x, mapy, pitch_y, dst, pitch_dst, dw, dh);
}
#undef VSTAB_RB_REMAP_ARGS

// Kernels of this translation unit (and the weight tables with them) are one code object: see preload_warp_kernels
vstab_status preload_resample_border_kernels() {
    hipFuncAttributes at;
    VSTAB_HIP_TRY(hipFuncGetAttributes(&at, reinterpret_cast<const void *>(&k_remap_cubic_border<1, VSTAB_BORDER_REPLICATE>)));
    return VSTAB_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Launchers: the resampler's kernel of a (map mode, output, border mode)
// ---------------------------------------------------------------------------------------------------------------------
template <bool LZ, int MODE, bool PLANAR, int BORDER>
static void launch_rb_warp(const CubicArgs &c, dim3 grid, const LaunchEvents &ev, hipStream_t st) {
    auto kernel = LZ ? k_warp_lanczos4_border<MODE, PLANAR, BORDER> : k_warp_cubic_border<MODE, PLANAR, BORDER>;
    if (ev.start) hipExtLaunchKernelGGL(kernel, grid, dim3(256), 0, st, ev.start, ev.stop, 0, c);
    else hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, c);
}

template <bool LZ, bool PLANAR, int BORDER>
static void launch_rb_warp_mode(const CubicArgs &c, int map_mode, dim3 grid, const LaunchEvents &ev, hipStream_t st) {
    switch (map_mode) {
        case VSTAB_MAP_CREATEMAP_CL: launch_rb_warp<LZ, MAP_CREATEMAP_CL, PLANAR, BORDER>(c, grid, ev, st); break;
        case VSTAB_MAP_FISH_TO_RECT: launch_rb_warp<LZ, MAP_FISH_TO_RECT, PLANAR, BORDER>(c, grid, ev, st); break;
        case VSTAB_MAP_FISH_TO_FISH: launch_rb_warp<LZ, MAP_FISH_TO_FISH, PLANAR, BORDER>(c, grid, ev, st); break;
        case VSTAB_MAP_RECT_TO_RECT: launch_rb_warp<LZ, MAP_RECT_TO_RECT, PLANAR, BORDER>(c, grid, ev, st); break;
        case VSTAB_MAP_RECT_TO_FISH: launch_rb_warp<LZ, MAP_RECT_TO_FISH, PLANAR, BORDER>(c, grid, ev, st); break;
        default: launch_rb_warp<LZ, MAP_CREATEMAP_CL_OPENCL, PLANAR, BORDER>(c, grid, ev, st); break;
    }
}

template <bool LZ, bool PLANAR>
static void launch_rb_warp_any(const CubicArgs &c, int map_mode, int border_mode, dim3 grid, const LaunchEvents &ev, hipStream_t st) {
    switch (border_mode) {
        case VSTAB_BORDER_REPLICATE: launch_rb_warp_mode<LZ, PLANAR, VSTAB_BORDER_REPLICATE>(c, map_mode, grid, ev, st); break;
        case VSTAB_BORDER_REFLECT: launch_rb_warp_mode<LZ, PLANAR, VSTAB_BORDER_REFLECT>(c, map_mode, grid, ev, st); break;
        default: launch_rb_warp_mode<LZ, PLANAR, VSTAB_BORDER_REFLECT_101>(c, map_mode, grid, ev, st); break;
    }
}

template <bool LZ, int CN, int BORDER>
static void launch_rb_remap(dim3 grid, hipStream_t s, const void *src, size_t pitch_src, int sw, int sh, const void *map_x, size_t pitch_x,
                            const void *map_y, size_t pitch_y, void *dst, size_t pitch_dst, int dw, int dh) {
    auto kernel = LZ ? k_remap_lanczos4_border<CN, BORDER> : k_remap_cubic_border<CN, BORDER>;
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, (const uint8_t *)src, pitch_src, sw, sh, (const float *)map_x, pitch_x, (const float *)map_y,
                       pitch_y, (uint8_t *)dst, pitch_dst, dw, dh);
}

template <bool LZ, int CN>
static void launch_rb_remap_any(int border_mode, dim3 grid, hipStream_t s, const void *src, size_t pitch_src, int sw, int sh, const void *map_x,
                                size_t pitch_x, const void *map_y, size_t pitch_y, void *dst, size_t pitch_dst, int dw, int dh) {
    switch (border_mode) {
        case VSTAB_BORDER_REPLICATE:
            launch_rb_remap<LZ, CN, VSTAB_BORDER_REPLICATE>(grid, s, src, pitch_src, sw, sh, map_x, pitch_x, map_y, pitch_y, dst, pitch_dst, dw, dh);
            break;
        case VSTAB_BORDER_REFLECT:
            launch_rb_remap<LZ, CN, VSTAB_BORDER_REFLECT>(grid, s, src, pitch_src, sw, sh, map_x, pitch_x, map_y, pitch_y, dst, pitch_dst, dw, dh);
            break;
        default:
            launch_rb_remap<LZ, CN, VSTAB_BORDER_REFLECT_101>(grid, s, src, pitch_src, sw, sh, map_x, pitch_x, map_y, pitch_y, dst, pitch_dst, dw, dh);
            break;
    }
}

static inline bool rb_aligned(const void *p, size_t a) { return (reinterpret_cast<uintptr_t>(p) % a) == 0; }

// vstab_remap_{cubic,lanczos4}_border: every argument checked, CONSTANT handed to the constant-border entry point
template <bool LZ>
static vstab_status remap_resample_border(const char *name, const void *src, size_t pitch_src, int sw, int sh, int channels, const void *map_x,
                                          size_t pitch_x, const void *map_y, size_t pitch_y, int border_mode, const int border[3], void *dst,
                                          size_t pitch_dst, int dw, int dh, void *stream) {
    const std::string n = name;
    if (!src || !map_x || !map_y || !dst) return fail(VSTAB_ERR_INVALID, n + ": null pointer");
    if (channels < 1 || channels > 3) return fail(VSTAB_ERR_INVALID, n + ": channels must be 1, 2 or 3");
    if (sw <= 0 || sh <= 0 || dw <= 0 || dh <= 0 || sw > 32767 || sh > 32767 || dw > 32767 || dh > 32767)
        return fail(VSTAB_ERR_INVALID, n + ": sizes must be in [1, 32767]");
    if (pitch_src < (size_t)sw * channels || pitch_dst < (size_t)dw * channels || pitch_x < (size_t)dw * 4 || pitch_y < (size_t)dw * 4 || pitch_x % 4 ||
        pitch_y % 4 || !rb_aligned(map_x, 4) || !rb_aligned(map_y, 4))
        return fail(VSTAB_ERR_INVALID, n + ": pitch smaller than a row, or map planes not 4-byte aligned");
    if (!border_mode_valid(border_mode))
        return fail(VSTAB_ERR_INVALID, n + ": border_mode must be VSTAB_BORDER_CONSTANT (0), _REPLICATE (1), _REFLECT (2) or _REFLECT_101 (4)");
    if (border_mode == VSTAB_BORDER_CONSTANT) {
        if (!border) return fail(VSTAB_ERR_INVALID, n + ": VSTAB_BORDER_CONSTANT needs the border values");
        return LZ ? vstab_remap_lanczos4(src, pitch_src, sw, sh, channels, map_x, pitch_x, map_y, pitch_y, border, dst, pitch_dst, dw, dh, stream)
                  : vstab_remap_cubic(src, pitch_src, sw, sh, channels, map_x, pitch_x, map_y, pitch_y, border, dst, pitch_dst, dw, dh, stream);
    }
    const dim3 grid(div_up(dw, 64), div_up(dh, 4));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (channels == 1) launch_rb_remap_any<LZ, 1>(border_mode, grid, s, src, pitch_src, sw, sh, map_x, pitch_x, map_y, pitch_y, dst, pitch_dst, dw, dh);
    else if (channels == 2) launch_rb_remap_any<LZ, 2>(border_mode, grid, s, src, pitch_src, sw, sh, map_x, pitch_x, map_y, pitch_y, dst, pitch_dst, dw, dh);
    else launch_rb_remap_any<LZ, 3>(border_mode, grid, s, src, pitch_src, sw, sh, map_x, pitch_x, map_y, pitch_y, dst, pitch_dst, dw, dh);
    VSTAB_HIP_TRY(hipGetLastError());
    return VSTAB_OK;
}

// vstab_warp_nv12_{cubic,lanczos4}_border: the argument rules of vstab_warp_nv12_cubic / vstab_warp_nv12_border, all checked before any launch
template <bool LZ>
static vstab_status warp_resample_border(const char *name, const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int sw, int sh,
                                         const float params[17], int map_mode, int out_format, int border_mode, void *dst, size_t pitch_dst,
                                         void *dst_uv, size_t pitch_dst_uv, int dw, int dh, void *stream) {
    const std::string n = name;
    if (!y || !uv || !dst || !params) return fail(VSTAB_ERR_INVALID, n + ": null pointer");
    if (sw <= 0 || sh <= 0 || (sw & 1) || (sh & 1) || sw > 32767 || sh > 32767)
        return fail(VSTAB_ERR_INVALID, n + ": source must be even-sized and <= 32767");
    if (dw <= 0 || dh <= 0 || dw > 32767 || dh > 32767) return fail(VSTAB_ERR_INVALID, n + ": output size must be in [1, 32767]");
    if (map_mode < VSTAB_MAP_CREATEMAP_CL || map_mode > VSTAB_MAP_CREATEMAP_CL_OPENCL) return fail(VSTAB_ERR_INVALID, n + ": unknown map mode");
    if (out_format != VSTAB_OUT_BGR8 && out_format != VSTAB_OUT_NV12_PLANAR)
        return fail(VSTAB_ERR_INVALID, n + ": emits VSTAB_OUT_BGR8 or VSTAB_OUT_NV12_PLANAR (NV12 through BGR is not served)");
    if (!border_mode_valid(border_mode))
        return fail(VSTAB_ERR_INVALID, n + ": border_mode must be VSTAB_BORDER_CONSTANT (0), _REPLICATE (1), _REFLECT (2) or _REFLECT_101 (4)");
    const bool planar = out_format == VSTAB_OUT_NV12_PLANAR;
    if (pitch_y < (size_t)sw || pitch_uv < (size_t)sw || pitch_dst < (size_t)dw * (planar ? 1 : 3))
        return fail(VSTAB_ERR_INVALID, n + ": pitch smaller than row");
    if (planar && (!dst_uv || pitch_dst_uv < (size_t)((dw + 1) / 2) * 2))
        return fail(VSTAB_ERR_INVALID, n + ": plane-wise output needs a chroma plane of 2*ceil(width/2) bytes per row");
    if (!rb_aligned(uv, 2) || pitch_uv % 2) return fail(VSTAB_ERR_INVALID, n + ": chroma plane must be 2-B aligned");
    if (border_mode == VSTAB_BORDER_CONSTANT)
        return LZ ? vstab_warp_nv12_lanczos4(y, pitch_y, uv, pitch_uv, sw, sh, params, map_mode, out_format, dst, pitch_dst, dst_uv, pitch_dst_uv, dw, dh,
                                             stream)
                  : vstab_warp_nv12_cubic(y, pitch_y, uv, pitch_uv, sw, sh, params, map_mode, out_format, dst, pitch_dst, dst_uv, pitch_dst_uv, dw, dh,
                                          stream);
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
    const dim3 grid(div_up(dw, RB_TW), div_up(dh, RB_TH));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const LaunchEvents ev = take_launch_events();  // a profiling caller's pair: the kernel's own start / end stamps
    if (planar) launch_rb_warp_any<LZ, true>(c, map_mode, border_mode, grid, ev, st);
    else launch_rb_warp_any<LZ, false>(c, map_mode, border_mode, grid, ev, st);
    VSTAB_HIP_TRY(hipGetLastError());
    return VSTAB_OK;
}

}  // namespace vstab

using namespace vstab;

extern "C" {

vstab_status vstab_remap_cubic_border(const void *src, size_t pitch_src, int sw, int sh, int channels, const void *map_x, size_t pitch_x,
                                      const void *map_y, size_t pitch_y, int border_mode, const int border[3], void *dst, size_t pitch_dst, int dw,
                                      int dh, void *stream) {
    return remap_resample_border<false>("vstab_remap_cubic_border", src, pitch_src, sw, sh, channels, map_x, pitch_x, map_y, pitch_y, border_mode,
                                        border, dst, pitch_dst, dw, dh, stream);
}

vstab_status vstab_remap_lanczos4_border(const void *src, size_t pitch_src, int sw, int sh, int channels, const void *map_x, size_t pitch_x,
                                         const void *map_y, size_t pitch_y, int border_mode, const int border[3], void *dst, size_t pitch_dst, int dw,
                                         int dh, void *stream) {
    return remap_resample_border<true>("vstab_remap_lanczos4_border", src, pitch_src, sw, sh, channels, map_x, pitch_x, map_y, pitch_y, border_mode,
                                       border, dst, pitch_dst, dw, dh, stream);
}

vstab_status vstab_warp_nv12_cubic_border(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int sw, int sh, const float params[17],
                                          int map_mode, int out_format, int border_mode, void *dst, size_t pitch_dst, void *dst_uv,
                                          size_t pitch_dst_uv, int dw, int dh, void *stream) {
    return warp_resample_border<false>("vstab_warp_nv12_cubic_border", y, pitch_y, uv, pitch_uv, sw, sh, params, map_mode, out_format, border_mode,
                                       dst, pitch_dst, dst_uv, pitch_dst_uv, dw, dh, stream);
}

vstab_status vstab_warp_nv12_lanczos4_border(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int sw, int sh, const float params[17],
                                             int map_mode, int out_format, int border_mode, void *dst, size_t pitch_dst, void *dst_uv,
                                             size_t pitch_dst_uv, int dw, int dh, void *stream) {
    return warp_resample_border<true>("vstab_warp_nv12_lanczos4_border", y, pitch_y, uv, pitch_uv, sw, sh, params, map_mode, out_format, border_mode,
                                      dst, pitch_dst, dst_uv, pitch_dst_uv, dw, dh, stream);
}

}  // extern "C"
