// vstab_warp_border.hip -- cv::remap's INTER_LINEAR with a border mode for gfx950: the fused NV12 -> BGR8 warp, the plane-wise NV12 -> NV12
// warp and the stateless remap of map planes.  Definition (include/vstab.h, vstab_warp_nv12_border; tests/warp_def.py): the map quantised
// to 1/32 pixel and blended as the bilinear warp does it ((sum of four products + 512) >> 10), each of the four taps (X + i, Y + j) read at
// (borderInterpolate(X + i, w), borderInterpolate(Y + j, h)) -- BORDER_REPLICATE, BORDER_REFLECT, BORDER_REFLECT_101 -- or, BORDER_CONSTANT,
// the border value where it lies outside the source.
//
// The warp kernels (k_warp_border) follow the resamplers' tile (vstab_resample.hpp) with the pieces it is made of -- the sources, the box, the
// staging, the row read -- and a tap, a map and a blend of their own: the tap carries its computed weights and, for the constant border,
// is clamped where it lies wholly outside; the map may take a rotation per output row.  64 x 16 output tiles, one workgroup of 256
// threads, four rows per thread:
//   1. map      the exact map of the thread's four pixels in registers (k_quantised_map's arithmetic for every mode; the per-row rotation of
//               vstab_warp_nv12_rs where RS), quantised;
//   2. box      min / max of X .. X + 1 and Y .. Y + 1 over every pixel of the tile, reduced over the workgroup, in VIRTUAL coordinates: a
//               reflected border has no pixel "wholly outside", so a tile far outside the source still reads (mirrored) picture;
//   3. stage    each virtual position of the box read once through borderInterpolate, converted (BGRx dwords; luma bytes / chroma pairs in
//               the plane-wise kernel);
//   4. blend    4 LDS reads per pixel at their natural alignment, v_dot2_i32_i16 on channel pairs gathered by v_perm_b32.
// A box over the LDS budget (the axis pixel of map mode 0 at -32768, strong minification) is sampled from global memory with the same
// arithmetic; so is every pixel of the stateless remap.
#include "vstab_warp_host.hpp"

namespace vstab {

// The tap, its read (border_taps) and its blend (border_channel) are in vstab_resample.hpp: the keep-edge kernels (vstab_warp_keep.hip)
// share them.
//
// k_warp_border -- NV12 in; PLANAR false: BGR8 out (cvtColor then cv::remap INTER_LINEAR, border mode BORDER; CONSTANT value 0); PLANAR
// true: the plane-wise warp (luma; chroma at the even pixels' positions halved over the chroma plane's own size; CONSTANT values 16 and
// (128, 128)).  MODE: map modes 0 .. 5, RS with modes 0 / 1 / 5 and with MAP_RS_FISHD_TO_RECT (the calibrated lens, map mode 1); without RS
// also MAP_RECTD_TO_RECT / _FISH (a rectilinear lens's five coefficients in ba.pd, map modes 3 / 4).
template <int MODE, bool PLANAR, bool RS, int BORDER>
__global__ void __launch_bounds__(256) k_warp_border(BorderArgs ba) {
    const WarpArgs &a = ba.c.w;
    __shared__ __attribute__((aligned(16))) uint8_t stage[RESAMPLE_LDS_BYTES];
    __shared__ __attribute__((aligned(16))) int red[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = blockIdx.x * RESAMPLE_TW + lane, y0 = blockIdx.y * RESAMPLE_TH + wave * RESAMPLE_RW;
    const float rfx = rcp_refined(a.p.ofx), rfy = rcp_refined(a.p.ofy);
    // 1. map (pixels right of / below the image are evaluated as the last column / row: never stored, inside the box)
    BorderTap t[RESAMPLE_RW];
    float ax[RESAMPLE_RW], ay[RESAMPLE_RW];
#pragma unroll
    for (int j = 0; j < RESAMPLE_RW; j++) {
        border_map<MODE, RS>(ba, min(x, a.dw - 1), min(y0 + j, a.dh - 1), rfx, rfy, ax[j], ay[j]);
        t[j] = border_tap<BORDER>(ax[j], ay[j], a.sw, a.sh);
    }
    // 2. box of the luma / BGR taps: every pixel, no "touches the source" filter
    int mnx = INT_MAX, mxx = INT_MIN, mny = INT_MAX, mxy = INT_MIN;
#pragma unroll
    for (int j = 0; j < RESAMPLE_RW; j++) mnx = min(mnx, t[j].X), mxx = max(mxx, t[j].X), mny = min(mny, t[j].Y), mxy = max(mxy, t[j].Y);
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
            uint32_t v[4];
            border_taps<BORDER>(src, b, lds, t[j], v);
            uint8_t *o = a.dst + (size_t)y * a.pitch_dst + (size_t)x * 3;
            o[0] = (uint8_t)border_channel<0>(v[0], v[1], v[2], v[3], t[j]);
            o[1] = (uint8_t)border_channel<1>(v[0], v[1], v[2], v[3], t[j]);
            o[2] = (uint8_t)border_channel<2>(v[0], v[1], v[2], v[3], t[j]);
        }
    } else {
        // chroma sample (x / 2, y / 2) of every even output pixel: the map halved (exact) and quantised again, over the chroma plane's size
        const int cw = a.sw >> 1, ch = a.sh >> 1;
        const bool cact = !(lane & 1);
        BorderTap tc[RESAMPLE_RW / 2];
        int cmnx = INT_MAX, cmxx = INT_MIN, cmny = INT_MAX, cmxy = INT_MIN;
#pragma unroll
        for (int k = 0; k < RESAMPLE_RW / 2; k++) {
            tc[k] = border_tap<BORDER>(ax[2 * k] * 0.5f, ay[2 * k] * 0.5f, cw, ch);
            if (cact) cmnx = min(cmnx, tc[k].X), cmxx = max(cmxx, tc[k].X), cmny = min(cmny, tc[k].Y), cmxy = max(cmxy, tc[k].Y);
        }
        const BorderBytes<1, BORDER> sy = {a.y, a.pitch_y, a.sw, a.sh, 16u};
        const BorderBytes<2, BORDER> suv = {a.uv, a.pitch_uv, cw, ch, 0x8080u};
        uint8_t *lds_y = stage;                                                      // luma bytes: half the budget
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
            uint32_t v[4];
            border_taps<BORDER>(sy, by, lds_y, t[j], v);
            a.dst[(size_t)y * a.pitch_dst + x] = (uint8_t)border_channel<0>(v[0], v[1], v[2], v[3], t[j]);
            if (cact && !(j & 1)) {
                const BorderTap &q = tc[j / 2];
                border_taps<BORDER>(suv, bc, lds_c, q, v);
                uint8_t *o = a.dst_uv + (size_t)(y >> 1) * a.pitch_dst_uv + (size_t)x;  // chroma sample x / 2: bytes x, x + 1
                o[0] = (uint8_t)border_channel<0>(v[0], v[1], v[2], v[3], q), o[1] = (uint8_t)border_channel<1>(v[0], v[1], v[2], v[3], q);
            }
        }
    }
}

// k_remap_border -- cv::remap(INTER_LINEAR, BORDER) of CN interleaved 8-bit channels with float map planes (CONSTANT value 0): the stateless
// building block (any map, NaN / huge / tie entries included).  One thread per output pixel, taps from global memory.
template <int CN, int BORDER>
__global__ void __launch_bounds__(256) k_remap_border(const uint8_t *__restrict__ src, size_t pitch_src, int sw, int sh, const float *__restrict__ mapx,
                                                      size_t pitch_x, const float *__restrict__ mapy, size_t pitch_y, uint8_t *__restrict__ dst,
                                                      size_t pitch_dst, int dw, int dh) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= dw || y >= dh) return;
    const float mx = reinterpret_cast<const float *>(reinterpret_cast<const uint8_t *>(mapx) + (size_t)y * pitch_x)[x];
    const float my = reinterpret_cast<const float *>(reinterpret_cast<const uint8_t *>(mapy) + (size_t)y * pitch_y)[x];
    const BorderTap t = border_tap<BORDER>(mx * 32.0f, my * 32.0f, sw, sh);
    const BorderBytes<CN, BORDER> s = {src, pitch_src, sw, sh, 0u};
    const TileBox none = {0, 0, 0, 0, false};
    uint32_t v[4];
    border_taps<BORDER>(s, none, (const uint32_t *)nullptr, t, v);
    uint8_t *o = dst + (size_t)y * pitch_dst + (size_t)x * CN;
    o[0] = (uint8_t)border_channel<0>(v[0], v[1], v[2], v[3], t);
    if constexpr (CN > 1) o[1] = (uint8_t)border_channel<1>(v[0], v[1], v[2], v[3], t);
    if constexpr (CN > 2) o[2] = (uint8_t)border_channel<2>(v[0], v[1], v[2], v[3], t);
}

// Kernels of this translation unit are one code object: see preload_warp_kernels
vstab_status preload_border_kernels() {
    hipFuncAttributes at;
    VSTAB_HIP_TRY(hipFuncGetAttributes(&at, reinterpret_cast<const void *>(&k_remap_border<1, VSTAB_BORDER_CONSTANT>)));
    return VSTAB_OK;
}

// k_warp_border of a route (WARP_BORDER) on its grid.  What is instantiated is what is served: the map modes 0 .. 5 with every border mode,
// and with a rotation per output row for modes 0, 1 and 5; a calibrated fisheye lens (ba.c.p32.d) with one rotation under a non-constant
// border (INTER_LINEAR with the constant border is k_warp_fused / k_warp_planar) and, as MAP_RS_FISHD_TO_RECT, with a rotation per row under
// every border mode; a rectilinear lens (ba.pd) with one rotation under every border mode.
vstab_status launch_warp_border(const BorderArgs &ba, const WarpRoute &r, int out_format, int border_mode, void *stream) {
    with_kernel_mode(route_kernel_mode(r.mode), [&](auto mode) {
        with_border_mode(border_mode, [&](auto border) {
            with_bool(out_format == VSTAB_OUT_NV12_PLANAR, [&](auto planar) {
                with_bool(map_mode_is_rs(r.mode), [&](auto rs_c) {
                    constexpr int MODE = decltype(mode)::value, BORDER = decltype(border)::value;
                    constexpr bool RS = decltype(rs_c)::value;
                    constexpr bool served = MODE == MAP_RS_FISHD_TO_RECT ? RS
                                            : ModeTraits<MODE>::rectd    ? !RS
                                            : ModeTraits<MODE>::dist     ? !RS && BORDER != VSTAB_BORDER_CONSTANT
                                                                         : MODE <= MAP_CREATEMAP_CL_OPENCL && (!RS || map_mode_fish_to_pinhole(MODE));
                    if constexpr (served) launch_tiles(k_warp_border<MODE, decltype(planar)::value, RS, BORDER>, ba, ba.c.w.dw, ba.c.w.dh, stream);
                });
            });
        });
    });
    VSTAB_HIP_TRY(hipGetLastError());
    return VSTAB_OK;
}

}  // namespace vstab

using namespace vstab;

extern "C" {

vstab_status vstab_remap_bilinear_border(const void *src, size_t pitch_src, int sw, int sh, int channels, const void *map_x, size_t pitch_x,
                                         const void *map_y, size_t pitch_y, int border_mode, void *dst, size_t pitch_dst, int dw, int dh,
                                         void *stream) {
    uint32_t none;
    const vstab_status st = check_remap("vstab_remap_bilinear_border", src, pitch_src, sw, sh, channels, map_x, pitch_x, map_y, pitch_y, &border_mode, false,
                                        nullptr, dst, pitch_dst, dw, dh, none);
    if (st != VSTAB_OK) return st;
    const dim3 grid(div_up(dw, 64), div_up(dh, 4));
    hipStream_t s = static_cast<hipStream_t>(stream);
    with_channels(channels, [&](auto cn) {
        with_border_mode(border_mode, [&](auto border) {
            hipLaunchKernelGGL((k_remap_border<decltype(cn)::value, decltype(border)::value>), grid, dim3(256), 0, s, (const uint8_t *)src, pitch_src, sw, sh,
                               (const float *)map_x, pitch_x, (const float *)map_y, pitch_y, (uint8_t *)dst, pitch_dst, dw, dh);
        });
    });
    VSTAB_HIP_TRY(hipGetLastError());
    return VSTAB_OK;
}

vstab_status vstab_warp_nv12_border(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int sw, int sh, const float params[17],
                                    const float *rot_bottom, int map_mode, int out_format, int border_mode, void *dst, size_t pitch_dst, void *dst_uv,
                                    size_t pitch_dst_uv, int dw, int dh, void *stream) {
    return warp_nv12({.e = ENTRY_BORDER, .y = y, .pitch_y = pitch_y, .uv = uv, .pitch_uv = pitch_uv, .sw = sw, .sh = sh, .params = params, .rot_bottom = rot_bottom,
                      .map_mode = map_mode, .border_mode = border_mode, .out_format = out_format, .dst = dst, .pitch_dst = pitch_dst, .dst_uv = dst_uv,
                      .pitch_dst_uv = pitch_dst_uv, .dw = dw, .dh = dh, .stream = stream});
}

}  // extern "C"
