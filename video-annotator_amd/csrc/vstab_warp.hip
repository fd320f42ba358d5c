// vstab_warp.hip -- the bilinear NV12 warp's C entry points for gfx950 (MI355X): their argument checks, the choice between the direct-gather
// kernel, the fused tile kernel (vstab_warp_fused.hip) and the plane-wise kernel (vstab_warp_planar.hip), and the two direct-gather
// kernels themselves, k_warp_nv12_bgr and k_warp_nearest.  Compiled with -ffp-contract=off.
//
// HBM-bound gather work (no MFMA): coalesced wide stores, enough workgroups to fill 256 CUs, the map in registers.
#include <cstdlib>

#include "vstab_warp_host.hpp"

namespace vstab {

// =============================================================================================
// k_warp_nv12_bgr (v1, direct gather) -- the fused hot kernel:
//   createMap.cl:13-50  ->  remap quantisation (:306-312)  ->  4 NV12 taps converted with the
//   cvtColor arithmetic (:401)  ->  fixed-point bilinear blend  ->  BGR8.
// Converting each tap and then blending is exactly what the reference's cvtColor-then-remap
// sequence computes, so the output is bit-identical to the un-fused operators.
//
// Block = 16 x 16 threads; a thread owns 4 adjacent columns (12 output bytes = 3 dwords per
// row) and ROWS_PER_THREAD rows 16 apart, so the column terms of the rotated ray (and their
// divisions) are computed once per thread and the row terms once per row.
// =============================================================================================
constexpr int WARP_ROWS_PER_THREAD = 4;
constexpr int WARP_TILE_W = 64, WARP_TILE_H = 16 * WARP_ROWS_PER_THREAD;

__device__ __forceinline__ uint32_t warp_pixel(const WarpArgs &a, const ColTerm &ct, const RowTerm &rt) {
    float mx, my;
    map_pixel(a.p, ct, rt, mx, my);
    const Tap t = quantise(mx, my);
    if (t.far || t.X >= a.sw || t.X + 1 < 0 || t.Y >= a.sh || t.Y + 1 < 0) return 0;
    const int w00 = (32 - t.fx) * (32 - t.fy), w01 = t.fx * (32 - t.fy), w10 = (32 - t.fx) * t.fy,
              w11 = t.fx * t.fy;
    int b0, g0, r0, b1, g1, r1, b2, g2, r2, b3, g3, r3;
    fetch_tap(a, t.X, t.Y, b0, g0, r0);
    fetch_tap(a, t.X + 1, t.Y, b1, g1, r1);
    fetch_tap(a, t.X, t.Y + 1, b2, g2, r2);
    fetch_tap(a, t.X + 1, t.Y + 1, b3, g3, r3);
    const uint32_t B = (uint32_t)(b0 * w00 + b1 * w01 + b2 * w10 + b3 * w11 + 512) >> 10;
    const uint32_t G = (uint32_t)(g0 * w00 + g1 * w01 + g2 * w10 + g3 * w11 + 512) >> 10;
    const uint32_t R = (uint32_t)(r0 * w00 + r1 * w01 + r2 * w10 + r3 * w11 + 512) >> 10;
    return B | (G << 8) | (R << 16);
}

__global__ void __launch_bounds__(256) k_warp_nv12_bgr(WarpArgs a, int vec_ok) {
    const int x0 = blockIdx.x * WARP_TILE_W + threadIdx.x * 4;
    if (x0 >= a.dw) return;
    ColTerm ct[4];
#pragma unroll
    for (int i = 0; i < 4; i++) ct[i] = col_term(a.p, x0 + i);
#pragma unroll 1
    for (int j = 0; j < WARP_ROWS_PER_THREAD; j++) {
        const int y = blockIdx.y * WARP_TILE_H + j * 16 + threadIdx.y;
        if (y >= a.dh) break;
        const RowTerm rt = row_term(a.p, y);
        uint32_t px[4];
#pragma unroll
        for (int i = 0; i < 4; i++) px[i] = warp_pixel(a, ct[i], rt);
        uint8_t *o = a.dst + (size_t)y * a.pitch_dst + (size_t)x0 * 3;
        if (vec_ok && x0 + 4 <= a.dw) {
            uint32_t *o32 = reinterpret_cast<uint32_t *>(o);
            o32[0] = px[0] | (px[1] << 24);
            o32[1] = (px[1] >> 8) | (px[2] << 16);
            o32[2] = (px[2] >> 16) | (px[3] << 8);
        } else {
            for (int i = 0; i < 4 && x0 + i < a.dw; i++) {
                o[3 * i] = px[i] & 255, o[3 * i + 1] = (px[i] >> 8) & 255, o[3 * i + 2] = (px[i] >> 16) & 255;
            }
        }
    }
}

// k_warp_nearest -- the fused warp with cv::remap's INTER_NEAREST (FrameSourceWarp.hpp:90 admits the flag, :311 passes it
// on; the reference itself only ever passes INTER_LINEAR): createMap.cl's map, cvRound (half to even) + saturate_cast<short>
// per coordinate, ONE tap converted with the cvtColor arithmetic, 0 outside the source.  Direct gather: this mode is
// about completeness, the bilinear kernel carries the rate.
template <bool OCL>  // OCL: the map in the arithmetic of the reference's kernel as built for this GPU (VSTAB_MAP_CREATEMAP_CL_OPENCL)
__global__ void __launch_bounds__(256) k_warp_nearest(WarpArgs a) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= a.dw || y >= a.dh) return;
    float mx, my;
    if constexpr (OCL) {
        const float vx = ocl_div((float)x - a.p.ocx, a.p.ofx), vy = ocl_div((float)y - a.p.ocy, a.p.ofy);
        map_pixel_ocl_literal(a.p.icx, a.p.icy, a.p.ifx, a.p.ify, a.p.r, a.p.r[0] * vx, a.p.r[3] * vx, a.p.r[6] * vx, vy, mx, my);
    } else {
        map_pixel(a.p, col_term(a.p, x), row_term(a.p, y), mx, my);
    }
    // cvRound -> int (NaN / out of range: INT_MIN on x86), then saturate_cast<short>
    const bool far = !(fabsf(mx) < 2147483520.0f) || !(fabsf(my) < 2147483520.0f);
    const int sx = far ? -32768 : min(max((int)__builtin_rintf(mx), -32768), 32767), sy = far ? -32768 : min(max((int)__builtin_rintf(my), -32768), 32767);
    int b, g, r;
    fetch_tap(a, sx, sy, b, g, r);
    uint8_t *o = a.dst + (size_t)y * a.pitch_dst + (size_t)x * 3;
    o[0] = (uint8_t)b, o[1] = (uint8_t)g, o[2] = (uint8_t)r;
}

namespace {

// The arguments of vstab_warp_nv12_ex / _rs / _mapped, checked, into the kernel argument; every message under vstab_warp_nv12 but the
// per-row rule.  check_warp_nv12 (vstab_warp_host.hpp) makes the same checks under the caller's name, with a narrower output format.
vstab_status check_warp_bilinear(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int sw, int sh, const float params[17],
                                 const float *rot_bottom, int map_mode, int out_format, void *dst, size_t pitch_dst, void *dst_uv, size_t pitch_dst_uv,
                                 int dw, int dh, WarpArgs &a) {
    if (!y || !uv || !dst || !params) return fail(VSTAB_ERR_INVALID, "vstab_warp_nv12: null pointer");
    if (sw <= 0 || sh <= 0 || (sw & 1) || (sh & 1) || sw > 32767 || sh > 32767)
        return fail(VSTAB_ERR_INVALID, "vstab_warp_nv12: source must be even-sized and <= 32767");
    if (dw <= 0 || dh <= 0 || dw > 32767 || dh > 32767)
        return fail(VSTAB_ERR_INVALID, "vstab_warp_nv12: output size must be in [1, 32767]");
    if (map_mode < VSTAB_MAP_CREATEMAP_CL || map_mode > VSTAB_MAP_CREATEMAP_CL_OPENCL) return fail(VSTAB_ERR_INVALID, "vstab_warp_nv12: unknown map mode");
    if (out_format != VSTAB_OUT_BGR8 && out_format != VSTAB_OUT_NV12 && out_format != VSTAB_OUT_NV12_PLANAR)
        return fail(VSTAB_ERR_INVALID, "vstab_warp_nv12: unknown output format");
    const bool nv12_out = out_format != VSTAB_OUT_BGR8;
    if (pitch_y < (size_t)sw || pitch_uv < (size_t)sw || pitch_dst < (size_t)dw * (nv12_out ? 1 : 3))
        return fail(VSTAB_ERR_INVALID, "vstab_warp_nv12: pitch smaller than row");
    if (nv12_out && (!dst_uv || pitch_dst_uv < (size_t)((dw + 1) / 2) * 2))
        return fail(VSTAB_ERR_INVALID, "vstab_warp_nv12: NV12 output needs a chroma plane of 2*ceil(width/2) bytes per row");
    if (!ptr_aligned(uv, 2) || pitch_uv % 2) return fail(VSTAB_ERR_INVALID, "vstab_warp_nv12: chroma plane must be 2-B aligned");
    if (rot_bottom && !map_mode_fish_to_pinhole(map_mode))
        return fail(VSTAB_ERR_INVALID, "vstab_warp_nv12_rs: the per-row warp exists for the fisheye -> pinhole modes (0, 1, 5) only");
    fill_warp_args(a, y, pitch_y, uv, pitch_uv, sw, sh, params, dst, pitch_dst, dst_uv, pitch_dst_uv, dw, dh);
    return VSTAB_OK;
}

// Checked arguments on the kernel that serves them: the plane-wise kernel for VSTAB_OUT_NV12_PLANAR, else the direct-gather kernel or the
// fused tile kernel.  qmap: vstab_warp_nv12_mapped's quantised map, rot_bottom: vstab_warp_nv12_rs's rotation of the last row, dist: the
// input lens's k1..k4 (vstab_warp_nv12_dist); null each where the entry point has none.
vstab_status launch_warp_bilinear(const WarpArgs &a, const float params[17], int map_mode, int out_format, const void *qmap, int qpitch,
                                  const float *rot_bottom, const float *dist, void *stream) {
    const bool planar = out_format == VSTAB_OUT_NV12_PLANAR;
    const bool nv12_out = out_format == VSTAB_OUT_NV12 || planar;
    hipStream_t st = static_cast<hipStream_t>(stream);
    // a chroma plane of 4 GiB or more (staged_offsets32: rows without chroma) is sampled from global memory with 64-bit addresses: the direct
    // kernel in plain mode, the gather path of the tiled kernels otherwise
    const StagedOffsets32 off32 = staged_offsets32(a.pitch_y, a.pitch_uv, a.sh);
    const bool small_pitch = off32.rows, stage32 = off32.chroma;
    const bool plain = map_mode == VSTAB_MAP_CREATEMAP_CL && !nv12_out && !qmap && !rot_bottom;
    if (!plain && !small_pitch) return fail(VSTAB_ERR_INVALID, "vstab_warp_nv12: source pitch too large for this mode");
    if (planar) {  // the plane-wise warp: its own kernel (vstab_warp_planar.hip); the map is always evaluated
        if (qmap) return fail(VSTAB_ERR_UNSUPPORTED, "vstab_warp_nv12_mapped: the quantised map holds no chroma positions -- VSTAB_OUT_NV12_PLANAR goes through vstab_warp_nv12_ex");
        if (a.sw < 16 || a.sh < 2) return fail(VSTAB_ERR_INVALID, "vstab_warp_nv12: the plane-wise warp needs a source of at least 16 x 2");
        const bool src16 = stage32 && ptr_aligned(a.y, 16) && ptr_aligned(a.uv, 16) && a.pitch_y % 16 == 0 && a.pitch_uv % 16 == 0;  // 16-byte staging loads
        const bool dst16 = ptr_aligned(a.dst, 16) && ptr_aligned(a.dst_uv, 16) && a.pitch_dst % 16 == 0 && a.pitch_dst_uv % 16 == 0;
        return launch_warp_planar(a, params, map_mode, 8, 0, src16, dst16, rot_bottom, st, dist);
    }
    const bool vec_ok = ptr_aligned(a.dst, 4) && a.pitch_dst % 4 == 0 && (!nv12_out || (ptr_aligned(a.dst_uv, 4) && a.pitch_dst_uv % 4 == 0));
    const bool src_vec_ok = stage32 && ptr_aligned(a.y, 8) && ptr_aligned(a.uv, 8) && a.pitch_y % 8 == 0 && a.pitch_uv % 8 == 0;  // 8-byte staging loads
    bool direct = !small_pitch || (plain && !stage32);
#ifdef VSTAB_DEV
    static const int variant = getenv("VSTAB_WARP_VARIANT") ? atoi(getenv("VSTAB_WARP_VARIANT")) : 2;
    direct = direct || (plain && variant == 1);
#endif
    if (!direct) return launch_warp_fused(a, params, map_mode, nv12_out, src_vec_ok, vec_ok, qmap, qpitch, rot_bottom, st, dist);
    // planes of 4 GiB and more: the direct-gather kernel with 64-bit addressing
    hipLaunchKernelGGL(k_warp_nv12_bgr, dim3(div_up(a.dw, WARP_TILE_W), div_up(a.dh, WARP_TILE_H)), dim3(16, 16), 0, st, a, (int)vec_ok);
    VSTAB_HIP_TRY(hipGetLastError());
    return VSTAB_OK;
}

// vstab_warp_nv12_dist_ex, and vstab_warp_nv12_dist as its default resampler with the constant border (two checks that cannot fire then),
// each under its own name n.  The order: check_warp_nv12's checks -- handed a mode it accepts, so that every mode but 1 and 2, known or
// not, gets the one message behind them --, the resampler, the map mode, the coefficients.
vstab_status warp_dist(const std::string &n, const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int sw, int sh, const float params[17],
                       const float dist[4], int map_mode, int resample, int border_mode, int out_format, void *dst, size_t pitch_dst, void *dst_uv,
                       size_t pitch_dst_uv, int dw, int dh, void *stream) {
    if (!dist) return fail(VSTAB_ERR_INVALID, n + ": null pointer");
    const bool fish_in = map_mode_takes_distortion(map_mode);
    CubicArgs c;
    VSTAB_TRY(check_warp_nv12(n, "the distorted-lens warp ", y, pitch_y, uv, pitch_uv, sw, sh, params, nullptr,
                              fish_in ? map_mode : (int)VSTAB_MAP_FISH_TO_RECT, out_format, &border_mode, dst, pitch_dst, dst_uv, pitch_dst_uv, dw, dh, c,
                              dist));
    if (resample != VSTAB_RESAMPLE_DEFAULT && resample != VSTAB_RESAMPLE_CUBIC && resample != VSTAB_RESAMPLE_LANCZOS4)
        return fail(VSTAB_ERR_INVALID, n + ": resample must be VSTAB_RESAMPLE_DEFAULT (0), _CUBIC (2) or _LANCZOS4 (4)");
    if (!fish_in) return fail(VSTAB_ERR_INVALID, n + ": distortion belongs to a fisheye input (map modes 1 and 2)");
    VSTAB_TRY(check_distortion(n, dist));
    if (resample == VSTAB_RESAMPLE_CUBIC) return launch_warp_cubic_dist(c, map_mode, out_format, border_mode, stream);
    if (resample == VSTAB_RESAMPLE_LANCZOS4) return launch_warp_lanczos4_dist(c, map_mode, out_format, border_mode, stream);
    if (border_mode != VSTAB_BORDER_CONSTANT) return launch_warp_border_dist(c, map_mode, out_format, border_mode, stream);
    // no check_warp_bilinear: check_warp_nv12 made the same checks with a narrower output format (and there is no rotation per row), so
    // whatever passed it passes those, and c.w is the kernel argument they would fill
    return launch_warp_bilinear(c.w, params, map_mode, out_format, nullptr, 0, nullptr, dist, stream);
}

}  // namespace

// Kernels of this translation unit are one code object, loaded by the runtime at the first launch of any of them.  Touching one of them
// here (vstab_preload_kernels) moves that load to a moment the caller chooses.
vstab_status preload_warp_kernels() {
    hipFuncAttributes at;
    VSTAB_HIP_TRY(hipFuncGetAttributes(&at, reinterpret_cast<const void *>(&k_warp_nv12_bgr)));
    return VSTAB_OK;
}

}  // namespace vstab

using namespace vstab;

extern "C" {

vstab_status vstab_warp_nv12_ex(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int sw, int sh,
                                const float params[17], int map_mode, int out_format, void *dst, size_t pitch_dst,
                                void *dst_uv, size_t pitch_dst_uv, int dw, int dh, void *stream) {
    WarpArgs a;
    VSTAB_TRY(check_warp_bilinear(y, pitch_y, uv, pitch_uv, sw, sh, params, nullptr, map_mode, out_format, dst, pitch_dst, dst_uv, pitch_dst_uv, dw, dh, a));
    return launch_warp_bilinear(a, params, map_mode, out_format, nullptr, 0, nullptr, nullptr, stream);
}

vstab_status vstab_warp_nv12_rs(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int sw, int sh, const float params[17],
                                const float rot_bottom[9], int map_mode, int out_format, void *dst, size_t pitch_dst, void *dst_uv,
                                size_t pitch_dst_uv, int dw, int dh, void *stream) {
    if (!rot_bottom) return fail(VSTAB_ERR_INVALID, "vstab_warp_nv12_rs: null pointer");
    WarpArgs a;
    VSTAB_TRY(check_warp_bilinear(y, pitch_y, uv, pitch_uv, sw, sh, params, rot_bottom, map_mode, out_format, dst, pitch_dst, dst_uv, pitch_dst_uv, dw, dh, a));
    return launch_warp_bilinear(a, params, map_mode, out_format, nullptr, 0, rot_bottom, nullptr, stream);
}

vstab_status vstab_warp_nv12_mapped(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int sw, int sh, const void *qmap,
                                    int out_format, void *dst, size_t pitch_dst, void *dst_uv, size_t pitch_dst_uv, int dw, int dh,
                                    void *stream) {
    if (!qmap || !ptr_aligned(qmap, 16)) return fail(VSTAB_ERR_INVALID, "vstab_warp_nv12_mapped: the quantised map must be a 16-byte aligned device buffer");
    static const float unused[17] = {0};
    WarpArgs a;
    VSTAB_TRY(check_warp_bilinear(y, pitch_y, uv, pitch_uv, sw, sh, unused, nullptr, VSTAB_MAP_CREATEMAP_CL, out_format, dst, pitch_dst, dst_uv, pitch_dst_uv,
                                  dw, dh, a));
    return launch_warp_bilinear(a, unused, VSTAB_MAP_CREATEMAP_CL, out_format, qmap, (dw + 3) & ~3, nullptr, nullptr, stream);
}

vstab_status vstab_warp_nv12_dist(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int sw, int sh, const float params[17],
                                  const float dist[4], int map_mode, int out_format, void *dst, size_t pitch_dst, void *dst_uv, size_t pitch_dst_uv,
                                  int dw, int dh, void *stream) {
    return warp_dist("vstab_warp_nv12_dist", y, pitch_y, uv, pitch_uv, sw, sh, params, dist, map_mode, VSTAB_RESAMPLE_DEFAULT, VSTAB_BORDER_CONSTANT,
                     out_format, dst, pitch_dst, dst_uv, pitch_dst_uv, dw, dh, stream);
}

vstab_status vstab_warp_nv12_dist_ex(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int sw, int sh, const float params[17],
                                     const float dist[4], int map_mode, int resample, int border_mode, int out_format, void *dst, size_t pitch_dst,
                                     void *dst_uv, size_t pitch_dst_uv, int dw, int dh, void *stream) {
    return warp_dist("vstab_warp_nv12_dist_ex", y, pitch_y, uv, pitch_uv, sw, sh, params, dist, map_mode, resample, border_mode, out_format, dst, pitch_dst,
                     dst_uv, pitch_dst_uv, dw, dh, stream);
}

vstab_status vstab_warp_nv12_rs_ex(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int sw, int sh, const float params[17],
                                   const float *rot_bottom, const float *dist, int map_mode, int resample, int border_mode, int out_format, void *dst,
                                   size_t pitch_dst, void *dst_uv, size_t pitch_dst_uv, int dw, int dh, void *stream) {
    const std::string n = "vstab_warp_nv12_rs_ex";
    BorderArgs ba;
    VSTAB_TRY(check_warp_nv12(n, "the per-row warp ", y, pitch_y, uv, pitch_uv, sw, sh, params, rot_bottom, map_mode, out_format, &border_mode, dst, pitch_dst,
                              dst_uv, pitch_dst_uv, dw, dh, ba.c, dist));
    if (resample != VSTAB_RESAMPLE_DEFAULT && resample != VSTAB_RESAMPLE_CUBIC && resample != VSTAB_RESAMPLE_LANCZOS4)
        return fail(VSTAB_ERR_INVALID, n + ": resample must be VSTAB_RESAMPLE_DEFAULT (0), _CUBIC (2) or _LANCZOS4 (4)");
    if (dist) {
        if (!map_mode_takes_distortion(map_mode)) return fail(VSTAB_ERR_INVALID, n + ": distortion belongs to a fisheye input (map modes 1 and 2)");
        VSTAB_TRY(check_distortion(n, dist));
    }
    const bool constant = border_mode == VSTAB_BORDER_CONSTANT, cubic = resample == VSTAB_RESAMPLE_CUBIC;
    // what an older entry point serves is that entry point's
    if (!rot_bottom && dist)
        return vstab_warp_nv12_dist_ex(y, pitch_y, uv, pitch_uv, sw, sh, params, dist, map_mode, resample, border_mode, out_format, dst, pitch_dst, dst_uv,
                                       pitch_dst_uv, dw, dh, stream);
    if (resample == VSTAB_RESAMPLE_DEFAULT && !dist) {
        if (!rot_bottom && constant)
            return vstab_warp_nv12_ex(y, pitch_y, uv, pitch_uv, sw, sh, params, map_mode, out_format, dst, pitch_dst, dst_uv, pitch_dst_uv, dw, dh, stream);
        return vstab_warp_nv12_border(y, pitch_y, uv, pitch_uv, sw, sh, params, rot_bottom, map_mode, out_format, border_mode, dst, pitch_dst, dst_uv,
                                      pitch_dst_uv, dw, dh, stream);
    }
    if (!rot_bottom) {
        if (constant)
            return (cubic ? vstab_warp_nv12_cubic : vstab_warp_nv12_lanczos4)(y, pitch_y, uv, pitch_uv, sw, sh, params, map_mode, out_format, dst, pitch_dst,
                                                                              dst_uv, pitch_dst_uv, dw, dh, stream);
        return (cubic ? vstab_warp_nv12_cubic_border : vstab_warp_nv12_lanczos4_border)(y, pitch_y, uv, pitch_uv, sw, sh, params, map_mode, out_format,
                                                                                        border_mode, dst, pitch_dst, dst_uv, pitch_dst_uv, dw, dh, stream);
    }
    // new ground: a rotation per row under the cubic and Lanczos resamplers, and under every resampler through a calibrated lens (map mode 1:
    // rot_bottom admits modes 0, 1 and 5, dist modes 1 and 2)
    fill_rolling_shutter(ba, params, rot_bottom, dh);
    if (resample == VSTAB_RESAMPLE_DEFAULT) return launch_warp_border(ba, map_mode, true, true, out_format, border_mode, stream);
    return (cubic ? launch_warp_cubic_rs : launch_warp_lanczos4_rs)(ba, map_mode, dist != nullptr, out_format, border_mode, stream);
}

// A rectilinear input lens with OpenCV's (k1, k2, p1, p2, k3): include/vstab.h, "Pinhole lens distortion".  The order: dist, check_warp_nv12's
// checks -- handed a mode it accepts, so that every mode but 3 and 4, known or not, gets the one message behind them --, the resampler, the
// map mode, the coefficients.  All zero: the older entry point's launch.
vstab_status vstab_warp_nv12_pinhole(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int sw, int sh, const float params[17],
                                     const float dist[5], int map_mode, int resample, int border_mode, int out_format, void *dst, size_t pitch_dst,
                                     void *dst_uv, size_t pitch_dst_uv, int dw, int dh, void *stream) {
    const std::string n = "vstab_warp_nv12_pinhole";
    if (!dist) return fail(VSTAB_ERR_INVALID, n + ": null pointer");
    const bool rect_in = map_mode_takes_pinhole(map_mode);
    BorderArgs ba;
    VSTAB_TRY(check_warp_nv12(n, "the pinhole-lens warp ", y, pitch_y, uv, pitch_uv, sw, sh, params, nullptr, rect_in ? map_mode : (int)VSTAB_MAP_RECT_TO_RECT,
                              out_format, &border_mode, dst, pitch_dst, dst_uv, pitch_dst_uv, dw, dh, ba.c));
    if (resample != VSTAB_RESAMPLE_DEFAULT && resample != VSTAB_RESAMPLE_CUBIC && resample != VSTAB_RESAMPLE_LANCZOS4)
        return fail(VSTAB_ERR_INVALID, n + ": resample must be VSTAB_RESAMPLE_DEFAULT (0), _CUBIC (2) or _LANCZOS4 (4)");
    if (!rect_in) return fail(VSTAB_ERR_INVALID, n + ": pinhole distortion belongs to a rectilinear input (map modes 3 and 4)");
    VSTAB_TRY(check_pinhole_distortion(n, dist));
    const bool constant = border_mode == VSTAB_BORDER_CONSTANT, cubic = resample == VSTAB_RESAMPLE_CUBIC;
    if (dist[0] == 0.0f && dist[1] == 0.0f && dist[2] == 0.0f && dist[3] == 0.0f && dist[4] == 0.0f) {  // the ideal pinhole: what served it before
        if (resample == VSTAB_RESAMPLE_DEFAULT) {
            if (constant)
                return vstab_warp_nv12_ex(y, pitch_y, uv, pitch_uv, sw, sh, params, map_mode, out_format, dst, pitch_dst, dst_uv, pitch_dst_uv, dw, dh, stream);
            return vstab_warp_nv12_border(y, pitch_y, uv, pitch_uv, sw, sh, params, nullptr, map_mode, out_format, border_mode, dst, pitch_dst, dst_uv,
                                          pitch_dst_uv, dw, dh, stream);
        }
        if (constant)
            return (cubic ? vstab_warp_nv12_cubic : vstab_warp_nv12_lanczos4)(y, pitch_y, uv, pitch_uv, sw, sh, params, map_mode, out_format, dst, pitch_dst,
                                                                              dst_uv, pitch_dst_uv, dw, dh, stream);
        return (cubic ? vstab_warp_nv12_cubic_border : vstab_warp_nv12_lanczos4_border)(y, pitch_y, uv, pitch_uv, sw, sh, params, map_mode, out_format,
                                                                                        border_mode, dst, pitch_dst, dst_uv, pitch_dst_uv, dw, dh, stream);
    }
    fill_rolling_shutter(ba, params, nullptr, dh);
    for (int k = 0; k < 5; k++) ba.pd[k] = dist[k];
    if (resample == VSTAB_RESAMPLE_DEFAULT) return launch_warp_border_pinhole(ba, map_mode, out_format, border_mode, stream);
    return (cubic ? launch_warp_cubic_pinhole : launch_warp_lanczos4_pinhole)(ba, map_mode, out_format, border_mode, stream);
}

vstab_status vstab_warp_nv12_nearest_ex(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int sw, int sh, const float params[17],
                                        int map_mode, void *dst, size_t pitch_dst, int dw, int dh, void *stream) {
    if (!y || !uv || !dst || !params) return fail(VSTAB_ERR_INVALID, "vstab_warp_nv12_nearest: null pointer");
    if (sw <= 0 || sh <= 0 || (sw & 1) || (sh & 1) || sw > 32767 || sh > 32767 || dw <= 0 || dh <= 0 || dw > 32767 || dh > 32767)
        return fail(VSTAB_ERR_INVALID, "vstab_warp_nv12_nearest: sizes must be in [1, 32767], source even");
    if (pitch_y < (size_t)sw || pitch_uv < (size_t)sw || pitch_dst < (size_t)dw * 3 || !ptr_aligned(uv, 2) || pitch_uv % 2)
        return fail(VSTAB_ERR_INVALID, "vstab_warp_nv12_nearest: bad pitch or chroma alignment");
    if (map_mode != VSTAB_MAP_CREATEMAP_CL && map_mode != VSTAB_MAP_CREATEMAP_CL_OPENCL)
        return fail(VSTAB_ERR_INVALID, "vstab_warp_nv12_nearest: the nearest-neighbour warp exists for the reference's own map (modes 0 and 5)");
    WarpArgs a;
    fill_warp_args(a, y, pitch_y, uv, pitch_uv, sw, sh, params, dst, pitch_dst, nullptr, 0, dw, dh);
    with_bool(map_mode == VSTAB_MAP_CREATEMAP_CL_OPENCL, [&](auto ocl) {
        launch_kernel(k_warp_nearest<decltype(ocl)::value>, dim3(div_up(dw, 64), div_up(dh, 4)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    });
    VSTAB_HIP_TRY(hipGetLastError());
    return VSTAB_OK;
}

vstab_status vstab_warp_nv12_nearest(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int sw, int sh, const float params[17],
                                     void *dst, size_t pitch_dst, int dw, int dh, void *stream) {
    return vstab_warp_nv12_nearest_ex(y, pitch_y, uv, pitch_uv, sw, sh, params, VSTAB_MAP_CREATEMAP_CL, dst, pitch_dst, dw, dh, stream);
}

vstab_status vstab_warp_nv12_bgr(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int sw, int sh,
                                 const float params[17], void *dst, size_t pitch_dst, int dw, int dh,
                                 void *stream) {
    return vstab_warp_nv12_ex(y, pitch_y, uv, pitch_uv, sw, sh, params, VSTAB_MAP_CREATEMAP_CL, VSTAB_OUT_BGR8, dst, pitch_dst,
                              nullptr, 0, dw, dh, stream);
}

}  // extern "C"
