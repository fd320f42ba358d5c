// vstab_warp.hip -- the 8-bit NV12 warps' one host path for gfx950 (MI355X), warp_nv12: a WarpRequest checked, routed and launched; the
// bilinear entry points' own argument checks and their choice between the direct-gather kernel, the fused tile kernel
// (vstab_warp_fused.hip) and the plane-wise kernel (vstab_warp_planar.hip); the C entry points that are not a resampler's, a border's or
// the keep-edge warp's; and the two direct-gather kernels themselves, k_warp_nv12_bgr and k_warp_nearest.  Compiled with -ffp-contract=off.
//
// HBM-bound gather work (no MFMA): coalesced wide stores, enough workgroups to fill 256 CUs, the map in registers.
#include <cstdlib>

#include "vstab_colour.hpp"
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

// A request of vstab_warp_nv12_ex / _rs / _mapped, checked, into the kernel argument; every message under vstab_warp_nv12 but the
// per-row rule.  check_warp_nv12 (vstab_warp_host.hpp) makes the same checks under the caller's name, with a narrower output format.
vstab_status check_warp_bilinear(const WarpRequest &q, WarpArgs &a) {
    if (!q.y || !q.uv || !q.dst || !q.params) return fail(VSTAB_ERR_INVALID, "vstab_warp_nv12: null pointer");
    if (q.sw <= 0 || q.sh <= 0 || (q.sw & 1) || (q.sh & 1) || q.sw > 32767 || q.sh > 32767)
        return fail(VSTAB_ERR_INVALID, "vstab_warp_nv12: source must be even-sized and <= 32767");
    if (q.dw <= 0 || q.dh <= 0 || q.dw > 32767 || q.dh > 32767)
        return fail(VSTAB_ERR_INVALID, "vstab_warp_nv12: output size must be in [1, 32767]");
    if (q.map_mode < VSTAB_MAP_CREATEMAP_CL || q.map_mode > VSTAB_MAP_CREATEMAP_CL_OPENCL) return fail(VSTAB_ERR_INVALID, "vstab_warp_nv12: unknown map mode");
    if (q.out_format != VSTAB_OUT_BGR8 && q.out_format != VSTAB_OUT_NV12 && q.out_format != VSTAB_OUT_NV12_PLANAR)
        return fail(VSTAB_ERR_INVALID, "vstab_warp_nv12: unknown output format");
    const bool nv12_out = q.out_format != VSTAB_OUT_BGR8;
    if (q.pitch_y < (size_t)q.sw || q.pitch_uv < (size_t)q.sw || q.pitch_dst < (size_t)q.dw * (nv12_out ? 1 : 3))
        return fail(VSTAB_ERR_INVALID, "vstab_warp_nv12: pitch smaller than row");
    if (nv12_out && (!q.dst_uv || q.pitch_dst_uv < (size_t)((q.dw + 1) / 2) * 2))
        return fail(VSTAB_ERR_INVALID, "vstab_warp_nv12: NV12 output needs a chroma plane of 2*ceil(width/2) bytes per row");
    if (!ptr_aligned(q.uv, 2) || q.pitch_uv % 2) return fail(VSTAB_ERR_INVALID, "vstab_warp_nv12: chroma plane must be 2-B aligned");
    if (q.rot_bottom && !map_mode_fish_to_pinhole(q.map_mode))
        return fail(VSTAB_ERR_INVALID, "vstab_warp_nv12_rs: the per-row warp exists for the fisheye -> pinhole modes (0, 1, 5) only");
    // a colour spec (ENTRY_COLOUR, a pull of a handle with vstab_set_colour): behind every other check, under the entry point's own name
    VSTAB_TRY(check_colour_spec(q.e.name, q.colour_matrix, q.colour_range));
    if (q.colour() && q.out_format == VSTAB_OUT_NV12_PLANAR)
        return fail(VSTAB_ERR_INVALID, std::string(q.e.name) + ": VSTAB_OUT_NV12_PLANAR converts nothing, a colour spec belongs to VSTAB_OUT_BGR8 and VSTAB_OUT_NV12");
    fill_warp_args(a, q, true);
    return VSTAB_OK;
}

// A checked request on the bilinear kernel that serves it (WARP_PLANAR, WARP_FUSED): the plane-wise kernel for VSTAB_OUT_NV12_PLANAR, else
// the fused tile kernel or, for planes of 4 GiB and more, the direct-gather kernel.  What only the planes decide is refused here, under
// the fixed name vstab_warp_nv12, and with it the one checked request without a route: a quantised map with plane-wise output.
vstab_status launch_warp_bilinear(const WarpArgs &a, const WarpRequest &q) {
    const bool planar = q.planar();
    const bool nv12_out = q.out_format == VSTAB_OUT_NV12 || planar;
    hipStream_t st = static_cast<hipStream_t>(q.stream);
    // a chroma plane of 4 GiB or more (staged_offsets32: rows without chroma) is sampled from global memory with 64-bit addresses: the direct
    // kernel in plain mode, the gather path of the tiled kernels otherwise
    const StagedOffsets32 off32 = staged_offsets32(a.pitch_y, a.pitch_uv, a.sh);
    const bool small_pitch = off32.rows, stage32 = off32.chroma;
    const bool plain = q.map_mode == VSTAB_MAP_CREATEMAP_CL && !nv12_out && !q.qmap && !q.rot_bottom;
    // (the direct-gather kernel has cvtColor's constants: with a colour spec only the tiled kernels serve, staged or not)
    if (q.colour() && !small_pitch) return fail(VSTAB_ERR_UNSUPPORTED, std::string(q.e.name) + ": source planes of 4 GiB and more are served with (VSTAB_COLOUR_CVTCOLOR, VSTAB_RANGE_LIMITED) only");
    if (!plain && !small_pitch) return fail(VSTAB_ERR_INVALID, "vstab_warp_nv12: source pitch too large for this mode");
    if (planar) {  // the plane-wise warp: its own kernel (vstab_warp_planar.hip); the map is always evaluated
        if (q.qmap) return fail(VSTAB_ERR_UNSUPPORTED, "vstab_warp_nv12_mapped: the quantised map holds no chroma positions -- VSTAB_OUT_NV12_PLANAR goes through vstab_warp_nv12_ex");
        if (a.sw < 16 || a.sh < 2) return fail(VSTAB_ERR_INVALID, "vstab_warp_nv12: the plane-wise warp needs a source of at least 16 x 2");
        const bool src16 = stage32 && ptr_aligned(a.y, 16) && ptr_aligned(a.uv, 16) && a.pitch_y % 16 == 0 && a.pitch_uv % 16 == 0;  // 16-byte staging loads
        const bool dst16 = ptr_aligned(a.dst, 16) && ptr_aligned(a.dst_uv, 16) && a.pitch_dst % 16 == 0 && a.pitch_dst_uv % 16 == 0;
        return launch_warp_planar(a, q.params, q.map_mode, 8, 0, src16, dst16, q.rot_bottom, st, q.dist);
    }
    const bool vec_ok = ptr_aligned(a.dst, 4) && a.pitch_dst % 4 == 0 && (!nv12_out || (ptr_aligned(a.dst_uv, 4) && a.pitch_dst_uv % 4 == 0));
    const bool src_vec_ok = stage32 && ptr_aligned(a.y, 8) && ptr_aligned(a.uv, 8) && a.pitch_y % 8 == 0 && a.pitch_uv % 8 == 0;  // 8-byte staging loads
    if (q.colour()) {
        if (q.qmap || q.rot_bottom || q.dist) return fail(VSTAB_ERR_UNSUPPORTED, std::string(q.e.name) + ": a colour spec is served with one rotation per frame through an ideal lens, the map evaluated");
        return launch_warp_fused_colour(a, q.params, q.map_mode, nv12_out, src_vec_ok, vec_ok, colour_coefficients(q.colour_matrix, q.colour_range), st);
    }
    bool direct = !small_pitch || (plain && !stage32);
#ifdef VSTAB_DEV
    static const int variant = getenv("VSTAB_WARP_VARIANT") ? atoi(getenv("VSTAB_WARP_VARIANT")) : 2;
    direct = direct || (plain && variant == 1);
#endif
    if (!direct) return launch_warp_fused(a, q.params, q.map_mode, nv12_out, src_vec_ok, vec_ok, q.qmap, q.qpitch, q.rot_bottom, st, q.dist);
    // planes of 4 GiB and more: the direct-gather kernel with 64-bit addressing
    hipLaunchKernelGGL(k_warp_nv12_bgr, dim3(div_up(a.dw, WARP_TILE_W), div_up(a.dh, WARP_TILE_H)), dim3(16, 16), 0, st, a, (int)vec_ok);
    VSTAB_HIP_TRY(hipGetLastError());
    return VSTAB_OK;
}

}  // namespace

// Every 8-bit NV12 warp: checked once, routed once (warp_route), launched once.  ba is the argument block of every family: the kernels
// take it whole (ARGS_BORDER; ARGS_KEEP adds the history to it) or its ba.c (ARGS_CUBIC) or its ba.c.w (ARGS_WARP).
vstab_status warp_nv12(const WarpRequest &q) {
    BorderArgs ba;
    if (q.e.who) VSTAB_TRY(check_warp_nv12(q, ba.c));
    else VSTAB_TRY(check_warp_bilinear(q, ba.c.w));
    bool in_place = false;
    if (q.keep) VSTAB_TRY(check_keep_prev(q, in_place));
    const WarpRoute r = warp_route(q);
    fill_rolling_shutter(ba, q.params, q.rot_bottom, q.dh);
    if (q.pinhole)
        for (int k = 0; k < 5; k++) ba.pd[k] = q.pinhole[k];
    switch (r.family) {
        case WARP_BORDER: return launch_warp_border(ba, r, q.out_format, q.border_mode, q.stream);
        case WARP_CUBIC: return launch_warp_cubic(ba, r, q.out_format, q.border_mode, q.stream);
        case WARP_LANCZOS4: return launch_warp_lanczos4(ba, r, q.out_format, q.border_mode, q.stream);
        case WARP_KEEP: return launch_warp_keep(ba, r, q, in_place);
        default: return launch_warp_bilinear(ba.c.w, q);  // (WARP_NONE: refused there)
    }
}

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
    return warp_nv12({.e = ENTRY_EX, .y = y, .pitch_y = pitch_y, .uv = uv, .pitch_uv = pitch_uv, .sw = sw, .sh = sh, .params = params, .map_mode = map_mode,
                      .out_format = out_format, .dst = dst, .pitch_dst = pitch_dst, .dst_uv = dst_uv, .pitch_dst_uv = pitch_dst_uv, .dw = dw, .dh = dh, .stream = stream});
}

vstab_status vstab_warp_nv12_colour(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int sw, int sh, const float params[17], int map_mode,
                                    int out_format, void *dst, size_t pitch_dst, void *dst_uv, size_t pitch_dst_uv, int dw, int dh, int matrix, int range,
                                    void *stream) {
    return warp_nv12({.e = ENTRY_COLOUR, .y = y, .pitch_y = pitch_y, .uv = uv, .pitch_uv = pitch_uv, .sw = sw, .sh = sh, .params = params, .map_mode = map_mode,
                      .out_format = out_format, .dst = dst, .pitch_dst = pitch_dst, .dst_uv = dst_uv, .pitch_dst_uv = pitch_dst_uv, .dw = dw, .dh = dh, .stream = stream,
                      .colour_matrix = matrix, .colour_range = range});
}

vstab_status vstab_warp_nv12_rs(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int sw, int sh, const float params[17],
                                const float rot_bottom[9], int map_mode, int out_format, void *dst, size_t pitch_dst, void *dst_uv,
                                size_t pitch_dst_uv, int dw, int dh, void *stream) {
    if (!rot_bottom) return fail(VSTAB_ERR_INVALID, "vstab_warp_nv12_rs: null pointer");
    return warp_nv12({.e = ENTRY_RS, .y = y, .pitch_y = pitch_y, .uv = uv, .pitch_uv = pitch_uv, .sw = sw, .sh = sh, .params = params, .rot_bottom = rot_bottom,
                      .map_mode = map_mode, .out_format = out_format, .dst = dst, .pitch_dst = pitch_dst, .dst_uv = dst_uv, .pitch_dst_uv = pitch_dst_uv, .dw = dw,
                      .dh = dh, .stream = stream});
}

vstab_status vstab_warp_nv12_mapped(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int sw, int sh, const void *qmap,
                                    int out_format, void *dst, size_t pitch_dst, void *dst_uv, size_t pitch_dst_uv, int dw, int dh,
                                    void *stream) {
    if (!qmap || !ptr_aligned(qmap, 16)) return fail(VSTAB_ERR_INVALID, "vstab_warp_nv12_mapped: the quantised map must be a 16-byte aligned device buffer");
    static const float unused[17] = {0};
    return warp_nv12({.e = ENTRY_MAPPED, .y = y, .pitch_y = pitch_y, .uv = uv, .pitch_uv = pitch_uv, .sw = sw, .sh = sh, .params = unused, .qmap = qmap,
                      .qpitch = (dw + 3) & ~3, .out_format = out_format, .dst = dst, .pitch_dst = pitch_dst, .dst_uv = dst_uv, .pitch_dst_uv = pitch_dst_uv, .dw = dw,
                      .dh = dh, .stream = stream});
}

// vstab_warp_nv12_dist is vstab_warp_nv12_dist_ex's default resampler with the constant border (two checks that cannot fire then), each
// under its own name
vstab_status vstab_warp_nv12_dist(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int sw, int sh, const float params[17],
                                  const float dist[4], int map_mode, int out_format, void *dst, size_t pitch_dst, void *dst_uv, size_t pitch_dst_uv,
                                  int dw, int dh, void *stream) {
    return warp_nv12({.e = ENTRY_DIST, .y = y, .pitch_y = pitch_y, .uv = uv, .pitch_uv = pitch_uv, .sw = sw, .sh = sh, .params = params, .dist = dist,
                      .map_mode = map_mode, .out_format = out_format, .dst = dst, .pitch_dst = pitch_dst, .dst_uv = dst_uv, .pitch_dst_uv = pitch_dst_uv, .dw = dw,
                      .dh = dh, .stream = stream});
}

vstab_status vstab_warp_nv12_dist_ex(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int sw, int sh, const float params[17],
                                     const float dist[4], int map_mode, int resample, int border_mode, int out_format, void *dst, size_t pitch_dst,
                                     void *dst_uv, size_t pitch_dst_uv, int dw, int dh, void *stream) {
    return warp_nv12({.e = ENTRY_DIST_EX, .y = y, .pitch_y = pitch_y, .uv = uv, .pitch_uv = pitch_uv, .sw = sw, .sh = sh, .params = params, .dist = dist,
                      .map_mode = map_mode, .resample = resample, .border_mode = border_mode, .out_format = out_format, .dst = dst, .pitch_dst = pitch_dst,
                      .dst_uv = dst_uv, .pitch_dst_uv = pitch_dst_uv, .dw = dw, .dh = dh, .stream = stream});
}

vstab_status vstab_warp_nv12_rs_ex(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int sw, int sh, const float params[17],
                                   const float *rot_bottom, const float *dist, int map_mode, int resample, int border_mode, int out_format, void *dst,
                                   size_t pitch_dst, void *dst_uv, size_t pitch_dst_uv, int dw, int dh, void *stream) {
    return warp_nv12({.e = ENTRY_RS_EX, .y = y, .pitch_y = pitch_y, .uv = uv, .pitch_uv = pitch_uv, .sw = sw, .sh = sh, .params = params, .rot_bottom = rot_bottom,
                      .dist = dist, .map_mode = map_mode, .resample = resample, .border_mode = border_mode, .out_format = out_format, .dst = dst,
                      .pitch_dst = pitch_dst, .dst_uv = dst_uv, .pitch_dst_uv = pitch_dst_uv, .dw = dw, .dh = dh, .stream = stream});
}

// A rectilinear input lens with OpenCV's (k1, k2, p1, p2, k3): include/vstab.h, "Pinhole lens distortion"
vstab_status vstab_warp_nv12_pinhole(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int sw, int sh, const float params[17],
                                     const float dist[5], int map_mode, int resample, int border_mode, int out_format, void *dst, size_t pitch_dst,
                                     void *dst_uv, size_t pitch_dst_uv, int dw, int dh, void *stream) {
    return warp_nv12({.e = ENTRY_PINHOLE, .y = y, .pitch_y = pitch_y, .uv = uv, .pitch_uv = pitch_uv, .sw = sw, .sh = sh, .params = params, .pinhole = dist,
                      .map_mode = map_mode, .resample = resample, .border_mode = border_mode, .out_format = out_format, .dst = dst, .pitch_dst = pitch_dst,
                      .dst_uv = dst_uv, .pitch_dst_uv = pitch_dst_uv, .dw = dw, .dh = dh, .stream = stream});
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
    return warp_nv12({.e = ENTRY_EX, .y = y, .pitch_y = pitch_y, .uv = uv, .pitch_uv = pitch_uv, .sw = sw, .sh = sh, .params = params, .dst = dst,
                      .pitch_dst = pitch_dst, .dst_uv = nullptr, .pitch_dst_uv = 0, .dw = dw, .dh = dh, .stream = stream});
}

}  // extern "C"
