// vstab_warp_host.hpp -- the host side of every warp translation unit (vstab_warp.hip, vstab_warp_fused.hip, vstab_warp_planar.hip,
// vstab_warp_p010.hip, vstab_warp_p010_resample.hip, vstab_warp_cubic.hip, vstab_warp_lanczos4.hip, vstab_warp_border.hip) and of vstab_plane_ops.hip: each fact once.  The alignment predicate, the
// kernel arguments from the C arguments (MapParams, MapParams32, WarpArgs, the rolling-shutter pair, FusedArgs' common part), the conditions
// for 32-bit staged offsets, the dispatch of a run-time mode to a template argument, the launch with a profiler's event pair, the
// argument checks of a WarpRequest (vstab_warp_request.hpp) and of the stateless remaps (every one before any launch, in one order, each
// message under the entry point's own name), and the resamplers' launch of a route.
#pragma once
#include <hip/hip_ext.h>

#include <type_traits>

#include "vstab_internal.hpp"
#include "vstab_resample.hpp"
#include "vstab_warp_request.hpp"

namespace vstab {

inline bool ptr_aligned(const void *p, size_t a) { return (reinterpret_cast<uintptr_t>(p) % a) == 0; }

// ---------------------------------------------------------------------------------------------------------------------
// Kernel arguments from the C arguments.  params[17]: the two cameras and the rotation, as include/vstab.h lays them out.
// ---------------------------------------------------------------------------------------------------------------------
inline MapParams map_params(const float params[17]) {
    MapParams m;
    m.icx = params[0], m.icy = params[1], m.ifx = params[2], m.ify = params[3];
    m.ocx = params[4], m.ocy = params[5], m.ofx = params[6], m.ofy = params[7];
    for (int i = 0; i < 9; i++) m.r[i] = params[8 + i];
    return m;
}
// the source camera scaled to the 1/32-pixel grid of cv::remap's quantisation, and the rotation's third column
// dist: k1..k4 of the input lens (the vstab_*_dist entry points), else null: zeros, which no other mode reads
inline MapParams32 map_params32(const float params[17], const float *dist = nullptr) {
    MapParams32 m = {params[0] * 32.0f, params[1] * 32.0f, params[2] * 32.0f, params[3] * 32.0f, params[10], params[13], params[16], {0.0f, 0.0f, 0.0f, 0.0f}};
    if (dist) m.d = {dist[0], dist[1], dist[2], dist[3]};
    return m;
}
inline void fill_warp_args(WarpArgs &a, const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int sw, int sh, const float params[17], void *dst,
                           size_t pitch_dst, void *dst_uv, size_t pitch_dst_uv, int dw, int dh) {
    a.y = (const uint8_t *)y, a.uv = (const uint8_t *)uv, a.dst = (uint8_t *)dst, a.dst_uv = (uint8_t *)dst_uv;
    a.pitch_y = pitch_y, a.pitch_uv = pitch_uv, a.pitch_dst = pitch_dst, a.pitch_dst_uv = pitch_dst_uv;
    a.sw = sw, a.sh = sh, a.dw = dw, a.dh = dh;
    a.p = map_params(params);
}
// The rotation per output row (FusedArgs, BorderArgs, P010Args: rs_d, rs_den): the last row's rotation minus the first's, fp32 as the
// definition forms it, and the row count it is spread over.  rot_bottom null: one rotation, rs_d all zero.
template <typename Args>
void fill_rolling_shutter(Args &a, const float params[17], const float *rot_bottom, int dh) {
    for (int k = 0; k < 9; k++) a.rs_d[k] = rot_bottom ? rot_bottom[k] - params[8 + k] : 0.0f;
    a.rs_den = (float)(dh > 1 ? dh - 1 : 1);
}
// what the three launchers of the tiled kernels set alike; the tile shape (tile_schedule) and the VSTAB_DEV fields' values are theirs
inline void fill_fused_args(FusedArgs &ta, const WarpArgs &a, const float params[17], bool src_vec_ok, bool dst_vec_ok, const void *qmap, int qpitch,
                            const float *rot_bottom, const float *dist = nullptr) {
    ta.w = a;
    ta.p32 = map_params32(params, dist);
    ta.src_vec_ok = src_vec_ok, ta.dst_vec_ok = dst_vec_ok;
    ta.qmap = static_cast<const int2 *>(qmap), ta.qpitch = qpitch;
    fill_rolling_shutter(ta, params, rot_bottom, a.dh);
#ifdef VSTAB_DEV
    ta.timing = nullptr, ta.ablate = 0, ta.lds_pad = 0;
#endif
    ta.col = ColourCoef{};  // (read by the COLOUR kernels alone: launch_warp_fused_colour)
}

// staged_offsets32 -- when the staged loads of the tiled kernels (warp_tile, warp_tile_planar) may form their row offsets in 32 bits.
//   rows    both pitches < 2^24 (operands of a 24-bit multiply) and pitch_y * sh < 2^32: every luma row offset fits.  Without it the tiled
//           kernels are not launched at all (the direct-gather kernel with 64-bit addresses, or a refusal).
//   chroma  and pitch_uv * (sh / 2) < 2^32: every chroma row offset fits as well.  Without it src_vec_ok is false: nothing is staged, the
//           tiled kernel samples every pixel from global memory with 64-bit addresses.
struct StagedOffsets32 {
    bool rows, chroma;
};
inline StagedOffsets32 staged_offsets32(size_t pitch_y, size_t pitch_uv, int sh) {
    const bool rows = pitch_y < (1u << 24) && pitch_uv < (1u << 24) && (uint64_t)pitch_y * sh < (1ull << 32);
    return {rows, rows && (uint64_t)pitch_uv * (sh / 2) < (1ull << 32)};
}

// ---------------------------------------------------------------------------------------------------------------------
// f(std::integral_constant<..., the mode>) for a checked run-time mode
// ---------------------------------------------------------------------------------------------------------------------
template <int M>
using mode_constant = std::integral_constant<int, M>;
template <typename F>
void with_map_mode(int map_mode, F &&f) {
    switch (map_mode) {
        case VSTAB_MAP_CREATEMAP_CL: f(mode_constant<MAP_CREATEMAP_CL>{}); break;
        case VSTAB_MAP_FISH_TO_RECT: f(mode_constant<MAP_FISH_TO_RECT>{}); break;
        case VSTAB_MAP_FISH_TO_FISH: f(mode_constant<MAP_FISH_TO_FISH>{}); break;
        case VSTAB_MAP_RECT_TO_RECT: f(mode_constant<MAP_RECT_TO_RECT>{}); break;
        case VSTAB_MAP_RECT_TO_FISH: f(mode_constant<MAP_RECT_TO_FISH>{}); break;
        default: f(mode_constant<MAP_CREATEMAP_CL_OPENCL>{}); break;
    }
}
// rs (a rotation per output row; checked: map modes 0, 1 and 5 only): the mode's MAP_RS_* form
template <typename F>
void with_map_mode(int map_mode, bool rs, F &&f) {
    if (!rs) return with_map_mode(map_mode, f);
    switch (map_mode) {
        case VSTAB_MAP_CREATEMAP_CL: f(mode_constant<MAP_RS_CREATEMAP_CL>{}); break;
        case VSTAB_MAP_CREATEMAP_CL_OPENCL: f(mode_constant<MAP_RS_CREATEMAP_CL_OPENCL>{}); break;
        default: f(mode_constant<MAP_RS_FISH_TO_RECT>{}); break;
    }
}
// the input lens's distortion (checked: map modes 1 and 2 only): the mode's MAP_FISHD_* form
template <typename F>
void with_dist_mode(int map_mode, F &&f) {
    if (map_mode == VSTAB_MAP_FISH_TO_RECT) f(mode_constant<MAP_FISHD_TO_RECT>{});
    else f(mode_constant<MAP_FISHD_TO_FISH>{});
}
// The one dispatch of the kernels that are launched for a route: the mode tag the routing chose (warp_route; kernel_mode_tag for the map
// kernels of vstab_plane_ops.hip) -> f(mode_constant<tag>).  f is instantiated for every tag: each launcher guards its kernel with
// `if constexpr` on the tags it serves, so that no other combination is instantiated.
template <typename F>
void with_kernel_mode(int mode, F &&f) {
    switch (mode) {
        case MAP_CREATEMAP_CL: f(mode_constant<MAP_CREATEMAP_CL>{}); break;
        case MAP_FISH_TO_RECT: f(mode_constant<MAP_FISH_TO_RECT>{}); break;
        case MAP_FISH_TO_FISH: f(mode_constant<MAP_FISH_TO_FISH>{}); break;
        case MAP_RECT_TO_RECT: f(mode_constant<MAP_RECT_TO_RECT>{}); break;
        case MAP_RECT_TO_FISH: f(mode_constant<MAP_RECT_TO_FISH>{}); break;
        case MAP_CREATEMAP_CL_OPENCL: f(mode_constant<MAP_CREATEMAP_CL_OPENCL>{}); break;
        case MAP_RS_CREATEMAP_CL: f(mode_constant<MAP_RS_CREATEMAP_CL>{}); break;
        case MAP_RS_FISH_TO_RECT: f(mode_constant<MAP_RS_FISH_TO_RECT>{}); break;
        case MAP_RS_CREATEMAP_CL_OPENCL: f(mode_constant<MAP_RS_CREATEMAP_CL_OPENCL>{}); break;
        case MAP_FISHD_TO_RECT: f(mode_constant<MAP_FISHD_TO_RECT>{}); break;
        case MAP_FISHD_TO_FISH: f(mode_constant<MAP_FISHD_TO_FISH>{}); break;
        case MAP_RS_FISHD_TO_RECT: f(mode_constant<MAP_RS_FISHD_TO_RECT>{}); break;
        case MAP_RECTD_TO_RECT: f(mode_constant<MAP_RECTD_TO_RECT>{}); break;
        default: f(mode_constant<MAP_RECTD_TO_FISH>{}); break;
    }
}
// the tags of one rotation per frame through an ideal or a calibrated fisheye lens: the map modes themselves and their MAP_FISHD_* forms
constexpr bool mode_plain_or_dist(int mode) { return mode <= MAP_CREATEMAP_CL_OPENCL || mode == MAP_FISHD_TO_RECT || mode == MAP_FISHD_TO_FISH; }
// the fisheye -> pinhole maps (modes 0, 1, 5): the only ones that take a rotation per output row (so the only ones with a MAP_RS_*
// form), and the only ones the 10-bit tiled kernels serve.  Asked of the public VSTAB_MAP_* values by the argument checks and of the
// kernels' MAP_* template values (a base mode: map_mode_base) by the launchers: the two enumerations agree on 0 .. 5, and the internal
// MAP_RS_* values 6 .. 8 are not among the three, so a caller's map_mode 6 is refused like any unknown mode.
static_assert((int)VSTAB_MAP_CREATEMAP_CL == (int)MAP_CREATEMAP_CL && (int)VSTAB_MAP_FISH_TO_RECT == (int)MAP_FISH_TO_RECT &&
                  (int)VSTAB_MAP_FISH_TO_FISH == (int)MAP_FISH_TO_FISH && (int)VSTAB_MAP_RECT_TO_RECT == (int)MAP_RECT_TO_RECT &&
                  (int)VSTAB_MAP_RECT_TO_FISH == (int)MAP_RECT_TO_FISH && (int)VSTAB_MAP_CREATEMAP_CL_OPENCL == (int)MAP_CREATEMAP_CL_OPENCL,
              "the public map modes and the kernels' template values are one numbering");
constexpr bool map_mode_fish_to_pinhole(int mode) { return mode == MAP_CREATEMAP_CL || mode == MAP_FISH_TO_RECT || mode == MAP_CREATEMAP_CL_OPENCL; }
template <typename F>
void with_border_mode(int border_mode, F &&f) {
    switch (border_mode) {
        case VSTAB_BORDER_CONSTANT: f(mode_constant<VSTAB_BORDER_CONSTANT>{}); break;
        case VSTAB_BORDER_REPLICATE: f(mode_constant<VSTAB_BORDER_REPLICATE>{}); break;
        case VSTAB_BORDER_REFLECT: f(mode_constant<VSTAB_BORDER_REFLECT>{}); break;
        default: f(mode_constant<VSTAB_BORDER_REFLECT_101>{}); break;
    }
}
template <typename F>
void with_channels(int channels, F &&f) {
    if (channels == 1) f(mode_constant<1>{});
    else if (channels == 2) f(mode_constant<2>{});
    else f(mode_constant<3>{});
}
template <typename F>
void with_bool(bool b, F &&f) {
    if (b) f(std::true_type{});
    else f(std::false_type{});
}
// one of two values of a template argument: rows per wave 8 / 4, output formats, blends
template <int A, int B, typename F>
void with_either(bool first, F &&f) {
    if (first) f(mode_constant<A>{});
    else f(mode_constant<B>{});
}

// A kernel that takes one argument block, launched; a profiling caller's event pair (take_launch_events) takes the kernel's own start / end stamps
template <typename Kernel, typename Args>
void launch_kernel(Kernel kernel, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const Args &args) {
    const LaunchEvents ev = take_launch_events();
    if (ev.start) hipExtLaunchKernelGGL(kernel, grid, block, lds_bytes, st, ev.start, ev.stop, 0, args);
    else hipLaunchKernelGGL(kernel, grid, block, lds_bytes, st, args);
}
// a resampler's tile kernel on its grid
template <typename Kernel, typename Args>
void launch_tiles(Kernel kernel, const Args &args, int dw, int dh, void *stream) {
    launch_kernel(kernel, dim3(div_up(dw, RESAMPLE_TW), div_up(dh, RESAMPLE_TH)), dim3(256), 0, static_cast<hipStream_t>(stream), args);
}

// The kernel argument of a request's planes.  chroma_out false: an output without a chroma plane (dst_uv null, whatever the caller passed).
inline void fill_warp_args(WarpArgs &a, const WarpRequest &q, bool chroma_out) {
    fill_warp_args(a, q.y, q.pitch_y, q.uv, q.pitch_uv, q.sw, q.sh, q.params, q.dst, q.pitch_dst, chroma_out ? q.dst_uv : nullptr, chroma_out ? q.pitch_dst_uv : 0,
                   q.dw, q.dh);
}

// A request of every entry point but the bilinear ones (those: check_warp_bilinear, vstab_warp.hip), checked, into the kernel argument:
// every check before any launch, in one order, each message under the entry point's own name.  The order: the planes; then the resampler,
// the map mode of the lens and its coefficients.
inline vstab_status check_warp_nv12(const WarpRequest &q, CubicArgs &c) {
    const auto refuse = [&](const std::string &what) { return fail(VSTAB_ERR_INVALID, std::string(q.e.name) + ": " + what); };
    // an entry point that exists for a lens needs its coefficients, and is checked here with a mode that passes, so that every mode but that
    // lens's, known or not, gets the one message behind these checks
    const bool fish_entry = q.e.lens == LENS_FISHEYE, rect_entry = q.e.lens == LENS_PINHOLE;
    const bool lens_mode = fish_entry ? map_mode_takes_distortion(q.map_mode) : rect_entry ? map_mode_takes_pinhole(q.map_mode) : true;
    const int map_mode = lens_mode ? q.map_mode : (int)VSTAB_MAP_FISH_TO_RECT;
    if (!q.y || !q.uv || !q.dst || !q.params || (fish_entry && !q.dist) || (rect_entry && !q.pinhole)) return refuse("null pointer");
    if (q.sw <= 0 || q.sh <= 0 || (q.sw & 1) || (q.sh & 1) || q.sw > 32767 || q.sh > 32767) return refuse("source must be even-sized and <= 32767");
    if (q.dw <= 0 || q.dh <= 0 || q.dw > 32767 || q.dh > 32767) return refuse("output size must be in [1, 32767]");
    if (map_mode < VSTAB_MAP_CREATEMAP_CL || map_mode > VSTAB_MAP_CREATEMAP_CL_OPENCL) return refuse("unknown map mode");
    if (q.rot_bottom && !map_mode_fish_to_pinhole(map_mode)) return refuse("a rotation per output row (rot_bottom) is served for map modes 0, 1 and 5");
    if (q.out_format != VSTAB_OUT_BGR8 && q.out_format != VSTAB_OUT_NV12_PLANAR)
        return refuse(std::string(q.e.who) + "emits VSTAB_OUT_BGR8 or VSTAB_OUT_NV12_PLANAR (NV12 through BGR is not served)");
    if (!border_mode_valid(q.border_mode))  // (an entry point without one: VSTAB_BORDER_CONSTANT)
        return refuse("border_mode must be VSTAB_BORDER_CONSTANT (0), _REPLICATE (1), _REFLECT (2) or _REFLECT_101 (4)");
    const bool planar = q.planar();
    if (q.pitch_y < (size_t)q.sw || q.pitch_uv < (size_t)q.sw || q.pitch_dst < (size_t)q.dw * (planar ? 1 : 3)) return refuse("pitch smaller than row");
    if (planar && (!q.dst_uv || q.pitch_dst_uv < (size_t)((q.dw + 1) / 2) * 2)) return refuse("plane-wise output needs a chroma plane of 2*ceil(width/2) bytes per row");
    if (!ptr_aligned(q.uv, 2) || q.pitch_uv % 2) return refuse("chroma plane must be 2-B aligned");
    fill_warp_args(c.w, q, planar);
    c.p32 = map_params32(q.params, q.dist);
    if (q.resample != VSTAB_RESAMPLE_DEFAULT && q.resample != VSTAB_RESAMPLE_CUBIC && q.resample != VSTAB_RESAMPLE_LANCZOS4)
        return refuse("resample must be VSTAB_RESAMPLE_DEFAULT (0), _CUBIC (2) or _LANCZOS4 (4)");
    if (q.dist) {
        if (!map_mode_takes_distortion(q.map_mode)) return refuse("distortion belongs to a fisheye input (map modes 1 and 2)");
        VSTAB_TRY(check_distortion(q.e.name, q.dist));
    }
    if (q.pinhole) {
        if (!map_mode_takes_pinhole(q.map_mode)) return refuse("pinhole distortion belongs to a rectilinear input (map modes 3 and 4)");
        VSTAB_TRY(check_pinhole_distortion(q.e.name, q.pinhole));
    }
    return VSTAB_OK;
}
// a keep request's history (vstab_internal.hpp), behind its other checks
inline vstab_status check_keep_prev(const WarpRequest &q, bool &in_place) {
    const KeepPlane planes[2] = {{q.prev, q.pitch_prev, q.dst, q.pitch_dst, (size_t)q.dw * (q.planar() ? 1 : 3), q.dh},
                                 {q.prev_uv, q.pitch_prev_uv, q.dst_uv, q.pitch_dst_uv, (size_t)((q.dw + 1) / 2) * 2, (q.dh + 1) / 2}};
    return check_keep_prev(q.e.name, planes, q.planar() ? 2 : 1, in_place);
}

// The stateless remaps' arguments, checked.  border_mode: null where the entry point has none (the border is constant, and its values are
// asked for with the first check).  border_values: the entry point takes border[]; packed: its values, one byte per channel, where the
// border is constant.
inline vstab_status check_remap(const std::string &n, const void *src, size_t pitch_src, int sw, int sh, int channels, const void *map_x, size_t pitch_x,
                                const void *map_y, size_t pitch_y, const int *border_mode, bool border_values, const int *border, void *dst,
                                size_t pitch_dst, int dw, int dh, uint32_t &packed) {
    if (!src || !map_x || !map_y || !dst || (!border_mode && !border)) return fail(VSTAB_ERR_INVALID, n + ": null pointer");
    if (channels < 1 || channels > 3) return fail(VSTAB_ERR_INVALID, n + ": channels must be 1, 2 or 3");
    if (sw <= 0 || sh <= 0 || dw <= 0 || dh <= 0 || sw > 32767 || sh > 32767 || dw > 32767 || dh > 32767)
        return fail(VSTAB_ERR_INVALID, n + ": sizes must be in [1, 32767]");
    if (pitch_src < (size_t)sw * channels || pitch_dst < (size_t)dw * channels || pitch_x < (size_t)dw * 4 || pitch_y < (size_t)dw * 4 || pitch_x % 4 ||
        pitch_y % 4 || !ptr_aligned(map_x, 4) || !ptr_aligned(map_y, 4))
        return fail(VSTAB_ERR_INVALID, n + ": pitch smaller than a row, or map planes not 4-byte aligned");
    if (border_mode && !border_mode_valid(*border_mode))
        return fail(VSTAB_ERR_INVALID, n + ": border_mode must be VSTAB_BORDER_CONSTANT (0), _REPLICATE (1), _REFLECT (2) or _REFLECT_101 (4)");
    packed = 0;
    if (border_values && (!border_mode || *border_mode == VSTAB_BORDER_CONSTANT)) {
        if (!border) return fail(VSTAB_ERR_INVALID, n + ": VSTAB_BORDER_CONSTANT needs the border values");
        for (int k = 0; k < channels; k++) {
            if (border[k] < 0 || border[k] > 255) return fail(VSTAB_ERR_INVALID, n + ": border values must be in [0, 255]");
            packed |= (uint32_t)border[k] << (8 * k);
        }
    }
    return VSTAB_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// A resampler (cubic, Lanczos) over its kernels KS: KS::warp<MODE, PLANAR, BORDER>(), KS::warp_rs<MODE, PLANAR, BORDER>() and
// KS::remap<CN, BORDER>(), the kernel of each combination (BORDER_CONSTANT: the kernels that carry the border value).  remap_resample's
// border_mode null: the constant-border entry points.
// ---------------------------------------------------------------------------------------------------------------------
// The warp kernel of a route on its grid.  ARGS_CUBIC: KS::warp over ba.c, one rotation per frame through an ideal or a calibrated fisheye
// lens.  ARGS_BORDER: KS::warp_rs over ba -- a rotation per output row (the map mode 0, 1 or 5 itself: the kernel's map is
// border_map<MODE, true>; MAP_RS_FISHD_TO_RECT: map mode 1 with the coefficients in ba.c.p32.d) or a rectilinear lens with (k1, k2, p1, p2,
// k3) in ba.pd (MAP_RECTD_*, whose map is border_map<MODE, false>; rs_d zero) --, every border mode, BORDER_CONSTANT included.
template <typename KS>
vstab_status launch_warp_resample(const BorderArgs &ba, const WarpRoute &r, int out_format, int border_mode, void *stream) {
    with_kernel_mode(route_kernel_mode(r.mode), [&](auto mode) {
        with_border_mode(border_mode, [&](auto border) {
            with_bool(out_format == VSTAB_OUT_NV12_PLANAR, [&](auto planar) {
                constexpr int MODE = decltype(mode)::value, BORDER = decltype(border)::value;
                constexpr bool PLANAR = decltype(planar)::value;
                if constexpr (mode_plain_or_dist(MODE))
                    if (r.block == ARGS_CUBIC) launch_tiles(KS::template warp<MODE, PLANAR, BORDER>(), ba.c, ba.c.w.dw, ba.c.w.dh, stream);
                if constexpr (map_mode_fish_to_pinhole(MODE) || MODE == MAP_RS_FISHD_TO_RECT || ModeTraits<MODE>::rectd)
                    if (r.block == ARGS_BORDER) launch_tiles(KS::template warp_rs<MODE, PLANAR, BORDER>(), ba, ba.c.w.dw, ba.c.w.dh, stream);
            });
        });
    });
    VSTAB_HIP_TRY(hipGetLastError());
    return VSTAB_OK;
}
// one launcher per unit of tile kernels: ba checked and filled (rs_d / rs_den by fill_rolling_shutter, pd), r the route that names the unit's family
vstab_status launch_warp_cubic(const BorderArgs &ba, const WarpRoute &r, int out_format, int border_mode, void *stream);
vstab_status launch_warp_lanczos4(const BorderArgs &ba, const WarpRoute &r, int out_format, int border_mode, void *stream);
vstab_status launch_warp_border(const BorderArgs &ba, const WarpRoute &r, int out_format, int border_mode, void *stream);
vstab_status launch_warp_keep(const BorderArgs &ba, const WarpRoute &r, const WarpRequest &q, bool in_place);
// the 10-bit plane-wise kernels (vstab_warp_p010_resample.hip): ba.c.w the P010 planes; map_mode 0 .. 5, rs (a rotation per output row) with
// 0, 1 and 5 alone; resample VSTAB_RESAMPLE_CUBIC or _LANCZOS4; every border mode
vstab_status launch_warp_resample10(const BorderArgs &ba, int map_mode, bool rs, int resample, int border_mode, void *stream);

template <typename KS>
vstab_status remap_resample(const char *name, const void *src, size_t pitch_src, int sw, int sh, int channels, const void *map_x, size_t pitch_x,
                            const void *map_y, size_t pitch_y, const int *border_mode, const int border[3], void *dst, size_t pitch_dst, int dw, int dh,
                            void *stream) {
    uint32_t b;
    const vstab_status st =
        check_remap(name, src, pitch_src, sw, sh, channels, map_x, pitch_x, map_y, pitch_y, border_mode, true, border, dst, pitch_dst, dw, dh, b);
    if (st != VSTAB_OK) return st;
    const dim3 grid(div_up(dw, 64), div_up(dh, 4));
    hipStream_t s = static_cast<hipStream_t>(stream);
    with_channels(channels, [&](auto cn) {
        with_border_mode(border_mode ? *border_mode : VSTAB_BORDER_CONSTANT, [&](auto bm) {
            constexpr int CN = decltype(cn)::value, BORDER = decltype(bm)::value;
            if constexpr (BORDER == VSTAB_BORDER_CONSTANT)
                hipLaunchKernelGGL((KS::template remap<CN, BORDER>()), grid, dim3(256), 0, s, (const uint8_t *)src, pitch_src, sw, sh, (const float *)map_x,
                                   pitch_x, (const float *)map_y, pitch_y, b, (uint8_t *)dst, pitch_dst, dw, dh);
            else
                hipLaunchKernelGGL((KS::template remap<CN, BORDER>()), grid, dim3(256), 0, s, (const uint8_t *)src, pitch_src, sw, sh, (const float *)map_x,
                                   pitch_x, (const float *)map_y, pitch_y, (uint8_t *)dst, pitch_dst, dw, dh);
        });
    });
    VSTAB_HIP_TRY(hipGetLastError());
    return VSTAB_OK;
}

}  // namespace vstab
