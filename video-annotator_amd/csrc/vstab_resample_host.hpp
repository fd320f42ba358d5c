// vstab_resample_host.hpp -- the host side of the entry points of vstab_warp_cubic.hip, vstab_warp_lanczos4.hip and vstab_warp_border.hip:
// the argument checks (every one before any launch, in one order, each message under the entry point's own name), the kernel argument, the
// dispatch of a run-time mode to a template argument, and the launches.
#pragma once
#include <hip/hip_ext.h>

#include <type_traits>

#include "vstab_internal.hpp"
#include "vstab_resample.hpp"

namespace vstab {

inline bool ptr_aligned(const void *p, size_t a) { return (reinterpret_cast<uintptr_t>(p) % a) == 0; }

// f(std::integral_constant<..., the mode>) for a checked run-time mode
template <typename F>
void with_map_mode(int map_mode, F &&f) {
    switch (map_mode) {
        case VSTAB_MAP_CREATEMAP_CL: f(std::integral_constant<int, MAP_CREATEMAP_CL>{}); break;
        case VSTAB_MAP_FISH_TO_RECT: f(std::integral_constant<int, MAP_FISH_TO_RECT>{}); break;
        case VSTAB_MAP_FISH_TO_FISH: f(std::integral_constant<int, MAP_FISH_TO_FISH>{}); break;
        case VSTAB_MAP_RECT_TO_RECT: f(std::integral_constant<int, MAP_RECT_TO_RECT>{}); break;
        case VSTAB_MAP_RECT_TO_FISH: f(std::integral_constant<int, MAP_RECT_TO_FISH>{}); break;
        default: f(std::integral_constant<int, MAP_CREATEMAP_CL_OPENCL>{}); break;
    }
}
template <typename F>
void with_border_mode(int border_mode, F &&f) {
    switch (border_mode) {
        case VSTAB_BORDER_CONSTANT: f(std::integral_constant<int, VSTAB_BORDER_CONSTANT>{}); break;
        case VSTAB_BORDER_REPLICATE: f(std::integral_constant<int, VSTAB_BORDER_REPLICATE>{}); break;
        case VSTAB_BORDER_REFLECT: f(std::integral_constant<int, VSTAB_BORDER_REFLECT>{}); break;
        default: f(std::integral_constant<int, VSTAB_BORDER_REFLECT_101>{}); break;
    }
}
template <typename F>
void with_channels(int channels, F &&f) {
    if (channels == 1) f(std::integral_constant<int, 1>{});
    else if (channels == 2) f(std::integral_constant<int, 2>{});
    else f(std::integral_constant<int, 3>{});
}
template <typename F>
void with_bool(bool b, F &&f) {
    if (b) f(std::true_type{});
    else f(std::false_type{});
}

// a tile kernel on its grid; a profiling caller's event pair takes the kernel's own start / end stamps
template <typename Kernel, typename Args>
void launch_tiles(Kernel kernel, const Args &args, int dw, int dh, void *stream) {
    const dim3 grid(div_up(dw, RESAMPLE_TW), div_up(dh, RESAMPLE_TH));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const LaunchEvents ev = take_launch_events();
    if (ev.start) hipExtLaunchKernelGGL(kernel, grid, dim3(256), 0, st, ev.start, ev.stop, 0, args);
    else hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, args);
}

// The NV12 warps' arguments, checked, into the kernel argument.  who: the subject of the output-format message ("the cubic warp "; "").
// rot_bottom: vstab_warp_nv12_border's rotation per output row, else null.  border_mode: null where the entry point has none.
inline vstab_status check_warp_nv12(const std::string &n, const char *who, const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int sw, int sh,
                                    const float params[17], const float *rot_bottom, int map_mode, int out_format, const int *border_mode, void *dst,
                                    size_t pitch_dst, void *dst_uv, size_t pitch_dst_uv, int dw, int dh, CubicArgs &c) {
    if (!y || !uv || !dst || !params) return fail(VSTAB_ERR_INVALID, n + ": null pointer");
    if (sw <= 0 || sh <= 0 || (sw & 1) || (sh & 1) || sw > 32767 || sh > 32767)
        return fail(VSTAB_ERR_INVALID, n + ": source must be even-sized and <= 32767");
    if (dw <= 0 || dh <= 0 || dw > 32767 || dh > 32767) return fail(VSTAB_ERR_INVALID, n + ": output size must be in [1, 32767]");
    if (map_mode < VSTAB_MAP_CREATEMAP_CL || map_mode > VSTAB_MAP_CREATEMAP_CL_OPENCL) return fail(VSTAB_ERR_INVALID, n + ": unknown map mode");
    if (rot_bottom && map_mode != VSTAB_MAP_CREATEMAP_CL && map_mode != VSTAB_MAP_FISH_TO_RECT && map_mode != VSTAB_MAP_CREATEMAP_CL_OPENCL)
        return fail(VSTAB_ERR_INVALID, n + ": a rotation per output row (rot_bottom) is served for map modes 0, 1 and 5");
    if (out_format != VSTAB_OUT_BGR8 && out_format != VSTAB_OUT_NV12_PLANAR)
        return fail(VSTAB_ERR_INVALID, n + ": " + who + "emits VSTAB_OUT_BGR8 or VSTAB_OUT_NV12_PLANAR (NV12 through BGR is not served)");
    if (border_mode && !border_mode_valid(*border_mode))
        return fail(VSTAB_ERR_INVALID, n + ": border_mode must be VSTAB_BORDER_CONSTANT (0), _REPLICATE (1), _REFLECT (2) or _REFLECT_101 (4)");
    const bool planar = out_format == VSTAB_OUT_NV12_PLANAR;
    if (pitch_y < (size_t)sw || pitch_uv < (size_t)sw || pitch_dst < (size_t)dw * (planar ? 1 : 3))
        return fail(VSTAB_ERR_INVALID, n + ": pitch smaller than row");
    if (planar && (!dst_uv || pitch_dst_uv < (size_t)((dw + 1) / 2) * 2))
        return fail(VSTAB_ERR_INVALID, n + ": plane-wise output needs a chroma plane of 2*ceil(width/2) bytes per row");
    if (!ptr_aligned(uv, 2) || pitch_uv % 2) return fail(VSTAB_ERR_INVALID, n + ": chroma plane must be 2-B aligned");
    WarpArgs &a = c.w;
    a.y = (const uint8_t *)y, a.uv = (const uint8_t *)uv, a.dst = (uint8_t *)dst, a.dst_uv = planar ? (uint8_t *)dst_uv : nullptr;
    a.pitch_y = pitch_y, a.pitch_uv = pitch_uv, a.pitch_dst = pitch_dst, a.pitch_dst_uv = planar ? pitch_dst_uv : 0;
    a.sw = sw, a.sh = sh, a.dw = dw, a.dh = dh;
    MapParams &p = a.p;
    p.icx = params[0], p.icy = params[1], p.ifx = params[2], p.ify = params[3];
    p.ocx = params[4], p.ocy = params[5], p.ofx = params[6], p.ofy = params[7];
    for (int i = 0; i < 9; i++) p.r[i] = params[8 + i];
    c.p32 = {params[0] * 32.0f, params[1] * 32.0f, params[2] * 32.0f, params[3] * 32.0f, params[10], params[13], params[16]};
    return VSTAB_OK;
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
// The entry points of a resampler (cubic, Lanczos) over its kernels KS: KS::warp<MODE, PLANAR, BORDER>() and KS::remap<CN, BORDER>(), the
// kernel of each combination (BORDER_CONSTANT: the kernels that carry the border value).  border_mode null: the constant-border entry points.
// ---------------------------------------------------------------------------------------------------------------------
template <typename KS>
vstab_status warp_resample(const char *name, const char *who, const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int sw, int sh,
                           const float params[17], int map_mode, int out_format, const int *border_mode, void *dst, size_t pitch_dst, void *dst_uv,
                           size_t pitch_dst_uv, int dw, int dh, void *stream) {
    CubicArgs c;
    const vstab_status st = check_warp_nv12(name, who, y, pitch_y, uv, pitch_uv, sw, sh, params, nullptr, map_mode, out_format, border_mode, dst, pitch_dst,
                                            dst_uv, pitch_dst_uv, dw, dh, c);
    if (st != VSTAB_OK) return st;
    with_map_mode(map_mode, [&](auto mode) {
        with_border_mode(border_mode ? *border_mode : VSTAB_BORDER_CONSTANT, [&](auto border) {
            with_bool(out_format == VSTAB_OUT_NV12_PLANAR, [&](auto planar) {
                launch_tiles(KS::template warp<decltype(mode)::value, decltype(planar)::value, decltype(border)::value>(), c, dw, dh, stream);
            });
        });
    });
    VSTAB_HIP_TRY(hipGetLastError());
    return VSTAB_OK;
}

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
