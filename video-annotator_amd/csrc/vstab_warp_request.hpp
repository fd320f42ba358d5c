// vstab_warp_request.hpp -- what an 8-bit NV12 warp entry point takes, as one struct, and the one routing from what a request asks for to
// the kernels that serve it ("Warp routing", has the table).  Host only: every stateless vstab_warp_nv12* entry point fills a
// WarpRequest and hands it to warp_nv12 (vstab_warp.hip), as does a pull (vstab_pull.cpp); warp_route is reached without a device through
// vstabx_warp_route (vstab_testhooks.cpp; tests/test_warp_routes_cpu.py).
#pragma once
#include "vstab_device.hpp"
#include "vstab_internal.hpp"

namespace vstab {

// the input lens of a request.  LENS_PINHOLE_ZERO: a rectilinear lens whose five coefficients are all zero -- the ideal pinhole
enum WarpLens { LENS_IDEAL = 0, LENS_FISHEYE = 1, LENS_PINHOLE = 2, LENS_PINHOLE_ZERO = 3 };
// The border mode of an entry point.  NONE: it has none (the constant border of its own kernels).  OWN: it exists for its border kernels,
// which serve every mode, the constant one included (vstab_warp_nv12_border, _cubic_border, _lanczos4_border).  OPTION: one option beside
// a resampler and a lens (vstab_warp_nv12_dist_ex, _rs_ex, _pinhole): INTER_LINEAR with the constant border and one rotation is the bilinear
// kernels', as it was before those entry points existed.
enum WarpBorderEntry { BORDER_ENTRY_NONE = 0, BORDER_ENTRY_OWN = 1, BORDER_ENTRY_OPTION = 2 };

// An entry point as the checks and the routing see it.  who: the subject of its output-format message ("the cubic warp "; ""); null: the
// bilinear entry points (vstab_warp_nv12_ex / _rs / _mapped / _bgr), whose messages stand under vstab_warp_nv12 and which emit
// VSTAB_OUT_NV12 as well.  lens: the lens the entry point exists for (its coefficients are required, and every map mode that lens does
// not belong to, known or not, gets the one message behind the other checks); LENS_IDEAL: whatever the request's pointers say.
struct WarpEntry {
    const char *name, *who;
    int border, lens;
};
constexpr WarpEntry ENTRY_EX = {"vstab_warp_nv12_ex", nullptr, BORDER_ENTRY_NONE, LENS_IDEAL};
constexpr WarpEntry ENTRY_RS = {"vstab_warp_nv12_rs", nullptr, BORDER_ENTRY_NONE, LENS_IDEAL};
constexpr WarpEntry ENTRY_MAPPED = {"vstab_warp_nv12_mapped", nullptr, BORDER_ENTRY_NONE, LENS_IDEAL};
constexpr WarpEntry ENTRY_DIST = {"vstab_warp_nv12_dist", "the distorted-lens warp ", BORDER_ENTRY_NONE, LENS_FISHEYE};
constexpr WarpEntry ENTRY_DIST_EX = {"vstab_warp_nv12_dist_ex", "the distorted-lens warp ", BORDER_ENTRY_OPTION, LENS_FISHEYE};
constexpr WarpEntry ENTRY_RS_EX = {"vstab_warp_nv12_rs_ex", "the per-row warp ", BORDER_ENTRY_OPTION, LENS_IDEAL};
constexpr WarpEntry ENTRY_PINHOLE = {"vstab_warp_nv12_pinhole", "the pinhole-lens warp ", BORDER_ENTRY_OPTION, LENS_PINHOLE};
constexpr WarpEntry ENTRY_BORDER = {"vstab_warp_nv12_border", "the border warp ", BORDER_ENTRY_OWN, LENS_IDEAL};
constexpr WarpEntry ENTRY_CUBIC = {"vstab_warp_nv12_cubic", "the cubic warp ", BORDER_ENTRY_NONE, LENS_IDEAL};
constexpr WarpEntry ENTRY_CUBIC_BORDER = {"vstab_warp_nv12_cubic_border", "", BORDER_ENTRY_OWN, LENS_IDEAL};
constexpr WarpEntry ENTRY_LANCZOS4 = {"vstab_warp_nv12_lanczos4", "the Lanczos warp ", BORDER_ENTRY_NONE, LENS_IDEAL};
constexpr WarpEntry ENTRY_LANCZOS4_BORDER = {"vstab_warp_nv12_lanczos4_border", "", BORDER_ENTRY_OWN, LENS_IDEAL};
constexpr WarpEntry ENTRY_COLOUR = {"vstab_warp_nv12_colour", nullptr, BORDER_ENTRY_NONE, LENS_IDEAL};  // a bilinear entry point with a colour spec
constexpr WarpEntry ENTRY_KEEP = {"vstab_warp_nv12_keep", "the keep-edge warp ", BORDER_ENTRY_NONE, LENS_IDEAL};

// One call of an 8-bit NV12 warp.  Null / zero / default where the entry point has no such argument.
struct WarpRequest {
    WarpEntry e;
    const void *y;
    size_t pitch_y;
    const void *uv;
    size_t pitch_uv;
    int sw, sh;
    const float *params;                 // [17]
    const float *rot_bottom = nullptr;   // [9]: a rotation per output row
    const float *dist = nullptr;         // [4]: k1..k4 of a fisheye input lens
    const float *pinhole = nullptr;      // [5]: k1, k2, p1, p2, k3 of a rectilinear input lens
    const void *qmap = nullptr;          // the quantised map of vstab_quantised_map, its pitch in pixels
    int qpitch = 0;
    bool keep = false;                   // a keep-edge warp: prev is the frame to keep
    const void *prev = nullptr;
    size_t pitch_prev = 0;
    const void *prev_uv = nullptr;
    size_t pitch_prev_uv = 0;
    int map_mode = VSTAB_MAP_CREATEMAP_CL, resample = VSTAB_RESAMPLE_DEFAULT, border_mode = VSTAB_BORDER_CONSTANT, out_format = VSTAB_OUT_BGR8;
    void *dst;
    size_t pitch_dst;
    void *dst_uv;
    size_t pitch_dst_uv;
    int dw, dh;
    void *stream;
    // the colour spec (vstab_warp_nv12_colour, vstab_set_colour); the default: cvtColor's arithmetic, every kernel as it was.  The routing does
    // not look at it: a spec other than the default is served by the COLOUR instantiations of the route's own fused kernel, or refused
    // (launch_warp_bilinear).
    int colour_matrix = VSTAB_COLOUR_CVTCOLOR, colour_range = VSTAB_RANGE_LIMITED;

    bool colour() const { return colour_matrix != VSTAB_COLOUR_CVTCOLOR || colour_range != VSTAB_RANGE_LIMITED; }
    bool planar() const { return out_format == VSTAB_OUT_NV12_PLANAR; }
    int lens() const {
        if (dist) return LENS_FISHEYE;
        if (!pinhole) return LENS_IDEAL;
        return pinhole[0] == 0.0f && pinhole[1] == 0.0f && pinhole[2] == 0.0f && pinhole[3] == 0.0f && pinhole[4] == 0.0f ? LENS_PINHOLE_ZERO : LENS_PINHOLE;
    }
};

// The request checked once, routed once and launched once (vstab_warp.hip).  A profiler's event pair is taken by the launch, or stays
// pending where the request is refused.
vstab_status warp_nv12(const WarpRequest &q);

// ---------------------------------------------------------------------------------------------------------------------
// The routing.  family: the kernels; block: the argument block they take; mode: their MODE template argument.
//   WARP_FUSED   k_warp_fused -- or, for a plain mode-0 BGR8 warp of planes of 4 GiB and more, the direct-gather k_warp_nv12_bgr (the
//                planes decide that at the launch, not the request); WARP_PLANAR: k_warp_planar
//   mode         MAP_* of the map mode; MAP_RS_* with a rotation per row; MAP_FISHD_* / MAP_RS_FISHD_TO_RECT through a calibrated fisheye
//                lens; MAP_RECTD_* through a rectilinear lens with coefficients.  The kernels that take a BorderArgs or a KeepArgs have the
//                rotation per row as a template argument of its own beside the base mode of MAP_RS_0 / _1 / _5 (route_kernel_mode).
// ---------------------------------------------------------------------------------------------------------------------
enum WarpFamily { WARP_NONE = 0, WARP_FUSED = 1, WARP_PLANAR = 2, WARP_BORDER = 3, WARP_CUBIC = 4, WARP_LANCZOS4 = 5, WARP_KEEP = 6 };
enum WarpBlock { ARGS_WARP = 0, ARGS_CUBIC = 1, ARGS_BORDER = 2, ARGS_KEEP = 3 };
struct WarpRoute {
    int family, block, mode;
};
constexpr int route_kernel_mode(int mode) { return mode == MAP_RS_FISHD_TO_RECT ? mode : map_mode_base(mode); }
// the mode tag of a checked (map mode, lens, rotation per row): rs with map modes 0, 1 and 5, a fisheye lens's coefficients with 1 and 2 (so
// with 1 alone under rs), a rectilinear lens's with 3 and 4
constexpr int kernel_mode_tag(int map_mode, int lens, bool rs) {
    if (lens == LENS_PINHOLE) return map_mode == VSTAB_MAP_RECT_TO_RECT ? MAP_RECTD_TO_RECT : MAP_RECTD_TO_FISH;
    if (lens == LENS_FISHEYE) return rs ? MAP_RS_FISHD_TO_RECT : map_mode == VSTAB_MAP_FISH_TO_RECT ? MAP_FISHD_TO_RECT : MAP_FISHD_TO_FISH;
    if (!rs) return map_mode;
    return map_mode == VSTAB_MAP_CREATEMAP_CL ? MAP_RS_CREATEMAP_CL : map_mode == VSTAB_MAP_FISH_TO_RECT ? MAP_RS_FISH_TO_RECT : MAP_RS_CREATEMAP_CL_OPENCL;
}

// Pure: integers in, the route out; WARP_NONE where nothing serves the combination (the argument checks refuse all of those but one, a
// quantised map with VSTAB_OUT_NV12_PLANAR, which launch_warp_bilinear refuses).  border_entry: WarpBorderEntry; lens: WarpLens.
inline WarpRoute warp_route(int map_mode, int lens, bool rs, int resample, int border_entry, int border_mode, int out_format, bool keep, bool qmap) {
    const WarpRoute none = {WARP_NONE, ARGS_WARP, 0};
    const bool fish_to_pinhole = map_mode == VSTAB_MAP_CREATEMAP_CL || map_mode == VSTAB_MAP_FISH_TO_RECT || map_mode == VSTAB_MAP_CREATEMAP_CL_OPENCL;
    const bool cubic = resample == VSTAB_RESAMPLE_CUBIC, resampled = cubic || resample == VSTAB_RESAMPLE_LANCZOS4;
    const bool constant = border_mode == VSTAB_BORDER_CONSTANT, planar = out_format == VSTAB_OUT_NV12_PLANAR;
    if (map_mode < VSTAB_MAP_CREATEMAP_CL || map_mode > VSTAB_MAP_CREATEMAP_CL_OPENCL || (rs && !fish_to_pinhole)) return none;
    if (!resampled && resample != VSTAB_RESAMPLE_DEFAULT) return none;
    if (!border_mode_valid(border_mode) || (border_entry == BORDER_ENTRY_NONE && !constant)) return none;
    if (lens == LENS_FISHEYE && !map_mode_takes_distortion(map_mode)) return none;
    if ((lens == LENS_PINHOLE || lens == LENS_PINHOLE_ZERO) && !map_mode_takes_pinhole(map_mode)) return none;
    const bool ideal = lens == LENS_IDEAL || lens == LENS_PINHOLE_ZERO;  // all five zero: what served the ideal pinhole before
    // NV12 through BGR: the bilinear entry points alone
    if (out_format == VSTAB_OUT_NV12 ? !ideal || resampled || keep || border_entry != BORDER_ENTRY_NONE : out_format != VSTAB_OUT_BGR8 && !planar) return none;
    const int bilinear = planar ? WARP_PLANAR : WARP_FUSED, resampler = cubic ? WARP_CUBIC : WARP_LANCZOS4;
    const int mode = kernel_mode_tag(map_mode, ideal ? (int)LENS_IDEAL : lens, rs);
    if (keep) return ideal && !resampled && !qmap && constant ? WarpRoute{WARP_KEEP, ARGS_KEEP, mode} : none;
    // the map written down: the CACHED kernels exist under MAP_CREATEMAP_CL, whatever mode the map was made in, and hold no chroma positions
    if (qmap) return ideal && !rs && !resampled && constant && !planar ? WarpRoute{WARP_FUSED, ARGS_WARP, MAP_CREATEMAP_CL} : none;
    // a rectilinear lens with coefficients (one rotation: map modes 3 and 4), a calibrated fisheye lens with a rotation per row (map mode 1:
    // the one mode both admit): the kernels that take a BorderArgs, under every resampler and border mode
    if (lens == LENS_PINHOLE || (lens == LENS_FISHEYE && rs)) return {resampled ? resampler : WARP_BORDER, ARGS_BORDER, mode};
    if (resampled) return {resampler, rs ? ARGS_BORDER : ARGS_CUBIC, mode};
    // INTER_LINEAR.  The bilinear kernels have the constant border built in; through an ideal lens they serve the entry points without a
    // border mode and, with one rotation, the constant border of the entry points where the border mode is an option.
    if (lens == LENS_FISHEYE ? constant : border_entry == BORDER_ENTRY_NONE || (border_entry == BORDER_ENTRY_OPTION && constant && !rs))
        return {bilinear, ARGS_WARP, mode};
    return {WARP_BORDER, ARGS_BORDER, mode};
}
inline WarpRoute warp_route(const WarpRequest &q) {
    return warp_route(q.map_mode, q.lens(), q.rot_bottom != nullptr, q.resample, q.e.border, q.border_mode, q.out_format, q.keep, q.qmap != nullptr);
}

}  // namespace vstab
