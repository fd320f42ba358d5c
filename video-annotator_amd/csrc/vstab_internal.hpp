// vstab_internal.hpp -- host-side helpers shared by the translation units of libvstab.so.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <string>

#include "../../include/vstab.h"

namespace vstab {

void set_error(const std::string &msg);

inline vstab_status fail(vstab_status st, const std::string &msg) {
    set_error(msg);
    return st;
}

#define VSTAB_HIP_TRY(expr)                                                                     \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess)                                                                   \
            return ::vstab::fail(VSTAB_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

inline unsigned div_up(unsigned a, unsigned b) { return (a + b - 1) / b; }

// One-shot event pair for the NEXT hot-kernel launch on this thread: the launcher hands it to hipExtLaunchKernelGGL, which
// stamps the kernel's own start and end (what rocprofv3's kernel trace reports) instead of the stream positions around the
// launch call, whose interval also holds the dispatch wait behind other streams' kernels.  take_launch_events() clears it.
struct LaunchEvents {
    hipEvent_t start = nullptr, stop = nullptr;
};
void set_launch_events(hipEvent_t start, hipEvent_t stop);
LaunchEvents take_launch_events();

// one per translation unit with kernels: loads that unit's code object now (vstab_preload_kernels)
vstab_status preload_pyramid_kernels();
vstab_status preload_corner_kernels();
vstab_status preload_corners_fused_kernels();
vstab_status preload_corner_block_kernels();
vstab_status preload_lk_kernels();
vstab_status preload_lk_win_kernels();
vstab_status preload_plane_kernels();
vstab_status preload_warp_kernels();
vstab_status preload_fused_kernels();
vstab_status preload_p010_kernels();
vstab_status preload_planar_kernels();
vstab_status preload_cubic_kernels();
vstab_status preload_lanczos4_kernels();
vstab_status preload_border_kernels();
vstab_status preload_keep_kernels();
vstab_status preload_p010_resample_kernels();
bool launch_events_pending();

// the cv::BorderTypes the border warps serve (vstab_warp_nv12_border, vstab_warp_nv12_cubic_border / _lanczos4_border, vstab_set_border_mode / _ex)
inline bool border_mode_valid(int m) {
    return m == VSTAB_BORDER_CONSTANT || m == VSTAB_BORDER_REPLICATE || m == VSTAB_BORDER_REFLECT || m == VSTAB_BORDER_REFLECT_101;
}

// The keep-edge entry points' history (include/vstab.h, "Keep edges"): each plane of prev beside the plane of dst it stands for.  prev is dst
// itself -- same pointer and same pitch, in every plane: in place -- or its bytes overlap no plane of dst.  The stateless entry points ask
// this behind their other checks, the pulls before a frame is dequeued; every message stands under the caller's name n.
struct KeepPlane {
    const void *prev;
    size_t pitch_prev;
    const void *dst;
    size_t pitch_dst, row_bytes;
    int rows;
};
inline vstab_status check_keep_prev(const char *n, const KeepPlane *pl, int planes, bool &in_place) {
    for (int k = 0; k < planes; k++)
        if (!pl[k].prev) return fail(VSTAB_ERR_INVALID, std::string(n) + ": null pointer");
    for (int k = 0; k < planes; k++)
        if (pl[k].pitch_prev < pl[k].row_bytes) return fail(VSTAB_ERR_INVALID, std::string(n) + ": prev pitch smaller than row");
    int same = 0;
    for (int k = 0; k < planes; k++) same += pl[k].prev == pl[k].dst && pl[k].pitch_prev == pl[k].pitch_dst;
    in_place = same == planes;
    bool overlap = same != 0 && !in_place;  // one plane in place, the other not
    for (int k = 0; k < planes && !in_place; k++)
        for (int m = 0; m < planes; m++) {
            const uintptr_t p0 = reinterpret_cast<uintptr_t>(pl[k].prev), d0 = reinterpret_cast<uintptr_t>(pl[m].dst);
            const uintptr_t p1 = p0 + pl[k].pitch_prev * (size_t)(pl[k].rows - 1) + pl[k].row_bytes;
            const uintptr_t d1 = d0 + pl[m].pitch_dst * (size_t)(pl[m].rows - 1) + pl[m].row_bytes;
            overlap = overlap || (p0 < d1 && d0 < p1);
        }
    if (overlap) return fail(VSTAB_ERR_INVALID, std::string(n) + ": prev must be dst itself (same pointer and pitch, every plane) or must not overlap it");
    return VSTAB_OK;
}

// k1..k4 of a fisheye lens as every entry point that takes them accepts them (vstab_geometry.cpp; n: its name, a string only in a refusal):
// all finite, and theta_d increasing
// on [0, pi/2] -- the warp kernels' perimeter probe bounds a tile's source box only for a map that does not fold
vstab_status check_distortion(const char *n, const double D[4]);
inline vstab_status check_distortion(const char *n, const float D[4]) {
    const double d[4] = {D[0], D[1], D[2], D[3]};
    return check_distortion(n, d);
}
// the map modes whose input camera is a fisheye lens, i.e. the ones the distortion belongs to
inline bool map_mode_takes_distortion(int map_mode) { return map_mode == VSTAB_MAP_FISH_TO_RECT || map_mode == VSTAB_MAP_FISH_TO_FISH; }

// (k1, k2, p1, p2, k3) of a rectilinear lens as every *_pinhole entry point accepts them: all five finite, in fp64 and after the cast to
// fp32.  No monotonicity rule: the kernels that serve them take a tile's box as the exact reduction of the tile's own map.
inline vstab_status check_pinhole_distortion(const char *n, const double D[5]) {
    for (int i = 0; i < 5; i++)
        if (!std::isfinite(D[i]) || !std::isfinite((float)D[i])) return fail(VSTAB_ERR_INVALID, std::string(n) + ": the five distortion coefficients must be finite");
    return VSTAB_OK;
}
inline vstab_status check_pinhole_distortion(const char *n, const float D[5]) {
    const double d[5] = {D[0], D[1], D[2], D[3], D[4]};
    return check_pinhole_distortion(n, d);
}
// the map modes whose input camera is rectilinear, i.e. the ones those coefficients belong to
inline bool map_mode_takes_pinhole(int map_mode) { return map_mode == VSTAB_MAP_RECT_TO_RECT || map_mode == VSTAB_MAP_RECT_TO_FISH; }

// vstab_pack_p010 with a choice of planes (vstab_plane_ops.hip): luma_only narrows the luma plane alone -- what the 10-bit
// pipeline needs for its tracker
vstab_status pack_p010_planes(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int width, int height, void *dst, bool luma_only,
                              void *stream);

// vstab_pack_nv12 with an optional event that completes with the copy kernel (bound to the launch: no marker packet on the stream)
vstab_status pack_nv12_planes(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int width, int height, void *dst, void *stream, hipEvent_t done);

#define VSTAB_TRY(expr)                   \
    do {                                  \
        vstab_status st_ = (expr);        \
        if (st_ != VSTAB_OK) return st_;  \
    } while (0)

struct DevBuf {
    void *p = nullptr;
    size_t n = 0;
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr, n = 0;
    }
    vstab_status ensure(size_t bytes) {
        if (bytes <= n) return VSTAB_OK;
        release();
        if (hipMalloc(&p, bytes) != hipSuccess) return fail(VSTAB_ERR_NOMEM, "hipMalloc failed");
        n = bytes;
        return VSTAB_OK;
    }
    template <typename T>
    T *as() const { return static_cast<T *>(p); }
};

struct PinnedBuf {  // host memory the device can read and write directly (mapped, coherent)
    void *p = nullptr;
    size_t n = 0;
    void *dev() const {
        void *d = nullptr;
        return hipHostGetDevicePointer(&d, p, 0) == hipSuccess ? d : nullptr;
    }
    ~PinnedBuf() {
        if (p) (void)hipHostFree(p);
    }
    vstab_status ensure(size_t bytes) {
        if (bytes <= n) return VSTAB_OK;
        if (p) (void)hipHostFree(p);
        p = nullptr, n = 0;
        if (hipHostMalloc(&p, bytes, hipHostMallocMapped | hipHostMallocPortable | hipHostMallocCoherent) != hipSuccess) return fail(VSTAB_ERR_NOMEM, "hipHostMalloc failed");
        n = bytes;
        return VSTAB_OK;
    }
    template <typename T>
    T *as() const { return static_cast<T *>(p); }
};

}  // namespace vstab
