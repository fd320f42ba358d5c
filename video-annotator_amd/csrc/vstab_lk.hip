// vstab_lk.hip -- pyramidal Lucas-Kanade tracker for gfx950.  Replaces the OpenCV call at FrameSourceWarp.cpp:252
// (calcOpticalFlowPyrLK).  Compiled with -ffp-contract=off: float results are bit-reproducible.
// The device code is vstab_lk_window.hpp, a text in the window size: this unit is its 21 x 21 instance -- k_lk_track and k_lk_track_opt,
// the kernels of every launch with calcOpticalFlowPyrLK's default winSize -- and the launcher of all sizes.  The kernels of the other
// offered windows are vstab_lk_win.hip, a code object of their own.
#include <climits>
#include <cstddef>

#include "vstab_internal.hpp"
#include "vstab_track.hpp"
#include "vstab_track_device.hpp"

#define VSTAB_LK_W 21
#include "vstab_lk_window.hpp"
#undef VSTAB_LK_W

namespace vstab {

static_assert(LKW == LK_WIN, "this unit holds the default window's kernels");

vstab_status launch_lk(const LkSegArgs &a, hipStream_t s) {
    if (a.n <= 0 || a.n_frames <= 0) return VSTAB_OK;
    if (a.n_frames > LK_SEG_MAX) return fail(VSTAB_ERR_INVALID, "launch_lk: too many frame pairs in one launch");
    if (!a.prev_pts && !a.chain_in) return fail(VSTAB_ERR_INVALID, "launch_lk: no input points");
    for (int i = 0; i <= a.n_frames; i++) {
        // (the kernel indexes the pyramid with levels - 1 before it tests anything else)
        if (a.pyr[i].levels < 1 || a.pyr[i].levels > LK_MAX_LEVELS) return fail(VSTAB_ERR_INVALID, "launch_lk: a pyramid has 1 .. LK_MAX_LEVELS levels");
        for (int l = 0; l < a.pyr[i].levels; l++)
            if (a.pyr[i].pitch[l] >= (1u << 24) || (uint64_t)a.pyr[i].pitch[l] * (uint64_t)a.pyr[i].h[l] >= (1ull << 32))
                return fail(VSTAB_ERR_INVALID, "launch_lk: image pitch must be below 2^24 and planes below 4 GiB");
    }
    if (a.max_iter < 1 || !(a.min_eig >= 0.0f) || !(a.eps2 >= 0.0)) return fail(VSTAB_ERR_INVALID, "launch_lk: the tracker's options are not set (lk_set_options)");
    if ((a.flags & ~(VSTAB_LK_USE_INITIAL_FLOW | VSTAB_LK_GET_MIN_EIGENVALS)) || ((a.flags & VSTAB_LK_USE_INITIAL_FLOW) != 0) != (a.init_pts != nullptr) ||
        ((a.flags & VSTAB_LK_GET_MIN_EIGENVALS) && !a.err))
        return fail(VSTAB_ERR_INVALID, "launch_lk: flags, guesses and err do not agree");
    if ((a.flags || a.err) && (a.n_frames != 1 || !a.prev_pts || a.chain_in))
        return fail(VSTAB_ERR_INVALID, "launch_lk: the initial flow and err belong to a launch of one frame pair from host points");
    // the window (vstab.h, "Tracker window"): any other than 21 has ONE kernel, whatever the options, on segments and chained launches too
    if (a.win != LK_WIN) return launch_lk_win(a, s);
    if (lk_default_launch(a)) hipLaunchKernelGGL(k_lk_track, dim3(a.n), dim3(LK_THREADS), 0, s, a);
    else hipLaunchKernelGGL(k_lk_track_opt, dim3(a.n), dim3(LK_THREADS), 0, s, a);
    VSTAB_HIP_TRY(hipGetLastError());
    return VSTAB_OK;
}

// Kernels of this translation unit are one code object, loaded by the runtime at the first launch of any of them.  Touching one of them
// here (vstab_preload_kernels) moves that load to a moment the caller chooses.
vstab_status preload_lk_kernels() {
    hipFuncAttributes at;
    VSTAB_HIP_TRY(hipFuncGetAttributes(&at, reinterpret_cast<const void *>(&k_lk_track)));
    return VSTAB_OK;
}

}  // namespace vstab
