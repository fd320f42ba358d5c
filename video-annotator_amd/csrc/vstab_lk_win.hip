// vstab_lk_win.hip -- the tracker kernels of the windows other than 21 x 21 (vstab.h, "Tracker window"): calcOpticalFlowPyrLK's winSize
// 15 and 31.  Each is vstab_lk_window.hpp included with its size -- the body, the four-wave organisation, the segment and chain protocol,
// the fetch-ahead, the options and both err modes of k_lk_track_opt (vstab_lk.hip) -- in a namespace of its own.  A further size is one
// more inclusion and one more entry of LK_WIN_KERNELS.  Compiled with -ffp-contract=off, as vstab_lk.hip is.
#include <climits>
#include <cstddef>

#include "vstab_internal.hpp"
#include "vstab_track.hpp"
#include "vstab_track_device.hpp"

#define VSTAB_LK_W 15
#include "vstab_lk_window.hpp"
#undef VSTAB_LK_W

#define VSTAB_LK_W 31
#include "vstab_lk_window.hpp"
#undef VSTAB_LK_W

namespace vstab {

namespace {
struct LkWinKernel {
    int win;
    void (*kernel)(LkSegArgs);
};
constexpr LkWinKernel LK_WIN_KERNELS[] = {{15, lkw15::k_lk_track_win}, {31, lkw31::k_lk_track_win}};
}  // namespace

bool lk_window_offered(int win) {
    if (win == LK_WIN) return true;
    for (const LkWinKernel &k : LK_WIN_KERNELS)
        if (k.win == win) return true;
    return false;
}

// launch_lk (vstab_lk.hip) has checked the launch; here only the window picks the kernel.  The block is the 256 threads of every tracker
// kernel (one workgroup of four waves per feature slot).
vstab_status launch_lk_win(const LkSegArgs &a, hipStream_t s) {
    for (const LkWinKernel &k : LK_WIN_KERNELS)
        if (k.win == a.win) {
            hipLaunchKernelGGL(k.kernel, dim3(a.n), dim3(256), 0, s, a);
            VSTAB_HIP_TRY(hipGetLastError());
            return VSTAB_OK;
        }
    return fail(VSTAB_ERR_INVALID, "launch_lk: no kernel for this window");
}

// this unit's code object (vstab_preload_kernels)
vstab_status preload_lk_win_kernels() {
    hipFuncAttributes at;
    VSTAB_HIP_TRY(hipFuncGetAttributes(&at, reinterpret_cast<const void *>(LK_WIN_KERNELS[0].kernel)));
    return VSTAB_OK;
}

}  // namespace vstab
