// vstab_corners_block.hip -- the corner detector's kernels for the block sizes other than 3 (vstab.h, "Corner block size":
// goodFeaturesToTrack's blockSize 5 and 7).  Each is vstab_corners_block.hpp included with its size, in a namespace of its own: one
// one-pass kernel and one dense-map kernel per size.  A further size is one more inclusion and one more entry of CB_KERNELS.
// launch_corners_fused (vstab_corners_fused.hip) and launch_corner_response (vstab_corners.hip) come here for a block other than 3;
// k_filter_keys, k_masked_max and the candidate kernels behind them serve every size.  Compiled with -ffp-contract=off.
#include <climits>

#include "vstab_internal.hpp"
#include "vstab_track.hpp"
#include "vstab_track_device.hpp"

#define VSTAB_CB_B 5
#include "vstab_corners_block.hpp"
#undef VSTAB_CB_B

#define VSTAB_CB_B 7
#include "vstab_corners_block.hpp"
#undef VSTAB_CB_B

namespace vstab {

namespace {
struct CornerBlockKernels {
    int block;
    void (*fused)(const uint8_t *, size_t, int, int, double, unsigned int *, unsigned long long *, unsigned int *, float *, int, const uint8_t *, size_t, int, int, float);
    void (*dense)(const uint8_t *, size_t, int, int, float *, int *, int, int, float);
};
constexpr CornerBlockKernels CB_KERNELS[] = {{5, cb5::k_corners_fused_block, cb5::k_corner_response_block}, {7, cb7::k_corners_fused_block, cb7::k_corner_response_block}};

const CornerBlockKernels *kernels_for(int block) {
    for (const CornerBlockKernels &k : CB_KERNELS)
        if (k.block == block) return &k;
    return nullptr;
}
}  // namespace

bool corner_block_offered(int block) { return block == 3 || kernels_for(block) != nullptr; }

// the first kernel of launch_corners_fused for spec.block other than 3: same grid, same scratch, same words
vstab_status launch_corners_fused_block(const uint8_t *src, size_t pitch, int w, int h, double quality, unsigned int *max_key, unsigned long long *slots,
                                        unsigned int *tile_counts, float *spill, dim3 grid, hipStream_t s, const DetectSpec &spec) {
    const CornerBlockKernels *k = kernels_for(spec.block);
    if (!k) return fail(VSTAB_ERR_INVALID, "launch_corners_fused: no kernel for this block size");
    const int vec_ok = reinterpret_cast<uintptr_t>(src) % 4 == 0 && pitch % 4 == 0;
    const int mvec_ok = reinterpret_cast<uintptr_t>(spec.mask) % 4 == 0 && spec.mask_pitch % 4 == 0;
    hipLaunchKernelGGL(k->fused, grid, dim3(256), 0, s, src, pitch, w, h, quality, max_key, slots, tile_counts, spill, vec_ok, spec.mask, spec.mask_pitch, mvec_ok,
                       (int)spec.harris, spec.kf);
    VSTAB_HIP_TRY(hipGetLastError());
    return VSTAB_OK;
}

// launch_corner_response's kernel for a block other than 3 (max_bits is initialised there)
vstab_status launch_corner_response_block(const uint8_t *src, size_t pitch, int w, int h, int block, bool harris, float kf, float *resp, int *max_bits, hipStream_t s) {
    const CornerBlockKernels *k = kernels_for(block);
    if (!k) return fail(VSTAB_ERR_INVALID, "launch_corner_response: no kernel for this block size");
    const int vec_ok = reinterpret_cast<uintptr_t>(src) % 4 == 0 && pitch % 4 == 0;
    hipLaunchKernelGGL(k->dense, dim3(div_up(w, CF_TW), div_up(h, CF_TH)), dim3(256), 0, s, src, pitch, w, h, resp, max_bits, vec_ok, (int)harris, kf);
    VSTAB_HIP_TRY(hipGetLastError());
    return VSTAB_OK;
}

// this unit's code object (vstab_preload_kernels)
vstab_status preload_corner_block_kernels() {
    hipFuncAttributes at;
    VSTAB_HIP_TRY(hipFuncGetAttributes(&at, reinterpret_cast<const void *>(CB_KERNELS[0].fused)));
    return VSTAB_OK;
}

}  // namespace vstab
