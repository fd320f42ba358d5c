// vstab_track.hpp -- launchers of the tracking kernels (vstab_pyramid.hip, vstab_corners.hip, vstab_corners_fused.hip, vstab_lk.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vstab.h"

namespace vstab {

constexpr int LK_MAX_LEVELS = 4;  // maxLevel 3 (calcOpticalFlowPyrLK default)
constexpr int LK_WIN = 21;        // winSize 21 x 21 (calcOpticalFlowPyrLK default); the other offered windows: lk_window_offered

struct LkPyramid {
    const uint8_t *img[LK_MAX_LEVELS];
    size_t pitch[LK_MAX_LEVELS];
    int w[LK_MAX_LEVELS], h[LK_MAX_LEVELS];
    int levels;
};

// number of levels buildOpticalFlowPyramid produces for maxLevel 3, winSize win x win
inline int lk_levels(int w, int h, int win = LK_WIN) {
    int n = 1;
    for (int l = 1; l < LK_MAX_LEVELS; l++) {
        w = (w + 1) / 2, h = (h + 1) / 2;
        if (w <= win || h <= win) break;
        n++;
    }
    return n;
}

// done (optional): an event that completes with the kernel, bound to the launch itself (no marker packet of its own on the stream)
vstab_status launch_pyr_down(const uint8_t *src, size_t spitch, int sw, int sh, uint8_t *dst, size_t dpitch, hipStream_t s, hipEvent_t done = nullptr);
// what launch_pyr_down / launch_pyr_down_x2 refuse, without the launch: VSTAB_OK, or the launcher's own status and message
vstab_status check_pyr_down(size_t spitch, int sw, int sh, size_t dpitch);
vstab_status check_pyr_down_x2(size_t spitch, int sw, int sh, size_t mpitch, size_t dpitch);
// the copy of an NV12 frame into the ring (what vstab_pack_nv12 writes: luma rows of pitch w, chroma rows behind them) and the first pyramid
// level of its luma in one launch; `copied` (optional) completes with it
bool pack_pyr_ok(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int w, int h, const void *ring, const void *dst, size_t dpitch);
vstab_status launch_pack_pyr(const uint8_t *y, size_t pitch_y, const uint8_t *uv, size_t pitch_uv, int w, int h, uint8_t *ring, uint8_t *dst, size_t dpitch, hipStream_t s,
                             hipEvent_t copied = nullptr);
// two levels in one launch: mid = pyrDown(src) ((sw+1)/2 x (sh+1)/2), dst = pyrDown(mid); only where pyr_down_x2_ok(sw, sh)
bool pyr_down_x2_ok(int sw, int sh);
vstab_status launch_pyr_down_x2(const uint8_t *src, size_t spitch, int sw, int sh, uint8_t *mid, size_t mpitch, uint8_t *dst, size_t dpitch, hipStream_t s,
                                hipEvent_t done = nullptr);
// k of the Harris response (vstab.h, "Harris response"): finite, 0 <= k < 0.25 -- from 0.25 on det - k tr^2 is never positive
inline bool harris_k_ok(double k) { return k >= 0.0 && k < 0.25; }
// 3, 5 or 7: the block sizes a kernel exists for (vstab.h, "Corner block size"; vstab_corners_block.hip holds the table)
bool corner_block_offered(int block);
// 3, 5 or 7: the gradient sizes a kernel exists for, with every block size (vstab.h, "Corner gradient size")
bool corner_gradient_offered(int gradient);
// cornerMinEigenVal(block, gradient) or, harris, cornerHarris(block, gradient, k) with kf = (float)k as a dense w x h map, and its int-bit
// maximum; with block 3 and gradient 3 exactly the launches there were before there was a block
vstab_status launch_corner_response(const uint8_t *src, size_t pitch, int w, int h, bool harris, float kf, float *resp, int *max_bits, hipStream_t s, int block = 3,
                                    int gradient = 3);
vstab_status launch_corner_response_block(const uint8_t *src, size_t pitch, int w, int h, int block, bool harris, float kf, float *resp, int *max_bits, hipStream_t s,
                                          int gradient = 3);
// What a detection reads beside the image (vstab.h, "Detection mask" and "Harris response"), as every launcher and the Detector take it:
//   mask    the detection mask, a w x h plane of bytes of pitch mask_pitch, non-zero = "a corner may be reported here"; NULL: none, the
//           launches of the unmasked detector
//   harris  cornerHarris(block, 3, k) with kf = (float)k in place of cornerMinEigenVal(block, 3) (kf is not looked at then)
//   block   goodFeaturesToTrack's blockSize, 3, 5 or 7: the window of the covariance sums; 3 makes the launches of a spec without one
//   gradient  goodFeaturesToTrack's gradientSize, 3, 5 or 7: the Sobel aperture of the derivatives; 3 makes the launches of a spec without one
// check_detect_spec (vstab_detect_host.hpp) is where the entry points refuse a bad one.
struct DetectSpec {
    const uint8_t *mask = nullptr;
    size_t mask_pitch = 0;
    bool harris = false;
    float kf = 0.0f;
    int block = 3;
    int gradient = 3;
    DetectSpec() = default;
    DetectSpec(const uint8_t *m, size_t pitch, bool h = false, float k = 0.0f, int b = 3, int g = 3)
        : mask(m), mask_pitch(m ? pitch : 0), harris(h), kf(h ? k : 0.0f), block(b), gradient(g) {}
};
// The detectors' 8 dwords of device memory (the fused launch zeroes all of them):
struct DetectorWords {
    unsigned int max;         // the frame maximum: biased float bits (unsigned order; 0 = no tile published one) from the fused kernels, int bits from the dense ones
    unsigned int masked_max;  // two-pass under a mask: the maximum over the masked-in pixels (launch_masked_max), int bits
    unsigned int pad0[2];
    unsigned int kept;        // keys above the final threshold (may exceed the key buffer's capacity: the result is complete iff it does not)
    unsigned int spilled;     // tiles of the fused detector that left a dense map (statistics)
    unsigned int pad1[2];
};
static_assert(sizeof(DetectorWords) == 32, "8 dwords");
// Harris: "this maximum says no response above zero", and then no corner -- its sign bit, in either encoding
inline bool no_positive_response(unsigned int max_word, bool biased) { return (int)(biased ? max_word ^ 0x80000000u : max_word) < 0; }
// Under a mask, max_bits of launch_corner_candidates is the MASKED maximum (launch_masked_max behind launch_corner_response); spec.harris is not looked at.
vstab_status launch_corner_candidates(const float *eig, int w, int h, const int *max_bits, double quality,
                                      unsigned long long *keys, unsigned int *count, unsigned int cap, hipStream_t s, const DetectSpec &spec = DetectSpec());
vstab_status launch_masked_max(const float *eig, int w, int h, const uint8_t *mask, size_t mpitch, int *masked_max_bits, hipStream_t s);
// The scratch of the fused detector for a w x h image, laid out in ONE place: a tile is CF_TW x CF_TH output pixels, and the buffer holds
// CF_SLOTS key slots per tile, then a dense CF_TW x CF_TH float map per tile (written only by a tile with more survivors than slots),
// then -- last -- one survivor count per tile (tile rows first).
constexpr int CF_TW = 64, CF_TH = 31, CF_SLOTS = 256;
struct CornersFusedScratch {
    int tiles_x, tiles_y, tiles;
    size_t slots_off, spill_off, counts_off, bytes;
    CornersFusedScratch(int w, int h)
        : tiles_x((w + CF_TW - 1) / CF_TW), tiles_y((h + CF_TH - 1) / CF_TH), tiles(tiles_x * tiles_y), slots_off(0),
          spill_off(slots_off + (size_t)tiles * CF_SLOTS * sizeof(unsigned long long)), counts_off(spill_off + (size_t)tiles * CF_TW * CF_TH * sizeof(float)),
          bytes(counts_off + (size_t)tiles * sizeof(unsigned int)) {}
};
size_t corners_fused_scratch_bytes(int w, int h);
vstab_status launch_corners_fused(const uint8_t *src, size_t pitch, int w, int h, double quality, void *scratch, unsigned long long *keys,
                                  unsigned int cap, DetectorWords *words, hipStream_t s, const DetectSpec &spec = DetectSpec());
// launch_corners_fused's first kernel for a (spec.block, spec.gradient) other than (3, 3) (vstab_corners_block.hip), into the same scratch; vec_ok, mvec_ok: the
// image's and the mask's base and pitch are 4-byte aligned, as launch_corners_fused found them
vstab_status launch_corners_fused_block(const uint8_t *src, size_t pitch, int w, int h, double quality, unsigned int *max_key, unsigned long long *slots,
                                        unsigned int *tile_counts, float *spill, dim3 grid, hipStream_t s, const DetectSpec &spec, int vec_ok, int mvec_ok);
// One tracker launch = a SEGMENT of up to LK_SEG_MAX consecutive frame pairs (k_lk_track): pair i is (pyr[i], pyr[i + 1]).
//   prev_pts  the n start points of pair 0 (device-readable), or NULL when
//   chain_in  the device records of the parent launch's last pair, whose sequence number is parent_seq: slot f starts from the
//             point record f holds (status 1) or reports status 2 ("lost earlier") for every pair; a record with another tag
//             is a bookkeeping error (status 3).  The parent must precede this launch on the same stream.
//   host_rec[i] / dev_rec[i] (either may be NULL): where pair i's n 16-byte records {x, seq[i], y, seq[i] << 2 | status} go --
//             mapped host memory the host polls / device memory for the launch chained behind this one
//   clk       development aid (VSTAB_LK_CLOCK): first-workgroup start / last-workgroup end stamps
// The options (vstab.h, "Tracker options") come last, so that everything k_lk_track reads stays where it was:
//   max_iter, min_eig, eps2   rules 3 and 4: the iteration cap, (float)min_eig_threshold and eps * eps in double
//   flags     VSTAB_LK_USE_INITIAL_FLOW: init_pts holds the n guesses (device-readable); VSTAB_LK_GET_MIN_EIGENVALS: what err reports
//   err       n floats (device-writable), or NULL; written with plain stores: read it behind a synchronisation of the stream
// launch_lk takes k_lk_track exactly when lk_default_launch(args), else k_lk_track_opt; flags, init_pts and err belong to a launch of ONE
// pair from host points (prev_pts) and are refused elsewhere.
constexpr int LK_SEG_MAX = 8;
struct LkSegArgs {
    LkPyramid pyr[LK_SEG_MAX + 1];
    uint4 *host_rec[LK_SEG_MAX];
    uint4 *dev_rec[LK_SEG_MAX];
    unsigned int seq[LK_SEG_MAX];
    int n_frames, n;
    const float2 *prev_pts;
    const uint4 *chain_in;
    unsigned int parent_seq;
    unsigned long long *clk;
    int max_iter;
    float min_eig;
    double eps2;
    int flags;
    const float2 *init_pts;
    float *err;
    int win;  // the window (vstab.h, "Tracker window"): picks the kernel (launch_lk), which has the size compiled in; allowed on every launch
};
// The tracker's options as an entry point takes them, checked by check_lk_options (vstab_track_host.hpp); the defaults are
// calcOpticalFlowPyrLK's.  max_level caps the pyramid (Tracker::init) and never reaches the kernel; win also sets the pyramid's depth.
struct LkOptions {
    int max_level = LK_MAX_LEVELS - 1, max_iter = 30;
    double eps = 0.01, min_eig = 1e-4;
    int win = LK_WIN;
};
inline void lk_set_options(LkSegArgs &a, const LkOptions &o) { a.max_iter = o.max_iter, a.min_eig = (float)o.min_eig, a.eps2 = o.eps * o.eps, a.win = o.win; }
// 15, 21 or 31: the windows a kernel exists for (vstab_lk_win.hip holds the table)
bool lk_window_offered(int win);
// launch_lk's second half for a window other than LK_WIN: "launch_lk: no kernel for this window" where there is none
vstab_status launch_lk_win(const LkSegArgs &args, hipStream_t s);
inline bool lk_default_launch(const LkSegArgs &a) {
    return a.max_iter == 30 && a.min_eig == 1e-4f && a.eps2 == 0.01 * 0.01 && a.flags == 0 && !a.init_pts && !a.err;
}
vstab_status launch_lk(const LkSegArgs &args, hipStream_t s);

}  // namespace vstab
