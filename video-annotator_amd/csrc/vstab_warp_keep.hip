// vstab_warp_keep.hip -- the keep-edge warp for gfx950: cv::remap's INTER_LINEAR where the 2 x 2 footprint lies wholly inside the plane it
// reads, the caller's previous frame everywhere else (vid.stab's `keep` border; cv::remap's BORDER_TRANSPARENT for 1- and 2-channel data).
// The fused NV12 -> BGR8 warp, the plane-wise NV12 -> NV12 warp and the stateless remap of map planes.  Definition (include/vstab.h, "Keep
// edges"; tests/warp_def.py): the map quantised to 1/32 pixel as everywhere; a sample is WRITTEN iff 0 <= X <= len_x - 2 and
// 0 <= Y <= len_y - 2, with the bytes of the bilinear warp ((sum of four products + 512) >> 10); every other sample is KEPT: dst receives
// the byte of prev at the same position, or is not stored at all when prev is dst (in place).
//
// The warp kernels (k_warp_keep) are the resamplers' tile (vstab_resample.hpp; k_warp_border's phases with its tap, map and blend): 64 x 16
// output pixels, one workgroup of 256 threads, four rows per thread:
//   1. map      the exact map of the thread's four pixels in registers (the per-row rotation of vstab_warp_nv12_rs where RS), quantised;
//   2. box      min / max of X .. X + 1 and Y .. Y + 1 over the WRITTEN pixels of the tile, reduced over the workgroup: a box always lies
//               inside the source; a thread with no written pixel gives no anchor, a tile with none has no box;
//   3. stage    each position of the box read once, as it is (no border value, no fold), converted (BGRx dwords; luma bytes / chroma pairs);
//   4. blend    written pixels: 4 LDS reads at their natural alignment, v_dot2_i32_i16 on channel pairs gathered by v_perm_b32 -- from global
//               memory with the same arithmetic when the box is over the LDS budget; kept pixels: prev's bytes, or nothing in place.
// A tile without a written sample in a plane neither stages nor blends that plane: it copies the tile's rows from prev, 16 bytes per lane
// where both planes allow it, or does nothing in place.
#include "vstab_warp_host.hpp"

namespace vstab {

struct KeepArgs {
    BorderArgs b;
    const uint8_t *prev, *prev_uv;  // the frame to keep; prev_uv: the plane-wise output's chroma plane
    size_t pitch_prev, pitch_prev_uv;
    int in_place;       // prev is dst (every plane): kept samples are not stored
    int vec, vec_uv;    // prev, dst and both pitches of the plane are 16-byte aligned: a tile without a written sample copies 16 bytes per lane
};

// the tap as quantised (border_tap of a non-constant mode: no clamp towards the source -- a kept sample's tap is never read)
__device__ __forceinline__ BorderTap keep_tap(float ax32, float ay32) { return border_tap<VSTAB_BORDER_REPLICATE>(ax32, ay32, 0, 0); }
// cv::remap's inlier test (unsigned)X < w - 1, (unsigned)Y < h - 1: the whole footprint inside (len 1: never)
__device__ __forceinline__ bool keep_written(const BorderTap &t, int w, int h) { return (unsigned)t.X < (unsigned)(w - 1) && (unsigned)t.Y < (unsigned)(h - 1); }

// the four taps of a written sample: from the staged box, or from the source (every tap is inside it)
template <typename T, typename Src>
__device__ __forceinline__ void keep_taps(const Src &s, const TileBox &b, const T *lds, const BorderTap &t, uint32_t (&v)[4]) {
    if (b.lds) {
        const T *q = lds + (t.Y - b.y0) * b.w + (t.X - b.x0);
        lds_row<2>(q, v), lds_row<2>(q + b.w, v + 2);
    } else {
        v[0] = s.at(t.X, t.Y), v[1] = s.at(t.X + 1, t.Y), v[2] = s.at(t.X, t.Y + 1), v[3] = s.at(t.X + 1, t.Y + 1);
    }
}

// A tile without a written sample: its ROWS rows of 16 * CHUNKS bytes from byte b0 of row r0 on, copied from prev -- 16 bytes per lane
// (vec), bytes otherwise and in the chunk that the plane's right edge (row_bytes) cuts; rows below the plane (rows) are left alone
template <int CHUNKS, int ROWS>
__device__ __forceinline__ void keep_copy_tile(const uint8_t *prev, size_t pitch_prev, uint8_t *dst, size_t pitch_dst, int b0, int row_bytes, int r0, int rows,
                                               bool vec) {
    for (int i = threadIdx.x; i < CHUNKS * ROWS; i += 256) {
        const int r = r0 + i / CHUNKS, c = b0 + (i % CHUNKS) * 16;
        if (r >= rows || c >= row_bytes) continue;
        const uint8_t *s = prev + (size_t)r * pitch_prev + c;
        uint8_t *d = dst + (size_t)r * pitch_dst + c;
        if (vec && c + 16 <= row_bytes) {
            *reinterpret_cast<uint4 *>(d) = *reinterpret_cast<const uint4 *>(s);
        } else {
            const int n = min(16, row_bytes - c);
            for (int k = 0; k < n; k++) d[k] = s[k];
        }
    }
}

// k_warp_keep -- NV12 in; PLANAR false: BGR8 out (cvtColor, then the keep-edge remap over the full-size frame); PLANAR true: the plane-wise
// warp (luma over the source; the interleaved chroma plane decided on its own, at the even pixels' positions halved over the chroma
// plane's size, U and V together).  MODE: map modes 0 .. 5, RS with modes 0 / 1 / 5.
// Six waves per SIMD, the six workgroups per CU the LDS budget allows: left to itself the compiler gave the plane-wise kernels 87 VGPRs
// (five waves) where k_warp_border's have 78; held to six it needs 72, and no scratch (profiles/keep_edges_4k.txt).
template <int MODE, bool PLANAR, bool RS>
__global__ void __launch_bounds__(256, 6) k_warp_keep(KeepArgs ka) {
    const BorderArgs &ba = ka.b;
    const WarpArgs &a = ba.c.w;
    __shared__ __attribute__((aligned(16))) uint8_t stage[RESAMPLE_LDS_BYTES];
    __shared__ __attribute__((aligned(16))) int red[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = blockIdx.x * RESAMPLE_TW + lane, y0 = blockIdx.y * RESAMPLE_TH + wave * RESAMPLE_RW;
    const float rfx = rcp_refined(a.p.ofx), rfy = rcp_refined(a.p.ofy);
    // 1. map (pixels right of / below the image are evaluated as the last column / row: never stored, and their anchors are that pixel's)
    // 2. box of the luma / BGR taps: the written pixels alone
    BorderTap t[RESAMPLE_RW];
    float ax[RESAMPLE_RW], ay[RESAMPLE_RW];
    unsigned wr = 0;  // bit j: pixel j of the thread is written
    int mnx = INT_MAX, mxx = INT_MIN, mny = INT_MAX, mxy = INT_MIN;
#pragma unroll
    for (int j = 0; j < RESAMPLE_RW; j++) {
        border_map<MODE, RS>(ba, min(x, a.dw - 1), min(y0 + j, a.dh - 1), rfx, rfy, ax[j], ay[j]);
        t[j] = keep_tap(ax[j], ay[j]);
        if (keep_written(t[j], a.sw, a.sh)) wr |= 1u << j, mnx = min(mnx, t[j].X), mxx = max(mxx, t[j].X), mny = min(mny, t[j].Y), mxy = max(mxy, t[j].Y);
    }
    if constexpr (!PLANAR) {
        const BorderNv12Bgr<VSTAB_BORDER_CONSTANT> src = {a.y, a.uv, a.pitch_y, a.pitch_uv, a.sw, a.sh};
        uint32_t *lds = reinterpret_cast<uint32_t *>(stage);
        const TileBox b = tile_box<0, 2, true>(mnx, mxx, mny, mxy, red, RESAMPLE_LDS_BYTES / 4);
        if (b.w == 0) {  // no written sample in the tile (uniform: every thread leaves here, behind tile_box's barriers)
            if (!ka.in_place)
                keep_copy_tile<RESAMPLE_TW * 3 / 16, RESAMPLE_TH>(ka.prev, ka.pitch_prev, a.dst, a.pitch_dst, blockIdx.x * RESAMPLE_TW * 3, a.dw * 3,
                                                                 blockIdx.y * RESAMPLE_TH, a.dh, ka.vec);
            return;
        }
        // 3. stage (the box is inside the source: stage_box reads it as it is)
        if (b.lds) stage_box<VSTAB_BORDER_CONSTANT, true>(src, b, lds);
        __syncthreads();
        // 4. blend the written pixels, keep the others
#pragma unroll
        for (int j = 0; j < RESAMPLE_RW; j++) {
            const int y = y0 + j;
            if (x >= a.dw || y >= a.dh) continue;
            uint8_t *o = a.dst + (size_t)y * a.pitch_dst + (size_t)x * 3;
            if (wr & (1u << j)) {
                uint32_t v[4];
                keep_taps(src, b, lds, t[j], v);
                o[0] = (uint8_t)border_channel<0>(v[0], v[1], v[2], v[3], t[j]);
                o[1] = (uint8_t)border_channel<1>(v[0], v[1], v[2], v[3], t[j]);
                o[2] = (uint8_t)border_channel<2>(v[0], v[1], v[2], v[3], t[j]);
            } else if (!ka.in_place) {
                const uint8_t *p = ka.prev + (size_t)y * ka.pitch_prev + (size_t)x * 3;
                o[0] = p[0], o[1] = p[1], o[2] = p[2];
            }
        }
    } else {
        // chroma sample (x / 2, y / 2) of every even output pixel of the image: the map halved (exact) and quantised again, decided over the
        // chroma plane's size
        const int cw = a.sw >> 1, ch = a.sh >> 1;
        const bool cact = !(lane & 1) && x < a.dw;
        BorderTap tc[RESAMPLE_RW / 2];
        unsigned cwr = 0;
        int cmnx = INT_MAX, cmxx = INT_MIN, cmny = INT_MAX, cmxy = INT_MIN;
#pragma unroll
        for (int k = 0; k < RESAMPLE_RW / 2; k++) {
            tc[k] = keep_tap(ax[2 * k] * 0.5f, ay[2 * k] * 0.5f);
            if (cact && y0 + 2 * k < a.dh && keep_written(tc[k], cw, ch))
                cwr |= 1u << k, cmnx = min(cmnx, tc[k].X), cmxx = max(cmxx, tc[k].X), cmny = min(cmny, tc[k].Y), cmxy = max(cmxy, tc[k].Y);
        }
        const BorderBytes<1, VSTAB_BORDER_CONSTANT> sy = {a.y, a.pitch_y, a.sw, a.sh, 0u};
        const BorderBytes<2, VSTAB_BORDER_CONSTANT> suv = {a.uv, a.pitch_uv, cw, ch, 0u};
        uint8_t *lds_y = stage;                                                          // luma bytes: half the budget
        uint16_t *lds_c = reinterpret_cast<uint16_t *>(stage + RESAMPLE_LDS_BYTES / 2);  // chroma pairs: the other half
        const TileBox by = tile_box<0, 2, true>(mnx, mxx, mny, mxy, red, RESAMPLE_LDS_BYTES / 2);
        const TileBox bc = tile_box<0, 2, true>(cmnx, cmxx, cmny, cmxy, red, RESAMPLE_LDS_BYTES / 4);
        if (by.w == 0 && bc.w == 0 && ka.in_place) return;  // (uniform)
        if (by.lds) stage_box<VSTAB_BORDER_CONSTANT, true>(sy, by, lds_y);
        if (bc.lds) stage_box<VSTAB_BORDER_CONSTANT, true>(suv, bc, lds_c);
        __syncthreads();  // reached by every thread whichever plane has a box: the branches below are uniform and hold no barrier
        if (by.w == 0) {
            if (!ka.in_place)
                keep_copy_tile<RESAMPLE_TW / 16, RESAMPLE_TH>(ka.prev, ka.pitch_prev, a.dst, a.pitch_dst, blockIdx.x * RESAMPLE_TW, a.dw, blockIdx.y * RESAMPLE_TH,
                                                             a.dh, ka.vec);
        } else {
#pragma unroll
            for (int j = 0; j < RESAMPLE_RW; j++) {
                const int y = y0 + j;
                if (x >= a.dw || y >= a.dh) continue;
                if (wr & (1u << j)) {
                    uint32_t v[4];
                    keep_taps(sy, by, lds_y, t[j], v);
                    a.dst[(size_t)y * a.pitch_dst + x] = (uint8_t)border_channel<0>(v[0], v[1], v[2], v[3], t[j]);
                } else if (!ka.in_place) {
                    a.dst[(size_t)y * a.pitch_dst + x] = ka.prev[(size_t)y * ka.pitch_prev + x];
                }
            }
        }
        if (bc.w == 0) {  // chroma rows y / 2 of the tile's even rows; bytes x, x + 1 of its even columns
            if (!ka.in_place)
                keep_copy_tile<RESAMPLE_TW / 16, RESAMPLE_TH / 2>(ka.prev_uv, ka.pitch_prev_uv, a.dst_uv, a.pitch_dst_uv, blockIdx.x * RESAMPLE_TW,
                                                                 ((a.dw + 1) >> 1) * 2, blockIdx.y * (RESAMPLE_TH / 2), (a.dh + 1) >> 1, ka.vec_uv);
        } else {
#pragma unroll
            for (int k = 0; k < RESAMPLE_RW / 2; k++) {
                const int y = y0 + 2 * k;
                if (!cact || y >= a.dh) continue;
                uint8_t *o = a.dst_uv + (size_t)(y >> 1) * a.pitch_dst_uv + (size_t)x;  // chroma sample x / 2: bytes x, x + 1
                if (cwr & (1u << k)) {
                    uint32_t v[4];
                    keep_taps(suv, bc, lds_c, tc[k], v);
                    o[0] = (uint8_t)border_channel<0>(v[0], v[1], v[2], v[3], tc[k]), o[1] = (uint8_t)border_channel<1>(v[0], v[1], v[2], v[3], tc[k]);
                } else if (!ka.in_place) {
                    const uint8_t *p = ka.prev_uv + (size_t)(y >> 1) * ka.pitch_prev_uv + (size_t)x;
                    o[0] = p[0], o[1] = p[1];
                }
            }
        }
    }
}

// k_remap_keep -- the keep-edge remap of CN interleaved 8-bit channels with float map planes: the stateless building block (any map, NaN /
// huge / tie entries included; all CN channels of a sample are written or kept together).  One thread per output pixel, taps from global
// memory.  prev and dst may be one plane (in_place): neither is __restrict__.
template <int CN>
__global__ void __launch_bounds__(256) k_remap_keep(VSTAB_REMAP_PARAMS, const uint8_t *prev, size_t pitch_prev, uint8_t *dst, size_t pitch_dst, int dw, int dh,
                                                    int in_place) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= dw || y >= dh) return;
    const float mx = reinterpret_cast<const float *>(reinterpret_cast<const uint8_t *>(mapx) + (size_t)y * pitch_x)[x];
    const float my = reinterpret_cast<const float *>(reinterpret_cast<const uint8_t *>(mapy) + (size_t)y * pitch_y)[x];
    const BorderTap t = keep_tap(mx * 32.0f, my * 32.0f);
    uint8_t *o = dst + (size_t)y * pitch_dst + (size_t)x * CN;
    if (keep_written(t, sw, sh)) {
        const BorderBytes<CN, VSTAB_BORDER_CONSTANT> s = {src, pitch_src, sw, sh, 0u};
        const TileBox none = {0, 0, 0, 0, false};
        uint32_t v[4];
        keep_taps(s, none, (const uint32_t *)nullptr, t, v);
        o[0] = (uint8_t)border_channel<0>(v[0], v[1], v[2], v[3], t);
        if constexpr (CN > 1) o[1] = (uint8_t)border_channel<1>(v[0], v[1], v[2], v[3], t);
        if constexpr (CN > 2) o[2] = (uint8_t)border_channel<2>(v[0], v[1], v[2], v[3], t);
    } else if (!in_place) {
        const uint8_t *p = prev + (size_t)y * pitch_prev + (size_t)x * CN;
#pragma unroll
        for (int k = 0; k < CN; k++) o[k] = p[k];
    }
}

// Kernels of this translation unit are one code object: see preload_warp_kernels
vstab_status preload_keep_kernels() {
    hipFuncAttributes at;
    VSTAB_HIP_TRY(hipFuncGetAttributes(&at, reinterpret_cast<const void *>(&k_remap_keep<1>)));
    return VSTAB_OK;
}

static bool keep_vec_ok(const void *prev, size_t pitch_prev, const void *dst, size_t pitch_dst) {
    return ptr_aligned(prev, 16) && ptr_aligned(dst, 16) && pitch_prev % 16 == 0 && pitch_dst % 16 == 0;
}

// k_warp_keep of a route (WARP_KEEP) on its grid: ba and the request's history (checked: check_keep_prev, which found in_place)
vstab_status launch_warp_keep(const BorderArgs &ba, const WarpRoute &r, const WarpRequest &q, bool in_place) {
    const bool planar = q.planar();
    KeepArgs ka;
    ka.b = ba;
    ka.prev = (const uint8_t *)q.prev, ka.pitch_prev = q.pitch_prev;
    ka.prev_uv = planar ? (const uint8_t *)q.prev_uv : nullptr, ka.pitch_prev_uv = planar ? q.pitch_prev_uv : 0;
    ka.in_place = in_place;
    ka.vec = keep_vec_ok(q.prev, q.pitch_prev, q.dst, q.pitch_dst), ka.vec_uv = planar && keep_vec_ok(q.prev_uv, q.pitch_prev_uv, q.dst_uv, q.pitch_dst_uv);
    with_kernel_mode(route_kernel_mode(r.mode), [&](auto mode) {
        with_bool(planar, [&](auto pl) {
            with_bool(map_mode_is_rs(r.mode), [&](auto rs) {
                constexpr int MODE = decltype(mode)::value;
                constexpr bool RS = decltype(rs)::value;
                if constexpr (MODE <= MAP_CREATEMAP_CL_OPENCL && (!RS || map_mode_fish_to_pinhole(MODE)))
                    launch_tiles(k_warp_keep<MODE, decltype(pl)::value, RS>, ka, q.dw, q.dh, q.stream);
            });
        });
    });
    VSTAB_HIP_TRY(hipGetLastError());
    return VSTAB_OK;
}

}  // namespace vstab

using namespace vstab;

extern "C" {

vstab_status vstab_remap_bilinear_keep(const void *src, size_t pitch_src, int sw, int sh, int channels, const void *map_x, size_t pitch_x, const void *map_y,
                                       size_t pitch_y, const void *prev, size_t pitch_prev, void *dst, size_t pitch_dst, int dw, int dh, void *stream) {
    static const char n[] = "vstab_remap_bilinear_keep";
    uint32_t none;
    const int constant = VSTAB_BORDER_CONSTANT;  // (no border mode and no border values to check)
    VSTAB_TRY(check_remap(n, src, pitch_src, sw, sh, channels, map_x, pitch_x, map_y, pitch_y, &constant, false, nullptr, dst, pitch_dst, dw, dh, none));
    const KeepPlane plane = {prev, pitch_prev, dst, pitch_dst, (size_t)dw * channels, dh};
    bool in_place;
    VSTAB_TRY(check_keep_prev(n, &plane, 1, in_place));
    const dim3 grid(div_up(dw, 64), div_up(dh, 4));
    with_channels(channels, [&](auto cn) {
        hipLaunchKernelGGL((k_remap_keep<decltype(cn)::value>), grid, dim3(256), 0, static_cast<hipStream_t>(stream), (const uint8_t *)src, pitch_src, sw, sh,
                           (const float *)map_x, pitch_x, (const float *)map_y, pitch_y, (const uint8_t *)prev, pitch_prev, (uint8_t *)dst, pitch_dst, dw, dh,
                           (int)in_place);
    });
    VSTAB_HIP_TRY(hipGetLastError());
    return VSTAB_OK;
}

vstab_status vstab_warp_nv12_keep(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int sw, int sh, const float params[17], const float *rot_bottom,
                                  int map_mode, int out_format, const void *prev, size_t pitch_prev, const void *prev_uv, size_t pitch_prev_uv, void *dst,
                                  size_t pitch_dst, void *dst_uv, size_t pitch_dst_uv, int dw, int dh, void *stream) {
    return warp_nv12({.e = ENTRY_KEEP, .y = y, .pitch_y = pitch_y, .uv = uv, .pitch_uv = pitch_uv, .sw = sw, .sh = sh, .params = params, .rot_bottom = rot_bottom,
                      .keep = true, .prev = prev, .pitch_prev = pitch_prev, .prev_uv = prev_uv, .pitch_prev_uv = pitch_prev_uv, .map_mode = map_mode,
                      .out_format = out_format, .dst = dst, .pitch_dst = pitch_dst, .dst_uv = dst_uv, .pitch_dst_uv = pitch_dst_uv, .dw = dw, .dh = dh,
                      .stream = stream});
}

}  // extern "C"
