// vstab_plane_ops.hip -- operators on whole planes for gfx950 (MI355X): NV12 / P010 packing, NV12 -> BGR and, with a colour spec, both ways, the map planes (createMap and the
// generalised map), the quantised map, remap from map planes and the debug markers, with their C entry points.  Compiled with
// -ffp-contract=off.
//
// All of this is HBM-bound byte/gather work (no MFMA): the design rules that matter are coalesced wide accesses, enough workgroups to
// fill 256 CUs, and keeping the map in registers.
#include <climits>

#include "vstab_colour.hpp"
#include "vstab_warp_host.hpp"

namespace vstab {

// =============================================================================================
// k_pack_nv12 -- replaces the two clEnqueueCopyImageToBuffer calls of
// FrameSourceFfmpegOpenCl.cpp:64-85.  One launch copies both planes: rows [0,h) come from the
// luma plane, rows [h, h*3/2) from the chroma plane.  16 B per lane when every pitch and base
// is 16-B aligned, bytes otherwise.
// =============================================================================================
template <typename V>
__global__ void __launch_bounds__(256) k_pack_nv12(const uint8_t *__restrict__ y, size_t pitch_y,
                                                   const uint8_t *__restrict__ uv, size_t pitch_uv,
                                                   int row_vecs, int h, uint8_t *__restrict__ dst,
                                                   size_t pitch_dst) {
    // flat grid-stride loop over (row, vector) pairs: a small persistent grid keeps the copy from
    // taking wave slots away from kernels running beside it on other streams
    const int rows = h + h / 2;
    const long total = (long)rows * row_vecs;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const int row = (int)(e / row_vecs), i = (int)(e - (long)row * row_vecs);
        const uint8_t *s = row < h ? y + (size_t)row * pitch_y : uv + (size_t)(row - h) * pitch_uv;
        uint8_t *d = dst + (size_t)row * pitch_dst;
        reinterpret_cast<V *>(d)[i] = reinterpret_cast<const V *>(s)[i];
    }
}

// =============================================================================================
// k_pack_p010 -- 10-bit input (BASELINE config 5: P010 / P016 planes, 16-bit little-endian samples with the
// significant bits at the top) narrowed to the 8-bit packed NV12 the reference path works on: byte = sample >> 8.
// No reference counterpart (the reference only ever sees 8-bit NV12, FrameSourceFfmpegOpenCl.cpp:53-56).
// One thread narrows 8 samples (one 16-B load, one 8-B store) when everything is aligned, else one sample.
// =============================================================================================
template <bool VEC>
__global__ void __launch_bounds__(256) k_pack_p010(const uint8_t *__restrict__ y, size_t pitch_y,
                                                   const uint8_t *__restrict__ uv, size_t pitch_uv, int row_units,
                                                   int h, int rows, uint8_t *__restrict__ dst, size_t pitch_dst) {
    const long total = (long)rows * row_units;  // rows = h + h / 2, or h when only the luma plane is wanted
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const int row = (int)(e / row_units), i = (int)(e - (long)row * row_units);
        const uint8_t *s = row < h ? y + (size_t)row * pitch_y : uv + (size_t)(row - h) * pitch_uv;
        uint8_t *d = dst + (size_t)row * pitch_dst;
        if constexpr (VEC) {
            const uint4 v = reinterpret_cast<const uint4 *>(s)[i];
            const uint32_t lo = __builtin_amdgcn_perm(v.y, v.x, 0x07050301u), hi = __builtin_amdgcn_perm(v.w, v.z, 0x07050301u);
            reinterpret_cast<uint2 *>(d)[i] = make_uint2(lo, hi);
        } else {
            d[i] = s[2 * i + 1];  // high byte of the little-endian sample
        }
    }
}

// =============================================================================================
// k_cvt_nv12_bgr -- cvtColor(COLOR_YUV2BGR_NV12), FrameSourceWarp.cpp:401.  Compatibility /
// parity kernel (the fused path never materialises the BGR frame).  One thread converts an
// 8 x 2 luma block: two 8-B luma loads, one 8-B chroma load, two 24-B BGR stores.
// =============================================================================================
__global__ void __launch_bounds__(256) k_cvt_nv12_bgr(const uint8_t *__restrict__ yp, size_t pitch_y,
                                                      const uint8_t *__restrict__ uvp, size_t pitch_uv,
                                                      int w, int h, uint8_t *__restrict__ dst,
                                                      size_t pitch_dst, int vec_ok) {
    const int bx = (blockIdx.x * blockDim.x + threadIdx.x) * 8;
    const int by = (blockIdx.y * blockDim.y + threadIdx.y) * 2;
    if (bx >= w || by >= h) return;
    const uint8_t *y0 = yp + (size_t)by * pitch_y + bx;
    const uint8_t *y1 = y0 + pitch_y;
    const uint8_t *uv = uvp + (size_t)(by >> 1) * pitch_uv + bx;
    uint8_t *d0 = dst + (size_t)by * pitch_dst + (size_t)bx * 3;
    uint8_t *d1 = d0 + pitch_dst;
    if (vec_ok && bx + 8 <= w) {
        const uint2 a = *reinterpret_cast<const uint2 *>(y0);
        const uint2 b = *reinterpret_cast<const uint2 *>(y1);
        const uint2 c = *reinterpret_cast<const uint2 *>(uv);
        const uint32_t ya[2] = {a.x, a.y}, yb[2] = {b.x, b.y}, cc[2] = {c.x, c.y};
        uint32_t o0[6], o1[6];
        uint8_t t0[24], t1[24];
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const int pair = i >> 1;
            const uint32_t cw = cc[pair >> 1] >> ((pair & 1) * 16);
            const ChromaTerm ct = chroma_term(cw & 255, (cw >> 8) & 255);
            int bb, gg, rr;
            yuv_to_bgr((ya[i >> 2] >> ((i & 3) * 8)) & 255, ct, bb, gg, rr);
            t0[3 * i] = bb, t0[3 * i + 1] = gg, t0[3 * i + 2] = rr;
            yuv_to_bgr((yb[i >> 2] >> ((i & 3) * 8)) & 255, ct, bb, gg, rr);
            t1[3 * i] = bb, t1[3 * i + 1] = gg, t1[3 * i + 2] = rr;
        }
#pragma unroll
        for (int i = 0; i < 6; i++) {
            o0[i] = t0[4 * i] | (t0[4 * i + 1] << 8) | (t0[4 * i + 2] << 16) | ((uint32_t)t0[4 * i + 3] << 24);
            o1[i] = t1[4 * i] | (t1[4 * i + 1] << 8) | (t1[4 * i + 2] << 16) | ((uint32_t)t1[4 * i + 3] << 24);
        }
#pragma unroll
        for (int i = 0; i < 3; i++) {
            reinterpret_cast<uint2 *>(d0)[i] = make_uint2(o0[2 * i], o0[2 * i + 1]);
            reinterpret_cast<uint2 *>(d1)[i] = make_uint2(o1[2 * i], o1[2 * i + 1]);
        }
    } else {
        for (int i = 0; i < 8 && bx + i < w; i++) {
            const ChromaTerm ct = chroma_term(uv[i & ~1], uv[(i & ~1) + 1]);
            int bb, gg, rr;
            yuv_to_bgr(y0[i], ct, bb, gg, rr);
            d0[3 * i] = bb, d0[3 * i + 1] = gg, d0[3 * i + 2] = rr;
            if (by + 1 < h) {
                yuv_to_bgr(y1[i], ct, bb, gg, rr);
                d1[3 * i] = bb, d1[3 * i + 1] = gg, d1[3 * i + 2] = rr;
            }
        }
    }
}

// =============================================================================================
// k_cvt_nv12_bgr_colour -- k_cvt_nv12_bgr with a colour spec's coefficients (include/vstab.h, "Colour matrix and range"): the same
// 8 x 2 block per thread, chroma_term / yuv_to_bgr (vstab_device.hpp) with the block k as their coefficient source.  A kernel of its own
// and not a second caller of one __device__ body: through such a body k_cvt_nv12_bgr's listing grows by three lines and this one's
// changes its order ("The coefficient source").
// =============================================================================================
__global__ void __launch_bounds__(256) k_cvt_nv12_bgr_colour(const uint8_t *__restrict__ yp, size_t pitch_y, const uint8_t *__restrict__ uvp, size_t pitch_uv,
                                                             int w, int h, uint8_t *__restrict__ dst, size_t pitch_dst, int vec_ok, ColourCoef k) {
    const int bx = (blockIdx.x * blockDim.x + threadIdx.x) * 8;
    const int by = (blockIdx.y * blockDim.y + threadIdx.y) * 2;
    if (bx >= w || by >= h) return;
    const uint8_t *y0 = yp + (size_t)by * pitch_y + bx;
    const uint8_t *y1 = y0 + pitch_y;
    const uint8_t *uv = uvp + (size_t)(by >> 1) * pitch_uv + bx;
    uint8_t *d0 = dst + (size_t)by * pitch_dst + (size_t)bx * 3;
    uint8_t *d1 = d0 + pitch_dst;
    if (vec_ok && bx + 8 <= w) {
        const uint2 a = *reinterpret_cast<const uint2 *>(y0);
        const uint2 b = *reinterpret_cast<const uint2 *>(y1);
        const uint2 c = *reinterpret_cast<const uint2 *>(uv);
        const uint32_t ya[2] = {a.x, a.y}, yb[2] = {b.x, b.y}, cc[2] = {c.x, c.y};
        uint32_t o0[6], o1[6];
        uint8_t t0[24], t1[24];
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const int pair = i >> 1;
            const uint32_t cw = cc[pair >> 1] >> ((pair & 1) * 16);
            const ChromaTerm ct = chroma_term(k, cw & 255, (cw >> 8) & 255);
            int bb, gg, rr;
            yuv_to_bgr(k, (ya[i >> 2] >> ((i & 3) * 8)) & 255, ct, bb, gg, rr);
            t0[3 * i] = bb, t0[3 * i + 1] = gg, t0[3 * i + 2] = rr;
            yuv_to_bgr(k, (yb[i >> 2] >> ((i & 3) * 8)) & 255, ct, bb, gg, rr);
            t1[3 * i] = bb, t1[3 * i + 1] = gg, t1[3 * i + 2] = rr;
        }
#pragma unroll
        for (int i = 0; i < 6; i++) {
            o0[i] = t0[4 * i] | (t0[4 * i + 1] << 8) | (t0[4 * i + 2] << 16) | ((uint32_t)t0[4 * i + 3] << 24);
            o1[i] = t1[4 * i] | (t1[4 * i + 1] << 8) | (t1[4 * i + 2] << 16) | ((uint32_t)t1[4 * i + 3] << 24);
        }
#pragma unroll
        for (int i = 0; i < 3; i++) {
            reinterpret_cast<uint2 *>(d0)[i] = make_uint2(o0[2 * i], o0[2 * i + 1]);
            reinterpret_cast<uint2 *>(d1)[i] = make_uint2(o1[2 * i], o1[2 * i + 1]);
        }
    } else {
        for (int i = 0; i < 8 && bx + i < w; i++) {
            const ChromaTerm ct = chroma_term(k, uv[i & ~1], uv[(i & ~1) + 1]);
            int bb, gg, rr;
            yuv_to_bgr(k, y0[i], ct, bb, gg, rr);
            d0[3 * i] = bb, d0[3 * i + 1] = gg, d0[3 * i + 2] = rr;
            if (by + 1 < h) {
                yuv_to_bgr(k, y1[i], ct, bb, gg, rr);
                d1[3 * i] = bb, d1[3 * i + 1] = gg, d1[3 * i + 2] = rr;
            }
        }
    }
}

// =============================================================================================
// k_cvt_bgr_nv12_colour -- the inverse (cvtColor(COLOR_BGR2YUV_I420)'s form with a spec's coefficients, NV12 planes out): luma for every
// pixel, chroma from the top-left pixel of each 2 x 2 block, through bgr_to_y / bgr_to_uv -- the functions the fused kernel's NV12 store
// calls.  One thread per 2 x 2 block (w and h are even): a parity operator, byte accesses.
// =============================================================================================
__global__ void __launch_bounds__(256) k_cvt_bgr_nv12_colour(const uint8_t *__restrict__ src, size_t pitch, int w, int h, uint8_t *__restrict__ dy,
                                                             size_t pitch_y, uint8_t *__restrict__ duv, size_t pitch_uv, ColourCoef k) {
    const int x = (blockIdx.x * 64 + (threadIdx.x & 63)) * 2, y = (blockIdx.y * 4 + (threadIdx.x >> 6)) * 2;
    if (x >= w || y >= h) return;
    uint32_t px[2][2];
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const uint8_t *s = src + (size_t)(y + j) * pitch + (size_t)(x + i) * 3;
            px[j][i] = (uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16);
        }
#pragma unroll
    for (int j = 0; j < 2; j++) {
        uint8_t *o = dy + (size_t)(y + j) * pitch_y + x;
        o[0] = (uint8_t)bgr_to_y(k, px[j][0]), o[1] = (uint8_t)bgr_to_y(k, px[j][1]);
    }
    const uint32_t c = bgr_to_uv(k, px[0][0]);
    *reinterpret_cast<uint16_t *>(duv + (size_t)(y >> 1) * pitch_uv + x) = (uint16_t)c;
}

// Four adjacent entries of both map planes, columns x0 .. x0 + 3 of row y: one 16-B store per plane when the planes are aligned
// (vec_ok) and the group is whole, the columns inside the map one by one otherwise.
__device__ __forceinline__ void store_map4(float *mapx, size_t pitch_x, float *mapy, size_t pitch_y, int x0, int y, int cols, int vec_ok,
                                           const float (&mx)[4], const float (&my)[4]) {
    float *px = reinterpret_cast<float *>(reinterpret_cast<uint8_t *>(mapx) + (size_t)y * pitch_x) + x0;
    float *py = reinterpret_cast<float *>(reinterpret_cast<uint8_t *>(mapy) + (size_t)y * pitch_y) + x0;
    if (vec_ok && x0 + 4 <= cols) {
        *reinterpret_cast<float4 *>(px) = make_float4(mx[0], mx[1], mx[2], mx[3]);
        *reinterpret_cast<float4 *>(py) = make_float4(my[0], my[1], my[2], my[3]);
    } else {
        for (int i = 0; i < 4 && x0 + i < cols; i++) px[i] = mx[i], py[i] = my[i];
    }
}

// =============================================================================================
// k_create_map -- createMap.cl:1-51 as a stand-alone kernel (parity / un-fused mode only).
// 16x16 threads, 4 columns per thread (one 16-B store per plane when aligned).
// =============================================================================================
__global__ void __launch_bounds__(256) k_create_map(float *__restrict__ mapx, size_t pitch_x,
                                                    float *__restrict__ mapy, size_t pitch_y,
                                                    int cols, int rows, MapParams p, int vec_ok) {
    const int x0 = (blockIdx.x * 16 + threadIdx.x) * 4;
    const int y = blockIdx.y * 16 + threadIdx.y;
    if (x0 >= cols || y >= rows) return;
    const RowTerm rt = row_term(p, y);
    float mx[4], my[4];
#pragma unroll
    for (int i = 0; i < 4; i++) map_pixel(p, col_term(p, x0 + i), rt, mx[i], my[i]);
    store_map4(mapx, pitch_x, mapy, pitch_y, x0, y, cols, vec_ok, mx, my);
}

// k_create_map_ex -- the generalised map (modes 1..4, vstab_map.hpp map_pixel_ex) as map planes.  Lens: the input lens's coefficients --
// Distortion (k1..k4 of a fisheye lens, MAP_FISHD_*; zero for the ideal modes) or PinholeLens (the five of a rectilinear lens, MAP_RECTD_*).
struct PinholeLens {
    float k[5];  // k1, k2, p1, p2, k3
};
__device__ __forceinline__ Distortion lens_fisheye(const Distortion &d) { return d; }
__device__ __forceinline__ Distortion lens_fisheye(const PinholeLens &) { return Distortion{0.0f, 0.0f, 0.0f, 0.0f}; }
__device__ __forceinline__ const float *lens_pinhole(const Distortion &) { return nullptr; }
__device__ __forceinline__ const float *lens_pinhole(const PinholeLens &d) { return d.k; }
template <int MODE, typename Lens = Distortion>
__global__ void __launch_bounds__(256) k_create_map_ex(float *__restrict__ mapx, size_t pitch_x,
                                                       float *__restrict__ mapy, size_t pitch_y,
                                                       int cols, int rows, MapParams p, int vec_ok, Lens d) {
    const int x0 = (blockIdx.x * 16 + threadIdx.x) * 4;
    const int y = blockIdx.y * 16 + threadIdx.y;
    if (x0 >= cols || y >= rows) return;
    const MapParams32 in = {p.icx, p.icy, p.ifx, p.ify, p.r[2], p.r[5], p.r[8], lens_fisheye(d)};  // unscaled here
    constexpr bool OCL = MODE == MAP_CREATEMAP_CL_OPENCL;
    const float vy = OCL ? ocl_div((float)y - p.ocy, p.ofy) : ((float)y - p.ocy) / p.ofy;
    float mx[4], my[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const float vx = OCL ? ocl_div((float)(x0 + i) - p.ocx, p.ofx) : ((float)(x0 + i) - p.ocx) / p.ofx;
        // the map-plane operator runs the OpenCL build's instruction stream literally; the fused kernel and the
        // quantised map use its shortened form with this one as the fall-back (vstab_map.hpp)
        if constexpr (OCL) map_pixel_ocl_literal(p.icx, p.icy, p.ifx, p.ify, p.r, p.r[0] * vx, p.r[3] * vx, p.r[6] * vx, vy, mx[i], my[i]);
        else map_at<MODE>(in, p, vx, vy, mx[i], my[i], lens_pinhole(d));
    }
    store_map4(mapx, pitch_x, mapy, pitch_y, x0, y, cols, vec_ok, mx, my);
}

// =============================================================================================
// k_remap_bilinear -- cv::remap(INTER_LINEAR, BORDER_CONSTANT 0), FrameSourceWarp.cpp:306-312,
// reading float map planes (un-fused compatibility mode).  One thread per output pixel.
// =============================================================================================
template <int CN>
__global__ void __launch_bounds__(256) k_remap_bilinear(const uint8_t *__restrict__ src, size_t pitch_src,
                                                        int sw, int sh, const float *__restrict__ mapx,
                                                        size_t pitch_x, const float *__restrict__ mapy,
                                                        size_t pitch_y, uint8_t *__restrict__ dst,
                                                        size_t pitch_dst, int dw, int dh) {
    const int x = blockIdx.x * 64 + threadIdx.x;
    const int y = blockIdx.y * 4 + threadIdx.y;
    if (x >= dw || y >= dh) return;
    const float mx = reinterpret_cast<const float *>(reinterpret_cast<const uint8_t *>(mapx) + (size_t)y * pitch_x)[x];
    const float my = reinterpret_cast<const float *>(reinterpret_cast<const uint8_t *>(mapy) + (size_t)y * pitch_y)[x];
    const Tap t = quantise(mx, my);
    uint8_t *o = dst + (size_t)y * pitch_dst + (size_t)x * CN;
    if (t.far || t.X >= sw || t.X + 1 < 0 || t.Y >= sh || t.Y + 1 < 0) {
#pragma unroll
        for (int c = 0; c < CN; c++) o[c] = 0;
        return;
    }
    const int w00 = (32 - t.fx) * (32 - t.fy), w01 = t.fx * (32 - t.fy), w10 = (32 - t.fx) * t.fy,
              w11 = t.fx * t.fy;
    const bool x0 = t.X >= 0, x1 = t.X + 1 < sw, y0 = t.Y >= 0, y1 = t.Y + 1 < sh;
    const uint8_t *r0 = src + (size_t)max(t.Y, 0) * pitch_src, *r1 = src + (size_t)min(t.Y + 1, sh - 1) * pitch_src;
    const size_t c0 = (size_t)max(t.X, 0) * CN, c1 = (size_t)min(t.X + 1, sw - 1) * CN;
#pragma unroll
    for (int c = 0; c < CN; c++) {
        const int p00 = (x0 && y0) ? r0[c0 + c] : 0, p01 = (x1 && y0) ? r0[c1 + c] : 0;
        const int p10 = (x0 && y1) ? r1[c0 + c] : 0, p11 = (x1 && y1) ? r1[c1 + c] : 0;
        o[c] = (uint8_t)((p00 * w00 + p01 * w01 + p10 * w10 + p11 * w11 + 512) >> 10);
    }
}

// k_quantised_map -- the map of every output pixel as cv::remap quantises it (32 * map rounded half to even; a NaN
// entry gets x = INT_MIN), written once for a run of frames that share their warp parameters (see CACHED above).
// The map arithmetic of k_warp_fused; its cvRound is the plain formulation (rint, NaN -> INT_MIN).
template <int MODE>
__global__ void __launch_bounds__(256) k_quantised_map(int2 *__restrict__ qmap, int qpitch, int dw, int dh, MapParams p, MapParams32 p32) {
    const int x0 = (blockIdx.x * 16 + (threadIdx.x & 15)) * 4, y = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (x0 >= qpitch || y >= dh) return;
    const float rfx = rcp_refined(p.ofx), rfy = rcp_refined(p.ofy);
    const float vy = norm_coord<MODE>((float)y - p.ocy, p.ofy, rfy);
    int q[8];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        float ax, ay;
        map_at<MODE>(p32, p, norm_coord<MODE>((float)(x0 + i) - p.ocx, p.ofx, rfx), vy, ax, ay);
        const bool ok = !__builtin_isunordered(ax, ay);
        q[2 * i] = ok ? (int)__builtin_rintf(ax) : INT_MIN, q[2 * i + 1] = (int)__builtin_rintf(ay);
    }
    uint4 *o = reinterpret_cast<uint4 *>(qmap + (size_t)y * qpitch + x0);
    o[0] = make_uint4((uint32_t)q[0], (uint32_t)q[1], (uint32_t)q[2], (uint32_t)q[3]);
    o[1] = make_uint4((uint32_t)q[4], (uint32_t)q[5], (uint32_t)q[6], (uint32_t)q[7]);
}

// k_draw_markers -- the debug overlay of the lens surface (libdewobble's `debug` option, render.ts:678): a filled
// (2 * half + 1)^2 square at every tracked feature, clipped to the image.  One workgroup per feature.
__global__ void __launch_bounds__(64) k_draw_markers(uint8_t *__restrict__ dst, size_t pitch, int w, int h, int channels,
                                                     const int2 *__restrict__ centres, int half, uint32_t bgr) {
    const int2 c = centres[blockIdx.x];
    const int side = 2 * half + 1;
    for (int e = threadIdx.x; e < side * side; e += 64) {
        const int x = c.x - half + e % side, y = c.y - half + e / side;
        if (x < 0 || y < 0 || x >= w || y >= h) continue;
        uint8_t *o = dst + (size_t)y * pitch + (size_t)x * channels;
        o[0] = bgr & 255;
        if (channels == 3) o[1] = (bgr >> 8) & 255, o[2] = (bgr >> 16) & 255;
    }
}

namespace {

// f(a value of the copy kernel's vector type) for a vector of 16, 8, 4 bytes, or 1
template <typename F>
void with_copy_vector(int bytes, F &&f) {
    if (bytes == 16) f(uint4{});
    else if (bytes == 8) f(uint2{});
    else if (bytes == 4) f(uint32_t{});
    else f(uint8_t{});
}

// the map mode of an entry point that takes the input lens's coefficients (with_dist: modes 1 and 2), or of one that takes none
vstab_status check_map_mode(const std::string &n, int map_mode, bool with_dist) {
    if (with_dist && !map_mode_takes_distortion(map_mode)) return fail(VSTAB_ERR_INVALID, n + ": distortion belongs to a fisheye input (map modes 1 and 2)");
    if (!with_dist && (map_mode < VSTAB_MAP_CREATEMAP_CL || map_mode > VSTAB_MAP_CREATEMAP_CL_OPENCL)) return fail(VSTAB_ERR_INVALID, n + ": unknown map mode");
    return VSTAB_OK;
}

// the map planes' arguments, checked; with_dist: vstab_create_map_dist (map modes 1 and 2 with the input lens's polynomial)
vstab_status create_map_impl(const std::string &n, void *map_x, size_t pitch_x, void *map_y, size_t pitch_y, int cols, int rows, const float params[17],
                             const float *dist, bool with_dist, int map_mode, void *stream) {
    if (!map_x || !map_y || !params || (with_dist && !dist)) return fail(VSTAB_ERR_INVALID, n + ": null pointer");
    if (cols <= 0 || rows <= 0 || cols > 32767 || rows > 32767)
        return fail(VSTAB_ERR_INVALID, n + ": size must be in [1, 32767] (createMap.cl:10-11)");
    if (pitch_x < (size_t)cols * 4 || pitch_y < (size_t)cols * 4 || pitch_x % 4 || pitch_y % 4)
        return fail(VSTAB_ERR_INVALID, n + ": bad pitch");
    VSTAB_TRY(check_map_mode(n, map_mode, with_dist));
    if (with_dist) VSTAB_TRY(check_distortion(n.c_str(), dist));
    const int vec_ok = ptr_aligned(map_x, 16) && ptr_aligned(map_y, 16) && pitch_x % 16 == 0 && pitch_y % 16 == 0;
    dim3 grid(div_up(div_up(cols, 4), 16), div_up(rows, 16));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const Distortion d = with_dist ? Distortion{dist[0], dist[1], dist[2], dist[3]} : Distortion();
    with_kernel_mode(kernel_mode_tag(map_mode, with_dist ? LENS_FISHEYE : LENS_IDEAL, false), [&](auto mode) {
        constexpr int MODE = decltype(mode)::value;
        if constexpr (MODE == MAP_CREATEMAP_CL)  // createMap.cl itself
            hipLaunchKernelGGL(k_create_map, grid, dim3(16, 16), 0, s, (float *)map_x, pitch_x, (float *)map_y, pitch_y, cols, rows, map_params(params), vec_ok);
        else if constexpr (mode_plain_or_dist(MODE))
            hipLaunchKernelGGL(k_create_map_ex<MODE>, grid, dim3(16, 16), 0, s, (float *)map_x, pitch_x, (float *)map_y, pitch_y, cols, rows,
                               map_params(params), vec_ok, d);
    });
    VSTAB_HIP_TRY(hipGetLastError());
    return VSTAB_OK;
}

// vstab_create_map_pinhole: the map planes of modes 3 / 4 through a rectilinear lens's (k1, k2, p1, p2, k3)
vstab_status create_map_pinhole_impl(const std::string &n, void *map_x, size_t pitch_x, void *map_y, size_t pitch_y, int cols, int rows,
                                     const float params[17], const float dist[5], int map_mode, void *stream) {
    if (!map_x || !map_y || !params || !dist) return fail(VSTAB_ERR_INVALID, n + ": null pointer");
    if (cols <= 0 || rows <= 0 || cols > 32767 || rows > 32767) return fail(VSTAB_ERR_INVALID, n + ": size must be in [1, 32767] (createMap.cl:10-11)");
    if (pitch_x < (size_t)cols * 4 || pitch_y < (size_t)cols * 4 || pitch_x % 4 || pitch_y % 4) return fail(VSTAB_ERR_INVALID, n + ": bad pitch");
    if (!map_mode_takes_pinhole(map_mode)) return fail(VSTAB_ERR_INVALID, n + ": pinhole distortion belongs to a rectilinear input (map modes 3 and 4)");
    VSTAB_TRY(check_pinhole_distortion(n.c_str(), dist));
    const int vec_ok = ptr_aligned(map_x, 16) && ptr_aligned(map_y, 16) && pitch_x % 16 == 0 && pitch_y % 16 == 0;
    dim3 grid(div_up(div_up(cols, 4), 16), div_up(rows, 16));
    const PinholeLens d = {{dist[0], dist[1], dist[2], dist[3], dist[4]}};
    with_kernel_mode(kernel_mode_tag(map_mode, LENS_PINHOLE, false), [&](auto mode) {
        if constexpr (ModeTraits<decltype(mode)::value>::rectd)
            hipLaunchKernelGGL((k_create_map_ex<decltype(mode)::value, PinholeLens>), grid, dim3(16, 16), 0, static_cast<hipStream_t>(stream), (float *)map_x, pitch_x,
                               (float *)map_y, pitch_y, cols, rows, map_params(params), vec_ok, d);
    });
    VSTAB_HIP_TRY(hipGetLastError());
    return VSTAB_OK;
}

// the quantised map's arguments, checked; with_dist: vstab_quantised_map_dist, which checks the coefficients last
vstab_status quantised_map_impl(const std::string &n, void *qmap, int dw, int dh, const float params[17], const float *dist, bool with_dist, int map_mode,
                                void *stream) {
    if (!qmap || !params || (with_dist && !dist) || dw <= 0 || dh <= 0 || dw > 32767 || dh > 32767) return fail(VSTAB_ERR_INVALID, n + ": bad argument");
    VSTAB_TRY(check_map_mode(n, map_mode, with_dist));
    if (!ptr_aligned(qmap, 16)) return fail(VSTAB_ERR_INVALID, n + ": the buffer must be 16-byte aligned");
    if (with_dist) VSTAB_TRY(check_distortion(n.c_str(), dist));
    const int qpitch = (dw + 3) & ~3;
    dim3 grid(div_up(qpitch / 4, 16), div_up(dh, 16));
    hipStream_t st = static_cast<hipStream_t>(stream);
    with_kernel_mode(kernel_mode_tag(map_mode, with_dist ? LENS_FISHEYE : LENS_IDEAL, false), [&](auto mode) {
        if constexpr (mode_plain_or_dist(decltype(mode)::value))
            hipLaunchKernelGGL(k_quantised_map<decltype(mode)::value>, grid, dim3(256), 0, st, static_cast<int2 *>(qmap), qpitch, dw, dh, map_params(params),
                               map_params32(params, dist));
    });
    VSTAB_HIP_TRY(hipGetLastError());
    return VSTAB_OK;
}

}  // namespace

// luma_only: the 10-bit pipeline narrows the luma plane for the tracker and warps from the 16-bit planes
vstab_status pack_p010_planes(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int width, int height, void *dst, bool luma_only,
                              void *stream) {
    if (!y || !uv || !dst) return fail(VSTAB_ERR_INVALID, "vstab_pack_p010: null pointer");
    if (width <= 0 || height <= 0 || (width & 1) || (height & 1)) return fail(VSTAB_ERR_INVALID, "Mismatched image dimensions");
    if (pitch_y < (size_t)width * 2 || pitch_uv < (size_t)width * 2) return fail(VSTAB_ERR_INVALID, "vstab_pack_p010: pitch smaller than row");
    const int rows = luma_only ? height : height + height / 2;
    const bool vec = ptr_aligned(y, 16) && ptr_aligned(uv, 16) && ptr_aligned(dst, 8) && pitch_y % 16 == 0 && pitch_uv % 16 == 0 && width % 8 == 0;
    const int units = vec ? width / 8 : width;  // per row: groups of 8 samples, or samples
    dim3 grid(std::min<unsigned>(div_up((unsigned)((long)units * rows), 256), 2048));
    with_bool(vec, [&](auto v) {
        hipLaunchKernelGGL(k_pack_p010<decltype(v)::value>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), (const uint8_t *)y, pitch_y,
                           (const uint8_t *)uv, pitch_uv, units, height, rows, (uint8_t *)dst, (size_t)width);
    });
    VSTAB_HIP_TRY(hipGetLastError());
    return VSTAB_OK;
}

// vstab_pack_nv12 with an optional event that completes with the copy kernel -- bound to the launch itself (hipExtLaunchKernelGGL's
// stop event), no marker packet on the stream: the pipeline waits for THAT before it lets upstream recycle a surface, not for the
// pyramid kernels enqueued behind the copy
vstab_status pack_nv12_planes(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int width, int height, void *dst, void *stream, hipEvent_t done) {
    if (!y || !uv || !dst) return fail(VSTAB_ERR_INVALID, "vstab_pack_nv12: null pointer");
    if (width <= 0 || height <= 0 || (width & 1) || (height & 1))
        return fail(VSTAB_ERR_INVALID, "Mismatched image dimensions");  // FrameSourceFfmpegOpenCl.cpp:53-56
    if (pitch_y < (size_t)width || pitch_uv < (size_t)width)
        return fail(VSTAB_ERR_INVALID, "vstab_pack_nv12: pitch smaller than row");
    // the widest vector that every base, every pitch (the destination's is the width) and the row length are a multiple of
    const uintptr_t all = reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(uv) | reinterpret_cast<uintptr_t>(dst) | pitch_y | pitch_uv |
                          (uintptr_t)width;
    const int bytes = all % 16 == 0 ? 16 : all % 8 == 0 ? 8 : all % 4 == 0 ? 4 : 1;
    const int vecs = width / bytes, rows = height + height / 2;
    dim3 grid(std::min<unsigned>(div_up((unsigned)((long)vecs * rows), 256), 1024));
    with_copy_vector(bytes, [&](auto v) {
        hipExtLaunchKernelGGL(k_pack_nv12<decltype(v)>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), nullptr, done, 0, (const uint8_t *)y,
                              pitch_y, (const uint8_t *)uv, pitch_uv, vecs, height, (uint8_t *)dst, (size_t)width);
    });
    VSTAB_HIP_TRY(hipGetLastError());
    return VSTAB_OK;
}

// Kernels of this translation unit are one code object: see preload_warp_kernels
vstab_status preload_plane_kernels() {
    hipFuncAttributes at;
    VSTAB_HIP_TRY(hipFuncGetAttributes(&at, reinterpret_cast<const void *>(&k_pack_nv12<uint32_t>)));
    return VSTAB_OK;
}

}  // namespace vstab

using namespace vstab;

extern "C" {

vstab_status vstab_pack_nv12(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int width,
                             int height, void *dst, void *stream) {
    return pack_nv12_planes(y, pitch_y, uv, pitch_uv, width, height, dst, stream, nullptr);
}

vstab_status vstab_pack_p010(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int width, int height,
                             void *dst, void *stream) {
    return pack_p010_planes(y, pitch_y, uv, pitch_uv, width, height, dst, false, stream);
}

vstab_status vstab_cvt_nv12_bgr(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int width,
                                int height, void *dst, size_t pitch_dst, void *stream) {
    if (!y || !uv || !dst) return fail(VSTAB_ERR_INVALID, "vstab_cvt_nv12_bgr: null pointer");
    if (width <= 0 || height <= 0 || (width & 1) || (height & 1))
        return fail(VSTAB_ERR_INVALID, "vstab_cvt_nv12_bgr: width and height must be even");  // OpenCV asserts
    if (pitch_y < (size_t)width || pitch_uv < (size_t)width || pitch_dst < (size_t)width * 3)
        return fail(VSTAB_ERR_INVALID, "vstab_cvt_nv12_bgr: pitch smaller than row");
    const int vec_ok = ptr_aligned(y, 8) && ptr_aligned(uv, 8) && ptr_aligned(dst, 8) && pitch_y % 8 == 0 &&
                       pitch_uv % 8 == 0 && pitch_dst % 8 == 0;
    dim3 block(32, 8);
    dim3 grid(div_up(div_up(width, 8), 32), div_up(div_up(height, 2), 8));
    hipLaunchKernelGGL(k_cvt_nv12_bgr, grid, block, 0, static_cast<hipStream_t>(stream), (const uint8_t *)y,
                       pitch_y, (const uint8_t *)uv, pitch_uv, width, height, (uint8_t *)dst, pitch_dst, vec_ok);
    VSTAB_HIP_TRY(hipGetLastError());
    return VSTAB_OK;
}

vstab_status vstab_cvt_nv12_bgr_colour(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int width, int height, void *dst, size_t pitch_dst,
                                       int matrix, int range, void *stream) {
    VSTAB_TRY(check_colour_spec("vstab_cvt_nv12_bgr_colour", matrix, range));
    if (colour_spec_default(matrix, range)) return vstab_cvt_nv12_bgr(y, pitch_y, uv, pitch_uv, width, height, dst, pitch_dst, stream);
    if (!y || !uv || !dst) return fail(VSTAB_ERR_INVALID, "vstab_cvt_nv12_bgr_colour: null pointer");
    if (width <= 0 || height <= 0 || (width & 1) || (height & 1)) return fail(VSTAB_ERR_INVALID, "vstab_cvt_nv12_bgr_colour: width and height must be even");
    if (pitch_y < (size_t)width || pitch_uv < (size_t)width || pitch_dst < (size_t)width * 3)
        return fail(VSTAB_ERR_INVALID, "vstab_cvt_nv12_bgr_colour: pitch smaller than row");
    const int vec_ok = ptr_aligned(y, 8) && ptr_aligned(uv, 8) && ptr_aligned(dst, 8) && pitch_y % 8 == 0 && pitch_uv % 8 == 0 && pitch_dst % 8 == 0;
    dim3 block(32, 8);
    dim3 grid(div_up(div_up(width, 8), 32), div_up(div_up(height, 2), 8));
    hipLaunchKernelGGL(k_cvt_nv12_bgr_colour, grid, block, 0, static_cast<hipStream_t>(stream), (const uint8_t *)y, pitch_y, (const uint8_t *)uv, pitch_uv, width,
                       height, (uint8_t *)dst, pitch_dst, vec_ok, colour_coefficients(matrix, range));
    VSTAB_HIP_TRY(hipGetLastError());
    return VSTAB_OK;
}

vstab_status vstab_cvt_bgr_nv12_colour(const void *src_bgr, size_t pitch, int width, int height, void *dst_y, size_t pitch_y, void *dst_uv, size_t pitch_uv,
                                       int matrix, int range, void *stream) {
    VSTAB_TRY(check_colour_spec("vstab_cvt_bgr_nv12_colour", matrix, range));
    if (!src_bgr || !dst_y || !dst_uv) return fail(VSTAB_ERR_INVALID, "vstab_cvt_bgr_nv12_colour: null pointer");
    if (width <= 0 || height <= 0 || (width & 1) || (height & 1)) return fail(VSTAB_ERR_INVALID, "vstab_cvt_bgr_nv12_colour: width and height must be even");
    if (pitch < (size_t)width * 3 || pitch_y < (size_t)width || pitch_uv < (size_t)width)
        return fail(VSTAB_ERR_INVALID, "vstab_cvt_bgr_nv12_colour: pitch smaller than row");
    if (!ptr_aligned(dst_uv, 2) || pitch_uv % 2) return fail(VSTAB_ERR_INVALID, "vstab_cvt_bgr_nv12_colour: chroma plane must be 2-B aligned");
    hipLaunchKernelGGL(k_cvt_bgr_nv12_colour, dim3(div_up(width / 2, 64), div_up(height / 2, 4)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       (const uint8_t *)src_bgr, pitch, width, height, (uint8_t *)dst_y, pitch_y, (uint8_t *)dst_uv, pitch_uv, colour_coefficients(matrix, range));
    VSTAB_HIP_TRY(hipGetLastError());
    return VSTAB_OK;
}

vstab_status vstab_create_map_ex(void *map_x, size_t pitch_x, void *map_y, size_t pitch_y, int cols, int rows,
                                 const float params[17], int map_mode, void *stream) {
    return create_map_impl("vstab_create_map", map_x, pitch_x, map_y, pitch_y, cols, rows, params, nullptr, false, map_mode, stream);
}

vstab_status vstab_create_map_dist(void *map_x, size_t pitch_x, void *map_y, size_t pitch_y, int cols, int rows, const float params[17],
                                   const float dist[4], int map_mode, void *stream) {
    return create_map_impl("vstab_create_map_dist", map_x, pitch_x, map_y, pitch_y, cols, rows, params, dist, true, map_mode, stream);
}

vstab_status vstab_create_map_pinhole(void *map_x, size_t pitch_x, void *map_y, size_t pitch_y, int cols, int rows, const float params[17],
                                      const float dist[5], int map_mode, void *stream) {
    return create_map_pinhole_impl("vstab_create_map_pinhole", map_x, pitch_x, map_y, pitch_y, cols, rows, params, dist, map_mode, stream);
}

vstab_status vstab_create_map(void *map_x, size_t pitch_x, void *map_y, size_t pitch_y, int cols, int rows,
                              const float params[17], void *stream) {
    return vstab_create_map_ex(map_x, pitch_x, map_y, pitch_y, cols, rows, params, VSTAB_MAP_CREATEMAP_CL, stream);
}

size_t vstab_quantised_map_bytes(int dst_width, int dst_height) {
    return dst_width > 0 && dst_height > 0 ? (size_t)((dst_width + 3) & ~3) * dst_height * 8 : 0;
}

vstab_status vstab_quantised_map(void *qmap, int dw, int dh, const float params[17], int map_mode, void *stream) {
    return quantised_map_impl("vstab_quantised_map", qmap, dw, dh, params, nullptr, false, map_mode, stream);
}

vstab_status vstab_quantised_map_dist(void *qmap, int dw, int dh, const float params[17], const float dist[4], int map_mode, void *stream) {
    return quantised_map_impl("vstab_quantised_map_dist", qmap, dw, dh, params, dist, true, map_mode, stream);
}

vstab_status vstab_remap_bilinear(const void *src, size_t pitch_src, int sw, int sh, int channels,
                                  const void *map_x, size_t pitch_x, const void *map_y, size_t pitch_y,
                                  void *dst, size_t pitch_dst, int dw, int dh, void *stream) {
    if (!src || !map_x || !map_y || !dst) return fail(VSTAB_ERR_INVALID, "vstab_remap_bilinear: null pointer");
    if (channels != 1 && channels != 3) return fail(VSTAB_ERR_INVALID, "vstab_remap_bilinear: channels must be 1 or 3");
    if (sw <= 0 || sh <= 0 || dw <= 0 || dh <= 0 || sw > 32767 || sh > 32767)
        return fail(VSTAB_ERR_INVALID, "vstab_remap_bilinear: bad size");
    if (pitch_src < (size_t)sw * channels || pitch_dst < (size_t)dw * channels || pitch_x < (size_t)dw * 4 ||
        pitch_y < (size_t)dw * 4)
        return fail(VSTAB_ERR_INVALID, "vstab_remap_bilinear: pitch smaller than row");
    dim3 grid(div_up(dw, 64), div_up(dh, 4));
    with_either<3, 1>(channels == 3, [&](auto cn) {
        hipLaunchKernelGGL(k_remap_bilinear<decltype(cn)::value>, grid, dim3(64, 4), 0, static_cast<hipStream_t>(stream), (const uint8_t *)src, pitch_src,
                           sw, sh, (const float *)map_x, pitch_x, (const float *)map_y, pitch_y, (uint8_t *)dst, pitch_dst, dw, dh);
    });
    VSTAB_HIP_TRY(hipGetLastError());
    return VSTAB_OK;
}

vstab_status vstab_draw_markers(void *dst, size_t pitch, int width, int height, int channels, const int *centres_xy, int n, int half,
                                unsigned int bgr, void *stream) {
    if (!dst || width <= 0 || height <= 0 || (channels != 1 && channels != 3) || pitch < (size_t)width * channels || n < 0 || half < 0 ||
        half > 16 || (n > 0 && !centres_xy))
        return fail(VSTAB_ERR_INVALID, "vstab_draw_markers: bad argument");
    if (n == 0) return VSTAB_OK;
    hipLaunchKernelGGL(k_draw_markers, dim3(n), dim3(64), 0, static_cast<hipStream_t>(stream), (uint8_t *)dst, pitch, width, height, channels,
                       reinterpret_cast<const int2 *>(centres_xy), half, bgr);
    VSTAB_HIP_TRY(hipGetLastError());
    return VSTAB_OK;
}

}  // extern "C"
