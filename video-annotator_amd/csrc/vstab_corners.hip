// vstab_corners.hip -- the dense corner responses and the two-pass detector for gfx950: k_min_eig / k_corner_harris (also behind
// vstab_min_eig / vstab_corner_harris), k_masked_max, k_corner_candidates / k_corner_candidates_masked.  The detector falls back to them
// from the one-pass kernels of vstab_corners_fused.hip.  Replaces the OpenCV call at FrameSourceWarp.cpp:230 (goodFeaturesToTrack).
// Compiled with -ffp-contract=off: float results are bit-reproducible.
#include <climits>

#include "vstab_corners_tile.hpp"
#include "vstab_internal.hpp"

namespace vstab {

// =============================================================================================
// k_min_eig -- cornerMinEigenVal(blockSize 3, ksize 3): Sobel
// derivatives scaled by 1/(4*3*255) in the documented operation order, products, 3x3 box sum
// (exact in double), minimum eigenvalue in float; also reduces the frame maximum.
// 64 x 16 outputs per workgroup (4 per thread).  Source tile (halo 2, REFLECT_101) and derivative
// tile (halo 1) live in LDS.  The derivative the box filter needs at a position reflected across
// the image border is the derivative AT the mirrored position; computed from the mirrored tile it
// comes out with the sign of the mirrored axis flipped, so dx (dy) is negated for entries whose
// column (row) lies outside the image -- negation is exact, so the floats equal the direct form.
// =============================================================================================
constexpr int ME_TW = 64, ME_TH = 16, ME_SW = ME_TW + 8, ME_SH = ME_TH + 4;  // tile starts at ox - 4 (dword aligned)

template <bool HARRIS>
__device__ __forceinline__ void me_response(const uint8_t *__restrict__ src, size_t pitch, int w, int h, float *__restrict__ eig, int *__restrict__ max_bits, int vec_ok,
                                            float kf) {
    __shared__ __attribute__((aligned(16))) uint8_t tile[ME_SH][ME_SW];
    __shared__ float dxs[ME_TH + 2][ME_TW + 2 + 1], dys[ME_TH + 2][ME_TW + 2 + 1];
    __shared__ int bmax;
    const int tid = threadIdx.x;
    const int ox = blockIdx.x * ME_TW, oy = blockIdx.y * ME_TH;
    const int sx0 = ox - 4, sy0 = oy - 2;
    if (tid == 0) bmax = INT_MIN;
    for (int e = tid; e < ME_SH * (ME_SW / 4); e += 256) {
        const int ry = e / (ME_SW / 4), rd = e - ry * (ME_SW / 4);
        reinterpret_cast<uint32_t *>(&tile[ry][0])[rd] = load4_reflect(src, (uint32_t)pitch, w, h, sx0 + 4 * rd, sy0 + ry, vec_ok != 0);
    }
    __syncthreads();
    const float scale = (float)(1.0 / (4.0 * 3.0 * 255.0));
    const float k0 = 2.0f * scale, k1 = scale;
    // derivative entry (ry, rx) <-> image coordinate (oy - 1 + ry, ox - 1 + rx) <-> tile[ry + 1][rx + 3]
    for (int e = tid; e < (ME_TH + 2) * (ME_TW + 2); e += 256) {
        const int ry = e / (ME_TW + 2), rx = e - ry * (ME_TW + 2);
        const uint8_t *c = &tile[ry + 1][rx + 3];
        const int a00 = c[-ME_SW - 1], a01 = c[-ME_SW], a02 = c[-ME_SW + 1];
        const int a10 = c[-1], a12 = c[1];
        const int a20 = c[ME_SW - 1], a21 = c[ME_SW], a22 = c[ME_SW + 1];
        const float d0 = (float)(a02 - a00), d1 = (float)(a12 - a10), d2 = (float)(a22 - a20);
        float dx = (d0 + d2) * k1 + d1 * k0;
        const float s0 = (float)a01 * k0 + ((float)a00 + (float)a02) * k1;
        const float s2 = (float)a21 * k0 + ((float)a20 + (float)a22) * k1;
        float dy = s2 - s0;
        const int gx = ox - 1 + rx, gy = oy - 1 + ry;
        if (gx < 0 || gx >= w) dx = -dx;
        if (gy < 0 || gy >= h) dy = -dy;
        dxs[ry][rx] = dx, dys[ry][rx] = dy;
    }
    __syncthreads();
    const int q = tid & 15, ty = tid >> 4;
    const int x = ox + 4 * q, y = oy + ty;
    int best = INT_MIN;
    if (x < w && y < h) {
        float a_[3][6], b_[3][6];
#pragma unroll
        for (int j = 0; j < 3; j++)
#pragma unroll
            for (int i = 0; i < 6; i++) a_[j][i] = dxs[ty + j][4 * q + i], b_[j][i] = dys[ty + j][4 * q + i];
        float ev[4];
#pragma unroll
        for (int c = 0; c < 4; c++) {
            double sxx = 0, sxy = 0, syy = 0;
#pragma unroll
            for (int j = 0; j < 3; j++)
#pragma unroll
                for (int i = 0; i < 3; i++) {
                    const float a = a_[j][c + i], b = b_[j][c + i];
                    sxx += (double)(a * a), sxy += (double)(a * b), syy += (double)(b * b);
                }
            if (HARRIS) {
                const float a = (float)sxx, b = (float)sxy, cc = (float)syy, t = a + cc;
                ev[c] = (a * cc - b * b) - (kf * t) * t;
            } else {
                const float a = (float)sxx * 0.5f, b = (float)sxy, cc = (float)syy * 0.5f;
                ev[c] = (a + cc) - sqrtf((a - cc) * (a - cc) + b * b);
            }
            if (x + c < w) best = max(best, __float_as_int(ev[c]));
        }
        float *o = eig + (size_t)y * w + x;
        if (vec_ok && (w & 3) == 0 && x + 4 <= w) {
            *reinterpret_cast<float4 *>(o) = make_float4(ev[0], ev[1], ev[2], ev[3]);
        } else {
            for (int c = 0; c < 4 && x + c < w; c++) o[c] = ev[c];
        }
    }
    // frame maximum: the maximum inside each 16-lane row, one LDS atomic per row, one global atomic per block
    best = row_max_i32(best);
    if (q == 15) atomicMax(&bmax, best);
    __syncthreads();
    if (tid == 0) atomicMax(max_bits, bmax);
}

__global__ void __launch_bounds__(256) k_min_eig(const uint8_t *__restrict__ src, size_t pitch, int w, int h,
                                                 float *__restrict__ eig, int *__restrict__ max_bits, int vec_ok) {
    me_response<false>(src, pitch, w, h, eig, max_bits, vec_ok, 0.0f);
}

// k_corner_harris -- cornerHarris(blockSize 3, ksize 3, k) as a dense map (vstab.h, "Harris response"; kf = (float)k): k_min_eig but for
// the response R = (a c - b b) - (kf t) t, t = a + c, over the box sums as they are -- one body, me_response<HARRIS>, behind both names.
// (Through the shared body the compiler puts some 40 instructions near the tile load of either kernel in another order and numbers
// registers differently: the same instructions and resources, and the same run time -- profiles/detector_split.txt.)  The frame maximum is taken in the same int-bit order:
// its SIGN is right also where the order among negative values is not, and the sign is all the host asks it for when the maximum is not positive.
__global__ void __launch_bounds__(256) k_corner_harris(const uint8_t *__restrict__ src, size_t pitch, int w, int h,
                                                       float *__restrict__ eig, int *__restrict__ max_bits, int vec_ok, float kf) {
    me_response<true>(src, pitch, w, h, eig, max_bits, vec_ok, kf);
}

// =============================================================================================
// k_corner_candidates -- goodFeaturesToTrack steps 4-5: threshold at
// quality*max (THRESH_TOZERO, strict >), 3x3 dilate-compare, interior pixels only.  A candidate is
// emitted as the 64-bit key (float bits << 32 | raster index): sorting keys descending gives
// OpenCV's order (value descending, ties -> later raster position first).
// =============================================================================================
template <bool MASKED>
__device__ __forceinline__ void corner_candidates(const float *__restrict__ eig, int w, int h, const int *__restrict__ max_bits, double quality,
                                                  unsigned long long *__restrict__ keys, unsigned int *__restrict__ count, unsigned int cap,
                                                  const uint8_t *__restrict__ mask, size_t mpitch) {
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x < 1 || y < 1 || x >= w - 1 || y >= h - 1) return;
    if (MASKED && mask[(size_t)y * mpitch + x] == 0) return;
    const float thr = (float)((double)__int_as_float(*max_bits) * quality);
    const float *p = eig + (size_t)y * w + x;
    const float v = p[0];
    if (!(v > thr)) return;
    float m = v;
    m = fmaxf(m, p[-w - 1]), m = fmaxf(m, p[-w]), m = fmaxf(m, p[-w + 1]);
    m = fmaxf(m, p[-1]), m = fmaxf(m, p[1]);
    m = fmaxf(m, p[w - 1]), m = fmaxf(m, p[w]), m = fmaxf(m, p[w + 1]);
    if (v != m) return;
    const unsigned int slot = atomicAdd(count, 1u);
    if (slot < cap) keys[slot] = ((unsigned long long)__float_as_uint(v) << 32) | (unsigned int)(y * w + x);
}

__global__ void __launch_bounds__(256) k_corner_candidates(const float *__restrict__ eig, int w, int h,
                                                           const int *__restrict__ max_bits, double quality,
                                                           unsigned long long *__restrict__ keys,
                                                           unsigned int *__restrict__ count, unsigned int cap) {
    corner_candidates<false>(eig, w, h, max_bits, quality, keys, count, cap, nullptr, 0);
}

// k_corner_candidates_masked -- k_corner_candidates plus the gate: a candidate has a non-zero mask byte.  The threshold (max_bits: the
// masked maximum) and the 3 x 3 maximum test run over every pixel, masked out or not.
__global__ void __launch_bounds__(256) k_corner_candidates_masked(const float *__restrict__ eig, int w, int h, const int *__restrict__ max_bits, double quality,
                                                                  unsigned long long *__restrict__ keys, unsigned int *__restrict__ count, unsigned int cap,
                                                                  const uint8_t *__restrict__ mask, size_t mpitch) {
    corner_candidates<true>(eig, w, h, max_bits, quality, keys, count, cap, mask, mpitch);
}

// The two-pass detector under a mask: k_min_eig as it is, then
// k_masked_max -- minMaxLoc(eig, ., &maxVal, ., ., mask): the maximum of the eigenvalue map over the pixels with a non-zero mask byte, in
// the int-bit order and into a word initialised as k_min_eig's (launch_masked_max).  64 x 16 pixels per workgroup, a wave per 4 rows;
// reduced inside the wave (DPP), one LDS atomic per wave, one global atomic per workgroup.
__global__ void __launch_bounds__(256) k_masked_max(const float *__restrict__ eig, int w, int h, const uint8_t *__restrict__ mask, size_t mpitch,
                                                    int *__restrict__ max_bits) {
    __shared__ int bmax;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) bmax = INT_MIN;
    __syncthreads();
    const int x = blockIdx.x * 64 + lane;
    int best = INT_MIN;
    if (x < w) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int y = blockIdx.y * 16 + wave * 4 + r;
            if (y < h && mask[(size_t)y * mpitch + x] != 0) best = max(best, __float_as_int(eig[(size_t)y * w + x]));
        }
    }
    best = wave_max_i32(best);
    if (lane == 63) atomicMax(&bmax, best);
    __syncthreads();
    if (tid == 0) atomicMax(max_bits, bmax);
}

// the dense response map (k_min_eig, or k_corner_harris with kf = (float)k) and *max_bits, its int-bit maximum
// (block or gradient other than 3: the kernels of vstab_corners_block.hip)
vstab_status launch_corner_response(const uint8_t *src, size_t pitch, int w, int h, bool harris, float kf, float *resp, int *max_bits, hipStream_t s, int block,
                                    int gradient) {
    VSTAB_HIP_TRY(hipMemsetAsync(max_bits, 0x80, sizeof(int), s));  // INT_MIN-ish (0x80808080): any value wins
    if (block != 3 || gradient != 3) return launch_corner_response_block(src, pitch, w, h, block, harris, kf, resp, max_bits, s, gradient);
    const int vec_ok = reinterpret_cast<uintptr_t>(src) % 4 == 0 && pitch % 4 == 0 && reinterpret_cast<uintptr_t>(resp) % 16 == 0;
    dim3 grid(div_up(w, ME_TW), div_up(h, ME_TH));
    if (harris) hipLaunchKernelGGL(k_corner_harris, grid, dim3(256), 0, s, src, pitch, w, h, resp, max_bits, vec_ok, kf);
    else hipLaunchKernelGGL(k_min_eig, grid, dim3(256), 0, s, src, pitch, w, h, resp, max_bits, vec_ok);
    VSTAB_HIP_TRY(hipGetLastError());
    return VSTAB_OK;
}

// the masked maximum of a response map (behind launch_corner_response, whose max_bits holds the maximum of the whole frame) into *masked_max_bits
vstab_status launch_masked_max(const float *eig, int w, int h, const uint8_t *mask, size_t mpitch, int *masked_max_bits, hipStream_t s) {
    VSTAB_HIP_TRY(hipMemsetAsync(masked_max_bits, 0x80, sizeof(int), s));  // as launch_corner_response
    hipLaunchKernelGGL(k_masked_max, dim3(div_up(w, 64), div_up(h, 16)), dim3(256), 0, s, eig, w, h, mask, mpitch, masked_max_bits);
    VSTAB_HIP_TRY(hipGetLastError());
    return VSTAB_OK;
}

vstab_status launch_corner_candidates(const float *eig, int w, int h, const int *max_bits, double quality,
                                      unsigned long long *keys, unsigned int *count, unsigned int cap, hipStream_t s, const DetectSpec &spec) {
    VSTAB_HIP_TRY(hipMemsetAsync(count, 0, sizeof(unsigned int), s));
    dim3 grid(div_up(w, 64), div_up(h, 4));
    if (spec.mask) hipLaunchKernelGGL(k_corner_candidates_masked, grid, dim3(64, 4), 0, s, eig, w, h, max_bits, quality, keys, count, cap, spec.mask, spec.mask_pitch);
    else hipLaunchKernelGGL(k_corner_candidates, grid, dim3(64, 4), 0, s, eig, w, h, max_bits, quality, keys, count, cap);
    VSTAB_HIP_TRY(hipGetLastError());
    return VSTAB_OK;
}

// Kernels of this translation unit are one code object, loaded by the runtime at the first launch of any of them.  Touching one of them
// here (vstab_preload_kernels) moves that load to a moment the caller chooses.  (The one-pass detector is a unit, and a code object, of
// its own: preload_corners_fused_kernels.)
vstab_status preload_corner_kernels() {
    hipFuncAttributes at;
    VSTAB_HIP_TRY(hipFuncGetAttributes(&at, reinterpret_cast<const void *>(&k_min_eig)));
    // (k_corner_harris, k_masked_max and the two candidate kernels are kernels of this unit: the same code object, loaded with it)
    return VSTAB_OK;
}

}  // namespace vstab
