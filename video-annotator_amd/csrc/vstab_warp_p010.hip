// vstab_warp_p010.hip -- BASELINE.json config 5: the undistort-remap with a 10-bit pixel path.
// No reference counterpart (the reference is 8-bit throughout): the arithmetic is DEFINED in the oracle
// (its warp_p010 chain) and reproduced here bit for bit.
//   P010 planes (16-bit samples, 10 significant bits at the top)  ->  sample >> 6
//   BT.601 limited range at 10 bits: the 8-bit cvtColor constants and shift with offsets 64 / 512 (the definition sums in
//     64 bits: 959 * CY + 511 * CUB exceeds int32)  ->  B, G, R in [0, 1023]
//   the map of vstab_create_map_ex (all five projection pairs), optionally with a rotation per output row
//     (vstab_warp_nv12_rs's interpolation), quantised like cv::remap
//   blend of the four converted taps: VSTAB_BLEND_EXACT  (sum p*w + 512) >> 10, integers, as the 8-bit path;
//     VSTAB_BLEND_FP16  four fused multiply-adds in binary16 with the weights as w / 1024 (exact in binary16),
//     taps in the order 00, 01, 10, 11, then round-to-nearest-even and clamp -- the "fp16 blend" of config 5,
//     within 2 levels of the exact one
//   BGR, three 16-bit samples per pixel, values 0..1023.
// Direct gather, two output pixels per thread: this path is about the format, the 8-bit kernel carries the rate.
#include <cstdlib>

#include "vstab_colour.hpp"
#include "vstab_device10.hpp"
#include "vstab_warp_host.hpp"

namespace vstab {

struct P010Args {
    const uint8_t *y, *uv;
    uint16_t *dst;
    size_t pitch_y, pitch_uv, pitch_dst;  // bytes
    int sw, sh, dw, dh;
    MapParams p;
    float rs_d[9];  // rotation of the last output row minus rotation of the first (all zero: one rotation)
    float rs_den;   // (float)max(dh - 1, 1)
    int rs;
    // the COLOUR kernels' coefficients (vstab_warp_p010_colour); behind everything the other kernels read, which stays where it was
    ColourCoef col;
};

// the four taps of one output pixel, converted and blended; sx, sy = cvRound(32 * map)
template <int BLEND, bool COLOUR>
__device__ __forceinline__ void sample10(const P010Args &a, float ax, float ay, uint16_t *o) {
    const bool far = !(fabsf(ax) < 1073741824.0f) || !(fabsf(ay) < 1073741824.0f);
    const int sx = (int)__builtin_rintf(ax), sy = (int)__builtin_rintf(ay);
    const int X = sx >> 5, Y = sy >> 5, fx = sx & 31, fy = sy & 31;
    int B = 0, G = 0, R = 0;
    if (!(far || X >= a.sw || X + 1 < 0 || Y >= a.sh || Y + 1 < 0)) {
        const int w00 = (32 - fx) * (32 - fy), w01 = fx * (32 - fy), w10 = (32 - fx) * fy, w11 = fx * fy;
        int b0, g0, r0, b1, g1, r1, b2, g2, r2, b3, g3, r3;
        // the coefficient source (vstab_device10.hpp): a.col itself, not a copy of it, or cvtColor's constants
        const auto &k = [&]() -> decltype(auto) { if constexpr (COLOUR) return (a.col); else return CvtColor10{}; }();
        fetch_row10(a, k, X, Y, b0, g0, r0, b1, g1, r1);
        fetch_row10(a, k, X, Y + 1, b2, g2, r2, b3, g3, r3);
        if constexpr (BLEND == VSTAB_BLEND_FP16) {
            B = blend_fp16(b0, b1, b2, b3, w00, w01, w10, w11);
            G = blend_fp16(g0, g1, g2, g3, w00, w01, w10, w11);
            R = blend_fp16(r0, r1, r2, r3, w00, w01, w10, w11);
        } else {
            B = (b0 * w00 + b1 * w01 + b2 * w10 + b3 * w11 + 512) >> 10;
            G = (g0 * w00 + g1 * w01 + g2 * w10 + g3 * w11 + 512) >> 10;
            R = (r0 * w00 + r1 * w01 + r2 * w10 + r3 * w11 + 512) >> 10;
        }
    }
    o[0] = (uint16_t)B, o[1] = (uint16_t)G, o[2] = (uint16_t)R;
}

// The map of two pixels of one column, map mode 0 or 1 (FISH_TO_RECT): fish_chain (vstab_map.hpp) over f32x2.  a = column terms, b = row terms,
// r = third column of the rotation, each for the two rows.  The rays are formed here, not in the kernel: there its eight instantiations
// came out another (903 -> 905 lines, 30 -> 29 registers, and the like).
template <bool FISH_TO_RECT>
__device__ __forceinline__ void map_pair(float icx32, float icy32, float ifx32, float ify32, f32x2 r02, f32x2 r12, f32x2 r22,
                                         f32x2 a0, f32x2 a1, f32x2 a2, f32x2 b0, f32x2 b1, f32x2 b2, f32x2 &ax, f32x2 &ay) {
    const f32x2 wz = (a2 + b2) + r22;
    const struct {
        f32x2 icx32, icy32, ifx32, ify32;
    } cam = {splat2(icx32), splat2(icy32), splat2(ifx32), splat2(ify32)};
    fish_chain<FISH_TO_RECT, false>(cam, (a0 + b0) + r02, (a1 + b1) + r12, wz, ax, ay);
    if constexpr (FISH_TO_RECT) {  // behind the camera: outside
        const i32x2 ok = wz > splat2(0.0f);
        ax = ok ? ax : splat2(__builtin_nanf("")), ay = ok ? ay : splat2(__builtin_nanf(""));
    }
}
// A thread owns two vertically adjacent output pixels, so that the map of the fisheye-input modes runs as packed fp32
// (fish_chain over f32x2: the hand-scheduled IEEE sequences of the 8-bit kernel, two pixels per instruction; 32 * map, an
// exact power-of-two scaling of the map the definition quantises).
// COLOUR (vstab_warp_p010_colour): the taps are converted with the coefficients of a.col, a spec's row of the 10-bit table.
template <int MODE, int BLEND, bool COLOUR = false>
__global__ void __launch_bounds__(256) k_warp_p010(P010Args a) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y0 = (blockIdx.y * 4 + (threadIdx.x >> 6)) * 2;
    if (x >= a.dw || y0 >= a.dh) return;
    float m[2][9];
#pragma unroll
    for (int r = 0; r < 2; r++) {
        const float t = (float)(y0 + r) / a.rs_den;
#pragma unroll
        for (int k = 0; k < 9; k++) m[r][k] = a.rs ? __builtin_fmaf(t, a.rs_d[k], a.p.r[k]) : a.p.r[k];
    }
    constexpr bool OCL = MODE == MAP_CREATEMAP_CL_OPENCL;  // createMap.cl as ROCm's OpenCL compiler builds it: reciprocal-based divisions
    const float vx = OCL ? ocl_div((float)x - a.p.ocx, a.p.ofx) : ((float)x - a.p.ocx) / a.p.ofx;
    const float vy[2] = {OCL ? ocl_div((float)y0 - a.p.ocy, a.p.ofy) : ((float)y0 - a.p.ocy) / a.p.ofy,
                         OCL ? ocl_div((float)(y0 + 1) - a.p.ocy, a.p.ofy) : ((float)(y0 + 1) - a.p.ocy) / a.p.ofy};
    float ax[2], ay[2];
    if constexpr (MODE == MAP_CREATEMAP_CL || MODE == MAP_FISH_TO_RECT) {
        // the rays of the two rows: column terms, row terms and third column each of the row's own rotation
        f32x2 px, py;
        map_pair<MODE == MAP_FISH_TO_RECT>(a.p.icx * 32.0f, a.p.icy * 32.0f, a.p.ifx * 32.0f, a.p.ify * 32.0f, (f32x2){m[0][2], m[1][2]},
                                           (f32x2){m[0][5], m[1][5]}, (f32x2){m[0][8], m[1][8]}, (f32x2){m[0][0] * vx, m[1][0] * vx},
                                           (f32x2){m[0][3] * vx, m[1][3] * vx}, (f32x2){m[0][6] * vx, m[1][6] * vx},
                                           (f32x2){m[0][1] * vy[0], m[1][1] * vy[1]}, (f32x2){m[0][4] * vy[0], m[1][4] * vy[1]},
                                           (f32x2){m[0][7] * vy[0], m[1][7] * vy[1]}, px, py);
        ax[0] = px.x, ax[1] = px.y, ay[0] = py.x, ay[1] = py.y;
    } else {
#pragma unroll
        for (int r = 0; r < 2; r++) {
            MapParams q = a.p;
#pragma unroll
            for (int k = 0; k < 9; k++) q.r[k] = m[r][k];
            // the preamble in place, not through map_at: that reorders the four MAP_RECT_TO_RECT kernels (19 to 44 lines in place)
            const ColTerm ct = {q.r[0] * vx, q.r[3] * vx, q.r[6] * vx};
            const RowTerm rt = {q.r[1] * vy[r], q.r[4] * vy[r], q.r[7] * vy[r]};
            const MapParams32 in = {q.icx, q.icy, q.ifx, q.ify, q.r[2], q.r[5], q.r[8]};  // unscaled
            float mx, my;
            map_pixel_ex<MODE>(in, q, ct, rt, vx, vy[r], mx, my);
            ax[r] = mx * 32.0f, ay[r] = my * 32.0f;
        }
    }
#pragma unroll
    for (int r = 0; r < 2; r++) {
        if (y0 + r >= a.dh) break;
        sample10<BLEND, COLOUR>(a, ax[r], ay[r], reinterpret_cast<uint16_t *>(reinterpret_cast<uint8_t *>(a.dst) + (size_t)(y0 + r) * a.pitch_dst) + 3 * (size_t)x);
    }
}

// k_cvt_bgr10_p010 -- the encoder hand-off of the 10-bit path: BGR (0..1023 in 16-bit containers) -> P010 planes, the BGR -> YUV
// arithmetic of the NV12 output (cvtColor's BT.601 constants, 20-bit shift) at 10 bits: offsets 64 / 512, saturation to
// [0, 1023], sample << 6; chroma from the top-left pixel of each 2 x 2 block (definition: include/vstab.h).  One
// thread converts two adjacent pixels of a row: 12 bytes in, one luma dword out, on even rows one (U, V) dword.
__global__ void __launch_bounds__(256) k_cvt_bgr10_p010(const uint8_t *__restrict__ src, size_t pitch_src, int w, int h, uint8_t *__restrict__ dy,
                                                        size_t pitch_y, uint8_t *__restrict__ duv, size_t pitch_uv) {
    const int px = (blockIdx.x * 64 + (threadIdx.x & 63)) * 2, y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (px >= w || y >= h) return;
    const uint16_t *s = reinterpret_cast<const uint16_t *>(src + (size_t)y * pitch_src) + 3 * (size_t)px;
    const bool two = px + 1 < w;
    const int B0 = s[0], G0 = s[1], R0 = s[2], B1 = two ? s[3] : 0, G1 = two ? s[4] : 0, R1 = two ? s[5] : 0;
    using C = CvtColor10;  // cvtColor's constants at 10 bits (vstab_device.hpp)
    constexpr int half = 1 << 19;
    const int y0 = sat10((C::cry * R0 + C::cgy * G0 + C::cby * B0 + half + (C::yoff << 20)) >> 20), y1 = sat10((C::cry * R1 + C::cgy * G1 + C::cby * B1 + half + (C::yoff << 20)) >> 20);
    uint16_t *oy = reinterpret_cast<uint16_t *>(dy + (size_t)y * pitch_y) + px;
    if (two && (reinterpret_cast<uintptr_t>(oy) & 3) == 0) *reinterpret_cast<uint32_t *>(oy) = ((uint32_t)y0 << 6) | ((uint32_t)y1 << 22);
    else {
        oy[0] = (uint16_t)(y0 << 6);
        if (two) oy[1] = (uint16_t)(y1 << 6);
    }
    if (!(y & 1)) {
        const int U = sat10((C::cru * R0 + C::cgu * G0 + C::cbu * B0 + half + (512 << 20)) >> 20), V = sat10((C::cbu * R0 + C::cgv * G0 + C::cbv * B0 + half + (512 << 20)) >> 20);
        *reinterpret_cast<uint32_t *>(duv + (size_t)(y >> 1) * pitch_uv + (size_t)px * 2) = ((uint32_t)U << 6) | ((uint32_t)V << 22);
    }
}

// k_cvt_bgr10_p010 with a colour spec: the inverse of "Colour matrix and range at 10 bits" (include/vstab.h), k: the spec's row.  Its own
// body: bgr10_to_y / bgr10_to_uv with cvtColor's constants do not compile to k_cvt_bgr10_p010's instructions.
__global__ void __launch_bounds__(256) k_cvt_bgr10_p010_colour(const uint8_t *__restrict__ src, size_t pitch_src, int w, int h, uint8_t *__restrict__ dy,
                                                               size_t pitch_y, uint8_t *__restrict__ duv, size_t pitch_uv, ColourCoef k) {
    const int px = (blockIdx.x * 64 + (threadIdx.x & 63)) * 2, y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (px >= w || y >= h) return;
    const uint16_t *s = reinterpret_cast<const uint16_t *>(src + (size_t)y * pitch_src) + 3 * (size_t)px;
    const bool two = px + 1 < w;
    // (the definition takes B, G, R in [0, 1023]; the low ten bits of a container are what every sum below is sized for)
    const int B0 = s[0] & 1023, G0 = s[1] & 1023, R0 = s[2] & 1023, B1 = two ? s[3] & 1023 : 0, G1 = two ? s[4] & 1023 : 0, R1 = two ? s[5] & 1023 : 0;
    const uint32_t y0 = bgr10_to_y(k, B0, G0, R0), y1 = bgr10_to_y(k, B1, G1, R1);
    uint16_t *oy = reinterpret_cast<uint16_t *>(dy + (size_t)y * pitch_y) + px;
    if (two && (reinterpret_cast<uintptr_t>(oy) & 3) == 0) *reinterpret_cast<uint32_t *>(oy) = (y0 << 6) | (y1 << 22);
    else {
        oy[0] = (uint16_t)(y0 << 6);
        if (two) oy[1] = (uint16_t)(y1 << 6);
    }
    if (!(y & 1)) *reinterpret_cast<uint32_t *>(duv + (size_t)(y >> 1) * pitch_uv + (size_t)px * 2) = bgr10_to_uv(k, B0, G0, R0) << 6;
}

// k_cvt_p010_bgr16_colour -- P010 planes -> BGR (0..1023 in 16-bit containers) with a colour spec: the forward conversion of "Colour matrix
// and range at 10 bits", the low six bits of every source word ignored.  One thread converts the two pixels of a chroma pair: one luma
// dword and one chroma dword in, 12 bytes out, as three dwords where the row is 4-byte aligned, as six words otherwise.
__global__ void __launch_bounds__(256) k_cvt_p010_bgr16_colour(const uint8_t *__restrict__ sy, size_t pitch_y, const uint8_t *__restrict__ suv, size_t pitch_uv,
                                                               int w, int h, uint8_t *__restrict__ dst, size_t pitch_dst, ColourCoef k) {
    const int px = (blockIdx.x * 64 + (threadIdx.x & 63)) * 2, y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (px >= w || y >= h) return;  // (w is even: a pair is whole)
    const uint32_t yy = reinterpret_cast<const Dword1 *>(sy + (size_t)y * pitch_y + (size_t)px * 2)->v;  // (a luma row is 2-byte aligned)
    const uint32_t cw = *reinterpret_cast<const uint32_t *>(suv + (size_t)(y >> 1) * pitch_uv + (size_t)px * 2);
    int b0, g0, r0, b1, g1, r1;
    convert_tap10(k, yy & 0xffffu, cw, true, b0, g0, r0);
    convert_tap10(k, yy >> 16, cw, true, b1, g1, r1);
    uint8_t *o = dst + (size_t)y * pitch_dst + (size_t)px * 6;
    if ((reinterpret_cast<uintptr_t>(o) & 3) == 0) {
        uint32_t *o4 = reinterpret_cast<uint32_t *>(o);
        o4[0] = (uint32_t)b0 | ((uint32_t)g0 << 16), o4[1] = (uint32_t)r0 | ((uint32_t)b1 << 16), o4[2] = (uint32_t)g1 | ((uint32_t)r1 << 16);
    } else {
        uint16_t *o2 = reinterpret_cast<uint16_t *>(o);
        o2[0] = (uint16_t)b0, o2[1] = (uint16_t)g0, o2[2] = (uint16_t)r0, o2[3] = (uint16_t)b1, o2[4] = (uint16_t)g1, o2[5] = (uint16_t)r1;
    }
}


// Kernels of this translation unit are one code object, loaded by the runtime at the first launch of any of them.  Touching one of them
// here (vstab_preload_kernels) moves that load to a moment the caller chooses.
vstab_status preload_p010_kernels() {
    hipFuncAttributes at;
    VSTAB_HIP_TRY(hipFuncGetAttributes(&at, reinterpret_cast<const void *>(&k_warp_p010<MAP_CREATEMAP_CL, VSTAB_BLEND_EXACT>)));
    return VSTAB_OK;
}

}  // namespace vstab

using namespace vstab;

namespace {

// The three P010 warps differ in what leaves them -- 16-bit BGR (vstab_warp_p010), P010 planes from the fused kernel (_planes), P010 planes
// plane by plane (_planar; _planar_ex, the cubic and Lanczos resamplers: _planar's checks but for the pitch limit of its 32-bit offsets) --
// and in which of the shared checks they make.
enum P010Out { P010_BGR16, P010_PLANES, P010_PLANAR, P010_PLANAR_EX };

// Their arguments, checked in one order with each message under the entry point's own name n, into the kernel argument.  dst / dst_uv: the
// output planes (BGR16: dst alone).  _planes leaves the source planes and the map mode to its tiled_ok (VSTAB_ERR_UNSUPPORTED, not _INVALID).
vstab_status check_warp_p010(const std::string &n, P010Out out, const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int sw, int sh,
                             const float params[17], const float *rot_bottom, int map_mode, int blend, void *dst, size_t pitch_dst, void *dst_uv,
                             size_t pitch_dst_uv, int dw, int dh, WarpArgs &a) {
    const bool planes = out != P010_BGR16;
    if (!y || !uv || !dst || (planes && !dst_uv) || !params) return fail(VSTAB_ERR_INVALID, n + ": null pointer");
    if (sw < (planes ? 8 : 4) || sh < 2 || (sw & 1) || (sh & 1) || dw <= 0 || dh <= 0 || sw > 32767 || sh > 32767 || dw > 32767 || dh > 32767)
        return fail(VSTAB_ERR_INVALID, n + ": sizes must be in [1, 32767], source even and at least " + (planes ? "8 x 2" : "4 x 2"));
    const bool src_bad = pitch_y < (size_t)sw * 2 || pitch_uv < (size_t)sw * 2 || pitch_y % 2 || pitch_uv % 4 || !ptr_aligned(y, 2) || !ptr_aligned(uv, 4);
    const bool dst_bad = planes ? pitch_dst < (size_t)dw * 2 || pitch_dst % 2 || pitch_dst_uv < (size_t)((dw + 1) / 2) * 4 || pitch_dst_uv % 4 ||
                                      !ptr_aligned(dst, 2) || !ptr_aligned(dst_uv, 4)
                                : pitch_dst < (size_t)dw * 6 || pitch_dst % 2 || !ptr_aligned(dst, 2);
    if (out == P010_BGR16 && (src_bad || dst_bad)) return fail(VSTAB_ERR_INVALID, n + ": bad pitch or alignment (16-bit samples; chroma pairs 4-byte aligned)");
    const bool planar = out == P010_PLANAR || out == P010_PLANAR_EX;
    if (planar && src_bad)
        return fail(VSTAB_ERR_INVALID, n + ": bad source pitch or alignment (16-bit samples; chroma pairs 4-byte aligned)");
    if (planes && dst_bad) return fail(VSTAB_ERR_INVALID, n + ": bad output pitch or alignment (16-bit samples; chroma pairs 4-byte aligned)");
    if (out != P010_PLANES && (map_mode < VSTAB_MAP_CREATEMAP_CL || map_mode > VSTAB_MAP_CREATEMAP_CL_OPENCL))
        return fail(VSTAB_ERR_INVALID, n + ": unknown map mode");
    if (blend != VSTAB_BLEND_EXACT && blend != VSTAB_BLEND_FP16) return fail(VSTAB_ERR_INVALID, n + ": unknown blend");
    if (planar) {
        if (rot_bottom && !map_mode_fish_to_pinhole(map_mode))
            return fail(VSTAB_ERR_INVALID, n + ": the per-row warp exists for the fisheye -> pinhole modes (0, 1, 5) only");
        if (out == P010_PLANAR && !staged_offsets32(pitch_y, pitch_uv, sh).rows) return fail(VSTAB_ERR_INVALID, n + ": source pitch too large");
    }
    fill_warp_args(a, y, pitch_y, uv, pitch_uv, sw, sh, params, dst, pitch_dst, planes ? dst_uv : nullptr, planes ? pitch_dst_uv : 0, dw, dh);
    return VSTAB_OK;
}

// the planes and pitches of the source allow 16-byte staging loads
bool source_16(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv) {
    return ptr_aligned(y, 16) && ptr_aligned(uv, 16) && pitch_y % 16 == 0 && pitch_uv % 16 == 0;
}

}  // namespace

// The same warp with P010 planes out, fused (FMT 3 of the tiled kernel): VSTAB_ERR_UNSUPPORTED when the planes do not allow the tiled
// kernel (the caller then warps to 16-bit BGR and converts: vstab_pull_frame_p010 does).
// n: the entry point's name; matrix, range: its colour spec (the twin without one passes the default, which launches the default kernel)
static vstab_status warp_p010_planes(const char *n, const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int sw, int sh, const float params[17],
                                     const float *rot_bottom, int map_mode, int blend, void *dst_y, size_t pitch_dst_y, void *dst_uv, size_t pitch_dst_uv,
                                     int dw, int dh, int matrix, int range, void *stream) {
    WarpArgs wa;
    const vstab_status st = check_warp_p010(n, P010_PLANES, y, pitch_y, uv, pitch_uv, sw, sh, params, rot_bottom, map_mode, blend, dst_y,
                                            pitch_dst_y, dst_uv, pitch_dst_uv, dw, dh, wa);
    if (st != VSTAB_OK) return st;
    const StagedOffsets32 off32 = staged_offsets32(pitch_y, pitch_uv, sh);
    const bool tiled_ok = map_mode_fish_to_pinhole(map_mode) && source_16(y, pitch_y, uv, pitch_uv) && pitch_y >= (size_t)sw * 2 && pitch_uv >= (size_t)sw * 2 &&
                          off32.rows && (uint64_t)pitch_dst_y * dh < (1ull << 32);
    if (!tiled_ok) return fail(VSTAB_ERR_UNSUPPORTED, std::string(n) + ": needs 16-byte aligned source planes and a fisheye -> pinhole map");
    VSTAB_TRY(check_colour_spec(n, matrix, range));
    // a chroma plane of 4 GiB or more (staged_offsets32) is sampled from global memory (64-bit addresses)
    const bool vec = ptr_aligned(dst_y, 8) && ptr_aligned(dst_uv, 8) && pitch_dst_y % 8 == 0 && pitch_dst_uv % 8 == 0;
    const ColourCoef col = colour_coefficients10(matrix, range);
    return launch_warp_fused10(wa, params, map_mode, blend, rot_bottom, true, off32.chroma, vec, static_cast<hipStream_t>(stream),
                               colour_spec_default(matrix, range) ? nullptr : &col);
}

extern "C" vstab_status vstab_warp_p010_planes(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int sw, int sh, const float params[17],
                                               const float *rot_bottom, int map_mode, int blend, void *dst_y, size_t pitch_dst_y, void *dst_uv,
                                               size_t pitch_dst_uv, int dw, int dh, void *stream) {
    return warp_p010_planes("vstab_warp_p010_planes", y, pitch_y, uv, pitch_uv, sw, sh, params, rot_bottom, map_mode, blend, dst_y, pitch_dst_y, dst_uv, pitch_dst_uv, dw,
                            dh, VSTAB_COLOUR_CVTCOLOR, VSTAB_RANGE_LIMITED, stream);
}

extern "C" vstab_status vstab_warp_p010_planes_colour(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int sw, int sh, const float params[17],
                                                      const float *rot_bottom, int map_mode, int blend, void *dst_y, size_t pitch_dst_y, void *dst_uv,
                                                      size_t pitch_dst_uv, int dw, int dh, int matrix, int range, void *stream) {
    return warp_p010_planes("vstab_warp_p010_planes_colour", y, pitch_y, uv, pitch_uv, sw, sh, params, rot_bottom, map_mode, blend, dst_y, pitch_dst_y, dst_uv, pitch_dst_uv,
                            dw, dh, matrix, range, stream);
}

// The plane-wise 10-bit warp (vstab_warp_planar.hip, DEPTH 10): P010 planes in and out, no colour conversion at all.
extern "C" vstab_status vstab_warp_p010_planar(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int sw, int sh, const float params[17],
                                               const float *rot_bottom, int map_mode, int blend, void *dst_y, size_t pitch_dst_y, void *dst_uv,
                                               size_t pitch_dst_uv, int dw, int dh, void *stream) {
    WarpArgs wa;
    const vstab_status st = check_warp_p010("vstab_warp_p010_planar", P010_PLANAR, y, pitch_y, uv, pitch_uv, sw, sh, params, rot_bottom, map_mode, blend, dst_y,
                                            pitch_dst_y, dst_uv, pitch_dst_uv, dw, dh, wa);
    if (st != VSTAB_OK) return st;
    // 16-byte staging loads; a chroma plane of 4 GiB or more (staged_offsets32) is sampled from global memory instead
    const bool src16 = source_16(y, pitch_y, uv, pitch_uv) && staged_offsets32(pitch_y, pitch_uv, sh).chroma;
    const bool dst16 = ptr_aligned(dst_y, 16) && ptr_aligned(dst_uv, 16) && pitch_dst_y % 16 == 0 && pitch_dst_uv % 16 == 0;
    return launch_warp_planar(wa, params, map_mode, 10, blend, src16, dst16, rot_bottom, static_cast<hipStream_t>(stream));
}

// The plane-wise 10-bit warp with cv::remap's cubic or Lanczos resampler and a border mode (vstab_warp_p010_resample.hip): _planar's
// argument checks under this name, then the resampler, then the border mode -- all before any launch.
extern "C" vstab_status vstab_warp_p010_planar_ex(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int sw, int sh, const float params[17],
                                                  const float *rot_bottom, int map_mode, int resample, int border_mode, void *dst_y, size_t pitch_dst_y,
                                                  void *dst_uv, size_t pitch_dst_uv, int dw, int dh, void *stream) {
    const std::string n = "vstab_warp_p010_planar_ex";
    BorderArgs ba;
    const vstab_status st = check_warp_p010(n, P010_PLANAR_EX, y, pitch_y, uv, pitch_uv, sw, sh, params, rot_bottom, map_mode, VSTAB_BLEND_EXACT, dst_y,
                                            pitch_dst_y, dst_uv, pitch_dst_uv, dw, dh, ba.c.w);
    if (st != VSTAB_OK) return st;
    if (resample == VSTAB_RESAMPLE_DEFAULT)
        return fail(VSTAB_ERR_UNSUPPORTED, n + ": VSTAB_RESAMPLE_DEFAULT (the bilinear warp) is served by vstab_warp_p010_planar");
    if (resample != VSTAB_RESAMPLE_CUBIC && resample != VSTAB_RESAMPLE_LANCZOS4)
        return fail(VSTAB_ERR_INVALID, n + ": resample must be VSTAB_RESAMPLE_CUBIC (2) or VSTAB_RESAMPLE_LANCZOS4 (4)");
    if (!border_mode_valid(border_mode))
        return fail(VSTAB_ERR_INVALID, n + ": border_mode must be VSTAB_BORDER_CONSTANT (0), _REPLICATE (1), _REFLECT (2) or _REFLECT_101 (4)");
    ba.c.p32 = map_params32(params);
    fill_rolling_shutter(ba, params, rot_bottom, dh);
    return launch_warp_resample10(ba, map_mode, rot_bottom != nullptr, resample, border_mode, stream);
}

static vstab_status cvt_bgr16_p010(const std::string &n, const void *src_bgr16, size_t pitch_src, int width, int height, void *dst_y, size_t pitch_y, void *dst_uv,
                                   size_t pitch_uv, int matrix, int range, void *stream) {
    if (!src_bgr16 || !dst_y || !dst_uv) return fail(VSTAB_ERR_INVALID, n + ": null pointer");
    if (width <= 0 || height <= 0 || width > 32767 || height > 32767) return fail(VSTAB_ERR_INVALID, n + ": sizes must be in [1, 32767]");
    if (pitch_src < (size_t)width * 6 || pitch_src % 2 || pitch_y < (size_t)width * 2 || pitch_y % 2 || pitch_uv < (size_t)((width + 1) / 2) * 4 || pitch_uv % 4 ||
        !ptr_aligned(src_bgr16, 2) || !ptr_aligned(dst_y, 2) || !ptr_aligned(dst_uv, 4))
        return fail(VSTAB_ERR_INVALID, n + ": bad pitch or alignment (16-bit samples; chroma pairs 4-byte aligned)");
    VSTAB_TRY(check_colour_spec(n.c_str(), matrix, range));
    const dim3 grid(div_up(div_up(width, 2), 64), div_up(height, 4));
    if (colour_spec_default(matrix, range))
        hipLaunchKernelGGL(k_cvt_bgr10_p010, grid, dim3(256), 0, static_cast<hipStream_t>(stream), static_cast<const uint8_t *>(src_bgr16), pitch_src, width, height,
                           static_cast<uint8_t *>(dst_y), pitch_y, static_cast<uint8_t *>(dst_uv), pitch_uv);
    else
        hipLaunchKernelGGL(k_cvt_bgr10_p010_colour, grid, dim3(256), 0, static_cast<hipStream_t>(stream), static_cast<const uint8_t *>(src_bgr16), pitch_src, width,
                           height, static_cast<uint8_t *>(dst_y), pitch_y, static_cast<uint8_t *>(dst_uv), pitch_uv, colour_coefficients10(matrix, range));
    VSTAB_HIP_TRY(hipGetLastError());
    return VSTAB_OK;
}

extern "C" vstab_status vstab_cvt_bgr16_p010(const void *src_bgr16, size_t pitch_src, int width, int height, void *dst_y, size_t pitch_y, void *dst_uv,
                                             size_t pitch_uv, void *stream) {
    return cvt_bgr16_p010("vstab_cvt_bgr16_p010", src_bgr16, pitch_src, width, height, dst_y, pitch_y, dst_uv, pitch_uv, VSTAB_COLOUR_CVTCOLOR, VSTAB_RANGE_LIMITED, stream);
}

extern "C" vstab_status vstab_cvt_bgr16_p010_colour(const void *src_bgr16, size_t pitch_src, int width, int height, void *dst_y, size_t pitch_y, void *dst_uv,
                                                    size_t pitch_uv, int matrix, int range, void *stream) {
    return cvt_bgr16_p010("vstab_cvt_bgr16_p010_colour", src_bgr16, pitch_src, width, height, dst_y, pitch_y, dst_uv, pitch_uv, matrix, range, stream);
}

// The forward conversion as an operator: P010 planes (even width and height) -> 16-bit BGR.  Every spec, the default included, runs the one kernel.
extern "C" vstab_status vstab_cvt_p010_bgr16_colour(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int width, int height, void *dst, size_t pitch_dst,
                                                    int matrix, int range, void *stream) {
    const std::string n = "vstab_cvt_p010_bgr16_colour";
    if (!y || !uv || !dst) return fail(VSTAB_ERR_INVALID, n + ": null pointer");
    if (width < 2 || height < 2 || (width & 1) || (height & 1) || width > 32767 || height > 32767)
        return fail(VSTAB_ERR_INVALID, n + ": sizes must be even and in [2, 32767]");
    if (pitch_y < (size_t)width * 2 || pitch_y % 2 || pitch_uv < (size_t)width * 2 || pitch_uv % 4 || pitch_dst < (size_t)width * 6 || pitch_dst % 2 ||
        !ptr_aligned(y, 2) || !ptr_aligned(uv, 4) || !ptr_aligned(dst, 2))
        return fail(VSTAB_ERR_INVALID, n + ": bad pitch or alignment (16-bit samples; chroma pairs 4-byte aligned)");
    VSTAB_TRY(check_colour_spec(n.c_str(), matrix, range));
    hipLaunchKernelGGL(k_cvt_p010_bgr16_colour, dim3(div_up(width / 2, 64), div_up(height, 4)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const uint8_t *>(y), pitch_y, static_cast<const uint8_t *>(uv), pitch_uv, width, height, static_cast<uint8_t *>(dst), pitch_dst,
                       colour_coefficients10(matrix, range));
    VSTAB_HIP_TRY(hipGetLastError());
    return VSTAB_OK;
}

static vstab_status warp_p010(const char *n, const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int sw, int sh, const float params[17],
                              const float *rot_bottom, int map_mode, int blend, void *dst, size_t pitch_dst, int dw, int dh, int matrix, int range, void *stream) {
    WarpArgs wa;
    const vstab_status st = check_warp_p010(n, P010_BGR16, y, pitch_y, uv, pitch_uv, sw, sh, params, rot_bottom, map_mode, blend, dst, pitch_dst,
                                            nullptr, 0, dw, dh, wa);
    if (st != VSTAB_OK) return st;
    VSTAB_TRY(check_colour_spec(n, matrix, range));
    const bool colour = !colour_spec_default(matrix, range);
    const ColourCoef col = colour_coefficients10(matrix, range);
    // The LDS-tiled kernel (the 8-bit hot kernel's structure with a 10:10:10 LDS pixel) serves the fisheye -> pinhole maps when
    // the planes allow its 16-byte staging loads and 32-bit staged offsets; everything else takes the direct-gather kernel below.  Same results.
    const bool tiled_ok = map_mode_fish_to_pinhole(map_mode) && sw >= 8 && source_16(y, pitch_y, uv, pitch_uv) && staged_offsets32(pitch_y, pitch_uv, sh).chroma;
    static const bool force_direct = getenv("VSTAB_P010_DIRECT") != nullptr;  // development: the direct-gather kernel for every call
    if (tiled_ok && !force_direct)
        return launch_warp_fused10(wa, params, map_mode, blend, rot_bottom, false, true, true, static_cast<hipStream_t>(stream), colour ? &col : nullptr);
    P010Args a;
    a.y = wa.y, a.uv = wa.uv, a.dst = static_cast<uint16_t *>(dst);
    a.pitch_y = pitch_y, a.pitch_uv = pitch_uv, a.pitch_dst = pitch_dst;
    a.sw = sw, a.sh = sh, a.dw = dw, a.dh = dh;
    a.p = wa.p;
    a.rs = rot_bottom != nullptr;
    fill_rolling_shutter(a, params, rot_bottom, dh);
    a.col = col;  // (read by the COLOUR kernels alone)
    const dim3 grid(div_up(dw, 64), div_up(dh, 8));  // 64 columns x 4 pairs of rows per workgroup
    with_map_mode(map_mode, [&](auto mode) {  // (the rotation per row is the kernel's run-time a.rs: no MAP_RS_* forms here)
        with_either<VSTAB_BLEND_FP16, VSTAB_BLEND_EXACT>(blend == VSTAB_BLEND_FP16, [&](auto blend_c) {
            with_bool(colour, [&](auto colour_c) {
                launch_kernel(k_warp_p010<decltype(mode)::value, decltype(blend_c)::value, decltype(colour_c)::value>, grid, dim3(256), 0,
                              static_cast<hipStream_t>(stream), a);
            });
        });
    });
    VSTAB_HIP_TRY(hipGetLastError());
    return VSTAB_OK;
}

extern "C" vstab_status vstab_warp_p010(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int sw, int sh, const float params[17],
                                        const float *rot_bottom, int map_mode, int blend, void *dst, size_t pitch_dst, int dw, int dh, void *stream) {
    return warp_p010("vstab_warp_p010", y, pitch_y, uv, pitch_uv, sw, sh, params, rot_bottom, map_mode, blend, dst, pitch_dst, dw, dh, VSTAB_COLOUR_CVTCOLOR,
                     VSTAB_RANGE_LIMITED, stream);
}

extern "C" vstab_status vstab_warp_p010_colour(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int sw, int sh, const float params[17],
                                               const float *rot_bottom, int map_mode, int blend, void *dst, size_t pitch_dst, int dw, int dh, int matrix, int range,
                                               void *stream) {
    return warp_p010("vstab_warp_p010_colour", y, pitch_y, uv, pitch_uv, sw, sh, params, rot_bottom, map_mode, blend, dst, pitch_dst, dw, dh, matrix, range, stream);
}
