// vstab_lk_window.hpp -- the tracker's device code for ONE window size, as a text: included once per size with VSTAB_LK_W defined (an odd
// window side; vstab.h, "Tracker window").  No include guard.  vstab_lk.hip includes it with 21 and gets k_lk_track and k_lk_track_opt in
// namespace vstab, under the names and with the statements they always had; vstab_lk_win.hip includes it once per further size and gets
// k_lk_track_win in namespace vstab::lkw<W> (the body with OPT = true).  Everything that was a literal 21, 22, 24 or 32 is a constant
// derived from VSTAB_LK_W below, each with the static_assert that makes the derivation safe for that size.
// Why a text and not templates on W: k_lk_track's time is its schedule (the note above the kernels), and "the default tracker is the
// kernel it was" is kept as a property of the build (tools/asm_kernel_diff.py).  With the helpers turned into templates the compiler is
// free to order its inlining differently; with the same tokens it is not.  A further size is one inclusion and one table entry
// (vstab_lk_win.hip).
// The includer provides: <climits>, <cstddef>, vstab_internal.hpp, vstab_track.hpp, vstab_track_device.hpp.
#ifndef VSTAB_LK_W
#error "vstab_lk_window.hpp is included with VSTAB_LK_W defined (vstab_lk.hip, vstab_lk_win.hip)"
#endif
#define VSTAB_LK_CAT2(a, b) a##b
#define VSTAB_LK_CAT(a, b) VSTAB_LK_CAT2(a, b)

namespace vstab {
#if VSTAB_LK_W != 21
namespace VSTAB_LK_CAT(lkw, VSTAB_LK_W) {
#endif

// =============================================================================================
// k_lk_track -- LKTrackerInvoker for all pyramid levels, one wavefront per
// feature.  Window 21x21 = 441 pixels -> 7 per lane.  Per level: the 24x24 neighbourhood of the
// previous image goes to LDS (REFLECT_101 padding), Scharr derivatives are computed on the fly
// for the 22x22 taps (zero outside the image, as the reference's zero-padded derivative buffer),
// the patch (I, Ix, Iy as int16 x32 fixed point) lives in registers, and the Gauss-Newton loop
// stages a 22x22 block of the next image per iteration.  All sums are exact integers reduced
// with wave shuffles (order free), converted once to float; the 2x2 solve follows the reference's
// float operation order.
// =============================================================================================
// (the figures in this file's comments are those of the 21 x 21 window; the geometry of every size: DESIGN.md section 34)
constexpr int lk_roundup4(int n) { return (n + 3) & ~3; }
constexpr int LKW = VSTAB_LK_W, LKT = LKW + 1;       // the window; its tap block (a window pixel interpolates 2 x 2 taps)
constexpr int LKR = lk_roundup4(LKW + 3);            // previous-image neighbourhood: the taps and a Scharr ring (columns past LKW + 3 are loaded, never read)
constexpr int LKJM = 5, LKJR = lk_roundup4(LKT + 2 * LKJM);  // next-image region: 22x22 taps + 5 px of slack each side
static_assert(LKW % 2 == 1 && LKW >= 3 && LKW <= 31, "an odd window; the exact-sum bounds below are worked out up to 31");
static_assert(LKR % 4 == 0 && LKJR % 4 == 0 && LKR >= LKW + 3 && LKJR >= LKT + 2 * LKJM, "LkStage splits rows into dwords");

#define LK_DESCALE(x, n) (((x) + (1 << ((n)-1))) >> (n))
// 2^-l as a float, exactly what (float)(1.0 / (double)(1 << l)) gives -- without a double-precision division in the kernel
__device__ __forceinline__ float lk_level_scale(int l) { return __uint_as_float((uint32_t)(127 - l) << 23); }
// 32-bit integer multiplies run at a quarter of the rate of the 24-bit ones, and every product here has operands well inside 24 bits
// (pixels < 2^8, weights <= 2^14, Scharr derivatives and interpolated patch values < 2^15) and a result inside 32
__device__ __forceinline__ int lk_mul(int a, int b) { return __mul24(a, b); }
// a * b + c with a 24-bit multiply, spelled out: where b is a constant the compiler turns __mul24 back into a full 32-bit multiply
// (it cannot see that the LDS values are small) and the Scharr taps became v_mul_lo_u32 / v_mad_u64_u32 pairs
__device__ __forceinline__ int lk_mad(int a, int b, int c) {
    int d;
    asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
    return d;
}
// e / 22 and k / 21 for the indices of the 22 x 22 tap block and the 21 x 21 window (< 600): one 24-bit multiply and a shift
// instead of the 64-bit multiply-high the compiler emits for a division by a constant
// The constant is ceil(2^16 / d): 2979 and 3121 for 22 and 21; for a tap block of 16 or 32 it is a power of two and the compiler is
// left with the shift.  Checked over the true ranges: a tap index is below LKT^2, a window index below 64 * ceil(LKW^2 / 64) (the last
// lanes' pad pixels are divided too).
constexpr int lk_div_magic(int d) { return (65536 + d - 1) / d; }
static_assert(lk_div_magic(22) == 2979 && lk_div_magic(21) == 3121, "the constants of the 21 x 21 window");
static_assert(div_magic_ok(LKT, lk_div_magic(LKT), LKT * LKT) && div_magic_ok(LKW, lk_div_magic(LKW), (LKW * LKW + 63) / 64 * 64), "division constants");
__device__ __forceinline__ int lk_div_tap(int e) { return __mul24(e, lk_div_magic(LKT)) >> 16; }  // e / LKT
__device__ __forceinline__ int lk_div_win(int k) { return __mul24(k, lk_div_magic(LKW)) >> 16; }  // k / LKW

// k_lk_track: ONE WORKGROUP OF 4 WAVES PER FEATURE.  The tracker is latency bound (<= 200 features, a dependent
// Gauss-Newton chain of up to 4 x 30 iterations per frame pair): a wave alone on its SIMD issues a dependent instruction
// only every ~8 cycles, so what counts is the NUMBER of instructions on the chain, not the arithmetic in them.  Four waves
// stage the image blocks (one memory latency for all of them) and prepare the previous image's side of the four pyramid
// levels, one level per wave; the iterations of a level run on one wave with seven window pixels per lane (see below).
// Integer sums are exact whatever the decomposition: per-lane partials are split into a signed high part and a 16-bit low
// part so that every wave sum stays inside int32; hi * 65536 + lo is exact in double and the one double -> float
// conversion equals (float)(int64 total).
constexpr int LK_THREADS = 256, LK_WAVES = 4;
#ifndef VSTAB_LK_PRIO
#define VSTAB_LK_PRIO 1
#endif
constexpr int LK_WPAD = (LKW * LKW + 63) & ~63;  // window pixels rounded up to whole waves

// The 2 x 2 matrix of a level from the exact sums of Ix Ix, Ix Iy, Iy Iy (as floats): A11, A12, A22, 1 / D and whether the level is
// rejected (minEig < 1e-4 or D < FLT_EPSILON), in the reference's float operation order.  Evaluated by whoever prepared the level --
// for the lower levels a wave in the shadow of the top level's iterations -- so that the square root and the two divisions are not
// on the iterating wave's dependent chain; the same instructions give the same bits wherever they run.
// OPT (k_lk_track_opt; vstab.h, "Tracker options"): the threshold is the launch's (rule 4), and minEig itself leaves through the spare
// slot 5 -- what VSTAB_LK_GET_MIN_EIGENVALS reports (rule 6), rejected or not.
template <bool OPT>
__device__ __forceinline__ void lk_level_matrix(const LkSegArgs &args, float s0, float s1, float s2, float *out) {
    const float FLT_SCALE = 1.0f / (1 << 20);
    const float A11 = s0 * FLT_SCALE, A12 = s1 * FLT_SCALE, A22 = s2 * FLT_SCALE;
    const float D = A11 * A22 - A12 * A12;
    const float minEig = ((A22 + A11) - sqrtf((A11 - A22) * (A11 - A22) + (4.f * A12) * A12)) / (float)(2 * LKW * LKW);
    out[0] = A11, out[1] = A12, out[2] = A22, out[3] = 1.f / D;
    if constexpr (OPT) {
        out[4] = minEig < args.min_eig || D < 1.1920928955078125e-7f ? 1.0f : 0.0f;
        out[5] = minEig;
    } else {
        out[4] = minEig < 1e-4f || D < 1.1920928955078125e-7f ? 1.0f : 0.0f;
    }
}

// Full-wave integer sums by DPP (row_shr 1, 2, 4, 8, then row_bcast 15 / 31); the totals are read from lane 63 and broadcast through
// SGPRs.  Integer addition is associative, so the order is free.  The N wave reductions advance in lockstep: every DPP step is applied to all of them before the next one, so the
// two wait states a DPP read needs behind the write of its source are filled by the other chains instead of s_nop
// (written one chain after the other, the compiler serialised the first pair: 12 steps with a nop each).
template <int N>
__device__ __forceinline__ void wave_sums_i32(int (&t)[N]) {
#define VSTAB_DPP_STEP(ctrl, rows)                                                          \
    _Pragma("unroll") for (int i = 0; i < N; i++) t[i] += __builtin_amdgcn_update_dpp(0, t[i], ctrl, rows, 0xf, false)
    VSTAB_DPP_STEP(0x111, 0xf);
    VSTAB_DPP_STEP(0x112, 0xf);
    VSTAB_DPP_STEP(0x114, 0xf);
    VSTAB_DPP_STEP(0x118, 0xf);
    VSTAB_DPP_STEP(0x142, 0xa);
    VSTAB_DPP_STEP(0x143, 0xc);
#undef VSTAB_DPP_STEP
#pragma unroll
    for (int i = 0; i < N; i++) t[i] = __builtin_amdgcn_readlane(t[i], 63);
}

// Staging in two phases -- every global load of a block is issued before the first LDS store waits for one -- so
// a block costs ONE memory latency instead of one per loop trip.  The tracker is a dependent chain at one
// workgroup per CU: exposed latency is what it is made of (measured: staging was half of a workgroup's time).
template <int SIDE, int THREADS = LK_THREADS>
struct LkStage {
    // SIDE x SIDE bytes as SIDE * SIDE / 4 dwords: a thread fetches FOUR consecutive pixels of a row with one (unaligned)
    // dword load and writes them to LDS as four ints with one 16-byte store -- a quarter of the loads, index arithmetic and LDS
    // stores of the byte-by-byte form it replaces (which is kept for blocks that touch the image border: REFLECT_101 per byte).
    static_assert(SIDE % 4 == 0, "rows are split into dwords");
    static constexpr int ROWW = SIDE / 4, NW = SIDE * ROWW, N = (NW + THREADS - 1) / THREADS;
    uint32_t v[N];
    __device__ __forceinline__ void load(const uint8_t *img, uint32_t pitch, int w, int h, int x0, int y0, int tid) {
        const bool interior = x0 >= 0 && y0 >= 0 && x0 + SIDE <= w && y0 + SIDE <= h;  // uniform
#pragma unroll
        for (int k = 0; k < N; k++) {
            const int e = tid + THREADS * k;
            v[k] = 0;
            if (e < NW) {
                const int ry = e / ROWW, rx = 4 * (e - ry * ROWW);
                if (interior) {
                    // (row * pitch with the 24-bit multiplier: rows < 2^15, pitches < 2^24 -- launch_lk checks -- and planes < 4 GiB)
                    __builtin_memcpy(&v[k], img + __umul24((uint32_t)(y0 + ry), pitch) + (uint32_t)(x0 + rx), 4);  // one global_load_dword (any alignment)
                } else {
                    const uint8_t *row = img + __umul24((uint32_t)reflect101(y0 + ry, h), pitch);
                    v[k] = (uint32_t)row[reflect101(x0 + rx, w)] | ((uint32_t)row[reflect101(x0 + rx + 1, w)] << 8) |
                           ((uint32_t)row[reflect101(x0 + rx + 2, w)] << 16) | ((uint32_t)row[reflect101(x0 + rx + 3, w)] << 24);
                }
            }
        }
    }
    // a block that lies inside the image (the caller checked): no border handling, a handful of instructions per dword
    __device__ __forceinline__ void load_interior(const uint8_t *img, uint32_t pitch, int x0, int y0, int tid) {
#pragma unroll
        for (int k = 0; k < N; k++) {
            const int e = min(tid + THREADS * k, NW - 1);  // (a thread past the end loads the last dword again and never stores it)
            const int ry = e / ROWW, rx = 4 * (e - ry * ROWW);
            __builtin_memcpy(&v[k], img + __umul24((uint32_t)(y0 + ry), pitch) + (uint32_t)(x0 + rx), 4);
        }
    }
    // the OUT x OUT window of the block whose corner sits at (dx, dy) of it, as a row-major OUT x OUT int array (the window's place in the
    // block is only known after the block was fetched: the previous-image neighbourhoods fetched ahead, k_lk_track)
    template <int OUT>
    __device__ __forceinline__ void store_window(int *dst, int tid, int dx, int dy) const {
#pragma unroll
        for (int k = 0; k < N; k++) {
            const int e = tid + THREADS * k;
            const int ry = e / ROWW, rx = 4 * (e - ry * ROWW);
            const int Y = ry - dy, X = rx - dx;
            if (e < NW && (unsigned)Y < (unsigned)OUT) {
                int *o = dst + lk_mul(Y, OUT) + X;
#pragma unroll
                for (int i = 0; i < 4; i++)
                    if ((unsigned)(X + i) < (unsigned)OUT) o[i] = (int)((v[k] >> (8 * i)) & 255u);
            }
        }
    }
    __device__ __forceinline__ void store(int *dst, int tid) const {  // dst 16-byte aligned
#pragma unroll
        for (int k = 0; k < N; k++) {
            const int e = tid + THREADS * k;
            if (e < NW) *reinterpret_cast<int4 *>(dst + 4 * e) = make_int4((int)(v[k] & 255u), (int)((v[k] >> 8) & 255u), (int)((v[k] >> 16) & 255u), (int)(v[k] >> 24));
        }
    }
};

// A result record for the polling host thread (Tracker::track_wait) and for the chained launch of the next frame: two
// naturally aligned 8-byte granules {x, seq} and {y, seq << 2 | status}, each validated by its own tag, written by one
// 16-byte store to fine-grained host memory.  Nothing in HIP or PCIe promises that a 16-byte store arrives as one
// indivisible write, so the reader checks the tag of each half: a torn record cannot pair a new tag with stale data
// (aligned 8-byte granules written by one store are the hand-off unit of /opt/skills/guides/MI355X_MICROARCH.md,
// "handoff-1to1").  No fence and no wait: a system-scope release would write back the XCD's whole L2 200 times per
// frame under the warp kernel that merges partial output lines there (warp beside the tracker 72 us against 52), and
// four ordered stores with a wait for their acknowledgement cost the tracker chain a third of the pipeline's rate.
__device__ __forceinline__ uint4 make_record(float x, float y, unsigned int status, unsigned int seq) {
    return make_uint4(__float_as_uint(x), seq, __float_as_uint(y), (seq << 2) | status);
}
__device__ __forceinline__ unsigned int record_status(const uint4 &r) { return r.w & 3u; }

// The device copy of a record is what the NEXT launch starts from, slot by slot.  A chained launch sits on the SAME stream
// behind its parent, so the record is complete when the child starts: a plain 16-byte store here, a plain load there, and the
// child checks the tag (a mismatch means the host chained the wrong buffers: reported as status 3, never tracked from).
// Slot f's record of frame pair i goes to the copies the launch asked for: coherent host memory the host polls (host_rec), device
// memory for the launch chained behind this one (dev_rec).
__device__ __forceinline__ void lk_write_record(const LkSegArgs &args, int i, int f, const uint4 &rec) {
    if (args.dev_rec[i]) args.dev_rec[i][f] = rec;
    if (args.host_rec[i]) args.host_rec[i][f] = rec;
}
// the rest of the segment is dead: pairs first .. n_frames - 1 of slot f report `status` (2 "lost earlier", 3 bookkeeping error) and no point
__device__ __forceinline__ void lk_write_dead(const LkSegArgs &args, int first, int f, unsigned int status) {
    for (int i = first; i < args.n_frames; i++) lk_write_record(args, i, f, make_record(0.0f, 0.0f, status, args.seq[i]));
}

// who a thread is: its feature slot, its index in the workgroup, its lane and its wave
// (wave as a scalar: what is indexed with it -- the pyramid level a wave prepares -- is then read with scalar loads from the
// kernel arguments instead of per-lane global loads, each of which was a memory latency inside the dependent chain)
struct LkThread {
    int f, tid, lane, wave;
};

#undef LK_STAMP
#undef LK_NOW
#if defined(VSTAB_DEV) && VSTAB_LK_W == 21
// development builds (the 21 x 21 kernels only: the stamps have one buffer and one extern "C" setter): sixteen 100 MHz wall-clock stamps per feature and launch (tools/lk_timeline.py):
// [0] entry, [1] start point known, [2] blocks staged, then per level (3 -> 0): [3 + 3 i] derivatives + patch matrix done,
// [4 + 3 i] iterations done, [5 + 3 i] iteration count; [15] end
// (LK_STAMP reads the LkThread `t` and the sequence number `seq` of the scope it stands in)
__device__ unsigned long long *g_lk_timing = nullptr;
extern "C" __attribute__((visibility("default"))) void vstab_dev_set_lk_timing(void *p) {
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_lk_timing), &p, sizeof(p));
}
#define LK_STAMP(k, v) \
    if (g_lk_timing && t.tid == 0) g_lk_timing[(((size_t)(seq & 63u) * 256 + (size_t)t.f) << 5) + (k)] = (v)
#define LK_NOW() __builtin_amdgcn_s_memrealtime()
#else
#define LK_STAMP(k, v)
#define LK_NOW() 0ull
#endif

// The workgroup's LDS state, declared once in the kernel.  regI and regJ are 16-byte aligned (LkStage::store writes int4): the kernel
// aligns the struct, and the offsets are checked below.  The small arrays are ordered so that each keeps the alignment of its own size
// (their pairs and quads are read and written with one LDS operation); the 12 bytes of s_result come last.
struct LkShared {
    int regJ[2][LKJR * LKJR];                     // next-image blocks: one for the level that runs, one for the level staged behind it
    int regI[LK_MAX_LEVELS][LKR * LKR];           // the 24 x 24 previous-image neighbourhood of every level
    uint32_t dpk[LK_MAX_LEVELS][LKT * LKT];       // Scharr derivative pairs of the 22 x 22 taps: dx | dy << 16 (int16 each)
    short patch_i[LK_MAX_LEVELS][LK_WPAD];        // the interpolated window of every level: I ...
    uint32_t patch_xy[LK_MAX_LEVELS][LK_WPAD];    // ... and Ix | Iy << 16 (int16 each), as the iterations hold them in registers
    float level_mat[LK_MAX_LEVELS][8];            // A11, A12, A22, 1 / D of the level's 2 x 2 matrix, its rejection flag and (k_lk_track_opt) minEig (lk_level_matrix)
    int s_pf[LK_MAX_LEVELS][4];                   // origins of the blocks fetched ahead: neighbourhood x, y, next-image block x, y (PF_NONE: no block)
    int s_top[LK_WAVES][6];                       // the waves' shares of the top level's matrix sums
    float s_est[2][2];                            // wave 0 -> all, by level parity: where the feature stands in the next image after that level
    int s_jorg[2][2];                             // waves 1 - 3 -> wave 0, by buffer: origin of the next-image block staged for the coming level
    float s_result[3];                            // wave 0 -> all: the point the frame pair ended on and its status
};
static_assert(offsetof(LkShared, regI) % 16 == 0 && offsetof(LkShared, regJ) % 16 == 0, "LkStage::store writes int4");
static_assert(LKW != 21 || sizeof(LkShared) == 36236, "the LDS footprint of k_lk_track");
// 15: 23244 bytes; 31: 77516 bytes -- above the 64 KiB a workgroup had before gfx950, inside the 160 KiB of a gfx950 CU (two workgroups fit)
static_assert(sizeof(LkShared) <= 80 * 1024, "two workgroups a CU");
static_assert(LK_MAX_LEVELS <= LK_WAVES, "wave 0 iterates, waves 1 .. prepare one lower level each");

constexpr float LK_HALF = (LKW - 1) * 0.5f;
constexpr int PF_NONE = INT_MIN / 2;         // "no block" as an origin
constexpr int PF_SLACK = (LKJR - LKR) / 2;   // a neighbourhood fetched ahead: 4 pixels of slack each side

// the bilinear weights of the fractional position (a, b), 14-bit fixed point, summing to 2^14
__device__ __forceinline__ void lk_bilinear_weights(float a, float b, int &w00, int &w01, int &w10, int &w11) {
    w00 = (int)rintf((1.f - a) * (1.f - b) * 16384.f);
    w01 = (int)rintf(a * (1.f - b) * 16384.f);
    w10 = (int)rintf((1.f - a) * b * 16384.f);
    w11 = 16384 - w00 - w01 - w10;
}
// The range test of a window origin floor(q) against [-LKW, w) x [-LKW, h), on the floats themselves: floor(q) >= -LKW iff q >= -LKW and
// floor(q) < w iff q < w (both bounds are integers a float holds exactly), so every finite q decides as the reference's integer test
// does.  A NaN fails it, as it fails the reference's -- whose conversion turns NaN and everything outside int into INT_MIN; the
// conversion here turns NaN into 0, which the integer test would take for a window at the image's corner.
__device__ __forceinline__ bool lk_origin_in_range(float qx, float qy, int w, int h) {
    return qx >= -(float)LKW && qx < (float)w && qy >= -(float)LKW && qy < (float)h;
}
// Where the window of a point sits in level l (w x h) of the previous image: its top-left pixel floor(p 2^-l - half), whether the level
// is tracked at all (the origin lies in [-LKW, w) x [-LKW, h): the staging, the preparation and the level loop all skip it otherwise;
// never for a NaN or infinite coordinate), and the weights of the four taps of a window pixel.
struct LkLevelGeom {
    int ipx, ipy, iw00, iw01, iw10, iw11;
    bool ok;
};
__device__ __forceinline__ LkLevelGeom lk_level_geom(float2 p, int l, int w, int h) {
    const float ls = lk_level_scale(l);
    float qx = p.x * ls, qy = p.y * ls;
    qx -= LK_HALF, qy -= LK_HALF;
    LkLevelGeom g;
    g.ipx = (int)floorf(qx), g.ipy = (int)floorf(qy);
    g.ok = lk_origin_in_range(qx, qy, w, h);
    lk_bilinear_weights(qx - (float)g.ipx, qy - (float)g.ipy, g.iw00, g.iw01, g.iw10, g.iw11);
    return g;
}

// exact totals: the signed high parts and the 16-bit low parts of the per-lane partials are summed separately (each stays inside
// int32); hi * 65536 + lo is exact in double and the one double -> float conversion equals (float)(int64 total)
__device__ __forceinline__ float lk_exact_total(int hi, int lo) { return (float)__builtin_fma((double)hi, 65536.0, (double)lo); }

// Whether a block of side LKJR at origin floor(c) - margin may be fetched ahead of the moment its centre is known for certain: c lies
// where a window origin may lie (false for NaN: a diverged estimate is not chased) and -- `inside`: for the blocks that are loaded
// without border handling -- the block lies inside the w x h image (a block across the image border is left to the pair's own
// staging).  The origin comes back as scalars.
__device__ __forceinline__ bool lk_block_origin(float cx, float cy, int margin, int w, int h, bool inside, int &ox, int &oy) {
    if (!(cx > -(float)(LKW + 1) && cx < (float)w && cy > -(float)(LKW + 1) && cy < (float)h)) return false;
    ox = __builtin_amdgcn_readfirstlane((int)floorf(cx)) - margin, oy = __builtin_amdgcn_readfirstlane((int)floorf(cy)) - margin;
    return !inside || (ox >= 0 && oy >= 0 && ox + LKJR <= w && oy + LKJR <= h);
}

// ---- start point of the slot: the host's point list, or the record the parent launch left for it -------------------------------------
// false: the slot has nothing to track, and every pair of the segment has its dead record.
__device__ __forceinline__ bool lk_start_point(const LkSegArgs &args, const LkThread &t, float2 &pp) {
    if (!args.chain_in) {
        pp = args.prev_pts[t.f];
        return true;
    }
    // chained launch: this slot's input is the record the parent launch wrote for it in its LAST frame pair -- the point it
    // tracked to, if it survived (status 1).  Slots that were lost earlier stay lost (status 2) and are skipped by the
    // host, which is exactly the status filter of FrameSourceWarp.cpp:261-268.
    const uint4 r = args.chain_in[t.f];
    const bool tagged = r.y == args.parent_seq && (r.w >> 2) == (args.parent_seq & 0x3fffffffu);
    if (!tagged || record_status(r) != 1u) {  // uniform for the workgroup
        if (t.tid == 0) lk_write_dead(args, 0, t.f, tagged && record_status(r) != 3u ? 2u : 3u);
        return false;
    }
    pp = make_float2(__uint_as_float(r.x), __uint_as_float(r.z));
    return true;
}

// The Gauss-Newton iterations of a level run on ONE wave (wave 0), seven window pixels per lane: k = lane + 64 m (441 pixels;
// the last 7 lanes have six).  With the window spread over four waves (two pixels per lane) an iteration was ~300 instructions of
// splitting, reducing, exchanging through LDS and a barrier around eight tap reads -- and a wave alone on its SIMD issues a
// dependent instruction every ~8 cycles whatever it does (the measured 0.8 - 1.1 us per iteration).  Seven independent pixels per
// lane pipeline at the issue rate, one DPP reduction gives the total, nothing is exchanged and nobody waits at a barrier; the
// other three waves stage the next level's block and sleep at the level's barrier.  The sums are exact integers either way.
constexpr int LK_PPL = (LKW * LKW + 63) / 64;  // 7 (15: 4, 31: 16)
// The exact sums, for every window this file is included with.  |Ix|, |Iy| <= 4080 (Scharr of bytes, x32 / 2^5 after the interpolation),
// |diff| <= 8160 (bytes x32, one against another; bounded below with twice that, as the 21 x 21 kernel always was).  A lane's partial holds at most LK_PPL pixels on the
// single-wave paths (fewer where four waves share the window) and must stay inside int32; it is then split into a signed high part
// (< 2^15) and a 16-bit low part, and 256 lanes' worth of either stays inside int32 with room to spare.  The residual's total is an
// integer below 2^24: exact as a float.
static_assert((long long)LK_PPL * 4080 * 4080 < (1ll << 31) && (long long)LK_PPL * 16320 * 4080 < (1ll << 31), "per-lane partial sums");
static_assert(256ll * 65535 < (1ll << 31) && 256ll * (1ll << 15) < (1ll << 31), "wave totals of the hi and lo parts");
static_assert((long long)LKW * LKW * 8160 < (1ll << 24), "the residual is exact as a float");
// offset of window pixel k inside a staged next-image block (a pixel the lane does not have: 0, with a zero patch)
__device__ __forceinline__ void lk_window_offsets(int (&koff)[LK_PPL], int lane) {
#pragma unroll
    for (int m = 0; m < LK_PPL; m++) {
        const int k = lane + 64 * m;
        const int wy = lk_div_win(k), wx = k - lk_mul(wy, LKW);
        koff[m] = k < LKW * LKW ? lk_mul(wy, LKJR) + wx : 0;
    }
}

// Fetched AHEAD, during the last level of a frame pair, for the NEXT pair of the segment -- by waves 1 - 3, in the shadow of wave 0's
// iterations; the dwords wait in registers: (a) the previous-image neighbourhoods of all levels -- blocks of the current next image
// around where the feature stands now, wide enough (32 x 32 for a 24 x 24 neighbourhood) to hold the neighbourhood of the point the
// pair finally ends on: the top level's by the three waves together (it is needed first), every lower level's by the wave that will
// prepare that level (it alone writes the neighbourhood to LDS, right before it reads it) -- and (b) the TOP level's next-image
// block around the position PREDICTED there: this pair's end plus this pair's motion.  Without them a pair began with one exposed
// memory latency (2.2 - 2.9 of a feature's 18 us in the 4K pipeline).  A block that turns out not to hold what is needed -- the
// motion changed by more than the slack, or the block would cross the image border (blocks fetched ahead are loaded without border
// handling) -- is fetched as before.  Where a block sits never changes a value: it holds image bytes either way.  The origins
// travel through LDS (s_pf), so that wave 0 spends no instruction on any of it.  (The lower levels' next-image blocks fetched ahead
// the same way were measured and dropped: the fetch one level ahead already hides their latency, and a predicted block is left by
// the Gauss-Newton window more often than one centred on the running estimate.)
struct LkAhead {
    LkStage<LKJR, LK_THREADS - 64> It, Jt;  // the top level's neighbourhood and next-image block: waves 1 - 3 together
    LkStage<LKJR, 64> Io;                   // the neighbourhood of the lower level this wave prepares
};

// ---- staging at the start of a pair ----------------------------------------------------------------------------------------------------
// What was not fetched ahead (the first pair of a launch; a block that does not hold what is needed) is loaded now, in one
// exposed latency: the previous-image neighbourhood of EVERY level (it depends on the feature position only) and the top
// level's next-image block.  The block of each lower level is fetched one level ahead, while the level above computes, around
// the position the feature is expected at; if the Gauss-Newton window ends up outside it, the block is staged again around
// the window.
//   jorg_x, jorg_y  origin of the block in regJ[0], staged for the top level (PF_NONE: the top level is not tracked)
//   own_dx, own_dy  waves 1 - 3: the neighbourhood of the level this wave prepares lies in pf.Io, at this offset (-1: it is in regI)
// Returns what was served from the blocks fetched ahead (bit 0: the top neighbourhood, bit 1: the top next-image block; LK_STAMP 17).
// OPT with VSTAB_LK_USE_INITIAL_FLOW: the top level's search starts at the caller's guess gp (level-0 pixels), so its next-image block
// is staged around the guess.  A guess is any float.  The previous point passed the range test before anything of it became an address
// (g.ok); the guess has to pass one too: lk_block_origin lets only a window corner in (-22, w) x (-22, h) through -- never a NaN or an
// infinity, which fail every comparison, and never a value whose floor would leave int -- so the block's origin lies in [-27, w - 6] x
// [-27, h - 6] and LkStage::load's REFLECT_101 folds every tap into the image (it folds any overshoot; here at most 27 pixels).  A
// refused guess stages nothing and leaves PF_NONE: the first iteration refuses the same estimate with its own, narrower range test
// ([-21, w) x [-21, h)) before it looks at the block, so an estimate it accepts always has its block; and were the origin PF_NONE all
// the same, "window outside the block" holds for it and the loop stages afresh around the window it has just range-tested.
template <bool OPT>
__device__ __forceinline__ int lk_stage_pair(LkShared &sh, const LkSegArgs &args, const LkPyramid &I, const LkPyramid &J, float2 pp, float2 gp, int fi, int max_level,
                                             const LkThread &t, const LkAhead &pf, int &jorg_x, int &jorg_y, int &own_dx, int &own_dy) {
    const int tid = t.tid, wave = t.wave;
    LkStage<LKR> si[LK_MAX_LEVELS];
    LkStage<LKJR> sj;
    bool iok[LK_MAX_LEVELS];  // the level's neighbourhood is loaded now
    int top_dx = -1, top_dy = -1;
    bool top_ahead = false;
#pragma unroll
    for (int l = 0; l < LK_MAX_LEVELS; l++) {
        iok[l] = false;
        if (l > max_level) continue;
        int ax = PF_NONE, ay = PF_NONE;
        if (fi) ax = __builtin_amdgcn_readfirstlane(sh.s_pf[l][0]), ay = __builtin_amdgcn_readfirstlane(sh.s_pf[l][1]);  // (published by the previous pair's last level)
        const LkLevelGeom g = lk_level_geom(pp, l, I.w[l], I.h[l]);
        if (!g.ok) continue;
        const int dx = g.ipx - 1 - ax, dy = g.ipy - 1 - ay;  // (huge without a block)
        if ((unsigned)dx <= (unsigned)(2 * PF_SLACK) && (unsigned)dy <= (unsigned)(2 * PF_SLACK)) {
            if (l == max_level) top_dx = dx, top_dy = dy;
            else if (l == max_level - wave) own_dx = dx, own_dy = dy;
        } else {
            iok[l] = true;
            si[l].load(I.img[l], (uint32_t)I.pitch[l], I.w[l], I.h[l], g.ipx - 1, g.ipy - 1, tid);
        }
        bool guessed = false;
        if constexpr (OPT) guessed = (args.flags & VSTAB_LK_USE_INITIAL_FLOW) != 0;  // uniform
        if (l == max_level && guessed) {  // the top level starts at the caller's guess (see above): range test, then the load
            const float ls = lk_level_scale(l);
            int ox = PF_NONE, oy = PF_NONE;
            if (lk_block_origin(gp.x * ls - LK_HALF, gp.y * ls - LK_HALF, LKJM, I.w[l], I.h[l], false, ox, oy)) {
                jorg_x = ox, jorg_y = oy;
                sj.load(J.img[l], (uint32_t)J.pitch[l], I.w[l], I.h[l], jorg_x, jorg_y, tid);
            }
        } else if (l == max_level) {  // the top level starts at the feature position itself
            int bx = PF_NONE, by = PF_NONE;
            if (fi) bx = __builtin_amdgcn_readfirstlane(sh.s_pf[l][2]), by = __builtin_amdgcn_readfirstlane(sh.s_pf[l][3]);
            if (g.ipx - 2 >= bx && g.ipy - 2 >= by && g.ipx + LKT + 2 <= bx + LKJR && g.ipy + LKT + 2 <= by + LKJR) {
                jorg_x = bx, jorg_y = by, top_ahead = true;
            } else {
                jorg_x = g.ipx - LKJM, jorg_y = g.ipy - LKJM;
                sj.load(J.img[l], (uint32_t)J.pitch[l], I.w[l], I.h[l], jorg_x, jorg_y, tid);
            }
        }
    }
#pragma unroll
    for (int l = 0; l < LK_MAX_LEVELS; l++)
        if (iok[l]) si[l].store(sh.regI[l], tid);
    if (top_ahead && wave != 0) pf.Jt.store(sh.regJ[0], tid - 64);
    if (top_dx >= 0 && wave != 0) pf.It.store_window<LKR>(sh.regI[max_level], tid - 64, top_dx, top_dy);
    if (jorg_x != PF_NONE && !top_ahead) sj.store(sh.regJ[0], tid);
    return (top_dx >= 0 ? 1 : 0) | (top_ahead ? 2 : 0);
}

// ---- the previous image's side of a level: derivatives, interpolated window (I, Ix, Iy), sums of the 2 x 2 matrix ----------------------
// They depend on the feature's position in the previous image only -- not on anything the Gauss-Newton iterations produce.
// Scharr derivative pairs of taps e = first, first + stride, ... of level l's 22 x 22 tap block (zero outside the w x h image)
__device__ __forceinline__ void lk_level_derivatives(LkShared &sh, int l, const LkLevelGeom &g, int w, int h, int first, int stride) {
    const int *rI = sh.regI[l];
    for (int e = first; e < LKT * LKT; e += stride) {
        const int tyy = lk_div_tap(e), txx = e - lk_mul(tyy, LKT);
        const int X = g.ipx + txx, Y = g.ipy + tyy;
        int dx = 0, dy = 0;
        if (X >= 0 && Y >= 0 && X < w && Y < h) {
            const int *c = &rI[lk_mul(tyy + 1, LKR) + (txx + 1)];
            const int t0m = lk_mad(c[-1], 10, lk_mad(c[-LKR - 1] + c[LKR - 1], 3, 0)), t0p = lk_mad(c[1], 10, lk_mad(c[-LKR + 1] + c[LKR + 1], 3, 0));
            const int t1m = c[LKR - 1] - c[-LKR - 1], t1c = c[LKR] - c[-LKR], t1p = c[LKR + 1] - c[-LKR + 1];
            dx = (short)(t0p - t0m), dy = (short)lk_mad(t1c, 10, lk_mad(t1p + t1m, 3, 0));
        }
        sh.dpk[l][e] = ((uint32_t)dx & 0xffffu) | ((uint32_t)dy << 16);
    }
}
// window pixels k = first, first + stride, ... of level l -> patch[l]; this lane's share of the matrix sums -> t (hi / lo parts)
__device__ __forceinline__ void lk_level_window(LkShared &sh, int l, const LkLevelGeom &g, int first, int stride, int (&t)[6]) {
    const int *rI = sh.regI[l];
    int pA[3] = {0, 0, 0};  // per-lane partial sums: 7 * 4080^2 < 2^27
    for (int k = first; k < LKW * LKW; k += stride) {
        const int wy = lk_div_win(k), wx = k - lk_mul(wy, LKW);
        const int *c = &rI[lk_mul(wy + 1, LKR) + (wx + 1)];
        const int ival = LK_DESCALE(lk_mul(c[0], g.iw00) + lk_mul(c[1], g.iw01) + lk_mul(c[LKR], g.iw10) + lk_mul(c[LKR + 1], g.iw11), 9);
        const uint32_t *d = &sh.dpk[l][lk_mul(wy, LKT) + wx];
        const uint32_t d00 = d[0], d01 = d[1], d10 = d[LKT], d11 = d[LKT + 1];
        const int ixval = LK_DESCALE(lk_mul((int)(short)(d00 & 0xffffu), g.iw00) + lk_mul((int)(short)(d01 & 0xffffu), g.iw01) +
                                         lk_mul((int)(short)(d10 & 0xffffu), g.iw10) + lk_mul((int)(short)(d11 & 0xffffu), g.iw11), 14);
        const int iyval = LK_DESCALE(lk_mul((int)d00 >> 16, g.iw00) + lk_mul((int)d01 >> 16, g.iw01) + lk_mul((int)d10 >> 16, g.iw10) +
                                         lk_mul((int)d11 >> 16, g.iw11), 14);
        sh.patch_i[l][k] = (short)ival, sh.patch_xy[l][k] = ((uint32_t)ixval & 0xffffu) | ((uint32_t)iyval << 16);
        pA[0] += lk_mul(ixval, ixval), pA[1] += lk_mul(ixval, iyval), pA[2] += lk_mul(iyval, iyval);
    }
#pragma unroll
    for (int q = 0; q < 3; q++) t[2 * q] = pA[q] >> 16, t[2 * q + 1] = pA[q] & 0xffff;
    wave_sums_i32(t);  // uniform; hi * 65536 + lo is the exact total of this wave's pixels
}

// ---- top-level preparation by all four waves -------------------------------------------------------------------------------------------
// The TOP level is needed first: all four waves prepare it together (two derivative taps and two window pixels per lane, the
// matrix sums joined through LDS), which takes a quarter of the time one wave needs for a level.  Then wave 0 starts iterating
// on it while waves 1 .. 3 prepare the lower levels, one level each, in its shadow (lk_prepare_lower_level) -- before,
// every level was prepared up front, one wave per level, and the top level's iterations waited for all of them (3.8 of a
// feature's ~19 us).  The sums are exact integers whatever the decomposition, so every float derived from them is unchanged.
template <bool OPT>
__device__ __forceinline__ void lk_prepare_top_level(LkShared &sh, const LkSegArgs &args, const LkPyramid &I, float2 pp, int max_level, const LkThread &t) {
    const LkLevelGeom gt = lk_level_geom(pp, max_level, I.w[max_level], I.h[max_level]);
    const bool ok = max_level >= 0 && gt.ok;
    __syncthreads();  // the staged neighbourhoods are visible
    if (ok) lk_level_derivatives(sh, max_level, gt, I.w[max_level], I.h[max_level], t.tid, LK_THREADS);
    __syncthreads();  // the top level's derivative pairs are visible to every wave
    int s[6] = {0, 0, 0, 0, 0, 0};
    if (ok) lk_level_window(sh, max_level, gt, t.tid, LK_THREADS, s);
    if (t.lane == 0) {
#pragma unroll
        for (int i = 0; i < 6; i++) sh.s_top[t.wave][i] = s[i];
    }
    __syncthreads();  // the top level's window and sums, the block staged for it: wave 0 can start iterating
    if (t.tid == 0) {
        float sums[3];
#pragma unroll
        for (int q = 0; q < 3; q++) {
            int hi = 0, lo = 0;
#pragma unroll
            for (int wv = 0; wv < LK_WAVES; wv++) hi += sh.s_top[wv][2 * q], lo += sh.s_top[wv][2 * q + 1];
            sums[q] = lk_exact_total(hi, lo);
        }
        lk_level_matrix<OPT>(args, sums[0], sums[1], sums[2], sh.level_mat[max_level]);  // (read back by this wave only)
    }
}

// ---- waves 1 - 3: everything around the iterations, so that the iterating wave spends no instruction on it and never waits
// for global memory -------------------------------------------------------------------------------------------------------------------
// The next (finer) level's next-image block; it lands while this level iterates.  It is centred on where the feature is
// EXPECTED there -- the estimate this level starts from, doubled -- not on the zero-flow position: with the block around the
// previous frame's position a frame-to-frame motion of more than LKJM pixels at that level (the 4K bench clip moves 4 - 12)
// meant staging the block again inside the iteration loop, a global-memory latency on the dependent chain.  A window that leaves
// its block is staged afresh by wave 0.  Loads only: the caller stores the block (sn, origin nx0, ny0) behind its other work.
// gp: where the top level's search started, in level-0 pixels -- the previous point pp or, k_lk_track_opt with VSTAB_LK_USE_INITIAL_FLOW, the
// caller's guess (any float: lk_block_origin's range test stands before the load here too, see lk_stage_pair).
__device__ __forceinline__ void lk_fetch_finer_block(LkShared &sh, const LkPyramid &I, const LkPyramid &J, float2 gp, int level, int max_level, float lscale, int jb,
                                                     const LkThread &t, LkStage<LKJR, LK_THREADS - 64> &sn, int &nx0, int &ny0) {
    const int w1 = I.w[level - 1], h1 = I.h[level - 1];
    const float ex = level == max_level ? gp.x * lscale : sh.s_est[(level + 1) & 1][0] * 2.0f, ey = level == max_level ? gp.y * lscale : sh.s_est[(level + 1) & 1][1] * 2.0f;
    if (lk_block_origin(ex * 2.0f - LK_HALF, ey * 2.0f - LK_HALF, LKJM, w1, h1, false, nx0, ny0))
        sn.load(J.img[level - 1], (uint32_t)J.pitch[level - 1], w1, h1, nx0, ny0, t.tid - 64);  // (else nx0, ny0 stay PF_NONE)
    if (t.tid == 64) sh.s_jorg[jb ^ 1][0] = nx0, sh.s_jorg[jb ^ 1][1] = ny0;
}
// The last level of the pair: fetch ahead for the next pair (LkAhead).  Where the feature stands now: level 1's result, doubled; its
// motion in this pair: that minus the pair's start point.
__device__ __forceinline__ void lk_fetch_ahead(LkShared &sh, const LkSegArgs &args, const LkPyramid &I, const LkPyramid &J, int fi, float2 pp, int max_level,
                                               const LkThread &t, LkAhead &pf) {
    const bool ahead = fi + 1 < args.n_frames && max_level >= 1;  // uniform
    const LkPyramid &J2 = args.pyr[ahead ? fi + 2 : fi + 1];
    const float e0x = sh.s_est[1][0] * 2.0f, e0y = sh.s_est[1][1] * 2.0f;
    const float p0x = e0x + (e0x - pp.x), p0y = e0y + (e0y - pp.y);
    int oix[LK_MAX_LEVELS], oiy[LK_MAX_LEVELS], ojx[LK_MAX_LEVELS], ojy[LK_MAX_LEVELS];
#pragma unroll
    for (int l = LK_MAX_LEVELS - 1; l >= 0; l--) {  // needed first: the neighbourhoods in what is now the next image, top level first
        oix[l] = oiy[l] = PF_NONE;
        if (!ahead || l > max_level) continue;
        const float ls = lk_level_scale(l);
        int ox, oy;
        if (lk_block_origin(e0x * ls - LK_HALF, e0y * ls - LK_HALF, 1 + PF_SLACK, I.w[l], I.h[l], true, ox, oy)) {
            oix[l] = ox, oiy[l] = oy;
            if (l == max_level) pf.It.load_interior(J.img[l], (uint32_t)J.pitch[l], ox, oy, t.tid - 64);
            else if (l == max_level - t.wave) pf.Io.load_interior(J.img[l], (uint32_t)J.pitch[l], ox, oy, t.lane);
        }
    }
#pragma unroll
    for (int l = 0; l < LK_MAX_LEVELS; l++) ojx[l] = ojy[l] = PF_NONE;
    if (ahead) {  // then the top-level block of the image after it, around the predicted position
        const float ls = lk_level_scale(max_level);
        int ox, oy;
        if (lk_block_origin(p0x * ls - LK_HALF, p0y * ls - LK_HALF, LKJM, I.w[max_level], I.h[max_level], true, ox, oy)) {
#pragma unroll
            for (int l = 0; l < LK_MAX_LEVELS; l++)
                if (l == max_level) ojx[l] = ox, ojy[l] = oy;
            pf.Jt.load_interior(J2.img[max_level], (uint32_t)J2.pitch[max_level], ox, oy, t.tid - 64);
        }
    }
    if (t.tid == 64) {
#pragma unroll
        for (int l = 0; l < LK_MAX_LEVELS; l++) sh.s_pf[l][0] = oix[l], sh.s_pf[l][1] = oiy[l], sh.s_pf[l][2] = ojx[l], sh.s_pf[l][3] = ojy[l];
    }
}
// In the shadow of the top level's iterations: this wave prepares level l on its own (a wave reads back only what it wrote
// itself: LDS operations of one wave execute in order); published by that level's barrier.  The matrix is evaluated here too, so
// that the square root and the two divisions are not on the iterating wave's dependent chain (lk_level_matrix).
template <bool OPT>
__device__ __forceinline__ void lk_prepare_lower_level(LkShared &sh, const LkSegArgs &args, const LkPyramid &I, float2 pp, int l, int own_dx, int own_dy, const LkThread &t,
                                                       const LkAhead &pf) {
    const LkLevelGeom g = lk_level_geom(pp, l, I.w[l], I.h[l]);
    if (!g.ok) return;
    if (own_dx >= 0) pf.Io.store_window<LKR>(sh.regI[l], t.lane, own_dx, own_dy);  // fetched ahead by this wave
    lk_level_derivatives(sh, l, g, I.w[l], I.h[l], t.lane, 64);
    int s[6];
    lk_level_window(sh, l, g, t.lane, 64, s);
    if (t.lane == 0) lk_level_matrix<OPT>(args, lk_exact_total(s[0], s[1]), lk_exact_total(s[2], s[3]), lk_exact_total(s[4], s[5]), sh.level_mat[l]);
}
// the helper waves' work of a level: the next finer level's block or, at level 0, the fetch-ahead for the next pair; in the top level's
// shadow the lower levels' preparation, wave w level max_level - w
template <bool OPT>
__device__ __forceinline__ void lk_helper_level(LkShared &sh, const LkSegArgs &args, const LkPyramid &I, const LkPyramid &J, int fi, float2 pp, float2 gp, int level,
                                                int max_level, float lscale, int jb, int own_dx, int own_dy, const LkThread &t, LkAhead &pf) {
    LkStage<LKJR, LK_THREADS - 64> sn;
    int nx0 = PF_NONE, ny0 = PF_NONE;
    if (level > 0) lk_fetch_finer_block(sh, I, J, gp, level, max_level, lscale, jb, t, sn, nx0, ny0);
    else lk_fetch_ahead(sh, args, I, J, fi, pp, max_level, t, pf);
    if (level == max_level && t.wave <= max_level) lk_prepare_lower_level<OPT>(sh, args, I, pp, max_level - t.wave, own_dx, own_dy, t, pf);
    // the finer level's block goes into the other buffer: nobody reads that one now (wave 0 left it before this level's
    // barrier); the next barrier publishes it
    if (nx0 != PF_NONE) sn.store(sh.regJ[jb ^ 1], t.tid - 64);
}

// ---- publishing the pair's result ------------------------------------------------------------------------------------------------------
// wave 0 holds the result: hand it to the other waves (the next frame pair starts from it; a lost slot ends here), then one 16-byte
// record per feature and frame pair (make_record).  The device copy of the LAST pair feeds the launch chained behind this one.
__device__ __forceinline__ void lk_publish_pair(LkShared &sh, const LkSegArgs &args, int fi, unsigned int seq, const LkThread &t, float2 &np, int &st) {
    if (t.tid == 0) sh.s_result[0] = np.x, sh.s_result[1] = np.y, sh.s_result[2] = __int_as_float(st);
    __syncthreads();
    np = make_float2(sh.s_result[0], sh.s_result[1]), st = __float_as_int(sh.s_result[2]);
    LK_STAMP(15, LK_NOW());
    if (t.tid == 0) {
        lk_write_record(args, fi, t.f, make_record(np.x, np.y, (unsigned int)st, seq));
        if (!st) lk_write_dead(args, fi + 1, t.f, 2u);  // lost here: the remaining pairs of the segment report "lost earlier"
        if (args.clk) atomicMax(&args.clk[1], wall_clock64());
    }
}

// One launch tracks every feature slot through args.n_frames CONSECUTIVE frame pairs (a "segment"): frame pair i is
// (args.pyr[i], args.pyr[i + 1]); a slot starts pair 0 from the host's point list (prev_pts) or from the record the parent
// launch left for it (chain_in), and pair i + 1 from the point it tracked to in pair i -- FrameSourceWarp.cpp:427, where the
// surviving points of one frame are the next frame's input.  Every slot runs down its own chain at its own pace: the launch
// lasts as long as the slowest slot's SUM over the frames instead of the sum over the frames of each frame's slowest slot, and
// the gap between launches is paid once per segment.  Results leave per frame pair (host_rec[i], dev_rec[i]) as soon as the
// slot has them.  A slot that loses its feature reports status 0 for that pair and status 2 ("lost earlier") for the rest.
//
// ONE BODY, TWO KERNELS (vstab.h, "Tracker options").  k_lk_track is calcOpticalFlowPyrLK with default parameters and what every launch
// without options runs; k_lk_track_opt reads the launch's options.  Every option is read under `if constexpr (OPT)`, so the default
// instantiation is the kernel it was before the options existed: the same instructions (profiles/lk_options.txt).  launch_lk routes.
// The body is ONE TEXT (vstab_lk_body.hpp) that stands in both kernels, not a __forceinline__ function template they call.  It was
// written as one first: the compiler then simplifies the body once as a function of its own and a second time after inlining it into the
// kernel, and what came out for OPT = false was a different k_lk_track (148 VGPRs against 150, 25 instructions fewer, another schedule) --
// with the parent's statements word for word.  This kernel's schedule is what its time is made of (see the iteration loop's comment), so
// "the same kernel" is kept as a property of the build, tools/asm_kernel_diff.py on the two listings, rather than measured again.  The
// helpers above ARE function templates on OPT: they were functions before.
//
// A THIRD KERNEL PER FURTHER WINDOW (vstab.h, "Tracker window"): k_lk_track_win is the body with OPT = true, whatever the launch's options --
// a second pair of twins per size would buy the default options a few scalar loads.  Waves per SIMD asked of the compiler: three up to
// eight window pixels a lane (168 VGPRs, what the 21 x 21 kernels live in), two above (256 VGPRs: at sixteen pixels a lane the patch, the
// offsets and the blocks fetched ahead do not fit 168 without scratch).  At 31 the LDS allows two workgroups a CU anyway.
#define VSTAB_LK_BODY_FROM_KERNEL
constexpr int LK_MIN_WAVES = LK_PPL <= 8 ? 3 : 2;
#if VSTAB_LK_W == 21
__global__ void __launch_bounds__(LK_THREADS, 3) k_lk_track(LkSegArgs args) {
    __shared__ __attribute__((aligned(16))) LkShared sh;
    constexpr bool OPT = false;
#include "vstab_lk_body.hpp"
}
__global__ void __launch_bounds__(LK_THREADS, 3) k_lk_track_opt(LkSegArgs args) {
    __shared__ __attribute__((aligned(16))) LkShared sh;
    constexpr bool OPT = true;
#include "vstab_lk_body.hpp"
}
#else
__global__ void __launch_bounds__(LK_THREADS, LK_MIN_WAVES) k_lk_track_win(LkSegArgs args) {
    __shared__ __attribute__((aligned(16))) LkShared sh;
    constexpr bool OPT = true;
#include "vstab_lk_body.hpp"
}
#endif
#undef VSTAB_LK_BODY_FROM_KERNEL

#if VSTAB_LK_W != 21
}  // namespace lkw<W>
#endif
}  // namespace vstab
#undef LK_DESCALE
