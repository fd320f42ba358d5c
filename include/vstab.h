/*
 * vstab.h -- C ABI of the MI355X-native stabilisation / fisheye-undistort hot path.
 *
 * Drop-in boundary for the reference's FrameSource -> FrameSourceWarp stage
 * (reference paths are relative to /root/reference/opencv/).  Plain pointers and sizes only;
 * no C++, OpenCV, HIP or torch types cross this interface.  `stream` arguments are a
 * hipStream_t passed as void* (NULL = the default stream); every device pointer must belong
 * to the device that is current on the calling thread.  Stateless entry points enqueue work
 * on `stream` and return without synchronising unless they say otherwise.
 *
 * Error model: the reference throws `int` (EOF == -1 for end of stream,
 * FrameSourceWarp.cpp:466; other values for failures, :181,:303).  Nothing is thrown across
 * this ABI; the same information travels as vstab_status return codes and
 * vstab_last_error().  include/vstab_frame_source.hpp re-throws them as `int` so C++ callers
 * see the reference's behaviour.
 */
#ifndef VSTAB_H_
#define VSTAB_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VSTAB_API __attribute__((visibility("default")))

typedef enum vstab_status {
    VSTAB_OK = 0,
    VSTAB_EOF = -1,          /* == EOF thrown at FrameSourceWarp.cpp:466 */
    VSTAB_ERR_INVALID = -2,  /* bad argument / unsupported geometry */
    VSTAB_ERR_DEVICE = -3,   /* HIP runtime error (details in vstab_last_error) */
    VSTAB_ERR_NOMEM = -4,
    VSTAB_ERR_SOURCE = -5,   /* upstream callback failed with a code other than EOF */
    VSTAB_ERR_UNSUPPORTED = -6 /* a valid request this entry point does not serve (the text says which one does) */
} vstab_status;

/* CameraPreset, FrameSourceWarp.hpp:14-21 (same order, same values) */
typedef enum vstab_camera_preset {
    VSTAB_GOPRO_H4B_WIDE43_PUBLISHED = 0,
    VSTAB_GOPRO_H4B_WIDE43_MEASURED = 1,
    VSTAB_GOPRO_H4B_WIDE43_MEASURED_STABILISATION = 2,
    VSTAB_GOPRO_H4B_WIDE169_PUBLISHED = 3,
    VSTAB_GOPRO_H4B_WIDE169_MEASURED = 4,
    VSTAB_GOPRO_H4B_WIDE169_MEASURED_STABILISATION = 5
} vstab_camera_preset;

/* Thread-local text of the last failure of any call on this thread. */
VSTAB_API const char *vstab_last_error(void);
/* "vstab <version> gfx950" -- also proves the HIP code object is embedded. */
VSTAB_API const char *vstab_version(void);
/* Number of HIP devices visible, or a negative vstab_status. */
VSTAB_API int vstab_device_count(void);
/* sizeof() of the ABI structs as this library was compiled, for bindings to check their mirrors against:
 * 0 vstab_frame, 1 vstab_source, 2 vstab_config, 3 vstab_frame_log, 4 vstab_profile; -1 for any other index. */
VSTAB_API int vstab_struct_size(int which);
/* Layout version of the structs above.  It changes whenever one of them gains, loses or re-orders a member; a caller built against
 * another version of this header must not share a vstab_config / vstab_frame with this library.  vstab_config carries it
 * (vstab_config.abi_version, written by vstab_config_default) and vstab_create refuses any other value -- so a vstab_config MUST be
 * initialised with vstab_config_default() and then modified, never zero-filled or assembled by hand.  vstab_frame is always
 * allocated and zeroed by the library before a source callback fills it in.  Version 4: abi_version, vstab_frame.dmabuf_modifier;
 * map_precision defaults to VSTAB_MAP_PRECISION_OPENCL.  Version 5: vstab_config.read_ahead, two more counters in vstab_profile.
 * Version 6: vstab_config.resample.
 * The value is "VSB" + the version in the low byte: no field an older layout had at this offset (a preset 0..5) can hold it, so a
 * struct filled in against an older header is refused whatever its contents -- and with it every later call that would write a
 * larger vstab_profile into that caller's smaller one, since no handle is ever created for it. */
#define VSTAB_ABI_VERSION 0x56534206
VSTAB_API int vstab_abi_version(void);

/* ------------------------------------------------------------------------------------------
 * Cameras (host, fp64).  Replaces get_preset_camera / get_output_camera,
 * FrameSourceWarp.cpp:27-86 and :88-165, including their integer quirks.
 * Matrices are row-major 3x3 doubles.
 * ------------------------------------------------------------------------------------------ */
VSTAB_API vstab_status vstab_get_preset_camera(int preset, int width, int height, double K[9]);
VSTAB_API vstab_status vstab_get_output_camera(const double K_in[9], int width, int height,
                                               double scale, int crop_borders, double zoom,
                                               double K_out[9], int *out_width, int *out_height);
/* cv::fisheye::undistortPoints with zero distortion (calls at :93, :322, :333).
 * R and P may be NULL (identity).  pts/out are n (x,y) double pairs. */
VSTAB_API vstab_status vstab_fisheye_undistort_points(const double *pts, int n, const double K[9],
                                                      const double *R, const double *P,
                                                      double *out);
/* The 17 cl_float kernel arguments of createMap in argument order (:283-299):
 * src cx,cy,fx,fy ; out cx,cy,fx,fy ; rot00..rot22 (double -> float casts). */
VSTAB_API void vstab_map_params(const double K_in[9], const double K_out[9], const double R[9],
                                float params[17]);

/* ------------------------------------------------------------------------------------------
 * Stateless device operators (one HIP kernel each; all pointers are DEVICE pointers).
 * ------------------------------------------------------------------------------------------ */

/* Replaces convert_ocl_images_to_nv12_umat, FrameSourceFfmpegOpenCl.cpp:12-93: packs a pitched
 * luma plane (w x h) and a pitched interleaved chroma plane (w/2 x h/2 texels of 2 bytes) into
 * one contiguous (h*3/2) x w buffer.  w and h must be even ("Mismatched image dimensions"). */
VSTAB_API vstab_status vstab_pack_nv12(const void *y, size_t pitch_y, const void *uv,
                                       size_t pitch_uv, int width, int height, void *dst_nv12,
                                       void *stream);

/* Replaces cvtColor(COLOR_YUV2BGR_NV12), FrameSourceWarp.cpp:401.  dst is BGR8, pitch_dst bytes
 * per row (>= 3*width). */
/* 10-bit input (BASELINE config 5): P010 / P016 planes -- 16-bit little-endian samples, significant bits at the top,
 * pitches in bytes -- narrowed to packed 8-bit NV12 (byte = sample >> 8), which the rest of the path works on.
 * No reference counterpart: the reference only accepts 8-bit NV12 (FrameSourceFfmpegOpenCl.cpp:53-56). */
VSTAB_API vstab_status vstab_pack_p010(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv,
                                       int width, int height, void *dst_packed_nv12, void *stream);
VSTAB_API vstab_status vstab_cvt_nv12_bgr(const void *y, size_t pitch_y, const void *uv,
                                          size_t pitch_uv, int width, int height, void *dst_bgr,
                                          size_t pitch_dst, void *stream);

/* Replaces the createMap OpenCL kernel, createMap.cl:1-51 + launch at FrameSourceWarp.cpp:275-304.
 * map_x / map_y: float planes, pitch in bytes.  cols, rows <= 32767 (createMap.cl:10-11 uses
 * short indices). */
VSTAB_API vstab_status vstab_create_map(void *map_x, size_t pitch_x, void *map_y, size_t pitch_y,
                                        int cols, int rows, const float params[17], void *stream);

/* Replaces cv::remap(INTER_LINEAR, BORDER_CONSTANT 0), FrameSourceWarp.cpp:306-312, for an
 * 8-bit source of `channels` (1 or 3) interleaved channels. */
VSTAB_API vstab_status vstab_remap_bilinear(const void *src, size_t pitch_src, int src_width,
                                            int src_height, int channels, const void *map_x,
                                            size_t pitch_x, const void *map_y, size_t pitch_y,
                                            void *dst, size_t pitch_dst, int dst_width,
                                            int dst_height, void *stream);

/* The fused hot kernel: cvtColor (:401) + createMap (createMap.cl) + remap (:306-312) in one
 * pass, NV12 in -> BGR8 out, map never written to memory.  Bit-identical to running the three
 * operators above in sequence. */
VSTAB_API vstab_status vstab_warp_nv12_bgr(const void *y, size_t pitch_y, const void *uv,
                                           size_t pitch_uv, int src_width, int src_height,
                                           const float params[17], void *dst_bgr, size_t pitch_dst,
                                           int dst_width, int dst_height, void *stream);

/* The same fused warp with cv::remap's INTER_NEAREST: FrameSourceWarp.hpp:90 takes an InterpolationFlags argument and
 * FrameSourceWarp.cpp:311 hands it to cv::remap; the reference's callers only ever pass INTER_LINEAR.  OpenCV's CPU path:
 * cvRound (half to even) + saturate_cast<short> of each map entry, one source pixel, 0 outside (BORDER_CONSTANT). */
VSTAB_API vstab_status vstab_warp_nv12_nearest(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv,
                                               int src_width, int src_height, const float params[17], void *dst_bgr,
                                               size_t pitch_dst, int dst_width, int dst_height, void *stream);
/* The same with the map arithmetic chosen: VSTAB_MAP_CREATEMAP_CL (0, what the call above uses) or VSTAB_MAP_CREATEMAP_CL_OPENCL (5). */
VSTAB_API vstab_status vstab_warp_nv12_nearest_ex(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv,
                                                  int src_width, int src_height, const float params[17], int map_mode, void *dst_bgr,
                                                  size_t pitch_dst, int dst_width, int dst_height, void *stream);

/* ------------------------------------------------------------------------------------------
 * the camera surface of the CLI's libdewobble filter (render.ts:611-617,
 * 669-683, 711-717: in_p / out_p in {fish, rect}) and NV12 output for the encoder hand-off
 * (render.ts:275-281).  libdewobble is not part of the reference tree: these modes are defined by this
 * library and have no reference output to compare with.
 * ------------------------------------------------------------------------------------------ */
typedef enum vstab_map_mode {
    VSTAB_MAP_CREATEMAP_CL = 0, /* the reference kernel, quirks included (0/0 on the axis, mirrored rays behind the camera) */
    VSTAB_MAP_FISH_TO_RECT = 1, /* fisheye input -> pinhole output: createMap.cl's arithmetic without those two quirks */
    VSTAB_MAP_FISH_TO_FISH = 2,
    VSTAB_MAP_RECT_TO_RECT = 3,
    VSTAB_MAP_RECT_TO_FISH = 4,
    /* createMap.cl with the arithmetic the reference's OWN kernel has when ROCm's OpenCL compiler builds it for this GPU
     * (oracle/_ref/createMap.gfx950.co: contracted multiply-adds, reciprocal-based division, v_sqrt_f32, ocml's atan --
     * all inside OpenCL 1.2's error bounds, none IEEE-rounded).  Bit-identical to that code object run on the same
     * device (tests/test_refcl_gpu.py) and the arithmetic the pipeline object uses by default
     * (vstab_config.map_precision); mode 0 is the same kernel with every operation IEEE-rounded, reproducible on a
     * CPU.  The two differ in the last bits of the map.  Served wherever mode 0 is: map planes,
     * quantised map, fused warp, per-row (rolling-shutter) warp, nearest-neighbour warp, 10-bit warp. */
    VSTAB_MAP_CREATEMAP_CL_OPENCL = 5
} vstab_map_mode;
typedef enum vstab_out_format {
    VSTAB_OUT_BGR8 = 0, /* what FrameSourceWarp emits (FrameSourceWarp.cpp:313) */
    VSTAB_OUT_NV12 = 1, /* BGR result converted with cvtColor(COLOR_BGR2YUV_I420) arithmetic, chroma interleaved */
    /* PLANE-WISE warp, no colour round trip (SURVEY.md 8(f) row 2 as written: what a filter between NV12 surfaces does,
     * render.ts:606-607, 664-665, 688): the two planes of the source are remapped as they are.
     *   luma    cv::remap(INTER_LINEAR, BORDER_CONSTANT 16) of the Y plane with the map and 1/32-pixel quantisation of the BGR path;
     *   chroma  cv::remap(INTER_LINEAR, BORDER_CONSTANT (128, 128)) of the interleaved UV plane (2 channels, w/2 x h/2).  Output chroma
     *           sample (cx, cy) -- ceil(dst_width / 2) x ceil(dst_height / 2) of them -- sits on luma pixel (2 cx, 2 cy), as source
     *           chroma sample (i, j) sits on source luma pixel (2 i, 2 j): the siting the BGR path's conversions imply (NV12 -> BGR
     *           replicates a chroma sample over its 2 x 2 block, BGR -> NV12 takes the block's top-left pixel).  Its position in the
     *           source chroma plane is that luma pixel's map entry halved, (mapx / 2, mapy / 2) -- exact in fp32 -- and cv::remap
     *           quantises it like any map: cvRound(32 * (map / 2)).  A sample offset common to both frames (MPEG-2's half-pixel
     *           vertical shift) cancels to first order;
     *   border  limited-range black (Y 16, U = V 128): what the BGR path's border, cv::remap's Scalar(0), is in this colour space
     *           (a border of 0 would be green).  As in cv::remap a footprint wholly outside the source gives the border value
     *           and a tap outside it enters the blend as the border value.
     * Not the bytes of VSTAB_OUT_NV12 (which blends converted BGR pixels and converts back); on in-gamut content the two agree within
     * a level.  No reference counterpart: defined here and in the test infrastructure's plain-C statement (vo_remap_plane). */
    VSTAB_OUT_NV12_PLANAR = 2
} vstab_out_format;
/* vstab_create_map with a projection pair.  params as for vstab_create_map (focal lengths in pixels). */
VSTAB_API vstab_status vstab_create_map_ex(void *map_x, size_t pitch_x, void *map_y, size_t pitch_y,
                                           int cols, int rows, const float params[17], int map_mode,
                                           void *stream);
/* vstab_warp_nv12_bgr with a projection pair and an output format.  VSTAB_OUT_NV12 / VSTAB_OUT_NV12_PLANAR: dst is the luma
 * plane (width bytes per row), dst_uv the interleaved chroma plane (ceil(height/2) rows of 2*ceil(width/2) bytes);
 * dst_uv is ignored for VSTAB_OUT_BGR8. */
VSTAB_API vstab_status vstab_warp_nv12_ex(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv,
                                          int src_width, int src_height, const float params[17], int map_mode,
                                          int out_format, void *dst, size_t pitch_dst, void *dst_uv,
                                          size_t pitch_dst_uv, int dst_width, int dst_height, void *stream);

/* Rolling-shutter warp (BASELINE.json config 5: "rolling-shutter per-row warp"; no counterpart in the reference, whose gyro
 * path is a stub: gpmf.cpp:5-11): vstab_warp_nv12_ex for map modes 0 / 1 / 5 with a rotation per OUTPUT ROW.  Row y is mapped
 * with the matrix whose nine entries are interpolated in fp32 between params[8..16] (first row) and rot_bottom (last row):
 * t = (float)y / (float)max(dst_height - 1, 1) (IEEE division), m_k = fmaf(t, rot_bottom[k] - params[8 + k], params[8 + k]);
 * the row is then what the mode's createMap arithmetic makes of m -- in mode 5, what the reference's kernel returns for that
 * row when it is handed m as its rotation. */
VSTAB_API vstab_status vstab_warp_nv12_rs(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv,
                                          int src_width, int src_height, const float params[17], const float rot_bottom[9],
                                          int map_mode, int out_format, void *dst, size_t pitch_dst, void *dst_uv,
                                          size_t pitch_dst_uv, int dst_width, int dst_height, void *stream);


/* 10-bit pixel path (BASELINE.json config 5: "4K P010, fp16 blend, rolling-shutter per-row warp"; the reference is 8-bit
 * throughout, so this operator is DEFINED here and in the oracle, vo_warp_p010).  y / uv: P010 planes, 16-bit
 * little-endian samples with the 10 significant bits at the top, pitches in bytes, chroma interleaved U,V at half
 * resolution.  Conversion: BT.601 limited range with the cvtColor constants at 10 bits (offsets 64 / 512).  Map: as
 * vstab_warp_nv12_ex (all five modes); rot_bottom != NULL adds vstab_warp_nv12_rs's rotation per output row.  Blend:
 * VSTAB_BLEND_EXACT = the integer four-product sum of the 8-bit path, (sum + 512) >> 10; VSTAB_BLEND_FP16 = four fused
 * multiply-adds in binary16 (weights w / 1024, taps 00, 01, 10, 11), round to nearest even, clamp: within 2 levels of
 * the exact blend.  dst: BGR, three 16-bit samples per pixel, values 0..1023 (low-aligned). */
enum { VSTAB_BLEND_EXACT = 0, VSTAB_BLEND_FP16 = 1 };
VSTAB_API vstab_status vstab_warp_p010(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv,
                                       int src_width, int src_height, const float params[17], const float *rot_bottom,
                                       int map_mode, int blend, void *dst_bgr16, size_t pitch_dst, int dst_width,
                                       int dst_height, void *stream);

/* The plane-wise warp at 10 bits: P010 planes in, P010 planes out, no colour round trip -- VSTAB_OUT_NV12_PLANAR's definition on
 * the ten significant bits of each word (sample = word >> 6; border 64 / 512; result word = value << 6).  blend: VSTAB_BLEND_EXACT,
 * (sum + 512) >> 10 per sample, or VSTAB_BLEND_FP16, vstab_warp_p010's binary16 chain per sample.  All map modes; rot_bottom != NULL
 * adds the rotation per output row (modes 0 / 1 / 5).  dst_y: dst_width words per row; dst_uv: ceil(dst_height / 2) rows of
 * ceil(dst_width / 2) (U, V) word pairs.  Pitches in bytes; planes 2-byte aligned, chroma pairs 4-byte aligned. */
VSTAB_API vstab_status vstab_warp_p010_planar(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int src_width, int src_height,
                                              const float params[17], const float *rot_bottom, int map_mode, int blend, void *dst_y,
                                              size_t pitch_dst_y, void *dst_uv, size_t pitch_dst_uv, int dst_width, int dst_height, void *stream);

/* vstab_warp_p010 with P010 planes out in the same kernel (no 16-bit BGR frame in memory): the blended 10-bit BGR pixel is converted
 * in registers by vstab_cvt_bgr16_p010's arithmetic (below).  Served by the LDS-tiled kernel only: VSTAB_ERR_UNSUPPORTED unless the
 * source planes and pitches are 16-byte aligned and the map is VSTAB_MAP_CREATEMAP_CL or VSTAB_MAP_FISH_TO_RECT -- then warp to BGR and convert. */
VSTAB_API vstab_status vstab_warp_p010_planes(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int src_width, int src_height,
                                              const float params[17], const float *rot_bottom, int map_mode, int blend, void *dst_y,
                                              size_t pitch_dst_y, void *dst_uv, size_t pitch_dst_uv, int dst_width, int dst_height, void *stream);

/* The 10-bit path's encoder hand-off: BGR as vstab_warp_p010 writes it -> P010 planes (16-bit samples, significant bits at the top;
 * chroma interleaved U, V, ceil(w/2) x ceil(h/2) pairs, from the top-left pixel of each 2 x 2 block).  The BGR -> YUV arithmetic of the
 * NV12 output (cvtColor's BT.601 constants) at 10 bits, offsets 64 / 512; defined in the oracle (vo_cvt_bgr10_p010).  Pitches in bytes. */
VSTAB_API vstab_status vstab_cvt_bgr16_p010(const void *src_bgr16, size_t pitch_src, int width, int height, void *dst_y, size_t pitch_y,
                                            void *dst_uv, size_t pitch_uv, void *stream);

/* ------------------------------------------------------------------------------------------
 * Bicubic resampling: cv::remap's INTER_CUBIC, which FrameSourceWarp.hpp:90 admits and FrameSourceWarp.cpp:311 hands to cv::remap.
 * OpenCV 4.5's CPU path for 8-bit data, restated (tests/warp_def.py holds it in numpy, tests/golden/cubic_kat.npz pins it):
 *   quantisation  as INTER_LINEAR: sx = cvRound(32 * mapx) (half to even; NaN / out of int range -> INT_MIN), X = saturate_cast<short>(sx >> 5),
 *                 fx = sx & 31; the same for y;
 *   footprint     rows Y - 1 .. Y + 2, columns X - 1 .. X + 2;
 *   weights       entry fy * 32 + fx of OpenCV's fixed-point table (initInterTab2D(INTER_CUBIC)): interpolateCubic (A = -0.75) in fp32,
 *                 w[k1][k2] = saturate_cast<short>(cvRound(c_fy[k1] * c_fx[k2] * 32768.f)), then the correction that makes the 16 weights
 *                 sum to 32768 (vstab_cubic_weights returns the table);
 *   blend         per channel sat_u8((sum_k w_k * (tap_k inside ? S_k : border) + (1 << 14)) >> 15) -- cubic overshoots, so it saturates.
 * ------------------------------------------------------------------------------------------ */
/* The weight table: 1024 entries (index fy * 32 + fx) of 16 int16 weights, w[k1 * 4 + k2] for tap (X - 1 + k2, Y - 1 + k1).  Host memory. */
VSTAB_API vstab_status vstab_cubic_weights(int16_t out[16384]);
/* cv::remap(INTER_CUBIC, BORDER_CONSTANT) of an 8-bit source of `channels` (1, 2 or 3) interleaved channels with float map planes (pitches in
 * bytes; map planes 4-byte aligned).  border[0 .. channels - 1] in [0, 255]: the value of every tap outside the source; a footprint wholly
 * outside gives the border value. */
VSTAB_API vstab_status vstab_remap_cubic(const void *src, size_t pitch_src, int src_width, int src_height, int channels, const void *map_x,
                                         size_t pitch_x, const void *map_y, size_t pitch_y, const int border[3], void *dst, size_t pitch_dst,
                                         int dst_width, int dst_height, void *stream);
/* vstab_warp_nv12_ex with INTER_CUBIC in place of INTER_LINEAR, map modes 0 .. 5 (the map of each mode bit for bit).  out_format:
 *   VSTAB_OUT_BGR8         cvtColor(NV12 -> BGR) of the frame, then the cubic remap with border 0;
 *   VSTAB_OUT_NV12_PLANAR  the plane-wise definition above (vstab_out_format) with the cubic remap: luma with the map, border 16; the
 *                          interleaved chroma plane with map(2 cx, 2 cy) * 0.5f, border (128, 128).  dst_uv as for vstab_warp_nv12_ex.
 * VSTAB_OUT_NV12 (through BGR) and any other value are refused with VSTAB_ERR_INVALID.  Source even-sized, chroma plane 2-byte aligned. */
VSTAB_API vstab_status vstab_warp_nv12_cubic(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int src_width, int src_height,
                                             const float params[17], int map_mode, int out_format, void *dst, size_t pitch_dst, void *dst_uv,
                                             size_t pitch_dst_uv, int dst_width, int dst_height, void *stream);

/* ------------------------------------------------------------------------------------------
 * Lanczos resampling: cv::remap's INTER_LANCZOS4 (4), the fourth mode FrameSourceWarp.hpp:90 can hand to cv::remap.  OpenCV 4.5's CPU
 * path for 8-bit data, restated (tests/warp_def.py holds it in numpy, tests/golden/lanczos4_kat.npz pins it):
 *   quantisation  as INTER_LINEAR and INTER_CUBIC (above);
 *   footprint     rows Y - 3 .. Y + 4, columns X - 3 .. X + 4;
 *   1-D rows      interpolateLanczos4(x), x = k / 32: s0 = sin(y0), c0 = cos(y0) of y0 = -(x + 3) * pi / 4 in double; coefficient i =
 *                 (float)((cs[i][0] * s0 + cs[i][1] * c0) / (y * y)), y = -(x + 3 - i) * pi / 4; summed in fp32 in order i = 0..7, each
 *                 multiplied by 1.f / sum in fp32; x = 0 gives [0, 0, 0, 1, 0, 0, 0, 0];
 *   weights       entry fy * 32 + fx of OpenCV's fixed-point table (initInterTab2D(INTER_LANCZOS4)): w[k1][k2] =
 *                 saturate_cast<short>(cvRound(c_fy[k1] * c_fx[k2] * 32768.f)), the product in fp32, then the correction that makes the
 *                 64 weights sum to 32768, searched in k1, k2 in {4, 5} (vstab_lanczos4_weights returns the table).  Entry 0 is not the
 *                 identity: 32767 at tap (3, 3) and 1 at tap (4, 4);
 *   blend         per channel sat_u8((sum_k w_k * (tap_k inside ? S_k : border) + (1 << 14)) >> 15).
 * ------------------------------------------------------------------------------------------ */
/* The weight table: 1024 entries (index fy * 32 + fx) of 64 int16 weights, w[k1 * 8 + k2] for tap (X - 3 + k2, Y - 3 + k1).  Host memory. */
VSTAB_API vstab_status vstab_lanczos4_weights(int16_t out[65536]);
/* vstab_remap_cubic with INTER_LANCZOS4: the same arguments and the same checks. */
VSTAB_API vstab_status vstab_remap_lanczos4(const void *src, size_t pitch_src, int src_width, int src_height, int channels, const void *map_x,
                                            size_t pitch_x, const void *map_y, size_t pitch_y, const int border[3], void *dst, size_t pitch_dst,
                                            int dst_width, int dst_height, void *stream);
/* vstab_warp_nv12_cubic with INTER_LANCZOS4: the same arguments, output formats (VSTAB_OUT_BGR8, VSTAB_OUT_NV12_PLANAR) and checks. */
VSTAB_API vstab_status vstab_warp_nv12_lanczos4(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int src_width, int src_height,
                                                const float params[17], int map_mode, int out_format, void *dst, size_t pitch_dst, void *dst_uv,
                                                size_t pitch_dst_uv, int dst_width, int dst_height, void *stream);

/* ------------------------------------------------------------------------------------------
 * Border modes: cv::remap(src, dst, mapx, mapy, INTER_LINEAR, borderMode, borderValue), whose borderMode FrameSourceWarp.cpp:306-312 leaves
 * at BORDER_CONSTANT / Scalar().  The values are OpenCV's cv::BorderTypes.  ffmpeg's deshake `edge` option maps onto them: clamp =
 * BORDER_REPLICATE, mirror = BORDER_REFLECT_101, blank = BORDER_CONSTANT.  OpenCV 4.5's CPU path for 8-bit data, restated
 * (tests/warp_def.py holds it in numpy, tests/golden/border_kat.npz pins it):
 *   quantisation  as INTER_LINEAR above: sx = cvRound(32 * mapx), X = saturate_cast<short>(sx >> 5), fx = sx & 31; the same for y;
 *   taps          (X + i, Y + j), i, j in {0, 1}, read at (borderInterpolate(X + i, w, mode), borderInterpolate(Y + j, h, mode)):
 *                 REPLICATE clamps to [0, len - 1]; REFLECT / REFLECT_101 run OpenCV's loop
 *                 do { p = p < 0 ? -p - 1 + delta : len - 1 - (p - len) - delta; } while ((unsigned)p >= len), delta = 1 for REFLECT_101,
 *                 and len == 1 gives 0.  Every output pixel reads four source pixels: no pixel lies "wholly outside", and a NaN map entry
 *                 (X = Y = -32768, the 0/0 axis pixel of map mode 0) is interpolated like any other position;
 *   blend         sat_u8((w00 p00 + w01 p01 + w10 p10 + w11 p11 + 512) >> 10), w00 = (32 - fx)(32 - fy), w01 = fx (32 - fy),
 *                 w10 = (32 - fx) fy, w11 = fx fy -- the bilinear warp's;
 *   CONSTANT      taps outside take the border value, byte for byte what the warp without a border mode gives (BGR 0; plane-wise 16 and
 *                 (128, 128); vstab_remap_bilinear's 0).
 * WRAP (3), TRANSPARENT (5) and any other value are refused with VSTAB_ERR_INVALID.
 * ------------------------------------------------------------------------------------------ */
enum { VSTAB_BORDER_CONSTANT = 0, VSTAB_BORDER_REPLICATE = 1, VSTAB_BORDER_REFLECT = 2, VSTAB_BORDER_REFLECT_101 = 4 };
/* cv::remap(INTER_LINEAR, border_mode) of an 8-bit source of `channels` (1, 2 or 3) interleaved channels with float map planes (pitches in
 * bytes; map planes 4-byte aligned).  CONSTANT: border value 0, the bytes of vstab_remap_bilinear for channels 1 and 3. */
VSTAB_API vstab_status vstab_remap_bilinear_border(const void *src, size_t pitch_src, int src_width, int src_height, int channels,
                                                   const void *map_x, size_t pitch_x, const void *map_y, size_t pitch_y, int border_mode,
                                                   void *dst, size_t pitch_dst, int dst_width, int dst_height, void *stream);
/* vstab_warp_nv12_ex with a border mode, map modes 0 .. 5 (the map of each mode bit for bit); rot_bottom != NULL adds vstab_warp_nv12_rs's
 * rotation per output row (map modes 0, 1 and 5; the others are refused with VSTAB_ERR_INVALID).  out_format:
 *   VSTAB_OUT_BGR8         cvtColor(NV12 -> BGR) of the frame, then the remap with border_mode (CONSTANT: value 0);
 *   VSTAB_OUT_NV12_PLANAR  the plane-wise definition above (vstab_out_format): luma with the map; the interleaved chroma plane with
 *                          map(2 cx, 2 cy) * 0.5f, border-interpolated over the chroma plane's own size src_width / 2 x src_height / 2
 *                          (CONSTANT: values 16 and (128, 128)).  dst_uv as for vstab_warp_nv12_ex.
 * VSTAB_OUT_NV12 (through BGR) and any other value are refused with VSTAB_ERR_INVALID.  Source even-sized and <= 32767, chroma plane
 * 2-byte aligned.  CONSTANT gives the bytes of vstab_warp_nv12_ex / vstab_warp_nv12_rs. */
VSTAB_API vstab_status vstab_warp_nv12_border(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int src_width, int src_height,
                                              const float params[17], const float *rot_bottom, int map_mode, int out_format, int border_mode,
                                              void *dst, size_t pitch_dst, void *dst_uv, size_t pitch_dst_uv, int dst_width, int dst_height,
                                              void *stream);

/* ------------------------------------------------------------------------------------------
 * Border modes of the cubic and Lanczos resamplers: cv::remap(src, dst, mapx, mapy, INTER_CUBIC or INTER_LANCZOS4, borderMode, borderValue),
 * the interpolation and the border chosen independently as cv::remap takes them.  OpenCV 4.5's CPU remapBicubic / remapLanczos4 for 8-bit
 * data on the branch taken when borderMode is not BORDER_CONSTANT (tests/warp_def.py holds it in numpy,
 * tests/golden/resample_border_kat.npz pins it):
 *   quantisation, weights, blend  as "Bicubic resampling" / "Lanczos resampling" above: (sum + 2^14) >> 15, saturated;
 *   taps          tap (X - 1 + i, Y - 1 + j) (cubic) or (X - 3 + i, Y - 3 + j) (Lanczos) is read at (borderInterpolate(x, w, mode),
 *                 borderInterpolate(y, h, mode)) with the modes of "Border modes" above.  Every output pixel reads its full footprint; a NaN
 *                 map entry (X = Y = -32768) is folded like any other position, so positions reach -32771 .. 32771;
 *   sum           OpenCV's cval * ONE + sum((S - cval) * w) is sum(S * w) here: every entry of both tables sums to 32768.
 * BORDER_CONSTANT through these entry points gives exactly the bytes of vstab_remap_cubic / _lanczos4 (with border[]) and
 * vstab_warp_nv12_cubic / _lanczos4.  WRAP (3), TRANSPARENT (5) and any other value are refused with VSTAB_ERR_INVALID.
 * ------------------------------------------------------------------------------------------ */
/* vstab_remap_cubic / vstab_remap_lanczos4 with a border mode: the same arguments and checks, plus border_mode.  border[] is read under
 * VSTAB_BORDER_CONSTANT only (and may be NULL otherwise). */
VSTAB_API vstab_status vstab_remap_cubic_border(const void *src, size_t pitch_src, int src_width, int src_height, int channels, const void *map_x,
                                                size_t pitch_x, const void *map_y, size_t pitch_y, int border_mode, const int border[3], void *dst,
                                                size_t pitch_dst, int dst_width, int dst_height, void *stream);
VSTAB_API vstab_status vstab_remap_lanczos4_border(const void *src, size_t pitch_src, int src_width, int src_height, int channels,
                                                   const void *map_x, size_t pitch_x, const void *map_y, size_t pitch_y, int border_mode,
                                                   const int border[3], void *dst, size_t pitch_dst, int dst_width, int dst_height, void *stream);
/* vstab_warp_nv12_cubic / vstab_warp_nv12_lanczos4 with a border mode: the same arguments and output formats (VSTAB_OUT_BGR8,
 * VSTAB_OUT_NV12_PLANAR), plus border_mode.  VSTAB_OUT_NV12_PLANAR folds luma over the source and the interleaved chroma plane, with
 * map(2 cx, 2 cy) * 0.5f, over its own size src_width / 2 x src_height / 2, as vstab_warp_nv12_border does.  Source even-sized and
 * <= 32767, chroma plane 2-byte aligned; every argument is checked before any launch. */
VSTAB_API vstab_status vstab_warp_nv12_cubic_border(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int src_width, int src_height,
                                                    const float params[17], int map_mode, int out_format, int border_mode, void *dst,
                                                    size_t pitch_dst, void *dst_uv, size_t pitch_dst_uv, int dst_width, int dst_height, void *stream);
VSTAB_API vstab_status vstab_warp_nv12_lanczos4_border(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int src_width,
                                                       int src_height, const float params[17], int map_mode, int out_format, int border_mode,
                                                       void *dst, size_t pitch_dst, void *dst_uv, size_t pitch_dst_uv, int dst_width,
                                                       int dst_height, void *stream);

/* ------------------------------------------------------------------------------------------
 * Keep edges: where the warped frame does not cover the output, the output keeps what the caller had there -- vid.stab's default border
 * (`keep`), how deshake and Gyroflow users hide moving black wedges without inventing mirrored picture, and cv::remap's own
 * BORDER_TRANSPARENT.  The feature has entry points of its own (the border modes above keep refusing TRANSPARENT (5)), and the history
 * belongs to the caller, who passes the frame to keep as `prev`: encoders and players hold their last output anyway.  INTER_LINEAR, 8-bit
 * (tests/warp_def.py holds the definition in numpy, tests/golden/keep_kat.npz pins it):
 *   quantisation  as INTER_LINEAR above: sx = cvRound(32 * mapx) (NaN / outside the int range: INT_MIN), X = saturate_cast<short>(sx >> 5),
 *                 fx = sx & 31; the same for y;
 *   written       an output sample is WRITTEN iff its 2 x 2 footprint lies wholly inside the plane it reads: 0 <= X <= len_x - 2 and
 *                 0 <= Y <= len_y - 2 -- cv::remap's inlier test (unsigned)X < w - 1.  A written sample has exactly the bytes the
 *                 constant-border bilinear warp gives, (sum of four products + 512) >> 10; no border value enters it;
 *   kept          every other sample: dst receives the byte of prev at the same position, or is not stored at all when prev == dst.
 * So: an exact hit on the last column or row (X == len_x - 1, fx == 0) is kept, as in OpenCV; a NaN map entry (X = Y = -32768) is kept; a
 * plane with len < 2 keeps everything.
 * Planes.  BGR8: the colour conversion comes before the remap, and the samples are decided over the full-size frame, all three channels
 * together.  Plane-wise NV12: luma is decided over src_width x src_height; the interleaved chroma plane is decided independently, with
 * map(2 cx, 2 cy) * 0.5f over its own size src_width / 2 x src_height / 2, the pair (U, V) kept or written together -- as
 * vstab_warp_nv12_border treats the planes.  This is cv::remap BORDER_TRANSPARENT's rule for 1- and 2-channel data; for 3-channel data
 * (BGR) the rule is DEFINED here, not claimed equal to OpenCV's branch for it.
 * Aliasing.  prev may be exactly dst -- the same pointer and the same pitch; for plane-wise output both planes -- which is the in-place
 * case, BORDER_TRANSPARENT itself.  Any other overlap of the byte ranges of prev and dst is refused with VSTAB_ERR_INVALID, and so is
 * prev == NULL.  prev is never written.
 * Out of scope, and not offered in a keep-edge form: the calibrated lens, INTER_CUBIC, INTER_LANCZOS4, INTER_NEAREST and the 10-bit warps.
 * ------------------------------------------------------------------------------------------ */
/* The keep-edge remap of an 8-bit source of `channels` (1, 2 or 3) interleaved channels with float map planes (pitches in bytes; map planes
 * 4-byte aligned).  vstab_remap_bilinear_border's checks in their order, then prev: "null pointer", "prev pitch smaller than row", the
 * aliasing rule. */
VSTAB_API vstab_status vstab_remap_bilinear_keep(const void *src, size_t pitch_src, int src_width, int src_height, int channels,
                                                 const void *map_x, size_t pitch_x, const void *map_y, size_t pitch_y, const void *prev,
                                                 size_t pitch_prev, void *dst, size_t pitch_dst, int dst_width, int dst_height, void *stream);
/* The keep-edge warp of an NV12 frame, map modes 0 .. 5 (the map of each mode bit for bit); rot_bottom != NULL adds vstab_warp_nv12_rs's
 * rotation per output row (map modes 0, 1 and 5; the others are refused with VSTAB_ERR_INVALID).  out_format: VSTAB_OUT_BGR8 (prev, dst:
 * BGR frames; prev_uv, dst_uv ignored) or VSTAB_OUT_NV12_PLANAR (prev / prev_uv, dst / dst_uv: the luma and the chroma planes, dst_uv as
 * for vstab_warp_nv12_ex); every other value is VSTAB_ERR_INVALID.  vstab_warp_nv12_border's checks in their order, then prev as above;
 * every check runs before any launch. */
VSTAB_API vstab_status vstab_warp_nv12_keep(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int src_width, int src_height,
                                            const float params[17], const float *rot_bottom, int map_mode, int out_format, const void *prev,
                                            size_t pitch_prev, const void *prev_uv, size_t pitch_prev_uv, void *dst, size_t pitch_dst,
                                            void *dst_uv, size_t pitch_dst_uv, int dst_width, int dst_height, void *stream);

/* ------------------------------------------------------------------------------------------
 * Tracking front-end (device images in; small point lists on the host, as in the reference where
 * goodFeaturesToTrack / calcOpticalFlowPyrLK return std::vector<Point2f>).  These calls
 * synchronise `stream` before returning because their outputs live in host memory.
 * ------------------------------------------------------------------------------------------ */

/* cv::pyrDown (5x5 binomial, REFLECT_101) as used for the LK pyramid; dst is ((w+1)/2, (h+1)/2). */
VSTAB_API vstab_status vstab_pyr_down(const void *src, size_t pitch_src, int width, int height,
                                      void *dst, size_t pitch_dst, void *stream);

/* Two pyramid levels in one launch, as the pipeline builds levels 2 and 3 of the LK pyramid: mid = pyrDown(src) ((w+1)/2 x (h+1)/2),
 * dst = pyrDown(mid) -- the bytes of two vstab_pyr_down calls (the small levels are launch- and latency-bound as kernels of their own). */
VSTAB_API vstab_status vstab_pyr_down_x2(const void *src, size_t pitch_src, int width, int height, void *mid, size_t pitch_mid,
                                         void *dst, size_t pitch_dst, void *stream);

/* cornerMinEigenVal(blockSize 3, ksize 3): dense width x height float response (device). */
VSTAB_API vstab_status vstab_min_eig(const void *gray, size_t pitch, int width, int height,
                                     void *eig_f32, void *stream);

/* Replaces find_corners -> goodFeaturesToTrack(gray, max_corners, quality, min_distance),
 * FrameSourceWarp.cpp:228-240 (the reference passes 200, 0.01, 30).  xy receives up to
 * max_corners (x,y) float pairs in acceptance order; *count the number found.
 * Arguments, as goodFeaturesToTrack asserts them: quality > 0 and min_distance >= 0; NaN fails either.  quality = +inf passes and finds
 * no corner (nothing lies above an infinite threshold), as every quality >= 1 does under the strict >.  min_distance = +inf or beyond the
 * image's diagonal passes and gives one corner, the strongest.  vstab_good_features, _ex, _mask and _harris refuse anything else with
 * VSTAB_ERR_INVALID and "<function>: quality must be > 0 and min_distance >= 0" -- behind "<function>: bad argument" (max_corners <= 0
 * is one) and before the mask's and k's checks. */
VSTAB_API vstab_status vstab_good_features(const void *gray, size_t pitch, int width, int height,
                                           int max_corners, double quality, double min_distance,
                                           float *xy, int *count, void *stream);

/* The same with a choice of detector.  AUTO: one fused pass (eigenvalue, threshold and 3x3 maximum test in one kernel,
 * the eigenvalue map is never stored); a frame with more than 2^18 corners above the threshold (an eigenvalue plateau
 * over most of a large frame) falls back to TWO_PASS, which stores the map (vstab_min_eig), scans it and grows its key
 * buffer as needed.  Both give the same corners.  *detector_used (may be NULL) receives VSTAB_DETECTOR_FUSED or
 * VSTAB_DETECTOR_TWO_PASS. */
enum { VSTAB_DETECTOR_AUTO = 0, VSTAB_DETECTOR_TWO_PASS = 1, VSTAB_DETECTOR_FUSED = 2 };
VSTAB_API vstab_status vstab_good_features_ex(const void *gray, size_t pitch, int width, int height,
                                              int max_corners, double quality, double min_distance, int detector,
                                              float *xy, int *count, int *detector_used, void *stream);

/* ---- Detection mask ----------------------------------------------------------------------------------------------------------------
 * goodFeaturesToTrack's `mask` argument, as OpenCV 4.5's goodFeaturesToTrack(gray, corners, max_corners, quality, min_distance, mask, 3,
 * false, 0.04) applies it on its CPU path.  mask: width x height bytes, pitch_mask >= width; non-zero = "a corner may be reported here".
 *   1. The eigenvalue map is cornerMinEigenVal(3, 3) of the whole image: the mask plays no part in it, the derivative and box windows
 *      read masked-out pixels.
 *   2. maxVal is the maximum of the map over the pixels with mask != 0 (minMaxLoc(eig, 0, &maxVal, 0, 0, mask)); with no such pixel the
 *      result is 0 corners.
 *   3. The threshold is (float)((double)maxVal * quality), strict >, applied to every pixel.
 *   4. The 3 x 3 maximum test runs over all pixels: a masked-out neighbour competes, and a masked-in pixel beside a stronger masked-out one
 *      is not a corner (dilate knows no mask).
 *   5. A pixel is a candidate iff it is an interior pixel, passes 3 and 4, and mask != 0 there.
 *   6. The order (value descending, ties: later raster index first), the min_distance grid and max_corners are those of
 *      vstab_good_features.
 * A mask that is non-zero everywhere gives the corners of vstab_good_features_ex bit for bit.  The detectors take the maximum in the order of
 * the floats' bits read as int32, which is the float order while the maximum is not negative: a frame whose maximum -- under a mask, whose
 * maximum over the masked-in pixels -- is negative (a frame of rounding noise around zero) is outside what this definition covers, with
 * or without a mask.  The mask governs DETECTION only: the tracker follows a corner wherever it goes, into masked-out areas too, as
 * calcOpticalFlowPyrLK does.
 *
 * vstab_good_features_mask is vstab_good_features_ex with a device mask.  mask == NULL: the launches and the corners of
 * vstab_good_features_ex.  detector: VSTAB_DETECTOR_AUTO and VSTAB_DETECTOR_FUSED (the same here: the fused pass, and the two-pass detector
 * behind it when more than 2^18 keys survive) or VSTAB_DETECTOR_TWO_PASS; all honour the mask and give the same corners.  Refused with
 * VSTAB_ERR_INVALID before any launch, in this order: "vstab_good_features_mask: bad argument" (what vstab_good_features_ex refuses, an
 * unknown detector included); "vstab_good_features_mask: quality must be > 0 and min_distance >= 0" (vstab_good_features above);
 * with a mask, "vstab_good_features_mask: the mask's pitch is smaller than the image's width" and
 * "vstab_good_features_mask: mask planes of 4 GiB or more are not supported" ((uint64_t)pitch_mask * height >= 2^32). */
VSTAB_API vstab_status vstab_good_features_mask(const void *gray, size_t pitch, int width, int height, const void *mask, size_t pitch_mask,
                                                int max_corners, double quality, double min_distance, int detector,
                                                float *xy, int *count, int *detector_used, void *stream);

/* ---- Harris response -----------------------------------------------------------------------------------------------------------------
 * goodFeaturesToTrack's `useHarrisDetector` and `k`, and cornerHarris as a dense map, as OpenCV 4.5 computes them on its CPU path:
 * cornerHarris(gray, dst, 3, 3, k) and goodFeaturesToTrack(gray, corners, max_corners, quality, min_distance, mask, 3, true, k).
 *   1. Covariance sums.  a, b, c are the three box sums of cornerMinEigenVal(3, 3) exactly as vstab_min_eig forms them: Sobel derivatives
 *      scaled by 1 / (4 * 3 * 255) in the documented operation order, the float products dx dx, dx dy, dy dy, the un-normalised 3 x 3 box
 *      sum under REFLECT_101 (exact in double), each sum rounded once to float.  They are those floats BEFORE the minimum-eigenvalue
 *      formula halves two of them: OpenCV uses one scale for both responses.
 *   2. Response.  kf = (float)k, t = a + c, R = (a c - b b) - (kf t) t: every operation rounded to binary32, in that order, nothing
 *      contracted.  This is the arithmetic of OpenCV's vector path (v_float32, k set as a float), which computes all but the last few
 *      columns of a row; its scalar tail keeps k in double.  This library uses the vector form for EVERY pixel.  It claims no bit equality
 *      with OpenCV: like the minimum-eigenvalue detector, this is a restatement.
 *   3. Detector.  The steps of vstab_good_features_mask ("Detection mask" above) on R in place of the eigenvalue: the maximum over the
 *      masked-in pixels (all pixels without a mask), the threshold (float)((double)maxVal * quality) with strict >, the 3 x 3 maximum test
 *      over all pixels, interior pixels only, the mask gate, the order of the keys, the min_distance grid and max_corners.
 *   4. A (masked) maximum that is not positive gives no corner.  R is negative over about half of an ordinary frame, and over all of a
 *      frame of stripes or of a ramp (edges and flat ground, no corner): with maxVal <= 0 nothing lies above maxVal * quality but what
 *      OpenCV's THRESH_TOZERO then sets to zero and its `val != 0` test drops.  The detectors take maxima in the order of the floats' bits
 *      read as int32; that order is wrong among negative values but right about the sign: if any value is >= +0 the maximum's bits are
 *      >= 0.  The sign of the published maximum decides this rule, on every path.
 *   5. k is finite with 0 <= k < 0.25: from 0.25 on, det - k tr^2 is never positive.  Anything else is refused.
 * The minimum-eigenvalue detector keeps its definition and its caveat ("Detection mask" above) word for word.  gradientSize 5 and 7 are
 * "Corner gradient size" below; blockSize 5 and 7 are "Corner block size" below.
 *
 * vstab_corner_harris is vstab_min_eig's twin: response_f32 is a dense width x height device map of R.  Refused with VSTAB_ERR_INVALID
 * before any launch: "vstab_corner_harris: bad argument" (what vstab_min_eig refuses), then "vstab_corner_harris: k lies in [0, 0.25)".
 * vstab_good_features_harris is vstab_good_features_mask with the Harris response; mask == NULL means no mask.  Its refusals are those of
 * vstab_good_features_mask under this name, in that order, then "vstab_good_features_harris: k lies in [0, 0.25)". */
enum { VSTAB_CORNER_MIN_EIGENVAL = 0, VSTAB_CORNER_HARRIS = 1 };
VSTAB_API vstab_status vstab_corner_harris(const void *gray, size_t pitch, int width, int height, double k, void *response_f32, void *stream);
VSTAB_API vstab_status vstab_good_features_harris(const void *gray, size_t pitch, int width, int height, const void *mask, size_t pitch_mask,
                                                  int max_corners, double quality, double min_distance, double k, int detector,
                                                  float *xy, int *count, int *detector_used, void *stream);

/* ---- Corner block size ------------------------------------------------------------------------------------------------------------
 * goodFeaturesToTrack's `blockSize`: the window of the covariance sums.  B = block_size is 3, 5 or 7, r = (B - 1) / 2; everything else is
 * refused, not clamped (even sizes, 1, 9 and larger).  gradientSize is "Corner gradient size" below.  Like the rest of the detector this restates OpenCV 4.5's CPU
 * path -- cornerMinEigenVal(gray, B, 3), cornerHarris(gray, B, 3, k), goodFeaturesToTrack(..., mask, B, useHarris, k) -- in this library's
 * arithmetic; no bit equality with OpenCV is claimed.
 *   1. Derivatives.  The 3 x 3 Sobel pair of vstab_min_eig in its documented operation order, REFLECT_101 of the source, with the scale
 *      scale_B = (float)(1.0 / (4.0 * B * 255.0)), k1 = scale_B, k0 = 2.0f * scale_B.
 *   2. Products.  dx dx, dx dy, dy dy, each one binary32 product.
 *   3. Box sum.  The un-normalised B x B sum centred on the pixel, over the product planes extended by REFLECT_101: the product AT the
 *      mirrored position.  The extension folds as often as it takes (an image narrower than r + 1 folds more than once; a 1-pixel axis
 *      repeats its pixel).  The order is part of the definition, all in double: column sums first, top to bottom,
 *      c(y, x') = (((p(y-r, x') + p(y-r+1, x')) + ...) + p(y+r, x')); then left to right, S(y, x) = (((c(y, x-r) + c(y, x-r+1)) + ...) +
 *      c(y, x+r)); then ONE rounding to float.  The order matters: within one frame the float products can span 77 bits (dy may be a
 *      rounding residue far below k1), and sums of 25 or 49 of them are not always exact in double; the 9 of block 3 are.
 *   4. Response.  On a = S_xx, b = S_xy, c = S_yy: the minimum-eigenvalue formula of vstab_min_eig with its two halvings, or the formula of
 *      "Harris response" rule 2; both unchanged, nothing contracted.
 *   5. Detector.  Everything behind the response is untouched by B: the maximum (over the masked-in pixels under a mask), the threshold
 *      (float)((double)maxVal * quality) with strict >, the 3 x 3 maximum test over all pixels (OpenCV's dilate does not grow with
 *      blockSize), interior pixels only (1 .. width - 2, 1 .. height - 2, whatever B is), the mask gate, rule 4 of the Harris response,
 *      the order of the keys, the min_distance grid and max_corners.
 * With block_size 3 each of the three calls below IS its block-3 twin (vstab_min_eig, vstab_corner_harris, and vstab_good_features_mask or
 * vstab_good_features_harris): the same kernels, the same bytes.
 *
 * vstab_good_features_block is goodFeaturesToTrack's whole argument list in one call: mask == NULL means no mask; use_harris is 0 or 1, and
 * k is looked at only with use_harris = 1.  Refused with VSTAB_ERR_INVALID before any launch, in this order (fn = the call's name):
 * "<fn>: bad argument" (what the block-3 twin refuses; use_harris outside {0, 1} belongs here); "<fn>: block_size is 3, 5 or 7"; then
 * the twin's remaining messages under this name in their order -- "quality must be > 0 and min_distance >= 0", the mask's pitch, the
 * mask's size, "k lies in [0, 0.25)". */
VSTAB_API vstab_status vstab_min_eig_block(const void *gray, size_t pitch, int width, int height, int block_size, void *eig_f32, void *stream);
VSTAB_API vstab_status vstab_corner_harris_block(const void *gray, size_t pitch, int width, int height, int block_size, double k, void *response_f32,
                                                 void *stream);
VSTAB_API vstab_status vstab_good_features_block(const void *gray, size_t pitch, int width, int height, const void *mask, size_t pitch_mask,
                                                 int max_corners, double quality, double min_distance, int block_size, int use_harris, double k,
                                                 int detector, float *xy, int *count, int *detector_used, void *stream);

/* ---- Corner gradient size ---------------------------------------------------------------------------------------------------------
 * goodFeaturesToTrack's `gradientSize`: the Sobel aperture of cornerMinEigenVal / cornerHarris.  G = gradient_size is 3, 5 or 7,
 * g = (G - 1) / 2; everything else is refused, not clamped (1, even sizes, 9 and larger, OpenCV's -1 for Scharr).  B = block_size is 3, 5
 * or 7 as in "Corner block size"; all nine pairs are served.  Like the rest of the detector this restates OpenCV 4.5's CPU path --
 * cornerMinEigenVal(gray, B, G), cornerHarris(gray, B, G, k), goodFeaturesToTrack(gray, corners, maxCorners, quality, minDistance, mask, B,
 * G, useHarris, k) -- in this library's arithmetic; no bit equality with OpenCV is claimed.
 *   1. Kernels.  getDerivKernels' integer Sobel pair.  Smoothing s, from the centre outwards: G = 3 (2, 1); G = 5 (6, 4, 1); G = 7
 *      (20, 15, 6, 1).  Derivative d on the positive side, antisymmetric, d_0 = 0: G = 3 (1); G = 5 (2, 1); G = 7 (5, 4, 1).
 *   2. Scale.  sigma = 1.0 / ((double)(1 << (G - 1)) * B * 255.0) in double; the scaled smoothing coefficients are
 *      k_i = (float)((double)s_i * sigma).  For G = 3 these are k1 = scale_B, k0 = 2.0f * scale_B of "Corner block size" bit for bit.
 *   3. dx.  Row pass: D(y, x) = sum over i = 1 .. g of d_i * (I(y, x + i) - I(y, x - i)) over the REFLECT_101 extension of the source:
 *      whole numbers of magnitude <= 2550, exact as floats.  Column pass in binary32, nothing contracted, the outermost pair first and the
 *      centre last: dx = (...((D(y - g) + D(y + g)) * k_g + (D(y - g + 1) + D(y + g - 1)) * k_(g-1)) + ...) + D(y) * k_0.
 *   4. dy.  Row pass in binary32, the centre first and outwards, added left to right:
 *      S(y, x) = ((I(x) * k_0 + (I(x - 1) + I(x + 1)) * k_1) + (I(x - 2) + I(x + 2)) * k_2) + ...; column pass
 *      dy = ((float)d_1 * (S(y + 1) - S(y - 1)) + (float)d_2 * (S(y + 2) - S(y - 2))) + ..., ascending i.
 *   5. Everything else is "Corner block size" rules 2 - 5, unchanged: the three float products, the B x B box sum over the product planes
 *      extended by REFLECT_101 in its defined order, the two response formulas, and a detector in which nothing depends on G (interior
 *      pixels are 1 .. width - 2 and 1 .. height - 2 whatever G is).  With G other than 3 the order of the box sum is part of the
 *      definition for B = 3 as well: the nine-product sums that are exact in double at G = 3 are not always exact at G = 5 and 7.
 * With gradient_size 3 each of the three calls below IS its "Corner block size" twin: the same kernels, the same bytes.
 *
 * vstab_good_features_grad is goodFeaturesToTrack's ten-argument overload.  The refusals (VSTAB_ERR_INVALID, before any launch) are those
 * of the _block twin under the new name, in its order, with "<fn>: gradient_size is 3, 5 or 7" directly behind
 * "<fn>: block_size is 3, 5 or 7". */
VSTAB_API vstab_status vstab_min_eig_grad(const void *gray, size_t pitch, int width, int height, int block_size, int gradient_size, void *eig_f32,
                                          void *stream);
VSTAB_API vstab_status vstab_corner_harris_grad(const void *gray, size_t pitch, int width, int height, int block_size, int gradient_size, double k,
                                                void *response_f32, void *stream);
VSTAB_API vstab_status vstab_good_features_grad(const void *gray, size_t pitch, int width, int height, const void *mask, size_t pitch_mask,
                                                int max_corners, double quality, double min_distance, int block_size, int gradient_size,
                                                int use_harris, double k, int detector, float *xy, int *count, int *detector_used, void *stream);

/* Replaces calcOpticalFlowPyrLK with default parameters (win 21x21, maxLevel 3, 30 iterations,
 * eps 0.01, minEigThreshold 1e-4), FrameSourceWarp.cpp:252.  prev/next: device gray images of the
 * same size; prev_xy: n host (x,y) pairs; next_xy / status: host outputs (n pairs / n bytes).
 * A start point with a NaN or infinite coordinate, or one whose window origin lies outside int, is never tracked: status 0 and the
 * point returned as it came (a NaN stays a NaN), as OpenCV's float-to-int conversion (INT_MIN for all of these) decides it. */
VSTAB_API vstab_status vstab_pyr_lk(const void *prev, size_t pitch_prev, const void *next,
                                    size_t pitch_next, int width, int height, const float *prev_xy,
                                    int n, float *next_xy, unsigned char *status, void *stream);

/* ---- Tracker options -----------------------------------------------------------------------------------------------------------------
 * calcOpticalFlowPyrLK's maxLevel, criteria (count and epsilon), minEigThreshold, flags and err: a restatement of OpenCV 4.5's CPU
 * LKTrackerInvoker in this library's arithmetic (exact integer sums converted once, the float operations in the documented order).  It
 * claims no bit equality with OpenCV.  winSize is 21 x 21 here; the other offered windows are "Tracker window" below (the detector's gradientSize is
 * "Corner gradient size" above).
 *   1. Levels.  The pyramid has min(levels of vstab_pyr_lk, max_level + 1) levels.  Everything else about a level is as in vstab_pyr_lk.
 *   2. Start of the top level.  With VSTAB_LK_USE_INITIAL_FLOW next_xy is also an input: the top level L starts the next-image estimate at
 *      next_xy[i] * (float)(1.0 / (1 << L)); without the flag at the scaled previous point.  The previous image's side -- the window, the
 *      derivatives, the matrix and the per-level range test of the previous point -- is untouched.  A guess is caller data and may be any
 *      float; vstab_pyr_lk's rule holds with the guess in the start point's place: a NaN, infinite or out-of-int guess fails the range test
 *      of the first iteration at every level and gives status 0 and the guess back bit for bit.  A guess equal to prev_xy gives the bytes
 *      of the call without the flag.
 *   3. Iterations.  A level runs at most max_iter Gauss-Newton steps and ends on (double)dx*dx + (double)dy*dy <= (double)eps * (double)eps.
 *      The oscillation rule (two successive steps that cancel to within 0.01) keeps OpenCV's fixed 0.01.
 *   4. Rejection.  A level is rejected when minEig < (float)min_eig_threshold || D < FLT_EPSILON, minEig being the smaller eigenvalue of the
 *      level's 2 x 2 gradient matrix divided by 2 * 21 * 21, in float.
 *   5. err, default mode.  At level 0, for a point whose status is still 1 after the final range test: f = next - 10 in float, the origin is
 *      floor(f), the four 14-bit weights are those of its fraction, S = the sum over the 441 window pixels of
 *      |DESCALE(interpolated next image, 9) - interpolated previous window|.  S is an integer <= 441 * 8160 < 2^24, so OpenCV's float
 *      accumulation of it is exact and its order free.  err = (float)S / 14112.0f (32 * 21 * 21), one binary32 division.  Every point with
 *      status 0 gets err = 0.
 *   6. err with VSTAB_LK_GET_MIN_EIGENVALS.  err is the minEig of rule 4 of the finest level whose matrix was formed -- a level whose
 *      previous-point range test passed --, written before the rejection test, so a rejected point still reports it; 0 if no level got
 *      that far.  Status does not gate it.
 * OpenCV clamps where this library refuses.  vstab_pyr_lk_ex is refused with VSTAB_ERR_INVALID before any launch, in this order:
 * "vstab_pyr_lk_ex: bad argument" (what vstab_pyr_lk refuses); "vstab_pyr_lk_ex: max_level lies in 0 .. 3"; "vstab_pyr_lk_ex: max_iter
 * lies in 1 .. 100"; "vstab_pyr_lk_ex: eps is finite and lies in [0, 10]"; "vstab_pyr_lk_ex: min_eig_threshold is finite and not
 * negative"; "vstab_pyr_lk_ex: unknown flag"; "vstab_pyr_lk_ex: VSTAB_LK_GET_MIN_EIGENVALS needs err".
 * err: n host floats, or NULL.  With every option at its default (3, 30, 0.01, 1e-4), no flag and err == NULL the call is vstab_pyr_lk:
 * the same kernel and the same bytes. */
enum { VSTAB_LK_USE_INITIAL_FLOW = 4, VSTAB_LK_GET_MIN_EIGENVALS = 8 }; /* OpenCV's values */
VSTAB_API vstab_status vstab_pyr_lk_ex(const void *prev, size_t pitch_prev, const void *next, size_t pitch_next, int width, int height,
                                       const float *prev_xy, int n, float *next_xy, unsigned char *status, float *err /* may be NULL */,
                                       int max_level, int max_iter, double eps, double min_eig_threshold, int flags, void *stream);

/* ---- Tracker window ------------------------------------------------------------------------------------------------------------------
 * calcOpticalFlowPyrLK's winSize: a square odd window of W x W pixels, W = 15, 21 or 31.  Every other value is refused, not clamped -- even
 * sizes, other odd sizes; there is no rectangular form.  "Tracker options" rules 1 - 6 hold with W in the place of 21:
 *   Half.          half = (float)((W - 1) / 2): 7, 10 or 15.
 *   Window origin. floor(p * 2^-l - half) in float, for the previous point, an iteration's estimate and the final position alike.
 *   Range test.    The origin is tested against [-W, w_l) x [-W, h_l); NaN, infinities and values outside int fail, as in vstab_pyr_lk.
 *   Levels.        The pyramid has min(levels_W(width, height), max_level + 1) levels, at most 4.  levels_W halves with (n + 1) / 2 and stops
 *                  before the first level with w_l <= W || h_l <= W: the window sets the pyramid's depth as buildOpticalFlowPyramid does.
 *   Padding.       REFLECT_101 of both images, folded as often as it takes (a 31-pixel window on a 20-pixel image folds more than once);
 *                  derivatives outside the image are zero.
 *   minEig.        The divisor of rule 4 (and what rule 6 reports) is (float)(2 * W * W).
 *   err.           Rule 5 with f = next - half over the W * W window pixels and err = (float)S / (float)(32 * W * W); S is an integer
 *                  <= W * W * 8160 < 2^24 for W <= 31.
 *   Unchanged.     The iteration cap, eps^2, the oscillation rule's 0.01, the 2^-20 scale of the sums and the 14-bit weights.
 * With W = 21 this is "Tracker options" bit for bit.  No bit equality with OpenCV is claimed, as before.
 * vstab_pyr_lk_win takes vstab_pyr_lk_ex's arguments and win_size.  With win_size = 21 it is vstab_pyr_lk_ex: the same kernel and the same
 * bytes.  Refused with VSTAB_ERR_INVALID before any launch, in this order: "vstab_pyr_lk_win: bad argument"; "vstab_pyr_lk_win: win_size
 * is 15, 21 or 31"; then vstab_pyr_lk_ex's option and flag messages under this name, in their order. */
VSTAB_API vstab_status vstab_pyr_lk_win(const void *prev, size_t pitch_prev, const void *next, size_t pitch_next, int width, int height,
                                        const float *prev_xy, int n, float *next_xy, unsigned char *status, float *err /* may be NULL */,
                                        int max_level, int max_iter, double eps, double min_eig_threshold, int flags, int win_size, void *stream);

/* ------------------------------------------------------------------------------------------
 * Host-side motion model.
 * ------------------------------------------------------------------------------------------ */

/* Replaces guess_camera_rotation, FrameSourceWarp.cpp:316-375: undistort both point sets, random
 * depths (seeded PCG32 instead of the reference's un-seeded rand()), PnP-RANSAC (100 iterations,
 * 8 px, 0.99), Rodrigues.  prev_xy/cur_xy: n (x,y) float pairs in input pixels.  R: row-major
 * rotation since the last frame; *inliers: RANSAC inlier count (the reference's return value). */
VSTAB_API vstab_status vstab_estimate_rotation(const float *prev_xy, const float *cur_xy, int n,
                                               const double K_in[9], const double K_out[9],
                                               uint64_t seed, double R[9], int *inliers);

/* Savitzky-Golay weights of gram_sg::SavitzkyGolayFilterConfig(m, 0, 2, 0) (:212): 2m+1 doubles. */
VSTAB_API vstab_status vstab_sg_weights(int m, double *weights);

/* gram_sg::RotationFilter replacement (:212,444,459,471): ring of 2m+1 matrices that starts
 * zero-filled; filter() = polar factor U*V^T of the weighted sum. */
typedef struct vstab_rotation_filter vstab_rotation_filter;
VSTAB_API vstab_status vstab_rotation_filter_create(int m, vstab_rotation_filter **out);
VSTAB_API vstab_status vstab_rotation_filter_add(vstab_rotation_filter *f, const double R[9]);
VSTAB_API vstab_status vstab_rotation_filter_filter(const vstab_rotation_filter *f, double R_out[9]);
VSTAB_API void vstab_rotation_filter_destroy(vstab_rotation_filter *f);

/* Gyro samples -> the per-frame rotations the pipeline takes from an external sensor (vstab_frame.delta_rotation,
 * vstab_frame.readout_rotation): the step the reference stubbed (gpmf.cpp:5-11 declares GyroFrame {start_ts, end_ts, roll,
 * pitch, yaw} and the commented-out reader fills one per GPMF "GYRO" sample; AvFrameSourceFileVaapi.cpp:121-123 "TODO process
 * GPMF packet").  vstab_gyro_sample IS that record: an angular rate held from start_ts to end_ts (seconds on the clock the
 * frame timestamps use), about the camera's z (roll), x (pitch) and y (yaw) axes, x right, y down, z along the optical axis.
 * Over an interval [a, b] the rotation is the ordered product of exponential maps, later samples on the left (the
 * accumulation order of FrameSourceWarp.cpp:441):
 *     R(a, b) = exp([w_n] dt_n) ... exp([w_1] dt_1),   w_i = rate_scale * (pitch_i, yaw_i, roll_i),
 *     dt_i = length of [start_ts_i, end_ts_i] inside [a, b]   (time not covered by any sample contributes nothing).
 * rate_scale = -1 for a gyro that reports the rate of the camera BODY in rad/s (points of the scene then move by R in camera
 * coordinates, which is what guess_camera_rotation returns); it also absorbs unit conversion (-pi/180 for deg/s).
 * R_delta = R(t_prev_first_row, t_first_row): the camera's rotation since the previous frame; R_readout =
 * R(t_first_row, t_last_row): its rotation during this frame's read-out (rolling shutter).  Either may be NULL.  Samples
 * must be ordered by start_ts with end_ts >= start_ts.  fp64, host only.  GPMF container parsing (gpmf-parser) stays upstream. */
typedef struct vstab_gyro_sample {
    double start_ts, end_ts, roll, pitch, yaw; /* field order of the reference's GyroFrame */
} vstab_gyro_sample;
VSTAB_API vstab_status vstab_gyro_integrate(const vstab_gyro_sample *samples, int n, double rate_scale,
                                            double t_prev_first_row, double t_first_row, double t_last_row,
                                            double R_delta[9], double R_readout[9]);

/* GPMF payload -> gyro samples: the reader the reference sketched and left commented out (opencv/gpmf.cpp:33-114, with gpmf-parser;
 * AvFrameSourceFileVaapi.cpp:121-123 "TODO process GPMF packet").  payload / n: one packet of the camera's metadata stream as the
 * demuxer hands it over; pkt_ts / pkt_dur: the packet's time stamp and duration in seconds (AVPacket.pts / .duration times the
 * stream's time base).  GoPro's published KLV layout is walked directly (no gpmf-parser): items of {FourCC key, type character,
 * structure size (1 byte), repeat count (2 bytes)} + repeat * size bytes, everything big-endian and padded to four bytes; type 0
 * nests (DEVC > STRM > items).  Inside a stream, SCAL holds the divisor -- one for all elements or one per element -- that turns
 * the raw GYRO integers (type 's', three per sample; 'S' 'l' 'L' 'b' 'B' 'f' 'd' are accepted too) into rad/s.  As gpmf.cpp:95-101
 * intends, a block's samples share the packet's span evenly -- sample i of m: start_ts = pkt_ts + pkt_dur * i / m, end_ts = start_ts
 * + pkt_dur / m -- and elements 0, 1, 2 go to roll, pitch, yaw: the order GoPro documents for HERO5 and later, Z (the optical axis),
 * X (to the right), Y (downwards), which is vstab_gyro_sample's convention.  The result feeds vstab_gyro_integrate (rate_scale = -1
 * for these body rates).  Up to `cap` samples are written to out; *n_out = the number found (call again with a larger buffer if it
 * exceeds cap).  Every GYRO block of the payload is taken, in order.  VSTAB_ERR_INVALID for a payload that is not well formed: an
 * item that runs past its container, a truncated header, nesting deeper than eight levels, a GYRO block that does not have three
 * elements per sample, a SCAL of zero or not finite, a packet time stamp or duration that is not finite.  Host only; reads nothing
 * outside [payload, payload + n). */
VSTAB_API vstab_status vstab_gpmf_parse_gyro(const void *payload, size_t n, double pkt_ts, double pkt_dur, vstab_gyro_sample *out, int cap,
                                             int *n_out);

/* A map that does not change between frames (tracking off: undistort only, the CLI's stab=none re-projections) need
 * not be evaluated per frame as the reference does (FrameSourceWarp.cpp:283-304): vstab_quantised_map writes, once,
 * what cv::remap makes of every map entry (32 * map rounded to int; vstab_quantised_map_bytes() bytes, 16-byte aligned
 * device memory), and vstab_warp_nv12_mapped warps with it -- same integers, same pixels as vstab_warp_nv12_ex. */
VSTAB_API size_t vstab_quantised_map_bytes(int dst_width, int dst_height);
VSTAB_API vstab_status vstab_quantised_map(void *qmap, int dst_width, int dst_height, const float params[17],
                                           int map_mode, void *stream);
VSTAB_API vstab_status vstab_warp_nv12_mapped(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv,
                                              int src_width, int src_height, const void *qmap, int out_format,
                                              void *dst, size_t pitch_dst, void *dst_uv, size_t pitch_dst_uv,
                                              int dst_width, int dst_height, void *stream);

/* The `debug` overlay of the filter surface (render.ts:678): a filled (2*half+1)^2 square of colour bgr (0x00RRGGBB;
 * the low byte alone for a 1-channel plane) at each of n centres (x, y int pairs in DEVICE memory), clipped. */
VSTAB_API vstab_status vstab_draw_markers(void *dst, size_t pitch, int width, int height, int channels,
                                          const int *centres_xy_device, int n, int half, unsigned int bgr,
                                          void *stream);

/* ------------------------------------------------------------------------------------------
 * Lens distortion: OpenCV's fisheye (Kannala-Brandt) model on the INPUT camera, the `distortion_coefficients` k1 .. k4 the reference's
 * Camera carries (FrameSourceWarp.hpp) and hands to every fisheye::undistortPoints call:
 *   theta_d = theta (1 + k1 theta^2 + k2 theta^4 + k3 theta^6 + k4 theta^8),   image radius = f theta_d.
 * All zero is the ideal equidistant lens of every other entry point, bit for bit.  dist / D: the four coefficients, floats in the device
 * operators (like params), doubles in the host functions.
 *   map     the operations of map modes 1 / 2 (VSTAB_MAP_FISH_TO_RECT / _FISH_TO_FISH) up to theta = atan(rad); then, every operation
 *           an IEEE binary32 operation of its own (nothing fused):
 *             s2 = theta * theta;  g = k4;  g = g * s2 + k3;  g = g * s2 + k2;  g = g * s2 + k1;  theta_d = theta * (1 + g * s2);
 *           and k = theta_d / rad (1 on the axis), map = centre + (p * k) * focal; outside (NaN) exactly where modes 1 / 2 are.
 *           tests/distort_def.py states it in numpy, tests/golden/distort_kat.npz pins it.
 *   points  OpenCV 4.5's fisheye::undistortPoints: theta_d clipped to pi/2; Newton from theta = theta_d with
 *           fix = (theta (1 + k1 theta^2 + ...) - theta_d) / (1 + 3 k1 theta^2 + 5 k2 theta^4 + 7 k3 theta^6 + 9 k4 theta^8), at most 10
 *           steps, stop at |fix| < 1e-8; scale = tan(theta) / theta_d; a point that did not converge, or whose theta changed sign, becomes
 *           (-1e6, -1e6).
 * Accepted coefficients: all four finite, and 1 + 3 k1 theta^2 + 5 k2 theta^4 + 7 k3 theta^6 + 9 k4 theta^8 > 0 at the 1025 points
 * theta = i (pi/2) / 1024 (fp64): theta_d must increase on [0, pi/2] -- the warp kernels bound a tile's source box by the map on the tile's
 * perimeter, which holds for a map that does not fold.  Anything else is VSTAB_ERR_INVALID ("the distortion must keep theta_d increasing
 * on [0, pi/2]"), from every entry point below.  map_mode: VSTAB_MAP_FISH_TO_RECT or VSTAB_MAP_FISH_TO_FISH; any other is
 * VSTAB_ERR_INVALID ("distortion belongs to a fisheye input (map modes 1 and 2)").
 * Served with distortion: INTER_LINEAR with the constant border (vstab_warp_nv12_dist), and every 8-bit resampler with every border mode as
 * a fused kernel (vstab_warp_nv12_dist_ex).  Not served with distortion: the output camera, the rotation per output row, 10-bit planes,
 * INTER_NEAREST, and NV12 through BGR -- the stateless vstab_remap_* operators take the planes of vstab_create_map_dist.
 * ------------------------------------------------------------------------------------------ */
/* vstab_fisheye_undistort_points through the distorted lens. */
VSTAB_API vstab_status vstab_fisheye_undistort_points_d(const double *pts, int n, const double K[9], const double D[4], const double *R,
                                                        const double *P, double *out);
/* vstab_estimate_rotation with the input lens's coefficients: both point sets are undistorted with D. */
VSTAB_API vstab_status vstab_estimate_rotation_d(const float *prev_xy, const float *cur_xy, int n, const double K_in[9], const double K_out[9],
                                                 const double D[4], uint64_t seed, double R[9], int *inliers);
/* vstab_create_map_ex / vstab_quantised_map with the polynomial. */
VSTAB_API vstab_status vstab_create_map_dist(void *map_x, size_t pitch_x, void *map_y, size_t pitch_y, int cols, int rows, const float params[17],
                                             const float dist[4], int map_mode, void *stream);
VSTAB_API vstab_status vstab_quantised_map_dist(void *qmap, int dst_width, int dst_height, const float params[17], const float dist[4], int map_mode,
                                                void *stream);
/* vstab_warp_nv12_ex with the polynomial: the LDS-tiled kernels of modes 1 / 2 (small or unaligned sources: their gather path).
 * out_format: VSTAB_OUT_BGR8 or VSTAB_OUT_NV12_PLANAR; VSTAB_OUT_NV12 (through BGR) and any other value are refused with
 * VSTAB_ERR_INVALID.  Arguments are checked as vstab_warp_nv12_cubic checks them and in its order, except the map mode: it is checked
 * behind all of them (pointers, sizes, output format, pitches, chroma alignment), then the coefficients, last. */
VSTAB_API vstab_status vstab_warp_nv12_dist(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int src_width, int src_height,
                                            const float params[17], const float dist[4], int map_mode, int out_format, void *dst, size_t pitch_dst,
                                            void *dst_uv, size_t pitch_dst_uv, int dst_width, int dst_height, void *stream);
/* vstab_warp_nv12_dist for every 8-bit resampler and border mode.  resample: VSTAB_RESAMPLE_DEFAULT (INTER_LINEAR), _CUBIC or _LANCZOS4;
 * border_mode: VSTAB_BORDER_CONSTANT, _REPLICATE, _REFLECT or _REFLECT_101; map_mode: 1 or 2; out_format: VSTAB_OUT_BGR8 or
 * VSTAB_OUT_NV12_PLANAR.  Nothing new is defined: the frame is the map of "Lens distortion" above (tests/distort_def.py: maps) fed to the
 * resampler's own definition -- vstab_warp_nv12_cubic / _lanczos4 (tests/warp_def.py: remap, bgr and planar),
 * vstab_warp_nv12_border and the border modes of the cubic and Lanczos resamplers (the same remap with another border_mode).
 * DEFAULT with CONSTANT is vstab_warp_nv12_dist itself, same bytes; DEFAULT with another mode runs vstab_warp_nv12_border's tile kernel,
 * CUBIC / LANCZOS4 the resampler's tile kernel for that border, each with the distorted map: the tile's source box is the exact
 * reduction over the tile's own map, as without distortion.  The quantised map (vstab_quantised_map_dist) serves DEFAULT + CONSTANT only.
 * Every refusal is VSTAB_ERR_INVALID, made before any device work, in this order, each message behind "vstab_warp_nv12_dist_ex: ":
 *   1. dist NULL: "null pointer";
 *   2. vstab_warp_nv12_cubic_border's checks in its order: "null pointer" (y, uv, dst, params), "source must be even-sized and <= 32767",
 *      "output size must be in [1, 32767]", "the distorted-lens warp emits VSTAB_OUT_BGR8 or VSTAB_OUT_NV12_PLANAR (NV12 through BGR is
 *      not served)", "border_mode must be VSTAB_BORDER_CONSTANT (0), _REPLICATE (1), _REFLECT (2) or _REFLECT_101 (4)", "pitch smaller
 *      than row", "plane-wise output needs a chroma plane of 2*ceil(width/2) bytes per row", "chroma plane must be 2-B aligned";
 *   3. "resample must be VSTAB_RESAMPLE_DEFAULT (0), _CUBIC (2) or _LANCZOS4 (4)";
 *   4. every map mode but 1 and 2, known or not: "distortion belongs to a fisheye input (map modes 1 and 2)";
 *   5. "the distortion must keep theta_d increasing on [0, pi/2]". */
VSTAB_API vstab_status vstab_warp_nv12_dist_ex(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int src_width, int src_height,
                                               const float params[17], const float dist[4], int map_mode, int resample, int border_mode,
                                               int out_format, void *dst, size_t pitch_dst, void *dst_uv, size_t pitch_dst_uv, int dst_width,
                                               int dst_height, void *stream);
/* The whole 8-bit surface behind one call: a rotation per output row (rot_bottom, as vstab_warp_nv12_rs; NULL: one rotation), a
 * calibrated lens (dist = k1..k4; NULL: the ideal lens), a resampler (VSTAB_RESAMPLE_DEFAULT, _CUBIC, _LANCZOS4), a border mode
 * (VSTAB_BORDER_*), out_format VSTAB_OUT_BGR8 or VSTAB_OUT_NV12_PLANAR.  Nothing new is defined: the frame is the map fed to the
 * resampler's own definition (tests/warp_def.py: maps).  The map without dist: map_mode's, row y with the rotation
 * m_k = fmaf(t, rot_bottom[k] - params[8 + k], params[8 + k]), t = (float)y / (float)max(dst_height - 1, 1) (IEEE), for map modes 0, 1
 * and 5.  With dist: the map of "Lens distortion" above, modes 1 and 2 without rot_bottom, mode 1 with it, the row's m in place of the
 * rotation.  Chroma from map(2cx, 2cy) * 0.5f over the chroma plane's own size, as everywhere else.
 * Where an older entry point serves the combination the call is that entry point's launch, same bytes: vstab_warp_nv12_ex, _cubic[_border],
 * _lanczos4[_border], _border (no rot_bottom, no dist); vstab_warp_nv12_dist_ex (dist alone); vstab_warp_nv12_border (DEFAULT with
 * rot_bottom).  CUBIC / LANCZOS4 with rot_bottom run k_warp_cubic_rs / k_warp_lanczos4_rs, DEFAULT with dist and rot_bottom k_warp_border.
 * Every refusal is VSTAB_ERR_INVALID, made before any device work, in this order, each message behind "vstab_warp_nv12_rs_ex: ":
 *   1. vstab_warp_nv12_border's checks in its order: "null pointer" (y, uv, dst, params), "source must be even-sized and <= 32767", "output
 *      size must be in [1, 32767]", "unknown map mode", "a rotation per output row (rot_bottom) is served for map modes 0, 1 and 5", "the
 *      per-row warp emits VSTAB_OUT_BGR8 or VSTAB_OUT_NV12_PLANAR (NV12 through BGR is not served)", "border_mode must be
 *      VSTAB_BORDER_CONSTANT (0), _REPLICATE (1), _REFLECT (2) or _REFLECT_101 (4)", "pitch smaller than row", "plane-wise output needs a
 *      chroma plane of 2*ceil(width/2) bytes per row", "chroma plane must be 2-B aligned";
 *   2. "resample must be VSTAB_RESAMPLE_DEFAULT (0), _CUBIC (2) or _LANCZOS4 (4)";
 *   3. with dist: "distortion belongs to a fisheye input (map modes 1 and 2)", then "the distortion must keep theta_d increasing on
 *      [0, pi/2]". */
VSTAB_API vstab_status vstab_warp_nv12_rs_ex(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int src_width, int src_height,
                                             const float params[17], const float *rot_bottom, const float *dist, int map_mode, int resample,
                                             int border_mode, int out_format, void *dst, size_t pitch_dst, void *dst_uv, size_t pitch_dst_uv,
                                             int dst_width, int dst_height, void *stream);

/* ------------------------------------------------------------------------------------------
 * Pinhole lens distortion: OpenCV's Brown-Conrady model on a RECTILINEAR input camera (in_projection VSTAB_PROJ_RECT, map modes 3 and 4),
 * the (k1, k2, p1, p2, k3) of cv::calibrateCamera, in that order.  All zero is the ideal pinhole of every other entry point.  dist / D: the
 * five coefficients, floats in the device operators (like params), doubles in the host functions.
 *   map     the operations of map modes 3 / 4 (VSTAB_MAP_RECT_TO_RECT / _RECT_TO_FISH) up to x = wx / wz, y = wy / wz; then, every
 *           operation an IEEE binary32 operation of its own (nothing fused):
 *             xx = x * x;  yy = y * y;  xy = x * y;  r2 = xx + yy;
 *             g = k3;  g = g * r2 + k2;  g = g * r2 + k1;  rad = 1 + g * r2;
 *             a = 2 * xy;  dx = p1 * a + p2 * (r2 + 2 * xx);  dy = p1 * (r2 + 2 * yy) + p2 * a;
 *             xd = x * rad + dx;  yd = y * rad + dy;
 *           and map = centre + (xd, yd) * focal; outside (NaN) exactly where modes 3 / 4 are (wz <= 0; mode 4: rho >= pi).  Infinities
 *           and NaN the polynomial produces far off the axis are quantised as everywhere (cvRound: INT_MIN, outside the source).
 *           tests/pinhole_def.py states it in numpy, tests/golden/pinhole_kat.npz pins it.
 *   points  OpenCV 4.5's cv::undistortPoints with its default criteria: x0 = (u - cx) / fx, y0 = (v - cy) / fy, start at (x0, y0), exactly
 *           five steps and no epsilon test:
 *             r2 = x x + y y;  icdist = 1 / (1 + ((k3 r2 + k2) r2 + k1) r2);  icdist < 0: (x, y) = (x0, y0), stop;
 *             dX = 2 p1 x y + p2 (r2 + 2 x x);  dY = p1 (r2 + 2 y y) + 2 p2 x y;  x = (x0 - dX) icdist;  y = (y0 - dY) icdist;
 *           then R and P as vstab_fisheye_undistort_points applies them.
 * Accepted coefficients: all five finite, in fp64 and after the cast to fp32.  Anything else is VSTAB_ERR_INVALID ("the five distortion
 * coefficients must be finite").  There is no monotonicity rule (OpenCV has none): the kernels that serve these modes take a tile's source
 * box as the exact reduction over the tile's own map, which needs no monotone map.  map_mode: VSTAB_MAP_RECT_TO_RECT or
 * VSTAB_MAP_RECT_TO_FISH; any other is VSTAB_ERR_INVALID ("pinhole distortion belongs to a rectilinear input (map modes 3 and 4)").
 * Not served: 10-bit planes, a rotation per output row, the keep-edge warp, the quantised map, INTER_NEAREST, NV12 through BGR, the
 * rational and thin-prism terms (k4..k6, s1..s4), a distorted output camera.
 * ------------------------------------------------------------------------------------------ */
/* cv::undistortPoints(pts, K, D, R, P) as stated above.  R, P: NULL = identity.  "bad argument" for a NULL pts / K / D / out or n < 0. */
VSTAB_API vstab_status vstab_undistort_points_pinhole(const double *pts, int n, const double K[9], const double D[5], const double *R,
                                                      const double *P, double *out);
/* vstab_estimate_rotation for a rectilinear input lens with D: both point sets are undistorted as above.  D = 0: the estimate a
 * rectilinear pipeline handle makes without a calibration. */
VSTAB_API vstab_status vstab_estimate_rotation_pinhole(const float *prev_xy, const float *cur_xy, int n, const double K_in[9], const double K_out[9],
                                                       const double D[5], uint64_t seed, double R[9], int *inliers);
/* vstab_create_map_ex of modes 3 / 4 with the polynomial.  Checked in this order: "null pointer", "size must be in [1, 32767]
 * (createMap.cl:10-11)", "bad pitch", the map mode, the coefficients. */
VSTAB_API vstab_status vstab_create_map_pinhole(void *map_x, size_t pitch_x, void *map_y, size_t pitch_y, int cols, int rows, const float params[17],
                                                const float dist[5], int map_mode, void *stream);
/* The warp through the distorted rectilinear lens, every 8-bit resampler and border mode.  resample: VSTAB_RESAMPLE_DEFAULT (INTER_LINEAR),
 * _CUBIC or _LANCZOS4; border_mode: VSTAB_BORDER_CONSTANT, _REPLICATE, _REFLECT or _REFLECT_101; map_mode: 3 or 4; out_format:
 * VSTAB_OUT_BGR8 or VSTAB_OUT_NV12_PLANAR.  Nothing new is defined behind the map: the frame is the map above (tests/pinhole_def.py: maps)
 * fed to the resampler's own definition, as for vstab_warp_nv12_dist_ex.  DEFAULT runs vstab_warp_nv12_border's tile kernel (the constant
 * border included), CUBIC / LANCZOS4 the tile kernels that vstab_warp_nv12_rs_ex runs for them, each with the distorted map and one
 * rotation.  With dist all zero the call is the older entry point's launch, same bytes: vstab_warp_nv12_ex, _border, _cubic[_border] or
 * _lanczos4[_border].
 * Every refusal is VSTAB_ERR_INVALID, made before any device work, in this order, each message behind "vstab_warp_nv12_pinhole: ":
 *   1. dist NULL: "null pointer";
 *   2. vstab_warp_nv12_cubic_border's checks in its order: "null pointer" (y, uv, dst, params), "source must be even-sized and <= 32767",
 *      "output size must be in [1, 32767]", "the pinhole-lens warp emits VSTAB_OUT_BGR8 or VSTAB_OUT_NV12_PLANAR (NV12 through BGR is
 *      not served)", "border_mode must be VSTAB_BORDER_CONSTANT (0), _REPLICATE (1), _REFLECT (2) or _REFLECT_101 (4)", "pitch smaller
 *      than row", "plane-wise output needs a chroma plane of 2*ceil(width/2) bytes per row", "chroma plane must be 2-B aligned";
 *   3. "resample must be VSTAB_RESAMPLE_DEFAULT (0), _CUBIC (2) or _LANCZOS4 (4)";
 *   4. every map mode but 3 and 4, known or not: "pinhole distortion belongs to a rectilinear input (map modes 3 and 4)";
 *   5. "the five distortion coefficients must be finite". */
VSTAB_API vstab_status vstab_warp_nv12_pinhole(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int src_width, int src_height,
                                               const float params[17], const float dist[5], int map_mode, int resample, int border_mode,
                                               int out_format, void *dst, size_t pitch_dst, void *dst_uv, size_t pitch_dst_uv, int dst_width,
                                               int dst_height, void *stream);

/* ------------------------------------------------------------------------------------------
 * The pipeline object: drop-in for FrameSourceWarp behind the FrameSource pull interface
 * (FrameSource.hpp:9-24, FrameSourceWarp.hpp:83-91).
 * ------------------------------------------------------------------------------------------ */

/* One NV12 frame handed over by the upstream source (what FrameSourceFfmpegOpenCl produces,
 * FrameSourceFfmpegOpenCl.cpp:58-85).  A packed (h*3/2 x w) buffer is uv = y + pitch_y*height.
 * By default the planes only need to stay valid until the callback is called again (see `hold`) or the
 * handle is destroyed: the library copies them into its own HBM ring. */
typedef struct vstab_frame {
    const void *y;
    const void *uv;
    size_t pitch_y, pitch_uv;
    int width, height; /* luma size; both even */
    int mem;           /* 0 = device memory, 1 = host memory, 2 (VSTAB_MEM_DMABUF) = a DMA-BUF: see dmabuf_fd below */
    int64_t pts;
    const double *delta_rotation; /* optional (NULL = none): 3x3 row-major rotation of the camera since the previous
                          frame from an external sensor -- the gyro path the reference stubs (gpmf.cpp:5-11,
                          AvFrameSourceFileVaapi.cpp:121-123).  Used in place of the optical-flow
                          estimate (guess_camera_rotation's return value, FrameSourceWarp.cpp:429) when
                          vstab_config.tracking == 0; read during the callback only. */
    int bit_depth;     /* 0 or 8: 8-bit NV12.  10 / 12 / 16: P010-style planes (16-bit little-endian samples, significant
                          bits at the top, pitches in bytes), narrowed to 8 bits on ingest (vstab_pack_p010). */
    int hold;          /* how many FURTHER pull callbacks these planes stay valid and unchanged for.  0 (default): only
                          until the next callback -- the library then waits for its copy of this frame to finish before
                          it calls upstream again (a decoder that recycles one output surface).  Ref-counted or pooled
                          frames can say how deep the pool is and the wait disappears from the frame loop.  From
                          smooth_radius + read_ahead + 6 on (smooth_radius + 18 with the default read-ahead of twelve), the
                          planes are not copied at all but read in place by the tracker and
                          by the warp (which runs on vstab_config.stream): the callback at which the promise runs out
                          first waits, on the host, for that warp to finish.  1 << 29 or more: never waited for.
                          That threshold is the 8-BIT rule.  16-bit (P010) frames are always narrowed into library
                          memory for the tracker; their own planes are read in place by the 10-bit warp only with
                          hold >= 1 << 29 (the promise has to cover a warp that runs smooth_radius frames later, and
                          finite promises are not tracked for them) -- anything less and they are copied on ingest. */
    const double *readout_rotation; /* optional (NULL = global shutter): 3x3 row-major rotation of the camera between the
                          exposure of this frame's first and last row (rolling shutter, from the same sensor as
                          delta_rotation; BASELINE.json config 5).  The frame is then warped with a rotation per output row:
                          the stabilising rotation W for the first row, readout_rotation * W for the last, matrix entries
                          interpolated in between (vstab_warp_nv12_rs; preset and fisheye -> rectilinear maps only).  Read
                          during the callback only. */
    int dmabuf_fd;     /* mem == VSTAB_MEM_DMABUF: the frame lives in a DMA-BUF object -- what a VAAPI / AMF decoder surface is
                          once exported (av_hwframe_map(..., AV_PIX_FMT_DRM_PRIME) -> AVDRMFrameDescriptor: objects[0].fd /
                          .size, layers[].planes[].offset / .pitch).  `y` and `uv` are then BYTE OFFSETS of the two planes
                          inside the object (cast to pointers), pitch_y / pitch_uv as usual.  The library imports the object
                          into the HIP address space (hipImportExternalMemory; cached per object, the fd is not consumed and
                          may be closed after the callback) and uses the planes as device memory under the `hold` rules above:
                          the zero-copy replacement of the reference's VAAPI -> host -> OpenCL double copy
                          (AvFrameSourceMapOpenCl.cpp:17-66).  Ignored for other `mem` values. */
    size_t dmabuf_size; /* size of the object in bytes (AVDRMObjectDescriptor.size) */
    uint64_t dmabuf_modifier; /* AVDRMObjectDescriptor.format_modifier of the object: how its bytes are arranged.  The kernels read
                          rows of `pitch` bytes, so only DRM_FORMAT_MOD_LINEAR (0) is accepted -- and DRM_FORMAT_MOD_INVALID
                          (0x00ffffffffffffff: "no modifier given", which libav reports for implicit-layout exports; such a surface
                          is the exporter's to keep linear).  Any other value (a tiled / compressed surface) is refused with
                          VSTAB_ERR_UNSUPPORTED instead of being read as garbage: map the surface linear (hwmap) first. */
} vstab_frame;
#define VSTAB_DRM_FORMAT_MOD_LINEAR 0ull
#define VSTAB_DRM_FORMAT_MOD_INVALID 0x00ffffffffffffffull
enum { VSTAB_MEM_DEVICE = 0, VSTAB_MEM_HOST = 1, VSTAB_MEM_DMABUF = 2 };

/* Upstream FrameSource (FrameSource.hpp:14,20): return 0 and fill *out, VSTAB_EOF (-1) at end of
 * stream, any other value on failure (propagated as VSTAB_ERR_SOURCE, like a rethrown int). */
typedef struct vstab_source {
    int (*pull)(void *user, vstab_frame *out);
    int (*peek)(void *user, vstab_frame *out);
    void *user;
} vstab_source;

/* SG = the reference (gram_sg, FrameSourceWarp.cpp:212); NONE = no correction (libdewobble stab=none with tracking on);
 * FIXED = hold the first frame's orientation (libdewobble stab=fixed, render.ts:676); KALMAN = opencv/kalman constants. */
enum { VSTAB_SMOOTHER_SG = 0, VSTAB_SMOOTHER_KALMAN = 1, VSTAB_SMOOTHER_NONE = 2, VSTAB_SMOOTHER_FIXED = 3 };

/* Lens description of the CLI's libdewobble filter (render.ts:611-617,669-683): projection + diagonal field of view. */
typedef enum vstab_projection { VSTAB_PROJ_RECT = 0, VSTAB_PROJ_FISH = 1 } vstab_projection;
/* Camera matrix of such a lens: f = (d/2)/tan(dfov/2) (rect) or (d/2)/(dfov/2) (fish, equidistant), d = the image
 * diagonal in pixels; principal point (cx, cy), negative = the image centre (width/2, height/2) as render.ts:682-683. */
VSTAB_API vstab_status vstab_lens_camera(int projection, double dfov_deg, int width, int height, double cx,
                                         double cy, double K[9]);

/* Constructor arguments of FrameSourceWarp (FrameSourceWarp.hpp:83-91) plus what the reference
 * hard-codes.  vstab_config_default fills the reference's defaults. */
typedef struct vstab_config {
    int abi_version;     /* VSTAB_ABI_VERSION, written by vstab_config_default; vstab_create refuses anything else */
    int preset;          /* vstab_camera_preset */
    double scale;        /* 1 */
    int crop_borders;    /* 0 */
    double zoom;         /* 1 */
    int smooth_radius;   /* 30.  >= 1 is the reference's filter; 0 (where gram_sg's weights divide by zero) is defined here as
                            "no smoothing": the single weight is 1 and every frame is warped by the identity correction */
    int interpolation;   /* cv::InterpolationFlags: 1 = INTER_LINEAR (the only mode the reference ever passes), 0 = INTER_NEAREST
                            (lens_mode 0, 8-bit BGR output, no read-out rotations); others are refused */
    int smoother;        /* VSTAB_SMOOTHER_SG (reference behaviour) */
    int tracking;        /* 1; 0 = no optical flow: rotations are identity (BASELINE config 1: undistort only) or the
                            upstream-supplied vstab_frame.delta_rotation (external gyro), smoothed the same way */
    uint64_t seed;       /* PCG32 seed replacing the reference's un-seeded rand() */
    void *stream;        /* hipStream_t the warp (and so dst) is enqueued on; NULL = default stream.  Ingest and
                            tracking run on internal streams that overlap it; ordering is by events.  The runtime has
                            four hardware queues per process: beside a NULL stream the handle creates three streams
                            (tracking, read-ahead, speculative corner detection), beside a stream of the caller's two
                            (the detection then queues on the read-ahead stream; VSTAB_DETECT_STREAM=1 in the
                            environment gives it its own) -- INTEGRATION.md section 3. */
    /* libdewobble-style lens surface.  lens_mode 0 (default) = the reference's preset cameras
     * and createMap.cl; 1 = the fields below replace preset / scale / crop_borders / zoom. */
    int lens_mode;
    int in_projection;   /* in_p: vstab_projection */
    int out_projection;  /* out_p */
    double in_dfov;      /* in_dfov, degrees, (0, 360) for fish and (0, 180) for rect */
    double out_dfov;     /* out_dfov; 0 = in_dfov (render.ts:673) */
    int out_width;       /* out_w; 0 = input width (render.ts:678) */
    int out_height;      /* out_h; 0 = input height */
    double out_cx;       /* out_fx "focal point"; negative = out_width / 2 (render.ts:682) */
    double out_cy;       /* out_fy; negative = out_height / 2 */
    int debug;           /* debug (render.ts:678): mark the features tracked into each emitted frame (green 7x7 squares;
                            luma 235 in NV12 output) at the positions the warp sends them to.  Works in both lens modes. */
    int pixel_depth;     /* 8 (default, 0 = 8): the reference's 8-bit path; P010 input is narrowed on ingest.  10 (BASELINE.json
                            config 5): upstream must hand P010 device frames (vstab_frame.bit_depth > 8); the tracker runs on
                            the narrowed luma exactly as in the 8-bit path, the frame is warped from the 16-bit planes with
                            vstab_warp_p010 and emitted by vstab_pull_frame_bgr16. */
    int blend;           /* pixel_depth 10: VSTAB_BLEND_EXACT (default) or VSTAB_BLEND_FP16 */
    int read_ahead;      /* frames the library pulls from upstream AHEAD of the frame it returns, beyond smooth_radius: 0 = the default
                            (12), else 1 .. 16.  The read-ahead is what lets copy, pyramid, corner detection and tracking overlap the
                            host's work; every output is identical for any value.  A live source sees a latency of
                            smooth_radius + read_ahead + 2 frames (the reference: smooth_radius) -- a capture pipeline that cares
                            lowers it (1: 30 + 3 frames at the reference's radius) and pays in frames/s. */
    int map_precision;   /* lens_mode 0: VSTAB_MAP_PRECISION_OPENCL (default; VSTAB_MAP_CREATEMAP_CL_OPENCL: the arithmetic the reference's
                            own kernel -- createMap.cl through ROCm's OpenCL compiler -- has on this GPU, bit-identical to it) or
                            VSTAB_MAP_PRECISION_IEEE (createMap.cl with every operation IEEE-rounded: reproducible by a CPU, a few
                            output bytes per frame away from the reference's GPU result).  Every path of the
                            handle honours it: cached map (tracking off), read-out rotations, INTER_NEAREST, pixel_depth 10.
                            lens_mode 1 ignores it (those maps are this library's own definitions, IEEE throughout). */
    int resample;        /* VSTAB_RESAMPLE_DEFAULT (0): `interpolation` decides, as before.  VSTAB_RESAMPLE_CUBIC (2 = cv::INTER_CUBIC): every
                            8-bit BGR and plane-wise NV12 pull warps with vstab_warp_nv12_cubic (both lens modes, both map precisions, tracking
                            on or off); rotations, frame log and look-ahead are those of the default.  Needs interpolation = 1 and 8-bit
                            pixels (vstab_create refuses it with INTER_NEAREST or pixel_depth 10).  At pull time the NV12-through-BGR
                            pull is refused before any frame is taken (the frame can still be pulled in a served format); a frame
                            that carries a readout_rotation is refused and consumed, as with INTER_NEAREST.  (A separate field: `interpolation` keeps refusing 2.)
                            VSTAB_RESAMPLE_LANCZOS4 (4 = cv::INTER_LANCZOS4): the same, with vstab_warp_nv12_lanczos4 (`interpolation` refuses 4). */
} vstab_config;
enum { VSTAB_MAP_PRECISION_IEEE = 0, VSTAB_MAP_PRECISION_OPENCL = 1 };
enum { VSTAB_RESAMPLE_DEFAULT = 0, VSTAB_RESAMPLE_CUBIC = 2, VSTAB_RESAMPLE_LANCZOS4 = 4 };

typedef struct vstab_handle vstab_handle;

VSTAB_API void vstab_config_default(vstab_config *cfg);
/* FrameSourceWarp::FrameSourceWarp (:199-226): peeks the first upstream frame for the size,
 * derives both cameras, allocates the look-ahead ring in HBM. */
VSTAB_API vstab_status vstab_create(const vstab_config *cfg, const vstab_source *src, vstab_handle **out);
VSTAB_API vstab_status vstab_get_output_info(const vstab_handle *h, int *width, int *height,
                                             double K_in[9], double K_out[9]);
/* FrameSourceWarp::pull_frame (:452-476): consumes upstream frames until smooth_radius+1 are
 * buffered (or EOF), then warps the oldest buffered frame into dst (device BGR8).  Returns
 * VSTAB_EOF when the stream is drained.  The first input frame is never emitted (:403-407).
 * dst is complete once vstab_config.stream is synchronised.  Upstream frames handed to the callbacks
 * must already be complete in memory when the callback returns (they are read on an internal stream).
 * Read-ahead: to overlap copy, pyramid, corner detection and tracking with the host work, the library pulls
 * upstream up to vstab_config.read_ahead + 2 (by default fourteen) frames earlier than the reference's loop would (same frames,
 * same order, same outputs). */
VSTAB_API vstab_status vstab_pull_frame(vstab_handle *h, void *dst_bgr, size_t pitch_dst);
/* The consumer's loop (DisplayImage.cpp:60-70: `while (true) { frame = source.pull_frame(); ... }`) as one call: n consecutive
 * vstab_pull_frame calls, frame i into dst[(first + i) % n_dst] with pitch[(first + i) % n_dst] -- an encoder's ring of output
 * surfaces.  Stops at the first call that does not return VSTAB_OK and returns its status (VSTAB_EOF at end of stream);
 * *n_done (may be NULL) = frames emitted.  Nothing else differs from calling vstab_pull_frame n times. */
VSTAB_API vstab_status vstab_pull_frames(vstab_handle *h, int n, void *const *dst_bgr, const size_t *pitch_dst, int n_dst, int first,
                                         int *n_done);
/* pull_frame with NV12 output for the encoder hand-off (render.ts:275-281): the same frame,
 * converted as vstab_warp_nv12_ex(VSTAB_OUT_NV12) defines.  dst_y: width bytes per row; dst_uv: ceil(height/2) rows
 * of 2*ceil(width/2) bytes.  BGR and NV12 pulls may be mixed freely on one handle. */
VSTAB_API vstab_status vstab_pull_frame_nv12(vstab_handle *h, void *dst_y, size_t pitch_y, void *dst_uv,
                                             size_t pitch_uv);
/* The same pull with the frame warped PLANE BY PLANE -- no colour round trip (VSTAB_OUT_NV12_PLANAR: the Y and UV planes of the
 * source remapped as they are, limited-range black outside; SURVEY.md 8(f) row 2, the route the CLI's filter takes between NV12
 * surfaces, render.ts:606-607, 664-665, 688): fewer instructions per pixel than any route through BGR, 23.0 MB instead of 33.6 MB
 * moved per 4K frame.  Same look-ahead, same rotations, same planes' shapes as vstab_pull_frame_nv12; the map is evaluated for every
 * frame (the quantised-map cache holds no chroma positions).  May be mixed with the other 8-bit pulls on one handle. */
VSTAB_API vstab_status vstab_pull_frame_nv12_planar(vstab_handle *h, void *dst_y, size_t pitch_y, void *dst_uv, size_t pitch_uv);
/* pull_frame into HOST memory (what a cv::Mat / imshow consumer of DisplayImage.cpp:63-65 needs): the frame is warped
 * into a buffer of the handle and copied out; returns when the copy has completed. */
VSTAB_API vstab_status vstab_pull_frame_host(vstab_handle *h, void *dst_bgr_host, size_t pitch_dst);
/* pull_frame of a handle created with pixel_depth = 10: device BGR, three 16-bit samples per pixel (values 0..1023),
 * pitch_dst in bytes, >= 6 * width and even.  The 8-bit pull functions refuse such a handle and vice versa. */
VSTAB_API vstab_status vstab_pull_frame_bgr16(vstab_handle *h, void *dst_bgr16, size_t pitch_dst);
/* pull_frame of a pixel_depth = 10 handle as P010 planes for a 10-bit encoder (the counterpart of vstab_pull_frame_nv12): the frame is
 * warped and converted in one kernel (vstab_warp_p010_planes) when the frame's planes allow it, else warped into a 16-bit BGR buffer of the
 * handle and converted by vstab_cvt_bgr16_p010. */
VSTAB_API vstab_status vstab_pull_frame_p010(vstab_handle *h, void *dst_y, size_t pitch_y, void *dst_uv, size_t pitch_uv);
/* pull_frame of a pixel_depth = 10 handle warped plane by plane (vstab_warp_p010_planar): P010 planes in, P010 planes out, no
 * conversion to BGR and back; vstab_config.blend selects the blend of each sample. */
VSTAB_API vstab_status vstab_pull_frame_p010_planar(vstab_handle *h, void *dst_y, size_t pitch_y, void *dst_uv, size_t pitch_uv);
/* FrameSourceWarp::peek_frame (:478-480) IS pull_frame in the reference (destructive); kept. */
VSTAB_API vstab_status vstab_peek_frame(vstab_handle *h, void *dst_bgr, size_t pitch_dst);
VSTAB_API void vstab_destroy(vstab_handle *h);

/* Introspection for parity tests and profiling: what consume_frame (:397-450) decided for the
 * index-th consumed frame that produced a rotation (index 0 = second input frame). */
typedef struct vstab_frame_log {
    int key_frame;       /* corners re-detected before tracking this frame (:415-419) */
    int n_corners;       /* corners fed to the tracker */
    int n_tracked;       /* pairs with status != 0 (:263-268) */
    int n_inliers;       /* guess_camera_rotation's return value */
    int fallback;        /* 1 if n_inliers < 40 and the previous rotation / identity was reused (:432-438) */
    double R_frame[9];   /* rotation since last frame actually used */
    double R_accum[9];   /* accumulated measured rotation (:441-442) */
} vstab_frame_log;
/* Indices are absolute (frames since the start); only the most recent 65536 entries are retained. */
VSTAB_API int vstab_frame_log_count(const vstab_handle *h);
VSTAB_API vstab_status vstab_get_frame_log(const vstab_handle *h, int index, vstab_frame_log *out);
/* The rotation handed to the warp for the index-th emitted frame (rotation_correction.inv(), :475). */
VSTAB_API vstab_status vstab_get_warp_rotation(const vstab_handle *h, int index, double R[9]);

/* Per-stage profiler: the role of the reference's Profiler / FrameSourceProfile decorators
 * (Profiler.cpp:14-35), with GPU stages timed by HIP events on the handle's stream (microsecond
 * resolution instead of the reference's whole-millisecond truncation).
 * GPU stages exclude host waits; host stages are steady_clock wall time. */
typedef struct vstab_profile {
    long frames_consumed, frames_emitted, key_frames;
    double gpu_ingest_ms, gpu_pyramid_ms, gpu_corners_ms, gpu_lk_ms, gpu_warp_ms; /* sums of kernel time */
    double host_corners_ms, host_track_wait_ms, host_estimate_ms, host_smooth_ms;  /* sums of wall time */
    long warp_launches;
    long warp_timed;     /* warp launches that gpu_warp_ms sums over (level 1 samples every 8th) */
    long dmabuf_imports, dmabuf_evictions, dmabuf_cached; /* VSTAB_MEM_DMABUF: objects imported so far, unmapped again (least recently
                            used, once more than 256 are cached and none of the window's frames can still refer to them), mapped now */
    long corner_selections_by_caller, corner_selections_by_helper; /* speculative corner detections (planned key frames) whose corners were
                            selected by the calling thread itself because the helper thread had not woken up / by the helper thread */
    long epochs_in_turn; /* planned key frames whose detection and tracker launches ran on the second of the handle's two epoch streams, beside
                            the epoch still being tracked on the first (frames up to 1920 x 1200 with a caller on the default stream; 0 otherwise) */
} vstab_profile;
/* Loads the library's eleven GPU code objects now.  The HIP runtime loads a code object at the first launch of one of its kernels -- tens of
 * milliseconds in the middle of the first frames -- and on ROCm 7.2 such a late load can FAULT ("write access to a read-only page") when the
 * process has unloaded another module before it (hipModuleUnload; an OpenCL program released by a filter next door): the new code object may
 * be placed where the old one was still mapped read-only.  vstab_create calls this itself; a host that uses the stateless operators
 * (vstab_warp_nv12, vstab_pyr_lk, ...) without a handle, or wants the load at start-up, calls it once after selecting the device. */
VSTAB_API vstab_status vstab_preload_kernels(void);
/* level 0 = off, 1 = time every 8th warp launch only (event records are expensive host calls), 2 = every GPU stage */
VSTAB_API vstab_status vstab_enable_profiling(vstab_handle *h, int level);
/* cv::remap's borderMode for the frames this handle warps (the Border modes above), from the next pull on; it may change between pulls, and
 * each frame is warped with the mode in force when it is pulled.  VSTAB_BORDER_CONSTANT (the default) keeps the handle's usual warp kernels
 * and output.  Any other mode routes the 8-bit BGR pulls (vstab_pull_frame / _frames / _host / vstab_peek_frame) and the plane-wise pull
 * (vstab_pull_frame_nv12_planar) to vstab_warp_nv12_border, with a frame's read-out rotation where it has one; vstab_pull_frame_nv12 (NV12
 * through BGR) is then refused with VSTAB_ERR_INVALID before any frame is taken.  A non-constant mode is VSTAB_ERR_UNSUPPORTED on handles with
 * pixel_depth 10, interpolation 0 (INTER_NEAREST) or resample != VSTAB_RESAMPLE_DEFAULT; unknown modes and a NULL handle are VSTAB_ERR_INVALID. */
VSTAB_API vstab_status vstab_set_border_mode(vstab_handle *h, int border_mode);
/* vstab_set_border_mode for every 8-bit resampler: the same handle state, and vstab_set_border_mode is the INTER_LINEAR subset of it.  On
 * handles with resample VSTAB_RESAMPLE_CUBIC or VSTAB_RESAMPLE_LANCZOS4 a non-constant mode routes the BGR pulls and the plane-wise pull to
 * vstab_warp_nv12_cubic_border / _lanczos4_border (such handles keep refusing frames that carry a read-out rotation); NV12 through BGR is
 * refused as above.  A non-constant mode is VSTAB_ERR_UNSUPPORTED on handles with pixel_depth 10 or interpolation 0 (INTER_NEAREST); unknown
 * modes and a NULL handle are VSTAB_ERR_INVALID. */
VSTAB_API vstab_status vstab_set_border_mode_ex(vstab_handle *h, int border_mode);
/* The calibrated input lens of a handle (Lens distortion above): K, a row-major camera matrix with fx, fy > 0, zero skew and last row
 * 0 0 1 (NULL keeps the camera vstab_create derived from in_dfov), and the four coefficients D.  From then on the rotation estimate
 * undistorts the tracked points with D (vstab_estimate_rotation_d), the warp is vstab_warp_nv12_dist (a run of frames with equal parameters:
 * vstab_quantised_map_dist once, then vstab_warp_nv12_mapped), and the `debug` markers are projected through the distorted lens.  Served
 * pulls: vstab_pull_frame, _frames, _host, _nv12_planar and vstab_peek_frame; vstab_pull_frame_nv12 is refused before a frame is taken, a
 * frame that carries a readout_rotation is refused and consumed (as INTER_NEAREST does).  D = 0 gives the frames of a handle without the call.
 * Allowed on a handle with lens_mode 1, in_projection VSTAB_PROJ_FISH, resample VSTAB_RESAMPLE_DEFAULT, 8-bit pixels and the constant
 * border, before the first pull; anything else, a bad K and coefficients that are not accepted are VSTAB_ERR_INVALID, the message naming
 * the cause, and the handle is unchanged.  On a handle calibrated through this call vstab_set_border_mode / _ex refuse a non-constant mode
 * with VSTAB_ERR_INVALID (vstab_set_input_calibration_ex below lifts the two restrictions). */
VSTAB_API vstab_status vstab_set_input_calibration(vstab_handle *h, const double K[9], const double D[4]);
/* vstab_set_input_calibration for every 8-bit resampler and border mode: the same call and the same refusals, message for message under
 * this name, except that a handle with resample VSTAB_RESAMPLE_CUBIC or _LANCZOS4 and a handle with a non-constant border mode set are
 * accepted.  The warp is vstab_warp_nv12_dist_ex with the handle's resampler and the border mode in force at the pull (the quantised map
 * serves VSTAB_RESAMPLE_DEFAULT with VSTAB_BORDER_CONSTANT only); on a handle calibrated this way vstab_set_border_mode / _ex behave as on
 * a handle without a calibration, and the mode may change between pulls.  What stays refused (VSTAB_ERR_INVALID, the handle unchanged):
 * lens_mode other than 1, an input that is not a fisheye lens, pixel_depth 10, a call after the first pull, a bad K, coefficients that are
 * not accepted.  vstab_pull_frame_nv12 is refused before a frame is taken, a frame that carries a readout_rotation is refused and consumed.
 * The rotation estimate and the `debug` markers go through the distorted lens as with vstab_set_input_calibration: they do not depend on
 * the resampler. */
VSTAB_API vstab_status vstab_set_input_calibration_ex(vstab_handle *h, const double K[9], const double D[4]);
/* "Pinhole lens distortion" on a handle: a rectilinear input camera with D = (k1, k2, p1, p2, k3), and
 * optionally its calibrated camera matrix K (NULL keeps the camera vstab_create derived from in_dfov; the rule for K is
 * vstab_set_input_calibration's).  The handle then estimates its rotations with D (both point sets through cv::undistortPoints as above),
 * inverts the lens where it places the debug markers, and warps every BGR, _frames, _host, peek and plane-wise pull through
 * vstab_warp_nv12_pinhole with its resampler and the border mode in force at the pull (vstab_set_border_mode / _ex, before or after this
 * call, as on an uncalibrated handle).  The quantised-map cache steps aside.  Accepted: a handle with lens_mode 1, in_projection
 * VSTAB_PROJ_RECT, 8-bit pixels, INTER_LINEAR or resample VSTAB_RESAMPLE_CUBIC / _LANCZOS4, not yet pulled from.  Each refusal is
 * VSTAB_ERR_INVALID behind "vstab_set_input_pinhole: " and leaves the handle as it was: "null argument" (h, D), "a calibration belongs to
 * lens_mode 1 (the preset path derives its output camera from the input's)", "pinhole distortion belongs to a rectilinear input
 * (in_projection VSTAB_PROJ_RECT)", "the pinhole-lens warp takes 8-bit pixels, this is a pixel_depth 10 handle", "the pinhole-lens warp
 * resamples with INTER_LINEAR, INTER_CUBIC or INTER_LANCZOS4, this handle with INTER_NEAREST", "the calibration must be set before the
 * first pull", "K must be a camera matrix with fx, fy > 0, zero skew and last row 0 0 1", "the five distortion coefficients must be
 * finite".  Such a handle refuses: NV12 through BGR (vstab_pull_frame_nv12), before a frame is taken, with VSTAB_ERR_INVALID; the keep-edge
 * pulls with VSTAB_ERR_UNSUPPORTED; and a frame that carries a readout_rotation, which is refused and consumed whatever
 * vstab_set_readout_warp says (the refusal every rectilinear input makes when it takes such a frame from upstream).
 * vstab_set_input_calibration[_ex] keep refusing a rectilinear input. */
VSTAB_API vstab_status vstab_set_input_pinhole(vstab_handle *h, const double K[9], const double D[5]);
/* What a handle does with a frame that carries a readout_rotation where its warp used to have no rotation per row: handles with resample
 * VSTAB_RESAMPLE_CUBIC or _LANCZOS4, calibrated handles (vstab_set_input_calibration / _ex), or both.  VSTAB_READOUT_REFUSE (the default):
 * as before, the frame is refused and consumed.  VSTAB_READOUT_PER_ROW: the frame is warped by vstab_warp_nv12_rs_ex -- the first row with
 * the stabilising rotation W, the last with readout * W -- with the handle's resampler, the border mode in force at the pull and the
 * handle's coefficients, in the BGR pulls and in vstab_pull_frame_nv12_planar.  The mode may change between pulls.  Frames without a
 * read-out rotation are untouched, the quantised map of a calibrated handle included: a frame with a read-out rotation neither uses nor
 * refreshes it.  Still refused: vstab_pull_frame_nv12 (NV12 through BGR), INTER_NEAREST handles and, at ingest, any map other than
 * fisheye -> pinhole.  VSTAB_ERR_UNSUPPORTED on handles with pixel_depth 10 or interpolation 0; an unknown mode and a NULL handle are
 * VSTAB_ERR_INVALID. */
enum { VSTAB_READOUT_REFUSE = 0, VSTAB_READOUT_PER_ROW = 1 };
VSTAB_API vstab_status vstab_set_readout_warp(vstab_handle *h, int mode);
/* The detection mask of a handle ("Detection mask" above): every corner detection of the handle -- the first frame's, a key frame's, the
 * one run ahead of a planned key frame -- reports corners only where mask != 0.  mask: bytes of the size of the input luma plane
 * (the vstab_frame width x height upstream delivers; a pixel_depth 10 handle takes one as well, its detector reads the luma narrowed to 8 bits either way), in
 * device (mem = VSTAB_MEM_DEVICE) or host memory (VSTAB_MEM_HOST), rows pitch_mask bytes apart.  The handle copies it into device memory of
 * its own; the call returns when the copy is complete, and the caller may free the mask (a device mask is read
 * on the null stream: writes to it on a non-blocking stream have to be complete).  mask == NULL removes the mask (pitch_mask and mem
 * are not looked at).  Allowed before the first pull only.  A handle without a mask behaves as it always did.  Refused with VSTAB_ERR_INVALID,
 * the handle unchanged, in this order: "vstab_set_detection_mask: null handle"; "vstab_set_detection_mask: no detector runs on this handle
 * (tracking = 0)"; "vstab_set_detection_mask: the mask must be set before the first pull"; with a mask, "vstab_set_detection_mask: the
 * mask's pitch is smaller than the frame's width" and "vstab_set_detection_mask: mem must be VSTAB_MEM_DEVICE (0) or VSTAB_MEM_HOST (1)".
 * A static overlay (a burnt-in clock, a logo, a bonnet) is best masked out together with a margin of about 16 px: the tracker's 21 x 21
 * window reaches that far from a corner on the first pyramid level. */
VSTAB_API vstab_status vstab_set_detection_mask(vstab_handle *h, const void *mask, size_t pitch_mask, int mem);
/* The corner response of a handle ("Harris response" above): every corner detection of the handle -- the first frame's, a key frame's, the
 * one run ahead of a planned key frame -- uses it, with a detection mask or without, on pixel_depth 10 handles too.  response:
 * VSTAB_CORNER_HARRIS with k (goodFeaturesToTrack's useHarrisDetector = true), or VSTAB_CORNER_MIN_EIGENVAL, which does not look at k and
 * restores the handle as it always was.  Allowed before the first pull only.  Refused with VSTAB_ERR_INVALID, the handle unchanged, in this
 * order: "vstab_set_corner_response: null handle"; "vstab_set_corner_response: no detector runs on this handle (tracking = 0)";
 * "vstab_set_corner_response: the response must be set before the first pull"; "vstab_set_corner_response: response must be
 * VSTAB_CORNER_MIN_EIGENVAL (0) or VSTAB_CORNER_HARRIS (1)"; "vstab_set_corner_response: k lies in [0, 0.25)". */
VSTAB_API vstab_status vstab_set_corner_response(vstab_handle *h, int response, double k);
/* The corner block size of a handle ("Corner block size" above): every corner detection of the handle uses block_size (3, 5 or 7) as
 * goodFeaturesToTrack's blockSize, with any response and with a detection mask or without, on pixel_depth 10 handles too.  Independent of
 * vstab_set_corner_response and vstab_set_detection_mask: the three may be called in any order.  Without this call, or with 3, the handle
 * runs what it always ran.  Allowed before the first pull only.  Refused with VSTAB_ERR_INVALID, the handle unchanged, in this order:
 * "vstab_set_corner_block: null handle"; "vstab_set_corner_block: no detector runs on this handle (tracking = 0)";
 * "vstab_set_corner_block: the block size must be set before the first pull"; "vstab_set_corner_block: block_size is 3, 5 or 7". */
VSTAB_API vstab_status vstab_set_corner_block(vstab_handle *h, int block_size);
/* The corner gradient size of a handle ("Corner gradient size" above): every corner detection of the handle uses gradient_size (3, 5 or 7)
 * as goodFeaturesToTrack's gradientSize, with any block size and response and with a detection mask or without, on pixel_depth 10 handles
 * too.  Independent of vstab_set_corner_block, vstab_set_corner_response and vstab_set_detection_mask: the four may be called in any
 * order.  Without this call, or with 3, the handle runs what it always ran.  Allowed before the first pull only.  Refused with
 * VSTAB_ERR_INVALID, the handle unchanged, in this order: "vstab_set_corner_gradient: null handle"; "vstab_set_corner_gradient: no detector
 * runs on this handle (tracking = 0)"; "vstab_set_corner_gradient: the gradient size must be set before the first pull";
 * "vstab_set_corner_gradient: gradient_size is 3, 5 or 7". */
VSTAB_API vstab_status vstab_set_corner_gradient(vstab_handle *h, int gradient_size);

/* The handle's tracker options ("Tracker options" above, rules 1, 3 and 4): every tracker launch of the handle runs with them, and the
 * handle's pyramids have min(levels, max_level + 1) levels.  It takes no flags: err and the initial flow are stateless only
 * (vstab_pyr_lk_ex).  Without this call, or with (3, 30, 0.01, 1e-4), the handle runs what it ran before the options existed.
 * Refused with VSTAB_ERR_INVALID and the handle unchanged, in this order: "vstab_set_tracker_options: null handle";
 * "vstab_set_tracker_options: no tracker runs on this handle (tracking = 0)"; "vstab_set_tracker_options: the options must be set before
 * the first pull"; then vstab_pyr_lk_ex's four option messages under this name. */
VSTAB_API vstab_status vstab_set_tracker_options(vstab_handle *h, int max_level, int max_iter, double eps, double min_eig_threshold);
/* The handle's tracker window ("Tracker window" above): every tracker launch of the handle -- its segments, its chained launches and what
 * they fetch ahead -- runs with it, and the handle's pyramids have min(levels_W(width, height), max_level + 1) levels.  Independent of
 * vstab_set_tracker_options: the two may be called in either order.  Without this call, or with 21, the handle runs what it always ran.
 * Refused with VSTAB_ERR_INVALID and the handle unchanged, in this order: "vstab_set_tracker_window: null handle";
 * "vstab_set_tracker_window: no tracker runs on this handle (tracking = 0)"; "vstab_set_tracker_window: the window must be set before the
 * first pull"; "vstab_set_tracker_window: win_size is 15, 21 or 31". */
VSTAB_API vstab_status vstab_set_tracker_window(vstab_handle *h, int win_size);
/* vstab_pull_frame / vstab_pull_frame_nv12_planar with kept edges ("Keep edges" above): the next frame, warped by vstab_warp_nv12_keep with
 * the caller's previous output prev (prev_y / prev_uv) -- a second buffer (a ring of two outputs), or dst itself (in place).  A frame that
 * carries a read-out rotation is warped per row, as a plain INTER_LINEAR pull warps it.  Keep pulls and plain pulls may alternate frame by
 * frame; a keep pull neither reads nor refreshes the quantised map.  The debug markers (vstab_config.debug) are drawn after the warp, as
 * in every pull, so with the history in place they persist in kept areas.  Refused before any frame is dequeued, in this order: a NULL argument
 * (VSTAB_ERR_INVALID); a pixel_depth 10 handle (VSTAB_ERR_INVALID, vstab_pull_frame's message); VSTAB_ERR_UNSUPPORTED for a handle with
 * resample VSTAB_RESAMPLE_CUBIC or _LANCZOS4, interpolation 0, a border mode in force other than VSTAB_BORDER_CONSTANT, a calibrated
 * handle; a prev pitch smaller than a row and the aliasing rule (VSTAB_ERR_INVALID).  There is no vstab_pull_frames / _host / vstab_peek_frame form. */
VSTAB_API vstab_status vstab_pull_frame_keep(vstab_handle *h, void *dst_bgr, size_t pitch_dst, const void *prev_bgr, size_t pitch_prev);
VSTAB_API vstab_status vstab_pull_frame_nv12_planar_keep(vstab_handle *h, void *dst_y, size_t pitch_y, void *dst_uv, size_t pitch_uv,
                                                         const void *prev_y, size_t pitch_prev_y, const void *prev_uv, size_t pitch_prev_uv);
/* ---- Colour matrix and range ----------------------------------------------------------------------------------------------------------
 * The NV12 <-> BGR conversion of the BGR path as a choice of (matrix, range).  (VSTAB_COLOUR_CVTCOLOR, VSTAB_RANGE_LIMITED) is
 * cvtColor(COLOR_YUV2BGR_NV12) / cvtColor(COLOR_BGR2YUV_I420) with OpenCV's constants, byte for byte, and is the default everywhere;
 * (VSTAB_COLOUR_CVTCOLOR, VSTAB_RANGE_FULL) does not exist and is refused.  The other six specs use the same 20-bit fixed-point forms with
 * coefficients derived from (Kr, Kb): BT601 (0.299, 0.114), BT709 (0.2126, 0.0722), BT2020 non-constant luminance (0.2627, 0.0593);
 * Kg = 1 - Kr - Kb.  Limited range: sy = 255/219, sc = 255/224, yoff = 16.  Full range: sy = sc = 1, yoff = 0.  rint is round half to even
 * of the exact rational value.
 *   forward   CY = rint(2^20 sy), CVR = rint(2^20 sc 2(1 - Kr)), CUB = rint(2^20 sc 2(1 - Kb)),
 *             CUG = -rint(2^20 sc 2 Kb (1 - Kb) / Kg), CVG = -rint(2^20 sc 2 Kr (1 - Kr) / Kg); with u = U - 128, v = V - 128 and
 *             y = max(Y - yoff, 0) CY + 2^19:
 *               B = sat8((y + CUB u) >> 20), G = sat8((y + CVG v + CUG u) >> 20), R = sat8((y + CVR v) >> 20)
 *   inverse   CRY = rint(2^20 Kr / sy), CGY = rint(2^20 Kg / sy), CBY = rint(2^20 Kb / sy), CBU = rint(2^20 / (2 sc)) (also R's in V),
 *             CRU = -rint(2^20 Kr / (2(1 - Kb) sc)), CGU = -rint(2^20 Kg / (2(1 - Kb) sc)),
 *             CGV = -rint(2^20 Kg / (2(1 - Kr) sc)), CBV = -rint(2^20 Kb / (2(1 - Kr) sc));
 *               Y = sat8((CRY R + CGY G + CBY B + 2^19 + (yoff << 20)) >> 20)
 *               U = sat8((CRU R + CGU G + CBU B + 2^19 + (128 << 20)) >> 20)
 *               V = sat8((CBU R + CGV G + CBV B + 2^19 + (128 << 20)) >> 20)
 *             chroma from the top-left pixel of each 2 x 2 block.  The saturation is part of the definition: with CVTCOLOR it never acts,
 *             with full range it does (pure blue gives an unsaturated U of 256).
 * Every coefficient is below 2^23 and every forward sum below 5.8e8 in magnitude, so 24-bit multiplies and int32 sums hold for every spec.
 * A warp with a colour spec is the warp with the conversion exchanged: BGR8 = cvt(frame, spec) then cv::remap INTER_LINEAR with border 0;
 * NV12 through BGR = that frame converted back with the inverse of the same spec. */
enum { VSTAB_COLOUR_CVTCOLOR = 0, VSTAB_COLOUR_BT601 = 1, VSTAB_COLOUR_BT709 = 2, VSTAB_COLOUR_BT2020 = 3 }; /* matrix */
enum { VSTAB_RANGE_LIMITED = 0, VSTAB_RANGE_FULL = 1 };                                                   /* range  */
/* out = CY, CUB, CUG, CVG, CVR, yoff, CRY, CGY, CBY, CRU, CGU, CBU, CGV, CBV of a spec (host memory; no device needed).  An unknown matrix,
 * an unknown range, (CVTCOLOR, FULL) and a NULL pointer are VSTAB_ERR_INVALID. */
VSTAB_API vstab_status vstab_colour_coefficients(int matrix, int range, int32_t out[14]);
/* vstab_cvt_nv12_bgr with a colour spec. */
VSTAB_API vstab_status vstab_cvt_nv12_bgr_colour(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int width, int height, void *dst,
                                                 size_t pitch_dst, int matrix, int range, void *stream);
/* The inverse as an operator: 8-bit BGR (even width and height) to NV12 planes, dst_uv with width bytes per row, 2-byte aligned. */
VSTAB_API vstab_status vstab_cvt_bgr_nv12_colour(const void *src_bgr, size_t pitch, int width, int height, void *dst_y, size_t pitch_y, void *dst_uv,
                                                 size_t pitch_uv, int matrix, int range, void *stream);
/* vstab_warp_nv12_ex with a colour spec: VSTAB_OUT_BGR8 and VSTAB_OUT_NV12 (through BGR, converted back with the spec's inverse).
 * VSTAB_OUT_NV12_PLANAR converts nothing and is refused with VSTAB_ERR_INVALID, as is a bad spec.  (CVTCOLOR, LIMITED) is vstab_warp_nv12_ex
 * itself.  With any other spec, source planes of 4 GiB and more are VSTAB_ERR_UNSUPPORTED. */
VSTAB_API vstab_status vstab_warp_nv12_colour(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int src_width, int src_height,
                                              const float params[17], int map_mode, int out_format, void *dst, size_t pitch_dst, void *dst_uv,
                                              size_t pitch_dst_uv, int dst_width, int dst_height, int matrix, int range, void *stream);
/* The colour spec of a handle's BGR path, from the next pull on; it may change between pulls.  Served on 8-bit handles with INTER_LINEAR, the
 * constant border and an ideal lens: there vstab_pull_frame, _frames, _host, vstab_peek_frame and vstab_pull_frame_nv12 convert with the
 * spec (vstab_warp_nv12_colour); the plane-wise pull converts nothing and is served unchanged.  With a spec other than the default the
 * quantised-map cache steps aside (as it does for keep pulls).  A handle that never calls this, or sets (CVTCOLOR, LIMITED), runs what it
 * ran before.  Refused, the handle unchanged: a NULL handle and a bad spec (VSTAB_ERR_INVALID); a spec other than the default on a handle
 * with pixel_depth 10, interpolation 0, resample VSTAB_RESAMPLE_CUBIC / _LANCZOS4, a calibration (vstab_set_input_calibration[_ex],
 * vstab_set_input_pinhole) or a non-constant border mode in force (VSTAB_ERR_UNSUPPORTED).  While such a spec is set,
 * vstab_set_border_mode[_ex] refuse non-constant modes, the calibration setters and the keep pulls refuse (VSTAB_ERR_UNSUPPORTED), and a
 * frame that carries a readout_rotation is refused and consumed by the converting pulls, as INTER_NEAREST does. */
VSTAB_API vstab_status vstab_set_colour(vstab_handle *h, int matrix, int range);

/* ---- Colour matrix and range at 10 bits -----------------------------------------------------------------------------------------------
 * The P010 <-> 16-bit BGR conversion of the 10-bit path (vstab_warp_p010, vstab_warp_p010_planes, vstab_cvt_bgr16_p010, the pulls of a
 * pixel_depth 10 handle) as a choice of the same (matrix, range) pair, with a coefficient table of its own.  (CVTCOLOR, FULL) does not
 * exist and is refused.
 *   table     (VSTAB_COLOUR_CVTCOLOR, VSTAB_RANGE_LIMITED) is the 8-bit cvtColor row with yoff = 64: the 10-bit path's arithmetic as it
 *             always was, byte for byte, and the default everywhere.  The other six specs use the formulas of "Colour matrix and range"
 *             with the 10-bit scales: limited range sy = 1023/876, sc = 1023/896, yoff = 64; full range sy = sc = 1, yoff = 0.  The chroma
 *             offset is 512.  rint is round half to even of the exact rational value.  E.g. BT2020 limited: CY 1224536, CUB 2252416,
 *             CUG -197003, CVG -684025, CVR 1765394; BT709 full: 1048576, 1945738, -196424, -490864, 1651297.
 *   forward   y10 = word >> 6 (the low six bits of a P010 word are ignored), u = (U >> 6) - 512, v = (V >> 6) - 512, and with
 *             y = max(y10 - yoff, 0) CY + 2^19, the sums exact (64-bit):
 *               B = sat10((y + CUB u) >> 20), G = sat10((y + CVG v + CUG u) >> 20), R = sat10((y + CVR v) >> 20)
 *   inverse   B, G, R in [0, 1023] (the low ten bits of a 16-bit container):
 *               Y = sat10((CRY R + CGY G + CBY B + 2^19 + (yoff << 20)) >> 20)
 *               U = sat10((CRU R + CGU G + CBU B + 2^19 + (512 << 20)) >> 20)
 *               V = sat10((CBU R + CGV G + CBV B + 2^19 + (512 << 20)) >> 20)
 *             chroma from the top-left pixel of each 2 x 2 block; the output word is value << 6.  The saturation is part of the definition:
 *             with full range, pure blue's U is 1024 before it.
 *   overflow  Every coefficient is below 2^23 (the largest is 2 252 416).  The luma term is at most 1023 CY <= 1.2527e9; every chroma term
 *             with the luma offset folded in, 2^19 - yoff CY + C uv, lies in [-1.2311e9, 1.0732e9].  Each fits int32 and 24-bit multiplies
 *             hold; only their single sum can pass 2^31 (2.3259e9 at most, BT2020 limited), and whenever it does the true channel is at
 *             least 2048 and saturates to 1023, which is what a saturating 32-bit add gives; the sum never goes below -1.24e9.  Inverse sums
 *             are at most 2^30 (U of pure blue at full range).
 * A 10-bit warp with a colour spec is the warp with the conversion exchanged: the frame converted with the spec's forward form, then the
 * bilinear remap with the chosen blend; planes out are that frame through the inverse of the same spec. */
/* out = the 14 integers of a spec's 10-bit row, in vstab_colour_coefficients' order (host memory; no device needed).  Same refusals. */
VSTAB_API vstab_status vstab_colour_coefficients10(int matrix, int range, int32_t out[14]);
/* vstab_warp_p010 / vstab_warp_p010_planes with a colour spec: the argument lists, routing and refusals of their twins (VSTAB_ERR_UNSUPPORTED
 * from _planes included); a bad spec is VSTAB_ERR_INVALID under the entry point's own name, behind the other argument checks and before
 * any launch.  (CVTCOLOR, LIMITED) launches the twin's kernel.  vstab_warp_p010_planar converts nothing and has no such twin. */
VSTAB_API vstab_status vstab_warp_p010_colour(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int src_width, int src_height,
                                              const float params[17], const float *rot_bottom, int map_mode, int blend, void *dst_bgr16,
                                              size_t pitch_dst, int dst_width, int dst_height, int matrix, int range, void *stream);
VSTAB_API vstab_status vstab_warp_p010_planes_colour(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int src_width, int src_height,
                                                     const float params[17], const float *rot_bottom, int map_mode, int blend, void *dst_y,
                                                     size_t pitch_dst_y, void *dst_uv, size_t pitch_dst_uv, int dst_width, int dst_height,
                                                     int matrix, int range, void *stream);
/* The forward conversion as an operator: P010 planes (even width and height in [2, 32767]; luma 2-byte, chroma pairs 4-byte aligned) to 16-bit
 * BGR, values 0..1023, 2-byte aligned rows of at least 6 * width bytes. */
VSTAB_API vstab_status vstab_cvt_p010_bgr16_colour(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int width, int height, void *dst_bgr16,
                                                   size_t pitch_dst, int matrix, int range, void *stream);
/* vstab_cvt_bgr16_p010 with a colour spec (any size). */
VSTAB_API vstab_status vstab_cvt_bgr16_p010_colour(const void *src_bgr16, size_t pitch_src, int width, int height, void *dst_y, size_t pitch_y,
                                                   void *dst_uv, size_t pitch_uv, int matrix, int range, void *stream);
/* The colour spec of a pixel_depth 10 handle, from the next pull on; it may change between pulls.  vstab_pull_frame_bgr16 converts with the
 * spec (vstab_warp_p010_colour); vstab_pull_frame_p010 converts with it on both of its routes, which give the same bytes
 * (vstab_warp_p010_planes_colour, or vstab_warp_p010_colour into the handle's buffer and vstab_cvt_bgr16_p010_colour);
 * vstab_pull_frame_p010_planar converts nothing and is served unchanged.  Frames that carry a readout_rotation are warped per row, as they
 * are without a spec.  Refused, the handle unchanged: a NULL handle and a bad spec (VSTAB_ERR_INVALID); an 8-bit handle
 * (VSTAB_ERR_UNSUPPORTED: its spec is vstab_set_colour's). */
VSTAB_API vstab_status vstab_set_colour10(vstab_handle *h, int matrix, int range);

/* Cubic and Lanczos resampling at 10 bits: the plane-wise 10-bit warp (vstab_warp_p010_planar; no colour conversion) with cv::remap's
 * INTER_CUBIC or INTER_LANCZOS4 and a border mode.  A definition of this library's, like the rest of the 10-bit path (OpenCV's own CV_16U
 * remap blends with float tables): the 8-bit definition -- "Bicubic resampling", "Lanczos resampling", "Border modes of the cubic and Lanczos
 * resamplers" -- applied to the ten significant bits, as VSTAB_BLEND_EXACT defines the bilinear 10-bit blend.
 *   sample    s = word >> 6, in 0..1023 (the low six bits of a source word are ignored); the output word is v << 6.
 *   map       the map, its quantisation (cvRound(32 map), X = sat16(sx >> 5), f = fy * 32 + fx), the footprints (cubic 4 x 4 at X - 1, Y - 1;
 *             Lanczos 8 x 8 at X - 3, Y - 3) and the int16 tables (vstab_cubic_weights, vstab_lanczos4_weights; every entry sums to 32768)
 *             are the 8-bit path's, unchanged.
 *   chroma    as VSTAB_OUT_NV12_PLANAR: sampled at the even pixels of even rows, with 0.5f * map quantised again, the border decided over
 *             the chroma plane's own size (src_width / 2, src_height / 2), U and V blended separately.
 *   taps      VSTAB_BORDER_CONSTANT: a tap outside the plane enters as 64 (luma) or 512 (chroma), vstab_warp_p010_planar's border values,
 *             and a pixel whose footprint does not touch the plane is that value.  _REPLICATE, _REFLECT, _REFLECT_101: every tap is read
 *             at its borderInterpolate position.
 *   blend     v = clamp((sum w s + 2^14) >> 15, 0, 1023), an arithmetic shift: overshoot clamps at both ends, the upper one at 1023.
 *             int32 holds the sum: the largest sum of |w| of an entry is 61952 (cubic) and 96336 (Lanczos), so |sum| <= 96336 * 1023 + 2^14.
 * vstab_config.blend plays no part: these blends have no binary16 form.
 *
 * vstab_warp_p010_planar_ex: planes, pitches, alignments and sizes as for vstab_warp_p010_planar (source even and at least 8 x 2, 16-bit
 * samples 2-byte aligned, chroma pairs 4-byte aligned); all six map modes; rot_bottom (may be NULL) with map modes 0, 1 and 5.  Addresses
 * are formed in 64 bits: the bilinear kernel's "source pitch too large" limit does not apply.  Refusals, each before any launch, in this
 * order and with these texts behind "vstab_warp_p010_planar_ex: " (VSTAB_ERR_INVALID unless stated):
 *   "null pointer"; "sizes must be in [1, 32767], source even and at least 8 x 2";
 *   "bad source pitch or alignment (16-bit samples; chroma pairs 4-byte aligned)";
 *   "bad output pitch or alignment (16-bit samples; chroma pairs 4-byte aligned)"; "unknown map mode";
 *   "the per-row warp exists for the fisheye -> pinhole modes (0, 1, 5) only";
 *   resample VSTAB_RESAMPLE_DEFAULT: VSTAB_ERR_UNSUPPORTED, "VSTAB_RESAMPLE_DEFAULT (the bilinear warp) is served by vstab_warp_p010_planar";
 *   any other value but _CUBIC and _LANCZOS4: "resample must be VSTAB_RESAMPLE_CUBIC (2) or VSTAB_RESAMPLE_LANCZOS4 (4)";
 *   "border_mode must be VSTAB_BORDER_CONSTANT (0), _REPLICATE (1), _REFLECT (2) or _REFLECT_101 (4)". */
VSTAB_API vstab_status vstab_warp_p010_planar_ex(const void *y, size_t pitch_y, const void *uv, size_t pitch_uv, int src_width, int src_height,
                                                 const float params[17], const float *rot_bottom, int map_mode, int resample, int border_mode,
                                                 void *dst_y, size_t pitch_dst_y, void *dst_uv, size_t pitch_dst_uv, int dst_width, int dst_height,
                                                 void *stream);
/* The resampler and border mode of a pixel_depth 10 handle's plane-wise pull, from the next pull on; it may be called between pulls.
 * (vstab_create still refuses vstab_config.resample with pixel_depth 10, and vstab_set_border_mode / _ex such a handle: this is the way in.)
 * While a resampler is set, vstab_pull_frame_p010_planar warps with vstab_warp_p010_planar_ex (a frame that carries a readout_rotation per
 * row, as without one), and vstab_pull_frame_bgr16 / vstab_pull_frame_p010 are refused with VSTAB_ERR_INVALID before a frame is taken
 * ("vstab_pull_frame: VSTAB_RESAMPLE_CUBIC on a pixel_depth 10 handle (vstab_set_resample10) emits plane-wise P010 frames
 * (vstab_pull_frame_p010_planar), not 16-bit BGR or P010 through BGR"; or ..._LANCZOS4 ...): the frame stays pullable plane-wise.
 * (VSTAB_RESAMPLE_DEFAULT, VSTAB_BORDER_CONSTANT) restores the handle as it always was.  vstab_set_colour10 is untouched: the plane-wise
 * pull converts nothing.  Refusals, the handle unchanged, in this order and with these texts behind "vstab_set_resample10: ":
 *   VSTAB_ERR_INVALID      "null handle"; "resample must be VSTAB_RESAMPLE_DEFAULT (0), _CUBIC (2) or _LANCZOS4 (4)";
 *                          "border_mode must be VSTAB_BORDER_CONSTANT (0), _REPLICATE (1), _REFLECT (2) or _REFLECT_101 (4)"
 *   VSTAB_ERR_UNSUPPORTED  _DEFAULT with another border mode than _CONSTANT: "VSTAB_RESAMPLE_DEFAULT (the bilinear warp) has the constant
 *                          border at 10 bits; border modes are served with _CUBIC and _LANCZOS4";
 *                          an 8-bit handle: "served for pixel_depth 10 handles; an 8-bit handle takes its resampler from
 *                          vstab_config.resample and its border mode from vstab_set_border_mode_ex" */
VSTAB_API vstab_status vstab_set_resample10(vstab_handle *h, int resample, int border_mode);

/* Synchronises the stream, folds all pending event pairs into the sums and returns them. */
VSTAB_API vstab_status vstab_get_profile(vstab_handle *h, vstab_profile *out);

/* Profiling aid for the stateless warp operators (vstab_warp_nv12_*, vstab_warp_p010): the NEXT such call on this thread
 * launches its kernel with hipExtLaunchKernelGGL and the two events (hipEvent_t with timing enabled, owned by the caller),
 * which then hold the kernel's own start and end -- the duration rocprofv3's kernel trace reports, without launch gaps.
 * One-shot; a call that launches no such kernel leaves the request pending. */
VSTAB_API void vstab_time_next_launch(void *start_event, void *stop_event);

/* Utility upstream source for benchmarks and tests: cycles over n_frames caller-owned device
 * frames (packed NV12, same size) for total_frames pulls, then reports EOF.  Plays the role of
 * the decode chain upstream of FrameSourceWarp (DisplayImage.cpp:42-53), which is out of scope. */
typedef struct vstab_ring_source vstab_ring_source;
VSTAB_API vstab_status vstab_ring_source_create(const void *const *frames, int n_frames, int width, int height,
                                                size_t pitch, long total_frames, vstab_ring_source **out,
                                                vstab_source *as_source);
/* The same for P010-style frames (bit_depth 10 / 12 / 16: 16-bit samples, pitch in bytes, chroma plane at
 * frame + pitch * height) and/or with a read-out rotation per ring frame (9 doubles each, copied; may be NULL). */
VSTAB_API vstab_status vstab_ring_source_create_ex(const void *const *frames, int n_frames, int width, int height,
                                                   size_t pitch, long total_frames, int bit_depth,
                                                   const double *readout_rotations, vstab_ring_source **out,
                                                   vstab_source *as_source);
/* vstab_frame.hold the source reports for every frame.  Default 1 << 30: the frames belong to the caller for the life of the
 * source and are used in place, nothing is copied.  0 = the contract of a decoder that recycles its output surface: every
 * frame is copied into the library's ring (vstab_pack_nv12) before the next callback. */
VSTAB_API void vstab_ring_source_set_hold(vstab_ring_source *s, int hold);
VSTAB_API void vstab_ring_source_destroy(vstab_ring_source *s);

#ifdef __cplusplus
}
#endif
#endif /* VSTAB_H_ */
