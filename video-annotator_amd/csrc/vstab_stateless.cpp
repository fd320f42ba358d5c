// vstab_stateless.cpp -- the entry points of the C ABI that involve no handle: struct sizes and defaults, vstab_preload_kernels, the ring
// source, the stateless tracking / motion operators and the rotation-filter object.
#include <cstring>

#include "vstab_detect_host.hpp"
#include "vstab_motion.hpp"
#include "vstab_track_host.hpp"

using namespace vstab;

extern "C" {

int vstab_struct_size(int which) {
    switch (which) {
        case 0: return (int)sizeof(vstab_frame);
        case 1: return (int)sizeof(vstab_source);
        case 2: return (int)sizeof(vstab_config);
        case 3: return (int)sizeof(vstab_frame_log);
        case 4: return (int)sizeof(vstab_profile);
        default: return -1;
    }
}

int vstab_abi_version(void) { return VSTAB_ABI_VERSION; }

void vstab_config_default(vstab_config *cfg) {
    if (!cfg) return;
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->abi_version = VSTAB_ABI_VERSION;
    cfg->preset = VSTAB_GOPRO_H4B_WIDE169_MEASURED;
    cfg->scale = 1, cfg->crop_borders = 0, cfg->zoom = 1, cfg->smooth_radius = 30;  // FrameSourceWarp.hpp:86-89
    cfg->interpolation = 1, cfg->smoother = VSTAB_SMOOTHER_SG, cfg->tracking = 1, cfg->seed = 1, cfg->stream = nullptr;
    cfg->lens_mode = 0, cfg->in_projection = VSTAB_PROJ_FISH, cfg->out_projection = VSTAB_PROJ_RECT;
    cfg->in_dfov = 0, cfg->out_dfov = 0, cfg->out_width = 0, cfg->out_height = 0, cfg->out_cx = -1, cfg->out_cy = -1, cfg->debug = 0;
    cfg->pixel_depth = 8, cfg->blend = VSTAB_BLEND_EXACT;
    // the reference's map is what ITS kernel computes on this GPU (createMap.cl through ROCm's OpenCL compiler): the default
    cfg->map_precision = VSTAB_MAP_PRECISION_OPENCL;
    cfg->read_ahead = 0;  // the library's default (PREFETCH_DEPTH)
    cfg->resample = VSTAB_RESAMPLE_DEFAULT;
}

vstab_status vstab_preload_kernels(void) {
    VSTAB_TRY(preload_pyramid_kernels());
    VSTAB_TRY(preload_corner_kernels());
    VSTAB_TRY(preload_corners_fused_kernels());
    VSTAB_TRY(preload_corner_block_kernels());
    VSTAB_TRY(preload_lk_kernels());
    VSTAB_TRY(preload_lk_win_kernels());
    VSTAB_TRY(preload_plane_kernels());
    VSTAB_TRY(preload_warp_kernels());
    VSTAB_TRY(preload_fused_kernels());
    VSTAB_TRY(preload_p010_kernels());
    VSTAB_TRY(preload_planar_kernels());
    VSTAB_TRY(preload_cubic_kernels());
    VSTAB_TRY(preload_lanczos4_kernels());
    VSTAB_TRY(preload_border_kernels());
    VSTAB_TRY(preload_keep_kernels());
    VSTAB_TRY(preload_p010_resample_kernels());
    return VSTAB_OK;
}

// ---------------------------------------------------------------------------------------------
// ring source
// ---------------------------------------------------------------------------------------------
struct vstab_ring_source {
    std::vector<const void *> frames;
    int w, h;
    size_t pitch;
    long total, pos;
    int bit_depth = 8;
    int hold = 1 << 30;  // what the source promises: by default the caller owns the frames for the life of the source and never rewrites them
    std::vector<double> readout;  // optional: 9 doubles per ring frame (vstab_frame.readout_rotation)
};

static int ring_fill(vstab_ring_source *s, vstab_frame *out) {
    if (s->pos >= s->total) return VSTAB_EOF;
    const uint8_t *p = static_cast<const uint8_t *>(s->frames[(size_t)(s->pos % (long)s->frames.size())]);
    out->y = p, out->uv = p + s->pitch * s->h, out->pitch_y = out->pitch_uv = s->pitch;
    out->width = s->w, out->height = s->h, out->mem = 0, out->pts = s->pos;
    out->hold = s->hold;
    out->bit_depth = s->bit_depth;
    if (!s->readout.empty()) out->readout_rotation = &s->readout[9 * (size_t)(s->pos % (long)s->frames.size())];
    return 0;
}
static int ring_pull(void *user, vstab_frame *out) {
    vstab_ring_source *s = static_cast<vstab_ring_source *>(user);
    const int rc = ring_fill(s, out);
    if (rc == 0) s->pos++;
    return rc;
}
static int ring_peek(void *user, vstab_frame *out) { return ring_fill(static_cast<vstab_ring_source *>(user), out); }

void vstab_ring_source_set_hold(vstab_ring_source *s, int hold) {
    if (s) s->hold = hold < 0 ? 0 : hold;
}

vstab_status vstab_ring_source_create(const void *const *frames, int n_frames, int width, int height, size_t pitch,
                                      long total_frames, vstab_ring_source **out, vstab_source *as_source) {
    if (!frames || n_frames <= 0 || !out || !as_source || width <= 0 || height <= 0 || pitch < (size_t)width)
        return fail(VSTAB_ERR_INVALID, "vstab_ring_source_create: bad argument");
    vstab_ring_source *s = new vstab_ring_source;
    s->frames.assign(frames, frames + n_frames);
    s->w = width, s->h = height, s->pitch = pitch, s->total = total_frames, s->pos = 0;
    as_source->pull = ring_pull, as_source->peek = ring_peek, as_source->user = s;
    *out = s;
    return VSTAB_OK;
}

vstab_status vstab_ring_source_create_ex(const void *const *frames, int n_frames, int width, int height, size_t pitch, long total_frames, int bit_depth,
                                         const double *readout_rotations, vstab_ring_source **out, vstab_source *as_source) {
    if (bit_depth != 8 && bit_depth != 10 && bit_depth != 12 && bit_depth != 16) return fail(VSTAB_ERR_INVALID, "vstab_ring_source_create: bit_depth must be 8, 10, 12 or 16");
    if (pitch < (size_t)width * (bit_depth > 8 ? 2 : 1)) return fail(VSTAB_ERR_INVALID, "vstab_ring_source_create: bad argument");
    VSTAB_TRY(vstab_ring_source_create(frames, n_frames, width, height, pitch, total_frames, out, as_source));
    (*out)->bit_depth = bit_depth;
    if (readout_rotations) (*out)->readout.assign(readout_rotations, readout_rotations + 9 * (size_t)n_frames);
    return VSTAB_OK;
}

void vstab_ring_source_destroy(vstab_ring_source *s) { delete s; }

// ---------------------------------------------------------------------------------------------
// stateless tracking / motion entry points
// ---------------------------------------------------------------------------------------------
vstab_status vstab_pyr_down(const void *src, size_t pitch_src, int width, int height, void *dst, size_t pitch_dst, void *stream) {
    if (!src || !dst || width <= 0 || height <= 0 || pitch_src < (size_t)width || pitch_dst < (size_t)((width + 1) / 2))
        return fail(VSTAB_ERR_INVALID, "vstab_pyr_down: bad argument");
    return launch_pyr_down((const uint8_t *)src, pitch_src, width, height, (uint8_t *)dst, pitch_dst, static_cast<hipStream_t>(stream));
}

vstab_status vstab_pyr_down_x2(const void *src, size_t pitch_src, int width, int height, void *mid, size_t pitch_mid, void *dst, size_t pitch_dst, void *stream) {
    const int mw = (width + 1) / 2, mh = (height + 1) / 2;
    if (!src || !mid || !dst || width <= 0 || height <= 0 || pitch_src < (size_t)width || pitch_mid < (size_t)mw || pitch_dst < (size_t)((mw + 1) / 2))
        return fail(VSTAB_ERR_INVALID, "vstab_pyr_down_x2: bad argument");
    if (!pyr_down_x2_ok(width, height)) {  // tiny images: two single-level launches, the same bytes
        // (both launches' planes are looked at before the first kernel runs: a call that is refused writes nothing)
        VSTAB_TRY(check_pyr_down(pitch_src, width, height, pitch_mid));
        VSTAB_TRY(check_pyr_down(pitch_mid, mw, mh, pitch_dst));
        VSTAB_TRY(launch_pyr_down((const uint8_t *)src, pitch_src, width, height, (uint8_t *)mid, pitch_mid, static_cast<hipStream_t>(stream)));
        return launch_pyr_down((const uint8_t *)mid, pitch_mid, mw, mh, (uint8_t *)dst, pitch_dst, static_cast<hipStream_t>(stream));
    }
    return launch_pyr_down_x2((const uint8_t *)src, pitch_src, width, height, (uint8_t *)mid, pitch_mid, (uint8_t *)dst, pitch_dst, static_cast<hipStream_t>(stream));
}

// the dense maps: vstab_min_eig, vstab_corner_harris (harris: k is checked, last) and their _block and _grad forms ("Corner block size" and
// "Corner gradient size" in vstab.h)
static vstab_status corner_response_op(const char *fn, const void *gray, size_t pitch, int width, int height, int block, bool harris, double k, void *out, void *stream,
                                       int gradient = 3) {
    if (!gray || !out || width <= 0 || height <= 0 || pitch < (size_t)width) return fail(VSTAB_ERR_INVALID, std::string(fn) + ": bad argument");
    VSTAB_TRY(check_corner_block(fn, block));
    VSTAB_TRY(check_corner_gradient(fn, gradient));  // (the _grad forms only)
    if (harris && !harris_k_ok(k)) return fail(VSTAB_ERR_INVALID, std::string(fn) + ": k lies in [0, 0.25)");
    DevBuf mb;
    VSTAB_TRY(mb.ensure(16));
    VSTAB_TRY(launch_corner_response((const uint8_t *)gray, pitch, width, height, harris, harris ? (float)k : 0.0f, (float *)out, mb.as<int>(),
                                     static_cast<hipStream_t>(stream), block, gradient));
    VSTAB_HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    return VSTAB_OK;
}

vstab_status vstab_min_eig(const void *gray, size_t pitch, int width, int height, void *eig, void *stream) {
    return corner_response_op("vstab_min_eig", gray, pitch, width, height, 3, false, 0.0, eig, stream);
}

// vstab_min_eig's twin: cornerHarris(gray, response, 3, 3, k) as a dense device map ("Harris response" in vstab.h)
vstab_status vstab_corner_harris(const void *gray, size_t pitch, int width, int height, double k, void *response, void *stream) {
    return corner_response_op("vstab_corner_harris", gray, pitch, width, height, 3, true, k, response, stream);
}

vstab_status vstab_min_eig_block(const void *gray, size_t pitch, int width, int height, int block_size, void *eig, void *stream) {
    return corner_response_op("vstab_min_eig_block", gray, pitch, width, height, block_size, false, 0.0, eig, stream);
}

vstab_status vstab_corner_harris_block(const void *gray, size_t pitch, int width, int height, int block_size, double k, void *response, void *stream) {
    return corner_response_op("vstab_corner_harris_block", gray, pitch, width, height, block_size, true, k, response, stream);
}

vstab_status vstab_min_eig_grad(const void *gray, size_t pitch, int width, int height, int block_size, int gradient_size, void *eig, void *stream) {
    return corner_response_op("vstab_min_eig_grad", gray, pitch, width, height, block_size, false, 0.0, eig, stream, gradient_size);
}

vstab_status vstab_corner_harris_grad(const void *gray, size_t pitch, int width, int height, int block_size, int gradient_size, double k, void *response, void *stream) {
    return corner_response_op("vstab_corner_harris_grad", gray, pitch, width, height, block_size, true, k, response, stream, gradient_size);
}

// vstab_good_features_ex (fn "vstab_good_features", no mask, VSTAB_DETECTOR_FUSED refused as ever), vstab_good_features_mask and
// vstab_good_features_harris (harris: the Harris response with k, checked last); vstab_good_features_block and vstab_good_features_grad: all
// of them in one call, with the block size, the gradient size and use_harris as the caller gives them
static vstab_status good_features_op(const char *fn, bool fused_ok, const void *gray, size_t pitch, int width, int height, const void *mask, size_t pitch_mask,
                                     int max_corners, double quality, double min_distance, int detector, float *xy, int *count, int *detector_used,
                                     void *stream, bool harris = false, double k = 0.0, int block = 3, int gradient = 3) {
    if (!gray || !xy || !count || width < 3 || height < 3 || pitch < (size_t)width || max_corners <= 0 ||
        (detector != VSTAB_DETECTOR_AUTO && detector != VSTAB_DETECTOR_TWO_PASS && !(fused_ok && detector == VSTAB_DETECTOR_FUSED)))
        return fail(VSTAB_ERR_INVALID, std::string(fn) + ": bad argument");
    VSTAB_TRY(check_corner_block(fn, block));        // (vstab_good_features_block and _grad only)
    VSTAB_TRY(check_corner_gradient(fn, gradient));  // (vstab_good_features_grad only)
    // goodFeaturesToTrack's own assertion (NaN fails both halves; quality = +inf passes and finds no corner)
    if (!(quality > 0.0) || !(min_distance >= 0.0)) return fail(VSTAB_ERR_INVALID, std::string(fn) + ": quality must be > 0 and min_distance >= 0");
    DetectSpec spec;
    VSTAB_TRY(check_detect_spec(fn, mask, pitch_mask, harris, k, width, height, spec, block, gradient));
    Detector t;
    VSTAB_TRY(t.init(width, height));
    t.set_two_pass_detector(detector == VSTAB_DETECTOR_TWO_PASS);
    t.set_mask(spec.mask, spec.mask_pitch);
    t.set_response(spec.harris, spec.kf);
    t.set_block(spec.block);
    t.set_gradient(spec.gradient);
    std::vector<float> out;
    VSTAB_TRY(t.good_features((const uint8_t *)gray, pitch, max_corners, quality, min_distance, out, static_cast<hipStream_t>(stream)));
    *count = (int)(out.size() / 2);
    std::memcpy(xy, out.data(), sizeof(float) * out.size());
    if (detector_used) *detector_used = (detector == VSTAB_DETECTOR_TWO_PASS || t.fused_overflows()) ? VSTAB_DETECTOR_TWO_PASS : VSTAB_DETECTOR_FUSED;
    return VSTAB_OK;
}

vstab_status vstab_good_features_ex(const void *gray, size_t pitch, int width, int height, int max_corners, double quality,
                                    double min_distance, int detector, float *xy, int *count, int *detector_used, void *stream) {
    return good_features_op("vstab_good_features", false, gray, pitch, width, height, nullptr, 0, max_corners, quality, min_distance, detector, xy, count,
                            detector_used, stream);
}

vstab_status vstab_good_features_mask(const void *gray, size_t pitch, int width, int height, const void *mask, size_t pitch_mask, int max_corners,
                                      double quality, double min_distance, int detector, float *xy, int *count, int *detector_used, void *stream) {
    return good_features_op("vstab_good_features_mask", true, gray, pitch, width, height, mask, pitch_mask, max_corners, quality, min_distance, detector, xy,
                            count, detector_used, stream);
}

vstab_status vstab_good_features_harris(const void *gray, size_t pitch, int width, int height, const void *mask, size_t pitch_mask, int max_corners,
                                        double quality, double min_distance, double k, int detector, float *xy, int *count, int *detector_used, void *stream) {
    return good_features_op("vstab_good_features_harris", true, gray, pitch, width, height, mask, pitch_mask, max_corners, quality, min_distance, detector, xy,
                            count, detector_used, stream, true, k);
}

// vstab.h, "Corner block size": goodFeaturesToTrack's whole argument list; with block_size 3 the launches of the entry points above
vstab_status vstab_good_features_block(const void *gray, size_t pitch, int width, int height, const void *mask, size_t pitch_mask, int max_corners, double quality,
                                       double min_distance, int block_size, int use_harris, double k, int detector, float *xy, int *count, int *detector_used,
                                       void *stream) {
    if (use_harris != 0 && use_harris != 1) return fail(VSTAB_ERR_INVALID, "vstab_good_features_block: bad argument");
    return good_features_op("vstab_good_features_block", true, gray, pitch, width, height, mask, pitch_mask, max_corners, quality, min_distance, detector, xy, count,
                            detector_used, stream, use_harris == 1, k, block_size);
}

// vstab.h, "Corner gradient size": goodFeaturesToTrack's ten-argument overload; with gradient_size 3 it is vstab_good_features_block
vstab_status vstab_good_features_grad(const void *gray, size_t pitch, int width, int height, const void *mask, size_t pitch_mask, int max_corners, double quality,
                                      double min_distance, int block_size, int gradient_size, int use_harris, double k, int detector, float *xy, int *count,
                                      int *detector_used, void *stream) {
    if (use_harris != 0 && use_harris != 1) return fail(VSTAB_ERR_INVALID, "vstab_good_features_grad: bad argument");
    return good_features_op("vstab_good_features_grad", true, gray, pitch, width, height, mask, pitch_mask, max_corners, quality, min_distance, detector, xy, count,
                            detector_used, stream, use_harris == 1, k, block_size, gradient_size);
}

vstab_status vstab_good_features(const void *gray, size_t pitch, int width, int height, int max_corners, double quality,
                                 double min_distance, float *xy, int *count, void *stream) {
    return vstab_good_features_ex(gray, pitch, width, height, max_corners, quality, min_distance, VSTAB_DETECTOR_AUTO, xy, count, nullptr, stream);
}

// vstab_pyr_lk and vstab_pyr_lk_ex (vstab.h, "Tracker options"): `ex` is whether the options, the flags and err are the caller's; without it
// they are calcOpticalFlowPyrLK's defaults and the launches are the ones vstab_pyr_lk always made
static vstab_status pyr_lk_op(const char *fn, bool ex, const void *prev, size_t pitch_prev, const void *next, size_t pitch_next, int width, int height,
                              const float *prev_xy, int n, float *next_xy, unsigned char *status, float *err, int max_level, int max_iter, double eps,
                              double min_eig_threshold, int flags, void *stream, int win_size = LK_WIN) {
    if (!prev || !next || (n > 0 && (!prev_xy || !next_xy || !status)) || n < 0 || width <= 0 || height <= 0 ||
        pitch_prev < (size_t)width || pitch_next < (size_t)width)
        return fail(VSTAB_ERR_INVALID, std::string(fn) + ": bad argument");
    if (!lk_window_offered(win_size)) return fail(VSTAB_ERR_INVALID, std::string(fn) + ": win_size is 15, 21 or 31");  // (vstab_pyr_lk_win only)
    LkOptions opt;
    if (ex) {
        VSTAB_TRY(check_lk_options(fn, max_level, max_iter, eps, min_eig_threshold, opt));
        if (flags & ~(VSTAB_LK_USE_INITIAL_FLOW | VSTAB_LK_GET_MIN_EIGENVALS)) return fail(VSTAB_ERR_INVALID, std::string(fn) + ": unknown flag");
        if ((flags & VSTAB_LK_GET_MIN_EIGENVALS) && !err) return fail(VSTAB_ERR_INVALID, std::string(fn) + ": VSTAB_LK_GET_MIN_EIGENVALS needs err");
    }
    opt.win = win_size;
    hipStream_t st = static_cast<hipStream_t>(stream);
    Tracker t;
    VSTAB_TRY(t.init(width, height, opt));
    VSTAB_TRY(t.build_pyramid(0, (const uint8_t *)prev, pitch_prev, st));
    VSTAB_TRY(t.build_pyramid(1, (const uint8_t *)next, pitch_next, st));
    std::vector<float> p(prev_xy, prev_xy + 2 * (size_t)n), q;
    std::vector<uint8_t> s;
    const LkPyramid I = t.pyramid(0, (const uint8_t *)prev, pitch_prev), J = t.pyramid(1, (const uint8_t *)next, pitch_next);
    if (flags || err) VSTAB_TRY(t.track_ex(I, J, p, next_xy, flags, err, q, s, st));
    else VSTAB_TRY(t.track(I, J, p, q, s, st));
    if (n > 0) {
        std::memcpy(next_xy, q.data(), sizeof(float) * q.size());
        std::memcpy(status, s.data(), s.size());
    }
    return VSTAB_OK;
}

vstab_status vstab_pyr_lk(const void *prev, size_t pitch_prev, const void *next, size_t pitch_next, int width, int height,
                          const float *prev_xy, int n, float *next_xy, unsigned char *status, void *stream) {
    return pyr_lk_op("vstab_pyr_lk", false, prev, pitch_prev, next, pitch_next, width, height, prev_xy, n, next_xy, status, nullptr, 0, 0, 0.0, 0.0, 0, stream);
}

vstab_status vstab_pyr_lk_ex(const void *prev, size_t pitch_prev, const void *next, size_t pitch_next, int width, int height, const float *prev_xy, int n,
                             float *next_xy, unsigned char *status, float *err, int max_level, int max_iter, double eps, double min_eig_threshold, int flags,
                             void *stream) {
    return pyr_lk_op("vstab_pyr_lk_ex", true, prev, pitch_prev, next, pitch_next, width, height, prev_xy, n, next_xy, status, err, max_level, max_iter, eps,
                     min_eig_threshold, flags, stream);
}

// vstab.h, "Tracker window": with win_size 21 this is vstab_pyr_lk_ex -- the same launches
vstab_status vstab_pyr_lk_win(const void *prev, size_t pitch_prev, const void *next, size_t pitch_next, int width, int height, const float *prev_xy, int n,
                              float *next_xy, unsigned char *status, float *err, int max_level, int max_iter, double eps, double min_eig_threshold, int flags,
                              int win_size, void *stream) {
    return pyr_lk_op("vstab_pyr_lk_win", true, prev, pitch_prev, next, pitch_next, width, height, prev_xy, n, next_xy, status, err, max_level, max_iter, eps,
                     min_eig_threshold, flags, stream, win_size);
}

}  // extern "C"

// D: the input lens's k1..k4 (vstab_estimate_rotation_d) or, in_fish false, the rectilinear lens's (k1, k2, p1, p2, k3)
// (vstab_estimate_rotation_pinhole), else null
static vstab_status estimate_rotation_impl(const std::string &name, const float *prev_xy, const float *cur_xy, int n, const double K_in[9], const double K_out[9],
                                           const double *D, uint64_t seed, double R[9], int *inliers, bool in_fish = true) {
    if ((n > 0 && (!prev_xy || !cur_xy)) || n < 0 || !K_in || !K_out || !R || !inliers) return fail(VSTAB_ERR_INVALID, name + ": bad argument");
    if (D) VSTAB_TRY(in_fish ? check_distortion(name.c_str(), D) : check_pinhole_distortion(name.c_str(), D));
    Mat3 ki, ko, r;
    std::memcpy(ki.m, K_in, sizeof(ki.m)), std::memcpy(ko.m, K_out, sizeof(ko.m));
    Pcg32 rng(seed);
    *inliers = estimate_rotation(prev_xy, cur_xy, n, ki, ko, rng, r, in_fish, D);
    std::memcpy(R, r.m, sizeof(r.m));
    return VSTAB_OK;
}

extern "C" {

vstab_status vstab_estimate_rotation(const float *prev_xy, const float *cur_xy, int n, const double K_in[9], const double K_out[9],
                                     uint64_t seed, double R[9], int *inliers) {
    return estimate_rotation_impl("vstab_estimate_rotation", prev_xy, cur_xy, n, K_in, K_out, nullptr, seed, R, inliers);
}

vstab_status vstab_estimate_rotation_d(const float *prev_xy, const float *cur_xy, int n, const double K_in[9], const double K_out[9], const double D[4],
                                       uint64_t seed, double R[9], int *inliers) {
    if (!D) return fail(VSTAB_ERR_INVALID, "vstab_estimate_rotation_d: bad argument");
    return estimate_rotation_impl("vstab_estimate_rotation_d", prev_xy, cur_xy, n, K_in, K_out, D, seed, R, inliers);
}

vstab_status vstab_estimate_rotation_pinhole(const float *prev_xy, const float *cur_xy, int n, const double K_in[9], const double K_out[9], const double D[5],
                                             uint64_t seed, double R[9], int *inliers) {
    if (!D) return fail(VSTAB_ERR_INVALID, "vstab_estimate_rotation_pinhole: bad argument");
    return estimate_rotation_impl("vstab_estimate_rotation_pinhole", prev_xy, cur_xy, n, K_in, K_out, D, seed, R, inliers, false);
}

vstab_status vstab_sg_weights(int m, double *weights) {
    if (m < 0 || !weights) return fail(VSTAB_ERR_INVALID, "vstab_sg_weights: bad argument");
    const std::vector<double> w = sg_weights(m);
    std::memcpy(weights, w.data(), sizeof(double) * w.size());
    return VSTAB_OK;
}

struct vstab_rotation_filter {
    RotationFilterSG f;
    explicit vstab_rotation_filter(int m) : f(m) {}
};

vstab_status vstab_rotation_filter_create(int m, vstab_rotation_filter **out) {
    if (m < 0 || !out) return fail(VSTAB_ERR_INVALID, "vstab_rotation_filter_create: bad argument");
    *out = new vstab_rotation_filter(m);
    return VSTAB_OK;
}
vstab_status vstab_rotation_filter_add(vstab_rotation_filter *f, const double R[9]) {
    if (!f || !R) return fail(VSTAB_ERR_INVALID, "vstab_rotation_filter_add: null argument");
    Mat3 r;
    std::memcpy(r.m, R, sizeof(r.m));
    f->f.add(r);
    return VSTAB_OK;
}
vstab_status vstab_rotation_filter_filter(const vstab_rotation_filter *f, double R_out[9]) {
    if (!f || !R_out) return fail(VSTAB_ERR_INVALID, "vstab_rotation_filter_filter: null argument");
    const Mat3 r = f->f.filter();
    std::memcpy(R_out, r.m, sizeof(r.m));
    return VSTAB_OK;
}
void vstab_rotation_filter_destroy(vstab_rotation_filter *f) { delete f; }

}  // extern "C"
