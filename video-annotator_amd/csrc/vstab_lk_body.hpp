// vstab_lk_body.hpp -- the body of the tracker kernels, included by vstab_lk_window.hpp into k_lk_track (OPT = false) and k_lk_track_opt
// (OPT = true) of the 21 x 21 window and into k_lk_track_win (OPT = true) of every other one, and by nothing else.  No include guard: it is
// statements, not declarations.  In scope where it is included: the kernel's argument `args` (LkSegArgs), its LDS state `sh` (LkShared),
// `constexpr bool OPT` and the window's constants (LKW, LKT, LKJR, LK_PPL, LK_HALF ...).  Why a text and not a function:
// vstab_lk_window.hpp, above the kernels.
#ifndef VSTAB_LK_BODY_FROM_KERNEL
#error "vstab_lk_body.hpp is the body of the kernels of vstab_lk_window.hpp"
#endif
    const LkThread t = {(int)blockIdx.x, (int)threadIdx.x, (int)threadIdx.x & 63, __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6)};
    if (t.f >= args.n) return;
    __builtin_amdgcn_s_setprio(VSTAB_LK_PRIO);  // with the warp, above the pyramid and detector kernels (vstab_warp_fused.hip: VSTAB_WARP_PRIO)
    // development aid (VSTAB_LK_CLOCK): first workgroup start / last workgroup end on the 100 MHz wall clock
    if (args.clk && t.tid == 0) atomicMin(&args.clk[0], wall_clock64());
    unsigned int seq = args.seq[0];
    LK_STAMP(0, LK_NOW());
    float2 pp;
    if (!lk_start_point(args, t, pp)) return;
    // rule 3: the iteration cap and eps^2; rule 2: gp, where the top level's search starts (level-0 pixels) -- the previous point or the guess
    int max_iter = 30;
    double eps2 = 0.01 * 0.01;
    if constexpr (OPT) max_iter = args.max_iter, eps2 = args.eps2;
    int koff[LK_PPL];
    lk_window_offsets(koff, t.lane);
    LkAhead pf;
#pragma unroll 1
    for (int fi = 0; fi < args.n_frames; fi++) {
        const LkPyramid &I = args.pyr[fi], &J = args.pyr[fi + 1];
        seq = args.seq[fi];
        if (fi) LK_STAMP(0, LK_NOW());
        LK_STAMP(1, LK_NOW());
        float2 np = make_float2(0.f, 0.f);
        int st = 1;
        const int max_level = I.levels - 1;
        int jb = 0;                               // regJ[jb] holds the block staged for the level about to run
        int jorg_x = PF_NONE, jorg_y = PF_NONE;   // its origin (none yet)
        int own_dx = -1, own_dy = -1;
        float2 gp = pp;
        float errv = 0.0f;  // (OPT, wave 0) what the pair reports in `err`: rules 5 and 6
        if constexpr (OPT) {
            if (args.flags & VSTAB_LK_USE_INITIAL_FLOW) gp = args.init_pts[t.f];  // (launch_lk: a launch with a guess has one pair and host points)
        }
        const int served = lk_stage_pair<OPT>(sh, args, I, J, pp, gp, fi, max_level, t, pf, jorg_x, jorg_y, own_dx, own_dy);
        LK_STAMP(17, (unsigned long long)served);
        (void)served;  // read by the development build's stamps only
        LK_STAMP(2, LK_NOW());
        LK_STAMP(16, (unsigned long long)fi);
        lk_prepare_top_level<OPT>(sh, args, I, pp, max_level, t);
        for (int level = max_level; level >= 0; level--) {
            int n_iter = 0;
            const uint8_t *jmg = J.img[level];
            const int w = I.w[level], h = I.h[level];
            const uint32_t jpitch = (uint32_t)J.pitch[level];
            const float lscale = lk_level_scale(level);
            // the block staged for this level, wave 0's estimate after the level above and the level's window are visible (the top level:
            // behind the last barrier of lk_prepare_top_level)
            if (level != max_level) __syncthreads();
            LK_STAMP(18 + 3 * (max_level - level), LK_NOW());
            if (t.wave != 0) lk_helper_level<OPT>(sh, args, I, J, fi, pp, gp, level, max_level, lscale, jb, own_dx, own_dy, t, pf);
            if (t.wave == 0 && level != max_level) jorg_x = sh.s_jorg[jb][0], jorg_y = sh.s_jorg[jb][1];  // (published by this level's barrier)
            LK_STAMP(19 + 3 * (max_level - level), LK_NOW());
            // ---- wave 0: the Gauss-Newton iterations of the level ("break" = the reference's "continue").  jorg_x, jorg_y: origin of the block
            // staged for it in regJ[jb]; np: in, the estimate after the level above, out, after this level (a skipped level leaves it at its
            // start value); st: cleared when level 0 loses the feature.  Left in the kernel body on purpose: as a function of its own the same
            // statements were scheduled with every LDS read of the seven window pixels waiting for the one before it (14 round trips per
            // iteration on the dependent chain instead of 5 waits; k_lk_track 129 us against 98 in the isolated 4K timing, profiles/track_split_4k.txt).
            if (t.wave == 0) do {
                float npx, npy;
                if (level == max_level)
                    npx = gp.x * lscale, npy = gp.y * lscale;
                else
                    npx = np.x * 2.0f, npy = np.y * 2.0f;
                np = make_float2(npx, npy);
                if (!lk_level_geom(pp, level, w, h).ok) {
                    if (level == 0) st = 0;
                    break;
                }
                int *rJ = sh.regJ[jb];
                int jx0 = jorg_x, jy0 = jorg_y;  // origin of the next-image block staged for this level
                int Iw[LK_PPL], Ixy[LK_PPL];     // this lane's pixels of the interpolated window: I, and Ix | Iy << 16
#pragma unroll
                for (int m = 0; m < LK_PPL; m++) {
                    const int k = t.lane + 64 * m;
                    const bool have = k < LKW * LKW;  // (the pad entries of the last row of lanes are never written)
                    Iw[m] = have ? (int)sh.patch_i[level][k] : 0;
                    Ixy[m] = have ? (int)sh.patch_xy[level][k] : 0;
                }
                const float FLT_SCALE = 1.0f / (1 << 20);
                const float A11 = sh.level_mat[level][0], A12 = sh.level_mat[level][1], A22 = sh.level_mat[level][2], D = sh.level_mat[level][3];
                if constexpr (OPT) {
                    // rule 6: the matrix of this level was formed (its previous-point range test passed just above); the levels run from coarse
                    // to fine, so the last one to get here is the finest.  Before the rejection test: a rejected point reports it too.
                    if (args.flags & VSTAB_LK_GET_MIN_EIGENVALS) errv = sh.level_mat[level][5];
                }
                if (sh.level_mat[level][4] != 0.0f) {  // minEig < 1e-4 (OPT: the launch's threshold) || D < FLT_EPSILON
                    if (level == 0) st = 0;
                    break;
                }
                npx -= LK_HALF, npy -= LK_HALF;
                float pdx = 0.f, pdy = 0.f;
                LK_STAMP(3 + 3 * (max_level - level), LK_NOW());
                for (int j = 0; j < max_iter; j++) {
                    n_iter++;
                    const int inx = (int)floorf(npx), iny = (int)floorf(npy);
                    if (!lk_origin_in_range(npx, npy, w, h)) {
                        if (level == 0) st = 0;
                        break;
                    }
                    int iw00, iw01, iw10, iw11;
                    lk_bilinear_weights(npx - (float)inx, npy - (float)iny, iw00, iw01, iw10, iw11);
                    if (inx < jx0 || iny < jy0 || inx + LKT > jx0 + LKJR || iny + LKT > jy0 + LKJR) {
                        // the window is outside the staged block: this wave stages a block centred on the window (wave-uniform branch;
                        // LDS operations of one wave execute in order, and the other waves write the OTHER buffer)
                        jx0 = inx - LKJM, jy0 = iny - LKJM;
                        LkStage<LKJR, 64> sj;
                        sj.load(jmg, jpitch, w, h, jx0, jy0, t.lane);
                        sj.store(rJ, t.lane);
                    }
                    const int jbase = lk_mul(iny - jy0, LKJR) + (inx - jx0);
                    int pb0 = 0, pb1 = 0;  // per-lane partial sums: 7 * 16320 * 4080 < 2^29
#pragma unroll
                    for (int m = 0; m < LK_PPL; m++) {
                        const int *c = &rJ[jbase + koff[m]];
                        const int diff = LK_DESCALE(lk_mul(c[0], iw00) + lk_mul(c[1], iw01) + lk_mul(c[LKJR], iw10) + lk_mul(c[LKJR + 1], iw11), 9) - Iw[m];
                        pb0 += lk_mul(diff, (int)(short)(Ixy[m] & 0xffff)), pb1 += lk_mul(diff, Ixy[m] >> 16);
                    }
                    int s[4] = {pb0 >> 16, pb0 & 0xffff, pb1 >> 16, pb1 & 0xffff};  // (lk_exact_total)
                    wave_sums_i32(s);  // uniform (SGPR) results
                    const float b1 = lk_exact_total(s[0], s[1]) * FLT_SCALE, b2 = lk_exact_total(s[2], s[3]) * FLT_SCALE;
                    const float dx = (A12 * b2 - A22 * b1) * D, dy = (A12 * b1 - A11 * b2) * D;
                    npx += dx, npy += dy;
                    np = make_float2(npx + LK_HALF, npy + LK_HALF);
                    if ((double)dx * dx + (double)dy * dy <= eps2) break;
                    if (j > 0 && fabs((double)(dx + pdx)) < 0.01 && fabs((double)(dy + pdy)) < 0.01) {
                        np.x -= dx * 0.5f, np.y -= dy * 0.5f;
                        break;
                    }
                    pdx = dx, pdy = dy;
                }
                // OpenCV's LKTrackerInvoker, behind the loop (the reference passes `err`, FrameSourceWarp.cpp:250-259): at
                // level 0 the final position -- the stored point minus the half window -- is tested against the image once
                // more, and a feature whose last step (or half-step correction) carried its window out is dropped.
                if (level == 0 && st) {
                    if (!lk_origin_in_range(np.x - LK_HALF, np.y - LK_HALF, w, h)) st = 0;
                }
                if constexpr (OPT) {
                    // rule 5, the residual: behind the final range test, so the window origin floor(np - 10) lies in [-21, w) x [-21, h) as an
                    // iteration's does, and the same tap body runs once more -- against Iw[] still in registers.  st is 1 only if every
                    // iteration passed its range test, so the block in rJ is one the loop staged or accepted; if the final window (the last
                    // step, or the half-step correction) left it, it is staged afresh exactly as the loop does.  A lane's pad pixels
                    // (k >= 441: offset 0, Iw 0) must not count: the iterations multiply them by a zero derivative, a sum of |.| cannot.
                    if (level == 0 && st && args.err && !(args.flags & VSTAB_LK_GET_MIN_EIGENVALS)) {
                        const float fx = np.x - LK_HALF, fy = np.y - LK_HALF;
                        const int inx = (int)floorf(fx), iny = (int)floorf(fy);
                        int iw00, iw01, iw10, iw11;
                        lk_bilinear_weights(fx - (float)inx, fy - (float)iny, iw00, iw01, iw10, iw11);
                        if (inx < jx0 || iny < jy0 || inx + LKT > jx0 + LKJR || iny + LKT > jy0 + LKJR) {
                            jx0 = inx - LKJM, jy0 = iny - LKJM;
                            LkStage<LKJR, 64> sj;
                            sj.load(jmg, jpitch, w, h, jx0, jy0, t.lane);
                            sj.store(rJ, t.lane);
                        }
                        const int jbase = lk_mul(iny - jy0, LKJR) + (inx - jx0);
                        int pr = 0;  // per-lane partial: 7 * 8160 < 2^16; the wave's total <= 441 * 8160 < 2^22
#pragma unroll
                        for (int m = 0; m < LK_PPL; m++) {
                            const int *c = &rJ[jbase + koff[m]];
                            const int diff = LK_DESCALE(lk_mul(c[0], iw00) + lk_mul(c[1], iw01) + lk_mul(c[LKJR], iw10) + lk_mul(c[LKJR + 1], iw11), 9) - Iw[m];
                            pr += t.lane + 64 * m < LKW * LKW ? (diff < 0 ? -diff : diff) : 0;
                        }
                        int s[1] = {pr};
                        wave_sums_i32(s);
                        errv = (float)s[0] / (float)(32 * LKW * LKW);  // an integer below 2^24: exact as a float, one division
                    }
                }
            } while (false);
            if (t.tid == 0) sh.s_est[level & 1][0] = np.x, sh.s_est[level & 1][1] = np.y;  // (a skipped level leaves np at its start value, as the reference does)
            LK_STAMP(4 + 3 * (max_level - level), LK_NOW());
            LK_STAMP(5 + 3 * (max_level - level), (unsigned long long)n_iter);
            (void)n_iter;  // read by the development build's stamps only
            jb ^= 1;
        }
        lk_publish_pair(sh, args, fi, seq, t, np, st);
        if constexpr (OPT) {
            // a plain store: `err` is read behind a synchronisation of the stream, not behind the record's tags (which promise nothing
            // about a second store).  A point that ends with status 0 never reached the residual and reports the 0 errv started from.
            if (args.err && t.tid == 0) args.err[t.f] = errv;
        }
        if (!st) return;  // uniform
        pp = np;          // FrameSourceWarp.cpp:427
        __syncthreads();  // the last readers of this pair's LDS state are through before the next pair's staging overwrites it
    }
