// vstab_warp_bands.hpp -- cost-weighted XCD bands for the fused 8-bit warp (host code only).
//
// tile_schedule (vstab_warp_tile.hpp) deals the half-height tile rows of the output evenly to the 8 XCDs, and a launch lasts as long as
// its slowest XCD.  Tiles do not cost the same: a dead tile (tile_dead_rule) only stores zeros, and a live tile's cost grows with the
// source area it stages -- at a fisheye source the dead tiles sit in the first and last bands and the large boxes in the middle ones.
// weighted_bands() moves the band boundaries so that every XCD gets about the same COST instead of the same number of rows; everything
// else -- the tall / half-height split, the tail, the grid, the kernels' block -> tile prologue -- is tile_schedule's.  Placement only
// affects speed, never results: the host's guess of which tiles are dead decides no pixel.
#pragma once
#include <array>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <vector>

#include "vstab_warp_tile.hpp"

namespace vstab {

// Rewrites ta.band_y / ta.split_y (after tile_schedule has filled ta) from cost[0 .. n_cost), one entry per half-height tile row, and
// returns the grid.  Band boundary k is the largest row count whose cost prefix is at most k / 8 of the total (integers: a uniform
// vector gives exactly tile_schedule's (k * half_rows / 8)); an all-zero vector or one of the wrong length keeps the even bands.
// Invariants (tests/test_band_schedule_cpu.py): band_y[0] == 0, band_y[8] == dh, non-decreasing multiples of the half-tile height,
// split_y - band_y a multiple of the tall height, the same tail rule per band, grid == 8 * max(share); surplus workgroups of the bands
// with fewer tiles leave through the kernels' `ys >= y_hi` return.
static inline unsigned weighted_bands(FusedArgs &ta, int rwb, int lds_kb, double tail_rounds, const uint32_t *cost, int n_cost) {
    const unsigned even_grid = tile_schedule(ta, rwb, lds_kb, tail_rounds);
    const WarpArgs &a = ta.w;
    const int th = 4 * rwb, ts = th / 2;
    const int half_rows = (int)div_up(a.dh, ts);
    if (!cost || n_cost != half_rows) return even_grid;
    uint64_t total = 0;
    for (int i = 0; i < half_rows; i++) total += cost[i];
    if (total == 0) return even_grid;
    const int slots = 32 * std::max(1, std::min(8, (int)(160 / lds_kb)));
    int h = 0;
    uint64_t prefix = 0;
    ta.band_y[0] = 0;
    for (int k = 1; k < 8; k++) {
        while (h < half_rows && 8 * (prefix + cost[h]) <= (uint64_t)k * total) prefix += cost[h++];
        ta.band_y[k] = std::min(a.dh, h * ts);
    }
    ta.band_y[8] = a.dh;
    int share = 0;
    for (int k = 0; k < 8; k++) {  // as tile_schedule
        const int rows = ta.band_y[k + 1] - ta.band_y[k];
        const int tall_rows_max = rows / th;
        const int tail_tall_rows = (int)std::min<long>(tall_rows_max, std::lround(tail_rounds * slots / ta.tiles_x));
        const int tall_rows = tall_rows_max - tail_tall_rows;
        ta.split_y[k] = ta.band_y[k] + tall_rows * th;
        const int n = tall_rows * ta.tiles_x + (int)div_up(ta.band_y[k + 1] - ta.split_y[k], ts) * ta.tiles_x;
        share = std::max(share, n);
    }
    return 8u * (unsigned)share;
}

// The cost model: what a 64 x ts half-height tile (a tall tile is two of them) holds a workgroup slot for, in relative units -- an XCD is
// through with its band when its 128 slots have worked off the durations of the band's tiles.  First fitted to the per-workgroup
// durations of one launch at the 4K headline (tools/wg_timeline.py, tools/fit_band_costs.py; profiles/dead_tiles_bands_4k.txt), a unit
// then being 0.01 us: a dead tall tile 2.7 us, a live one 4.4 us + 0.0058 us per staged block of 8 x 2 source pixels.  The static
// instruction census (a dead tile about 70 vector instructions per thread against 630 + 157 per trip of the staging loop) put a dead
// tile at a ninth of a live one; by the clock it was 0.44, because a dead tile is all latency -- the probe's dependent chain on one wave,
// a barrier, the stores -- and bands weighed with the census ratios overloaded the outer XCDs (32 - 33 us against 23 - 25 us in the middle).
// The clock's fit is a starting point, not the optimum (profiles/dead_store_4k.txt): its eight stamps are about 0.8 us of every tile, a
// third of a dead one (a later dump reads dead tall 2.60 us, live tall 5.69 us + 0.0031 us per block), the model leaves out that
// workgroups are dealt in blockIdx order, and the bands are a step function of the constants.  The per-block cost is therefore chosen by
// the kernel's own time in the product build: 0.45 was the best of the four sets tried (0.58, 0.45, 0.30 per block at 135 / 220, and
// 135 / 260 / 0.58), by 0.1 to 0.3 us of 27.4 us, at ONE shape (the 4K headline) with the identity rotation -- it rests on that; in the
// pipeline (rotations of a shaky clip) the same constant is worth 2 % of the headline.  BAND_COST_DEAD and the floor of a live tile stay
// as tests/test_band_schedule_cpu.py pins them.
constexpr uint32_t BAND_COST_DEAD = 135, BAND_COST_LIVE = 220;
constexpr double BAND_COST_PER_BLOCK = 0.45;

// cost[r] of half-height tile row r (64 x ts tiles) of a dw x dh output under params (the 17 map parameters; fisheye -> pinhole): the
// exact map in double at the tile corners; a tile whose four corners lie beyond the same source edge counts as dead, any other as live
// with the source box its corners span.  nan_behind: rays with wz <= 0 map nowhere (MAP_FISH_TO_RECT).
static inline void band_costs(const float params[17], bool nan_behind, int sw, int sh, int dw, int dh, int ts, std::vector<uint32_t> &cost) {
    const int tiles_x = (int)div_up(dw, 64), half_rows = (int)div_up(dh, ts);
    const double icx = params[0], icy = params[1], ifx = params[2], ify = params[3], ocx = params[4], ocy = params[5], ofx = params[6], ofy = params[7];
    const float *r = params + 8;
    std::vector<double> X((size_t)(tiles_x + 1) * 2), Y((size_t)(tiles_x + 1) * 2);  // two rows of corners: above and below the tile row
    auto corners = [&](int row, double *xo, double *yo) {
        const double vy = ((double)std::min(row * ts, dh - 1) - ocy) / ofy;
        for (int c = 0; c <= tiles_x; c++) {
            const double vx = ((double)std::min(c * 64, dw - 1) - ocx) / ofx;
            const double wx = r[0] * vx + r[1] * vy + r[2], wy = r[3] * vx + r[4] * vy + r[5], wz = r[6] * vx + r[7] * vy + r[8];
            if (!(wz > 0.0) && (nan_behind || wz == 0.0)) {
                xo[c] = yo[c] = NAN;
                continue;
            }
            const double ux = wx / wz, uy = wy / wz, rad = std::sqrt(ux * ux + uy * uy), k = rad > 0.0 ? std::atan(rad) / rad : 1.0;
            xo[c] = icx + ifx * ux * k, yo[c] = icy + ify * uy * k;
        }
    };
    cost.assign((size_t)half_rows, 0u);
    double *x0 = X.data(), *x1 = x0 + tiles_x + 1, *y0 = Y.data(), *y1 = y0 + tiles_x + 1;
    corners(0, x0, y0);
    for (int row = 0; row < half_rows; row++) {
        corners(row + 1, x1, y1);
        uint32_t sum = 0;
        for (int c = 0; c < tiles_x; c++) {
            const double xs[4] = {x0[c], x0[c + 1], x1[c], x1[c + 1]}, ys[4] = {y0[c], y0[c + 1], y1[c], y1[c + 1]};
            double mnx = xs[0], mxx = xs[0], mny = ys[0], mxy = ys[0];
            bool finite = true;
            for (int i = 0; i < 4; i++) {
                finite = finite && std::isfinite(xs[i]) && std::isfinite(ys[i]);
                mnx = std::min(mnx, xs[i]), mxx = std::max(mxx, xs[i]), mny = std::min(mny, ys[i]), mxy = std::max(mxy, ys[i]);
            }
            double blocks = 64.0 * ts * 4.0 / 16.0;  // a map that runs wild inside the tile: a large box
            if (finite) {
                if (mxx < -1.0 || mnx >= (double)sw || mxy < -1.0 || mny >= (double)sh) {
                    sum += BAND_COST_DEAD;
                    continue;
                }
                const double bw = std::min(mxx + 2.0, (double)sw) - std::max(mnx - 1.0, -1.0) + 8.0;  // the probe's margins and the 8 x 2 alignment
                const double bh = std::min(mxy + 2.0, (double)sh) - std::max(mny - 1.0, -1.0) + 2.0;
                blocks = std::max(bw, 8.0) * std::max(bh, 2.0) / 16.0;
            }
            sum += BAND_COST_LIVE + (uint32_t)std::min(blocks * BAND_COST_PER_BLOCK, 4096.0);
        }
        cost[(size_t)row] = sum;
        std::swap(x0, x1), std::swap(y0, y1);
    }
}

// The bands of recent launches.  The cost vector depends on the cameras, the sizes, the mode, the tile shape and the rotation; only the
// rotation changes from frame to frame, and it moves the dead boundary by about half a tile row per degree at a GoPro-wide lens.  An
// entry serves every launch with the same key whose rotation lies within BAND_CACHE_ANGLE of the one the entry was computed for
// (boundaries then off by under a tile row out of the 15 to 40 a band holds); a bounded camera shake fills the cache with a few
// entries and then always hits.  A hit is a mutex, a scan of at most BAND_CACHE_ENTRIES keys and 17 integers copied.
constexpr double BAND_CACHE_ANGLE = 1.5 * 3.14159265358979323846 / 180.0;
constexpr int BAND_CACHE_ENTRIES = 32;
struct BandCache {
    struct Entry {
        float fixed[8];  // the two cameras
        int dims[8];     // sw, sh, dw, dh, mode, rwb, lds_kb, tail_rounds in 1 / 64
        float rot[9];
        int band_y[9], split_y[8];
        unsigned grid;
    };
    std::mutex mu;
    std::vector<Entry> entries;
    size_t next = 0;
    long hits = 0, misses = 0;

    // fills ta.band_y / ta.split_y (ta as fill_fused_args left it) and returns the grid
    unsigned schedule(FusedArgs &ta, const float params[17], int map_mode, int rwb, int lds_kb, double tail_rounds) {
        const WarpArgs &a = ta.w;
        const int dims[8] = {a.sw, a.sh, a.dw, a.dh, map_mode, rwb, lds_kb, (int)std::lround(tail_rounds * 64.0)};
        const double min_trace = 1.0 + 2.0 * std::cos(BAND_CACHE_ANGLE);  // trace(Ra^T Rb) = 1 + 2 cos(angle between them)
        std::lock_guard<std::mutex> lock(mu);
        for (const Entry &e : entries) {
            if (std::memcmp(e.fixed, params, sizeof e.fixed) || std::memcmp(e.dims, dims, sizeof dims)) continue;
            double tr = 0.0;
            for (int i = 0; i < 9; i++) tr += (double)e.rot[i] * params[8 + i];
            if (!(tr >= min_trace)) continue;
            tile_schedule(ta, rwb, lds_kb, tail_rounds);  // lds_capacity_px, tiles_x
            std::memcpy(ta.band_y, e.band_y, sizeof e.band_y), std::memcpy(ta.split_y, e.split_y, sizeof e.split_y);
            hits++;
            return e.grid;
        }
        misses++;
        std::vector<uint32_t> cost;
        band_costs(params, map_mode == MAP_FISH_TO_RECT, a.sw, a.sh, a.dw, a.dh, 2 * rwb, cost);
        Entry e;
        std::memcpy(e.fixed, params, sizeof e.fixed), std::memcpy(e.dims, dims, sizeof dims), std::memcpy(e.rot, params + 8, sizeof e.rot);
        e.grid = weighted_bands(ta, rwb, lds_kb, tail_rounds, cost.data(), (int)cost.size());
        std::memcpy(e.band_y, ta.band_y, sizeof e.band_y), std::memcpy(e.split_y, ta.split_y, sizeof e.split_y);
        if ((int)entries.size() < BAND_CACHE_ENTRIES) entries.push_back(e);
        else entries[next++ % BAND_CACHE_ENTRIES] = e;
        return e.grid;
    }
};

}  // namespace vstab
