// pt_adaptive.hpp — adaptive sampling at the granularity of the 16x16 tile: a frame is rendered in
// sample windows, and after each window every tile that is still active is judged by the relative standard error of
// its luminance, estimated by batch means from the windows' running sums (§3.9's estimate); a tile that meets the
// target, or reaches the cap, is divided out into the frame and never touched again.  The windows go through
// launch_render into a sums plane -- over ranges of the tile list (adaptive_runs), or over the list of the active tiles
// in one launch (adaptive_list) -- and this pass runs on that plane.  f64, one
// fixed order of operations, no transcendental function, so the GPU, the host build (tests/native/Makefile) and
// the numpy restatement (tests/adaptiveref.py) give the same bits.
//
// Window k = 1..K covers samples [e_{k-1}, e_k), e_k = min(k * window, max_samples), n_k = e_k - e_{k-1}; K >= 2.
// An element is one double of the frame (d_out's layout, the shard layout included); its state is three doubles of
// workspace: sum (the render's running sum), prev and q.  After window k's render, per element of an active tile:
//   S    = sum
//   b    = k == 1 ? S : S - prev             the window's batch sum
//   t    = (b * b) / (double)n_k
//   q    = k == 1 ? t : q + t
//   prev = S
// The tile is evaluated when k >= 2 and e_k >= min_samples.  Per pixel, with L = (0.2126, 0.7152, 0.0722):
//   m2_c  = q_c - (S_c * S_c) / (double)e_k
//   var_c = (m2_c < 0 ? 0 : m2_c) / D_k      D_k = (double)(k - 1) * (double)e_k, computed by the host; the clamp
//                                            keeps a NaN (m2 is never -0: q >= +0), so a NaN or inf sum reaches lhs
//   vl    = ((L0*L0) * var_0 + (L1*L1) * var_1) + (L2*L2) * var_2
//   l     = ((L0 * S_0 + L1 * S_1) + L2 * S_2) / (double)e_k
// Per tile, V and Lm are the sums of vl and l over the tile's 256 pixels (a pixel outside the frame gives +0.0) in
// a fixed balanced tree on the tile-local index i = lx + 16 * ly: for d = 1, 2, 4, ..., 128, a[i] = a[i] + a[i + d]
// for every i that is a multiple of 2d.  With nn = (double)(the tile's pixels inside the frame):
//   lhs  = V * nn
//   m    = Lm > floor * nn ? Lm : floor * nn
//   rhs  = (thr2 * m) * m                     thr2 = threshold * threshold, computed by the host
//   converged = lhs <= rhs                    (a NaN anywhere: false, so the tile runs to the cap)
//   err2 = lhs / (m * m)                      the tile's squared relative standard error
// The tile stops when it is converged or e_k == max_samples: every pixel inside the frame writes out_c = S_c /
// (double)e_k (wf_reduce's own division, so the pixel is the e_k-sample frame's) and var_c into the optional variance
// plane, a shard's padding pixel writes 0, and the tile writes tile_samples = e_k and tile_error = err2.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <vector>

#include "pt_device.hpp"
#include "pt_dims.hpp"

namespace pt {

constexpr size_t ADAPTIVE_WORK_PLANES = 3;  // sums, then prev, then q: `count` doubles each
constexpr double ADAPTIVE_L0 = 0.2126, ADAPTIVE_L1 = 0.7152, ADAPTIVE_L2 = 0.0722;
constexpr uint32_t ADAPTIVE_WINDOW = 8;         // the documented defaults (Python, pt_render)
constexpr double ADAPTIVE_FLOOR = 0.01;
constexpr uint32_t ADAPTIVE_MERGE_GAP = 1024;   // measured: DESIGN.md §3.10

namespace dev {

// One window's constants, from the host (adaptive_consts).
struct AdaptiveConsts {
    double nk;     // (double)n_k
    double ek;     // (double)e_k
    double d;      // (double)(k - 1) * (double)e_k
    double thr2;   // threshold * threshold
    double floor;  // luminance_floor
    uint32_t e_k;
    uint32_t evaluate;  // k >= 2 && e_k >= min_samples
    uint32_t cap;       // e_k == max_samples
};

// Where the tiles of a rank's list lie and how their pixels are kept: the tile geometry (pt_tiles.hpp) under this
// pass's own type name, which the kernel's and the launch's symbols carry.
struct AdaptiveGeom : TileGeom {};

// This pass's two views of it, in the tile-local index i = lx + 16 * ly that its threads and its tree run on: the
// element offset of pixel i of tile ti in d_out's layout, false outside the frame (a compact shard still has the
// offset: its padding); and the tile's pixels inside the frame.
PT_HD bool adaptive_pixel_at(const AdaptiveGeom &g, uint32_t ti, uint32_t i, size_t *at) {
    const TilePixel p = tile_pixel(g, ti, i & (TILE - 1), i / TILE);
    *at = p.at;
    return p.inside;
}
PT_HD uint32_t adaptive_tile_pixels(const AdaptiveGeom &g, uint32_t ti) { return tile_pixels_inside(g, ti); }

// One element after one window's render: S is its running sum; prev and q are not read when FIRST.  Returns q.
template <bool FIRST>
PT_HD double adaptive_element(double S, const AdaptiveConsts &k, double *prev, double *q) {
    const double b = FIRST ? S : S - *prev;
    const double t = (b * b) / k.nk;
    const double qn = FIRST ? t : *q + t;
    *q = qn;
    *prev = S;
    return qn;
}

// The variance of the element's mean after e_k samples.
PT_HD double adaptive_variance(double S, double q, const AdaptiveConsts &k) {
    const double m2 = q - (S * S) / k.ek;
    return (m2 < 0.0 ? 0.0 : m2) / k.d;  // a NaN stays a NaN: the tile then never passes as converged
}

// A pixel's share of the tile's two sums: the variance of its luminance's mean, and its mean luminance.
PT_HD void adaptive_pixel(const double S[3], const double var[3], const AdaptiveConsts &k, double *vl, double *l) {
    *vl = ((ADAPTIVE_L0 * ADAPTIVE_L0) * var[0] + (ADAPTIVE_L1 * ADAPTIVE_L1) * var[1]) +
          (ADAPTIVE_L2 * ADAPTIVE_L2) * var[2];
    *l = ((ADAPTIVE_L0 * S[0] + ADAPTIVE_L1 * S[1]) + ADAPTIVE_L2 * S[2]) / k.ek;
}

// The stop rule on the tile's sums; nn = (double)(pixels inside the frame).
PT_HD bool adaptive_converged(double V, double Lm, double nn, const AdaptiveConsts &k, double *err2) {
    const double lhs = V * nn;
    const double fl = k.floor * nn;
    const double m = Lm > fl ? Lm : fl;
    const double rhs = (k.thr2 * m) * m;
    *err2 = lhs / (m * m);
    return lhs <= rhs;
}

}  // namespace dev

// e_k: the end of window k (k = 0: 0).
inline uint32_t adaptive_edge(uint32_t k, uint32_t window, uint32_t max_samples) {
    const uint64_t e = (uint64_t)k * window;
    return e < max_samples ? (uint32_t)e : max_samples;
}

// K: the windows a frame has at most.
inline uint32_t adaptive_windows(uint32_t window, uint32_t max_samples) {
    return (uint32_t)(((uint64_t)max_samples + window - 1) / window);
}

inline dev::AdaptiveConsts adaptive_consts(uint32_t k, uint32_t window, uint32_t min_samples, uint32_t max_samples,
                                           double threshold, double luminance_floor) {
    const uint32_t e0 = adaptive_edge(k - 1, window, max_samples), e1 = adaptive_edge(k, window, max_samples);
    dev::AdaptiveConsts c;
    c.nk = (double)(e1 - e0);
    c.ek = (double)e1;
    c.d = (double)(k - 1) * (double)e1;
    c.thr2 = threshold * threshold;
    c.floor = luminance_floor;
    c.e_k = e1;
    c.evaluate = k >= 2 && e1 >= min_samples;
    c.cap = e1 == max_samples;
    return c;
}

// Doubles of workspace for `count` elements; 0 when the size does not fit.
inline size_t adaptive_workspace_doubles(uint64_t count) {
    if (count > (uint64_t)SIZE_MAX / (ADAPTIVE_WORK_PLANES * sizeof(double))) return 0;
    return (size_t)count * ADAPTIVE_WORK_PLANES;
}

// The render launches of one window: [begin, begin + count) ranges of the rank's tile list.  A run is a maximal
// stretch of active tiles (active[i] != 0); two runs are joined when at most merge_gap stopped tiles lie between
// them.  The runs ascend, start and end on an active tile and cover every active tile.
struct AdaptiveRun {
    uint32_t begin, count;
};
inline std::vector<AdaptiveRun> adaptive_runs(const uint8_t *active, uint32_t ntiles, uint32_t merge_gap) {
    std::vector<AdaptiveRun> runs;
    for (uint32_t i = 0; i < ntiles; i++) {
        if (!active[i]) continue;
        if (!runs.empty() && i - (runs.back().begin + runs.back().count) <= merge_gap)
            runs.back().count = i + 1 - runs.back().begin;
        else
            runs.push_back(AdaptiveRun{i, 1});
    }
    return runs;
}

// A listed launch's tiles (launch_render's `tiles`): n >= 1 entries of the rank's tile list, strictly
// ascending (so distinct: two chunks never write one pixel) and each below ntiles.
inline bool tile_list_ok(const uint32_t *list, size_t n, uint32_t ntiles) {
    if (!list || n < 1) return false;
    for (size_t i = 0; i < n; i++)
        if (list[i] >= ntiles || (i > 0 && list[i] <= list[i - 1])) return false;
    return true;
}

// The window's one listed launch: the active tiles, ascending.
inline std::vector<uint32_t> adaptive_list(const uint8_t *active, uint32_t ntiles) {
    std::vector<uint32_t> list;
    for (uint32_t i = 0; i < ntiles; i++)
        if (active[i]) list.push_back(i);
    return list;
}

// One window's pass over the `ntiles` tiles of the rank's list, queued on st: one launch of one 256-thread block per
// tile, no host sync, no allocation, no atomics.  work holds 3 * count doubles (sums, prev, q); out, tile_samples
// always, variance and tile_error when not null.  The first window marks every tile active (tile_samples = 0); a tile
// with tile_samples != 0 is neither read nor written.  The arguments are checked by the caller (pt_api.cpp).
hipError_t launch_adaptive_tiles(const dev::AdaptiveGeom &g, uint32_t ntiles, size_t count,
                                 const dev::AdaptiveConsts &k, bool first, double *work, double *out, double *variance,
                                 uint32_t *tile_samples, double *tile_error, hipStream_t st);

}  // namespace pt
