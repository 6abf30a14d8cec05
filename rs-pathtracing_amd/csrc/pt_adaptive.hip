// pt_adaptive.hip — the per-tile error and stop rule of adaptive sampling for MI355X (gfx950): the kernel of
// pt_adaptive.hpp.  Its own translation unit: nothing of the render path is compiled here, and this object is not
// part of the render path's identity (PT_SRC_SHA, Makefile).
#include <hip/hip_runtime.h>

#include "pt_adaptive.hpp"

namespace pt {

// One workgroup = one 16x16 tile of the rank's list, placed by pt_tiles.hpp, but not its lane_pixel: thread t owns the
// pixel of tile-local index i = t = lx + 16 * ly (the tree below runs on i), so wave w holds i in [64w, 64w + 64) and
// a row of the tile is one run of 384 bytes.
// A stopped tile's block returns at once: tile_samples[ti] is one word, the same for the whole block.  The two tile
// sums run together: steps 1..32 of the tree are shuffles inside the wave (lane i takes lane i + d's value; only the
// lanes that are multiples of 2d hold tree values afterwards, and only lane 0's is used), steps 64 and 128 are the
// four wave partials through 64 bytes of LDS, as (p0 + p1) + (p2 + p3), behind one barrier.  Every thread reads the
// four partials (a broadcast) and takes the same decision.  No atomics.  FIRST (k == 1) reads neither prev nor q,
// never evaluates, and marks the tile active.
// Resources (gfx950, -O3): FIRST 38 VGPRs, else 32; 0 AGPRs, no scratch, 64 bytes of LDS (FIRST: none), 8 waves per
// SIMD.
template <bool FIRST>
__global__ __launch_bounds__(256) void adaptive_tiles(dev::AdaptiveGeom g, dev::AdaptiveConsts k,
                                                      const double *__restrict__ sums, double *__restrict__ prev,
                                                      double *__restrict__ q, double *__restrict__ out,
                                                      double *__restrict__ variance, uint32_t *tile_samples,
                                                      double *__restrict__ tile_error) {
    const uint32_t ti = blockIdx.x, i = threadIdx.x;
    if (!FIRST && tile_samples[ti] != 0) return;  // stopped: its pixels are in `out`
    size_t at;
    const bool inside = dev::adaptive_pixel_at(g, ti, i, &at);
    const bool evaluate = !FIRST && k.evaluate != 0;
    double S[3] = {0.0, 0.0, 0.0}, var[3] = {0.0, 0.0, 0.0}, vl = 0.0, l = 0.0;  // outside the frame: +0.0
    if (inside) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            S[c] = sums[at + c];
            const double qn = dev::adaptive_element<FIRST>(S[c], k, &prev[at + c], &q[at + c]);
            if (evaluate) var[c] = dev::adaptive_variance(S[c], qn, k);
        }
        if (evaluate) dev::adaptive_pixel(S, var, k, &vl, &l);
    }
    if (FIRST) {
        if (i == 0) tile_samples[ti] = 0;
        return;
    }
    if (!evaluate) return;  // (a kernel argument: uniform)
    __shared__ double part[2][4];
#pragma unroll
    for (int d = 1; d <= 32; d <<= 1) {
        vl = vl + __shfl_down(vl, d, 64);
        l = l + __shfl_down(l, d, 64);
    }
    if ((i & 63u) == 0) {
        part[0][i >> 6] = vl;
        part[1][i >> 6] = l;
    }
    __syncthreads();
    const double V = (part[0][0] + part[0][1]) + (part[0][2] + part[0][3]);
    const double Lm = (part[1][0] + part[1][1]) + (part[1][2] + part[1][3]);
    double err2;
    const bool converged = dev::adaptive_converged(V, Lm, (double)dev::adaptive_tile_pixels(g, ti), k, &err2);
    if (!converged && !k.cap) return;
    if (inside) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            out[at + c] = S[c] / k.ek;
            if (variance) variance[at + c] = var[c];
        }
    } else if (g.compact) {  // a shard's padding
#pragma unroll
        for (int c = 0; c < 3; c++) {
            out[at + c] = 0.0;
            if (variance) variance[at + c] = 0.0;
        }
    }
    // every thread of the block read tile_samples[ti] before the barrier above
    if (i == 0) {
        tile_samples[ti] = k.e_k;
        if (tile_error) tile_error[ti] = err2;
    }
}

hipError_t launch_adaptive_tiles(const dev::AdaptiveGeom &g, uint32_t ntiles, size_t count,
                                 const dev::AdaptiveConsts &k, bool first, double *work, double *out, double *variance,
                                 uint32_t *tile_samples, double *tile_error, hipStream_t st) {
    if (ntiles == 0 || count == 0 || !work || !out || !tile_samples) return hipErrorInvalidValue;
    double *sums = work, *prev = work + count, *q = prev + count;
    uint32_t *ts = tile_samples;
    if (first) adaptive_tiles<true><<<ntiles, 256, 0, st>>>(g, k, sums, prev, q, out, variance, ts, tile_error);
    else adaptive_tiles<false><<<ntiles, 256, 0, st>>>(g, k, sums, prev, q, out, variance, ts, tile_error);
    return hipGetLastError();
}

}  // namespace pt
