// pt_temporal.hip — temporal accumulation for MI355X (gfx950): the kernel of pt_temporal.hpp.  Its own translation
// unit and its own kernel: nothing of the render path is compiled here, and this object is not part of the render
// path's identity (PT_SRC_SHA, Makefile).
#include <hip/hip_runtime.h>

#include "pt_temporal.hpp"
#include "pt_tiles.hpp"

namespace pt {

using dev::DRec;

// The whole pass, over the whole frame in pt_tiles.hpp's geometry: one workgroup = one 16x16 tile, 8x8 pixels per
// wave64.  A small camera motion maps a wave's 8x8 pixels onto a patch of about 9x9 history pixels, so its four taps
// fall into a few contiguous runs of records; every record access is a 16-byte load or store, the three frames are
// read and the frame written as 8-byte accesses of 24-byte pixels.  FIRST is the first frame: every pixel resets and
// the previous history is not read (its pointers are null).  rgb and out may be the same buffer (each lane reads its
// own pixel before it writes it), so neither is __restrict__.  No LDS, no atomics.
// Resources (gfx950, -O3): the steady build 67 VGPRs, 62 SGPRs, 7 waves per SIMD; the first-frame build 30 VGPRs,
// 8 waves per SIMD; both 0 AGPRs, no scratch, no LDS.  Measured times: DESIGN.md §3.12.
template <bool FIRST>
__global__ __launch_bounds__(256) void temporal_tiles(const double *rgb, const double *__restrict__ normal,
                                                      const double *__restrict__ depth, const DRec *__restrict__ hc,
                                                      const DRec *__restrict__ hg, uint32_t w, uint32_t h,
                                                      uint32_t tiles_x, dev::TemporalConsts k, DRec *__restrict__ oc,
                                                      DRec *__restrict__ og, double *out) {
    const dev::LanePixel lp = dev::lane_pixel(threadIdx.x);
    const dev::TilePixel px = dev::tile_pixel(dev::whole_frame(w, h, tiles_x), blockIdx.x, lp.lx, lp.ly);
    if (!px.inside) return;
    const uint32_t x = px.x, y = px.y;
    DRec c, g;
    dev::temporal_pixel<FIRST>(rgb, normal, depth, hc, hg, w, h, x, y, k, &c, &g);
    const size_t p = (size_t)y * w + x;
    out[p * 3] = c.a;
    out[p * 3 + 1] = c.b;
    out[p * 3 + 2] = c.c;
    oc[p] = c;
    og[p] = g;
}

hipError_t launch_temporal(const double *rgb, const double *normal, const double *depth, uint32_t w, uint32_t h,
                           const dev::TemporalConsts &k, const double *history_in, double *history_out, double *out,
                           hipStream_t st) {
    const size_t npix = (size_t)w * h;
    if (npix == 0 || !tile_grid_ok(w, h)) return hipErrorInvalidValue;  // the tile grid is 32-bit
    const uint32_t tiles_x = tiles_across(w), tiles = tiles_x * tiles_across(h);
    DRec *oc = (DRec *)history_out, *og = oc + npix;
    if (history_in) {
        const DRec *hc = (const DRec *)history_in, *hg = hc + npix;
        temporal_tiles<false><<<tiles, 256, 0, st>>>(rgb, normal, depth, hc, hg, w, h, tiles_x, k, oc, og, out);
    } else {
        temporal_tiles<true><<<tiles, 256, 0, st>>>(rgb, normal, depth, nullptr, nullptr, w, h, tiles_x, k, oc, og, out);
    }
    return hipGetLastError();
}

}  // namespace pt
