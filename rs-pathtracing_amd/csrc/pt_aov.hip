// pt_aov.hip — the guide-plane pass for MI355X (gfx950): first-hit albedo, normal and depth of a frame's own
// samples (pt_aov.hpp).  Its own translation unit and its own kernel: nothing of the render path is compiled
// here, and this object is not part of the render path's identity (PT_SRC_SHA, Makefile).
#include <hip/hip_runtime.h>

#include "pt_aov.hpp"

namespace pt {

using dev::V3;

// render_tiles' geometry and deal (pt_tiles.hpp), so a rank's shard of a plane lines up with its shard of the beauty
// frame: one workgroup = one tile of the rank's list, one pixel per lane; the tile is placed before the lanes, the
// order render_tiles computes them in.  The nine sums, the hit count and the minimum stay in registers; one write per
// wanted plane.  A null plane is neither computed nor stored (a kernel argument: the test is wave-uniform).  A lane
// that marches holds its wave here; trace_pixel's state machine avoids that, and this pass does without it (DESIGN.md
// §3.7 has the measured cost).
// Resources (gfx950, -O3): EXT 256 VGPRs + 14 AGPRs, 1 wave per SIMD; plain 189 VGPRs, 2 waves per SIMD; no
// scratch, no LDS in either.
template <bool EXT>
__global__ __launch_bounds__(256) void aov_tiles(dev::Scene sc, FrameParams P, double *__restrict__ albedo,
                                                 double *__restrict__ normal, double *__restrict__ depth) {
    const uint32_t ti = P.tile_begin + blockIdx.x;  // index in this rank's tile list
    const dev::TileGeom g = dev::tile_geom(P);
    const dev::Tile tile = dev::tile_of(g, ti);
    const dev::LanePixel lp = dev::lane_pixel(threadIdx.x);
    const dev::TilePixel px = dev::tile_pixel(g, tile, lp.lx, lp.ly);
    if (!px.inside && !P.compact) return;
    V3 a = dev::v3(0.0, 0.0, 0.0), n = a, d = a;  // a compact shard's pixels outside the frame
    if (px.inside) dev::aov_pixel<EXT>(sc, P, px.x, px.y, albedo != nullptr, normal != nullptr, &a, &n, &d);
    if (albedo) dev::store_rgb(albedo + px.at, 0, a);
    if (normal) dev::store_rgb(normal + px.at, 0, n);
    if (depth) dev::store_rgb(depth + px.at, 0, d);
}

hipError_t launch_aov(const dev::Scene &sc, const FrameParams &P, double *albedo, double *normal, double *depth,
                      hipStream_t st) {
    if (P.tile_count == 0) return hipSuccess;
    if (!albedo && !normal && !depth) return hipErrorInvalidValue;
    if (dev::aov_ext(sc)) aov_tiles<true><<<P.tile_count, 256, 0, st>>>(sc, P, albedo, normal, depth);
    else aov_tiles<false><<<P.tile_count, 256, 0, st>>>(sc, P, albedo, normal, depth);
    return hipGetLastError();
}

}  // namespace pt
