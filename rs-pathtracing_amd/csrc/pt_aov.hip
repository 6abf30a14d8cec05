// pt_aov.hip — the guide-plane pass for MI355X (gfx950): first-hit albedo, normal and depth of a frame's own
// samples (pt_aov.hpp).  Its own translation unit and its own kernel: nothing of the render path is compiled
// here, and this object is not part of the render path's identity (PT_SRC_SHA, Makefile).
#include <hip/hip_runtime.h>

#include "pt_aov.hpp"

namespace pt {

using dev::V3;

// render_tiles' geometry and deal, so a rank's shard of a plane lines up with its shard of the beauty frame: one
// workgroup = one 16x16 tile, 4 wave64s of 8x8 pixels, one pixel per lane, tile k -> rank k % world.  The nine sums,
// the hit count and the minimum stay in registers; one write per wanted plane.  A null plane is neither computed
// nor stored (a kernel argument: the test is wave-uniform).  A lane that marches holds its wave here; trace_pixel's
// state machine avoids that, and this pass does without it (DESIGN.md §3.7 has the measured cost).
// Resources (gfx950, -O3): EXT 256 VGPRs + 14 AGPRs, 1 wave per SIMD; plain 189 VGPRs, 2 waves per SIMD; no
// scratch, no LDS in either.
template <bool EXT>
__global__ __launch_bounds__(256) void aov_tiles(dev::Scene sc, FrameParams P, double *__restrict__ albedo,
                                                 double *__restrict__ normal, double *__restrict__ depth) {
    const uint32_t ti = P.tile_begin + blockIdx.x;  // index in this rank's tile list
    const uint32_t k = dev::tile_position(P.rank + ti * P.world, P.tiles_x, P.world);  // global tile id
    const uint32_t tx = k % P.tiles_x, ty = k / P.tiles_x;
    const uint32_t w = threadIdx.x >> 6, l = threadIdx.x & 63;
    const uint32_t lx = ((w & 1u) << 3) | (l & 7u), ly = ((w >> 1) << 3) | (l >> 3);
    const uint32_t x = tx * TILE + lx, y = ty * TILE + ly;
    const size_t at = P.compact ? ((size_t)ti * (TILE * TILE) + ly * TILE + lx) * 3 : ((size_t)y * P.width + x) * 3;
    const bool inside = x < P.width && y < P.height;
    if (!inside && !P.compact) return;
    V3 a = dev::v3(0.0, 0.0, 0.0), n = a, d = a;  // a compact shard's pixels outside the frame
    if (inside) dev::aov_pixel<EXT>(sc, P, x, y, albedo != nullptr, normal != nullptr, &a, &n, &d);
    if (albedo) dev::store_rgb(albedo + at, 0, a);
    if (normal) dev::store_rgb(normal + at, 0, n);
    if (depth) dev::store_rgb(depth + at, 0, d);
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
