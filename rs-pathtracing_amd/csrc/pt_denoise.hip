// pt_denoise.hip — the guided à-trous denoiser for MI355X (gfx950): the kernels of pt_denoise.hpp.  Its own
// translation unit and its own kernels: nothing of the render path is compiled here, and this object is not part of
// the render path's identity (PT_SRC_SHA, Makefile).
#include <hip/hip_runtime.h>

#include "pt_denoise.hpp"
#include "pt_tiles.hpp"

namespace pt {

using dev::DRec;

// One thread per pixel: the four frames (24-byte pixels) become the 32-byte work records.
__global__ __launch_bounds__(256) void denoise_records(const double *__restrict__ rgb, const double *__restrict__ albedo,
                                                       const double *__restrict__ normal,
                                                       const double *__restrict__ depth, uint32_t flags, size_t npix,
                                                       DRec *__restrict__ u, DRec *__restrict__ g) {
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p < npix) dev::denoise_prepare(rgb, albedo, normal, depth, flags, p, u, g);
}

// One iteration.  The whole frame in pt_tiles.hpp's geometry: one workgroup = one 16x16 tile, 8x8 pixels per wave64,
// so each tap row of a wave is one contiguous run of 8 records (256 bytes), and every tap is 16-byte loads.  The
// stride is a kernel argument; the colour term is a template argument (off, the default, does not pay for xc);
// LAST fuses the remodulation and writes the frame instead of the next colour buffer.
// Resources (gfx950, -O3): colour off 58 VGPRs (LAST 54), colour on 62; 0 AGPRs, no scratch, no LDS, 8 waves per
// SIMD in all four builds (denoise_records: 40 VGPRs).  Measured at 1920x1080, 5 iterations: 0.96 ms in all,
// 150 to 245 us per launch.
template <bool COLOUR, bool LAST>
__global__ __launch_bounds__(256) void denoise_tiles(const DRec *__restrict__ u, const DRec *__restrict__ g,
                                                     uint32_t w, uint32_t h, uint32_t tiles_x, uint32_t s, double rn,
                                                     double rz, double rc, DRec *__restrict__ u_next,
                                                     const double *__restrict__ albedo, uint32_t flags,
                                                     double *__restrict__ out) {
    const dev::LanePixel lp = dev::lane_pixel(threadIdx.x);
    const dev::TilePixel px = dev::tile_pixel(dev::whole_frame(w, h, tiles_x), blockIdx.x, lp.lx, lp.ly);
    if (!px.inside) return;
    const uint32_t x = px.x, y = px.y;
    const DRec v = dev::denoise_pixel<COLOUR>(u, g, w, h, x, y, s, rn, rz, rc);
    const size_t p = (size_t)y * w + x;
    if (LAST) dev::denoise_finish(v, albedo, flags, p, out);
    else u_next[p] = v;
}

// ---- the variance term (pt_denoise.hpp): kernels of its own beside the ones above ----
__global__ __launch_bounds__(256) void denoise_records_variance(
    const double *__restrict__ rgb, const double *__restrict__ albedo, const double *__restrict__ normal,
    const double *__restrict__ depth, const double *__restrict__ variance, uint32_t flags, size_t npix,
    DRec *__restrict__ u, DRec *__restrict__ g) {
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p < npix) dev::denoise_prepare_variance(rgb, albedo, normal, depth, variance, flags, p, u, g);
}

// denoise_tiles' geometry; the colour record's fourth slot is read (25 taps and the 9 of the prefilter) and written.
// Resources (gfx950, -O3): 78 VGPRs (LAST 70), 0 AGPRs, no scratch, no LDS, 6 waves per SIMD (LAST 7);
// denoise_records_variance 46 VGPRs.  The kernels above keep theirs (58, 54, 62, 40).
template <bool LAST>
__global__ __launch_bounds__(256) void denoise_tiles_variance(const DRec *__restrict__ u, const DRec *__restrict__ g,
                                                              uint32_t w, uint32_t h, uint32_t tiles_x, uint32_t s,
                                                              double rn, double rz, double rv,
                                                              DRec *__restrict__ u_next,
                                                              const double *__restrict__ albedo, uint32_t flags,
                                                              double *__restrict__ out) {
    const dev::LanePixel lp = dev::lane_pixel(threadIdx.x);
    const dev::TilePixel px = dev::tile_pixel(dev::whole_frame(w, h, tiles_x), blockIdx.x, lp.lx, lp.ly);
    if (!px.inside) return;
    const uint32_t x = px.x, y = px.y;
    const DRec v = dev::denoise_pixel_variance(u, g, w, h, x, y, s, rn, rz, rv);
    const size_t p = (size_t)y * w + x;
    if (LAST) dev::denoise_finish(v, albedo, flags, p, out);
    else u_next[p] = v;
}

// Both filters: the frame's records, then `iterations` launches that ping-pong the colour buffer, the last of which
// writes the frame.  variance is null for the plain filter (its colour term as k.colour says), else the plane of the
// variance-guided one, whose every iteration takes rv where the plain filter takes k.rc[i].
using TilesKernel = void (*)(const DRec *, const DRec *, uint32_t, uint32_t, uint32_t, uint32_t, double, double, double,
                             DRec *, const double *, uint32_t, double *);
static hipError_t launch_filter(const double *rgb, const double *albedo, const double *normal, const double *depth,
                                const double *variance, uint32_t w, uint32_t h, uint32_t iterations,
                                const dev::DenoiseConsts &k, double rv, uint32_t flags, double *out, double *work,
                                hipStream_t st) {
    const size_t npix = (size_t)w * h;
    // the tile grid and the prepare grid are 32-bit
    if (npix == 0 || iterations == 0 || iterations > DENOISE_MAX_ITERATIONS || !tile_grid_ok(w, h))
        return hipErrorInvalidValue;
    const uint32_t tiles_x = tiles_across(w), tiles = tiles_x * tiles_across(h);
    DRec *u0 = (DRec *)work, *u1 = u0 + npix, *g = u1 + npix;
    const unsigned blocks = (unsigned)((npix + 255) / 256);
    if (variance)
        denoise_records_variance<<<blocks, 256, 0, st>>>(rgb, albedo, normal, depth, variance, flags, npix, u0, g);
    else
        denoise_records<<<blocks, 256, 0, st>>>(rgb, albedo, normal, depth, flags, npix, u0, g);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    static const TilesKernel tiles_kernel[3][2] = {  // [filter][the last iteration]
        {denoise_tiles<true, false>, denoise_tiles<true, true>},
        {denoise_tiles<false, false>, denoise_tiles<false, true>},
        {denoise_tiles_variance<false>, denoise_tiles_variance<true>}};
    const TilesKernel *const kernel = tiles_kernel[variance ? 2 : k.colour ? 0 : 1];
    for (uint32_t i = 0; i < iterations; i++) {
        const DRec *src = i & 1u ? u1 : u0;
        DRec *dst = i & 1u ? u0 : u1;
        const double r = variance ? rv : k.rc[i];
        if (i + 1 < iterations)
            kernel[0]<<<tiles, 256, 0, st>>>(src, g, w, h, tiles_x, 1u << i, k.rn, k.rz, r, dst, nullptr, flags, nullptr);
        else
            kernel[1]<<<tiles, 256, 0, st>>>(src, g, w, h, tiles_x, 1u << i, k.rn, k.rz, r, nullptr, albedo, flags, out);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_denoise(const double *rgb, const double *albedo, const double *normal, const double *depth,
                          uint32_t w, uint32_t h, uint32_t iterations, const dev::DenoiseConsts &k, uint32_t flags,
                          double *out, double *work, hipStream_t st) {
    return launch_filter(rgb, albedo, normal, depth, nullptr, w, h, iterations, k, 0.0, flags, out, work, st);
}

hipError_t launch_denoise_variance(const double *rgb, const double *albedo, const double *normal, const double *depth,
                                   const double *variance, uint32_t w, uint32_t h, uint32_t iterations,
                                   const dev::DenoiseConsts &k, double rv, uint32_t flags, double *out, double *work,
                                   hipStream_t st) {
    if (!variance) return hipErrorInvalidValue;
    return launch_filter(rgb, albedo, normal, depth, variance, w, h, iterations, k, rv, flags, out, work, st);
}

}  // namespace pt
