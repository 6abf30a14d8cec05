// pt_denoise.hip — the guided à-trous denoiser for MI355X (gfx950): the kernels of pt_denoise.hpp.  Its own
// translation unit and its own kernels: nothing of the render path is compiled here, and this object is not part of
// the render path's identity (PT_SRC_SHA, Makefile).
#include <hip/hip_runtime.h>

#include "pt_denoise.hpp"
#include "pt_dims.hpp"

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

// One iteration.  aov_tiles' geometry: one workgroup = one 16x16 tile, 4 wave64s of 8x8 pixels, one pixel per lane,
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
    const uint32_t tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
    const uint32_t wv = threadIdx.x >> 6, l = threadIdx.x & 63;
    const uint32_t lx = ((wv & 1u) << 3) | (l & 7u), ly = ((wv >> 1) << 3) | (l >> 3);
    const uint32_t x = tx * TILE + lx, y = ty * TILE + ly;
    if (x >= w || y >= h) return;
    const DRec v = dev::denoise_pixel<COLOUR>(u, g, w, h, x, y, s, rn, rz, rc);
    const size_t p = (size_t)y * w + x;
    if (LAST) dev::denoise_finish(v, albedo, flags, p, out);
    else u_next[p] = v;
}

template <bool COLOUR>
static hipError_t launch_iterations(const double *albedo, uint32_t w, uint32_t h, uint32_t iterations,
                                    const dev::DenoiseConsts &k, uint32_t flags, double *out, DRec *u0, DRec *u1,
                                    const DRec *g, hipStream_t st) {
    const uint32_t tiles_x = (w + TILE - 1) / TILE, tiles_y = (h + TILE - 1) / TILE;
    const uint32_t tiles = tiles_x * tiles_y;
    for (uint32_t i = 0; i < iterations; i++) {
        const DRec *src = i & 1u ? u1 : u0;
        DRec *dst = i & 1u ? u0 : u1;
        if (i + 1 < iterations)
            denoise_tiles<COLOUR, false><<<tiles, 256, 0, st>>>(src, g, w, h, tiles_x, 1u << i, k.rn, k.rz, k.rc[i], dst,
                                                                nullptr, flags, nullptr);
        else
            denoise_tiles<COLOUR, true><<<tiles, 256, 0, st>>>(src, g, w, h, tiles_x, 1u << i, k.rn, k.rz, k.rc[i],
                                                               nullptr, albedo, flags, out);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_denoise(const double *rgb, const double *albedo, const double *normal, const double *depth,
                          uint32_t w, uint32_t h, uint32_t iterations, const dev::DenoiseConsts &k, uint32_t flags,
                          double *out, double *work, hipStream_t st) {
    const size_t npix = (size_t)w * h;
    // the tile grid and the prepare grid are 32-bit
    const uint64_t tiles = (uint64_t)((w + TILE - 1) / TILE) * ((h + TILE - 1) / TILE);
    if (npix == 0 || iterations == 0 || iterations > DENOISE_MAX_ITERATIONS || tiles > 0x7fffffffull)
        return hipErrorInvalidValue;
    DRec *u0 = (DRec *)work, *u1 = u0 + npix, *g = u1 + npix;
    denoise_records<<<(unsigned)((npix + 255) / 256), 256, 0, st>>>(rgb, albedo, normal, depth, flags, npix, u0, g);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return k.colour ? launch_iterations<true>(albedo, w, h, iterations, k, flags, out, u0, u1, g, st)
                    : launch_iterations<false>(albedo, w, h, iterations, k, flags, out, u0, u1, g, st);
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
    const uint32_t tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
    const uint32_t wv = threadIdx.x >> 6, l = threadIdx.x & 63;
    const uint32_t lx = ((wv & 1u) << 3) | (l & 7u), ly = ((wv >> 1) << 3) | (l >> 3);
    const uint32_t x = tx * TILE + lx, y = ty * TILE + ly;
    if (x >= w || y >= h) return;
    const DRec v = dev::denoise_pixel_variance(u, g, w, h, x, y, s, rn, rz, rv);
    const size_t p = (size_t)y * w + x;
    if (LAST) dev::denoise_finish(v, albedo, flags, p, out);
    else u_next[p] = v;
}

hipError_t launch_denoise_variance(const double *rgb, const double *albedo, const double *normal, const double *depth,
                                   const double *variance, uint32_t w, uint32_t h, uint32_t iterations,
                                   const dev::DenoiseConsts &k, double rv, uint32_t flags, double *out, double *work,
                                   hipStream_t st) {
    const size_t npix = (size_t)w * h;
    const uint32_t tiles_x = (w + TILE - 1) / TILE, tiles_y = (h + TILE - 1) / TILE;
    const uint64_t tiles = (uint64_t)tiles_x * tiles_y;
    if (npix == 0 || iterations == 0 || iterations > DENOISE_MAX_ITERATIONS || tiles > 0x7fffffffull)
        return hipErrorInvalidValue;
    DRec *u0 = (DRec *)work, *u1 = u0 + npix, *g = u1 + npix;
    denoise_records_variance<<<(unsigned)((npix + 255) / 256), 256, 0, st>>>(rgb, albedo, normal, depth, variance, flags,
                                                                             npix, u0, g);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    for (uint32_t i = 0; i < iterations; i++) {
        const DRec *src = i & 1u ? u1 : u0;
        DRec *dst = i & 1u ? u0 : u1;
        if (i + 1 < iterations)
            denoise_tiles_variance<false><<<(unsigned)tiles, 256, 0, st>>>(src, g, w, h, tiles_x, 1u << i, k.rn, k.rz, rv,
                                                                           dst, nullptr, flags, nullptr);
        else
            denoise_tiles_variance<true><<<(unsigned)tiles, 256, 0, st>>>(src, g, w, h, tiles_x, 1u << i, k.rn, k.rz, rv,
                                                                          nullptr, albedo, flags, out);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace pt
