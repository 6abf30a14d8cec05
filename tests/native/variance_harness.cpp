// Test-only host build of the variance accumulation (dev::variance_element, pt_variance.hpp) and of the denoiser's
// variance term (dev::denoise_prepare_variance, dev::denoise_pixel_variance, dev::denoise_finish, pt_denoise.hpp):
// the functions the variance_window, denoise_records_variance and denoise_tiles_variance kernels run per lane,
// compiled for the CPU and run over every element or pixel in the launches' order, with the host's own constants.
// tests/test_variance_host.py compares the results with tests/varianceref.py bit for bit.  Never used by the product.
#include <vector>

#include "../../rs-pathtracing_amd/csrc/pt_denoise.hpp"
#include "../../rs-pathtracing_amd/csrc/pt_variance.hpp"

using namespace pt;

template <bool FIRST, bool LAST>
static void window_on_host(const double *out, size_t count, const dev::VarConsts &k, double *prev, double *q,
                           double *variance) {
    for (size_t i = 0; i < count; i++) {
        double v = 0.0;
        dev::variance_element<FIRST, LAST>(out[i], k, &prev[i], &q[i], &v);
        if (LAST) variance[i] = v;
    }
}

// pt_variance_window_device's arguments (checked by the caller); returns the doubles of workspace it used.
extern "C" size_t vr_window(const double *out, size_t count, uint32_t n_k, uint32_t samples, uint32_t window,
                            uint32_t windows, double *work, double *variance) {
    const dev::VarConsts k = variance_consts(n_k, samples, windows);
    double *prev = work, *q = work + count;
    if (window == 1) window_on_host<true, false>(out, count, k, prev, q, variance);
    else if (window == windows) window_on_host<false, true>(out, count, k, prev, q, variance);
    else window_on_host<false, false>(out, count, k, prev, q, variance);
    return variance_workspace_doubles(count);
}

extern "C" uint32_t vr_edge(uint32_t k, uint32_t samples, uint32_t windows) { return variance_edge(k, samples, windows); }

// pt_denoise_variance's arguments (checked by the caller), w*h*3 doubles into out, which may be rgb.  Returns the
// doubles of workspace it used.
extern "C" size_t vr_denoise(const double *rgb, const double *albedo, const double *normal, const double *depth,
                             const double *variance, uint32_t w, uint32_t h, uint32_t iterations, double sigma_normal,
                             double sigma_depth, double sigma_variance, uint32_t flags, double *out) {
    const size_t npix = (size_t)w * h;
    std::vector<dev::DRec> work(npix * DENOISE_WORK_RECORDS);
    dev::DRec *u0 = work.data(), *u1 = u0 + npix, *g = u1 + npix;
    const dev::DenoiseConsts k = denoise_consts(iterations, sigma_normal, sigma_depth, 0.0);
    const double rv = denoise_variance_rv(sigma_variance);
    for (size_t p = 0; p < npix; p++) dev::denoise_prepare_variance(rgb, albedo, normal, depth, variance, flags, p, u0, g);
    for (uint32_t i = 0; i < iterations; i++) {
        const dev::DRec *src = i & 1u ? u1 : u0;
        dev::DRec *dst = i & 1u ? u0 : u1;
        for (uint32_t y = 0; y < h; y++)
            for (uint32_t x = 0; x < w; x++) {
                const dev::DRec v = dev::denoise_pixel_variance(src, g, w, h, x, y, 1u << i, k.rn, k.rz, rv);
                const size_t p = (size_t)y * w + x;
                if (i + 1 < iterations) dst[p] = v;
                else dev::denoise_finish(v, albedo, flags, p, out);
            }
    }
    return denoise_workspace_doubles(w, h);
}
