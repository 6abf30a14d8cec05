// Test-only host build of the temporal accumulation: dev::temporal_pixel (pt_temporal.hpp), the function the
// temporal_tiles kernel runs per lane, compiled for the CPU and run over every pixel of a frame, with the host's own
// constants (temporal_consts).  The caster values come from the caller (the product derives them with caster_params).
// tests/test_temporal_host.py compares the frame and the history with tests/temporalref.py bit for bit.  Never used
// by the product.
#include "../../rs-pathtracing_amd/csrc/pt_temporal.hpp"

using namespace pt;

// 17 doubles per camera: pos, right, up, left_top, res, direction, focal length
static dev::TemporalCam cam_of(const double *c) {
    dev::TemporalCam t;
    for (int k = 0; k < 3; k++) {
        t.pos[k] = c[k];
        t.right[k] = c[3 + k];
        t.up[k] = c[6 + k];
        t.lt[k] = c[9 + k];
    }
    t.res = c[12];
    return t;
}

// pt_temporal's frame and history (arguments checked by the caller), out may be rgb; prev and history_in are both
// null on the first frame.  Returns the doubles of one history.
extern "C" size_t tp_temporal(const double *rgb, const double *normal, const double *depth, const double *cam,
                              const double *prev, uint32_t w, uint32_t h, const double *history_in,
                              double *history_out, uint32_t max_count, double sigma_normal, double sigma_depth,
                              double *out) {
    const size_t npix = (size_t)w * h;
    const dev::TemporalCam now = cam_of(cam);
    dev::TemporalCam before{};
    if (prev) before = cam_of(prev);
    const dev::TemporalConsts k = temporal_consts(now, prev ? &before : nullptr, prev ? prev + 13 : nullptr,
                                                  prev ? prev[16] : 0.0, max_count, sigma_normal, sigma_depth);
    const dev::DRec *hc = (const dev::DRec *)history_in, *hg = hc ? hc + npix : nullptr;
    dev::DRec *oc = (dev::DRec *)history_out, *og = oc + npix;
    for (uint32_t y = 0; y < h; y++)
        for (uint32_t x = 0; x < w; x++) {
            dev::DRec c, g;
            if (history_in) dev::temporal_pixel<false>(rgb, normal, depth, hc, hg, w, h, x, y, k, &c, &g);
            else dev::temporal_pixel<true>(rgb, normal, depth, nullptr, nullptr, w, h, x, y, k, &c, &g);
            const size_t p = (size_t)y * w + x;
            out[p * 3] = c.a;
            out[p * 3 + 1] = c.b;
            out[p * 3 + 2] = c.c;
            oc[p] = c;
            og[p] = g;
        }
    return temporal_history_doubles(w, h);
}
