// pt_denoise.hpp — the guided denoiser for a beauty frame and its guide planes: an edge-avoiding
// à-trous wavelet filter (Dammertz et al. 2010) in f64, with no transcendental function and a fixed summation
// order, so the GPU, the host build (tests/native/Makefile) and the numpy restatement (tests/denoiseref.py) give
// the same bits.  A pass of its own: it reads four whole frames in the colour buffer's layout (world == 1), knows
// nothing of scenes or renderers, and the render kernels do not know about it.
//
// Per pixel p: colour c, albedo a, normal n (the guide plane's mean, not renormalised), z = depth[0] (the mean t).
//   prepare   den_k = a_k > 1e-3 ? a_k : 1.0 and u_k = c_k / den_k (PT_DENOISE_DEMODULATE; else den = 1, u = c);
//             the work records are {u0, u1, u2, 0} and {n0, n1, n2, z}
//   iteration i (stride s = 1 << i), reading iteration i-1's u whole: over dy = -2..2 (outer), dx = -2..2 (inner),
//             q = p + s*(dx, dy), a tap outside the frame skipped:
//               h = K[|dx|] * K[|dy|], K = {3/8, 1/4, 1/16}
//               xn = ((dn0*dn0 + dn1*dn1) + dn2*dn2) * rn, dn = n(p) - n(q)
//               t = (z(p) - z(q)) * r(p), r(p) = z(p) > 0 ? 1.0 / z(p) : 0.0;  xz = (t*t) * rz
//               f(x) = m*m, m = max(0.0, 1.0 - x)
//               w = (h * f(xn)) * f(xz); with the colour term, w = w * f(xc),
//                   xc = ((du0*du0 + du1*du1) + du2*du2) * rc_i, du = u(p) - u(q)
//               acc_k = acc_k + w * u_k(q);  ws = ws + w
//             u_k(p) = acc_k / ws (the centre tap weighs 9/64, so ws > 0)
//   finish    out_k = u_k * den_k
// The host computes rn = 1 / (sigma_normal^2), rz = 1 / (sigma_depth^2) and, with sigma_colour > 0,
// rc_i = 1 / (sc_i * sc_i), sc_i = sigma_colour / (double)s, in double (denoise_consts).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "pt_dims.hpp"

namespace pt {

constexpr uint32_t DENOISE_DEMODULATE = 1u;     // PT_DENOISE_DEMODULATE
constexpr uint32_t DENOISE_MAX_ITERATIONS = 8;  // PT_DENOISE_MAX_ITERATIONS
constexpr size_t DENOISE_WORK_RECORDS = 3;      // per pixel: two colour records (ping-pong) and one guide record

namespace dev {

// A 32-byte work record, read and written as two 16-byte accesses: the colour {u0, u1, u2, 0} or the guide
// {n0, n1, n2, z}.
struct alignas(16) DRec {
    double a, b, c, d;
};

struct DenoiseConsts {
    double rn, rz;
    double rc[DENOISE_MAX_ITERATIONS];  // per iteration; read only with the colour term
    bool colour;
};

PT_HD double denoise_den(double a) { return a > 1e-3 ? a : 1.0; }
PT_HD double denoise_f(double x) {
    const double v = 1.0 - x;
    const double m = v > 0.0 ? v : 0.0;
    return m * m;
}

// Pixel p's two work records from the four frames (albedo is read only with the flag).
PT_HD void denoise_prepare(const double *rgb, const double *albedo, const double *normal, const double *depth,
                           uint32_t flags, size_t p, DRec *u, DRec *g) {
    double c0 = rgb[p * 3], c1 = rgb[p * 3 + 1], c2 = rgb[p * 3 + 2];
    if (flags & DENOISE_DEMODULATE) {
        c0 = c0 / denoise_den(albedo[p * 3]);
        c1 = c1 / denoise_den(albedo[p * 3 + 1]);
        c2 = c2 / denoise_den(albedo[p * 3 + 2]);
    }
    u[p] = DRec{c0, c1, c2, 0.0};
    g[p] = DRec{normal[p * 3], normal[p * 3 + 1], normal[p * 3 + 2], depth[p * 3]};
}

// One iteration's new colour of pixel (x, y): the 25 taps in the order above.  A tap's records are loaded at an
// index clamped into the frame, so the loads do not wait for the test; a tap outside adds nothing.
template <bool COLOUR>
PT_HD DRec denoise_pixel(const DRec *__restrict__ u, const DRec *__restrict__ g, uint32_t w, uint32_t h, uint32_t x,
                         uint32_t y, uint32_t s, double rn, double rz, double rc) {
    const double K[3] = {3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0};
    const size_t p = (size_t)y * w + x;
    const DRec gp = g[p];
    const DRec up = COLOUR ? u[p] : DRec{0.0, 0.0, 0.0, 0.0};
    const double r = gp.d > 0.0 ? 1.0 / gp.d : 0.0;
    double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0, ws = 0.0;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
        const int64_t qy = (int64_t)y + (int64_t)s * dy;
        const bool iny = qy >= 0 && qy < (int64_t)h;
        const size_t row = (size_t)(iny ? qy : (int64_t)y) * w;
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const int64_t qx = (int64_t)x + (int64_t)s * dx;
            const bool in = iny && qx >= 0 && qx < (int64_t)w;
            const size_t q = row + (size_t)(in ? qx : (int64_t)x);
            const DRec gq = g[q];
            const DRec uq = u[q];
            if (!in) continue;
            const double hk = K[dx < 0 ? -dx : dx] * K[dy < 0 ? -dy : dy];
            const double dn0 = gp.a - gq.a, dn1 = gp.b - gq.b, dn2 = gp.c - gq.c;
            const double xn = ((dn0 * dn0 + dn1 * dn1) + dn2 * dn2) * rn;
            const double t = (gp.d - gq.d) * r;
            const double xz = (t * t) * rz;
            double wt = (hk * denoise_f(xn)) * denoise_f(xz);
            if (COLOUR) {
                const double du0 = up.a - uq.a, du1 = up.b - uq.b, du2 = up.c - uq.c;
                const double xc = ((du0 * du0 + du1 * du1) + du2 * du2) * rc;
                wt = wt * denoise_f(xc);
            }
            acc0 = acc0 + wt * uq.a;
            acc1 = acc1 + wt * uq.b;
            acc2 = acc2 + wt * uq.c;
            ws = ws + wt;
        }
    }
    return DRec{acc0 / ws, acc1 / ws, acc2 / ws, 0.0};
}

// The frame's value of pixel p from the last iteration's colour: den is recomputed from the albedo.
PT_HD void denoise_finish(DRec u, const double *albedo, uint32_t flags, size_t p, double *out) {
    double d0 = 1.0, d1 = 1.0, d2 = 1.0;
    if (flags & DENOISE_DEMODULATE) {
        d0 = denoise_den(albedo[p * 3]);
        d1 = denoise_den(albedo[p * 3 + 1]);
        d2 = denoise_den(albedo[p * 3 + 2]);
    }
    out[p * 3] = u.a * d0;
    out[p * 3 + 1] = u.b * d1;
    out[p * 3 + 2] = u.c * d2;
}

// ---- the variance term: a colour weight scaled by each pixel's own luminance variance ----
// The colour record's fourth slot carries v, the variance of the demodulated luminance l = (L0*u0 + L1*u1) + L2*u2,
// L = (0.2126, 0.7152, 0.0722), and the filter carries it along with the colour:
//   prepare   u and den as above; v = ((L0*L0) * (var0 / (den0*den0)) + (L1*L1) * (var1 / (den1*den1)))
//                                     + (L2*L2) * (var2 / (den2*den2)), var the frame's variance plane (pt_variance.hpp)
//   iteration g(p) = the normalised 3x3 filter of the iteration's input v at unit stride: dy = -1..1 (outer),
//             dx = -1..1 (inner), a tap outside the frame skipped, weight B[|dx|] * B[|dy|], B = {1/2, 1/4},
//             gs = gs + weight * v(q), gw = gw + weight, g = gs / gw;  rl(p) = rv / (g(p) + 1e-10)
//             per tap, beside the above: dl = l(p) - l(q), xl = (dl*dl) * rl(p),
//               w = ((h * f(xn)) * f(xz)) * f(xl);  av = av + (w*w) * v(q)
//             u_k(p) = acc_k / ws,  v(p) = av / (ws*ws)
//   finish    as above
// The host computes rv = 1 / (sigma_variance^2); +inf gives rv = 0, xl = 0 and f(xl) = 1, so the colour is then
// denoise_pixel<false>'s bit for bit.
constexpr double DENOISE_L0 = 0.2126, DENOISE_L1 = 0.7152, DENOISE_L2 = 0.0722;

PT_HD double denoise_lum(const DRec &u) { return (DENOISE_L0 * u.a + DENOISE_L1 * u.b) + DENOISE_L2 * u.c; }

PT_HD void denoise_prepare_variance(const double *rgb, const double *albedo, const double *normal,
                                    const double *depth, const double *variance, uint32_t flags, size_t p, DRec *u,
                                    DRec *g) {
    double d0 = 1.0, d1 = 1.0, d2 = 1.0;
    if (flags & DENOISE_DEMODULATE) {
        d0 = denoise_den(albedo[p * 3]);
        d1 = denoise_den(albedo[p * 3 + 1]);
        d2 = denoise_den(albedo[p * 3 + 2]);
    }
    double c0 = rgb[p * 3], c1 = rgb[p * 3 + 1], c2 = rgb[p * 3 + 2];
    if (flags & DENOISE_DEMODULATE) {
        c0 = c0 / d0;
        c1 = c1 / d1;
        c2 = c2 / d2;
    }
    const double v = ((DENOISE_L0 * DENOISE_L0) * (variance[p * 3] / (d0 * d0)) +
                      (DENOISE_L1 * DENOISE_L1) * (variance[p * 3 + 1] / (d1 * d1))) +
                     (DENOISE_L2 * DENOISE_L2) * (variance[p * 3 + 2] / (d2 * d2));
    u[p] = DRec{c0, c1, c2, v};
    g[p] = DRec{normal[p * 3], normal[p * 3 + 1], normal[p * 3 + 2], depth[p * 3]};
}

// One iteration's new colour record {u0, u1, u2, v} of pixel (x, y).  The nine prefilter taps read the records'
// fourth slot alone (8 bytes each) at unit stride whatever s is; at s = 1 they are lines the 25 taps load anyway.
PT_HD DRec denoise_pixel_variance(const DRec *__restrict__ u, const DRec *__restrict__ g, uint32_t w, uint32_t h,
                                  uint32_t x, uint32_t y, uint32_t s, double rn, double rz, double rv) {
    const double K[3] = {3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0};
    const double B[2] = {1.0 / 2.0, 1.0 / 4.0};
    const size_t p = (size_t)y * w + x;
    double gs = 0.0, gw = 0.0;
#pragma unroll
    for (int dy = -1; dy <= 1; dy++) {
        const int64_t qy = (int64_t)y + dy;
        const bool iny = qy >= 0 && qy < (int64_t)h;
        const size_t row = (size_t)(iny ? qy : (int64_t)y) * w;
#pragma unroll
        for (int dx = -1; dx <= 1; dx++) {
            const int64_t qx = (int64_t)x + dx;
            const bool in = iny && qx >= 0 && qx < (int64_t)w;
            const double vq = u[row + (size_t)(in ? qx : (int64_t)x)].d;
            if (!in) continue;
            const double bk = B[dx < 0 ? -dx : dx] * B[dy < 0 ? -dy : dy];
            gs = gs + bk * vq;
            gw = gw + bk;
        }
    }
    const double rl = rv / (gs / gw + 1e-10);
    const DRec gp = g[p];
    const double lp = denoise_lum(u[p]);
    const double r = gp.d > 0.0 ? 1.0 / gp.d : 0.0;
    double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0, ws = 0.0, av = 0.0;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
        const int64_t qy = (int64_t)y + (int64_t)s * dy;
        const bool iny = qy >= 0 && qy < (int64_t)h;
        const size_t row = (size_t)(iny ? qy : (int64_t)y) * w;
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const int64_t qx = (int64_t)x + (int64_t)s * dx;
            const bool in = iny && qx >= 0 && qx < (int64_t)w;
            const size_t q = row + (size_t)(in ? qx : (int64_t)x);
            const DRec gq = g[q];
            const DRec uq = u[q];
            if (!in) continue;
            const double hk = K[dx < 0 ? -dx : dx] * K[dy < 0 ? -dy : dy];
            const double dn0 = gp.a - gq.a, dn1 = gp.b - gq.b, dn2 = gp.c - gq.c;
            const double xn = ((dn0 * dn0 + dn1 * dn1) + dn2 * dn2) * rn;
            const double t = (gp.d - gq.d) * r;
            const double xz = (t * t) * rz;
            const double dl = lp - denoise_lum(uq);
            const double xl = (dl * dl) * rl;
            const double wt = ((hk * denoise_f(xn)) * denoise_f(xz)) * denoise_f(xl);
            acc0 = acc0 + wt * uq.a;
            acc1 = acc1 + wt * uq.b;
            acc2 = acc2 + wt * uq.c;
            ws = ws + wt;
            av = av + (wt * wt) * uq.d;
        }
    }
    return DRec{acc0 / ws, acc1 / ws, acc2 / ws, av / (ws * ws)};
}

}  // namespace dev

// The host's constants, in double.  A sigma of +inf gives a reciprocal of 0: that term weighs 1.
inline dev::DenoiseConsts denoise_consts(uint32_t iterations, double sigma_normal, double sigma_depth,
                                         double sigma_colour) {
    dev::DenoiseConsts k{};
    k.rn = 1.0 / (sigma_normal * sigma_normal);
    k.rz = 1.0 / (sigma_depth * sigma_depth);
    k.colour = sigma_colour > 0.0;
    for (uint32_t i = 0; i < iterations && i < DENOISE_MAX_ITERATIONS; i++) {
        const double sc = sigma_colour / (double)(1u << i);
        k.rc[i] = k.colour ? 1.0 / (sc * sc) : 0.0;
    }
    return k;
}

// Doubles of workspace for a w x h frame: DENOISE_WORK_RECORDS records of 4 doubles per pixel; 0 when a size is 0 or
// the count does not fit.
inline size_t denoise_workspace_doubles(uint32_t w, uint32_t h) {
    const uint64_t npix = (uint64_t)w * h;
    if (npix > (uint64_t)SIZE_MAX / (DENOISE_WORK_RECORDS * 4 * sizeof(double))) return 0;
    return (size_t)npix * DENOISE_WORK_RECORDS * 4;
}

// The whole pass, queued on st: one prepare launch, then `iterations` launches, the last one writing out (which
// may be rgb; no other overlap).  No host sync, no allocation, no atomics, no LDS.  work holds
// denoise_workspace_doubles(w, h) doubles, 16-byte aligned; the arguments are checked by the caller (pt_api.cpp).
hipError_t launch_denoise(const double *rgb, const double *albedo, const double *normal, const double *depth,
                          uint32_t w, uint32_t h, uint32_t iterations, const dev::DenoiseConsts &k, uint32_t flags,
                          double *out, double *work, hipStream_t st);

// The variance term's constant, in double: +inf gives 0.
inline double denoise_variance_rv(double sigma_variance) { return 1.0 / (sigma_variance * sigma_variance); }

// The same pass with the variance term (no colour term): variance is the frame's variance plane, w*h*3 doubles; rv
// is denoise_variance_rv(sigma_variance); k's rn and rz are read.  The same workspace, launches and rules.
hipError_t launch_denoise_variance(const double *rgb, const double *albedo, const double *normal, const double *depth,
                                   const double *variance, uint32_t w, uint32_t h, uint32_t iterations,
                                   const dev::DenoiseConsts &k, double rv, uint32_t flags, double *out, double *work,
                                   hipStream_t st);

}  // namespace pt
