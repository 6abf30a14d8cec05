// pt_temporal.hpp — temporal accumulation for a moving camera: the accumulated frame of the last
// camera is reprojected through the new frame's first-hit distance into the new camera, rejected where the geometry
// disagrees, and the new frame is blended in.  Built the way the denoiser is (pt_denoise.hpp): f64, no transcendental
// function, one fixed order, so the GPU, the host build (tests/native/Makefile) and the numpy restatement
// (tests/temporalref.py) give the same bits.  A pass of its own: it reads three whole frames in the colour buffer's
// layout (world == 1) and a history buffer, knows nothing of scenes or renderers, and the render kernels do not know
// about it.
//
// The history of a w x h frame is w*h*8 doubles, 16-byte aligned: two 32-byte records (dev::DRec) per pixel, first
// all colour records, then all guide records, pixel p = x + y*w at index p of each:
//   colour record {h0, h1, h2, n}   the accumulated colour and the number of frames it stands for (>= 1 once written)
//   guide record  {m0, m1, m2, z}   the normal plane's value and the hit distance of the frame that wrote it; z = 0
//                                   for a pixel with no hit
//
// dot(a, b) = (a0*b0 + a1*b1) + a2*b2.  pos, right, up, lt (left_top), res (pixel_resolution) are caster_params' values
// of the new camera, the primed ones those of the previous camera, dir' and f' its direction and focal length.
// Per pixel p = x + y*w: c = rgb[3p..], nrm = normal[3p..], d0 = depth[3p], d1 = depth[3p+1].
//   1 hit distance  zt = d1 > 0 ? d0 / d1 : 0 (the mean t over the hitting samples); !(zt > 0) or zt infinite: reset,
//                   and the guide record's z is 0
//   2 world point   the centre ray, dev::camera_ray's expressions at u = v = 0.5:
//                   sx = res*((double)x + 0.5), sy = res*((double)y + 0.5), dk = (lt_k + right_k*sx) - up_k*sy,
//                   g = d - pos, e_k = g_k / sqrt(dot(g, g)), X_k = pos_k + e_k*zt
//   3 old camera    v = X - pos', vd = dot(v, dir'); !(vd > 0): reset
//                   s = f' / vd, P_k = pos'_k + v_k*s, q = P - lt'
//                   fx = dot(q, right') / res' - 0.5, fy = dot(lt' - P, up') / res' - 0.5
//                   !(fx > -1 && fx < (double)w && fy > -1 && fy < (double)h): reset (a NaN fails this)
//   4 snap          rx = floor(fx + 0.5); |fx - rx| <= 1/1024: fx = rx.  The same for fy.  (A camera that did not
//                   move fetches pixel p itself and nothing of its neighbours.)
//   5 taps          x0 = floor(fx), ax = fx - x0, the same for y; zp = sqrt(dot(v, v)), r = 1.0 / zp
//                   taps (x0, y0), (x0+1, y0), (x0, y0+1), (x0+1, y0+1) in this order, wt = wx*wy, wx = 1.0 - ax or
//                   ax, wy = 1.0 - ay or ay.  A tap q counts if wt > 0, q is inside the frame, n(q) >= 1, z(q) > 0,
//                   xn < 1.0 (dn = nrm - m(q), xn = dot(dn, dn)*rn) and xz < 1.0 (t = (zp - z(q))*r, xz = (t*t)*rz):
//                   acc_k = acc_k + wt*h_k(q), cn = cn + wt*n(q), ws = ws + wt.  !(ws > 0): reset
//   6 blend         hk = acc_k / ws, hn = cn / ws, nn = hn + 1.0, nn > (double)max_count: nn = (double)max_count,
//                   a = 1.0 / nn, out_k = hk + (c_k - hk)*a.  A reset is out = c, nn = 1.0
//   7 write         out[3p..] = out, colour record {out, nn}, guide record {nrm, zt}
// The host computes rn = 1 / (sigma_normal^2) and rz = 1 / (sigma_depth^2) in double (temporal_consts); +inf gives 0
// and that test always passes.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "pt_denoise.hpp"  // dev::DRec, PT_HD

namespace pt {

constexpr size_t TEMPORAL_RECORDS = 2;  // per pixel: one colour record and one guide record

namespace dev {

// caster_params' values of one camera
struct TemporalCam {
    double pos[3], right[3], up[3], lt[3], res;
};

struct TemporalConsts {
    TemporalCam now, prev;  // prev, dir and f are not read on the first frame
    double dir[3], f;       // the previous camera's direction and focal length
    double rn, rz, max_count;
};

PT_HD double temporal_dot(double a0, double a1, double a2, double b0, double b1, double b2) {
    return (a0 * b0 + a1 * b1) + a2 * b2;
}

// One bilinear tap: the records are loaded at an index clamped into the frame, so the loads do not wait for the
// tests; a tap that does not count adds nothing.
PT_HD void temporal_tap(const DRec *__restrict__ hc, const DRec *__restrict__ hg, uint32_t w, uint32_t h, double tx,
                        double ty, double wt, double n0, double n1, double n2, double zp, double r, double rn,
                        double rz, double &acc0, double &acc1, double &acc2, double &cn, double &ws) {
    const bool in = tx >= 0.0 && tx < (double)w && ty >= 0.0 && ty < (double)h;
    const double qx = tx < 0.0 ? 0.0 : tx < (double)w ? tx : (double)(w - 1);
    const double qy = ty < 0.0 ? 0.0 : ty < (double)h ? ty : (double)(h - 1);
    const size_t q = (size_t)qy * w + (size_t)qx;
    const DRec cq = hc[q];
    const DRec gq = hg[q];
    const double dn0 = n0 - gq.a, dn1 = n1 - gq.b, dn2 = n2 - gq.c;
    const double xn = temporal_dot(dn0, dn1, dn2, dn0, dn1, dn2) * rn;
    const double t = (zp - gq.d) * r;
    const double xz = (t * t) * rz;
    if (!(wt > 0.0 && in && cq.d >= 1.0 && gq.d > 0.0 && xn < 1.0 && xz < 1.0)) return;
    acc0 = acc0 + wt * cq.a;
    acc1 = acc1 + wt * cq.b;
    acc2 = acc2 + wt * cq.c;
    cn = cn + wt * cq.d;
    ws = ws + wt;
}

// Pixel (x, y)'s two new history records; the colour record's first three values are the frame's.  hc and hg are the
// previous history's colour and guide records and are not read when FIRST.
template <bool FIRST>
PT_HD void temporal_pixel(const double *rgb, const double *__restrict__ normal, const double *__restrict__ depth,
                          const DRec *__restrict__ hc, const DRec *__restrict__ hg, uint32_t w, uint32_t h, uint32_t x,
                          uint32_t y, const TemporalConsts &K, DRec *oc, DRec *og) {
    const size_t p = (size_t)y * w + x;
    const double c0 = rgb[p * 3], c1 = rgb[p * 3 + 1], c2 = rgb[p * 3 + 2];
    const double n0 = normal[p * 3], n1 = normal[p * 3 + 1], n2 = normal[p * 3 + 2];
    const double d0 = depth[p * 3], d1 = depth[p * 3 + 1];
    // 1
    double zt = d1 > 0.0 ? d0 / d1 : 0.0;
    const bool hit = zt > 0.0 && zt < __builtin_inf();
    if (!hit) zt = 0.0;
    *oc = DRec{c0, c1, c2, 1.0};
    *og = DRec{n0, n1, n2, zt};
    if (FIRST || !hit) return;
    // 2
    const TemporalCam &A = K.now, &B = K.prev;
    const double sx = A.res * ((double)x + 0.5), sy = A.res * ((double)y + 0.5);
    const double g0 = ((A.lt[0] + A.right[0] * sx) - A.up[0] * sy) - A.pos[0];
    const double g1 = ((A.lt[1] + A.right[1] * sx) - A.up[1] * sy) - A.pos[1];
    const double g2 = ((A.lt[2] + A.right[2] * sx) - A.up[2] * sy) - A.pos[2];
    const double gl = sqrt(temporal_dot(g0, g1, g2, g0, g1, g2));
    const double X0 = A.pos[0] + (g0 / gl) * zt, X1 = A.pos[1] + (g1 / gl) * zt, X2 = A.pos[2] + (g2 / gl) * zt;
    // 3
    const double v0 = X0 - B.pos[0], v1 = X1 - B.pos[1], v2 = X2 - B.pos[2];
    const double vd = temporal_dot(v0, v1, v2, K.dir[0], K.dir[1], K.dir[2]);
    if (!(vd > 0.0)) return;
    const double s = K.f / vd;
    const double P0 = B.pos[0] + v0 * s, P1 = B.pos[1] + v1 * s, P2 = B.pos[2] + v2 * s;
    double fx = temporal_dot(P0 - B.lt[0], P1 - B.lt[1], P2 - B.lt[2], B.right[0], B.right[1], B.right[2]) / B.res - 0.5;
    double fy = temporal_dot(B.lt[0] - P0, B.lt[1] - P1, B.lt[2] - P2, B.up[0], B.up[1], B.up[2]) / B.res - 0.5;
    if (!(fx > -1.0 && fx < (double)w && fy > -1.0 && fy < (double)h)) return;
    // 4
    const double rx = floor(fx + 0.5), ry = floor(fy + 0.5);
    if (fabs(fx - rx) <= 1.0 / 1024.0) fx = rx;
    if (fabs(fy - ry) <= 1.0 / 1024.0) fy = ry;
    // 5
    const double x0 = floor(fx), y0 = floor(fy);
    const double ax = fx - x0, ay = fy - y0;
    const double bx = 1.0 - ax, by = 1.0 - ay;
    const double zp = sqrt(temporal_dot(v0, v1, v2, v0, v1, v2));
    const double r = 1.0 / zp;
    double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0, cn = 0.0, ws = 0.0;
    temporal_tap(hc, hg, w, h, x0, y0, bx * by, n0, n1, n2, zp, r, K.rn, K.rz, acc0, acc1, acc2, cn, ws);
    temporal_tap(hc, hg, w, h, x0 + 1.0, y0, ax * by, n0, n1, n2, zp, r, K.rn, K.rz, acc0, acc1, acc2, cn, ws);
    temporal_tap(hc, hg, w, h, x0, y0 + 1.0, bx * ay, n0, n1, n2, zp, r, K.rn, K.rz, acc0, acc1, acc2, cn, ws);
    temporal_tap(hc, hg, w, h, x0 + 1.0, y0 + 1.0, ax * ay, n0, n1, n2, zp, r, K.rn, K.rz, acc0, acc1, acc2, cn, ws);
    if (!(ws > 0.0)) return;
    // 6
    const double h0 = acc0 / ws, h1 = acc1 / ws, h2 = acc2 / ws, hn = cn / ws;
    double nn = hn + 1.0;
    if (nn > K.max_count) nn = K.max_count;
    const double a = 1.0 / nn;
    *oc = DRec{h0 + (c0 - h0) * a, h1 + (c1 - h1) * a, h2 + (c2 - h2) * a, nn};
}

}  // namespace dev

// The host's constants, in double.  A sigma of +inf gives a reciprocal of 0: that test always passes.  prev, dir and f
// may be null (the first frame).
inline dev::TemporalConsts temporal_consts(const dev::TemporalCam &now, const dev::TemporalCam *prev, const double *dir,
                                           double f, uint32_t max_count, double sigma_normal, double sigma_depth) {
    dev::TemporalConsts k{};
    k.now = now;
    if (prev) k.prev = *prev;
    for (int i = 0; i < 3; i++) k.dir[i] = dir ? dir[i] : 0.0;
    k.f = f;
    k.rn = 1.0 / (sigma_normal * sigma_normal);
    k.rz = 1.0 / (sigma_depth * sigma_depth);
    k.max_count = (double)max_count;
    return k;
}

// Doubles of history for a w x h frame: TEMPORAL_RECORDS records of 4 doubles per pixel; 0 when a size is 0 or the
// count does not fit.
inline size_t temporal_history_doubles(uint32_t w, uint32_t h) {
    const uint64_t npix = (uint64_t)w * h;
    if (npix > (uint64_t)SIZE_MAX / (TEMPORAL_RECORDS * 4 * sizeof(double))) return 0;
    return (size_t)npix * TEMPORAL_RECORDS * 4;
}

// The whole pass, queued on st: one launch.  history_in null is the first frame (it is then not read); out may be
// rgb, history_in and history_out must not overlap.  No host sync, no allocation, no atomics, no LDS.  The histories
// hold temporal_history_doubles(w, h) doubles, 16-byte aligned; the arguments are checked by the caller (pt_api.cpp).
hipError_t launch_temporal(const double *rgb, const double *normal, const double *depth, uint32_t w, uint32_t h,
                           const dev::TemporalConsts &k, const double *history_in, double *history_out, double *out,
                           hipStream_t st);

}  // namespace pt
