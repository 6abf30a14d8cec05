// pt_cull.hpp — which shapes the camera rays of one 8x8 pixel block can reach (host and device).
//
// camera_ray has no lens: every ray of a frame leaves FrameParams::pos, and its unnormalised direction
// d(px, py) = ((left_top + right * res * px) - up * res * py) - pos is affine in the jittered pixel coordinates
// (px, py).  The rays of pixel block (bx, by) = (x >> 3, y >> 3) have (px, py) in [8 bx, 8 bx + 8) x [8 by, 8 by + 8),
// so each direction is a convex combination of the four directions at the block's corners: the rays lie inside the
// pyramid through them, apex pos.  first_cull_mask() tests the padded world box (Accel::boxes: every point a shape
// test can return lies inside it) of each entry of the uniform list and of each marched shape against that pyramid,
// widened by one whole pixel on every side (about 1e13 times the rounding of sx, sy and d in camera_ray), and clears
// the entry's bit only when all 8 corners of its box lie strictly outside one of the pyramid's four side planes.
//
// That can fail to cull but never culls wrongly: the box is convex and on the open outer side of the plane, while a
// point pos + t dir with t >= T_MIN > 0 of a ray in the closed pyramid is on its inner side.  An entry whose bit is
// clear therefore has no hit for any camera ray of the block, and a marched shape whose bit is clear fails the slab
// test of its box (and so shape_bound_k's bound, which lies inside the box) for every one of them.
//
// Whenever the argument does not hold as stated the mask is all ones: a non-finite corner direction, plane normal or
// box coordinate, a pixel_resolution that is not positive (a zero or NaN resolution, a field of view beyond 180
// degrees), a corner direction at right angles to the view axis (a field of view of 180 degrees), or a corner
// direction that is not on the inner side of all four planes (a degenerate pyramid).
//
// Bit k (k < 32): position k of Scene::lin; bit 32 + k: position k of Scene::march.  Positions 32 and beyond carry no
// bit (the caller always tests them), bits of positions the lists do not have are clear.  The BVH is not culled.
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#endif

#include <cmath>
#include <cstdint>

#include "pt_dims.hpp"
#include "pt_types.hpp"

namespace pt {
namespace cull {

constexpr uint32_t BLOCK = 8;        // pixels per block side: one wave of wf_bounce<FIRST> (slot_pixel)
constexpr int LIST_BITS = 32;        // uniform-list positions with a bit; the marched positions follow
constexpr uint64_t ALL = ~0ull;
// "strictly outside": n . (q - pos) < -EPS (|nx vx| + |ny vy| + |nz vz|); the dot product's own rounding is below
// 2^-50 of that sum.  The same margin decides whether a corner direction is inside a plane.
constexpr double EPS = 1e-9;
// the least cosine between a block's corner direction and the view axis: 89.99994 degrees off the axis
constexpr double MIN_COS = 1e-6;

PT_HD uint32_t blocks_across(uint32_t pixels) { return (pixels + BLOCK - 1) / BLOCK; }

struct Plane {
    double x, y, z;
};
// n . v and the sum of the products' magnitudes
PT_HD double pdot(const Plane &n, double vx, double vy, double vz, double *mag) {
    const double a = n.x * vx, b = n.y * vy, c = n.z * vz;
    *mag = fabs(a) + fabs(b) + fabs(c);
    return a + b + c;
}
PT_HD bool finite3(double x, double y, double z) {
    const double s = x + y + z;  // inf or NaN if any term is
    return s - s == 0.0;
}

// The mask of pixel block (bx, by); lin / march / boxes as in dev::Scene (entries of lin may carry LIN_GROUPED).
PT_HD uint64_t first_cull_mask(const FrameParams &P, const int32_t *lin, int nlin, const int32_t *march, int nmarch,
                               const DBox *boxes, uint32_t bx, uint32_t by) {
    if (!(P.pixel_resolution > 0.0)) return ALL;
    // corner directions of the widened block, in order around it: camera_ray's expressions
    const double px[4] = {(double)(BLOCK * bx) - 1.0, (double)(BLOCK * bx + BLOCK) + 1.0,
                          (double)(BLOCK * bx + BLOCK) + 1.0, (double)(BLOCK * bx) - 1.0};
    const double py[4] = {(double)(BLOCK * by) - 1.0, (double)(BLOCK * by) - 1.0, (double)(BLOCK * by + BLOCK) + 1.0,
                          (double)(BLOCK * by + BLOCK) + 1.0};
    double c[4][3], axis[3];  // (axis: the direction through the frame's centre)
    const double ax = P.pixel_resolution * (0.5 * (double)P.width), ay = P.pixel_resolution * (0.5 * (double)P.height);
    for (int a = 0; a < 3; a++) axis[a] = ((P.left_top[a] + P.right[a] * ax) - P.up[a] * ay) - P.pos[a];
    const double aa = axis[0] * axis[0] + axis[1] * axis[1] + axis[2] * axis[2];
    for (int j = 0; j < 4; j++) {
        const double sx = P.pixel_resolution * px[j], sy = P.pixel_resolution * py[j];
        for (int a = 0; a < 3; a++) c[j][a] = ((P.left_top[a] + P.right[a] * sx) - P.up[a] * sy) - P.pos[a];
        if (!finite3(c[j][0], c[j][1], c[j][2])) return ALL;
        // a corner direction within MIN_COS of perpendicular to the view axis: a field of view of 180 degrees as
        // floating point has it (tan(fov / 2) ~ 1e16), where the image plane's distance drowns in the corners' size
        const double ca = c[j][0] * axis[0] + c[j][1] * axis[1] + c[j][2] * axis[2];
        const double cc = c[j][0] * c[j][0] + c[j][1] * c[j][1] + c[j][2] * c[j][2];
        if (!(ca > 0.0 && ca * ca > (MIN_COS * MIN_COS) * (cc * aa))) return ALL;
    }
    const double mid[3] = {(c[0][0] + c[1][0]) + (c[2][0] + c[3][0]), (c[0][1] + c[1][1]) + (c[2][1] + c[3][1]),
                           (c[0][2] + c[1][2]) + (c[2][2] + c[3][2])};
    // side plane j through pos and corners j, j + 1, its normal towards the block's centre direction
    Plane n[4];
    for (int j = 0; j < 4; j++) {
        const double *u = c[j], *w = c[(j + 1) & 3];
        Plane q{u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]};
        double mag;
        if (pdot(q, mid[0], mid[1], mid[2], &mag) < 0.0) q = Plane{-q.x, -q.y, -q.z};
        if (!finite3(q.x, q.y, q.z)) return ALL;
        n[j] = q;
        // the two corners off the plane are strictly inside it, the two on it are not outside
        for (int i = 0; i < 4; i++) {
            const double d = pdot(q, c[i][0], c[i][1], c[i][2], &mag);
            const bool on = i == j || i == ((j + 1) & 3);
            if (on ? !(d >= -EPS * mag) : !(d > EPS * mag)) return ALL;
        }
    }
    auto reachable = [&](int shape, bool *ok) {
        const DBox &b = boxes[shape];
        if (!finite3(b.lo[0], b.lo[1], b.lo[2]) || !finite3(b.hi[0], b.hi[1], b.hi[2])) {
            *ok = false;
            return true;
        }
        for (int j = 0; j < 4; j++) {
            bool all_out = true;
            for (int k = 0; k < 8 && all_out; k++) {
                const double vx = ((k & 1) ? b.hi[0] : b.lo[0]) - P.pos[0];
                const double vy = ((k & 2) ? b.hi[1] : b.lo[1]) - P.pos[1];
                const double vz = ((k & 4) ? b.hi[2] : b.lo[2]) - P.pos[2];
                double mag;
                const double d = pdot(n[j], vx, vy, vz, &mag);
                all_out = d < -EPS * mag;
            }
            if (all_out) return false;
        }
        return true;
    };
    uint64_t mask = 0;
    bool ok = true;
    for (int k = 0; k < nlin && k < LIST_BITS; k++)
        if (reachable(lin[k] & LIN_ID_MASK, &ok)) mask |= 1ull << k;
    for (int k = 0; k < nmarch && k < 64 - LIST_BITS; k++)
        if (reachable(march[k], &ok)) mask |= 1ull << (LIST_BITS + k);
    return ok ? mask : ALL;
}

// What the table of a frame depends on besides the acceleration data: the caster part of FrameParams and the frame's
// size.  Compared bytewise (every field is set; no padding between them).
struct CasterKey {
    double pos[3], right[3], up[3], left_top[3], pixel_resolution;
    uint32_t width, height;
};
inline CasterKey caster_key(const FrameParams &P) {
    CasterKey k;
    for (int a = 0; a < 3; a++) k.pos[a] = P.pos[a], k.right[a] = P.right[a], k.up[a] = P.up[a], k.left_top[a] = P.left_top[a];
    k.pixel_resolution = P.pixel_resolution;
    k.width = P.width;
    k.height = P.height;
    return k;
}
static_assert(sizeof(CasterKey) == 13 * 8 + 8, "CasterKey is compared bytewise: no padding");

}  // namespace cull
}  // namespace pt
