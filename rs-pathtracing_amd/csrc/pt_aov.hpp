// pt_aov.hpp — the first-hit guide planes of a frame (albedo, shading normal, depth), for denoisers, compositing
// and debugging.  A pass of its own beside the sample path: it re-generates each sample's camera
// ray from the frame's own RNG key and asks the sample path's device functions for the first hit, so the planes
// belong to the beauty frame's samples exactly, and the render kernels do not know about it.
//
// Sample s of pixel p = x + y * width is the primary ray of the beauty frame's sample s: Rng{sample_key(seed, p,
// s)}, camera_ray draws u then v, nothing else is drawn.  who = closest(ray, T_MIN, inf, &t); on a hit h =
// finish(shape, ray, t) and m is the shape's material.  Per pixel, each value below is the in-order f64 sum over
// s = 0 .. spp-1 divided by spp once (trace_pixel's order and division for the beauty mean):
//   albedo  the first hit's colour: Lambertian / Metal the albedo (its texture's value at the hit when it has
//           one), Dielectric (1, 1, 1), DiffuseLight its emit (or texture value), not clamped, EmptyMaterial
//           (0, 0, 0); a miss background(ray.d)
//   normal  h.n (unit, turned against the ray); a miss (0, 0, 0); the mean is not renormalised
//   depth   x: sum of t over the hitting samples / spp (t is the world distance: directions are unit),
//           y: hits / spp (the coverage), z: the smallest t of the hitting samples, 0 when none hits
// A march the guard drops is a miss here as in the frame, and is counted (pt_march_guard_drops).
#pragma once
#include "pt_device.hpp"

namespace pt {
namespace dev {

// EXT, here and below: the extended build (closest<false, true>, the one closest_hit_probe runs), which takes every
// scene: non-solid textures, the Torus, small and large trees.  EXT = false is for the scenes that need none of
// that (dev::Scene::ext == 0: no Torus, every material's tex < 0): the same values without the quartic and the
// texture code, 189 VGPRs against 256 + 14 AGPRs (2 waves per SIMD against 1) and 25 % less time on cornell_box
// (profiles/r9/aov_ab.txt).  aov_ext names the build a scene gets.
PT_HD bool aov_ext(const Scene &sc) { return sc.ext != 0; }

// The first hit's colour (see above); (u, v) and the texture only where the material has one.
template <bool EXT = true>
PT_HD V3 aov_hit_colour(const Scene &sc, const DShape &s, const DMaterial &m, const Ray &ray, double t, V3 p) {
    const bool lit = m.type == DIFFUSE_LIGHT;
    if (m.type == LAMBERTIAN || m.type == METAL || lit) {
        if (EXT && m.tex >= 0) {
            double u, v;
            hit_uv(s, ray, t, &u, &v);
            return tex_value(sc, m.tex, u, v, p);
        }
        return lit ? v3(m.emit[0], m.emit[1], m.emit[2]) : v3(m.albedo[0], m.albedo[1], m.albedo[2]);
    }
    return m.type == DIELECTRIC ? v3(1.0, 1.0, 1.0) : v3(0.0, 0.0, 0.0);
}

// One pixel's three values.  A plane that is not wanted costs nothing it alone needs: no (u, v) and no texture
// without the albedo, no hit frame (finish) unless the normal or a textured colour asks for it; its output is
// left (0, 0, 0).
template <bool EXT = true>
PT_HD void aov_pixel(const Scene &sc, const FrameParams &P, uint32_t x, uint32_t y, bool want_albedo, bool want_normal,
                     V3 *albedo, V3 *normal, V3 *depth) {
    const uint64_t pixel = (uint64_t)x + (uint64_t)y * P.width;
    V3 a = v3(0.0, 0.0, 0.0), n = v3(0.0, 0.0, 0.0);
    double tsum = 0.0, tmin = 0.0;
    uint32_t hits = 0;
    for (uint32_t s = 0; s < P.spp; s++) {
        Rng rng{sample_key(P.seed, pixel, s)};
        const Ray ray = camera_ray(P, x, y, rng);
        double t;
        const int who = closest<false, EXT>(sc, ray, T_MIN, __builtin_inf(), &t);
        if (who < 0) {
            if (want_albedo) a = add(a, background(ray.d));
            continue;  // (0, 0, 0) to the normal's sum, nothing to the depth's
        }
        tsum = tsum + t;
        tmin = hits == 0 || t < tmin ? t : tmin;
        hits++;
        const DShape &S = sc.shapes[who];
        const DMaterial &m = sc.mats[S.material];
        const bool textured =
            EXT && want_albedo && m.tex >= 0 && (m.type == LAMBERTIAN || m.type == METAL || m.type == DIFFUSE_LIGHT);
        V3 p = v3(0.0, 0.0, 0.0);
        if (want_normal || textured) {
            const Hit h = finish(S, ray, t);
            n = add(n, h.n);
            p = h.p;
        }
        if (want_albedo) a = add(a, aov_hit_colour<EXT>(sc, S, m, ray, t, p));
    }
    const double spp = (double)P.spp;
    *albedo = divs(a, spp);
    *normal = divs(n, spp);
    *depth = v3(tsum / spp, (double)hits / spp, tmin);
}

}  // namespace dev

// The pass over this rank's tiles of P (render_tiles' tiles, deal and shard layout; P.depth, the sample window and
// the stop flag are not read): each plane that is not null gets width*height*3 doubles (P.compact = 0) or
// tile_count*256*3 (compact shards, pixels outside the frame 0).  Queued on st; pt_aov.hip.
hipError_t launch_aov(const dev::Scene &sc, const FrameParams &P, double *albedo, double *normal, double *depth,
                      hipStream_t st);

}  // namespace pt
