// Test-only stand-alone program (host build of the product headers): the first bounce launch's cull masks
// (cull::first_cull_mask, pt_cull.hpp) against the product's own camera rays and shape tests.
//   first_cull_harness safety <scene.json> <random_spheres> <scene_seed> [camera ...]
//       every pixel block of 64x64, 128x72 and 100x52 frames, for the scene's camera and each listed one, 16 samples
//       per pixel from sample_key / camera_ray: the list entry the plain closest_nomarch returns must have its bit,
//       so must every marched shape whose shape_bound_k holds, and the culled scan (closest_nomarch's CULL form and
//       the bounce kernel's pre-check loop) must give the plain one's (best, who) and march decision bit for bit
//   first_cull_harness count <scene.json> <random_spheres> <scene_seed> <width> <height> [camera]
//       the table of one frame: set bits in all, per list position, and over the lights
//   first_cull_harness degenerate <scene.json> <random_spheres> <scene_seed>
//       cameras the argument does not cover: every mask must be all ones
// A camera is 11 numbers: position, direction, up (3 each), focal length, field of view in degrees.
// Prints "key value" lines; exit status 1 on any violation.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <vector>

#include "../../rs-pathtracing_amd/csrc/pt_accel.hpp"
#include "../../rs-pathtracing_amd/csrc/pt_cull.hpp"
#include "../../rs-pathtracing_amd/csrc/pt_device.hpp"
#include "../../rs-pathtracing_amd/csrc/pt_scene.hpp"

using namespace pt;

struct Host {
    Scene sc;
    Accel acc;
    std::vector<DShape> shapes;
    std::vector<DMaterial> mats;
    std::vector<DQGrid> qbuf;
    dev::Scene v{};
};

static bool load(const char *path, bool random_spheres, uint64_t seed, Host *h) {
    std::ifstream f(path);
    if (!f) {
        fprintf(stderr, "cannot read %s\n", path);
        return false;
    }
    std::stringstream ss;
    ss << f.rdbuf();
    const std::string js = ss.str();
    h->sc = scene_from_json(js.c_str(), js.size(), random_spheres, seed);
    h->acc = build_accel(h->sc, h->sc.json_shapes);
    for (auto &s : h->sc.shapes) h->shapes.push_back(to_device(s));
    for (auto &m : h->sc.materials) h->mats.push_back(to_device(m));
    h->qbuf = pack_qnodes(h->acc);
    view_of_host(h->v, h->sc, h->acc, h->shapes, h->mats, h->qbuf);
    return true;
}

static pt_camera camera_arg(char **a) {
    double n[11];
    for (int k = 0; k < 11; k++) n[k] = atof(a[k]);
    pt_camera c;
    camera_new(n, n + 3, n + 6, n[9], n[10] * 3.141592653589793 / 180.0, &c);
    return c;
}

static uint64_t mask_of(const Host &h, const FrameParams &P, uint32_t bx, uint32_t by) {
    return cull::first_cull_mask(P, h.v.lin, h.v.nlin, h.v.march, h.v.nmarch, h.v.boxes, bx, by);
}

static bool same_bits(double a, double b) { return memcmp(&a, &b, 8) == 0; }

// The bounce kernel's march pre-check (wf_bounce), with the mask's marched bits (all ones: the plain loop).
static bool pre_check(const dev::Scene &sc, const dev::Ray &ray, dev::V3 inv, double best, uint64_t mask) {
    bool need = false;
    for (int k = 0; k < sc.nmarch && !need; k++) {
        if (k < 64 - cull::LIST_BITS && !((mask >> (cull::LIST_BITS + k)) & 1ull)) continue;
        const int s = sc.march[k];
        const DBox &bx = sc.boxes[s];
        if (!dev::slab(bx.lo, bx.hi, ray, inv, T_MIN, best)) continue;
        const DShape &S = sc.shapes[s];
        const dev::V3 o = dev::xf_point(S.inv, ray.o), d = dev::xf_vector(S.inv, ray.d);
        double st = 0.0, en = 0.0;
        need = march::shape_bound_k<march::F_ANY>(dev::shape_params(S), o.x, o.y, o.z, d.x, d.y, d.z, &st, &en);
        need = need && march::clip_to_best(best, S.p[0], &st, &en);
    }
    return need;
}

struct Tally {
    long cases = 0, blocks = 0, rays = 0, who_violations = 0, march_violations = 0, differ = 0;
    long bits = 0, candidates = 0, all_ones = 0, list_hits = 0, bounds_held = 0;
};

static void safety_frame(const Host &h, const pt_camera &cam, uint32_t W, uint32_t H, uint32_t spp, Tally *T) {
    const dev::Scene &sc = h.v;
    const FrameParams P = frame_params(cam, W, H, spp, 8, 1, uniform_incl_scale(-1.0, 1.0));
    std::vector<int> pos_of(h.shapes.size(), -1);  // shape -> its position in the uniform list
    for (int k = 0; k < sc.nlin; k++) pos_of[sc.lin[k] & LIN_ID_MASK] = k;
    const uint32_t nbx = cull::blocks_across(W), nby = cull::blocks_across(H);
    T->cases++;
    for (uint32_t by = 0; by < nby; by++)
        for (uint32_t bx = 0; bx < nbx; bx++) {
            const uint64_t mask = mask_of(h, P, bx, by);
            T->blocks++;
            T->all_ones += mask == cull::ALL;
            T->bits += __builtin_popcountll(mask);
            T->candidates += (sc.nlin < 32 ? sc.nlin : 32) + (sc.nmarch < 32 ? sc.nmarch : 32);
            for (uint32_t y = by * 8; y < by * 8 + 8 && y < H; y++)
                for (uint32_t x = bx * 8; x < bx * 8 + 8 && x < W; x++)
                    for (uint32_t s = 0; s < spp; s++) {
                        dev::Rng rng{dev::sample_key(P.seed, (uint64_t)x + (uint64_t)y * W, s)};
                        const dev::Ray ray = dev::camera_ray(P, x, y, rng);
                        const dev::V3 inv = dev::v3(1.0 / ray.d.x, 1.0 / ray.d.y, 1.0 / ray.d.z);
                        T->rays++;
                        double best = INFINITY, cbest = INFINITY;
                        int who = -1, cwho = -1;
                        dev::closest_nomarch<false, true>(sc, ray, inv, T_MIN, &best, &who);
                        dev::closest_nomarch<false, true, false, false, 3, true>(sc, ray, inv, T_MIN, &cbest, &cwho,
                                                                                 nullptr, false, mask);
                        if (who >= 0 && pos_of[who] >= 0) {
                            T->list_hits++;
                            const int k = pos_of[who];
                            if (k < cull::LIST_BITS && !((mask >> k) & 1ull)) {
                                if (T->who_violations++ < 10)
                                    printf("violation: %ux%u pixel (%u, %u) sample %u hits shape %d at list position %d, "
                                           "mask %016llx\n", W, H, x, y, s, who, k, (unsigned long long)mask);
                            }
                        }
                        for (int k = 0; k < sc.nmarch; k++) {
                            const DShape &S = sc.shapes[sc.march[k]];
                            const dev::V3 o = dev::xf_point(S.inv, ray.o), d = dev::xf_vector(S.inv, ray.d);
                            double st, en;
                            if (!march::shape_bound_k<march::F_ANY>(dev::shape_params(S), o.x, o.y, o.z, d.x, d.y, d.z,
                                                                    &st, &en))
                                continue;
                            T->bounds_held++;
                            if (k < 64 - cull::LIST_BITS && !((mask >> (cull::LIST_BITS + k)) & 1ull)) {
                                if (T->march_violations++ < 10)
                                    printf("violation: %ux%u pixel (%u, %u) sample %u enters the bound of marched "
                                           "shape %d, mask %016llx\n", W, H, x, y, s, k, (unsigned long long)mask);
                            }
                        }
                        const bool need = pre_check(sc, ray, inv, best, cull::ALL);
                        const bool cneed = pre_check(sc, ray, inv, cbest, mask);
                        if (who != cwho || !same_bits(best, cbest) || need != cneed) {
                            if (T->differ++ < 10)
                                printf("differ: %ux%u pixel (%u, %u) sample %u plain (%d, %.17g, %d) culled (%d, %.17g, "
                                       "%d), mask %016llx\n", W, H, x, y, s, who, best, (int)need, cwho, cbest,
                                       (int)cneed, (unsigned long long)mask);
                        }
                    }
        }
}

static int safety(const Host &h, const std::vector<pt_camera> &cams) {
    const uint32_t sizes[3][2] = {{64, 64}, {128, 72}, {100, 52}};
    Tally T;
    for (const pt_camera &c : cams)
        for (auto &wh : sizes) safety_frame(h, c, wh[0], wh[1], 16, &T);
    printf("safety_cameras %zu\n", cams.size());
    printf("safety_cases %ld\n", T.cases);
    printf("safety_blocks %ld\n", T.blocks);
    printf("safety_rays %ld\n", T.rays);
    printf("safety_list_hits %ld\n", T.list_hits);
    printf("safety_bounds_held %ld\n", T.bounds_held);
    printf("safety_who_violations %ld\n", T.who_violations);
    printf("safety_march_violations %ld\n", T.march_violations);
    printf("safety_differ %ld\n", T.differ);
    printf("safety_bits %ld\n", T.bits);
    printf("safety_candidates %ld\n", T.candidates);
    printf("safety_all_ones_blocks %ld\n", T.all_ones);
    return T.who_violations || T.march_violations || T.differ ? 1 : 0;
}

static int count(const Host &h, const pt_camera &cam, uint32_t W, uint32_t H) {
    const dev::Scene &sc = h.v;
    const FrameParams P = frame_params(cam, W, H, 1, 8, 1, uniform_incl_scale(-1.0, 1.0));
    const uint32_t nbx = cull::blocks_across(W), nby = cull::blocks_across(H);
    long bits = 0, none = 0, most = 0, light = 0, all_ones = 0;
    std::vector<long> per(64, 0);
    for (uint32_t by = 0; by < nby; by++)
        for (uint32_t bx = 0; bx < nbx; bx++) {
            const uint64_t m = mask_of(h, P, bx, by);
            const long n = __builtin_popcountll(m);
            bits += n;
            none += n == 0;
            all_ones += m == cull::ALL;
            most = n > most ? n : most;
            for (int k = 0; k < 64; k++) per[k] += (m >> k) & 1ull;
            for (int k = 0; k < sc.nlin && k < cull::LIST_BITS; k++)
                if (h.mats[h.shapes[sc.lin[k] & LIN_ID_MASK].material].type == DIFFUSE_LIGHT) light += (m >> k) & 1ull;
        }
    printf("count_blocks %ld\n", (long)nbx * nby);
    printf("count_bits %ld\n", bits);
    printf("count_blocks_with_none %ld\n", none);
    printf("count_most_per_block %ld\n", most);
    printf("count_all_ones_blocks %ld\n", all_ones);
    printf("count_light_bits %ld\n", light);
    printf("count_list %d\n", sc.nlin);
    printf("count_marched %d\n", sc.nmarch);
    for (int k = 0; k < sc.nlin && k < cull::LIST_BITS; k++)
        printf("count_list_%d_shape_%d %ld\n", k, sc.lin[k] & LIN_ID_MASK, per[k]);
    for (int k = 0; k < sc.nmarch && k < 64 - cull::LIST_BITS; k++)
        printf("count_marched_%d_shape_%d %ld\n", k, sc.march[k], per[cull::LIST_BITS + k]);
    return 0;
}

// masks that are not all ones over a 128x72 frame
static long not_all_ones(const Host &h, const FrameParams &P) {
    long bad = 0;
    for (uint32_t by = 0; by < cull::blocks_across(P.height); by++)
        for (uint32_t bx = 0; bx < cull::blocks_across(P.width); bx++) bad += mask_of(h, P, bx, by) != cull::ALL;
    return bad;
}

static int degenerate(const Host &h) {
    const double s11 = uniform_incl_scale(-1.0, 1.0), PI = 3.141592653589793;
    long bad = 0, n;
    auto frame = [&](const pt_camera &c) { return frame_params(c, 128, 72, 1, 8, 1, s11); };
    pt_camera c = h.sc.camera;
    printf("degenerate_valid_camera_culls %ld\n", not_all_ones(h, frame(c)));  // (the checks below are not vacuous)
    c.position[1] = NAN;
    bad += n = not_all_ones(h, frame(c));
    printf("degenerate_nan_position %ld\n", n);
    c = h.sc.camera;
    c.direction[0] = NAN;
    bad += n = not_all_ones(h, frame(c));
    printf("degenerate_nan_direction %ld\n", n);
    c = h.sc.camera;
    c.position[2] = INFINITY;
    bad += n = not_all_ones(h, frame(c));
    printf("degenerate_inf_position %ld\n", n);
    for (double fov : {180.0, 200.0, 270.0, 359.0}) {
        c = h.sc.camera;
        c.fov = fov * PI / 180.0;
        bad += n = not_all_ones(h, frame(c));
        printf("degenerate_fov_%d %ld\n", (int)fov, n);
    }
    c = h.sc.camera;
    c.fov = 0.0;  // zero pixel_resolution
    bad += n = not_all_ones(h, frame(c));
    printf("degenerate_zero_resolution %ld\n", n);
    FrameParams P = frame(h.sc.camera);
    P.pixel_resolution = 0.0;
    bad += n = not_all_ones(h, P);
    printf("degenerate_zero_resolution_field %ld\n", n);
    P = frame(h.sc.camera);
    for (int a = 0; a < 3; a++) P.up[a] = P.right[a];  // a flat pyramid: up along right
    bad += n = not_all_ones(h, P);
    printf("degenerate_flat_pyramid %ld\n", n);
    printf("degenerate_not_all_ones %ld\n", bad);
    return bad ? 1 : 0;
}

int main(int argc, char **argv) {
    if (argc < 5) {
        fprintf(stderr, "usage: first_cull_harness safety|count|degenerate <scene.json> <random_spheres> <seed> ...\n");
        return 2;
    }
    Host h;
    try {
        if (!load(argv[2], atoi(argv[3]) != 0, (uint64_t)atoll(argv[4]), &h)) return 2;
    } catch (const SceneError &e) {
        fprintf(stderr, "%s\n", e.msg.c_str());
        return 2;
    }
    if (!strcmp(argv[1], "safety")) {
        std::vector<pt_camera> cams{h.sc.camera};
        for (int a = 5; a + 11 <= argc; a += 11) cams.push_back(camera_arg(argv + a));
        return safety(h, cams);
    }
    if (!strcmp(argv[1], "count") && argc >= 7) {
        const pt_camera cam = argc >= 18 ? camera_arg(argv + 7) : h.sc.camera;
        return count(h, cam, (uint32_t)atoi(argv[5]), (uint32_t)atoi(argv[6]));
    }
    if (!strcmp(argv[1], "degenerate")) return degenerate(h);
    return 2;
}
