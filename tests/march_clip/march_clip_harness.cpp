// Test-only stand-alone program (host build of the product headers): replays march jobs through the plain march
// (the whole bound interval, then the caller's `t > best` test) and the clipped one (march::clip_to_best first),
// and counts every job whose (accepted, t) differs, bit for bit, and the iterations each form takes.
//   march_clip_harness capture <scene.json> <pixels> <spp>   the jobs of the product's host path (trace_pixel at
//                                                            1920x1080, depth 8), each with the best hit it starts
//                                                            against
//   march_clip_harness synth                                 synthetic Heart jobs with `best` placed around every
//                                                            point the exactness argument speaks about
// Prints "key value" lines; exit status 1 if any job differs.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <vector>

struct Job {
    double step;
    int passes;
    double o[3], d[3];
    double best;
};
static std::vector<Job> g_jobs;
static bool g_capture = false;
// a march start of the host path, and the best hit its interval is clipped to right after (trace_pixel's PH_SELECT)
#define PT_MCAPTURE(step0, passes, ox, oy, oz, dx, dy, dz)                                       \
    do {                                                                                          \
        if (g_capture) g_jobs.push_back(Job{step0, passes, {ox, oy, oz}, {dx, dy, dz}, INFINITY}); \
    } while (0)
#define PT_MCLIP(best_, step0, start, end)                            \
    do {                                                              \
        if (g_capture && !g_jobs.empty()) g_jobs.back().best = best_; \
    } while (0)

#include "../../rs-pathtracing_amd/csrc/pt_accel.hpp"
#include "../../rs-pathtracing_amd/csrc/pt_device.hpp"
#include "../../rs-pathtracing_amd/csrc/pt_scene.hpp"

using namespace pt;

struct Res {
    bool started, accepted;
    int status;
    double t, start, end;
    long iters;
};

// One job against `best`: the march as wf_march / trace_pixel run it, with or without the clip.
template <int FK>
static Res run(const Job &j, double best, bool clip) {
    march::FParams F{};
    F.func = march::F_HEART;
    march::MarchState m;
    Res r{false, false, march::M_MISS, 0.0, 0.0, 0.0, 0};
    if (!march::march_begin<FK>(F, j.step, j.passes, j.o[0], j.o[1], j.o[2], j.d[0], j.d[1], j.d[2], &m)) return r;
    r.start = m.start;
    r.end = m.end;
    if (clip && !march::clip_to_best(best, j.step, &m.start, &m.end)) return r;
    r.started = true;
    march::MarchStats st{0, 0, 0, 0};
    do {
        r.status = march::march_step<false, true, FK>(m, &st);
        r.iters++;
    } while (r.status == march::M_RUNNING);
    r.t = m.t;
    r.accepted = r.status == march::M_DONE && !(m.t < T_MIN || m.t > best);  // ray_marching.rs:55-57
    return r;
}

struct Tally {
    long jobs = 0, differ = 0, guard = 0;
    long plain_iters = 0, clip_iters = 0, plain_started = 0, clip_started = 0;
    long chord_cut = 0, dropped = 0, done_discarded = 0, cut_plain_iters = 0, cut_clip_iters = 0;
};

template <int FK>
static void compare(const Job &j, double best, Tally *T) {
    const Res a = run<FK>(j, best, false), b = run<FK>(j, best, true);
    T->jobs++;
    const bool same = a.accepted == b.accepted && (!a.accepted || memcmp(&a.t, &b.t, 8) == 0);
    if (!same) {
        if (T->differ < 10)
            printf("differ: best %.17g step %.17g passes %d plain (%d, %.17g) clipped (%d, %.17g) chord [%.17g, %.17g]\n",
                   best, j.step, j.passes, (int)a.accepted, a.t, (int)b.accepted, b.t, a.start, a.end);
        T->differ++;
    }
    T->guard += (a.status == march::M_GUARD) + (b.status == march::M_GUARD);
    T->plain_iters += a.iters;
    T->clip_iters += b.iters;
    T->plain_started += a.started;
    T->clip_started += b.started;
    if (!a.started) return;
    const double cap = best + 4.0 * fabs(j.step);
    const bool cut = a.end > cap;
    T->chord_cut += cut;
    T->dropped += a.start > cap;
    T->done_discarded += a.status == march::M_DONE && !a.accepted;
    if (cut) {
        T->cut_plain_iters += a.iters;
        T->cut_clip_iters += b.iters;
    }
}

static void report(const char *what, const Tally &T) {
    printf("%s_jobs %ld\n", what, T.jobs);
    printf("%s_differ %ld\n", what, T.differ);
    printf("%s_guard %ld\n", what, T.guard);
    printf("%s_chord_beyond_cap %ld\n", what, T.chord_cut);
    printf("%s_chord_starts_behind_cap %ld\n", what, T.dropped);
    printf("%s_done_then_discarded %ld\n", what, T.done_discarded);
    printf("%s_marches_plain %ld\n", what, T.plain_started);
    printf("%s_marches_clipped %ld\n", what, T.clip_started);
    printf("%s_iters_plain %ld\n", what, T.plain_iters);
    printf("%s_iters_clipped %ld\n", what, T.clip_iters);
    printf("%s_cut_jobs_iters_plain %ld\n", what, T.cut_plain_iters);
    printf("%s_cut_jobs_iters_clipped %ld\n", what, T.cut_clip_iters);
}

static int capture(const char *path, long npx, uint32_t spp) {
    std::ifstream f(path);
    if (!f) {
        fprintf(stderr, "cannot read %s\n", path);
        return 2;
    }
    std::stringstream ss;
    ss << f.rdbuf();
    const std::string js = ss.str();
    Scene sc = scene_from_json(js.c_str(), js.size(), true, 1);
    Accel acc = build_accel(sc, sc.json_shapes);
    std::vector<DShape> shapes;
    std::vector<DMaterial> mats;
    for (auto &s : sc.shapes) shapes.push_back(to_device(s));
    for (auto &m : sc.materials) mats.push_back(to_device(m));
    const std::vector<DQGrid> qbuf = pack_qnodes(acc);
    dev::Scene v{};
    view_of_host(v, sc, acc, shapes, mats, qbuf);
    const uint32_t W = 1920, H = 1080;
    const FrameParams P = frame_params(sc.camera, W, H, spp, 8, 1, uniform_incl_scale(-1.0, 1.0));
    g_capture = true;
    Ctr ctr;
    memset(&ctr, 0, sizeof ctr);
    for (long i = 0; i < npx; i++) {  // a scattered sample of the frame's pixels
        const uint64_t pix = (uint64_t)(i * 2654435761ull) % (W * H);
        dev::trace_pixel<4, true>(v, P, (uint32_t)(pix % W), (uint32_t)(pix / W), &ctr);
    }
    g_capture = false;
    Tally T;
    for (const Job &j : g_jobs) compare<march::F_HEART>(j, j.best, &T);
    report("capture", T);
    return T.differ ? 1 : 0;
}

static uint64_t g_seed = 0x243F6A8885A308D3ull;
static uint64_t next_u64() {
    g_seed += 0x9E3779B97F4A7C15ull;
    uint64_t z = g_seed;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static double unit() { return (double)(next_u64() >> 11) * (1.0 / 9007199254740992.0) * 2.0 - 1.0; }
static void in_ball(double r, double *p) {
    do {
        for (int k = 0; k < 3; k++) p[k] = unit();
    } while (p[0] * p[0] + p[1] * p[1] + p[2] * p[2] > 1.0);
    for (int k = 0; k < 3; k++) p[k] *= r;
}

// Every placement of `best` for one job: around the chord's ends, the coarse crossing (the end of pass 0) and the
// final t, by whole steps and single ulps, and where the cap (best + 4 steps) itself falls on those points.
template <int FK>
static void placements(const Job &j, Tally *T) {
    const Res full = run<FK>(j, INFINITY, false);
    if (!full.started) return;
    Job j1 = j;
    j1.passes = 1;
    const Res coarse = run<FK>(j1, INFINITY, false);
    const double s = fabs(j.step), up = INFINITY, dn = -INFINITY;
    std::vector<double> bs = {full.start - s,  nextafter(full.start, dn), full.start, nextafter(full.start, up),
                              full.start - 4.0 * s, nextafter(full.start - 4.0 * s, dn), nextafter(full.start - 4.0 * s, up),
                              full.end,        nextafter(full.end, dn),   nextafter(full.end, up),
                              full.end - 4.0 * s, full.end + 10.0 * s,    full.end * 2.0, INFINITY,
                              0.5 * (full.start + full.end)};
    std::vector<double> bases;
    if (coarse.status == march::M_DONE) {
        bases.push_back(coarse.t);
        bs.push_back(0.5 * (full.start + coarse.t));  // between the start and the coarse crossing
    }
    if (full.status == march::M_DONE) bases.push_back(full.t);
    for (double b : bases) {
        bs.push_back(b);
        bs.push_back(nextafter(b, dn));
        bs.push_back(nextafter(b, up));
        for (double k : {1.0, 2.0, 3.0, 4.0, 5.0, 6.0}) {
            bs.push_back(b - k * s);
            bs.push_back(b + k * s);
        }
        // the cap on the point itself, and one ulp and one fine step (1 % of a step) to either side
        const double c = b - 4.0 * s;
        for (double q : {nextafter(c, dn), nextafter(c, up), c - 0.01 * s, c + 0.01 * s, c - 1.02 * s, c + 1.02 * s})
            bs.push_back(q);
    }
    for (double b : bs) compare<FK>(j, b, T);
}

static int synth() {
    Tally T;
    const double scales[2] = {1.0, 82.5};  // the Heart at unit scale and at cornell_box.json's
    const double steps[2] = {0.01, 0.003};
    for (int si = 0; si < 2; si++)
        for (int ti = 0; ti < 2; ti++)
            for (int passes = 1; passes <= 4; passes++)
                for (int n = 0; n < 96; n++) {
                    Job j{};
                    j.step = steps[ti];
                    j.passes = passes;
                    j.best = INFINITY;
                    double target[3];
                    in_ball(n % 4 == 3 ? 1.44 : 1.1, target);  // (every fourth ray: anywhere in the bound, most of them misses)
                    if (n % 8 == 5) {
                        in_ball(1.4, j.o);  // the origin inside the bound (and now and then inside the Heart)
                    } else {
                        double dir[3];
                        in_ball(1.0, dir);
                        const double l = sqrt(dir[0] * dir[0] + dir[1] * dir[1] + dir[2] * dir[2]) + 1e-300;
                        for (int k = 0; k < 3; k++) j.o[k] = dir[k] / l * (2.0 + 2.0 * fabs(unit()));
                    }
                    double d[3] = {target[0] - j.o[0], target[1] - j.o[1], target[2] - j.o[2]};
                    const double l = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) + 1e-300;
                    // a world-space unit direction through the inverse of a uniform scale: t runs in world units
                    for (int k = 0; k < 3; k++) j.d[k] = d[k] / l / scales[si];
                    if (n & 1) placements<march::F_HEART>(j, &T);
                    else placements<march::F_ANY>(j, &T);
                }
    report("synth", T);
    return T.differ ? 1 : 0;
}

int main(int argc, char **argv) {
    if (argc >= 5 && !strcmp(argv[1], "capture")) return capture(argv[2], atol(argv[3]), (uint32_t)atoi(argv[4]));
    if (argc >= 2 && !strcmp(argv[1], "synth")) return synth();
    fprintf(stderr, "usage: march_clip_harness capture <scene.json> <pixels> <spp> | synth\n");
    return 2;
}
