// pt_builds.hpp — which kernel build runs: the tuning knobs and their legal values, the lists of the builds that
// are instantiated, and builds::choose, which picks a frame's engine and builds once, before anything is launched
// (DESIGN.md §2 has the rules as a table).  The launchers (pt_kernel.hip, pt_wave.hip) only look the chosen
// build up in its list.  Standard library only, so the host compiler builds it for tests/test_builds.py.
#pragma once
#include <cstdint>
#include <cstring>

#include "pt_dims.hpp"

namespace pt {

// Tuning knobs of the render engines (pt_renderer_set_option; the option names
// are the field names).  The defaults are the measured optimum on MI355X
// (DESIGN.md §5); bench.py reports every knob that differs from its default.
struct Tuning {
    int engine = 0;                  // 0 auto (builds::choose below), 1 megakernel, 2 wavefront
    int mega_waves = 4;              // megakernel register budget, waves per SIMD (2..5; C5 (100k spheres, compact
                                     // BVH): 2 waves 845-849, 3: 1044, 4: 1109 M samples/s)
    int diag = 0;                    // bit 0: skip ray-marched shapes (a timing ablation, not the reference)
    int wf_slots = 2;                // sample chunks in flight, one stream each (1..4)
    int64_t wf_paths = 0;            // path slots per chunk (256 .. 2^28; 0: 48M up to depth 16, else 256M).  Deep
                                     // frames spend a quarter of a chunk in its tail of latency-bound iterations:
                                     // C2 depth 50 48M 1156, 96M 1226, 128M 1230-1241, 160M 1235 M samples/s (~58 GB
                                     // per chunk stream at 128M); at depth 8 128M costs the bounce 3 % (C2 2010 vs
                                     // 2039), C1, C3, C5 unchanged (round 5 r5w-r5y)
    int wf_min_chunks = 1;           // at least this many sample chunks per frame (1..4096)
    int wf_bounce_waves = 3;         // wf_bounce register budget (2, 3, 4, 5, 6, 8)
    int wf_march_slice = 256;        // march-queue run dealt to a block (0 = contiguous share)
    int wf_walk = 5;                 // large-tree scenes without marched shapes: the BVH walk in its own kernel (wf_walk)
                                     // at this register budget, waves per SIMD (4, 5, 6, 8; 0: the walk in the bounce)
    int bvh_leaf = 1;                // shapes per BVH leaf (1..16; C5 677 / 609 / 534 M samples/s at 1 / 2 / 4)
};
// the measured defaults; a renderer changes them only through pt_renderer_set_option
inline Tuning tuning_defaults() { return Tuning{}; }

constexpr int WF_MAX_SLOTS = 4;  // chunk streams a renderer can hold (WaveWorkspace)

// The knobs whose legal values are a set and not a range.  tuning_set, builds::choose and the test read these.
constexpr int MEGA_WAVES[] = {2, 3, 4, 5};
constexpr int BOUNCE_WAVES[] = {2, 3, 4, 5, 6, 8};  // also the budgets of the small-tree Heart bounce builds
constexpr int BOUNCE_WAVES_BIG[] = {3, 4, 5};       // the budgets the large-tree bounce builds without a Heart have
constexpr int WALK_WAVES[] = {0, 4, 5, 6, 8};       // 0: no wf_walk; the others are the quantized walk's budgets

// One row per option, in the order the API reports them (pt_option_name).  A value is legal when it is in
// [lo, hi] and in `set` (when there is one), or when it is 0 and or_zero says so (wf_paths: 0 = by depth).
struct Knob {
    const char *name;
    int Tuning::*i;       // the member, or
    int64_t Tuning::*l;   // the 64-bit member
    int64_t lo, hi;
    const int *set;
    int nset;
    bool or_zero;
};
#define PT_KNOB_SET(a) a, (int)(sizeof(a) / sizeof(a[0]))
constexpr Knob KNOBS[] = {
    {"engine", &Tuning::engine, nullptr, 0, 2, nullptr, 0, false},
    {"mega_waves", &Tuning::mega_waves, nullptr, 2, 5, PT_KNOB_SET(MEGA_WAVES), false},
    {"diag", &Tuning::diag, nullptr, 0, 1, nullptr, 0, false},
    {"wf_slots", &Tuning::wf_slots, nullptr, 1, WF_MAX_SLOTS, nullptr, 0, false},
    {"wf_paths", nullptr, &Tuning::wf_paths, 256, (int64_t)1 << 28, nullptr, 0, true},
    {"wf_min_chunks", &Tuning::wf_min_chunks, nullptr, 1, 4096, nullptr, 0, false},
    {"wf_bounce_waves", &Tuning::wf_bounce_waves, nullptr, 2, 8, PT_KNOB_SET(BOUNCE_WAVES), false},
    {"wf_march_slice", &Tuning::wf_march_slice, nullptr, 0, 1 << 20, nullptr, 0, false},
    {"wf_walk", &Tuning::wf_walk, nullptr, 0, 8, PT_KNOB_SET(WALK_WAVES), false},
    {"bvh_leaf", &Tuning::bvh_leaf, nullptr, 1, 16, nullptr, 0, false},
};
#undef PT_KNOB_SET
constexpr int KNOB_COUNT = (int)(sizeof(KNOBS) / sizeof(KNOBS[0]));

inline bool in_set(const int *set, int n, int64_t v) {
    for (int k = 0; k < n; k++)
        if (set[k] == v) return true;
    return false;
}
inline const Knob *knob(const char *name) {
    for (const Knob &k : KNOBS)
        if (name && !strcmp(name, k.name)) return &k;
    return nullptr;
}
// false for an unknown name or an illegal value (t is then unchanged)
inline bool tuning_set(Tuning *t, const char *name, int64_t v) {
    const Knob *k = knob(name);
    if (!k) return false;
    const bool legal = v >= k->lo && v <= k->hi && (!k->set || in_set(k->set, k->nset, v));
    if (!legal && !(k->or_zero && v == 0)) return false;
    if (k->l) t->*(k->l) = v;
    else t->*(k->i) = (int)v;
    return true;
}
inline bool tuning_get(const Tuning &t, const char *name, int64_t *v) {
    const Knob *k = knob(name);
    if (!k) return false;
    *v = k->l ? t.*(k->l) : (int64_t)(t.*(k->i));
    return true;
}

namespace builds {

// Frames of at least this many samples take the wavefront engine even
// without ray-marched shapes: on C5 (100k spheres, BVH) it runs 1394 against
// the megakernel's 1026 M samples/s (the path state is dense by position and
// the bounce waves stay full where the megakernel's lanes idle on finished
// paths and unequal BVH walks); below it the per-chunk launches cost more
// than they save.
constexpr uint64_t WAVE_MIN_SAMPLES = 1ull << 22;
// Chunks of fewer pixels unwind in their own pass (wf_unwind) before their reduce.  This is per chunk, so the
// launch decides it and not choose().
constexpr uint32_t UNWIND_PIXELS = 1u << 18;

// Attenuation-stack width by depth, in 64-bit words: one 32-bit material id per bounce.  The widest build holds
// MAX_REG_DEPTH ids; deeper calls go elsewhere (the wavefront engine, the memory-stack probe) or are refused.
constexpr int stack_words(uint32_t depth) { return depth <= 8 ? 4 : depth <= 16 ? 8 : depth <= 32 ? 16 : 32; }
static_assert(MAX_REG_DEPTH == 2 * 32, "IdStack<32> holds 64 ids");

// The builds that are instantiated, one list per kernel, as template arguments.  The launchers expand them
// into "if the chosen build is this entry, launch this instantiation"; tests/test_builds.py checks that choose()
// only ever names an entry and that every entry is chosen by some frame.
// render_tiles<NW, WAVES, FK>
#define PT_MEGA_BUILDS(X)                                                                                  \
    X(4, 2, march::F_HEART) X(4, 3, march::F_HEART) X(4, 4, march::F_HEART) X(4, 5, march::F_HEART)       \
    X(4, 2, march::F_ANY) X(8, 2, march::F_ANY) X(16, 2, march::F_ANY) X(32, 2, march::F_ANY)
// wf_bounce<FIRST, WAVES, FK, EXT, BIGBVH, SPLIT, DEEP>, each for both values of FIRST
#define PT_BOUNCE_BUILDS(X)                                                                                \
    X(2, march::F_ANY, true, false, false, true) X(2, march::F_ANY, false, false, false, true)            \
    X(3, march::F_NONE, false, true, true, false) X(4, march::F_NONE, false, true, true, false)           \
    X(5, march::F_NONE, false, true, true, false)                                                          \
    X(2, march::F_ANY, true, false, false, false) X(2, march::F_ANY, false, false, false, false)          \
    X(3, march::F_NONE, false, true, false, false) X(4, march::F_NONE, false, true, false, false)         \
    X(5, march::F_NONE, false, true, false, false)                                                         \
    X(3, march::F_HEART, false, true, false, false)                                                        \
    X(2, march::F_HEART, false, false, false, false) X(3, march::F_HEART, false, false, false, false)     \
    X(4, march::F_HEART, false, false, false, false) X(5, march::F_HEART, false, false, false, false)     \
    X(6, march::F_HEART, false, false, false, false) X(8, march::F_HEART, false, false, false, false)
// wf_walk<WAVES, QN>
#define PT_WALK_BUILDS(X) X(5, false) X(4, true) X(5, true) X(6, true) X(8, true)
// wf_march<FK>
#define PT_MARCH_BUILDS(X) X(march::F_HEART) X(march::F_ANY)

enum Engine : int { MEGA = 0, WAVE = 1, REFUSE = 2 };

struct Mega {
    int nw, waves, fk;
    bool is(int n, int w, int f) const { return nw == n && waves == w && fk == f; }
};
struct Bounce {
    int waves, fk;
    bool ext, bigbvh, split, deep;
    bool diag;  // launched with the workspace's diag buffer (diagnostic builds); no build of its own
    bool is(int w, int f, bool e, bool b, bool s, bool d) const {
        return waves == w && fk == f && ext == e && bigbvh == b && split == s && deep == d;
    }
};
struct Walk {
    bool on;  // the new rays' BVH walk runs in wf_walk, after the compaction
    int waves;
    bool qn;
    bool is(int w, bool q) const { return waves == w && qn == q; }
};
struct March {
    bool on;
    int fk;
    bool diag;  // launched with the workspace's diag buffer, when there is one
    bool is(int f) const { return fk == f; }
};

// What the choice depends on.
struct Inputs {
    bool ext;          // DeviceScene::ext: non-solid textures or a Torus
    int fkind;         // DeviceScene::fkind: F_HEART (every marched shape is a Heart, or there is none) or F_ANY
    int nnodes, nmarch;
    bool has_qnodes;   // the tree has its quantized form
    int scene_diag;    // DeviceScene::diag
    uint32_t depth;
    uint64_t samples;  // tile_count * 256 * spp
    bool window;       // the launch renders a window of the frame's samples: s_begin > 0 || (s_end && s_end < spp)
    bool window_empty;
    bool wave_diag_on;  // a PT_WAVE_DIAG build with pt_wave_diag enabled
    bool diag_buffer;   // the workspace has a diag buffer
    Tuning tune;
};

// A frame's engine and builds.  Only the chosen engine's parts are filled in; the rest stay zero.
struct Choice {
    Engine engine;
    Mega mega;
    Bounce bounce;
    Walk walk;
    March march;
    bool presel;  // march jobs pre-selected by the bounce kernel (plan::Input::presel)
    bool ext;     // the wf_unwind / wf_reduce builds
};

// A build's template arguments in its list's column order as one number: sum((field + 2) << (6 * j)) (a field is in
// [-2, 32]: one base-64 digit each; a bool counts as 0 or 1).  tests/test_builds.py packs its chosen sets the same way.
constexpr int64_t key() { return 0; }
template <class... T>
constexpr int64_t key(int field, T... rest) {
    return (int64_t)(field + 2) + (key(rest...) << 6);
}

// What the last launch_render call launched (WaveWorkspace::ran): written by the launchers in the branch that
// launches, never from choose()'s output, and read through pt_renderer_get_option as "ran_engine" (0 megakernel,
// 1 wavefront) and "ran_mega", "ran_bounce", "ran_walk", "ran_march" (the build's key; FIRST is no part of it).
// -1: the call launched none of that kernel (ran_engine: nothing at all, e.g. a refused call).
struct Ran {
    int64_t engine = -1, mega = -1, bounce = -1, walk = -1, march = -1;
};
inline bool ran_get(const Ran &r, const char *name, int64_t *v) {
    static constexpr struct {
        const char *name;
        int64_t Ran::*m;
    } NAMES[] = {{"ran_engine", &Ran::engine}, {"ran_mega", &Ran::mega}, {"ran_bounce", &Ran::bounce},
                 {"ran_walk", &Ran::walk}, {"ran_march", &Ran::march}};
    for (const auto &n : NAMES)
        if (name && !strcmp(name, n.name)) {
            *v = r.*(n.m);
            return true;
        }
    return false;
}

// knob when the builds of `set` have that budget, else the default build's
template <int N>
inline int budget(const int (&set)[N], int knob, int dflt) {
    return in_set(set, N, knob) ? knob : dflt;
}

// The first rule that matches wins, in every part.
inline Choice choose(const Inputs &in) {
    using namespace march;
    const Tuning &tu = in.tune;
    Choice c{};
    const bool deep = in.depth > MAX_REG_DEPTH;  // the wavefront engine's id stacks live in memory: never the megakernel
    if (deep || in.window)  // (a sample window: only the wavefront engine keeps running sums across launches)
        c.engine = in.window && in.window_empty ? REFUSE : WAVE;
    else if (in.ext)  // textures / Torus: the extended builds live in the wavefront engine
        c.engine = WAVE;
    else if (tu.engine != 0)
        c.engine = tu.engine == 1 ? MEGA : WAVE;
    else
        c.engine = (in.scene_diag & 1) == 0 && (in.nmarch > 0 || in.samples >= WAVE_MIN_SAMPLES) ? WAVE : MEGA;

    if (c.engine == MEGA) {
        // Heart-only (or no marched shape) at depth <= 8: the single-function build at Tuning::mega_waves; the
        // generic build and the deeper ones (wider attenuation stacks) use the 2-wave budget
        if (in.depth <= 8 && in.fkind == F_HEART) c.mega = Mega{4, budget(MEGA_WAVES, tu.mega_waves, 4), F_HEART};
        else c.mega = Mega{stack_words(in.depth), 2, F_ANY};
    }
    if (c.engine != WAVE) return c;

    const bool big = in.nnodes >= BIG_BVH_NODES;
    // the BVH walk in wf_walk: a large tree (C5's 100k-sphere tree has ~200k nodes, cornell's ~960), no marched shape
    const bool split = !deep && tu.wf_walk != 0 && !in.ext && big && in.nmarch == 0;
    const int knob = tu.wf_bounce_waves;
    Bounce &b = c.bounce;
    if (deep)  // the generic builds with the stack count in the id stack, whatever the scene
        b = Bounce{2, F_ANY, in.ext, false, false, true, false};
    else if (split)  // shade and store the new ray only: wf_walk traces it
        b = Bounce{budget(BOUNCE_WAVES_BIG, knob, 3), F_NONE, false, true, true, false, false};
    else if (in.ext)  // the generic extended build
        b = Bounce{2, F_ANY, true, false, false, false, false};
    else if (in.fkind != F_HEART)  // another ray-marched function: the generic build
        b = Bounce{2, F_ANY, false, false, false, false, false};
    else if (in.wave_diag_on)
        b = Bounce{2, F_HEART, false, false, false, false, true};
    else if (big && in.nmarch == 0)  // the FMA slab build without march pre-check or Heart code
        b = Bounce{budget(BOUNCE_WAVES_BIG, knob, 3), F_NONE, false, true, false, false, false};
    else if (big && knob == 3)  // the default budget, a large BVH with a marched shape
        b = Bounce{3, F_HEART, false, true, false, false, false};
    else
        b = Bounce{budget(BOUNCE_WAVES, knob, 3), F_HEART, false, false, false, false, false};

    if (split) {
        if (!in.has_qnodes) c.walk = Walk{true, 5, false};
        else c.walk = Walk{true, budget(WALK_WAVES, tu.wf_walk, 5), true};  // (wf_walk is not 0 here)
    }
    if (in.nmarch != 0) {  // else the march queue is always empty
        // a deep frame has no Heart-only march; the generic build takes no diagnostics
        if (deep || in.fkind != F_HEART) c.march = March{true, F_ANY, false};
        else c.march = March{true, F_HEART, true};
    }
    // pre-selected march jobs (one marched shape): the bounce kernel hands the march its object-space ray
    // and bound (C2 +9 %: iso march 340 -> 275 ms, bounce 248 -> 256, round 1)
    c.presel = in.nmarch == 1 && !in.diag_buffer;
    c.ext = in.ext;
    return c;
}

}  // namespace builds
}  // namespace pt
