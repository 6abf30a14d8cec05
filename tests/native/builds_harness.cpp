// The choice of kernel builds and the knob table (pt_builds.hpp) behind a C boundary, for tests/test_builds.py.
#include "../../rs-pathtracing_amd/csrc/pt_builds.hpp"

using namespace pt;
using namespace pt::builds;

extern "C" {

// n cases.  in: 16 words each: ext, fkind, nnodes, nmarch, has_qnodes, scene_diag, depth, samples, window,
// window_empty, wave_diag_on, diag_buffer, then the knobs engine, mega_waves, wf_bounce_waves, wf_walk.
// out: 19 words each: engine, mega (nw, waves, fk), bounce (waves, fk, ext, bigbvh, split, deep, diag),
// walk (on, waves, qn), march (on, fk, diag), presel, ext.
void builds_choose(const int64_t *in, int64_t n, int64_t *out) {
    for (int64_t k = 0; k < n; k++) {
        const int64_t *w = in + k * 16;
        Inputs i{};
        i.ext = w[0] != 0;
        i.fkind = (int)w[1];
        i.nnodes = (int)w[2];
        i.nmarch = (int)w[3];
        i.has_qnodes = w[4] != 0;
        i.scene_diag = (int)w[5];
        i.depth = (uint32_t)w[6];
        i.samples = (uint64_t)w[7];
        i.window = w[8] != 0;
        i.window_empty = w[9] != 0;
        i.wave_diag_on = w[10] != 0;
        i.diag_buffer = w[11] != 0;
        i.tune.engine = (int)w[12];
        i.tune.mega_waves = (int)w[13];
        i.tune.wf_bounce_waves = (int)w[14];
        i.tune.wf_walk = (int)w[15];
        const Choice c = choose(i);
        const int64_t v[19] = {c.engine,      c.mega.nw,       c.mega.waves,   c.mega.fk,     c.bounce.waves,
                               c.bounce.fk,   c.bounce.ext,    c.bounce.bigbvh, c.bounce.split, c.bounce.deep,
                               c.bounce.diag, c.walk.on,       c.walk.waves,   c.walk.qn,     c.march.on,
                               c.march.fk,    c.march.diag,    c.presel,       c.ext};
        for (int j = 0; j < 19; j++) out[k * 19 + j] = v[j];
    }
}

// The instantiated builds of kernel `which` (0 megakernel: nw, waves, fk; 1 bounce: waves, fk, ext, bigbvh, split,
// deep; 2 walk: waves, qn; 3 march: fk), row after row; returns how many there are (out may be null).
int builds_list(int which, int64_t *out) {
    int n = 0;
#define PUT(...)                                                            \
    {                                                                       \
        const int64_t row[] = {__VA_ARGS__};                                \
        const int cols = (int)(sizeof(row) / sizeof(row[0]));               \
        for (int j = 0; out && j < cols; j++) out[n * cols + j] = row[j];   \
        n++;                                                                \
    }
    if (which == 0) { PT_MEGA_BUILDS(PUT) }
    if (which == 1) { PT_BOUNCE_BUILDS(PUT) }
    if (which == 2) { PT_WALK_BUILDS(PUT) }
    if (which == 3) { PT_MARCH_BUILDS(PUT) }
#undef PUT
    return n;
}

// The record of what a frame launched (builds::Ran, builds::key).  ran_keys: builds::key of every instantiated build
// of kernel `which`, in list order (the expression the launchers record); returns how many.  One Ran, empty after
// ran_reset: ran_note writes a field as the launchers do (0 engine, 1 mega, 2 bounce, 3 walk, 4 march), ran_read
// is ran_get (0: no such name; *v is then untouched).
int ran_keys(int which, int64_t *out) {
    int n = 0;
#define KEY(...) out[n++] = key(__VA_ARGS__);
    if (which == 0) { PT_MEGA_BUILDS(KEY) }
    if (which == 1) { PT_BOUNCE_BUILDS(KEY) }
    if (which == 2) { PT_WALK_BUILDS(KEY) }
    if (which == 3) { PT_MARCH_BUILDS(KEY) }
#undef KEY
    return n;
}
static Ran g_ran;
void ran_reset() { g_ran = Ran{}; }
void ran_note(int field, int64_t v) {
    int64_t Ran::*const m[] = {&Ran::engine, &Ran::mega, &Ran::bounce, &Ran::walk, &Ran::march};
    g_ran.*(m[field]) = v;
}
int ran_read(const char *name, int64_t *v) { return ran_get(g_ran, name, v) ? 1 : 0; }

// The knob table: names in the API's order, and a row's range, set (up to 8 values) and zero rule.
int knob_count() { return KNOB_COUNT; }
const char *knob_name(int k) { return k >= 0 && k < KNOB_COUNT ? KNOBS[k].name : nullptr; }
// out[3 + nset]: lo, hi, or_zero, then the set; returns nset (0: the whole range)
int knob_legal(int k, int64_t *out) {
    const Knob &kn = KNOBS[k];
    out[0] = kn.lo, out[1] = kn.hi, out[2] = kn.or_zero;
    for (int j = 0; j < kn.nset; j++) out[3 + j] = kn.set[j];
    return kn.nset;
}

// One Tuning, at its defaults after knobs_reset: set (1 accepted, 0 refused) and get (0: unknown name).
static Tuning g_tune;
void knobs_reset() { g_tune = tuning_defaults(); }
int knobs_set(const char *name, int64_t v) { return tuning_set(&g_tune, name, v) ? 1 : 0; }
int knobs_get(const char *name, int64_t *v) { return tuning_get(g_tune, name, v) ? 1 : 0; }
}
