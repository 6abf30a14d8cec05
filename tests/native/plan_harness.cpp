// The wavefront frame plan (pt_plan.hpp) behind a C boundary, for tests/test_wave_plan.py.
// Inputs are 12 words: ntiles, s_begin, s_end, spp, depth, progressive, textured, presel, wf_paths, wf_slots,
// wf_min_chunks, avail_bytes (all ones: unknown).
#include "../../rs-pathtracing_amd/csrc/pt_plan.hpp"

using namespace pt::plan;

static Input input(const uint64_t *w) {
    Input in;
    in.ntiles = (uint32_t)w[0];
    in.s_begin = (uint32_t)w[1];
    in.s_end = (uint32_t)w[2];
    in.spp = (uint32_t)w[3];
    in.depth = (uint32_t)w[4];
    in.progressive = w[5] != 0;
    in.textured = w[6] != 0;
    in.presel = w[7] != 0;
    in.wf_paths = (int64_t)w[8];
    in.wf_slots = (int)w[9];
    in.wf_min_chunks = (int)w[10];
    in.avail_bytes = (size_t)w[11];
    return in;
}

extern "C" {

// out[10]: cap_want, group_tiles, npix_max, ns, cap, cap_tiles, slots, iters, cnt_words, bytes
void plan_make(const uint64_t *w, uint64_t *out) {
    const Plan pl = make_plan(input(w));
    const uint64_t v[10] = {pl.cap_want, pl.group_tiles,      pl.npix_max,        pl.ns,        pl.cap,
                            pl.cap_tiles, (uint64_t)pl.slots, (uint64_t)pl.iters, pl.cnt_words, pl.bytes};
    for (int k = 0; k < 10; k++) out[k] = v[k];
}

// out[26]: the regions' offsets, their sizes (0: absent), slot_stride, acc, acc_size, total
void plan_layout(const uint64_t *w, uint64_t *out) {
    const Layout L = make_plan(input(w)).lay;
    for (int r = 0; r < R_COUNT; r++) out[r] = L.off[r], out[R_COUNT + r] = L.size[r];
    out[2 * R_COUNT + 0] = L.slot_stride;
    out[2 * R_COUNT + 1] = L.acc;
    out[2 * R_COUNT + 2] = L.acc_size;
    out[2 * R_COUNT + 3] = L.total;
}

// The chunk records (g0, gt, s0, ns, slot, step), the first `max` of them; returns how many there are.
uint64_t plan_chunks(const uint64_t *w, uint32_t *out, uint64_t max) {
    const Input in = input(w);
    const std::vector<Chunk> list = chunk_list(in, make_plan(in));
    for (size_t c = 0; c < list.size() && c < max; c++) {
        const Chunk &ch = list[c];
        const uint32_t v[6] = {ch.g0, ch.gt, ch.s0, ch.ns, (uint32_t)ch.slot, ch.step};
        for (int k = 0; k < 6; k++) out[c * 6 + k] = v[k];
    }
    return list.size();
}
}
