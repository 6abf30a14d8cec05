// The frame plan of deep frames (depth > 64) behind a C boundary, for tests/test_deep_plan.py: plan_harness.cpp's
// entry points (the plan as make_plan gives it), and the memory fit launch_render_wave applies on top of it
// (plan::make_plan_fit, plan::fits_device, plan::fits).  Standard C++ only: the test builds it with the host compiler.
#include "plan_harness.cpp"

extern "C" {

// plan_fit(w, hard_bytes, out): the plan launch_render_wave runs or refuses on a device that can hold hard_bytes
// (free memory plus the workspace held, no reserve).  out[0..9] as plan_make, out[10] the chunk streams the plan was
// made for (wf_slots after the cut to one), out[11] the device can hold it (1) or the frame is refused (0),
// out[12..22] the regions' sizes.
void plan_fit(const uint64_t *w, uint64_t hard_bytes, uint64_t *out) {
    Input in = input(w);
    const Plan pl = make_plan_fit(&in, (size_t)hard_bytes);
    const uint64_t v[10] = {pl.cap_want, pl.group_tiles,      pl.npix_max,        pl.ns,        pl.cap,
                            pl.cap_tiles, (uint64_t)pl.slots, (uint64_t)pl.iters, pl.cnt_words, pl.bytes};
    for (int k = 0; k < 10; k++) out[k] = v[k];
    out[10] = (uint64_t)in.wf_slots;
    out[11] = fits_device(pl, (size_t)hard_bytes) ? 1 : 0;
    for (int r = 0; r < R_COUNT; r++) out[12 + r] = pl.lay.size[r];
}

// fits() of the plan make_plan gives: within avail_bytes, the free memory less the reserve
int plan_fits(const uint64_t *w) {
    const Input in = input(w);
    return fits(in, make_plan(in)) ? 1 : 0;
}

// the limits: MAX_DEPTH, PACKED_COUNT_DEPTH, MIN_CHUNK_PATHS, RESERVE_BYTES
void plan_limits(uint64_t *out) {
    out[0] = MAX_DEPTH;
    out[1] = PACKED_COUNT_DEPTH;
    out[2] = MIN_CHUNK_PATHS;
    out[3] = RESERVE_BYTES;
    out[4] = deep(PACKED_COUNT_DEPTH) ? 1 : 0;
    out[5] = deep(PACKED_COUNT_DEPTH + 1) ? 1 : 0;
    out[6] = depth_ok(MAX_DEPTH) ? 1 : 0;
    out[7] = depth_ok(MAX_DEPTH + 1) ? 1 : 0;
}
}
