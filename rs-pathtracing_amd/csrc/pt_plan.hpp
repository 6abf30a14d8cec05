// pt_plan.hpp — the wavefront engine's frame plan: everything launch_render_wave (pt_wave.hip) decides before it
// touches the device, as plain integer arithmetic.  Tile groups, samples per chunk, chunk streams, the workspace
// layout and the chunk list.  Standard library only, so the host compiler builds it for tests/test_wave_plan.py.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "pt_dims.hpp"

namespace pt {
namespace plan {

// Chunks keep at least MIN_CHUNK_PATHS paths to fill the device (Tuning::wf_min_chunks).
constexpr uint32_t MIN_CHUNK_PATHS = 1u << 21;
// Device memory the workspace leaves free: Input::avail_bytes is what is free plus what the workspace holds now,
// less this.
constexpr size_t RESERVE_BYTES = (size_t)2 << 30;
// Input::avail_bytes when the device's free memory is unknown: the plan is not shrunk to fit.
constexpr size_t MEM_UNKNOWN = ~(size_t)0;
// The largest depth a renderer takes (PT_MAX_DEPTH in rs_pathtracing.h).  Every product below is in size_t, which
// must be 64 bits: at this depth a path's id stack alone is 16 KiB, a chunk of 2^28 paths 4 TiB (the fit then halves
// it), iters is 4098 and cnt_words 16400.
constexpr uint32_t MAX_DEPTH = 4096;
static_assert(sizeof(size_t) >= 8, "the region sizes are 64-bit products");
static_assert((uint64_t)MAX_DEPTH + 4 < (1u << 28), "iters and cnt_words fit an int");
static_assert(((uint64_t)1 << 32) * 24 * ((uint64_t)MAX_DEPTH + 1) < ((uint64_t)1 << 62), "cap * 24 * (depth + 1)");
// Frames deeper than this keep the attenuation-stack count outside the path's who word, whose 7 spare bits hold
// counts up to 64 only (pt_wave.hip pack_who): in the spare top level of the slot's id stack, ids[depth * cap + id]
// (R_IDS has depth + 1 levels and a path pushes at most depth ids).  No region changes size.
constexpr uint32_t PACKED_COUNT_DEPTH = 64;
constexpr bool deep(uint32_t depth) { return depth > PACKED_COUNT_DEPTH; }
// The depths the plan is made for.  plan_for plans a larger one as MAX_DEPTH, so that no quantity below wraps
// whatever a caller passes; launch_render_wave refuses such a frame before it plans.
constexpr bool depth_ok(uint32_t depth) { return depth <= MAX_DEPTH; }

// Path slots per chunk when Tuning::wf_paths is 0, by depth (deep frames: bigger chunks, fewer tails).
// (deep frames: 256M paths, two chunks of a 1080p x 256-spp frame in one step, ~120 GB per chunk stream at depth
// 50: one tail of late iterations instead of two, C2 depth 50 1237 -> 1251, profiles/r6/ab/r6aa_*; 128M until round 6)
constexpr uint32_t default_paths(uint32_t depth) { return depth > 16 ? 1u << 28 : 3u << 24; }

struct Input {
    uint32_t ntiles;          // this rank's tiles
    uint32_t s_begin, s_end;  // the launch's samples: the frame's, or a resumable frame's window of them
    uint32_t spp, depth;
    bool progressive;  // a progressive frame's band (FrameParams::stop set)
    bool textured;     // per-path attenuation values (the scene has non-solid textures)
    bool presel;       // march jobs pre-selected by the bounce kernel (WfView::jo)
    int64_t wf_paths;  // Tuning
    int wf_slots, wf_min_chunks;
    size_t avail_bytes;  // what the workspace may take, or MEM_UNKNOWN
};

// One slot's regions (a chunk in flight's path state), in workspace order.
enum Region : int { R_SET0, R_SET1, R_IDS, R_LEAF, R_LIST, R_MQ, R_STATUS, R_CP_BLK, R_CNT, R_ATT, R_JO, R_COUNT };

// The workspace: `slots` slots of slot_stride bytes, region r of slot k at k * slot_stride + off[r], then the
// running per-pixel sums the slots share.  Every region starts on a 256-byte boundary.
struct Layout {
    size_t off[R_COUNT];   // from the slot's base
    size_t size[R_COUNT];  // bytes in use; 0: the region is absent (R_ATT, R_JO)
    size_t slot_stride;
    size_t acc, acc_size;  // the shared sums, from the workspace's base
    size_t total;
};

struct Plan {
    uint32_t cap_want;  // path slots per chunk asked for, after the halving to fit
    uint32_t group_tiles, npix_max;  // tiles (pixels) of a tile group: only frames beyond cap_want pixels have several
    uint32_t ns;                     // samples per chunk, at most
    uint32_t cap, cap_tiles;         // path slots of a chunk; compaction tiles (status padded to them)
    int slots;                       // chunks in flight, one stream each
    int iters;                       // bounce launches per chunk
    size_t cnt_words;                // WfView::cnt
    size_t bytes;                    // the workspace (Layout::total)
    Layout lay;
};

struct Chunk {
    uint32_t g0, gt, s0, ns;  // tiles [g0, g0 + gt) of the rank's list, samples [s0, s0 + ns)
    int slot;
    uint32_t step;  // chunks of one step run side by side, one per slot
};

inline size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

// The chunk plan for cap_want path slots per chunk: tile groups, then sample chunks, the streams, and the workspace.
inline Plan plan_for(const Input &in, uint32_t cap_want) {
    Plan pl;
    const uint32_t ntiles = in.ntiles, nsw = in.s_end - in.s_begin;
    const uint32_t depth = depth_ok(in.depth) ? in.depth : MAX_DEPTH;
    pl.cap_want = cap_want;
    pl.iters = (int)depth + 2;  // traces per path <= depth + 1, then one last shade
    pl.cnt_words = (size_t)(pl.iters + 2) * 4;
    const uint32_t tiles_per_group = cap_want / (TILE * TILE) ? cap_want / (TILE * TILE) : 1;
    pl.group_tiles = ntiles < tiles_per_group ? ntiles : tiles_per_group;
    pl.npix_max = pl.group_tiles * TILE * TILE;
    uint32_t ns = cap_want / pl.npix_max;
    if (ns < 1) ns = 1;
    if (ns > nsw) ns = nsw;
    // A small frame (one rank's share of a multi-GPU frame) still gets at least wf_min_chunks sample
    // chunks, so the pipelined slots overlap one chunk's short tail iterations with the next chunk's work;
    // chunks keep at least MIN_CHUNK_PATHS paths to fill the device.  (A progressive frame's band gets at
    // least two: one per chunk stream; and any frame at least one per chunk stream while its chunks keep
    // MIN_CHUNK_PATHS paths, whatever wf_paths allows.)
    uint32_t mc = in.progressive && in.wf_min_chunks < 2 ? 2u : (uint32_t)in.wf_min_chunks;
    if (mc < (uint32_t)in.wf_slots) mc = (uint32_t)in.wf_slots;
    if (mc > 1 && ntiles <= pl.group_tiles) {
        uint32_t want = (nsw + mc - 1) / mc;
        const uint32_t floor_ns = (MIN_CHUNK_PATHS + pl.npix_max - 1) / pl.npix_max;
        if (want < floor_ns) want = floor_ns;
        if (want < ns) ns = want;
    }
    pl.ns = ns;
    pl.cap = ns * pl.npix_max;
    pl.cap_tiles = (pl.cap + CP_TILE - 1) / CP_TILE;
    // no more slots than chunks
    const uint64_t chunks = (uint64_t)((ntiles + pl.group_tiles - 1) / pl.group_tiles) * ((nsw + ns - 1) / ns);
    pl.slots = in.wf_slots;
    if ((uint64_t)pl.slots > chunks) pl.slots = (int)chunks;
    // a slot: two path-state sets, id stacks, 32-byte leaf records (end_path), live list and march queue,
    // statuses, the compaction's tile counts (CpLayout: 3 x per * 256 words), counters, textured attenuation
    // values, pre-selected march jobs
    const size_t cap = pl.cap, d1 = (size_t)depth + 1;
    const size_t need[R_COUNT] = {cap * PATH_BYTES,
                                  cap * PATH_BYTES,
                                  cap * 4 * d1,
                                  cap * 32,
                                  cap * 4,
                                  cap * 4,
                                  (size_t)pl.cap_tiles * CP_TILE,
                                  ((size_t)pl.cap_tiles + CP_BLOCK) * 12,
                                  pl.cnt_words * 4,
                                  in.textured ? cap * 24 * d1 : 0,
                                  in.presel ? cap * 64 : 0};
    Layout &L = pl.lay;
    size_t p = 0;
    for (int r = 0; r < R_COUNT; r++) {
        L.off[r] = need[r] ? p : 0;
        L.size[r] = need[r];
        p += align256(need[r]);
    }
    L.slot_stride = p;
    L.acc = p * (size_t)pl.slots;
    L.acc_size = (size_t)pl.npix_max * 24;
    L.total = L.acc + align256(L.acc_size) + 8192;
    pl.bytes = L.total;
    return pl;
}

// Path slots per chunk: Tuning::wf_paths, or by depth, halved until the plan fits the device memory the workspace
// may take: a deep textured frame's per-slot attenuation values ((depth + 1) * 24 B per path) would otherwise ask
// for more than the device has (1080p, 256 spp, depth 50 at 128M paths needed ~430 GB).
inline Plan make_plan(const Input &in) {
    uint32_t cap_want = in.wf_paths ? (uint32_t)in.wf_paths : default_paths(in.depth);
    Plan pl = plan_for(in, cap_want);
    while (pl.bytes > in.avail_bytes && cap_want > MIN_CHUNK_PATHS) {
        cap_want = cap_want / 2 > MIN_CHUNK_PATHS ? cap_want / 2 : MIN_CHUNK_PATHS;
        pl = plan_for(in, cap_want);
    }
    return pl;
}

// Whether the workspace of the plan fits what it may take (avail_bytes: the free memory less the reserve).
// make_plan stops halving at MIN_CHUNK_PATHS, and the plan it returns then may still be too large (a very deep
// textured frame: (depth + 1) * 28 B per path and slot).  The reserve is a margin for sizing chunks, not a limit: a
// plan that does not fit in this sense is still run when the device can hold it (fits_device).
inline bool fits(const Input &in, const Plan &pl) { return pl.bytes <= in.avail_bytes; }
// Whether the device can hold the plan's workspace at all.  hard_bytes: what is free plus what the workspace holds
// now, nothing kept back (or MEM_UNKNOWN); a workspace that already covers the plan always can.
inline bool fits_device(const Plan &pl, size_t hard_bytes) { return pl.bytes <= hard_bytes; }

// The plan launch_render_wave runs: make_plan's, whenever the device can hold it (so every frame that could be
// allocated before is planned as before, the small frame on a nearly full device included).  Only when it cannot,
// the plan is made once more for a single chunk stream (half the workspace); when fits_device still says no, the
// caller refuses the frame.  *in is left as the plan was made from (chunk_list takes the same).
inline Plan make_plan_fit(Input *in, size_t hard_bytes) {
    Plan pl = make_plan(*in);
    if (!fits_device(pl, hard_bytes) && in->wf_slots > 1) {
        in->wf_slots = 1;
        pl = make_plan(*in);
    }
    return pl;
}

// Sample chunks of a tile group: as few as fit ns samples each, rounded up to whole rounds of `slots` (no round
// with an idle stream), with the samples spread evenly over them (no short last chunk).  The per-pixel sums take
// the chunks in sample order either way.  Chunk c of a group runs in slot c % slots; a group's steps follow the
// previous group's.
inline std::vector<Chunk> chunk_list(const Input &in, const Plan &pl) {
    const uint32_t nsw = in.s_end - in.s_begin, S = (uint32_t)pl.slots;
    uint32_t nchunks = (nsw + pl.ns - 1) / pl.ns;
    if (S > 1 && nchunks > 1 && nchunks % S) nchunks += S - nchunks % S;
    if (nchunks > nsw) nchunks = nsw;
    std::vector<Chunk> list;
    uint32_t step0 = 0;
    for (uint32_t g0 = 0; g0 < in.ntiles; g0 += pl.group_tiles) {
        const uint32_t gt = in.ntiles - g0 < pl.group_tiles ? in.ntiles - g0 : pl.group_tiles;
        uint32_t s0 = in.s_begin;
        for (uint32_t c = 0; c < nchunks; c++) {
            // <= ceil(nsw / nchunks) <= ns samples
            const uint32_t s1 = in.s_begin + (uint32_t)((uint64_t)nsw * (c + 1) / nchunks);
            list.push_back(Chunk{g0, gt, s0, s1 - s0, (int)(c % S), step0 + c / S});
            s0 = s1;
        }
        step0 += (nchunks + S - 1) / S;
    }
    return list;
}

}  // namespace plan
}  // namespace pt
