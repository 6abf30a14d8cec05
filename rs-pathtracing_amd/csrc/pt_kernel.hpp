// pt_kernel.hpp — host-side launchers of the HIP kernels (pt_kernel.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/rs_pathtracing.h"
#include "pt_builds.hpp"  // Tuning, tuning_set / tuning_get, the choice of kernel builds
#include "pt_cull.hpp"
#include "pt_types.hpp"

namespace pt {

// One device's scene: the kernels' view of its buffers (dev::Scene, filled by view_set_scene / view_set_accel,
// pt_accel.hpp; this owns the buffers, view_buffers), and what the choice of builds needs beside it.
struct DeviceScene {
    dev::Scene view = {};
    int nshapes = 0;
    int fkind = 0;  // scene_builds(): 0: every marched shape is a Heart (or none) -> Heart-only kernel builds; -1: any
    // counts the acceleration structures this device has been given (commit_accel): what was derived from one
    // (WaveWorkspace::first_cull) is stale once it moves, even if a later structure's buffers reuse its addresses
    uint64_t accel_gen = 0;
};

// Per-kernel launch timing (pt_kernel_timing): HIP events recorded on the
// launch stream around every render-path kernel while enabled.
// (kind 5 was the wavefront tail kernel until round 6; it now times the per-slot unwind, wf_unwind)
enum KernelKind : int { K_BOUNCE = 0, K_MARCH = 1, K_SELECT = 2, K_REDUCE = 3, K_MEGA = 4, K_UNWIND = 5, K_WALK = 6, K_KINDS = 7 };
struct KernelTimer;
KernelTimer *timer_new();
void timer_free(KernelTimer *t);
hipError_t timer_begin(KernelTimer *t, hipStream_t st, int kind);  // no-op when t is null
hipError_t timer_end(KernelTimer *t, hipStream_t st);
hipError_t timer_collect(KernelTimer *t, double *ms, uint32_t *launches);  // sums since last collect

// Diagnostic builds of the wavefront kernels (pt_wave_diag: wave-level s_memtime per bounce section and march
// phase): make EXTRA=-DPT_WAVE_DIAG=1.  In the product build the instrumentation is compiled out of every
// kernel (it is no template parameter of the hot kernels) and pt_wave_diag refuses to enable it.
#ifndef PT_WAVE_DIAG
#define PT_WAVE_DIAG 0
#endif

// Device workspace of the wavefront engine (pt_wave.hip), grown on demand and
// reused by every frame of a renderer.
struct WaveWorkspace {
    Tuning tune;  // this renderer's knobs (both engines read them from here)
    void *base = nullptr;
    size_t bytes = 0;
    unsigned long long *diag = nullptr;  // march-kernel phase diagnostics (pt_wave_diag), when enabled
    KernelTimer *timer = nullptr;         // per-kernel timing (pt_kernel_timing), when enabled
    // chunk pipeline: extra launch streams (chunk c runs on stream c % slots,
    // stream 0 being the caller's) and the events that order them
    static constexpr int MAX_SLOTS = WF_MAX_SLOTS;
    hipStream_t side[MAX_SLOTS - 1] = {};
    hipEvent_t fork = nullptr, join[MAX_SLOTS - 1] = {}, reduced = nullptr;
    // recorded on the launch stream after a frame's last use of the workspace;
    // the next frame (on any stream) waits for it
    hipEvent_t done = nullptr;
    bool used = false;
    // the launches' argument blocks of the last frame (pt_wave.hip WfArgs): pinned staging and device copy;
    // args_ev is recorded after the frame's copy (the staging buffer is free once it has run)
    void *args_host = nullptr, *args_dev = nullptr;
    size_t args_bytes = 0;
    hipEvent_t args_ev = nullptr;
    bool args_pending = false;
    int device = -1;
    // why launch_render refused the last frame without a HIP failure (empty: it did not): a frame whose workspace
    // the device cannot hold (pt_wave.hip launch_render_wave)
    char refusal[320] = {};
    // the engine and the kernel builds the last launch_render call launched (pt_renderer_get_option "ran_*")
    builds::Ran ran;
    // The first bounce launch's cull table (pt_cull.hpp): one mask per 8x8 pixel block of the frame, filled on the
    // frame's stream before its chunks fork (pt_wave.hip first_cull_table) and kept for the frames after it: it is
    // remade only when the caster part of FrameParams, the frame's size or the device's acceleration data change.
    struct FirstCull {
        uint64_t *table = nullptr;
        size_t cap = 0;      // masks the buffer holds
        size_t blocks = 0;   // masks of the table in it
        bool valid = false;  // the table is the one of (key, accel_gen, boxes)
        cull::CasterKey key = {};
        uint64_t accel_gen = 0;  // DeviceScene::accel_gen, and the buffer the boxes were read from
        const void *boxes = nullptr;
        bool used = false;  // the last launch_render call's frame read the table ("first_cull_bits")
    } first_cull;
};
void wave_workspace_free(WaveWorkspace *ws);
// The set bits over the cull table that the last launch_render call's frame read, once that frame is done; -1: it
// read none (the megakernel, a SPLIT build's frame, a scene with nothing to cull).
hipError_t first_cull_bits(const WaveWorkspace &ws, int64_t *bits);

// Renders this rank's tiles of P into out with the engine and the kernel builds that builds::choose picks
// (pt_builds.hpp).  An error with ws.refusal set is a refusal, not a HIP failure.
// tiles (a host array of P.tile_count entries that passes tile_list_ok, with P.tile_begin 0; null: none): a listed
// launch, which renders entries tiles[0..tile_count) of the rank's tile list and touches no other tile (DESIGN.md
// §3.11).  It always runs the wavefront engine; the list is copied before the call returns.
hipError_t launch_render(const DeviceScene &s, const FrameParams &P, double *out, hipStream_t st, WaveWorkspace &ws,
                         const uint32_t *tiles = nullptr);
// rows [y0, y1) of the frame from gathered shards (pt_unshard_device)
hipError_t launch_unshard(const double *gathered, uint32_t width, uint32_t height, uint32_t world, double *frame,
                          hipStream_t st, uint32_t y0 = 0, uint32_t y1 = ~0u);
// display encode of pixels [p0, p1) (pt_encode_rgba8_device); rgba is 4-byte aligned
hipError_t launch_encode_rgba8(const double *rgb, size_t p0, size_t p1, uint8_t *rgba, hipStream_t st);
hipError_t launch_closest_hit(const DeviceScene &s, const double *rays, size_t n, double min_t, double max_t,
                              pt_hit *out, hipStream_t st);
hipError_t launch_ray_color(const DeviceScene &s, const double *rays, uint64_t *states, size_t n, uint32_t depth,
                            double s11, double *out, hipStream_t st);
hipError_t launch_trace_pixels(const DeviceScene &s, const FrameParams &P, const uint32_t *pixels, size_t n,
                               double *out, hipStream_t st);

hipError_t launch_count_work(const DeviceScene &s, const FrameParams &P, const uint32_t *pixels, size_t n,
                             unsigned long long *ctr, hipStream_t st);

hipError_t launch_march_probe(const double *jobs, size_t n, double *t, int32_t *status, uint32_t *iters,
                              hipStream_t st);
hipError_t launch_render_timed(const DeviceScene &s, const FrameParams &P, double *out, unsigned long long *acc,
                               hipStream_t st);

}  // namespace pt
