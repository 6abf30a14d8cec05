// pt_api.cpp — the C-ABI (include/rs_pathtracing.h).  No exception escapes:
// each entry point catches, stores a thread-local message and returns a
// status.  The renderer owns one HIP stream on its device; start_rendering
// queues the frame as bands of tile rows, each closed by an event, so a
// non-blocking render_step can hand back finished bands while the rest of the
// frame is still on the GPU (src/renderer/step_by_step.rs:101-121).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <new>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/rs_pathtracing.h"
#include "pt_accel.hpp"
#include "pt_adaptive.hpp"
#include "pt_aov.hpp"
#include "pt_denoise.hpp"
#include "pt_kernel.hpp"
#include "pt_plan.hpp"
#include "pt_scene.hpp"
#include "pt_temporal.hpp"
#include "pt_tiles.hpp"
#include "pt_variance.hpp"

using namespace pt;

namespace {
thread_local std::string g_err;

int fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}
int hip_fail(hipError_t e, const char *what) {
    return fail(PT_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}
#define HIP_TRY(expr)                                  \
    do {                                               \
        hipError_t e_ = (expr);                        \
        if (e_ != hipSuccess) return hip_fail(e_, #expr); \
    } while (0)

static_assert(PT_MAX_DEPTH == plan::MAX_DEPTH, "the header states the plan's depth limit");
// the depth limit of the create calls and pt_ray_color
int depth_refused(uint32_t depth) {
    if (depth <= PT_MAX_DEPTH) return PT_OK;
    return fail(PT_ERR_UNSUPPORTED, "depth " + std::to_string(depth) + " is above the largest supported depth, " +
                                        std::to_string(PT_MAX_DEPTH) + " (PT_MAX_DEPTH)");
}
// the calls that run the register id stacks only (64 ids)
int reg_depth_refused(uint32_t depth, const char *call) {
    if (depth <= MAX_REG_DEPTH) return PT_OK;
    return fail(PT_ERR_UNSUPPORTED, std::string(call) + " supports depth <= " + std::to_string(MAX_REG_DEPTH) +
                                        " (the renderer's depth is " +
                                        std::to_string(depth) + "); frames and pt_ray_color take any depth up to " +
                                        std::to_string(PT_MAX_DEPTH));
}

// the smallest band of a progressive frame, in samples (enough paths to fill the device)
constexpr uint64_t BAND_MIN_SAMPLES = (uint64_t)1 << 24;

}  // namespace

namespace {
// A device buffer for the length of a call: the host forms and the probes stage their arrays in these.
template <class T>
struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    ~DevBuf() { (void)hipFree(p); }
    hipError_t alloc(size_t count) {
        n = count;
        return hipMalloc(&p, (n ? n : 1) * sizeof(T));
    }
    // alloc, and the host array copied in; an optional array that is not given (null) gets no buffer: p stays null
    hipError_t upload(const T *host, size_t count) {
        if (!host) return hipSuccess;
        const hipError_t e = alloc(count);
        return e != hipSuccess ? e : hipMemcpy(p, host, n * sizeof(T), hipMemcpyHostToDevice);
    }
    // the buffer copied out to the host array it was staged for (none: nothing to copy)
    hipError_t download(T *host) const {
        return host ? hipMemcpy(host, p, n * sizeof(T), hipMemcpyDeviceToHost) : hipSuccess;
    }
};

// The refusals that recur: each message stands here once, and an entry point calls them in its own order.
int refuse_if(bool bad, const char *msg) { return bad ? fail(PT_ERR_INVALID, msg) : PT_OK; }
int frame_refused(uint32_t w, uint32_t h) { return refuse_if(w == 0 || h == 0, "width and height must be > 0"); }
int frame_refused(uint32_t w, uint32_t h, uint32_t spp) {
    return refuse_if(w == 0 || h == 0 || spp == 0, "width, height and samples_number must be > 0");
}
int rank_refused(uint32_t rank, uint32_t world) { return refuse_if(world == 0 || rank >= world, "rank must be < world"); }
int sample_window_refused(uint32_t s_begin, uint32_t s_end, uint32_t spp) {
    return refuse_if(s_begin >= s_end || s_end > spp,
                     "sample window must satisfy 0 <= s_begin < s_end <= samples_number");
}
int windows_refused(uint32_t windows, uint32_t spp) {
    return refuse_if(windows < 2 || windows > spp, "windows must be 2..samples_number");
}
int sigmas_refused(double sigma_normal, double sigma_depth) {
    return refuse_if(!(sigma_normal > 0.0) || !(sigma_depth > 0.0), "sigma_normal and sigma_depth must be > 0");
}
int workspace_refused(const void *d_work) {
    if (!d_work) return fail(PT_ERR_INVALID, "null argument");
    return refuse_if(((uintptr_t)d_work & 15u) != 0, "the workspace must be 16-byte aligned");
}
}  // namespace

struct pt_scene {
    Scene s;
};

// One device of a renderer: its own copy of the scene, wavefront workspace
// and stream.  A single-device renderer has one; a multi-device
// renderer (pt_renderer_create_multi) deals the frame's tiles to several,
// rank g = gpus[g], and gathers the shards on gpus[0].
struct GpuShare {
    int device = 0;
    hipStream_t stream = nullptr;
    DeviceScene ds;
    WaveWorkspace ws;
    double *d_shard = nullptr;  // compact tile shard of a multi-device frame (ranks >= 1)
    size_t shard_cap = 0;
    hipEvent_t shard_ev = nullptr;  // a band's shard copy to gpus[0] is done
};

struct pt_renderer {
    pt_scene *scene = nullptr;
    uint32_t depth = 0;
    double s11 = 0;
    std::vector<GpuShare> gpus;  // gpus[0] holds the frame

    // frame in flight (render_start .. render_step)
    bool started = false;
    uint32_t width = 0, height = 0;
    double *d_frame = nullptr;  // w*h*3 on gpus[0]
    size_t frame_cap = 0;
    uint8_t *d_rgba = nullptr;  // w*h*4 display encode of d_frame, on gpus[0]
    size_t rgba_cap = 0;
    double *d_gather = nullptr;  // multi-device: world shards back to back, on gpus[0]
    size_t gather_cap = 0;
    int peer_pairs = 0, peer_enabled = 0;  // distinct (gpus[0], gpus[k]) device pairs; with peer access both ways
    int fault_accel_alloc = 0;  // test hook (option "fault_accel_alloc"): this renderer's next BVH rebuild fails
    // A progressive frame is a list of bands of tile rows.  A feeder thread
    // queues them on the device(s), keeping two bands ahead of the GPU (one
    // running, one queued), so the device never idles between bands and
    // stop_rendering only has to drain at most two of them.
    struct Band {
        uint32_t t0, t1;      // tile rows
        uint32_t row0, row1;  // pixel rows
        hipEvent_t ev;        // recorded on gpus[0].stream once the band is queued
        bool copied;
    };
    std::vector<Band> bands;
    FrameParams frame{};
    std::thread feeder;
    std::atomic<bool> stop_req{false};
    std::atomic<uint32_t> bands_queued{0};  // bands [0, n) are queued (their events recorded)
    std::atomic<int> feed_rc{0};            // the feeder's failure status (feed_err holds the message)
    std::string feed_err;
    // The progressive frame's stop flag (FrameParams::stop), host-mapped and
    // coherent so the kernels see pt_render_stop's store at once: while it is
    // set, a queued launch of the frame does no work, so the stop returns
    // after the launches already running instead of two whole bands.  Frames
    // queued by pt_render_device / pt_render_frame_device carry no flag.
    int *h_stop = nullptr;
    const int *d_stop = nullptr;

    int device() const { return gpus[0].device; }
    hipStream_t stream() const { return gpus[0].stream; }
};

static int in_flight_refused(const pt_renderer *r) {
    if (r->started) return fail(PT_ERR_STATE, "a progressive frame is in flight (render_step it to the end or stop it)");
    return PT_OK;
}

extern "C" {

const char *pt_last_error(void) { return g_err.c_str(); }
__attribute__((visibility("hidden"))) void pt_set_last_error(const char *msg) { g_err = msg ? msg : ""; }  // for pt_image.cpp
#ifndef PT_SRC_SHA
#define PT_SRC_SHA "unknown"
#endif
const char *pt_version(void) {
    return "rs-pathtracing-amd 0.4.3 (gfx950, f64 megakernel + wavefront march engine; src " PT_SRC_SHA ")";
}
uint32_t pt_abi_version(void) { return PT_ABI_VERSION; }

int pt_abi_layout(int which, uint32_t *out, size_t n) {
    std::vector<size_t> v;
#define PT_F(T, f) v.push_back(offsetof(T, f))
    switch (which) {
    case PT_ABI_SCENE_OPTS:
        v.push_back(sizeof(pt_scene_opts));
        PT_F(pt_scene_opts, random_spheres), PT_F(pt_scene_opts, struct_size), PT_F(pt_scene_opts, seed);
        PT_F(pt_scene_opts, load_image), PT_F(pt_scene_opts, image_user);
        break;
    case PT_ABI_CAMERA:
        v.push_back(sizeof(pt_camera));
        PT_F(pt_camera, position), PT_F(pt_camera, direction), PT_F(pt_camera, up), PT_F(pt_camera, right);
        PT_F(pt_camera, fov), PT_F(pt_camera, focal_length);
        break;
    case PT_ABI_SHAPE_INFO:
        v.push_back(sizeof(pt_shape_info));
        PT_F(pt_shape_info, type), PT_F(pt_shape_info, material), PT_F(pt_shape_info, inverse_normal);
        PT_F(pt_shape_info, depth), PT_F(pt_shape_info, func), PT_F(pt_shape_info, pad0);
        PT_F(pt_shape_info, direct), PT_F(pt_shape_info, inverse);
        PT_F(pt_shape_info, x0), PT_F(pt_shape_info, y0), PT_F(pt_shape_info, x1), PT_F(pt_shape_info, y1);
        PT_F(pt_shape_info, step), PT_F(pt_shape_info, a), PT_F(pt_shape_info, b), PT_F(pt_shape_info, c);
        PT_F(pt_shape_info, d), PT_F(pt_shape_info, sphere_radius), PT_F(pt_shape_info, radius);
        PT_F(pt_shape_info, tube_radius);
        break;
    case PT_ABI_MATERIAL_INFO:
        v.push_back(sizeof(pt_material_info));
        PT_F(pt_material_info, type), PT_F(pt_material_info, texture), PT_F(pt_material_info, albedo);
        PT_F(pt_material_info, fuzz), PT_F(pt_material_info, ior), PT_F(pt_material_info, emit);
        break;
    case PT_ABI_HIT:
        v.push_back(sizeof(pt_hit));
        PT_F(pt_hit, t), PT_F(pt_hit, point), PT_F(pt_hit, normal), PT_F(pt_hit, front_face);
        PT_F(pt_hit, shape), PT_F(pt_hit, material), PT_F(pt_hit, pad0);
        break;
    case PT_ABI_CHECKPOINT:
        v.push_back(sizeof(pt_checkpoint));
        PT_F(pt_checkpoint, width), PT_F(pt_checkpoint, height), PT_F(pt_checkpoint, samples_number);
        PT_F(pt_checkpoint, samples_done), PT_F(pt_checkpoint, rank), PT_F(pt_checkpoint, world);
        PT_F(pt_checkpoint, depth), PT_F(pt_checkpoint, reserved), PT_F(pt_checkpoint, seed);
        PT_F(pt_checkpoint, scene_key), PT_F(pt_checkpoint, count);
        break;
    default:
        return fail(PT_ERR_INVALID, "pt_abi_layout: unknown struct " + std::to_string(which));
    }
#undef PT_F
    if (n && !out) return fail(PT_ERR_INVALID, "null argument");
    for (size_t k = 0; k < n && k < v.size(); k++) out[k] = (uint32_t)v[k];
    return (int)v.size();
}

uint64_t pt_sample_key(uint64_t seed, uint64_t pixel, uint64_t sample) { return sample_key(seed, pixel, sample); }

int pt_scene_create_from_json(const char *json, size_t len, const pt_scene_opts *opts, pt_scene **out) {
    if (!json || !out) return fail(PT_ERR_INVALID, "null argument");
    *out = nullptr;
    // struct_size versions the options (header): no byte at or past
    // opts + struct_size is read; 0 is a 0.1.0 (16-byte struct) or 0.2.0
    // (32-byte) caller with `reserved` = 0 in this field, which 0 cannot tell
    // apart, so only the 16 bytes both have are read (no image loader)
    const size_t osz = !opts ? 0 : (opts->struct_size ? opts->struct_size : (size_t)PT_SCENE_OPTS_LEGACY_SIZE);
    if (opts && osz < PT_SCENE_OPTS_MIN_SIZE)
        return fail(PT_ERR_INVALID, "pt_scene_opts.struct_size " + std::to_string(osz) +
                                        " is below the 16 bytes of {random_spheres, struct_size, seed}");
    bool rs = opts ? opts->random_spheres != 0 : true;
    uint64_t seed = opts ? opts->seed : 1;
    ImageSource img;
    if (opts && osz >= offsetof(pt_scene_opts, load_image) + sizeof(opts->load_image)) img.load = opts->load_image;
    if (opts && osz >= offsetof(pt_scene_opts, image_user) + sizeof(opts->image_user)) img.user = opts->image_user;
    try {
        pt_scene *s = new pt_scene;
        try {
            s->s = scene_from_json(json, len, rs, seed, img);
        } catch (...) {
            delete s;
            throw;
        }
        *out = s;
        return PT_OK;
    } catch (const SceneError &e) {
        return fail(e.code, e.msg);
    } catch (const std::bad_alloc &) {
        return fail(PT_ERR_INVALID, "out of memory");
    } catch (const std::exception &e) {
        return fail(PT_ERR_INVALID, e.what());
    }
}

void pt_scene_destroy(pt_scene *s) { delete s; }

int pt_scene_camera(const pt_scene *s, pt_camera *out) {
    if (!s || !out) return fail(PT_ERR_INVALID, "null argument");
    *out = s->s.camera;
    return PT_OK;
}
int pt_scene_num_shapes(const pt_scene *s) { return s ? (int)s->s.shapes.size() : fail(PT_ERR_INVALID, "null scene"); }
int pt_scene_num_materials(const pt_scene *s) {
    return s ? (int)s->s.materials.size() : fail(PT_ERR_INVALID, "null scene");
}
int pt_scene_get_shape(const pt_scene *s, int i, pt_shape_info *o) {
    if (!s || !o || i < 0 || i >= (int)s->s.shapes.size()) return fail(PT_ERR_INVALID, "shape index out of range");
    const HostShape &h = s->s.shapes[i];
    std::memset(o, 0, sizeof *o);
    o->type = h.type;
    o->material = h.material;
    o->inverse_normal = h.inverse_normal;
    o->depth = h.depth;
    o->func = h.func;
    std::memcpy(o->direct, h.direct, sizeof o->direct);
    std::memcpy(o->inverse, h.inverse, sizeof o->inverse);
    o->x0 = h.x0;
    o->y0 = h.y0;
    o->x1 = h.x1;
    o->y1 = h.y1;
    o->step = h.step;
    o->a = h.fa;
    o->b = h.fb;
    o->c = h.fc;
    o->d = h.fd;
    o->sphere_radius = h.fr;
    o->radius = h.radius;
    o->tube_radius = h.tube_radius;
    return PT_OK;
}
int pt_scene_get_material(const pt_scene *s, int i, pt_material_info *o) {
    if (!s || !o || i < 0 || i >= (int)s->s.materials.size())
        return fail(PT_ERR_INVALID, "material index out of range");
    const HostMaterial &m = s->s.materials[i];
    std::memset(o, 0, sizeof *o);
    o->type = m.type;
    o->texture = m.tex;
    for (int k = 0; k < 3; k++) {
        o->albedo[k] = m.albedo[k];
        o->emit[k] = m.emit[k];
    }
    o->fuzz = m.fuzz;
    o->ior = m.ior;
    return PT_OK;
}

int pt_camera_new(const double position[3], const double direction[3], const double up[3], double focal_length,
                  double fov_radians, pt_camera *out) {
    if (!position || !direction || !up || !out) return fail(PT_ERR_INVALID, "null argument");
    camera_new(position, direction, up, focal_length, fov_radians, out);
    return PT_OK;
}

// ------------------------------------------------------------- renderer
}  // extern "C"

namespace {

void free_buffers(const dev::Scene &v, size_t count) {
    const auto bufs = view_buffers(v);
    for (size_t k = 0; k < count; k++)
        if (bufs[k]) (void)hipFree(const_cast<void *>(bufs[k]));
}

void free_share(GpuShare &g) {
    (void)hipSetDevice(g.device);
    if (g.stream) (void)hipStreamSynchronize(g.stream);
    free_buffers(g.ds.view, view_buffers(g.ds.view).size());
    g.ds = DeviceScene{};
    if (g.d_shard) (void)hipFree(g.d_shard);
    g.d_shard = nullptr;
    g.shard_cap = 0;
    wave_workspace_free(&g.ws);
    if (g.shard_ev) (void)hipEventDestroy(g.shard_ev);
    g.shard_ev = nullptr;
    if (g.stream) (void)hipStreamDestroy(g.stream);
    g.stream = nullptr;
}

// The acceleration structure on one device: octant-threaded BVH nodes, leaf
// shape ids, the wave-uniform and marched lists and the padded boxes.  A new
// structure is first staged in buffers of its own (stage_accel); only when
// every device has staged it are the old buffers swapped out and freed
// (commit_accel), so a failed upload leaves every device on its old, complete
// structure.  A staged structure is a view with only its acceleration part set.
using StagedAccel = dev::Scene;

void free_staged(int device, StagedAccel &a) {
    (void)hipSetDevice(device);
    free_buffers(a, VIEW_ACCEL_BUFS);
    a = StagedAccel{};
}

// A host vector in a device buffer of its own (one element's room for an empty vector), unless an earlier step
// failed (err): the buffer, also when the copy into it failed, for the caller to free.
// Test hook (renderer option "fault_accel_alloc" = n, kept per renderer): the
// n-th device allocation of that renderer's next BVH rebuild fails as if the
// device were out of memory.  `fault` is the renderer's counter (null when
// creating a renderer: no hook).
template <class T>
const T *upload(hipError_t &err, const std::vector<T> &vec, int *fault = nullptr) {
    T *d = nullptr;
    if (err == hipSuccess && fault && *fault > 0 && (*fault)-- == 1) err = hipErrorOutOfMemory;
    if (err == hipSuccess) err = hipMalloc((void **)&d, (vec.empty() ? 1 : vec.size()) * sizeof(T));
    if (err == hipSuccess && !vec.empty())
        err = hipMemcpy(d, vec.data(), vec.size() * sizeof(T), hipMemcpyHostToDevice);
    return d;
}

int stage_accel(int device, const Accel &acc, StagedAccel *out, int *fault = nullptr) {
    const std::vector<DQGrid> qbuf = pack_qnodes(acc);
    hipError_t err = hipSetDevice(device);
    // (the allocations in this order, the quantized buffer last when there is one: the test hook counts them)
    const DNodeC *nodes = upload(err, acc.cnodes, fault);
    const int32_t *leaf = upload(err, acc.leaf, fault);
    const int32_t *lin = upload(err, acc.lin, fault);
    const int32_t *march = upload(err, acc.march, fault);
    const DBox *boxes = upload(err, acc.boxes, fault);
    const DQGrid *qnodes = qbuf.empty() ? nullptr : upload(err, qbuf, fault);
    StagedAccel a{};
    view_set_accel(a, acc, nodes, qnodes, leaf, lin, march, boxes);
    if (err != hipSuccess) {
        free_staged(device, a);
        return hip_fail(err, "uploading the acceleration structure");
    }
    *out = a;
    return PT_OK;
}

// Swaps a staged structure in; the old one is freed once the device's queued
// work (which may still read it) is done.
int commit_accel(GpuShare &g, StagedAccel &a) {
    HIP_TRY(hipSetDevice(g.device));
    HIP_TRY(hipDeviceSynchronize());
    StagedAccel old = g.ds.view;
    view_set_accel(g.ds.view, a);
    g.ds.accel_gen++;  // (what the workspace derived from the old structure is stale: its first-bounce cull table)
    a = StagedAccel{};
    free_staged(g.device, old);
    return PT_OK;
}

// Uploads the realized scene to one device and creates its stream.
int init_share(GpuShare &g, int device, const Scene &S, const Accel &acc, const std::vector<DShape> &hs,
               const std::vector<DMaterial> &hm) {
    g.device = device;
    HIP_TRY(hipSetDevice(device));
    hipError_t err = hipStreamCreateWithFlags(&g.stream, hipStreamNonBlocking);
    const DShape *shapes = upload(err, hs);
    const DMaterial *mats = upload(err, hm);
    const bool tex = !S.textures.empty();
    const DTexture *textures = tex ? upload(err, S.textures) : nullptr;
    const DPerlin *perlins = tex ? upload(err, S.perlins) : nullptr;
    const DImage *images = tex ? upload(err, S.images) : nullptr;
    const uint8_t *pixels = tex ? upload(err, S.pixels) : nullptr;
    view_set_scene(g.ds.view, S, shapes, mats, textures, perlins, images, pixels);
    if (err == hipSuccess) err = hipEventCreateWithFlags(&g.shard_ev, hipEventDisableTiming);
    // device counters: [0] march guard drops, [1] stop-gated launches that found the frame stopped, [2] of those,
    // launches that still had work (pt_render_stop_stats)
    if (err == hipSuccess) err = hipMalloc((void **)&g.ds.view.guard, 4 * sizeof(unsigned long long));
    if (err == hipSuccess) err = hipMemset(g.ds.view.guard, 0, 4 * sizeof(unsigned long long));
    if (err != hipSuccess) return hip_fail(err, "uploading the scene");
    StagedAccel a{};
    if (int rc = stage_accel(device, acc, &a)) return rc;
    if (int rc = commit_accel(g, a)) return rc;
    g.ws.tune = tuning_defaults();
    g.ds.view.diag = g.ws.tune.diag;
    g.ds.nshapes = (int)hs.size();
    g.ds.fkind = scene_builds(S).fkind;
    return PT_OK;
}

void release_bands(pt_renderer *r) {
    for (auto &b : r->bands) (void)hipEventDestroy(b.ev);
    r->bands.clear();
}

int sync_all(pt_renderer *r) {
    for (auto &g : r->gpus) {
        HIP_TRY(hipSetDevice(g.device));
        HIP_TRY(hipStreamSynchronize(g.stream));
    }
    return PT_OK;
}

FrameParams frame_params(const pt_renderer *r, const pt_camera &cam, uint32_t w, uint32_t h, uint32_t spp,
                         uint64_t seed) {
    FrameParams P = pt::frame_params(cam, w, h, spp, r->depth, seed, r->s11);
    P.rank = 0;
    P.world = 1;
    P.tiles_x = tiles_across(w);
    return P;
}

// The FrameParams of one rank's whole shard (world > 1: in the compact layout).
FrameParams shard_params(const pt_renderer *r, const pt_camera &cam, uint32_t w, uint32_t h, uint32_t spp,
                         uint64_t seed, uint32_t rank, uint32_t world) {
    FrameParams P = frame_params(r, cam, w, h, spp, seed);
    P.rank = rank;
    P.world = world;
    P.compact = world > 1 ? 1 : 0;
    P.tile_begin = 0;
    P.tile_count = shard_tiles(w, h, rank, world);
    return P;
}

// The part [*i0, *i1) of rank's tile list whose logical tiles lie in [a, b):
// logical tile k belongs to rank k % world at list index k / world.
void rank_range(uint32_t a, uint32_t b, uint32_t rank, uint32_t world, uint32_t *i0, uint32_t *i1) {
    *i0 = a > rank ? (a - rank + world - 1) / world : 0;
    *i1 = b > rank ? (b - rank + world - 1) / world : 0;
}

// launch_render on g's device: a refusal (WaveWorkspace::refusal: a deep frame whose workspace does not fit) is
// PT_ERR_UNSUPPORTED with its message, anything else a HIP failure.
// tiles: a listed launch (launch_render).
int render_on(GpuShare &g, const FrameParams &P, double *dst, hipStream_t st, const uint32_t *tiles = nullptr) {
    const hipError_t e = launch_render(g.ds, P, dst, st, g.ws, tiles);
    if (e == hipSuccess) return PT_OK;
    if (g.ws.refusal[0]) return fail(PT_ERR_UNSUPPORTED, g.ws.refusal);
    return hip_fail(e, "launch_render");
}

template <class T>
int grow(T **p, size_t *cap, size_t n) {
    const size_t bytes = n * sizeof(T);
    if (bytes <= *cap) return PT_OK;
    if (*p) HIP_TRY(hipFree(*p));
    *p = nullptr;
    *cap = 0;
    HIP_TRY(hipMalloc((void **)p, bytes));
    *cap = bytes;
    return PT_OK;
}

// Buffers of a frame on the renderer's devices (world > 1: the shards and the
// gather buffer), and the fork: the other devices' streams start after
// everything queued so far on gpus[0]'s stream.
int frame_prologue(pt_renderer *r, uint32_t w, uint32_t h) {
    const uint32_t world = (uint32_t)r->gpus.size();
    if (world == 1) return PT_OK;
    GpuShare &g0 = r->gpus[0];
    const size_t per = shard_tiles(w, h, 0, world);
    HIP_TRY(hipSetDevice(g0.device));
    if (int rc = grow(&r->d_gather, &r->gather_cap, (size_t)world * per * TILE * TILE * 3)) return rc;
    HIP_TRY(hipEventRecord(g0.shard_ev, g0.stream));
    for (uint32_t k = 1; k < world; k++) {
        GpuShare &g = r->gpus[k];
        HIP_TRY(hipSetDevice(g.device));
        if (int rc = grow(&g.d_shard, &g.shard_cap, per * TILE * TILE * 3)) return rc;
        HIP_TRY(hipStreamWaitEvent(g.stream, g0.shard_ev, 0));
    }
    return PT_OK;
}

// Queues tile rows [t0, t1) of the frame: every device renders its tiles of
// the band (world > 1: into its compact shard, then copied to gpus[0] over
// the peer link), gpus[0] un-interleaves the band into d_frame, encodes it
// into d_rgba (if given) and records `ev` (if given).
int enqueue_band(pt_renderer *r, const FrameParams &P0, double *d_frame, uint8_t *d_rgba, uint32_t t0, uint32_t t1,
                 hipEvent_t ev) {
    const uint32_t world = (uint32_t)r->gpus.size();
    const uint32_t w = P0.width, h = P0.height, tx = P0.tiles_x;
    GpuShare &g0 = r->gpus[0];
    const size_t per = shard_tiles(w, h, 0, world);
    const uint32_t row0 = t0 * TILE, row1 = t1 * TILE < h ? t1 * TILE : h;
    for (uint32_t k = 0; k < world; k++) {
        GpuShare &g = r->gpus[k];
        HIP_TRY(hipSetDevice(g.device));
        FrameParams P = P0;
        P.rank = k;
        P.world = world;
        P.compact = world > 1 ? 1 : 0;
        uint32_t i0, i1;
        rank_range(t0 * tx, t1 * tx, k, world, &i0, &i1);
        P.tile_begin = i0;
        P.tile_count = i1 - i0;
        double *dst = world == 1 ? d_frame : (k == 0 ? r->d_gather : g.d_shard);
        if (int rc = render_on(g, P, dst, g.stream)) return rc;
        if (k > 0) {
            if (i1 > i0) {
                const size_t off = (size_t)i0 * TILE * TILE * 3, n = (size_t)(i1 - i0) * TILE * TILE * 3;
                HIP_TRY(hipMemcpyPeerAsync(r->d_gather + (size_t)k * per * TILE * TILE * 3 + off, g0.device,
                                           g.d_shard + off, g.device, n * sizeof(double), g.stream));
            }
            HIP_TRY(hipEventRecord(g.shard_ev, g.stream));
            HIP_TRY(hipSetDevice(g0.device));
            HIP_TRY(hipStreamWaitEvent(g0.stream, g.shard_ev, 0));
        }
    }
    HIP_TRY(hipSetDevice(g0.device));
    if (world > 1) HIP_TRY(launch_unshard(r->d_gather, w, h, world, d_frame, g0.stream, row0, row1));
    if (d_rgba) HIP_TRY(launch_encode_rgba8(d_frame, (size_t)row0 * w, (size_t)row1 * w, d_rgba, g0.stream));
    if (ev) HIP_TRY(hipEventRecord(ev, g0.stream));
    return PT_OK;
}

// The feeder thread of a progressive frame: queues band b once band b - 2 is
// done, until the frame is queued or stop_rendering asks it to stop.
void feed_bands(pt_renderer *r) {
    const size_t n = r->bands.size();
    for (size_t b = 0; b < n; b++) {
        if (r->stop_req.load()) return;
        if (b >= 2) {
            (void)hipSetDevice(r->device());
            hipError_t e = hipEventSynchronize(r->bands[b - 2].ev);
            if (e != hipSuccess) {
                r->feed_err = std::string("hipEventSynchronize: ") + hipGetErrorString(e);
                r->feed_rc.store(PT_ERR_HIP);
                return;
            }
            if (r->stop_req.load()) return;
        }
        const auto &B = r->bands[b];
        if (int rc = enqueue_band(r, r->frame, r->d_frame, r->d_rgba, B.t0, B.t1, B.ev)) {
            r->feed_err = g_err;  // this thread's message
            r->feed_rc.store(rc);
            return;
        }
        r->bands_queued.store((uint32_t)(b + 1));
    }
}

void join_feeder(pt_renderer *r) {
    if (r->feeder.joinable()) r->feeder.join();
}

// Peer access between gpus[0] (which holds the frame) and every other distinct
// device, both ways, so hipMemcpyPeerAsync of a shard goes device to device
// over xGMI instead of staging through the host.  A pair the hardware cannot
// reach stays on the staged copy (still correct).
int enable_peers(pt_renderer *r) {
    const int d0 = r->gpus[0].device;
    std::vector<int> seen;
    for (size_t k = 1; k < r->gpus.size(); k++) {
        const int dk = r->gpus[k].device;
        if (dk == d0 || std::find(seen.begin(), seen.end(), dk) != seen.end()) continue;
        seen.push_back(dk);
        r->peer_pairs++;
        int a = 0, b = 0;
        HIP_TRY(hipDeviceCanAccessPeer(&a, dk, d0));
        HIP_TRY(hipDeviceCanAccessPeer(&b, d0, dk));
        if (!a || !b) continue;
        bool ok = true;
        for (int way = 0; way < 2; way++) {
            HIP_TRY(hipSetDevice(way == 0 ? dk : d0));
            const hipError_t e = hipDeviceEnablePeerAccess(way == 0 ? d0 : dk, 0);
            // "already enabled" is success; any other error leaves this pair on the staged
            // hipMemcpyPeerAsync (still correct): clear the error and carry on
            if (e != hipSuccess) (void)hipGetLastError();
            ok = ok && (e == hipSuccess || e == hipErrorPeerAccessAlreadyEnabled);
        }
        if (ok) r->peer_enabled++;
    }
    return PT_OK;
}

int create_renderer(pt_scene *scene, const std::vector<int> &devices, uint32_t depth, pt_renderer **out) {
    *out = nullptr;
    if (int rc = depth_refused(depth)) return rc;
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count == 0) return fail(PT_ERR_HIP, "no HIP device available (the GPU path has no CPU fallback)");
    for (int d : devices)
        if (d < 0 || d >= count) return fail(PT_ERR_INVALID, "device ordinal out of range");
    pt_renderer *r = new (std::nothrow) pt_renderer;
    if (!r) return fail(PT_ERR_INVALID, "out of memory");
    r->scene = scene;
    r->depth = depth;
    r->s11 = uniform_incl_scale(-1.0, 1.0);
    try {
        std::vector<DShape> hs;
        std::vector<DMaterial> hm;
        for (auto &s : scene->s.shapes) hs.push_back(to_device(s));
        for (auto &m : scene->s.materials) hm.push_back(to_device(m));
        if (hm.empty()) hm.push_back(DMaterial{});
        const Accel acc = build_accel(scene->s, scene->s.json_shapes, tuning_defaults().bvh_leaf);
        r->gpus.resize(devices.size());
        for (size_t k = 0; k < devices.size(); k++) {
            if (int rc = init_share(r->gpus[k], devices[k], scene->s, acc, hs, hm)) {
                pt_renderer_destroy(r);
                return rc;
            }
        }
    } catch (const std::bad_alloc &) {
        pt_renderer_destroy(r);
        return fail(PT_ERR_INVALID, "out of memory");
    }
    if (int rc = enable_peers(r)) {
        pt_renderer_destroy(r);
        return rc;
    }
    (void)hipSetDevice(devices[0]);
    {
        void *dp = nullptr;
        hipError_t e = hipHostMalloc((void **)&r->h_stop, sizeof(int),
                                     hipHostMallocPortable | hipHostMallocMapped | hipHostMallocCoherent);
        if (e == hipSuccess) {
            __atomic_store_n(r->h_stop, 0, __ATOMIC_SEQ_CST);
            e = hipHostGetDevicePointer(&dp, r->h_stop, 0);
        }
        if (e != hipSuccess) {
            pt_renderer_destroy(r);
            return hip_fail(e, "allocating the stop flag");
        }
        r->d_stop = (const int *)dp;
    }
    *out = r;
    return PT_OK;
}

}  // namespace

extern "C" {

int pt_renderer_create(pt_scene *scene, int device, uint32_t depth, pt_renderer **out) {
    if (!scene || !out) return fail(PT_ERR_INVALID, "null argument");
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0)
        return fail(PT_ERR_HIP, "no HIP device available (the GPU path has no CPU fallback)");
    if (device < 0) HIP_TRY(hipGetDevice(&device));
    return create_renderer(scene, {device}, depth, out);
}

int pt_renderer_create_multi(pt_scene *scene, const int *devices, int ngpu, uint32_t depth, pt_renderer **out) {
    if (!scene || !out) return fail(PT_ERR_INVALID, "null argument");
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0)
        return fail(PT_ERR_HIP, "no HIP device available (the GPU path has no CPU fallback)");
    if (ngpu <= 0) {
        if (devices) return fail(PT_ERR_INVALID, "ngpu must be > 0 when devices are listed");
        ngpu = count;
    }
    std::vector<int> dv((size_t)ngpu);
    for (int k = 0; k < ngpu; k++) dv[k] = devices ? devices[k] : k;
    return create_renderer(scene, dv, depth, out);
}

int pt_renderer_set_option(pt_renderer *r, const char *name, int64_t value) {
    if (!r || !name) return fail(PT_ERR_INVALID, "null argument");
    if (r->started) return fail(PT_ERR_STATE, "options cannot change while a frame is in flight");
    if (!std::strcmp(name, "bvh_leaf") && value != r->gpus[0].ws.tune.bvh_leaf) {
        // the BVH is rebuilt with the new leaf size on every device
        Tuning t = r->gpus[0].ws.tune;
        if (!tuning_set(&t, name, value))
            return fail(PT_ERR_INVALID, "bvh_leaf out of range (1..16): " + std::to_string((long long)value));
        std::vector<StagedAccel> staged(r->gpus.size());
        auto drop = [&] {
            for (size_t k = 0; k < staged.size(); k++) free_staged(r->gpus[k].device, staged[k]);
        };
        try {
            const Accel acc = build_accel(r->scene->s, r->scene->s.json_shapes, t.bvh_leaf);
            // every device stages the new tree before any device lets go of the old one
            for (size_t k = 0; k < r->gpus.size(); k++)
                if (int rc = stage_accel(r->gpus[k].device, acc, &staged[k], &r->fault_accel_alloc)) {
                    drop();
                    return rc;
                }
        } catch (const std::exception &e) {
            drop();
            return fail(PT_ERR_INVALID, std::string("rebuilding the BVH: ") + e.what());
        }
        for (size_t k = 0; k < r->gpus.size(); k++)
            if (int rc = commit_accel(r->gpus[k], staged[k])) {
                drop();  // the devices before k run the new tree, k and after the old one: both complete
                return rc;
            }
    }
    if (!std::strcmp(name, "fault_accel_alloc")) {  // test hook of this renderer, see stage_accel
        if (value < 0 || value > 64) return fail(PT_ERR_INVALID, "fault_accel_alloc out of range (0..64)");
        r->fault_accel_alloc = (int)value;
        return PT_OK;
    }
    for (auto &g : r->gpus) {
        Tuning t = g.ws.tune;
        if (!tuning_set(&t, name, value))
            return fail(PT_ERR_INVALID, std::string("unknown option or value out of range: ") + name + " = " +
                                            std::to_string((long long)value));
        // the workspace may be in use by a frame queued on any stream
        HIP_TRY(hipSetDevice(g.device));
        HIP_TRY(hipDeviceSynchronize());
        g.ws.tune = t;
        g.ds.view.diag = t.diag;
    }
    return PT_OK;
}

int pt_renderer_get_option(const pt_renderer *r, const char *name, int64_t *value) {
    if (!r || !name || !value) return fail(PT_ERR_INVALID, "null argument");
    if (!std::strcmp(name, "bvh_nodes")) {  // read-only state
        *value = r->gpus[0].ds.view.nnodes;
        return PT_OK;
    }
    // read-only too: what device 0's last launch_render call launched (builds::Ran; set_option knows no such name)
    if (ran_get(r->gpus[0].ws.ran, name, value)) return PT_OK;
    if (!std::strcmp(name, "first_cull_bits")) {  // read-only: the first-bounce cull table of device 0's last frame
        HIP_TRY(hipSetDevice(r->gpus[0].device));
        HIP_TRY(first_cull_bits(r->gpus[0].ws, value));
        return PT_OK;
    }
    if (!tuning_get(r->gpus[0].ws.tune, name, value)) return fail(PT_ERR_INVALID, std::string("unknown option: ") + name);
    return PT_OK;
}

const char *pt_option_name(int index) {
    return index >= 0 && index < KNOB_COUNT ? KNOBS[index].name : nullptr;
}

int pt_renderer_peer_access(const pt_renderer *r, int *pairs, int *enabled) {
    if (!r) return fail(PT_ERR_INVALID, "null renderer");
    if (pairs) *pairs = r->peer_pairs;
    if (enabled) *enabled = r->peer_enabled;
    return PT_OK;
}

int pt_renderer_num_devices(const pt_renderer *r) { return r ? (int)r->gpus.size() : fail(PT_ERR_INVALID, "null renderer"); }

void pt_renderer_destroy(pt_renderer *r) {
    if (!r) return;
    if (r->started) (void)pt_render_stop(r);
    join_feeder(r);
    (void)sync_all(r);
    release_bands(r);
    if (!r->gpus.empty()) {
        (void)hipSetDevice(r->device());
        if (r->d_frame) (void)hipFree(r->d_frame);
        if (r->d_rgba) (void)hipFree(r->d_rgba);
        if (r->d_gather) (void)hipFree(r->d_gather);
    }
    for (auto &g : r->gpus) free_share(g);
    if (r->h_stop) (void)hipHostFree(r->h_stop);
    delete r;
}

int pt_render_start(pt_renderer *r, const pt_camera *cam, uint32_t w, uint32_t h, uint32_t spp, uint64_t seed) {
    if (!r || !cam) return fail(PT_ERR_INVALID, "null argument");
    if (int rc = frame_refused(w, h, spp)) return rc;
    if (r->started) {  // a new frame replaces the one in flight (the reference stops it first, main.rs:268)
        if (int rc = pt_render_stop(r)) return rc;
    }
    HIP_TRY(hipSetDevice(r->device()));
    if (int rc = grow(&r->d_frame, &r->frame_cap, (size_t)w * h * 3)) return rc;
    if (int rc = grow(&r->d_rgba, &r->rgba_cap, (size_t)w * h * 4)) return rc;
    if (int rc = frame_prologue(r, w, h)) return rc;
    r->frame = frame_params(r, *cam, w, h, spp, seed);
    r->frame.stop = r->d_stop;
    // ~8 bands of whole tile rows, each a pass of the engine over 1/8 of the frame, but no band under
    // BAND_MIN_SAMPLES: a band of the reference GUI's 1-spp preview at 1600x900 (main.rs:264) would otherwise be
    // 160k samples, a chain of ~260 launches that each find a few paths (a 78 ms frame, round 5).  The stop
    // latency does not depend on the band size (stop_gate runs at every chunk start and compaction).
    const uint32_t ty = tiles_across(h);
    const uint64_t row_samples = (uint64_t)tiles_across(w) * TILE * TILE * spp;
    const uint32_t min_rows = (uint32_t)((BAND_MIN_SAMPLES + row_samples - 1) / row_samples);
    uint32_t band = ty >= 8 ? ty / 8 : 1;
    if (band < min_rows) band = min_rows < ty ? min_rows : ty;
    release_bands(r);
    for (uint32_t t0 = 0; t0 < ty; t0 += band) {
        pt_renderer::Band b;
        b.t0 = t0;
        b.t1 = t0 + band < ty ? t0 + band : ty;
        b.row0 = t0 * TILE;
        b.row1 = b.t1 * TILE < h ? b.t1 * TILE : h;
        b.copied = false;
        hipError_t e = hipEventCreateWithFlags(&b.ev, hipEventDisableTiming);
        if (e != hipSuccess) {
            release_bands(r);
            return hip_fail(e, "hipEventCreateWithFlags");
        }
        r->bands.push_back(b);
    }
    r->width = w;
    r->height = h;
    r->stop_req.store(false);
    r->bands_queued.store(0);
    r->feed_rc.store(0);
    r->feed_err.clear();
    try {
        r->feeder = std::thread(feed_bands, r);
    } catch (const std::exception &ex) {
        release_bands(r);
        return fail(PT_ERR_INVALID, std::string("cannot start the band feeder: ") + ex.what());
    }
    r->started = true;
    return PT_OK;
}

// Renderer::render_step: copy every band finished since the last call into
// rgb (linear f64) and / or rgba (display encode); 1 once the frame is complete.
int pt_render_step_rgba8(pt_renderer *r, double *rgb, uint8_t *rgba, int blocking) {
    if (!r || (!rgb && !rgba)) return fail(PT_ERR_INVALID, "null argument");
    if (!r->started) return fail(PT_ERR_STATE, "render_step before start_rendering");
    HIP_TRY(hipSetDevice(r->device()));
    if (blocking) join_feeder(r);  // every band queued (or the feeder failed)
    if (r->feed_rc.load()) {
        join_feeder(r);
        const int rc = r->feed_rc.load();
        const std::string msg = r->feed_err;
        (void)pt_render_stop(r);
        return fail(rc, "queueing the frame: " + msg);
    }
    const uint32_t queued = r->bands_queued.load();
    bool done = true;
    for (uint32_t k = 0; k < r->bands.size(); k++) {
        auto &b = r->bands[k];
        if (b.copied) continue;
        if (k >= queued) {  // not queued yet (non-blocking only)
            done = false;
            continue;
        }
        if (blocking) {
            HIP_TRY(hipEventSynchronize(b.ev));
        } else {
            hipError_t q = hipEventQuery(b.ev);
            if (q == hipErrorNotReady) {
                (void)hipGetLastError();
                done = false;
                continue;
            }
            if (q != hipSuccess) return hip_fail(q, "hipEventQuery");
        }
        const size_t p0 = (size_t)b.row0 * r->width, np = (size_t)(b.row1 - b.row0) * r->width;
        if (rgb) HIP_TRY(hipMemcpy(rgb + p0 * 3, r->d_frame + p0 * 3, np * 3 * sizeof(double), hipMemcpyDeviceToHost));
        if (rgba) HIP_TRY(hipMemcpy(rgba + p0 * 4, r->d_rgba + p0 * 4, np * 4, hipMemcpyDeviceToHost));
        b.copied = true;
    }
    if (done) {
        join_feeder(r);
        release_bands(r);
        r->started = false;
        return 1;
    }
    return 0;
}

int pt_render_step(pt_renderer *r, double *rgb, int blocking) {
    if (!r || !rgb) return fail(PT_ERR_INVALID, "null argument");
    return pt_render_step_rgba8(r, rgb, nullptr, blocking);
}

// Renderer::stop_rendering: the feeder queues no further band and the stop
// flag turns the frame's queued launches into no-ops, so the wait is for the
// launches already running; the flag is cleared once the streams are idle
// and the frame is forgotten.
int pt_render_stop(pt_renderer *r) {
    if (!r) return fail(PT_ERR_INVALID, "null argument");
    r->stop_req.store(true);
    const bool flag = r->started && r->h_stop;
    if (flag) __atomic_store_n(r->h_stop, 1, __ATOMIC_SEQ_CST);
    join_feeder(r);
    int rc = sync_all(r);
    if (flag) __atomic_store_n(r->h_stop, 0, __ATOMIC_SEQ_CST);
    release_bands(r);
    r->started = false;
    return rc;
}

uint32_t pt_shard_tiles(uint32_t w, uint32_t h, uint32_t rank, uint32_t world) {
    return shard_tiles(w, h, rank, world);
}

int pt_render_device(pt_renderer *r, const pt_camera *cam, uint32_t w, uint32_t h, uint32_t spp, uint64_t seed,
                     uint32_t rank, uint32_t world, double *d_out, void *stream) {
    return pt_render_device_samples(r, cam, w, h, spp, seed, rank, world, 0, spp, d_out, stream);
}

namespace {
// One window of a rank's shard: the whole shard (tiles null), or the listed tiles of it (a listed launch, launch_render).
static int render_shard(pt_renderer *r, const pt_camera *cam, uint32_t w, uint32_t h, uint32_t spp, uint64_t seed,
                 uint32_t rank, uint32_t world, uint32_t s_begin, uint32_t s_end, bool listed, const uint32_t *tiles,
                 uint32_t tile_count, double *d_out, void *stream) {
    if (!r || !cam || !d_out || (listed && !tiles)) return fail(PT_ERR_INVALID, "null argument");
    if (int rc = frame_refused(w, h, spp)) return rc;
    if (int rc = rank_refused(rank, world)) return rc;
    if (int rc = sample_window_refused(s_begin, s_end, spp)) return rc;
    if (listed && !tile_list_ok(tiles, tile_count, shard_tiles(w, h, rank, world)))
        return fail(PT_ERR_INVALID, "tiles must be 1 or more strictly ascending entries of the rank's tile list");
    if (int rc = in_flight_refused(r)) return rc;
    GpuShare &g = r->gpus[0];
    HIP_TRY(hipSetDevice(g.device));
    FrameParams P = shard_params(r, *cam, w, h, spp, seed, rank, world);
    if (listed) P.tile_count = tile_count;  // positions of the list, which launch_render copies before it returns
    P.s_begin = s_begin;
    P.s_end = s_end;
    // any HIP stream of the renderer's (first) device, 0 being the null stream
    // as everywhere in HIP (pt_unshard_device takes the same handle, so a
    // caller's render -> gather -> unshard stays ordered)
    return render_on(g, P, d_out, (hipStream_t)stream, tiles);
}
}  // namespace

int pt_render_device_samples(pt_renderer *r, const pt_camera *cam, uint32_t w, uint32_t h, uint32_t spp,
                             uint64_t seed, uint32_t rank, uint32_t world, uint32_t s_begin, uint32_t s_end,
                             double *d_out, void *stream) {
    return render_shard(r, cam, w, h, spp, seed, rank, world, s_begin, s_end, false, nullptr, 0, d_out, stream);
}

int pt_render_device_tiles(pt_renderer *r, const pt_camera *cam, uint32_t w, uint32_t h, uint32_t spp, uint64_t seed,
                           uint32_t rank, uint32_t world, uint32_t s_begin, uint32_t s_end, const uint32_t *tiles,
                           uint32_t tile_count, double *d_out, void *stream) {
    return render_shard(r, cam, w, h, spp, seed, rank, world, s_begin, s_end, true, tiles, tile_count, d_out, stream);
}

int pt_render_frame_device(pt_renderer *r, const pt_camera *cam, uint32_t w, uint32_t h, uint32_t spp, uint64_t seed,
                           double *d_frame, void *stream) {
    if (!r || !cam || !d_frame) return fail(PT_ERR_INVALID, "null argument");
    if (int rc = frame_refused(w, h, spp)) return rc;
    if (int rc = in_flight_refused(r)) return rc;
    GpuShare &g0 = r->gpus[0];
    HIP_TRY(hipSetDevice(g0.device));
    hipStream_t st = (hipStream_t)stream;
    // the frame runs on the renderer's streams, after everything queued on st;
    // st resumes when the frame is in d_frame
    HIP_TRY(hipEventRecord(g0.shard_ev, st));
    HIP_TRY(hipStreamWaitEvent(g0.stream, g0.shard_ev, 0));
    const FrameParams P = frame_params(r, *cam, w, h, spp, seed);
    if (int rc = frame_prologue(r, w, h)) return rc;
    if (int rc = enqueue_band(r, P, d_frame, nullptr, 0, tiles_across(h), nullptr)) return rc;
    HIP_TRY(hipSetDevice(g0.device));
    HIP_TRY(hipEventRecord(g0.shard_ev, g0.stream));
    HIP_TRY(hipStreamWaitEvent(st, g0.shard_ev, 0));
    return PT_OK;
}

// ---- first-hit guide planes (pt_aov.hpp): a pass beside the frame, on the first device ----
namespace {
int aov_args_refused(const pt_renderer *r, const pt_camera *cam, uint32_t w, uint32_t h, uint32_t spp, uint32_t rank,
                     uint32_t world, const double *a, const double *n, const double *d) {
    if (!r || !cam) return fail(PT_ERR_INVALID, "null argument");
    if (!a && !n && !d) return fail(PT_ERR_INVALID, "at least one of the albedo, normal and depth planes must be given");
    if (int rc = frame_refused(w, h, spp)) return rc;
    if (int rc = rank_refused(rank, world)) return rc;
    if (int rc = in_flight_refused(r)) return rc;
    return PT_OK;
}
}  // namespace

int pt_render_aov_device(pt_renderer *r, const pt_camera *cam, uint32_t w, uint32_t h, uint32_t spp, uint64_t seed,
                         uint32_t rank, uint32_t world, double *d_albedo, double *d_normal, double *d_depth,
                         void *stream) {
    if (int rc = aov_args_refused(r, cam, w, h, spp, rank, world, d_albedo, d_normal, d_depth)) return rc;
    GpuShare &g = r->gpus[0];
    HIP_TRY(hipSetDevice(g.device));
    // the frame's own parameters (pt_render_device's): the pass reads the camera, the seed and the tile deal of them
    FrameParams P = shard_params(r, *cam, w, h, spp, seed, rank, world);
    HIP_TRY(launch_aov(g.ds.view, P, d_albedo, d_normal, d_depth, (hipStream_t)stream));
    return PT_OK;
}

int pt_render_aov(pt_renderer *r, const pt_camera *cam, uint32_t w, uint32_t h, uint32_t spp, uint64_t seed,
                  double *albedo, double *normal, double *depth) {
    if (int rc = aov_args_refused(r, cam, w, h, spp, 0, 1, albedo, normal, depth)) return rc;
    HIP_TRY(hipSetDevice(r->device()));
    const size_t count = (size_t)w * h * 3;
    double *host[3] = {albedo, normal, depth};
    DevBuf<double> dev[3];  // staging of the wanted planes, freed on return
    for (int k = 0; k < 3; k++)
        if (host[k]) HIP_TRY(dev[k].alloc(count));
    if (int rc = pt_render_aov_device(r, cam, w, h, spp, seed, 0, 1, dev[0].p, dev[1].p, dev[2].p, r->stream())) return rc;
    HIP_TRY(hipStreamSynchronize(r->stream()));
    for (int k = 0; k < 3; k++) HIP_TRY(dev[k].download(host[k]));
    return PT_OK;
}

int pt_unshard_device(int device, const double *g, uint32_t w, uint32_t h, uint32_t world, double *frame,
                      void *stream) {
    if (!g || !frame || world == 0) return fail(PT_ERR_INVALID, "bad argument");
    if (device >= 0) HIP_TRY(hipSetDevice(device));
    HIP_TRY(launch_unshard(g, w, h, world, frame, (hipStream_t)stream));
    return PT_OK;
}

int pt_encode_rgba8_device(int device, const double *d_rgb, size_t npix, uint8_t *d_rgba, void *stream) {
    if (npix && (!d_rgb || !d_rgba)) return fail(PT_ERR_INVALID, "null argument");
    if (((uintptr_t)d_rgba & 3u) != 0) return fail(PT_ERR_INVALID, "rgba must be 4-byte aligned");
    if (device >= 0) HIP_TRY(hipSetDevice(device));
    HIP_TRY(launch_encode_rgba8(d_rgb, 0, npix, d_rgba, (hipStream_t)stream));
    return PT_OK;
}

// ---- guided à-trous denoiser (pt_denoise.hpp): a pass over four frames, needs no renderer ----
static_assert(PT_DENOISE_DEMODULATE == DENOISE_DEMODULATE && PT_DENOISE_MAX_ITERATIONS == DENOISE_MAX_ITERATIONS,
              "the header states the denoiser's flag and iteration limit");
namespace {
// Both filters behind one pair of functions: `variance` is null for the plain one, whose `sigma` is sigma_colour, and
// the plane of the variance-guided one (pt_denoise_variance*, which refuse a null plane themselves), whose `sigma` is
// sigma_variance.  The checks the device form and the host form share (the pointers are device or host memory alike):
int denoise_args_refused(const double *rgb, const double *albedo, const double *normal, const double *depth,
                         const double *variance, uint32_t w, uint32_t h, uint32_t iterations, double sigma_normal,
                         double sigma_depth, double sigma, uint32_t flags, const double *out) {
    if (variance && !(sigma > 0.0)) return fail(PT_ERR_INVALID, "sigma_variance must be > 0");
    if (!rgb || !normal || !depth || !out) return fail(PT_ERR_INVALID, "null argument");
    if (flags & ~PT_DENOISE_DEMODULATE) return fail(PT_ERR_INVALID, "unknown denoise flag");
    if ((flags & PT_DENOISE_DEMODULATE) && !albedo)
        return fail(PT_ERR_INVALID, "PT_DENOISE_DEMODULATE needs the albedo plane");
    if (int rc = frame_refused(w, h)) return rc;
    if (iterations < 1 || iterations > PT_DENOISE_MAX_ITERATIONS)
        return fail(PT_ERR_INVALID, "iterations must be 1.." + std::to_string(PT_DENOISE_MAX_ITERATIONS));
    if (int rc = sigmas_refused(sigma_normal, sigma_depth)) return rc;
    if (!variance && !(sigma >= 0.0)) return fail(PT_ERR_INVALID, "sigma_colour must be >= 0");
    if (denoise_workspace_doubles(w, h) == 0 || !tile_grid_ok(w, h))
        return fail(PT_ERR_INVALID, "the frame is too large to denoise in one call");
    return PT_OK;
}

static int denoise_device(int device, const double *d_rgb, const double *d_albedo, const double *d_normal,
                   const double *d_depth, const double *d_variance, uint32_t w, uint32_t h, uint32_t iterations,
                   double sigma_normal, double sigma_depth, double sigma, uint32_t flags, double *d_out, double *d_work,
                   void *stream) {
    if (int rc = denoise_args_refused(d_rgb, d_albedo, d_normal, d_depth, d_variance, w, h, iterations, sigma_normal,
                                      sigma_depth, sigma, flags, d_out))
        return rc;
    if (int rc = workspace_refused(d_work)) return rc;
    if (device >= 0) HIP_TRY(hipSetDevice(device));
    const dev::DenoiseConsts k = denoise_consts(iterations, sigma_normal, sigma_depth, d_variance ? 0.0 : sigma);
    if (d_variance)
        HIP_TRY(launch_denoise_variance(d_rgb, d_albedo, d_normal, d_depth, d_variance, w, h, iterations, k,
                                        denoise_variance_rv(sigma), flags, d_out, d_work, (hipStream_t)stream));
    else
        HIP_TRY(launch_denoise(d_rgb, d_albedo, d_normal, d_depth, w, h, iterations, k, flags, d_out, d_work,
                               (hipStream_t)stream));
    return PT_OK;
}

static int denoise_host(int device, const double *rgb, const double *albedo, const double *normal, const double *depth,
                 const double *variance, uint32_t w, uint32_t h, uint32_t iterations, double sigma_normal,
                 double sigma_depth, double sigma, uint32_t flags, double *out) {
    if (int rc = denoise_args_refused(rgb, albedo, normal, depth, variance, w, h, iterations, sigma_normal, sigma_depth,
                                      sigma, flags, out))
        return rc;
    if (device >= 0) HIP_TRY(hipSetDevice(device));
    const size_t count = (size_t)w * h * 3;
    const double *host[5] = {rgb, (flags & PT_DENOISE_DEMODULATE) ? albedo : nullptr, normal, depth, variance};
    DevBuf<double> dev[5], work;  // staging, freed on return; the frame is denoised in place in dev[0]
    for (int k = 0; k < 5; k++) HIP_TRY(dev[k].upload(host[k], count));
    HIP_TRY(work.alloc(denoise_workspace_doubles(w, h)));
    if (int rc = denoise_device(-1, dev[0].p, dev[1].p, dev[2].p, dev[3].p, dev[4].p, w, h, iterations, sigma_normal,
                                sigma_depth, sigma, flags, dev[0].p, work.p, nullptr))
        return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    HIP_TRY(dev[0].download(out));
    return PT_OK;
}
}  // namespace

size_t pt_denoise_workspace_doubles(uint32_t w, uint32_t h) { return denoise_workspace_doubles(w, h); }

int pt_denoise_device(int device, const double *d_rgb, const double *d_albedo, const double *d_normal,
                      const double *d_depth, uint32_t w, uint32_t h, uint32_t iterations, double sigma_normal,
                      double sigma_depth, double sigma_colour, uint32_t flags, double *d_out, double *d_work,
                      void *stream) {
    return denoise_device(device, d_rgb, d_albedo, d_normal, d_depth, nullptr, w, h, iterations, sigma_normal,
                          sigma_depth, sigma_colour, flags, d_out, d_work, stream);
}

int pt_denoise(int device, const double *rgb, const double *albedo, const double *normal, const double *depth,
               uint32_t w, uint32_t h, uint32_t iterations, double sigma_normal, double sigma_depth,
               double sigma_colour, uint32_t flags, double *out) {
    return denoise_host(device, rgb, albedo, normal, depth, nullptr, w, h, iterations, sigma_normal, sigma_depth,
                        sigma_colour, flags, out);
}

// ---- temporal accumulation (pt_temporal.hpp): the last frame reprojected into a moved camera, needs no renderer ----
namespace {
// the checks the device form and the host form share (the pointers are device or host memory alike)
int temporal_args_refused(const double *rgb, const double *normal, const double *depth, const pt_camera *camera,
                          const pt_camera *prev_camera, uint32_t w, uint32_t h, const double *history_in,
                          const double *history_out, uint32_t max_count, double sigma_normal, double sigma_depth,
                          const double *out) {
    if (!rgb || !normal || !depth || !camera || !history_out || !out) return fail(PT_ERR_INVALID, "null argument");
    if (int rc = frame_refused(w, h)) return rc;
    if (max_count == 0) return fail(PT_ERR_INVALID, "max_count must be > 0");
    if (int rc = sigmas_refused(sigma_normal, sigma_depth)) return rc;
    if ((prev_camera == nullptr) != (history_in == nullptr))
        return fail(PT_ERR_INVALID, "prev_camera and history_in are given together, or neither (the first frame)");
    const size_t doubles = temporal_history_doubles(w, h);
    if (doubles == 0 || !tile_grid_ok(w, h))
        return fail(PT_ERR_INVALID, "the frame is too large to accumulate in one call");
    if (history_in) {
        const uintptr_t a = (uintptr_t)history_in, b = (uintptr_t)history_out, bytes = doubles * sizeof(double);
        if (a < b + bytes && b < a + bytes) return fail(PT_ERR_INVALID, "history_in and history_out overlap");
    }
    return PT_OK;
}

dev::TemporalCam temporal_cam(const pt_camera &c, uint32_t w, uint32_t h) {
    FrameParams fp;
    caster_params(c, w, h, &fp);  // the very values the render uses
    dev::TemporalCam t;
    for (int k = 0; k < 3; k++) {
        t.pos[k] = fp.pos[k];
        t.right[k] = fp.right[k];
        t.up[k] = fp.up[k];
        t.lt[k] = fp.left_top[k];
    }
    t.res = fp.pixel_resolution;
    return t;
}
}  // namespace

size_t pt_temporal_history_doubles(uint32_t w, uint32_t h) { return temporal_history_doubles(w, h); }

int pt_temporal_device(int device, const double *d_rgb, const double *d_normal, const double *d_depth,
                       const pt_camera *camera, const pt_camera *prev_camera, uint32_t w, uint32_t h,
                       const double *d_history_in, double *d_history_out, uint32_t max_count, double sigma_normal,
                       double sigma_depth, double *d_out, void *stream) {
    if (int rc = temporal_args_refused(d_rgb, d_normal, d_depth, camera, prev_camera, w, h, d_history_in,
                                       d_history_out, max_count, sigma_normal, sigma_depth, d_out))
        return rc;
    if ((((uintptr_t)d_history_in | (uintptr_t)d_history_out) & 15u) != 0)
        return fail(PT_ERR_INVALID, "the histories must be 16-byte aligned");
    if (device >= 0) HIP_TRY(hipSetDevice(device));
    const dev::TemporalCam now = temporal_cam(*camera, w, h);
    dev::TemporalCam prev{};
    if (prev_camera) prev = temporal_cam(*prev_camera, w, h);
    HIP_TRY(launch_temporal(d_rgb, d_normal, d_depth, w, h,
                            temporal_consts(now, prev_camera ? &prev : nullptr,
                                            prev_camera ? prev_camera->direction : nullptr,
                                            prev_camera ? prev_camera->focal_length : 0.0, max_count, sigma_normal,
                                            sigma_depth),
                            d_history_in, d_history_out, d_out, (hipStream_t)stream));
    return PT_OK;
}

int pt_temporal(int device, const double *rgb, const double *normal, const double *depth, const pt_camera *camera,
                const pt_camera *prev_camera, uint32_t w, uint32_t h, const double *history_in, double *history_out,
                uint32_t max_count, double sigma_normal, double sigma_depth, double *out) {
    if (int rc = temporal_args_refused(rgb, normal, depth, camera, prev_camera, w, h, history_in, history_out,
                                       max_count, sigma_normal, sigma_depth, out))
        return rc;
    if (device >= 0) HIP_TRY(hipSetDevice(device));
    const size_t count = (size_t)w * h * 3, hist = temporal_history_doubles(w, h);
    const double *host[3] = {rgb, normal, depth};
    DevBuf<double> dev[3], hin, hout;  // staging, freed on return; the frame is written in place in dev[0]
    for (int k = 0; k < 3; k++) HIP_TRY(dev[k].upload(host[k], count));
    HIP_TRY(hin.upload(history_in, hist));  // (none on the first frame)
    HIP_TRY(hout.alloc(hist));
    if (int rc = pt_temporal_device(-1, dev[0].p, dev[1].p, dev[2].p, camera, prev_camera, w, h, hin.p, hout.p,
                                    max_count, sigma_normal, sigma_depth, dev[0].p, nullptr))
        return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    HIP_TRY(dev[0].download(out));
    HIP_TRY(hout.download(history_out));
    return PT_OK;
}

// ---- per-pixel variance from sample windows (pt_variance.hpp) and the denoiser's variance term ----
namespace {
// elements of one rank's d_out; 0 on a zero size, rank >= world, or a count whose workspace does not fit
uint64_t variance_count(uint32_t w, uint32_t h, uint32_t rank, uint32_t world) {
    if (w == 0 || h == 0 || world == 0 || rank >= world) return 0;
    const uint64_t count = shard_elements(w, h, rank, world);
    return variance_workspace_doubles(count) ? count : 0;
}

int variance_window_refused(const double *d_out, size_t count, uint32_t n_k, uint32_t spp, uint32_t window,
                            uint32_t windows, const double *d_work, const double *d_variance) {
    if (!d_out || !d_work || !d_variance) return fail(PT_ERR_INVALID, "null argument");
    if (count == 0 || variance_workspace_doubles(count) == 0 || (count + 255) / 256 > 0x7fffffffull)
        return fail(PT_ERR_INVALID, "count must be > 0 and fit one launch");
    if (int rc = windows_refused(windows, spp)) return rc;
    if (window < 1 || window > windows) return fail(PT_ERR_INVALID, "window must be 1..windows");
    if (n_k < 1 || n_k > spp) return fail(PT_ERR_INVALID, "n_k must be 1..samples_number");
    return PT_OK;
}
}  // namespace

size_t pt_variance_workspace_doubles(uint32_t w, uint32_t h, uint32_t rank, uint32_t world) {
    return variance_workspace_doubles(variance_count(w, h, rank, world));
}

int pt_variance_window_device(int device, const double *d_out, size_t count, uint32_t n_k, uint32_t spp,
                              uint32_t window, uint32_t windows, double *d_work, double *d_variance, void *stream) {
    if (int rc = variance_window_refused(d_out, count, n_k, spp, window, windows, d_work, d_variance)) return rc;
    if (device >= 0) HIP_TRY(hipSetDevice(device));
    HIP_TRY(launch_variance_window(d_out, count, variance_consts(n_k, spp, windows), window == 1, window == windows,
                                   d_work, d_variance, (hipStream_t)stream));
    return PT_OK;
}

int pt_render_variance_device(pt_renderer *r, const pt_camera *cam, uint32_t w, uint32_t h, uint32_t spp,
                              uint64_t seed, uint32_t rank, uint32_t world, uint32_t windows, double *d_out,
                              double *d_variance, double *d_work, void *stream) {
    if (!r || !cam || !d_out || !d_variance || !d_work) return fail(PT_ERR_INVALID, "null argument");
    if (int rc = frame_refused(w, h, spp)) return rc;
    if (int rc = rank_refused(rank, world)) return rc;
    if (int rc = windows_refused(windows, spp)) return rc;
    const uint64_t count = variance_count(w, h, rank, world);
    if (count == 0 || (count + 255) / 256 > 0x7fffffffull)
        return fail(PT_ERR_INVALID, "the frame is too large for the variance pass (or the rank has no tile)");
    if (int rc = in_flight_refused(r)) return rc;
    // the frame's own windows, each followed by its accumulate launch on the same stream: no sync of ours
    for (uint32_t k = 1; k <= windows; k++) {
        const uint32_t e0 = variance_edge(k - 1, spp, windows), e1 = variance_edge(k, spp, windows);
        if (int rc = pt_render_device_samples(r, cam, w, h, spp, seed, rank, world, e0, e1, d_out, stream)) return rc;
        if (int rc = pt_variance_window_device(-1, d_out, (size_t)count, e1 - e0, spp, k, windows, d_work, d_variance,
                                               stream))
            return rc;
    }
    return PT_OK;
}

int pt_render_variance(pt_renderer *r, const pt_camera *cam, uint32_t w, uint32_t h, uint32_t spp, uint64_t seed,
                       uint32_t windows, double *rgb, double *variance) {
    if (!r || !cam || !rgb || !variance) return fail(PT_ERR_INVALID, "null argument");
    if (int rc = frame_refused(w, h, spp)) return rc;
    if (int rc = windows_refused(windows, spp)) return rc;
    const uint64_t count = variance_count(w, h, 0, 1);
    if (count == 0) return fail(PT_ERR_INVALID, "the frame is too large for the variance pass");
    if (int rc = in_flight_refused(r)) return rc;
    HIP_TRY(hipSetDevice(r->device()));
    DevBuf<double> out, var, work;  // staging, freed on return
    HIP_TRY(out.alloc((size_t)count));
    HIP_TRY(var.alloc((size_t)count));
    HIP_TRY(work.alloc(variance_workspace_doubles(count)));
    if (int rc = pt_render_variance_device(r, cam, w, h, spp, seed, 0, 1, windows, out.p, var.p, work.p, r->stream()))
        return rc;
    HIP_TRY(hipStreamSynchronize(r->stream()));
    HIP_TRY(out.download(rgb));
    HIP_TRY(var.download(variance));
    return PT_OK;
}

int pt_denoise_variance_device(int device, const double *d_rgb, const double *d_albedo, const double *d_normal,
                               const double *d_depth, const double *d_variance, uint32_t w, uint32_t h,
                               uint32_t iterations, double sigma_normal, double sigma_depth, double sigma_variance,
                               uint32_t flags, double *d_out, double *d_work, void *stream) {
    if (!d_variance) return fail(PT_ERR_INVALID, "null argument");
    return denoise_device(device, d_rgb, d_albedo, d_normal, d_depth, d_variance, w, h, iterations, sigma_normal,
                          sigma_depth, sigma_variance, flags, d_out, d_work, stream);
}

int pt_denoise_variance(int device, const double *rgb, const double *albedo, const double *normal,
                        const double *depth, const double *variance, uint32_t w, uint32_t h, uint32_t iterations,
                        double sigma_normal, double sigma_depth, double sigma_variance, uint32_t flags, double *out) {
    if (!variance) return fail(PT_ERR_INVALID, "null argument");
    return denoise_host(device, rgb, albedo, normal, depth, variance, w, h, iterations, sigma_normal, sigma_depth,
                        sigma_variance, flags, out);
}

// ---- adaptive sampling: every tile stops at a noise target (pt_adaptive.hpp) ----
namespace {
static_assert(PT_ADAPTIVE_WINDOW == ADAPTIVE_WINDOW && PT_ADAPTIVE_LUMINANCE_FLOOR == ADAPTIVE_FLOOR &&
                  PT_ADAPTIVE_MERGE_GAP == ADAPTIVE_MERGE_GAP,
              "the header states the recommended defaults");
int adaptive_refused(const void *r, const void *cam, uint32_t w, uint32_t h, uint32_t window, uint32_t min_samples,
                     uint32_t max_samples, double threshold, double luminance_floor, uint32_t rank, uint32_t world,
                     const void *out, const void *tile_samples) {
    if (!r || !cam || !out || !tile_samples) return fail(PT_ERR_INVALID, "null argument");
    if (w == 0 || h == 0 || window == 0) return fail(PT_ERR_INVALID, "width, height and window must be > 0");
    if (max_samples <= window) return fail(PT_ERR_INVALID, "max_samples must be above window (two windows at least)");
    if (max_samples > 0xfffffffeu) return fail(PT_ERR_INVALID, "max_samples must be at most 2^32 - 2");
    if (min_samples > max_samples) return fail(PT_ERR_INVALID, "min_samples must be at most max_samples");
    if (!(threshold >= 0.0)) return fail(PT_ERR_INVALID, "threshold must be >= 0");
    if (!(luminance_floor >= 0.0)) return fail(PT_ERR_INVALID, "luminance_floor must be >= 0");
    if (int rc = rank_refused(rank, world)) return rc;
    if (shard_tiles(w, h, rank, world) == 0 || adaptive_workspace_doubles(variance_count(w, h, rank, world)) == 0)
        return fail(PT_ERR_INVALID, "the frame is too large for the adaptive pass (or the rank has no tile)");
    return PT_OK;
}
}  // namespace

size_t pt_adaptive_workspace_doubles(uint32_t w, uint32_t h, uint32_t rank, uint32_t world) {
    return adaptive_workspace_doubles(variance_count(w, h, rank, world));
}

namespace {
// The adaptive frame on the device, for the run-based and the listed entries: they differ only in how a window's
// still-active tiles are launched (listed: one launch over adaptive_list; else one per run of adaptive_runs).
int adaptive_device(pt_renderer *r, const pt_camera *cam, uint32_t w, uint32_t h, uint32_t window,
                    uint32_t min_samples, uint32_t max_samples, double threshold, double luminance_floor,
                    bool listed, uint32_t merge_gap, uint64_t seed, uint32_t rank, uint32_t world, double *d_out,
                    double *d_variance, uint32_t *d_tile_samples, double *d_tile_error, double *d_work,
                    void *stream, uint64_t *samples_rendered) {
    if (int rc = adaptive_refused(r, cam, w, h, window, min_samples, max_samples, threshold, luminance_floor, rank,
                                  world, d_out, d_tile_samples))
        return rc;
    if (int rc = workspace_refused(d_work)) return rc;
    if (int rc = in_flight_refused(r)) return rc;
    GpuShare &g = r->gpus[0];
    HIP_TRY(hipSetDevice(g.device));
    hipStream_t st = (hipStream_t)stream;
    const size_t count = (size_t)variance_count(w, h, rank, world);
    const uint32_t ntiles = shard_tiles(w, h, rank, world);
    // Every window is a window of a frame one sample longer than the cap, so s_end < spp always holds and the render
    // leaves sums, never means: spp reaches only wf_reduce's final division and the engine choice (a windowed frame
    // always runs the wavefront engine; the samples' keys come from their indices).
    FrameParams P = shard_params(r, *cam, w, h, max_samples + 1, seed, rank, world);
    const dev::AdaptiveGeom geom{dev::tile_geom(P)};
    std::vector<uint8_t> active(ntiles, 1);
    std::vector<uint32_t> pixels(ntiles), stopped(ntiles);
    for (uint32_t i = 0; i < ntiles; i++) pixels[i] = dev::adaptive_tile_pixels(geom, i);
    uint64_t launched = 0;
    const uint32_t windows = adaptive_windows(window, max_samples);
    for (uint32_t k = 1; k <= windows; k++) {
        const dev::AdaptiveConsts c = adaptive_consts(k, window, min_samples, max_samples, threshold, luminance_floor);
        P.s_begin = adaptive_edge(k - 1, window, max_samples);
        P.s_end = c.e_k;
        // the window's samples of the still-active tiles, into the sums plane: one listed launch, or one launch per run
        std::vector<AdaptiveRun> runs;
        if (listed) {
            const std::vector<uint32_t> list = adaptive_list(active.data(), ntiles);
            if (list.empty()) break;
            P.tile_begin = 0;
            P.tile_count = (uint32_t)list.size();
            if (int rc = render_on(g, P, d_work, st, list.data())) return rc;
            for (uint32_t i : list) launched += (uint64_t)pixels[i] * (P.s_end - P.s_begin);
        } else {
            runs = adaptive_runs(active.data(), ntiles, merge_gap);
            if (runs.empty()) break;
        }
        for (const AdaptiveRun &run : runs) {
            P.tile_begin = run.begin;
            P.tile_count = run.count;
            if (int rc = render_on(g, P, d_work, st)) return rc;
            for (uint32_t i = run.begin; i < run.begin + run.count; i++)
                launched += (uint64_t)pixels[i] * (P.s_end - P.s_begin);
        }
        HIP_TRY(launch_adaptive_tiles(geom, ntiles, count, c, k == 1, d_work, d_out, d_variance, d_tile_samples,
                                      d_tile_error, st));
        if (!c.evaluate || c.cap) continue;  // no tile can have stopped, or every tile has
        // the host decides the next window's launches: 4 bytes per tile
        HIP_TRY(hipMemcpyAsync(stopped.data(), d_tile_samples, (size_t)ntiles * sizeof(uint32_t),
                               hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (uint32_t i = 0; i < ntiles; i++) active[i] = stopped[i] == 0;
    }
    HIP_TRY(hipStreamSynchronize(st));
    if (samples_rendered) *samples_rendered = launched;
    return PT_OK;
}

// The host form: staging buffers around adaptive_device.
int adaptive_host(pt_renderer *r, const pt_camera *cam, uint32_t w, uint32_t h, uint32_t window, uint32_t min_samples,
                  uint32_t max_samples, double threshold, double luminance_floor, bool listed, uint32_t merge_gap,
                  uint64_t seed, double *rgb, double *variance, uint32_t *tile_samples, double *tile_error,
                  uint64_t *samples_rendered) {
    if (int rc = adaptive_refused(r, cam, w, h, window, min_samples, max_samples, threshold, luminance_floor, 0, 1,
                                  rgb, tile_samples))
        return rc;
    if (int rc = in_flight_refused(r)) return rc;
    HIP_TRY(hipSetDevice(r->device()));
    const size_t count = (size_t)w * h * 3, ntiles = shard_tiles(w, h, 0, 1);
    DevBuf<double> out, var, err, work;  // staging, freed on return
    DevBuf<uint32_t> ts;
    HIP_TRY(out.alloc(count));
    if (variance) HIP_TRY(var.alloc(count));
    if (tile_error) HIP_TRY(err.alloc(ntiles));
    HIP_TRY(ts.alloc(ntiles));
    HIP_TRY(work.alloc(adaptive_workspace_doubles(count)));
    uint64_t launched = 0;
    if (int rc = adaptive_device(r, cam, w, h, window, min_samples, max_samples, threshold, luminance_floor, listed,
                                 merge_gap, seed, 0, 1, out.p, var.p, ts.p, err.p, work.p, r->stream(), &launched))
        return rc;
    HIP_TRY(out.download(rgb));
    HIP_TRY(var.download(variance));
    HIP_TRY(ts.download(tile_samples));
    HIP_TRY(err.download(tile_error));
    if (samples_rendered) *samples_rendered = launched;
    return PT_OK;
}
}  // namespace

int pt_render_adaptive_device(pt_renderer *r, const pt_camera *cam, uint32_t w, uint32_t h, uint32_t window,
                              uint32_t min_samples, uint32_t max_samples, double threshold, double luminance_floor,
                              uint32_t merge_gap, uint64_t seed, uint32_t rank, uint32_t world, double *d_out,
                              double *d_variance, uint32_t *d_tile_samples, double *d_tile_error, double *d_work,
                              void *stream, uint64_t *samples_rendered) {
    return adaptive_device(r, cam, w, h, window, min_samples, max_samples, threshold, luminance_floor, false, merge_gap,
                           seed, rank, world, d_out, d_variance, d_tile_samples, d_tile_error, d_work, stream,
                           samples_rendered);
}

int pt_render_adaptive(pt_renderer *r, const pt_camera *cam, uint32_t w, uint32_t h, uint32_t window,
                       uint32_t min_samples, uint32_t max_samples, double threshold, double luminance_floor,
                       uint32_t merge_gap, uint64_t seed, double *rgb, double *variance, uint32_t *tile_samples,
                       double *tile_error, uint64_t *samples_rendered) {
    return adaptive_host(r, cam, w, h, window, min_samples, max_samples, threshold, luminance_floor, false, merge_gap,
                         seed, rgb, variance, tile_samples, tile_error, samples_rendered);
}

int pt_render_adaptive_list_device(pt_renderer *r, const pt_camera *cam, uint32_t w, uint32_t h, uint32_t window,
                                   uint32_t min_samples, uint32_t max_samples, double threshold,
                                   double luminance_floor, uint64_t seed, uint32_t rank, uint32_t world, double *d_out,
                                   double *d_variance, uint32_t *d_tile_samples, double *d_tile_error, double *d_work,
                                   void *stream, uint64_t *samples_rendered) {
    return adaptive_device(r, cam, w, h, window, min_samples, max_samples, threshold, luminance_floor, true, 0, seed,
                           rank, world, d_out, d_variance, d_tile_samples, d_tile_error, d_work, stream,
                           samples_rendered);
}

int pt_render_adaptive_list(pt_renderer *r, const pt_camera *cam, uint32_t w, uint32_t h, uint32_t window,
                            uint32_t min_samples, uint32_t max_samples, double threshold, double luminance_floor,
                            uint64_t seed, double *rgb, double *variance, uint32_t *tile_samples, double *tile_error,
                            uint64_t *samples_rendered) {
    return adaptive_host(r, cam, w, h, window, min_samples, max_samples, threshold, luminance_floor, true, 0, seed, rgb,
                         variance, tile_samples, tile_error, samples_rendered);
}

// ---------------------------------------------------------------- probes

int pt_closest_hit(pt_renderer *r, const double *rays, size_t n, double min_t, double max_t, pt_hit *out) {
    if (!r || (n && (!rays || !out))) return fail(PT_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(r->device()));
    DevBuf<double> dr;
    DevBuf<pt_hit> dh;
    HIP_TRY(dr.upload(rays, n * 6));
    HIP_TRY(dh.alloc(n));
    HIP_TRY(launch_closest_hit(r->gpus[0].ds, dr.p, n, min_t, max_t, dh.p, r->stream()));
    HIP_TRY(hipStreamSynchronize(r->stream()));
    HIP_TRY(dh.download(out));
    return PT_OK;
}

int pt_ray_color(pt_renderer *r, const double *rays, uint64_t *states, size_t n, uint32_t depth, double *out) {
    if (!r || (n && (!rays || !states || !out))) return fail(PT_ERR_INVALID, "null argument");
    if (int rc = depth_refused(depth)) return rc;
    HIP_TRY(hipSetDevice(r->device()));
    DevBuf<double> dr, dout;
    DevBuf<uint64_t> ds;
    HIP_TRY(dr.upload(rays, n * 6));
    HIP_TRY(ds.upload(states, n));
    HIP_TRY(dout.alloc(n * 3));
    HIP_TRY(launch_ray_color(r->gpus[0].ds, dr.p, ds.p, n, depth, r->s11, dout.p, r->stream()));
    HIP_TRY(hipStreamSynchronize(r->stream()));
    HIP_TRY(dout.download(out));
    HIP_TRY(ds.download(states));
    return PT_OK;
}

// the checks of the two probes that trace listed pixels, after their null checks
static int pixel_probe_refused(const pt_renderer *r, uint32_t w, uint32_t h, uint32_t spp, const uint32_t *pixels,
                               size_t n, const char *call) {
    if (int rc = frame_refused(w, h, spp)) return rc;
    for (size_t i = 0; i < n; i++)
        if (pixels[i] >= (uint64_t)w * h) return fail(PT_ERR_INVALID, "pixel index out of range");
    return reg_depth_refused(r->depth, call);
}

int pt_trace_pixel_samples(pt_renderer *r, const pt_camera *cam, uint32_t w, uint32_t h, uint32_t spp, uint64_t seed,
                           const uint32_t *pixels, size_t n, double *out) {
    if (!r || !cam || (n && (!pixels || !out))) return fail(PT_ERR_INVALID, "null argument");
    if (int rc = pixel_probe_refused(r, w, h, spp, pixels, n, "pt_trace_pixel_samples")) return rc;
    HIP_TRY(hipSetDevice(r->device()));
    FrameParams P = frame_params(r, *cam, w, h, spp, seed);
    DevBuf<uint32_t> dp;
    DevBuf<double> dout;
    HIP_TRY(dp.upload(pixels, n));
    HIP_TRY(dout.alloc(n * 3));
    HIP_TRY(launch_trace_pixels(r->gpus[0].ds, P, dp.p, n, dout.p, r->stream()));
    HIP_TRY(hipStreamSynchronize(r->stream()));
    HIP_TRY(dout.download(out));
    return PT_OK;
}

int pt_count_work(pt_renderer *r, const pt_camera *cam, uint32_t w, uint32_t h, uint32_t spp, uint64_t seed,
                  const uint32_t *pixels, size_t n, uint64_t *counters) {
    static_assert(C_COUNT == PT_NUM_COUNTERS, "counter list matches the header");
    if (!r || !cam || !counters || (n && !pixels)) return fail(PT_ERR_INVALID, "null argument");
    if (int rc = pixel_probe_refused(r, w, h, spp, pixels, n, "pt_count_work")) return rc;
    HIP_TRY(hipSetDevice(r->device()));
    FrameParams P = frame_params(r, *cam, w, h, spp, seed);
    DevBuf<uint32_t> dp;
    DevBuf<unsigned long long> dc;
    HIP_TRY(dp.upload(pixels, n));
    HIP_TRY(dc.alloc(C_COUNT));
    HIP_TRY(hipMemsetAsync(dc.p, 0, C_COUNT * sizeof(unsigned long long), r->stream()));
    HIP_TRY(launch_count_work(r->gpus[0].ds, P, dp.p, n, dc.p, r->stream()));
    HIP_TRY(hipStreamSynchronize(r->stream()));
    HIP_TRY(dc.download((unsigned long long *)counters));
    return PT_OK;
}

int pt_march_jobs(pt_renderer *r, const double *jobs, size_t n, double *t_out, int32_t *status, uint32_t *iters) {
    if (!r || (n && (!jobs || !t_out || !status || !iters))) return fail(PT_ERR_INVALID, "null argument");
    if (n == 0) return PT_OK;
    HIP_TRY(hipSetDevice(r->device()));
    DevBuf<double> dj, dt;
    DevBuf<int32_t> ds;
    DevBuf<uint32_t> di;
    HIP_TRY(dj.alloc(n * 8));
    HIP_TRY(dt.alloc(n));
    HIP_TRY(ds.alloc(n));
    HIP_TRY(di.alloc(n));
    HIP_TRY(hipMemcpyAsync(dj.p, jobs, n * 8 * sizeof(double), hipMemcpyHostToDevice, r->stream()));
    HIP_TRY(launch_march_probe(dj.p, n, dt.p, ds.p, di.p, r->stream()));
    HIP_TRY(hipMemcpyAsync(t_out, dt.p, n * sizeof(double), hipMemcpyDeviceToHost, r->stream()));
    HIP_TRY(hipMemcpyAsync(status, ds.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, r->stream()));
    HIP_TRY(hipMemcpyAsync(iters, di.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, r->stream()));
    HIP_TRY(hipStreamSynchronize(r->stream()));
    return PT_OK;
}

namespace {
// Device counters [first, first + n) of every device (init_share lists them), summed into out and cleared.
static int drain_counters(pt_renderer *r, int first, int n, uint64_t *out) {
    if (int rc = in_flight_refused(r)) return rc;
    unsigned long long c[2], total[2] = {0, 0};
    for (auto &g : r->gpus) {
        HIP_TRY(hipSetDevice(g.device));
        HIP_TRY(hipDeviceSynchronize());  // frames on any stream of the device
        HIP_TRY(hipMemcpy(c, g.ds.view.guard + first, n * sizeof *c, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemset(g.ds.view.guard + first, 0, n * sizeof *c));
        for (int k = 0; k < n; k++) total[k] += c[k];
    }
    for (int k = 0; k < n; k++) out[k] = total[k];
    return PT_OK;
}
}  // namespace

int pt_march_guard_drops(pt_renderer *r, uint64_t *count) {
    if (!r || !count) return fail(PT_ERR_INVALID, "null argument");
    return drain_counters(r, 0, 1, count);
}

int pt_render_stop_stats(pt_renderer *r, uint64_t *skipped, uint64_t *worked) {
    if (!r || !skipped || !worked) return fail(PT_ERR_INVALID, "null argument");
    uint64_t c[2];
    if (int rc = drain_counters(r, 1, 2, c)) return rc;
    *skipped = c[0];
    *worked = c[1];
    return PT_OK;
}

int pt_kernel_timing(pt_renderer *r, int enable, double *ms, uint32_t *launches, size_t nkinds) {
    if (!r) return fail(PT_ERR_INVALID, "null argument");
    // the band feeder pushes into the timer and may queue timed launches
    if (int rc = in_flight_refused(r)) return rc;
    HIP_TRY(hipSetDevice(r->device()));
    double m[K_KINDS];
    uint32_t l[K_KINDS];
    HIP_TRY(timer_collect(r->gpus[0].ws.timer, m, l));
    for (size_t k = 0; k < nkinds && k < (size_t)K_KINDS; k++) {
        if (ms) ms[k] = m[k];
        if (launches) launches[k] = l[k];
    }
    if (enable && !r->gpus[0].ws.timer) r->gpus[0].ws.timer = timer_new();
    if (!enable && r->gpus[0].ws.timer) {
        timer_free(r->gpus[0].ws.timer);
        r->gpus[0].ws.timer = nullptr;
    }
    return PT_OK;
}

int pt_wave_diag(pt_renderer *r, int enable, uint64_t *out, size_t n) {
    if (!r) return fail(PT_ERR_INVALID, "null argument");
    // the band feeder may queue launches that use the diag buffer
    if (int rc = in_flight_refused(r)) return rc;
    if (enable && !PT_WAVE_DIAG)
        return fail(PT_ERR_UNSUPPORTED, "wave diagnostics are compiled out of this build (make EXTRA=-DPT_WAVE_DIAG=1)");
    HIP_TRY(hipSetDevice(r->device()));
    HIP_TRY(hipStreamSynchronize(r->stream()));
    if (out && n && r->gpus[0].ws.diag) HIP_TRY(hipMemcpy(out, r->gpus[0].ws.diag, (n < 64 ? n : 64) * 8, hipMemcpyDeviceToHost));
    if (enable && !r->gpus[0].ws.diag) HIP_TRY(hipMalloc(&r->gpus[0].ws.diag, 64 * 8));
    if (r->gpus[0].ws.diag) HIP_TRY(hipMemset(r->gpus[0].ws.diag, 0, 64 * 8));
    if (!enable && r->gpus[0].ws.diag) {
        HIP_TRY(hipFree(r->gpus[0].ws.diag));
        r->gpus[0].ws.diag = nullptr;
    }
    return PT_OK;
}

int pt_profile_phases(pt_renderer *r, const pt_camera *cam, uint32_t w, uint32_t h, uint32_t spp, uint64_t seed,
                      uint64_t *out) {
    if (!r || !cam || !out) return fail(PT_ERR_INVALID, "null argument");
    if (r->depth > 8) return fail(PT_ERR_UNSUPPORTED, "phase profiling supports depth <= 8");
    HIP_TRY(hipSetDevice(r->device()));
    const FrameParams P = shard_params(r, *cam, w, h, spp, seed, 0, 1);
    DevBuf<double> frame;
    DevBuf<unsigned long long> acc;
    HIP_TRY(frame.alloc((size_t)w * h * 3));
    HIP_TRY(acc.alloc(10));
    HIP_TRY(hipMemsetAsync(acc.p, 0, 10 * sizeof(unsigned long long), r->stream()));
    HIP_TRY(launch_render_timed(r->gpus[0].ds, P, frame.p, acc.p, r->stream()));
    HIP_TRY(hipStreamSynchronize(r->stream()));
    HIP_TRY(hipMemcpy(out, acc.p, 10 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return PT_OK;
}

// Display encode (src/bin/main.rs:281-289): f64::clamp keeps NaN, `as u8`
// saturates NaN to 0.
int pt_encode_rgba8(const double *rgb, size_t npix, uint8_t *rgba) {
    if (npix && (!rgb || !rgba)) return fail(PT_ERR_INVALID, "null argument");
    for (size_t i = 0; i < npix; i++) {
        for (int c = 0; c < 3; c++) {
            double v = std::sqrt(rgb[i * 3 + c]);
            if (v < 0.0) v = 0.0;
            if (v > 0.999) v = 0.999;
            double s = v * 256.0;
            rgba[i * 4 + c] = std::isnan(s) ? 0 : (uint8_t)s;
        }
        rgba[i * 4 + 3] = 255;
    }
    return PT_OK;
}

}  // extern "C"
