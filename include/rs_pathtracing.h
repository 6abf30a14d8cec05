/*
 * rs_pathtracing.h — C-ABI boundary of the MI355X-native path-tracing sample loop.
 *
 * This is what the reference's Rust host would bind with `extern "C"` to
 * replace its CPU renderer (INTEGRATION.md shows the binding).  Each entry
 * point names the reference interface it replaces (paths relative to the
 * dkarpushkin/rs-pathtracing checkout).  Plain pointers and sizes only; no
 * exception or abort crosses this boundary: every call returns a status
 * (PT_OK = 0, negative = error) and pt_last_error() gives the message of the
 * last failing call on the calling thread.
 *
 * Buffers: colour buffers are `Vec<Vector3d>` laid out as w*h*3 doubles,
 * row-major, index x + y*w, y = 0 at the top (src/camera/ray_caster.rs:35),
 * linear radiance (no gamma, no clamp) — the buffer render_step fills in
 * src/renderer/step_by_step.rs:115-117.
 */
#ifndef RS_PATHTRACING_H
#define RS_PATHTRACING_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PT_OK 0
#define PT_ERR_INVALID -1     /* bad argument / unknown material name           */
#define PT_ERR_PARSE -2       /* JSON syntax or schema (serde_json::Error)        */
#define PT_ERR_UNSUPPORTED -3 /* valid reference JSON the GPU path does not take  */
#define PT_ERR_HIP -4         /* HIP runtime failure                               */
#define PT_ERR_STATE -5       /* call out of order (e.g. step before start)       */
#define PT_ERR_IO -6          /* unreadable / corrupt file (pt_checkpoint_load)   */

/* shape kinds */
#define PT_SPHERE 0    /* src/world/shapes/mod.rs:304-399 */
#define PT_RECTANGLE 1 /* src/world/shapes/mod.rs:150-221 */
#define PT_CUBE 2      /* src/world/shapes/mod.rs:223-302 */
#define PT_MARCH 3     /* RayMarchingShape, src/world/shapes/ray_marching.rs:10-110 */
#define PT_TORUS 4     /* src/world/shapes/mod.rs:400-494 */
#define PT_FUNC_HEART 0 /* ShapeFunctions, ray_marching.rs:121-520 */
#define PT_FUNC_SINE 1
#define PT_FUNC_STAR 2
#define PT_FUNC_DUPIN_CYCLIDE 3
#define PT_FUNC_HUNTS_SURFACE 4
#define PT_FUNC_CUSHION 5

/* material kinds (src/world/material.rs) */
#define PT_LAMBERTIAN 0
#define PT_METAL 1
#define PT_DIELECTRIC 2
#define PT_DIFFUSE_LIGHT 3
#define PT_EMPTY 4

typedef struct pt_scene pt_scene;
typedef struct pt_renderer pt_renderer;

/* Scene::from_json options.  The reference appends ~480 spheres drawn from an
 * unseeded thread_rng (src/world/json_models.rs:44, 50-133); here the draw is
 * seeded so a scene is reproducible, and it can be switched off. */
/* ImageTexture decoding: the reference calls image::open(image_filename) and
 * into_rgba8() at deserialization (src/world/texture.rs:119-130).  A loader
 * returns PT_OK with a width x height RGBA8 row-major buffer that stays valid
 * until pt_scene_create_from_json returns (the library copies it), or
 * PT_ERR_UNSUPPORTED to decline the file.  Without a loader, or for a
 * declined file, the built-in reader takes binary PPM (P6, maxval 255). */
typedef int (*pt_image_loader)(void *user, const char *filename, uint32_t *width, uint32_t *height,
                               const uint8_t **rgba8);

/* The struct is versioned by struct_size, which the library honours: it reads
 * no byte at or past opts + struct_size.  A caller sets struct_size =
 * sizeof(pt_scene_opts) of the header it was compiled against (or uses
 * PT_SCENE_OPTS_INIT).  struct_size == 0 is a caller built against 0.1.0 or
 * 0.2.0, where this field was `reserved` (always 0): 0.1.0's struct was the 16
 * bytes {random_spheres, reserved, seed}, 0.2.0's added load_image and
 * image_user, and a 0 cannot tell the two apart, so 0 reads the 16 bytes both
 * have and never a loader (ABI version 4; a 0.2.0 caller's ImageTexture files
 * then go to the built-in PPM reader).  An image loader is used only with a
 * struct_size that covers it.  A size between 1 and 15 is rejected
 * (PT_ERR_INVALID); a size of 16 to 31 reads only the fields it covers (16: no
 * loader); fields a newer caller appends past sizeof(pt_scene_opts) are
 * ignored. */
typedef struct {
    uint32_t random_spheres; /* 1 = reference behaviour (default), 0 = JSON shapes only */
    uint32_t struct_size;    /* sizeof(pt_scene_opts); 0 = a 0.1.0 / 0.2.0 caller: its first 16 bytes only */
    uint64_t seed; /* seed of the add_random_spheres stream and of the NoiseTexture Perlin tables */
    pt_image_loader load_image; /* NULL: built-in PPM reader (read only if struct_size covers it) */
    void *image_user;
} pt_scene_opts;
#define PT_SCENE_OPTS_MIN_SIZE 16    /* {random_spheres, struct_size, seed} */
#define PT_SCENE_OPTS_LEGACY_SIZE 16 /* what struct_size == 0 means: the bytes 0.1.0 and 0.2.0 structs share */
#define PT_SCENE_OPTS_INIT {1u, (uint32_t)sizeof(pt_scene_opts), 1u, NULL, NULL}

/* Camera (src/camera/mod.rs:36-46).  fov in radians, as Camera::new takes it. */
typedef struct {
    double position[3], direction[3], up[3], right[3];
    double fov, focal_length;
} pt_camera;

/* Realized shape record (introspection / parity).  Matrices are 4x4 row-major. */
typedef struct {
    int32_t type, material, inverse_normal, depth, func, pad0;
    double direct[16], inverse[16];
    double x0, y0, x1, y1, step;
    double a, b, c, d, sphere_radius; /* ray-marched function parameters (JSON) */
    double radius, tube_radius;       /* Torus */
} pt_shape_info;

typedef struct {
    int32_t type;
    int32_t texture; /* -1: SolidColor (albedo / emit hold it); else the root of a non-solid texture */
    double albedo[3];
    double fuzz, ior;
    double emit[3];
} pt_material_info;

/* RayHit (src/world/ray.rs:21-29) for the closest_hit probe. */
typedef struct {
    double t;
    double point[3];
    double normal[3];
    int32_t front_face, shape, material, pad0;
} pt_hit;

/* ---- scene: Scene::from_json (src/world/mod.rs:46-49) ------------------ */
int pt_scene_create_from_json(const char *json, size_t len, const pt_scene_opts *opts, pt_scene **out);
void pt_scene_destroy(pt_scene *scene);
/* Scene::camera (src/world/mod.rs:193-197) */
int pt_scene_camera(const pt_scene *scene, pt_camera *out);
int pt_scene_num_shapes(const pt_scene *scene);
int pt_scene_get_shape(const pt_scene *scene, int index, pt_shape_info *out);
int pt_scene_num_materials(const pt_scene *scene);
int pt_scene_get_material(const pt_scene *scene, int index, pt_material_info *out);

/* Camera::new (src/camera/mod.rs:71-88) */
int pt_camera_new(const double position[3], const double direction[3], const double up[3],
                  double focal_length, double fov_radians, pt_camera *out);

/* ---- renderer: trait Renderer (src/renderer/mod.rs:47-56) -------------- */
/* ThreadPoolRenderer::new(scene, thread_number, depth)
 * (src/renderer/step_by_step.rs:37): `device` (HIP ordinal, -1 = current)
 * replaces thread_number.  The scene must outlive the renderer.
 * depth: any value up to PT_MAX_DEPTH, as the reference takes any u32 (its
 * own recursion does not survive arbitrarily large ones); above it the create
 * calls return PT_ERR_UNSUPPORTED with a message naming the limit.  A frame
 * of depth > 64 always runs the wavefront engine's generic kernels and keeps
 * (depth + 1) * 4 bytes of id stack per path in flight ((depth + 1) * 28 in a
 * textured scene); when the device's free memory cannot hold that workspace
 * even at the smallest chunks on one stream, the render call returns PT_ERR_UNSUPPORTED
 * and pt_last_error says what was needed and what was available. */
#define PT_MAX_DEPTH 4096
int pt_renderer_create(pt_scene *scene, int device, uint32_t depth, pt_renderer **out);
/* The same constructor with the parallelism knob spread over GPUs (the
 * thread_number of step_by_step.rs:37 -> ngpu): devices[0..ngpu) are HIP
 * ordinals (NULL: 0 .. ngpu-1; ngpu <= 0 with NULL devices: every visible
 * device; an ordinal may repeat, e.g. to rehearse the deal on one GPU).
 * Each device gets its own copy of the scene and its own stream.  A frame's
 * 16x16 tiles are dealt to the devices as to the ranks of pt_render_device
 * (logical tile k -> device k % ngpu, diagonal deal); each device renders
 * its tiles into a compact shard, the shards are copied to devices[0] over
 * the peer link (xGMI) and un-interleaved there.  render_start / render_step
 * / stop_rendering then drive all devices; the frame is bit-identical to a
 * one-device render (the RNG is keyed per (pixel, sample)). */
int pt_renderer_create_multi(pt_scene *scene, const int *devices, int ngpu, uint32_t depth, pt_renderer **out);
int pt_renderer_num_devices(const pt_renderer *r);
/* Peer access of a multi-device renderer.  Create enables it both ways
 * between devices[0] and every other distinct device that can reach it
 * (hipDeviceCanAccessPeer, then hipDeviceEnablePeerAccess; "already enabled"
 * counts as enabled), so the shard copies go device to device over xGMI.  A
 * pair that cannot be enabled still works: hipMemcpyPeerAsync stages it.
 * *pairs = distinct (devices[0], devices[k]) pairs, *enabled = those with
 * peer access on both ways.  A repeated ordinal is no pair. */
int pt_renderer_peer_access(const pt_renderer *r, int *pairs, int *enabled);
/* Tuning knobs of the render engines (not part of the reference; defaults are
 * the measured optimum): "engine" (0 auto, 1 megakernel,
 * 2 wavefront), "mega_waves", "diag", "wf_slots", "wf_paths", "wf_min_chunks",
 * "wf_bounce_waves", "wf_march_slice", "wf_walk", "bvh_leaf" (shapes per BVH
 * leaf: setting it rebuilds the BVH on every device).  (ABI 4's
 * "wf_march_blocks_per_cu", "wf_side_priority", "wf_pingpong", "wf_stagger"
 * and "wf_tail_paths" were measured slower and removed; setting one is
 * PT_ERR_INVALID.)  A new renderer
 * starts from the defaults; set_option changes them for every device of the
 * renderer (not while a render_start frame is in flight).  No knob changes the
 * image: every setting renders the same bits.  pt_option_name(i) lists the
 * names (NULL past the end).  get_option also reads "bvh_nodes" (read-only:
 * nodes per octant layout of the renderer's BVH; from 32768 on, the bounce
 * runs its large-tree build, whose node slab test is f32), and what the
 * renderer's first device launched for its last frame, set where the launch
 * is made (read-only as well; set_option refuses the names): "ran_engine"
 * (0 megakernel, 1 wavefront, -1 nothing launched yet or the call refused)
 * and "ran_mega", "ran_bounce", "ran_walk", "ran_march" (-1: the frame
 * launched none of that kernel; else the kernel build's template arguments
 * as sum((argument + 2) << (6 * position)), in the order of pt_builds.hpp's
 * lists of builds).  "first_cull_bits" (read-only too) is
 * the number of set bits over the first bounce launch's cull table of that
 * frame (one mask per 8x8 pixel block), read once the frame
 * is done; -1: the frame used no table. */
int pt_renderer_set_option(pt_renderer *r, const char *name, int64_t value);
int pt_renderer_get_option(const pt_renderer *r, const char *name, int64_t *value);
const char *pt_option_name(int index);
void pt_renderer_destroy(pt_renderer *r);
/* Renderer::start_rendering (mod.rs:48-53): queues the whole frame on the
 * GPU(s), in ~8 bands of tile rows, and returns at once.  seed keys the
 * per-(pixel, sample) RNG stream.  A frame still in flight is stopped first
 * (the GUI calls stop_rendering before every start, src/bin/main.rs:268). */
int pt_render_start(pt_renderer *r, const pt_camera *camera, uint32_t width, uint32_t height,
                    uint32_t samples_number, uint64_t seed);
/* Renderer::render_step (mod.rs:54): copies every finished band of rows into
 * rgb (w*h*3 doubles) and returns 1 once the frame is complete, 0 while work
 * is pending (blocking = 0, step_by_step.rs:101-121 semantics), or blocks
 * until done (blocking = 1, thread_pool_new.rs:96-126 semantics). */
int pt_render_step(pt_renderer *r, double *rgb, int blocking);
/* render_step plus the GUI's display encode (src/bin/main.rs:281-289), done on
 * the GPU right after each band: rgba (w*h*4 bytes, R G B A per pixel) gets
 * the encoded rows of every finished band; rgb (may be NULL) the linear ones.
 * Same return values as pt_render_step. */
int pt_render_step_rgba8(pt_renderer *r, double *rgb, uint8_t *rgba, int blocking);
/* Renderer::stop_rendering (mod.rs:55): the frame in flight is abandoned.  No
 * further band is queued, and the renderer's stop flag (host-mapped, read at
 * each sample chunk's start and after each compaction) turns the launches
 * already queued into no-ops; the call returns once the device streams are
 * idle, i.e. after
 * the kernels that were running when it was called (milliseconds, not the
 * seconds two whole bands take at 4K x 4096 spp).  Bands already copied by
 * render_step stay valid; the rest of the buffer is not written.  Frames
 * queued by pt_render_device / pt_render_frame_device are not affected. */
int pt_render_stop(pt_renderer *r);

/* ---- device-resident frame (benchmarks, multi-GPU) --------------------- */
/* Renders this rank's share of the frame straight into device memory on
 * `hip_stream` (a hipStream_t; 0 = the null stream, as in every HIP call and
 * in pt_unshard_device), on the renderer's first device.  Pixels are cut into
 * 16x16 tiles; logical tile k belongs to rank k % world and sits in
 * tile row k / tiles_x at column (k % tiles_x + row) % tiles_x (a diagonal
 * deal, so a rank's columns change from row to row).  world == 1: d_out is
 * the w*h*3 frame.  world > 1: d_out holds this rank's tiles in order,
 * pt_shard_tiles(...) * 256 * 3 doubles (pixels outside the frame are 0). */
int pt_render_device(pt_renderer *r, const pt_camera *camera, uint32_t width, uint32_t height,
                     uint32_t samples_number, uint64_t seed, uint32_t rank, uint32_t world,
                     double *d_out, void *hip_stream);
/* The whole frame over all of the renderer's devices (pt_renderer_create_multi)
 * into d_frame (w*h*3 doubles on the first device), ordered after the work
 * queued on hip_stream (a stream of the first device; 0 = null stream), which
 * resumes once d_frame holds the frame.  Not while a render_start frame is in
 * flight (PT_ERR_STATE). */
int pt_render_frame_device(pt_renderer *r, const pt_camera *camera, uint32_t width, uint32_t height,
                           uint32_t samples_number, uint64_t seed, double *d_frame, void *hip_stream);
uint32_t pt_shard_tiles(uint32_t width, uint32_t height, uint32_t rank, uint32_t world);
/* Rebuild the frame from `world` gathered shard buffers laid out back to back,
 * each padded to pt_shard_tiles(w, h, 0, world) tiles, on HIP device `device`
 * (-1 = the calling thread's current device) and its stream hip_stream.
 * (ABI version 3 added the leading `device`; see PT_ABI_VERSION.) */
int pt_unshard_device(int device, const double *d_gathered, uint32_t width, uint32_t height, uint32_t world,
                      double *d_frame, void *hip_stream);

/* ---- first-hit guide planes (albedo, normal, depth) ---------------------- */
/* What a denoiser, a compositor or a debugger wants beside the beauty frame
 * (the reference renders none): the first hit of every camera sample of the
 * frame (camera, width, height, samples_number, seed).  Sample s of pixel
 * p = x + y*width is the primary ray of the beauty frame's sample s (its RNG
 * key is pt_sample_key(seed, p, s); the camera draws u, then v), so the
 * planes carry the frame's own jitter.  Each plane is width*height*3 doubles
 * laid out like the colour buffer; each value is the in-order sum over the
 * samples divided by samples_number once.
 *   albedo: the first hit's colour.  Lambertian, Metal: the albedo (its
 *     texture's value at the hit).  Dielectric: (1, 1, 1).  DiffuseLight: its
 *     emit (or texture value), NOT clamped (a caller that wants [0, 1]
 *     clamps).  EmptyMaterial: (0, 0, 0).  A miss: the background colour.
 *   normal: the world normal of pt_hit (unit, turned against the ray); a miss
 *     adds (0, 0, 0); the mean is not renormalised.
 *   depth: [0] sum of t over the hitting samples / samples_number (t is the
 *     world distance: directions are unit), [1] hits / samples_number (the
 *     coverage), [2] the smallest t of the hitting samples, 0 when none hits.
 * A pass of its own, independent of the renderer's depth, options and
 * workspace; PT_ERR_INVALID when all planes are NULL, a size or
 * samples_number is 0 or rank >= world; PT_ERR_STATE while a render_start
 * frame is in flight.  (Library 0.4.3; no ABI change.) */
/* First-hit guide planes of the frame pt_render_device(..., samples_number, seed, rank, world, ...) renders:
 * same tiles, same shard layout, same per-sample camera rays.  Any of the three device pointers may be NULL
 * (not all).  Queued on hip_stream on the renderer's first device; independent of the renderer's depth. */
int pt_render_aov_device(pt_renderer *r, const pt_camera *camera, uint32_t width, uint32_t height,
                         uint32_t samples_number, uint64_t seed, uint32_t rank, uint32_t world,
                         double *d_albedo, double *d_normal, double *d_depth, void *hip_stream);
/* The whole frame's planes into host buffers (w*h*3 doubles each, any may be NULL, not all); blocks. */
int pt_render_aov(pt_renderer *r, const pt_camera *camera, uint32_t width, uint32_t height,
                  uint32_t samples_number, uint64_t seed, double *albedo, double *normal, double *depth);

/* ---- guided denoiser for the beauty frame and its guide planes ---------- */
/* An edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) over a whole
 * frame (world == 1 layout: width*height*3 doubles each, all finite): the
 * colour, and the albedo, normal and depth planes of pt_render_aov (of depth
 * only [0], the mean t, is read).  f64, no transcendental function, sums in a
 * fixed order: the result is the same bits on every run and equals the numpy
 * restatement in tests/denoiseref.py.  The filter, step by step, is in
 * rs-pathtracing_amd/csrc/pt_denoise.hpp and DESIGN.md 3.8: the colour is
 * divided by the albedo (PT_DENOISE_DEMODULATE; a channel <= 1e-3 divides by
 * 1), filtered `iterations` times with a 5x5 kernel at strides 1, 2, 4, ...
 * whose taps are weighted by the distance of normals (sigma_normal), of depth
 * relative to the pixel's own (sigma_depth) and, when sigma_colour > 0, of
 * the filtered colours (sigma_colour / stride), and multiplied by the albedo
 * again.
 * Defaults: 5 iterations, sigma_normal 0.5, sigma_depth 0.1, sigma_colour 0,
 * flags PT_DENOISE_DEMODULATE.  sigma_colour 0 switches the colour term off,
 * and it is off by default: without a variance estimate it keeps a 4-spp
 * frame's fireflies.  +inf is a legal sigma and means that term weighs 1.
 * d_out == d_rgb is allowed; no other overlap is.  d_albedo may be NULL only
 * without PT_DENOISE_DEMODULATE.  PT_ERR_INVALID: a NULL required pointer, a
 * zero size, iterations outside 1..PT_DENOISE_MAX_ITERATIONS, an unknown flag
 * bit, sigma_normal or sigma_depth not greater than 0 or NaN, sigma_colour
 * below 0 or NaN, a d_work that is not 16-byte aligned, a frame of more than
 * 2^31 - 1 tiles of 16x16.  A refused call writes nothing.  Sharded frames
 * (world > 1) are denoised after pt_unshard_device.  (Library 0.4.3; no ABI
 * change.) */
#define PT_DENOISE_DEMODULATE 1u
#define PT_DENOISE_MAX_ITERATIONS 8
/* doubles of device workspace pt_denoise_device needs for a width x height frame (0 if either is 0) */
size_t pt_denoise_workspace_doubles(uint32_t width, uint32_t height);
/* queued on hip_stream of HIP device `device` (-1 = current), like pt_encode_rgba8_device; needs no renderer */
int pt_denoise_device(int device, const double *d_rgb, const double *d_albedo, const double *d_normal,
                      const double *d_depth, uint32_t width, uint32_t height, uint32_t iterations,
                      double sigma_normal, double sigma_depth, double sigma_colour, uint32_t flags,
                      double *d_out, double *d_work, void *hip_stream);
/* the same from and to host buffers; allocates, copies, blocks */
int pt_denoise(int device, const double *rgb, const double *albedo, const double *normal, const double *depth,
               uint32_t width, uint32_t height, uint32_t iterations, double sigma_normal, double sigma_depth,
               double sigma_colour, uint32_t flags, double *out);

/* ---- temporal accumulation: the last frame reprojected into a moved camera ---- */
/* For a caller whose camera moves a little from frame to frame (an orbiting
 * viewer at 1 spp): instead of starting every frame from nothing, the
 * accumulated frame of the previous camera is reprojected into the new one
 * through the new frame's first-hit distance, rejected where the geometry
 * disagrees, and the new frame is blended in, so the denoiser that follows
 * sees the samples of many frames.  All frames are in the colour buffer's
 * layout (world == 1: width*height*3 doubles each, all finite): the colour,
 * and the normal and depth planes of pt_render_aov for the same camera (of
 * depth, [0] and [1] are read: their quotient is the mean hit distance).
 * The history is pt_temporal_history_doubles(width, height) = width*height*8
 * doubles, 16-byte aligned: two 32-byte records per pixel p = x + y*width,
 * first all colour records, then all guide records:
 *   colour record {h0, h1, h2, n}: the accumulated colour and the number of
 *     frames it stands for (a double, at least 1 once written);
 *   guide record {m0, m1, m2, z}: the normal plane's value and the hit
 *     distance of the frame that wrote it; z = 0 for a pixel with no hit.
 * A call reads history_in (written by the call for prev_camera) and writes
 * history_out; a caller keeps two and swaps them.  history_in == NULL together
 * with prev_camera == NULL is the first frame: every pixel starts at n = 1.
 * Per pixel: the point the centre ray hits at the mean hit distance is
 * projected into prev_camera; the four history pixels around it are weighted
 * bilinearly (a position within 1/1024 of a pixel centre takes that pixel
 * alone, so a still camera accumulates without blur); a tap counts only if
 * its normal lies within sigma_normal of the new one and its hit distance
 * within sigma_depth, relative, of the point's distance to prev_camera; the
 * new colour is blended in with weight 1/n, n = the taps' count + 1 capped at
 * max_count.  A pixel with no hit, a point behind or outside prev_camera's
 * frame, or no counting tap starts again at n = 1.  f64, no transcendental
 * function, one fixed order: the same bits on every run, equal to the numpy
 * restatement in tests/temporalref.py.  Step by step:
 * rs-pathtracing_amd/csrc/pt_temporal.hpp and DESIGN.md 3.12.
 * Defaults: max_count 32, sigma_normal 0.5, sigma_depth 0.1; +inf is a legal
 * sigma and means that test always passes.  d_out (the accumulated frame,
 * equal to the colour records) may be d_rgb; history_in and history_out must
 * not overlap.  PT_ERR_INVALID, the call writing nothing: a NULL required
 * pointer, a zero size, max_count 0, a sigma not greater than 0 or NaN,
 * exactly one of prev_camera and history_in NULL, a device history pointer
 * that is not 16-byte aligned, history_in overlapping history_out, a frame of
 * more than 2^31 - 1 tiles of 16x16.  Objects that move, sky pixels and
 * sharded frames (accumulate after pt_unshard_device) are not handled.
 * (Library 0.4.3; no ABI change.) */
/* doubles of one history buffer for a width x height frame (0 if either is 0) */
size_t pt_temporal_history_doubles(uint32_t width, uint32_t height);
/* queued on hip_stream of HIP device `device` (-1 = current), like pt_denoise_device; needs no renderer */
int pt_temporal_device(int device, const double *d_rgb, const double *d_normal, const double *d_depth,
                       const pt_camera *camera, const pt_camera *prev_camera, uint32_t width, uint32_t height,
                       const double *d_history_in, double *d_history_out, uint32_t max_count,
                       double sigma_normal, double sigma_depth, double *d_out, void *hip_stream);
/* the same from and to host buffers (the histories too); allocates, copies, blocks */
int pt_temporal(int device, const double *rgb, const double *normal, const double *depth,
                const pt_camera *camera, const pt_camera *prev_camera, uint32_t width, uint32_t height,
                const double *history_in, double *history_out, uint32_t max_count,
                double sigma_normal, double sigma_depth, double *out);

/* ---- per-pixel variance from sample windows, and the denoiser's variance term ---- */
/* How far a frame is from converged, per pixel and channel: the variance of the
 * pixel's mean (its square root is the standard error), estimated by batch
 * means from the frame's own sample windows.  pt_render_device_samples leaves
 * running sums in d_out between windows; pt_variance_window_device, run on
 * d_out right after window `window` of `windows` (1-based; the first when 1,
 * the last when it equals windows), differences them.  Window k covers samples
 * [e_{k-1}, e_k), e_k = (uint64_t)k * samples_number / windows, n_k = e_k -
 * e_{k-1}.  d_work holds pt_variance_workspace_doubles doubles (2 * count; the
 * first window overwrites them, they need not be cleared) and must be kept
 * between the windows of one frame; d_variance (count doubles, d_out's layout,
 * the shard layout included; a padding element is 0) is written only by the
 * last window, yet must be given on every call.  count is width*height*3 when
 * world == 1, else pt_shard_tiles(...) * 768.  The arithmetic, step by step,
 * is in rs-pathtracing_amd/csrc/pt_variance.hpp and DESIGN.md 3.9: f64, one
 * fixed order, bit for bit the numpy restatement in tests/varianceref.py.
 * pt_render_variance_device queues the whole frame: the windows through
 * pt_render_device_samples, each followed by its accumulate launch, with no
 * host synchronisation of its own; d_out ends bit-identical to
 * pt_render_device's.  pt_denoise_variance_device is pt_denoise_device with,
 * in place of the colour term, a luminance weight scaled by each pixel's own
 * variance (d_variance: the plane above, of a whole frame), so it backs off
 * where the frame has converged; sigma_variance (8 is the recommended default)
 * = +inf weighs 1 and gives pt_denoise_device's frame at sigma_colour 0 bit
 * for bit.  Same workspace as pt_denoise_device.  PT_ERR_INVALID, the call
 * writing nothing: a NULL pointer (d_albedo alone may be NULL without
 * PT_DENOISE_DEMODULATE), a zero size, windows < 2 or > samples_number, window
 * outside 1..windows, n_k outside 1..samples_number, rank >= world (or a rank
 * that holds no tile), sigma_variance not greater than 0 or NaN, and
 * pt_denoise_device's cases.  PT_ERR_STATE while a pt_render_start frame is
 * in flight.  The accumulation state is not checkpointed.  (Library 0.4.3; no
 * ABI change.) */
/* 2 * count; 0 on a zero size or rank >= world */
size_t pt_variance_workspace_doubles(uint32_t width, uint32_t height, uint32_t rank, uint32_t world);
int pt_variance_window_device(int device, const double *d_out, size_t count, uint32_t n_k, uint32_t samples_number,
                              uint32_t window, uint32_t windows, double *d_work, double *d_variance,
                              void *hip_stream);
int pt_render_variance_device(pt_renderer *r, const pt_camera *camera, uint32_t width, uint32_t height,
                              uint32_t samples_number, uint64_t seed, uint32_t rank, uint32_t world,
                              uint32_t windows, double *d_out, double *d_variance, double *d_work,
                              void *hip_stream);
/* the same into host buffers (world 1); allocates, copies, blocks */
int pt_render_variance(pt_renderer *r, const pt_camera *camera, uint32_t width, uint32_t height,
                       uint32_t samples_number, uint64_t seed, uint32_t windows, double *rgb, double *variance);
int pt_denoise_variance_device(int device, const double *d_rgb, const double *d_albedo, const double *d_normal,
                               const double *d_depth, const double *d_variance, uint32_t width, uint32_t height,
                               uint32_t iterations, double sigma_normal, double sigma_depth, double sigma_variance,
                               uint32_t flags, double *d_out, double *d_work, void *hip_stream);
/* the same from and to host buffers; allocates, copies, blocks */
int pt_denoise_variance(int device, const double *rgb, const double *albedo, const double *normal,
                        const double *depth, const double *variance, uint32_t width, uint32_t height,
                        uint32_t iterations, double sigma_normal, double sigma_depth, double sigma_variance,
                        uint32_t flags, double *out);

/* ---- adaptive sampling: every 16x16 tile stops at a noise target ---------- */
/* The frame is rendered in sample windows of `window` samples, up to
 * max_samples (the last window may be short; max_samples > window, so there
 * are two windows at least).  After each window every tile that is still
 * active is judged from the windows' running sums: the batch-means variance of
 * each pixel's mean (the estimate of pt_render_variance), summed over the tile
 * as the variance of its luminance, against the tile's mean luminance floored
 * at luminance_floor.  A tile stops when that relative standard error is at
 * most `threshold`, at the second window and e_k >= min_samples at the
 * earliest, or when it reaches max_samples; its pixels then are, bit for bit,
 * those of pt_render_device's frame at the tile's own sample count, and the
 * tile is neither rendered nor written again.  threshold 0 runs every tile
 * that is not constant to max_samples; +inf stops every tile at the first
 * evaluation.  The arithmetic, step by step, is in
 * rs-pathtracing_amd/csrc/pt_adaptive.hpp and DESIGN.md 3.10: f64, one fixed
 * order, bit for bit the numpy restatement in tests/adaptiveref.py.
 * d_out and d_variance (may be NULL; the variance of each element's mean at
 * the tile's sample count) have pt_render_device's layout, the shard layout
 * included (a padding element is 0); d_tile_samples (and d_tile_error, may be
 * NULL: the squared relative standard error the tile stopped with) have
 * pt_shard_tiles(width, height, rank, world) entries in the rank's tile order;
 * d_work holds pt_adaptive_workspace_doubles doubles (3 * count, count as for
 * pt_variance_workspace_doubles; need not be cleared), 16-byte aligned.
 * Between windows the still-active tiles are grouped into runs, one render
 * launch each; runs with at most merge_gap stopped tiles between them are
 * joined (their stopped tiles are rendered again and ignored: the frame does
 * not depend on merge_gap, only the time does).  samples_rendered (may be
 * NULL) receives the pixel-samples launched, that waste included.  The call
 * blocks: it synchronises hip_stream once per window, because the host picks
 * the next launches.  Recommended: window 8, min_samples 0, luminance_floor
 * 0.01, merge_gap 1024.  PT_ERR_INVALID, the call writing nothing: a NULL
 * required pointer, a zero size or window, max_samples <= window or above
 * 2^32 - 2, min_samples > max_samples, threshold or luminance_floor negative
 * or NaN, rank >= world (or a rank that holds no tile), a misaligned
 * workspace.  PT_ERR_STATE while a pt_render_start frame is in flight.  The
 * accumulation state is not checkpointed.  Stopping on a variance estimated
 * from the same samples biases the frame slightly dark where bright paths
 * are rare.  (Library 0.4.3; no ABI change.) */
#define PT_ADAPTIVE_WINDOW 8            /* the recommended defaults (Python's and pt_render's) */
#define PT_ADAPTIVE_LUMINANCE_FLOOR 0.01
#define PT_ADAPTIVE_MERGE_GAP 1024
/* 3 * count; 0 on a zero size or rank >= world */
size_t pt_adaptive_workspace_doubles(uint32_t width, uint32_t height, uint32_t rank, uint32_t world);
int pt_render_adaptive_device(pt_renderer *r, const pt_camera *camera, uint32_t width, uint32_t height,
                              uint32_t window, uint32_t min_samples, uint32_t max_samples, double threshold,
                              double luminance_floor, uint32_t merge_gap, uint64_t seed, uint32_t rank,
                              uint32_t world, double *d_out, double *d_variance, uint32_t *d_tile_samples,
                              double *d_tile_error, double *d_work, void *hip_stream, uint64_t *samples_rendered);
/* the same into host buffers (world 1); allocates, copies, blocks */
int pt_render_adaptive(pt_renderer *r, const pt_camera *camera, uint32_t width, uint32_t height, uint32_t window,
                       uint32_t min_samples, uint32_t max_samples, double threshold, double luminance_floor,
                       uint32_t merge_gap, uint64_t seed, double *rgb, double *variance, uint32_t *tile_samples,
                       double *tile_error, uint64_t *samples_rendered);
/* The same frame with each window rendered in ONE launch over the list of the
 * still-active tiles (pt_render_device_tiles) instead of one launch per run:
 * pt_render_adaptive_device's parameters without merge_gap.  d_out,
 * d_variance, d_tile_samples and d_tile_error are bit for bit those of
 * pt_render_adaptive_device (the frame never depended on merge_gap);
 * samples_rendered is exactly the sum over the tiles of pixels * tile_samples:
 * no stopped tile is rendered again.  The same errors, the same blocking once
 * per window, the same workspace (the list is kept by the renderer, not in
 * d_work).  (Library 0.4.3; no ABI change.) */
int pt_render_adaptive_list_device(pt_renderer *r, const pt_camera *camera, uint32_t width, uint32_t height,
                                   uint32_t window, uint32_t min_samples, uint32_t max_samples, double threshold,
                                   double luminance_floor, uint64_t seed, uint32_t rank, uint32_t world,
                                   double *d_out, double *d_variance, uint32_t *d_tile_samples, double *d_tile_error,
                                   double *d_work, void *hip_stream, uint64_t *samples_rendered);
/* the same into host buffers (world 1); allocates, copies, blocks */
int pt_render_adaptive_list(pt_renderer *r, const pt_camera *camera, uint32_t width, uint32_t height,
                            uint32_t window, uint32_t min_samples, uint32_t max_samples, double threshold,
                            double luminance_floor, uint64_t seed, double *rgb, double *variance,
                            uint32_t *tile_samples, double *tile_error, uint64_t *samples_rendered);

/* ---- resumable frames (checkpoint / resume) ----------------------------- */
/* The reference renders a frame in one go and keeps nothing between runs
 * (Renderer::render, src/renderer/mod.rs:67-114; its GUI saves only the
 * encoded image, src/bin/main.rs:281-289).  A frame here can be cut into
 * sample windows instead: pt_render_device_samples renders samples
 * [s_begin, s_end) of exactly the frame pt_render_device(..., samples_number,
 * ...) renders, into the same d_out layout.  d_out holds per-pixel running
 * sums between windows: read when s_begin > 0 (the sums of samples
 * [0, s_begin)), written as sums when s_end < samples_number and as the
 * means when s_end == samples_number.  Each sample keeps its frame-wide
 * index (its RNG key, pt_sample_key) and the sums add samples in index
 * order, so windows [0, a), [a, b), ..., [z, spp) leave d_out bit-identical to
 * one pt_render_device call.  0 <= s_begin < s_end <= samples_number, else
 * PT_ERR_INVALID.  Always runs the wavefront engine. */
int pt_render_device_samples(pt_renderer *r, const pt_camera *camera, uint32_t width, uint32_t height,
                             uint32_t samples_number, uint64_t seed, uint32_t rank, uint32_t world,
                             uint32_t s_begin, uint32_t s_end, double *d_out, void *hip_stream);
/* pt_render_device_samples restricted to a list of tiles: `tiles` (a host
 * array, copied before the call returns) holds tile_count >= 1 strictly
 * ascending indices into the rank's tile list, each below
 * pt_shard_tiles(width, height, rank, world).  The listed tiles' elements of
 * d_out are read (s_begin > 0) and written exactly as
 * pt_render_device_samples reads and writes them, bit for bit, a listed
 * partial tile's shard padding included; every other element of d_out is
 * neither read nor written.  One launch sequence whatever the list's gaps, so
 * a caller that renders few tiles of a frame (adaptive sampling, a region of
 * interest, a repaired tile) pays for those tiles alone.  PT_ERR_INVALID,
 * writing nothing: pt_render_device_samples' own argument errors, a NULL
 * `tiles`, tile_count 0, an entry out of range or not above the entry before
 * it.  PT_ERR_STATE while a pt_render_start frame is in flight.  Always runs
 * the wavefront engine.  (Library 0.4.3; no ABI change.) */
int pt_render_device_tiles(pt_renderer *r, const pt_camera *camera, uint32_t width, uint32_t height,
                           uint32_t samples_number, uint64_t seed, uint32_t rank, uint32_t world,
                           uint32_t s_begin, uint32_t s_end, const uint32_t *tiles, uint32_t tile_count,
                           double *d_out, void *hip_stream);
/* A checkpoint file: the 8 bytes "PTCKPT01", this header, `count` doubles
 * (the running sums of one rank's d_out after samples [0, samples_done)) and
 * a 64-bit FNV-1a checksum over the preceding bytes taken as little-endian
 * 64-bit words; all little-endian.  scene_key is the caller's: any value
 * that names the scene, camera and renderer options the sums belong to (the
 * Python mirror hashes the scene JSON, the camera and the depth); a resumed
 * frame must present the same key (checked by the caller). */
typedef struct pt_checkpoint {
    uint32_t width, height, samples_number, samples_done;
    uint32_t rank, world, depth, reserved; /* reserved: 0 */
    uint64_t seed;
    uint64_t scene_key;
    uint64_t count; /* doubles of sums: width*height*3 (world 1) or pt_shard_tiles(...)*768 */
} pt_checkpoint;
/* Writes header + sums[0..count) to path (atomically: a temporary file, synced
 * to disk, renamed over it, then the directory synced, so a crash or a power
 * loss leaves the old file or the new one).  The header must be consistent (samples_done <= samples_number,
 * rank < world, count as above), else PT_ERR_INVALID. */
int pt_checkpoint_save(const char *path, const pt_checkpoint *c, const double *sums);
/* Reads path's header into *c and, when sums is not NULL, its count sums
 * (capacity: doubles available at sums; fewer than count -> PT_ERR_INVALID)
 * and checks the checksum (a header-only read checks format, header and file
 * size).  A file that is missing, short, long, of another format, with an
 * inconsistent header or a checksum mismatch -> PT_ERR_IO with a message;
 * sums is zeroed on a checksum mismatch. */
int pt_checkpoint_load(const char *path, pt_checkpoint *c, double *sums, uint64_t capacity);

/* ---- probes on the GPU (reference pub fns) ----------------------------- */
/* Scene::closest_hit (src/world/mod.rs:42-44) for n rays (origin, direction:
 * 6 doubles each).  out[i].shape = -1 on a miss. */
int pt_closest_hit(pt_renderer *r, const double *rays, size_t n, double min_t, double max_t,
                   pt_hit *out);
/* ray_color (src/renderer/mod.rs:23-45) for n rays; rng_states[i] is the
 * stream state for ray i and is advanced in place.  depth <= PT_MAX_DEPTH
 * (above 64 the id stacks live in device memory: n * depth * 4 bytes). */
int pt_ray_color(pt_renderer *r, const double *rays, uint64_t *rng_states, size_t n, uint32_t depth,
                 double *out);
/* trace_pixel_samples (src/renderer/mod.rs:151-155) for an explicit list of
 * pixel indices (x + y*w); out is n*3 means.  Renderers of depth <= 64 only
 * (PT_ERR_UNSUPPORTED above, naming the call: this probe and pt_count_work
 * run the register id stacks; pt_profile_phases takes depth <= 8). */
int pt_trace_pixel_samples(pt_renderer *r, const pt_camera *camera, uint32_t width, uint32_t height,
                           uint32_t samples_number, uint64_t seed, const uint32_t *pixels, size_t n,
                           double *out);

/* Work counters of the kernel's own traversal policy over the listed pixels
 * (a diagnostic build of the same path): counters[PT_NUM_COUNTERS] receives,
 * in order, samples, bounces, sphere/rectangle/cube/marched-shape leaf tests,
 * BVH node slabs, marched-shape box slabs, literal march steps, march jump
 * attempts, march jumps, hits, Lambertian/Metal/Dielectric scatters,
 * rejection-sampling tries, attenuation multiplies, Torus tests, marches
 * dropped by the march guard.  Used for the FLOP side
 * of the roofline. */
#define PT_NUM_COUNTERS 19
int pt_count_work(pt_renderer *r, const pt_camera *camera, uint32_t width, uint32_t height,
                  uint32_t samples_number, uint64_t seed, const uint32_t *pixels, size_t n,
                  uint64_t *counters);

/* The RayMarchingShape march alone (src/world/shapes/ray_marching.rs:20-74,
 * Heart) on n object-space jobs of 8 doubles {step, passes, o[3], d[3]}:
 * t_out = the march's final t, status = 1 if the passes ended (a hit before
 * the caller's [min_t, max_t] test), 2 if the march guard dropped it, else 0,
 * iters = skipping-march iterations.  Diagnostic / parity probe. */
int pt_march_jobs(pt_renderer *r, const double *jobs, size_t n, double *t_out, int32_t *status, uint32_t *iters);

/* Marches the guard dropped since the last call (read and cleared), summed over
 * the renderer's devices.  A march that has not ended after 2^24 skipping
 * iterations (each >= 1 reference step) is one the reference would not finish
 * either — e.g. a step below the rounding of t, where t + step == t and
 * ray_marching.rs:37-51 loops forever; it is taken as a miss (the ray goes on
 * to the shape's neighbours) and counted here.  Waits for the devices.
 * PT_ERR_STATE while a render_start frame is in flight. */
int pt_march_guard_drops(pt_renderer *r, uint64_t *count);

/* What pt_render_stop did on the devices since the last call (read and
 * cleared, summed over the renderer's devices): *skipped = launches of the
 * stop-gated paths (wavefront bounce, march and sample-reduce launches,
 * megakernel blocks) that found their frame stopped and did nothing;
 * *worked = launches that found it stopped and still had work (0 unless the
 * gate is broken: every launch queued behind a fired gate must be a no-op).
 * The mechanism behind stop_rendering's latency (step_by_step.rs:73-77: the
 * workers check a flag between chunks).  Waits for the devices; PT_ERR_STATE
 * while a render_start frame is in flight. */
int pt_render_stop_stats(pt_renderer *r, uint64_t *skipped, uint64_t *worked);

/* Per-kernel launch timing of the render path (bench / roofline): returns
 * the summed HIP-event durations (ms) and launch counts per kernel kind since
 * the last call — [0] bounce, [1] march, [2] list compaction, [3] sample
 * reduce, [4] megakernel, [5] per-slot unwind before the reduce (wf_unwind;
 * until round 6 the removed wavefront tail kernel), [6] BVH walk (wf_walk) — into ms[nkinds] / launches[nkinds] (either may be
 * NULL), then turns recording on (enable = 1) or off.  Events are recorded on
 * the stream each kernel is launched on.  PT_ERR_STATE while a render_start
 * frame is in flight (its band feeder records into the same timer). */
#define PT_KERNEL_KINDS 7
int pt_kernel_timing(pt_renderer *r, int enable, double *ms, uint32_t *launches, size_t nkinds);

/* Diagnostic of the wavefront kernels: returns (and clears) the counters
 * accumulated since the last call into out[min(n, 64)] — the march kernel's
 * trips and s_memtime cycles per mix of lane phases (16 + 16), lanes per
 * phase (4), then the bounce kernel's cycles per section (list load, state
 * loads, shade, unwind, trace, march pre-check, stores; each section ended by
 * a full s_waitcnt, so the waits it causes are charged to it) — and turns the
 * instrumented build on (enable = 1) or off.  PT_ERR_STATE while a
 * render_start frame is in flight; PT_ERR_UNSUPPORTED (enable = 1) unless the
 * library was built with the instrumentation (make EXTRA=-DPT_WAVE_DIAG=1). */
int pt_wave_diag(pt_renderer *r, int enable, uint64_t *out, size_t n);

/* Diagnostic: render the whole frame (depth <= 8) with a timing build of the
 * megakernel and return wave-level s_memtime cycles summed over waves per
 * phase of its per-lane loop and pass counts: out[10] = {trace, march, select,
 * shade cycles, lane passes (sum), lane march passes (sum), max lane passes,
 * then shade split into: hit finish + material fetch, scatter, unwind/restart}. */
int pt_profile_phases(pt_renderer *r, const pt_camera *camera, uint32_t width, uint32_t height,
                      uint32_t samples_number, uint64_t seed, uint64_t *out);

/* ---- display encode and image output (src/bin/main.rs:71-82, 281-289) -- */
/* sqrt -> clamp [0, 0.999] -> *256 -> u8 (NaN -> 0), alpha 255; rgba is
 * npix*4 bytes.  Host-side. */
int pt_encode_rgba8(const double *rgb, size_t npix, uint8_t *rgba);
/* The same encode on the GPU: d_rgb / d_rgba in device memory of `device`
 * (-1 = current), d_rgba 4-byte aligned, queued on hip_stream. */
int pt_encode_rgba8_device(int device, const double *d_rgb, size_t npix, uint8_t *d_rgba, void *hip_stream);
/* image::save_buffer(path, rgba, w, h, ColorType::Rgba8) of the GUI's "F"
 * key: an RGBA8 PNG (stored deflate blocks), or binary PPM (P6, alpha
 * dropped). */
int pt_write_png(const char *path, const uint8_t *rgba, uint32_t width, uint32_t height);
int pt_write_ppm(const char *path, const uint8_t *rgba, uint32_t width, uint32_t height);

/* ---- RNG spec shared with the parity oracle ---------------------------- */
uint64_t pt_sample_key(uint64_t seed, uint64_t pixel, uint64_t sample);

const char *pt_last_error(void);
const char *pt_version(void);

/* ---- ABI self-description ----------------------------------------------- */
/* PT_ABI_VERSION changes whenever an entry point's signature or a struct's
 * layout or meaning changes (3: pt_scene_opts.struct_size, pt_unshard_device's
 * leading `device`, pt_abi_layout; 4: struct_size 0 reads 16 bytes, no
 * loader).  A binding compares it with the value it was
 * written for before calling anything else. */
#define PT_ABI_VERSION 4
uint32_t pt_abi_version(void);
/* Layout of a boundary struct as the library was compiled: out[0] = sizeof,
 * out[1 + k] = offsetof of the k-th field in declaration order.  Writes
 * min(n, fields + 1) values and returns fields + 1, or PT_ERR_INVALID for an
 * unknown `which`.  A binding (ctypes, Rust #[repr(C)]) checks its own
 * declarations against it. */
#define PT_ABI_SCENE_OPTS 0    /* 5 fields */
#define PT_ABI_CAMERA 1        /* 6 fields: position, direction, up, right, fov, focal_length */
#define PT_ABI_SHAPE_INFO 2    /* 20 fields, as declared */
#define PT_ABI_MATERIAL_INFO 3 /* 6 fields */
#define PT_ABI_HIT 4           /* 7 fields */
#define PT_ABI_CHECKPOINT 5    /* 11 fields, as declared */
int pt_abi_layout(int which, uint32_t *out, size_t n);

#ifdef __cplusplus
}
#endif
#endif
