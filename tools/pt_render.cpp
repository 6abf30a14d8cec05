// pt_render — headless renderer over the C-ABI: the reference GUI's scene -> frame -> image path without the
// window.  The reference binaries take `scene [spp [w h]]` (src/bin/main_raylib.rs:22-41), render with depth 50
// (src/bin/main.rs:229-240) and save the display-encoded frame as images/rendered.png on "F"
// (src/bin/main.rs:71-83, 281-289).  This does the same in one go, on the GPU:
//
//   pt_render scene.json [spp [w h]] [-d depth] [-s seed] [-o image.png|image.ppm] [-f frame.f64]
//             [-c checkpoint -n window_spp [-x windows]] [-a prefix] [-D denoised.png] [-V var.f64 [-W windows]]
//             [-A threshold [-B window] [-M tiles.u32]]
//
// -o: the encoded image (PNG, or PPM by extension; default rendered.png, the name of the reference's "F" save).
// -f: the linear f64 frame (w*h*3, row-major), for comparisons.
// -c/-n: a resumable frame: samples in windows of window_spp; after each window but the last the
//     running sums go to the checkpoint file; a run that finds the file resumes from it (same scene, camera,
//     depth, size, spp and seed, else it refuses).  -x stops after that many windows of this run (exit status 3,
//     the checkpoint kept): an interruption, for tests.  The finished frame is bit-identical to a run without -c.
// -a: the frame's first-hit guide planes (pt_render_aov: the same samples' camera rays), written after the frame as
//     prefix.albedo.png (the display encode), prefix.normal.png ((n + 1) / 2 per channel, linear, x 255.999) and
//     prefix.depth.png (grey: mean t / coverage over the frame's largest such value; black where nothing is hit);
//     with -f also the three raw planes, albedo then normal then depth, as prefix.aov.f64.
// -D: the frame denoised on the device with its guide planes (pt_denoise_device at its defaults: 5 iterations,
//     sigma_normal 0.5, sigma_depth 0.1, no colour term, demodulated), as a PNG through the display encode; with -f
//     also the linear f64 frame as denoised.png.f64.  The planes are -a's when it was given, else they are rendered
//     on the device for this.  -o and -f still get the noisy frame.  (-d is the depth, so the letter is a capital.)
// -V: the variance of each pixel's mean, per channel, estimated from the frame's own sample windows
//     (pt_render_variance), as linear f64 in -f's format (w*h*3, row-major); the frame is the same bits.
//     -W: the number of windows (default 8, or spp when that is less).  With -V, -D uses the denoiser's variance
//     term (pt_denoise_variance_device, sigma_variance 8).  -V with -c is a usage error: the accumulation state is
//     not checkpointed.
// -A: adaptive sampling (pt_render_adaptive): spp is the cap, and every 16x16 tile stops once the
//     relative standard error of its luminance is at most the threshold (0: run every tile that is not constant to
//     the cap; inf: stop every tile at the second window), judged after each window of -B samples (default 8;
//     min_samples 0, luminance floor 0.01, the library's recommended merge_gap).  -M: the samples each tile stopped
//     at, as uint32, tiles row-major.  With -A, -V writes the adaptive frame's variance plane (each pixel's at its
//     tile's own sample count) and -D uses it.  -L: every window is one launch over the list of the still-active
//     tiles (pt_render_adaptive_list): the same files, bit for bit, and no stopped tile rendered again.
//     -A with -c or -W, and -B, -M or -L without -A, are usage errors: the accumulation state is not checkpointed.
// Exit status: 0 done, 1 error (the library's message on stderr), 2 usage, 3 stopped with a checkpoint.
#include <hip/hip_runtime_api.h>

#include <sys/stat.h>

#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../include/rs_pathtracing.h"

namespace {

int usage() {
    std::fprintf(stderr,
                 "usage: pt_render scene.json [spp [w h]] [-d depth] [-s seed] [-o image.png|.ppm] [-f frame.f64]\n"
                 "                 [-c checkpoint -n window_spp [-x windows]] [-a aov_prefix] [-D denoised.png]\n"
                 "                 [-V variance.f64 [-W windows]]   (-V cannot be combined with -c)\n"
                 "                 [-A threshold [-B window] [-M tiles.u32] [-L]]   (spp is the cap; not with -c or -W;\n"
                 "                                                                   -L: one launch per window)\n");
    return 2;
}

int fail(const char *what, int rc) {
    std::fprintf(stderr, "pt_render: %s: %s (status %d)\n", what, pt_last_error(), rc);
    return 1;
}

bool read_file(const char *path, std::string *out) {
    FILE *f = std::fopen(path, "rb");
    if (!f) return false;
    char buf[1 << 16];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) out->append(buf, n);
    std::fclose(f);
    return true;
}

// 64-bit FNV-1a over bytes: the checkpoint's scene key (scene text, camera, depth)
uint64_t fnv(uint64_t h, const void *p, size_t n) {
    const unsigned char *b = (const unsigned char *)p;
    for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 0x100000001b3ull;
    return h;
}

bool write_doubles(const std::string &path, const std::vector<double> &v) {
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f || std::fwrite(v.data(), sizeof(double), v.size(), f) != v.size() || std::fclose(f) != 0) {
        std::fprintf(stderr, "pt_render: cannot write %s\n", path.c_str());
        return false;
    }
    return true;
}

bool ends_with(const std::string &s, const char *suf) {
    const size_t n = std::strlen(suf);
    return s.size() >= n && s.compare(s.size() - n, n, suf) == 0;
}

}  // namespace

int main(int argc, char **argv) {
    std::vector<const char *> pos;
    uint32_t depth = 50, window = 0, stop_after = 0, var_windows = 0, ad_window = 0;
    uint64_t seed = 1;
    double ad_threshold = 0.0;
    bool adaptive = false, ad_window_given = false, ad_list = false;
    std::string out_img = "rendered.png", out_f64, ckpt, aov, denoised, out_var, out_tiles;
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        auto val = [&](const char *name) -> const char * {
            if (i + 1 >= argc) {
                std::fprintf(stderr, "pt_render: %s needs a value\n", name);
                std::exit(usage());
            }
            return argv[++i];
        };
        if (a == "-d") depth = (uint32_t)std::strtoul(val("-d"), nullptr, 10);
        else if (a == "-s") seed = std::strtoull(val("-s"), nullptr, 10);
        else if (a == "-o") out_img = val("-o");
        else if (a == "-f") out_f64 = val("-f");
        else if (a == "-c") ckpt = val("-c");
        else if (a == "-n") window = (uint32_t)std::strtoul(val("-n"), nullptr, 10);
        else if (a == "-a") aov = val("-a");
        else if (a == "-D") denoised = val("-D");
        else if (a == "-V") out_var = val("-V");
        else if (a == "-W") var_windows = (uint32_t)std::strtoul(val("-W"), nullptr, 10);
        else if (a == "-A") {
            const char *v = val("-A");
            char *end = nullptr;
            ad_threshold = std::strtod(v, &end);
            if (end == v || *end) return usage();
            adaptive = true;
        } else if (a == "-B") {
            ad_window = (uint32_t)std::strtoul(val("-B"), nullptr, 10);
            ad_window_given = true;
        } else if (a == "-M") out_tiles = val("-M");
        else if (a == "-L") ad_list = true;
        else if (a == "-x") stop_after = (uint32_t)std::strtoul(val("-x"), nullptr, 10);
        else if (a.size() > 1 && a[0] == '-') return usage();
        else pos.push_back(argv[i]);
    }
    if (pos.empty() || pos.size() == 3 || pos.size() > 4 || (!ckpt.empty() && window == 0)) return usage();
    if (!out_var.empty() && !ckpt.empty()) return usage();
    if (adaptive && (!ckpt.empty() || var_windows != 0)) return usage();
    if (!adaptive && (ad_window_given || !out_tiles.empty() || ad_list)) return usage();
    const uint32_t spp = pos.size() >= 2 ? (uint32_t)std::strtoul(pos[1], nullptr, 10) : 100;  // the GUI's 100
    const uint32_t w = pos.size() == 4 ? (uint32_t)std::strtoul(pos[2], nullptr, 10) : 1600;    // main.rs:26
    const uint32_t h = pos.size() == 4 ? (uint32_t)std::strtoul(pos[3], nullptr, 10) : 900;
    std::string json;
    if (!read_file(pos[0], &json)) {
        std::fprintf(stderr, "pt_render: cannot read %s\n", pos[0]);
        return 1;
    }
    pt_scene_opts opts = PT_SCENE_OPTS_INIT;
    pt_scene *scene = nullptr;
    pt_renderer *r = nullptr;
    pt_camera cam;
    int rc;
    if ((rc = pt_scene_create_from_json(json.data(), json.size(), &opts, &scene))) return fail(pos[0], rc);
    if ((rc = pt_scene_camera(scene, &cam))) return fail("camera", rc);
    if ((rc = pt_renderer_create(scene, -1, depth, &r))) return fail("renderer", rc);
    const size_t npix = (size_t)w * h;
    std::vector<double> rgb(npix * 3), variance;
    if (adaptive) {
        // every tile to its noise target, spp at the most; the variance plane serves -V and -D
        const uint32_t tiles = ((w + 15) / 16) * ((h + 15) / 16);
        std::vector<uint32_t> tile_samples(tiles);
        uint64_t launched = 0;
        variance.resize(npix * 3);
        if (!ad_window_given) ad_window = PT_ADAPTIVE_WINDOW;
        rc = ad_list ? pt_render_adaptive_list(r, &cam, w, h, ad_window, 0, spp, ad_threshold,
                                               PT_ADAPTIVE_LUMINANCE_FLOOR, seed, rgb.data(), variance.data(),
                                               tile_samples.data(), nullptr, &launched)
                     : pt_render_adaptive(r, &cam, w, h, ad_window, 0, spp, ad_threshold, PT_ADAPTIVE_LUMINANCE_FLOOR,
                                          PT_ADAPTIVE_MERGE_GAP, seed, rgb.data(), variance.data(),
                                          tile_samples.data(), nullptr, &launched);
        if (rc) return fail("adaptive render", rc);
        std::fprintf(stderr, "pt_render: %llu of %llu pixel-samples rendered\n", (unsigned long long)launched,
                     (unsigned long long)npix * spp);
        if (!out_var.empty() && !write_doubles(out_var, variance)) return 1;
        if (!out_tiles.empty()) {
            FILE *f = std::fopen(out_tiles.c_str(), "wb");
            if (!f || std::fwrite(tile_samples.data(), sizeof(uint32_t), tiles, f) != tiles || std::fclose(f) != 0) {
                std::fprintf(stderr, "pt_render: cannot write %s\n", out_tiles.c_str());
                return 1;
            }
        }
    } else if (!out_var.empty()) {
        // the frame in sample windows, with the variance of each pixel's mean beside it
        variance.resize(npix * 3);
        if (var_windows == 0) var_windows = spp < 8 ? spp : 8;
        if ((rc = pt_render_variance(r, &cam, w, h, spp, seed, var_windows, rgb.data(), variance.data())))
            return fail("render with variance", rc);
        if (!write_doubles(out_var, variance)) return 1;
    } else if (ckpt.empty()) {
        if ((rc = pt_render_start(r, &cam, w, h, spp, seed)) || (rc = pt_render_step(r, rgb.data(), 1)) != 1)
            return fail("render", rc);
    } else {
        // a resumable frame: sample windows into a device buffer, the running sums checkpointed between them
        const uint64_t key = fnv(fnv(fnv(0xcbf29ce484222325ull, json.data(), json.size()), &cam, sizeof cam),
                                 &depth, sizeof depth);
        double *d_out = nullptr;
        if (hipMalloc((void **)&d_out, npix * 3 * sizeof(double)) != hipSuccess) {
            std::fprintf(stderr, "pt_render: hipMalloc failed\n");
            return 1;
        }
        uint32_t done = 0;
        pt_checkpoint c;
        // start fresh only when there is no checkpoint file; an existing one that does not load (corrupt, not a
        // checkpoint, unreadable) is an error, never overwritten
        struct stat sb;
        const bool exists = ::stat(ckpt.c_str(), &sb) == 0 || errno != ENOENT;
        if (exists && (rc = pt_checkpoint_load(ckpt.c_str(), &c, nullptr, 0)) != PT_OK) return fail(ckpt.c_str(), rc);
        if (exists) {
            if (c.width != w || c.height != h || c.samples_number != spp || c.seed != seed || c.depth != depth ||
                c.scene_key != key || c.world != 1) {
                std::fprintf(stderr, "pt_render: %s belongs to another frame\n", ckpt.c_str());
                return 1;
            }
            if ((rc = pt_checkpoint_load(ckpt.c_str(), &c, rgb.data(), rgb.size()))) return fail(ckpt.c_str(), rc);
            if (hipMemcpy(d_out, rgb.data(), rgb.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
                return 1;
            done = c.samples_done;
            std::fprintf(stderr, "pt_render: resuming at sample %u of %u\n", done, spp);
        }
        uint32_t windows = 0;
        while (done < spp) {
            const uint32_t end = spp - done > window ? done + window : spp;
            if ((rc = pt_render_device_samples(r, &cam, w, h, spp, seed, 0, 1, done, end, d_out, nullptr)))
                return fail("render window", rc);
            if (hipDeviceSynchronize() != hipSuccess) return 1;
            done = end;
            if (done == spp) break;
            if (hipMemcpy(rgb.data(), d_out, rgb.size() * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
                return 1;
            std::memset(&c, 0, sizeof c);
            c.width = w;
            c.height = h;
            c.samples_number = spp;
            c.samples_done = done;
            c.rank = 0;
            c.world = 1;
            c.depth = depth;
            c.seed = seed;
            c.scene_key = key;
            c.count = rgb.size();
            if ((rc = pt_checkpoint_save(ckpt.c_str(), &c, rgb.data()))) return fail(ckpt.c_str(), rc);
            if (stop_after && ++windows >= stop_after) {
                std::fprintf(stderr, "pt_render: stopped at sample %u of %u, checkpoint %s\n", done, spp, ckpt.c_str());
                return 3;
            }
        }
        if (hipMemcpy(rgb.data(), d_out, rgb.size() * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return 1;
        (void)hipFree(d_out);
        std::remove(ckpt.c_str());
    }
    if (!out_f64.empty() && !write_doubles(out_f64, rgb)) return 1;
    if (!out_img.empty()) {
        std::vector<uint8_t> rgba(npix * 4);
        if ((rc = pt_encode_rgba8(rgb.data(), npix, rgba.data()))) return fail("encode", rc);
        rc = ends_with(out_img, ".ppm") ? pt_write_ppm(out_img.c_str(), rgba.data(), w, h)
                                        : pt_write_png(out_img.c_str(), rgba.data(), w, h);
        if (rc) return fail(out_img.c_str(), rc);
    }
    std::vector<double> planes;  // -a: albedo, normal, depth
    if (!aov.empty()) {
        planes.resize(npix * 9);
        double *alb = planes.data(), *nrm = alb + npix * 3, *dep = nrm + npix * 3;
        if ((rc = pt_render_aov(r, &cam, w, h, spp, seed, alb, nrm, dep))) return fail("guide planes", rc);
        if (!out_f64.empty() && !write_doubles(aov + ".aov.f64", planes)) return 1;
        std::vector<uint8_t> rgba(npix * 4);
        auto save = [&](const char *plane) {
            const std::string path = aov + "." + plane + ".png";
            const int e = pt_write_png(path.c_str(), rgba.data(), w, h);
            return e ? fail(path.c_str(), e) : 0;
        };
        if ((rc = pt_encode_rgba8(alb, npix, rgba.data()))) return fail("encode", rc);
        if (save("albedo")) return 1;
        auto byte = [](double v) { return (uint8_t)(v > 0.0 ? (v < 1.0 ? v * 255.999 : 255.0) : 0.0); };  // NaN -> 0
        for (size_t i = 0; i < npix; i++) {
            for (int c = 0; c < 3; c++) rgba[i * 4 + c] = byte((nrm[i * 3 + c] + 1.0) / 2.0);
            rgba[i * 4 + 3] = 255;
        }
        if (save("normal")) return 1;
        double far = 0.0;  // the largest mean distance of the hitting samples (mean t / coverage)
        for (size_t i = 0; i < npix; i++)
            if (dep[i * 3 + 1] > 0.0 && dep[i * 3] / dep[i * 3 + 1] > far) far = dep[i * 3] / dep[i * 3 + 1];
        for (size_t i = 0; i < npix; i++) {
            const uint8_t g = dep[i * 3 + 1] > 0.0 && far > 0.0 ? byte(dep[i * 3] / dep[i * 3 + 1] / far) : 0;
            rgba[i * 4 + 0] = rgba[i * 4 + 1] = rgba[i * 4 + 2] = g;
            rgba[i * 4 + 3] = 255;
        }
        if (save("depth")) return 1;
    }
    if (!denoised.empty()) {
        // on the device: the frame, the three planes and the workspace in one allocation
        // (and the variance plane after the workspace, with -V)
        const size_t plane = npix * 3, work = pt_denoise_workspace_doubles(w, h);
        double *d = nullptr;
        uint8_t *d_rgba = nullptr;
        if (hipMalloc((void **)&d, (plane * (variance.empty() ? 4 : 5) + work) * sizeof(double)) != hipSuccess ||
            hipMalloc((void **)&d_rgba, npix * 4) != hipSuccess ||
            hipMemcpy(d, rgb.data(), plane * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) {
            std::fprintf(stderr, "pt_render: no device memory for the denoiser\n");
            return 1;
        }
        double *alb = d + plane, *nrm = alb + plane, *dep = nrm + plane;
        if (!planes.empty()) {
            if (hipMemcpy(alb, planes.data(), plane * 3 * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) return 1;
        } else if ((rc = pt_render_aov_device(r, &cam, w, h, spp, seed, 0, 1, alb, nrm, dep, nullptr))) {
            return fail("guide planes", rc);
        }
        if (variance.empty()) {
            if ((rc = pt_denoise_device(-1, d, alb, nrm, dep, w, h, 5, 0.5, 0.1, 0.0, PT_DENOISE_DEMODULATE, d,
                                        dep + plane, nullptr)))
                return fail("denoise", rc);
        } else {
            double *d_var = dep + plane + work;
            if (hipMemcpy(d_var, variance.data(), plane * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) return 1;
            if ((rc = pt_denoise_variance_device(-1, d, alb, nrm, dep, d_var, w, h, 5, 0.5, 0.1, 8.0,
                                                 PT_DENOISE_DEMODULATE, d, dep + plane, nullptr)))
                return fail("denoise", rc);
        }
        if ((rc = pt_encode_rgba8_device(-1, d, npix, d_rgba, nullptr))) return fail("encode", rc);
        std::vector<uint8_t> rgba(npix * 4);
        std::vector<double> clean(plane);
        if (hipDeviceSynchronize() != hipSuccess ||
            hipMemcpy(rgba.data(), d_rgba, rgba.size(), hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(clean.data(), d, plane * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) {
            std::fprintf(stderr, "pt_render: the denoiser failed on the device\n");
            return 1;
        }
        (void)hipFree(d_rgba);
        (void)hipFree(d);
        if ((rc = pt_write_png(denoised.c_str(), rgba.data(), w, h))) return fail(denoised.c_str(), rc);
        if (!out_f64.empty() && !write_doubles(denoised + ".f64", clean)) return 1;
    }
    std::printf("rendered %ux%u at %u spp, depth %u\n", w, h, spp, depth);
    pt_renderer_destroy(r);
    pt_scene_destroy(scene);
    return 0;
}
