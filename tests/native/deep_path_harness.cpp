// Test-only host build of the deep path (depth > 64): ray_color with the attenuation-id stack in memory
// (dev::MemStack through dev::shade and dev::unwind, pt_device.hpp: the one memory stack, the type of the wavefront
// engine's per-slot stacks of every frame and of ray_color_probe_deep), on a scene realized as path_harness.cpp does.  tests/test_deep_host.py compares it with the oracle bit for
// bit.  With DEEP_HARNESS_MAIN it is a stand-alone program (for a sanitizer build): it also walks the plan of deep
// frames (pt_plan.hpp).  Never used by the product.
#include <cstdio>
#include <fstream>
#include <iterator>
#include <string>

#include "../../rs-pathtracing_amd/csrc/pt_plan.hpp"
#include "path_harness.cpp"

// n rays (6 doubles each) with their RNG states, the stacks laid out as the GPU probe's: lane i's id k at
// ids[k * n + i], its textured value of level k, component c at vals[(k * 3 + c) * n + i].
extern "C" void h_ray_color_mem(void *p, const double *rays, uint64_t *states, size_t n, uint32_t depth, double *out) {
    Bundle *b = (Bundle *)p;
    std::vector<uint32_t> ids(n * (size_t)depth + 1);
    std::vector<double> vals(n * ((size_t)depth + 1) * 3);
    for (size_t i = 0; i < n; i++) {
        const dev::Ray r = dev::load_ray(rays, i);
        dev::Rng rng{states[i]};
        const dev::V3 c = dev::ray_color_mem<true>(b->view, r, depth, rng, b->s11, ids.data() + i, vals.data() + i, n);
        states[i] = rng.s;
        dev::store_rgb(out, i, c);
    }
}

#ifdef DEEP_HARNESS_MAIN
// deep_path_main scene.json rays.bin depth out.bin: rays.bin holds n records of 6 doubles and one u64 state;
// out.bin receives n records of 3 doubles and the advanced state.
int main(int argc, char **argv) {
    if (argc != 5) return 2;
    std::ifstream sf(argv[1], std::ios::binary);
    const std::string json((std::istreambuf_iterator<char>(sf)), std::istreambuf_iterator<char>());
    std::ifstream rf(argv[2], std::ios::binary);
    const std::string raw((std::istreambuf_iterator<char>(rf)), std::istreambuf_iterator<char>());
    const uint32_t depth = (uint32_t)std::stoul(argv[3]);
    const size_t n = raw.size() / 56;
    if (json.empty() || n == 0 || raw.size() != n * 56) return 2;
    std::vector<double> rays(n * 6), out(n * 3);
    std::vector<uint64_t> states(n);
    for (size_t i = 0; i < n; i++) {
        std::memcpy(&rays[i * 6], raw.data() + i * 56, 48);
        std::memcpy(&states[i], raw.data() + i * 56 + 48, 8);
    }
    void *h = h_scene_new(json.data(), json.size(), 0, 1);
    if (!h) return 3;
    h_ray_color_mem(h, rays.data(), states.data(), n, depth, out.data());
    h_scene_free(h);
    std::ofstream of(argv[4], std::ios::binary);
    for (size_t i = 0; i < n; i++) {
        of.write((const char *)&out[i * 3], 24);
        of.write((const char *)&states[i], 8);
    }
    // the plan of a 1080p, 256-spp frame at this depth and at the limit, with and without the device's memory
    size_t sum = 0;
    for (uint32_t d : {depth, plan::MAX_DEPTH})
        for (int tex = 0; tex < 2; tex++)
            for (size_t hard : {plan::MEM_UNKNOWN, (size_t)288 << 30, (size_t)3 << 30}) {
                plan::Input in{};
                in.ntiles = 8160, in.s_begin = 0, in.s_end = in.spp = 256, in.depth = d;
                in.textured = tex != 0, in.presel = true;
                in.wf_paths = 0, in.wf_slots = 2, in.wf_min_chunks = 1;
                in.avail_bytes = hard == plan::MEM_UNKNOWN ? hard : hard - plan::RESERVE_BYTES;
                const plan::Plan pl = plan::make_plan_fit(&in, hard);
                const std::vector<plan::Chunk> cl = plan::chunk_list(in, pl);
                sum += pl.bytes / 1024 + cl.size() + (plan::fits(in, pl) ? 1 : 0);
                sum += plan::fits_device(pl, hard) ? 2 : 0;
            }
    std::printf("ok %zu rays depth %u plans %zu\n", n, depth, sum);
    return 0;
}
#endif
