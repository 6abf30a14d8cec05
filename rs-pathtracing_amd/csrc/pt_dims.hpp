// pt_dims.hpp — the sizes and kinds that the kernels, the wavefront frame plan (pt_plan.hpp) and the choice of
// kernel builds (pt_builds.hpp) all count in.
#pragma once
#include <cstddef>
#include <cstdint>

// A function of the device code that a test-only host build compiles too; the plain host compiler sees plain C++.
#ifdef __HIPCC__
#define PT_HD __host__ __device__ __forceinline__
#else
#define PT_HD inline
#endif

namespace pt {

constexpr uint32_t TILE = 16;  // 16x16 pixels = one 256-thread workgroup
// compaction (pt_wave.hip cp_count / cp_scan / cp_scatter): statuses per thread, threads per block, statuses per tile
constexpr int CP_ITEMS = 16, CP_BLOCK = 256, CP_TILE = CP_ITEMS * CP_BLOCK;
constexpr size_t PATH_BYTES = 8 * 8 + 2 * 4;  // wavefront path state per path and set (pt_wave.hip PathSoA)

constexpr int BIG_BVH_NODES = 1 << 15;  // binary nodes from which the bounce runs its large-tree builds (C5)

// The deepest call the register id stacks take (IdStack<32>: the megakernel, trace_pixels_probe, count_work and
// ray_color_probe).  Deeper frames run the wavefront engine, deeper pt_ray_color calls the memory-stack probe.
constexpr uint32_t MAX_REG_DEPTH = 64;

namespace march {

// The ray-marched implicit functions (pt_funcs.hpp).
enum FuncKind : int32_t { F_HEART = 0, F_SINE = 1, F_STAR = 2, F_DUPIN = 3, F_HUNTS = 4, F_CUSHION = 5 };
// Compile-time function kind: FK >= 0 instantiates one function (a scene
// whose marched shapes are all Hearts runs the Heart-only build: no dispatch,
// no unused constants in registers); FK = F_ANY dispatches on F.func.
constexpr int F_ANY = -1;
// F_NONE: the scene has no ray-marched shape (the bounce build for large BVHs without one, C5): pt_funcs.hpp's
// helpers are never reached at run time and compile to nothing
constexpr int F_NONE = -2;

}  // namespace march
}  // namespace pt
