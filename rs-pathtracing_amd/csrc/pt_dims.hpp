// pt_dims.hpp — the sizes that both the kernels and the wavefront frame plan (pt_plan.hpp) count in.
#pragma once
#include <cstddef>
#include <cstdint>

namespace pt {

constexpr uint32_t TILE = 16;  // 16x16 pixels = one 256-thread workgroup
// compaction (pt_wave.hip cp_count / cp_scan / cp_scatter): statuses per thread, threads per block, statuses per tile
constexpr int CP_ITEMS = 16, CP_BLOCK = 256, CP_TILE = CP_ITEMS * CP_BLOCK;
constexpr size_t PATH_BYTES = 8 * 8 + 2 * 4;  // wavefront path state per path and set (pt_wave.hip PathSoA)

}  // namespace pt
