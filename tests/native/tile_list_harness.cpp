// Test-only host build of the listed launch's host pieces (pt_adaptive.hpp: tile_list_ok, adaptive_list) behind a C
// boundary, for tests/test_tile_list_host.py.  Never used by the product.
#include <vector>

#include "../../rs-pathtracing_amd/csrc/pt_adaptive.hpp"

using namespace pt;

extern "C" int tl_ok(const uint32_t *list, size_t n, uint32_t ntiles) { return tile_list_ok(list, n, ntiles) ? 1 : 0; }

// adaptive_list into out (room for ntiles entries); returns its length.
extern "C" uint32_t tl_adaptive_list(const uint8_t *active, uint32_t ntiles, uint32_t *out) {
    const std::vector<uint32_t> list = adaptive_list(active, ntiles);
    for (size_t i = 0; i < list.size(); i++) out[i] = list[i];
    return (uint32_t)list.size();
}
