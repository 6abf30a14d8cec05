// Test-only host build of the tile geometry (pt_tiles.hpp) with the plain host compiler: the very functions the pass
// kernels and pt_api.cpp call.  tests/test_tiles_host.py holds them against the numpy restatement (shard_pixels).
// Never used by the product.
#include "../../rs-pathtracing_amd/csrc/pt_tiles.hpp"

using namespace pt;

extern "C" uint32_t tg_tiles_across(uint32_t n) { return tiles_across(n); }
extern "C" int tg_grid_ok(uint32_t w, uint32_t h) { return tile_grid_ok(w, h); }
extern "C" uint32_t tg_shard_tiles(uint32_t w, uint32_t h, uint32_t rank, uint32_t world) {
    return shard_tiles(w, h, rank, world);
}
extern "C" uint64_t tg_shard_elements(uint32_t w, uint32_t h, uint32_t rank, uint32_t world) {
    return shard_elements(w, h, rank, world);
}
extern "C" uint32_t tg_position(uint32_t k, uint32_t tiles_x, uint32_t world) {
    return dev::tile_position(k, tiles_x, world);
}
extern "C" uint32_t tg_logical(uint32_t p, uint32_t tiles_x, uint32_t world) {
    return dev::tile_logical(p, tiles_x, world);
}
extern "C" void tg_lane_pixel(uint32_t t, uint32_t *lx, uint32_t *ly) {
    const dev::LanePixel p = dev::lane_pixel(t);
    *lx = p.lx;
    *ly = p.ly;
}

// Every slot of rank's list, tile by tile and row-major in the tile (slot = ti * 256 + ly * 16 + lx): pixel[slot] =
// y * w + x, or -1 outside the frame; at[slot] = tile_pixel's element offset; inside[ti] = tile_pixels_inside.
// The geometry is filled from a FrameParams-like struct, as pt_api.cpp fills it.  Returns the tiles of the list.
struct Params {
    uint32_t width, height, rank, world, tiles_x, compact;
};
extern "C" uint32_t tg_shard(uint32_t w, uint32_t h, uint32_t rank, uint32_t world, uint32_t compact, int64_t *pixel,
                             uint64_t *at, uint32_t *inside) {
    const dev::TileGeom g = dev::tile_geom(Params{w, h, rank, world, tiles_across(w), compact});
    const uint32_t ntiles = shard_tiles(w, h, rank, world);
    for (uint32_t ti = 0; ti < ntiles; ti++) {
        inside[ti] = dev::tile_pixels_inside(g, ti);
        for (uint32_t ly = 0; ly < TILE; ly++)
            for (uint32_t lx = 0; lx < TILE; lx++) {
                const dev::TilePixel p = dev::tile_pixel(g, ti, lx, ly);
                const size_t slot = ((size_t)ti * TILE + ly) * TILE + lx;
                pixel[slot] = p.inside ? (int64_t)p.y * w + p.x : -1;
                at[slot] = p.at;
            }
    }
    return ntiles;
}
