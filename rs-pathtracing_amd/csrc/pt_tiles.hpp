// pt_tiles.hpp — the geometry of the 16x16 tile, stated once for the passes beside the render path and for the
// host: how many tiles a frame has, which tiles a rank owns, where a tile of a rank's list lies in
// the frame, which pixel of it a thread of the 256-thread workgroup owns, and where that pixel is kept.  Standard
// C++ only, so the plain host compiler builds it too (tests/native/tiles_harness.cpp); tests/test_tiles_host.py
// holds every function here against the numpy restatement (shard_pixels in the Python package).
#pragma once
#include "pt_dims.hpp"

namespace pt {

PT_HD uint32_t tiles_across(uint32_t n) { return (n + TILE - 1) / TILE; }

// A launch of one workgroup per tile has a 32-bit grid: the frames whose tile count fits one.
PT_HD bool tile_grid_ok(uint32_t w, uint32_t h) { return (uint64_t)tiles_across(w) * tiles_across(h) <= 0x7fffffffull; }

// The tiles of rank's list: logical tile k belongs to rank k % world at list index k / world.
PT_HD uint32_t shard_tiles(uint32_t w, uint32_t h, uint32_t rank, uint32_t world) {
    if (world == 0 || rank >= world) return 0;
    const uint32_t total = tiles_across(w) * tiles_across(h);
    return rank < total ? (total - rank + world - 1) / world : 0;
}

// The doubles of one rank's frame: the frame itself for world == 1, else the compact shard, whole tiles back to back.
PT_HD uint64_t shard_elements(uint32_t w, uint32_t h, uint32_t rank, uint32_t world) {
    return world == 1 ? (uint64_t)w * h * 3 : (uint64_t)shard_tiles(w, h, rank, world) * (TILE * TILE * 3);
}

namespace dev {

// Multi-rank tile deal (world > 1): rank r owns logical tiles k = r + i*world;
// logical tile k sits at column (k % tiles_x + row) % tiles_x of its row, so a
// rank's columns shift by one per row (a diagonal deal) instead of repeating
// in every row when tiles_x is a multiple of world.  world == 1: identity.
PT_HD uint32_t tile_position(uint32_t k, uint32_t tiles_x, uint32_t world) {
    if (world <= 1) return k;
    const uint32_t ty = k / tiles_x;
    return ty * tiles_x + (k % tiles_x + ty) % tiles_x;
}
PT_HD uint32_t tile_logical(uint32_t p, uint32_t tiles_x, uint32_t world) {
    if (world <= 1) return p;
    const uint32_t ty = p / tiles_x;
    return ty * tiles_x + (p % tiles_x + tiles_x - ty % tiles_x) % tiles_x;
}

// Thread t of a tile's workgroup -> its pixel of the tile: 4 wave64s of 8x8 pixels, wave w on quadrant
// (w & 1, w >> 1), lane l on (l & 7, l >> 3) of it.  The layout is the render path's, which still spells it out
// (render_tiles and render_tiles_timed in pt_kernel.hip, slot_pixel in pt_wave.hip).
struct LanePixel {
    uint32_t lx, ly;
};
PT_HD LanePixel lane_pixel(uint32_t t) {
    const uint32_t w = t >> 6, l = t & 63;
    return LanePixel{((w & 1u) << 3) | (l & 7u), ((w >> 1) << 3) | (l >> 3)};
}

// A frame as one rank renders it: where the tiles of the rank's list lie, and how their pixels are kept (compact: the
// rank's shard, 256 pixels per tile in list order, row-major in the tile; else the frame itself).
struct TileGeom {
    uint32_t width, height, rank, world, tiles_x, compact;
};
// Of FrameParams (pt_types.hpp), or of anything with its fields.
template <class Params>
PT_HD TileGeom tile_geom(const Params &P) {
    return TileGeom{P.width, P.height, P.rank, P.world, P.tiles_x, P.compact};
}

// The whole frame as the one rank of a world of one; tiles_x = tiles_across(w), which the kernels take as an argument.
PT_HD TileGeom whole_frame(uint32_t w, uint32_t h, uint32_t tiles_x) { return TileGeom{w, h, 0, 1, tiles_x, 0}; }

// Tile ti of the rank's list: its column and row in the frame.
struct Tile {
    uint32_t ti, tx, ty;
};
PT_HD Tile tile_of(const TileGeom &g, uint32_t ti) {
    const uint32_t k = tile_position(g.rank + ti * g.world, g.tiles_x, g.world);  // global tile id
    return Tile{ti, k % g.tiles_x, k / g.tiles_x};
}

// Pixel (lx, ly) of a tile: its frame coordinates, its element offset in the layout, and whether it lies inside the
// frame (a compact shard keeps an offset for the ones that do not: its padding).
struct TilePixel {
    uint32_t x, y;
    size_t at;
    bool inside;
};
PT_HD TilePixel tile_pixel(const TileGeom &g, const Tile &t, uint32_t lx, uint32_t ly) {
    // lx < TILE already.  Saying so here, where the compiler optimises this function on its own before it inlines it,
    // keeps the two arms of `at` apart until then: aov_tiles' machine code is then what the open-coded form gave.
    lx &= TILE - 1;
    const uint32_t x = t.tx * TILE + lx, y = t.ty * TILE + ly;
    const size_t at = g.compact ? ((size_t)t.ti * (TILE * TILE) + ly * TILE + lx) * 3 : ((size_t)y * g.width + x) * 3;
    return TilePixel{x, y, at, x < g.width && y < g.height};
}
PT_HD TilePixel tile_pixel(const TileGeom &g, uint32_t ti, uint32_t lx, uint32_t ly) {
    return tile_pixel(g, tile_of(g, ti), lx, ly);
}

// The tile's pixels inside the frame.
PT_HD uint32_t tile_pixels_inside(const TileGeom &g, const Tile &t) {
    const uint32_t x0 = t.tx * TILE, y0 = t.ty * TILE;
    const uint32_t nx = g.width - x0 < TILE ? g.width - x0 : TILE, ny = g.height - y0 < TILE ? g.height - y0 : TILE;
    return nx * ny;
}
PT_HD uint32_t tile_pixels_inside(const TileGeom &g, uint32_t ti) { return tile_pixels_inside(g, tile_of(g, ti)); }

}  // namespace dev
}  // namespace pt
