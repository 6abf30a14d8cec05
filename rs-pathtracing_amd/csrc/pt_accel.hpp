// pt_accel.hpp — closest-hit acceleration for the GPU path (host build).
//
// The reference wraps the shape list in a randomly split BvhNode tree
// (src/world/shapes/mod.rs:620-729); its result is the ShapeCollection linear
// minimum (mod.rs:587-596) up to exact ties.  Here the realized list is split
// into three groups, all tested with one acceptance rule — accept t if
// t < best or (t == best and shape index > best index) — which reproduces the
// linear scan's "later shape wins a tie" in any visiting order:
//   * `lin`   — the JSON shapes when there are few, and every Torus: a
//               wave-uniform loop;
//   * BVH     — everything else that is not ray-marched (random spheres,
//               large scenes), median-split, threaded, padded f64 boxes;
//   * `march` — ray-marched shapes, tested last behind their padded box
//               against the best distance so far.
#pragma once
#include <array>
#include <cstdint>
#include <vector>

#include "pt_scene.hpp"
#include "pt_types.hpp"

namespace pt {

// The BVH is stored as 8 threaded (stackless, skip-pointer) layouts of the same
// tree, one per ray-direction octant: layout o = (d.x < 0) | (d.y < 0) << 1 |
// (d.z < 0) << 2 visits, at every interior node, the child on the ray's near
// side of the split first, so the best hit shrinks early and far subtrees are
// skipped by their boxes.  Skip indices are relative to the layout; the leaf
// id ranges are shared.  8x the node memory (C5: ~50 MB of the 288 GB HBM)
// buys front-to-back order without a per-lane stack.
constexpr int BVH_OCTANTS = 8;
struct Accel {
    std::vector<DNode> nodes;    // BVH_OCTANTS layouts of nodes_per_octant() nodes each
    std::vector<DNodeC> cnodes;  // the same nodes in the device form (f32 boxes rounded outward)
    int nodes_per_octant() const { return (int)(nodes.size() / BVH_OCTANTS); }
    std::vector<int32_t> leaf;   // shape ids referenced by leaf nodes
    std::vector<int32_t> lin;    // wave-uniform list (shape ids; LIN_GROUPED marks, pt_types.hpp)
    std::vector<int32_t> march;  // ray-marched shapes
    std::vector<DBox> boxes;     // padded world AABB per shape
    float bvh_bound = 0.f;  // >= |every plane of cnodes| (dev::Scene::bvh_bound)
    // the quantized nodes (trees of at least BIG_BVH_NODES nodes per layout; empty otherwise) and their grid
    std::vector<DNodeQ> qnodes;
    // the one-shape leaves' records (DLeafRec, octant 0's order), which their quantized links name
    std::vector<DLeafRec> qleaves;
    double qg0[3] = {0, 0, 0}, qgs[3] = {0, 0, 0};
    float qbound = 0.f;  // >= |every quantized plane| and >= |qg0|
};

constexpr int LIN_MAX = 32;  // JSON shape count up to which the JSON shapes form `lin`

// leaf_max: shapes per BVH leaf (the renderer option "bvh_leaf")
Accel build_accel(const Scene &sc, int json_shapes, int leaf_max = 1);
// Orders a uniform list so that rectangles whose inverse transforms have the same linear part sit next to each
// other, every one after a group's first marked LIN_GROUPED (build_accel does this to Accel::lin)
void group_rectangles(std::vector<int32_t> &lin, const Scene &sc);
// the quantized nodes of a's layouts (build_accel does this for trees of at least BIG_BVH_NODES nodes per layout;
// tests call it for smaller ones)
void build_qnodes(Accel &a, const Scene &sc);

// The quantized nodes' buffer as wf_walk reads it, whole: the grid at byte 0, the eight layouts from byte 64, one
// zeroed DNodeQ after the last layout (the walk reads one node past it), zeros up to qleaf_offset(nodes_per_octant())
// and the one-shape leaves' records from there.  Empty for a tree without quantized nodes.
std::vector<DQGrid> pack_qnodes(const Accel &a);
static_assert(sizeof(DLeafRec) % sizeof(DQGrid) == 0, "pack_qnodes sizes its buffer in DQGrid units");

// The kernels' view (dev::Scene, pt_types.hpp) is filled here and nowhere else, in two parts, from whatever buffers
// the caller holds (device memory in the library, host vectors in the tests' and tools' host builds); the counts and
// bounds come from the Scene / Accel.  `diag` and `guard` belong to the renderer.  A field added to dev::Scene
// must be set by one of the two:
static_assert(sizeof(dev::Scene) == 136, "a new dev::Scene field must be set by view_set_scene or view_set_accel");
// the scene part; tex .. pixels are null for a scene without non-solid textures
inline void view_set_scene(dev::Scene &v, const Scene &sc, const DShape *shapes, const DMaterial *mats,
                           const DTexture *tex, const DPerlin *perlin, const DImage *images, const uint8_t *pixels) {
    v.shapes = shapes;
    v.mats = mats;
    v.tex = tex;
    v.perlin = perlin;
    v.images = images;
    v.pixels = pixels;
    v.nmats = (int)sc.materials.size();
    v.ext = scene_builds(sc).ext;
}
// the acceleration part; qnodes is the pack_qnodes buffer (null without one)
inline void view_set_accel(dev::Scene &v, const DNodeC *nodes, const DQGrid *qnodes, const int32_t *leaf,
                           const int32_t *lin, const int32_t *march, const DBox *boxes, int nnodes, int nlin,
                           int nmarch, float bvh_bound) {
    v.nodes = nodes;
    v.qnodes = qnodes;
    v.leaf = leaf;
    v.lin = lin;
    v.march = march;
    v.boxes = boxes;
    v.nnodes = nnodes;  // per octant layout
    v.nlin = nlin;
    v.nmarch = nmarch;
    v.bvh_bound = bvh_bound;
}
inline void view_set_accel(dev::Scene &v, const Accel &a, const DNodeC *nodes, const DQGrid *qnodes,
                           const int32_t *leaf, const int32_t *lin, const int32_t *march, const DBox *boxes) {
    view_set_accel(v, nodes, qnodes, leaf, lin, march, boxes, a.nodes_per_octant(), (int)a.lin.size(),
                   (int)a.march.size(), a.bvh_bound);
}
// ... of another view (a staged structure's, when it is committed)
inline void view_set_accel(dev::Scene &v, const dev::Scene &a) {
    view_set_accel(v, a.nodes, a.qnodes, a.leaf, a.lin, a.march, a.boxes, a.nnodes, a.nlin, a.nmarch, a.bvh_bound);
}
// The buffers a view's owner frees: the acceleration part's first.
constexpr size_t VIEW_ACCEL_BUFS = 6;
inline std::array<const void *, 13> view_buffers(const dev::Scene &v) {
    return {v.nodes, v.qnodes, v.leaf,   v.lin,    v.march,  v.boxes, v.shapes,
            v.mats,  v.tex,    v.perlin, v.images, v.pixels, v.guard};
}
// A view over host vectors: what a host build of the device functions runs on.  qbuf: pack_qnodes(a), kept by the
// caller.  A pointer is null exactly when its vector is empty.
inline void view_of_host(dev::Scene &v, const Scene &sc, const Accel &a, const std::vector<DShape> &shapes,
                         const std::vector<DMaterial> &mats, const std::vector<DQGrid> &qbuf) {
    auto ptr = [](const auto &vec) { return vec.empty() ? nullptr : vec.data(); };
    view_set_scene(v, sc, ptr(shapes), ptr(mats), ptr(sc.textures), ptr(sc.perlins), ptr(sc.images), ptr(sc.pixels));
    view_set_accel(v, a, ptr(a.cnodes), ptr(qbuf), ptr(a.leaf), ptr(a.lin), ptr(a.march), ptr(a.boxes));
}

// conservative world AABB of one shape (reference get_bounding_box + padding)
DBox shape_box(const HostShape &s);

}  // namespace pt
