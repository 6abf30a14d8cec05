// Test-only host build of the rectangle groups (tests/test_rect_groups_host.py): build_accel orders the uniform
// list so that rectangles whose inverse transforms share the linear part sit next to each other (group_rectangles),
// and closest_nomarch forms a group's products with the ray once.  The same scene is scanned here with the grouped
// list and with a plain one (ids in scene order, nothing marked, so every rectangle computes its own values): both
// must give the same (t, who) for every ray.  Never used by the product.
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../rs-pathtracing_amd/csrc/pt_accel.hpp"
#include "../../rs-pathtracing_amd/csrc/pt_device.hpp"
#include "../../rs-pathtracing_amd/csrc/pt_scene.hpp"

using namespace pt;

struct Bundle {
    Scene sc;
    Accel acc;
    std::vector<int32_t> plain;  // the uniform list before grouping
    std::vector<DQGrid> qbuf;
    std::vector<DShape> shapes;
    std::vector<DMaterial> mats;
    dev::Scene grouped, ungrouped;
};

extern "C" void *h_new(const char *json, size_t len) {
    try {
        Bundle *b = new Bundle();
        b->sc = scene_from_json(json, len, false, 1);
        b->acc = build_accel(b->sc, b->sc.json_shapes);
        for (auto &s : b->sc.shapes) b->shapes.push_back(to_device(s));
        for (auto &m : b->sc.materials) b->mats.push_back(to_device(m));
        view_of_host(b->grouped, b->sc, b->acc, b->shapes, b->mats, b->qbuf);
        for (int32_t e : b->acc.lin) b->plain.push_back(e & LIN_ID_MASK);
        std::sort(b->plain.begin(), b->plain.end());
        b->ungrouped = b->grouped;
        b->ungrouped.lin = b->plain.data();
        return b;
    } catch (...) {
        return nullptr;
    }
}
extern "C" void h_free(void *p) { delete (Bundle *)p; }

// The uniform list as build_accel left it: out[k] = shape id, marked[k] = 1 for a LIN_GROUPED entry, types[k] the
// shape's type.  Returns the list's length (at most cap entries are written).
extern "C" int h_lin(void *p, int32_t *out, int32_t *marked, int32_t *types, int cap) {
    Bundle *b = (Bundle *)p;
    const int n = (int)b->acc.lin.size();
    for (int k = 0; k < n && k < cap; k++) {
        out[k] = b->acc.lin[k] & LIN_ID_MASK;
        marked[k] = (b->acc.lin[k] & LIN_GROUPED) != 0;
        types[k] = b->shapes[out[k]].type;
    }
    return n;
}

// closest_nomarch over n rays (6 doubles each) with the grouped (1) or the plain (0) list; counters: the STATS
// build's event counts summed over the rays.
extern "C" void h_scan(void *p, const double *rays, size_t n, int grouped, double *t, int32_t *who, uint64_t *counters) {
    Bundle *b = (Bundle *)p;
    const dev::Scene &v = grouped ? b->grouped : b->ungrouped;
    Ctr c;
    std::memset(&c, 0, sizeof c);
    for (size_t i = 0; i < n; i++) {
        const dev::Ray r = dev::load_ray(rays, i);
        const dev::V3 inv = dev::v3(1.0 / r.d.x, 1.0 / r.d.y, 1.0 / r.d.z);
        double best = __builtin_inf();
        int w = -1;
        dev::closest_nomarch<true>(v, r, inv, T_MIN, &best, &w, &c);
        t[i] = best;
        who[i] = w;
    }
    for (int k = 0; k < C_COUNT; k++) counters[k] = c.c[k];
}

// group_rectangles on n rectangles whose inverse transforms have the given z rows (rows[3 k ..]) and are the
// identity elsewhere (so the x and y rows are equal throughout and the z rows decide), from the list 0 .. n-1.  out[k] = id, marked[k] as in h_lin.
extern "C" void h_group_rows(const double *rows, int n, int32_t *out, int32_t *marked) {
    Scene sc;
    std::vector<int32_t> lin;
    for (int k = 0; k < n; k++) {
        HostShape s;
        s.type = RECTANGLE;
        for (int i = 0; i < 4; i++)
            for (int j = 0; j < 4; j++) s.direct[i][j] = s.inverse[i][j] = i == j ? 1.0 : 0.0;
        for (int j = 0; j < 3; j++) s.inverse[2][j] = rows[3 * k + j];
        sc.shapes.push_back(s);
        lin.push_back(k);
    }
    group_rectangles(lin, sc);
    for (int k = 0; k < n; k++) {
        out[k] = lin[k] & LIN_ID_MASK;
        marked[k] = (lin[k] & LIN_GROUPED) != 0;
    }
}
