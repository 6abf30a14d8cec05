"""The oracle's hit (u, v) and texture values, per ray, against mpmath at 50 digits (tests/texrays.py) on the ray sets
the GPU file tests/test_gpu_texture_rays.py runs: what makes the oracle more than a second copy of the device's
formulas.  Host code only.

Per case (one light-emitting shape whose `emit` is the texture):
* the object-space point the reference starts from is the oracle's own (through `direct` it is the oracle's world
  point, bit for bit);
* closest_hit's u and v are within 8 * 2^-53 absolute of mpmath's (NaN where the formula leaves acos / asin's domain);
* texture_value selects what mpmath selects (odd / even child, texel) unless mpmath certifies a decision boundary,
  and no random ray of the committed sets sits on one (so the GPU file's "at most 2 excused rays" has none to excuse
  on the reference side); edge rays are on boundaries by construction and only counted;
* a NoiseTexture value is within 4 * 2^-52 of 0.5 (1 + sin(arg)) in mpmath of the f64 argument;
* ray_color(depth=1) returns that texture value and leaves the RNG state alone.
"""
import math

import numpy as np
import pytest

import texrays as T


def run_case(shape, tex):
    osc = T.oracle_scene(shape, tex)
    sh = osc.shape(0)
    rays, edge = T.case_rays(shape, tex, list(sh.direct))
    states = T.ray_states(len(rays))
    out = {"hits": 0, "edge_hits": 0, "certified_random": 0, "certified_edge": 0, "uv_max": 0.0, "noise_max": 0.0,
           "nan_uv": 0, "bad": []}
    torus = T.kind(shape) == "torus"
    for i, ray in enumerate(rays):
        h = osc.closest_hit(ray[:3], ray[3:])
        col, st = osc.ray_color(ray[:3], ray[3:], 1, int(states[i]))
        assert st == int(states[i]), i  # a light draws no random number
        if h is None:
            continue
        if torus and not T.torus_decidable(sh, ray):
            continue
        out["hits"] += 1
        out["edge_hits"] += bool(edge[i])
        p = T.obj_point(sh, ray, h.t)
        T.check_obj_point(sh, p, h)
        val = osc.texture_value(0, h.u, h.v, list(h.point))
        assert list(col) == list(val), i
        if tex != "chk" and tex != "noise":
            for got, want in zip((h.u, h.v), T.mp_uv(sh, p)):
                if want is T.NAN or math.isnan(got):
                    out["nan_uv"] += 1
                    if not ((want is T.NAN and math.isnan(got)) or T.torus_domain_edge(sh, p)):
                        out["bad"].append(("nan", i, got))
                    continue
                err = abs(float(got - want))
                out["uv_max"] = max(out["uv_max"], err)
                if err > T.UV_TOL and not T.torus_domain_edge(sh, p):
                    out["bad"].append(("uv", i, got, err))
        want, boundary = T.reference_at(tex, sh, ray, h)
        if tex == "noise":
            dev = float(np.max(np.abs(val - np.array(want))))
            out["noise_max"] = max(out["noise_max"], dev)
            if dev > T.NOISE_TOL:
                out["bad"].append(("noise", i, dev))
            continue
        if boundary:
            out["certified_edge" if edge[i] else "certified_random"] += 1
        elif list(val) != want:
            out["bad"].append(("select", i, list(val), want))
    out["n"], out["n_edge"] = len(rays), int(edge.sum())
    return out


@pytest.mark.parametrize("shape,tex", T.CASES, ids=T.CASE_IDS)
def test_oracle_uv_and_texture_against_mpmath(shape, tex):
    r = run_case(shape, tex)
    print("%s-%s: %s" % (shape, tex, {k: v for k, v in r.items() if k != "bad"}))
    assert not r["bad"], r["bad"][:5]
    assert r["certified_random"] == 0  # the seeds are chosen so: nothing for the GPU file to excuse
    assert r["uv_max"] <= T.UV_TOL and r["noise_max"] <= T.NOISE_TOL
    # the sets do what they are for: most random rays hit, and the edge rays land
    assert r["hits"] - r["edge_hits"] >= (0.15 if T.kind(shape) in ("torus", "dupin", "rect") else 0.5) * T.N_RANDOM
    if r["n_edge"]:
        assert r["edge_hits"] >= 0.5 * r["n_edge"]


def test_edge_rays_reach_the_edges_they_are_for():
    """The deliberate rays sit where they are meant to: u = 0 and u = 1 on the Sphere's seam, both poles, u * 7 and
    v * 5 on every integer 0..7 / 0..5 of the texel Rectangle, |p| ties on the identity Cube, NaN on the Torus' rings,
    and floor(p.x) beyond 2^31 on the far Rectangle."""
    osc = T.oracle_scene("sphere", "img")
    sh = osc.shape(0)
    rays, edge = T.case_rays("sphere", "img", list(sh.direct))
    hs = [osc.closest_hit(r[:3], r[3:]) for r in rays[edge]]
    us, vs = {h.u for h in hs if h}, {h.v for h in hs if h}
    assert 0.0 in us and 1.0 in us and 0.0 in vs and 1.0 in vs

    osc = T.oracle_scene("rect_texel", "img")
    sh = osc.shape(0)
    rays, edge = T.case_rays("rect_texel", "img", list(sh.direct))
    hs = [osc.closest_hit(r[:3], r[3:]) for r in rays[edge]]
    assert all(h is not None for h in hs)
    assert {round(h.u * T.IMG_W, 9) for h in hs} == set(range(T.IMG_W + 1))
    assert {round(h.v * T.IMG_H, 9) for h in hs} == set(range(T.IMG_H + 1))
    assert {h.u for h in hs} >= {0.0, 1.0} and {h.v for h in hs} >= {0.0, 1.0}

    osc = T.oracle_scene("cube", "img")
    sh = osc.shape(0)
    rays, edge = T.case_rays("cube", "img", list(sh.direct))
    ties = 0
    for r in rays[edge]:
        h = osc.closest_hit(r[:3], r[3:])
        if h is not None:
            a = sorted(abs(c) for c in T.obj_point(sh, r, h.t))
            ties += a[2] == a[1]
    assert ties >= 20

    osc = T.oracle_scene("torus", "uv")
    sh = osc.shape(0)
    rays, edge = T.case_rays("torus", "uv", list(sh.direct))
    nan = near = 0
    for r in rays[edge]:
        h = osc.closest_hit(r[:3], r[3:])
        if h is not None:
            nan += math.isnan(h.v)
            near += abs(abs(T.obj_point(sh, r, h.t)[2]) - sh.tube_radius) < 1e-12
    assert near >= 40 and nan >= 1

    osc = T.oracle_scene("rect_far", "noise")
    sh = osc.shape(0)
    rays, _ = T.case_rays("rect_far", "noise", list(sh.direct))
    hs = [osc.closest_hit(r[:3], r[3:]) for r in rays]
    assert sum(h is not None and math.floor(h.point[0]) > 2 ** 31 for h in hs) >= 0.15 * len(rays)
