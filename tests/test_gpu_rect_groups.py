"""The rectangle groups on the GPU, bit for bit against the oracle.

closest_nomarch tests rectangles whose inverse transforms share the linear part from one set of products with the
ray (dz and its fellows, formed by the group's first rectangle).  Every value must be the one the ungrouped test
gives: closest hits on a scene of parallel rectangles, a rotated cube and a sphere, for ordinary rays and for the
rays that make a divisor zero or leave the ordinary range, and whole frames through both engines (the sphere scene's
too: its uniform list holds no rectangle, and nothing about it may move).
"""
import json

import numpy as np
import pytest

import oracle as O
from conftest import host_threads

pytestmark = pytest.mark.gpu

NRAYS = 4096


def rect(t, rot, x0=-2.0, x1=2.0, y0=-2.0, y1=2.0, s=(1, 1, 1)):
    return {"type": "Rectangle", "x0": x0, "x1": x1, "y0": y0, "y1": y1,
            "transform": {"translate": list(t), "rotate": list(rot), "scale": list(s)}, "material": "M"}


def group_scene():
    """Three parallel rectangles facing z (unrotated: the z row is (0, 0, 1), so a direction in their plane has
    dz = +-0 exactly), two parallel ones turned 90 degrees about y, a rotated cube and a sphere."""
    shapes = [rect((0, 0, 4), (0, 0, 0)), rect((0.5, 0, 0), (0, 90, 0)), rect((0, 0.25, 6), (0, 0, 0)),
              {"type": "Cube", "name": "C", "transform": {"translate": [0.3, -0.2, 1.0], "rotate": [20, 35, 10],
                                                           "scale": [0.6, 0.4, 0.5]}, "material": "M"},
              rect((-1.5, 0, 0), (0, 90, 0)), rect((0, -0.25, 5), (0, 0, 0)),
              {"type": "Sphere", "name": "S", "transform": {"translate": [-0.6, 0.5, 2.0], "rotate": [0, 0, 0],
                                                             "scale": [0.5, 0.5, 0.5]}, "material": "M"}]
    return json.dumps({
        "camera": {"position": [0, 0, -5], "direction": [0, 0, 1], "up": [0, 1, 0], "fov": 40, "focal_length": 1},
        "shapes": shapes, "materials": {"M": {"type": "EmptyMaterial"}}, "background": [0, 0, 0]})


def group_rays():
    rng = np.random.default_rng(41)
    n = NRAYS // 8

    def unit(d):
        return d / np.linalg.norm(d, axis=1, keepdims=True)

    parts = []
    o = rng.uniform([-2, -2, -3], [2, 2, 7], size=(3 * n, 3))            # ordinary rays
    parts.append(np.concatenate([o, unit(rng.normal(size=(3 * n, 3)))], axis=1))
    o = rng.uniform([-2, -2, -3], [2, 2, 7], size=(n, 3))                  # origins on a wall's plane
    o[: n // 2, 2] = rng.choice([4.0, 6.0, 5.0], n // 2)
    o[n // 2:, 0] = rng.choice([0.5, -1.5], n - n // 2)
    parts.append(np.concatenate([o, unit(rng.normal(size=(n, 3)))], axis=1))
    o = rng.uniform([-2, -2, -3], [2, 2, 7], size=(n, 3))                  # directions parallel to a wall
    d = rng.normal(size=(n, 3))
    d[: n // 2, 2] = rng.choice([0.0, -0.0], n // 2)
    d[n // 2:, 0] = rng.choice([0.0, -0.0], n - n // 2)
    parts.append(np.concatenate([o, unit(d)], axis=1))
    o = rng.uniform([-2, -2, -3], [2, 2, 7], size=(n, 3))                  # grazing directions
    d = rng.normal(size=(n, 3))
    k = rng.integers(0, 3, n)
    d[np.arange(n), k] = rng.choice([1e-9, -1e-12, 1e-16, -1e-150, 1e-300, -5e-324], n)
    parts.append(np.concatenate([o, unit(d)], axis=1))
    o = rng.uniform([-2, -2, -3], [2, 2, 7], size=(n, 3))                  # a component of 1e300
    d = unit(rng.normal(size=(n, 3)))
    k = rng.integers(0, 3, n)
    big = rng.choice([1e300, -1e300], n)
    o[: n // 2][np.arange(n // 2), k[: n // 2]] = big[: n // 2]
    d[n // 2:][np.arange(n - n // 2), k[n // 2:]] = big[n // 2:]
    parts.append(np.concatenate([o, d], axis=1))
    tgt = rng.uniform([-0.4, -0.7, 0.4], [1.0, 0.4, 1.7], size=(n, 3))    # aimed at the cube and the sphere
    tgt[n // 2:] = rng.uniform([-1.1, 0.0, 1.5], [-0.1, 1.0, 2.5], size=(n - n // 2, 3))
    o = rng.uniform([-2, -2, -3], [2, 2, 3.5], size=(n, 3))
    parts.append(np.concatenate([o, unit(tgt - o)], axis=1))
    rays = np.ascontiguousarray(np.concatenate(parts))
    assert len(rays) == NRAYS
    return rays


SPHERE_ID = 6


def oracle_hit(osc, ray):
    """The oracle's closest hit.  A component of 1e300 makes the sphere's discriminant inf - inf, and the reference's
    range test lets the NaN root through as a hit that replaces any other (the sphere is the last shape).  The GPU
    path has never followed the reference there: the uniform list tests a sphere's padded box first, which such a
    ray misses.  For those rays the expectation is the oracle's closest hit over the other shapes, by the linear
    scan's rule (nearest, the later shape on a tie): what this test is about, the grouped rectangles' values for
    such a ray, is checked on them all the same."""
    h = osc.closest_hit(ray[:3], ray[3:])
    if h is None or h.t == h.t:
        return h
    assert h.shape == SPHERE_ID
    best = None
    for i in range(SPHERE_ID):
        g = osc.shape_hit(i, ray[:3], ray[3:])
        if g is not None:
            assert g.t == g.t
            g.shape = i
            if best is None or g.t <= best.t:
                best = g
    return best


def test_grouped_rectangles_cube_and_sphere_hits_per_ray(pt):
    text = group_scene()
    osc = O.Scene(text, random_spheres=False)
    ps = pt.Scene.from_json(text, random_spheres=False)
    rays = group_rays()
    with np.errstate(all="ignore"):
        got = pt.HipRenderer(ps, depth=8).closest_hit(rays)
    hits = [oracle_hit(osc, r) for r in rays]
    want_who = np.array([-1 if h is None else h.shape for h in hits])
    want_t = np.array([0.0 if h is None else h.t for h in hits])
    hit = want_who >= 0
    per_shape = np.bincount(want_who[hit], minlength=7)
    print("hits per shape:", per_shape, "misses:", (~hit).sum())
    assert np.all(per_shape >= 20)  # every shape is somebody's closest hit
    assert not np.isnan(want_t).any()
    bad = np.flatnonzero((got["shape"] != want_who) | (hit & (got["t"].view(np.uint64) != want_t.view(np.uint64))))
    assert len(bad) == 0, "%d of %d rays differ, first %d: %r got (%r, %d) want (%r, %d)" % (
        len(bad), NRAYS, bad[0], list(rays[bad[0]]), got["t"][bad[0]], got["shape"][bad[0]], want_t[bad[0]],
        want_who[bad[0]])
    for i in np.flatnonzero(hit)[::7]:  # and what finish() normalizes
        assert list(got["normal"][i]) == list(hits[i].normal) and list(got["point"][i]) == list(hits[i].point), i


@pytest.fixture(scope="module")
def frames(pt, cornell_text, spheres_text):
    """scene name -> (GPU scene, oracle frame) at 64x64, 4 spp, depth 8: the oracle renders each once"""
    out = {}
    for name, text, seed in (("cornell", cornell_text, 1), ("spheres", spheres_text, 3)):
        ref = O.Scene(text, seed=seed).render(64, 64, 4, 8, 17, threads=host_threads())
        out[name] = (pt.Scene.from_json(text, seed=seed), ref)
    return out


@pytest.mark.parametrize("engine", [2, 1], ids=["wavefront", "megakernel"])
@pytest.mark.parametrize("name", ["cornell", "spheres"])
def test_frames_bit_for_bit(pt, frames, name, engine):
    ps, ref = frames[name]
    r = pt.HipRenderer(ps, depth=8)
    r.set_option("engine", engine)
    img = r.render(ps.camera(), pt.ImageParams(64, 64), 4, seed=17)
    assert np.all(np.isfinite(img)) and img.mean() > 0.01
    same = np.all(img.view(np.uint64) == ref.view(np.uint64), axis=1)
    assert same.all(), "%d of %d pixels differ" % ((~same).sum(), len(same))
