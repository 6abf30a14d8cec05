"""Adversarial rays for the exact skipping march (pt_march.hpp), shared by the
host-build test (test_march_adversarial.py) and the GPU test
(test_gpu_fullframe.py).  Each family aims at a place where the closed-form
accumulation or the Bernstein sign proof could differ from the reference's
literal march (src/world/shapes/ray_marching.rs:20-74):

* grazing: rays tangent to the Heart surface, shifted along the normal by
  0, +-1e-12 .. +-1e-3 of the object scale (f stays within a hair of 0 for
  many steps: the proof margin is what decides);
* frozen / zero-crossing: object-space rays with a direction component
  exactly 0 (that coordinate never changes: the c == 0 closed form), rays
  lying in a coordinate plane, and rays through the object origin (every
  coordinate crosses 0 at once: no binade segment is long there);
* binade edges: origins with power-of-two coordinates and directions that
  keep a coordinate on a binade edge for a while;
* scale: the same families at cornell's 82.5x Heart and at scale 1.

The second half restates the families for any marched function (CASES,
object_rays_for) and holds what the tests of the other five functions share
(test_marched_adversarial.py on the host build, test_gpu_marched_adversarial.py
on the GPU): the scenes, the oracle's hits and colours computed once per
setting, and a comparison of hits in which NaN equals NaN.
"""
import functools
import json

import numpy as np

HEART_XF = {"translate": [212.5, 200, 147.5], "rotate": [-95, -18, 0], "scale": [82.5, 82.5, 82.5]}
UNIT_XF = {"translate": [0, 0, 0], "rotate": [0, 0, 0], "scale": [1, 1, 1]}
SCALED_XF = {"translate": [0, 0, 0], "rotate": [0, 0, 0], "scale": [82.5, 82.5, 82.5]}


def heart_json(xf, step=0.01, depth=None):
    sh = {"type": "BruteForsableShape", "name": "Heart", "shape": {"type": "Heart", "sphere_radius": 1.45},
          "step": step, "transform": xf, "material": "Red"}
    if depth is not None:
        sh["depth"] = depth
    return json.dumps({
        "camera": {"position": [278, 278, -800], "direction": [0, 0, 1], "up": [0, 1, 0], "fov": 40,
                   "focal_length": 1},
        "shapes": [sh],
        "materials": {"Red": {"type": "Lambertian", "albedo": {"type": "SolidColor", "color": [0.65, 0.05, 0.05]}}},
        "background": [0, 0, 0]})


def heart_f(p):
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    a = x * x + 2.25 * y * y + z * z - 1.0
    return a ** 3 - x * x * z ** 3 - 0.1125 * y * y * z ** 3


def heart_grad(p, h=1e-7):
    g = np.zeros_like(p)
    for k in range(3):
        e = np.zeros(3)
        e[k] = h
        g[..., k] = (heart_f(p + e) - heart_f(p - e)) / (2 * h)
    return g


def surface_points(rng, n):
    """Points on f = 0 along random directions from the object origin (f(0) = -1)."""
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    lo = np.zeros(n)
    hi = np.full(n, 1.6)
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        inside = heart_f(u * mid[:, None]) < 0
        lo = np.where(inside, mid, lo)
        hi = np.where(inside, hi, mid)
    return u * lo[:, None]


def object_rays(rng, n_graze=400):
    """(origin, direction) pairs in object space, not normalised."""
    rays = []
    # grazing: tangent at a surface point, shifted along the normal
    p = surface_points(rng, n_graze)
    g = heart_grad(p)
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    t = np.cross(g, rng.normal(size=(n_graze, 3)))
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    shifts = np.array([0.0, 1e-12, -1e-12, 1e-9, -1e-9, 1e-6, -1e-6, 1e-3, -1e-3])
    s = shifts[rng.integers(0, len(shifts), n_graze)]
    o = p + g * s[:, None] - 2.5 * t
    rays += [np.concatenate([o, t], 1)]
    # frozen coordinates and coordinate planes: one or two direction components exactly 0
    m = 240
    o = rng.uniform(-3, 3, size=(m, 3))
    d = rng.normal(size=(m, 3))
    for i in range(m):
        k = i % 3
        d[i, k] = 0.0
        if i % 2 == 0:
            o[i, k] = 0.0  # the frozen coordinate sits exactly at 0
        if i % 5 == 0:
            d[i, (k + 1) % 3] = 0.0
    aim = -o + rng.normal(scale=0.3, size=(m, 3))  # point roughly back at the heart
    for i in range(m):
        for k in range(3):
            if d[i, k] != 0.0:
                d[i, k] = aim[i, k]
    rays += [np.concatenate([o, d], 1)]
    # through the object origin: every coordinate crosses 0 together
    m = 120
    d = rng.normal(size=(m, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = -d * rng.uniform(1.6, 4.0, size=(m, 1))
    rays += [np.concatenate([o, d], 1)]
    # binade edges: power-of-two origins, one direction component tiny
    m = 120
    pw = 2.0 ** rng.integers(-3, 2, size=(m, 3)) * rng.choice([-1.0, 1.0], size=(m, 3))
    d = -pw + rng.normal(scale=0.05, size=(m, 3))
    d[np.arange(m), rng.integers(0, 3, m)] *= 1e-9
    rays += [np.concatenate([pw * 2.0, d], 1)]
    return np.concatenate(rays)


def world_rays(direct, obj):
    """World rays (normalised directions) for object-space rays under `direct` (4x4 row-major)."""
    D = np.asarray(direct, float).reshape(4, 4)
    o = obj[:, :3] @ D[:3, :3].T + D[:3, 3]
    d = obj[:, 3:] @ D[:3, :3].T
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([o, d], 1)


# ------------------------------------------------------------------------------------- every marched function
# Sine, Star, DupinCyclide, HuntsSurface and Cushion (ray_marching.rs:185-520) go through the generic march (the
# F_ANY builds) inside a sphere of the JSON sphere_radius.  What the Heart does not have: singular lines and points
# (the Sine is exactly 0 with a zero gradient on x = +-y, z = 0 and its permutations; the Cushion and the Sine are
# singular at the origin), |f| in the thousands (Hunts), and a bound that the scene file chooses.

def _xyz(p):
    return p[..., 0], p[..., 1], p[..., 2]


def sine_f(a):
    def f(p):
        x, y, z = _xyz(p)
        return a * a * (x - y - z) * (x + y - z) * (x - y + z) * (x + y + z) + 4.0 * x * x * y * y * z * z
    return f


def star_f(a):
    def f(p):
        x, y, z = _xyz(p)
        x2, y2, z2 = x * x, y * y, z * z
        return a * (x2 * y2 + x2 * z2 + y2 * z2) + (x2 + y2 + z2 - 1.0) ** 3
    return f


def dupin_f(a, b, c, d):
    def f(p):
        x, y, z = _xyz(p)
        e = x * x + y * y + z * z + b * b - d * d
        g = a * x - c * d
        return e * e - 4.0 * (g * g + b * b * y * y)
    return f


def hunts_f(p):
    x, y, z = _xyz(p)
    x2, y2, z2 = x * x, y * y, z * z
    return 4.0 * (x2 + y2 + z2 - 13.0) ** 3 + 27.0 * (3.0 * x2 + y2 - 4.0 * z2 - 12.0) ** 2


def cushion_f(p):
    x, y, z = _xyz(p)
    x2, y2, z2 = x * x, y * y, z * z
    return (z2 * x2 - z2 * z2 - 2.0 * z * x2 + 2.0 * z * z2 + x2 - z2 - (x2 - z) ** 2 - y2 * y2 - 2.0 * x2 * y2
            - y2 * z2 + 2.0 * y2 * z + y2)


def _plane_points(radius):
    """The Sine at a = 0 is 4 x^2 y^2 z^2 >= 0: it has no sign change to bisect, its zero set is the three
    coordinate planes.  Points in them, with the plane's normal in place of the (zero) gradient."""
    def surface(rng, n):
        p = rng.uniform(-0.6 * radius, 0.6 * radius, size=(n, 3))
        g = np.zeros((n, 3))
        k = np.arange(n) % 3
        p[np.arange(n), k] = 0.0
        g[np.arange(n), k] = 1.0
        return p, g
    return surface


MATERIALS = {  # scenes/marched.json's
    "Chalk": {"type": "Lambertian", "albedo": {"type": "SolidColor", "color": [0.8, 0.8, 0.75]}},
    "Copper": {"type": "Metal", "albedo": {"type": "SolidColor", "color": [0.8, 0.5, 0.3]}, "fuzz": 0.2},
    "Glass": {"type": "Dielectric", "index_of_refraction": 1.5},
    "Steel": {"type": "Metal", "albedo": {"type": "SolidColor", "color": [0.6, 0.6, 0.65]}, "fuzz": 0},
}


def _case(name, material, f, shape, **more):
    return dict(name=name, material=material, f=f, shape=shape, radius=shape["sphere_radius"], **more)


_DUPIN = dict(a=1.11, b=0.99, c=0.5, d=0.1)
_PINCH = dict(a=1.0, b=0.8, c=0.6, d=0.6)  # d = c: a cyclide with pinch points
# The oracle's hits of the marched shape at step 0.01, depth 4 and the identity transform, of the 576 rays of
# case_rays(): total | grazing, frozen, origin, axis | hits with a NaN normal at identity + scale 40 + rotated
# (test_marched_adversarial.py::test_oracle_hits_enough prints every transform and family and asserts the floors):
#   sine        419 | 199  60 60 48 |   8 +   8 + 0      star_a8     318 |  50 112 60 54 | 0
#   star        384 |  82 120 60 54 |   0                star_r09      0 (see below)
#   dupin       191 |  67  66 15 24 |   0                star_r12    154 | 111  22  2 18 | 0
#   hunts       460 | 164 113 60 54 |   0                dupin_pinch 332 |  60 104 60 54 | 0
#   cushion     378 | 109 107 60 52 |   0                hunts_r2    212 |  45  61 31 30 | 0
#   sine_a0     360 | 174  60 60 54 | 138 + 138 + 1      cushion_r6  274 |  99  42 60 52 | 0
#   sine_a3     438 | 200  59 60 48 |   8 +   8 + 0
CASES = [
    # scenes/marched.json's parameters
    _case("sine", "Chalk", sine_f(1.0), {"type": "Sine", "a": 1.0, "sphere_radius": 1.5}),
    _case("star", "Glass", star_f(-1.0), {"type": "Star", "a": -1.0, "sphere_radius": 1.6}),
    _case("dupin", "Copper", dupin_f(**_DUPIN), dict({"type": "DupinCyclide", "sphere_radius": 2.5}, **_DUPIN)),
    _case("hunts", "Steel", hunts_f, {"type": "HuntsSurface", "sphere_radius": 4.0}),
    _case("cushion", "Chalk", cushion_f, {"type": "Cushion", "sphere_radius": 1.5}),
    # parameter variants
    _case("sine_a0", "Chalk", sine_f(0.0), {"type": "Sine", "a": 0.0, "sphere_radius": 1.5},
          surface=_plane_points(1.5)),
    _case("sine_a3", "Chalk", sine_f(3.0), {"type": "Sine", "a": 3.0, "sphere_radius": 2.5}),
    _case("star_a8", "Glass", star_f(8.0), {"type": "Star", "a": 8.0, "sphere_radius": 1.2}),
    # a bound inside the solid: with a = -1, f = -(x2 y2 + x2 z2 + y2 z2) + (r2 - 1)^3 < 0 wherever r < 1, so the
    # whole surface (r from 1 on the axes to 1.49 on the diagonals) lies outside this sphere and every march starts
    # and ends inside the solid.  The grazing rays are placed at the surface all the same (search).
    _case("star_r09", "Glass", star_f(-1.0), {"type": "Star", "a": -1.0, "sphere_radius": 0.9}, search=1.6),
    # ... and the bound that the surface does poke out of: the arms leave it, the axes' dents stay inside
    _case("star_r12", "Glass", star_f(-1.0), {"type": "Star", "a": -1.0, "sphere_radius": 1.2}),
    _case("dupin_pinch", "Copper", dupin_f(**_PINCH), dict({"type": "DupinCyclide", "sphere_radius": 2.5}, **_PINCH)),
    _case("hunts_r2", "Steel", hunts_f, {"type": "HuntsSurface", "sphere_radius": 2.0}),
    _case("cushion_r6", "Chalk", cushion_f, {"type": "Cushion", "sphere_radius": 6.0}),
]
CASE = {c["name"]: c for c in CASES}
# star_r09 cannot be hit at a step of 0.01 (above); every other case is held to the floors
NEVER_HIT = ("star_r09",)

FAMILIES = ("grazing", "frozen", "origin", "axis", "pow2", "bound_tangent", "bound_origin")
MUST_HIT = ("grazing", "frozen", "origin", "axis")
SHIFTS = np.array([0.0, 1e-12, -1e-12, 1e-9, -1e-9, 1e-6, -1e-6, 1e-3, -1e-3])
AXES = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [1, 0, 1], [0, 1, 1], [1, 1, 1], [1, -1, 0],
                 [1, 1, -1]], float)


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _in_ball(rng, n, radius):
    return _unit(rng.normal(size=(n, 3))) * (radius * rng.uniform(size=(n, 1)) ** (1.0 / 3.0))


def gradient_of(f, p, h=1e-6):
    g = np.zeros_like(p)
    for k in range(3):
        e = np.zeros(3)
        e[k] = h
        g[..., k] = (f(p + e) - f(p - e)) / (2 * h)
    return g


def surface_points_of(case, rng, n):
    """n points on f = 0 and unit normals there: the first sign change of f along random chords of the ball
    (`search`, by default the bound), bisected."""
    if "surface" in case:
        return case["surface"](rng, n)
    f, radius = case["f"], case.get("search", case["radius"])
    found = []
    for _ in range(40):
        a, b = _in_ball(rng, 4 * n, radius), _in_ball(rng, 4 * n, radius)
        s = np.linspace(0.0, 1.0, 65)
        v = f(a[:, None, :] + (b - a)[:, None, :] * s[None, :, None])
        change = v[:, :-1] * v[:, 1:] < 0
        rows = np.nonzero(change.any(1))[0]
        first = change[rows].argmax(1)
        lo, hi = s[first], s[first + 1]
        a, b, neg = a[rows], b[rows], v[rows, first] < 0
        for _ in range(80):
            mid = 0.5 * (lo + hi)
            same = (f(a + (b - a) * mid[:, None]) < 0) == neg
            lo, hi = np.where(same, mid, lo), np.where(same, hi, mid)
        found.append(a + (b - a) * lo[:, None])
        if sum(len(x) for x in found) >= n:
            break
    p = np.concatenate(found)[:n]
    assert len(p) == n, "no surface of %s along the chords" % case["name"]
    g = gradient_of(f, p)
    flat = np.linalg.norm(g, axis=1) < 1e-9  # a singular point: any direction serves
    g[flat] = rng.normal(size=(int(flat.sum()), 3))
    return p, _unit(g)


def object_rays_for(case, rng, n_graze=200):
    """(rays, family): (origin, direction) pairs in the case's object space, not normalised, and each ray's index
    into FAMILIES.  Deterministic from the generator."""
    R = case["radius"]
    rays, fam = [], []

    def add(name, o, d):
        rays.append(np.concatenate([o, d], 1))
        fam.append(np.full(len(o), FAMILIES.index(name)))

    # grazing: tangent at a surface point, shifted along the gradient
    p, g = surface_points_of(case, rng, n_graze)
    t = _unit(np.cross(g, rng.normal(size=(n_graze, 3))))
    s = SHIFTS[rng.integers(0, len(SHIFTS), n_graze)]
    add("grazing", p + g * s[:, None] - 2.2 * case.get("search", R) * t, t)
    # frozen coordinates: one or two direction components exactly 0, the frozen coordinate at exactly 0 for half
    m = 120
    o = rng.uniform(-2 * R, 2 * R, size=(m, 3))
    d = rng.normal(size=(m, 3))
    for i in range(m):
        k = i % 3
        d[i, k] = 0.0
        o[i, k] = 0.0 if i % 2 == 0 else rng.uniform(-0.5 * R, 0.5 * R)
        if i % 5 == 0:
            d[i, (k + 1) % 3] = 0.0
            o[i, (k + 1) % 3] = rng.uniform(-0.5 * R, 0.5 * R)
    aim = -o + rng.normal(scale=0.2 * R, size=(m, 3))  # roughly back at the shape
    d = np.where(d != 0.0, aim, 0.0)
    add("frozen", o, d)
    # through the object origin: every coordinate crosses 0 together
    m = 60
    d = _unit(rng.normal(size=(m, 3)))
    add("origin", -d * rng.uniform(1.1 * R, 2.5 * R, size=(m, 1)), d)
    # along the axes and diagonals through the origin (the singular lines), exactly, and 1e-9 and 1e-3 beside them
    o, d = [], []
    for v in AXES:
        k = int(np.argmin(np.abs(v)))
        side = _unit(np.cross(v, np.eye(3)[k]))
        for sign in (1.0, -1.0):
            for off in (0.0, 1e-9, 1e-3):
                o.append(-8.0 * sign * v + off * side)  # 8 v is exact and outside every bound here
                d.append(sign * v)
    add("axis", np.array(o), np.array(d))
    # binade edges: power-of-two origins, one direction component tiny
    m = 60
    pw = 2.0 ** rng.integers(-3, 2, size=(m, 3)) * rng.choice([-1.0, 1.0], size=(m, 3))
    d = -pw + rng.normal(scale=0.05, size=(m, 3))
    d[np.arange(m), rng.integers(0, 3, m)] *= 1e-9
    add("pow2", pw * 2.0, d)
    # tangent to the bound sphere (disc zero or tiny), and just inside and outside it
    o, d = [], []
    for eps in (0.0, 1e-15, -1e-15, 1e-9, -1e-9, -1e-3):
        r = R * (1.0 + eps)
        for k in range(3):  # axis-parallel: at eps = 0 the discriminant is exactly 0
            e, u = np.eye(3)[k], np.eye(3)[(k + 1) % 3]
            o.append(r * e - 3.0 * u)
            d.append(u)
        q = _unit(rng.normal(size=(4, 3)))
        u = _unit(np.cross(q, rng.normal(size=(4, 3))))
        o += list(r * q - 2.0 * R * u)
        d += list(u)
    add("bound_tangent", np.array(o), np.array(d))
    # origins exactly on the bound sphere, and inside it
    m = 20
    q = _unit(rng.normal(size=(m, 3)))
    add("bound_origin", R * q, -q + rng.normal(scale=0.5, size=(m, 3)))
    add("bound_origin", _in_ball(rng, m, R), rng.normal(size=(m, 3)))
    return np.concatenate(rays), np.concatenate(fam)


# ----------------------------------------------------------------------------- scenes, settings and the oracle
IDENT_XF = UNIT_XF
SCALE40_XF = {"translate": [0, 0, 0], "rotate": [0, 0, 0], "scale": [40, 40, 40]}
# (step, depth) of a march: the scene files' setting, coarse, fine, backwards, one pass, no pass, and a step longer
# than many chords
SETTINGS = [(0.01, 4), (0.05, 3), (0.003, 4), (-0.01, 4), (0.01, 1), (0.01, 0), (0.5, 4)]
FLOOR_SETTING = (0.01, 4)
MIN_HITS, MIN_NAN_NORMALS = 100, 4
# Rays on which the reference's literal march does not end (the oracle runs for minutes): left out by case and
# index into case_rays(), each with its reason; at most 2 per case.
LEFT_OUT = {}


def transforms():
    from texrays import ROT
    return {"identity": IDENT_XF, "scale40": SCALE40_XF, "rot": ROT}


def marched_json(case, xf, step, depth):
    """One marched shape under `xf` and a camera looking at it (the reference's sky colours the paths that leave,
    whatever `background` says: src/world/mod.rs:199-202)."""
    reach = 4.0 * case["radius"] * max(xf["scale"])
    tr = xf["translate"]
    return json.dumps({
        "camera": {"position": [tr[0], tr[1], tr[2] - reach], "direction": [0, 0, 1], "up": [0, 1, 0], "fov": 40,
                   "focal_length": 1},
        "shapes": [{"type": "BruteForsableShape", "name": case["name"], "shape": case["shape"], "step": step,
                    "depth": depth, "transform": xf, "material": case["material"]}],
        "materials": {case["material"]: MATERIALS[case["material"]]},
        "background": [0, 0, 0]})


@functools.lru_cache(maxsize=None)
def case_text(name, xf, step, depth):
    return marched_json(CASE[name], transforms()[xf], step, depth)


@functools.lru_cache(maxsize=None)
def case_scene(name, xf, step, depth):
    import oracle as O
    return O.Scene(case_text(name, xf, step, depth), random_spheres=False)


@functools.lru_cache(maxsize=None)
def case_rays(name, xf):
    """(world rays, family) of a case under a transform: the same object-space rays under every transform; shared
    and never written to."""
    k = [c["name"] for c in CASES].index(name)
    obj, fam = object_rays_for(CASE[name], np.random.default_rng(1900 + k))
    keep = np.setdiff1d(np.arange(len(obj)), LEFT_OUT.get(name, []))
    rays = world_rays(case_scene(name, xf, *FLOOR_SETTING).shape(0).direct, obj[keep])
    rays.setflags(write=False)
    return rays, fam[keep]


HITS = np.dtype([("shape", "<i4"), ("t", "<f8"), ("point", "<f8", 3), ("normal", "<f8", 3), ("front_face", "<i4")])


def hit_records(n):
    out = np.zeros(n, dtype=HITS)
    out["shape"] = -1
    return out


def oracle_hit_records(osc, rays):
    out = hit_records(len(rays))
    for i, ray in enumerate(rays):
        h = osc.closest_hit(ray[:3], ray[3:])
        if h is not None:
            out[i] = (h.shape, h.t, list(h.point), list(h.normal), h.front_face)
    return out


def gpu_hit_records(got):
    """HipRenderer.closest_hit's records (HIT_DTYPE) as HITS."""
    out = hit_records(len(got))
    hit = got["shape"] >= 0
    for k in HITS.names:
        out[k][hit] = got[k][hit]
    return out


def hit_differences(got, want):
    """Indices at which two HITS arrays differ: a miss against a hit, another shape, or another t, point, normal or
    front face, where NaN equals NaN (a hit at a singular point has the normalised zero gradient for its normal)."""
    assert len(got) == len(want)
    bad = []
    for i in range(len(want)):
        g, w = got[i], want[i]
        if g["shape"] != w["shape"]:
            bad.append(i)
        elif w["shape"] >= 0 and not all(np.array_equal(g[k], w[k], equal_nan=True)
                                         for k in ("t", "point", "normal", "front_face")):
            bad.append(i)
    return bad


@functools.lru_cache(maxsize=None)
def oracle_hits(name, xf, step, depth):
    """The oracle's closest hits of case_rays(name, xf) at a march setting; computed once, never written to."""
    out = oracle_hit_records(case_scene(name, xf, step, depth), case_rays(name, xf)[0])
    out.setflags(write=False)
    return out


PATH_DEPTH = 8


@functools.lru_cache(maxsize=None)
def oracle_paths(name, xf):
    """(rng states before, colours, rng states after) of Scene.ray_color at PATH_DEPTH over case_rays(name, xf), at
    FLOOR_SETTING, one generator state per ray."""
    rays, _ = case_rays(name, xf)
    osc = case_scene(name, xf, *FLOOR_SETTING)
    k = [c["name"] for c in CASES].index(name)
    before = np.random.default_rng(2900 + k).integers(0, 2 ** 63, size=len(rays), dtype=np.uint64)
    col, after = np.zeros((len(rays), 3)), np.zeros(len(rays), dtype=np.uint64)
    for i, ray in enumerate(rays):
        col[i], after[i] = osc.ray_color(ray[:3], ray[3:], PATH_DEPTH, int(before[i]))
    for a in (before, col, after):
        a.setflags(write=False)
    return before, col, after


def hit_counts(name, xf):
    """The oracle alone at FLOOR_SETTING: (hits of the marched shape, {family: hits}, hits with a NaN normal)."""
    h, fam = oracle_hits(name, xf, *FLOOR_SETTING), case_rays(name, xf)[1]
    hit = h["shape"] == 0
    by = {f: int(np.sum(hit & (fam == k))) for k, f in enumerate(FAMILIES)}
    return int(hit.sum()), by, int(np.sum(hit & np.isnan(h["normal"]).any(1)))
