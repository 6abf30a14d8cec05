"""Shared helpers of the per-ray texture and Torus tests (tests/test_texture_exact.py,
tests/test_gpu_texture_rays.py, tests/test_gpu_torus_rays.py): the scenes, the ray sets and an independent mpmath
reference (50 digits) of hit_uv / tex_value.

A DiffuseLight whose `emit` is a texture returns tex_value(hit_uv(...), point) as the leaf of ray_color(depth=1)
(material.rs:135-137): one texture lookup per ray, no random number, no bounce.

The mpmath reference starts from the f64 object-space point of the oracle's hit.  The oracle does not hand that
point out, so it is recomputed here in Python floats with the oracle's own operation order (inverse * origin +
(inverse * direction) * t: one IEEE operation per source operation on both sides) and proven to be the oracle's:
taken through `direct` it must give the oracle's world point bit for bit (check_obj_point).  Taking the world point
back through `inverse` instead would cost a few ulp of the coordinates, which acos near a pole or atan2 near the
seam amplify beyond the 8 * 2^-53 the (u, v) check asks for.  From that point on every math-library call (acos,
atan2, asin, cos, sin) is mpmath's; the f64 constants of the formulas (PI = 3.141592653589793, the multipliers) and
the f64 products that feed a sine directly (CheckerTexture, NoiseTexture) stay as the formulas have them.
"""
import ctypes as C
import json
import math

import mpmath as mp
import numpy as np

import oracle as O

mp.mp.dps = 50
PI = mp.mpf(math.pi)  # the formulas' f64 constant
ODD, EVEN = [0.1, 0.2, 0.8], [0.9, 0.2, 0.1]
BOUNDARY = 1e-12  # the project's TEX_REL: > 10x the 40 pi 2^-51 a 2-ulp acos / atan2 moves a sine's argument
UV_TOL = 8 * 2.0 ** -53
NOISE_TOL = 4 * 2.0 ** -52  # half of a 2-ulp sine of magnitude <= 1, plus two roundings
SCENE_SEED = 1

IMG_NAME, IMG_W, IMG_H = "mem7x5.png", 7, 5
# every texel distinct in every channel pair: r names the column, g the row, b both
IMG_RGBA = bytes(c for y in range(IMG_H) for x in range(IMG_W)
                 for c in (5 + 30 * x, 3 + 50 * y, 7 * (x + IMG_W * y), 255))
IMAGES = {IMG_NAME: (IMG_W, IMG_H, IMG_RGBA)}


def _solid(c):
    return {"type": "SolidColor", "color": c}


TEXTURES = {
    "uv": {"type": "UVChecker", "odd": _solid(ODD), "even": _solid(EVEN), "multipliers": [40.0, 30.0]},
    "chk": {"type": "CheckerTexture", "scale": 4.0, "odd": _solid(ODD), "even": _solid(EVEN),
            "multipliers": {"x": 5, "y": 5, "z": 5}},
    "img": {"type": "ImageTexture", "image_filename": IMG_NAME},
    "noise": {"type": "NoiseTexture", "scale": 4.0},
    # a SolidColor child behind a node that decides without a sine's sign: sin(0) * sin(0) = +0 is never < 0, so every
    # hit takes `even`.  The extended build's walk to a SolidColor child, with nothing to excuse.
    "solid": {"type": "UVChecker", "odd": _solid(ODD), "even": _solid(EVEN), "multipliers": [0.0, 0.0]},
}
ROT = {"translate": [0.4, -0.3, 0.6], "rotate": [30, 40, 10], "scale": [1, 1.5, 0.7]}
IDENT = {"translate": [0, 0, 0], "rotate": [0, 0, 0], "scale": [1, 1, 1]}
FAR = 3e9  # floor(p.x) beyond 2^31: Perlin's `floor(p.x) as i32` saturates, the checker's sine reduces 1.5e10

SHAPES = {
    "sphere": ({"type": "Sphere"}, IDENT),
    "sphere_rot": ({"type": "Sphere"}, ROT),
    "sphere_inv": ({"type": "Sphere", "inverse_normal": True}, IDENT),
    "rect_rot": ({"type": "Rectangle", "x0": -1.3, "y0": -0.8, "x1": 1.1, "y1": 0.9}, ROT),
    # 3.5 = 7 * 0.5 wide and 2.5 = 5 * 0.5 high: an axis-parallel ray at a multiple of 0.5 has u * 7 and v * 5 on an
    # integer in exact arithmetic, u = 0 and u = 1 at the rims
    "rect_texel": ({"type": "Rectangle", "x0": -1.75, "y0": -1.25, "x1": 1.75, "y1": 1.25}, IDENT),
    "rect_far": ({"type": "Rectangle", "x0": -1.5, "y0": -1.0, "x1": 1.5, "y1": 1.0},
                 {"translate": [FAR, 0, 0], "rotate": [25, 35, 15], "scale": [1, 1, 1]}),  # tilted: z = 0 zeroes a sine
    "cube_rot": ({"type": "Cube"}, ROT),
    "cube": ({"type": "Cube"}, IDENT),
    "torus": ({"type": "Torus", "radius": 1.0, "tube_radius": 0.3}, IDENT),
    "torus_rot": ({"type": "Torus", "radius": 1.0, "tube_radius": 0.3}, ROT),
    "dupin_rot": ({"type": "BruteForsableShape", "step": 0.01, "depth": 4,
                   "shape": {"type": "DupinCyclide", "a": 1.11, "b": 0.99, "c": 0.5, "d": 0.1, "sphere_radius": 2.5}},
                  {"translate": [0.4, -0.3, 0.6], "rotate": [30, 40, 10], "scale": [1.2, 1.2, 1.2]}),
}

FOUR = ("uv", "chk", "img", "noise")
# (shape, texture): the issue's table, then the SolidColor-child cases and the edge-only cases
CASES = [(s, t) for s in ("sphere", "sphere_rot", "sphere_inv", "rect_rot", "cube_rot") for t in FOUR] \
    + [("torus", "uv"), ("torus", "img"), ("torus_rot", "uv"), ("torus_rot", "img"), ("dupin_rot", "uv")] \
    + [("sphere_rot", "solid"), ("rect_rot", "solid"), ("cube_rot", "solid")] \
    + [("rect_texel", "img"), ("rect_far", "noise"), ("rect_far", "chk"), ("cube", "img")]
CASE_IDS = ["%s-%s" % c for c in CASES]
N_RANDOM = 1500


def kind(shape):
    return shape.split("_")[0]


def scene_json(shape, tex):
    rec, tr = SHAPES[shape]
    s = dict(rec, name="S", transform=tr, material="M")
    return json.dumps({"camera": {"position": [0, 0, -5], "direction": [0, 0, 1], "up": [0, 1, 0], "fov": 40,
                                  "focal_length": 1},
                       "shapes": [s], "materials": {"M": {"type": "DiffuseLight", "emit": TEXTURES[tex]}},
                       "background": [0, 0, 0]})


def oracle_scene(shape, tex):
    return O.Scene(scene_json(shape, tex), random_spheres=False, seed=SCENE_SEED, images=IMAGES)


def product_scene(pt, shape, tex):
    return pt.Scene.from_json(scene_json(shape, tex), random_spheres=False, seed=SCENE_SEED, images=IMAGES)


# ------------------------------------------------------------------ rays
def mpoint(m, p):
    """mat4 * point in the oracle's (and the device's) operation order, Python floats."""
    return [p[0] * m[4 * r] + p[1] * m[4 * r + 1] + p[2] * m[4 * r + 2] + m[4 * r + 3] for r in range(3)]


def mvector(m, v):
    return [v[0] * m[4 * r] + v[1] * m[4 * r + 1] + v[2] * m[4 * r + 2] for r in range(3)]


def _world(direct, pts):
    return np.array([mpoint(direct, [float(c) for c in p]) for p in pts])


def _aim(org, tgt):
    d = tgt - org
    return np.concatenate([org, d / np.linalg.norm(d, axis=1, keepdims=True)], axis=1)


def _bound(shape):
    rec = SHAPES[shape][0]
    k = kind(shape)
    if k == "rect":
        return np.array([rec["x0"], rec["y0"], 0.0]), np.array([rec["x1"], rec["y1"], 0.0])
    if k == "torus":
        a, b = rec["radius"] + rec["tube_radius"], rec["tube_radius"]
        return np.array([-a, -a, -b]), np.array([a, a, b])
    if k == "dupin":
        return np.full(3, -2.0), np.full(3, 2.0)
    return np.full(3, -1.0), np.full(3, 1.0)


def case_rays(shape, tex, direct):
    """(rays (n, 6), edge (n,) bool) of a case: N_RANDOM random rays aimed into the shape's bound from outside (Sphere
    and Cube: a third of them from inside), then the case's edge rays.  `direct` is the shape's object-to-world
    matrix (row-major 16).  Deterministic: the seed is the case's place in CASES."""
    rng = np.random.default_rng(1000 + CASES.index((shape, tex)))
    k = kind(shape)
    lo, hi = _bound(shape)
    centre = np.array(mpoint(direct, [0.0, 0.0, 0.0]))
    n = N_RANDOM
    tgt = _world(direct, rng.uniform(lo, hi, size=(n, 3)))
    dirs = rng.normal(size=(n, 3))
    org = centre + 6.0 * dirs / np.linalg.norm(dirs, axis=1, keepdims=True)
    rays = _aim(org, tgt)
    if k in ("sphere", "cube"):
        m = n // 3
        rays[:m, :3] = _world(direct, rng.uniform(-0.55, 0.55, size=(m, 3)))
    edge = []
    far = lambda pts, f=3.0: _aim(_world(direct, np.asarray(pts) * f), _world(direct, np.asarray(pts)))  # noqa: E731
    if k == "sphere":
        a = np.linspace(-1.5, 1.5, 41)
        seam = np.stack([-np.cos(a), np.sin(a), np.zeros_like(a)], axis=1)  # object plane z = 0, x < 0: u -> 0 or 1
        e = far(seam)
        if SHAPES[shape][1] is IDENT:  # p.z = -1e-300 (a -0.0 does not survive inverse * origin): atan2 = +pi, u = 1
            e2 = e.copy()
            e2[:, 2] = -1e-300
            e = np.concatenate([e, e2])
        edge.append(e)
        edge.append(far([[0.0, 1.0, 0.0], [0.0, -1.0, 0.0]]))  # the poles, along the axis
        near = np.array([[s * 10.0 ** -p, y, q * 10.0 ** -p] for p in (3, 6, 9, 12) for y in (1.0, -1.0)
                         for s, q in ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, -1))])
        near /= np.linalg.norm(near, axis=1, keepdims=True)
        edge.append(far(near))
    elif k == "cube":
        pts = [[x, y, z] for x in (-1.0, 1.0) for y in (-1.0, 1.0) for z in (-1.0, -0.3, 0.0, 0.7, 1.0)]
        pts += [[p[2], p[0], p[1]] for p in pts] + [[p[1], p[2], p[0]] for p in pts]
        pts = np.array(pts)
        org = pts.copy()  # along the diagonal of the tied axes: |p| ties in two (edges) or three (corners) components
        org[np.abs(pts) == 1.0] *= 3.0
        edge.append(_aim(_world(direct, org), _world(direct, pts)))
    elif k == "torus":
        rec = SHAPES[shape][0]
        R, r = rec["radius"], rec["tube_radius"]
        a = np.linspace(0.0, 2 * np.pi, 40, endpoint=False) + 0.05
        for z in (r, -r):  # the rings z = +-r, from straight above / below and slanted: asin sees |x| >= 1 or just less
            ring = np.stack([R * np.cos(a), R * np.sin(a), np.full_like(a, z)], axis=1)
            up = ring + np.array([0.0, 0.0, 4.0 * np.sign(z)])
            edge.append(_aim(_world(direct, up), _world(direct, ring)))
            slant = ring * np.array([1.5, 1.5, 1.0]) + np.array([0.0, 0.0, 3.0 * np.sign(z)])
            edge.append(_aim(_world(direct, slant), _world(direct, ring)))
    if (shape, tex) == ("rect_texel", "img"):
        xs = np.arange(-1.75, 1.7501, 0.5)  # u * 7 = 0 .. 7
        ys = np.arange(-1.25, 1.2501, 0.5)  # v * 5 = 0 .. 5
        for z0, dz in ((-3.0, 1.0), (2.0, -1.0)):
            e = np.array([[x, y, z0, 0.0, 0.0, dz] for x in xs for y in ys])
            edge.append(e)
    edge = np.concatenate(edge) if edge else np.zeros((0, 6))
    allr = np.ascontiguousarray(np.concatenate([rays, edge]))
    mask = np.zeros(len(allr), bool)
    mask[n:] = True
    return allr, mask


def ray_states(n, seed=77):
    return np.random.default_rng(seed).integers(0, 2 ** 63, size=n, dtype=np.uint64)


# ------------------------------------------------------------------ the oracle's object-space point
def obj_point(sh, ray, t):
    """The f64 object-space hit point as the oracle's finish_hit computes it (see the module docstring)."""
    inv = list(sh.inverse)
    o = mpoint(inv, [float(c) for c in ray[:3]])
    d = mvector(inv, [float(c) for c in ray[3:]])
    return [o[0] + d[0] * t, o[1] + d[1] * t, o[2] + d[2] * t]


def check_obj_point(sh, p_obj, hit):
    assert mpoint(list(sh.direct), p_obj) == list(hit.point), (p_obj, list(hit.point))


# ------------------------------------------------------------------ mpmath reference
NAN = None  # an mp value that the f64 formula makes NaN (acos / asin outside [-1, 1])


def _atan2(y, x):
    """atan2 of two f64 with IEEE signed zeros (mpmath has no -0)."""
    if y == 0.0:
        neg = math.copysign(1.0, y) < 0
        if x > 0.0 or (x == 0.0 and math.copysign(1.0, x) > 0):
            return mp.mpf(0)  # +-0: the sign is lost in `+ PI` anyway
        return -mp.pi if neg else +mp.pi
    return mp.atan2(mp.mpf(y), mp.mpf(x))


def mp_uv(sh, p):
    """(u, v) of hit_uv from the f64 object-space point p, in mpmath; NAN where the f64 formula gives NaN."""
    t = sh.type
    if t == O.SPHERE:
        u = (_atan2(-p[2], p[0]) + PI) / (2 * PI)
        v = mp.acos(mp.mpf(-p[1])) / PI if abs(p[1]) <= 1.0 else NAN
        return u, v
    if t == O.RECT:
        return ((mp.mpf(p[0]) - mp.mpf(sh.x0)) / (mp.mpf(sh.x1) - mp.mpf(sh.x0)),
                (mp.mpf(p[1]) - mp.mpf(sh.y0)) / (mp.mpf(sh.y1) - mp.mpf(sh.y0)))
    if t == O.CUBE:
        ax, ay, az = abs(p[0]), abs(p[1]), abs(p[2])
        mc = max(ax, ay, az)
        u, v = (p[1], p[2]) if mc == ax else ((p[0], p[2]) if mc == ay else (p[0], p[1]))
        return mp.mpf(u), mp.mpf(v)
    if t == O.TORUS:
        q = p[2] / sh.tube_radius  # one f64 division, the same on every side; asin's domain is decided on it
        if abs(q) > 1.0:
            return NAN, NAN
        theta = mp.asin(mp.mpf(q))
        x = mp.mpf(p[2]) / (mp.mpf(sh.radius) + mp.mpf(sh.tube_radius) * mp.cos(theta))
        return (mp.acos(x) + PI) / (2 * PI), theta / PI
    return mp.mpf(p[0]), mp.mpf(p[1])  # DupinCyclide


def torus_domain_edge(sh, p):
    """A Torus hit whose asin argument is within BOUNDARY of +-1: NaN or not is a decision boundary (and asin's
    slope is unbounded there)."""
    return sh.type == O.TORUS and abs(abs(p[2] / sh.tube_radius) - 1.0) < BOUNDARY


def _clamp01(x):
    return mp.mpf(0) if x < 0 else (mp.mpf(1) if x > 1 else x)


def mp_texture(tex, sh, p_obj, p_world, turb=None):
    """(colour, on_boundary) of TEXTURES[tex] at a hit, in mpmath.  on_boundary certifies a decision boundary: some
    sine factor below BOUNDARY (checkers), u * w or (1 - v) * h within BOUNDARY * w (resp. h) of an integer
    (ImageTexture), or a Torus hit at the rim of asin's domain.  For "noise" the colour is the mpmath value of
    0.5 (1 + sin(arg)) of the f64 argument, and `turb` is the oracle's f64 turbulence at p_world."""
    if tex == "noise":
        arg = TEXTURES["noise"]["scale"] * p_world[2] + 10.0 * turb
        s = float((1 + mp.sin(mp.mpf(arg))) / 2)
        return [s, s, s], False
    if tex == "chk":
        m = TEXTURES["chk"]["multipliers"]
        f = [mp.sin(mp.mpf(float(m[k]) * c)) for k, c in zip("xyz", p_world)]  # the products are f64, as in the formula
        return (ODD if f[0] * f[1] * f[2] < 0 else EVEN), min(abs(x) for x in f) < BOUNDARY
    u, v = mp_uv(sh, p_obj)
    edge = torus_domain_edge(sh, p_obj)
    if tex == "solid":
        return EVEN, False  # sin(+-0) * sin(+-0) and NaN alike are not < 0
    if tex == "uv":
        m = TEXTURES[tex]["multipliers"]
        if u is NAN or v is NAN:
            return EVEN, edge  # NaN < 0 is false
        f = [mp.sin(v * m[0] * PI), mp.sin(u * m[1] * PI)]
        return (ODD if f[0] * f[1] < 0 else EVEN), edge or min(abs(x) for x in f) < BOUNDARY
    # ImageTexture: NaN fails both clamps, and `NaN as u32` is 0.  The texel changes at the interior integers only:
    # below 0 and at w the index is clamped to the texel next to it.
    def texel(c, n):
        if c is NAN:
            return 0, False
        cn = c * n
        k = int(mp.nint(cn))
        return min(int(mp.floor(cn)), n - 1), 0 < k < n and abs(cn - k) < BOUNDARY * n

    x, near_x = texel(NAN if u is NAN else _clamp01(u), IMG_W)
    y, near_y = texel(NAN if v is NAN else 1 - _clamp01(v), IMG_H)
    near = near_x or near_y
    px = IMG_RGBA[(y * IMG_W + x) * 4:(y * IMG_W + x) * 4 + 3]
    return [c * (1.0 / 255.0) for c in px], near or edge


def turb_at(p_world, k=0):
    return O.lib().or_perlin_turb(SCENE_SEED, k, (C.c_double * 3)(*p_world))


def reference_at(tex, sh, ray, hit):
    """mp_texture for an oracle hit, with the object-space point proven to be the oracle's."""
    p = obj_point(sh, ray, hit.t)
    check_obj_point(sh, p, hit)
    pw = list(hit.point)
    return mp_texture(tex, sh, p, pw, turb_at(pw) if tex == "noise" else None)


# ------------------------------------------------------------------ Torus decidability
def quartic_roots(a, b, c, d, e):
    re, im = (C.c_double * 4)(), (C.c_double * 4)()
    O.lib().or_solve_quartic(a, b, c, d, e, re, im)
    return list(re), list(im)


def torus_coefficients(sh, ray):
    """The quartic of Torus::ray_intersect (mod.rs:434-447) from the object-space ray, in f64 as torus_t builds it."""
    inv = list(sh.inverse)
    ox, oy, oz = mpoint(inv, [float(c) for c in ray[:3]])
    dx, dy, dz = mvector(inv, [float(c) for c in ray[3:]])
    R, r = sh.radius, sh.tube_radius
    t = 4.0 * R * R
    g = t * (dx * dx + dy * dy)
    h = 2.0 * t * (ox * dx + oy * dy)
    i = t * (ox * ox + oy * oy)
    j = dx * dx + dy * dy + dz * dz
    k = 2.0 * (ox * dx + oy * dy + oz * dz)
    l = ox * ox + oy * oy + oz * oz + R * R - r * r  # noqa: E741
    return j * j, 2.0 * j * k, 2.0 * j * l + k * k - g, 2.0 * k * l - h, l * l - i


IM_EPS = 1e-15  # approx_equal(im, 0.0), equation.rs / mod.rs:451


def torus_decidable(sh, ray):
    """False when the oracle's own solver puts some root's |im| within 16x of the hit-or-miss threshold 1e-15: a
    math library an ulp away may decide the other way."""
    _, im = quartic_roots(*torus_coefficients(sh, ray))
    return not any(IM_EPS / 16 <= abs(x) <= 16 * IM_EPS for x in im)


def exact_root_near(coef, t):
    """The real part of the exact root (mpmath.polyroots of the f64 coefficients) nearest to t, and whether it is
    the smallest root above min_t = 0.001 that is real to 1e-9 (tangent rays have a close pair instead)."""
    roots = mp.polyroots([mp.mpf(c) for c in coef], maxsteps=200, extraprec=200)
    best = min(roots, key=lambda z: abs(z - t))
    real = [z.real for z in roots if abs(z.imag) < 1e-9 and z.real > 0.001]
    return best.real, bool(real) and min(real) == best.real
