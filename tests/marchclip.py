"""Scenes and rays of tests/test_gpu_march_clip.py: a Heart whose bounding ellipsoid a cube cuts from below (as
cornell_box.json's Cube2 cuts its Heart's) with a rectangle in front of it, so that a ray's best non-marched hit falls
before the march's chord, inside it in front of the Heart, inside it behind the Heart, or nowhere."""
import json

import numpy as np

GREY = {"type": "Lambertian", "albedo": {"type": "SolidColor", "color": [0.7, 0.7, 0.7]}}
RED = {"type": "Lambertian", "albedo": {"type": "SolidColor", "color": [0.65, 0.05, 0.05]}}
HEART_ID, CUBE_ID, RECT_ID = 0, 1, 2
HEART_BOUND = (1.45, 1.45 / 2.05, 1.45)  # Heart::intersect_bound's ellipsoid, object space


def clip_scene(materials=None, heart_material="Red"):
    shapes = [
        {"type": "BruteForsableShape", "name": "Heart", "shape": {"type": "Heart"}, "step": 0.01,
         "transform": {"translate": [0, 0, 0], "rotate": [-90, 20, 0], "scale": [1, 1, 1]},
         "material": heart_material},
        # its top face (y = -0.55) lies inside the bound and under the Heart's lobes, its tip dips into the cube
        {"type": "Cube", "name": "Cube", "transform": {"translate": [0.1, -1.35, 0.1], "rotate": [0, -18, 0],
                                                        "scale": [1.1, 0.8, 1.1]}, "material": "Grey"},
        # in front of the bound, covering a part of it as seen from the camera
        {"type": "Rectangle", "x0": 0.2, "x1": 1.5, "y0": -0.2, "y1": 1.2,
         "transform": {"translate": [0, 0, -2.2], "rotate": [0, 0, 0], "scale": [1, 1, 1]}, "material": "Grey"},
    ]
    return json.dumps({
        "camera": {"position": [0, 0.3, -6], "direction": [0, -0.05, 1], "up": [0, 1, 0], "fov": 40,
                   "focal_length": 1},
        "shapes": shapes, "materials": materials or {"Red": RED, "Grey": GREY}, "background": [0, 0, 0]})


def clip_rays(n):
    """n rays (n, 6): three quarters from outside the bound into it, a quarter from points inside it (the rays
    after a bounce off the cube's top or off the Heart)."""
    rng = np.random.default_rng(1717)

    def unit(v):
        return v / np.linalg.norm(v, axis=1, keepdims=True)

    k = n // 4
    o = unit(rng.normal(size=(3 * k, 3))) * rng.uniform(2.5, 6.0, size=(3 * k, 1))
    o[:k] = [0, 0.3, -6]  # the camera's
    o[:k] += rng.normal(size=(k, 3)) * 0.05
    tgt = unit(rng.normal(size=(3 * k, 3))) * rng.uniform(0.0, 1.5, size=(3 * k, 1))
    outside = np.concatenate([o, unit(tgt - o)], axis=1)
    o = unit(rng.normal(size=(n - 3 * k, 3))) * rng.uniform(0.0, 1.4, size=(n - 3 * k, 1))
    inside = np.concatenate([o, unit(rng.normal(size=(n - 3 * k, 3)))], axis=1)
    return np.ascontiguousarray(np.concatenate([outside, inside]))


def heart_chord(inverse, ray):
    """The march's chord [start, end] of a world ray through the Heart's bound (None: it misses the bound), from the
    shape's 4x4 row-major inverse matrix.  For sorting rays into classes only: plain numpy, not bit-exact."""
    m = np.array(inverse).reshape(4, 4)
    o = m[:3, :3] @ ray[:3] + m[:3, 3]
    d = m[:3, :3] @ ray[3:]
    r = np.array(HEART_BOUND)
    o, d = o / r, d / r
    a, b, c = d @ d, o @ d, o @ o - 1.0
    disc = b * b - a * c
    if disc < 0:
        return None
    s = np.sqrt(disc)
    return (-b - s) / a, (-b + s) / a
