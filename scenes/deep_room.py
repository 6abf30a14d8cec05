"""The closed room of the deep-path tests (tests/test_gpu_deep.py, tests/test_deep_host.py) and of
scripts/deep_depth.py: our own scene, written here as JSON text.  Nothing ends a path in it but the lamp or depth 0, so a large share of its paths runs past 64 bounces: on
the oracle, 32x32 at 2 spp, a sample asks for 57 closest hits at depth 64, 98 at 127, 168 at 300 and 206 at 500.

Three variants: plain (analytic shapes only), heart (a ray-marched Heart: the march queue and the pre-selected march
jobs) and textured (a checker on the wall: the EXT kernel builds and the per-level attenuation values)."""
import json

VARIANTS = ("plain", "heart", "textured")
WALL = [0.95, 0.9, 0.85]


def _xf(translate, scale):
    return {"translate": list(translate), "rotate": [0, 0, 0], "scale": [scale, scale, scale]}


def _solid(c):
    return {"type": "SolidColor", "color": list(c)}


def room_json(variant="plain"):
    assert variant in VARIANTS
    shapes = [
        {"type": "Sphere", "name": "Room", "transform": _xf((0, 0, 0), 10), "material": "Wall"},
        {"type": "Sphere", "name": "Lamp", "transform": _xf((0, 6, 0), 0.7), "material": "Lamp"},
        {"type": "Sphere", "name": "Glass", "transform": _xf((-3, -1, 2), 2), "material": "Glass"},
        {"type": "Sphere", "name": "Ball", "transform": _xf((3, -2, 1), 1.5), "material": "Metal"},
    ]
    wall = _solid(WALL)
    if variant == "heart":
        shapes.append({"type": "BruteForsableShape", "name": "Heart", "shape": {"type": "Heart", "sphere_radius": 1.45},
                       "step": 0.01, "transform": _xf((0, -3, 3), 1.5), "material": "Metal"})
    if variant == "textured":
        wall = {"type": "CheckerTexture", "scale": 1.0, "odd": _solid(WALL), "even": _solid([0.85, 0.9, 0.95]),
                "multipliers": {"x": 2, "y": 2, "z": 2}}
    materials = {
        "Wall": {"type": "Lambertian", "albedo": wall},
        "Lamp": {"type": "DiffuseLight", "emit": _solid([40, 40, 40])},
        "Glass": {"type": "Dielectric", "index_of_refraction": 1.5},
        "Metal": {"type": "Metal", "albedo": _solid([0.8, 0.5, 0.3]), "fuzz": 0.2},
    }
    camera = {"position": [0, 0, -8], "direction": [0, 0, 1], "up": [0, 1, 0], "fov": 60, "focal_length": 1}
    return json.dumps({"camera": camera, "shapes": shapes, "materials": materials, "background": [0, 0, 0]})


def inside_rays(n, rng):
    """n rays (origin, unit direction) starting inside the room, clear of its wall."""
    import numpy as np
    o = rng.normal(size=(n, 3))
    o *= (rng.uniform(0, 1, size=(n, 1)) ** (1 / 3)) * 9.0 / np.linalg.norm(o, axis=1, keepdims=True)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([o, d], axis=1)
