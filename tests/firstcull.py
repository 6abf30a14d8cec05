"""What the first-bounce cull tests share (tests/test_first_cull_host.py, tests/test_gpu_first_cull.py): the
stand-alone host harness (tests/first_cull), three synthetic scenes and the cameras every scene is looked at with.

A camera is (position, direction, up, focal length, field of view in degrees): the scene's own camera comes first in
every list, and the last one of each list is rolled and looks off the scene's axis.
"""
import json
import math
import subprocess

from conftest import ROOT

HARNESS = ROOT / "tests" / "first_cull"
SIZES = ((64, 64), (128, 72), (100, 52))  # the last is no multiple of the 8-pixel block


def run_harness(*args):
    """The harness' "key value" lines as a dict; its exit status is 1 when it saw a violation."""
    subprocess.run(["make", "-C", str(HARNESS)], check=True, capture_output=True)
    p = subprocess.run([str(HARNESS / "_build" / "first_cull_harness"), *[str(a) for a in args]], capture_output=True,
                       text=True)
    print(p.stdout)
    assert p.returncode in (0, 1), p.stderr
    out = {}
    for line in p.stdout.splitlines():
        k, _, v = line.partition(" ")
        if v.strip().lstrip("-").isdigit():
            out[k] = int(v)
    out["status"] = p.returncode
    return out


def camera_args(cam):
    pos, direction, up, focal, fov = cam
    return [repr(float(v)) for v in (*pos, *direction, *up, focal, fov)]


def tr(t, r=(0, 0, 0), s=(1, 1, 1)):
    return {"translate": list(t), "rotate": list(r), "scale": list(s)}


def rect(t, r, x, y, mat):
    return {"type": "Rectangle", "x0": x[0], "x1": x[1], "y0": y[0], "y1": y[1], "transform": tr(t, r), "material": mat}


def sphere(t, radius, mat):
    return {"type": "Sphere", "name": "S", "transform": tr(t, (0, 0, 0), (radius,) * 3), "material": mat}


def heart(t, r, s, mat):
    return {"type": "BruteForsableShape", "name": "Heart", "shape": {"type": "Heart"}, "step": 0.01,
            "transform": tr(t, r, (s,) * 3), "material": mat}


MATERIALS = {
    "White": {"type": "Lambertian", "albedo": {"type": "SolidColor", "color": [0.73, 0.73, 0.73]}},
    "Red": {"type": "Lambertian", "albedo": {"type": "SolidColor", "color": [0.65, 0.05, 0.05]}},
    "Mirror": {"type": "Metal", "albedo": {"type": "SolidColor", "color": [0.7, 0.6, 0.5]}, "fuzz": 0},
    "Light": {"type": "DiffuseLight", "emit": {"type": "SolidColor", "color": [6, 6, 6]}},
}
CAMERA = {"position": [0, 0, -5], "direction": [0, 0, 1], "up": [0, 1, 0], "fov": 40, "focal_length": 1}


def scene(shapes):
    return json.dumps({"camera": CAMERA, "shapes": shapes, "materials": MATERIALS, "background": [0, 0, 0]})


def edges_scene():
    """A rectangle whose left and lower edges lie in the planes x = 0 and y = 0 through the camera (the side planes
    between the two middle block columns and rows of a 64x64 or 128x72 frame), a sphere far smaller than a pixel, a
    sphere behind the camera, a turned cube and a light."""
    return scene([
        rect((0, 0, 6), (0, 0, 0), (0, 3), (0, 2), "White"),
        sphere((0.7, -0.4, 3.0), 1e-3, "Red"),
        sphere((0, 0, -9), 1.0, "Mirror"),
        {"type": "Cube", "name": "C", "transform": tr((-1.5, -1.0, 4.0), (20, 35, 10), (0.6, 0.4, 0.5)), "material": "White"},
        rect((-2, 3.5, 2), (90, 0, 0), (0, 4), (0, 4), "Light"),
    ])


def inside_scene():
    """A cube that contains the camera and everything else: a Heart, a sphere behind the camera, a small mirror cube
    and a light under the lid."""
    return scene([
        {"type": "Cube", "name": "Room", "transform": tr((0, 0, 0), (0, 0, 0), (8, 6, 12)), "material": "White"},
        heart((1.0, 0.5, 1.0), (-90, 25, 0), 1.2, "Red"),
        sphere((0, 0, -9), 1.0, "Mirror"),
        {"type": "Cube", "name": "C", "transform": tr((-2.0, -1.5, 2.0), (0, 30, 0), (0.7, 0.7, 0.7)), "material": "Mirror"},
        rect((-2, 5, -1), (90, 0, 0), (0, 4), (0, 4), "Light"),
    ])


def groups_scene():
    """Two groups of parallel rectangles whose first member (the group's head in the uniform list) is a small one in
    a corner of the view, outside most pixel blocks, while the others cover the middle; a Heart and a tiny sphere."""
    return scene([
        rect((-3.2, 1.4, 8), (0, 0, 0), (0, 0.4), (0, 0.4), "Red"),       # head of the z-facing group
        rect((3.0, -1.5, 3), (0, 90, 0), (0, 0.3), (0, 0.3), "Red"),      # head of the x-facing group
        rect((-2, -2, 9), (0, 0, 0), (0, 4), (0, 4), "White"),
        heart((0.3, -0.2, 5.0), (-90, -25, 0), 0.8, "Red"),
        rect((-1.5, -1, 2), (0, 90, 0), (0, 5), (0, 2), "White"),
        rect((-1, -1, 7), (0, 0, 0), (0, 2), (0, 2), "Mirror"),
        rect((1.5, -1, 2), (0, 90, 0), (0, 5), (0, 2), "White"),
        sphere((-0.5, 0.6, 2.0), 2e-3, "Mirror"),
        rect((-2, 3.0, 2), (90, 0, 0), (0, 4), (0, 4), "Light"),
    ])


SYNTHETIC = {"edges": edges_scene, "inside": inside_scene, "groups": groups_scene}

# the cameras after each scene's own
SYNTHETIC_CAMERAS = [
    ((1.5, 0.5, -4.0), (-0.3, -0.1, 1.0), (0, 1, 0), 1.0, 55.0),
    ((-2.5, 1.0, 1.0), (1.0, -0.2, 0.6), (0, 1, 0), 1.0, 70.0),
    ((0.5, -0.5, -3.0), (0.1, 0.3, -1.0), (0, 1, 0), 1.0, 40.0),   # looking back, at what is behind the first camera
    ((0.8, 1.2, -4.5), (-0.25, -0.35, 1.0), (0.5, 0.85, 0.1), 2.0, 33.0),  # rolled, off-axis
]
CORNELL_CAMERAS = [
    ((100.0, 400.0, -300.0), (0.3, -0.25, 1.0), (0, 1, 0), 1.0, 50.0),
    ((278.0, 300.0, 100.0), (-0.4, -0.3, 1.0), (0, 1, 0), 1.0, 75.0),   # inside the box
    ((450.0, 120.0, -500.0), (-0.35, 0.2, 1.0), (0.45, 0.88, 0.0), 1.5, 35.0),  # rolled, off-axis
]
SPHERES_CAMERAS = [
    ((10.0, 3.0, -20.0), (-0.5, -0.1, 1.0), (0, 1, 0), 1.0, 35.0),
    ((0.0, 25.0, -5.0), (0.0, -1.0, 0.2), (0, 0, 1), 1.0, 50.0),        # from above
    ((-12.0, 2.0, 9.0), (1.0, -0.05, -0.8), (0.3, 0.9, 0.2), 3.0, 25.0),  # rolled, off-axis
]


def degrees(cam):
    return math.radians(cam[4])
