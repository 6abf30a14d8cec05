"""cull::first_cull_mask (pt_cull.hpp) on the host: the mask of an 8x8 pixel block never lacks the bit of a shape one
of the block's camera rays can hit.  tests/first_cull/first_cull_harness.cpp is a stand-alone host build of the product
headers; these tests build it (a few seconds; nothing to do after build()) and run it.

Safety: cornell_box.json, spheres.json and the three synthetic scenes of tests/firstcull.py, each from its own camera
and three or four more (the last rolled and off-axis), at 64x64, 128x72 and 100x52, every block, every pixel, 16
samples per pixel from the product's sample_key / camera_ray.  The list entry the plain closest_nomarch returns and
every marched shape whose shape_bound_k holds must have its bit; the culled scan (closest_nomarch's CULL form, with its
"products valid" flag for the rectangle groups, and the bounce kernel's pre-check loop) must give the plain scan's
(best, who, needs a march) bit for bit.  0 violations, 0 differences.

Effect: cornell_box.json at 1920x1080 from its own camera: fewer than 2.0 set bits per block on average, and the
light's bit clear in every block.  (A run's figures: profiles/r18/first_cull_host.txt.)

Degenerate input: a NaN or infinite camera, a field of view of 180 degrees and more, a zero pixel_resolution and a flat
pyramid all give all-ones masks.
"""
import pytest

import firstcull as fc
from conftest import ROOT

SCENES = ROOT / "scenes"


def safety(path, random_spheres, seed, cameras):
    args = ["safety", path, int(random_spheres), seed]
    for cam in cameras:
        args += fc.camera_args(cam)
    s = fc.run_harness(*args)
    assert s["safety_cameras"] == len(cameras) + 1 >= 4
    assert s["safety_cases"] == 3 * (len(cameras) + 1)
    # every block of every frame, every pixel, 16 samples
    blocks = sum(-(-w // 8) * -(-h // 8) for w, h in fc.SIZES)
    assert s["safety_blocks"] == blocks * (len(cameras) + 1)
    assert s["safety_rays"] == 16 * sum(w * h for w, h in fc.SIZES) * (len(cameras) + 1)
    assert s["safety_who_violations"] == 0 and s["safety_march_violations"] == 0 and s["safety_differ"] == 0
    assert s["status"] == 0
    # the rays do hit the list's shapes, and the masks do cull
    assert s["safety_list_hits"] > s["safety_rays"] // 20
    assert s["safety_bits"] < s["safety_candidates"]
    return s


def test_safety_cornell():
    s = safety(SCENES / "cornell_box.json", True, 1, fc.CORNELL_CAMERAS)
    assert s["safety_bounds_held"] > 1000 and s["safety_all_ones_blocks"] == 0


def test_safety_spheres():
    s = safety(SCENES / "spheres.json", True, 3, fc.SPHERES_CAMERAS)
    assert s["safety_bounds_held"] > 1000


@pytest.mark.parametrize("name", sorted(fc.SYNTHETIC))
def test_safety_synthetic(name, tmp_path):
    path = tmp_path / (name + ".json")
    path.write_text(fc.SYNTHETIC[name]())
    s = safety(path, False, 1, fc.SYNTHETIC_CAMERAS)
    if name != "edges":
        assert s["safety_bounds_held"] > 1000  # the Heart is entered


def test_effect_cornell_1080p():
    c = fc.run_harness("count", SCENES / "cornell_box.json", 1, 1, 1920, 1080)
    assert c["count_blocks"] == 240 * 135 and c["count_list"] == 8 and c["count_marched"] == 1
    mean = c["count_bits"] / c["count_blocks"]
    print("mean set bits per block: %.3f" % mean)
    assert mean < 2.0
    assert c["count_light_bits"] == 0
    assert c["count_all_ones_blocks"] == 0


def test_degenerate_cameras_cull_nothing():
    d = fc.run_harness("degenerate", SCENES / "cornell_box.json", 1, 1)
    assert d["degenerate_valid_camera_culls"] > 0  # the scene's own camera does cull at this size
    for key in ("nan_position", "nan_direction", "inf_position", "fov_180", "fov_200", "fov_270", "fov_359",
                "zero_resolution", "zero_resolution_field", "flat_pyramid"):
        assert d["degenerate_" + key] == 0, key
    assert d["degenerate_not_all_ones"] == 0 and d["status"] == 0
