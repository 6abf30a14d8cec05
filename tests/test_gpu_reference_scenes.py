"""The reference's own scene files (tests/golden/reference_scenes/, recorded in tests/golden/reference_scenes.json) on
the GPU.  Until now only the loader saw them: an ellipsoid, non-uniformly scaled cubes, an image texture, a Perlin
ground and a scene with zero JSON shapes never reached a kernel.

Every file that loads (detached_materials.json with the stand-in image its record names) renders 32x18 at 2 spp,
depth 8, scene seed from the fixture, and gives the same bits from both engines.  Against the oracle:
* a scene of solid colours is bit-exact (check_image);
* a scene whose materials carry a non-solid texture runs the device math library (sin in NoiseTexture, acos / atan2
  in hit_uv) and takes the texture tolerance check_image_tol: detached_materials.json (ImageTexture) and
  light_source.json, whose ground and sphere are a NoiseTexture Lambertian (1 of its 576 pixels differs from the
  oracle on an MI355X, by the last bits of a sine; tests/test_gpu_texture_rays.py bounds that sine per ray).  For
  the NoiseTexture-only scene every pixel must also be within 1e-12 relative: a noise value is continuous in the
  sine, so no pixel may move by more than depth x the per-ray bound 4 * 2^-52.
dupin.json is refused exactly as recorded.

empty.json has zero JSON shapes.  The reference never renders zero shapes: Scene::from_json always adds the random
spheres (json_models.rs:44), and BvhNode::new on an empty list never returns (shapes/mod.rs:702-713).  So the file is
rendered as the reference realizes it (482 random spheres and nothing else: the uniform list of JSON shapes is
empty), frame and 64 closest hits equal to the oracle; with the random spheres off the library refuses the scene
(PT_ERR_INVALID, "scene has no shapes"), and the oracle's linear scan, which has no BVH to build, sees background
and misses only.  Reads the committed fixtures only.
"""
import json

import numpy as np
import pytest

import oracle as O
from test_gpu_parity import TEX_REL, check_image, check_image_tol
from test_reference_scenes import FIXTURE, NAMES, REF_SCENES, _images

pytestmark = pytest.mark.gpu

W, H, SPP, DEPTH = 32, 18, 2, 8
LOADS = [n for n in NAMES if FIXTURE["scenes"][n]["outcome"] == "ok" or "with_loader" in FIXTURE["scenes"][n]]


def load(pt, name):
    rec = FIXTURE["scenes"][name]
    text = (REF_SCENES / name).read_text()
    images = _images(rec) if "with_loader" in rec else None
    return (pt.Scene.from_json(text, seed=FIXTURE["seed"], images=images),
            O.Scene(text, seed=FIXTURE["seed"], images=images))


def textures_of(name):
    """The non-solid texture types of a scene file's materials."""
    found = set()

    def walk(node):
        if isinstance(node, dict):
            if str(node.get("type", "")).endswith(("Texture", "UVChecker")):
                found.add(node["type"])
            for v in node.values():
                walk(v)
    walk(json.loads((REF_SCENES / name).read_text())["materials"])
    return found


def test_which_reference_scenes_are_textured():
    assert {n: sorted(textures_of(n)) for n in LOADS if textures_of(n)} == {
        "detached_materials.json": ["CheckerTexture", "ImageTexture", "UVChecker"],
        "light_source.json": ["NoiseTexture"]}


@pytest.mark.parametrize("name", LOADS)
def test_reference_scene_frame(pt, name):
    ps, osc = load(pt, name)
    r = pt.HipRenderer(ps, depth=DEPTH)
    cam, ip = ps.camera(), pt.ImageParams(W, H)
    ref = osc.render(W, H, SPP, DEPTH, FIXTURE["seed"])
    r.set_option("engine", 1)  # megakernel
    mega = r.render(cam, ip, SPP, seed=FIXTURE["seed"])
    r.set_option("engine", 2)  # wavefront
    wave = r.render(cam, ip, SPP, seed=FIXTURE["seed"])
    assert np.array_equal(mega, wave)
    tex = textures_of(name)
    print("%s: textures %s, bit-exact pixels %d of %d, max relative deviation %.3e" % (
        name, sorted(tex), np.all(mega == ref, axis=1).sum(), len(ref),
        np.max(np.abs(mega - ref) / np.maximum(np.abs(ref), 1e-300))))
    if tex:
        check_image_tol(mega, ref)
        if tex == {"NoiseTexture"}:
            assert np.all(np.abs(mega - ref) <= TEX_REL * np.abs(ref))
    else:
        check_image(mega, ref)
    assert mega.mean() > 0.05  # not a black frame


def test_empty_scene(pt):
    """empty.json (see the module docstring): as the reference realizes it, 64 closest hits equal the oracle's; with
    the random spheres off it is refused, and the oracle sees only background."""
    ps, osc = load(pt, "empty.json")
    assert ps.num_shapes == FIXTURE["scenes"]["empty.json"]["shapes"] == osc.num_shapes
    rng = np.random.default_rng(2)
    tgt = rng.uniform([-11, 0, -11], [11, 0.5, 11], size=(64, 3))  # the field of random spheres
    org = rng.uniform([-30, 1, -30], [30, 5, 30], size=(64, 3))
    d = tgt - org
    rays = np.concatenate([org, d / np.linalg.norm(d, axis=1, keepdims=True)], axis=1)
    got = pt.HipRenderer(ps, depth=DEPTH).closest_hit(rays)
    hit = 0
    for g, ray in zip(got, rays):
        h = osc.closest_hit(ray[:3], ray[3:])
        if h is None:
            assert g["shape"] == -1
            continue
        hit += 1
        assert (g["shape"], g["t"], list(g["point"]), list(g["normal"]), bool(g["front_face"])) == \
               (h.shape, h.t, list(h.point), list(h.normal), bool(h.front_face))
    assert hit >= 16
    text = (REF_SCENES / "empty.json").read_text()
    with pytest.raises(pt.PtError) as e:
        pt.Scene.from_json(text, random_spheres=False)
    assert e.value.code == pt.PT_ERR_INVALID and "no shapes" in str(e.value)
    bare = O.Scene(text, random_spheres=False)
    assert bare.num_shapes == 0
    img = bare.render(W, H, SPP, DEPTH, 3)
    # Scene::background (mod.rs:199-202): a blend of white and (0.5, 0.7, 1.0)
    assert np.all(np.abs(img[:, 2] - 1.0) < 1e-12) and np.all((img[:, 0] >= 0.5) & (img[:, 0] <= 1.0))
    assert all(bare.closest_hit(ray[:3], ray[3:]) is None for ray in rays)


def test_dupin_is_refused_as_recorded(pt):
    rec = FIXTURE["scenes"]["dupin.json"]
    assert rec["outcome"] == "error"
    with pytest.raises(pt.PtError) as e:
        pt.Scene.from_json((REF_SCENES / "dupin.json").read_text(), seed=FIXTURE["seed"])
    assert str(e.value) == rec["error"]
