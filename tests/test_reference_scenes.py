"""The reference's own scene set through the product loader and the oracle.

The drop-in claim is that the host loads the reference's scenes/*.json as
today (Scene::from_json, src/world/mod.rs:46-49; SceneJson,
src/world/json_models.rs:23-48).  tests/golden/reference_scenes.json records,
for every file of the reference's scenes/ (kept as test data in
tests/golden/reference_scenes/; the record is made by
tests/golden/make_reference_scenes.py), the outcome of pt.Scene.from_json and
a digest of the realized shapes with their materials:

* each file must load (or be refused) exactly as recorded, and the oracle must
  realize the same shapes and materials bit for bit;
* the two scenes the benchmarks use were re-authored in scenes/ (not copied):
  they must realize exactly what the reference's files realize, which is
  checked against the recorded digests.

Outcomes that match the reference's: dupin.json is in an older schema (no
`camera`, no `materials` map) and serde fails on it too; detached_materials.json
names a JPEG that the reference decodes with image::open, which this library
leaves to the host's loader (pt_scene_opts.load_image): without one the file is
refused, with one it loads.  Host code only: runs without a GPU.
"""
import hashlib
import json
import sys
from pathlib import Path

import pytest

import oracle as O

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE / "golden"))
import make_reference_scenes as M  # noqa: E402

REF_SCENES = HERE / "golden" / "reference_scenes"
FIXTURE = json.loads((HERE / "golden" / "reference_scenes.json").read_text())
NAMES = sorted(FIXTURE["scenes"])


def _images(rec):
    return {n: M.STAND_IN_IMAGE for n in rec["with_loader"]["images"]}


def test_fixture_covers_the_reference_scene_set():
    files = sorted(f.name for f in REF_SCENES.glob("*.json"))
    assert files == NAMES
    for n in NAMES:
        assert hashlib.sha256((REF_SCENES / n).read_bytes()).hexdigest() == FIXTURE["scenes"][n]["sha256"], n


@pytest.mark.parametrize("name", NAMES)
def test_reference_scene_loads_as_recorded(pt, name):
    rec = FIXTURE["scenes"][name]
    text = (REF_SCENES / name).read_text()
    got = M.outcome(pt, text)
    assert got["outcome"] == rec["outcome"], got
    if rec["outcome"] == "error":
        assert got["error"] == rec["error"]
        with pytest.raises(Exception):  # the oracle's loader refuses it too
            O.Scene(text, seed=FIXTURE["seed"])
    else:
        assert (got["shapes"], got["materials"], got["digest"]) == (rec["shapes"], rec["materials"], rec["digest"])
    if "with_loader" in rec:
        wl = rec["with_loader"]
        got = M.outcome(pt, text, images=_images(rec))
        assert (got["outcome"], got["shapes"], got["materials"], got["digest"]) == \
               (wl["outcome"], wl["shapes"], wl["materials"], wl["digest"])


@pytest.mark.parametrize("name", [n for n in NAMES if FIXTURE["scenes"][n]["outcome"] == "ok"
                                  or "with_loader" in FIXTURE["scenes"][n]])
def test_reference_scene_realized_bit_equal_to_oracle(pt, name):
    """Every shape's matrices and parameters and every material, product vs
    oracle, field by field (the digest condenses the same comparison)."""
    rec = FIXTURE["scenes"][name]
    text = (REF_SCENES / name).read_text()
    images = _images(rec) if "with_loader" in rec else None
    p = pt.Scene.from_json(text, seed=FIXTURE["seed"], images=images)
    o = O.Scene(text, seed=FIXTURE["seed"], images=images)
    assert (p.num_shapes, p.num_materials) == (o.num_shapes, o.num_materials)
    for i in range(p.num_shapes):
        a, b = p.shape(i), o.shape(i)
        assert (a.type, a.material, a.inverse_normal) == (b.type, b.material, b.inverse_normal), i
        assert list(a.direct) == list(b.direct) and list(a.inverse) == list(b.inverse), i
        assert (a.x0, a.y0, a.x1, a.y1, a.step) == (b.x0, b.y0, b.x1, b.y1, b.step), i
    for i in range(p.num_materials):
        a, b = p.material(i), o.material(i)
        assert a.type == b.type and list(a.albedo) == list(b.albedo) and list(a.emit) == list(b.emit), i
        assert (a.fuzz, a.ior) == (b.fuzz, b.ior), i
    assert M.realized_digest(p) == M.realized_digest(o)


@pytest.mark.parametrize("name", ["cornell_box.json", "spheres.json"])
def test_reauthored_scene_realizes_like_the_reference_file(pt, name):
    """scenes/cornell_box.json and scenes/spheres.json (re-authored by
    scenes/make_scenes.py) realize the same shapes, transforms and materials as
    the reference's files of the same name (random spheres on, seed 1): the
    benchmark workload is the reference's scene."""
    text = (HERE.parent / "scenes" / name).read_text()
    sc = pt.Scene.from_json(text, seed=FIXTURE["seed"])
    assert sc.num_shapes == FIXTURE["scenes"][name]["shapes"]
    assert M.realized_digest(sc) == FIXTURE["scenes"][name]["digest"]
