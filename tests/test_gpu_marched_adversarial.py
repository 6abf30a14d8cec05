"""The adversarial rays of test_marched_adversarial.py (tests/adversarial.py: CASES, object_rays_for) through the
gfx950 kernels: HipRenderer.closest_hit and HipRenderer.ray_color against the oracle's literal march, bit for bit
with NaN equal to NaN, for Sine, Star, DupinCyclide, HuntsSurface and Cushion and their parameter variants.  These
go through the generic march (the F_ANY builds: approx_rcp, floor_div and the device's code for shape_f / shape_poly
/ shape_mag by run-time function id), which the Heart's adversarial tests never enter.  The oracle's side is
computed once per setting (adversarial.oracle_hits / oracle_paths) and held to the same floors as on the host."""
import json

import numpy as np
import pytest

import adversarial as A
import oracle as O
from conftest import scene_text
from deep_checks import check_image

pytestmark = pytest.mark.gpu

NAMES = [c["name"] for c in A.CASES]
XFS = ["identity", "scale40", "rot"]
# the three transforms at the scene files' setting, then the identity at a coarse step, backwards, one pass, and a
# step longer than many chords
GPU_SETTINGS = [(xf,) + A.FLOOR_SETTING for xf in XFS] + [("identity", 0.05, 3), ("identity", -0.01, 4),
                                                         ("identity", 0.01, 1), ("identity", 0.5, 4)]
HEART, ANY = 0, -1  # march::F_HEART, F_ANY (pt_dims.hpp)


def renderer(pt, name, xf, step, depth):
    ps = pt.Scene.from_json(A.case_text(name, xf, step, depth), random_spheres=False)
    return ps, pt.HipRenderer(ps, depth=A.PATH_DEPTH)


def test_oracle_hits_enough():
    """The floors of the host test, on the rays as this machine builds them (the oracle's hits are shared with
    the comparisons below)."""
    nan_normals = 0
    for name in NAMES:
        for xf in XFS:
            n, by, nn = A.hit_counts(name, xf)
            nan_normals += nn
            if name in A.NEVER_HIT:
                assert n == 0
                continue
            assert n >= A.MIN_HITS, (name, xf, n)
            assert all(by[f] >= 1 for f in A.MUST_HIT), (name, xf, by)
    assert nan_normals >= A.MIN_NAN_NORMALS


@pytest.mark.parametrize("name", NAMES)
def test_closest_hits_exact(pt, name):
    for xf, step, depth in GPU_SETTINGS:
        rays, _ = A.case_rays(name, xf)
        _, r = renderer(pt, name, xf, step, depth)
        got = A.gpu_hit_records(r.closest_hit(rays))
        bad = A.hit_differences(got, A.oracle_hits(name, xf, step, depth))
        assert not bad, "%s step %g depth %d: %d of %d rays differ, first %s: %s" % (
            xf, step, depth, len(bad), len(rays), bad[:5], rays[bad[0]].tolist())
        assert pt.march_guard_drops(r) == 0


@pytest.mark.parametrize("name", NAMES)
def test_whole_paths_exact(pt, name):
    for xf in XFS:
        rays, _ = A.case_rays(name, xf)
        before, want, after = A.oracle_paths(name, xf)
        _, r = renderer(pt, name, xf, *A.FLOOR_SETTING)
        states = before.copy()
        col = r.ray_color(rays, states, depth=A.PATH_DEPTH)
        bad = [i for i in range(len(rays))
               if not (np.array_equal(col[i], want[i], equal_nan=True) and states[i] == after[i])]
        assert not bad, "%s: %d of %d paths differ, first %s: %s" % (xf, len(bad), len(rays), bad[:5],
                                                                     rays[bad[0]].tolist())
        assert np.any(want > 0.0)
        assert pt.march_guard_drops(r) == 0


@pytest.mark.parametrize("name", NAMES)
def test_frames_run_the_generic_builds(pt, name):
    """closest_hit and ray_color are probes; what a frame launches is on record (last_builds).  A small frame of the
    case's scene on each engine: the generic march build ran, no Heart build did, and the frame is the oracle's
    (NaN for NaN: a path that has scattered from a singular point may carry one)."""
    w, h, spp, seed = 16, 9, 2, 5
    ps, r = renderer(pt, name, "identity", *A.FLOOR_SETTING)
    ref = A.case_scene(name, "identity", *A.FLOOR_SETTING).render(w, h, spp, A.PATH_DEPTH, seed)
    r.set_option("engine", 2)  # wavefront
    img = r.render(ps.camera(), pt.ImageParams(w, h), spp, seed=seed)
    ran = r.last_builds()
    assert ran["engine"] == 1 and ran["mega"] is None and ran["bounce"][1] == ANY and ran["march"] == (ANY,), ran
    assert np.array_equal(img, ref, equal_nan=True)
    r.set_option("engine", 1)  # megakernel
    img = r.render(ps.camera(), pt.ImageParams(w, h), spp, seed=seed)
    ran = r.last_builds()
    assert ran["engine"] == 0 and ran["mega"][2] == ANY and ran["bounce"] is None and ran["march"] is None, ran
    assert np.array_equal(img, ref, equal_nan=True)
    assert pt.march_guard_drops(r) == 0


def variants_text():
    """scenes/marched.json without its Heart, the Dupin with pinch points and the Sine at a = 0."""
    js = json.loads(scene_text("marched.json"))
    js["shapes"] = [s for s in js["shapes"] if s.get("name") != "Heart"]
    by = {s.get("name"): s for s in js["shapes"]}
    by["Dupin"]["shape"] = A.CASE["dupin_pinch"]["shape"]
    by["Sine"]["shape"] = A.CASE["sine_a0"]["shape"]
    assert [s["shape"]["type"] for s in js["shapes"][2:]] == ["DupinCyclide", "Sine", "Star", "HuntsSurface",
                                                              "Cushion"]
    return json.dumps(js)


def test_five_functions_side_by_side_on_both_engines(pt):
    w, h, spp, seed = 32, 18, 2, 3
    text = variants_text()
    ps = pt.Scene.from_json(text, random_spheres=False)
    ref = O.Scene(text, random_spheres=False).render(w, h, spp, A.PATH_DEPTH, seed)
    assert ref.mean() > 0.01
    r = pt.HipRenderer(ps, depth=A.PATH_DEPTH)
    for engine, ran_engine in ((2, 1), (1, 0)):
        r.set_option("engine", engine)
        img = r.render(ps.camera(), pt.ImageParams(w, h), spp, seed=seed)
        ran = r.last_builds()
        assert ran["engine"] == ran_engine, ran
        assert (ran["march"] == (ANY,) and ran["bounce"][1] == ANY) if ran_engine else ran["mega"][2] == ANY, ran
        check_image(img, ref)
        assert pt.march_guard_drops(r) == 0
