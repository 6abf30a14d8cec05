"""One frame on the GPU per instantiated kernel build, against the oracle.

pt_builds.hpp instantiates 8 render_tiles builds, 17 wf_bounce builds (each for both values of FIRST), 5 wf_walk builds
and 2 wf_march builds; tests/test_builds.py proves on the CPU that builds::choose names only those and names each for
some frame.  This file renders them.  Every row of ROWS is one small frame: the renderer reports the builds it launched
(HipRenderer.last_builds, the "ran_*" names of pt_renderer_get_option, recorded where the launch is made), the row
asserts that they are the builds it was written for, and then that the frame is the oracle's: the bar of
test_gpu_parity.check_image, restated here as deep_checks.py restates it (every pixel bit-exact, per-channel RMS <=
1e-4); the textured rows call the device's math library and take test_gpu_parity's texture bar, restated as well.

The last test is the completeness check: the union of the builds the rows reported is, kernel by kernel, the list of
the instantiated builds that tests/native's libbuilds.so reads from pt_builds.hpp, apart from EXCEPTIONS.  A build
instantiated later without a row fails it, and so does a session in which not every row ran and passed."""
import ctypes as C
import functools
import json
import subprocess
import sys

import numpy as np
import pytest

import oracle as O
from conftest import ROOT, host_threads, native_lib, scene_text
from deep_checks import RMS_TOL, check_image, rms
from deep_checks import deep_room as R

sys.path.insert(0, str(ROOT / "scenes"))
import make_scenes  # noqa: E402

pytestmark = pytest.mark.gpu

HEART, ANY, NONE = 0, -1, -2  # march::F_HEART, F_ANY, F_NONE (pt_march.hpp)
BIG = 1 << 15                 # BIG_BVH_NODES (pt_dims.hpp)
BIG_SPHERES = BIG // 2 + 1    # one leaf per sphere, 2 n - 1 nodes per layout (tests/test_scene_view.py's big_tree)
# test_gpu_parity.py's bar for frames whose textures call sin / acos / atan2 (device math library against glibc)
TEX_REL = 1e-12
TEX_CLOSE_MIN = 0.998


def check_image_tol(img, ref):
    assert np.all(np.isfinite(img))
    assert np.all(rms(img, ref) <= RMS_TOL), rms(img, ref)
    close = np.mean(np.all(np.abs(img - ref) <= TEX_REL * np.abs(ref), axis=1))
    assert close >= TEX_CLOSE_MIN, "pixels within %g relative: %.6f" % (TEX_REL, close)


# ------------------------------------------------------------------------------------------------------- scenes
# name -> (JSON text, add the random spheres, scene seed, the oracle takes its BvhNode traversal, textured)
def field(heart):
    """The random-sphere field just above BIG_BVH_NODES nodes per layout (tests/test_scene_view.py's big_tree: the
    full 128 x 128 grid and one sphere more); with the Heart of test_gpu_bvh_extremes.with_heart above it."""
    doc = make_scenes.synthetic(BIG_SPHERES - 1)
    extra = json.loads(json.dumps(doc["shapes"][-1]))
    extra["name"] = "Extra"
    extra["transform"]["translate"][1] += 0.5
    doc["shapes"].append(extra)
    assert len(doc["shapes"]) == 1 + BIG_SPHERES  # (the ground sphere joins the uniform list)
    if heart:
        src = make_scenes.marched()
        shape = json.loads(json.dumps(next(s for s in src["shapes"] if s.get("name") == "Heart")))
        shape["transform"]["translate"] = [0.0, 1.2, 0.0]
        doc["shapes"].append(shape)
        doc["materials"]["Copper"] = src["materials"]["Copper"]
    return json.dumps(doc)


@functools.lru_cache(maxsize=None)
def scene_spec(name):
    if name in ("cornell_box", "marched", "textured"):
        return scene_text(name + ".json"), name == "cornell_box", 1, False, name == "textured"
    if name.startswith("room-"):
        return R.room_json(name[5:]), False, 1, False, name == "room-textured"
    return field(name == "field-heart"), False, 1, True, False


@functools.lru_cache(maxsize=None)
def gpu_scene(name):
    from conftest import load_package
    text, spheres, seed, _, _ = scene_spec(name)
    return load_package().Scene.from_json(text, random_spheres=spheres, seed=seed)


@functools.lru_cache(maxsize=None)
def oracle_frame(name, w, h, spp, depth, seed):
    """The oracle's frame, computed once per (scene, frame) and shared by the rows that render it; never written
    to.  The large trees go through the reference's BvhNode traversal (use_bvh(True, 7)), the others its list scan."""
    text, spheres, scene_seed, bvh, _ = scene_spec(name)
    osc = O.Scene(text, random_spheres=spheres, seed=scene_seed)
    if bvh:
        osc.use_bvh(True, 7)
    img = osc.render(w, h, spp, depth, seed, threads=host_threads())
    img.setflags(write=False)
    return img


# ------------------------------------------------------------------------------------------------------- the rows
def row(name, scene, frame, options, engine, mega=None, bounce=None, walk=None, march=None):
    """frame: (width, height, spp, depth, seed).  engine: 0 megakernel, 1 wavefront, as ran_engine reports it."""
    return pytest.param(scene, frame, options, {"engine": engine, "mega": mega, "bounce": bounce, "walk": walk,
                                                "march": march}, id=name)


CORNELL = (64, 36, 3, 8, 21)  # test_gpu_parity.test_bounce_register_budgets' frame: a small tree and a Heart
GENERIC = (64, 36, 2, 8, 3)
TEXTURED = (64, 36, 4, 8, 1)  # test_gpu_parity.test_textured_frames' frame
ROOM65 = (32, 32, 2, 65, 3)   # test_gpu_deep.py's frame
FIELD = (96, 54, 2, 8, 3)


def room(depth):
    return (32, 32, 8, depth, 3)  # test_gpu_stacks.py's frame: the top levels of each stack width are read back


ROWS = (
    # render_tiles<NW, WAVES, FK>: the Heart-only build at every budget, the generic one, the wider stacks
    [row("mega-heart-%dw" % w, "cornell_box", CORNELL, {"engine": 1, "mega_waves": w}, 0, mega=(4, w, HEART))
     for w in (2, 3, 4, 5)]
    + [row("mega-any", "marched", GENERIC, {"engine": 1}, 0, mega=(4, 2, ANY))]
    + [row("mega-any-%dwords" % nw, "room-heart", room(depth), {"engine": 1}, 0, mega=(nw, 2, ANY))
       for nw, depth in ((8, 16), (16, 32), (32, 64))]
    # wf_bounce<FIRST, WAVES, FK, EXT, BIGBVH, SPLIT, DEEP> (DESIGN §2.0's bounce table, row by row) and wf_march<FK>
    + [row("bounce-1-deep", "room-plain", ROOM65, {}, 1, bounce=(2, ANY, 0, 0, 0, 1)),
       row("bounce-1-deep-march", "room-heart", ROOM65, {}, 1, bounce=(2, ANY, 0, 0, 0, 1), march=(ANY,)),
       row("bounce-1-deep-ext", "room-textured", ROOM65, {}, 1, bounce=(2, ANY, 1, 0, 0, 1))]
    + [row("bounce-2-split-%dw-walk-%dw" % (b, k), "field", FIELD,
           {"engine": 2, "wf_bounce_waves": b, "wf_walk": k}, 1, bounce=(b, NONE, 0, 1, 1, 0), walk=(k, 1))
       for b, k in ((3, 5), (3, 4), (3, 6), (3, 8), (4, 5), (5, 5))]
    + [row("bounce-3-ext", "textured", TEXTURED, {}, 1, bounce=(2, ANY, 1, 0, 0, 0), march=(ANY,)),
       row("bounce-4-any", "marched", GENERIC, {"engine": 2}, 1, bounce=(2, ANY, 0, 0, 0, 0), march=(ANY,))]
    + [row("bounce-6-big-%dw" % b, "field", FIELD, {"engine": 2, "wf_bounce_waves": b, "wf_walk": 0}, 1,
           bounce=(b, NONE, 0, 1, 0, 0)) for b in (3, 4, 5)]
    + [row("bounce-7-big-heart", "field-heart", FIELD, {"engine": 2}, 1, bounce=(3, HEART, 0, 1, 0, 0),
           march=(HEART,))]
    + [row("bounce-8-heart-%dw" % b, "cornell_box", CORNELL, {"engine": 2, "wf_bounce_waves": b}, 1,
           bounce=(b, HEART, 0, 0, 0, 0), march=(HEART,)) for b in (2, 3, 4, 5, 6, 8)]
)
ROW_IDS = [p.id for p in ROWS]

# The instantiated builds that no row renders, each with its reason: at most this one.
EXCEPTIONS = {
    # wf_walk over unquantized nodes runs only when make_grid refuses the tree, which takes a root extent that
    # overflows f64 (spheres at +-1.5e308, tests/test_path_host.py's test_quantized_grid_refuses_unbounded_extents).
    # In such a scene the sphere test's discriminant is NaN and the oracle's own two traversals disagree (its list
    # scan and its BvhNode traversal differ on 99 % of the pixels of a 96x54, 2-spp, depth-8 frame of
    # make_scenes.synthetic(17000) with that test's 80 far spheres), so there is no reference to hold the device to.
    # A scene that reaches this build and on which the oracle's two traversals agree on every pixel gets a row here.
    ("walk", (5, 0)): "reached only by a tree whose extent overflows f64, where the oracle disagrees with itself",
}

REPORTED = {}  # row id -> last_builds() of its frame, entered once the frame has matched the oracle


def test_a_frame_reports_what_it_launched(pt):
    """The record itself (tests/test_builds.py has its CPU side): a fresh renderer has launched nothing; a frame
    reports its engine and builds; every call starts from an empty record; the names are read-only and are no
    options."""
    ps = gpu_scene("cornell_box")
    r = pt.HipRenderer(ps, depth=8)
    nothing = {"engine": -1, "mega": None, "bounce": None, "walk": None, "march": None}
    assert r.last_builds() == nothing
    assert [r.get_option("ran_" + k) for k in ("engine", "mega", "bounce", "walk", "march")] == [-1] * 5
    before = r.options()
    assert before == pt.OPTION_DEFAULTS and not [k for k in before if k.startswith("ran_")]
    assert not [k for k in pt.option_names() if k.startswith("ran_")]
    w, h, spp, depth, seed = CORNELL
    cam, ip = ps.camera(), pt.ImageParams(w, h)
    wave = r.render(cam, ip, spp, seed=seed)  # (the default engine of a scene with a marched shape: the wavefront)
    assert r.last_builds() == {"engine": 1, "mega": None, "bounce": (3, HEART, 0, 0, 0, 0), "walk": None,
                               "march": (HEART,)}
    assert r.get_option("ran_bounce") == sum((f + 2) << (6 * j) for j, f in enumerate((3, HEART, 0, 0, 0, 0)))
    for name in ("ran_engine", "ran_mega", "ran_bounce", "ran_walk", "ran_march"):
        for value in (0, -1, 1):
            with pytest.raises(pt.PtError) as e:
                r.set_option(name, value)
            assert e.value.code == pt.PT_ERR_INVALID, name
    assert r.last_builds()["engine"] == 1 and r.options() == before
    r.set_option("engine", 1)
    mega = r.render(cam, ip, spp, seed=seed)  # the next call's record holds nothing of the last one's
    assert r.last_builds() == {"engine": 0, "mega": (4, 4, HEART), "bounce": None, "walk": None, "march": None}
    assert r.options() == dict(before, engine=1)
    assert np.array_equal(wave, mega)
    check_image(wave, oracle_frame("cornell_box", *CORNELL))
    two = pt.HipRenderer(ps, depth=8, devices=[0, 0])  # several devices: the first one's record
    assert two.last_builds() == nothing
    assert np.array_equal(two.render(cam, ip, spp, seed=seed), wave)
    assert two.last_builds()["engine"] == 1 and two.last_builds()["bounce"] == (3, HEART, 0, 0, 0, 0)


@pytest.mark.parametrize("scene,frame,options,expected", ROWS)
def test_build_renders_the_oracles_frame(pt, request, monkeypatch, scene, frame, options, expected):
    monkeypatch.chdir(ROOT)  # (textured.json names its image file relative to the repository)
    w, h, spp, depth, seed = frame
    ps = gpu_scene(scene)
    r = pt.HipRenderer(ps, depth=depth)
    for k, v in options.items():
        r.set_option(k, v)
    if scene.startswith("field"):
        assert BIG <= r.get_option("bvh_nodes") <= BIG + 2, "not the smallest large tree"
    img = r.render(ps.camera(), pt.ImageParams(w, h), spp, seed=seed)
    ran = r.last_builds()
    print("\n%s -> %s" % (request.node.callspec.id, ran))
    assert ran == expected
    ref = oracle_frame(scene, *frame)
    assert ref.mean() > 0.01  # not a black frame
    if scene == "field-heart":
        assert np.any(ref != oracle_frame("field", *frame)), "the Heart is not in the frame"
    (check_image_tol if scene_spec(scene)[4] else check_image)(img, ref)
    REPORTED[request.node.callspec.id] = ran


def test_every_instantiated_build_has_rendered(request):
    """Completeness.  Kept last in the file: it stands on what the rows above reported in this session."""
    missing = [k for k in ROW_IDS if k not in REPORTED]
    assert not missing, "rows that did not run and pass in this session: %s" % missing
    subprocess.run(["make", "-s", "-C", str(ROOT / "tests" / "native"), "_build/libbuilds.so"], check=True)
    L = C.CDLL(native_lib("libbuilds.so"))
    L.builds_list.argtypes = [C.c_int, C.c_void_p]
    assert len(EXCEPTIONS) <= 1 and all(EXCEPTIONS.values())
    for which, (kernel, cols) in enumerate((("mega", 3), ("bounce", 6), ("walk", 2), ("march", 1))):
        n = L.builds_list(which, None)
        out = np.zeros((n, cols), dtype=np.int64)
        assert L.builds_list(which, out.ctypes.data) == n and n > 0
        instantiated = {tuple(r) for r in out.tolist()}
        rendered = {ran[kernel] for ran in REPORTED.values() if ran[kernel] is not None}
        excepted = {b for k, b in EXCEPTIONS if k == kernel}
        assert excepted <= instantiated, "%s: excepted but not instantiated: %s" % (kernel, excepted - instantiated)
        assert not rendered & excepted, "%s: excepted but rendered: %s" % (kernel, rendered & excepted)
        assert rendered <= instantiated, "%s: rendered but not in the list: %s" % (kernel, rendered - instantiated)
        lacking = instantiated - rendered - excepted
        assert not lacking, "%s: instantiated but rendered by no row: %s" % (kernel, sorted(lacking))
