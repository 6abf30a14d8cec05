"""The first bounce launch's cull table on the GPU (pt_cull.hpp; wf_bounce<FIRST> skips the list entries and marched
shapes that no camera ray of its wave's 8x8 pixel block can reach).  Nothing the oracle computes may move: every frame
here is the oracle's, every pixel, bit for bit.

cornell_box.json at 64x64, 128x72 and 100x52 and depths 0, 1, 4 and 8, each as one chunk, as two chunks on two
streams, as rank 1 of 3 and as a listed launch of a few tiles; spheres.json (two Hearts: wf_march selects its own
jobs); a textured (EXT) scene; the synthetic scenes of tests/firstcull.py from their own and a rolled camera.  One
renderer through two cameras, another size and a rebuilt acceleration structure: a stale table would show as wrong
pixels.  `first_cull_bits` is the host harness's count for the same camera, scene and size (the cull is on, not
silently all ones), and -1 for a megakernel frame and a split (wf_walk) frame.
"""
import functools
import json
import math
import sys
import tempfile
from pathlib import Path

import numpy as np
import pytest

import firstcull as fc
import marchclip as M
import oracle as O
import temporalref
import texrays as T
from conftest import ROOT, host_threads, scene_text

pytestmark = pytest.mark.gpu

SEED = 17
SPP = 4
SIZES = {"%dx%d" % wh: wh for wh in fc.SIZES}


def same_pixels(img, ref, what=""):
    assert np.all(np.isfinite(img))
    bad = np.flatnonzero(np.any(img.view(np.uint64) != ref.view(np.uint64), axis=1))
    assert bad.size == 0, "%s: %d of %d pixels differ (first %s)" % (what, bad.size, len(img), bad[:8].tolist())


def gpu_camera(pt, cam):
    pos, direction, up, focal, fov = cam
    return pt.Camera.new(pos, direction, up, focal, math.radians(fov))


# name -> (JSON text, add the random spheres, scene seed, images)
@functools.lru_cache(maxsize=None)
def scene_spec(name):
    if name == "cornell":
        return scene_text("cornell_box.json"), True, 1, None
    if name == "spheres":
        return scene_text("spheres.json"), True, 3, None
    if name == "textured":
        img = {"type": "Lambertian", "albedo": T.TEXTURES["img"]}
        return M.clip_scene(materials={"Red": M.RED, "Grey": img}), False, 1, T.IMAGES
    return fc.SYNTHETIC[name](), False, 1, None


@functools.lru_cache(maxsize=None)
def scenes(name):
    from conftest import load_package
    text, spheres, seed, images = scene_spec(name)
    kw = {"images": images} if images else {}
    return (load_package().Scene.from_json(text, random_spheres=spheres, seed=seed, **kw),
            O.Scene(text, random_spheres=spheres, seed=seed, **kw))


@functools.lru_cache(maxsize=None)
def scratch_dir():
    return tempfile.mkdtemp(prefix="first_cull_")


@functools.lru_cache(maxsize=None)
def oracle_frame(name, w, h, depth, cam=None):
    """The oracle's frame, rendered once and shared; cam: one of firstcull's cameras (None: the scene's own)."""
    ps, osc = scenes(name)
    camera = None
    if cam is not None:
        camera = temporalref.camera_like(gpu_camera(sys.modules["rs_pathtracing_amd"], cam))
    img = osc.render(w, h, SPP, depth, SEED, threads=host_threads(), camera=camera)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def host_bits(name, w, h, cam=None):
    """The harness's count of the set bits over the frame's table."""
    text, spheres, seed, _ = scene_spec(name)
    path = Path(scratch_dir()) / (name + ".json")
    path.write_text(text)
    args = ["count", path, int(spheres), seed, w, h] + (fc.camera_args(cam) if cam is not None else [])
    c = fc.run_harness(*args)
    assert 0 < c["count_bits"] < 64 * c["count_blocks"] and c["count_all_ones_blocks"] == 0
    return c["count_bits"]


def wave_renderer(pt, ps, depth):
    r = pt.HipRenderer(ps, depth=depth)
    r.set_option("engine", 2)
    return r


@pytest.mark.parametrize("depth", [0, 1, 4, 8])
@pytest.mark.parametrize("size", list(SIZES))
def test_cornell_frames(pt, size, depth):
    """One chunk; two chunks of two samples on the two streams; rank 1 of 3; a listed launch of a few tiles."""
    import torch
    w, h = SIZES[size]
    ps, _ = scenes("cornell")
    ref = oracle_frame("cornell", w, h, depth)
    cam = ps.camera()
    stream = torch.cuda.current_stream().cuda_stream
    tiles = ((w + 15) // 16) * ((h + 15) // 16)

    r = wave_renderer(pt, ps, depth)
    assert r.get_option("first_cull_bits") == -1  # nothing rendered yet
    same_pixels(r.render(cam, pt.ImageParams(w, h), SPP, seed=SEED), ref, "one chunk")
    assert r.last_builds()["engine"] == 1 and r.last_builds()["bounce"][4] == 0  # the wavefront engine, not SPLIT
    assert r.get_option("first_cull_bits") == host_bits("cornell", w, h)
    assert pt.march_guard_drops(r) == 0

    r = wave_renderer(pt, ps, depth)
    r.set_option("wf_paths", tiles * 256 * 2)
    assert r.get_option("wf_slots") == 2
    frame = torch.zeros(w * h * 3, dtype=torch.float64, device="cuda")
    pt.kernel_timing(r, True)
    r.render_device(cam, w, h, SPP, SEED, 0, 1, frame.data_ptr(), stream)
    torch.cuda.synchronize()
    assert pt.kernel_timing(r, False)["reduce"][1] == 2  # two chunks, one per stream
    same_pixels(frame.view(-1, 3).cpu().numpy(), ref, "two chunks")
    assert r.get_option("first_cull_bits") == host_bits("cornell", w, h)
    assert pt.march_guard_drops(r) == 0

    rank, world = 1, 3
    r = wave_renderer(pt, ps, depth)
    s = torch.zeros(pt.shard_tiles(w, h, 0, world) * 256 * 3, dtype=torch.float64, device="cuda")
    r.render_device(cam, w, h, SPP, SEED, rank, world, s.data_ptr(), stream)
    torch.cuda.synchronize()
    idx = pt.shard_pixels(w, h, rank, world)
    ok = idx >= 0
    assert ok.sum() >= w * h // world - 256
    same_pixels(s.view(-1, 3).cpu().numpy()[: len(idx)][ok], ref[idx[ok]], "rank 1 of 3")
    assert pt.march_guard_drops(r) == 0

    listed = [1, tiles // 2, tiles - 1]  # the last tile is a partial one at 100x52 and 128x72
    r = wave_renderer(pt, ps, depth)
    out = torch.full((w * h, 3), -7.0, dtype=torch.float64, device="cuda")
    r.render_device_tiles(cam, w, h, SPP, SEED, 0, 1, 0, SPP, listed, out.data_ptr(), stream)
    torch.cuda.synchronize()
    y, x = np.divmod(np.arange(w * h), w)
    on = np.isin((y // 16) * ((w + 15) // 16) + x // 16, listed)
    got = out.cpu().numpy()
    same_pixels(got[on], ref[on], "listed tiles")
    assert np.all(got[~on] == -7.0)
    assert r.get_option("first_cull_bits") == host_bits("cornell", w, h)
    assert pt.march_guard_drops(r) == 0


def test_spheres_two_hearts(pt):
    ps, _ = scenes("spheres")
    r = wave_renderer(pt, ps, 8)
    same_pixels(r.render(ps.camera(), pt.ImageParams(64, 64), SPP, seed=SEED), oracle_frame("spheres", 64, 64, 8))
    assert r.last_builds()["march"] is not None
    assert r.get_option("first_cull_bits") == host_bits("spheres", 64, 64)
    assert pt.march_guard_drops(r) == 0


def test_textured_scene(pt):
    """An EXT build of the first launch; the image texture's lookups on the cube and the rectangle call no library
    function (tests/test_gpu_march_clip.py), so the frame is the oracle's bit for bit."""
    ps, _ = scenes("textured")
    r = wave_renderer(pt, ps, 8)
    same_pixels(r.render(ps.camera(), pt.ImageParams(100, 52), SPP, seed=SEED), oracle_frame("textured", 100, 52, 8))
    assert r.last_builds()["bounce"][2] == 1  # an EXT build
    assert r.get_option("first_cull_bits") > 0
    assert pt.march_guard_drops(r) == 0


@pytest.mark.parametrize("cam", [None, fc.SYNTHETIC_CAMERAS[-1]], ids=["own", "rolled"])
@pytest.mark.parametrize("size", ["64x64", "100x52"])
@pytest.mark.parametrize("name", sorted(fc.SYNTHETIC))
def test_synthetic_scenes(pt, name, size, cam):
    w, h = SIZES[size]
    ps, _ = scenes(name)
    r = wave_renderer(pt, ps, 4)
    camera = ps.camera() if cam is None else gpu_camera(pt, cam)
    same_pixels(r.render(camera, pt.ImageParams(w, h), SPP, seed=SEED), oracle_frame(name, w, h, 4, cam))
    assert r.get_option("first_cull_bits") == host_bits(name, w, h, cam)
    assert pt.march_guard_drops(r) == 0


def test_one_renderer_through_cameras_sizes_and_a_rebuild(pt):
    """The table is keyed on the camera, the size and the acceleration data: each step against the oracle."""
    ps, _ = scenes("cornell")
    r = wave_renderer(pt, ps, 8)
    a, b = None, fc.CORNELL_CAMERAS[1]  # the scene's own camera; one inside the box, looking at a corner
    assert host_bits("cornell", 64, 64, a) != host_bits("cornell", 64, 64, b)

    def step(cam, w, h, what):
        camera = ps.camera() if cam is None else gpu_camera(pt, cam)
        same_pixels(r.render(camera, pt.ImageParams(w, h), SPP, seed=SEED), oracle_frame("cornell", w, h, 8, cam), what)
        assert r.get_option("first_cull_bits") == host_bits("cornell", w, h, cam), what

    step(a, 64, 64, "camera A")
    step(a, 64, 64, "camera A again")
    step(b, 64, 64, "camera B")
    step(b, 100, 52, "another size")
    nodes = r.get_option("bvh_nodes")
    r.set_option("bvh_leaf", 4)  # rebuilds the acceleration data and swaps every buffer of it
    assert r.get_option("bvh_nodes") < nodes
    step(b, 100, 52, "after the rebuild")
    step(a, 64, 64, "camera A after the rebuild")
    assert pt.march_guard_drops(r) == 0


def test_no_table_for_the_megakernel_and_the_split_engine(pt):
    ps, _ = scenes("cornell")
    r = pt.HipRenderer(ps, depth=8)
    r.set_option("engine", 2)
    r.render(ps.camera(), pt.ImageParams(64, 64), 1, seed=SEED)
    assert r.get_option("first_cull_bits") == host_bits("cornell", 64, 64)
    r.set_option("engine", 1)
    r.render(ps.camera(), pt.ImageParams(64, 64), 1, seed=SEED)
    assert r.last_builds()["engine"] == 0 and r.get_option("first_cull_bits") == -1
    # read-only, and no knob
    with pytest.raises(pt.PtError) as e:
        r.set_option("first_cull_bits", 0)
    assert e.value.code == pt.PT_ERR_INVALID
    assert "first_cull_bits" not in pt.option_names() and "first_cull_bits" not in r.options()

    # C5's engine: a tree of at least 2^15 nodes per layout and no marched shape, traced by wf_walk (a SPLIT bounce)
    sys.path.insert(0, str(ROOT / "scenes"))
    import make_scenes
    doc = make_scenes.synthetic(1 << 14)  # (tests/test_gpu_builds.py's field: the full grid and one sphere more)
    extra = json.loads(json.dumps(doc["shapes"][-1]))
    extra["name"] = "Extra"
    extra["transform"]["translate"][1] += 0.5
    doc["shapes"].append(extra)
    field = pt.Scene.from_json(json.dumps(doc), random_spheres=False, seed=1)
    r = pt.HipRenderer(field, depth=8)
    r.set_option("engine", 2)
    img = r.render(field.camera(), pt.ImageParams(96, 54), 2, seed=3)
    assert np.all(np.isfinite(img))
    assert r.last_builds()["bounce"][4] == 1 and r.last_builds()["walk"] is not None  # SPLIT, with its walk
    assert r.get_option("first_cull_bits") == -1
