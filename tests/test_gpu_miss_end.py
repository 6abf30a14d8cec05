"""The wavefront engine ends a missed path in the bounce launch that traces it (pt_wave.hip wf_bounce, when no
march is pending; dev::shade_decided), on every bounce build that traces: one Heart, two Hearts (the march selects
its own jobs), the generic marched functions, the extended (textured) build, and the large tree with a Heart; the
first launch (camera rays that miss) as well as the later ones.  Each frame is compared with the oracle on every
pixel, bit for bit.  The textured frame is compared bit for bit with the megakernel's on the same device instead,
which this path does not touch (textures are tolerance-only against the oracle: device libm).
"""
import json
import sys
from pathlib import Path

import numpy as np
import pytest

import oracle as O
from conftest import ROOT, host_threads, scene_text

pytestmark = pytest.mark.gpu

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "scenes"))

RED = {"Red": {"type": "Lambertian", "albedo": {"type": "SolidColor", "color": [0.65, 0.05, 0.05]}}}


def same_pixels(img, ref):
    assert np.all(np.isfinite(img))
    bad = np.flatnonzero(np.any(img != ref, axis=1))
    assert bad.size == 0, "%d of %d pixels differ (first %s)" % (bad.size, len(img), bad[:8].tolist())


def wave_frame(pt, ps, w, h, spp, depth, seed, **opts):
    r = pt.HipRenderer(ps, depth=depth)
    r.set_option("engine", 2)
    for k, v in opts.items():
        r.set_option(k, v)
    return r.render(ps.camera(), pt.ImageParams(w, h), spp, seed=seed)


# ------------------------------------------------------------ 1. one Heart alone against the sky
HEART_SKY = json.dumps({
    "camera": {"position": [0, 0, -6], "direction": [0, 0, 1], "up": [0, 1, 0], "fov": 40, "focal_length": 1},
    "shapes": [{"type": "BruteForsableShape", "name": "Heart", "shape": {"type": "Heart"}, "step": 0.01,
                "transform": {"translate": [0, 0, 0], "rotate": [-90, 20, 0], "scale": [1, 1, 1]},
                "material": "Red"}],
    "materials": RED, "background": [0, 0, 0]})


@pytest.fixture(scope="module")
def heart_sky(pt):
    return pt.Scene.from_json(HEART_SKY, random_spheres=False), O.Scene(HEART_SKY, random_spheres=False)


@pytest.mark.parametrize("depth", [0, 1, 2, 8])
def test_one_heart_against_the_sky(pt, heart_sky, depth):
    """Nothing but a marched shape: every ray that misses the (empty) list and tree either enters the Heart's
    bound, and must then wait for the march, or ends at once.  Ending a miss with a march pending would lose the
    Heart."""
    ps, osc = heart_sky
    w, h, spp, seed = 48, 32, 4, 5
    ref = osc.render(w, h, spp, depth, seed)
    img = wave_frame(pt, ps, w, h, spp, depth, seed)
    same_pixels(img, ref)
    sky = osc.render(w, h, 1, 0, seed)  # depth 0: a hit is black, a miss the sky
    heart = int(np.count_nonzero(np.all(sky == 0.0, axis=1)))
    assert 300 < heart < 600, heart  # the Heart covers about 440 of the 1536 pixels


# ------------------------------------------------------------ 2. every camera ray misses
ALL_MISS = json.dumps({
    "camera": {"position": [0, 0, 0], "direction": [0, 0, 1], "up": [0, 1, 0], "fov": 40, "focal_length": 1},
    "shapes": [{"type": "Sphere", "name": "Behind",
                "transform": {"translate": [0, 0, -100], "rotate": [0, 0, 0], "scale": [1, 1, 1]},
                "material": "Red"}],
    "materials": RED, "background": [0, 0, 0]})


def test_every_camera_ray_misses(pt):
    """The only shape is behind the camera: every path ends in the first launch and every later list is empty."""
    import torch
    ps = pt.Scene.from_json(ALL_MISS, random_spheres=False)
    w, h, spp, depth, seed = 40, 24, 3, 8, 2
    ref = O.Scene(ALL_MISS, random_spheres=False).render(w, h, spp, depth, seed)
    assert np.all(ref >= 0.5 - 1e-9) and np.allclose(ref[:, 2], 1.0)  # the sky's gradient: blue is 1 everywhere
    r = pt.HipRenderer(ps, depth=depth)
    r.set_option("engine", 2)
    frame = torch.zeros(w * h * 3, dtype=torch.float64, device="cuda")
    r.render_device(ps.camera(), w, h, spp, seed, 0, 1, frame.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    same_pixels(frame.view(-1, 3).cpu().numpy(), ref)


# ------------------------------------------------------------ 3. cornell: chunks on both streams, and a shard
@pytest.fixture(scope="module")
def cornell_ref(cornell_text):
    return O.Scene(cornell_text, seed=1).render(96, 54, 8, 8, 11, threads=host_threads())


def test_cornell_chunks_on_two_streams(pt, cornell_text, cornell_ref):
    import torch
    w, h, spp, depth, seed = 96, 54, 8, 8, 11
    ps = pt.Scene.from_json(cornell_text, seed=1)
    r = pt.HipRenderer(ps, depth=depth)
    r.set_option("engine", 2)
    r.set_option("wf_paths", 6144 * 2)  # 24 tiles = 6144 pixels: chunks of 2 of the 8 samples
    assert r.get_option("wf_slots") == 2
    frame = torch.zeros(w * h * 3, dtype=torch.float64, device="cuda")
    pt.kernel_timing(r, True)
    r.render_device(ps.camera(), w, h, spp, seed, 0, 1, frame.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    kt = pt.kernel_timing(r, False)
    assert kt["reduce"][1] == 4  # four chunks, two rounds of the two streams, one per-pixel reduce each
    same_pixels(frame.view(-1, 3).cpu().numpy(), cornell_ref)


def test_cornell_rank_1_of_3(pt, cornell_text, cornell_ref):
    import torch
    w, h, spp, depth, seed, rank, world = 96, 54, 8, 8, 11, 1, 3
    ps = pt.Scene.from_json(cornell_text, seed=1)
    r = pt.HipRenderer(ps, depth=depth)
    r.set_option("engine", 2)
    per = pt.shard_tiles(w, h, 0, world)
    s = torch.zeros(per * 256 * 3, dtype=torch.float64, device="cuda")
    r.render_device(ps.camera(), w, h, spp, seed, rank, world, s.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    idx = pt.shard_pixels(w, h, rank, world)
    got = s.view(-1, 3).cpu().numpy()[: len(idx)]
    ok = idx >= 0
    assert ok.sum() >= w * h // world - 256
    same_pixels(got[ok], cornell_ref[idx[ok]])


# ------------------------------------------------------------ 4. two Hearts: the march selects its own jobs
@pytest.mark.parametrize("depth", [8, 50])
def test_spheres_two_hearts(pt, spheres_text, depth):
    w, h, spp, seed = 64, 64, 4, 3
    ps = pt.Scene.from_json(spheres_text, seed=1)
    ref = O.Scene(spheres_text, seed=1).render(w, h, spp, depth, seed, threads=host_threads())
    same_pixels(wave_frame(pt, ps, w, h, spp, depth, seed), ref)


# ------------------------------------------------------------ 5. the generic marched functions (F_ANY build)
def test_marched_functions(pt):
    text = scene_text("marched.json")
    w, h, spp, depth, seed = 48, 27, 2, 8, 3
    ps = pt.Scene.from_json(text, random_spheres=False)
    ref = O.Scene(text, random_spheres=False).render(w, h, spp, depth, seed, threads=host_threads())
    same_pixels(wave_frame(pt, ps, w, h, spp, depth, seed), ref)


# ------------------------------------------------------------ 6. the extended build against the megakernel
def test_textured_wavefront_equals_megakernel(pt, monkeypatch):
    monkeypatch.chdir(ROOT)  # (the scene's image texture is named relative to the repository)
    text = scene_text("textured.json")
    w, h, spp, depth, seed = 48, 27, 4, 8, 1
    ps = pt.Scene.from_json(text, seed=1)
    r = pt.HipRenderer(ps, depth=depth)
    cam, ip = ps.camera(), pt.ImageParams(w, h)
    r.set_option("engine", 2)
    wave = r.render(cam, ip, spp, seed=seed)
    r.set_option("engine", 1)
    mega = r.render(cam, ip, spp, seed=seed)
    same_pixels(wave, mega)
    assert wave.mean() > 0.05


# ------------------------------------------------------------ 7. the large tree with a Heart (non-split build)
def test_large_tree_with_a_heart(pt):
    """A marched shape keeps the large-tree scene off the split engine: the bounce kernel walks the tree itself
    and queues the Heart's march jobs."""
    import make_scenes
    doc = make_scenes.synthetic(20000)
    doc["shapes"].append({"type": "BruteForsableShape", "name": "Heart", "shape": {"type": "Heart"}, "step": 0.01,
                          "transform": {"translate": [0, 2.5, 0], "rotate": [-90, 0, 0], "scale": [1.5, 1.5, 1.5]},
                          "material": "Ground"})
    text = json.dumps(doc)
    w, h, spp, depth, seed = 64, 36, 2, 8, 3
    ps = pt.Scene.from_json(text, seed=1)
    r = pt.HipRenderer(ps, depth=depth)
    r.set_option("engine", 2)
    assert r.get_option("bvh_nodes") >= 1 << 15, "not the large-tree build"
    img = r.render(ps.camera(), pt.ImageParams(w, h), spp, seed=seed)
    ref = O.Scene(text, seed=1).use_bvh(True, 7).render(w, h, spp, depth, seed, threads=host_threads())
    same_pixels(img, ref)
    del doc["shapes"][-1]
    plain = O.Scene(json.dumps(doc), seed=1).use_bvh(True, 7).render(w, h, spp, depth, seed, threads=host_threads())
    assert np.count_nonzero(np.any(plain != ref, axis=1)) > 100  # the Heart is in the frame
