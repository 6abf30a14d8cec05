"""A march job ends at the best non-marched hit (march::clip_to_best, pt_march.hpp): the wavefront engine clips the
job's chord in wf_bounce (one marched shape) or in wf_march's own select (several), the megakernel in trace_pixel.
Nothing the oracle computes may move: closest hits per ray and whole frames, every pixel, bit for bit.

The scene of tests/marchclip.py puts a cube into the Heart's bound from below, as cornell_box.json's Cube2 does, and
a rectangle in front of it, so the best hit falls before the chord (the job is dropped), inside it in front of the
Heart (the march stops short), inside it behind the Heart (the crossing lies before the cap) and nowhere (+inf).
"""
import numpy as np
import pytest

import marchclip as M
import oracle as O
import texrays as T
from conftest import host_threads

pytestmark = pytest.mark.gpu

NRAYS = 4096
SEED = 17
SIZES = {"64x64": (64, 64), "128x72": (128, 72)}
SPP = 4


def same_pixels(img, ref):
    assert np.all(np.isfinite(img))
    bad = np.flatnonzero(np.any(img.view(np.uint64) != ref.view(np.uint64), axis=1))
    assert bad.size == 0, "%d of %d pixels differ (first %s)" % (bad.size, len(img), bad[:8].tolist())


def test_closest_hit_per_ray(pt):
    text = M.clip_scene()
    osc = O.Scene(text, random_spheres=False)
    ps = pt.Scene.from_json(text, random_spheres=False)
    rays = M.clip_rays(NRAYS)
    r = pt.HipRenderer(ps, depth=8)
    got = r.closest_hit(rays)
    inverse = list(osc.shape(M.HEART_ID).inverse)
    seen = {"before": 0, "front": 0, "behind": 0, "heart_alone": 0, "past": 0}
    bad = []
    for i, ray in enumerate(rays):
        h = osc.closest_hit(ray[:3], ray[3:])
        want = (-1, 0.0) if h is None else (h.shape, h.t)
        if got["shape"][i] != want[0] or (h is not None and got["t"][i] != want[1]):
            bad.append(i)
        elif h is not None:
            assert list(got["point"][i]) == list(h.point) and list(got["normal"][i]) == list(h.normal), i
        chord = M.heart_chord(inverse, ray)
        if chord is None or chord[1] < 0.001:
            continue
        heart = osc.shape_hit(M.HEART_ID, ray[:3], ray[3:])
        other = [g.t for g in (osc.shape_hit(k, ray[:3], ray[3:]) for k in (M.CUBE_ID, M.RECT_ID)) if g is not None]
        if not other:
            seen["heart_alone"] += heart is not None
        elif min(other) < chord[0]:
            seen["before"] += 1
        elif min(other) > chord[1]:
            seen["past"] += 1
        elif heart is None or min(other) < heart.t:
            seen["front"] += 1
        else:
            seen["behind"] += 1
    print("best hit against the chord:", seen)
    assert all(v >= 100 for v in seen.values()), seen
    assert not bad, "%d of %d rays differ, first %d: %r got (%d, %r)" % (
        len(bad), NRAYS, bad[0], list(rays[bad[0]]), got["shape"][bad[0]], got["t"][bad[0]])
    assert pt.march_guard_drops(r) == 0


# ------------------------------------------------------------------ wavefront frames, every pixel
@pytest.fixture(scope="module")
def scenes(pt, cornell_text):
    """name -> (GPU scene, oracle scene, {}): each oracle frame is rendered once and kept"""
    clip = M.clip_scene()
    return {"clip": (pt.Scene.from_json(clip, random_spheres=False), O.Scene(clip, random_spheres=False), {}),
            "cornell": (pt.Scene.from_json(cornell_text, seed=1), O.Scene(cornell_text, seed=1), {})}


def oracle_frame(entry, w, h, depth):
    _, osc, kept = entry
    if (w, h, depth) not in kept:
        kept[(w, h, depth)] = osc.render(w, h, SPP, depth, SEED, threads=host_threads())
    return kept[(w, h, depth)]


@pytest.mark.parametrize("depth", [1, 4, 8])
@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("name", ["clip", "cornell"])
def test_wavefront_frames(pt, scenes, name, size, depth):
    """Two chunks of two samples on the two streams, then rank 1 of 3."""
    import torch
    w, h = SIZES[size]
    ps = scenes[name][0]
    ref = oracle_frame(scenes[name], w, h, depth)
    assert ref.mean() > 0.01
    tiles = ((w + 15) // 16) * ((h + 15) // 16)
    stream = torch.cuda.current_stream().cuda_stream
    r = pt.HipRenderer(ps, depth=depth)
    r.set_option("engine", 2)
    r.set_option("wf_paths", tiles * 256 * 2)
    assert r.get_option("wf_slots") == 2
    frame = torch.zeros(w * h * 3, dtype=torch.float64, device="cuda")
    pt.kernel_timing(r, True)
    r.render_device(ps.camera(), w, h, SPP, SEED, 0, 1, frame.data_ptr(), stream)
    torch.cuda.synchronize()
    kt = pt.kernel_timing(r, False)
    assert kt["reduce"][1] == 2  # two chunks, one per stream
    assert r.last_builds()["march"] is not None
    same_pixels(frame.view(-1, 3).cpu().numpy(), ref)
    assert pt.march_guard_drops(r) == 0

    rank, world = 1, 3
    r = pt.HipRenderer(ps, depth=depth)
    r.set_option("engine", 2)
    per = pt.shard_tiles(w, h, 0, world)
    s = torch.zeros(per * 256 * 3, dtype=torch.float64, device="cuda")
    r.render_device(ps.camera(), w, h, SPP, SEED, rank, world, s.data_ptr(), stream)
    torch.cuda.synchronize()
    idx = pt.shard_pixels(w, h, rank, world)
    got = s.view(-1, 3).cpu().numpy()[: len(idx)]
    ok = idx >= 0
    assert ok.sum() >= w * h // world - 256
    same_pixels(got[ok], ref[idx[ok]])
    assert pt.march_guard_drops(r) == 0


@pytest.mark.parametrize("engine", [2, 1], ids=["wavefront", "megakernel"])
def test_clip_scene_both_engines(pt, scenes, engine):
    """trace_pixel's select (the megakernel) clips as the wavefront kernels do."""
    ps = scenes["clip"][0]
    ref = oracle_frame(scenes["clip"], 64, 64, 8)
    r = pt.HipRenderer(ps, depth=8)
    r.set_option("engine", engine)
    same_pixels(r.render(ps.camera(), pt.ImageParams(64, 64), SPP, seed=SEED), ref)
    assert pt.march_guard_drops(r) == 0


@pytest.mark.parametrize("engine", [2, 1], ids=["wavefront", "megakernel"])
def test_spheres_two_hearts(pt, spheres_text, engine):
    """Two marched shapes: wf_march selects its own jobs and clips each against the best hit so far, the other
    Heart's included."""
    ps = pt.Scene.from_json(spheres_text, seed=3)
    ref = O.Scene(spheres_text, seed=3).render(64, 64, SPP, 8, SEED, threads=host_threads())
    r = pt.HipRenderer(ps, depth=8)
    r.set_option("engine", engine)
    same_pixels(r.render(ps.camera(), pt.ImageParams(64, 64), SPP, seed=SEED), ref)
    assert pt.march_guard_drops(r) == 0


def test_textured_heart_scene(pt):
    """The extended (EXT) builds: the cube and the rectangle carry the image texture, whose lookups on those two
    shapes call no library function (tests/test_gpu_texture_rays.py holds them to exact equality), so the frame is
    the oracle's bit for bit."""
    img = {"type": "Lambertian", "albedo": T.TEXTURES["img"]}
    text = M.clip_scene(materials={"Red": M.RED, "Grey": img})
    ps = pt.Scene.from_json(text, random_spheres=False, images=T.IMAGES)
    ref = O.Scene(text, random_spheres=False, images=T.IMAGES).render(64, 64, SPP, 8, SEED, threads=host_threads())
    plain = O.Scene(M.clip_scene(), random_spheres=False).render(64, 64, SPP, 8, SEED, threads=host_threads())
    assert np.count_nonzero(np.any(ref != plain, axis=1)) > 100  # the texture is in the frame
    r = pt.HipRenderer(ps, depth=8)
    r.set_option("engine", 2)
    out = r.render(ps.camera(), pt.ImageParams(64, 64), SPP, seed=SEED)
    assert r.last_builds()["bounce"][2] == 1  # an EXT build
    same_pixels(out, ref)
    assert pt.march_guard_drops(r) == 0
