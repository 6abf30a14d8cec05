"""Frames and probes deeper than 64 bounces on the GPU, against the C oracle on the closed room of scenes/deep_room.py
(nothing ends a path there but the lamp or depth 0, so most paths run deep) and on the reference's cornell box.

Above depth 64 every frame runs the wavefront engine's DEEP bounce builds (the attenuation-stack count in the spare
level of the slot's id stack instead of the path's who word) and pt_ray_color its memory-stack probe; the bar is the
one of test_gpu_parity.py (deep_checks.check_image): every pixel bit-exact, and per-channel RMS <= 1e-4."""
import functools
import subprocess
from pathlib import Path

import numpy as np
import pytest

import oracle as O
from deep_checks import RMS_TOL, check_image, rms
from deep_checks import deep_room as R

ROOT = Path(__file__).resolve().parent.parent
gpu = pytest.mark.gpu
W, H, SPP, SEED = 32, 32, 2, 3
DEPTHS = (65, 127, 128, 500)


@functools.lru_cache(maxsize=None)
def oracle_scene(variant):
    return O.Scene(R.room_json(variant), random_spheres=False, seed=1)


@functools.lru_cache(maxsize=None)
def oracle_frame(variant, depth):
    """The oracle's 32x32, 2-spp frame of the room, computed once per (variant, depth) and never written to."""
    img = oracle_scene(variant).render(W, H, SPP, depth, SEED)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def gpu_scene(variant):
    from conftest import load_package
    return load_package().Scene.from_json(R.room_json(variant), random_spheres=False, seed=1)


def gpu_frame(pt, variant, depth, devices=None, **opts):
    ps = gpu_scene(variant)
    r = pt.HipRenderer(ps, depth=depth, devices=devices)
    for k, v in opts.items():
        r.set_option(k, v)
    return r.render(ps.camera(), pt.ImageParams(W, H), SPP, seed=SEED)


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_room_paths_run_deep(variant):
    """The condition of every test below, on the oracle alone: the depth-500 frame differs from the depth-127 frame
    in more than a quarter of the pixels (measured 0.69, 0.68, 0.65), so paths longer than 127 bounces decide most of
    the picture and a count that wrapped at 64 or 128 could not pass."""
    differ = np.mean(np.any(oracle_frame(variant, 500) != oracle_frame(variant, 127), axis=1))
    assert differ > 0.25, differ


@gpu
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("variant", R.VARIANTS)
def test_deep_frame_parity(pt, variant, depth):
    img = gpu_frame(pt, variant, depth)
    ref = oracle_frame(variant, depth)
    exact = np.mean(np.all(img == ref, axis=1))
    print("\n%s depth %d: rms %s, bit-exact pixels %.6f" % (variant, depth, rms(img, ref), exact))
    assert np.all(np.isfinite(img)) and img.mean() > 0.05
    assert np.all(rms(img, ref) <= RMS_TOL), rms(img, ref)
    # every pixel bit-exact.  The textured room too: its checker calls the device's sin, so the tolerance above is
    # its bar as in the existing textured tests, but all four depths measured bit-exact on an MI355X and the
    # assertion holds the engine to that
    check_image(img, ref)


@gpu
@pytest.mark.parametrize("variant,n", [("plain", 500), ("textured", 500), ("heart", 150)])
def test_ray_color_probe_depth_300(pt, variant, n):
    """pt_ray_color at depth 300: the id stack of each ray in device memory.  Colour and returned RNG state bit for
    bit, the textured room included (measured bit-exact on an MI355X)."""
    ps, osc = gpu_scene(variant), oracle_scene(variant)
    r = pt.HipRenderer(ps, depth=8)
    rng = np.random.default_rng(300)
    rays = R.inside_rays(n, rng)
    states = rng.integers(0, 2 ** 63, size=n, dtype=np.uint64)
    st_gpu = states.copy()
    col = r.ray_color(rays, st_gpu, depth=300)
    bad = 0
    for i in range(n):
        c, s = osc.ray_color(rays[i, :3], rays[i, 3:], 300, int(states[i]))
        bad += not (list(col[i]) == list(c) and int(st_gpu[i]) == s)
    assert bad == 0, "%d of %d rays differ" % (bad, n)


@gpu
def test_both_sides_of_the_switch(pt):
    """Depth 64 (the packed count, the specialised builds) and depth 65 (the DEEP builds) both match the oracle."""
    for depth in (64, 65):
        check_image(gpu_frame(pt, "plain", depth), oracle_frame("plain", depth))
        check_image(gpu_frame(pt, "heart", depth), oracle_frame("heart", depth))


@gpu
def test_deep_progressive_frame(pt):
    """render_start / render_step without blocking: the progressive band feeder, stop gates in every iteration."""
    ps = gpu_scene("heart")
    r = pt.HipRenderer(ps, depth=200)
    buf = np.zeros((W * H, 3))
    r.start_rendering(ps.camera(), pt.ImageParams(W, H), SPP, seed=SEED)
    polls = 0
    while not r.render_step(buf):
        polls += 1
        assert polls < 10_000_000
    check_image(buf, oracle_frame("heart", 200))


@gpu
def test_deep_sample_windows(pt):
    """A depth-200 frame in two sample windows (pt_render_device_samples): running sums across two launches."""
    import torch
    ps = gpu_scene("plain")
    r = pt.HipRenderer(ps, depth=200)
    out = torch.full((W * H * 3,), float("nan"), dtype=torch.float64, device="cuda")
    for a, b in ((0, 1), (1, SPP)):
        r.render_device_samples(ps.camera(), W, H, SPP, SEED, 0, 1, a, b, out.data_ptr())
        torch.cuda.synchronize()
    check_image(out.cpu().numpy().reshape(-1, 3), oracle_frame("plain", 200))


@gpu
def test_deep_small_chunks_alternate_slots(pt):
    """wf_paths 256 on two slots: eight one-tile chunks per frame alternate the two slots' path state, so every
    slot's spare id level is reused by the next chunk's counts."""
    for variant in ("plain", "heart"):
        check_image(gpu_frame(pt, variant, 200, wf_paths=256, wf_slots=2), oracle_frame(variant, 200))


@gpu
def test_deep_frame_whatever_the_engine(pt):
    """engine 1 asks for the megakernel, whose register stack holds 64 ids: a deep frame takes the wavefront engine
    all the same; so do a two-rank renderer's shards (pt_renderer_create_multi, one device twice)."""
    ref = oracle_frame("plain", 200)
    check_image(gpu_frame(pt, "plain", 200, engine=1), ref)
    check_image(gpu_frame(pt, "plain", 200, devices=[0, 0]), ref)


@gpu
def test_depth_limit(pt):
    ps = gpu_scene("plain")
    assert pt.MAX_DEPTH >= 4096
    for make in (lambda: pt.HipRenderer(ps, depth=pt.MAX_DEPTH + 1),
                 lambda: pt.HipRenderer(ps, depth=pt.MAX_DEPTH + 1, devices=[0]),
                 lambda: pt.HipRenderer(ps, depth=2 ** 32 - 1)):
        with pytest.raises(pt.PtError) as e:
            make()
        assert e.value.code == pt.PT_ERR_UNSUPPORTED and str(pt.MAX_DEPTH) in str(e.value)
    r = pt.HipRenderer(ps, depth=8)
    ray, st = np.array([[0.0, 0, 0, 0, 0, 1]]), np.array([1], dtype=np.uint64)
    with pytest.raises(pt.PtError) as e:
        r.ray_color(ray, st, depth=pt.MAX_DEPTH + 1)
    assert e.value.code == pt.PT_ERR_UNSUPPORTED and str(pt.MAX_DEPTH) in str(e.value)
    # the limit itself is taken
    deep = pt.HipRenderer(ps, depth=pt.MAX_DEPTH)
    assert deep.ray_color(ray, st.copy(), depth=pt.MAX_DEPTH).shape == (1, 3)
    # the probes that run the register stacks say so by name
    with pytest.raises(pt.PtError) as e:
        deep.trace_pixel_samples(ps.camera(), pt.ImageParams(W, H), 1, np.array([5], np.uint32), seed=1)
    assert e.value.code == pt.PT_ERR_UNSUPPORTED and "pt_trace_pixel_samples" in str(e.value)
    with pytest.raises(pt.PtError) as e:
        pt.count_work(deep, ps.camera(), pt.ImageParams(W, H), 1, np.array([5], np.uint32), seed=1)
    assert e.value.code == pt.PT_ERR_UNSUPPORTED and "pt_count_work" in str(e.value)


@gpu
def test_frame_at_the_depth_limit(pt):
    """A small frame at PT_MAX_DEPTH: 4098 iterations queued per chunk, counts up to 4096."""
    img = gpu_frame(pt, "plain", pt.MAX_DEPTH)
    check_image(img, oracle_scene("plain").render(W, H, SPP, pt.MAX_DEPTH, SEED))


@gpu
def test_workspace_misfit_is_refused_before_any_launch(pt):
    """One sample of a 1080p frame of the textured room at PT_MAX_DEPTH needs 240 GB of workspace at the smallest
    chunk (2,088,960 paths x (4097 x 28 + 185) bytes and the shared sums, one stream).  With all but 200 GB of the
    device held elsewhere the frame is refused: PT_ERR_UNSUPPORTED, and the message says what did not fit.  Nothing
    was queued: the renderer then renders a frame that fits."""
    import torch
    ps = gpu_scene("textured")
    r = pt.HipRenderer(ps, depth=pt.MAX_DEPTH)
    w, h = 1920, 1080
    out = torch.zeros(w * h * 3, dtype=torch.float64, device="cuda")
    free, _ = torch.cuda.mem_get_info()
    hog = torch.empty(max(free - 200 * 10**9, 1), dtype=torch.uint8, device="cuda")
    try:
        with pytest.raises(pt.PtError) as e:
            r.render_device_samples(ps.camera(), w, h, 1, SEED, 0, 1, 0, 1, out.data_ptr())
    finally:
        del hog
        torch.cuda.empty_cache()
    msg = str(e.value)
    assert e.value.code == pt.PT_ERR_UNSUPPORTED, msg
    assert "does not fit" in msg and "depth %d, textured scene" % pt.MAX_DEPTH in msg, msg
    assert "2088960 paths per chunk on 1 stream(s)" in msg and " bytes available" in msg, msg
    need = int(msg.split(" need ")[1].split(" bytes")[0])
    assert need == 240073811200, msg  # the plan's bytes (pt_plan.hpp; tests/test_deep_plan.py checks the arithmetic)
    small = r.render(ps.camera(), pt.ImageParams(W, H), SPP, seed=SEED)
    check_image(small, oracle_scene("textured").render(W, H, SPP, pt.MAX_DEPTH, SEED))


@gpu
def test_large_tree_depth_65(pt):
    """20,000 spheres: a tree of at least 2^15 nodes, which up to depth 64 runs the large-tree bounce builds and the
    wf_walk route.  A deep frame takes the generic DEEP build all the same."""
    import json
    import make_scenes  # (scenes/, on the path through deep_checks)
    from conftest import host_threads
    text = json.dumps(make_scenes.synthetic(20000))
    ps = pt.Scene.from_json(text, seed=1)
    r = pt.HipRenderer(ps, depth=65)
    assert r.get_option("bvh_nodes") >= 1 << 15, "not a large tree"
    img = r.render(ps.camera(), pt.ImageParams(48, 27), 2, seed=3)
    ref = O.Scene(text, seed=1).use_bvh(True, 7).render(48, 27, 2, 65, 3, threads=host_threads())
    check_image(img, ref)


@gpu
def test_cornell_depth_65(pt, cornell_text):
    """The reference's own scene through the DEEP builds: the Heart's march, the BVH of the random spheres."""
    ps, osc = pt.Scene.from_json(cornell_text, seed=1), O.Scene(cornell_text, seed=1)
    img = pt.HipRenderer(ps, depth=65).render(ps.camera(), pt.ImageParams(48, 27), 2, seed=1)
    check_image(img, osc.render(48, 27, 2, 65, 1))


@gpu
def test_cli_depth_200_with_checkpointed_windows(pt, cornell_text, tmp_path):
    """tools/pt_render -d 200 (refused before the cap was lifted), in sample windows with a checkpoint between them:
    the frame is the library's one-shot frame."""
    exe = str(ROOT / "tools" / "pt_render")
    p = subprocess.run([exe, str(ROOT / "scenes" / "cornell_box.json"), "4", "48", "27", "-d", "200", "-s", "3",
                        "-c", str(tmp_path / "f.ckpt"), "-n", "2", "-f", str(tmp_path / "f.f64"), "-o", ""],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    assert "depth 200" in p.stdout
    ps = pt.Scene.from_json(cornell_text, seed=1)
    want = pt.HipRenderer(ps, depth=200).render(ps.camera(), pt.ImageParams(48, 27), 4, seed=3)
    assert (tmp_path / "f.f64").read_bytes() == want.tobytes()
