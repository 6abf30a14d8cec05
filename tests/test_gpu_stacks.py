"""The attenuation stacks at every width, tested where the stack is read.

A path that ends at depth 0 multiplies black by its whole stack of attenuations, so only a path that ends on a light
(or the sky) after many bounces shows what its deep stack levels held.  The spheres and cornell frames of
test_gpu_parity.py have next to none of those; the closed room of scenes/deep_room.py has little else.  Here the
room's `plain` and `heart` variants, 32x32 at 8 spp, go through every stack width of 64 ids or fewer: the megakernel's
register stacks of 8, 16 and 32 words (render_tiles<NW, 2, F_ANY>, builds::stack_words) on both sides of each width,
the wavefront engine's memory stacks at the same depths, and the probes' builds of those widths (pt_ray_color,
pt_trace_pixel_samples, pt_count_work).  test_gpu_deep.py has the depths above 64.

A third scene, `plain-lamp-first`, is `plain` with its materials listed in another order, the lamp first.  In the room
as written material 0 is the wall, which nearly every deep bounce hits, so a stack that lost an id and read back 0
would mostly read the right material: a host build whose IdStack<8> zeroes its top word renders the depth-16 frames of
`plain` and `heart` without one wrong pixel, and one that zeroes its upper four words changes 0.023 and 0.039 of
their pixels.  With the lamp as material 0 the same two builds change 0.013 and 0.196 of the pixels.  The order of
the materials decides no pixel (the first test asserts it), so the oracle's frames are those of `plain`.

The bar is the one of test_gpu_parity.py (deep_checks.check_image): every pixel bit-exact, per-channel RMS <= 1e-4.
The first test is the condition the others rest on, on the oracle alone."""
import ctypes as C
import functools
import json
import subprocess
from pathlib import Path

import numpy as np
import pytest

import oracle as O
from conftest import native_lib
from deep_checks import check_image
from deep_checks import deep_room as R

gpu = pytest.mark.gpu
W, H, SPP, SEED = 32, 32, 8, 3
VARIANTS = ("plain", "heart", "plain-lamp-first")
F_ANY = -1
NRAYS = 500


def stack_words(depth):
    """builds::stack_words (pt_builds.hpp): 64-bit words of the register id stack, two ids each."""
    return 4 if depth <= 8 else 8 if depth <= 16 else 16 if depth <= 32 else 32


@functools.lru_cache(maxsize=None)
def room_json(variant):
    if variant != "plain-lamp-first":
        return R.room_json(variant)
    doc = json.loads(R.room_json("plain"))
    doc["materials"] = {k: doc["materials"][k] for k in ("Lamp", "Wall", "Glass", "Metal")}
    return json.dumps(doc)


@functools.lru_cache(maxsize=None)
def oracle_scene(variant):
    return O.Scene(room_json(variant), random_spheres=False, seed=1)


@functools.lru_cache(maxsize=None)
def oracle_frame(variant, depth):
    """The oracle's 32x32, 8-spp frame of the room, computed once per (variant, depth) and never written to."""
    img = oracle_scene(variant).render(W, H, SPP, depth, SEED)
    img.setflags(write=False)
    return img


def probe_rays():
    """The rays and RNG states of test_gpu_deep.test_ray_color_probe_depth_300 at n = 500."""
    rng = np.random.default_rng(300)
    rays = R.inside_rays(NRAYS, rng)
    return rays, rng.integers(0, 2 ** 63, size=NRAYS, dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def oracle_rays(variant, depth):
    """(colours, returned RNG states) of the probe rays at this depth, once per (variant, depth)."""
    osc = oracle_scene(variant)
    rays, states = probe_rays()
    got = [osc.ray_color(rays[i, :3], rays[i, 3:], depth, int(states[i])) for i in range(NRAYS)]
    col, st = np.array([c for c, _ in got]), np.array([s for _, s in got], dtype=np.uint64)
    col.setflags(write=False)
    st.setflags(write=False)
    return col, st


@functools.lru_cache(maxsize=None)
def gpu_scene(variant):
    from conftest import load_package
    return load_package().Scene.from_json(room_json(variant), random_spheres=False, seed=1)


def gpu_frame(pt, variant, depth, engine):
    ps = gpu_scene(variant)
    r = pt.HipRenderer(ps, depth=depth)
    r.set_option("engine", engine)
    return r.render(ps.camera(), pt.ImageParams(W, H), SPP, seed=SEED), r.last_builds()


@pytest.mark.parametrize("variant", VARIANTS)
def test_deep_stack_levels_decide_pixels(variant):
    """The condition of every GPU test below, on the oracle alone: going from depth 8 to 16, 16 to 32 and 32 to 64
    changes at least 0.15, 0.30 and 0.45 of the frame's pixels (measured 0.238, 0.427, 0.645 on `plain` and 0.237,
    0.421, 0.630 on `heart`; the floors sit well under that because the share depends on spp and seed, not on the
    device) and at least 15, 20 and 30 of the 500 probe rays (measured 24, 31, 50 and 23, 29, 47).  So ids in the
    upper half of each stack width are read back and decide a large part of the picture.  `plain-lamp-first` is
    `plain` bit for bit, frames and rays."""
    if variant == "plain-lamp-first":
        assert json.loads(room_json(variant))["materials"].keys() == json.loads(room_json("plain"))["materials"].keys()
        assert list(json.loads(room_json(variant))["materials"])[0] == "Lamp"
        for depth in (8, 16, 32, 64):
            assert np.array_equal(oracle_frame(variant, depth), oracle_frame("plain", depth))
            for got, want in zip(oracle_rays(variant, depth), oracle_rays("plain", depth)):
                assert np.array_equal(got, want)
    for (a, b), share, count in zip(((16, 8), (32, 16), (64, 32)), (0.15, 0.30, 0.45), (15, 20, 30)):
        differ = np.mean(np.any(oracle_frame(variant, a) != oracle_frame(variant, b), axis=1))
        rays = int(np.sum(np.any(oracle_rays(variant, a)[0] != oracle_rays(variant, b)[0], axis=1)))
        print("\n%s depth %d vs %d: share of pixels %.4f (floor %.2f), rays %d (floor %d)" % (
            variant, a, b, differ, share, rays, count))
        assert differ >= share, (a, b, differ)
        assert rays >= count, (a, b, rays)


@gpu
@pytest.mark.parametrize("depth", [9, 16, 17, 32, 33, 64])
@pytest.mark.parametrize("variant", VARIANTS)
def test_megakernel_register_stacks(pt, variant, depth):
    """render_tiles at 8, 16 and 32 words with the top levels live, on both sides of each width."""
    img, ran = gpu_frame(pt, variant, depth, engine=1)
    assert ran["engine"] == 0 and ran["mega"] == (stack_words(depth), 2, F_ANY), ran
    assert ran["bounce"] is None and ran["walk"] is None and ran["march"] is None, ran
    check_image(img, oracle_frame(variant, depth))


@gpu
@pytest.mark.parametrize("depth", [16, 17, 32, 33, 64])
@pytest.mark.parametrize("variant", VARIANTS)
def test_wavefront_memory_stacks(pt, variant, depth):
    """The wavefront engine's id stacks in memory at the same depths (up to 64 the specialised builds, the count
    packed beside the path's who word)."""
    img, ran = gpu_frame(pt, variant, depth, engine=2)
    assert ran["engine"] == 1 and ran["mega"] is None and ran["bounce"] is not None, ran
    assert ran["bounce"][5] == 0, ran  # not a DEEP build
    assert (ran["march"] is not None) == (variant == "heart"), ran  # (launched iff the scene has a marched shape)
    check_image(img, oracle_frame(variant, depth))


@gpu
@pytest.mark.parametrize("depth", [16, 32, 64])
@pytest.mark.parametrize("variant", VARIANTS)
def test_ray_color_probe_stack_widths(pt, variant, depth):
    """pt_ray_color's builds of 8, 16 and 32 words: colour and returned RNG state bit for bit."""
    r = pt.HipRenderer(gpu_scene(variant), depth=8)
    rays, states = probe_rays()
    st_gpu = states.copy()
    col = r.ray_color(rays, st_gpu, depth=depth)
    want_col, want_st = oracle_rays(variant, depth)
    bad = np.flatnonzero(np.any(col != want_col, axis=1) | (st_gpu != want_st))
    assert bad.size == 0, "%d of %d rays differ (first %s)" % (bad.size, NRAYS, bad[:8].tolist())


@gpu
@pytest.mark.parametrize("depth", [16, 64])
@pytest.mark.parametrize("variant", VARIANTS)
def test_trace_pixel_samples_stack_widths(pt, variant, depth):
    """pt_trace_pixel_samples over every pixel of the frame: the oracle's render of those pixels."""
    ps = gpu_scene(variant)
    r = pt.HipRenderer(ps, depth=depth)
    pixels = np.arange(W * H, dtype=np.uint32)
    got = r.trace_pixel_samples(ps.camera(), pt.ImageParams(W, H), SPP, pixels, seed=SEED)
    ref = oracle_scene(variant).render(W, H, SPP, depth, SEED, pixels=pixels)
    assert np.array_equal(ref, oracle_frame(variant, depth))
    check_image(got, ref)


@gpu
@pytest.mark.parametrize("variant", VARIANTS)
def test_count_work_depth_16(pt, variant):
    """pt_count_work's 8-word build: samples = pixels x spp, and every counter equals the host build's of the same
    code (tests/native/path_harness.cpp), as test_gpu_parity.test_count_work_matches_host_build has it at depth 8."""
    native = Path(__file__).resolve().parent / "native"
    subprocess.run(["make", "-s", "-C", str(native)], check=True)
    L = C.CDLL(native_lib("libpath.so"))
    L.h_scene_new.restype = C.c_void_p
    L.h_scene_new.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.c_uint64]
    L.h_scene_free.argtypes = [C.c_void_p]
    L.h_count_work.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64,
                               C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(C.c_uint64)]
    raw = room_json(variant).encode()
    h = L.h_scene_new(raw, len(raw), 0, 1)
    assert h
    ps = gpu_scene(variant)
    r = pt.HipRenderer(ps, depth=16)
    px = np.arange(W * H, dtype=np.uint32)
    got = pt.count_work(r, ps.camera(), pt.ImageParams(W, H), SPP, px, seed=SEED)
    want = (C.c_uint64 * len(pt.COUNTERS))()
    L.h_count_work(h, W, H, SPP, 16, SEED, px.ctypes.data_as(C.POINTER(C.c_uint32)), len(px), want)
    L.h_scene_free(h)
    assert got["samples"] == W * H * SPP
    assert got["bounces"] > 8 * got["samples"]  # (paths do run deep: more than 8 bounces a sample on average)
    assert got == dict(zip(pt.COUNTERS, list(want)))
