"""Texture and (u, v) lookups on the GPU, one ray at a time: the extended (EXT) builds' hit_uv and tex_value, where
the device leaves plain f64 arithmetic for the ROCm math library (acos, atan2, asin, cos, sin).

One light-emitting shape per scene whose `emit` is the texture, so HipRenderer.ray_color(rays, states, depth=1)
returns tex_value(hit_uv(...), point) per ray: no random number, no bounce, nothing averaged.  Cases, rays and the
mpmath reference are tests/texrays.py's; tests/test_texture_exact.py holds the oracle to the same reference on the
same rays, on the CPU.

Per case:
* Sphere, Rectangle, Cube: closest_hit equals the oracle in shape, t, point, normal and front_face (no library call
  lies on that path);
* the colour equals the oracle's ray_color(depth=1) and the RNG state comes back untouched;
* exact equality, nothing excused: Rectangle and Cube with the ImageTexture, every SolidColor-child case ("solid"),
  every deliberate texel-edge ray (rect_texel);
* elsewhere a differing ray is excused only when mpmath certifies a decision boundary at the oracle's hit (a sine
  factor below 1e-12, a texel edge within 1e-12 * w, the rim of asin's domain on the Torus), and at most 2 per case;
* Torus cases compare colours only on rays the Torus test calls decidable, and only where both sides hit;
* NoiseTexture: |gpu - 0.5 (1 + sin(arg))| <= 4 * 2^-52 per channel, mpmath's sine of the f64 argument, on up to
  300 hit rays per case.
"""
import numpy as np
import pytest

import texrays as T

pytestmark = pytest.mark.gpu

EXACT = {("rect_rot", "img"), ("cube_rot", "img"), ("cube", "img"), ("rect_texel", "img"),
         ("sphere_rot", "solid"), ("rect_rot", "solid"), ("cube_rot", "solid")}
MAX_EXCUSED = 2
MP_SAMPLE = 300


def check_case(pt, shape, tex):
    osc = T.oracle_scene(shape, tex)
    ps = T.product_scene(pt, shape, tex)
    sh = osc.shape(0)
    rays, edge = T.case_rays(shape, tex, list(sh.direct))
    states = T.ray_states(len(rays))
    r = pt.HipRenderer(ps, depth=8)
    got = r.closest_hit(rays)
    st_gpu = states.copy()
    col = r.ray_color(rays, st_gpu, depth=1)
    assert np.array_equal(st_gpu, states)  # a light draws no random number
    k = T.kind(shape)
    exact_hits = k in ("sphere", "rect", "cube")
    excused, differing, noise_checked, noise_max, hits_seen = 0, [], 0, 0.0, 0
    noise_stride = None
    for i, ray in enumerate(rays):
        h = osc.closest_hit(ray[:3], ray[3:])
        c, s = osc.ray_color(ray[:3], ray[3:], 1, int(states[i]))
        g = got[i]
        if exact_hits:
            if h is None:
                assert g["shape"] == -1, i
            else:
                assert (g["shape"], g["t"], list(g["point"]), list(g["normal"]), bool(g["front_face"])) == \
                       (h.shape, h.t, list(h.point), list(h.normal), bool(h.front_face)), (i, list(ray))
        if k == "torus" and (not T.torus_decidable(sh, ray) or (h is None) != (g["shape"] < 0)):
            continue  # hit or miss is tests/test_gpu_torus_rays.py's subject
        if h is None:
            assert list(col[i]) == list(c), i  # the sky, no library call
            continue
        hits_seen += 1
        if tex == "noise":
            if noise_stride is None:
                noise_stride = max(1, int(0.9 * len(rays)) // MP_SAMPLE)
            if hits_seen % noise_stride == 0:
                want, _ = T.reference_at(tex, sh, ray, h)
                dev = float(np.max(np.abs(col[i] - np.array(want))))
                noise_max = max(noise_max, dev)
                noise_checked += 1
                assert dev <= T.NOISE_TOL, (i, list(ray), list(col[i]), want, dev)
            continue
        if list(col[i]) == list(c):
            continue
        differing.append(i)
        assert (shape, tex) not in EXACT, (i, list(ray), list(col[i]), list(c))
        want, boundary = T.reference_at(tex, sh, ray, h)
        assert boundary, "ray %d %r: gpu %r, oracle %r, mpmath %r: no decision boundary here" % (
            i, list(ray), list(col[i]), list(c), want)
        excused += 1
    print("%s-%s: %d rays, %d hits, %d differ (all boundary-certified), noise: %d checked, max deviation %.3e"
          % (shape, tex, len(rays), hits_seen, excused, noise_checked, noise_max))
    assert excused <= MAX_EXCUSED, differing
    assert hits_seen >= 0.15 * len(rays)
    if tex == "noise":
        assert noise_checked >= 100
    return {"excused": excused, "noise_max": noise_max, "hits": hits_seen}


@pytest.mark.parametrize("shape,tex", T.CASES, ids=T.CASE_IDS)
def test_texture_lookup_per_ray(pt, shape, tex):
    check_case(pt, shape, tex)


def test_uvchecker_sphere_frame_both_engines(pt):
    """One UVChecker Sphere as a 32x18, 2-spp frame at depth 8 through the megakernel (engine 1) and the wavefront
    engine (2): the same bits, so what the per-ray probe pins holds for both engines' EXT builds."""
    ps = T.product_scene(pt, "sphere_rot", "uv")
    r = pt.HipRenderer(ps, depth=8)
    cam, ip = ps.camera(), pt.ImageParams(32, 18)
    r.set_option("engine", 1)
    mega = r.render(cam, ip, 2, seed=5)
    r.set_option("engine", 2)
    wave = r.render(cam, ip, 2, seed=5)
    assert np.array_equal(mega, wave)
    lit = np.all(np.isin(np.round(mega, 12), np.round(np.array(T.ODD + T.EVEN), 12)), axis=1)
    assert lit.sum() >= 10  # the sphere is in view: pixels whose both samples took one child
