"""The guide-plane pass on the CPU: dev::aov_pixel (rs-pathtracing_amd/csrc/pt_aov.hpp), the function the
aov_tiles kernel runs per lane, compiled for the host by tests/native/Makefile and run over every pixel, against the
planes tests/aovref.py computes from the oracle's pieces.  Bit for bit, except the textured scene (host libm on
both sides here, but the project's frame tolerance is what the planes promise).  tests/test_gpu_aov.py repeats the
comparison with the same code compiled for gfx950."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import aovref
from conftest import ROOT, native_lib

NATIVE = Path(__file__).resolve().parent / "native"


@pytest.fixture(scope="module")
def A():
    subprocess.run(["make", "-s", "-C", str(NATIVE), "_build/libaov.so"], check=True)
    L = C.CDLL(native_lib("libaov.so"))
    d = C.POINTER(C.c_double)
    L.a_scene_new.restype = C.c_void_p
    L.a_scene_new.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.c_uint64]
    L.a_scene_free.argtypes = [C.c_void_p]
    L.a_planes.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_int, C.c_int, C.c_int,
                           d, d, d]
    L.a_planes.restype = C.c_int
    return L


SENTINEL = -7.25


def host_planes(A, name, want_albedo=True, want_normal=True, ext=-1, ran=None):
    """ext: -1 the build the launcher picks for the scene, 1 the extended build, 0 the plain one; ran (a list)
    receives the build that ran."""
    text, rs, w, h, spp, _, _ = aovref.case(name)
    raw = text.encode()
    hs = A.a_scene_new(raw, len(raw), 1 if rs else 0, 1)
    assert hs
    try:
        out = {p: np.full((w * h, 3), SENTINEL) for p in aovref.PLANES}
        d = C.POINTER(C.c_double)
        got = A.a_planes(hs, w, h, spp, aovref.FRAME_SEED, ext, int(want_albedo), int(want_normal),
                         *[out[p].ctypes.data_as(d) for p in aovref.PLANES])
        if ran is not None:
            ran.append(got)
    finally:
        A.a_scene_free(hs)
    return out


@pytest.mark.parametrize("name", ["spheres", "cornell", "marched"])
def test_planes_equal_the_oracle(A, name):
    ref = aovref.case(name)[6]
    aovref.assert_not_degenerate(ref["depth"])
    aovref.same_planes(host_planes(A, name), ref)


@pytest.mark.parametrize("name", ["spheres", "cornell", "marched", "light"])
def test_the_extended_build_takes_plain_scenes(A, name):
    """A scene without a Torus or a non-solid texture gets the plain build; the extended one (every scene's) gives
    the same bits on it."""
    ran = []
    auto = host_planes(A, name, ran=ran)
    ext = host_planes(A, name, ext=1, ran=ran)
    assert ran == [0, 1]
    aovref.same_planes(ext, auto)
    aovref.same_planes(ext, aovref.case(name)[6])


def test_first_hits_cover_the_materials():
    """spheres.json shows the camera Lambertian, Metal and Dielectric first hits (the albedo plane's three
    ordinary branches)."""
    import oracle as O
    text, rs, w, h, spp, osc, ref = aovref.case("spheres")
    L = O.lib()
    k = osc.caster(w, h)
    o, d = (C.c_double * 3)(), (C.c_double * 3)()
    kinds = set()
    for p in range(0, w * h, 3):
        st = C.c_uint64(L.or_sample_key(aovref.FRAME_SEED, p, 0))
        u, v = L.or_gen_f64(C.byref(st)), L.or_gen_f64(C.byref(st))
        L.or_caster_ray(C.byref(k), p % w + u, p // w + v, o, d)
        hit = osc.closest_hit(o, d)
        if hit is not None:
            kinds.add(osc.material(hit.material).type)
    assert {O.LAMBERTIAN, O.METAL, O.DIELECTRIC} <= kinds, kinds


def test_light_is_not_clamped(A):
    ref = aovref.case("light")[6]
    got = host_planes(A, "light")
    aovref.same_planes(got, ref)
    none, full, part = aovref.coverage_kinds(ref["depth"])
    assert none >= 100 and full >= 100 and part >= 10, (none, full, part)
    lit = got["depth"][:, 1] == 1.0
    assert np.all(got["albedo"][lit] == 15.0)
    assert np.all(got["normal"][lit] == [0.0, 0.0, -1.0])  # the lamp's normal, turned against the ray


def test_all_miss(A):
    import oracle as O
    text, rs, w, h, spp, osc, ref = aovref.case("all_miss")
    got = host_planes(A, "all_miss")
    aovref.same_planes(got, ref)
    assert np.all(got["normal"] == 0.0) and np.all(got["depth"] == 0.0)
    sky = osc.render(w, h, spp, 0, aovref.FRAME_SEED)  # depth 0: every miss is the sky
    assert np.array_equal(got["albedo"], sky)
    assert np.all(sky >= 0.5 - 1e-9) and np.allclose(sky[:, 2], 1.0)  # the sky's gradient: blue is 1 everywhere


def test_textured_within_the_frame_tolerance(A, monkeypatch):
    monkeypatch.chdir(ROOT)  # (the scene's image texture is named relative to the repository)
    import oracle as O
    text, rs, w, h, spp, osc, ref = aovref.case("textured")
    aovref.assert_not_degenerate(ref["depth"])
    # first hits on textured Lambertian and textured Metal: some albedo pixel's value is a texture's
    mats = [osc.material(i) for i in range(osc.num_materials)]
    assert any(m.type == O.LAMBERTIAN and m.tex >= 0 for m in mats)
    assert any(m.type == O.METAL and m.tex >= 0 for m in mats)
    ran = []
    aovref.close_planes(host_planes(A, "textured", ran=ran), ref)
    assert ran == [1]  # the launcher's choice for a textured scene: the extended build


@pytest.mark.parametrize("name", ["cornell", "marched"])
def test_without_the_albedo_the_others_keep_their_bits(A, name):
    ref = aovref.case(name)[6]
    got = host_planes(A, name, want_albedo=False)
    assert np.all(got["albedo"] == SENTINEL)
    aovref.same_planes(got, ref, ("normal", "depth"))


def test_depth_alone(A):
    """Neither albedo nor normal: no hit frame is computed, the depth plane keeps its bits."""
    ref = aovref.case("spheres")[6]
    got = host_planes(A, "spheres", want_albedo=False, want_normal=False)
    assert np.all(got["albedo"] == SENTINEL) and np.all(got["normal"] == SENTINEL)
    aovref.same_planes(got, ref, ("depth",))


def test_exports(pt):
    """Both entry points are in the binding's list and in the library (tests/test_abi.py checks the whole
    header)."""
    L = C.CDLL(str(pt.LIB_PATH))
    for name in ("pt_render_aov", "pt_render_aov_device"):
        assert name in pt.EXPORTS and hasattr(L, name)
    assert "0.4.3" in pt.version()
