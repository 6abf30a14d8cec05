"""The deep path on the CPU: ray_color with the attenuation-id stack in memory (dev::MemStack through dev::shade
and dev::unwind, pt_device.hpp: the stack type of the wavefront engine's frames, and what ray_color_probe_deep runs on
the GPU for depth > 64), compiled for the host from tests/native/deep_path_harness.cpp, against the oracle bit for bit on the closed room (scenes/deep_room.py).  The same
harness as a stand-alone program under AddressSanitizer and UBSan covers the new host code (the stack, the plan of
deep frames)."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import oracle as O
from deep_checks import deep_room as R

NATIVE = Path(__file__).resolve().parent / "native"
CSRC = NATIVE.parent.parent / "rs-pathtracing_amd" / "csrc"
HIPCC = "/opt/rocm/bin/hipcc"
# tests/native/Makefile's flags for host builds of the device headers
HFLAGS = ["-std=c++17", "-ffp-contract=off", "-x", "hip", "--offload-arch=gfx950", "--offload-host-only"]
SOURCES = [str(NATIVE / "deep_path_harness.cpp"), str(CSRC / "pt_scene.cpp"), str(CSRC / "pt_accel.cpp")]
DEPTHS = (65, 128, 500)


def build(out, flags, link):
    """The harness and the product sources it needs, one compiler process per source, then the link."""
    objs = [out.parent / (out.name + ".%d.o" % k) for k in range(len(SOURCES))]
    procs = [subprocess.Popen([HIPCC, *HFLAGS, *flags, "-c", src, "-o", str(obj)]) for src, obj in zip(SOURCES, objs)]
    assert [p.wait() for p in procs] == [0] * len(procs)
    subprocess.run([HIPCC, "--offload-arch=gfx950", "--offload-host-only", *link, "-o", str(out), *map(str, objs)],
                   check=True)


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    out = tmp_path_factory.mktemp("deep_host") / "libdeeppath.so"
    build(out, ["-O2", "-fPIC"], ["-shared"])
    L = C.CDLL(str(out))
    d = C.POINTER(C.c_double)
    L.h_scene_new.restype = C.c_void_p
    L.h_scene_new.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.c_uint64]
    L.h_scene_free.argtypes = [C.c_void_p]
    L.h_ray_color_mem.argtypes = [C.c_void_p, d, C.POINTER(C.c_uint64), C.c_size_t, C.c_uint32, d]
    L.h_ray_color.argtypes = [C.c_void_p, d, C.POINTER(C.c_uint64), C.c_uint32, d]
    return L


def rays_and_states(n, seed):
    rng = np.random.default_rng(seed)
    return R.inside_rays(n, rng), rng.integers(0, 2 ** 63, size=n, dtype=np.uint64)


def host_colors(H, text, rays, states, depth):
    raw = text.encode()
    h = H.h_scene_new(raw, len(raw), 0, 1)
    assert h
    st = states.copy()
    out = np.zeros((len(rays), 3))
    rays = np.ascontiguousarray(rays)
    H.h_ray_color_mem(h, rays.ctypes.data_as(C.POINTER(C.c_double)), st.ctypes.data_as(C.POINTER(C.c_uint64)),
                      len(rays), depth, out.ctypes.data_as(C.POINTER(C.c_double)))
    H.h_scene_free(h)
    return out, st


def oracle_colors(text, rays, states, depth):
    osc = O.Scene(text, random_spheres=False, seed=1)
    col, st = np.zeros((len(rays), 3)), np.zeros(len(rays), dtype=np.uint64)
    for i in range(len(rays)):
        c, s = osc.ray_color(rays[i, :3], rays[i, 3:], depth, int(states[i]))
        col[i], st[i] = list(c), s
    return col, st


@pytest.mark.parametrize("variant", R.VARIANTS)
@pytest.mark.parametrize("depth", DEPTHS)
def test_memory_stack_matches_oracle(H, variant, depth):
    text = R.room_json(variant)
    rays, states = rays_and_states(60 if variant == "heart" else 150, 100 + depth)
    col, st = host_colors(H, text, rays, states, depth)
    ref, rst = oracle_colors(text, rays, states, depth)
    assert np.array_equal(col, ref) and np.array_equal(st, rst)


def test_paths_really_run_deep():
    """The condition of the tests above: a good share of these rays' paths is still alive after 64 bounces (their
    colour at depth 500 is not their colour at depth 64)."""
    text = R.room_json("plain")
    rays, states = rays_and_states(150, 7)
    a, _ = oracle_colors(text, rays, states, 64)
    b, _ = oracle_colors(text, rays, states, 500)
    assert np.mean(np.any(a != b, axis=1)) > 0.25


def test_memory_stack_equals_register_stack_up_to_64(H):
    """Up to depth 64 the memory stack (MemStack, the wavefront engine's) and the register stack (h_ray_color,
    IdStack<32>) give the same bits."""
    text = R.room_json("textured")
    rays, states = rays_and_states(100, 3)
    raw = text.encode()
    h = H.h_scene_new(raw, len(raw), 0, 1)
    d = C.POINTER(C.c_double)
    for depth in (0, 1, 33, 64):
        col, st = host_colors(H, text, rays, states, depth)
        for i in range(len(rays)):
            s = C.c_uint64(int(states[i]))
            out = (C.c_double * 3)()
            H.h_ray_color(h, np.ascontiguousarray(rays[i]).ctypes.data_as(d), C.byref(s), depth, out)
            assert list(out) == list(col[i]) and s.value == int(st[i]), (depth, i)
    H.h_scene_free(h)


def test_sanitized_standalone_program(tmp_path):
    """The harness as a program of its own under ASan and UBSan: the deep ray_color at depth 500 on the textured room
    (ids and values of every level written and read back) and the plan of deep frames; its colours are the
    oracle's."""
    exe = tmp_path / "deep_path_main"
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-gpu-sanitize"]
    build(exe, ["-O1", "-DDEEP_HARNESS_MAIN", "-fno-omit-frame-pointer", *san], san)
    text = R.room_json("textured")
    rays, states = rays_and_states(40, 9)
    (tmp_path / "scene.json").write_text(text)
    rec = np.zeros(len(rays), dtype=[("ray", "<f8", 6), ("state", "<u8")])
    rec["ray"], rec["state"] = rays, states
    rec.tofile(tmp_path / "rays.bin")
    p = subprocess.run([str(exe), str(tmp_path / "scene.json"), str(tmp_path / "rays.bin"), "500",
                        str(tmp_path / "out.bin")], capture_output=True, text=True,
                       env={"ASAN_OPTIONS": "detect_leaks=1:halt_on_error=1", "UBSAN_OPTIONS": "halt_on_error=1"})
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.startswith("ok 40 rays depth 500") and "ERROR" not in p.stderr
    got = np.fromfile(tmp_path / "out.bin", dtype=[("col", "<f8", 3), ("state", "<u8")])
    ref, rst = oracle_colors(text, rays, states, 500)
    assert np.array_equal(got["col"], ref) and np.array_equal(got["state"], rst)
