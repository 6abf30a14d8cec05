"""The invariant the wavefront engine's early end rests on, pinned on the CPU.

wf_bounce ends a path whose new ray hit nothing (and has no march pending) in the launch that traced it, with
dev::decided_leaf's leaf, instead of storing its state and letting the next launch's dev::shade end it.  The frame
stays bit-identical only while shade, given who = -1, ends the path with background(ray.d) and touches nothing
else: no random number, no stack push, no change of depth or ray.  A change to shade that breaks this fails here.

The harness (tests/native/shade_miss_harness.cpp) is the product's pt_device.hpp compiled for the host with the
flags of tests/native/Makefile (-ffp-contract=off: the leaf's bits are the device's).
"""
import ctypes as C
import os
import re
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

HERE = Path(__file__).resolve().parent
DEPTHS = (1, 2, 8, 64)
BUILDS = {"heart": 0, "any": 1, "ext": 2}
NRAYS = 300


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    mk = (HERE / "native" / "Makefile").read_text()
    flags = re.search(r"^HFLAGS\s*=\s*(.*)$", mk, re.M).group(1).split()
    assert "-ffp-contract=off" in flags and "--offload-host-only" in flags
    hipcc = os.environ.get("HIPCC", re.search(r"^HIPCC\s*\?=\s*(\S+)", mk, re.M).group(1))
    lib = tmp_path_factory.mktemp("shade_miss") / "libshade_miss.so"
    subprocess.run([hipcc, *flags, "-o", str(lib), str(HERE / "native" / "shade_miss_harness.cpp")], check=True)
    L = C.CDLL(str(lib))
    L.h_shade_miss.argtypes = [C.c_int, C.POINTER(C.c_double), C.c_uint64, C.c_uint32, C.c_int,
                               C.POINTER(C.c_uint64)]
    L.h_shade_miss.restype = C.c_int
    L.h_decided_hit.argtypes = [C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    L.h_decided_hit.restype = None
    return L


def rays(n, seed):
    """Random origins and unit directions, with the axes, near-axis directions and a zero-length one among them."""
    rng = np.random.default_rng(seed)
    o = rng.uniform(-600.0, 600.0, size=(n, 3))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    special = [[0, 1, 0], [0, -1, 0], [1, 0, 0], [0, 0, -1], [1e-300, 1, 0], [0.6, -0.8, 0.0], [0, 0, 0]]
    d[: len(special)] = special
    return np.ascontiguousarray(np.concatenate([o, d], axis=1))


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def background_bits(dy):
    """background(d) (the reference's sky, renderer/mod.rs:42-44) in Python floats: IEEE doubles, one rounding per
    operation, as the harness computes it without contraction."""
    t = 0.5 * (dy + 1.0)
    u = 1.0 * (1.0 - t)
    return [bits(u + 0.5 * t), bits(u + 0.7 * t), bits(u + 1.0 * t)]


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("build", sorted(BUILDS))
def test_shade_of_a_miss_ends_with_the_background_and_touches_nothing(H, build, depth):
    R = rays(NRAYS, 100 + depth)
    rng = np.random.default_rng(7 * depth)
    states = rng.integers(0, 2 ** 63, size=NRAYS, dtype=np.uint64)
    counts = rng.integers(0, min(depth, 64) + 1, size=NRAYS)  # a path at this depth may have pushed this many ids
    out = (C.c_uint64 * 15)()
    for i in range(NRAYS):
        ray = R[i]
        assert H.h_shade_miss(BUILDS[build], ray.ctypes.data_as(C.POINTER(C.c_double)), int(states[i]), depth,
                              int(counts[i]), out) == 0
        o = list(out)
        assert o[0] == 1, "shade did not end the path"
        assert o[1:4] == o[4:7], "leaf is not background(ray.d)"
        assert o[1:4] == background_bits(ray[4])
        assert o[10] == 1 and o[7:10] == o[1:4], "shade_decided disagrees with shade"
        assert o[11] == int(states[i]), "a random number was drawn"
        assert o[12] == depth, "the depth changed"
        assert o[13] == int(counts[i]), "the stack count changed"
        assert o[14] == 1, "the ray or the stack changed"


def test_shade_decided_on_a_hit(H):
    """A hit is decided only at depth 0 (black, as shade's second branch); above it the shade has work to do."""
    ray = rays(8, 3)[7]
    out = (C.c_uint64 * 4)()
    H.h_decided_hit(0, ray.ctypes.data_as(C.POINTER(C.c_double)), out)
    assert list(out) == [1, bits(0.0), bits(0.0), bits(0.0)]
    for depth in DEPTHS:
        H.h_decided_hit(depth, ray.ctypes.data_as(C.POINTER(C.c_double)), out)
        assert list(out)[0] == 0
