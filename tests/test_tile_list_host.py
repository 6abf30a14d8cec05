"""Listed launches on the CPU: the host pieces of pt_adaptive.hpp (tile_list_ok, adaptive_list; the host build
tests/native/tile_list_harness.cpp) exhaustively; the exports, Python signatures and argument errors of
pt_render_device_tiles, pt_render_adaptive_list_device and pt_render_adaptive_list (no HIP call is made: every check
comes before the first use of the renderer, so a stand-in renderer pointer is never dereferenced)."""
import ctypes as C
import inspect
import itertools
import subprocess
from pathlib import Path

import numpy as np
import pytest

from conftest import native_lib

NATIVE = Path(__file__).resolve().parent / "native"
NAN = float("nan")
d = C.POINTER(C.c_double)
u32p = C.POINTER(C.c_uint32)
NAMES = ("pt_render_device_tiles", "pt_render_adaptive_list_device", "pt_render_adaptive_list")


@pytest.fixture(scope="module")
def T():
    subprocess.run(["make", "-s", "-C", str(NATIVE), "_build/libtilelist.so"], check=True)
    L = C.CDLL(native_lib("libtilelist.so"))
    L.tl_ok.restype = C.c_int
    L.tl_ok.argtypes = [u32p, C.c_size_t, C.c_uint32]
    L.tl_adaptive_list.restype = C.c_uint32
    L.tl_adaptive_list.argtypes = [C.POINTER(C.c_uint8), C.c_uint32, u32p]
    return L


# ---- tile_list_ok, adaptive_list ----

def test_tile_list_ok_exhaustive(T):
    """Every list of up to 4 entries drawn from 0..5, ntiles 5: only the strictly ascending in-range lists of one
    entry or more pass."""
    ntiles, passed = 5, 0
    for n in range(0, 5):
        for entries in itertools.product(range(6), repeat=n):
            a = np.array(entries, dtype=np.uint32)
            want = n >= 1 and all(e < ntiles for e in entries) and all(x < y for x, y in zip(entries, entries[1:]))
            assert T.tl_ok(a.ctypes.data_as(u32p), n, ntiles) == int(want), entries
            passed += want
    assert passed == 5 + 10 + 10 + 5  # the subsets of 0..4 of 1 to 4 elements
    assert T.tl_ok(None, 0, ntiles) == 0 and T.tl_ok(None, 3, ntiles) == 0
    one = np.array([0], dtype=np.uint32)
    assert T.tl_ok(one.ctypes.data_as(u32p), 1, 0) == 0 and T.tl_ok(one.ctypes.data_as(u32p), 1, 1) == 1
    top = np.array([0xFFFFFFFE, 0xFFFFFFFF], dtype=np.uint32)
    assert T.tl_ok(top.ctypes.data_as(u32p), 2, 0xFFFFFFFF) == 0 and T.tl_ok(top.ctypes.data_as(u32p), 1, 0xFFFFFFFF) == 1


def test_adaptive_list_exhaustive(T):
    out = np.zeros(12, dtype=np.uint32)
    for n in range(0, 13):
        for mask in range(1 << n):
            active = np.array([(mask >> i) & 1 for i in range(n)], dtype=np.uint8) * 3  # (any nonzero byte is active)
            cnt = T.tl_adaptive_list(active.ctypes.data_as(C.POINTER(C.c_uint8)), n, out.ctypes.data_as(u32p))
            want = [i for i in range(n) if (mask >> i) & 1]
            assert out[:cnt].tolist() == want
            if cnt:  # what adaptive_list gives is a list a listed launch takes
                assert T.tl_ok(out.ctypes.data_as(u32p), cnt, n) == 1


# ---- the C-ABI: exports, signatures ----

def test_exports(pt):
    L = C.CDLL(str(pt.LIB_PATH))
    header = (Path(__file__).resolve().parent.parent / "include" / "rs_pathtracing.h").read_text()
    for name in NAMES:
        assert name in pt.EXPORTS and hasattr(L, name)
        assert "int " + name + "(" in header
    assert "0.4.3" in pt.version() and pt.lib().pt_abi_version() == 4
    assert pt.adaptive_workspace_doubles(40, 24) == 40 * 24 * 3 * 3  # the list is the renderer's, not the workspace's


def test_python_signatures(pt):
    p = inspect.signature(pt.HipRenderer.render_device_tiles).parameters
    assert list(p) == ["self", "camera", "width", "height", "spp", "seed", "rank", "world", "s_begin", "s_end", "tiles",
                       "out_ptr", "stream_ptr"]
    assert p["stream_ptr"].default == 0
    for f in (pt.HipRenderer.render_adaptive, pt.HipRenderer.render_adaptive_device):
        q = inspect.signature(f).parameters
        assert q["tile_list"].default is False
        assert q["merge_gap"].default == pt.ADAPTIVE_MERGE_GAP  # the run-based entries keep their default
    # the signature table: the adaptive entries' without merge_gap; pt_render_device_samples' with the list
    L = pt.lib()
    assert len(L.pt_render_adaptive_list_device.argtypes) == len(L.pt_render_adaptive_device.argtypes) - 1
    assert len(L.pt_render_adaptive_list.argtypes) == len(L.pt_render_adaptive.argtypes) - 1
    assert len(L.pt_render_device_tiles.argtypes) == len(L.pt_render_device_samples.argtypes) + 2


# ---- argument errors: PT_ERR_INVALID, nothing written ----

TILES_BAD = {
    "null_renderer": dict(r=None),
    "null_camera": dict(cam=None),
    "null_out": dict(out=None),
    "null_tiles": dict(tiles=None),
    "zero_width": dict(w=0),
    "zero_height": dict(h=0),
    "zero_spp": dict(spp=0, s0=0, s1=0),
    "world_zero": dict(world=0),
    "rank_equals_world": dict(rank=2, world=2),
    "window_empty": dict(s0=2, s1=2),
    "window_reversed": dict(s0=3, s1=1),
    "window_past_spp": dict(s1=5),
    "count_zero": dict(n=0),
    "entry_out_of_range": dict(tiles=[0, 6]),
    "entry_out_of_range_for_the_rank": dict(tiles=[0, 3], rank=1, world=2),  # 6 tiles, 3 per rank
    "duplicate": dict(tiles=[1, 1, 2]),
    "descending": dict(tiles=[2, 1]),
    "unsorted_tail": dict(tiles=[0, 2, 4, 3]),
}


@pytest.mark.parametrize("case", list(TILES_BAD))
def test_render_device_tiles_argument_errors(pt, cornell_text, case):
    L = pt.lib()
    sc = pt.Scene.from_json(cornell_text)
    w, h = 40, 24  # 3 x 2 tiles
    stand_in = np.zeros(4096, dtype=np.uint8)
    out = np.full(w * h * 3, -7.25)
    a = dict(r=stand_in.ctypes.data, cam=C.byref(sc.camera()._c), w=w, h=h, spp=4, rank=0, world=1, s0=0, s1=4,
             tiles=[0, 2, 5], out=out.ctypes.data, n=None)
    a.update(TILES_BAD[case])
    tiles = None if a["tiles"] is None else np.array(a["tiles"], dtype=np.uint32)
    n = (0 if tiles is None else tiles.size) if a["n"] is None else a["n"]
    before = None if tiles is None else tiles.copy()
    rc = L.pt_render_device_tiles(a["r"], a["cam"], a["w"], a["h"], a["spp"], 1, a["rank"], a["world"], a["s0"],
                                  a["s1"], None if tiles is None else tiles.ctypes.data_as(u32p), n, a["out"], None)
    assert rc == pt.PT_ERR_INVALID, (case, rc)
    assert L.pt_last_error()
    assert np.all(out == -7.25) and not stand_in.any()
    assert tiles is None or np.array_equal(tiles, before)


def test_render_device_tiles_python_refuses_what_is_no_index(pt):
    """The wrapper turns `tiles` into uint32 itself: a negative or too large entry is refused before the call (it
    would wrap into a valid one)."""
    class Stub:
        _h = None
    with pytest.raises(ValueError):
        pt.HipRenderer.render_device_tiles(Stub(), None, 40, 24, 4, 1, 0, 1, 0, 4, [0, -1], 0)
    with pytest.raises(ValueError):
        pt.HipRenderer.render_device_tiles(Stub(), None, 40, 24, 4, 1, 0, 1, 0, 4, [1 << 32], 0)


ADAPTIVE_BAD = {
    "null_renderer": dict(r=None),
    "null_camera": dict(cam=None),
    "null_rgb": dict(rgb=None),
    "null_tile_samples": dict(ts=None),
    "zero_width": dict(w=0),
    "zero_height": dict(h=0),
    "zero_window": dict(window=0),
    "cap_equals_window": dict(cap=8),
    "cap_below_window": dict(cap=5),
    "cap_zero": dict(cap=0),
    "cap_above_2_32_minus_2": dict(cap=0xFFFFFFFF),
    "min_above_cap": dict(min_samples=65),
    "threshold_negative": dict(threshold=-0.1),
    "threshold_nan": dict(threshold=NAN),
    "floor_negative": dict(floor=-1.0),
    "floor_nan": dict(floor=NAN),
}


@pytest.mark.parametrize("case", list(ADAPTIVE_BAD))
def test_render_adaptive_list_argument_errors(pt, cornell_text, case):
    """pt_render_adaptive's own cases (tests/test_adaptive_host.py), through the list entry."""
    L = pt.lib()
    sc = pt.Scene.from_json(cornell_text)
    w, h = 40, 24
    stand_in = np.zeros(4096, dtype=np.uint8)
    rgb, var = np.full((w * h, 3), -7.25), np.full((w * h, 3), -7.25)
    ts, te = np.full(6, 0xDEAD, dtype=np.uint32), np.full(6, -7.25)
    launched = C.c_uint64(77)
    a = dict(r=C.c_void_p(stand_in.ctypes.data), cam=C.byref(sc.camera()._c), w=w, h=h, window=8, min_samples=0, cap=64,
             threshold=0.1, floor=0.01, rgb=rgb.ctypes.data_as(d), ts=ts.ctypes.data_as(u32p))
    a.update(ADAPTIVE_BAD[case])
    rc = L.pt_render_adaptive_list(a["r"], a["cam"], a["w"], a["h"], a["window"], a["min_samples"], a["cap"],
                                   a["threshold"], a["floor"], 1, a["rgb"], var.ctypes.data_as(d), a["ts"],
                                   te.ctypes.data_as(d), C.byref(launched))
    assert rc == pt.PT_ERR_INVALID, (case, rc)
    assert L.pt_last_error()
    assert np.all(rgb == -7.25) and np.all(var == -7.25) and np.all(ts == 0xDEAD) and np.all(te == -7.25)
    assert launched.value == 77 and not stand_in.any()


def test_render_adaptive_list_device_argument_errors(pt, cornell_text):
    L = pt.lib()
    sc = pt.Scene.from_json(cornell_text)
    cam = C.byref(sc.camera()._c)
    w, h = 40, 24
    buf = np.zeros(w * h * 3 * 5 + 2)
    base = buf.ctypes.data
    work = (base + w * h * 3 * 8 + 15) & ~15
    stand_in = np.zeros(4096, dtype=np.uint8)
    launched = C.c_uint64(77)

    def dev(r=stand_in.ctypes.data, cam=cam, rank=0, world=1, out=base, ts=base, wk=work, cap=64, window=8, w=w, h=h,
            min_samples=0, thr=0.1, floor=0.01):
        return L.pt_render_adaptive_list_device(r, cam, w, h, window, min_samples, cap, thr, floor, 1, rank, world, out,
                                                None, ts, None, wk, None, C.byref(launched))

    for bad in (dict(r=None), dict(cam=None), dict(out=None), dict(ts=None), dict(wk=None), dict(rank=1),
                dict(world=0), dict(rank=6, world=7), dict(cap=8), dict(cap=0xFFFFFFFF), dict(window=0), dict(w=0),
                dict(h=0), dict(min_samples=65), dict(thr=-0.1), dict(thr=NAN), dict(floor=-1.0), dict(floor=NAN)):
        assert dev(**bad) == pt.PT_ERR_INVALID, bad
        assert L.pt_last_error()
    assert dev(wk=work + 8) == pt.PT_ERR_INVALID and b"aligned" in L.pt_last_error()
    assert np.all(buf == 0.0) and not stand_in.any() and launched.value == 77
