"""Adaptive sampling on the CPU: the host build of pt_adaptive.hpp (tests/native/adaptive_harness.cpp) against the
numpy restatement tests/adaptiveref.py, bit for bit, on seeded synthetic running sums; adaptive_runs exhaustively;
the C-ABI's exports, Python signatures and argument errors (no HIP call is made).

NaN payloads are no part of the contract: where both sides hold a NaN they count as equal."""
import ctypes as C
import inspect
import subprocess
from pathlib import Path

import numpy as np
import pytest

import adaptiveref
from conftest import native_lib

NATIVE = Path(__file__).resolve().parent / "native"
INF = float("inf")
NAN = float("nan")
d = C.POINTER(C.c_double)
u32p = C.POINTER(C.c_uint32)
PLANS = [(1, 2), (3, 7), (8, 20), (8, 64)]  # (window, cap)


@pytest.fixture(scope="module")
def A():
    subprocess.run(["make", "-s", "-C", str(NATIVE), "_build/libadaptive.so"], check=True)
    L = C.CDLL(native_lib("libadaptive.so"))
    L.ad_window.restype = C.c_size_t
    L.ad_window.argtypes = ([C.c_uint32] * 5 + [C.c_size_t] + [C.c_uint32] * 4 +
                            [C.c_double, C.c_double, d, d, d, u32p, d])
    L.ad_edge.restype = C.c_uint32
    L.ad_edge.argtypes = [C.c_uint32] * 3
    L.ad_windows.restype = C.c_uint32
    L.ad_windows.argtypes = [C.c_uint32] * 2
    L.ad_runs.restype = C.c_uint32
    L.ad_runs.argtypes = [C.POINTER(C.c_uint8), C.c_uint32, C.c_uint32, u32p]
    return L


def host_adaptive(A, sums, w, h, window, cap, threshold, floor=0.01, min_samples=0, rank=0, world=1,
                  with_optional=True):
    """Every window through the host build, on a workspace that starts as garbage.  sums: per window, d_out's layout
    for this rank (the whole frame, or the compact shard).  Returns (out, variance, tile_samples, tile_error) and
    checks that a stopped tile is never written again."""
    count = sums[0].size
    tx, ty = adaptiveref.tiles_of(w, h)
    ntiles = len(range(rank, tx * ty, world))
    work = np.full(3 * count, np.nan)
    out, var = np.full(count, -7.25), np.full(count, -7.25)
    ts, te = np.full(ntiles, 0xDEAD, dtype=np.uint32), np.full(ntiles, -7.25)
    for k in range(1, len(sums) + 1):
        work[:count] = np.asarray(sums[k - 1], dtype=np.float64).reshape(-1)
        before = (out.copy(), var.copy(), ts.copy(), te.copy())
        assert A.ad_window(w, h, rank, world, ntiles, count, k, window, min_samples, cap, threshold, floor,
                           work.ctypes.data_as(d), out.ctypes.data_as(d),
                           var.ctypes.data_as(d) if with_optional else None, ts.ctypes.data_as(u32p),
                           te.ctypes.data_as(d) if with_optional else None) == 3 * count
        if k > 1:
            done = before[2] != 0
            assert np.all(ts[done] == before[2][done])
            assert np.array_equal(te[done], before[3][done], equal_nan=True)
        else:
            assert np.all(ts == 0) and np.all(out == -7.25)
    return out, var, ts, te


def same(got, ref, what):
    got, ref = np.asarray(got).reshape(-1), np.asarray(ref).reshape(-1)
    bad = np.flatnonzero(~((got == ref) | (np.isnan(got) & np.isnan(ref))))
    assert bad.size == 0, "%s: %d of %d differ (first %s)" % (what, bad.size, ref.size, bad[:8].tolist())
    finite = np.isfinite(ref)  # the sign of a zero too
    assert np.all(np.signbit(got[finite]) == np.signbit(ref[finite])), what


def check_frame(A, w, h, window, cap, threshold, floor=0.01, min_samples=0):
    snaps = adaptiveref.synthetic(w, h, window, cap)
    rgb, var, ts, te = adaptiveref.adaptive(snaps, w, h, window, cap, threshold, floor, min_samples)
    out, v, s, e = host_adaptive(A, snaps, w, h, window, cap, threshold, floor, min_samples)
    assert np.array_equal(s, ts), (s.tolist(), ts.tolist())
    same(e, te, "tile_error")
    same(out, rgb, "frame")
    same(v, var, "variance")
    return snaps, rgb, var, ts, te


# ---- the windows ----

def test_window_edges(A):
    assert adaptiveref.edges(8, 20) == [0, 8, 16, 20]
    for window, cap in PLANS + [(32, 256), (5, 6)]:
        k = A.ad_windows(window, cap)
        assert [A.ad_edge(j, window, cap) for j in range(k + 1)] == adaptiveref.edges(window, cap)
        assert k >= 2
    cap = 0xFFFFFFFE  # the product k * window is taken in 64 bits
    assert A.ad_windows(0x80000000, cap) == 2 and A.ad_edge(2, 0x80000000, cap) == cap
    assert A.ad_edge(1, 0x80000000, cap) == 0x80000000


# ---- the pass, bit for bit against the restatement ----

@pytest.mark.parametrize("window,cap", PLANS)
def test_synthetic_sums_equal_the_restatement(A, window, cap):
    w, h = 40, 24
    snaps, rgb, var, ts, te = check_frame(A, w, h, window, cap, 0.02)
    # the inputs hold what they are for
    tiles = adaptiveref.to_tiles(snaps[-1], w, h)
    assert np.all(tiles[1] == tiles[1][0, 0]) and np.all(tiles[2] == 0.0)      # all equal; zero luminance
    assert np.isnan(tiles[3]).sum() == 1 and np.isinf(tiles[4]).sum() == 1
    second = adaptiveref.edges(window, cap)[2]
    assert ts[1] == second and ts[2] == second                # zero variance converges at the first evaluation
    assert te[1] == 0.0 and te[2] == 0.0                      # (the floor: 0 / (floor * nn)^2, not 0 / 0)
    assert ts[3] == cap and ts[4] == cap and np.isnan(te[3]) and np.isnan(te[4])  # NaN, inf: never converged
    assert np.all(var[np.isfinite(var)] >= 0.0)
    if cap == 64:
        # the rule is exercised: tiles stop at different windows
        assert len(set(ts.tolist())) >= 4 and 16 < ts[0] < ts[5] < cap


def test_m2_clamp():
    """An element whose samples are all equal can round m2 below 0: it is clamped to +0."""
    snaps = adaptiveref.synthetic(40, 24, 3, 7)
    e = adaptiveref.edges(3, 7)
    s = [np.asarray(a) for a in snaps]
    with np.errstate(all="ignore"):
        q = (s[0] * s[0]) / 3.0 + ((s[1] - s[0]) * (s[1] - s[0])) / 3.0 + ((s[2] - s[1]) * (s[2] - s[1])) / 1.0
        m2 = q - (s[2] * s[2]) / np.float64(e[3])
    assert np.sum(m2 < 0.0) >= 5


@pytest.mark.parametrize("threshold", [0.0, INF, 0.2])
def test_threshold_extremes(A, threshold):
    w, h, window, cap = 40, 24, 8, 64
    _, _, _, ts, _ = check_frame(A, w, h, window, cap, threshold)
    if threshold == 0.0:  # only a tile without variance converges
        assert sorted(set(ts.tolist())) == [16, 64] and ts[1] == 16 and ts[2] == 16
    if threshold == INF:  # every tile stops at the first evaluation, but for the NaN and inf tiles
        assert np.all(np.delete(ts, [3, 4]) == 16) and ts[3] == 64 and ts[4] == 64


@pytest.mark.parametrize("min_samples", [17, 24, 25, 64])
def test_min_samples_above_two_windows(A, min_samples):
    w, h, window, cap = 40, 24, 8, 64
    _, _, _, ts, _ = check_frame(A, w, h, window, cap, INF, min_samples=min_samples)
    first = min(e for e in adaptiveref.edges(window, cap)[2:] if e >= min_samples)
    assert np.all(np.delete(ts, [3, 4]) == first)


def test_floor(A):
    """The floor decides for a dark tile: with none a zero tile is 0 <= 0 still, and a dim noisy one runs longer."""
    w, h, window, cap = 40, 24, 8, 64
    _, _, _, ts_a, _ = check_frame(A, w, h, window, cap, 0.02, floor=0.0)
    _, _, _, ts_b, _ = check_frame(A, w, h, window, cap, 0.02, floor=100.0)
    assert np.all(ts_b <= ts_a) and np.any(ts_b < ts_a)


@pytest.mark.parametrize("w,h", [(20, 13), (17, 1), (1, 1)])
def test_small_shapes(A, w, h):
    for window, cap in PLANS:
        check_frame(A, w, h, window, cap, 0.02)


def test_optional_planes_may_be_null(A):
    w, h, window, cap = 20, 13, 3, 7
    snaps = adaptiveref.synthetic(w, h, window, cap)
    a = host_adaptive(A, snaps, w, h, window, cap, 0.02)
    b = host_adaptive(A, snaps, w, h, window, cap, 0.02, with_optional=False)
    same(b[0], a[0], "frame")
    assert np.array_equal(a[2], b[2]) and np.all(b[1] == -7.25) and np.all(b[3] == -7.25)


@pytest.mark.parametrize("world", [2, 3, 4])
def test_compact_shard_with_padding(A, world):
    """40x24 is 3x2 tiles, the lower row's with 8 of 16 rows in the frame: a rank's compact shard gives its tiles of
    the whole frame's result, and its padding elements are written as 0."""
    w, h, window, cap = 40, 24, 8, 20
    snaps = adaptiveref.synthetic(w, h, window, cap)
    rgb, var, ts, te = adaptiveref.adaptive(snaps, w, h, window, cap, 0.02)
    ins = adaptiveref.inside(w, h)
    for rank in range(world):
        ids = adaptiveref.rank_tiles(w, h, rank, world)
        shard = [adaptiveref.to_tiles(s, w, h)[ids] for s in snaps]
        out, v, s, e = host_adaptive(A, shard, w, h, window, cap, 0.02, rank=rank, world=world)
        assert np.array_equal(s, ts[ids])
        same(e, te[ids], "tile_error")
        same(out, adaptiveref.to_tiles(rgb, w, h)[ids], "shard")
        same(v, adaptiveref.to_tiles(var, w, h)[ids], "variance shard")
        pad = ~ins[ids]
        assert np.all(out.reshape(-1, 256, 3)[pad] == 0.0) and np.all(v.reshape(-1, 256, 3)[pad] == 0.0)
    assert sorted(np.concatenate([adaptiveref.rank_tiles(w, h, r, 3) for r in range(3)]).tolist()) == list(range(6))


def test_the_error_is_the_relative_standard_error():
    """Against the textbook form in plain numpy, within rounding: a full tile of independent pixels."""
    g = np.random.default_rng(5)
    n, window = 64, 8
    x = g.random((n, 1, 256, 3)) + 0.5
    sums = np.cumsum(x, axis=0)
    snaps = [sums[e - 1] for e in adaptiveref.edges(window, n)[1:]]
    _, var, ts, te = adaptiveref.adaptive_tiles(snaps, np.ones((1, 256), dtype=bool), window, n, 0.0)
    assert ts[0] == n
    means = x.reshape(8, 8, 256, 3).mean(axis=1)  # the eight batch means
    v = means.var(axis=0, ddof=1) / 8.0           # variance of the mean
    assert np.allclose(var[0], v, rtol=1e-9)
    lw = np.array(adaptiveref.L)
    rel = np.sqrt(np.mean(v @ (lw * lw))) / np.mean(x.mean(axis=0).reshape(256, 3) @ lw)
    assert np.isclose(np.sqrt(te[0]), rel, rtol=1e-9)


# ---- adaptive_runs ----

def test_runs_exhaustive(A):
    out = np.zeros(24, dtype=np.uint32)
    for n in range(0, 13):
        for mask in range(1 << n):
            active = np.array([(mask >> i) & 1 for i in range(n)], dtype=np.uint8)
            for gap in range(4):
                cnt = A.ad_runs(active.ctypes.data_as(C.POINTER(C.c_uint8)), n, gap, out.ctypes.data_as(u32p))
                runs = [(int(out[2 * i]), int(out[2 * i + 1])) for i in range(cnt)]
                assert runs == adaptiveref.runs(active, gap)
                covered = np.zeros(n, dtype=bool)
                end = None
                for b, c in runs:
                    assert c >= 1 and b + c <= n
                    assert active[b] and active[b + c - 1]            # starts and ends on an active tile
                    if end is not None:
                        assert b - end > gap                          # ascending, more than merge_gap apart
                    stopped = 0
                    for i in range(b, b + c):                         # no inner gap above merge_gap
                        stopped = 0 if active[i] else stopped + 1
                        assert stopped <= gap
                    covered[b:b + c] = True
                    end = b + c
                assert np.all(covered[active != 0])                   # every active tile is covered
                if gap == 0:
                    assert np.array_equal(covered, active != 0)


def test_runs_join_everything(A):
    active = np.zeros(1000, dtype=np.uint8)
    active[[3, 500, 998]] = 1
    out = np.zeros(2000, dtype=np.uint32)
    assert A.ad_runs(active.ctypes.data_as(C.POINTER(C.c_uint8)), 1000, 0xFFFFFFFF, out.ctypes.data_as(u32p)) == 1
    assert out[0] == 3 and out[1] == 996


# ---- the C-ABI: exports, signatures and argument errors (no HIP call is made) ----

NAMES = ("pt_adaptive_workspace_doubles", "pt_render_adaptive_device", "pt_render_adaptive")


def test_exports(pt):
    L = C.CDLL(str(pt.LIB_PATH))
    for name in NAMES:
        assert name in pt.EXPORTS and hasattr(L, name)
    assert pt.adaptive_workspace_doubles(40, 24) == 40 * 24 * 3 * 3
    assert pt.adaptive_workspace_doubles(40, 24, 1, 3) == 2 * 768 * 3  # 6 tiles over 3 ranks
    assert pt.adaptive_workspace_doubles(40, 24, 3, 4) == 768 * 3
    assert pt.adaptive_workspace_doubles(0, 24) == 0 and pt.adaptive_workspace_doubles(40, 0) == 0
    assert pt.adaptive_workspace_doubles(40, 24, 3, 3) == 0 and pt.adaptive_workspace_doubles(40, 24, 0, 0) == 0
    assert "0.4.3" in pt.version() and pt.lib().pt_abi_version() == 4
    header = (Path(__file__).resolve().parent.parent / "include" / "rs_pathtracing.h").read_text()
    for name in NAMES:
        assert name + "(" in header


def test_python_signatures(pt):
    p = inspect.signature(pt.HipRenderer.render_adaptive).parameters
    assert list(p)[:5] == ["self", "camera", "img_params", "max_samples", "threshold"]
    assert p["window"].default == 8 and p["min_samples"].default == 0 and p["luminance_floor"].default == 0.01
    assert p["merge_gap"].default == pt.ADAPTIVE_MERGE_GAP and p["seed"].default is None
    q = inspect.signature(pt.HipRenderer.render_adaptive_device).parameters
    for name in ("camera", "width", "height", "max_samples", "threshold", "seed", "rank", "world", "out_ptr",
                 "variance_ptr", "tile_samples_ptr", "tile_error_ptr", "work_ptr", "stream_ptr", "window",
                 "min_samples", "luminance_floor", "merge_gap"):
        assert name in q
    assert q["window"].default == 8 and q["stream_ptr"].default == 0
    assert list(inspect.signature(pt.adaptive_workspace_doubles).parameters) == ["width", "height", "rank", "world"]


BAD = {
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


@pytest.mark.parametrize("case", list(BAD))
def test_render_adaptive_argument_errors(pt, cornell_text, case):
    """The host form's checks come before its first use of the renderer and its first HIP call, so a stand-in
    renderer pointer is never dereferenced (no renderer can be made without a GPU; PT_ERR_STATE is tried there)."""
    L = pt.lib()
    sc = pt.Scene.from_json(cornell_text)
    w, h = 40, 24
    stand_in = np.zeros(4096, dtype=np.uint8)
    rgb, var = np.full((w * h, 3), -7.25), np.full((w * h, 3), -7.25)
    ts, te = np.full(6, 0xDEAD, dtype=np.uint32), np.full(6, -7.25)
    launched = C.c_uint64(77)
    a = dict(r=C.c_void_p(stand_in.ctypes.data), cam=C.byref(sc.camera()._c), w=w, h=h, window=8, min_samples=0, cap=64,
             threshold=0.1, floor=0.01, rgb=rgb.ctypes.data_as(d), ts=ts.ctypes.data_as(u32p))
    a.update(BAD[case])
    rc = L.pt_render_adaptive(a["r"], a["cam"], a["w"], a["h"], a["window"], a["min_samples"], a["cap"],
                              a["threshold"], a["floor"], 4, 1, a["rgb"], var.ctypes.data_as(d), a["ts"],
                              te.ctypes.data_as(d), C.byref(launched))
    assert rc == pt.PT_ERR_INVALID, (case, rc)
    assert L.pt_last_error()
    assert np.all(rgb == -7.25) and np.all(var == -7.25) and np.all(ts == 0xDEAD) and np.all(te == -7.25)
    assert launched.value == 77 and not stand_in.any()


def test_device_form_argument_errors(pt, cornell_text):
    L = pt.lib()
    sc = pt.Scene.from_json(cornell_text)
    cam = C.byref(sc.camera()._c)
    w, h = 40, 24
    buf = np.zeros(w * h * 3 * 5 + 2)
    base = buf.ctypes.data
    work = (base + w * h * 3 * 8 + 15) & ~15
    stand_in = np.zeros(4096, dtype=np.uint8)

    def dev(r=stand_in.ctypes.data, rank=0, world=1, out=base, ts=base, wk=work, cap=64, window=8):
        return L.pt_render_adaptive_device(r, cam, w, h, window, 0, cap, 0.1, 0.01, 4, 1, rank, world, out, None, ts,
                                           None, wk, None, None)

    for bad in (dict(r=None), dict(out=None), dict(ts=None), dict(wk=None), dict(rank=1), dict(world=0),
                dict(rank=6, world=7), dict(cap=8), dict(window=0)):
        assert dev(**bad) == pt.PT_ERR_INVALID, bad
        assert L.pt_last_error()
    assert dev(wk=work + 8) == pt.PT_ERR_INVALID and b"aligned" in L.pt_last_error()
    assert np.all(buf == 0.0) and not stand_in.any()
