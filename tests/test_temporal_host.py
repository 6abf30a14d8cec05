"""Temporal accumulation on the CPU: dev::temporal_pixel of rs-pathtracing_amd/csrc/pt_temporal.hpp (the function the
temporal_tiles kernel runs per lane), compiled for the host by tests/native/Makefile and run over every pixel,
against the numpy restatement tests/temporalref.py, bit for bit; the properties that need no reference; the relations
the accumulated frame must keep against a converged oracle frame; and pt_temporal's argument checks, which return
before any HIP call.  tests/test_gpu_temporal.py repeats the comparison with the same code compiled for gfx950."""
import ctypes as C
import inspect
import json
import subprocess
from pathlib import Path

import numpy as np
import pytest

import aovref
import temporalref as T
from conftest import ROOT, native_lib

NATIVE = Path(__file__).resolve().parent / "native"
GOLDEN = Path(__file__).resolve().parent / "golden"
INF = float("inf")
NAN = float("nan")
SENTINEL = -7.25
W, H = 40, 24


@pytest.fixture(scope="module")
def D():
    subprocess.run(["make", "-s", "-C", str(NATIVE), "_build/libtemporal.so"], check=True)
    L = C.CDLL(native_lib("libtemporal.so"))
    d = C.POINTER(C.c_double)
    L.tp_temporal.restype = C.c_size_t
    L.tp_temporal.argtypes = [d, d, d, d, d, C.c_uint32, C.c_uint32, d, d, C.c_uint32, C.c_double, C.c_double, d]
    return L


def host(D, rgb, normal, depth, w, h, cam, prev=None, history=None, in_place=False, **kw):
    """(out, history_out) of the host build; the frame equals the history's colour records."""
    kw = {**T.DEFAULTS, **kw}
    d = C.POINTER(C.c_double)
    arrs = [np.array(a, dtype=np.float64, order="C") for a in (rgb, normal, depth)]
    cv = T.caster_values(T.caster(w, h, cam), cam)
    pv = None if prev is None else T.caster_values(T.caster(w, h, prev), prev)
    hin = None if history is None else np.array(history, dtype=np.float64, order="C")
    out = arrs[0] if in_place else np.full((w * h, 3), SENTINEL)
    hout = np.full(w * h * 8, SENTINEL)
    used = D.tp_temporal(*[a.ctypes.data_as(d) for a in arrs], cv.ctypes.data_as(d),
                         None if pv is None else pv.ctypes.data_as(d), w, h,
                         None if hin is None else hin.ctypes.data_as(d), hout.ctypes.data_as(d), kw["max_count"],
                         kw["sigma_normal"], kw["sigma_depth"], out.ctypes.data_as(d))
    assert used == w * h * 8
    if hin is not None:
        assert np.array_equal(hin, history)  # the previous history is read only
    assert np.array_equal(out, hout.reshape(2, w * h, 4)[0][:, :3])
    return out.reshape(w * h, 3), hout


def same(got, ref):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and np.all(np.isfinite(got))
    bad = np.flatnonzero(got.reshape(-1) != ref.reshape(-1))
    assert bad.size == 0, "%d of %d values differ (first %s)" % (bad.size, ref.size, bad[:8].tolist())


def kinds(info):
    return {int(k): int(np.sum(info["stage"] == k)) for k in np.unique(info["stage"])}


# ---- bit for bit against the numpy restatement, on seeded planes and histories ----

SETTINGS = {
    "defaults": {},
    "max_count_1": dict(max_count=1),
    "max_count_3": dict(max_count=3),
    "sigma_inf": dict(sigma_normal=INF, sigma_depth=INF),
}
CASES = [(camera, setting) for camera in T.SYN_CAMERAS for setting in SETTINGS]


def check_not_degenerate(camera, setting, info, rgb, out):
    """What each case is there for is really in it."""
    k = kinds(info)
    assert k.get(T.NO_HIT, 0) >= 50  # the plane's misses
    if camera == "behind":
        assert k.get(T.BEHIND, 0) >= 500 and T.BLENDED not in k
        return
    assert k.get(T.BLENDED, 0) >= 100
    # max_count 1 blends with a = 1: hk + (c - hk) is the new frame up to that sum's rounding
    if setting == "max_count_1":
        assert np.allclose(out, rgb, rtol=0.0, atol=4 * 2.0 ** -52)
    else:
        assert np.sum(np.any(np.abs(out - rgb) > 1e-3, axis=1)) >= 100
    if camera == "same":
        assert np.sum(info["snapped"]) >= 500 and np.all(info["taps"] <= 1)
    else:
        assert np.sum(info["taps"] >= 2) >= 20 and k.get(T.OUTSIDE, 0) >= 20
    if camera == "rotated_30":
        assert k[T.OUTSIDE] >= 400  # most of the new frame was never seen
    if setting == "sigma_inf":
        if camera != "rotated_30":
            assert np.sum(info["taps"] == 4) >= 100 or camera == "same"
    else:
        assert k.get(T.NO_TAP, 0) >= 50  # the guide tests reject
    if setting == "max_count_1":
        assert np.array_equal(info["clamped"], info["stage"] == T.BLENDED)
    else:
        assert np.sum(info["clamped"]) >= 10


@pytest.mark.parametrize("camera,setting", CASES)
def test_seeded_planes_equal_the_restatement(D, camera, setting):
    rgb, normal, depth, history = T.synthetic(W, H)
    # the planes hold what they are for: misses, coverage strictly between 0 and 1, a history with zero counts,
    # counts above max_count, and history pixels without a hit
    assert np.sum(depth[:, 1] == 0.0) >= 50 and np.sum((depth[:, 1] > 0.0) & (depth[:, 1] < 1.0)) >= 50
    hn, hz = T.counts_of(history), history.reshape(2, -1, 4)[1][:, 3]
    assert np.sum(hn == 0.0) >= 20 and np.sum(hn > 32.0) >= 50 and np.sum(hz == 0.0) >= 50
    cam, prev, kw = T.syn_camera("same"), T.syn_camera(camera), SETTINGS[setting]
    ref_out, ref_hist, info = T.temporal(rgb, normal, depth, W, H, cam, prev, history, **kw)
    check_not_degenerate(camera, setting, info, rgb, ref_out)
    out, hist = host(D, rgb, normal, depth, W, H, cam, prev, history, **kw)
    same(out, ref_out)
    same(hist, ref_hist)


def test_the_cases_cover_every_way_out():
    """The case set as a whole: a reset at step 1, at step 3 (both causes) and at step 5, a pixel reused through
    four taps, a snapped pixel and a pixel clamped at max_count."""
    rgb, normal, depth, history = T.synthetic(W, H)
    seen, four, snapped, clamped = set(), 0, 0, 0
    for camera, setting in CASES:
        _, _, info = T.temporal(rgb, normal, depth, W, H, T.syn_camera("same"), T.syn_camera(camera), history,
                                **SETTINGS[setting])
        seen |= set(kinds(info))
        four += int(np.sum((info["taps"] == 4) & (info["stage"] == T.BLENDED)))
        snapped += int(np.sum(info["snapped"] & (info["stage"] == T.BLENDED)))
        clamped += int(np.sum(info["clamped"]))
    assert seen >= {T.BLENDED, T.NO_HIT, T.BEHIND, T.OUTSIDE, T.NO_TAP}
    assert four >= 100 and snapped >= 100 and clamped >= 100


def small_case(cw, ch):
    full = T.synthetic(W, H)
    if (cw, ch) != (1, 1):
        return T.crop(full, W, H, cw, ch)
    # one pixel: the first one a still camera reuses (that depends on the pixel's own values alone)
    _, _, info = T.temporal(*full[:3], W, H, T.syn_camera("same"), T.syn_camera("same"), full[3])
    p = int(np.flatnonzero(info["stage"] == T.BLENDED)[0])
    return (*[a[p:p + 1].copy() for a in full[:3]], full[3].reshape(2, -1, 4)[:, p].reshape(-1).copy())


@pytest.mark.parametrize("cw,ch", [(20, 13), (17, 1), (1, 1)])
@pytest.mark.parametrize("camera", ["same", "rotated_2"])
def test_small_shapes(D, cw, ch, camera):
    rgb, normal, depth, history = small_case(cw, ch)
    cam, prev = T.syn_camera("same"), T.syn_camera(camera)
    ref_out, ref_hist, info = T.temporal(rgb, normal, depth, cw, ch, cam, prev, history)
    k = kinds(info)
    if camera == "same":
        assert k.get(T.BLENDED, 0) >= 1 and np.any(ref_out != rgb)
    else:
        # two degrees are 2 / 40 of the frame's width: sub-pixel at 1x1 and 17x1, two pixels at 20x13
        assert k.get(T.BLENDED, 0) >= (10 if cw > 17 else 1)
        assert np.any(info["taps"] >= 2) or cw == 1
    out, hist = host(D, rgb, normal, depth, cw, ch, cam, prev, history)
    same(out, ref_out)
    same(hist, ref_hist)


def test_first_frame(D):
    """Every pixel resets, the previous history is not read (a null pointer), and the guide records hold the
    normals and the mean hit distance."""
    rgb, normal, depth, _ = T.synthetic(W, H)
    cam = T.syn_camera("same")
    ref_out, ref_hist, info = T.temporal(rgb, normal, depth, W, H, cam)
    assert set(kinds(info)) == {T.FIRST, T.NO_HIT}
    out, hist = host(D, rgb, normal, depth, W, H, cam)
    same(out, ref_out)
    same(hist, ref_hist)
    assert np.array_equal(out, rgb) and np.all(T.counts_of(hist) == 1.0)
    g = hist.reshape(2, -1, 4)[1]
    hit = depth[:, 1] > 0.0
    assert np.array_equal(g[:, :3], normal)
    assert np.array_equal(g[hit, 3], depth[hit, 0] / depth[hit, 1]) and np.all(g[~hit, 3] == 0.0)
    part = (depth[:, 1] > 0.0) & (depth[:, 1] < 1.0)
    assert np.all(g[part, 3] > depth[part, 0])  # the mean over the hitting samples, not over all


def test_a_history_of_zero_counts_is_not_reused(D):
    rgb, normal, depth, history = T.synthetic(W, H)
    empty = history.reshape(2, -1, 4).copy()
    empty[0][:, 3] = 0.0
    cam = T.syn_camera("same")
    out, hist = host(D, rgb, normal, depth, W, H, cam, T.syn_camera("sideways"), empty.reshape(-1))
    same(hist, T.temporal(rgb, normal, depth, W, H, cam, T.syn_camera("sideways"), empty.reshape(-1))[1])
    assert np.array_equal(out, rgb) and np.all(T.counts_of(hist) == 1.0)


# ---- properties without the reference ----

def test_a_still_camera_gives_the_running_mean_of_the_pixel_alone(D):
    """The same camera, both sigmas +inf: frame k of a hitting pixel is h + (c - h) * (1 / k), h the frame before,
    with nothing of its neighbours (the position snaps onto the pixel, one tap of weight 1, acc = 0 + 1 * h,
    ws = 1, hn = n)."""
    _, normal, depth, _ = T.synthetic(W, H)
    cam = T.syn_camera("same")
    hit = depth[:, 1] > 0.0
    assert 500 <= np.sum(hit) < W * H
    g = np.random.default_rng(5)
    hist, expect = None, None
    for k in range(1, 7):
        c = g.random((W * H, 3)) * 3.0
        prev = None if k == 1 else cam
        ref = T.temporal(c, normal, depth, W, H, cam, prev, hist, sigma_normal=INF, sigma_depth=INF)
        out, hist = host(D, c, normal, depth, W, H, cam, prev, hist, sigma_normal=INF, sigma_depth=INF)
        same(out, ref[0])
        same(hist, ref[1])
        expect = c if k == 1 else np.where(hit[:, None], expect + (c - expect) * (1.0 / np.float64(k)), c)
        assert np.array_equal(out, expect)
        assert np.array_equal(T.counts_of(hist), np.where(hit, float(k), 1.0))
    # the mean it converges to, up to the blends' rounding
    assert np.allclose(out[hit].mean(), 1.5, atol=0.05)


def test_in_place(D):
    rgb, normal, depth, history = T.synthetic(W, H)
    cam, prev = T.syn_camera("same"), T.syn_camera("sideways")
    out, hist = host(D, rgb, normal, depth, W, H, cam, prev, history, in_place=True)
    ref = T.temporal(rgb, normal, depth, W, H, cam, prev, history)
    same(out, ref[0])
    same(hist, ref[1])


# ---- quality on the oracle's frames, as relations ----

def cornell_errors(moving):
    _, _, w, h, _, _, _ = aovref.case("cornell")
    ref = np.load(GOLDEN / "denoise_cornell_ref.npy")
    assert ref.shape == (w * h, 3)
    seq = T.cornell_sequence(moving)
    assert len(seq) == 8
    out, hist, infos = T.accumulate(seq, w, h)
    single, acc = T.rms(seq[-1][1], ref), T.rms(out, ref)
    n = T.counts_of(hist)
    print("cornell %s: single frame %.4f, accumulated %.4f (%.4fx), pixels with n > 1: %.4f, mean n %.2f, reset per "
          "frame %s" % ("orbit" if moving else "still", single, acc, acc / single, np.mean(n > 1.0), n.mean(),
                        ["%.3f" % np.mean(i["stage"] != T.BLENDED) for i in infos[1:]]))
    return single, acc, n, seq


def test_cornell_still_camera_quality():
    """cornell 96x54, depth 8, 1 spp, 8 frames with different frame seeds at the scene's camera, against the
    converged frame tests/golden/denoise_cornell_ref.npy: the accumulated frame is nearer to it than the last
    frame alone, and at least half of its pixels stand for more than one frame."""
    single, acc, n, seq = cornell_errors(False)
    assert acc < single
    assert np.mean(n > 1.0) >= 0.5
    assert n.max() == 8.0


def test_cornell_orbit_quality():
    """The same with a camera that orbits 1 degree per frame about the vertical axis through the point it looks at
    and ends on the scene's own camera (the one the converged frame was rendered at)."""
    single, acc, n, seq = cornell_errors(True)
    cams = [np.array(c.position[:]) for c, _, _ in seq]
    assert all(np.any(a != b) for a, b in zip(cams, cams[1:]))  # it did move, every frame
    assert np.array_equal(cams[-1], np.array(aovref.case("cornell")[5].camera().position[:]))
    assert acc < single
    assert np.mean(n > 1.0) >= 0.5


def test_cornell_quality_of_the_host_build(D):
    """The orbit through the product's own code (the host build), bit for bit the restatement's frames."""
    _, _, w, h, _, _, _ = aovref.case("cornell")
    hist, prev = None, None
    for cam, img, pl in T.cornell_sequence(True):
        ref = T.temporal(img, pl["normal"], pl["depth"], w, h, cam, prev, hist)
        out, hist = host(D, img, pl["normal"], pl["depth"], w, h, cam, prev, hist)
        same(out, ref[0])
        same(hist, ref[1])
        prev = cam
    assert T.counts_of(hist).max() > 4.0


# ---- the C-ABI: exports, signatures and argument errors (no HIP call is made) ----

def test_exports_and_signatures(pt):
    L = C.CDLL(str(pt.LIB_PATH))
    for name in ("pt_temporal_history_doubles", "pt_temporal_device", "pt_temporal"):
        assert name in pt.EXPORTS and hasattr(L, name)
    assert pt.temporal_history_doubles(0, 7) == 0 and pt.temporal_history_doubles(7, 0) == 0
    assert pt.temporal_history_doubles(40, 24) == 40 * 24 * 8
    assert (pt.TEMPORAL_MAX_COUNT, pt.TEMPORAL_SIGMA_NORMAL, pt.TEMPORAL_SIGMA_DEPTH) == (32, 0.5, 0.1)
    assert "0.4.3" in pt.version() and pt.lib().pt_abi_version() == 4
    dev = list(inspect.signature(pt.temporal_device).parameters)
    assert dev == ["rgb_ptr", "normal_ptr", "depth_ptr", "camera", "prev_camera", "width", "height", "history_in_ptr",
                   "history_out_ptr", "out_ptr", "max_count", "sigma_normal", "sigma_depth", "stream_ptr", "device"]
    hst = inspect.signature(pt.temporal).parameters
    assert list(hst) == ["rgb", "normal", "depth", "camera", "prev_camera", "width", "height", "history_in",
                         "max_count", "sigma_normal", "sigma_depth", "device"]
    assert hst["max_count"].default == 32 and hst["sigma_normal"].default == 0.5 and hst["sigma_depth"].default == 0.1


def test_the_source_id_is_the_render_paths(pt):
    """The pass is no part of the render path's identity: the build's id is still the one the newest committed
    measurement of the render path names (profiles/r14/adaptive_list.txt)."""
    rec = json.loads((ROOT / "profiles" / "r14" / "adaptive_list.txt").read_text().splitlines()[0])
    assert "src %s)" % pt.source_id() in rec["version"]


BAD = {
    "null_rgb": dict(rgb=None),
    "null_normal": dict(normal=None),
    "null_depth": dict(depth=None),
    "null_camera": dict(camera=None),
    "null_history_out": dict(hout=None),
    "null_out": dict(out=None),
    "zero_width": dict(w=0),
    "zero_height": dict(h=0),
    "max_count_zero": dict(max_count=0),
    "sigma_normal_zero": dict(sn=0.0),
    "sigma_normal_negative": dict(sn=-0.5),
    "sigma_normal_nan": dict(sn=NAN),
    "sigma_depth_zero": dict(sd=0.0),
    "sigma_depth_nan": dict(sd=NAN),
    "history_without_camera": dict(prev=None),
    "camera_without_history": dict(hin=None),
    "histories_overlap": dict(overlap=8),
    "histories_equal": dict(overlap=0),
    "too_many_tiles": dict(w=1 << 20, h=1 << 20),  # 2^32 tiles of 16x16
    "history_does_not_fit": dict(w=0xffffffff, h=0xffffffff),
}


# two bad arguments at once: the order of the checks decides which message wins
BAD.update({
    "null_rgb_and_zero_width": dict(rgb=None, w=0),
    "zero_height_and_max_count_zero": dict(h=0, max_count=0),
    "max_count_zero_and_sigma_normal_zero": dict(max_count=0, sn=0.0),
    "sigma_depth_nan_and_history_without_camera": dict(sd=NAN, prev=None),
    "camera_without_history_and_too_many_tiles": dict(hin=None, w=1 << 20, h=1 << 20),
})


# pt_last_error() of each case, recorded from the build before the checks were given one spelling each
MESSAGES = {'null_rgb': b'null argument',
 'null_normal': b'null argument',
 'null_depth': b'null argument',
 'null_camera': b'null argument',
 'null_history_out': b'null argument',
 'null_out': b'null argument',
 'zero_width': b'width and height must be > 0',
 'zero_height': b'width and height must be > 0',
 'max_count_zero': b'max_count must be > 0',
 'sigma_normal_zero': b'sigma_normal and sigma_depth must be > 0',
 'sigma_normal_negative': b'sigma_normal and sigma_depth must be > 0',
 'sigma_normal_nan': b'sigma_normal and sigma_depth must be > 0',
 'sigma_depth_zero': b'sigma_normal and sigma_depth must be > 0',
 'sigma_depth_nan': b'sigma_normal and sigma_depth must be > 0',
 'history_without_camera': b'prev_camera and history_in are given together, or neither (the first frame)',
 'camera_without_history': b'prev_camera and history_in are given together, or neither (the first frame)',
 'histories_overlap': b'history_in and history_out overlap',
 'histories_equal': b'history_in and history_out overlap',
 'too_many_tiles': b'the frame is too large to accumulate in one call',
 'history_does_not_fit': b'the frame is too large to accumulate in one call',
 'null_rgb_and_zero_width': b'null argument',
 'zero_height_and_max_count_zero': b'width and height must be > 0',
 'max_count_zero_and_sigma_normal_zero': b'max_count must be > 0',
 'sigma_depth_nan_and_history_without_camera': b'sigma_normal and sigma_depth must be > 0',
 'camera_without_history_and_too_many_tiles': b'prev_camera and history_in are given together, or neither (the first'
                                              b' frame)'}
MESSAGES_DEVICE = {'misaligned_out_history': b'the histories must be 16-byte aligned',
 'misaligned_in_history': b'the histories must be 16-byte aligned',
 'first_frame_misaligned': b'the histories must be 16-byte aligned',
 'overlap': b'history_in and history_out overlap',
 'null_out_history': b'null argument',
 'null_in_history': b'prev_camera and history_in are given together, or neither (the first frame)',
 'history_without_camera': b'prev_camera and history_in are given together, or neither (the first frame)',
 'max_count_zero': b'max_count must be > 0',
 'sigma_normal_nan': b'sigma_normal and sigma_depth must be > 0',
 'misaligned_and_max_count_zero': b'max_count must be > 0',
 'misaligned_and_overlap': b'history_in and history_out overlap',
 'null_out_history_and_sigma_normal_nan': b'null argument'}


def host_refusal(pt, bad):
    """pt_temporal with the arguments of `bad` replaced: (status, message, the out buffer, the histories)."""
    w, h = 8, 4
    d = C.POINTER(C.c_double)
    cam = pt.Camera.new((0, 0, 0), (0, 0, 1), (0, 1, 0), 1.0, 0.7)
    hist = np.full(w * h * 8 * 2 + 16, SENTINEL)
    a = dict(rgb=np.ones((w * h, 3)), normal=np.zeros((w * h, 3)), depth=np.ones((w * h, 3)),
             out=np.full((w * h, 3), SENTINEL), hin=hist[:w * h * 8], hout=hist[w * h * 8:w * h * 16], camera=cam,
             prev=cam, w=w, h=h, max_count=32, sn=0.5, sd=0.1)
    out = a["out"]
    a.update(bad)
    if "overlap" in a:
        a["hout"] = hist[a["overlap"]:a["overlap"] + w * h * 8]
    ptr = {k: None if a[k] is None else a[k].ctypes.data_as(d) for k in ("rgb", "normal", "depth", "out", "hin", "hout")}
    cams = {k: None if a[k] is None else C.byref(a[k]._c) for k in ("camera", "prev")}
    rc = pt.lib().pt_temporal(-1, ptr["rgb"], ptr["normal"], ptr["depth"], cams["camera"], cams["prev"], a["w"],
                              a["h"], ptr["hin"], ptr["hout"], a["max_count"], a["sn"], a["sd"], ptr["out"])
    return rc, pt.lib().pt_last_error(), out, hist


@pytest.mark.parametrize("case", list(BAD))
def test_argument_errors(pt, case):
    rc, message, out, hist = host_refusal(pt, BAD[case])
    assert rc == pt.PT_ERR_INVALID, (case, rc)
    assert message == MESSAGES[case]  # the text, as recorded before the checks were given one spelling each
    assert np.all(out == SENTINEL) and np.all(hist == SENTINEL)  # a refused call writes nothing


# the device form: (hin, hout) as offsets in bytes from two aligned, well separated histories, None for a null pointer
BAD_DEVICE = {
    "misaligned_out_history": dict(hout=8),
    "misaligned_in_history": dict(hin=8),
    "first_frame_misaligned": dict(hin=None, hout=8, prev=None),
    "overlap": dict(hout="hin+16"),
    "null_out_history": dict(hout=None),
    "null_in_history": dict(hin=None),
    "history_without_camera": dict(prev=None),
    "max_count_zero": dict(max_count=0),
    "sigma_normal_nan": dict(sn=NAN),
    "misaligned_and_max_count_zero": dict(hout=8, max_count=0),  # two at once: the shared checks come first
    "misaligned_and_overlap": dict(hin=8, hout="hin+16"),
    "null_out_history_and_sigma_normal_nan": dict(hout=None, sn=NAN),
}


def device_refusal(pt, bad):
    """pt_temporal_device likewise; the pointers are never dereferenced on the host.  (status, message, the buffer)"""
    w, h = 8, 4
    buf = np.zeros(w * h * 3 + w * h * 16 + 12)
    base = buf.ctypes.data
    hin = (base + w * h * 24 + 15) & ~15
    hout = hin + w * h * 64 + 32  # a gap, so that a pointer moved by 8 bytes does not overlap
    cam = pt.Camera.new((0, 0, 0), (0, 0, 1), (0, 1, 0), 1.0, 0.7)
    a = dict(hin=0, hout=0, prev=cam, max_count=32, sn=0.5)
    a.update(bad)
    p_in = None if a["hin"] is None else hin + a["hin"]
    p_out = None if a["hout"] is None else (p_in + 16 if a["hout"] == "hin+16" else hout + a["hout"])
    L = pt.lib()
    rc = L.pt_temporal_device(-1, base, base, base, C.byref(cam._c), None if a["prev"] is None else C.byref(a["prev"]._c),
                              w, h, p_in, p_out, a["max_count"], a["sn"], 0.1, base, None)
    return rc, L.pt_last_error(), buf


def test_device_form_argument_errors(pt):
    """The device form's checks come before its first HIP call too: the shared ones and a misaligned history."""
    for case, bad in BAD_DEVICE.items():
        rc, message, buf = device_refusal(pt, bad)
        assert rc == pt.PT_ERR_INVALID, (case, rc)
        assert message == MESSAGES_DEVICE[case], case
        assert np.all(buf == 0.0)
    w, h = 8, 4
    buf = np.zeros(w * h * 3 + w * h * 16 + 12)
    base = buf.ctypes.data
    hin = (base + w * h * 24 + 15) & ~15
    hout = hin + w * h * 64 + 32
    cam = pt.Camera.new((0, 0, 0), (0, 0, 1), (0, 1, 0), 1.0, 0.7)
    with pytest.raises(pt.PtError) as e:
        pt.temporal_device(base, base, base, cam, cam, w, h, hin, hout + 8, base)
    assert e.value.code == pt.PT_ERR_INVALID
    with pytest.raises(pt.PtError):
        pt.temporal(np.ones((w * h, 3)), np.ones((w * h, 3)), np.ones((w * h, 3)), cam, None, w, h,
                    history_in=np.ones(w * h * 8))
    assert np.all(buf == 0.0)
