"""Temporal accumulation on the MI355X (temporal_tiles, rs-pathtracing_amd/csrc/pt_temporal.hip) through the Python
mirror: frames and planes that never leave the device, at three cameras, against the numpy restatement
tests/temporalref.py bit for bit; the host test's seeded planes and small shapes; in place; a stream of the
caller's; the host form; argument errors; and that the pass leaves a renderer as it found it.  Every device call
here runs with sentinels before and after the frame, after the new history and around the previous one, and the
previous history must come back unchanged."""
import ctypes as C

import numpy as np
import pytest

import aovref
import temporalref as T

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
GUARD = 64  # doubles of sentinel on each side (512 bytes: the records behind it stay 16-byte aligned)
INF = float("inf")


def same(got, ref):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and np.all(np.isfinite(got))
    bad = np.flatnonzero(got.reshape(-1) != ref.reshape(-1))
    assert bad.size == 0, "%d of %d values differ (first %s)" % (bad.size, ref.size, bad[:8].tolist())


def on_device(arr):
    import torch
    return torch.from_numpy(np.array(arr, dtype=np.float64, order="C").reshape(-1)).cuda()


def pt_camera(pt, c):
    """The product's camera with the fields of an oracle camera."""
    s = pt.CameraStruct()
    for name in ("position", "direction", "up", "right"):
        getattr(s, name)[:] = getattr(c, name)[:]
    s.fov, s.focal_length = c.fov, c.focal_length
    return pt.Camera(s)


class Buffers:
    """[guard | frame | guard], [new history | guard] and [guard | previous history | guard] on the device, the
    guards, the frame and the new history filled with the sentinel."""

    def __init__(self, pt, w, h, history=None):
        import torch
        self.n, self.hn = w * h * 3, pt.temporal_history_doubles(w, h)
        assert self.hn == w * h * 8
        self.out = torch.full((self.n + 2 * GUARD,), SENTINEL, dtype=torch.float64, device="cuda")
        self.hout = torch.full((self.hn + GUARD,), SENTINEL, dtype=torch.float64, device="cuda")
        self.hin, self.hin_host = None, None
        if history is not None:
            self.hin_host = np.array(history, dtype=np.float64).reshape(-1)
            assert self.hin_host.size == self.hn
            self.hin = torch.full((self.hn + 2 * GUARD,), SENTINEL, dtype=torch.float64, device="cuda")
            self.hin[GUARD:GUARD + self.hn] = on_device(self.hin_host)
        assert self.hout.data_ptr() % 16 == 0 and self.hin_ptr % 16 == 0

    out_ptr = property(lambda s: s.out.data_ptr() + GUARD * 8)
    hout_ptr = property(lambda s: s.hout.data_ptr())
    hin_ptr = property(lambda s: 0 if s.hin is None else s.hin.data_ptr() + GUARD * 8)

    def results(self):
        """(frame, new history) on the host, every sentinel and the previous history checked."""
        import torch
        torch.cuda.synchronize()
        out, hout = self.out.cpu().numpy(), self.hout.cpu().numpy()
        assert np.all(out[:GUARD] == SENTINEL) and np.all(out[-GUARD:] == SENTINEL), "wrote beside the frame"
        assert np.all(hout[self.hn:] == SENTINEL), "wrote past the new history"
        if self.hin is not None:
            hin = self.hin.cpu().numpy()
            assert np.all(hin[:GUARD] == SENTINEL) and np.all(hin[-GUARD:] == SENTINEL), "wrote beside the history"
            assert np.array_equal(hin[GUARD:-GUARD], self.hin_host), "the previous history changed"
        frame, hist = out[GUARD:-GUARD].reshape(-1, 3).copy(), hout[:self.hn].copy()
        assert np.array_equal(frame, hist.reshape(2, -1, 4)[0][:, :3])  # d_out is the colour records' colour
        return frame, hist


def device_temporal(pt, rgb, normal, depth, w, h, cam, prev=None, history=None, stream_ptr=0, **kw):
    """pt.temporal_device on host planes uploaded here (cam, prev: oracle cameras); (frame, history) back on the
    host."""
    dev = [on_device(a) for a in (rgb, normal, depth)]
    b = Buffers(pt, w, h, history)
    pt.temporal_device(*[t.data_ptr() for t in dev], pt_camera(pt, cam), None if prev is None else pt_camera(pt, prev),
                       w, h, b.hin_ptr, b.hout_ptr, b.out_ptr, stream_ptr=stream_ptr, **kw)
    got = b.results()
    for t, a in zip(dev, (rgb, normal, depth)):
        assert np.array_equal(t.cpu().numpy(), np.asarray(a).reshape(-1))  # the inputs are read only
    return got


# ---- frames that never leave the device ----

ORBIT = (2.0, 1.0, 0.0)  # degrees: two small orbits, then the scene's own camera
SPP = 2


@pytest.mark.parametrize("name", ["cornell", "spheres", "marched"])
def test_frames_on_the_device_equal_the_restatement(pt, name):
    """Three frames at three cameras, rendered by render_device and render_aov_device and accumulated with ping-pong
    histories without leaving the device.  After every frame the result equals the restatement on the GPU's own
    downloaded inputs; for cornell and spheres it equals the restatement's own chain on the oracle's frames and
    planes too.  (cornell: 54 rows, the last tile row is padded.)"""
    import torch
    text, rs, w, h, _, osc, _ = aovref.case(name)
    ps = pt.Scene.from_json(text, random_spheres=rs, seed=1)
    r = pt.HipRenderer(ps, depth=8)
    st = torch.cuda.current_stream().cuda_stream
    rgb, normal, depth = (torch.zeros(w * h * 3, dtype=torch.float64, device="cuda") for _ in range(3))
    prev, prev_hist, oracle_hist, reused = None, None, None, 0
    for i, deg in enumerate(ORBIT):
        cam = T.orbit_camera(osc, deg)
        pcam = pt_camera(pt, cam)
        if deg == 0.0:
            assert bytes(pcam._c) == bytes(ps.camera()._c)  # the scene's own camera, the same bits
        seed = 40 + i
        r.render_device(pcam, w, h, SPP, seed, 0, 1, rgb.data_ptr(), st)
        r.render_aov_device(pcam, w, h, SPP, seed, 0, 1, 0, normal.data_ptr(), depth.data_ptr(), st)
        b = Buffers(pt, w, h, prev_hist)
        pt.temporal_device(rgb.data_ptr(), normal.data_ptr(), depth.data_ptr(), pcam,
                           None if prev is None else pt_camera(pt, prev), w, h, b.hin_ptr, b.hout_ptr, b.out_ptr,
                           stream_ptr=st)
        out, hist = b.results()
        own = [t.cpu().numpy().reshape(-1, 3) for t in (rgb, normal, depth)]
        ref_out, ref_hist, info = T.temporal(*own, w, h, cam, prev, prev_hist)
        same(out, ref_out)
        same(hist, ref_hist)
        if i:
            reused += int(np.sum(info["stage"] == T.BLENDED))
            assert np.sum(info["taps"] >= 2) >= 100  # the camera moved: bilinear taps, not the pixel alone
        if name != "marched":
            img = osc.render(w, h, SPP, 8, seed, camera=cam)
            pl = T.planes_at(osc, w, h, SPP, seed, cam)
            o_out, oracle_hist, _ = T.temporal(img, pl["normal"], pl["depth"], w, h, cam, prev, oracle_hist)
            same(out, o_out)
            same(hist, oracle_hist)
        prev, prev_hist = cam, hist
    assert reused >= w * h // 2 and T.counts_of(prev_hist).max() == 3.0


# ---- the host test's seeded planes, on the device ----

SETTINGS = {"defaults": {}, "max_count_1": dict(max_count=1), "max_count_3": dict(max_count=3),
            "sigma_inf": dict(sigma_normal=INF, sigma_depth=INF)}


@pytest.mark.parametrize("camera", list(T.SYN_CAMERAS))
def test_seeded_planes(pt, camera):
    w, h = 40, 24
    rgb, normal, depth, history = T.synthetic(w, h)
    cam, prev = T.syn_camera("same"), T.syn_camera(camera)
    for setting in (SETTINGS if camera in ("sideways", "rotated_30") else ("defaults", "sigma_inf")):
        kw = SETTINGS[setting]
        ref_out, ref_hist, info = T.temporal(rgb, normal, depth, w, h, cam, prev, history, **kw)
        assert len(np.unique(info["stage"])) >= 2
        out, hist = device_temporal(pt, rgb, normal, depth, w, h, cam, prev, history, **kw)
        same(out, ref_out)
        same(hist, ref_hist)


def test_first_frame_does_not_read_a_history(pt):
    w, h = 40, 24
    rgb, normal, depth, _ = T.synthetic(w, h)
    cam = T.syn_camera("same")
    out, hist = device_temporal(pt, rgb, normal, depth, w, h, cam)
    ref = T.temporal(rgb, normal, depth, w, h, cam)
    same(out, ref[0])
    same(hist, ref[1])
    assert np.array_equal(out, rgb) and np.all(T.counts_of(hist) == 1.0)


@pytest.mark.parametrize("cw,ch", [(20, 13), (17, 1), (1, 1)])
def test_small_shapes(pt, cw, ch):
    rgb, normal, depth, history = T.crop(T.synthetic(40, 24), 40, 24, cw, ch)
    cam = T.syn_camera("same")
    for camera in ("same", "rotated_2"):
        prev = T.syn_camera(camera)
        ref = T.temporal(rgb, normal, depth, cw, ch, cam, prev, history)
        out, hist = device_temporal(pt, rgb, normal, depth, cw, ch, cam, prev, history)
        same(out, ref[0])
        same(hist, ref[1])
    first = device_temporal(pt, rgb, normal, depth, cw, ch, cam)
    same(first[1], T.temporal(rgb, normal, depth, cw, ch, cam)[1])


def test_in_place_on_a_stream_of_the_callers(pt):
    """d_out == d_rgb, queued on a non-null stream after the uploads."""
    import torch
    w, h = 40, 24
    rgb, normal, depth, history = T.synthetic(w, h)
    cam, prev = T.syn_camera("same"), T.syn_camera("sideways")
    ref = T.temporal(rgb, normal, depth, w, h, cam, prev, history)
    s = torch.cuda.Stream()
    b = Buffers(pt, w, h, history)
    s.wait_stream(torch.cuda.current_stream())  # the sentinel fills and the history's upload
    with torch.cuda.stream(s):
        dev = [on_device(a) for a in (normal, depth)]
        b.out[GUARD:GUARD + b.n] = on_device(rgb)
        pt.temporal_device(b.out_ptr, dev[0].data_ptr(), dev[1].data_ptr(), pt_camera(pt, cam), pt_camera(pt, prev), w,
                           h, b.hin_ptr, b.hout_ptr, b.out_ptr, stream_ptr=s.cuda_stream)
    s.synchronize()
    out, hist = b.results()
    same(out, ref[0])
    same(hist, ref[1])
    assert np.any(out != rgb)


def test_host_form_equals_the_device_form(pt):
    w, h = 40, 24
    rgb, normal, depth, history = T.synthetic(w, h)
    cam, prev = T.syn_camera("same"), T.syn_camera("rotated_2")
    for kw in ({}, dict(max_count=3, sigma_depth=INF)):
        out, hist = pt.temporal(rgb, normal, depth, pt_camera(pt, cam), pt_camera(pt, prev), w, h, history, **kw)
        assert out.shape == (w * h, 3) and hist.shape == (w * h * 8,)
        dev = device_temporal(pt, rgb, normal, depth, w, h, cam, prev, history, **kw)
        same(out, dev[0])
        same(hist, dev[1])
    out, hist = pt.temporal(rgb, normal, depth, pt_camera(pt, cam), None, w, h)
    ref = T.temporal(rgb, normal, depth, w, h, cam)
    same(out, ref[0])
    same(hist, ref[1])


def test_the_pass_leaves_the_renderer_alone(pt):
    import torch
    text, rs, w, h, _, _, _ = aovref.case("cornell")
    ps = pt.Scene.from_json(text, random_spheres=rs, seed=1)
    r = pt.HipRenderer(ps, depth=8)
    cam, ip = ps.camera(), pt.ImageParams(w, h)
    first = r.render(cam, ip, 8, seed=11)
    opts, builds = r.options(), r.last_builds()
    planes = r.render_aov(cam, ip, 8, seed=11)
    builds_after_planes = r.last_builds()
    ocam = T.camera_like(cam)
    device_temporal(pt, first, planes["normal"], planes["depth"], w, h, ocam)
    assert r.last_builds() == builds_after_planes
    again = r.render(cam, ip, 8, seed=11)
    assert np.array_equal(first, again) and first.mean() > 0.01
    assert r.options() == opts and r.last_builds() == builds
    assert pt.march_guard_drops(r) == 0
    torch.cuda.synchronize()


def test_argument_errors_write_nothing(pt):
    import torch
    w, h = 40, 24
    rgb, normal, depth, history = T.synthetic(w, h)
    fr = [on_device(a) for a in (rgb, normal, depth)]
    before = [t.clone() for t in fr]
    b = Buffers(pt, w, h, history)
    p = [t.data_ptr() for t in fr]
    cam = pt_camera(pt, T.syn_camera("same"))
    nan = float("nan")
    bad = [
        dict(args=[0, p[1], p[2]]), dict(args=[p[0], 0, p[2]]), dict(args=[p[0], p[1], 0]), dict(cam=None),
        dict(out=0), dict(hout=0), dict(hin=0), dict(prev=None), dict(hout=b.hout_ptr + 8), dict(hin=b.hin_ptr + 8),
        dict(hout=b.hin_ptr + 64), dict(hout=b.hin_ptr), dict(w=0), dict(h=0), dict(max_count=0),
        dict(sigma_normal=0.0), dict(sigma_normal=nan), dict(sigma_depth=-1.0), dict(sigma_depth=nan),
    ]
    for case in bad:
        case = dict(case)
        args = case.pop("args", p)
        c, prev = case.pop("cam", cam), case.pop("prev", cam)
        hin, hout, out = case.pop("hin", b.hin_ptr), case.pop("hout", b.hout_ptr), case.pop("out", b.out_ptr)
        cw, ch = case.pop("w", w), case.pop("h", h)
        with pytest.raises(pt.PtError) as e:
            pt.temporal_device(*args, c, prev, cw, ch, hin, hout, out, **case)
        assert e.value.code == pt.PT_ERR_INVALID, case
    torch.cuda.synchronize()
    assert bool(torch.all(b.out == SENTINEL)) and bool(torch.all(b.hout == SENTINEL))
    assert np.array_equal(b.hin.cpu().numpy()[GUARD:-GUARD], history)
    for t, t0 in zip(fr, before):
        assert bool(torch.equal(t, t0))
