"""The guided denoiser on the MI355X (denoise_records and denoise_tiles, rs-pathtracing_amd/csrc/pt_denoise.hip)
through the Python mirror: frames and planes that never leave the device, against the numpy restatement
tests/denoiseref.py bit for bit; seeded planes and small shapes; the colour term; in place; a stream of the caller's;
memory around the frame and past the workspace; the host form; and that the pass leaves a renderer as it found it.
Every device call here runs with sentinels before and after the frame and after the workspace."""
import numpy as np
import pytest

import aovref
import denoiseref
from conftest import ROOT

pytestmark = pytest.mark.gpu

SEED = aovref.FRAME_SEED
SENTINEL = -7.25
GUARD = 64  # doubles of sentinel on each side


def same(got, ref):
    assert np.all(np.isfinite(got))
    bad = np.flatnonzero(np.any(got != ref, axis=1))
    assert bad.size == 0, "%d of %d pixels differ (first %s)" % (bad.size, len(ref), bad[:8].tolist())


class Buffers:
    """[guard | frame | guard] and [workspace | guard] on the device, the guards and the frame filled with the
    sentinel."""

    def __init__(self, pt, w, h):
        import torch
        self.n = w * h * 3
        self.work_n = pt.denoise_workspace_doubles(w, h)
        assert self.work_n == w * h * 12
        self.out = torch.full((self.n + 2 * GUARD,), SENTINEL, dtype=torch.float64, device="cuda")
        self.work = torch.full((self.work_n + GUARD,), SENTINEL, dtype=torch.float64, device="cuda")
        assert self.work.data_ptr() % 16 == 0

    @property
    def out_ptr(self):
        return self.out.data_ptr() + GUARD * 8

    def frame(self):
        import torch
        torch.cuda.synchronize()
        host = self.out.cpu().numpy()
        assert np.all(host[:GUARD] == SENTINEL) and np.all(host[-GUARD:] == SENTINEL), "wrote beside the frame"
        assert bool(torch.all(self.work[self.work_n:] == SENTINEL)), "wrote past the workspace"
        return host[GUARD:-GUARD].reshape(-1, 3).copy()


def on_device(arr):
    import torch
    return None if arr is None else torch.from_numpy(np.array(arr, dtype=np.float64, order="C")).cuda()


def device_denoise(pt, fr, w, h, stream_ptr=0, **kw):
    """pt.denoise_device on host planes uploaded here; the frame back on the host, the sentinels checked."""
    dev = [on_device(a) for a in fr]
    b = Buffers(pt, w, h)
    pt.denoise_device(*[0 if t is None else t.data_ptr() for t in dev], w, h, b.out_ptr, b.work.data_ptr(),
                      stream_ptr=stream_ptr, **kw)
    return b.frame()


def rendered_on_device(pt, name, depth=8):
    """The case's beauty frame and guide planes in device memory: pt_render_device, then pt_render_aov_device."""
    import torch
    text, rs, w, h, spp, _, _ = aovref.case(name)
    ps = pt.Scene.from_json(text, random_spheres=rs, seed=1)
    r = pt.HipRenderer(ps, depth=depth)
    bufs = [torch.zeros(w * h * 3, dtype=torch.float64, device="cuda") for _ in range(4)]
    st = torch.cuda.current_stream().cuda_stream
    r.render_device(ps.camera(), w, h, spp, SEED, 0, 1, bufs[0].data_ptr(), st)
    r.render_aov_device(ps.camera(), w, h, spp, SEED, 0, 1, *[b.data_ptr() for b in bufs[1:]], st)
    return ps, r, w, h, bufs, st


@pytest.mark.parametrize("name", ["cornell", "spheres", "marched"])
def test_frames_on_the_device_equal_the_restatement(pt, name):
    """The frame and its planes never leave the device; the result equals the restatement on the oracle's frame and
    planes.  (cornell: 54 rows, the last tile row is padded.)"""
    ps, r, w, h, bufs, st = rendered_on_device(pt, name)
    b = Buffers(pt, w, h)
    pt.denoise_device(*[t.data_ptr() for t in bufs], w, h, b.out_ptr, b.work.data_ptr(), stream_ptr=st)
    got = b.frame()
    _, _, img, pl = denoiseref.frame(name)
    same(got, denoiseref.denoise(img, pl["albedo"], pl["normal"], pl["depth"], w, h))
    assert np.any(got != img)


def test_textured_equals_the_restatement_on_the_gpus_own_frame(pt, monkeypatch):
    """The textured frame differs from the oracle's in the last bits of libm; the filter has no libm call, so on the
    GPU's own frame and planes it is bit for bit too."""
    monkeypatch.chdir(ROOT)  # (the scene's image texture is named relative to the repository)
    ps, r, w, h, bufs, st = rendered_on_device(pt, "textured")
    b = Buffers(pt, w, h)
    pt.denoise_device(*[t.data_ptr() for t in bufs], w, h, b.out_ptr, b.work.data_ptr(), stream_ptr=st)
    got = b.frame()
    fr = [t.cpu().numpy().reshape(-1, 3) for t in bufs]
    same(got, denoiseref.denoise(*fr, w, h))


@pytest.mark.parametrize("setting", ["defaults", "colour_on", "no_demodulation", "one_iteration", "eight_iterations"])
def test_random_planes(pt, setting):
    kw = {"defaults": {}, "colour_on": dict(sigma_colour=4.0), "no_demodulation": dict(demodulate=False),
          "one_iteration": dict(iterations=1), "eight_iterations": dict(iterations=8)}[setting]
    w, h = 40, 24
    fr = denoiseref.random_planes(w, h)
    ref = denoiseref.denoise(*fr, w, h, **kw)
    same(device_denoise(pt, fr, w, h, **kw), ref)
    if setting == "no_demodulation":
        same(device_denoise(pt, (fr[0], None, fr[2], fr[3]), w, h, **kw), ref)  # no albedo: a null pointer


@pytest.mark.parametrize("cw,ch", [(20, 13), (17, 1), (1, 1)])
def test_small_shapes(pt, cw, ch):
    full = denoiseref.random_planes(40, 24)
    fr = tuple(np.ascontiguousarray(a.reshape(24, 40, 3)[:ch, :cw]).reshape(cw * ch, 3) for a in full)
    same(device_denoise(pt, fr, cw, ch), denoiseref.denoise(*fr, cw, ch))
    same(device_denoise(pt, fr, cw, ch, sigma_colour=4.0), denoiseref.denoise(*fr, cw, ch, sigma_colour=4.0))


def test_in_place_on_a_stream_of_the_callers(pt):
    """d_out == d_rgb, queued on a non-null stream after the upload."""
    import torch
    w, h, img, pl = denoiseref.frame("spheres")
    fr = (img, pl["albedo"], pl["normal"], pl["depth"])
    ref = denoiseref.denoise(*fr, w, h)
    s = torch.cuda.Stream()
    b = Buffers(pt, w, h)
    s.wait_stream(torch.cuda.current_stream())  # the sentinel fills
    with torch.cuda.stream(s):
        dev = [on_device(a) for a in fr[1:]]
        b.out[GUARD:GUARD + b.n] = on_device(img).reshape(-1)
        pt.denoise_device(b.out_ptr, *[t.data_ptr() for t in dev], w, h, b.out_ptr, b.work.data_ptr(),
                          stream_ptr=s.cuda_stream)
    s.synchronize()
    same(b.frame(), ref)


def test_host_form_equals_the_device_form(pt):
    w, h = 40, 24
    fr = denoiseref.random_planes(w, h)
    for kw in ({}, dict(sigma_colour=4.0, iterations=3), dict(demodulate=False)):
        got = pt.denoise(*fr, w, h, **kw)
        assert got.shape == (w * h, 3)
        same(got, device_denoise(pt, fr, w, h, **kw))
    same(pt.denoise(fr[0], None, fr[2], fr[3], w, h, demodulate=False), denoiseref.denoise(*fr, w, h, demodulate=False))


def test_the_pass_leaves_the_renderer_alone(pt):
    import torch
    ps, r, w, h, bufs, st = rendered_on_device(pt, "cornell")
    opts = r.options()
    cam, ip = ps.camera(), pt.ImageParams(w, h)
    first = r.render(cam, ip, 8, seed=11)
    b = Buffers(pt, w, h)
    pt.denoise_device(*[t.data_ptr() for t in bufs], w, h, b.out_ptr, b.work.data_ptr(), stream_ptr=st)
    b.frame()
    again = r.render(cam, ip, 8, seed=11)
    assert np.array_equal(first, again) and first.mean() > 0.01
    assert r.options() == opts
    assert pt.march_guard_drops(r) == 0
    torch.cuda.synchronize()


def test_argument_errors_write_nothing(pt):
    import torch
    w, h = 40, 24
    fr = [on_device(a) for a in denoiseref.random_planes(w, h)]
    before = [t.clone() for t in fr]
    b = Buffers(pt, w, h)
    p = [t.data_ptr() for t in fr]
    nan = float("nan")
    bad = [
        dict(args=[0, p[1], p[2], p[3]]), dict(args=[p[0], 0, p[2], p[3]]), dict(args=[p[0], p[1], 0, p[3]]),
        dict(args=[p[0], p[1], p[2], 0]), dict(out=0), dict(work=0), dict(work=b.work.data_ptr() + 8),
        dict(w=0), dict(h=0), dict(iterations=0), dict(iterations=9), dict(sigma_normal=0.0),
        dict(sigma_normal=nan), dict(sigma_depth=-1.0), dict(sigma_depth=nan), dict(sigma_colour=-1.0),
        dict(sigma_colour=nan),
    ]
    for case in bad:
        case = dict(case)
        args = case.pop("args", p)
        out, work = case.pop("out", b.out_ptr), case.pop("work", b.work.data_ptr())
        cw, ch = case.pop("w", w), case.pop("h", h)
        with pytest.raises(pt.PtError) as e:
            pt.denoise_device(*args, cw, ch, out, work, **case)
        assert e.value.code == pt.PT_ERR_INVALID, case
    rc = pt.lib().pt_denoise_device(-1, p[0], p[1], p[2], p[3], w, h, 5, 0.5, 0.1, 0.0, 2, b.out_ptr,
                                    b.work.data_ptr(), None)  # an unknown flag bit
    assert rc == pt.PT_ERR_INVALID
    torch.cuda.synchronize()
    assert bool(torch.all(b.out == SENTINEL)) and bool(torch.all(b.work == SENTINEL))
    for t, t0 in zip(fr, before):
        assert bool(torch.equal(t, t0))
