"""The variance estimate and the denoiser's variance term on the MI355X (variance_window,
rs-pathtracing_amd/csrc/pt_variance.hip; denoise_records_variance and denoise_tiles_variance, pt_denoise.hip) through
the Python mirror, against the numpy restatement tests/varianceref.py bit for bit: the accumulation on synthetic
running sums and on the renderer's own windows, the windowed frame against the one-shot frame and the oracle, shards,
the denoiser on the GPU's own frames and on seeded planes, the identity with the plain denoiser, in place on a
caller's stream, the host forms and the argument errors.  Every device call here runs with sentinels around the
buffers it writes."""
import numpy as np
import pytest

import aovref
import denoiseref
import varianceref

pytestmark = pytest.mark.gpu

SEED = aovref.FRAME_SEED
SENTINEL = -7.25
GUARD = 64  # doubles of sentinel on each side
INF = float("inf")


def same_flat(got, ref):
    assert np.all(np.isfinite(got))
    bad = np.flatnonzero(got != ref)
    assert bad.size == 0, "%d of %d elements differ (first %s)" % (bad.size, ref.size, bad[:8].tolist())


def same(got, ref):
    same_flat(np.asarray(got).reshape(-1), np.asarray(ref).reshape(-1))


def on_device(arr):
    import torch
    return None if arr is None else torch.from_numpy(np.array(arr, dtype=np.float64, order="C")).cuda()


class Guarded:
    """[guard | n doubles | guard] on the device, all filled with the sentinel; `lead` extra doubles in front shift
    the payload's alignment."""

    def __init__(self, n, lead=0):
        import torch
        self.n, self.lead = n, lead
        self.t = torch.full((lead + n + 2 * GUARD,), SENTINEL, dtype=torch.float64, device="cuda")

    @property
    def ptr(self):
        return self.t.data_ptr() + (self.lead + GUARD) * 8

    def untouched(self):
        import torch
        return bool(torch.all(self.t == SENTINEL))

    def get(self):
        import torch
        torch.cuda.synchronize()
        host = self.t.cpu().numpy()
        a, b = self.lead + GUARD, self.lead + GUARD + self.n
        assert np.all(host[:a] == SENTINEL) and np.all(host[b:] == SENTINEL), "wrote beside the buffer"
        return host[a:b].copy()


# ---- pt_variance_window_device on synthetic running sums ----

def device_variance(pt, snaps, n, lead=0):
    """The K windows on the device: the workspace starts as sentinels, the plane is written by the last alone."""
    k, count = len(snaps), snaps[0].size
    assert pt.variance_workspace_doubles(count // 3, 1) == 2 * count
    e = varianceref.edges(n, k)
    work, var = Guarded(2 * count, lead), Guarded(count, lead)
    for j in range(1, k + 1):
        out = on_device(snaps[j - 1])
        assert var.untouched()
        pt.variance_window_device(out.data_ptr(), count, e[j] - e[j - 1], n, j, k, work.ptr, var.ptr)
    work.get()
    return var.get()


@pytest.mark.parametrize("n,k", varianceref.PLANS)
def test_synthetic_sums_equal_the_restatement(pt, n, k):
    snaps = varianceref.synthetic(40 * 24 * 3, n, k)
    same_flat(device_variance(pt, snaps, n), varianceref.variance(snaps, n))


@pytest.mark.parametrize("cw,ch", [(20, 13), (17, 1), (1, 1)])
def test_small_shapes(pt, cw, ch):
    """780 elements (even: 16-byte accesses), 51 and 3 (odd: the 8-byte kernel), each also with the buffers 8 bytes
    off 16-byte alignment."""
    for n, k in [(7, 3), (64, 8)]:
        snaps = varianceref.synthetic(cw * ch * 3, n, k)
        ref = varianceref.variance(snaps, n)
        same_flat(device_variance(pt, snaps, n), ref)
        same_flat(device_variance(pt, snaps, n, lead=1), ref)


def test_shard_count_with_padding(pt):
    count, padding = 2 * 768, 128 * 3
    assert pt.variance_workspace_doubles(40, 24, 1, 3) == 2 * count
    snaps = varianceref.synthetic(count, 7, 3, padding=padding)
    got = device_variance(pt, snaps, 7)
    same_flat(got, varianceref.variance(snaps, 7))
    assert np.all(got[-padding:] == 0.0)


# ---- pt_render_variance_device ----

RENDER_CASES = {
    "cornell": ("cornell", 16, 8, 0, 1),
    "spheres": ("spheres", 7, 3, 0, 1),
    "marched": ("marched", 2, 2, 0, 1),
    "cornell_rank_1_of_3": ("cornell", 16, 8, 1, 3),
}


@pytest.mark.parametrize("case", list(RENDER_CASES))
def test_render_variance_device(pt, case):
    import torch
    name, spp, windows, rank, world = RENDER_CASES[case]
    text, rs, w, h, _, osc, _ = aovref.case(name)
    ps = pt.Scene.from_json(text, random_spheres=rs, seed=1)
    r = pt.HipRenderer(ps, depth=8)
    cam, ip = ps.camera(), pt.ImageParams(w, h)
    count = w * h * 3 if world == 1 else pt.shard_tiles(w, h, rank, world) * 768
    assert pt.variance_workspace_doubles(w, h, rank, world) == 2 * count
    before = r.render(cam, ip, 4, seed=11)
    st = torch.cuda.current_stream().cuda_stream

    out, var, work = Guarded(count), Guarded(count), Guarded(2 * count)
    r.render_variance_device(cam, w, h, spp, SEED, rank, world, windows, out.ptr, var.ptr, work.ptr, st)
    got_out, got_var = out.get(), var.get()
    work.get()

    # the frame: pt_render_device's, bit for bit, and the oracle's where the whole frame is held
    one = torch.zeros(count, dtype=torch.float64, device="cuda")
    r.render_device(cam, w, h, spp, SEED, rank, world, one.data_ptr(), st)
    torch.cuda.synchronize()
    same_flat(got_out, one.cpu().numpy())
    if world == 1:
        same(got_out, osc.render(w, h, spp, 8, SEED))

    # the plane: the restatement on snapshots taken here with the same edges
    e = varianceref.edges(spp, windows)
    buf = torch.zeros(count, dtype=torch.float64, device="cuda")
    snaps = []
    for j in range(1, windows + 1):
        r.render_device_samples(cam, w, h, spp, SEED, rank, world, e[j - 1], e[j], buf.data_ptr(), st)
        torch.cuda.synchronize()
        snaps.append(buf.cpu().numpy().copy())
    same_flat(snaps[-1], got_out)
    ref = varianceref.variance(snaps, spp)
    same_flat(got_var, ref)
    assert np.sum(got_var > 0.0) >= count // 10
    if world > 1:
        # the elements of the shard's pixels outside the frame (cornell: 54 rows, the last tile row has 6)
        pad = np.flatnonzero(np.all(np.stack(snaps) == 0.0, axis=0))
        assert pad.size >= 10 * 16 * 3 and np.all(got_var[pad] == 0.0)

    again = r.render(cam, ip, 4, seed=11)
    assert np.array_equal(before, again) and before.mean() > 0.01
    assert pt.march_guard_drops(r) == 0


def test_host_form_of_render_variance(pt):
    text, rs, w, h, _, osc, _ = aovref.case("spheres")
    ps = pt.Scene.from_json(text, random_spheres=rs, seed=1)
    r = pt.HipRenderer(ps, depth=8)
    rgb, var = r.render_variance(ps.camera(), pt.ImageParams(w, h), 8, seed=SEED)  # 8 windows of 1 sample
    assert rgb.shape == var.shape == (w * h, 3)
    same(rgb, osc.render(w, h, 8, 8, SEED))
    assert np.all(var >= 0.0) and np.mean(var > 0.0) > 0.5
    # the device form's plane, bit for bit (that one is checked against the restatement above)
    import torch
    n = w * h * 3
    d_out, d_var, d_work = (torch.zeros(k * n, dtype=torch.float64, device="cuda") for k in (1, 1, 2))
    r.render_variance_device(ps.camera(), w, h, 8, SEED, 0, 1, 8, d_out.data_ptr(), d_var.data_ptr(), d_work.data_ptr())
    torch.cuda.synchronize()
    same(var, d_var.cpu().numpy())
    same(rgb, d_out.cpu().numpy())
    # another window count gives another estimate of the same frame
    rgb4, var4 = r.render_variance(ps.camera(), pt.ImageParams(w, h), 8, seed=SEED, windows=4)
    same(rgb4, rgb)
    assert np.any(var4 != var)


def test_render_variance_argument_errors_write_nothing(pt):
    import torch
    text, rs, w, h, _, _, _ = aovref.case("marched")
    ps = pt.Scene.from_json(text, random_spheres=rs, seed=1)
    r = pt.HipRenderer(ps, depth=8)
    cam = ps.camera()
    count = w * h * 3
    out, var, work = Guarded(count), Guarded(count), Guarded(2 * count)
    good = dict(w=w, h=h, spp=8, rank=0, world=1, windows=4, out=out.ptr, var=var.ptr, work=work.ptr)
    bad = [dict(out=0), dict(var=0), dict(work=0), dict(w=0), dict(h=0), dict(spp=0), dict(windows=1),
           dict(windows=0), dict(windows=9), dict(rank=1), dict(rank=3, world=3), dict(world=0)]
    for case in bad:
        a = dict(good, **case)
        with pytest.raises(pt.PtError) as e:
            r.render_variance_device(cam, a["w"], a["h"], a["spp"], SEED, a["rank"], a["world"], a["windows"],
                                     a["out"], a["var"], a["work"])
        assert e.value.code == pt.PT_ERR_INVALID, case
    for windows in (1, 9):
        with pytest.raises(pt.PtError) as e:
            r.render_variance(cam, pt.ImageParams(w, h), 8, seed=SEED, windows=windows)
        assert e.value.code == pt.PT_ERR_INVALID
    # a progressive frame in flight: PT_ERR_STATE
    r.start_rendering(cam, pt.ImageParams(w, h), 2, SEED)
    with pytest.raises(pt.PtError) as e:
        r.render_variance_device(cam, w, h, 8, SEED, 0, 1, 4, out.ptr, var.ptr, work.ptr)
    assert e.value.code == pt.PT_ERR_STATE
    r.stop_rendering()
    torch.cuda.synchronize()
    assert out.untouched() and var.untouched() and work.untouched()


# ---- pt_denoise_variance_device ----

class Buffers:
    """[guard | frame | guard] and [workspace | guard] on the device, filled with the sentinel."""

    def __init__(self, pt, w, h):
        import torch
        self.n = w * h * 3
        self.work_n = pt.denoise_workspace_doubles(w, h)
        self.out = Guarded(self.n)
        self.work = torch.full((self.work_n + GUARD,), SENTINEL, dtype=torch.float64, device="cuda")
        assert self.work.data_ptr() % 16 == 0

    def frame(self):
        import torch
        got = self.out.get().reshape(-1, 3)
        assert bool(torch.all(self.work[self.work_n:] == SENTINEL)), "wrote past the workspace"
        return got


def device_denoise(pt, fr, w, h, stream_ptr=0, **kw):
    dev = [on_device(a) for a in fr]
    b = Buffers(pt, w, h)
    pt.denoise_variance_device(*[0 if t is None else t.data_ptr() for t in dev], w, h, b.out.ptr, b.work.data_ptr(),
                               stream_ptr=stream_ptr, **kw)
    return b.frame()


def random_case(w=40, h=24):
    return denoiseref.random_planes(w, h) + (varianceref.random_variance(w, h),)


@pytest.mark.parametrize("name", ["cornell", "spheres"])
def test_the_gpus_own_frames_equal_the_restatement(pt, name):
    """Frame, variance plane and guide planes rendered on the device and never leaving it (16 spp, 8 windows)."""
    import torch
    text, rs, w, h, _, _, _ = aovref.case(name)
    ps = pt.Scene.from_json(text, random_spheres=rs, seed=1)
    r = pt.HipRenderer(ps, depth=8)
    n = w * h * 3
    bufs = [torch.zeros(n, dtype=torch.float64, device="cuda") for _ in range(5)]  # rgb, albedo, normal, depth, var
    vwork = torch.zeros(2 * n, dtype=torch.float64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    r.render_variance_device(ps.camera(), w, h, 16, SEED, 0, 1, 8, bufs[0].data_ptr(), bufs[4].data_ptr(),
                             vwork.data_ptr(), st)
    r.render_aov_device(ps.camera(), w, h, 16, SEED, 0, 1, *[b.data_ptr() for b in bufs[1:4]], st)
    b = Buffers(pt, w, h)
    pt.denoise_variance_device(*[t.data_ptr() for t in bufs], w, h, b.out.ptr, b.work.data_ptr(), stream_ptr=st)
    got = b.frame()
    fr = [t.cpu().numpy().reshape(-1, 3) for t in bufs]
    same(got, varianceref.denoise_variance(*fr, w, h))
    assert np.any(got != fr[0]) and np.any(got != denoiseref.denoise(*fr[:4], w, h))


SETTINGS = {"defaults": {}, "one_iteration": dict(iterations=1), "eight_iterations": dict(iterations=8),
            "no_demodulation": dict(demodulate=False), "sigma_variance_1": dict(sigma_variance=1.0)}


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_random_planes(pt, setting):
    w, h = 40, 24
    fr = random_case(w, h)
    kw = SETTINGS[setting]
    ref = varianceref.denoise_variance(*fr, w, h, **kw)
    same(device_denoise(pt, fr, w, h, **kw), ref)
    if setting == "no_demodulation":
        same(device_denoise(pt, (fr[0], None) + fr[2:], w, h, **kw), ref)  # no albedo: a null pointer


@pytest.mark.parametrize("cw,ch", [(20, 13), (17, 1), (1, 1)])
def test_small_shapes_of_the_denoiser(pt, cw, ch):
    fr = tuple(np.ascontiguousarray(a.reshape(24, 40, 3)[:ch, :cw]).reshape(cw * ch, 3) for a in random_case())
    same(device_denoise(pt, fr, cw, ch), varianceref.denoise_variance(*fr, cw, ch))
    same(device_denoise(pt, fr, cw, ch, iterations=8), varianceref.denoise_variance(*fr, cw, ch, iterations=8))


def test_all_zero_variance_plane(pt):
    w, h = 40, 24
    fr = denoiseref.random_planes(w, h) + (np.zeros((w * h, 3)),)
    same(device_denoise(pt, fr, w, h), varianceref.denoise_variance(*fr, w, h))


def test_infinite_sigma_variance_is_pt_denoise_device(pt):
    """The identity on the device, kernel against kernel: sigma_variance = +inf gives pt_denoise_device's frame."""
    w, h = 40, 24
    fr = random_case(w, h)
    for kw in ({}, dict(demodulate=False), dict(iterations=8)):
        dev = [on_device(a) for a in fr[:4]]
        b = Buffers(pt, w, h)
        pt.denoise_device(*[t.data_ptr() for t in dev], w, h, b.out.ptr, b.work.data_ptr(), **kw)
        plain = b.frame()
        same(device_denoise(pt, fr, w, h, sigma_variance=INF, **kw), plain)
        same(plain, denoiseref.denoise(*fr[:4], w, h, **kw))


def test_in_place_on_a_stream_of_the_callers(pt):
    import torch
    w, h = 40, 24
    fr = random_case(w, h)
    ref = varianceref.denoise_variance(*fr, w, h)
    s = torch.cuda.Stream()
    b = Buffers(pt, w, h)
    s.wait_stream(torch.cuda.current_stream())  # the sentinel fills
    with torch.cuda.stream(s):
        dev = [on_device(a) for a in fr[1:]]
        b.out.t[GUARD:GUARD + b.n] = on_device(fr[0]).reshape(-1)
        pt.denoise_variance_device(b.out.ptr, *[t.data_ptr() for t in dev], w, h, b.out.ptr, b.work.data_ptr(),
                                   stream_ptr=s.cuda_stream)
    s.synchronize()
    same(b.frame(), ref)


def test_host_form_equals_the_restatement(pt):
    w, h = 40, 24
    fr = random_case(w, h)
    for kw in ({}, dict(sigma_variance=1.0, iterations=3), dict(demodulate=False)):
        got = pt.denoise_variance(*fr, w, h, **kw)
        assert got.shape == (w * h, 3)
        same(got, varianceref.denoise_variance(*fr, w, h, **kw))
    same(pt.denoise_variance(fr[0], None, *fr[2:], w, h, demodulate=False),
         varianceref.denoise_variance(*fr, w, h, demodulate=False))


def test_denoise_variance_argument_errors_write_nothing(pt):
    import torch
    w, h = 40, 24
    fr = [on_device(a) for a in random_case(w, h)]
    before = [t.clone() for t in fr]
    b = Buffers(pt, w, h)
    p = [t.data_ptr() for t in fr]
    nan = float("nan")
    bad = [dict(args=[0] + p[1:]), dict(args=[p[0], 0] + p[2:]), dict(args=p[:2] + [0] + p[3:]),
           dict(args=p[:3] + [0, p[4]]), dict(args=p[:4] + [0]), dict(out=0), dict(work=0),
           dict(work=b.work.data_ptr() + 8), dict(w=0), dict(h=0), dict(iterations=0), dict(iterations=9),
           dict(sigma_normal=0.0), dict(sigma_depth=nan), dict(sigma_variance=0.0), dict(sigma_variance=-8.0),
           dict(sigma_variance=nan)]
    for case in bad:
        case = dict(case)
        args = case.pop("args", p)
        out, work = case.pop("out", b.out.ptr), case.pop("work", b.work.data_ptr())
        cw, ch = case.pop("w", w), case.pop("h", h)
        with pytest.raises(pt.PtError) as e:
            pt.denoise_variance_device(*args, cw, ch, out, work, **case)
        assert e.value.code == pt.PT_ERR_INVALID, case
    rc = pt.lib().pt_denoise_variance_device(-1, *p, w, h, 5, 0.5, 0.1, 8.0, 2, b.out.ptr, b.work.data_ptr(), None)
    assert rc == pt.PT_ERR_INVALID  # an unknown flag bit
    torch.cuda.synchronize()
    assert b.out.untouched() and bool(torch.all(b.work == SENTINEL))
    for t, t0 in zip(fr, before):
        assert bool(torch.equal(t, t0))
