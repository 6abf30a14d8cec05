"""Adaptive sampling on the GPU (pt_render_adaptive_device, pt_render_adaptive): the tile maps, the frame and the
variance plane against the numpy restatement tests/adaptiveref.py fed the GPU's own running sums, bit for bit; every
tile's pixels against the oracle's frame at that tile's own sample count, bit for bit; thresholds 0 and +inf against
pt_render_device; merge_gap, sharded frames, sentinels around every buffer, argument errors."""
import functools

import numpy as np
import pytest

import adaptiveref
import aovref

pytestmark = pytest.mark.gpu

SEED = aovref.FRAME_SEED
SENTINEL = -7.25
TS_SENTINEL = 0xDEADBEE
GUARD = 64
INF = float("inf")


def same(got, ref, what=""):
    got, ref = np.asarray(got).reshape(-1), np.asarray(ref).reshape(-1)
    assert np.all(np.isfinite(got)), what
    bad = np.flatnonzero(got != ref)
    assert bad.size == 0, "%s: %d of %d elements differ (first %s)" % (what, bad.size, ref.size, bad[:8].tolist())


class Guarded:
    """[guard | n elements | guard] on the device, all filled with a sentinel."""

    def __init__(self, n, dtype=None, sentinel=SENTINEL, align16=False):
        import torch
        self.n, self.sentinel = n, sentinel
        self.t = torch.full((n + 2 * GUARD,), sentinel, dtype=dtype or torch.float64, device="cuda")
        if align16:
            assert self.ptr % 16 == 0

    @property
    def ptr(self):
        return self.t.data_ptr() + GUARD * self.t.element_size()

    def untouched(self):
        import torch
        torch.cuda.synchronize()
        return bool(torch.all(self.t == self.sentinel))

    def get(self, payload_written=True):
        import torch
        torch.cuda.synchronize()
        host = self.t.cpu().numpy()
        a, b = GUARD, GUARD + self.n
        assert np.all(host[:a] == self.sentinel) and np.all(host[b:] == self.sentinel), "wrote beside the buffer"
        if payload_written:
            assert not np.any(host[a:b] == self.sentinel), "an element was left unwritten"
        return host[a:b].copy()


def renderer(pt, name, text=None):
    if text is None:
        text, rs, _, _, _, osc, _ = aovref.case(name)
    else:
        rs, osc = False, None
    ps = pt.Scene.from_json(text, random_spheres=rs, seed=1)
    return ps, pt.HipRenderer(ps, depth=8), osc


def run(pt, r, cam, w, h, window, cap, threshold, rank=0, world=1, merge_gap=None, floor=0.01, min_samples=0,
        stream=0, optional=True):
    """One adaptive frame into guarded buffers: (out, variance, tile_samples, tile_error, samples launched)."""
    import torch
    ntiles = pt.shard_tiles(w, h, rank, world)
    count = w * h * 3 if world == 1 else ntiles * 768
    assert pt.adaptive_workspace_doubles(w, h, rank, world) == 3 * count
    out, var, work = Guarded(count), Guarded(count), Guarded(3 * count, align16=True)
    ts, te = Guarded(ntiles, torch.int32, TS_SENTINEL), Guarded(ntiles)
    kw = {} if merge_gap is None else dict(merge_gap=merge_gap)
    launched = r.render_adaptive_device(cam, w, h, cap, threshold, SEED, rank, world, out.ptr,
                                        var.ptr if optional else 0, ts.ptr, te.ptr if optional else 0, work.ptr,
                                        stream, window=window, min_samples=min_samples, luminance_floor=floor, **kw)
    work.get(payload_written=False)
    if not optional:
        assert var.untouched() and te.untouched()
        return out.get(), None, ts.get().astype(np.uint32), None, launched
    return out.get(), var.get(), ts.get().astype(np.uint32), te.get(), launched


def gpu_sums(r, cam, w, h, window, cap):
    """The whole frame's running sums after each window, as the adaptive frame's renders leave them: windows of a
    frame of cap + 1 samples."""
    import torch
    buf = torch.zeros(w * h * 3, dtype=torch.float64, device="cuda")
    e = adaptiveref.edges(window, cap)
    snaps = []
    for k in range(1, len(e)):
        r.render_device_samples(cam, w, h, cap + 1, SEED, 0, 1, e[k - 1], e[k], buf.data_ptr())
        torch.cuda.synchronize()
        snaps.append(buf.cpu().numpy().reshape(-1, 3).copy())
    return snaps


def check_against_restatement(got, snaps, w, h, window, cap, threshold, floor=0.01, min_samples=0):
    rgb, var, ts, te = adaptiveref.adaptive(snaps, w, h, window, cap, threshold, floor, min_samples)
    assert np.array_equal(got[2], ts), (got[2].tolist(), ts.tolist())
    same(got[3], te, "tile_error")
    same(got[0], rgb, "frame")
    same(got[1], var, "variance")
    return ts, te


def device_frame(r, cam, w, h, spp, rank=0, world=1, count=None):
    import torch
    one = torch.zeros(count or w * h * 3, dtype=torch.float64, device="cuda")
    r.render_device(cam, w, h, spp, SEED, rank, world, one.data_ptr())
    torch.cuda.synchronize()
    return one.cpu().numpy()


def tile_of_pixel(w, h):
    tx, _ = adaptiveref.tiles_of(w, h)
    y, x = np.divmod(np.arange(w * h), w)
    return (y // 16) * tx + x // 16


# ---- cornell_box 96x54: window 8, cap 128, threshold 0.2 ----

CORNELL = dict(window=8, cap=128, threshold=0.2)


@functools.lru_cache(maxsize=None)
def cornell(pt):
    ps, r, osc = renderer(pt, "cornell")
    w, h = 96, 54
    before = r.render(ps.camera(), pt.ImageParams(w, h), 4, seed=11)
    got = run(pt, r, ps.camera(), w, h, **CORNELL)
    after = r.render(ps.camera(), pt.ImageParams(w, h), 4, seed=11)
    snaps = gpu_sums(r, ps.camera(), w, h, CORNELL["window"], CORNELL["cap"])
    return ps, r, osc, w, h, got, snaps, before, after


def test_cornell_equals_the_restatement(pt):
    _, r, _, w, h, got, snaps, before, after = cornell(pt)
    ts, te = check_against_restatement(got, snaps, w, h, **CORNELL)
    assert np.all(got[1] >= 0.0) and np.mean(got[1] > 0.0) > 0.9
    # the stop rule, tile by tile: stopped below the cap means converged there and at no evaluation before
    thr2 = CORNELL["threshold"] ** 2
    assert np.all(te[ts < CORNELL["cap"]] <= thr2 * (1 + 1e-12)) and np.any(te[ts == CORNELL["cap"]] > thr2)
    # pt_render_device gives the same bits before and after an adaptive frame
    assert np.array_equal(before, after) and before.mean() > 0.01
    assert pt.march_guard_drops(r) == 0


def test_cornell_tiles_equal_the_oracle_at_their_own_counts(pt):
    _, _, osc, w, h, got, _, _, _ = cornell(pt)
    rgb, ts = got[0].reshape(-1, 3), got[2]
    tile = tile_of_pixel(w, h)
    for n in sorted(set(ts.tolist())):
        px = np.flatnonzero(ts[tile] == n).astype(np.uint32)
        same(rgb[px], osc.render(w, h, int(n), 8, SEED, pixels=px), "tiles stopped at %d samples" % n)


def test_cornell_exercises_the_rule(pt):
    """The oracle-restated sums on the CPU give 9 distinct counts, one tile at 16 and 11 at 128."""
    _, _, _, _, _, got, _, _, _ = cornell(pt)
    ts = got[2]
    print("tile_samples", ts.tolist())
    assert ts.size == 24 and np.all(ts % 8 == 0) and ts.min() >= 16 and ts.max() <= 128
    assert len(set(ts.tolist())) >= 4
    assert np.sum(ts == 16) >= 1 and np.sum(ts == 128) >= 3
    # launched: every tile's pixels times its count (merge_gap's waste on top, none below)
    pixels = adaptiveref.inside(96, 54).sum(axis=1)
    assert got[4] >= int(np.sum(pixels * ts.astype(np.int64)))


# ---- spheres 64x64 ----

@functools.lru_cache(maxsize=None)
def spheres(pt):
    ps, r, osc = renderer(pt, "spheres")
    return ps, r, osc, 64, 64


def test_spheres_sky_tiles_stop_at_16(pt):
    """The tiles that show nothing but sky (no first hit in any pixel: coverage 0 in the guide planes) are all but
    noiseless -- the sky is a smooth gradient, and only the samples' jitter inside the pixel varies it -- and stop at
    the first evaluation."""
    ps, r, _, w, h = spheres(pt)
    got = run(pt, r, ps.camera(), w, h, 8, 64, 0.02)
    snaps = gpu_sums(r, ps.camera(), w, h, 8, 64)
    ts, te = check_against_restatement(got, snaps, w, h, 8, 64, 0.02)
    coverage = adaptiveref.to_tiles(aovref.case("spheres")[6]["depth"], w, h)[..., 1]
    sky = np.flatnonzero(np.all(coverage == 0.0, axis=1))
    print("tile_samples", ts.tolist(), "sky tiles", sky.tolist(), "their error", np.sqrt(te[sky]).tolist())
    assert sky.size == 4, sky.tolist()
    assert np.all(ts[sky] == 16) and np.all(np.sqrt(te[sky]) < 0.02 / 10)
    assert np.any(ts > 16) and len(set(ts.tolist())) >= 3  # the tiles with spheres in them go on


def test_spheres_threshold_zero_runs_to_the_cap(pt):
    ps, r, _, w, h = spheres(pt)
    got = run(pt, r, ps.camera(), w, h, 8, 24, 0.0)
    ts = got[2]
    var16 = adaptiveref.to_tiles(got[1], w, h)
    equal = np.all(var16 == 0.0, axis=(1, 2))
    assert np.all(ts[~equal] == 24) and np.all(ts[equal] == 16) and np.sum(~equal) >= 8
    full, early = device_frame(r, ps.camera(), w, h, 24), device_frame(r, ps.camera(), w, h, 16)
    sel = np.repeat(ts[tile_of_pixel(w, h)] == 24, 3)
    same(got[0][sel], full[sel], "tiles at the cap")
    same(got[0][~sel], early[~sel], "all-equal tiles")


def test_spheres_threshold_infinite_stops_at_16(pt):
    ps, r, _, w, h = spheres(pt)
    got = run(pt, r, ps.camera(), w, h, 8, 24, INF)
    assert np.all(got[2] == 16)
    same(got[0], device_frame(r, ps.camera(), w, h, 16), "frame")
    assert got[4] == 64 * 64 * 16


def test_min_samples_holds_every_tile_back(pt):
    ps, r, _, w, h = spheres(pt)
    got = run(pt, r, ps.camera(), w, h, 8, 40, INF, min_samples=25)
    assert np.all(got[2] == 32)
    same(got[0], device_frame(r, ps.camera(), w, h, 32), "frame")


def test_cap_not_a_multiple_of_the_window(pt):
    ps, r, _, w, h = spheres(pt)
    got = run(pt, r, ps.camera(), w, h, 8, 20, 0.02)
    snaps = gpu_sums(r, ps.camera(), w, h, 8, 20)
    ts, _ = check_against_restatement(got, snaps, w, h, 8, 20, 0.02)
    assert set(ts.tolist()) == {16, 20}
    full = device_frame(r, ps.camera(), w, h, 20)
    sel = np.repeat(ts[tile_of_pixel(w, h)] == 20, 3)
    same(got[0][sel], full[sel], "tiles at the cap of 20")


def test_a_20x13_frame(pt):
    """One partial column and one partial row: tiles of 16x13 and 4x13 pixels."""
    ps, r, osc, _, _ = spheres(pt)
    w, h = 20, 13
    got = run(pt, r, ps.camera(), w, h, 8, 32, 0.02)
    snaps = gpu_sums(r, ps.camera(), w, h, 8, 32)
    ts, _ = check_against_restatement(got, snaps, w, h, 8, 32, 0.02)
    tile = tile_of_pixel(w, h)
    for n in sorted(set(ts.tolist())):
        px = np.flatnonzero(ts[tile] == n).astype(np.uint32)
        same(got[0].reshape(-1, 3)[px], osc.render(w, h, int(n), 8, SEED, pixels=px), "tiles at %d" % n)


def test_optional_outputs_may_be_null_and_a_stream_of_the_callers(pt):
    import torch
    ps, r, _, w, h = spheres(pt)
    a = run(pt, r, ps.camera(), w, h, 8, 24, 0.02)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        b = run(pt, r, ps.camera(), w, h, 8, 24, 0.02, stream=st.cuda_stream, optional=False)
    same(b[0], a[0], "frame")
    assert np.array_equal(a[2], b[2]) and a[4] == b[4]


def test_marched_frame_equals_the_restatement(pt):
    from conftest import scene_text
    ps, r, _ = renderer(pt, None, text=scene_text("marched.json"))
    w, h = 32, 32
    got = run(pt, r, ps.camera(), w, h, 2, 6, 0.1)
    snaps = gpu_sums(r, ps.camera(), w, h, 2, 6)
    check_against_restatement(got, snaps, w, h, 2, 6, 0.1)
    assert pt.march_guard_drops(r) == 0


# ---- merge_gap, shards ----

def test_merge_gap_changes_only_the_work(pt):
    ps, r, _, w, h, got, _, _, _ = cornell(pt)
    runs = {g: run(pt, r, ps.camera(), w, h, merge_gap=g, **CORNELL) for g in (0, 1, 1000)}
    for g, b in runs.items():
        for k, what in enumerate(("frame", "variance", "tile_samples", "tile_error")):
            same(b[k], runs[0][k], "%s at merge_gap %d" % (what, g))
    same(runs[0][0], got[0], "the default merge_gap")
    assert runs[0][4] <= runs[1][4] <= runs[1000][4]
    pixels = adaptiveref.inside(w, h).sum(axis=1)
    assert runs[0][4] == int(np.sum(pixels * runs[0][2].astype(np.int64)))  # no waste without merging
    assert runs[1000][4] > runs[0][4]


@pytest.mark.parametrize("world", [2, 3])
def test_shards_equal_the_whole_frame(pt, world):
    import torch
    ps, r, _, w, h, whole, _, _, _ = cornell(pt)
    per = pt.shard_tiles(w, h, 0, world)
    gathered = {k: torch.zeros(world * per * 768, dtype=torch.float64, device="cuda") for k in ("out", "var")}
    frames = {k: torch.zeros(w * h * 3, dtype=torch.float64, device="cuda") for k in ("out", "var")}
    ts, te = np.zeros(24, dtype=np.uint32), np.zeros(24)
    for rank in range(world):
        out, var, s, e, _ = run(pt, r, ps.camera(), w, h, rank=rank, world=world, **CORNELL)
        ids = adaptiveref.rank_tiles(w, h, rank, world)
        ts[ids], te[ids] = s, e
        pad = ~adaptiveref.inside(w, h)[ids]
        assert np.all(out.reshape(-1, 256, 3)[pad] == 0.0) and np.all(var.reshape(-1, 256, 3)[pad] == 0.0)
        for k, a in (("out", out), ("var", var)):
            gathered[k][rank * per * 768: rank * per * 768 + a.size] = torch.from_numpy(a).cuda()
    for k in ("out", "var"):
        pt.unshard_device(gathered[k].data_ptr(), w, h, world, frames[k].data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(ts, whole[2])
    same(te, whole[3], "tile_error")
    same(frames["out"].cpu().numpy(), whole[0], "unsharded frame")
    same(frames["var"].cpu().numpy(), whole[1], "unsharded variance")


# ---- the host form, argument errors ----

def test_host_form(pt):
    ps, r, _, w, h = spheres(pt)
    rgb, ts, te, var, launched = r.render_adaptive(ps.camera(), pt.ImageParams(w, h), 24, 0.02, seed=SEED,
                                                   return_samples_rendered=True)
    assert rgb.shape == var.shape == (w * h, 3) and ts.shape == te.shape == (16,) and ts.dtype == np.uint32
    dev = run(pt, r, ps.camera(), w, h, 8, 24, 0.02)
    same(rgb, dev[0], "frame")
    same(var, dev[1], "variance")
    same(te, dev[3], "tile_error")
    assert np.array_equal(ts, dev[2]) and launched == dev[4]
    assert len(r.render_adaptive(ps.camera(), pt.ImageParams(w, h), 24, 0.02, seed=SEED)) == 4


def test_argument_errors_write_nothing(pt):
    import torch
    ps, r, _, w, h = spheres(pt)
    cam = ps.camera()
    count = w * h * 3
    out, var, work = Guarded(count), Guarded(count), Guarded(3 * count, align16=True)
    ts, te = Guarded(16, torch.int32, TS_SENTINEL), Guarded(16)
    good = dict(w=w, h=h, cap=24, thr=0.1, rank=0, world=1, out=out.ptr, ts=ts.ptr, work=work.ptr, window=8,
                min_samples=0, floor=0.01)
    bad = [dict(out=0), dict(ts=0), dict(work=0), dict(work=work.ptr + 8), dict(w=0), dict(h=0), dict(window=0),
           dict(cap=8), dict(cap=7), dict(cap=0xFFFFFFFF), dict(min_samples=25), dict(thr=-1.0),
           dict(thr=float("nan")), dict(floor=-0.5), dict(floor=float("nan")), dict(rank=1), dict(rank=16, world=17),
           dict(world=0)]

    def call(a):
        return r.render_adaptive_device(cam, a["w"], a["h"], a["cap"], a["thr"], SEED, a["rank"], a["world"],
                                        a["out"], var.ptr, a["ts"], te.ptr, a["work"], window=a["window"],
                                        min_samples=a["min_samples"], luminance_floor=a["floor"])

    for case in bad:
        with pytest.raises(pt.PtError) as e:
            call(dict(good, **case))
        assert e.value.code == pt.PT_ERR_INVALID, case
    with pytest.raises(pt.PtError) as e:
        r.render_adaptive(cam, pt.ImageParams(w, h), 8, 0.1)
    assert e.value.code == pt.PT_ERR_INVALID
    # a progressive frame in flight: PT_ERR_STATE
    r.start_rendering(cam, pt.ImageParams(w, h), 2, SEED)
    with pytest.raises(pt.PtError) as e:
        call(good)
    assert e.value.code == pt.PT_ERR_STATE
    r.stop_rendering()
    torch.cuda.synchronize()
    assert all(b.untouched() for b in (out, var, work, ts, te))
