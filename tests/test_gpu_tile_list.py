"""Listed launches on the GPU (pt_render_device_tiles; pt_render_adaptive_list_device, pt_render_adaptive_list): one
launch over a list of a rank's tiles.  A listed tile is pt_render_device_samples' tile bit for bit (and the oracle's),
every other element of the buffer keeps its sentinel; across chunk sizes, sample windows over different lists, partial
tiles, compact shards, the march, split and deep kernel families; the adaptive frame through the list against the
run-based frame bit for bit, with its launches counted; argument errors."""
import functools
import subprocess

import numpy as np
import pytest

import adaptiveref
from conftest import native_lib, scene_text
from test_gpu_adaptive import CORNELL, GUARD, SEED, SENTINEL, TS_SENTINEL, Guarded, renderer, same

pytestmark = pytest.mark.gpu

WAVE = 1  # ran_engine: the wavefront engine
LIST8 = [1, 2, 5, 7, 8, 13, 22, 23]


def device_frame(r, cam, w, h, spp, rank=0, world=1, s=None):
    """pt_render_device's frame (s: the running sums pt_render_device_samples leaves for the window s)."""
    import torch
    n = w * h * 3 if world == 1 else r_tiles(w, h, rank, world) * 768
    one = torch.zeros(n, dtype=torch.float64, device="cuda")
    if s is None:
        r.render_device(cam, w, h, spp, SEED, rank, world, one.data_ptr())
    else:
        r.render_device_samples(cam, w, h, spp, SEED, rank, world, s[0], s[1], one.data_ptr())
    torch.cuda.synchronize()
    return one.cpu().numpy()


def r_tiles(w, h, rank, world):
    tx, ty = adaptiveref.tiles_of(w, h)
    return len(range(rank, tx * ty, world))


def as_tiles(buf, w, h, world):
    """(ntiles, 256, 3) of a d_out buffer: the compact shard as it is, the frame cut into tiles (a sentinel outside
    the frame, where the frame has no element)."""
    if world > 1:
        return np.asarray(buf).reshape(-1, 256, 3)
    t = adaptiveref.to_tiles(np.asarray(buf).reshape(-1, 3), w, h)
    t[~adaptiveref.inside(w, h)] = SENTINEL
    return t


def listed(r, cam, w, h, spp, tiles, s0, s1, rank=0, world=1, into=None, stream=0):
    """One listed launch into a guarded buffer (a new one full of sentinels, or `into`); the buffer."""
    n = w * h * 3 if world == 1 else r_tiles(w, h, rank, world) * 768
    g = into or Guarded(n)
    r.render_device_tiles(cam, w, h, spp, SEED, rank, world, s0, s1, tiles, g.ptr, stream)
    return g


def check_listed(g, ref, w, h, tiles, rank=0, world=1, what=""):
    """The listed tiles are ref's, bit for bit; every other element holds the sentinel.  Returns the buffer in tiles."""
    got, want = as_tiles(g.get(payload_written=False), w, h, world), as_tiles(ref, w, h, world)
    on = np.zeros(got.shape[0], dtype=bool)
    on[np.asarray(tiles)] = True
    assert on.sum() == len(tiles) and 0 < on.sum() <= on.size
    same(got[on], want[on], what + " listed tiles")
    assert np.all(got[~on] == SENTINEL), what + ": a tile that is not listed was written"
    ins = adaptiveref.inside(w, h)[adaptiveref.rank_tiles(w, h, rank, world)]
    assert not np.any(got[on][ins[on]] == SENTINEL), what + ": a listed pixel was left unwritten"
    return got


@functools.lru_cache(maxsize=None)
def cornell(pt):
    """cornell 96x54 (24 tiles), depth 8: the renderer, the oracle scene and pt_render_device's 4-spp frame."""
    ps, r, osc = renderer(pt, "cornell")
    w, h = 96, 54
    ref = device_frame(r, ps.camera(), w, h, 4)
    ref.setflags(write=False)
    return ps, r, osc, w, h, ref


def tile_pixels(w, h, tiles):
    tx, _ = adaptiveref.tiles_of(w, h)
    y, x = np.divmod(np.arange(w * h), w)
    return np.flatnonzero(np.isin((y // 16) * tx + x // 16, tiles)).astype(np.uint32)


# ---- 1. listed tiles on cornell ----

def test_listed_tiles_on_cornell(pt):
    ps, r, osc, w, h, ref = cornell(pt)
    g = listed(r, ps.camera(), w, h, 4, LIST8, 0, 4)
    assert r.last_builds()["engine"] == WAVE
    check_listed(g, ref, w, h, LIST8, what="cornell")
    px = tile_pixels(w, h, LIST8)
    assert px.size == 6 * 256 + 2 * 16 * 6  # tiles 22 and 23 are 16x6
    same(g.get(payload_written=False).reshape(-1, 3)[px], osc.render(w, h, 4, 8, SEED, pixels=px), "against the oracle")
    assert pt.march_guard_drops(r) == 0
    # a numpy array of another integer type is a list too
    g2 = listed(r, ps.camera(), w, h, 4, np.array(LIST8, dtype=np.int16), 0, 4)
    same(g2.get(payload_written=False), g.get(payload_written=False), "int16 list")


# ---- 2. chunking ----

@pytest.mark.parametrize("wf_paths,tiles", [(256, LIST8), (1024, LIST8), (1024, LIST8[:7])],
                         ids=["one-tile-chunks", "groups-of-4", "partial-last-group"])
def test_chunking(pt, wf_paths, tiles):
    """wf_paths 256: one tile and one sample per chunk, so every chunk's first position goes through the list; 1024:
    groups of 4 tiles, with 7 entries a last group of 3."""
    ps, _, _, w, h, ref = cornell(pt)
    r = pt.HipRenderer(ps, depth=8)
    r.set_option("wf_paths", wf_paths)
    g = listed(r, ps.camera(), w, h, 4, tiles, 0, 4)
    check_listed(g, ref, w, h, tiles, what="wf_paths %d" % wf_paths)


# ---- 3. windows over different lists ----

def test_windows_over_different_lists(pt):
    ps, r, _ = renderer(pt, "spheres")
    w, h, spp = 64, 64, 8
    A, B = [0, 3, 5, 6, 9, 10, 15], [3, 6, 10]
    cam = ps.camera()
    g = listed(r, cam, w, h, spp, A, 0, 3)
    sums = device_frame(r, cam, w, h, spp, s=(0, 3))
    check_listed(g, sums, w, h, A, what="window [0, 3)")
    listed(r, cam, w, h, spp, B, 3, 8, into=g)
    got = as_tiles(g.get(payload_written=False), w, h, 1)
    full = as_tiles(device_frame(r, cam, w, h, spp), w, h, 1)
    rest = [t for t in A if t not in B]
    same(got[B], full[B], "the tiles of both windows are the 8-sample frame's")
    same(got[rest], as_tiles(sums, w, h, 1)[rest], "the tiles of the first window alone keep its sums")
    off = [t for t in range(16) if t not in A]
    assert np.all(got[off] == SENTINEL)
    assert np.any(full[B] != as_tiles(sums, w, h, 1)[B])  # (the second window did something)


# ---- 4. partial tiles ----

def test_partial_tile_alone(pt):
    """20x13: tile 1 is the 4x13 tile."""
    ps, r, osc = renderer(pt, "spheres")
    w, h = 20, 13
    g = listed(r, ps.camera(), w, h, 4, [1], 0, 4)
    got = g.get(payload_written=False).reshape(h, w, 3)
    assert np.all(got[:, :16] == SENTINEL) and not np.any(got[:, 16:] == SENTINEL)
    px = tile_pixels(w, h, [1])
    assert px.size == 4 * 13
    same(got.reshape(-1, 3)[px], osc.render(w, h, 4, 8, SEED, pixels=px), "the 4x13 tile")


# ---- 5. shards ----

@pytest.mark.parametrize("world", [2, 3])
def test_shards(pt, world):
    ps, r, _, w, h, _ = cornell(pt)
    partial = 0
    for rank in range(world):
        n = r_tiles(w, h, rank, world)
        tiles = list(range(1, n, 2))
        ref = device_frame(r, ps.camera(), w, h, 4, rank, world)
        g = listed(r, ps.camera(), w, h, 4, tiles, 0, 4, rank, world)
        got = check_listed(g, ref, w, h, tiles, rank, world, what="rank %d of %d" % (rank, world))
        pad = ~adaptiveref.inside(w, h)[adaptiveref.rank_tiles(w, h, rank, world)]
        assert np.all(got[tiles][pad[tiles]] == 0.0)  # a listed partial tile's padding is zeroed, as in the frame
        partial += int(pad[tiles].any(axis=1).sum())
    assert partial >= 2  # the 16x6 tiles of the last row are among the listed ones


# ---- 6. the other kernel families ----

def test_marched_scene(pt):
    ps, r, _ = renderer(pt, None, text=scene_text("marched.json"))
    w, h = 32, 32
    ref = device_frame(r, ps.camera(), w, h, 2)
    g = listed(r, ps.camera(), w, h, 2, [0, 3], 0, 2)
    assert r.last_builds()["march"] is not None
    check_listed(g, ref, w, h, [0, 3], what="marched")
    assert pt.march_guard_drops(r) == 0


def test_split_engine(pt):
    from test_gpu_builds import FIELD, gpu_scene
    w, h, spp, depth, _ = FIELD
    ps = gpu_scene("field")
    r = pt.HipRenderer(ps, depth=depth)
    for k, v in {"engine": 2, "wf_bounce_waves": 3, "wf_walk": 5}.items():
        r.set_option(k, v)
    tiles = [0, 7, 8, 20, 23]
    ref = device_frame(r, ps.camera(), w, h, spp)
    assert r.last_builds()["walk"] is not None
    g = listed(r, ps.camera(), w, h, spp, tiles, 0, spp)
    assert r.last_builds()["walk"] is not None and r.last_builds()["engine"] == WAVE
    check_listed(g, ref, w, h, tiles, what="split engine")


def test_depth_65(pt):
    from test_gpu_builds import ROOM65, gpu_scene
    w, h, spp, depth, _ = ROOM65
    ps = gpu_scene("room-plain")
    r = pt.HipRenderer(ps, depth=depth)
    ref = device_frame(r, ps.camera(), w, h, spp)
    g = listed(r, ps.camera(), w, h, spp, [1, 2], 0, spp)
    assert r.last_builds()["bounce"][5] == 1  # a DEEP build
    check_listed(g, ref, w, h, [1, 2], what="depth 65")


# ---- 7. adaptive frames ----

def run(pt, r, cam, w, h, window, cap, threshold, rank=0, world=1, stream=0, **kw):
    """One adaptive frame into guarded buffers: (out, variance, tile_samples, tile_error, samples launched)."""
    import torch
    ntiles = pt.shard_tiles(w, h, rank, world)
    count = w * h * 3 if world == 1 else ntiles * 768
    assert pt.adaptive_workspace_doubles(w, h, rank, world) == 3 * count
    out, var, work = Guarded(count), Guarded(count), Guarded(3 * count, align16=True)
    ts, te = Guarded(ntiles, torch.int32, TS_SENTINEL), Guarded(ntiles)
    launched = r.render_adaptive_device(cam, w, h, cap, threshold, SEED, rank, world, out.ptr, var.ptr, ts.ptr, te.ptr,
                                        work.ptr, stream, window=window, **kw)
    work.get(payload_written=False)
    return out.get(), var.get(), ts.get().astype(np.uint32), te.get(), launched


def same_frames(a, b, what):
    for k, name in enumerate(("frame", "variance", "tile_samples", "tile_error")):
        same(a[k], b[k], "%s: %s" % (what, name))


@functools.lru_cache(maxsize=None)
def cornell_adaptive(pt):
    """The CORNELL frame of test_gpu_adaptive.py through the list and at merge_gap 0, with the launches of each."""
    ps, r, _, w, h, _ = cornell(pt)
    cam = ps.camera()
    before = r.render(cam, pt.ImageParams(w, h), 4, seed=11)
    pt.kernel_timing(r, True)
    lst = run(pt, r, cam, w, h, tile_list=True, **CORNELL)
    kt_list = pt.kernel_timing(r, True)
    gap0 = run(pt, r, cam, w, h, merge_gap=0, **CORNELL)
    kt_gap0 = pt.kernel_timing(r, False)
    after = r.render(cam, pt.ImageParams(w, h), 4, seed=11)
    return lst, gap0, kt_list, kt_gap0, before, after


def test_adaptive_list_equals_the_run_based_frame(pt):
    lst, gap0, _, _, before, after = cornell_adaptive(pt)
    same_frames(lst, gap0, "list against merge_gap 0")
    ts = lst[2]
    assert len(set(ts.tolist())) >= 4 and ts.min() < CORNELL["cap"] == ts.max()  # tiles stop at different windows
    pixels = adaptiveref.inside(96, 54).sum(axis=1)
    assert lst[4] == int(np.sum(pixels * ts.astype(np.int64)))  # exactly: no stopped tile is rendered again
    assert np.array_equal(before, after) and before.mean() > 0.01


def test_adaptive_list_is_one_launch_per_window(pt):
    import sys
    from conftest import ROOT
    sys.path.insert(0, str(ROOT / "tests" / "golden"))
    import make_wave_plans as G
    lst, _, kt_list, kt_gap0, _, _ = cornell_adaptive(pt)
    ts = lst[2].astype(np.int64)
    e = adaptiveref.edges(CORNELL["window"], CORNELL["cap"])
    rendered = [k for k in range(1, len(e)) if np.any(ts >= e[k])]  # a window is rendered while a tile is active
    assert len(rendered) == len(e) - 1  # (some tile runs to the cap)
    # on the host: each of these windows is one chunk at the default options
    subprocess.run(["make", "-s", "-C", str(ROOT / "tests" / "native"), "_build/libplan.so"], check=True)
    L = G.load(native_lib("libplan.so"))
    for k in rendered:
        inp = {"ntiles": int(np.sum(ts >= e[k])), "s_begin": e[k - 1], "s_end": e[k], "spp": CORNELL["cap"] + 1,
               "depth": 8, "progressive": 0, "textured": 0, "presel": 1, "wf_paths": 0, "wf_slots": 2,
               "wf_min_chunks": 1, "avail_bytes": G.UNKNOWN}
        assert len(G.evaluate(L, inp)["chunks"]) == 1, k
    print("launches, list:", {k: v[1] for k, v in kt_list.items()}, "merge_gap 0:", {k: v[1] for k, v in kt_gap0.items()})
    assert kt_list["reduce"][1] == len(rendered)
    assert kt_list["reduce"][1] < kt_gap0["reduce"][1]
    assert kt_list["megakernel"][1] == 0 and kt_gap0["megakernel"][1] == 0


@pytest.mark.parametrize("world", [2, 3])
def test_adaptive_list_shards_equal_the_whole_frame(pt, world):
    import torch
    ps, r, _, w, h, _ = cornell(pt)
    whole = cornell_adaptive(pt)[0]
    per = pt.shard_tiles(w, h, 0, world)
    gathered = {k: torch.zeros(world * per * 768, dtype=torch.float64, device="cuda") for k in ("out", "var")}
    frames = {k: torch.zeros(w * h * 3, dtype=torch.float64, device="cuda") for k in ("out", "var")}
    ts, te = np.zeros(24, dtype=np.uint32), np.zeros(24)
    for rank in range(world):
        out, var, s, e, launched = run(pt, r, ps.camera(), w, h, rank=rank, world=world, tile_list=True, **CORNELL)
        ids = adaptiveref.rank_tiles(w, h, rank, world)
        ts[ids], te[ids] = s, e
        ins = adaptiveref.inside(w, h)[ids]
        assert np.all(out.reshape(-1, 256, 3)[~ins] == 0.0) and np.all(var.reshape(-1, 256, 3)[~ins] == 0.0)
        assert launched == int(np.sum(ins.sum(axis=1) * s.astype(np.int64)))
        for k, a in (("out", out), ("var", var)):
            gathered[k][rank * per * 768: rank * per * 768 + a.size] = torch.from_numpy(a).cuda()
    for k in ("out", "var"):
        pt.unshard_device(gathered[k].data_ptr(), w, h, world, frames[k].data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(ts, whole[2])
    same(te, whole[3], "tile_error")
    same(frames["out"].cpu().numpy(), whole[0], "unsharded frame")
    same(frames["var"].cpu().numpy(), whole[1], "unsharded variance")


def test_adaptive_list_marched_frame(pt):
    ps, r, _ = renderer(pt, None, text=scene_text("marched.json"))
    a = run(pt, r, ps.camera(), 32, 32, 2, 6, 0.1, tile_list=True)
    b = run(pt, r, ps.camera(), 32, 32, 2, 6, 0.1, merge_gap=0)
    same_frames(a, b, "marched")
    assert a[4] == b[4] and pt.march_guard_drops(r) == 0


def test_adaptive_list_host_form_and_a_stream_of_the_callers(pt):
    import torch
    ps, r, _ = renderer(pt, "spheres")
    w, h = 64, 64
    cam = ps.camera()
    dev = run(pt, r, cam, w, h, 8, 24, 0.02, merge_gap=0)
    rgb, ts, te, var, launched = r.render_adaptive(cam, pt.ImageParams(w, h), 24, 0.02, seed=SEED, tile_list=True,
                                                   return_samples_rendered=True)
    same_frames((rgb, var, ts, te), dev, "host form")
    assert launched == dev[4] == int(np.sum(256 * ts.astype(np.int64))) and len(set(ts.tolist())) >= 2
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        b = run(pt, r, cam, w, h, 8, 24, 0.02, stream=st.cuda_stream, tile_list=True)
    same_frames(b, dev, "a stream of the caller's")


# ---- 8. errors ----

def test_errors_write_nothing(pt):
    import torch
    ps, r, _ = renderer(pt, "spheres")
    w, h = 64, 64
    cam = ps.camera()
    out = Guarded(w * h * 3)
    good = dict(w=w, h=h, spp=4, rank=0, world=1, s0=0, s1=4, tiles=[0, 5, 15], out=out.ptr)
    bad = [dict(out=0), dict(w=0), dict(h=0), dict(spp=0), dict(world=0), dict(rank=1), dict(s0=4), dict(s1=5),
           dict(s0=2, s1=1), dict(tiles=[]), dict(tiles=[0, 16]), dict(tiles=[5, 5]), dict(tiles=[5, 0]),
           dict(tiles=[0, 8], rank=1, world=2)]

    def call(a):
        return r.render_device_tiles(cam, a["w"], a["h"], a["spp"], SEED, a["rank"], a["world"], a["s0"], a["s1"],
                                     a["tiles"], a["out"])

    for case in bad:
        with pytest.raises(pt.PtError) as e:
            call(dict(good, **case))
        assert e.value.code == pt.PT_ERR_INVALID, case
    # the adaptive list entries: their own arguments
    count = w * h * 3
    aout, var, work = Guarded(count), Guarded(count), Guarded(3 * count, align16=True)
    ts, te = Guarded(16, torch.int32, TS_SENTINEL), Guarded(16)

    def adaptive(**kw):
        a = dict(cap=24, thr=0.1, out=aout.ptr, ts=ts.ptr, work=work.ptr, window=8, rank=0, world=1)
        a.update(kw)
        return r.render_adaptive_device(cam, w, h, a["cap"], a["thr"], SEED, a["rank"], a["world"], a["out"], var.ptr,
                                        a["ts"], te.ptr, a["work"], window=a["window"], tile_list=True)

    for case in (dict(out=0), dict(ts=0), dict(work=0), dict(work=work.ptr + 8), dict(cap=8), dict(window=0),
                 dict(thr=-1.0), dict(rank=1), dict(world=0)):
        with pytest.raises(pt.PtError) as e:
            adaptive(**case)
        assert e.value.code == pt.PT_ERR_INVALID, case
    with pytest.raises(pt.PtError) as e:
        r.render_adaptive(cam, pt.ImageParams(w, h), 8, 0.1, tile_list=True)
    assert e.value.code == pt.PT_ERR_INVALID
    # a progressive frame in flight: PT_ERR_STATE
    r.start_rendering(cam, pt.ImageParams(w, h), 2, SEED)
    for f in (lambda: call(good), adaptive):
        with pytest.raises(pt.PtError) as e:
            f()
        assert e.value.code == pt.PT_ERR_STATE
    r.stop_rendering()
    torch.cuda.synchronize()
    assert all(b.untouched() for b in (out, aout, var, work, ts, te))
    assert GUARD > 0
