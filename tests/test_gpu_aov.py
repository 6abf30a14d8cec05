"""The guide-plane pass on the MI355X (aov_tiles, rs-pathtracing_amd/csrc/pt_aov.hip) through the Python mirror:
whole frames and a compact shard against the planes tests/aovref.py computes from the oracle's pieces (bit for bit;
the textured scene within the project's frame tolerance), a large tree, single planes, the identity that ties the
planes' jitter to the beauty frame's without the oracle, and that the pass leaves the renderer as it found it."""
import json

import numpy as np
import pytest

import aovref
import oracle as O
from conftest import ROOT

pytestmark = pytest.mark.gpu

SEED = aovref.FRAME_SEED


def renderer(pt, name, depth=8):
    text, rs, w, h, spp, _, ref = aovref.case(name)
    ps = pt.Scene.from_json(text, random_spheres=rs, seed=1)
    return ps, pt.HipRenderer(ps, depth=depth), w, h, spp, ref


@pytest.mark.parametrize("name", ["spheres", "cornell", "marched", "light"])
def test_whole_frame_equals_the_oracle(pt, name):
    ps, r, w, h, spp, ref = renderer(pt, name)
    none, full, part = aovref.coverage_kinds(ref["depth"])
    assert none >= 100 and full >= 100 and part >= 10, (none, full, part)
    got = r.render_aov(ps.camera(), pt.ImageParams(w, h), spp, seed=SEED)
    aovref.same_planes(got, ref)
    if name == "light":
        assert np.all(got["albedo"][got["depth"][:, 1] == 1.0] == 15.0)  # the emit, not clamped
    assert pt.march_guard_drops(r) == 0


def test_textured_within_the_frame_tolerance(pt, monkeypatch):
    monkeypatch.chdir(ROOT)  # (the scene's image texture is named relative to the repository)
    ps, r, w, h, spp, ref = renderer(pt, "textured")
    aovref.assert_not_degenerate(ref["depth"])
    aovref.close_planes(r.render_aov(ps.camera(), pt.ImageParams(w, h), spp, seed=SEED), ref)


def test_cornell_rank_1_of_3_compact_shards(pt):
    import torch
    ps, r, w, h, spp, ref = renderer(pt, "cornell")
    rank, world = 1, 3
    per = pt.shard_tiles(w, h, 0, world)
    bufs = [torch.full((per * 256 * 3,), -7.25, dtype=torch.float64, device="cuda") for _ in range(3)]
    r.render_aov_device(ps.camera(), w, h, spp, SEED, rank, world, *[b.data_ptr() for b in bufs],
                        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    idx = pt.shard_pixels(w, h, rank, world)
    ok = idx >= 0
    assert ok.sum() >= w * h // world - 256 and (~ok).sum() > 0  # 54 rows: the last tile row is padded
    for name, b in zip(aovref.PLANES, bufs):
        got = b.view(-1, 3).cpu().numpy()[: len(idx)]
        bad = np.flatnonzero(np.any(got[ok] != ref[name][idx[ok]], axis=1))
        assert bad.size == 0, (name, bad[:8].tolist())
        assert np.all(got[~ok] == 0.0), name  # pixels outside the frame


def test_large_tree(pt):
    """The 32-byte nodes of a tree the render path walks in its quantized form: closest_hit_probe's build takes
    it as it is."""
    import make_scenes  # (scenes/ is on the path: aovref)
    text = json.dumps(make_scenes.synthetic(20000))
    w, h, spp = 64, 36, 2
    ps = pt.Scene.from_json(text, seed=1)
    r = pt.HipRenderer(ps, depth=8)
    assert r.get_option("bvh_nodes") >= 1 << 15, "not the large-tree build"
    ref = aovref.planes(O.Scene(text, seed=1).use_bvh(True, 7), w, h, spp, SEED)
    assert aovref.coverage_kinds(ref["depth"])[1] >= 100
    aovref.same_planes(r.render_aov(ps.camera(), pt.ImageParams(w, h), spp, seed=SEED), ref)


def test_normal_alone(pt):
    """Only the normal's pointer: the plane is the three-plane call's, and memory the call was not given stays as
    it was."""
    import torch
    ps, r, w, h, spp, ref = renderer(pt, "cornell")
    n = w * h * 3
    normal = torch.zeros(n, dtype=torch.float64, device="cuda")
    others = [torch.full((n,), -7.25, dtype=torch.float64, device="cuda") for _ in range(2)]
    r.render_aov_device(ps.camera(), w, h, spp, SEED, 0, 1, 0, normal.data_ptr(), 0,
                        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    three = r.render_aov(ps.camera(), pt.ImageParams(w, h), spp, seed=SEED)
    assert np.array_equal(normal.view(-1, 3).cpu().numpy(), three["normal"])
    aovref.same_planes(three, ref)
    for b in others:
        assert bool(torch.all(b == -7.25))
    one = r.render_aov(ps.camera(), pt.ImageParams(w, h), spp, seed=SEED, planes=("depth",))
    assert list(one) == ["depth"] and np.array_equal(one["depth"], three["depth"])


def test_jitter_is_the_beauty_frames(pt, spheres_text):
    """Without the oracle: a depth-0 frame is the sky where a sample misses and black where it hits, sample by
    sample, so it equals the albedo plane wherever no sample hits and is exactly 0 wherever all do, only if the
    pass casts the frame's own camera rays."""
    w, h, spp = 64, 64, 4
    ps = pt.Scene.from_json(spheres_text, seed=1)
    r0 = pt.HipRenderer(ps, depth=0)
    beauty = r0.render(ps.camera(), pt.ImageParams(w, h), spp, seed=SEED)
    got = r0.render_aov(ps.camera(), pt.ImageParams(w, h), spp, seed=SEED)
    cov = got["depth"][:, 1]
    assert np.sum(cov == 0.0) >= 100 and np.sum(cov == 1.0) >= 100 and np.sum((cov > 0) & (cov < 1)) >= 10
    assert np.array_equal(beauty[cov == 0.0], got["albedo"][cov == 0.0])
    assert np.all(beauty[cov == 1.0] == 0.0)
    part = (cov > 0.0) & (cov < 1.0)  # an edge pixel: some of the sky's samples, so darker than the whole sky
    assert np.all(beauty[part].sum(axis=1) > 0.0)


def test_the_pass_leaves_the_renderer_alone(pt):
    ps, r, w, h, _, _ = renderer(pt, "cornell", depth=8)
    r.set_option("engine", 2)
    opts = r.options()
    cam, ip = ps.camera(), pt.ImageParams(w, h)
    first = r.render(cam, ip, 8, seed=11)
    planes = r.render_aov(cam, ip, 8, seed=11)
    again = r.render(cam, ip, 8, seed=11)
    assert np.array_equal(first, again) and first.mean() > 0.01
    assert np.all(np.isfinite(planes["albedo"]))
    assert r.options() == opts
    assert pt.march_guard_drops(r) == 0


def test_argument_errors(pt):
    import torch
    ps, r, w, h, spp, _ = renderer(pt, "cornell")
    cam = ps.camera()
    buf = torch.zeros(w * h * 3, dtype=torch.float64, device="cuda")
    with pytest.raises(pt.PtError) as e:
        r.render_aov_device(cam, w, h, spp, SEED, 0, 1, 0, 0, 0)
    assert e.value.code == pt.PT_ERR_INVALID
    with pytest.raises(pt.PtError) as e:
        r.render_aov_device(cam, w, h, spp, SEED, 3, 3, buf.data_ptr(), 0, 0)
    assert e.value.code == pt.PT_ERR_INVALID
    for bad in [(0, h, spp), (w, 0, spp), (w, h, 0)]:
        with pytest.raises(pt.PtError) as e:
            r.render_aov_device(cam, bad[0], bad[1], bad[2], SEED, 0, 1, buf.data_ptr(), 0, 0)
        assert e.value.code == pt.PT_ERR_INVALID
    r.start_rendering(cam, pt.ImageParams(w, h), 2, seed=1)
    try:
        with pytest.raises(pt.PtError) as e:
            r.render_aov(cam, pt.ImageParams(w, h), spp, seed=SEED)
        assert e.value.code == pt.PT_ERR_STATE
        with pytest.raises(pt.PtError) as e:
            r.render_aov_device(cam, w, h, spp, SEED, 0, 1, buf.data_ptr(), 0, 0)
        assert e.value.code == pt.PT_ERR_STATE
    finally:
        r.stop_rendering()
    torch.cuda.synchronize()
    assert bool(torch.all(buf == 0.0))  # no refused call wrote anything
