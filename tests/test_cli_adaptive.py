"""tools/pt_render scene MAX_SPP w h -A THRESHOLD [-B window] [-M tiles.u32]: an adaptive frame through
pt_render_adaptive, the per-tile sample counts as uint32, and with -A the -V plane and the -D denoiser on the adaptive
frame's variance plane.  The usage errors run on the CPU; the renders need the GPU."""
import subprocess

import numpy as np
import pytest

import varianceref
from conftest import ROOT
from test_image_io import read_png

EXE = ROOT / "tools" / "pt_render"


@pytest.fixture(scope="module")
def exe():
    import fcntl
    with open(ROOT / "tools" / ".build.lock", "w") as lk:  # pytest-xdist workers: one make at a time
        fcntl.flock(lk, fcntl.LOCK_EX)
        subprocess.run(["make", "-s", "-C", str(ROOT / "tools"), "pt_render"], check=True)
    return str(EXE)


def usage_error(exe, args):
    r = subprocess.run([exe, "a.json", "64"] + args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "usage" in r.stderr, args
    assert "-A" in r.stderr and "-B" in r.stderr and "-M" in r.stderr, args


def test_A_with_a_checkpoint_is_a_usage_error(exe, tmp_path):
    usage_error(exe, ["-A", "0.1", "-c", str(tmp_path / "c.ckpt"), "-n", "2"])
    assert not (tmp_path / "c.ckpt").exists()


def test_usage_errors(exe, tmp_path):
    usage_error(exe, ["-A"])                                    # no value
    usage_error(exe, ["-A", "soon"])                            # not a number
    usage_error(exe, ["-A", "0.1x"])
    usage_error(exe, ["-A", "0.1", "-B"])
    usage_error(exe, ["-A", "0.1", "-M"])
    usage_error(exe, ["-B", "8"])                               # -B and -M belong to -A
    usage_error(exe, ["-M", str(tmp_path / "t.u32")])
    usage_error(exe, ["-A", "0.1", "-V", str(tmp_path / "v.f64"), "-W", "4"])  # -W is the uniform frame's
    assert not list(tmp_path.iterdir())


@pytest.mark.gpu
def test_adaptive_frame_tile_map_variance_and_denoise(exe, pt, tmp_path):
    w, h, cap = 64, 64, 32
    scene = ROOT / "scenes" / "spheres.json"
    base = [exe, str(scene), str(cap), str(w), str(h), "-d", "8", "-s", "3", "-o", str(tmp_path / "f.png")]
    r = subprocess.run(base + ["-A", "0.02", "-f", str(tmp_path / "f.f64"), "-M", str(tmp_path / "t.u32"),
                               "-V", str(tmp_path / "v.f64"), "-a", str(tmp_path / "OUT"),
                               "-D", str(tmp_path / "clean.png")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "pixel-samples rendered" in r.stderr
    frame = np.fromfile(tmp_path / "f.f64").reshape(w * h, 3)
    var = np.fromfile(tmp_path / "v.f64").reshape(w * h, 3)
    tiles = np.fromfile(tmp_path / "t.u32", dtype=np.uint32)
    ps = pt.Scene.from_json(scene.read_text(), seed=1)
    rr = pt.HipRenderer(ps, depth=8)
    rgb, ts, _, v = rr.render_adaptive(ps.camera(), pt.ImageParams(w, h), cap, 0.02, seed=3)
    assert np.array_equal(tiles, ts) and tiles.size == 16 and len(set(tiles.tolist())) >= 2
    assert np.array_equal(frame, rgb) and np.array_equal(var, v)
    gw, gh, px = read_png(tmp_path / "f.png")
    assert (gw, gh) == (w, h) and np.array_equal(px, pt.encode_rgba8(frame))
    # -D with -A: the variance-guided denoiser on the adaptive frame's own plane
    planes = np.fromfile(tmp_path / "OUT.aov.f64").reshape(3, w * h, 3)
    clean = np.fromfile(tmp_path / "clean.png.f64").reshape(w * h, 3)
    assert np.array_equal(clean, varianceref.denoise_variance(frame, planes[0], planes[1], planes[2], var, w, h))
    # -B 4: other windows, another map; -M alone
    r = subprocess.run(base + ["-A", "0.02", "-B", "4", "-M", str(tmp_path / "t4.u32")], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    _, ts4, _, _ = rr.render_adaptive(ps.camera(), pt.ImageParams(w, h), cap, 0.02, window=4, seed=3)
    assert np.array_equal(np.fromfile(tmp_path / "t4.u32", dtype=np.uint32), ts4) and ts4.min() == 8
    # inf: every tile at the second window
    r = subprocess.run(base + ["-A", "inf", "-M", str(tmp_path / "ti.u32")], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    assert np.all(np.fromfile(tmp_path / "ti.u32", dtype=np.uint32) == 16)
    # a cap the library refuses (not above the window): status 1 with its message
    r = subprocess.run([exe, str(scene), "8", str(w), str(h), "-d", "8", "-A", "0.1", "-o", str(tmp_path / "g.png")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "max_samples" in r.stderr
