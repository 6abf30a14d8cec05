"""tools/pt_render -V PATH [-W windows]: the variance plane of the frame's own sample windows as linear f64, the
frame unchanged; with -D the denoiser's variance term.  The usage errors run on the CPU; the renders need the GPU."""
import subprocess

import numpy as np
import pytest

import denoiseref
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


def test_V_with_a_checkpoint_is_a_usage_error(exe, tmp_path):
    r = subprocess.run([exe, "a.json", "8", "-V", str(tmp_path / "v.f64"), "-c", str(tmp_path / "c.ckpt"), "-n", "2"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "usage" in r.stderr and "-V" in r.stderr and "-W" in r.stderr
    assert not (tmp_path / "v.f64").exists() and not (tmp_path / "c.ckpt").exists()


def test_bare_V_and_W_are_usage_errors(exe):
    for flag in ("-V", "-W"):
        r = subprocess.run([exe, "a.json", flag], capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and "usage" in r.stderr


@pytest.mark.gpu
def test_variance_plane_and_guided_denoise(exe, pt, tmp_path):
    """-V writes the plane pt_render_variance gives (8 windows by default, -W otherwise), -f is the frame of a run
    without -V bit for bit, and -D with -V is the restatement's variance-guided frame on the CLI's own raw outputs."""
    w, h, spp = 64, 64, 16
    scene = ROOT / "scenes" / "spheres.json"
    base = [exe, str(scene), str(spp), str(w), str(h), "-d", "8", "-s", "3", "-o", str(tmp_path / "f.png")]
    r = subprocess.run(base + ["-f", str(tmp_path / "plain.f64")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    r = subprocess.run(base + ["-f", str(tmp_path / "f.f64"), "-V", str(tmp_path / "v.f64"), "-a", str(tmp_path / "OUT"),
                               "-D", str(tmp_path / "clean.png")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    frame = np.fromfile(tmp_path / "f.f64").reshape(w * h, 3)
    var = np.fromfile(tmp_path / "v.f64").reshape(w * h, 3)
    assert np.array_equal(frame, np.fromfile(tmp_path / "plain.f64").reshape(w * h, 3))
    ps = pt.Scene.from_json(scene.read_text(), seed=1)
    rr = pt.HipRenderer(ps, depth=8)
    rgb8, var8 = rr.render_variance(ps.camera(), pt.ImageParams(w, h), spp, seed=3, windows=8)
    assert np.array_equal(frame, rgb8) and np.array_equal(var, var8) and np.mean(var > 0.0) > 0.5
    planes = np.fromfile(tmp_path / "OUT.aov.f64").reshape(3, w * h, 3)
    clean = np.fromfile(tmp_path / "clean.png.f64").reshape(w * h, 3)
    want = varianceref.denoise_variance(frame, planes[0], planes[1], planes[2], var, w, h)
    assert np.array_equal(clean, want)
    assert np.any(clean != denoiseref.denoise(frame, planes[0], planes[1], planes[2], w, h))
    gw, gh, px = read_png(tmp_path / "clean.png")
    assert (gw, gh) == (w, h) and np.array_equal(px, pt.encode_rgba8(clean))
    # -W 4: another plane, the same frame
    r = subprocess.run(base + ["-f", str(tmp_path / "g.f64"), "-V", str(tmp_path / "v4.f64"), "-W", "4"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    _, var4 = rr.render_variance(ps.camera(), pt.ImageParams(w, h), spp, seed=3, windows=4)
    got4 = np.fromfile(tmp_path / "v4.f64").reshape(w * h, 3)
    assert np.array_equal(got4, var4) and np.any(got4 != var)
    assert np.array_equal(np.fromfile(tmp_path / "g.f64").reshape(w * h, 3), frame)
    # a window count the library refuses: status 1 with its message
    r = subprocess.run(base + ["-V", str(tmp_path / "bad.f64"), "-W", "1"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "windows" in r.stderr
