"""tools/pt_render -D PATH: the frame denoised on the device with its guide planes, as a PNG (and the linear frame
with -f).  The usage error runs on the CPU; the render needs the GPU."""
import subprocess

import numpy as np
import pytest

import denoiseref
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


def test_bare_D_is_a_usage_error(exe):
    r = subprocess.run([exe, "a.json", "-D"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "usage" in r.stderr and "-D" in r.stderr


@pytest.mark.gpu
def test_denoised_frame_and_image(exe, pt, tmp_path):
    """PATH.f64 is the restatement on the CLI's own -f and -a raw outputs, the PNG is its display encode, -o and -f
    still hold the noisy frame, and without -a the planes are rendered for the denoiser alone."""
    w, h, spp = 64, 64, 2
    base = [exe, str(ROOT / "scenes" / "spheres.json"), str(spp), str(w), str(h), "-d", "8", "-s", "3"]
    r = subprocess.run(base + ["-a", str(tmp_path / "OUT"), "-o", str(tmp_path / "f.png"), "-f", str(tmp_path / "f.f64"),
                               "-D", str(tmp_path / "clean.png")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    noisy = np.fromfile(tmp_path / "f.f64").reshape(w * h, 3)
    planes = np.fromfile(tmp_path / "OUT.aov.f64").reshape(3, w * h, 3)  # albedo, normal, depth
    clean = np.fromfile(tmp_path / "clean.png.f64").reshape(w * h, 3)
    want = denoiseref.denoise(noisy, planes[0], planes[1], planes[2], w, h)
    assert np.array_equal(clean, want) and np.any(clean != noisy)
    gw, gh, px = read_png(tmp_path / "clean.png")
    assert (gw, gh) == (w, h) and np.array_equal(px, pt.encode_rgba8(clean))
    nw, nh, npx = read_png(tmp_path / "f.png")
    assert (nw, nh) == (w, h) and np.array_equal(npx, pt.encode_rgba8(noisy))  # -o is the noisy frame
    # without -a and -f: the same image, nothing else written
    r = subprocess.run(base + ["-o", str(tmp_path / "g.png"), "-D", str(tmp_path / "alone.png")], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert read_png(tmp_path / "alone.png")[2].tobytes() == px.tobytes()
    assert not (tmp_path / "alone.png.f64").exists()
