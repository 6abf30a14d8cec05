"""tools/pt_render -a PREFIX: the guide planes of the frame as three PNGs (and the raw planes with -f).  The usage
error runs on the CPU; the render needs the GPU."""
import subprocess

import numpy as np
import pytest

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


def test_bare_a_is_a_usage_error(exe):
    r = subprocess.run([exe, "a.json", "-a"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "usage" in r.stderr and "-a" in r.stderr


@pytest.mark.gpu
def test_planes_as_images(exe, tmp_path):
    w, h, spp = 64, 64, 2
    r = subprocess.run([exe, str(ROOT / "scenes" / "spheres.json"), str(spp), str(w), str(h), "-a",
                        str(tmp_path / "OUT"), "-o", str(tmp_path / "f.png"), "-f", str(tmp_path / "f.f64")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    planes = np.fromfile(tmp_path / "OUT.aov.f64").reshape(3, w * h, 3)  # albedo, normal, depth
    cov = planes[2][:, 1]
    assert np.sum(cov == 0.0) >= 100 and np.sum(cov == 1.0) >= 100
    img = {}
    for name in ("albedo", "normal", "depth"):
        gw, gh, px = read_png(tmp_path / ("OUT.%s.png" % name))
        assert (gw, gh) == (w, h) and np.all(px[:, 3] == 255)
        img[name] = px[:, :3]
    sky = cov == 0.0
    assert np.all(img["normal"][sky] == 127)  # (0 + 1) / 2 * 255.999
    assert np.all(img["depth"][sky] == 0)
    # the encodings, from the raw planes
    hit = cov > 0.0
    want_n = np.clip((planes[1] + 1.0) / 2.0 * 255.999, 0, 255).astype(np.uint8)
    assert np.array_equal(img["normal"], want_n)
    mean_t = np.where(hit, planes[2][:, 0] / np.where(hit, cov, 1.0), 0.0)
    want_d = (mean_t / mean_t.max() * 255.999).astype(np.uint8)
    want_d[mean_t == mean_t.max()] = 255
    assert np.array_equal(img["depth"], np.repeat(want_d[:, None], 3, axis=1))
    assert img["depth"][hit].max() == 255 and np.all(img["albedo"][sky].max(axis=1) > 0)  # the sky is not black
    assert (tmp_path / "f.png").exists()
