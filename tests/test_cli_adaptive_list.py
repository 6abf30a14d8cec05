"""tools/pt_render scene MAX_SPP w h -A THRESHOLD -L: the adaptive frame with each window rendered in one launch over
the list of the still-active tiles (pt_render_adaptive_list).  The usage errors run on the CPU; the render needs the
GPU and writes the files of the run without -L, bit for bit."""
import subprocess

import numpy as np
import pytest

from conftest import ROOT

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
    assert "-A" in r.stderr and "-L" in r.stderr, args


def test_usage_errors(exe, tmp_path):
    usage_error(exe, ["-L"])                                    # -L belongs to -A
    usage_error(exe, ["-L", "-B", "8"])
    usage_error(exe, ["-L", "-o", str(tmp_path / "f.png")])
    usage_error(exe, ["-L", "-V", str(tmp_path / "v.f64")])     # the uniform frame's variance has no list
    usage_error(exe, ["-A", "0.1", "-L", "-c", str(tmp_path / "c.ckpt"), "-n", "2"])  # -A's own rules hold with -L
    usage_error(exe, ["-A", "0.1", "-L", "-W", "4"])
    usage_error(exe, ["-A", "-L"])                              # -A's value is no number
    assert not list(tmp_path.iterdir())


@pytest.mark.gpu
def test_L_writes_the_same_frame_and_tile_counts(exe, tmp_path):
    w, h, cap = 96, 54, 128  # tests/test_gpu_adaptive.py's CORNELL frame: its tiles stop at different windows
    scene = ROOT / "scenes" / "cornell_box.json"
    base = [exe, str(scene), str(cap), str(w), str(h), "-d", "8", "-s", "3", "-A", "0.2"]
    runs = {}
    for name, extra in (("runs", []), ("list", ["-L"])):
        r = subprocess.run(base + extra + ["-o", str(tmp_path / (name + ".png")), "-f", str(tmp_path / (name + ".f64")),
                                           "-M", str(tmp_path / (name + ".u32")), "-V", str(tmp_path / (name + ".var"))],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert "pixel-samples rendered" in r.stderr
        runs[name] = (np.fromfile(tmp_path / (name + ".f64")), np.fromfile(tmp_path / (name + ".u32"), dtype=np.uint32),
                      np.fromfile(tmp_path / (name + ".var")), (tmp_path / (name + ".png")).read_bytes(),
                      int(r.stderr.split("pt_render: ")[1].split(" of ")[0]))
    a, b = runs["runs"], runs["list"]
    assert a[0].size == w * h * 3 and a[1].size == 24 and len(set(a[1].tolist())) >= 2 and np.all(np.isfinite(a[0]))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3]
    pixels = np.array([256] * 18 + [96] * 6)  # three rows of 16x16 tiles and one of 16x6
    assert b[4] == int((pixels * b[1]).sum()) <= a[4]  # the list renders no stopped tile again
