"""What the deep-path tests share (test_gpu_deep.py, test_deep_host.py, test_deep_plan.py): the closed room of
scenes/deep_room.py on the import path, and the parity bar of the GPU tests, the rule of tests/test_gpu_parity.py's
check_image restated here so that these tests stand on their own: every pixel bit-exact, and the per-channel RMS on
linear radiance within 1e-4."""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "scenes"))
import deep_room  # noqa: E402,F401

RMS_TOL = 1e-4


def rms(a, b):
    return np.sqrt(np.mean((a - b) ** 2, axis=0))


def check_image(img, ref):
    assert np.all(np.isfinite(img))
    assert np.all(rms(img, ref) <= RMS_TOL), rms(img, ref)
    exact = np.mean(np.all(img == ref, axis=1))
    assert exact == 1.0, "bit-exact pixels: %.6f" % exact
