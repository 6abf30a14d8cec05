"""Writes tests/golden/denoise_cornell_ref.npy: the converged frame tests/test_denoise_host.py measures the denoiser's
error against.  cornell_box (scene seed 1), 96x54, 1024 spp, depth 8, frame seed 77, from the CPU oracle: (96*54, 3)
float64, 124 KB.  About half a minute on 16 CPUs; the frame is deterministic, so a rerun writes the same bytes.

    python tests/golden/make_denoise_ref.py
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT / "oracle"))

W, H, SPP, DEPTH, SEED = 96, 54, 1024, 8, 77


def main():
    import oracle as O
    osc = O.Scene((ROOT / "scenes" / "cornell_box.json").read_text(), random_spheres=True, seed=1)
    ref = osc.render(W, H, SPP, DEPTH, SEED)
    assert ref.shape == (W * H, 3) and np.all(np.isfinite(ref))
    np.save(Path(__file__).resolve().parent / "denoise_cornell_ref.npy", ref)
    print("wrote denoise_cornell_ref.npy: mean", ref.mean(0))


if __name__ == "__main__":
    main()
