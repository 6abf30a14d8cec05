"""Writes tests/golden/variance_spheres_ref.npy: the converged frame tests/test_variance_host.py measures the
variance-guided denoiser's error and the variance estimate against (cornell's is denoise_cornell_ref.npy).
spheres.json with its random spheres (scene seed 1), 64x64, 2048 spp, depth 8, frame seed 77, from the CPU oracle:
(64*64, 3) float64, 96 KB.  Under a minute on 16 CPUs; the frame is deterministic, so a rerun writes the same bytes.

    python tests/golden/make_variance_ref.py
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT / "oracle"))

W, H, SPP, DEPTH, SEED = 64, 64, 2048, 8, 77


def main():
    import oracle as O
    osc = O.Scene((ROOT / "scenes" / "spheres.json").read_text(), random_spheres=True, seed=1)
    ref = osc.render(W, H, SPP, DEPTH, SEED)
    assert ref.shape == (W * H, 3) and np.all(np.isfinite(ref))
    np.save(Path(__file__).resolve().parent / "variance_spheres_ref.npy", ref)
    print("wrote variance_spheres_ref.npy: mean", ref.mean(0))


if __name__ == "__main__":
    main()
