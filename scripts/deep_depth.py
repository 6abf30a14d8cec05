"""What deep frames (depth > 64) cost: frame times over the depth, and the price of queueing depth + 2 iterations
per chunk whether or not a path is still alive (launch_render_wave has no early-out).

    python scripts/deep_depth.py [--reps 5]        (section 2 of profiles/r7/deep_depth.txt)

Two scenes at 1600x900, 1 spp: the closed room of scenes/deep_room.py (paths end on the lamp or at depth 0 only) and
scenes/cornell_box.json.  Per depth: the frame's wall time (median of --reps), and from the per-kernel HIP events of
one more frame on one chunk stream (pt_kernel_timing, wf_slots=1: every launch alone on the device) the kernel time
per kind.

The iterations with no live path: L is the first depth whose frame equals the deepest frame's bit for bit (no path
was cut at depth 0, so every path ended within L bounces; found by bisection).  Between two depths above L only
empty iterations are added, so their cost per iteration is the difference of the kernel times (and of the wall
times) over the difference of the depths; a frame of depth D > L spends (D - L) of them."""
import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scenes"))
import deep_room  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402

DEPTHS = (50, 65, 128, 500, 1000)
W, H, SPP, SEED = 1600, 900, 1, 3


def frame(pt, scene, depth, timing=False, reps=1):
    r = pt.HipRenderer(scene, depth=depth)
    cam, ip = scene.camera(), pt.ImageParams(W, H)
    if timing:
        r.set_option("wf_slots", 1)
        r.render(cam, ip, SPP, seed=SEED)
        pt.kernel_timing(r, True)
        img = r.render(cam, ip, SPP, seed=SEED)
        return img, pt.kernel_timing(r, False)
    img = r.render(cam, ip, SPP, seed=SEED)  # warm-up: the workspace, the code objects
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        img = r.render(cam, ip, SPP, seed=SEED)
        ts.append((time.perf_counter() - t) * 1e3)
    return img, ts


def longest_path(pt, scene, deepest):
    """The first depth whose frame equals the deepest frame's (None: paths are still cut at deepest - 1)."""
    ref, _ = frame(pt, scene, deepest)
    if not np.array_equal(frame(pt, scene, deepest - 1)[0], ref):
        return None
    lo, hi = 0, deepest - 1  # frame(hi) == ref
    while lo < hi:
        mid = (lo + hi) // 2
        if np.array_equal(frame(pt, scene, mid)[0], ref):
            hi = mid
        else:
            lo = mid + 1
    return lo


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    pt = load_package()
    print(pt.version())
    scenes = {"room": pt.Scene.from_json(deep_room.room_json("plain"), random_spheres=False, seed=1),
              "room+heart": pt.Scene.from_json(deep_room.room_json("heart"), random_spheres=False, seed=1),
              "cornell": pt.Scene.from_json((ROOT / "scenes" / "cornell_box.json").read_text(), seed=1)}
    for name, sc in scenes.items():
        print("\n== %s, %dx%d at %d spp (%d paths)" % (name, W, H, SPP, W * H * SPP))
        print("depth  frame ms (median, min..max)   kernel ms on one stream: bounce march select reduce+unwind "
              "megakernel | sum   launches")
        wall, kern = {}, {}
        for d in DEPTHS:
            _, ts = frame(pt, sc, d, reps=a.reps)
            _, kt = frame(pt, sc, d, timing=True)
            wall[d] = statistics.median(ts)
            k = {n: kt[n][0] for n in ("bounce", "march", "select")}
            k["reduce"] = kt["reduce"][0] + kt["unwind"][0]
            k["mega"] = kt["megakernel"][0]  # (a small frame without marched shapes up to depth 64: engine auto)
            kern[d] = sum(k.values())
            print("%5d  %9.2f (%.2f..%.2f)   %9.2f %9.2f %9.2f %9.2f %9.2f | %9.2f   %d" % (
                d, wall[d], min(ts), max(ts), k["bounce"], k["march"], k["select"], k["reduce"], k["mega"], kern[d],
                sum(v[1] for v in kt.values())))
        L = longest_path(pt, sc, DEPTHS[-1])
        if L is None:
            print("paths are still cut at depth %d: no iteration of these frames is empty (share 0 at every depth)"
                  % (DEPTHS[-1] - 1))
            continue
        print("longest path: %d bounces (the frame stops changing at depth %d)" % (L, L))
        above = [d for d in DEPTHS if d > L]
        if len(above) < 2:
            print("fewer than two measured depths above it: no empty-iteration cost from these frames")
            continue
        d0, d1 = above[0], above[-1]
        ck, cw = (kern[d1] - kern[d0]) / (d1 - d0), (wall[d1] - wall[d0]) / (d1 - d0)
        print("an empty iteration (between depths %d and %d): %.2f us of kernel time, %.2f us of frame time" % (
            d0, d1, ck * 1e3, cw * 1e3))
        for d in above:
            print("depth %5d: %4d empty iterations, %.1f %% of the kernel time, %.1f %% of the frame time" % (
                d, d - L, 100 * ck * (d - L) / kern[d], 100 * cw * (d - L) / wall[d]))


if __name__ == "__main__":
    main()
