"""What temporal accumulation costs and what it buys, on one MI355X.

Time: cornell_box at 1920x1080.  After a warm-up of each, five rounds of: the 1-spp depth-50 frame (what an
orbiting viewer renders per frame), its guide planes at 1 sample, the pass on its first frame, the pass in its steady
state (two cameras 1 degree apart, their frames and histories alternating, so every call reprojects through real
bilinear taps), and the denoiser (5 iterations, the defaults); each timed with device events on the stream, the two
pass builds and the denoiser as batches of --batch calls, so a window is not a fraction of a millisecond.  Beside
the times it prints the floor the pass cannot beat: the bytes it must move once (three frames in, the pixel's two
history records in, the frame and two records out; the first frame reads no history) over the device's measured copy
rate.

Quality: cornell_box, depth 8, 1 spp per frame, --frames frames (16) orbiting 1 degree per frame about the vertical
axis through the point the scene camera looks at (the first hit of its axis), ending on the scene's own camera, and
the same with a still camera.  The RMS of the linear difference of the last frame from a converged frame at that
camera (--converged spp, another seed), four ways: raw, accumulated, denoised, accumulated then denoised; and the
share of pixels that reset, per frame.  One row per setting: the starting defaults, max_count 8, 16 and 64,
sigma_depth 0.05 and 0.2, sigma_normal 0.25.  Prints one JSON line (profiles/r15/temporal.txt is this script's
output):

    python scripts/temporal_bench.py [--rounds 5] [--batch 20] [--frames 16] [--qwidth 960 --qheight 540]

Needs a GPU (there is no fallback)."""
import argparse
import json
import math
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

COPY_TBPS = 6.29  # the device's measured copy rate (read + write bytes over time), as in denoise_bench.py
SETTINGS = [
    ("start", dict(max_count=32, sigma_normal=0.5, sigma_depth=0.1)),
    ("max_count_8", dict(max_count=8, sigma_normal=0.5, sigma_depth=0.1)),
    ("max_count_16", dict(max_count=16, sigma_normal=0.5, sigma_depth=0.1)),
    ("max_count_64", dict(max_count=64, sigma_normal=0.5, sigma_depth=0.1)),
    ("sigma_depth_0.05", dict(max_count=32, sigma_normal=0.5, sigma_depth=0.05)),
    ("sigma_depth_0.2", dict(max_count=32, sigma_normal=0.5, sigma_depth=0.2)),
    ("sigma_normal_0.25", dict(max_count=32, sigma_normal=0.25, sigma_depth=0.1)),
]


def floor_bytes(w, h):
    """Bytes per call the pass must move once: (first frame, steady)."""
    npix = w * h
    first = 3 * 24 + 24 + 2 * 32  # three frames in, the frame and two records out
    return npix * first, npix * (first + 2 * 32)  # steady: each history record read once at least


def orbit_camera(pt, r, cam, degrees):
    """`cam` turned by `degrees` about the vertical axis (its up) through the first hit of its axis."""
    if degrees == 0:
        return cam
    pos, d = cam.position, cam.direction
    hit = r.closest_hit(np.concatenate([pos, d]))[0]
    if hit["shape"] < 0:
        raise SystemExit("temporal_bench: the camera's axis hits nothing to orbit about")
    up = np.array([0.0, 1.0, 0.0])
    pivot = pos + d * hit["t"]
    rel, a = pos - pivot, math.radians(degrees)
    rot = rel * math.cos(a) + np.cross(up, rel) * math.sin(a) + up * (up @ rel) * (1.0 - math.cos(a))
    return pt.Camera.new(pivot + rot, -rot, up, cam.focal_length, cam.fov)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="cornell_box.json")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--depth", type=int, default=50, help="the timed frame's depth")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=20, help="calls per timed window of the pass and the denoiser")
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--qwidth", type=int, default=960)
    ap.add_argument("--qheight", type=int, default=540)
    ap.add_argument("--qdepth", type=int, default=8)
    ap.add_argument("--converged", type=int, default=4096, help="samples of the converged frame")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--skip-quality", action="store_true")
    args = ap.parse_args()

    import torch

    import __graft_entry__ as entry
    pt = entry.load_package()
    if not torch.cuda.is_available():
        raise SystemExit("temporal_bench: no GPU")
    scene = pt.Scene.from_json((ROOT / "scenes" / args.scene).read_text(), seed=1)
    stream = torch.cuda.current_stream()
    st = stream.cuda_stream

    def buf(n):
        return torch.zeros(n, dtype=torch.float64, device="cuda")

    def timed(fn, calls=1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for i in range(calls):
            fn(i)
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b) / calls

    # ---- time ----
    w, h = args.width, args.height
    n, hn = w * h * 3, pt.temporal_history_doubles(w, h)
    r = pt.HipRenderer(scene, device=0, depth=args.depth)
    cams = [scene.camera(), orbit_camera(pt, r, scene.camera(), 1.0)]
    sets = [dict(rgb=buf(n), albedo=buf(n), normal=buf(n), depth=buf(n)) for _ in cams]
    hist = [buf(hn), buf(hn)]
    out, den, work = buf(n), buf(n), buf(pt.denoise_workspace_doubles(w, h))

    def frame(i):
        s = sets[i & 1]
        r.render_device(cams[i & 1], w, h, 1, args.seed + i, 0, 1, s["rgb"].data_ptr(), st)

    def aov(i):
        s = sets[i & 1]
        r.render_aov_device(cams[i & 1], w, h, 1, args.seed + i, 0, 1, s["albedo"].data_ptr(), s["normal"].data_ptr(),
                            s["depth"].data_ptr(), st)

    def first(i):
        s = sets[i & 1]
        pt.temporal_device(s["rgb"].data_ptr(), s["normal"].data_ptr(), s["depth"].data_ptr(), cams[i & 1], None, w, h,
                           0, hist[i & 1].data_ptr(), out.data_ptr(), stream_ptr=st)

    def steady(i):  # call i reads what call i - 1 wrote for the other camera
        s = sets[i & 1]
        pt.temporal_device(s["rgb"].data_ptr(), s["normal"].data_ptr(), s["depth"].data_ptr(), cams[i & 1],
                           cams[(i & 1) ^ 1], w, h, hist[(i & 1) ^ 1].data_ptr(), hist[i & 1].data_ptr(),
                           out.data_ptr(), stream_ptr=st)

    def denoise(i):
        s = sets[i & 1]
        pt.denoise_device(out.data_ptr(), s["albedo"].data_ptr(), s["normal"].data_ptr(), s["depth"].data_ptr(), w, h,
                          den.data_ptr(), work.data_ptr(), stream_ptr=st)

    legs = [("frame_1spp_depth%d" % args.depth, frame, 2), ("aov_1", aov, 2), ("temporal_first", first, args.batch),
            ("temporal_steady", steady, args.batch), ("denoise_5", denoise, args.batch)]
    for name, fn, calls in legs:  # warm-up: code objects, the workspace, both cameras' frames, planes and histories
        timed(fn, 2)
    ms = {name: [] for name, _, _ in legs}
    for _ in range(args.rounds):
        for name, fn, calls in legs:
            ms[name].append(timed(fn, calls))
    resets = float((hist[1].view(2, w * h, 4)[0][:, 3] == 1.0).double().mean())
    med = {k: statistics.median(v) for k, v in ms.items()}
    fb, sb = floor_bytes(w, h)
    res = {
        "workload": "%s %dx%d depth %d, 1 spp" % (args.scene, w, h, args.depth),
        "version": pt.version(),
        "device": torch.cuda.get_device_name(0),
        "rounds": args.rounds,
        "batch": args.batch,
        "ms_per_call": {k: [round(x, 4) for x in v] for k, v in ms.items()},
        "median_ms": {k: round(v, 4) for k, v in med.items()},
        "min_max_ms": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
        "floor": {"copy_tbps": COPY_TBPS, "first_bytes": fb, "steady_bytes": sb,
                  "first_ms": round(fb / (COPY_TBPS * 1e12) * 1e3, 4),
                  "steady_ms": round(sb / (COPY_TBPS * 1e12) * 1e3, 4),
                  "first_over_floor": round(med["temporal_first"] / (fb / (COPY_TBPS * 1e12) * 1e3), 2),
                  "steady_over_floor": round(med["temporal_steady"] / (sb / (COPY_TBPS * 1e12) * 1e3), 2),
                  "steady_tbps_achieved": round(sb / (med["temporal_steady"] * 1e-3) / 1e12, 2)},
        "steady_over_frame": round(med["temporal_steady"] / med["frame_1spp_depth%d" % args.depth], 5),
        "steady_over_denoise": round(med["temporal_steady"] / med["denoise_5"], 4),
        "steady_reset_share": round(resets, 4),
        "finite": bool(torch.isfinite(out).all()),
    }
    del r, sets, hist, out, den, work

    # ---- quality ----
    if not args.skip_quality:
        w, h = args.qwidth, args.qheight
        n, hn = w * h * 3, pt.temporal_history_doubles(w, h)
        r = pt.HipRenderer(scene, device=0, depth=args.qdepth)
        ref = buf(n)
        r.render_device(scene.camera(), w, h, args.converged, 77, 0, 1, ref.data_ptr(), st)
        work = buf(pt.denoise_workspace_doubles(w, h))

        def rms(t):
            return float(torch.sqrt(torch.mean((t - ref) ** 2)))

        def denoised(rgb, s):
            d = buf(n)
            pt.denoise_device(rgb.data_ptr(), s["albedo"].data_ptr(), s["normal"].data_ptr(), s["depth"].data_ptr(), w,
                              h, d.data_ptr(), work.data_ptr(), stream_ptr=st)
            return d

        quality = {}
        for moving in (True, False):
            seq = []  # the frames and planes of the sequence, rendered once, shared by every setting
            for i in range(args.frames):
                cam = orbit_camera(pt, r, scene.camera(), float(args.frames - 1 - i) if moving else 0.0)
                s = dict(rgb=buf(n), albedo=buf(n), normal=buf(n), depth=buf(n), cam=cam)
                r.render_device(cam, w, h, 1, 100 + i, 0, 1, s["rgb"].data_ptr(), st)
                r.render_aov_device(cam, w, h, 1, 100 + i, 0, 1, s["albedo"].data_ptr(), s["normal"].data_ptr(),
                                    s["depth"].data_ptr(), st)
                seq.append(s)
            last = seq[-1]
            rows = {"raw": round(rms(last["rgb"]), 5), "denoised": round(rms(denoised(last["rgb"], last)), 5),
                    "settings": {}}
            for name, kw in SETTINGS:
                hist, acc, reset = [buf(hn), buf(hn)], buf(n), []
                for i, s in enumerate(seq):
                    pt.temporal_device(s["rgb"].data_ptr(), s["normal"].data_ptr(), s["depth"].data_ptr(), s["cam"],
                                       seq[i - 1]["cam"] if i else None, w, h, hist[(i & 1) ^ 1].data_ptr() if i else 0,
                                       hist[i & 1].data_ptr(), acc.data_ptr(), stream_ptr=st, **kw)
                    if i:
                        reset.append(round(float((hist[i & 1].view(2, w * h, 4)[0][:, 3] == 1.0).double().mean()), 4))
                counts = hist[(len(seq) - 1) & 1].view(2, w * h, 4)[0][:, 3]
                rows["settings"][name] = {
                    **kw, "accumulated": round(rms(acc), 5),
                    "accumulated_denoised": round(rms(denoised(acc, last)), 5),
                    "reset_share_per_frame": reset, "mean_count": round(float(counts.mean()), 3),
                    "finite": bool(torch.isfinite(acc).all())}
            quality["orbit" if moving else "still"] = rows
        res["quality"] = {"workload": "%s %dx%d depth %d, 1 spp, %d frames; converged %d spp seed 77"
                                      % (args.scene, w, h, args.qdepth, args.frames, args.converged), **quality}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
