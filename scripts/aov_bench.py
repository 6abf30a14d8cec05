"""What the guide-plane pass costs beside the beauty frame, on the C2 workload: cornell_box,
1920x1080, one renderer of depth 8.  After a warm-up of each, five rounds of: the beauty frame at 256 spp, the
three-plane pass at 256 samples, the pass at 16 samples; each timed with device events on the stream.  Prints one
JSON line (profiles/r9/aov.txt is this script's output):

    python scripts/aov_bench.py [--rounds 5] [--width 1920 --height 1080 --spp 256 --low 16 --depth 8]

Needs a GPU (there is no fallback)."""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="cornell_box.json")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--low", type=int, default=16, help="the pass's second sample count")
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()

    import torch

    import __graft_entry__ as entry
    pt = entry.load_package()
    if not torch.cuda.is_available():
        raise SystemExit("aov_bench: no GPU")
    w, h = args.width, args.height
    scene = pt.Scene.from_json((ROOT / "scenes" / args.scene).read_text(), seed=1)
    r = pt.HipRenderer(scene, device=0, depth=args.depth)
    cam = scene.camera()
    n = w * h * 3
    frame = torch.zeros(n, dtype=torch.float64, device="cuda")
    planes = [torch.zeros(n, dtype=torch.float64, device="cuda") for _ in range(3)]
    stream = torch.cuda.current_stream()
    st = stream.cuda_stream

    def beauty():
        r.render_device(cam, w, h, args.spp, args.seed, 0, 1, frame.data_ptr(), st)

    def aov(spp):
        return lambda: r.render_aov_device(cam, w, h, spp, args.seed, 0, 1, *[p.data_ptr() for p in planes], st)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b)

    legs = [("beauty_%dspp" % args.spp, beauty), ("aov_%d" % args.spp, aov(args.spp)), ("aov_%d" % args.low, aov(args.low))]
    for _, fn in legs:  # warm-up: code objects, the wavefront workspace
        timed(fn)
    ms = {name: [] for name, _ in legs}
    for _ in range(args.rounds):
        for name, fn in legs:
            ms[name].append(timed(fn))
    b, a = ms[legs[0][0]], ms[legs[1][0]]
    ratios = [x / y for x, y in zip(a, b)]
    out = {
        "workload": "%s %dx%d depth %d" % (args.scene, w, h, args.depth),
        "version": pt.version(),
        "device": torch.cuda.get_device_name(0),
        "rounds": args.rounds,
        "ms": {k: [round(x, 3) for x in v] for k, v in ms.items()},
        "median_ms": {k: round(statistics.median(v), 3) for k, v in ms.items()},
        # the 256-sample pass over the beauty frame, round by round (each pair ran back to back)
        "aov_over_beauty": {"median": round(statistics.median(ratios), 4), "min": round(min(ratios), 4),
                            "max": round(max(ratios), 4)},
        "aov_msamples_per_s": round(w * h * args.spp / statistics.median(a) / 1e3, 1),
        "march_guard_drops": pt.march_guard_drops(r),
        "planes_finite": bool(all(torch.isfinite(p).all() for p in planes)),
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
