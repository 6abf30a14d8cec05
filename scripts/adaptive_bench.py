"""What adaptive sampling saves, on the C2 workload: cornell_box, 1920x1080, one renderer of depth
8, windows of 32 samples, a cap of 256.  After a warm-up of each, five alternating rounds of: the uniform frame with
the same window structure (pt_render_variance_device, 256 spp in 8 windows) and the adaptive frame
(pt_render_adaptive_device) at thresholds 0.05, 0.1 and 0.2, each with merge_gap 0, 4, 16, 64, 256, 1024 and "join
everything";
each timed with device events on the stream around the whole (blocking) call.  Beside the times: the pixel-samples
kept (each tile's pixels times the count it stopped at) and launched (the stopped tiles inside joined runs included)
against 256 * w * h, and the render launches' runs.  Then, outside the timed rounds, one adaptive frame per threshold
under the per-kind kernel timing (pt_kernel_timing), to show where the time goes.  Prints one JSON line
(profiles/r12/adaptive.txt is this script's output):

    python scripts/adaptive_bench.py [--rounds 5] [--width 1920 --height 1080 --cap 256 --window 32]

List mode (profiles/r14/adaptive_list.txt): "list" among --gaps is the frame whose windows are one
launch each over the list of the still-active tiles (pt_render_adaptive_list_device), and --list is short for --gaps
list,1024: the listed frame beside the run-based frame at the default merge_gap and the uniform frame, in the same
alternating rounds.  The result then has a "list" table: per threshold the samples kept, the listed frame's time, its
ratio to the uniform frame, the time a perfect conversion of samples into time would give (kept x uniform) and what
is left over, and the listed frame's launches and kernel time by kind.

    python scripts/adaptive_bench.py --list

Needs a GPU (there is no fallback)."""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

JOIN_ALL = 0xFFFFFFFF
LIST = -1  # not a merge_gap: the listed frame


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="cornell_box.json")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--cap", type=int, default=256)
    ap.add_argument("--window", type=int, default=32)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--thresholds", default="0.05,0.1,0.2")
    ap.add_argument("--gaps", default="0,4,16,64,256,1024,all")
    ap.add_argument("--list", action="store_true", help="the listed frame beside merge_gap 1024: --gaps list,1024")
    args = ap.parse_args()
    if args.list:
        args.gaps = "list,1024"

    import numpy as np
    import torch

    import __graft_entry__ as entry
    pt = entry.load_package()
    if not torch.cuda.is_available():
        raise SystemExit("adaptive_bench: no GPU")
    w, h, cap, window = args.width, args.height, args.cap, args.window
    windows = (cap + window - 1) // window
    thresholds = [float(t) for t in args.thresholds.split(",")]
    gaps = [JOIN_ALL if g == "all" else LIST if g == "list" else int(g) for g in args.gaps.split(",")]
    scene = pt.Scene.from_json((ROOT / "scenes" / args.scene).read_text(), seed=1)
    r = pt.HipRenderer(scene, device=0, depth=args.depth)
    cam = scene.camera()
    n = w * h * 3
    tx, ty = (w + 15) // 16, (h + 15) // 16
    ntiles = tx * ty
    pixels = (np.minimum(16, w - 16 * np.arange(tx))[None, :] * np.minimum(16, h - 16 * np.arange(ty))[:, None]).ravel()

    def buf(count=n, dtype=torch.float64):
        return torch.zeros(count, dtype=dtype, device="cuda")

    frame, var, uniform = buf(), buf(), buf()
    work = buf(pt.adaptive_workspace_doubles(w, h))  # 3 planes: the uniform frame's 2 fit in it
    ts, te = buf(ntiles, torch.int32), buf(ntiles)
    stream = torch.cuda.current_stream()
    st = stream.cuda_stream
    launched = {}

    def uniform_frame():
        r.render_variance_device(cam, w, h, cap, args.seed, 0, 1, windows, uniform.data_ptr(), var.data_ptr(),
                                 work.data_ptr(), st)

    def adaptive(threshold, gap):
        def fn():
            launched[(threshold, gap)] = r.render_adaptive_device(
                cam, w, h, cap, threshold, args.seed, 0, 1, frame.data_ptr(), var.data_ptr(), ts.data_ptr(),
                te.data_ptr(), work.data_ptr(), st, window=window,
                **(dict(tile_list=True) if gap == LIST else dict(merge_gap=gap)))
        return fn

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b)

    def gap_name(g):
        return "all" if g == JOIN_ALL else "list" if g == LIST else str(g)

    legs = [("uniform_%dspp_%dw" % (cap, windows), uniform_frame)]
    legs += [("thr%g_gap%s" % (t, gap_name(g)), adaptive(t, g)) for t in thresholds for g in gaps]
    tiles = {}
    for name, fn in legs:  # warm-up: code objects, the wavefront workspace at every run size
        timed(fn)
    for t in thresholds:   # the maps (the same for every merge_gap), and what a frame's runs look like
        timed(adaptive(t, gaps[0]))
        tiles[t] = ts.cpu().numpy().astype(np.int64)
    ms = {name: [] for name, _ in legs}
    for _ in range(args.rounds):
        for name, fn in legs:
            ms[name].append(timed(fn))
    finite = bool(torch.isfinite(frame).all()) and bool(torch.isfinite(var).all())

    # the uniform frame's tiles equal the adaptive frame's tiles that ran to the cap (the same samples, the same sums)
    timed(uniform_frame)
    timed(adaptive(thresholds[0], gaps[0]))
    at_cap = np.repeat(tiles[thresholds[0]].reshape(ty, tx) == cap, 16, axis=0)[:h]
    at_cap = np.repeat(at_cap, 16, axis=1)[:, :w].ravel()
    u, f = uniform.cpu().numpy().reshape(-1, 3), frame.cpu().numpy().reshape(-1, 3)
    cap_tiles_equal_uniform = bool(np.array_equal(u[at_cap], f[at_cap]))

    kinds = {}
    for t in thresholds:
        for g in (LIST, 0, 16):
            if g not in gaps:
                continue
            pt.kernel_timing(r, True)
            total = timed(adaptive(t, g))
            k = pt.kernel_timing(r, False)
            kinds["thr%g_gap%s" % (t, gap_name(g))] = {"frame_ms": round(total, 3),
                                             "kernel_ms": {a: round(v[0], 3) for a, v in k.items() if v[1]},
                                             "launches": {a: v[1] for a, v in k.items() if v[1]}}
    pt.kernel_timing(r, True)
    total = timed(uniform_frame)
    k = pt.kernel_timing(r, False)
    kinds[legs[0][0]] = {"frame_ms": round(total, 3), "kernel_ms": {a: round(v[0], 3) for a, v in k.items() if v[1]},
                         "launches": {a: v[1] for a, v in k.items() if v[1]}}

    full = cap * w * h
    med = {name: statistics.median(v) for name, v in ms.items()}
    base = med[legs[0][0]]
    table = []
    for t in thresholds:
        kept = int(np.sum(pixels * tiles[t]))
        hist = {int(c): int(np.sum(tiles[t] == c)) for c in sorted(set(tiles[t].tolist()))}
        for g in gaps:
            name = "thr%g_gap%s" % (t, gap_name(g))
            table.append({"threshold": t, "merge_gap": gap_name(g), "median_ms": round(med[name], 3),
                          "min_max_ms": [round(min(ms[name]), 3), round(max(ms[name]), 3)],
                          "time_over_uniform": round(med[name] / base, 4),
                          "samples_kept_over_full": round(kept / full, 4),
                          "samples_launched_over_full": round(launched[(t, g)] / full, 4)})
        table.append({"threshold": t, "tiles_by_samples": hist})
    listed = []
    if LIST in gaps:
        spread = max(ms[legs[0][0]]) - min(ms[legs[0][0]])
        for t in thresholds:
            name = "thr%g_gaplist" % t
            kept = int(np.sum(pixels * tiles[t])) / full
            spread_t = max(spread, max(ms[name]) - min(ms[name]))
            listed.append({"threshold": t, "samples_kept_over_full": round(kept, 4),
                           "samples_launched_over_full": round(launched[(t, LIST)] / full, 4),
                           "list_median_ms": round(med[name], 3),
                           "list_min_max_ms": [round(min(ms[name]), 3), round(max(ms[name]), 3)],
                           "time_over_uniform": round(med[name] / base, 4),
                           "perfect_conversion_ms": round(kept * base, 3),
                           "left_over_ms": round(med[name] - kept * base, 3),
                           "faster_than_uniform_by_more_than_the_spread": bool(base - med[name] > spread_t),
                           "kernel_timing": kinds.get(name)})
    res = {
        "workload": "%s %dx%d depth %d, window %d, cap %d" % (args.scene, w, h, args.depth, window, cap),
        "version": pt.version(),
        "device": torch.cuda.get_device_name(0),
        "rounds": args.rounds,
        "uniform_median_ms": round(base, 3),
        "uniform_min_max_ms": [round(min(ms[legs[0][0]]), 3), round(max(ms[legs[0][0]]), 3)],
        "table": table,
        **({"list": listed} if listed else {}),
        "ms": {name: [round(x, 3) for x in v] for name, v in ms.items()},
        "kernel_timing": kinds,
        "cap_tiles_equal_uniform_frame": cap_tiles_equal_uniform,
        "finite": finite,
    }
    print(json.dumps(res))


if __name__ == "__main__":
    main()
