"""What the guided denoiser costs beside the frame it cleans, on the C2 workload: cornell_box,
1920x1080, one renderer of depth 8.  After a warm-up of each, five rounds of: the beauty frame at 256 spp, the
three guide planes at 16 samples, the denoiser (5 iterations, the defaults) on that frame and those planes; each
timed with device events on the stream.  Beside the times it prints the floor the pass cannot beat: the bytes it
must move once (the four frames in, the work records out and in again per iteration, the frame out) over the
device's measured copy rate, and the cache reads the 25 taps make on top (25 x 64 B per pixel and iteration), which
are reported as a rate, not a time.  --trace DIR first runs the denoiser alone under `rocprofv3 --kernel-trace
--stats` in a child process of its own and adds the per-launch split (the prepare launch and each stride).  Prints
one JSON line (profiles/r10/denoise.txt is this script's output):

    python scripts/denoise_bench.py [--rounds 5] [--width 1920 --height 1080 --spp 256 --low 16] [--trace DIR]

Needs a GPU (there is no fallback)."""
import argparse
import csv
import json
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

COPY_TBPS = 6.29  # the device's measured copy rate (read + write bytes over time)


def floor(w, h, iterations):
    """Bytes per frame the pass must move once, and the taps' cache reads."""
    npix = w * h
    prepare = 4 * 24 + 2 * 32  # four frames in, the colour and guide records out
    middle = 2 * 32 + 32  # an iteration: the pixel's own two records in, the new colour out
    last = 2 * 32 + 24 + 24  # the last one: the albedo in and the frame out instead
    compulsory = npix * (prepare + (iterations - 1) * middle + last)
    cache = npix * iterations * 25 * 64
    return compulsory, cache


def traced(args):
    """The denoiser alone under the kernel trace, in a fresh process; {kernel or launch: microseconds}."""
    out = Path(args.trace)
    out.mkdir(parents=True, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", str(out), "--", sys.executable,
           str(Path(__file__).resolve()), "--only-denoise", "--rounds", "3", "--width", str(args.width), "--height",
           str(args.height), "--spp", "1", "--low", "1", "--iterations", str(args.iterations)]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=600)
    rows = []
    for f in out.rglob("*kernel_trace.csv"):
        with open(f, newline="") as fh:
            rows += [r for r in csv.DictReader(fh) if "denoise" in r.get("Kernel_Name", "")]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    per = args.iterations + 1  # launches per call: the prepare launch, then the strides
    if not rows or len(rows) % per:
        return {"error": "unexpected trace: %d denoise launches" % len(rows)}
    calls = [rows[i:i + per] for i in range(0, len(rows), per)][1:]  # the first call is the warm-up
    names = ["prepare"] + ["stride_%d" % (1 << i) for i in range(args.iterations)]
    us = {n: statistics.median((int(c[k]["End_Timestamp"]) - int(c[k]["Start_Timestamp"])) / 1e3 for c in calls)
          for k, n in enumerate(names)}
    return {"launch_us": {k: round(v, 1) for k, v in us.items()}, "kernel_sum_us": round(sum(us.values()), 1),
            "calls": len(calls)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="cornell_box.json")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--low", type=int, default=16, help="the guide planes' sample count")
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--trace", default=None, help="directory for one rocprofv3 kernel trace of the denoiser alone")
    ap.add_argument("--only-denoise", action="store_true", help="time the denoiser only (the traced child)")
    args = ap.parse_args()

    trace = None
    if args.trace:  # before this process opens the GPU; a trace that cannot be read does not cost the timing
        try:
            trace = traced(args)
        except (OSError, subprocess.SubprocessError, KeyError, ValueError) as e:
            trace = {"error": "%s: %s" % (type(e).__name__, e)}

    import torch

    import __graft_entry__ as entry
    pt = entry.load_package()
    if not torch.cuda.is_available():
        raise SystemExit("denoise_bench: no GPU")
    w, h = args.width, args.height
    scene = pt.Scene.from_json((ROOT / "scenes" / args.scene).read_text(), seed=1)
    r = pt.HipRenderer(scene, device=0, depth=args.depth)
    cam = scene.camera()
    n = w * h * 3
    frame = torch.zeros(n, dtype=torch.float64, device="cuda")
    planes = [torch.zeros(n, dtype=torch.float64, device="cuda") for _ in range(3)]
    out = torch.zeros(n, dtype=torch.float64, device="cuda")
    work = torch.zeros(pt.denoise_workspace_doubles(w, h), dtype=torch.float64, device="cuda")
    stream = torch.cuda.current_stream()
    st = stream.cuda_stream

    def beauty():
        r.render_device(cam, w, h, args.spp, args.seed, 0, 1, frame.data_ptr(), st)

    def aov():
        r.render_aov_device(cam, w, h, args.low, args.seed, 0, 1, *[p.data_ptr() for p in planes], st)

    def denoise():
        pt.denoise_device(frame.data_ptr(), *[p.data_ptr() for p in planes], w, h, out.data_ptr(), work.data_ptr(),
                          iterations=args.iterations, stream_ptr=st)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b)

    legs = [("beauty_%dspp" % args.spp, beauty), ("aov_%d" % args.low, aov), ("denoise_%d" % args.iterations, denoise)]
    for _, fn in legs:  # warm-up: code objects, the wavefront workspace; the frame and planes the denoiser reads
        timed(fn)
    if args.only_denoise:
        legs = legs[2:]
    ms = {name: [] for name, _ in legs}
    for _ in range(args.rounds):
        for name, fn in legs:
            ms[name].append(timed(fn))
    d = ms[legs[-1][0]]
    compulsory, cache = floor(w, h, args.iterations)
    med = statistics.median(d)
    res = {
        "workload": "%s %dx%d depth %d" % (args.scene, w, h, args.depth),
        "version": pt.version(),
        "device": torch.cuda.get_device_name(0),
        "rounds": args.rounds,
        "ms": {k: [round(x, 3) for x in v] for k, v in ms.items()},
        "median_ms": {k: round(statistics.median(v), 3) for k, v in ms.items()},
        "denoise_ms_min_max": [round(min(d), 3), round(max(d), 3)],
        "floor": {"compulsory_bytes": compulsory, "copy_tbps": COPY_TBPS,
                  "compulsory_ms": round(compulsory / (COPY_TBPS * 1e12) * 1e3, 3), "cache_read_bytes": cache,
                  "cache_read_tbps_achieved": round(cache / (med * 1e-3) / 1e12, 2)},
        "denoised_finite": bool(torch.isfinite(out).all()),
    }
    if not args.only_denoise:
        b = ms[legs[0][0]]
        res["denoise_over_beauty"] = round(med / statistics.median(b), 5)
    if trace is not None:
        res["trace"] = trace
    print(json.dumps(res))


if __name__ == "__main__":
    main()
