"""What the variance estimate and the denoiser's variance term cost, on the C2 workload:
cornell_box, 1920x1080, one renderer of depth 8.  After a warm-up of each, five alternating rounds of: the one-shot
frame at 256 spp (pt_render_device), the same frame in 8 sample windows with the variance plane
(pt_render_variance_device), the plain denoiser at its defaults (pt_denoise_device) and the variance-guided one
(pt_denoise_variance_device) on that frame, its variance plane and guide planes of 16 samples; each timed with
device events on the stream.  Then, outside the timed rounds, one frame of each kind with the per-kind kernel timing
(pt_kernel_timing) on, to show where a windowed frame's extra time goes, and the accumulate launches alone
(8 x pt_variance_window_device on the finished buffers).  Prints one JSON line (profiles/r11/variance.txt is this
script's output):

    python scripts/variance_bench.py [--rounds 5] [--width 1920 --height 1080 --spp 256 --windows 8 --low 16]

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
    ap.add_argument("--windows", type=int, default=8)
    ap.add_argument("--low", type=int, default=16, help="the guide planes' sample count")
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()

    import torch

    import __graft_entry__ as entry
    pt = entry.load_package()
    if not torch.cuda.is_available():
        raise SystemExit("variance_bench: no GPU")
    w, h, spp, K = args.width, args.height, args.spp, args.windows
    scene = pt.Scene.from_json((ROOT / "scenes" / args.scene).read_text(), seed=1)
    r = pt.HipRenderer(scene, device=0, depth=args.depth)
    cam = scene.camera()
    n = w * h * 3

    def buf(count=n):
        return torch.zeros(count, dtype=torch.float64, device="cuda")

    one, frame, var, out = buf(), buf(), buf(), buf()
    planes = [buf() for _ in range(3)]
    vwork = buf(pt.variance_workspace_doubles(w, h))
    dwork = buf(pt.denoise_workspace_doubles(w, h))
    stream = torch.cuda.current_stream()
    st = stream.cuda_stream

    def one_shot():
        r.render_device(cam, w, h, spp, args.seed, 0, 1, one.data_ptr(), st)

    def windowed():
        r.render_variance_device(cam, w, h, spp, args.seed, 0, 1, K, frame.data_ptr(), var.data_ptr(),
                                 vwork.data_ptr(), st)

    def denoise():
        pt.denoise_device(frame.data_ptr(), *[p.data_ptr() for p in planes], w, h, out.data_ptr(), dwork.data_ptr(),
                          stream_ptr=st)

    def denoise_variance():
        pt.denoise_variance_device(frame.data_ptr(), *[p.data_ptr() for p in planes], var.data_ptr(), w, h,
                                   out.data_ptr(), dwork.data_ptr(), stream_ptr=st)

    def accumulate_alone():
        for k in range(1, K + 1):
            n_k = k * spp // K - (k - 1) * spp // K
            pt.variance_window_device(frame.data_ptr(), n, n_k, spp, k, K, vwork.data_ptr(), out.data_ptr(), st)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b)

    r.render_aov_device(cam, w, h, args.low, args.seed, 0, 1, *[p.data_ptr() for p in planes], st)
    legs = [("one_shot_%dspp" % spp, one_shot), ("windowed_%dspp_%dw" % (spp, K), windowed), ("denoise", denoise),
            ("denoise_variance", denoise_variance)]
    for _, fn in legs:  # warm-up: code objects, the wavefront workspace; the frame and planes the denoisers read
        timed(fn)
    same_frame = bool(torch.equal(one, frame))
    ms = {name: [] for name, _ in legs}
    for _ in range(args.rounds):
        for name, fn in legs:
            ms[name].append(timed(fn))
    finite = bool(torch.isfinite(out).all()) and bool(torch.isfinite(var).all())
    var_mean = float(var.mean())

    # outside the timed rounds: the accumulate launches alone, and each frame kind under the per-kind kernel timing
    timed(accumulate_alone)
    acc = [timed(accumulate_alone) for _ in range(args.rounds)]
    kinds = {}
    for name, fn in legs[:2]:
        pt.kernel_timing(r, True)
        total = timed(fn)
        t = pt.kernel_timing(r, False)
        kinds[name] = {"frame_ms": round(total, 3),
                       "kernel_ms": {k: round(v[0], 3) for k, v in t.items() if v[1]},
                       "launches": {k: v[1] for k, v in t.items() if v[1]}}

    med = {k: statistics.median(v) for k, v in ms.items()}
    a, b, c, d = [name for name, _ in legs]
    res = {
        "workload": "%s %dx%d depth %d" % (args.scene, w, h, args.depth),
        "version": pt.version(),
        "device": torch.cuda.get_device_name(0),
        "rounds": args.rounds,
        "ms": {k: [round(x, 3) for x in v] for k, v in ms.items()},
        "median_ms": {k: round(v, 3) for k, v in med.items()},
        "min_max_ms": {k: [round(min(v), 3), round(max(v), 3)] for k, v in ms.items()},
        "windowed_over_one_shot": round(med[b] / med[a], 5),
        "windowed_over_one_shot_per_round": [round(y / x, 5) for x, y in zip(ms[a], ms[b])],
        "denoise_variance_over_denoise": round(med[d] / med[c], 4),
        "accumulate_alone_ms": {"median": round(statistics.median(acc), 3), "min_max": [round(min(acc), 3),
                                                                                       round(max(acc), 3)]},
        "kernel_timing": kinds,
        "windowed_frame_equals_one_shot": same_frame,
        "finite": finite,
        "variance_mean": var_mean,
    }
    print(json.dumps(res))


if __name__ == "__main__":
    main()
