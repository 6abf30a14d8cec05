"""march::clip_to_best (pt_march.hpp) on the host: the march clipped to the caller's best hit gives the same
(accepted, t) as the plain march over the whole chord followed by the caller's `t > best` test, bit for bit, and
takes fewer iterations.  tests/march_clip/march_clip_harness.cpp is a stand-alone host build of the product headers;
this test builds it (a few seconds; nothing to do after build()) and runs it twice:

* capture: the march jobs of the product's own host path on cornell_box.json (20,000 scattered pixels of the
  1920x1080 frame, 4 spp, depth 8), each against the best hit trace_pixel starts it with;
* synth: Heart jobs at unit scale and at cornell's scale, steps 0.01 and 0.003, passes 1 to 4, both the Heart build
  and the generic one, with `best` before, at and after the chord's start and end, between the start and the coarse
  crossing, within +-1 .. +-6 steps and +-1 ulp of the coarse crossing and of the final t, with the cap itself on
  those points, and +inf.

The cornell figures (profiles/r17/march_clip_host.txt holds a run's output) are properties of the scene and the
march, not of the machine; the bounds below are about half of what the capture shows, and a run prints the counts.
"""
import subprocess

from conftest import ROOT

HARNESS = ROOT / "tests" / "march_clip"


def run_harness(*args):
    subprocess.run(["make", "-C", str(HARNESS)], check=True, capture_output=True)
    p = subprocess.run([str(HARNESS / "_build" / "march_clip_harness"), *args], capture_output=True, text=True)
    print(p.stdout)
    assert p.returncode in (0, 1), p.stderr
    out = {}
    for line in p.stdout.splitlines():
        k, _, v = line.partition(" ")
        if v.strip().lstrip("-").isdigit():
            out[k] = int(v)
    return out


def test_cornell_capture_replay():
    c = run_harness("capture", str(ROOT / "scenes" / "cornell_box.json"), "20000", "4")
    assert c["capture_jobs"] >= 40000
    assert c["capture_differ"] == 0 and c["capture_guard"] == 0
    # the savings: jobs whose chord starts behind the cap are not marched at all, the others stop at it
    assert c["capture_marches_plain"] == c["capture_jobs"]
    assert c["capture_marches_clipped"] == c["capture_jobs"] - c["capture_chord_starts_behind_cap"]
    assert c["capture_chord_starts_behind_cap"] >= 0.03 * c["capture_jobs"]
    assert c["capture_chord_beyond_cap"] >= 0.09 * c["capture_jobs"]
    assert c["capture_iters_clipped"] <= 0.96 * c["capture_iters_plain"]
    assert c["capture_cut_jobs_iters_clipped"] < c["capture_cut_jobs_iters_plain"]


def test_synthetic_placements_of_best():
    s = run_harness("synth")
    assert s["synth_jobs"] >= 50000
    assert s["synth_differ"] == 0 and s["synth_guard"] == 0
    # the placements reach every case: chords cut, jobs dropped, marches that finish and are then discarded
    assert s["synth_chord_beyond_cap"] > 10000 and s["synth_chord_starts_behind_cap"] > 500
    assert s["synth_done_then_discarded"] > 10000
    assert s["synth_iters_clipped"] < s["synth_iters_plain"]
