"""Generates tests/golden/wave_plans.json: the wavefront engine's frame plan (rs-pathtracing_amd/csrc/pt_plan.hpp:
plan fields, slot layout, chunk list) for a seeded draw of inputs, as computed by tests/native/_build/libplan.so
(or the library named on the command line).  The file was written from the arithmetic of launch_render_wave as it
stood before the plan moved into its own header, so tests/test_wave_plan.py::test_golden_plans shows that the move
changed no plan.

    make -C tests/native && python tests/golden/make_wave_plans.py [libplan.so]
"""
import ctypes as C
import hashlib
import json
import random
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
UNKNOWN = 2**64 - 1
FIELDS = ("ntiles", "s_begin", "s_end", "spp", "depth", "progressive", "textured", "presel", "wf_paths",
          "wf_slots", "wf_min_chunks", "avail_bytes")
FULL_LIST = 48  # chunk lists up to this length are stored whole; every list by count and digest


def load(path=None):
    L = C.CDLL(str(path or HERE.parent / "native" / "_build" / "libplan.so"))
    u64p = C.POINTER(C.c_uint64)
    L.plan_make.argtypes = [u64p, u64p]
    L.plan_make.restype = None
    L.plan_layout.argtypes = [u64p, u64p]
    L.plan_layout.restype = None
    L.plan_chunks.argtypes = [u64p, C.POINTER(C.c_uint32), C.c_uint64]
    L.plan_chunks.restype = C.c_uint64
    return L


def evaluate(L, inp):
    """{"plan": 10 words, "layout": 26 words, "chunks": [[g0, gt, s0, ns, slot, step], ...]} (plan_harness.cpp)"""
    w = (C.c_uint64 * 12)(*[int(inp[f]) for f in FIELDS])
    plan, lay = (C.c_uint64 * 10)(), (C.c_uint64 * 26)()
    L.plan_make(w, plan)
    L.plan_layout(w, lay)
    n = L.plan_chunks(w, None, 0)
    buf = (C.c_uint32 * (6 * n))()
    assert L.plan_chunks(w, buf, n) == n
    flat = list(buf)
    return {"plan": list(plan), "layout": list(lay), "chunks": [flat[k:k + 6] for k in range(0, 6 * n, 6)]}


def draw(rng):
    """One input of the sweep.  Chunks number (tile groups) x (sample chunks), and the smallest wf_paths make a group
    of every tile or four: those draws keep to a few hundred tiles, and to a few samples beyond 16 tiles."""
    wf_paths = rng.choice([0, 256, 300, 1024, 2**22, 2**28])
    small = 0 < wf_paths <= 1024
    top = 400 if small else 40000
    ntiles = rng.choice([rng.randint(1, 16), rng.randint(1, min(top, 2000)), rng.randint(1, top)])
    spp = rng.choice([rng.randint(1, 8), rng.randint(1, 8 if small and ntiles > 16 else 300)])
    s_begin, s_end = 0, spp
    if rng.random() < 0.3:  # a resumable frame's window
        s_begin = rng.randint(0, spp - 1)
        s_end = rng.randint(s_begin + 1, spp)
    avail = rng.choice([UNKNOWN, UNKNOWN, 0, 2**30 * rng.randint(1, 300)])
    return {"ntiles": ntiles, "s_begin": s_begin, "s_end": s_end, "spp": spp,
            "depth": rng.choice([0, 1, 8, 50, 64]), "progressive": rng.randint(0, 1), "textured": rng.randint(0, 1),
            "presel": rng.randint(0, 1), "wf_paths": wf_paths, "wf_slots": rng.randint(1, 4),
            "wf_min_chunks": rng.randint(1, 8), "avail_bytes": avail}


def digest(chunks):
    return hashlib.sha256(json.dumps(chunks, separators=(",", ":")).encode()).hexdigest()


def main():
    L = load(sys.argv[1] if len(sys.argv) > 1 else None)
    rng = random.Random(20261019)
    cases = []
    for _ in range(40):
        inp = draw(rng)
        r = evaluate(L, inp)
        rec = {"input": inp, "plan": r["plan"], "layout": r["layout"], "nchunks": len(r["chunks"]),
               "chunks_sha256": digest(r["chunks"])}
        if len(r["chunks"]) <= FULL_LIST:
            rec["chunks"] = r["chunks"]
        cases.append(rec)
    out = HERE / "wave_plans.json"
    out.write_text("[\n" + ",\n".join(json.dumps(c, separators=(",", ":")) for c in cases) + "\n]\n")
    print("wrote", out, len(cases), "cases")


if __name__ == "__main__":
    main()
