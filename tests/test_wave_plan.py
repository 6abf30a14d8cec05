"""The wavefront engine's frame plan (rs-pathtracing_amd/csrc/pt_plan.hpp: tile groups, samples per chunk, chunk
streams, workspace layout, chunk list), built for the host by tests/native/Makefile and checked on the CPU: known
answers worked out by hand, the memory fit, the plans recorded before the plan moved out of launch_render_wave
(tests/golden/wave_plans.json), and the plan's invariants over a seeded sweep against a restatement in Python
integers."""
import json
import random
import subprocess
import sys
from pathlib import Path

import pytest

from conftest import native_lib

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE / "golden"))
import make_wave_plans as G  # noqa: E402

UNKNOWN = G.UNKNOWN
PLAN = ("cap_want", "group_tiles", "npix_max", "ns", "cap", "cap_tiles", "slots", "iters", "cnt_words", "bytes")
REGIONS = ("set0", "set1", "ids", "leaf", "list", "mq", "status", "cp_blk", "cnt", "att", "jo")
MIN_CHUNK_PATHS = 1 << 21
PATH_BYTES, CP_TILE, CP_BLOCK = 72, 4096, 256


@pytest.fixture(scope="module")
def L():
    subprocess.run(["make", "-s", "-C", str(HERE / "native"), "_build/libplan.so"], check=True)
    return G.load(native_lib("libplan.so"))


def tiles(w, h):
    return ((w + 15) // 16) * ((h + 15) // 16)


def frame(ntiles, spp, depth, wf_paths=0, slots=2, min_chunks=1, s_begin=0, s_end=None, progressive=0, textured=0,
          presel=1, avail=UNKNOWN):
    return {"ntiles": ntiles, "s_begin": s_begin, "s_end": spp if s_end is None else s_end, "spp": spp,
            "depth": depth, "progressive": progressive, "textured": textured, "presel": presel,
            "wf_paths": wf_paths, "wf_slots": slots, "wf_min_chunks": min_chunks, "avail_bytes": avail}


def plan_of(L, inp):
    r = G.evaluate(L, inp)
    return dict(zip(PLAN, r["plan"])), r["layout"], r["chunks"]


# ---------------------------------------------------------------- known answers
# (ntiles, spp, depth, knobs) -> group_tiles, ns, cap, slots, chunks, samples per chunk of the first group, bytes
KNOWN = {
    "c2_1080p_256spp": (frame(tiles(1920, 1080), 256, 8), 8160, 24, 50135040, 2, 12,
                        [256 * (c + 1) // 12 - 256 * c // 12 for c in range(12)], 28627416576),
    "1080p_256spp_depth50": (frame(tiles(1920, 1080), 256, 50), 8160, 128, 267386880, 2, 2, [128, 128],
                             242304231424),
    "1080p_8spp_4m": (frame(tiles(1920, 1080), 8, 8, 1 << 22), 8160, 2, 4177920, 2, 4, [2, 2, 2, 2], 2431588864),
    "2160p_2spp_4m": (frame(tiles(3840, 2160), 2, 8, 1 << 22), 16384, 1, 4194304, 2, 4, [1, 1], 2491456000),
    "900p_1spp_depth50": (frame(tiles(1600, 900), 1, 50), 5700, 1, 1459200, 1, 1, [1], 696058112),
    "smoke_48x27": (frame(tiles(48, 27), 2, 8), 6, 2, 3072, 1, 1, [2], 925184),
    "37x21_3spp_300": (frame(tiles(37, 21), 3, 8, 300), 1, 1, 256, 2, 18, [1, 1, 1], 175104),
    "37x21_5spp_3072": (frame(tiles(37, 21), 5, 8, 3072), 6, 2, 3072, 2, 4, [1, 1, 1, 2], 1805312),
    "70x45_2spp_1792_slots3": (frame(tiles(70, 45), 2, 8, 1792, slots=3), 7, 1, 1792, 3, 6, [1, 1], 1601024),
    "70x45_2spp_1792_slots1": (frame(tiles(70, 45), 2, 8, 1792, slots=1), 7, 1, 1792, 1, 6, [1, 1], 567808),
    "64x64_4spp_1024": (frame(tiles(64, 64), 4, 8, 1024), 4, 1, 1024, 2, 16, [1, 1, 1, 1], 629760),
    "96x54_4spp_768": (frame(tiles(96, 54), 4, 8, 768), 3, 1, 768, 2, 32, [1, 1, 1, 1], 478208),
}


@pytest.mark.parametrize("name", sorted(KNOWN))
def test_known_plans(L, name):
    inp, group_tiles, ns, cap, slots, nchunks, samples, nbytes = KNOWN[name]
    pl, lay, chunks = plan_of(L, inp)
    assert (pl["group_tiles"], pl["ns"], pl["cap"], pl["slots"]) == (group_tiles, ns, cap, slots)
    assert len(chunks) == nchunks
    assert [c[3] for c in chunks if c[0] == 0] == samples
    assert pl["bytes"] == nbytes == lay[25]


def test_known_plans_groups_and_steps(L):
    """What the table says beyond its columns: the tile groups' sizes, the steps, the C2 boundaries."""
    def groups(name):
        chunks = plan_of(L, KNOWN[name][0])[2]
        return sorted({(c[0], c[1]) for c in chunks})

    def steps(name):
        return [c[5] for c in plan_of(L, KNOWN[name][0])[2]]

    assert tiles(3840, 2160) == 16384 + 16016
    assert groups("2160p_2spp_4m") == [(0, 16384), (16384, 16016)]
    assert groups("70x45_2spp_1792_slots3") == [(0, 7), (7, 7), (14, 1)]
    assert len(groups("37x21_3spp_300")) == 6
    # two slots: a group's three chunks take two steps
    assert steps("37x21_3spp_300") == [2 * g + c // 2 for g in range(6) for c in range(3)]
    assert steps("37x21_3spp_300")[-1] == 11
    assert steps("70x45_2spp_1792_slots1") == list(range(6))
    assert [c[4] for c in plan_of(L, KNOWN["70x45_2spp_1792_slots3"][0])[2]] == [0, 1] * 3
    c2 = plan_of(L, KNOWN["c2_1080p_256spp"][0])[2]
    assert [c[2] for c in c2] == [256 * c // 12 for c in range(12)]
    assert [c[3] for c in c2][:3] == [21, 21, 22] and c2[-1][3] == 22
    assert [(c[4], c[5]) for c in c2] == [(c % 2, c // 2) for c in range(12)]


# ------------------------------------------------------------------- memory fit
def test_memory_fit(L):
    """A deep textured 1080p frame that selects its march jobs itself asks for more than any device has at the
    depth's default 2^28 paths, and is halved until it fits what the workspace may take."""
    deep = dict(ntiles=tiles(1920, 1080), spp=256, depth=50, textured=1, presel=0)
    need = {p: plan_of(L, frame(wf_paths=1 << p, **deep))[0]["bytes"] for p in (28, 27, 26)}
    assert abs(need[28] / 1e9 - 862.6) < 0.1 and abs(need[27] / 1e9 - 431.3) < 0.1 and abs(need[26] / 1e9 - 215.7) < 0.1
    # unknown: no halving
    pl = plan_of(L, frame(**deep))[0]
    assert pl["cap_want"] == 1 << 28 and pl["bytes"] == need[28]
    # 250 GB: two halvings
    pl = plan_of(L, frame(avail=250 * 10**9, **deep))[0]
    assert pl["cap_want"] == 1 << 26 and pl["bytes"] == need[26] <= 250 * 10**9
    # nothing fits: the smallest chunks, and still a plan (the allocation then fails)
    pl, lay, chunks = plan_of(L, frame(avail=0, **deep))
    assert pl["cap_want"] == MIN_CHUNK_PATHS and pl["bytes"] > 0 and pl["ns"] == 1
    assert sum(c[3] for c in chunks if c[0] == 0) == 256
    # a fit at the first try is left alone
    pl = plan_of(L, frame(avail=need[28], **deep))[0]
    assert pl["cap_want"] == 1 << 28


# ----------------------------------------------------------------- golden table
def test_golden_plans(L):
    cases = json.loads((HERE / "golden" / "wave_plans.json").read_text())
    assert len(cases) == 40
    for c in cases:
        r = G.evaluate(L, c["input"])
        assert r["plan"] == c["plan"], c["input"]
        assert r["layout"] == c["layout"], c["input"]
        assert len(r["chunks"]) == c["nchunks"], c["input"]
        assert G.digest(r["chunks"]) == c["chunks_sha256"], c["input"]
        if "chunks" in c:
            assert r["chunks"] == c["chunks"], c["input"]


# ------------------------------------------------------------------- invariants
def model(i):
    """The plan in Python integers (nothing wraps): the plan fields, the regions' sizes in layout order and the
    chunk list."""
    nsw = i["s_end"] - i["s_begin"]
    want = i["wf_paths"] or ((1 << 28) if i["depth"] > 16 else (3 << 24))

    def plan_for(want):
        group_tiles = min(i["ntiles"], max(want // 256, 1))
        npix = group_tiles * 256
        ns = min(max(want // npix, 1), nsw)
        mc = max(2 if i["progressive"] and i["wf_min_chunks"] < 2 else i["wf_min_chunks"], i["wf_slots"])
        if mc > 1 and i["ntiles"] <= group_tiles:
            ns = min(ns, max(-(-nsw // mc), -(-MIN_CHUNK_PATHS // npix)))
        cap = ns * npix
        cap_tiles = -(-cap // CP_TILE)
        slots = min(i["wf_slots"], -(-i["ntiles"] // group_tiles) * -(-nsw // ns))
        d1, cnt_words = i["depth"] + 1, (i["depth"] + 4) * 4
        sizes = [cap * PATH_BYTES, cap * PATH_BYTES, cap * 4 * d1, cap * 32, cap * 4, cap * 4, cap_tiles * CP_TILE,
                 (cap_tiles + CP_BLOCK) * 12, cnt_words * 4, cap * 24 * d1 if i["textured"] else 0,
                 cap * 64 if i["presel"] else 0]
        al = lambda n: -(-n // 256) * 256  # noqa: E731
        nbytes = slots * sum(al(s) for s in sizes) + al(npix * 24) + 8192
        return dict(cap_want=want, group_tiles=group_tiles, npix_max=npix, ns=ns, cap=cap, cap_tiles=cap_tiles,
                    slots=slots, iters=i["depth"] + 2, cnt_words=cnt_words, bytes=nbytes), sizes

    pl, sizes = plan_for(want)
    while pl["bytes"] > i["avail_bytes"] and want > MIN_CHUNK_PATHS:
        want = max(want // 2, MIN_CHUNK_PATHS)
        pl, sizes = plan_for(want)
    S = pl["slots"]
    n = -(-nsw // pl["ns"])
    if S > 1 and n > 1 and n % S:
        n += S - n % S
    n = min(n, nsw)
    chunks, step0 = [], 0
    for g0 in range(0, i["ntiles"], pl["group_tiles"]):
        gt = min(pl["group_tiles"], i["ntiles"] - g0)
        for c in range(n):
            s0, s1 = i["s_begin"] + nsw * c // n, i["s_begin"] + nsw * (c + 1) // n
            chunks.append([g0, gt, s0, s1 - s0, c % S, step0 + c // S])
        step0 += -(-n // S)
    return pl, sizes, chunks


def check_invariants(i, pl, lay, chunks):
    cap, S = pl["cap"], pl["slots"]
    assert cap % 64 == 0 and cap == pl["ns"] * pl["npix_max"] < 1 << 32
    assert 1 <= S <= min(i["wf_slots"], len(chunks))
    # every tile group's chunks cover [s_begin, s_end) once, in order, without an empty chunk; the groups the tiles
    g, s = 0, i["s_begin"]  # where the next chunk starts
    for g0, gt, s0, ns, slot, step in chunks:
        assert (g0, s0) == (g, s) and ns >= 1 and s0 + ns <= i["s_end"]
        assert gt == min(pl["group_tiles"], i["ntiles"] - g0) >= 1
        assert ns * gt * 256 <= cap
        s = s0 + ns
        if s == i["s_end"]:
            g, s = g0 + gt, i["s_begin"]
    assert (g, s) == (i["ntiles"], i["s_begin"])
    # steps: contiguous from 0, never decreasing; within one, slots 0, 1, ... in chunk order
    prev_step, prev_slot = -1, 0
    for *_, slot, step in chunks:
        if step != prev_step:
            assert step == prev_step + 1 and slot == 0
        else:
            assert slot == prev_slot + 1
        assert slot < S
        prev_step, prev_slot = step, slot
    # layout: 256-aligned regions that do not overlap and lie inside the workspace
    off, size = lay[:11], lay[11:22]
    stride, acc, acc_size, total = lay[22:]
    assert total == pl["bytes"]
    spans = []
    for k in range(S):
        for r in range(11):
            if size[r]:
                spans.append((k * stride + off[r], size[r]))
            else:
                assert REGIONS[r] in ("att", "jo")
    spans.append((acc, acc_size))
    end = 0
    for o, n in sorted(spans):
        assert o % 256 == 0 and o >= end
        end = o + n
    assert end <= total
    assert (size[9] != 0) == bool(i["textured"]) and (size[10] != 0) == bool(i["presel"])


def test_plan_invariants_sweep(L):
    rng = random.Random(7)
    for _ in range(3000):
        i = G.draw(rng)
        pl, lay, chunks = plan_of(L, i)
        mpl, msizes, mchunks = model(i)
        # the plan in Python integers: no 32-bit quantity wrapped, and every region holds what its user needs
        assert pl == mpl, i
        assert lay[11:22] == msizes and lay[24] == pl["npix_max"] * 24, i
        assert chunks == mchunks, i
        check_invariants(i, pl, lay, chunks)


def test_plan_invariants_of_known_frames(L):
    for name in KNOWN:
        i = KNOWN[name][0]
        check_invariants(i, *plan_of(L, i))
