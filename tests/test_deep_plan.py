"""The wavefront frame plan of deep frames (depth > 64, pt_plan.hpp), on the CPU: a host harness of its own
(tests/native/deep_plan_harness.cpp, built here with g++) gives the plan as make_plan makes it and the memory fit
launch_render_wave applies (make_plan_fit, fits_device, fits).  Checked against the same restatement in Python
integers as tests/test_wave_plan.py uses, where nothing can wrap."""
import ctypes as C
import random
import subprocess
import sys
from pathlib import Path

import pytest

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE / "golden"))
import make_wave_plans as G  # noqa: E402
import test_wave_plan as W  # noqa: E402  (model, check_invariants, frame, tiles: the parent's arithmetic restated)

UNKNOWN = G.UNKNOWN
MAX_DEPTH = 4096
MIN_CHUNK_PATHS = 1 << 21
# an MI355X: 288 GB of HBM the device can hold (hard), and what the workspace may take of it: less the 2 GiB reserve
MI355X_HARD = 288 * 10**9
MI355X_AVAIL = MI355X_HARD - (2 << 30)
RESERVE = 2 << 30
DEPTHS = (65, 1000, MAX_DEPTH)


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    out = tmp_path_factory.mktemp("deep_plan") / "libdeepplan.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-o", str(out),
                    str(HERE / "native" / "deep_plan_harness.cpp")], check=True)
    lib = G.load(out)
    u64p = C.POINTER(C.c_uint64)
    lib.plan_fit.argtypes = [u64p, C.c_uint64, u64p]
    lib.plan_fit.restype = None
    lib.plan_fits.argtypes = [u64p]
    lib.plan_fits.restype = C.c_int
    lib.plan_limits.argtypes = [u64p]
    lib.plan_limits.restype = None
    return lib


def words(inp):
    return (C.c_uint64 * 12)(*[int(inp[f]) for f in G.FIELDS])


def fit(L, inp, hard=None):
    """(plan, chunk streams planned for, the device can hold it, region sizes) of launch_render_wave's plan on a
    device that can hold `hard` bytes (default: avail_bytes plus the reserve, as hipMemGetInfo gives them)."""
    if hard is None:
        hard = UNKNOWN if inp["avail_bytes"] == UNKNOWN else inp["avail_bytes"] + RESERVE
    out = (C.c_uint64 * 23)()
    L.plan_fit(words(inp), hard, out)
    v = list(out)
    return dict(zip(W.PLAN, v[:10])), v[10], bool(v[11]), v[12:]


def test_limits(L):
    out = (C.c_uint64 * 8)()
    L.plan_limits(out)
    assert list(out) == [MAX_DEPTH, 64, MIN_CHUNK_PATHS, RESERVE, 0, 1, 1, 0]
    assert MAX_DEPTH >= 4096


def test_the_limit_has_one_value(pt):
    """PT_MAX_DEPTH in the header, plan::MAX_DEPTH (tied to it by a static_assert in pt_api.cpp) and the Python
    binding's MAX_DEPTH are the same number."""
    import re
    text = (HERE.parent / "include" / "rs_pathtracing.h").read_text()
    (value,) = re.findall(r"^#define PT_MAX_DEPTH (\d+)$", text, flags=re.M)
    assert int(value) == MAX_DEPTH == pt.MAX_DEPTH


def test_depth_above_the_limit_wraps_nothing(L):
    """plan_for plans any depth above the limit as the limit (launch_render_wave refuses such a frame first)."""
    at = W.plan_of(L, W.frame(W.tiles(64, 64), 4, MAX_DEPTH, textured=1))
    for depth in (MAX_DEPTH + 1, 2**31 - 2, 2**31 - 1, 2**32 - 1):
        assert W.plan_of(L, W.frame(W.tiles(64, 64), 4, depth, textured=1)) == at, depth
    assert at[0]["iters"] == MAX_DEPTH + 2


@pytest.mark.parametrize("textured", [0, 1])
@pytest.mark.parametrize("depth", DEPTHS)
def test_deep_plan_arithmetic(L, depth, textured):
    """iters, cnt_words and every region's size equal the formula in unbounded integers, for a small frame, a
    1080p 256-spp frame at the default 2^28 paths (the ids region alone passes 2^40 bytes at the limit) and the
    same frame on an MI355X's memory."""
    for inp in (W.frame(W.tiles(32, 32), 2, depth, textured=textured),
                W.frame(W.tiles(1920, 1080), 256, depth, textured=textured),
                W.frame(W.tiles(1920, 1080), 256, depth, textured=textured, slots=1, avail=MI355X_AVAIL),
                W.frame(W.tiles(3840, 2160), 7, depth, wf_paths=1 << 22, slots=3, textured=textured, presel=0,
                        s_begin=2, s_end=6)):
        pl, lay, chunks = W.plan_of(L, inp)
        mpl, msizes, mchunks = W.model(inp)
        assert pl["iters"] == depth + 2 and pl["cnt_words"] == (depth + 4) * 4
        assert pl == mpl, inp
        cap, d1 = pl["cap"], depth + 1
        assert lay[11:22] == msizes, inp
        assert lay[11 + 2] == cap * 4 * d1 and lay[11 + 9] == (cap * 24 * d1 if textured else 0)
        assert lay[11 + 8] == (depth + 4) * 16
        assert chunks == mchunks, inp
        assert pl["bytes"] < 2**63  # (and equal to the unbounded sum: pl == mpl)
        W.check_invariants(inp, pl, lay, chunks)


def test_deep_plan_halves_to_the_floor(L):
    inp = W.frame(W.tiles(1920, 1080), 256, 1000, textured=1, avail=10**9)
    pl, lay, chunks = W.plan_of(L, inp)
    assert pl["cap_want"] == MIN_CHUNK_PATHS and pl["ns"] == 1 and pl["bytes"] > 10**9
    assert pl == W.model(inp)[0]
    # with room for it, the halving stops at the first size that fits
    need = {p: W.plan_of(L, W.frame(W.tiles(1920, 1080), 256, 1000, wf_paths=1 << p))[0]["bytes"] for p in (28, 24, 23)}
    pl = W.plan_of(L, W.frame(W.tiles(1920, 1080), 256, 1000, avail=need[24]))[0]
    assert pl["cap_want"] == 1 << 24 and pl["bytes"] == need[24]
    pl = W.plan_of(L, W.frame(W.tiles(1920, 1080), 256, 1000, avail=need[24] - 1))[0]
    assert pl["cap_want"] == 1 << 23 and pl["bytes"] == need[23]


def test_fit_check_at_the_floor(L):
    """fits() says "does not fit" exactly when the plan's bytes exceed avail_bytes, which after make_plan can only
    be at the floor.  That alone refuses nothing: the plan is run while the device can hold it (fits_device); beyond
    that make_plan_fit tries one chunk stream, and the frame is refused when the device cannot hold that either."""
    base = dict(ntiles=W.tiles(1920, 1080), spp=256, depth=MAX_DEPTH, textured=1)
    floor2 = W.plan_of(L, W.frame(wf_paths=MIN_CHUNK_PATHS, **base))[0]
    floor1 = W.plan_of(L, W.frame(wf_paths=MIN_CHUNK_PATHS, slots=1, **base))[0]
    assert floor2["slots"] == 2 and floor1["slots"] == 1 and floor1["bytes"] < floor2["bytes"]
    # fits(): bytes against avail_bytes
    for avail, fits2 in ((UNKNOWN, 1), (floor2["bytes"], 1), (floor2["bytes"] - 1, 0), (0, 0)):
        inp = W.frame(avail=avail, **base)
        pl = W.plan_of(L, inp)[0]
        assert L.plan_fits(words(inp)) == fits2 == int(pl["bytes"] <= avail), avail
        if not fits2:
            assert pl["cap_want"] == MIN_CHUNK_PATHS
    # the device: (hard bytes) -> streams planned for, held or refused
    for hard, slots_used, held in ((UNKNOWN, 2, True), (floor2["bytes"], 2, True), (floor2["bytes"] - 1, 1, True),
                                   (floor1["bytes"], 1, True), (floor1["bytes"] - 1, 1, False), (0, 1, False)):
        avail = UNKNOWN if hard == UNKNOWN else max(hard - RESERVE, 0)
        inp = W.frame(avail=avail, **base)
        fpl, slots, ok, sizes = fit(L, inp, hard)
        assert (slots, ok) == (slots_used, held), hard
        assert ok == (fpl["bytes"] <= hard)
        assert fpl == W.plan_of(L, W.frame(avail=avail, **dict(base, slots=slots)))[0]
    # this frame on an MI355X: two streams of the smallest chunks cannot be held, one can
    fpl, slots, ok, sizes = fit(L, W.frame(avail=MI355X_AVAIL, **base), MI355X_HARD)
    assert (slots, ok, fpl["cap_want"]) == (1, True, MIN_CHUNK_PATHS)
    # a frame that fits is planned as make_plan plans it
    inp = W.frame(W.tiles(1920, 1080), 256, 128, avail=MI355X_AVAIL)
    assert fit(L, inp, MI355X_HARD)[:3] == (W.plan_of(L, inp)[0], 2, True)


def test_frames_that_could_be_allocated_before_are_planned_as_before(L):
    """The reserve is a margin, not a limit.  A small frame of depth <= 64 with avail_bytes at 0 (less than 2 GiB
    free) keeps make_plan's plan and is not refused while the device can hold its few megabytes; so is a frame whose
    workspace the renderer already holds (hard_bytes counts it), and a deep one alike."""
    for depth in (8, 50, 64, 65, 500):
        for inp in (W.frame(W.tiles(48, 27), 2, depth, avail=0),
                    W.frame(W.tiles(256, 256), 16, depth, avail=0, textured=1),
                    W.frame(W.tiles(1920, 1080), 4, depth, avail=0, progressive=1)):
            pl = W.plan_of(L, inp)[0]
            assert not L.plan_fits(words(inp)) and pl == W.model(inp)[0]
            for hard in (1 << 30, pl["bytes"]):  # 1 GiB free; or nothing free and the workspace held covers it
                if pl["bytes"] <= hard:
                    assert fit(L, inp, hard)[:3] == (pl, inp["wf_slots"], True), (inp, hard)
            # the device cannot hold it: one stream is tried, then the frame is refused
            fpl, slots, ok, _ = fit(L, inp, pl["bytes"] - 1)
            assert slots == 1 and ok == (fpl["bytes"] <= pl["bytes"] - 1)


def test_fit_sweep(L):
    rng = random.Random(11)
    for _ in range(1500):
        inp = G.draw(rng)
        inp["depth"] = rng.choice([8, 64, 65, 127, 128, 500, 1000, MAX_DEPTH])
        pl, lay, chunks = W.plan_of(L, inp)
        mpl, msizes, mchunks = W.model(inp)
        assert pl == mpl and lay[11:22] == msizes and chunks == mchunks, inp
        W.check_invariants(inp, pl, lay, chunks)
        fits = pl["bytes"] <= inp["avail_bytes"]
        assert L.plan_fits(words(inp)) == int(fits), inp
        assert fits or pl["cap_want"] <= MIN_CHUNK_PATHS, inp  # a misfit only at the floor
        # the device holds what is available and the reserve, or (drawn) exactly as much as a random share of it
        soft = inp["avail_bytes"]
        hard = UNKNOWN if soft == UNKNOWN else soft + rng.choice([RESERVE, 0, rng.randint(0, RESERVE)])
        fpl, slots, ok, sizes = fit(L, inp, hard)
        if pl["bytes"] <= hard or inp["wf_slots"] == 1:
            assert (fpl, slots, ok) == (pl, inp["wf_slots"], pl["bytes"] <= hard), inp
        else:
            one = dict(inp, wf_slots=1)
            assert slots == 1 and fpl == W.model(one)[0] and ok == (fpl["bytes"] <= hard), inp


def test_plans_up_to_depth_64_are_the_parents(L):
    """Depths 33..64 (tests/golden/wave_plans.json pins 0, 1, 8, 50 and 64): the plan is the arithmetic this file's
    model restates, which is the parent's (test_wave_plan.py checks the model against the golden table); and the
    plan launch_render_wave runs is that plan whenever the device can hold it, inside the reserve or not."""
    rng = random.Random(64)
    for k in range(1600):
        inp = G.draw(rng)
        inp["depth"] = 33 + k % 32
        pl, lay, chunks = W.plan_of(L, inp)
        mpl, msizes, mchunks = W.model(inp)
        assert pl == mpl and lay[11:22] == msizes and chunks == mchunks, inp
        W.check_invariants(inp, pl, lay, chunks)
        for hard in (UNKNOWN, pl["bytes"], pl["bytes"] + RESERVE):
            assert fit(L, inp, hard)[:3] == (pl, inp["wf_slots"], True), inp


def test_workspace_of_deep_1080p_frames(L):
    """1080p at 256 spp on an MI355X (profiles/r7/deep_depth.txt records these): the chunk shrinks with the depth, and
    every depth up to 1000 fits on two streams."""
    rows = []
    for textured in (0, 1):
        for depth in (128, 500, 1000):
            fpl, slots, ok, sizes = fit(L, W.frame(W.tiles(1920, 1080), 256, depth, textured=textured,
                                                   avail=MI355X_AVAIL), MI355X_HARD)
            assert ok and slots == 2 and fpl["bytes"] <= MI355X_AVAIL
            rows.append((textured, depth, fpl["cap_want"], fpl["cap"], fpl["bytes"]))
    print("\ntextured depth cap_want cap bytes")
    for r in rows:
        print(*r)
    assert [r[2] for r in rows[:3]] == sorted((r[2] for r in rows[:3]), reverse=True)
