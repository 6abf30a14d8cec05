"""Which kernel build runs (rs-pathtracing_amd/csrc/pt_builds.hpp: builds::choose, the lists of the instantiated
builds, the knob table), built for the host by tests/native/Makefile and checked on the CPU over the whole input
space against a restatement of the launch cascades the choice replaced.  The restatement is written from the
sources of commit 7d8f969, the last one with the cascades (pt_kernel.hip and pt_wave.hip there; the line numbers
below are that commit's), with numpy arrays where those sources have scalars.

A part of the choice that the chosen engine does not run (the wavefront builds of a megakernel frame, everything
of a refused frame) is all zeros, in the choice and in the restatement."""
import ctypes as C
import itertools
import subprocess
from pathlib import Path

import numpy as np
import pytest

from conftest import native_lib

HERE = Path(__file__).resolve().parent

F_HEART, F_ANY, F_NONE = 0, -1, -2
MEGA, WAVE, REFUSE = 0, 1, 2
BIG = 1 << 15  # BIG_BVH_NODES (pt_types.hpp:110)
OUT = ("engine", "mega_nw", "mega_waves", "mega_fk", "b_waves", "b_fk", "b_ext", "b_bigbvh", "b_split", "b_deep",
       "b_diag", "walk_on", "walk_waves", "walk_qn", "march_on", "march_fk", "march_diag", "presel", "ext")
LISTS = {"mega": (0, OUT[1:4]), "bounce": (1, OUT[4:10]), "walk": (2, OUT[12:14]), "march": (3, OUT[15:16])}
COUNTS = {"mega": 8, "bounce": 17, "walk": 5, "march": 2}  # bounce: 34 wf_bounce kernels, two (FIRST) per build

# the frames: the scene's part (a Python loop) and the rest (arrays, one element per combination)
SCENE = {"ext": (0, 1), "fkind": (F_HEART, F_ANY), "nnodes": (0, BIG - 1, BIG), "nmarch": (0, 1, 2),
         "has_qnodes": (0, 1), "scene_diag": (0, 1)}
FRAME = {"depth": (0, 8, 9, 16, 17, 32, 33, 64, 65, 4096), "samples": ((1 << 22) - 1, 1 << 22),
         "window": (0, 1, 2),  # no, yes, yes and empty
         "diag": (0, 1, 2),    # (wave_diag_on, diag_buffer) = (0, 0), (0, 1), (1, 1)
         "engine": (0, 1, 2), "mega_waves": (2, 3, 4, 5), "wf_bounce_waves": (2, 3, 4, 5, 6, 8),
         "wf_walk": (0, 4, 5, 6, 8)}


@pytest.fixture(scope="module")
def L():
    subprocess.run(["make", "-s", "-C", str(HERE / "native"), "_build/libbuilds.so"], check=True)
    lib = C.CDLL(native_lib("libbuilds.so"))
    i64p = np.ctypeslib.ndpointer(np.int64, flags="C_CONTIGUOUS")
    lib.builds_choose.argtypes = [i64p, C.c_int64, i64p]
    lib.builds_choose.restype = None
    lib.builds_list.argtypes = [C.c_int, C.c_void_p]
    lib.knob_name.argtypes = [C.c_int]
    lib.knob_name.restype = C.c_char_p
    lib.knob_legal.argtypes = [C.c_int, i64p]
    lib.knobs_set.argtypes = [C.c_char_p, C.c_int64]
    lib.knobs_get.argtypes = [C.c_char_p, C.POINTER(C.c_int64)]
    return lib


def build_list(L, which, cols):
    n = L.builds_list(which, None)
    out = np.zeros((n, cols), dtype=np.int64)
    assert L.builds_list(which, out.ctypes.data) == n
    return [tuple(r) for r in out.tolist()]


def pick(knob, values, default):
    """`switch (knob)` with a case per value and a default: arm."""
    return np.where(np.isin(knob, values), knob, default)


def restated(s, f):
    """The choice of commit 7d8f969 for scene s (scalars) and frames f (arrays), as {field: array}."""
    n = len(f["depth"])
    z = np.zeros(n, dtype=np.int64)
    depth, knob, walk = f["depth"], f["wf_bounce_waves"], f["wf_walk"]
    window, empty = f["window"] >= 1, f["window"] == 2
    wave_diag_on, diag_buffer = f["diag"] == 2, f["diag"] >= 1
    # ---- the engine: launch_render, pt_kernel.hip:385-401, and use_wavefront, :376-383 (ws is never null)
    deep = depth > 64                                                     # :389
    diag_ok = (s["scene_diag"] & 1) == 0
    use_wf = np.where(f["engine"] == 1, False,                            # :379
                      np.where(f["engine"] == 2, True,                    # :380
                               diag_ok & ((s["nmarch"] > 0) | (f["samples"] >= 1 << 22))))  # :381-382
    if s["ext"]:
        use_wf = np.ones(n, dtype=bool)                                   # :377
    engine = np.where(deep, np.where(window & empty, REFUSE, WAVE),      # :389-394
                      np.where(window, np.where(empty, REFUSE, WAVE),     # :396-399
                               np.where(use_wf, WAVE, MEGA)))             # :401
    mega, wave = engine == MEGA, engine == WAVE
    r = {"engine": engine}
    # ---- the megakernel: pt_kernel.hip:405-419, PT_DISPATCH_NW :283-298
    heart8 = (depth <= 8) & (s["fkind"] == F_HEART)                       # :405
    nw = np.where(depth <= 8, 4, np.where(depth <= 16, 8, np.where(depth <= 32, 16, 32)))
    r["mega_nw"] = np.where(mega, nw, 0)                                  # :410-418
    r["mega_waves"] = np.where(mega, np.where(heart8, pick(f["mega_waves"], (2, 3, 5), 4), 2), 0)  # :409-418
    r["mega_fk"] = np.where(mega, np.where(heart8, F_HEART, F_ANY), 0)    # render_tiles' default FK is F_ANY, :26
    # ---- the wavefront engine: launch_render_wave, pt_wave.hip:1437 and :1502-1504
    big = s["nnodes"] >= BIG
    split = ~deep & (walk != 0) & (not s["ext"] and big and s["nmarch"] == 0)  # :1503, walk_split :1264-1266
    fkind = np.where(deep, -1, s["fkind"])                                # :1504
    # the bounce: launch_bounce_build, pt_wave.hip:1268-1318; the template defaults are wf_bounce's, :316-317
    rows = [
        (deep, (2, F_ANY, s["ext"], 0, 0, 1, 0)),                                        # :1271-1277
        (split, (pick(knob, (4, 5), 3), F_NONE, 0, 1, 1, 0, 0)),                         # :1278-1285
        (np.full(n, bool(s["ext"])), (2, F_ANY, 1, 0, 0, 0, 0)),                         # :1286-1289
        (fkind != F_HEART, (2, F_ANY, 0, 0, 0, 0, 0)),                                   # :1290-1293
        (wave_diag_on, (2, F_HEART, 0, 0, 0, 0, 1)),                                     # :1294-1297
        (np.full(n, big and s["nmarch"] == 0), (pick(knob, (4, 5), 3), F_NONE, 0, 1, 0, 0, 0)),  # :1298-1305
        ((knob == 3) & big, (3, F_HEART, 0, 1, 0, 0, 0)),                                # :1306-1309
        (np.ones(n, dtype=bool), (pick(knob, (2, 4, 5, 6, 8), 3), F_HEART, 0, 0, 0, 0, 0)),      # :1310-1317
    ]
    for j, name in enumerate(OUT[4:11]):
        v = z
        for cond, build in reversed(rows):  # the first row that matches wins
            v = np.where(cond, build[j], v)
        r[name] = np.where(wave, v, 0)
    # the walk: launched iff split (:1582), launch_walk :1330-1341
    on = wave & split
    r["walk_on"] = on
    r["walk_waves"] = np.where(on, pick(walk, (4, 6, 8), 5) if s["has_qnodes"] else 5, 0)
    r["walk_qn"] = np.where(on, 1 if s["has_qnodes"] else 0, 0)
    # the march: launched iff nmarch != 0 (:1586), launch_march :1344-1351 with the fkind of :1504
    on = wave & (s["nmarch"] != 0)
    r["march_on"] = on
    r["march_fk"] = np.where(on, np.where(fkind != F_HEART, F_ANY, F_HEART), 0)
    r["march_diag"] = np.where(on, fkind == F_HEART, 0)  # the generic build is launched with nullptr, :1348
    r["presel"] = np.where(wave, (s["nmarch"] == 1) & ~diag_buffer, 0)    # :1437
    r["ext"] = np.where(wave, s["ext"], 0)                                # launch_unwind, launch_reduce :1354-1373
    return {k: np.asarray(v).astype(np.int64) for k, v in r.items()}


def test_choice_over_the_whole_input_space(L):
    grids = np.meshgrid(*[np.array(v, dtype=np.int64) for v in FRAME.values()], indexing="ij")
    f = {k: g.ravel() for k, g in zip(FRAME, grids)}
    n = len(f["depth"])
    lists = {k: build_list(L, which, len(cols)) for k, (which, cols) in LISTS.items()}
    for k, entries in lists.items():
        assert len(entries) == COUNTS[k] and len(set(entries)) == len(entries), (k, entries)
    chosen = {k: set() for k in LISTS}
    cases = 0
    for sv in itertools.product(*SCENE.values()):
        s = dict(zip(SCENE, sv))
        inp = np.empty((n, 16), dtype=np.int64)
        for j, k in enumerate(SCENE):
            inp[:, j] = s[k]
        inp[:, 6], inp[:, 7] = f["depth"], f["samples"]
        inp[:, 8], inp[:, 9] = f["window"] >= 1, f["window"] == 2
        inp[:, 10], inp[:, 11] = f["diag"] == 2, f["diag"] >= 1
        for j, k in enumerate(("engine", "mega_waves", "wf_bounce_waves", "wf_walk")):
            inp[:, 12 + j] = f[k]
        out = np.empty((n, len(OUT)), dtype=np.int64)
        L.builds_choose(inp, n, out)
        want = restated(s, f)
        for j, name in enumerate(OUT):
            bad = np.flatnonzero(out[:, j] != want[name])
            assert bad.size == 0, "%s: scene %s, frame %s: %d, restated %d (%d cases differ)" % (
                name, s, {k: int(v[bad[0]]) for k, v in f.items()}, out[bad[0], j], want[name][bad[0]], bad.size)
        # the builds the frames run: those of the chosen engine, the walk and the march only where launched
        runs = {"mega": out[:, 0] == MEGA, "bounce": out[:, 0] == WAVE, "walk": out[:, 11] == 1,
                "march": out[:, 14] == 1}
        for k, (_, cols) in LISTS.items():
            # (a build's fields are in [-2, 32]: one base-64 digit each)
            keys = sum((out[runs[k], OUT.index(c)] + 2) << (6 * j) for j, c in enumerate(cols))
            chosen[k] |= {tuple(((key >> (6 * j)) & 63) - 2 for j in range(len(cols)))
                          for key in np.unique(keys).tolist()}
        cases += n
    assert cases == 9331200
    for k, entries in lists.items():
        assert chosen[k] <= set(entries), "%s: chosen but not instantiated: %s" % (k, chosen[k] - set(entries))
        assert set(entries) <= chosen[k], "%s: instantiated but never chosen: %s" % (k, set(entries) - chosen[k])


def test_record_of_launched_builds(L):
    """builds::Ran, what a frame reports it launched (pt_renderer_get_option "ran_*"; the device side is
    tests/test_gpu_builds.py): builds::key packs every instantiated build as `chosen` is packed above, so that
    HipRenderer.last_builds unpacks the list's own row; an empty record reads -1 everywhere; the names are read-only
    (no knob is called so) and nothing else is a name."""
    i64p = np.ctypeslib.ndpointer(np.int64, flags="C_CONTIGUOUS")
    L.ran_keys.argtypes = [C.c_int, i64p]
    L.ran_note.argtypes = [C.c_int, C.c_int64]
    L.ran_read.argtypes = [C.c_char_p, C.POINTER(C.c_int64)]
    names = ("ran_engine", "ran_mega", "ran_bounce", "ran_walk", "ran_march")

    def read(name):
        v = C.c_int64(-77)
        ok = L.ran_read(name.encode() if name is not None else None, C.byref(v))
        return ok, v.value

    L.ran_reset()
    assert [read(n) for n in names] == [(1, -1)] * 5
    for name in ("ran", "ran_", "ran_engine ", "ran_first", "engine", "bvh_nodes", "", None):
        assert read(name) == (0, -77), name
    pt = __import__("conftest").load_package()  # (importing the mirror loads no library)
    assert list(pt.BUILD_COLUMNS.items()) == [(k, len(cols)) for k, (_, cols) in LISTS.items()]
    seen = set()
    for k, (which, cols) in LISTS.items():
        entries = build_list(L, which, len(cols))
        keys = np.full(len(entries) + 1, -5, dtype=np.int64)
        assert L.ran_keys(which, keys) == len(entries) and keys[-1] == -5
        for entry, key in zip(entries, keys.tolist()):
            assert key == sum((f + 2) << (6 * j) for j, f in enumerate(entry)) and key >= 0, (k, entry)
            assert tuple(((key >> (6 * j)) & 63) - 2 for j in range(len(cols))) == entry  # last_builds' unpacking
            L.ran_note(1 + which, key)
            assert read("ran_" + k) == (1, key)
            seen.add((k, key))
        assert len({key for kk, key in seen if kk == k}) == len(entries)  # no two builds share a key
    for engine in (MEGA, WAVE):
        L.ran_note(0, engine)
        assert read("ran_engine") == (1, engine)
    L.ran_reset()
    assert [read(n) for n in names] == [(1, -1)] * 5
    # read-only: no knob has such a name, so tuning_set, which is all pt_renderer_set_option has, refuses them
    for n in names:
        assert L.knobs_set(n.encode(), 0) == 0 and L.knobs_get(n.encode(), C.byref(C.c_int64())) == 0
        assert n not in [L.knob_name(k).decode() for k in range(L.knob_count())]


# The options in the order the API reports them and their legal values: TUNING_NAMES, tuning_field and tuning_set of
# commit 7d8f969 (pt_kernel.hip:301-351).  A range is (lo, hi); wf_paths also takes 0.
KNOBS = [("engine", (0, 2)), ("mega_waves", (2, 5)), ("diag", (0, 1)), ("wf_slots", (1, 4)),
         ("wf_paths", (256, 1 << 28)), ("wf_min_chunks", (1, 4096)), ("wf_bounce_waves", {2, 3, 4, 5, 6, 8}),
         ("wf_march_slice", (0, 1 << 20)), ("wf_walk", {0, 4, 5, 6, 8}), ("bvh_leaf", (1, 16))]


def legal(name, spec, v):
    if isinstance(spec, set):
        return v in spec
    return spec[0] <= v <= spec[1] or (name == "wf_paths" and v == 0)


def test_knob_table_and_tuning_set(L):
    assert [L.knob_name(k).decode() for k in range(L.knob_count())] == [k for k, _ in KNOBS]
    assert L.knob_name(L.knob_count()) is None
    for k, (name, spec) in enumerate(KNOBS):
        row = np.zeros(16, dtype=np.int64)
        nset = L.knob_legal(k, row)
        lo, hi, or_zero, table_set = int(row[0]), int(row[1]), bool(row[2]), set(row[3:3 + nset].tolist())
        edges = {lo, hi} | table_set | (spec if isinstance(spec, set) else set(spec)) | {0, 7, 100, 255, 256}
        values = sorted({e + d for e in edges for d in (-2, -1, 0, 1, 2)} | {-(1 << 40), 1 << 40})
        for v in values:
            by_table = (lo <= v <= hi and (not table_set or v in table_set)) or (or_zero and v == 0)
            assert by_table == legal(name, spec, v), (name, v)
            L.knobs_reset()
            before = C.c_int64(-1)
            assert L.knobs_get(name.encode(), C.byref(before)) == 1
            assert L.knobs_set(name.encode(), v) == int(by_table), (name, v)
            after = C.c_int64(-1)
            assert L.knobs_get(name.encode(), C.byref(after)) == 1
            assert after.value == (v if by_table else before.value), (name, v)
    L.knobs_reset()
    for name, v in (("wf_bounce_waves", 7), ("wf_walk", 7), ("wf_paths", 100), ("wf_paths", 255), ("wf_walk", 1),
                    ("mega_waves", 6), ("no_such_option", 1)):
        assert L.knobs_set(name.encode(), v) == 0, (name, v)
    assert L.knobs_get(b"no_such_option", C.byref(C.c_int64())) == 0
    # the defaults: struct Tuning of commit 7d8f969 (pt_kernel.hpp:47-63)
    defaults = {"engine": 0, "mega_waves": 4, "diag": 0, "wf_slots": 2, "wf_paths": 0, "wf_min_chunks": 1,
                "wf_bounce_waves": 3, "wf_march_slice": 256, "wf_walk": 5, "bvh_leaf": 1}
    for name, v in defaults.items():
        got = C.c_int64(-1)
        assert L.knobs_get(name.encode(), C.byref(got)) == 1 and got.value == v, (name, got.value)
