"""Adversarial rays for the five marched functions of the generic march (Sine, Star, DupinCyclide, HuntsSurface,
Cushion; tests/adversarial.py: CASES, object_rays_for) through the host build of the product's skipping march
(pt_march.hpp + pt_funcs.hpp in libpath.so) against the oracle's literal march (ray_marching.rs:20-74): rays
grazing the surface, frozen coordinates, the singular lines and points, power-of-two origins, rays tangent to the
bound sphere and origins on and inside it; at the identity, a uniform scale of 40 and a rotated non-uniform scale;
at seven step / depth settings.  Closest hits and whole paths are compared bit for bit, NaN equal to NaN: a march
stopped on a singular point has the normalised zero gradient for its normal, and the path that scatters from it
is NaN from there on.  The same rays run through the GPU kernels in test_gpu_marched_adversarial.py."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import adversarial as A
from test_march_exact import march_lib  # noqa: F401  (fixture)
from test_path_host import H, Pair  # noqa: F401  (fixture + helper)

NAMES = [c["name"] for c in A.CASES]
XFS = ["identity", "scale40", "rot"]


def host_hit_records(pair, rays):
    out = A.hit_records(len(rays))
    for i, ray in enumerate(rays):
        who, t, p, n, f = pair.closest(ray)
        if who >= 0:
            out[i] = (who, t, p, n, f)
    return out


class Dual:
    """A value and its three partial derivatives in exact rationals (forward mode)."""

    def __init__(self, v, g=(0, 0, 0)):
        self.v, self.g = Fraction(v), tuple(Fraction(x) for x in g)

    @staticmethod
    def lift(x):
        return x if isinstance(x, Dual) else Dual(x)

    def __add__(self, o):
        o = Dual.lift(o)
        return Dual(self.v + o.v, [a + b for a, b in zip(self.g, o.g)])

    def __mul__(self, o):
        o = Dual.lift(o)
        return Dual(self.v * o.v, [self.v * b + o.v * a for a, b in zip(self.g, o.g)])

    __radd__, __rmul__ = __add__, __mul__

    def __pow__(self, n):
        r = Dual(1)
        for _ in range(n):
            r = r * self
        return r


def magnitude_reference(shape, x, y, z):
    """What shape_mag has to return (pt_funcs.hpp, DM): the function as the reference writes it
    (ray_marching.rs:202-472), every subtraction an addition and every constant its absolute value, so that each
    intermediate of the f64 evaluation is bounded by the matching intermediate here; and that polynomial's partial
    derivatives, which bound |df/dx_k| in the same way.  Written out by hand, in exact rationals."""
    r2 = x * x + y * y + z * z
    kind = shape["type"]
    if kind == "Sine":
        aa = Fraction(float(shape["a"]) * float(shape["a"]))  # the f64 product the function forms first
        return aa * (x + y + z) ** 4 + 4 * x * x * y * y * z * z
    if kind == "Star":
        return abs(Fraction(shape["a"])) * (x * x * y * y + x * x * z * z + y * y * z * z) + (r2 + 1) ** 3
    if kind == "DupinCyclide":
        a, b, c, d = (Fraction(shape[k]) for k in "abcd")
        b2, cd, d2 = Fraction(float(b) * float(b)), Fraction(float(c) * float(d)), Fraction(float(d) * float(d))
        return (r2 + b2 + d2) ** 2 + 4 * ((abs(a) * x + abs(cd)) ** 2 + b2 * y * y)
    if kind == "HuntsSurface":
        return 4 * (r2 + 13) ** 3 + 27 * (3 * x * x + y * y + 4 * z * z + 12) ** 2
    assert kind == "Cushion"
    x2, y2, z2 = x * x, y * y, z * z
    return (z2 * x2 + z2 * z2 + 2 * z * x2 + 2 * z * z2 + x2 + z2 + (x2 + z) ** 2 + y2 * y2 + 2 * x2 * y2 + y2 * z2
            + 2 * y2 * z + y2)


@pytest.mark.parametrize("name", NAMES)
def test_magnitude_bound_is_the_absolute_polynomial(march_lib, name):
    """The margin of the sign proof is 1e-15 + 256 eps M + drift with (M, dM/dx_k) = shape_mag over the block's box.
    A bound half as large would still clear f's actual rounding error on every ray of this file (the 256 is that
    generous), so no ray shows it: M is held to its definition instead.  Every operation of shape_mag is a sum or a
    product of positive numbers, each rounding once (relative 2^-53), and no chain of them is longer than 64
    operations: the f64 result is within 64 * 2^-53 of the exact one.  It also bounds |f| inside the box."""
    import oracle as O
    case = A.CASE[name]
    shape = case["shape"]
    d = C.POINTER(C.c_double)
    march_lib.shape_mag_of.argtypes = [C.c_int, d, C.c_double, C.c_double, C.c_double, d]
    march_lib.shape_mag_of.restype = None
    if shape["type"] == "DupinCyclide":  # FParams::k as the loader fills it: a, b*b, c*d, d*d
        k = [shape["a"], shape["b"] * shape["b"], shape["c"] * shape["d"], shape["d"] * shape["d"]]
    else:
        k = [shape.get("a", 0.0), 0.0, 0.0, 0.0]
    rng = np.random.default_rng(7)
    R = case["radius"]
    boxes = np.concatenate([rng.uniform(0, R, size=(12, 3)), [[0, 0, 0], [R, 0, 0], [0, R, R], [R, R, R],
                                                               [1e-9, 2.0 ** -30, R], [40 * R, 40 * R, 40 * R]]])
    out = (C.c_double * 4)()
    for xm, ym, zm in boxes:
        march_lib.shape_mag_of(O.FUNC_IDS[shape["type"]], (C.c_double * 4)(*k), xm, ym, zm, out)
        want = magnitude_reference(shape, Dual(float(xm), (1, 0, 0)), Dual(float(ym), (0, 1, 0)),
                                   Dual(float(zm), (0, 0, 1)))
        for got, exact in zip(out, (want.v,) + want.g):
            assert abs(Fraction(got) - exact) <= 64 * Fraction(2) ** -53 * exact, (name, (xm, ym, zm), got, float(exact))
        p = rng.uniform(-1, 1, size=(200, 3)) * [xm, ym, zm]
        assert np.all(np.abs(case["f"](p)) <= out[0])


def test_comparison_takes_nan_for_nan_and_nothing_else():
    a = A.hit_records(4)
    a[1] = (0, 1.5, [1, 2, 3], [np.nan, np.nan, np.nan], 1)
    a[2] = (0, 2.5, [1, 2, 3], [0, 1, 0], 0)
    assert A.hit_differences(a, a.copy()) == []
    b = a.copy()
    b[0] = a[2]          # a hit against a miss
    b[1]["normal"][0] = 0.0  # a number against a NaN
    b[2]["front_face"] = 1
    b[3] = a[2]
    b[3]["shape"] = -1   # a miss is a miss whatever else its record holds
    assert A.hit_differences(b, a) == [0, 1, 2]
    for k, v in (("t", 2.5000000000000004), ("point", [1, 2, 3.0000000000000004]), ("normal", [0, 1, -1e-300])):
        b = a.copy()
        b[2][k] = v
        assert A.hit_differences(b, a) == [2], k


def test_rays_are_deterministic_and_cover_the_families():
    for case in A.CASES:
        r1, f1 = A.object_rays_for(case, np.random.default_rng(5))
        r2, f2 = A.object_rays_for(case, np.random.default_rng(5))
        assert np.array_equal(r1, r2) and np.array_equal(f1, f2)
        assert 500 <= len(r1) <= 600 and np.all(np.isfinite(r1))
        assert sorted(set(f1.tolist())) == list(range(len(A.FAMILIES)))
        assert len(A.LEFT_OUT.get(case["name"], [])) <= 2


def test_oracle_hits_enough():
    """The oracle alone, at step 0.01 and depth 4: per case and transform at least 100 hits of the marched shape
    and one in each family that can hit; over the table at least 4 hits with a NaN normal.  Without these the
    comparisons below could pass on misses."""
    nan_normals = 0
    print()
    for name in NAMES:
        for xf in XFS:
            n, by, nn = A.hit_counts(name, xf)
            print("%-12s %-8s hits %3d  %s  NaN normals %d" % (name, xf, n, " ".join(
                "%s %d" % (f, by[f]) for f in A.FAMILIES), nn))
            nan_normals += nn
            if name in A.NEVER_HIT:
                assert n == 0
                continue
            assert n >= A.MIN_HITS, (name, xf, n)
            for f in A.MUST_HIT:
                assert by[f] >= 1, (name, xf, f)
    assert nan_normals >= A.MIN_NAN_NORMALS


@pytest.mark.parametrize("xf", XFS)
@pytest.mark.parametrize("name", NAMES)
def test_closest_hits_exact(H, name, xf):  # noqa: F811
    rays, _ = A.case_rays(name, xf)
    for step, depth in A.SETTINGS:
        pair = Pair(H, A.case_text(name, xf, step, depth), random_spheres=False)
        want = A.oracle_hits(name, xf, step, depth)
        bad = A.hit_differences(host_hit_records(pair, rays), want)
        assert not bad, "step %g depth %d: %d of %d rays differ, first %s: %s" % (
            step, depth, len(bad), len(rays), bad[:5], rays[bad[0]].tolist())


@pytest.mark.parametrize("xf", XFS)
@pytest.mark.parametrize("name", NAMES)
def test_whole_paths_exact(H, name, xf):  # noqa: F811
    rays, _ = A.case_rays(name, xf)
    before, want, after = A.oracle_paths(name, xf)
    pair = Pair(H, A.case_text(name, xf, *A.FLOOR_SETTING), random_spheres=False)
    out = (C.c_double * 3)()
    for i, ray in enumerate(rays):
        st = C.c_uint64(int(before[i]))
        H.h_ray_color(pair.h, (C.c_double * 6)(*ray), C.byref(st), A.PATH_DEPTH, out)
        assert np.array_equal(np.array(out[:]), want[i], equal_nan=True) and st.value == int(after[i]), (
            i, ray.tolist(), list(out), want[i])
    assert np.any(want > 0.0)  # the sky reaches some path's end
