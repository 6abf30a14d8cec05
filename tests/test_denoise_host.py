"""The guided denoiser on the CPU: the per-pixel functions of rs-pathtracing_amd/csrc/pt_denoise.hpp (the ones the
denoise_records and denoise_tiles kernels run per lane), compiled for the host by tests/native/Makefile and run
over every pixel, against the numpy restatement tests/denoiseref.py, bit for bit; the identities that need no
reference; the filter's quality against converged oracle frames; and pt_denoise's argument checks, which return
before any HIP call.  tests/test_gpu_denoise.py repeats the comparison with the same code compiled for gfx950."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import aovref
import denoiseref
from conftest import native_lib

NATIVE = Path(__file__).resolve().parent / "native"
GOLDEN = Path(__file__).resolve().parent / "golden"
INF = float("inf")


@pytest.fixture(scope="module")
def D():
    subprocess.run(["make", "-s", "-C", str(NATIVE), "_build/libdenoise.so"], check=True)
    L = C.CDLL(native_lib("libdenoise.so"))
    d = C.POINTER(C.c_double)
    L.dn_denoise.restype = C.c_size_t
    L.dn_denoise.argtypes = [d, d, d, d, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double, C.c_double, C.c_double,
                             C.c_uint32, d]
    return L


def host(D, rgb, albedo, normal, depth, w, h, iterations=5, sigma_normal=0.5, sigma_depth=0.1, sigma_colour=0.0,
         demodulate=True):
    d = C.POINTER(C.c_double)
    arrs = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (rgb, albedo, normal, depth)]
    out = np.full((w * h, 3), -7.25)
    used = D.dn_denoise(*[None if a is None else a.ctypes.data_as(d) for a in arrs], w, h, iterations, sigma_normal,
                        sigma_depth, sigma_colour, 1 if demodulate else 0, out.ctypes.data_as(d))
    assert used == w * h * 12
    return out


def same(got, ref):
    assert np.all(np.isfinite(got))
    bad = np.flatnonzero(np.any(got != ref, axis=1))
    assert bad.size == 0, "%d of %d pixels differ (first %s)" % (bad.size, len(ref), bad[:8].tolist())


def planes_of(name):
    w, h, img, pl = denoiseref.frame(name)
    return w, h, (img, pl["albedo"], pl["normal"], pl["depth"])


# ---- bit for bit against the numpy restatement ----

@pytest.mark.parametrize("name", ["cornell", "spheres"])
def test_oracle_frames_equal_the_restatement(D, name):
    w, h, fr = planes_of(name)
    aovref.assert_not_degenerate(fr[3])
    got = host(D, *fr, w, h)
    same(got, denoiseref.denoise(*fr, w, h))
    assert np.any(got != fr[0])  # the filter did something


SETTINGS = {
    "defaults": {},
    "colour_on": dict(sigma_colour=4.0),
    "no_demodulation": dict(demodulate=False),
    "one_iteration": dict(iterations=1),
    "eight_iterations": dict(iterations=8),
    "sigma_inf": dict(sigma_normal=INF, sigma_depth=INF, sigma_colour=INF),
}


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_random_planes_equal_the_restatement(D, setting):
    w, h = 40, 24
    fr = denoiseref.random_planes(w, h)
    rgb, albedo, normal, depth = fr
    # the planes hold what they are for: zero coverage, albedo at, below and above the threshold
    assert np.sum(depth[:, 0] == 0.0) >= 50 and np.sum(albedo == 1e-3) >= 50 and np.sum(albedo < 1e-3) >= 50
    assert np.sum(albedo > 1e-3) >= 1000
    kw = SETTINGS[setting]
    got = host(D, *fr, w, h, **kw)
    ref = denoiseref.denoise(*fr, w, h, **kw)
    same(got, ref)
    if setting == "no_demodulation":
        same(host(D, rgb, None, normal, depth, w, h, **kw), ref)  # the albedo is not read
    if setting == "colour_on":
        assert np.any(got != denoiseref.denoise(*fr, w, h))  # the term is not a no-op


def crop(fr, w, cw, ch):
    """The top-left cw x ch pixels of (w*h, 3) planes."""
    return tuple(np.ascontiguousarray(a.reshape(-1, w, 3)[:ch, :cw]).reshape(cw * ch, 3) for a in fr)


@pytest.mark.parametrize("cw,ch", [(20, 13), (17, 1), (1, 1)])
def test_small_shapes(D, cw, ch):
    fr = crop(denoiseref.random_planes(40, 24), 40, cw, ch)
    got = host(D, *fr, cw, ch)
    same(got, denoiseref.denoise(*fr, cw, ch))
    if (cw, ch) == (20, 13):
        # lower than the fifth iteration's stride of 16, and in columns 4..15 narrower too (x - 16 < 0, x + 16 >=
        # 20): there that iteration has the centre tap alone, u' = (w * u) / w with w = 9/64.  That is u up to
        # the product's and the quotient's rounding (not bit for bit: 7 % of random doubles change in the last
        # place), and out = u * den rounds each side once more: four roundings of at most 2^-53 each between the
        # two frames, second-order terms under the fifth.  Columns 0..3 and 16..19 have a second tap in the frame.
        four = host(D, *fr, cw, ch, iterations=4)
        same(four, denoiseref.denoise(*fr, cw, ch, iterations=4))
        alone = np.zeros((ch, cw), dtype=bool)
        alone[:, 4:16] = True
        alone = alone.reshape(-1)
        assert np.allclose(got[alone], four[alone], rtol=5 * 2.0 ** -53, atol=0.0)
        assert not np.allclose(got[~alone], four[~alone], rtol=1e-6, atol=0.0)  # there it filtered
    if (cw, ch) == (1, 1):
        assert np.allclose(got, fr[0], rtol=1e-15, atol=0.0)  # every iteration is the centre tap alone


# ---- identities without the reference ----

def test_colour_equal_to_albedo_returns_the_albedo(D):
    """With every albedo channel above 1e-3, u is identically 1: acc and ws are the same sums of the same terms,
    acc / ws is 1.0 and the frame is the albedo, bit for bit.  (A channel at or below the threshold keeps u = a
    there, which its neighbours then see: the identity needs the whole plane above it.)"""
    w, h = 40, 24
    _, albedo, normal, depth = denoiseref.random_planes(w, h)
    albedo = np.where(albedo > 1e-3, albedo, 0.5)
    assert np.array_equal(host(D, albedo, albedo, normal, depth, w, h), albedo)
    assert np.array_equal(host(D, albedo, albedo, normal, depth, w, h, sigma_colour=4.0, iterations=8), albedo)


def test_constant_colour_is_preserved(D):
    """Under unit albedo.  A colour that is a power of two scales every weight exactly, so acc = c * ws and the
    quotient is c bit for bit.  Any other constant comes back within the sums' rounding: per iteration 25
    products, 24 + 24 additions of positive terms and one division, under 52 roundings of 2^-53 each, and an
    iteration passes the last one's error on as a convex combination, so 5 iterations stay under 5 * 52 of them."""
    w, h = 40, 24
    _, _, normal, depth = denoiseref.random_planes(w, h)
    one = np.ones((w * h, 3))
    rgb = np.tile([0.25, 2.0, 0.5], (w * h, 1))
    assert np.array_equal(host(D, rgb, one, normal, depth, w, h), rgb)
    assert np.array_equal(host(D, rgb, None, normal, depth, w, h, demodulate=False, sigma_colour=4.0), rgb)
    rgb = np.tile([0.3, 1.7, 0.05], (w * h, 1))
    assert np.allclose(host(D, rgb, one, normal, depth, w, h), rgb, rtol=5 * 52 * 2.0 ** -53, atol=0.0)


def test_in_place(D):
    w, h, fr = planes_of("spheres")
    buf = fr[0].copy()
    d = C.POINTER(C.c_double)
    p = [a.ctypes.data_as(d) for a in (buf, *[np.ascontiguousarray(a) for a in fr[1:]])]
    D.dn_denoise(*p, w, h, 5, 0.5, 0.1, 0.0, 1, p[0])
    same(buf, denoiseref.denoise(*fr, w, h))


# ---- quality against converged oracle frames ----

def test_cornell_quality():
    """cornell 96x54: 4 spp at seed 3 against 1024 spp at seed 77 (depth 8, scene seed 1; the committed
    tests/golden/denoise_cornell_ref.npy, written by tests/golden/make_denoise_ref.py).  The RMS of the linear
    difference falls to at most 0.20 of the noisy frame's; the unguided filter (both guide sigmas +inf) is worse
    than the guided one."""
    w, h, fr = planes_of("cornell")
    ref = np.load(GOLDEN / "denoise_cornell_ref.npy")
    assert ref.shape == (w * h, 3)
    before = denoiseref.rms(fr[0], ref)
    guided = denoiseref.rms(denoiseref.denoise(*fr, w, h), ref)
    unguided = denoiseref.rms(denoiseref.denoise(*fr, w, h, sigma_normal=INF, sigma_depth=INF), ref)
    print("cornell: before %.4f, guided %.4f (%.4fx), unguided %.4f (%.4fx)"
          % (before, guided, guided / before, unguided, unguided / before))
    assert guided / before <= 0.20
    assert unguided > guided


def test_cornell_quality_of_the_host_build(D):
    """The same figure from the product's own code (the host build), not the restatement."""
    w, h, fr = planes_of("cornell")
    ref = np.load(GOLDEN / "denoise_cornell_ref.npy")
    assert denoiseref.rms(host(D, *fr, w, h), ref) / denoiseref.rms(fr[0], ref) <= 0.20


def test_spheres_quality(D):
    """spheres 64x64: 4 spp at seed 3 against 512 spp at seed 77, rendered here (seconds)."""
    _, _, w, h, _, osc, _ = aovref.case("spheres")
    _, _, fr = planes_of("spheres")
    ref = osc.render(w, h, 512, 8, 77)
    before, after = denoiseref.rms(fr[0], ref), denoiseref.rms(host(D, *fr, w, h), ref)
    print("spheres: before %.5f, after %.5f (%.4fx)" % (before, after, after / before))
    assert after / before < 1.0


# ---- the C-ABI: exports and argument errors (no HIP call is made) ----

def test_exports(pt):
    L = C.CDLL(str(pt.LIB_PATH))
    for name in ("pt_denoise_workspace_doubles", "pt_denoise_device", "pt_denoise"):
        assert name in pt.EXPORTS and hasattr(L, name)
    assert pt.denoise_workspace_doubles(0, 7) == 0 and pt.denoise_workspace_doubles(7, 0) == 0
    assert pt.denoise_workspace_doubles(40, 24) == 40 * 24 * 12
    assert pt.DENOISE_DEMODULATE == 1 and pt.DENOISE_MAX_ITERATIONS == 8
    assert "0.4.3" in pt.version() and pt.lib().pt_abi_version() == 4


NAN = float("nan")
BAD = {
    "null_rgb": dict(rgb=None),
    "null_normal": dict(normal=None),
    "null_depth": dict(depth=None),
    "null_albedo_with_demodulation": dict(albedo=None),
    "null_out": dict(out=None),
    "zero_width": dict(w=0),
    "zero_height": dict(h=0),
    "no_iterations": dict(iterations=0),
    "nine_iterations": dict(iterations=9),
    "unknown_flag": dict(flags=3),
    "unknown_flag_alone": dict(flags=2),
    "sigma_normal_zero": dict(sn=0.0),
    "sigma_normal_negative": dict(sn=-0.5),
    "sigma_normal_nan": dict(sn=NAN),
    "sigma_depth_zero": dict(sd=0.0),
    "sigma_depth_nan": dict(sd=NAN),
    "sigma_colour_negative": dict(sc=-1.0),
    "sigma_colour_nan": dict(sc=NAN),
}


# two bad arguments at once: the order of the checks decides which message wins
BAD.update({
    "null_rgb_and_unknown_flag": dict(rgb=None, flags=2),
    "unknown_flag_and_zero_width": dict(flags=2, w=0),
    "null_albedo_and_zero_height": dict(albedo=None, h=0),
    "zero_width_and_no_iterations": dict(w=0, iterations=0),
    "nine_iterations_and_sigma_normal_zero": dict(iterations=9, sn=0.0),
    "sigma_depth_nan_and_sigma_colour_negative": dict(sd=NAN, sc=-1.0),
    "sigma_colour_nan_and_too_large": dict(sc=NAN, w=1 << 20, h=1 << 20),
})


# pt_last_error() of each case, recorded from the build before the checks were given one spelling each
MESSAGES = {'null_rgb': b'null argument',
 'null_normal': b'null argument',
 'null_depth': b'null argument',
 'null_albedo_with_demodulation': b'PT_DENOISE_DEMODULATE needs the albedo plane',
 'null_out': b'null argument',
 'zero_width': b'width and height must be > 0',
 'zero_height': b'width and height must be > 0',
 'no_iterations': b'iterations must be 1..8',
 'nine_iterations': b'iterations must be 1..8',
 'unknown_flag': b'unknown denoise flag',
 'unknown_flag_alone': b'unknown denoise flag',
 'sigma_normal_zero': b'sigma_normal and sigma_depth must be > 0',
 'sigma_normal_negative': b'sigma_normal and sigma_depth must be > 0',
 'sigma_normal_nan': b'sigma_normal and sigma_depth must be > 0',
 'sigma_depth_zero': b'sigma_normal and sigma_depth must be > 0',
 'sigma_depth_nan': b'sigma_normal and sigma_depth must be > 0',
 'sigma_colour_negative': b'sigma_colour must be >= 0',
 'sigma_colour_nan': b'sigma_colour must be >= 0',
 'null_rgb_and_unknown_flag': b'null argument',
 'unknown_flag_and_zero_width': b'unknown denoise flag',
 'null_albedo_and_zero_height': b'PT_DENOISE_DEMODULATE needs the albedo plane',
 'zero_width_and_no_iterations': b'width and height must be > 0',
 'nine_iterations_and_sigma_normal_zero': b'iterations must be 1..8',
 'sigma_depth_nan_and_sigma_colour_negative': b'sigma_normal and sigma_depth must be > 0',
 'sigma_colour_nan_and_too_large': b'sigma_colour must be >= 0'}
MESSAGES_DEVICE = {'null_work': b'null argument',
 'misaligned_work': b'the workspace must be 16-byte aligned',
 'nine_iterations': b'iterations must be 1..8',
 'sigma_normal_nan': b'sigma_normal and sigma_depth must be > 0',
 'null_work_and_nine_iterations': b'iterations must be 1..8',
 'misaligned_work_and_null_out': b'null argument',
 'null_work_and_zero_width': b'width and height must be > 0'}


def host_refusal(pt, bad):
    """pt_denoise with the arguments of `bad` replaced: (status, message, the out buffer)."""
    w, h = 8, 4
    d = C.POINTER(C.c_double)
    a = dict(rgb=np.ones((w * h, 3)), albedo=np.ones((w * h, 3)), normal=np.zeros((w * h, 3)),
             depth=np.ones((w * h, 3)), out=np.full((w * h, 3), -7.25), w=w, h=h, iterations=5, sn=0.5, sd=0.1, sc=0.0,
             flags=1)
    out = a["out"]
    a.update(bad)
    ptr = {k: None if a[k] is None else a[k].ctypes.data_as(d) for k in ("rgb", "albedo", "normal", "depth", "out")}
    rc = pt.lib().pt_denoise(-1, ptr["rgb"], ptr["albedo"], ptr["normal"], ptr["depth"], a["w"], a["h"],
                             a["iterations"], a["sn"], a["sd"], a["sc"], a["flags"], ptr["out"])
    return rc, pt.lib().pt_last_error(), out


@pytest.mark.parametrize("case", list(BAD))
def test_argument_errors(pt, case):
    rc, message, out = host_refusal(pt, BAD[case])
    assert rc == pt.PT_ERR_INVALID, (case, rc)
    assert message == MESSAGES[case]  # the text, as recorded before the checks were given one spelling each
    assert np.all(out == -7.25)  # a refused call writes nothing


def device_refusal(pt, bad):
    """pt_denoise_device likewise; the pointers are never dereferenced on the host.  (status, message, the buffer)"""
    w, h = 8, 4
    buf = np.zeros(w * h * 3 + w * h * 12 + 2)
    base = buf.ctypes.data
    a = dict(work=(base + w * h * 24 + 15) & ~15, iterations=5, sn=0.5, w=w, out=base)
    a.update(bad)
    if a["work"] == "misaligned":
        a["work"] = ((base + w * h * 24 + 15) & ~15) + 8
    L = pt.lib()
    rc = L.pt_denoise_device(-1, base, base, base, base, a["w"], h, a["iterations"], a["sn"], 0.1, 0.0, 1, a["out"],
                             a["work"], None)
    return rc, L.pt_last_error(), buf


BAD_DEVICE = {
    "null_work": dict(work=None),
    "misaligned_work": dict(work="misaligned"),
    "nine_iterations": dict(iterations=9),
    "sigma_normal_nan": dict(sn=NAN),
    "null_work_and_nine_iterations": dict(work=None, iterations=9),  # the shared checks come first
    "misaligned_work_and_null_out": dict(work="misaligned", out=None),
    "null_work_and_zero_width": dict(work=None, w=0),
}


def test_device_form_argument_errors(pt):
    """The device form's checks come before its first HIP call too: the shared ones, then a null and a misaligned
    workspace."""
    for case, bad in BAD_DEVICE.items():
        rc, message, buf = device_refusal(pt, bad)
        assert rc == pt.PT_ERR_INVALID, (case, rc)
        assert message == MESSAGES_DEVICE[case], case
        assert np.all(buf == 0.0)
