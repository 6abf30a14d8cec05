"""The guided à-trous denoiser (pt_denoise; rs-pathtracing_amd/csrc/pt_denoise.hpp) restated in numpy: the same
float64 operations in the same association and the same tap order (dy outer, dx inner), whole frames at a time.
Every product, sum and quotient below is one numpy ufunc on float64 arrays, so nothing is contracted or reordered.

Shared by tests/test_denoise_host.py (the host build of the per-pixel functions), tests/test_gpu_denoise.py and
tests/test_cli_denoise.py; the frames and planes they share come from aovref.case and are computed once per
process."""
import functools

import numpy as np

import aovref

K = (3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0)
DEFAULTS = dict(iterations=5, sigma_normal=0.5, sigma_depth=0.1, sigma_colour=0.0, demodulate=True)


def _f(x):
    v = 1.0 - x
    m = np.where(v > 0.0, v, 0.0)
    return m * m


def _sq3(d):
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def denoise(rgb, albedo, normal, depth, w, h, iterations=5, sigma_normal=0.5, sigma_depth=0.1, sigma_colour=0.0,
            demodulate=True):
    """(w*h, 3) float64: the denoised frame of the (w*h, 3) colour and guide planes (albedo may be None without
    demodulate)."""
    c = np.asarray(rgb, dtype=np.float64).reshape(h, w, 3)
    n = np.asarray(normal, dtype=np.float64).reshape(h, w, 3)
    z = np.asarray(depth, dtype=np.float64).reshape(h, w, 3)[..., 0]
    if demodulate:
        a = np.asarray(albedo, dtype=np.float64).reshape(h, w, 3)
        den = np.where(a > 1e-3, a, 1.0)
        u = c / den
    else:
        den = np.ones((h, w, 3))
        u = c.copy()
    pos = z > 0.0
    r = np.where(pos, 1.0 / np.where(pos, z, 1.0), 0.0)
    one = np.float64(1.0)
    with np.errstate(divide="ignore"):
        rn = one / (np.float64(sigma_normal) * np.float64(sigma_normal))
        rz = one / (np.float64(sigma_depth) * np.float64(sigma_depth))
    colour = sigma_colour > 0.0
    for i in range(iterations):
        s = 1 << i
        if colour:
            sc = np.float64(sigma_colour) / np.float64(s)
            rc = one / (sc * sc)
        acc = np.zeros((h, w, 3))
        ws = np.zeros((h, w))
        for dy in range(-2, 3):
            y0, y1 = max(0, -s * dy), min(h, h - s * dy)
            if y0 >= y1:
                continue
            for dx in range(-2, 3):
                x0, x1 = max(0, -s * dx), min(w, w - s * dx)
                if x0 >= x1:
                    continue
                P = (slice(y0, y1), slice(x0, x1))
                Q = (slice(y0 + s * dy, y1 + s * dy), slice(x0 + s * dx, x1 + s * dx))
                hk = K[abs(dx)] * K[abs(dy)]
                xn = _sq3(n[P] - n[Q]) * rn
                t = (z[P] - z[Q]) * r[P]
                xz = (t * t) * rz
                wt = (hk * _f(xn)) * _f(xz)
                if colour:
                    xc = _sq3(u[P] - u[Q]) * rc
                    wt = wt * _f(xc)
                acc[P] = acc[P] + wt[..., None] * u[Q]
                ws[P] = ws[P] + wt
        u = acc / ws[..., None]
    return (u * den).reshape(w * h, 3)


def rms(a, b):
    """The RMS of the linear difference of two frames."""
    return float(np.sqrt(np.mean((np.asarray(a) - np.asarray(b)) ** 2)))


@functools.lru_cache(maxsize=None)
def frame(name):
    """(w, h, noisy frame, planes) of a named aovref case: the oracle's depth-8 frame at the case's size, sample
    count and aovref.FRAME_SEED, and the reference planes of the same samples; computed once, never written to."""
    _, _, w, h, spp, osc, planes = aovref.case(name)
    img = osc.render(w, h, spp, 8, aovref.FRAME_SEED)
    img.setflags(write=False)
    return w, h, img, planes


@functools.lru_cache(maxsize=None)
def random_planes(w=40, h=24, seed=20):
    """Seeded planes that put every branch of the filter to work: a colour with outliers, albedo channels at, below
    and above 1e-3, pixels of zero coverage (n = 0, z = 0), normals of two orientations and depths on two levels
    (so the guide weights are neither all 0 nor all 1)."""
    g = np.random.default_rng(seed)
    npix = w * h
    rgb = g.random((npix, 3)) * 2.0
    rgb[g.random(npix) < 0.05] *= 40.0
    albedo = g.random((npix, 3))
    pick = g.random((npix, 3))
    albedo[pick < 0.10] = 1e-3
    albedo[(pick >= 0.10) & (pick < 0.20)] = 5e-4
    albedo[(pick >= 0.20) & (pick < 0.25)] = 0.0
    albedo[(pick >= 0.25) & (pick < 0.30)] = 1e-3 + 1e-9
    base = np.where(g.random((npix, 1)) < 0.5, [[0.0, 0.0, -1.0]], [[0.6, 0.0, -0.8]])
    normal = base + (g.random((npix, 3)) - 0.5) * 0.2
    level = np.where(g.random(npix) < 0.5, 4.0, 9.0)
    z = level * (1.0 + (g.random(npix) - 0.5) * 0.05)
    depth = np.stack([z, np.ones(npix), z], axis=1)
    empty = g.random(npix) < 0.15
    normal[empty] = 0.0
    depth[empty] = 0.0
    out = (rgb, albedo, normal, depth)
    for a in out:
        a.setflags(write=False)
    return out
