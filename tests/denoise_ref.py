"""denoise_ref.py — the edge-avoiding a-trous filter of rt_denoise_device, in numpy.

TEST INFRASTRUCTURE ONLY (a helper, not a test; tests/test_denoise_ref.py pins it
to a second, scalar restatement so it cannot drift).

The contract of DESIGN.md §4g, vectorised over the frame: every arithmetic step
is one float32 ufunc call (one IEEE binary32 operation, no fused multiply-add),
max is np.fmax (a NaN operand is dropped), `/` and sqrt are correctly rounded,
denormals are kept.  The 25 taps are accumulated dy outer, dx inner, as the
kernels do, so the GPU's radiance bits and RGBA8 equal this module's.
"""
from __future__ import annotations

import numpy as np

F = np.float32
H3 = (F(3.0 / 8.0), F(1.0 / 4.0), F(1.0 / 16.0))     # the B3 spline, by |offset|
LUM = (F(0.2126), F(0.7152), F(0.0722))

HIT_DTYPE = np.dtype([("t", "<f4"), ("tri", "<i4"), ("normal", "<f4", (3,)), ("pos", "<f4", (3,))])

DEFAULTS = dict(iterations=4, normal_power_log2=7, sigma_depth=0.005, sigma_color=0.5)


def luminance(c: np.ndarray) -> np.ndarray:
    return (LUM[0] * c[..., 0] + LUM[1] * c[..., 1]) + LUM[2] * c[..., 2]


def unorm8(rad: np.ndarray) -> np.ndarray:
    """The render's RGBA8 store: clamp, c * 255 to nearest even, alpha 255."""
    with np.errstate(invalid="ignore"):
        q = np.where(rad > F(0.0), np.where(rad < F(1.0), np.rint(rad * F(255.0)), F(255.0)), F(0.0)).astype(np.uint8)
    return np.concatenate([q, np.full(q.shape[:-1] + (1,), 255, np.uint8)], -1)


def denoise_linear(radiance, hits, iterations=4, normal_power_log2=7, sigma_depth=0.005, sigma_color=0.5):
    """The filter's passes on c = g * g: returns the linear colour after the
    last pass, float32 [H, W, 3]."""
    g = np.ascontiguousarray(radiance, dtype=F)
    H, W = g.shape[:2]
    hits = np.asarray(hits).reshape(H, W)
    tri = hits["tri"]
    t = hits["t"].astype(F)
    n = hits["normal"].astype(F)
    pos = hits["pos"].astype(F)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    ok_p = tri >= 0
    c = g * g
    with np.errstate(all="ignore"):
        isc = F(1.0) / F(sigma_color)
        kz = F(1.0) / (F(sigma_depth) * t)
        for i in range(iterations):
            s = 1 << i
            isc_i = isc * F(s)
            lum = luminance(c)
            acc = np.zeros((H, W, 3), F)
            wsum = np.zeros((H, W), F)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    qy, qx = ys + dy * s, xs + dx * s
                    inside = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
                    qy, qx = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
                    take = inside & (tri[qy, qx] >= 0) & ok_p
                    nq = n[qy, qx]
                    nd = np.fmax(F(0.0), (n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2])
                    for _ in range(normal_power_log2):
                        nd = nd * nd
                    e = pos[qy, qx] - pos
                    d = np.abs((n[..., 0] * e[..., 0] + n[..., 1] * e[..., 1]) + n[..., 2] * e[..., 2])
                    x = d * kz
                    y = np.abs(lum - lum[qy, qx]) * isc_i
                    w = ((H3[abs(dx)] * H3[abs(dy)]) * nd) / ((F(1.0) + x * x) * (F(1.0) + y * y))
                    acc = np.where(take[..., None], acc + w[..., None] * c[qy, qx], acc)
                    wsum = np.where(take, wsum + w, wsum)
            good = ok_p & (wsum > F(0.0))
            c = np.where(good[..., None], acc / wsum[..., None], c).astype(F)
    return c


def denoise(radiance, hits, iterations=4, normal_power_log2=7, sigma_depth=0.005, sigma_color=0.5):
    """(radiance float32 [H, W, 3], rgba uint8 [H, W, 4]) of the filtered frame."""
    c = denoise_linear(radiance, hits, iterations, normal_power_log2, sigma_depth, sigma_color)
    with np.errstate(invalid="ignore"):
        rad = np.sqrt(c).astype(F)
    return rad, unorm8(rad)
