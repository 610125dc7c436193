"""albedo_ref.py — rt_albedo_device's records and rt_denoise_albedo_device's filter, in numpy.

TEST INFRASTRUCTURE ONLY (a helper, not a test; tests/test_albedo_ref.py pins it
to denoise_ref and to a scalar restatement so it cannot drift).

The contract of DESIGN.md §4p: the first-hit albedo buffer, and §4g's passes run
on the illumination i = (g * g) / d instead of the colour, multiplied back by d
after the last pass.  As in denoise_ref, every arithmetic step is one float32
ufunc call (one IEEE binary32 operation), so the GPU's bits equal this module's.
"""
from __future__ import annotations

import numpy as np

import denoise_ref as D

F = np.float32
LO, HI = F(2.0 ** -10), F(2.0 ** 10)      # an albedo channel outside [LO, HI] is filtered as colour (d = 1)


def divisor(a) -> np.ndarray:
    """Per channel d = a where 2^-10 <= a <= 2^10, else 1 (NaN, negative, zero, denormal, infinite: 1)."""
    a = np.asarray(a, F)
    with np.errstate(invalid="ignore"):
        return np.where((a >= LO) & (a <= HI), a, F(1.0)).astype(F)


def albedo(hits, materials) -> np.ndarray:
    """rt_albedo_device's records, float32 [H, W, 4]: (d.rgb, type) of a pixel
    whose tri names one of the n_flat `materials` records (albedo.rgb, type),
    (1, 1, 1, -1) of every other pixel."""
    hits = np.asarray(hits)
    mats = np.asarray(materials, F).reshape(-1, 4)
    tri = hits["tri"].astype(np.int64)
    ok = (tri >= 0) & (tri < len(mats))
    out = np.empty(hits.shape + (4,), F)
    out[..., :3] = F(1.0)
    out[..., 3] = F(-1.0)
    if len(mats):
        m = mats[np.where(ok, tri, 0)]
        out[..., :3] = np.where(ok[..., None], divisor(m[..., :3]), out[..., :3])
        # the type's bits as they are (a NaN type keeps its payload)
        out[..., 3].view(np.uint32)[...] = np.where(ok, m[..., 3].view(np.uint32), out[..., 3].view(np.uint32))
    return out


def filter_linear(c, hits, iterations=4, normal_power_log2=7, sigma_depth=0.005, sigma_color=0.5) -> np.ndarray:
    """§4g's passes on a given linear colour c, float32 [H, W, 3]: what
    denoise_ref.denoise_linear does behind its c = g * g."""
    c = np.ascontiguousarray(c, dtype=F)
    H, W = c.shape[:2]
    hits = np.asarray(hits).reshape(H, W)
    tri = hits["tri"]
    t = hits["t"].astype(F)
    n = hits["normal"].astype(F)
    pos = hits["pos"].astype(F)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    ok_p = tri >= 0
    with np.errstate(all="ignore"):
        isc = F(1.0) / F(sigma_color)
        kz = F(1.0) / (F(sigma_depth) * t)
        for i in range(iterations):
            s = 1 << i
            isc_i = isc * F(s)
            lum = D.luminance(c)
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
                    w = ((D.H3[abs(dx)] * D.H3[abs(dy)]) * nd) / ((F(1.0) + x * x) * (F(1.0) + y * y))
                    acc = np.where(take[..., None], acc + w[..., None] * c[qy, qx], acc)
                    wsum = np.where(take, wsum + w, wsum)
            good = ok_p & (wsum > F(0.0))
            c = np.where(good[..., None], acc / wsum[..., None], c).astype(F)
    return c


def denoise_albedo(radiance, hits, alb, iterations=4, normal_power_log2=7, sigma_depth=0.005, sigma_color=0.5):
    """(radiance float32 [H, W, 3], rgba uint8 [H, W, 4]) of rt_denoise_albedo_device:
    alb is the albedo buffer, [H, W, 3] or [H, W, 4]; its first three words are
    the divisors as they stand (rt_albedo_device has applied divisor())."""
    g = np.ascontiguousarray(radiance, dtype=F)
    d = np.ascontiguousarray(np.asarray(alb, F)[..., :3])
    with np.errstate(all="ignore"):
        c = g * g
        i = (c / d).astype(F)
        out = filter_linear(i, hits, iterations, normal_power_log2, sigma_depth, sigma_color) * d
        rad = np.sqrt(out).astype(F)
    return rad, D.unorm8(rad)
