"""denoise_history_ref.py — the history-adaptive a-trous filter of
rt_denoise_history_device, in numpy.

TEST INFRASTRUCTURE ONLY (a helper, not a test; tests/test_denoise_history_ref.py
pins it to a second, scalar restatement so it cannot drift).

The contract of DESIGN.md §4i, vectorised over the frame the way denoise_ref.py
restates §4g: every arithmetic step is one float32 ufunc call (one IEEE binary32
operation, no fused multiply-add), max is np.fmax, `/` and sqrt are correctly
rounded, denormals are kept, the 25 taps are accumulated dy outer, dx inner.
The input is a history record (c.rgb linear, n samples) per pixel as
rt_temporal_device writes it; a pixel with n samples is filtered in the first
max(0, iterations - floor(log2 n)) passes only, its colour tolerance tightens
with n, and a tap counts by its samples.
"""
from __future__ import annotations

import numpy as np

from denoise_ref import F, H3, luminance, unorm8


def pass_counts(hist, hits, iterations=4):
    """(live bool [H, W], k int [H, W]): the pixels the filter touches at all and
    the number of passes each is filtered in (0 where not live)."""
    hist = np.asarray(hist, dtype=F)
    H, W = hist.shape[:2]
    tri = np.asarray(hits).reshape(H, W)["tri"]
    n = np.ascontiguousarray(hist[..., 3])
    with np.errstate(invalid="ignore"):
        live = (tri >= 0) & (n >= F(1.0))                      # a NaN n fails
    e = ((n.view(np.uint32) >> np.uint32(23)) & np.uint32(0xFF)).astype(np.int64) - 127   # floor(log2 n) where live
    return live, np.where(live, np.maximum(0, iterations - e), 0)


def denoise_history_linear(hist, hits, iterations=4, normal_power_log2=7, sigma_depth=0.005, sigma_color=0.5,
                           changed=None):
    """The filter's passes on c = hist.rgb: the linear colour after the last
    pass, float32 [H, W, 3].  `changed`, a list, receives per pass the bool
    [H, W] mask of the pixels whose colour bits the pass changed."""
    hist = np.ascontiguousarray(hist, dtype=F)
    H, W = hist.shape[:2]
    hits = np.asarray(hits).reshape(H, W)
    tri = hits["tri"]
    t = hits["t"].astype(F)
    n = hits["normal"].astype(F)
    pos = hits["pos"].astype(F)
    ns = np.ascontiguousarray(hist[..., 3])
    live, k = pass_counts(hist, hits, iterations)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    c = np.ascontiguousarray(hist[..., :3])
    with np.errstate(all="ignore"):
        isc = F(1.0) / F(sigma_color)
        kz = F(1.0) / (F(sigma_depth) * t)
        for i in range(iterations):
            s = 1 << i
            isc_p = (isc * F(s)) * ns
            active = live & (i < k)
            lum = luminance(c)
            acc = np.zeros((H, W, 3), F)
            wsum = np.zeros((H, W), F)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    qy, qx = ys + dy * s, xs + dx * s
                    inside = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
                    qy, qx = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
                    take = inside & live[qy, qx] & active
                    nq = n[qy, qx]
                    nd = np.fmax(F(0.0), (n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2])
                    for _ in range(normal_power_log2):
                        nd = nd * nd
                    e = pos[qy, qx] - pos
                    d = np.abs((n[..., 0] * e[..., 0] + n[..., 1] * e[..., 1]) + n[..., 2] * e[..., 2])
                    x = d * kz
                    y = np.abs(lum - lum[qy, qx]) * isc_p
                    w = (((H3[abs(dx)] * H3[abs(dy)]) * nd) * ns[qy, qx]) / ((F(1.0) + x * x) * (F(1.0) + y * y))
                    acc = np.where(take[..., None], acc + w[..., None] * c[qy, qx], acc)
                    wsum = np.where(take, wsum + w, wsum)
            good = active & (wsum > F(0.0))
            out = np.where(good[..., None], acc / wsum[..., None], c).astype(F)
            if changed is not None:
                changed.append((out.view(np.uint32) != c.view(np.uint32)).any(-1))
            c = out
    return c


def denoise_history(hist, hits, iterations=4, normal_power_log2=7, sigma_depth=0.005, sigma_color=0.5):
    """(radiance float32 [H, W, 3], rgba uint8 [H, W, 4]) of the filtered history."""
    c = denoise_history_linear(hist, hits, iterations, normal_power_log2, sigma_depth, sigma_color)
    with np.errstate(invalid="ignore"):
        rad = np.sqrt(c).astype(F)
    return rad, unorm8(rad)
