"""variance_ref.py — the temporal accumulation with luminance moments
(rt_temporal_moments_device) and the variance-guided a-trous filter
(rt_denoise_variance_device), in numpy.

TEST INFRASTRUCTURE ONLY (a helper, not a test; tests/test_variance_ref.py pins
it to a second, scalar restatement so it cannot drift).

The contract of DESIGN.md §4j, vectorised over the frame the way temporal_ref.py
and denoise_history_ref.py restate §4h and §4i: every arithmetic step is one
float32 ufunc call (one IEEE binary32 operation, no fused multiply-add), max and
min are np.fmax / np.fmin (a NaN operand is dropped), `/` and sqrt are correctly
rounded, denormals are kept; taps are accumulated dy outer, dx inner.
"""
from __future__ import annotations

import numpy as np

import temporal_ref as T
from denoise_history_ref import pass_counts
from denoise_ref import F, H3, luminance, unorm8

B2 = (F(0.5), F(0.25))                  # the 3x3 window's binomial, by |offset|

DEFAULTS = dict(iterations=4, normal_power_log2=7, sigma_depth=0.005, sigma_lum=1.0, min_history=4)


# ---- rt_temporal_moments_device -------------------------------------------------

def temporal_moments(radiance, hits, cam=None, prev_cam=None, hist_prev=None, hits_prev=None, mom_prev=None,
                     max_history=32, plane_tol=0.005, normal_min=0.9):
    """temporal_ref.temporal with a moments buffer float32 [H, W, 2] beside the
    history (mom_prev None exactly when the other previous-frame inputs are).
    Returns (history, radiance, rgba, reused, moments): the first four are
    temporal_ref.temporal's own return values."""
    hist, rad, rgba, reused = T.temporal(radiance, hits, cam, prev_cam, hist_prev, hits_prev,
                                         max_history, plane_tol, normal_min)
    g = np.ascontiguousarray(radiance, dtype=F)
    H, W = g.shape[:2]
    hits = np.asarray(hits).reshape(H, W)
    tri, t = hits["tri"], hits["t"].astype(F)
    nrm, pos = hits["normal"].astype(F), hits["pos"].astype(F)
    c = g * g
    lum = luminance(c)
    m = np.stack([lum, lum * lum], -1).astype(F)
    given = [x is not None for x in (prev_cam, hist_prev, hits_prev, mom_prev)]
    assert all(given) or not any(given)
    if not all(given):
        return hist, rad, rgba, reused, m
    hp = np.ascontiguousarray(hist_prev, dtype=F).reshape(H, W, 4)
    mp = np.ascontiguousarray(mom_prev, dtype=F).reshape(H, W, 2)
    hq = np.asarray(hits_prev).reshape(H, W)
    tri_q, nrm_q, pos_q = hq["tri"], hq["normal"].astype(F), hq["pos"].astype(F)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    with np.errstate(all="ignore"):                     # §4h's taps, line for line
        uc, vc, fc = T.project(T.camera_basis(cam), pos)
        up, vp, fp = T.project(T.camera_basis(prev_cam), pos)
        fW, fH = F(W), F(H)
        fx = xs.astype(F) + (up - uc) * fW
        fy = ys.astype(F) + (vc - vp) * fH
        ok = (tri >= 0) & fc & fp & (fx > F(-1.0)) & (fx < fW) & (fy > F(-1.0)) & (fy < fH)
        fx, fy = np.where(ok, fx, F(0.0)), np.where(ok, fy, F(0.0))
        x0, y0 = np.floor(fx), np.floor(fy)
        ax, ay = fx - x0, fy - y0
        tol = F(plane_tol) * t
        ix, iy = x0.astype(np.int64), y0.astype(np.int64)
        msum = np.zeros((H, W, 2), F)
        ws = np.zeros((H, W), F)
        nm = np.full((H, W), np.inf, F)
        for j in (0, 1):
            for i in (0, 1):
                qx, qy = ix + i, iy + j
                inside = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
                qx, qy = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
                wt = (ax if i else F(1.0) - ax) * (ay if j else F(1.0) - ay)
                hn = hp[qy, qx, 3]
                take = ok & inside & (tri_q[qy, qx] >= 0) & (hn > F(0.0)) & (wt > F(0.0))
                take &= T._dot(nrm, nrm_q[qy, qx]) >= F(normal_min)
                take &= np.abs(T._dot(nrm, (pos_q[qy, qx] - pos).astype(F))) <= tol
                msum = np.where(take[..., None], msum + wt[..., None] * mp[qy, qx], msum)
                ws = np.where(take, ws + wt, ws)
                nm = np.where(take, np.fmin(nm, hn), nm)
        took = ok & (ws > F(0.0))
        assert np.array_equal(took, reused)
        mh = msum / ws[..., None]
        inv = F(1.0) / np.fmin(nm + F(1.0), F(max_history))
        blend = mh + (m - mh) * inv[..., None]
        mom = np.where(took[..., None], blend, m).astype(F)
    return hist, rad, rgba, reused, mom


# ---- rt_denoise_variance_device ---------------------------------------------------

def _guides(hits, H, W):
    hits = np.asarray(hits).reshape(H, W)
    return hits["tri"], hits["t"].astype(F), hits["normal"].astype(F), hits["pos"].astype(F)


def _guide_terms(n, pos, kz, qy, qx, normal_power_log2):
    """(nd, x) of the tap at [qy, qx] for every centre pixel."""
    nq = n[qy, qx]
    nd = np.fmax(F(0.0), (n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2])
    for _ in range(normal_power_log2):
        nd = nd * nd
    e = pos[qy, qx] - pos
    d = np.abs((n[..., 0] * e[..., 0] + n[..., 1] * e[..., 1]) + n[..., 2] * e[..., 2])
    return nd, d * kz


def estimate(hist, mom, hits, normal_power_log2=7, sigma_depth=0.005, min_history=4, spatial=None):
    """The filter's first records: float32 [H, W, 4] = (c.rgb, v), v = -1 where
    the pixel is not live.  `spatial`, a list, receives the bool [H, W] mask of
    the pixels that took the 49-tap branch."""
    hist = np.ascontiguousarray(hist, dtype=F)
    mom = np.ascontiguousarray(mom, dtype=F)
    H, W = hist.shape[:2]
    tri, t, n, pos = _guides(hits, H, W)
    live, _ = pass_counts(hist, hits)
    c = np.ascontiguousarray(hist[..., :3])
    ns = np.ascontiguousarray(hist[..., 3])
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    with np.errstate(all="ignore"):
        m1, m2 = mom[..., 0], mom[..., 1]
        vt = np.fmax(F(0.0), m2 - m1 * m1) / np.fmax(ns - F(1.0), F(1.0))
        short = live & ~(ns >= F(min_history))
        kz = F(1.0) / (F(sigma_depth) * t)
        lum = luminance(c)
        s0 = np.zeros((H, W), F)
        s1 = np.zeros((H, W), F)
        s2 = np.zeros((H, W), F)
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                qy, qx = ys + dy, xs + dx
                inside = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
                qy, qx = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
                take = inside & live[qy, qx]
                nd, x = _guide_terms(n, pos, kz, qy, qx, normal_power_log2)
                w = nd / (F(1.0) + x * x)
                lq = lum[qy, qx]
                wl = w * lq
                s0 = np.where(take, s0 + w, s0)
                s1 = np.where(take, s1 + wl, s1)
                s2 = np.where(take, s2 + wl * lq, s2)
        mu = s1 / s0
        vs = np.fmax(F(0.0), s2 / s0 - mu * mu)
        v_short = np.where(s0 > F(0.0), np.fmax(vs, vt), vt)
        v = np.where(live, np.where(short, v_short, vt), F(-1.0)).astype(F)
    if spatial is not None:
        spatial.append(short)
    return np.concatenate([c, v[..., None]], -1).astype(F)


def variance_pass(rec, hist, hits, i, iterations=4, normal_power_log2=7, sigma_depth=0.005, sigma_lum=1.0):
    """Pass i (step 2^i) on records float32 [H, W, 4] = (c.rgb, v): the next records."""
    rec = np.ascontiguousarray(rec, dtype=F)
    H, W = rec.shape[:2]
    tri, t, n, pos = _guides(hits, H, W)
    ns = np.ascontiguousarray(np.asarray(hist, dtype=F)[..., 3])
    e = ((ns.view(np.uint32) >> np.uint32(23)) & np.uint32(0xFF)).astype(np.int64) - 127    # floor(log2 n)
    c, v = np.ascontiguousarray(rec[..., :3]), np.ascontiguousarray(rec[..., 3])
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    s = 1 << i
    with np.errstate(all="ignore"):
        active = ~(v < F(0.0)) & (e < iterations - i)       # i < k_p; a NaN v stays active
        tap_ok = v >= F(0.0)
        g = np.zeros((H, W), F)
        gw = np.zeros((H, W), F)
        for dy in range(-1, 2):
            for dx in range(-1, 2):
                qy, qx = ys + dy, xs + dx
                inside = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
                qy, qx = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
                take = inside & tap_ok[qy, qx]
                b = B2[abs(dx)] * B2[abs(dy)]
                g = np.where(take, g + b * v[qy, qx], g)
                gw = np.where(take, gw + b, gw)
        isl = F(1.0) / ((F(sigma_lum) * np.sqrt(g / gw)) + F(1e-6))
        kz = F(1.0) / (F(sigma_depth) * t)
        lum = luminance(c)
        acc = np.zeros((H, W, 3), F)
        wsum = np.zeros((H, W), F)
        vsum = np.zeros((H, W), F)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                qy, qx = ys + dy * s, xs + dx * s
                inside = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
                qy, qx = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
                take = inside & tap_ok[qy, qx]
                nd, x = _guide_terms(n, pos, kz, qy, qx, normal_power_log2)
                y = np.abs(lum - lum[qy, qx]) * isl
                w = ((H3[abs(dx)] * H3[abs(dy)]) * nd) / ((F(1.0) + x * x) * (F(1.0) + y * y))
                acc = np.where(take[..., None], acc + w[..., None] * c[qy, qx], acc)
                wsum = np.where(take, wsum + w, wsum)
                vsum = np.where(take, vsum + (w * w) * v[qy, qx], vsum)
        good = active & (wsum > F(0.0))
        out_c = np.where(good[..., None], acc / wsum[..., None], c)
        out_v = np.where(good, vsum / (wsum * wsum), v)
    return np.concatenate([out_c, out_v[..., None]], -1).astype(F)


def denoise_variance_records(hist, mom, hits, iterations=4, normal_power_log2=7, sigma_depth=0.005, sigma_lum=1.0,
                             min_history=4, changed=None, spatial=None):
    """The records (c.rgb, v) after the last pass.  `changed`, a list, receives
    per pass the bool [H, W] mask of the pixels whose colour bits it changed."""
    rec = estimate(hist, mom, hits, normal_power_log2, sigma_depth, min_history, spatial)
    for i in range(iterations):
        out = variance_pass(rec, hist, hits, i, iterations, normal_power_log2, sigma_depth, sigma_lum)
        if changed is not None:
            changed.append((out[..., :3].view(np.uint32) != rec[..., :3].view(np.uint32)).any(-1))
        rec = out
    return rec


def denoise_variance(hist, mom, hits, iterations=4, normal_power_log2=7, sigma_depth=0.005, sigma_lum=1.0,
                     min_history=4):
    """(radiance float32 [H, W, 3], rgba uint8 [H, W, 4]) of the filtered history."""
    rec = denoise_variance_records(hist, mom, hits, iterations, normal_power_log2, sigma_depth, sigma_lum, min_history)
    with np.errstate(invalid="ignore"):
        rad = np.sqrt(rec[..., :3]).astype(F)
    return rad, unorm8(rad)
