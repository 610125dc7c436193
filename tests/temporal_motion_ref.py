"""temporal_motion_ref.py — rt_temporal_motion_device in numpy: the temporal
accumulation reprojected per triangle across a geometry update.

TEST INFRASTRUCTURE ONLY (a helper, not a test; tests/test_temporal_motion_ref.py
pins it to a second, scalar restatement so it cannot drift).

The contract of DESIGN.md §4m, vectorised over the frame.  Everything of §4h
(temporal_ref.py) holds with P' and n' in the place of pos and normal on the
previous-frame side: a pixel's hit point is expressed in the barycentric
coordinates of its triangle as the current vertex records hold it and evaluated
on the same triangle of the previous records.  The edges are float32
differences; the barycentric block is binary64 on the exactly widened floats,
one operation per ufunc call in the order §4m writes them; everything else is
§4h's float32.  With moments (§4j) the same taps and weights carry (m1, m2).
"""
from __future__ import annotations

import numpy as np

import temporal_ref as T
from denoise_ref import luminance, unorm8

F = np.float32
D = np.float64

DEFAULTS = T.DEFAULTS


def vertex_records(verts) -> np.ndarray:
    """float32 [n, 3, 3]: the xyz of the three float4 of every 48-B vertex record."""
    return np.ascontiguousarray(verts, dtype=F).reshape(-1, 3, 4)[:, :, :3]


def _dot64(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross64(p, q):
    return np.stack([p[..., 1] * q[..., 2] - p[..., 2] * q[..., 1],
                     p[..., 2] * q[..., 0] - p[..., 0] * q[..., 2],
                     p[..., 0] * q[..., 1] - p[..., 1] * q[..., 0]], -1)


def previous_points(hits, verts_cur, verts_prev, n_tris=None):
    """(P' float32 [H, W, 3], n' float32 [H, W, 3], valid bool [H, W], moved bool
    [H, W]) of hit records [H, W]: valid is False where §4m gives a pixel with
    a hit no history (tri >= n_tris, or a P' or n' that is not finite)."""
    vc, vp = vertex_records(verts_cur), vertex_records(verts_prev)
    n = len(vc) if n_tris is None else int(n_tris)
    assert len(vp) >= n and len(vc) >= n
    tri = np.asarray(hits["tri"]).astype(np.int64)
    pos, nrm = hits["pos"].astype(F), hits["normal"].astype(F)
    in_range = (tri >= 0) & (tri < n)
    k = np.where(in_range, tri, 0)
    if n == 0:                                      # (never through the library: n_tris 0 is refused)
        return pos, nrm, in_range, np.zeros(tri.shape, bool)
    V, Vp = vc[k], vp[k]                            # [H, W, 3 vertices, 3]
    moved = (V.view(np.uint32) != Vp.view(np.uint32)).any((-1, -2)) & in_range
    with np.errstate(all="ignore"):
        e1, e2 = (V[..., 1, :] - V[..., 0, :]).astype(F), (V[..., 2, :] - V[..., 0, :]).astype(F)
        f1, f2 = (Vp[..., 1, :] - Vp[..., 0, :]).astype(F), (Vp[..., 2, :] - Vp[..., 0, :]).astype(F)
        e1, e2, f1, f2 = (x.astype(D) for x in (e1, e2, f1, f2))
        v0, u0 = V[..., 0, :].astype(D), Vp[..., 0, :].astype(D)
        w = pos.astype(D) - v0
        d11, d12, d22 = _dot64(e1, e1), _dot64(e1, e2), _dot64(e2, e2)
        w1, w2 = _dot64(w, e1), _dot64(w, e2)
        den = d11 * d22 - d12 * d12
        b1 = (d22 * w1 - d12 * w2) / den
        b2 = (d11 * w2 - d12 * w1) / den
        P = ((u0 + b1[..., None] * f1) + b2[..., None] * f2).astype(F)
        m, mp = _cross64(e1, e2), _cross64(f1, f2)
        s = np.where(_dot64(m, nrm.astype(D)) < 0.0, D(-1.0), D(1.0))
        N = ((mp / np.sqrt(_dot64(mp, mp))[..., None]) * s[..., None]).astype(F)
    finite = np.isfinite(P).all(-1) & np.isfinite(N).all(-1)
    P = np.where(moved[..., None], P, pos).astype(F)
    N = np.where(moved[..., None], N, nrm).astype(F)
    valid = in_range & (~moved | finite)
    return P, N, valid, moved


def temporal_motion(radiance, hits, cam, prev_cam, hist_prev, hits_prev, verts_cur, verts_prev, n_tris=None,
                    mom_prev=None, max_history=32, plane_tol=0.005, normal_min=0.9, taps=None):
    """One frame across a geometry update: temporal_ref.temporal's arguments
    (a previous frame is required), the current and the previous vertex
    records (float32, 12 per flattened triangle) and, with moments, the
    previous moments float32 [H, W, 2].  Returns (history, radiance, rgba,
    reused, moments or None).  taps: a list that receives the four taps'
    (taken mask, row, column) in the order they are accumulated."""
    g = np.ascontiguousarray(radiance, dtype=F)
    H, W = g.shape[:2]
    hits = np.asarray(hits).reshape(H, W)
    tri, t = hits["tri"], hits["t"].astype(F)
    pos = hits["pos"].astype(F)
    c = g * g
    lum = luminance(c)
    m = np.stack([lum, lum * lum], -1).astype(F)
    moments = mom_prev is not None
    hp = np.ascontiguousarray(hist_prev, dtype=F).reshape(H, W, 4)
    mp = np.ascontiguousarray(mom_prev, dtype=F).reshape(H, W, 2) if moments else np.zeros((H, W, 2), F)
    hq = np.asarray(hits_prev).reshape(H, W)
    tri_q, nrm_q, pos_q = hq["tri"], hq["normal"].astype(F), hq["pos"].astype(F)
    Pp, Np, valid, _ = previous_points(hits, verts_cur, verts_prev, n_tris)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    with np.errstate(all="ignore"):
        uc, vc, fc = T.project(T.camera_basis(cam), pos)
        up, vp, fp = T.project(T.camera_basis(prev_cam), Pp)
        fW, fH = F(W), F(H)
        fx = xs.astype(F) + (up - uc) * fW
        fy = ys.astype(F) + (vc - vp) * fH
        ok = (tri >= 0) & valid & fc & fp & (fx > F(-1.0)) & (fx < fW) & (fy > F(-1.0)) & (fy < fH)
        fx, fy = np.where(ok, fx, F(0.0)), np.where(ok, fy, F(0.0))
        x0, y0 = np.floor(fx), np.floor(fy)
        ax, ay = fx - x0, fy - y0
        tol = F(plane_tol) * t
        ix, iy = x0.astype(np.int64), y0.astype(np.int64)
        acc = np.zeros((H, W, 3), F)
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
                take &= T._dot(Np, nrm_q[qy, qx]) >= F(normal_min)
                take &= np.abs(T._dot(Np, (pos_q[qy, qx] - Pp).astype(F))) <= tol
                if taps is not None:
                    taps.append((take, qy, qx))
                acc = np.where(take[..., None], acc + wt[..., None] * hp[qy, qx, :3], acc)
                msum = np.where(take[..., None], msum + wt[..., None] * mp[qy, qx], msum)
                ws = np.where(take, ws + wt, ws)
                nm = np.where(take, np.fmin(nm, hn), nm)
        reused = ok & (ws > F(0.0))
        ch = acc / ws[..., None]
        nn = np.fmin(nm + F(1.0), F(max_history))
        inv = F(1.0) / nn
        blend = ch + (c - ch) * inv[..., None]
        out_c = np.where(reused[..., None], blend, c).astype(F)
        out_n = np.where(reused, nn, np.where(tri >= 0, F(1.0), F(0.0))).astype(F)
        mh = msum / ws[..., None]
        mom = np.where(reused[..., None], mh + (m - mh) * inv[..., None], m).astype(F)
    hist = np.concatenate([out_c, out_n[..., None]], -1).astype(F)
    with np.errstate(invalid="ignore"):
        rad = np.sqrt(out_c).astype(F)
    return hist, rad, unorm8(rad), reused, (mom if moments else None)
