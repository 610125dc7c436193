"""temporal_ref.py — the temporal accumulation of rt_temporal_device, in numpy.

TEST INFRASTRUCTURE ONLY (a helper, not a test; tests/test_temporal_ref.py pins
it to a second, scalar restatement so it cannot drift).

The contract of DESIGN.md §4h, vectorised over the frame: every arithmetic step
is one float32 ufunc call (one IEEE binary32 operation, no fused multiply-add),
min is np.fmin (a NaN operand is dropped), `/` and sqrt are correctly rounded,
denormals are kept.  The four taps are accumulated j outer, i inner, as the
kernel does, so the GPU's history, radiance bits and RGBA8 equal this module's.
"""
from __future__ import annotations

import numpy as np

from denoise_ref import HIT_DTYPE, unorm8  # noqa: F401  (HIT_DTYPE: for callers)

F = np.float32

DEFAULTS = dict(max_history=32, plane_tol=0.005, normal_min=0.9)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(p, q):
    return np.stack([p[..., 1] * q[..., 2] - p[..., 2] * q[..., 1],
                     p[..., 2] * q[..., 0] - p[..., 0] * q[..., 2],
                     p[..., 0] * q[..., 1] - p[..., 1] * q[..., 0]], -1).astype(F)


def camera_basis(camera_ubo: bytes) -> np.ndarray:
    """rt_temporal_camera_basis: float32[13] = origin, N, A, B, det of the 80 UBO bytes."""
    cam = np.frombuffer(bytes(camera_ubo), F)[:16].reshape(4, 4)[:, :3]
    org, llc, hor, ver = cam[0], cam[1], cam[2], cam[3]
    a = (llc - org).astype(F)
    n = _cross(hor, ver)
    return np.concatenate([org, n, _cross(ver, a), _cross(a, hor), [_dot(a, n)]]).astype(F)


def project(basis: np.ndarray, pos: np.ndarray):
    """project(C, P): (u, v, front) of world positions pos[..., 3]."""
    b = np.asarray(basis, F)
    with np.errstate(all="ignore"):
        w = (pos - b[0:3]).astype(F)
        dn = _dot(w, b[3:6])
        u = _dot(w, b[6:9]) / dn
        v = _dot(w, b[9:12]) / dn
        front = dn * b[12] > F(0.0)
    return u, v, front


def temporal(radiance, hits, cam=None, prev_cam=None, hist_prev=None, hits_prev=None,
             max_history=32, plane_tol=0.005, normal_min=0.9):
    """One frame of the accumulation: radiance float32 [H, W, 3] and HIT_DTYPE
    records [H, W] of the new frame, its 80 camera bytes; the previous frame's
    camera bytes, history float32 [H, W, 4] and hit records, all None for a
    first frame.  Returns (history float32 [H, W, 4], radiance float32
    [H, W, 3], rgba uint8 [H, W, 4], reused bool [H, W])."""
    g = np.ascontiguousarray(radiance, dtype=F)
    H, W = g.shape[:2]
    hits = np.asarray(hits).reshape(H, W)
    tri, t = hits["tri"], hits["t"].astype(F)
    nrm, pos = hits["normal"].astype(F), hits["pos"].astype(F)
    c = g * g
    out_c = c.copy()
    out_n = np.where(tri >= 0, F(1.0), F(0.0)).astype(F)
    reused = np.zeros((H, W), bool)
    given = [x is not None for x in (prev_cam, hist_prev, hits_prev)]
    assert all(given) or not any(given)
    if all(given):
        hp = np.ascontiguousarray(hist_prev, dtype=F).reshape(H, W, 4)
        hq = np.asarray(hits_prev).reshape(H, W)
        tri_q, nrm_q, pos_q = hq["tri"], hq["normal"].astype(F), hq["pos"].astype(F)
        ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        with np.errstate(all="ignore"):
            uc, vc, fc = project(camera_basis(cam), pos)
            up, vp, fp = project(camera_basis(prev_cam), pos)
            fW, fH = F(W), F(H)
            fx = xs.astype(F) + (up - uc) * fW
            fy = ys.astype(F) + (vc - vp) * fH
            ok = (tri >= 0) & fc & fp & (fx > F(-1.0)) & (fx < fW) & (fy > F(-1.0)) & (fy < fH)
            fx, fy = np.where(ok, fx, F(0.0)), np.where(ok, fy, F(0.0))
            x0, y0 = np.floor(fx), np.floor(fy)
            ax, ay = fx - x0, fy - y0
            tol = F(plane_tol) * t
            ix, iy = x0.astype(np.int64), y0.astype(np.int64)
            acc = np.zeros((H, W, 3), F)
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
                    take &= _dot(nrm, nrm_q[qy, qx]) >= F(normal_min)
                    take &= np.abs(_dot(nrm, (pos_q[qy, qx] - pos).astype(F))) <= tol
                    acc = np.where(take[..., None], acc + wt[..., None] * hp[qy, qx, :3], acc)
                    ws = np.where(take, ws + wt, ws)
                    nm = np.where(take, np.fmin(nm, hn), nm)
            reused = ok & (ws > F(0.0))
            ch = acc / ws[..., None]
            nn = np.fmin(nm + F(1.0), F(max_history))
            inv = F(1.0) / nn
            blend = ch + (c - ch) * inv[..., None]
            out_c = np.where(reused[..., None], blend, c).astype(F)
            out_n = np.where(reused, nn, out_n).astype(F)
    hist = np.concatenate([out_c, out_n[..., None]], -1).astype(F)
    with np.errstate(invalid="ignore"):
        rad = np.sqrt(out_c).astype(F)
    return hist, rad, unorm8(rad), reused
