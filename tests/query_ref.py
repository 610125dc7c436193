"""query_ref.py — the reference's closest hit of a batch of rays, in numpy.

TEST INFRASTRUCTURE ONLY (a helper, not a test; tests/test_query_ref.py pins it
to oracle/rt_oracle.c so it cannot drift).

One segment's walk of shaders/compute_dynamic_ray.comp:181-213 for every ray of
a batch at once, over the 48-byte reference nodes in the reference's own DFS
order (int stack[64]: push right, push left), in float32 throughout and in the
operation order of hit_aabb / hit_triangle (:88-129), with closest_t starting
at each ray's own t_max: the semantics include/rtamd.h states for rt_query_rays.
Written in the manner of oracle/shader_np.py (one IEEE operation per ufunc call,
no fused multiply-add, min / max = fmin / fmax).
"""
from __future__ import annotations

import numpy as np

F = np.float32
T_MIN = F(0.001)                 # :42
T_MAX = F(10000.0)               # :43

RAY_DTYPE = np.dtype([("origin", "<f4", (3,)), ("t_max", "<f4"), ("dir", "<f4", (3,)), ("reserved", "<u4")])
HIT_DTYPE = np.dtype([("t", "<f4"), ("tri", "<i4"), ("normal", "<f4", (3,)), ("pos", "<f4", (3,))])


def _dot(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def _cross(ax, ay, az, bx, by, bz):
    return ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx


def pcg(v):                                                    # :52-56
    v = v.astype(np.uint32)
    s = v * np.uint32(747796405) + np.uint32(2891336453)
    w = ((s >> ((s >> np.uint32(28)) + np.uint32(4))) ^ s) * np.uint32(277803737)
    return (w >> np.uint32(22)) ^ w


def make_rays(origin, direction, t_max=T_MAX) -> np.ndarray:
    """RAY_DTYPE records from (n, 3) origins and directions and a t_max (scalar or (n,))."""
    o = np.asarray(origin, F).reshape(-1, 3)
    r = np.zeros(len(o), RAY_DTYPE)
    r["origin"] = o
    r["dir"] = np.asarray(direction, F).reshape(-1, 3)
    r["t_max"] = np.asarray(t_max, F)
    return r


def primary_rays(camera_ubo: bytes, width: int, height: int, tile=None) -> np.ndarray:
    """Every pixel's primary ray (:164-173: seed, jitter, normalize) of the
    tile (x0, y0, tw, th), row-major, as RAY_DTYPE records with t_max = T_MAX."""
    x0, y0, tw, th = tile if tile is not None else (0, 0, width, height)
    cam = np.frombuffer(bytes(camera_ubo), np.float32)[:16].reshape(4, 4)[:, :3]
    org, llc, hor, ver = cam[0], cam[1], cam[2], cam[3]
    ys, xs = np.meshgrid(np.arange(y0, y0 + th), np.arange(x0, x0 + tw), indexing="ij")
    ys = ys.reshape(-1).astype(np.int64)
    xs = xs.reshape(-1).astype(np.int64)
    seed = (ys * width + xs).astype(np.uint32)                                 # :164
    seed = pcg(seed)
    ru = seed.astype(F) / F(4294967296.0)
    seed = pcg(seed)
    rv = seed.astype(F) / F(4294967296.0)
    u = (xs.astype(F) + ru) / F(width)                                          # :167
    v = ((height - 1 - ys).astype(F) + rv) / F(height)                          # :168
    d = [((llc[k] + hor[k] * u) + ver[k] * v) - org[k] for k in range(3)]
    ln = np.sqrt(_dot(d[0], d[1], d[2], d[0], d[1], d[2]))                      # :173
    return make_rays(np.broadcast_to(org, (xs.size, 3)), np.stack([d[0] / ln, d[1] / ln, d[2] / ln], 1))


def closest_hits(vertices, nodes, rays, on_node=None):
    """Returns (hits HIT_DTYPE[n], node_visits int64[n], tri_tests int64[n]).
    A ray with a non-finite origin / direction component or an all-zero
    direction is not walked (tri = -2, t = 0, no counts); t_max >= T_MAX or
    NaN is T_MAX; a miss has tri = -1 and t = the effective t_max.
    on_node(ray indices, the six slab products) sees every node visit."""
    V = np.frombuffer(bytes(vertices), np.float32)
    V = V[: (V.size // 12) * 12].reshape(-1, 3, 4)[:, :, :3]
    nb = np.frombuffer(bytes(nodes), np.uint8)
    nb = nb[: (nb.size // 48) * 48].reshape(-1, 48)
    BMIN = nb[:, 0:12].copy().view(np.float32).reshape(-1, 3)
    BMAX = nb[:, 16:28].copy().view(np.float32).reshape(-1, 3)
    DATA = nb[:, 32:36].copy().view(np.int32).reshape(-1)
    COUNT = nb[:, 36:40].copy().view(np.int32).reshape(-1)
    rays = np.asarray(rays)
    if rays.dtype != RAY_DTYPE:
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8).view(RAY_DTYPE).reshape(-1)
    n = len(rays)
    O = rays["origin"].astype(F)
    D = rays["dir"].astype(F)
    tm = rays["t_max"].astype(F)
    tm = np.where(tm < T_MAX, tm, T_MAX).astype(F)               # NaN or >= T_MAX: T_MAX
    valid = np.isfinite(O).all(1) & np.isfinite(D).all(1) & (D != 0).any(1)

    hits = np.zeros(n, HIT_DTYPE)
    hits["tri"] = -2
    node_visits = np.zeros(n, np.int64)
    tri_tests = np.zeros(n, np.int64)
    act = np.nonzero(valid)[0]
    A = act.size
    closest = tm[act].copy()
    hit = np.full(A, -1, np.int64)
    nx = np.zeros(A, F); ny = np.zeros(A, F); nz = np.zeros(A, F)
    rox, roy, roz = O[act, 0], O[act, 1], O[act, 2]
    rdx, rdy, rdz = D[act, 0], D[act, 1], D[act, 2]
    stack = np.zeros((A, 64), np.int64)
    sp = np.zeros(A, np.int64)
    nv = np.zeros(A, np.int64)
    nt = np.zeros(A, np.int64)
    if BMIN.shape[0] > 0:
        sp[:] = 1                                                                # stack[0] = the root (:185-186)
    while True:
        w = np.nonzero(sp > 0)[0]
        if w.size == 0:
            break
        sp[w] -= 1
        node = stack[w, sp[w]]
        nv[w] += 1
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):    # 1/0 = inf, as on the GPU
            ix = F(1.0) / rdx[w]; iy = F(1.0) / rdy[w]; iz = F(1.0) / rdz[w]    # hit_aabb :88-103
            t0x = (BMIN[node, 0] - rox[w]) * ix; t1x = (BMAX[node, 0] - rox[w]) * ix
            t0y = (BMIN[node, 1] - roy[w]) * iy; t1y = (BMAX[node, 1] - roy[w]) * iy
            t0z = (BMIN[node, 2] - roz[w]) * iz; t1z = (BMAX[node, 2] - roz[w]) * iz
        if on_node is not None:
            on_node(act[w], (t0x, t1x, t0y, t1y, t0z, t1z))
        te = np.fmax(np.fmax(np.fmin(t0x, t1x), np.fmin(t0y, t1y)), np.fmin(t0z, t1z))
        tx = np.fmin(np.fmin(np.fmax(t0x, t1x), np.fmax(t0y, t1y)), np.fmax(t0z, t1z))
        hb = (tx > te) & (tx > T_MIN) & (te < closest[w])
        leaf = hb & (COUNT[node] < 0)
        inner = hb & (COUNT[node] >= 0)
        wi = w[inner]; ni = node[inner]                                          # push right, then left
        stack[wi, sp[wi]] = COUNT[ni]; sp[wi] += 1
        stack[wi, sp[wi]] = DATA[ni]; sp[wi] += 1
        wl = w[leaf]
        if wl.size:                                                              # hit_triangle :105-129
            nt[wl] += 1
            tri = -(DATA[node[leaf]].astype(np.int64) + 1)
            v0 = V[tri, 0]; v1 = V[tri, 1]; v2 = V[tri, 2]
            e1x = v1[:, 0] - v0[:, 0]; e1y = v1[:, 1] - v0[:, 1]; e1z = v1[:, 2] - v0[:, 2]
            e2x = v2[:, 0] - v0[:, 0]; e2y = v2[:, 1] - v0[:, 1]; e2z = v2[:, 2] - v0[:, 2]
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                pxx, pxy, pxz = _cross(rdx[wl], rdy[wl], rdz[wl], e2x, e2y, e2z)
                det = _dot(e1x, e1y, e1z, pxx, pxy, pxz)
                ok = ~((det > F(-0.00001)) & (det < F(0.00001)))
                inv_det = F(1.0) / det
                sx = rox[wl] - v0[:, 0]; sy = roy[wl] - v0[:, 1]; sz = roz[wl] - v0[:, 2]
                uu = inv_det * _dot(sx, sy, sz, pxx, pxy, pxz)
                ok &= ~((uu < F(0.0)) | (uu > F(1.0)))
                qx, qy, qz = _cross(sx, sy, sz, e1x, e1y, e1z)
                vv = inv_det * _dot(rdx[wl], rdy[wl], rdz[wl], qx, qy, qz)
                ok &= ~((vv < F(0.0)) | ((uu + vv) > F(1.0)))
                t = inv_det * _dot(e2x, e2y, e2z, qx, qy, qz)
                ok &= (t > T_MIN) & (t < closest[wl])
                g = wl[ok]
                closest[g] = t[ok]
                hit[g] = tri[ok]
                cnx, cny, cnz = _cross(e1x[ok], e1y[ok], e1z[ok], e2x[ok], e2y[ok], e2z[ok])
                ln = np.sqrt(_dot(cnx, cny, cnz, cnx, cny, cnz))
                cnx, cny, cnz = cnx / ln, cny / ln, cnz / ln                     # :124
                flip = _dot(rdx[g], rdy[g], rdz[g], cnx, cny, cnz) > F(0.0)      # :125
            nx[g] = np.where(flip, -cnx, cnx); ny[g] = np.where(flip, -cny, cny); nz[g] = np.where(flip, -cnz, cnz)
        if (sp > 62).any():
            raise RuntimeError("stack overflow (reference int stack[64])")
    gh = hit >= 0
    out = np.zeros(A, HIT_DTYPE)
    out["t"] = closest                                                           # a miss: the effective t_max
    out["tri"] = hit
    with np.errstate(invalid="ignore", over="ignore"):
        pos = np.stack([rox + rdx * closest, roy + rdy * closest, roz + rdz * closest], 1)   # ray_at :77-79
    out["normal"] = np.where(gh[:, None], np.stack([nx, ny, nz], 1), F(0.0))
    out["pos"] = np.where(gh[:, None], pos, F(0.0))
    hits[act] = out
    node_visits[act] = nv
    tri_tests[act] = nt
    return hits, node_visits, tri_tests


def oracle_triangle_hits(vertices, rays, hits, closest_start):
    """orc_hit_triangle (oracle/rt_oracle.c, the contract's hit_triangle) on
    (ray i, triangle hits[i].tri) with closest_t = closest_start[i], for every
    record with tri >= 0: returns (indices, accepted bool[], t float32[],
    normal float32[, 3]) of those records."""
    import ctypes as C
    from oracle import oracle_lib
    L = oracle_lib.lib()
    V = np.frombuffer(bytes(vertices), np.float32)
    V = np.ascontiguousarray(V[: (V.size // 12) * 12].reshape(-1, 3, 4)[:, :, :3])
    idx = np.nonzero(hits["tri"] >= 0)[0]
    ok = np.zeros(idx.size, bool)
    t = np.zeros(idx.size, F)
    nrm = np.zeros((idx.size, 3), F)
    f3 = C.c_float * 3
    for k, i in enumerate(idx):
        c = C.c_float(float(closest_start[i]))
        n = f3()
        tri = V[int(hits["tri"][i])]
        ok[k] = L.orc_hit_triangle(f3(*rays["origin"][i]), f3(*rays["dir"][i]), f3(*tri[0]), f3(*tri[1]), f3(*tri[2]),
                                   C.byref(c), n) != 0
        t[k] = c.value
        nrm[k] = n[:]
    return idx, ok, t, nrm


def leaf_box_entered(nodes, rays, tris, closest):
    """orc_hit_aabb (the contract's hit_aabb, :88-103) of ray i against the
    leaf box of flattened triangle tris[i] at closest_t = closest[i]: bool[n].
    A hit at t0 whose own leaf box has t_enter >= t0 (rounding can put a
    triangle's t a little before its box's t_enter; DESIGN.md §4a calls such a
    hit inconsistent) is found only while closest_t is still above that
    t_enter, so lowering t_max to just above t0 loses it: in the reference
    too, since its hit_aabb compares t_enter < closest_t."""
    import ctypes as C
    from oracle import oracle_lib
    L = oracle_lib.lib()
    nb = np.frombuffer(bytes(nodes), np.uint8)
    nb = nb[: (nb.size // 48) * 48].reshape(-1, 48)
    BMIN = nb[:, 0:12].copy().view(np.float32).reshape(-1, 3)
    BMAX = nb[:, 16:28].copy().view(np.float32).reshape(-1, 3)
    DATA = nb[:, 32:36].copy().view(np.int32).reshape(-1)
    COUNT = nb[:, 36:40].copy().view(np.int32).reshape(-1)
    leaf_of = {int(-(d + 1)): i for i, (d, c) in enumerate(zip(DATA, COUNT)) if c < 0}
    f3 = C.c_float * 3
    out = np.zeros(len(tris), bool)
    for k, tri in enumerate(tris):
        i = leaf_of[int(tri)]
        out[k] = L.orc_hit_aabb(f3(*rays["origin"][k]), f3(*rays["dir"][k]), f3(*BMIN[i]), f3(*BMAX[i]),
                                float(T_MIN), float(closest[k])) != 0
    return out


def segment_rays(vertices, materials, nodes, camera_ubo: bytes, width: int, height: int, max_bounces: int):
    """The rays the reference's paths follow, bounce by bounce (bounce 0 = the
    primary rays; later origins lie on surfaces): RAY_DTYPE records with
    t_max = T_MAX, handed out by oracle/shader_np.render(on_segment=...)."""
    from oracle import shader_np
    got = []

    def on_segment(b, px, o, d, visits):
        got.append(make_rays(o, d))

    shader_np.render(vertices, materials, nodes, camera_ubo, width, height, max_bounces, on_segment=on_segment)
    return np.concatenate(got)
