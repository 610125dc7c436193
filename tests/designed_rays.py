"""designed_rays.py — rays and cameras built to land on the walk's edge cases.

TEST INFRASTRUCTURE ONLY (a helper, not a test; numpy only).

Every other ray the suite walks comes from a PCG-jittered camera or a scatter
off such a path, and such a ray almost never has a direction component that is
exactly +0.0, -0.0 or denormal, an origin exactly in a box plane (the slab
product (b - o) * (1 / d) is then 0 * inf = NaN), a hit exactly on a triangle's
edge or vertex, a second triangle at the same t, or a t_max equal to a hit's t.
Here every ray has some of these, over the "grid" scene of
test_accel_model._tie_scenes(): 300 triangles whose vertices are multiples of
4 in [-12, 12]^3, so box planes, edges and vertices lie at coordinates that
float32 rays reach exactly.

  scene()          the grid scene (built once)
  battery(scene)   (rays RAY_DTYPE[n], tags str[n]): the classes of CLASSES
  cameras()        {name: 80-byte UBO}: degenerate viewports (KINDS)
  stats(scene, rays)  what the conditions of tests/test_designed_rays.py need
"""
from __future__ import annotations

import functools
import itertools

import numpy as np

import query_ref as Q

F = np.float32
LATTICE = np.arange(-12.0, 13.0, 4.0, dtype=F)         # the 7 coordinates a vertex can have
FAR = F(40.0)                                          # where rays start, outside the mesh
CLASSES = ("axis", "plane", "diag", "denorm", "inside", "surface", "half")
KINDS = ("plane", "axis", "denorm", "negzero", "diag")


@functools.lru_cache(maxsize=None)
def scene():
    from test_accel_model import _tie_scenes
    return _tie_scenes()["grid"]


def _tables(built):
    """(V[n, 3, 3], BMIN[m, 3], BMAX[m, 3], DATA[m], COUNT[m]) of the scene's buffers."""
    V = np.frombuffer(bytes(built.model_vertex_data), F)
    V = V[: (V.size // 12) * 12].reshape(-1, 3, 4)[:, :, :3]
    nb = np.frombuffer(bytes(built.flat_bvh_data), np.uint8)
    nb = nb[: (nb.size // 48) * 48].reshape(-1, 48)
    return (V, nb[:, 0:12].copy().view(F).reshape(-1, 3), nb[:, 16:28].copy().view(F).reshape(-1, 3),
            nb[:, 32:36].copy().view(np.int32).reshape(-1), nb[:, 36:40].copy().view(np.int32).reshape(-1))


def _unit(d):
    """d / |d| in float32, in the operation order of the shader's normalize."""
    d = np.asarray(d, F).reshape(-1, 3)
    ln = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    return (d / ln[:, None]).astype(F)


def _vec(k, a, b, c):
    """The vector with a on axis k, b on the next axis and c on the one after."""
    v = np.empty(3, F)
    v[k], v[(k + 1) % 3], v[(k + 2) % 3] = a, b, c
    return v


def _signed_zero(negative):
    return F(-0.0) if negative else F(0.0)


# ----------------------------------------------------------------- classes --

def _axis():
    """From every lattice point of the six faces 40 out, straight in: +-1 on
    one axis, every sign combination of +0.0 / -0.0 on the other two."""
    o, d = [], []
    for k, s in itertools.product(range(3), (1.0, -1.0)):
        for a, b in itertools.product(LATTICE, LATTICE):
            for za, zb in itertools.product((False, True), repeat=2):
                org = np.empty(3, F)
                org[k], org[(k + 1) % 3], org[(k + 2) % 3] = -s * FAR, a, b
                dr = np.empty(3, F)
                dr[k], dr[(k + 1) % 3], dr[(k + 2) % 3] = s, _signed_zero(za), _signed_zero(zb)
                o.append(org)
                d.append(dr)
    return np.array(o), np.array(d)


def _plane(rng):
    """One component +-0.0 and the origin in a lattice plane of that axis; the
    other two components generic, aimed from outside at a point of the mesh."""
    o, d = [], []
    # (a ray in a face plane of the root box misses everything: +-12 twice, for the misses)
    for k, c, neg in itertools.product(range(3), tuple(LATTICE) + (-12.0, 12.0), (False, True)):
        for _ in range(8):
            ang = rng.uniform(0.0, 2.0 * np.pi)
            org = np.empty(3, F)
            org[k] = c
            org[(k + 1) % 3] = F(FAR * np.cos(ang))
            org[(k + 2) % 3] = F(FAR * np.sin(ang))
            at = rng.uniform(-13.0, 13.0, 3).astype(F)
            dr = (at - org).astype(F)
            dr[k] = 0.0
            dr = _unit(dr)[0]
            dr[k] = _signed_zero(neg)
            o.append(org)
            d.append(dr)
    return np.array(o), np.array(d)


def _diag():
    """Float-normalised lattice diagonals through lattice points, started 8
    lattice steps back: they run along triangle edges and through vertices."""
    o, d = [], []
    # in a lattice plane (one component exactly 0): slopes 1, 2 and 1/2
    for k in range(3):
        for a, b in ((1, 1), (1, -1), (-1, 1), (-1, -1), (1, 2), (-2, 1), (2, -1), (-1, -2)):
            for c, p, q in itertools.product((-12.0, -8.0, 0.0, 4.0, 12.0), (-12.0, -8.0, 0.0, 8.0), (-4.0, 4.0, 12.0)):
                v = _vec(k, 0.0, a, b)
                o.append((_vec(k, c, p, q) - F(32.0) * v).astype(F))        # exact: small integers
                d.append(_unit(v)[0])
    # a few body diagonals (no zero component, so no NaN: finite * 0 = 0)
    for v, p in zip(itertools.product((-1, 1), repeat=3), itertools.cycle(((0, 0, 0), (8, -8, 0), (-4, 4, 8)))):
        for m in (1.0, 2.0):
            v2 = np.array(v, F) * np.array((1.0, 1.0, m), F)
            o.append((np.array(p, F) - F(32.0) * v2).astype(F))
            d.append(_unit(v2)[0])
    return np.array(o), np.array(d)


DENORMALS = (1e-42, -1e-39, 1e-45, -1e-45, 1.1754942e-38, -3e-41)


def _denorm():
    """A +-1 beside denormal components (and one exact zero now and then), from
    lattice points and from points between them."""
    o, d = [], []
    coords = (-14.0, -12.0, -8.0, -6.0, -4.0, 0.0, 2.0, 4.0, 8.0, 12.0, 13.0)
    i = 0
    for k, s in itertools.product(range(3), (1.0, -1.0)):
        for a, b in itertools.product(coords, coords):
            org = np.empty(3, F)
            org[k], org[(k + 1) % 3], org[(k + 2) % 3] = -s * FAR, a, b
            dr = np.empty(3, F)
            dr[k] = s
            dr[(k + 1) % 3] = DENORMALS[i % 6]
            dr[(k + 2) % 3] = 0.0 if i % 5 == 0 else DENORMALS[(i // 6 + 3) % 6]
            o.append(org)
            d.append(dr)
            i += 1
    return np.array(o)[::2], np.array(d)[::2]


def _some_dirs():
    dirs = [v for v in itertools.product((-1, 0, 1), repeat=3) if any(v)]
    dirs += [(3, 1, -2), (-1, 4, 2), (2, -3, 5), (-5, -2, 1)]
    return _unit(np.array(dirs, F))


def _inside(built):
    """From the corners and the centres of leaf and inner boxes: the origin lies
    in box planes and t_enter is negative or zero."""
    _, BMIN, BMAX, _, COUNT = _tables(built)
    dirs = _some_dirs()
    o, d = [], []
    j = 0
    inner = np.nonzero(COUNT >= 0)[0]
    leaf = np.nonzero(COUNT < 0)[0]
    for nodes in (inner[:: max(1, len(inner) // 40)], leaf[:: max(1, len(leaf) // 40)]):
        for n in nodes:
            lo, hi = BMIN[n], BMAX[n]
            corner = np.where(np.array([(j >> 0) & 1, (j >> 1) & 1, (j >> 2) & 1], bool), hi, lo).astype(F)
            centre = ((lo + hi) * F(0.5)).astype(F)
            for p in (corner, centre):
                for q in range(3):
                    o.append(p)
                    d.append(dirs[(j * 7 + q * 11) % len(dirs)])
                j += 1
    return np.array(o), np.array(d)


def _surface(built):
    """Origins exactly on a triangle (a vertex, an edge midpoint, the centroid)
    with directions along its normal, against it and along an edge: t == 0
    on that triangle, so T_MIN decides."""
    V = _tables(built)[0]
    o, d = [], []
    for t in range(0, len(V), 5):
        v0, v1, v2 = V[t]
        e1, e2 = (v1 - v0).astype(F), (v2 - v0).astype(F)
        n = np.cross(e1, e2).astype(F)
        if not n.any():
            continue
        n = _unit(n)[0]
        pts = (v0, ((v0 + v1) * F(0.5)).astype(F), (((v0 + v1) + v2) / F(3.0)).astype(F))
        p = pts[(t // 5) % 3]
        for dr in (n, -n, _unit(e1)[0], _unit((v2 - v1).astype(F))[0]):
            o.append(p)
            d.append(dr)
    return np.array(o), np.array(d)


@functools.lru_cache(maxsize=None)
def _battery():
    built = scene()
    rng = np.random.default_rng(20)
    parts = [("axis", _axis()), ("plane", _plane(rng)), ("diag", _diag()), ("denorm", _denorm()),
             ("inside", _inside(built)), ("surface", _surface(built))]
    rays = [Q.make_rays(o, d) for _, (o, d) in parts]
    tags = [np.full(len(r), name) for (name, _), r in zip(parts, rays)]
    # directions scaled by 0.5 (exact, but for a denormal's last bit): no longer
    # unit, so the accel tree hands them to the reference-order walk
    some = np.concatenate(rays[:5])[3::9].copy()
    some["dir"] *= F(0.5)
    rays.append(some)
    tags.append(np.full(len(some), "half"))
    rays, tags = np.concatenate(rays), np.concatenate(tags)
    n2 = (rays["dir"].astype(np.float64) ** 2).sum(1)
    assert (np.abs(n2[tags != "half"] - 1.0) < 2.0 ** -11).all()
    rays.setflags(write=False)
    tags.setflags(write=False)
    return rays, tags


def battery(built=None):
    """(rays, tags) over scene(); read-only arrays shared by every caller."""
    assert built is None or built is scene()
    return _battery()


# ----------------------------------------------------------------- cameras --

class Ubo(bytes):
    """80 raw UBO bytes that also answer ubo_bytes(), so the suite's helpers
    written for rtamd's Camera (and the renderer, which takes bytes) accept them."""

    def ubo_bytes(self) -> bytes:
        return bytes(self)


def ubo(origin, lower_left, horizontal, vertical, frame_count=0) -> Ubo:
    """The 80-byte camera UBO: origin, lower_left, horizontal, vertical as vec4
    (w = 0), frame_count at byte 64, then sky_enabled = 1 and padding."""
    f = np.zeros(16, F)
    for i, v in enumerate((origin, lower_left, horizontal, vertical)):
        f[4 * i: 4 * i + 3] = np.asarray(v, F)
    return Ubo(f.tobytes() + np.array([frame_count, 1, 0, 0], np.int32).tobytes())


def _fan(k, s, c, f, vertical=0.0, negative=False, half=14.0):
    """A viewport that is a line: from (c on axis k, -s * 40 on axis k+1, f on
    axis k+2) a fan of rays over -half .. half of axis k+2, in the plane c of
    axis k (the mesh spans -12 .. 12: a half of 24 sends rays past it).  On
    axis k lower_left equals the origin and horizontal is 0, vertical is
    `vertical`; negative: those three are -0.0 against an origin of +0.0."""
    org = _vec(k, c, -s * FAR, f)
    z = F(-0.0) if negative else F(0.0)
    assert not (negative and c != 0.0)
    return ubo(org, _vec(k, z if negative else c, 0.0, -half), _vec(k, z, 0.0, 2.0 * half),
               _vec(k, z if negative else vertical, 0.0, 0.0))


@functools.lru_cache(maxsize=None)
def cameras():
    """Degenerate viewports, all aimed at the mesh from 40 out; k is the axis
    whose direction component is zero, the view runs along axis k+1 (cyclic)
    in the sign named p or n, the pixels fan out over axis k+2:
      plane:   horizontal along one axis only, vertical = 0: every pixel's ray
               has d[k] = +0.0 and lies in the plane c of axis k
      axis:    horizontal = vertical = 0: one axis-aligned ray for all pixels,
               whose paths part at the first scatter
      denorm:  plane with vertical[k] = 1e-42: d[k] is denormal (c = 0: any
               other origin absorbs it)
      negzero: plane with lower_left[k] = horizontal[k] = vertical[k] = -0.0
               and origin[k] = +0.0: d[k] = -0.0 on every pixel
      diag:    as axis, along a lattice diagonal through a lattice point
    Origins lie at the lattice coordinates 0, 4 and -12 and at 2, off the
    lattice.  -12 is never the plane's own c, nor an axis ray's: such a ray
    lies in a face plane of the root box and by the contract misses it."""
    out = {}
    for k, s in itertools.product(range(3), (1.0, -1.0)):
        ax = "xyz"[k] + ("p" if s > 0 else "n")
        for c, f in ((0.0, 0.0), (4.0, 2.0), (2.0, 4.0), (4.0, -12.0)):
            out[f"plane_{ax}_{c:g}_{f:g}"] = _fan(k, s, c, f, half=24.0 if f == -12.0 else 14.0)
    # (both other coordinates on the lattice, one, or none: hits on an edge, tied, or generic)
    for (k, s), (a, b) in zip(itertools.product(range(3), (1.0, -1.0)),
                              ((0.0, 0.0), (4.0, -8.0), (0.0, 4.0), (4.0, 4.0), (4.0, 0.0), (2.0, 4.0))):
        org = _vec(k, -s * FAR, a, b)
        out[f"axis_{'xyz'[k]}{'p' if s > 0 else 'n'}"] = ubo(org, _vec(k, 0.0, a, b), np.zeros(3), np.zeros(3))
    for k in range(3):
        s = 1.0 if k != 1 else -1.0
        out[f"denorm_{'xyz'[k]}"] = _fan(k, s, 0.0, (0.0, 4.0, 2.0)[k], vertical=1e-42)
        out[f"negzero_{'xyz'[k]}"] = _fan(k, -s, 0.0, (4.0, 2.0, -12.0)[k], negative=True, half=(14.0, 24.0, 24.0)[k])
    # diag: horizontal = vertical = 0 and a lattice diagonal: one ray through the
    # lattice point p, along edges and through box corners (t_exit == t_enter
    # there: both slabs give the same product, the direction's components being equal)
    for i, (v, p) in enumerate((((1, -1, 0), (-8, -8, 0)), ((1, 0, 1), (-8, -8, -4)), ((-1, 0, 1), (-8, -4, -4)),
                                ((0, 1, 1), (-8, -8, 4)), ((1, 1, 1), (-8, -8, -8)), ((-1, 1, -1), (-8, -8, 0)),
                                ((1, 2, 0), (-8, -4, -8)), ((0, -2, 1), (-8, 4, -8)), ((2, 0, -1), (-8, -8, 8)))):
        v, p = np.array(v, F), np.array(p, F)
        out[f"diag_{i}"] = ubo(p - F(32.0) * v, p, np.zeros(3), np.zeros(3))
    return out


def frame_of(ray):
    """The one-ray camera (horizontal = vertical = 0) whose 1 x 1 frame has
    exactly `ray` as its primary ray, or None where no viewport produces it.
    It exists for a direction that is a float-normalised vector of small
    integers v (normalize(32 v) has the same bits) from an origin of small
    integers, except for a -0.0 component: the viewport sum ends in
    (lower_left - origin), which is +0.0 on a zero axis unless the origin is
    +0.0 there and lower_left, horizontal and vertical are all -0.0."""
    o, d = ray["origin"].astype(F), ray["dir"].astype(F)
    if not np.isfinite(d).all() or not d.any():
        return None
    v = np.round(d / np.abs(d[d != 0]).min()).astype(F)
    neg = (d == 0) & np.signbit(d)
    z = np.where(neg, F(-0.0), F(0.0))
    u = ubo(o, np.where(neg & (o == 0), z, o + F(32.0) * v), z, z)
    return u if Q.primary_rays(u, 1, 1).tobytes() == ray.tobytes() else None


# ------------------------------------------------------------------- stats --

def slab_nan(built, rays):
    """bool[n]: some node the reference's walk of the ray visits has a NaN slab
    product.  (The walk below is query_ref.closest_hits's, hits included, so the
    nodes are the ones the reference tests.)"""
    seen = np.zeros(len(rays), bool)

    def on_node(idx, products):
        bad = np.zeros(len(idx), bool)
        for p in products:
            bad |= np.isnan(p)
        seen[idx[bad]] = True

    Q.closest_hits(built.model_vertex_data, built.flat_bvh_data, rays, on_node=on_node)
    return seen


def all_triangle_hits(built, rays):
    """hit_triangle (:105-129) of every ray against every distinct triangle,
    with closest_t = the ray's effective t_max: (ok bool[n, m], t, u, v
    float32[n, m], index int[m] of each distinct triangle's first copy)."""
    V = _tables(built)[0]
    _, first = np.unique(V.reshape(len(V), 9).view(np.uint32), axis=0, return_index=True)
    first = np.sort(first)
    V = V[first]
    O = rays["origin"][:, None, :].astype(F)
    D = rays["dir"][:, None, :].astype(F)
    tm = rays["t_max"].astype(F)
    tm = np.where(tm < Q.T_MAX, tm, Q.T_MAX).astype(F)[:, None]
    v0 = V[None, :, 0]
    e1 = (V[:, 1] - V[:, 0])[None]
    e2 = (V[:, 2] - V[:, 0])[None]
    c, dt = Q._cross, Q._dot
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        p = c(D[..., 0], D[..., 1], D[..., 2], e2[..., 0], e2[..., 1], e2[..., 2])
        det = dt(e1[..., 0], e1[..., 1], e1[..., 2], *p)
        ok = ~((det > F(-0.00001)) & (det < F(0.00001)))
        inv = F(1.0) / det
        s = [O[..., i] - v0[..., i] for i in range(3)]
        u = inv * dt(*s, *p)
        ok &= ~((u < F(0.0)) | (u > F(1.0)))
        q = c(*s, e1[..., 0], e1[..., 1], e1[..., 2])
        v = inv * dt(D[..., 0], D[..., 1], D[..., 2], *q)
        ok &= ~((v < F(0.0)) | ((u + v) > F(1.0)))
        t = inv * dt(e2[..., 0], e2[..., 1], e2[..., 2], *q)
        ok &= (t > Q.T_MIN) & (t < tm)
    return ok, t, u, v, first


def stats(built, rays):
    """{"nan": bool[n] a NaN slab product at some visited node, "hit": bool[n],
    "edge": bool[n] the hit has u == 0, v == 0 or u + v == 1 exactly,
    "tie": bool[n] a second, different triangle is hit at the same t}."""
    hits, _, _ = Q.closest_hits(built.model_vertex_data, built.flat_bvh_data, rays)
    hit = hits["tri"] >= 0
    ok, t, u, v, first = all_triangle_hits(built, rays)
    V = _tables(built)[0]
    same = ok & (t == hits["t"][:, None])
    # the hit's own triangle among the distinct ones
    key = {V[i].tobytes(): j for j, i in enumerate(first)}
    own = np.array([key[V[i].tobytes()] if i >= 0 else 0 for i in hits["tri"]])
    r = np.arange(len(rays))
    assert (same[r, own] | ~hit).all()
    uu, vv = u[r, own], v[r, own]
    edge = hit & ((uu == 0) | (vv == 0) | ((uu + vv) == F(1.0)))
    return {"nan": slab_nan(built, rays), "hit": hit, "edge": edge, "tie": hit & (same.sum(1) >= 2)}
