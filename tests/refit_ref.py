"""The refit in numpy: what rt_refit_scene writes into the
reference's buffers and what rt_accel_refit_records (and the device) write
into format-0 accel records, restated independently of csrc/.

Also the scenes and deformations the refit tests share."""
import math

import numpy as np

FORCE = np.uint32(1 << 29)          # accel_build.h kAccelForce
IDX = (1 << 29) - 1                 # a skip or a triangle index
EPS = 0.0001                        # Triangle.java:65


# ------------------------------------------------------------ reference side --

def _jmin(a, b):
    """java.lang.Math.min on doubles without NaN: -0.0 < +0.0."""
    return np.where((a == 0) & (b == 0), np.where(np.signbit(a), a, b), np.where(a <= b, a, b))


def _jmax(a, b):
    return np.where((a == 0) & (b == 0), np.where(np.signbit(a), b, a), np.where(a >= b, a, b))


def tri_boxes(tri_verts):
    """Triangle.calculateBoundingBox (Triangle.java:61-71) of (n, 9) doubles:
    (lo, hi), each (n, 3) doubles."""
    v = np.asarray(tri_verts, dtype=np.float64).reshape(-1, 3, 3)
    lo = _jmin(v[:, 0], _jmin(v[:, 1], v[:, 2]))
    hi = _jmax(v[:, 0], _jmax(v[:, 1], v[:, 2]))
    for k in range(3):                       # each add touches all three components (x + 0.0)
        flat = hi[:, k] - lo[:, k] < EPS
        add = np.zeros(3)
        add[k] = EPS
        hi[flat] = hi[flat] + add
    return lo, hi


def node_fields(nodes):
    """(data, count) int32 arrays of a node buffer."""
    w = np.ascontiguousarray(nodes, dtype=np.uint8).view(np.int32).reshape(-1, 12)
    return w[:, 8].copy(), w[:, 9].copy()


def refit_scene(built, tri_verts):
    """rt_refit_scene: (vertex floats, node bytes) of built's tree for the
    moved input triangles."""
    tri_verts = np.asarray(tri_verts, dtype=np.float64).reshape(-1, 9)
    src = np.asarray(built.flat_source, dtype=np.int64)
    verts = np.zeros((src.size, 12), dtype=np.float32)
    verts.reshape(-1, 3, 4)[:, :, :3] = tri_verts[src].reshape(-1, 3, 3).astype(np.float32)
    nodes = np.array(built.flat_bvh_data, dtype=np.uint8, copy=True)
    data, count = node_fields(nodes)
    tlo, thi = tri_boxes(tri_verts)
    n = data.size
    lo, hi = np.zeros((n, 3)), np.zeros((n, 3))
    for k in range(n - 1, -1, -1):           # children have higher preorder indices
        if count[k] < 0:
            t = src[-(int(data[k]) + 1)]
            lo[k], hi[k] = tlo[t], thi[t]
        else:
            lo[k] = _jmin(lo[data[k]], lo[count[k]])
            hi[k] = _jmax(hi[data[k]], hi[count[k]])
    f = nodes.view(np.float32).reshape(-1, 12)
    f[:, 0:3] = lo.astype(np.float32)
    f[:, 4:7] = hi.astype(np.float32)
    return verts.reshape(-1), nodes


# ---------------------------------------------------------------- accel side --

def thin(e1, e2):
    """accel_class(e1, e2) >= 7 (accel_build.cpp), in double from float edges."""
    a = [float(x) for x in e1]
    b = [float(x) for x in e2]
    c = [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
    den = math.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]) * math.sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2])
    num = math.sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2])
    if den == 0.0 or math.isnan(den):
        return True
    s = num / den
    if not s > 0.0:
        return True
    return math.floor(-math.log2(s)) >= 7


def refit_records(words, n_layouts, verts, nodes):
    """rt_accel_refit_records in numpy: a refitted copy of `words`."""
    w = np.array(words, dtype=np.uint32, copy=True)
    slots = (w.size - 16) // (8 * n_layouts)
    if slots == 0:
        return w
    fw = w.view(np.float32)
    v = np.asarray(verts, dtype=np.float32).reshape(-1, 3, 4)[:, :, :3]
    nf = np.ascontiguousarray(nodes, dtype=np.uint8).view(np.float32).reshape(-1, 12)
    data, count = node_fields(nodes)
    leaf_of = {}
    for k in np.flatnonzero(count < 0):
        t = -(int(data[k]) + 1)
        assert t not in leaf_of, f"two leaves name triangle {t}"
        leaf_of[t] = int(k)
    canon = {}                                # (least triangle, slots) of a subtree -> its box and bit

    def visit(s, layout0):
        """Returns (least triangle, slots) of the subtree at slot s."""
        base = 8 * s
        w3 = int(w[base + 3])
        if (w3 >> 30) & 1:
            tri = w3 & IDX
            k = leaf_of[tri]
            fw[base:base + 3] = nf[k, 0:3]
            fw[base + 4:base + 7] = nf[k, 4:7]
            e1 = v[tri, 1] - v[tri, 0]        # float32 differences
            e2 = v[tri, 2] - v[tri, 0]
            w[base + 3] = np.uint32((w3 & ~int(FORCE)) | (int(FORCE) if thin(e1, e2) else 0))
            fw[base + 7:base + 10] = v[tri, 0]
            fw[base + 10:base + 13] = e1
            fw[base + 13:base + 16] = e2
            return tri, 2
        skip = w3 & IDX
        a = s + 1
        ka = visit(a, layout0)
        b = a + ka[1]
        kb = visit(b, layout0)
        assert b + kb[1] == skip
        key = (min(ka[0], kb[0]), skip - s)
        if layout0:                          # the first child is the lower-centroid one: the first operand
            lo, hi = np.empty(3, np.float32), np.empty(3, np.float32)
            for q in range(3):
                x, y = fw[8 * a + q], fw[8 * b + q]
                lo[q] = y if y < x else x
                x, y = fw[8 * a + 4 + q], fw[8 * b + 4 + q]
                hi[q] = y if x < y else x
            bit = (int(w[8 * a + 3]) | int(w[8 * b + 3])) & int(FORCE)
            canon[key] = (lo.copy(), hi.copy(), bit)
        lo, hi, bit = canon[key]
        fw[base:base + 3] = lo
        fw[base + 4:base + 7] = hi
        w[base + 3] = np.uint32((w3 & ~int(FORCE)) | bit)
        return key

    for o in range(n_layouts):
        visit(o * slots, o == 0)
    return w


def broken_duplicates(words, n_layouts, verts, nodes):
    """The triangles a reference leaf names that the records do not hold (the
    accel build dropped them as byte-identical copies) and whose vertex record
    and leaf box are no longer any held triangle's: a scene a refit refuses."""
    if np.asarray(nodes).size < 48:
        return []
    held = set(leaf_bits(words, n_layouts)[0])
    v = np.ascontiguousarray(verts, dtype=np.float32).view(np.uint32).reshape(-1, 12)
    nb = np.ascontiguousarray(nodes, dtype=np.uint8).view(np.uint32).reshape(-1, 12)
    data, count = node_fields(nodes)
    key = {}
    for k in np.flatnonzero(count < 0):
        t = -(int(data[k]) + 1)
        key[t] = (tuple(v[t]), tuple(nb[k, [0, 1, 2, 4, 5, 6]]))
    have = {key[t] for t in held}
    return sorted(t for t in key if t not in held and key[t] not in have)


def leaf_bits(words, n_layouts):
    """{triangle: bit 29} of layout 0's leaves, and the root's bit."""
    w = np.asarray(words, dtype=np.uint32)
    slots = (w.size - 16) // (8 * n_layouts)
    out, s = {}, 0
    while s < slots:
        w3 = int(w[8 * s + 3])
        if (w3 >> 30) & 1:
            out[w3 & IDX] = bool(w3 & int(FORCE))
            s += 2
        else:
            s += 1
    return out, bool(int(w[3]) & int(FORCE)) if slots else False


# ------------------------------------------------------ scenes, deformations --

def _recorded_tie_inputs():
    """test_accel_model._tie_scenes' inputs: {name: (verts, mats, seed)}."""
    import rtamd
    import test_accel_model as T
    calls = []
    orig = rtamd.build_buffers

    def rec(verts, mats, seed=1):
        calls.append((np.array(verts, dtype=np.float64).reshape(-1, 9), np.array(mats, dtype=np.float32), seed))
        return orig(verts, mats, seed)
    rtamd.build_buffers = rec
    try:
        names = list(T._tie_scenes())
    finally:
        rtamd.build_buffers = orig
    return dict(zip(names, calls))


SCENES = (["random0", "random1", "random2", "random3", "twins", "twins_rev", "grid", "cube_both_diagonals", "config2"] +
          [f"tris{n}" for n in (0, 1, 2, 3, 5)])
_cache = {}


def scene(name):
    """(tri_verts (n, 9) doubles, mats, axis seed, part, camera) of a test scene;
    part = the input triangles of the object that deformations (b) and (e) move."""
    if name in _cache:
        return _cache[name]
    from rtamd import configs, triangles_of
    if name.startswith("random"):
        import test_accel_model as T
        k = int(name[6:])
        verts, mats, (eye, at), vfov = T.random_scene(k)
        tv = verts.astype(np.float64).reshape(-1, 9)
        out = (tv, mats, 1 + k % 3, np.arange(len(tv) // 3), configs.Camera(eye, at, (0.0, 1.0, 0.0), vfov, 64 / 48))
    elif name == "config2":
        tv, mats = triangles_of(configs.config2().scene)
        out = (tv, mats, 1, np.arange(2, len(tv)), configs.Camera.default(64, 48))       # the cube
    elif name.startswith("tris"):
        n = int(name[4:])
        rng = np.random.default_rng(100 + n)
        tv = rng.uniform(-20, 20, (n, 1, 3)) + rng.normal(size=(n, 3, 3)) * 8.0
        tv[:1, :, 2] = tv[:1, :1, 2]          # the first one upright (z constant): a needle once y is squashed
        tv = tv.reshape(n, 9)
        mats = np.concatenate([rng.uniform(0.1, 0.9, (n, 3)), rng.integers(0, 3, (n, 1))], 1).astype(np.float32)
        out = (tv, mats, 2, np.arange((n + 1) // 2), configs.Camera.default(64, 48))
    else:
        tv, mats, seed = _recorded_tie_inputs()[name]
        out = (tv, mats, seed, np.arange(2, min(14, len(tv))), configs.Camera.default(64, 48))
    _cache[name] = out
    return out


DEFORMATIONS = ("identity", "translate", "jitter", "squash", "flatten", "swap")


def deform(kind, tri_verts, part):
    """The states of the input triangles a deformation goes through (one, or
    two for "squash": y scaled by 1e-4 about the centroid, then the original)."""
    tv = np.asarray(tri_verts, dtype=np.float64).reshape(-1, 3, 3)
    if kind == "identity" or len(tv) == 0:
        return [tv.reshape(-1, 9).copy()] * (2 if kind == "squash" else 1)
    lo, hi = tv.reshape(-1, 3).min(0), tv.reshape(-1, 3).max(0)
    out = tv.copy()
    if kind == "translate":
        out[part] += np.array([1.5, 0.25, -2.0])
    elif kind == "jitter":
        out += np.random.default_rng(11).uniform(-1, 1, out.shape) * 0.05 * (hi - lo).max()
    elif kind == "squash":
        cy = tv[:, :, 1].mean()
        out[:, :, 1] = cy + (out[:, :, 1] - cy) * 1e-4
        return [out.reshape(-1, 9), tv.reshape(-1, 9).copy()]
    elif kind == "flatten":
        out[part, :, 1] = tv[part][:, :, 1].mean()
    elif kind == "swap":
        cx = tv[:, :, 0].mean(1)
        left = cx < np.median(cx)
        out[left, :, 0] += hi[0] - lo[0]
        out[~left, :, 0] -= hi[0] - lo[0]
    else:
        raise ValueError(kind)
    return [out.reshape(-1, 9)]
