"""tests/temporal_motion_ref.py (the numpy restatement of DESIGN.md §4m that the
GPU tests of rt_temporal_motion_device compare with) pinned from a second side
and checked for what it is for: with unmoved vertex records it is
temporal_ref.temporal bit for bit; a scalar, per-pixel restatement written from
§4m's text agrees bit for bit on translated, jittered and squashed triangles; a
rigid translation is followed to within a few spacings; on a checker that
slides one pixel per frame under a camera looking straight down no pixel mixes
the two albedos, where §4h's kernel with kept history does; degenerate
triangles and foreign triangle indices start over; the moments change no
colour; and on the CPU oracle's frames of a sliding checker it keeps most of
what the accumulation gains on a static scene."""
import functools

import numpy as np
import pytest

import denoise_ref as D
import query_ref as Q
import refit_ref as R
import temporal_motion_ref as M
import temporal_ref as T
import variance_ref as V
from test_denoise_ref import random_frame
from test_temporal_ref import look_at, random_camera_pair, random_history, share

F = np.float32


# ---- scenes -------------------------------------------------------------------

ALBEDO = ((0.8, 0.7, 0.2), (0.15, 0.2, 0.6))       # the checker's two Lambertian albedos
CELLS, CELL = 12, 1.5


def checker_scene():
    """Config 2's metal cube standing on a 12 x 12 checker of quads in the plane
    y = 0 (cells of 1.5 units, two alternating Lambertian albedos): (input
    triangles (n, 9) doubles, materials, the checker's input triangles)."""
    from rtamd import configs, triangles_of
    tv, mats = triangles_of(configs.config2().scene)
    cube, cube_mats = tv[2:].reshape(-1, 3, 3).copy(), mats[2:]
    cube[:, :, 1] += 10.0                                  # from resting on y = -10 to resting on y = 0
    quads, qm = [], []
    half = CELLS * CELL / 2.0
    for j in range(CELLS):
        for i in range(CELLS):
            x0, z0 = -half + i * CELL, -half + j * CELL
            a, b, c, d = (x0, 0.0, z0), (x0 + CELL, 0.0, z0), (x0 + CELL, 0.0, z0 + CELL), (x0, 0.0, z0 + CELL)
            quads += [a + c + b, a + d + c]                 # facing +y
            qm += [ALBEDO[(i + j) & 1] + (0.0,)] * 2
    n = len(quads)
    tv = np.concatenate([np.array(quads, np.float64), cube.reshape(-1, 9)])
    return tv, np.concatenate([np.array(qm, F), cube_mats]).astype(F), np.arange(n)


@functools.lru_cache(maxsize=None)
def checker_built():
    from rtamd import build_buffers
    tv, mats, part = checker_scene()
    return build_buffers(tv, mats, 1), tv, part


def moved_buffers(built, tv, part, offset):
    """built's buffers with the input triangles `part` translated by offset."""
    from rtamd import refit_buffers
    out = np.asarray(tv, np.float64).reshape(-1, 3, 3).copy()
    out[part] += np.asarray(offset, np.float64)
    return refit_buffers(built, out.reshape(-1, 9))


def guides(built, cam_bytes, w, h):
    """The first-hit records of a camera's frame-0 rays over built's buffers."""
    return Q.closest_hits(built.model_vertex_data, built.flat_bvh_data, Q.primary_rays(cam_bytes, w, h))[0].reshape(h, w)


def camera(w, h, orbit=0.0):
    """The default camera turned `orbit` degrees about the vertical axis through the origin."""
    from rtamd import configs
    a = np.radians(orbit)
    x, y, z = -25.0, 30.0, 140.0
    o = (x * np.cos(a) + z * np.sin(a), y, -x * np.sin(a) + z * np.cos(a))
    return configs.Camera(o, (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 20.0, float(w) / float(h))


def config2_pair(w, h, offset=(1.5, 0.25, -2.0), orbit=0.0):
    """Config 2 with the cube translated between two frames: (previous buffers,
    current buffers, previous camera bytes, current camera bytes)."""
    from rtamd import build_buffers
    tv, mats, seed, part, _ = R.scene("config2")
    built = build_buffers(tv, mats, seed)
    return built, moved_buffers(built, tv, part, offset), camera(w, h).ubo_bytes(), camera(w, h, orbit=orbit).ubo_bytes()


def frame_pair(prev, cur, prev_cam, cam, w, h, seed):
    """Guides of both states, a random radiance and a random history."""
    rng = np.random.default_rng(seed)
    rad = rng.uniform(0.0, 1.2, size=(h, w, 3)).astype(F)
    return rad, guides(cur, cam, w, h), guides(prev, prev_cam, w, h), random_history(h, w, rng)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, F).view(np.uint32), np.ascontiguousarray(b, F).view(np.uint32))


# ---- 1. identity ----------------------------------------------------------------

def test_unmoved_records_are_the_static_contract_on_rendered_guides():
    w, h = 48, 27
    for orbit in (0.0, 1.0):
        prev, _, prev_cam, cam = config2_pair(w, h, orbit=orbit)
        rad, hits, hits_prev, hist = frame_pair(prev, prev, prev_cam, cam, w, h, seed=3)
        assert (hits["tri"] >= 0).any() and (hits["tri"] < 0).any()
        v = prev.model_vertex_data
        want = T.temporal(rad, hits, cam, prev_cam, hist, hits_prev)
        got = M.temporal_motion(rad, hits, cam, prev_cam, hist, hits_prev, v, v.copy())
        assert want[3].any()
        for a, b in zip(got[:2], want[:2]):
            assert same_bits(a, b), orbit
        assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3]) and got[4] is None


@pytest.mark.parametrize("seed", [11, 12])
def test_unmoved_records_are_the_static_contract_on_synthetic_guides(seed):
    rng = np.random.default_rng(seed)
    H, W = 9, 13
    rad, hits = random_frame(H, W, seed=seed, nan_normals=3)
    _, hits_prev = random_frame(H, W, seed=seed + 100, nan_normals=3)
    same = rng.random((H, W)) < 0.6
    hits_prev["normal"][same] = hits["normal"][same]
    hits_prev["pos"][same] = hits["pos"][same] + rng.normal(size=(int(same.sum()), 3)).astype(F) * F(1e-3)
    hist, mom = random_history(H, W, rng), rng.uniform(0.0, 1.0, (H, W, 2)).astype(F)
    verts = rng.normal(size=(1000, 12)).astype(F)
    for (mh, tol, nmin), cams in zip(((32, 0.005, 0.9), (2, 50.0, -1.0)), (random_camera_pair(rng), None)):
        cam, prev_cam = cams if cams else (look_at((3.0, 4.0, 40.0)),) * 2      # a moving and a static camera
        want = V.temporal_moments(rad, hits, cam, prev_cam, hist, hits_prev, mom, mh, tol, nmin)
        got = M.temporal_motion(rad, hits, cam, prev_cam, hist, hits_prev, verts, verts.copy(), mom_prev=mom,
                                max_history=mh, plane_tol=tol, normal_min=nmin)
        for a, b in zip((got[0], got[1], got[4]), (want[0], want[1], want[4])):
            assert same_bits(a, b)
        assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])


# ---- 2. the scalar restatement ----------------------------------------------------

def scalar_motion(rad, hits, cam, prev_cam, hist_prev, hits_prev, vc, vp, n_tris, max_history, plane_tol, normal_min):
    """DESIGN.md §4m line by line, one scalar operation at a time: float32 [H, W, 4]."""
    from test_temporal_ref import scalar_basis
    H, W = rad.shape[:2]
    f64 = np.float64
    dot = lambda a, b: (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]    # noqa: E731
    cross = lambda p, q: [p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0]]  # noqa: E731
    cur, prev = scalar_basis(cam), scalar_basis(prev_cam)
    vc = np.asarray(vc, F).reshape(-1, 3, 4)
    vp = np.asarray(vp, F).reshape(-1, 3, 4)

    def project(Cb, P):
        o, n, A, B, det = Cb
        w = [P[k] - o[k] for k in range(3)]
        dn = dot(w, n)
        return dot(w, A) / dn, dot(w, B) / dn, bool(dn * det > 0)

    out = np.zeros((H, W, 4), F)
    with np.errstate(all="ignore"):
        for y in range(H):
            for x in range(W):
                c = [F(rad[y, x, k]) * F(rad[y, x, k]) for k in range(3)]
                hp = hits[y, x]
                tri = int(hp["tri"])
                if tri < 0:
                    out[y, x] = c + [F(0.0)]
                    continue
                out[y, x] = c + [F(1.0)]
                if tri >= n_tris:
                    continue
                nrm, pos = [F(v) for v in hp["normal"]], [F(v) for v in hp["pos"]]
                a, b = vc[tri, :, :3], vp[tri, :, :3]
                if a.tobytes() == b.tobytes():
                    Pq, nq = pos, nrm
                else:
                    e1, e2 = [F(a[1, k]) - F(a[0, k]) for k in range(3)], [F(a[2, k]) - F(a[0, k]) for k in range(3)]
                    g1, g2 = [F(b[1, k]) - F(b[0, k]) for k in range(3)], [F(b[2, k]) - F(b[0, k]) for k in range(3)]
                    e1, e2, g1, g2 = ([f64(v) for v in e] for e in (e1, e2, g1, g2))
                    w = [f64(pos[k]) - f64(a[0, k]) for k in range(3)]
                    d11, d12, d22, w1, w2 = dot(e1, e1), dot(e1, e2), dot(e2, e2), dot(w, e1), dot(w, e2)
                    den = d11 * d22 - d12 * d12
                    b1, b2 = (d22 * w1 - d12 * w2) / den, (d11 * w2 - d12 * w1) / den
                    Pq = [F((f64(b[0, k]) + b1 * g1[k]) + b2 * g2[k]) for k in range(3)]
                    m, mq = cross(e1, e2), cross(g1, g2)
                    s = f64(-1.0) if dot(m, [f64(v) for v in nrm]) < 0 else f64(1.0)
                    ln = np.sqrt(dot(mq, mq))
                    nq = [F((mq[k] / ln) * s) for k in range(3)]
                    if not all(np.isfinite(v) for v in Pq + nq):
                        continue
                uc, vcc, fc = project(cur, pos)
                up, vpp, fp = project(prev, Pq)
                fx = F(x) + (up - uc) * F(W)
                fy = F(y) + (vcc - vpp) * F(H)
                if not (fc and fp and fx > -1 and fx < F(W) and fy > -1 and fy < F(H)):
                    continue
                x0, y0 = np.floor(fx), np.floor(fy)
                ax, ay = fx - x0, fy - y0
                tol = F(plane_tol) * F(hp["t"])
                acc, ws, nm = [F(0.0)] * 3, F(0.0), F(np.inf)
                for j in (0, 1):
                    for i in (0, 1):
                        qx, qy = int(x0) + i, int(y0) + j
                        if qx < 0 or qx >= W or qy < 0 or qy >= H:
                            continue
                        wt = (ax if i else F(1.0) - ax) * (ay if j else F(1.0) - ay)
                        hq, rec = hits_prev[qy, qx], hist_prev[qy, qx]
                        if not (hq["tri"] >= 0 and rec[3] > 0 and wt > 0):
                            continue
                        if not dot(nq, [F(v) for v in hq["normal"]]) >= F(normal_min):
                            continue
                        if not abs(dot(nq, [F(hq["pos"][k]) - Pq[k] for k in range(3)])) <= tol:
                            continue
                        acc = [acc[k] + wt * F(rec[k]) for k in range(3)]
                        ws = ws + wt
                        nm = np.fmin(nm, F(rec[3]))
                if ws > 0:
                    ch = [acc[k] / ws for k in range(3)]
                    nn = np.fmin(nm + F(1.0), F(max_history))
                    inv = F(1.0) / nn
                    out[y, x] = [ch[k] + (c[k] - ch[k]) * inv for k in range(3)] + [nn]
    return out


def deformed_pairs(name, kind):
    """(previous buffers, current buffers) of every step of a deformation of a refit_ref scene, from rest."""
    from rtamd import build_buffers, refit_buffers
    tv, mats, seed, part, cam = R.scene(name)
    built = build_buffers(tv, mats, seed)
    states = [built] + [refit_buffers(built, s) for s in R.deform(kind, tv, part)]
    return list(zip(states[:-1], states[1:])), cam


@pytest.mark.parametrize("name,kind", [("config2", "translate"), ("random0", "jitter"), ("tris5", "squash"),
                                       ("random1", "squash")])
def test_scalar_restatement_agrees_bit_for_bit(name, kind):
    w, h = 48, 30
    pairs, cam = deformed_pairs(name, kind)
    from rtamd import configs
    cam = configs.Camera(cam.origin, cam.look_at, cam.v_up, cam.vfov, w / h).ubo_bytes()
    reused_any = moved_any = 0
    for step, (prev, cur) in enumerate(pairs):
        rad, hits, hits_prev, hist = frame_pair(prev, cur, cam, cam, w, h, seed=7 + step)
        vc, vp = cur.model_vertex_data, prev.model_vertex_data
        n = cur.triangle_count
        for mh, tol, nmin in ((32, 0.005, 0.9), (2, 50.0, -1.0)):
            want = scalar_motion(rad, hits, cam, cam, hist, hits_prev, vc, vp, n, mh, tol, nmin)
            got = M.temporal_motion(rad, hits, cam, cam, hist, hits_prev, vc, vp, max_history=mh, plane_tol=tol,
                                    normal_min=nmin)
            assert same_bits(got[0], want), (name, kind, step, mh)
            reused_any += int(got[3].sum())
        moved_any += int(M.previous_points(hits, vc, vp)[3].sum())
    assert moved_any > 20 and reused_any > 20               # the moved path and the gather were compared


# ---- 3. rigid translation -----------------------------------------------------------

# The largest |P' - (pos - d)| seen below is 16 spacings of the triangle's largest coordinate (DESIGN.md
# §4m); the bound asserted is twice that, rounded up to a power of two.  Most of it is the hit point's own
# distance from its triangle's plane (origin + t * direction in float, t near 150 where the triangle's
# coordinates are near 10), which the barycentric coordinates drop.
RIGID_BOUND = 32.0


def test_a_rigid_translation_is_followed():
    """V' = V - d exactly (vertices on a 2^-10 grid, d on it too): the hit point,
    which the oracle's walk places within rounding of the triangle's plane,
    moves by d to within a few spacings of the triangle's largest coordinate."""
    from rtamd import build_buffers, refit_buffers
    w, h = 48, 32
    d = np.array([1.5, 0.25, -2.0])
    worst = 0.0
    for name in ("config2", "random0", "random2", "tris5"):
        tv, mats, seed, part, cam = R.scene(name)
        tv = np.round(np.asarray(tv, np.float64) * 1024.0) / 1024.0
        built = build_buffers(tv, mats, seed)
        prev = refit_buffers(built, (tv.reshape(-1, 3, 3) - d).reshape(-1, 9))
        vc, vp = M.vertex_records(built.model_vertex_data), M.vertex_records(prev.model_vertex_data)
        assert np.array_equal(vc.astype(np.float64) - d, vp.astype(np.float64))
        hits = guides(built, cam.ubo_bytes(), w, h)
        P, _, valid, moved = M.previous_points(hits, built.model_vertex_data, prev.model_vertex_data)
        ok = (hits["tri"] >= 0) & valid
        assert ok.any() and moved[ok].all()
        tri = hits["tri"][ok]
        big = np.abs(np.concatenate([vc[tri], vp[tri]], 1)).max((1, 2))
        err = np.abs(P[ok].astype(np.float64) - (hits["pos"][ok].astype(np.float64) - d)).max(-1)
        worst = max(worst, float((err / np.spacing(big.astype(F)).astype(np.float64)).max()))
    print(f"rigid translation: largest |P' - (pos - d)| = {worst:.3f} spacings of the triangle's largest coordinate")
    assert worst <= RIGID_BOUND


# ---- 4. designed colours --------------------------------------------------------------

def top_down_camera(w, h, units_per_pixel=0.1, height=100.0):
    """Looks straight down at the origin from `height`, the plane y = 0 filling
    the frame at units_per_pixel: a slide of the checker by that much along x
    is a shift of one pixel."""
    vfov = 2.0 * np.degrees(np.arctan(0.5 * h * units_per_pixel / height))
    return look_at((0.0, height, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, -1.0), vfov, w / h)


def test_designed_colours_on_the_sliding_checker():
    """A bilinear gather mixes two coplanar cells wherever the reprojected point
    falls between pixels on either side of their edge: both taps pass the
    plane and the normal test.  So the camera is designed: straight down, 0.1
    units per pixel, and the slide of (0.1, 0, 0) is one pixel.  The
    reprojected point is then a pixel centre to within rounding, one tap
    carries all the weight but about 2^-17 (the float error of fx near 100),
    and nothing may be mixed; §4h's kernel reads the history one pixel off and
    mixes the albedos along every edge the slide crosses.

    The 2-spacing property is read along the sequence: a tap of the other
    albedo with weight 2^-17 leaves its pixel thousands of spacings (a few
    1e-6 of the albedos' distance) off, and a later pixel that gathers that
    record inherits it though its own taps all lie on its own albedo.  So a
    pixel counts as pure when its accepted taps lie on its own albedo and on
    records that were pure themselves; in the first reprojected frame that is
    the plain reading."""
    w, h, frames = 160, 90, 4
    built, tv, part = checker_built()
    cam = top_down_camera(w, h)
    mats = np.asarray(built.model_material_data, F).reshape(-1, 4)
    c_of = (np.array(ALBEDO, F) * np.array(ALBEDO, F)).astype(F)          # the linear colours c = g * g
    hist = {"motion": None, "naive": None}
    prev = prev_hits = None
    pure = np.ones((h, w), bool)
    for k in range(frames):
        cur = moved_buffers(built, tv, part, (0.1 * (k - (frames - 1)), 0.0, 0.0))
        hits = guides(cur, cam, w, h)
        rad = mats[np.maximum(hits["tri"], 0), :3].copy()                  # noise-free: the hit triangle's albedo
        rad[hits["tri"] < 0] = 0.5
        if k == 0:
            hist["motion"] = hist["naive"] = T.temporal(rad, hits)[0]
        else:
            taps = []
            got = M.temporal_motion(rad, hits, cam, cam, hist["motion"], prev_hits, cur.model_vertex_data,
                                    prev.model_vertex_data, taps=taps)
            naive = T.temporal(rad, hits, cam, cam, hist["naive"], prev_hits)
            hist["motion"], hist["naive"] = got[0], naive[0]
            on_checker = (hits["tri"] >= 0) & (mats[np.maximum(hits["tri"], 0), 3] == 0.0)
            which = (mats[np.maximum(hits["tri"], 0), 0] == F(ALBEDO[1][0])).astype(int)
            reused = got[3] & on_checker
            assert reused.sum() > 0.9 * on_checker.sum() and got[0][..., 3][reused].max() == k + 1
            own = reused.copy()                     # every accepted tap lies on a triangle of the pixel's albedo
            for take, qy, qx in taps:
                tq = np.maximum(prev_hits["tri"][qy, qx], 0)
                own &= ~take | ((mats[tq, 3] == 0.0) & (mats[tq, 0] == mats[np.maximum(hits["tri"], 0), 0]) &
                                pure[qy, qx])
            pure = ~got[3] | own
            assert own.sum() > 0.5 * reused.sum()
            want = c_of[which]
            assert (np.abs(got[0][..., :3] - want)[own] <= 2 * np.spacing(want)[own]).all()

            def blends(hc, mask):
                """Pixels of mask with a channel further than 1e-3 of the albedos' distance from both."""
                gap = np.abs(c_of[0] - c_of[1]) * F(1e-3)
                far = (np.abs(hc - c_of[0]) > gap) & (np.abs(hc - c_of[1]) > gap)
                return mask & far.any(-1)
            assert not blends(got[0][..., :3], reused).any(), k
            n_naive = int(blends(naive[0][..., :3], naive[3] & on_checker).sum())
            assert n_naive > 20, k                  # the scene discriminates: the unchanged kernel does mix them
        prev, prev_hits = cur, hits


# ---- 5. degenerates ---------------------------------------------------------------------

def test_degenerate_triangles_and_foreign_indices_start_over():
    H, W = 4, 6
    rng = np.random.default_rng(5)
    cam = look_at((3.0, 4.0, 40.0))
    hits = np.zeros((H, W), D.HIT_DTYPE)
    hits["normal"] = (0.0, 0.0, 1.0)
    hits["pos"] = rng.normal(size=(H, W, 3)).astype(F) * F(0.5)
    hits["pos"][..., 2] = 0.0
    hits["t"] = 40.0
    n_tris = 4
    tri_of_row = (0, 1, 2, n_tris)                        # unmoved, zero edge now, zero area before, foreign
    for y, t in enumerate(tri_of_row):
        hits["tri"][y] = t
    hits["tri"][3, 3:] = 1 << 30
    good = np.array([[-4, -4, 0, 1], [4, -4, 0, 1], [0, 4, 0, 1]], F)
    vc = np.stack([good, good, good, good]).copy()
    vp = vc.copy()
    vc[1, 1] = vc[1, 0]                                   # a current triangle with a zero edge
    vp[1] += F(0.25)
    vp[2, 2] = vp[2, 1] * F(2.0) - vp[2, 0]               # a previous triangle of zero area (collinear), moved
    vp[2, 2, 3] = 1.0
    rad = rng.uniform(0.1, 1.0, (H, W, 3)).astype(F)
    hist = random_history(H, W, rng)
    hist[..., 3] = 5.0
    mom = rng.uniform(0.0, 1.0, (H, W, 2)).astype(F)
    got = M.temporal_motion(rad, hits, cam, cam, hist, hits, vc, vp, n_tris=n_tris, mom_prev=mom)
    for out in (got[0], got[1], got[4]):
        assert np.isfinite(out).all()
    assert got[3][0].all() and (got[0][0, :, 3] == 6.0).all()              # the unmoved row reuses its history
    assert not got[3][1:].any()
    assert (got[0][1:, :, 3] == 1.0).all()
    assert same_bits(got[0][1:, :, :3], (rad * rad)[1:]) and same_bits(got[1][1:], rad[1:])


# ---- 6. moments ---------------------------------------------------------------------------

def test_the_moments_change_no_colour():
    w, h = 48, 27
    prev, cur, prev_cam, cam = config2_pair(w, h, orbit=1.0)
    rad, hits, hits_prev, hist = frame_pair(prev, cur, prev_cam, cam, w, h, seed=9)
    mom = np.random.default_rng(9).uniform(0.0, 1.0, (h, w, 2)).astype(F)
    args = (rad, hits, cam, prev_cam, hist, hits_prev, cur.model_vertex_data, prev.model_vertex_data)
    a, b = M.temporal_motion(*args), M.temporal_motion(*args, mom_prev=mom)
    assert a[4] is None and b[4] is not None and a[3].any()
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1]) and np.array_equal(a[2], b[2])
    moved = M.previous_points(hits, cur.model_vertex_data, prev.model_vertex_data)[3]
    assert (a[3] & moved).any()


# ---- 7. quality on the CPU oracle ------------------------------------------------------------

W_, H_, BOUNCES, FRAMES = 160, 90, 4, 8


def quality_camera():
    """Still, above the checker's corner: a cell spans about 7 pixels, the slide of 0.1 units about half a pixel."""
    from rtamd import configs
    return configs.Camera((-10.0, 16.0, 30.0), (0.0, 2.0, 0.0), (0.0, 1.0, 0.0), 30.0, W_ / H_)


def oracle_sample(built, cam, k):
    from oracle import oracle_lib
    cam.ubo.frame_count = k
    acc = np.zeros((H_, W_, 3), F)
    oracle_lib.render(built.model_vertex_data, built.model_material_data, built.flat_bvh_data, cam.ubo_bytes(), W_, H_,
                      BOUNCES, ext=oracle_lib.EXT_ACCUMULATE, accum=acc)
    cam.ubo.frame_count = 0
    return np.sqrt(acc)


def test_quality_on_the_oracle():
    """The sliding checker at (0.1, 0, 0) per frame, 8 frames ending at rest:
    the accumulated frame's mean squared radiance error against the 256-frame
    accumulation of the scene at rest, as a share of the raw last frame's
    (§4h's measure).  Below 0.25 on checker pixels (§4h's bound for Lambertian
    first hits, twice the ideal 1/8) and below §4h's kernel with kept history;
    at least 0.9 of the hit pixels reuse history; below 0.5 over the whole
    frame.  Measured shares: DESIGN.md §4m."""
    from oracle import oracle_lib
    built, tv, part = checker_built()
    cam = quality_camera()
    ubo = cam.ubo_bytes()
    mats = np.asarray(built.model_material_data, F).reshape(-1, 4)
    acc = np.zeros((H_, W_, 3), F)
    for f in range(256):
        cam.ubo.frame_count = f
        _, ref, _ = oracle_lib.render(built.model_vertex_data, built.model_material_data, built.flat_bvh_data,
                                      cam.ubo_bytes(), W_, H_, BOUNCES, ext=oracle_lib.EXT_ACCUMULATE, accum=acc)
    cam.ubo.frame_count = 0
    ref = ref.reshape(H_, W_, 3).astype(np.float64)
    hist = {"motion": None, "naive": None, "static": None}
    prev = prev_hits = None
    rest_hits = guides(built, ubo, W_, H_)
    for k in range(FRAMES):
        cur = moved_buffers(built, tv, part, (0.1 * (k - (FRAMES - 1)), 0.0, 0.0))
        raw, hits = oracle_sample(cur, cam, k), guides(cur, ubo, W_, H_)
        raw_static = oracle_sample(built, cam, k)
        if k == 0:
            hist["motion"] = hist["naive"] = T.temporal(raw, hits)
            hist["static"] = T.temporal(raw_static, rest_hits)
        else:
            hist["motion"] = M.temporal_motion(raw, hits, ubo, ubo, hist["motion"][0], prev_hits, cur.model_vertex_data,
                                               prev.model_vertex_data)
            hist["naive"] = T.temporal(raw, hits, ubo, ubo, hist["naive"][0], prev_hits)
            hist["static"] = T.temporal(raw_static, rest_hits, ubo, ubo, hist["static"][0], rest_hits)
        prev, prev_hits = cur, hits
    hit = hits["tri"] >= 0
    checker = hit & (mats[np.maximum(hits["tri"], 0), 3] == 0.0)
    cube = hit & ~checker
    s = {name: (share(v[1], raw if name != "static" else raw_static, ref),
                share(v[1], raw if name != "static" else raw_static, ref, checker),
                share(v[1], raw if name != "static" else raw_static, ref, cube)) for name, v in hist.items()}
    reuse = float(hist["motion"][3][hit].mean())
    n_checker = float(hist["motion"][0][..., 3][checker].mean())
    print(f"sliding checker (0.1, 0, 0) per frame, {FRAMES} frames: reuse {reuse:.4f}, mean history on the checker "
          f"{n_checker:.2f}; MSE share (whole frame, checker, cube): per-triangle {s['motion'][0]:.4f} {s['motion'][1]:.4f} "
          f"{s['motion'][2]:.4f}; kept history with the unchanged kernel {s['naive'][0]:.4f} {s['naive'][1]:.4f} "
          f"{s['naive'][2]:.4f}; static scene {s['static'][0]:.4f} {s['static'][1]:.4f} {s['static'][2]:.4f}")
    assert checker.sum() > 1000 and cube.any() and (~hit).any()
    assert s["motion"][1] < 0.25
    assert s["motion"][1] < s["naive"][1]
    assert reuse >= 0.9
    assert s["motion"][0] < 0.5
