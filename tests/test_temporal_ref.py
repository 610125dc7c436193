"""tests/temporal_ref.py (the numpy accumulation the GPU temporal tests compare
with) pinned from a second side: a scalar restatement of DESIGN.md §4h's
contract, one Python loop per pixel and tap in np.float32 scalars, agrees with
it bit for bit; rt_temporal_camera_basis (host code) equals camera_basis; an
unmoved camera returns the fed frame, K frames give the mean, a camera turned
away reuses nothing, pixels without a hit pass through; and on the CPU oracle's
frames of an orbiting camera it removes most of a 1-sample frame's error while
reusing nearly every hit pixel's history."""
import ctypes as C

import numpy as np
import pytest

import denoise_ref as D
import temporal_ref as T
from test_denoise_ref import random_frame

F = np.float32


def look_at(origin, target=(0.0, 0.0, 0.0), vup=(0.0, 1.0, 0.0), vfov=20.0, aspect=13.0 / 9.0) -> bytes:
    """80 camera UBO bytes of a look-at camera (numpy, in double, stored as floats:
    any floats are a valid input of the contract)."""
    o, t, up = (np.asarray(v, np.float64) for v in (origin, target, vup))
    hh = np.tan(np.radians(vfov) / 2.0)
    hw = aspect * hh
    w = (o - t) / np.linalg.norm(o - t)
    u = np.cross(up, w)
    u /= np.linalg.norm(u)
    v = np.cross(w, u)
    ubo = np.zeros(20, F)
    ubo[0:3] = o
    ubo[4:7] = o - hw * u - hh * v - w
    ubo[8:11] = 2.0 * hw * u
    ubo[12:15] = 2.0 * hh * v
    return ubo.tobytes()


def random_camera_pair(rng):
    """Two cameras a small step apart, both looking at the guides' cloud around the origin."""
    o = rng.normal(size=3)
    o = o / np.linalg.norm(o) * rng.uniform(30.0, 60.0)
    step = rng.normal(size=3) * rng.uniform(0.0, 0.6)
    roll = rng.normal(size=3) * 0.05
    return (look_at(o, rng.normal(size=3) * 0.3, (0.0, 1.0, 0.0)),
            look_at(o + step, rng.normal(size=3) * 0.3, np.array([0.0, 1.0, 0.0]) + roll))


def random_history(H, W, rng):
    hist = np.zeros((H, W, 4), F)
    hist[..., :3] = rng.uniform(0.0, 1.5, size=(H, W, 3))
    hist[..., 3] = rng.integers(1, 40, size=(H, W))
    hist[rng.random((H, W)) < 1.0 / 3.0, 3] = 0.0           # a third of the records hold no sample
    return hist


def scalar_basis(ubo: bytes):
    f = np.frombuffer(ubo, F)
    o, ll, h, v = ([F(x) for x in f[k:k + 3]] for k in (0, 4, 8, 12))
    a = [ll[k] - o[k] for k in range(3)]
    cross = lambda p, q: [p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0]]  # noqa: E731
    n = cross(h, v)
    return o, n, cross(v, a), cross(a, h), (a[0] * n[0] + a[1] * n[1]) + a[2] * n[2]


def scalar_temporal(rad, hits, cam, prev_cam, hist_prev, hits_prev, max_history, plane_tol, normal_min):
    """DESIGN.md §4h line by line, one np.float32 operation at a time: float32 [H, W, 4]."""
    H, W = rad.shape[:2]
    dot = lambda a, b: (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]   # noqa: E731
    cur, prev = scalar_basis(cam), scalar_basis(prev_cam)

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
                if hp["tri"] < 0:
                    out[y, x] = c + [F(0.0)]
                    continue
                out[y, x] = c + [F(1.0)]
                n_p, pos = [F(v) for v in hp["normal"]], [F(v) for v in hp["pos"]]
                uc, vc, fc = project(cur, pos)
                up, vp, fp = project(prev, pos)
                fx = F(x) + (up - uc) * F(W)
                fy = F(y) + (vc - vp) * F(H)
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
                        if not dot(n_p, [F(v) for v in hq["normal"]]) >= F(normal_min):
                            continue
                        if not abs(dot(n_p, [F(hq["pos"][k]) - pos[k] for k in range(3)])) <= tol:
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


PARAMS = ((32, 0.005, 0.9), (2, 50.0, -1.0), (1024, 0.5, 0.0))


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_scalar_restatement_agrees_bit_for_bit(seed):
    rng = np.random.default_rng(seed)
    H, W = 9, 13
    rad, hits = random_frame(H, W, seed=seed, nan_normals=3)
    _, hits_prev = random_frame(H, W, seed=seed + 100, nan_normals=3)
    # the previous frame saw mostly the same surfaces: a real share of the taps passes the tests
    same = rng.random((H, W)) < 0.6
    hits_prev["normal"][same] = hits["normal"][same]
    hits_prev["pos"][same] = hits["pos"][same] + rng.normal(size=(int(same.sum()), 3)).astype(F) * F(1e-3)
    hist = random_history(H, W, rng)
    reused_any = 0
    for mh, tol, nmin in PARAMS:
        cam, prev = random_camera_pair(rng)
        want = scalar_temporal(rad, hits, cam, prev, hist, hits_prev, mh, tol, nmin)
        got, got_rad, got_rgba, reused = T.temporal(rad, hits, cam, prev, hist, hits_prev, mh, tol, nmin)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (seed, mh)
        assert np.array_equal(got_rgba, D.unorm8(got_rad)) and (got_rgba[..., 3] == 255).all()
        reused_any += int(reused.sum())
    assert reused_any > 20                                  # the gather path was compared, not only the fallbacks
    # no history: every hit pixel starts from its own sample
    first = T.temporal(rad, hits)[0]
    assert np.array_equal(first[..., :3].view(np.uint32), (rad * rad).view(np.uint32))
    assert np.array_equal(first[..., 3], np.where(hits["tri"] >= 0, 1.0, 0.0))


def test_camera_basis_equals_the_library():
    """rt_temporal_camera_basis is pure host code: no GPU needed."""
    import rtamd
    from rtamd import configs
    rng = np.random.default_rng(5)
    cams = [configs.Camera.default(160, 90).ubo_bytes()] + [c for _ in range(20) for c in random_camera_pair(rng)]
    for ubo in cams:
        out = (C.c_float * 13)()
        assert rtamd.lib().rt_temporal_camera_basis(C.byref(rtamd.CameraUBO.from_buffer_copy(ubo)), out) == 0
        assert np.array_equal(np.array(out[:], F).view(np.uint32), T.camera_basis(ubo).view(np.uint32))
    assert rtamd.lib().rt_temporal_camera_basis(None, (C.c_float * 13)()) == -1
    q = rtamd.TemporalParams(1, 1.0, 0.0)
    rtamd.lib().rt_temporal_default_params(C.byref(q))
    assert (q.max_history, q.plane_tol, q.normal_min, q.reserved) == (32, F(0.005), F(0.9), 0)
    assert (rtamd.TemporalParams().max_history, rtamd.TemporalParams().plane_tol) == (32, F(0.005))


def front_frame(H, W, seed):
    """random_frame with the guides' cloud wholly in front of a camera 40 units away."""
    rad, hits = random_frame(H, W, seed=seed, nan_normals=2)
    return rad, hits, look_at((3.0, 4.0, 40.0))


def test_an_unmoved_camera_returns_the_fed_frame():
    rad, hits, cam = front_frame(11, 17, seed=21)
    first, rad1, rgba1, reused1 = T.temporal(rad, hits, cam)
    hist, rad2, rgba2, reused = T.temporal(rad, hits, cam, cam, first, hits)
    ok = (hits["tri"] >= 0) & np.isfinite(hits["normal"]).all(-1)
    assert not reused1.any() and np.array_equal(reused, ok) and ok.any() and not ok.all()
    assert np.array_equal(hist[..., :3].view(np.uint32), (rad * rad).view(np.uint32))
    assert np.array_equal(hist[..., 3], np.where(ok, 2.0, first[..., 3]))
    assert np.array_equal(rad2.view(np.uint32), rad.view(np.uint32)) and np.array_equal(rgba2, rgba1)   # sqrt(g * g) == g


@pytest.mark.parametrize("max_history", [8, 32])
def test_a_static_camera_accumulates_the_mean(max_history):
    """After K frames c is within K * 4 ulp of the float64 mean of the K linear colours."""
    K = 8
    _, hits, cam = front_frame(11, 17, seed=22)
    rng = np.random.default_rng(22)
    frames = [rng.uniform(0.05, 1.2, size=(11, 17, 3)).astype(F) for _ in range(K)]
    hist = None
    for g in frames:
        hist = T.temporal(g, hits, cam, cam if hist is not None else None, hist, hits if hist is not None else None,
                          max_history=max_history)[0]
    ok = (hits["tri"] >= 0) & np.isfinite(hits["normal"]).all(-1)
    assert (hist[..., 3][ok] == K).all()
    mean = np.mean([(g * g).astype(np.float64) for g in frames], axis=0)
    err = np.abs(hist[..., :3].astype(np.float64) - mean)[ok]
    ulp = np.spacing(mean.astype(F)).astype(np.float64)[ok]
    print(f"static camera, {K} frames: max error {float((err / ulp).max()):.2f} ulp of the mean")
    assert (err <= K * 4 * ulp).all()


def test_a_camera_turned_away_reuses_nothing():
    rad, hits, cam = front_frame(11, 17, seed=23)
    first = T.temporal(rad, hits, cam)[0]
    away = look_at((3.0, 4.0, 40.0), target=(6.0, 8.0, 80.0))        # the same origin, turned 180 degrees
    rad2, _ = random_frame(11, 17, seed=24)
    hist, out_rad, _, reused = T.temporal(rad2, hits, cam, away, first, hits)
    assert not reused.any()
    assert np.array_equal(hist[..., :3].view(np.uint32), (rad2 * rad2).view(np.uint32))
    assert np.array_equal(hist[..., 3], np.where(hits["tri"] >= 0, 1.0, 0.0))
    assert np.array_equal(out_rad.view(np.uint32), rad2.view(np.uint32))


def test_pixels_without_a_hit_pass_through():
    rad, hits, cam = front_frame(23, 37, seed=25)
    first = T.temporal(rad, hits, cam)[0]
    rad2, _ = random_frame(23, 37, seed=26)
    hist, out_rad, rgba, reused = T.temporal(rad2, hits, cam, cam, first, hits)
    miss = hits["tri"] < 0
    assert miss.any() and reused.any() and not reused[miss].any()
    assert (hist[..., 3][miss] == 0).all()
    assert np.array_equal(hist[..., :3][miss].view(np.uint32), (rad2 * rad2)[miss].view(np.uint32))
    assert np.array_equal(out_rad[miss].view(np.uint32), rad2[miss].view(np.uint32))
    assert np.array_equal(rgba[miss], D.unorm8(rad2)[miss])


def test_max_history_1_is_the_identity():
    """max_history 1: nn = 1 and inv = 1, so out = ch + (c - ch).  n is 1 exactly
    and the history has no weight; c itself comes back through two roundings,
    of c - ch and of the sum: |out - c| <= 2^-24 (|c - ch| + |out|), below two
    spacings of max(c, ch) for the non-negative colours (bit for bit whenever
    ch / 2 <= c <= 2 ch, where the subtraction is exact)."""
    rad, hits, cam = front_frame(11, 17, seed=27)
    first = T.temporal(rad, hits, cam)[0]
    rad2, _ = random_frame(11, 17, seed=28)
    hist, _, _, reused = T.temporal(rad2, hits, cam, cam, first, hits, max_history=1)
    assert reused.any()
    assert np.array_equal(hist[..., 3], np.where(hits["tri"] >= 0, 1.0, 0.0))
    c, ch = (rad2 * rad2).astype(F), first[..., :3]          # an unmoved camera: ch is the pixel's own record
    assert (np.abs(hist[..., :3] - c) <= 2 * np.spacing(np.maximum(c, ch)))[reused].all()
    exact = reused[..., None] & (c >= ch / 2) & (c <= 2 * ch)
    assert exact.any() and np.array_equal(hist[..., :3][exact].view(np.uint32), c[exact].view(np.uint32))
    assert np.array_equal(hist[..., :3][~reused].view(np.uint32), c[~reused].view(np.uint32))


# ---- quality on the CPU oracle ------------------------------------------------

W_, H_, BOUNCES, FRAMES = 160, 90, 4, 8


def orbit_camera(deg: float):
    """The default camera turned deg degrees about the vertical axis through the origin."""
    from rtamd import configs
    cam = configs.Camera.default(W_, H_)
    a = np.radians(deg)
    x, y, z = cam.origin
    cam.set_origin((x * np.cos(a) + z * np.sin(a), y, -x * np.sin(a) + z * np.cos(a)))
    return cam


@pytest.fixture(scope="module")
def oracle():
    """Config 2 at 160x90, 4 bounces, from the C oracle: sample(cam, k) = the
    radiance of frame k's sample (extension 4 with a zeroed sum leaves the
    sample's linear colour in it), guides(cam) = the first-hit records of the
    camera's frame-0 rays, and the 256-frame accumulation at the default camera."""
    import query_ref as Q
    from oracle import oracle_lib
    from rtamd import configs
    built = configs.config2().build()
    scene = (built.model_vertex_data, built.model_material_data, built.flat_bvh_data)

    def sample(cam, k):
        cam.ubo.frame_count = k
        acc = np.zeros((H_, W_, 3), F)
        oracle_lib.render(*scene, cam.ubo_bytes(), W_, H_, BOUNCES, ext=oracle_lib.EXT_ACCUMULATE, accum=acc)
        cam.ubo.frame_count = 0
        return np.sqrt(acc)

    def guides(cam):
        cam.ubo.frame_count = 0
        rays = Q.primary_rays(cam.ubo_bytes(), W_, H_)
        return Q.closest_hits(built.model_vertex_data, built.flat_bvh_data, rays)[0].reshape(H_, W_)

    cam = orbit_camera(0.0)
    acc = np.zeros((H_, W_, 3), F)
    for f in range(256):
        cam.ubo.frame_count = f
        _, ref, _ = oracle_lib.render(*scene, cam.ubo_bytes(), W_, H_, BOUNCES, ext=oracle_lib.EXT_ACCUMULATE, accum=acc)
    mats = np.asarray(built.model_material_data, F).reshape(-1, 4)
    return dict(sample=sample, guides=guides, ref=ref.reshape(H_, W_, 3).astype(np.float64), mat_type=mats[:, 3])


def run_sequence(oracle, step_deg):
    """FRAMES frames of a camera that ends at the default camera: (raw last frame,
    temporal radiance, reused mask, last hit records)."""
    hist = prev_cam = prev_hits = None
    for k in range(FRAMES):
        cam = orbit_camera(-step_deg * (FRAMES - 1 - k))
        raw, hits = oracle["sample"](cam, k), oracle["guides"](cam)
        ubo = cam.ubo_bytes()
        hist, rad, _, reused = T.temporal(raw, hits, ubo, prev_cam, hist, prev_hits)
        prev_cam, prev_hits = ubo, hits
    return raw, rad, reused, hits


def share(x, raw, ref, mask=None):
    m = np.ones(ref.shape[:2], bool) if mask is None else mask
    return float(np.mean((x.astype(np.float64) - ref)[m] ** 2) / np.mean((raw.astype(np.float64) - ref)[m] ** 2))


@pytest.mark.parametrize("step_deg", [1.0, 0.0])
def test_quality_on_the_oracle(oracle, step_deg):
    """The accumulated frame's mean squared radiance error against the 256-frame
    accumulation, as a share of the raw last frame's: below 0.5 over the whole
    frame, for the orbiting camera below 0.25 on Lambertian first hits (1/8 is
    the ideal of 8 samples; the factor 2 is for rejected pixels and resampling),
    with at least 0.9 of the hit pixels reusing history.  Measured shares:
    DESIGN.md §4h."""
    raw, rad, reused, hits = run_sequence(oracle, step_deg)
    ref = oracle["ref"]
    hit = hits["tri"] >= 0
    lamb = hit & (oracle["mat_type"][np.maximum(hits["tri"], 0)] == 0.0)
    metal = hit & (oracle["mat_type"][np.maximum(hits["tri"], 0)] == 1.0)
    reuse = float(reused[hit].mean())
    whole, on_lamb = share(rad, raw, ref), share(rad, raw, ref, lamb)
    t2 = D.denoise(rad, hits, iterations=2)[0]
    t4 = D.denoise(rad, hits)[0]
    alone = D.denoise(raw, hits)[0]
    print(f"{step_deg} deg/frame, {FRAMES} frames: reuse {reuse:.4f}; MSE share temporal {whole:.4f} "
          f"(Lambertian {on_lamb:.4f}, metal {share(rad, raw, ref, metal):.4f}, sky {share(rad, raw, ref, ~hit):.4f}), "
          f"temporal + 2-pass filter {share(t2, raw, ref):.4f} (Lambertian {share(t2, raw, ref, lamb):.4f}), "
          f"temporal + 4-pass filter {share(t4, raw, ref):.4f} (Lambertian {share(t4, raw, ref, lamb):.4f}), "
          f"filter alone {share(alone, raw, ref):.4f} (metal {share(alone, raw, ref, metal):.4f})")
    assert lamb.any() and (~hit).any()
    assert reuse >= 0.9
    assert whole < 0.5
    if step_deg:
        assert on_lamb < 0.25
