"""tests/denoise_ref.py (the numpy filter the GPU denoise tests compare with)
pinned from a second side: a scalar restatement of DESIGN.md §4g's contract,
one Python loop per pixel and tap in np.float32 scalars, agrees with it bit for
bit; sky pixels pass through, silhouettes do not mix, NaN guides pass through,
and on the CPU oracle's 1-sample frame it removes most of the error."""
import numpy as np
import pytest

import denoise_ref as D

F = np.float32


def scalar_denoise_linear(radiance, hits, iterations, normal_power_log2, sigma_depth, sigma_color):
    """DESIGN.md §4g line by line, one np.float32 operation at a time."""
    H, W = radiance.shape[:2]
    h = (F(3.0 / 8.0), F(1.0 / 4.0), F(1.0 / 16.0))
    c = [[[F(radiance[y, x, k]) * F(radiance[y, x, k]) for k in range(3)] for x in range(W)] for y in range(H)]
    isc = F(1.0) / F(sigma_color)
    with np.errstate(all="ignore"):
        for i in range(iterations):
            s = 1 << i
            isc_i = isc * F(s)
            lum = [[(F(0.2126) * c[y][x][0] + F(0.7152) * c[y][x][1]) + F(0.0722) * c[y][x][2] for x in range(W)]
                   for y in range(H)]
            out = [[None] * W for _ in range(H)]
            for py in range(H):
                for px in range(W):
                    hp = hits[py, px]
                    if hp["tri"] < 0:
                        out[py][px] = list(c[py][px])
                        continue
                    n_p = [F(v) for v in hp["normal"]]
                    pos_p = [F(v) for v in hp["pos"]]
                    kz = F(1.0) / (F(sigma_depth) * F(hp["t"]))
                    acc = [F(0.0), F(0.0), F(0.0)]
                    wsum = F(0.0)
                    for dy in range(-2, 3):
                        for dx in range(-2, 3):
                            qx, qy = px + dx * s, py + dy * s
                            if qx < 0 or qx >= W or qy < 0 or qy >= H or hits[qy, qx]["tri"] < 0:
                                continue
                            n_q = [F(v) for v in hits[qy, qx]["normal"]]
                            nd = np.fmax(F(0.0), (n_p[0] * n_q[0] + n_p[1] * n_q[1]) + n_p[2] * n_q[2])
                            for _ in range(normal_power_log2):
                                nd = nd * nd
                            e = [F(hits[qy, qx]["pos"][k]) - pos_p[k] for k in range(3)]
                            d = abs((n_p[0] * e[0] + n_p[1] * e[1]) + n_p[2] * e[2])
                            x = d * kz
                            y = abs(lum[py][px] - lum[qy][qx]) * isc_i
                            w = ((h[abs(dx)] * h[abs(dy)]) * nd) / ((F(1.0) + x * x) * (F(1.0) + y * y))
                            for k in range(3):
                                acc[k] = acc[k] + w * c[qy][qx][k]
                            wsum = wsum + w
                    out[py][px] = [acc[k] / wsum for k in range(3)] if wsum > 0 else list(c[py][px])
            c = out
    return np.array(c, dtype=F)


def random_frame(H, W, seed, nan_normals=3):
    """Random guides: unit-ish normals, positions, t in (1e-3, 1e4), a third of
    the pixels without a hit (tri -1 or -2), a few NaN normals, finite radiance."""
    rng = np.random.default_rng(seed)
    hits = np.zeros((H, W), D.HIT_DTYPE)
    n = rng.normal(size=(H, W, 3))
    # a few shared directions, so that many taps have aligned normals and real weights
    base = rng.normal(size=(4, 3))
    pick = rng.integers(0, 4, size=(H, W))
    n = base[pick] + 0.05 * n
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    hits["normal"] = n.astype(F)
    hits["pos"] = (rng.normal(size=(H, W, 3)) * 3.0).astype(F)
    hits["t"] = np.exp(rng.uniform(np.log(1e-3), np.log(1e4), size=(H, W))).astype(F)
    hits["tri"] = rng.integers(0, 1000, size=(H, W))
    miss = rng.random((H, W)) < 1.0 / 3.0
    hits["tri"][miss] = rng.choice([-1, -2], size=int(miss.sum()))
    ok = np.argwhere(~miss)
    for k in rng.choice(len(ok), size=min(nan_normals, len(ok)), replace=False):
        y, x = ok[k]
        hits["normal"][y, x, rng.integers(0, 3)] = np.nan
    rad = rng.uniform(0.0, 1.2, size=(H, W, 3)).astype(F)
    return rad, hits


@pytest.mark.parametrize("iterations", [1, 3, 6])
def test_scalar_restatement_agrees_bit_for_bit(iterations):
    rad, hits = random_frame(9, 13, seed=100 + iterations)
    for npow, sd, sc in ((7, 0.005, 0.5), (0, 3.0, 0.25), (2, 50.0, 4.0)):
        want = scalar_denoise_linear(rad, hits, iterations, npow, sd, sc)
        got = D.denoise_linear(rad, hits, iterations, npow, sd, sc)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (iterations, npow)
    # the filter did something: wide depth sigma, some hit pixel changed
    assert (D.denoise_linear(rad, hits, iterations, 0, 50.0, 4.0) != rad * rad).any()


def test_pixels_without_a_hit_pass_through():
    rad, hits = random_frame(23, 37, seed=7)
    out_rad, out_rgba = D.denoise(rad, hits)
    miss = hits["tri"] < 0
    assert miss.any() and (~miss).any()
    assert np.array_equal(out_rad[miss].view(np.uint32), rad[miss].view(np.uint32))   # sqrt(g * g) == g
    assert np.array_equal(out_rgba[miss], D.unorm8(rad)[miss])
    assert (out_rgba[..., 3] == 255).all()


def test_silhouettes_do_not_mix():
    """Two half-frames with perpendicular normals and different constant
    colours: max(0, n_p . n_q) is 0 across the edge, so every weight there is
    0 and a pixel averages its own side's constant colour.  At most 25 terms and
    one division, each within 2^-24 relative: 32 ulp covers it."""
    H, W = 20, 33
    hits = np.zeros((H, W), D.HIT_DTYPE)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    left = xs < 16
    hits["tri"] = 1
    hits["t"] = 10.0
    hits["normal"][left] = (0.0, 0.0, 1.0)
    hits["normal"][~left] = (1.0, 0.0, 0.0)
    hits["pos"][..., 0] = np.where(left, xs * 0.1, 1.6)
    hits["pos"][..., 1] = ys * 0.1
    hits["pos"][..., 2] = np.where(left, 0.0, (xs - 16) * 0.1)
    rad = np.zeros((H, W, 3), F)
    rad[left] = (0.9, 0.3, 0.1)
    rad[~left] = (0.2, 0.6, 0.8)
    for iterations in (1, 4, 6):
        lin = D.denoise_linear(rad, hits, iterations=iterations)
        want = rad * rad
        ulp = np.abs(lin.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
        print(f"silhouette, {iterations} passes: max {ulp.max()} ulp")
        assert ulp.max() <= 32, iterations


def test_nan_normal_passes_through():
    rad, hits = random_frame(11, 17, seed=3, nan_normals=0)
    hits["tri"] = np.abs(hits["tri"])                       # every pixel has a hit
    hits["normal"][5, 8, 1] = np.nan
    hits["normal"][0, 0] = np.nan
    lin = D.denoise_linear(rad, hits)
    sq = rad * rad
    for y, x in ((5, 8), (0, 0)):
        assert np.array_equal(lin[y, x].view(np.uint32), sq[y, x].view(np.uint32))
    assert np.isfinite(lin).all()                            # a NaN neighbour has weight 0, it spreads nowhere


@pytest.fixture(scope="module")
def oracle_frames():
    """Config 2 at 160x90, 4 bounces: the C oracle's frame 0, its 256-frame
    accumulation (extension 4) and the first-hit records of frame 0's rays."""
    import query_ref as Q
    from oracle import oracle_lib
    from rtamd import configs
    built = configs.config2().build()
    w, h, bounces = 160, 90, 4
    cam = configs.Camera.default(w, h)
    acc = np.zeros((h, w, 3), F)
    first = None
    for f in range(256):
        cam.ubo.frame_count = f
        _, rad, _ = oracle_lib.render(built.model_vertex_data, built.model_material_data, built.flat_bvh_data,
                                      cam.ubo_bytes(), w, h, bounces, ext=oracle_lib.EXT_ACCUMULATE, accum=acc)
        if f == 0:
            first = rad.copy()
    cam.ubo.frame_count = 0
    rays = Q.primary_rays(cam.ubo_bytes(), w, h)
    hits = Q.closest_hits(built.model_vertex_data, built.flat_bvh_data, rays)[0].reshape(h, w)
    return first.reshape(h, w, 3), rad.reshape(h, w, 3), hits


def test_quality_on_the_oracle(oracle_frames):
    """The filtered 1-sample frame's mean squared error against the 256-frame
    accumulation is below half the raw frame's (measured share: DESIGN.md §4g)."""
    raw, ref, hits = oracle_frames
    out, _ = D.denoise(raw, hits)
    sky = hits["tri"] < 0
    assert sky.any() and np.array_equal(out[sky].view(np.uint32), raw[sky].view(np.uint32))
    mse_raw = float(np.mean((raw.astype(np.float64) - ref) ** 2))
    mse_out = float(np.mean((out.astype(np.float64) - ref) ** 2))
    lin_raw = float(np.mean((raw.astype(np.float64) ** 2 - ref.astype(np.float64) ** 2) ** 2))
    lin_out = float(np.mean((out.astype(np.float64) ** 2 - ref.astype(np.float64) ** 2) ** 2))
    print(f"MSE of the radiance: raw {mse_raw:.6g}, filtered {mse_out:.6g}, share {mse_out / mse_raw:.4f}; "
          f"of the linear colour: share {lin_out / lin_raw:.4f}")
    assert mse_raw > 0
    assert mse_out < 0.5 * mse_raw
