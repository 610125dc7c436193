"""tests/albedo_ref.py (the numpy restatement the GPU albedo tests compare with)
pinned: its passes are denoise_ref's bit for bit, an all-ones albedo buffer
gives denoise_ref's filter, a scalar restatement of the record rule and of the
two new operations agrees bit for bit on every special albedo, and on the CPU
oracle's 1-sample frames the filter on the illumination does what DESIGN.md §4p
says: on the two-albedo checker it removes most of the error the colour filter
leaves, on flat albedo it changes nothing."""
import numpy as np
import pytest

import albedo_ref as A
import denoise_ref as D
from test_denoise_ref import oracle_frames, random_frame   # noqa: F401  (oracle_frames: a fixture)
from test_temporal_motion_ref import checker_built, guides, quality_camera

F = np.float32
U = np.uint32

# every special case of an albedo channel: 0, a denormal, just below / at / just above 2^-10 and 2^10, inf, NaN,
# negative, exactly 1 (and -0, -inf, the smallest normal)
SPECIAL = np.array([0.0, 1e-42, np.nextafter(F(2.0 ** -10), F(0)), 2.0 ** -10, np.nextafter(F(2.0 ** -10), F(1)),
                    np.nextafter(F(2.0 ** 10), F(0)), 2.0 ** 10, np.nextafter(F(2.0 ** 10), F(np.inf)), np.inf, np.nan,
                    -0.5, 1.0, -0.0, -np.inf, 1.17549435e-38], F)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, F).view(U), np.ascontiguousarray(b, F).view(U))


def special_materials(n, seed):
    """n material records whose albedo channels run through SPECIAL, the rest random in (0.05, 1)."""
    rng = np.random.default_rng(seed)
    mats = rng.uniform(0.05, 1.0, size=(n, 4)).astype(F)
    mats[:, 3] = rng.integers(0, 4, size=n)
    m = len(SPECIAL)
    assert n >= 2 * m
    mats[:m, :3] = SPECIAL[:, None]                     # material j carries SPECIAL[j] in all three channels
    mats[m:2 * m, 1] = SPECIAL                          # and the next m in one channel among ordinary ones
    return mats


def rendered_guides(w, h):
    """Config 2's first-hit records from its default camera, by query_ref."""
    from rtamd import configs
    built = configs.config2().build()
    return guides(built, configs.Camera.default(w, h).ubo_bytes(), w, h)


@pytest.mark.parametrize("iterations", [1, 2, 3, 4, 5, 6])
def test_the_passes_are_denoise_refs(iterations):
    rad, hits = random_frame(23, 37, seed=40 + iterations)
    frames = [(rad, hits)]
    if iterations in (1, 4, 6):
        g = rendered_guides(40, 24)
        assert (g["tri"] >= 0).any() and (g["tri"] < 0).any()
        frames.append((np.random.default_rng(iterations).uniform(0.0, 1.2, size=(24, 40, 3)).astype(F), g))
    for rad, hits in frames:
        for kw in ({}, {"normal_power_log2": 0, "sigma_depth": 50.0, "sigma_color": 4.0}):
            want = D.denoise_linear(rad, hits, iterations=iterations, **kw)
            assert same_bits(A.filter_linear(rad * rad, hits, iterations=iterations, **kw), want), (iterations, kw)


@pytest.mark.parametrize("iterations", [1, 4, 6])
def test_an_all_ones_buffer_is_the_colour_filter(iterations):
    rad, hits = random_frame(23, 37, seed=5)
    ones = np.ones((23, 37, 4), F)
    ones[..., 3] = np.nan                               # the fourth word is not read
    want_rad, want_rgba = D.denoise(rad, hits, iterations=iterations)
    got_rad, got_rgba = A.denoise_albedo(rad, hits, ones, iterations=iterations)
    assert same_bits(got_rad, want_rad) and np.array_equal(got_rgba, want_rgba)
    assert same_bits(A.denoise_albedo(rad, hits, ones[..., :3], iterations=iterations)[0], want_rad)


def scalar_divisor(a):
    a = F(a)
    if a >= F(2.0 ** -10) and a <= F(2.0 ** 10):        # a NaN fails both
        return a
    return F(1.0)


def scalar_albedo(hits, mats):
    H, W = hits.shape
    out = np.empty((H, W, 4), F)
    for y in range(H):
        for x in range(W):
            tri = int(hits[y, x]["tri"])
            if 0 <= tri < len(mats):
                out[y, x] = [scalar_divisor(mats[tri, k]) for k in range(3)] + [mats[tri, 3]]
            else:
                out[y, x] = (1.0, 1.0, 1.0, -1.0)
    return out


def scalar_denoise_albedo(rad, hits, alb, **kw):
    """The two new operations one np.float32 scalar at a time around the shared passes."""
    H, W = rad.shape[:2]
    i = np.empty((H, W, 3), F)
    with np.errstate(all="ignore"):
        for y in range(H):
            for x in range(W):
                for k in range(3):
                    c = F(rad[y, x, k]) * F(rad[y, x, k])
                    i[y, x, k] = c / F(alb[y, x, k])
        f = A.filter_linear(i, hits, **kw)
        out = np.empty((H, W, 3), F)
        for y in range(H):
            for x in range(W):
                for k in range(3):
                    out[y, x, k] = np.sqrt(F(f[y, x, k]) * F(alb[y, x, k]))
    return out


def test_scalar_restatement_on_every_special_albedo():
    n = 2 * len(SPECIAL) + 5
    mats = special_materials(n, seed=11)
    rad, hits = random_frame(13, 17, seed=12)
    hit = hits["tri"] >= 0
    hits["tri"][hit] = np.arange(int(hit.sum())) % (n + 3)          # every material, and three indices past them
    hits["tri"][0, 0], hits["tri"][0, 1], hits["tri"][0, 2] = n - 1, n, 1 << 29
    alb = A.albedo(hits, mats)
    assert same_bits(alb, scalar_albedo(hits, mats))
    # the rule itself, value by value
    d = A.divisor(SPECIAL)
    want = [1.0, 1.0, 1.0, 2.0 ** -10, float(SPECIAL[4]), float(SPECIAL[5]), 2.0 ** 10, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]
    assert same_bits(d, np.array(want, F))
    miss = ~((hits["tri"] >= 0) & (hits["tri"] < n))
    assert miss.any() and same_bits(alb[miss], np.broadcast_to(np.array([1, 1, 1, -1], F), alb[miss].shape))
    assert np.isfinite(alb[..., :3]).all() and (alb[..., :3] >= F(2.0 ** -10)).all() and (alb[..., :3] <= F(2.0 ** 10)).all()
    for kw in ({"iterations": 1}, {}, {"iterations": 3, "normal_power_log2": 0, "sigma_depth": 50.0}):
        got = A.denoise_albedo(rad, hits, alb, **kw)[0]
        assert same_bits(got, scalar_denoise_albedo(rad, hits, alb, **kw)), kw
        assert np.isfinite(got).all()
    # the filter reads the buffer as it stands: the raw special values too (IEEE: x / 0, x / inf, NaN)
    raw = np.ones((13, 17, 4), F)
    raw[..., :3].reshape(-1)[:3 * len(SPECIAL)] = np.repeat(SPECIAL, 3)
    got = A.denoise_albedo(rad, hits, raw, iterations=2)[0]
    assert same_bits(got, scalar_denoise_albedo(rad, hits, raw, iterations=2))


def test_sky_and_ones_keep_their_bits():
    rad, hits = random_frame(23, 37, seed=7)
    mats = special_materials(40, seed=8)
    hits["tri"][hits["tri"] >= 0] %= 40
    alb = A.albedo(hits, mats)
    out_rad, out_rgba = A.denoise_albedo(rad, hits, alb)
    miss = hits["tri"] < 0
    assert miss.any() and same_bits(out_rad[miss], rad[miss]) and np.array_equal(out_rgba[miss], D.unorm8(rad)[miss])
    assert (out_rad[~miss] != rad[~miss]).any()


# ---- quality on the oracle's frames ---------------------------

W_, H_, BOUNCES = 160, 90, 4


def mse(a, ref, mask=None):
    e = (np.asarray(a, np.float64) - ref) ** 2
    return float(e.mean() if mask is None else e[mask].mean())


def test_quality_on_the_checker():
    """The checker from quality_camera(), the oracle's sample 0 at 160 x 90 and 4
    bounces against its 256-frame accumulation, guides from query_ref.  On the
    Lambertian first hits (the floor) the filter on the illumination leaves less
    error than the colour filter and than the raw frame, and below half the
    colour filter's (measured 0.406); sky pixels keep their bits."""
    from oracle import oracle_lib
    built, _, _ = checker_built()
    cam = quality_camera()
    acc = np.zeros((H_, W_, 3), F)
    raw = None
    for f in range(256):
        cam.ubo.frame_count = f
        _, ref, _ = oracle_lib.render(built.model_vertex_data, built.model_material_data, built.flat_bvh_data,
                                      cam.ubo_bytes(), W_, H_, BOUNCES, ext=oracle_lib.EXT_ACCUMULATE, accum=acc)
        if f == 0:
            raw = ref.reshape(H_, W_, 3).copy()
    cam.ubo.frame_count = 0
    ref = ref.reshape(H_, W_, 3).astype(np.float64)
    hits = guides(built, cam.ubo_bytes(), W_, H_)
    mats = np.asarray(built.model_material_data, F).reshape(-1, 4)
    alb = A.albedo(hits, mats)
    shipped = D.denoise(raw, hits)[0]
    out = A.denoise_albedo(raw, hits, alb)[0]
    hit = hits["tri"] >= 0
    floor = hit & (alb[..., 3] == 0.0)
    assert floor.sum() > 1000 and (hit & ~floor).any() and (~hit).any()
    assert same_bits(out[~hit], raw[~hit])
    whole = (mse(raw, ref), mse(shipped, ref), mse(out, ref))
    lam = (mse(raw, ref, floor), mse(shipped, ref, floor), mse(out, ref, floor))
    print(f"checker, sample 0: whole frame raw {whole[0]:.4g}, colour filter {whole[1]:.4g}, on illumination "
          f"{whole[2]:.4g} (share of the colour filter's {whole[2] / whole[1]:.4f}); Lambertian first hits "
          f"({int(floor.sum())} px) raw {lam[0]:.4g}, colour filter {lam[1]:.4g}, on illumination {lam[2]:.4g} "
          f"(share {lam[2] / lam[1]:.4f}, of raw {lam[2] / lam[0]:.4f})")
    assert lam[2] < lam[1] and lam[2] < lam[0]
    assert lam[2] / lam[1] < 0.5


def test_quality_on_flat_albedo(oracle_frames):   # noqa: F811
    """Config 2 (one albedo per object) from (-25, 30, 140): the whole frame's
    error is at most 1.02 of the colour filter's (measured 1.003)."""
    from rtamd import configs
    raw, ref, hits = oracle_frames
    ref = ref.astype(np.float64)
    mats = np.asarray(configs.config2().build().model_material_data, F).reshape(-1, 4)
    alb = A.albedo(hits, mats)
    shipped = D.denoise(raw, hits)[0]
    out = A.denoise_albedo(raw, hits, alb)[0]
    sky = hits["tri"] < 0
    assert sky.any() and same_bits(out[sky], raw[sky])
    lam = (hits["tri"] >= 0) & (alb[..., 3] == 0.0)
    a, b = mse(shipped, ref), mse(out, ref)
    print(f"config 2, sample 0: whole frame raw {mse(raw, ref):.4g}, colour filter {a:.4g}, on illumination {b:.4g} "
          f"(share {b / a:.4f}); Lambertian first hits colour filter {mse(shipped, ref, lam):.4g}, on illumination "
          f"{mse(out, ref, lam):.4g}")
    assert b <= 1.02 * a
