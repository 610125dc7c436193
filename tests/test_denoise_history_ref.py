"""tests/denoise_history_ref.py (the numpy filter the GPU tests of
rt_denoise_history_device compare with) pinned from a second side: a scalar
restatement of DESIGN.md §4i's contract, one Python loop per pixel and tap in
np.float32 scalars, agrees with it bit for bit; with one sample everywhere it
is §4g's filter, with 2^iterations samples everywhere it is the identity;
pixels that are not live pass through; a pixel with 2^j samples is filtered in
exactly max(0, iterations - j) passes; and on the CPU oracle's 8-frame
accumulations it beats both fixed filters and, for a static camera, the
accumulation alone."""
import numpy as np
import pytest

import denoise_history_ref as A
import denoise_ref as D
import temporal_ref as T
import test_temporal_ref as TT
from test_denoise_ref import random_frame
from test_temporal_ref import oracle, run_sequence, share  # noqa: F401  (oracle is a fixture)

F = np.float32
N_SET = (0, 1, 2, 3, 4, 7, 8, 15, 16, 31, 32, 1024)


def scalar_history_linear(hist, hits, iterations, normal_power_log2, sigma_depth, sigma_color):
    """DESIGN.md §4i line by line, one np.float32 operation at a time."""
    H, W = hist.shape[:2]
    h = (F(3.0 / 8.0), F(1.0 / 4.0), F(1.0 / 16.0))
    c = [[[F(hist[y, x, k]) for k in range(3)] for x in range(W)] for y in range(H)]
    n = [[F(hist[y, x, 3]) for x in range(W)] for y in range(H)]
    isc = F(1.0) / F(sigma_color)

    def live(y, x):
        return bool(hits[y, x]["tri"] >= 0 and n[y][x] >= 1)          # a NaN n fails

    def passes(y, x):
        e = ((int(np.array(n[y][x], F).view(np.uint32)) >> 23) & 0xFF) - 127
        return max(0, iterations - e)

    with np.errstate(all="ignore"):
        for i in range(iterations):
            s = 1 << i
            lum = [[(F(0.2126) * c[y][x][0] + F(0.7152) * c[y][x][1]) + F(0.0722) * c[y][x][2] for x in range(W)]
                   for y in range(H)]
            out = [[None] * W for _ in range(H)]
            for py in range(H):
                for px in range(W):
                    if not (live(py, px) and i < passes(py, px)):
                        out[py][px] = list(c[py][px])
                        continue
                    hp = hits[py, px]
                    isc_p = (isc * F(s)) * n[py][px]
                    n_p = [F(v) for v in hp["normal"]]
                    pos_p = [F(v) for v in hp["pos"]]
                    kz = F(1.0) / (F(sigma_depth) * F(hp["t"]))
                    acc = [F(0.0), F(0.0), F(0.0)]
                    wsum = F(0.0)
                    for dy in range(-2, 3):
                        for dx in range(-2, 3):
                            qx, qy = px + dx * s, py + dy * s
                            if qx < 0 or qx >= W or qy < 0 or qy >= H or not live(qy, qx):
                                continue
                            n_q = [F(v) for v in hits[qy, qx]["normal"]]
                            nd = np.fmax(F(0.0), (n_p[0] * n_q[0] + n_p[1] * n_q[1]) + n_p[2] * n_q[2])
                            for _ in range(normal_power_log2):
                                nd = nd * nd
                            e = [F(hits[qy, qx]["pos"][k]) - pos_p[k] for k in range(3)]
                            d = abs((n_p[0] * e[0] + n_p[1] * e[1]) + n_p[2] * e[2])
                            x = d * kz
                            y = abs(lum[py][px] - lum[qy][qx]) * isc_p
                            w = (((h[abs(dx)] * h[abs(dy)]) * nd) * n[qy][qx]) / ((F(1.0) + x * x) * (F(1.0) + y * y))
                            for k in range(3):
                                acc[k] = acc[k] + w * c[qy][qx][k]
                            wsum = wsum + w
                    out[py][px] = [acc[k] / wsum for k in range(3)] if wsum > 0 else list(c[py][px])
            c = out
    return np.array(c, dtype=F)


def random_history(H, W, seed, n_set=N_SET):
    """random_frame's guides with a history record per pixel: linear colours in
    [0, 1.44), n drawn per pixel from n_set (pixels without a hit included)."""
    rad, hits = random_frame(H, W, seed=seed)
    rng = np.random.default_rng(seed + 5000)
    hist = np.zeros((H, W, 4), F)
    hist[..., :3] = rad * rad
    hist[..., 3] = rng.choice(np.array(n_set, F), size=(H, W))
    return hist, hits


@pytest.mark.parametrize("iterations", [1, 3, 4, 6])
def test_scalar_restatement_agrees_bit_for_bit(iterations):
    hist, hits = random_history(9, 13, seed=200 + iterations)
    hist[2, 3, 3] = np.nan                                   # not live, and no tap
    hist[4, 4, 3] = 1.5
    hist[6, 1, 3] = np.inf
    for npow, sd, sc in ((7, 0.005, 0.5), (0, 3.0, 0.25), (2, 50.0, 4.0)):
        want = scalar_history_linear(hist, hits, iterations, npow, sd, sc)
        got = A.denoise_history_linear(hist, hits, iterations, npow, sd, sc)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (iterations, npow)
    assert (A.denoise_history_linear(hist, hits, iterations, 0, 50.0, 4.0) != hist[..., :3]).any()


@pytest.mark.parametrize("iterations", [1, 4, 6])
def test_one_sample_everywhere_is_the_fixed_filter(iterations):
    """n = 1 on every hit pixel and c = g * g: every multiplication by n is exact,
    k = iterations, so the output is denoise_ref.denoise(g) bit for bit."""
    g, hits = random_frame(23, 37, seed=31)
    hist = np.concatenate([g * g, np.where(hits["tri"] >= 0, F(1.0), F(0.0))[..., None]], -1).astype(F)
    for npow, sd, sc in ((7, 0.005, 0.5), (0, 50.0, 4.0)):
        want_rad, want_rgba = D.denoise(g, hits, iterations, npow, sd, sc)
        got_rad, got_rgba = A.denoise_history(hist, hits, iterations, npow, sd, sc)
        assert np.array_equal(got_rad.view(np.uint32), want_rad.view(np.uint32))
        assert np.array_equal(got_rgba, want_rgba)
    assert (D.denoise(g, hits, iterations, 0, 50.0, 4.0)[0] != g).any()


@pytest.mark.parametrize("iterations", [1, 4, 6])
def test_a_long_history_everywhere_is_the_identity(iterations):
    """n >= 2^iterations on every pixel: no pixel is filtered, radiance = sqrt(c)."""
    hist, hits = random_history(23, 37, seed=32, n_set=(1 << iterations, (1 << iterations) + 1, 1024, 4096))
    rad, rgba = A.denoise_history(hist, hits, iterations, 0, 50.0, 4.0)
    want = np.sqrt(hist[..., :3])
    assert np.array_equal(rad.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(rgba, D.unorm8(want)) and (rgba[..., 3] == 255).all()


def test_pixels_that_are_not_live_pass_through():
    hist, hits = random_history(23, 37, seed=33)
    hist[3, 5, 3], hist[7, 9, 3], hist[8, 1, 3] = np.nan, 0.5, -4.0
    hits["tri"][3, 5] = hits["tri"][7, 9] = hits["tri"][8, 1] = 1
    live, k = A.pass_counts(hist, hits)
    assert not live[3, 5] and not live[7, 9] and not live[8, 1]
    assert (live == ((hits["tri"] >= 0) & (hist[..., 3] >= 1))).all() and live.any() and (~live).any()
    lin = A.denoise_history_linear(hist, hits, 4, 0, 50.0, 4.0)
    assert np.array_equal(lin[~live].view(np.uint32), hist[..., :3][~live].view(np.uint32))
    assert (lin[live & (k > 0)] != hist[..., :3][live & (k > 0)]).any()
    rad, rgba = A.denoise_history(hist, hits, 4, 0, 50.0, 4.0)
    assert np.array_equal(rad[~live].view(np.uint32), np.sqrt(hist[..., :3])[~live].view(np.uint32))
    assert np.array_equal(rgba[~live], D.unorm8(np.sqrt(hist[..., :3]))[~live])


@pytest.mark.parametrize("iterations", [1, 4, 6])
def test_two_to_the_j_samples_are_filtered_in_iterations_minus_j_passes(iterations):
    """One plane seen head-on (every normal and depth weight is 1) with random
    colours: a pixel that a pass filters gets a mean over differing neighbours,
    so its bits change.  Per pass, the pixels that changed are exactly those
    with i < max(0, iterations - j), n = 2^j.  The frame is wider than two of the
    last pass's steps, so every pixel has a tap besides itself in every pass."""
    H, W = 67, 71
    rng = np.random.default_rng(34)
    hits = np.zeros((H, W), D.HIT_DTYPE)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    hits["tri"], hits["t"] = 1, 10.0
    hits["normal"] = (0.0, 0.0, 1.0)
    hits["pos"][..., 0], hits["pos"][..., 1] = xs * 0.1, ys * 0.1
    hist = np.zeros((H, W, 4), F)
    hist[..., :3] = rng.uniform(0.1, 1.0, size=(H, W, 3))
    j = rng.integers(0, 8, size=(H, W))
    hist[..., 3] = np.exp2(j)
    changed = []
    A.denoise_history_linear(hist, hits, iterations, changed=changed)
    want_k = np.maximum(0, iterations - j)
    assert np.array_equal(A.pass_counts(hist, hits, iterations)[1], want_k)
    assert len(changed) == iterations
    for i, ch in enumerate(changed):
        print(f"{iterations} passes, pass {i}: {int(ch.sum())} of {H * W} pixels changed")
        assert np.array_equal(ch, i < want_k), i
    assert np.array_equal(np.sum(changed, axis=0), want_k)
    for k in range(iterations + 1):
        assert (want_k == k).any()


# ---- quality on the CPU oracle ------------------------------------------------

def run_sequence_with_history(oracle, step_deg, monkeypatch):
    """test_temporal_ref.run_sequence, keeping the last history record it computed."""
    kept = {}
    temporal = T.temporal

    def keeping(*a, **kw):
        out = temporal(*a, **kw)
        kept["hist"] = out[0]
        return out

    with monkeypatch.context() as m:
        m.setattr(TT.T, "temporal", keeping)
        raw, rad, reused, hits = run_sequence(oracle, step_deg)
    assert np.array_equal(np.sqrt(kept["hist"][..., :3]).view(np.uint32), rad.view(np.uint32))
    return raw, rad, hits, kept["hist"]


@pytest.mark.parametrize("step_deg", [0.0, 1.0])
def test_quality_on_the_oracle(oracle, step_deg, monkeypatch):
    """Config 2 at 160x90, 8 frames ending at the default camera: the mean squared
    radiance error against the 256-frame accumulation as a share of the raw last
    frame's.  The adaptive filter is below both fixed filters run after the
    accumulation at both cameras, below the accumulation alone for the static
    camera, and at most 1.05 times it (whole frame and Lambertian first hits)
    for the orbiting one.  Every figure compared is computed in this run."""
    raw, rad, hits, hist = run_sequence_with_history(oracle, step_deg, monkeypatch)
    ref = oracle["ref"]
    hit = hits["tri"] >= 0
    lamb = hit & (oracle["mat_type"][np.maximum(hits["tri"], 0)] == 0.0)
    t2 = D.denoise(rad, hits, iterations=2)[0]
    t4 = D.denoise(rad, hits)[0]
    ad = A.denoise_history(hist, hits)[0]
    fig = {name: (share(x, raw, ref), share(x, raw, ref, lamb))
           for name, x in (("temporal", rad), ("fixed 2-pass", t2), ("fixed 4-pass", t4), ("adaptive", ad))}
    print(f"{step_deg} deg/frame, {TT.FRAMES} frames, MSE share whole frame / Lambertian: "
          + ", ".join(f"{k} {v[0]:.4f} / {v[1]:.4f}" for k, v in fig.items()))
    assert lamb.any() and (~hit).any()
    assert fig["adaptive"][0] < fig["fixed 2-pass"][0]
    assert fig["adaptive"][0] < fig["fixed 4-pass"][0]
    if step_deg == 0.0:
        assert fig["adaptive"][0] < fig["temporal"][0]
    else:
        assert fig["adaptive"][0] <= 1.05 * fig["temporal"][0]
        assert fig["adaptive"][1] <= 1.05 * fig["temporal"][1]
