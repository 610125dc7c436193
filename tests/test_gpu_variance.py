"""rt_temporal_moments_device / rt_denoise_variance_device /
rt_render_temporal_variance on the GPU: every output bit equals
tests/variance_ref.py (the numpy restatement of DESIGN.md §4j).  The
accumulation on test_temporal_ref's random camera pairs and guides, in both lane
mappings, with and without a previous frame, at ragged and degenerate sizes,
its history and display outputs also equal to rt_temporal_device's on the GPU.
The filter on synthetic guides whose history lengths put both sides of
min_history and of every pass-count boundary into one wave and one LDS tile and
whose moments hold m2 above, equal to and below m1^2, for every pass count in
all three dispatches (option denoise_kernel).  Guard bytes, untouched inputs,
argument errors; rt_render_temporal_variance = the four device calls composed,
drops its history after a call that wrote no moments, refuses what
rt_render_temporal refuses and leaves the render state as an ordinary render
does."""
import ctypes as C

import numpy as np
import pytest

import denoise_history_ref as A
import denoise_ref as D
import variance_ref as V
from conftest import has_gpu
from test_denoise_ref import random_frame
from test_gpu_denoise import Guarded
from test_gpu_temporal import BOUNCES, camera, synthetic_pair
from test_gpu_temporal import run as run_temporal
from test_temporal_ref import look_at
from test_variance_ref import random_moments

pytestmark = pytest.mark.gpu

F = np.float32
FORMS = (0, 1, 2)     # options temporal_tile / denoise_kernel: the shipped choice and the two forms
SIZES = ((129, 65), (37, 23))
N_SET = (0, 1, 2, 3, 4, 5, 7, 8, 15, 16, 31, 32, 1024)


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


@pytest.fixture(scope="module")
def r():
    if not has_gpu():
        pytest.skip("no GPU")
    import rtamd
    from rtamd import configs
    rr = rtamd.Renderer((0,))
    rr.set_option("accel", 8)
    rr.upload_scene(configs.config2().build())
    yield rr
    rr.close()


# ---- rt_temporal_moments_device ---------------------------------------------------

def run_moments(r, rad, hits, cam, prev=None, params=None, form=0, rgba=True, radiance=True):
    """rt_temporal_moments_device on host arrays through guarded device buffers;
    prev = (camera bytes, history, hit records, moments) or None.  Returns
    (history, rgba or None, radiance or None, moments); asserts that nothing
    outside the outputs was written and that the inputs are unchanged."""
    import torch
    h, w = rad.shape[:2]
    rad = np.ascontiguousarray(rad, F)
    hits = np.ascontiguousarray(hits)
    d_rad, d_hit = Guarded(w * h * 12, rad), Guarded(w * h * 32, hits)
    ins = [(d_rad, rad), (d_hit, hits)]
    d_hp = d_hq = d_mp = None
    if prev is not None:
        hist_prev, hits_prev = np.ascontiguousarray(prev[1], F), np.ascontiguousarray(prev[2])
        mom_prev = np.ascontiguousarray(prev[3], F)
        d_hp, d_hq, d_mp = Guarded(w * h * 16, hist_prev), Guarded(w * h * 32, hits_prev), Guarded(w * h * 8, mom_prev)
        ins += [(d_hp, hist_prev), (d_hq, hits_prev), (d_mp, mom_prev)]
    o_hist, o_mom = Guarded(w * h * 16), Guarded(w * h * 8)
    o_rgba = Guarded(w * h * 4) if rgba else None
    o_rad = Guarded(w * h * 12) if radiance else None
    r.set_option("temporal_tile", form)
    try:
        r.temporal_moments_device(w, h, cam, d_rad.ptr, d_hit.ptr, o_hist.ptr, o_mom.ptr,
                                  prev[0] if prev is not None else None, d_hp.ptr if d_hp else None,
                                  d_hq.ptr if d_hq else None, d_mp.ptr if d_mp else None,
                                  o_rgba.ptr if rgba else None, o_rad.ptr if radiance else None, params,
                                  torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    finally:
        r.set_option("temporal_tile", 0)
    for b in (d_rad, d_hit, d_hp, d_hq, d_mp, o_hist, o_mom, o_rgba, o_rad):
        assert b is None or b.guards_intact()
    for buf, host in ins:
        assert buf.host(np.uint8, -1).tobytes() == host.tobytes()
    return (o_hist.host(F, (h, w, 4)), o_rgba.host(np.uint8, (h, w, 4)) if rgba else None,
            o_rad.host(F, (h, w, 3)) if radiance else None, o_mom.host(F, (h, w, 2)))


def check_moments(r, rad, hits, cam, prev=None, kw=None, forms=FORMS):
    """Every mapping equals the reference bit for bit, and rt_temporal_device on
    the GPU in its three outputs; returns the reference's (history, moments, reused)."""
    import rtamd
    import temporal_ref as T
    kw = {**T.DEFAULTS, **(kw or {})}
    p = prev if prev is not None else (None, None, None, None)
    want_hist, want_rad, want_rgba, reused, want_mom = V.temporal_moments(rad, hits, cam, p[0], p[1], p[2], p[3], **kw)
    params = rtamd.TemporalParams(**kw)
    for form in forms:
        hist, rgba, out, mom = run_moments(r, rad, hits, cam, prev, params, form)
        diff = bits(mom) != bits(want_mom)
        assert not diff.any(), (form, kw, int(diff.sum()), np.argwhere(diff)[:4].tolist())
        assert np.array_equal(bits(hist), bits(want_hist)), (form, kw)
        assert np.array_equal(bits(out), bits(want_rad)) and np.array_equal(rgba, want_rgba), (form, kw)
    t_hist, t_rgba, t_rad = run_temporal(r, rad, hits, cam, prev[:3] if prev is not None else None, params, 0)
    assert np.array_equal(bits(t_hist), bits(hist)) and np.array_equal(bits(t_rad), bits(out))
    assert np.array_equal(t_rgba, rgba)
    return want_hist, want_mom, reused


def moments_pair(h, w, seed):
    """test_gpu_temporal.synthetic_pair with moments for the previous history."""
    rad, hits, cam, prev = synthetic_pair(h, w, seed)
    return rad, hits, cam, prev + (random_moments(prev[1], seed + 9),)


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("kw", [dict(), dict(max_history=2, plane_tol=50.0, normal_min=-1.0)], ids=["defaults", "wide"])
def test_moments_equal_the_reference(r, size, kw):
    w, h = size
    rad, hits, cam, prev = moments_pair(h, w, seed=3000 + w)
    _, mom, reused = check_moments(r, rad, hits, cam, prev, kw)
    assert int(reused.sum()) > 20                               # the gather path was compared
    lum = V.luminance((rad * rad).astype(F))
    assert (bits(mom[..., 0])[reused] != bits(lum)[reused]).any()
    # a first frame: no previous set
    _, mom0, reused0 = check_moments(r, rad, hits, cam, None, kw)
    assert not reused0.any() and np.array_equal(bits(mom0), bits(np.stack([lum, lum * lum], -1)))


@pytest.mark.parametrize("w,h", [(1, 1), (3, 70), (70, 3)])
def test_moments_at_degenerate_sizes(r, w, h):
    rad, hits, cam, prev = moments_pair(h, w, seed=w * 100 + h)
    hits["tri"][0, 0] = 5                           # at least one pixel with a hit
    check_moments(r, rad, hits, cam)
    check_moments(r, rad, hits, cam, prev)
    check_moments(r, rad, hits, cam, prev, dict(max_history=2, plane_tol=50.0, normal_min=-1.0))
    # an unmoved camera on its own guides: every valid pixel reuses its own record
    cam0 = look_at((3.0, 4.0, 40.0))
    _, _, reused = check_moments(r, rad, hits, cam0, (cam0, prev[1], hits, prev[3]))
    ok = (hits["tri"] >= 0) & np.isfinite(hits["normal"]).all(-1) & (prev[1][..., 3] > 0)
    assert np.array_equal(reused, ok)


def test_moments_single_outputs_and_default_params(r):
    rad, hits, cam, prev = moments_pair(41, 67, seed=77)
    want = V.temporal_moments(rad, hits, cam, *prev)
    for form in (1, 2):
        hist, none, none2, mom = run_moments(r, rad, hits, cam, prev, None, form, rgba=False, radiance=False)
        assert none is None and none2 is None
        assert np.array_equal(bits(hist), bits(want[0])) and np.array_equal(bits(mom), bits(want[4]))
    hist, rgba, none, mom = run_moments(r, rad, hits, cam, prev, None, 0, rgba=True, radiance=False)
    assert none is None and np.array_equal(rgba, want[2]) and np.array_equal(bits(mom), bits(want[4]))


def test_moments_argument_errors(r):
    import torch
    import rtamd
    from rtamd import RtError, configs
    w, h = 16, 8
    n = w * h
    buf = lambda nbytes: torch.zeros(nbytes + 64, dtype=torch.uint8, device="cuda:0")   # noqa: E731
    rad, hit, hp, hq, oh, o1, o2 = buf(n * 12), buf(n * 32), buf(n * 16), buf(n * 32), buf(n * 16), buf(n * 4), buf(n * 12)
    mp, om = buf(n * 8), buf(n * 8)
    cam = configs.Camera.default(w, h)
    good = dict(width=w, height=h, camera=cam, d_radiance=rad.data_ptr(), d_hits=hit.data_ptr(),
                d_hist_out=oh.data_ptr(), d_mom_out=om.data_ptr(), prev_camera=cam, d_hist_prev=hp.data_ptr(),
                d_hits_prev=hq.data_ptr(), d_mom_prev=mp.data_ptr(), d_out_rgba=o1.data_ptr(),
                d_out_radiance=o2.data_ptr(), params=None)
    r.temporal_moments_device(**good)               # the baseline is accepted
    r.temporal_moments_device(**{**good, "prev_camera": None, "d_hist_prev": None, "d_hits_prev": None,
                                 "d_mom_prev": None, "d_out_rgba": None, "d_out_radiance": None})
    torch.cuda.synchronize()
    P = rtamd.TemporalParams
    bad = [
        dict(camera=None), dict(d_radiance=None), dict(d_hits=None), dict(d_hist_out=None), dict(d_mom_out=None),
        # a partial previous set
        dict(prev_camera=None), dict(d_hist_prev=None), dict(d_hits_prev=None), dict(d_mom_prev=None),
        dict(prev_camera=None, d_hist_prev=None, d_hits_prev=None),
        dict(d_hist_prev=None, d_hits_prev=None, d_mom_prev=None),
        dict(width=0), dict(height=-3), dict(width=1 << 16, height=1 << 16),
        dict(params=P(max_history=0)), dict(params=P(max_history=1025)),
        dict(params=P(plane_tol=0.0)), dict(params=P(plane_tol=float("nan"))),
        dict(params=P(normal_min=1.5)), dict(params=P(normal_min=float("nan"))),
        # alignment
        dict(d_hits=hit.data_ptr() + 8), dict(d_hits_prev=hq.data_ptr() + 8), dict(d_hist_prev=hp.data_ptr() + 4),
        dict(d_hist_out=oh.data_ptr() + 8), dict(d_radiance=rad.data_ptr() + 2), dict(d_out_rgba=o1.data_ptr() + 1),
        dict(d_out_radiance=o2.data_ptr() + 2), dict(d_mom_prev=mp.data_ptr() + 4), dict(d_mom_out=om.data_ptr() + 4),
        # overlaps
        dict(d_hist_out=hp.data_ptr()), dict(d_hist_out=hit.data_ptr()), dict(d_hist_out=rad.data_ptr()),
        dict(d_out_rgba=rad.data_ptr()), dict(d_out_radiance=hq.data_ptr()), dict(d_out_rgba=oh.data_ptr()),
        dict(d_out_radiance=o1.data_ptr()), dict(d_hist_out=mp.data_ptr()), dict(d_out_rgba=mp.data_ptr()),
        dict(d_mom_out=mp.data_ptr()), dict(d_mom_out=mp.data_ptr() + 8), dict(d_mom_out=rad.data_ptr()),
        dict(d_mom_out=hit.data_ptr() + 16), dict(d_mom_out=hp.data_ptr()), dict(d_mom_out=hq.data_ptr() + n * 16),
        dict(d_mom_out=oh.data_ptr() + 8), dict(d_mom_out=o1.data_ptr()), dict(d_mom_out=o2.data_ptr() + 8),
    ]
    for kw in bad:
        with pytest.raises(RtError, match="INVALID_ARG.*rt_temporal_moments_device") as ei:
            r.temporal_moments_device(**{**good, **kw})
        assert ei.value.code == -1, kw
    null = C.c_void_p()
    assert rtamd.lib().rt_temporal_moments_device(null, w, h, C.byref(cam.ubo), rad.data_ptr(), hit.data_ptr(), None,
                                                  None, None, None, oh.data_ptr(), None, None, None, None, None,
                                                  om.data_ptr()) == -1
    assert b"rt_temporal_moments_device" in rtamd.lib().rt_last_error()


# ---- rt_denoise_variance_device ---------------------------------------------------

def variance_frame(h, w, seed):
    """random_frame's guides, a history record per pixel (c = g * g, n drawn per
    pixel from N_SET: n = 1 with probability 0.3, the only filtered count at 1
    pass, 2 and 3 with 0.1 each, the others evenly) and random_moments' moments."""
    rad, hits = random_frame(h, w, seed=seed, nan_normals=3)
    rng = np.random.default_rng(seed + 7000)
    ns = np.array(N_SET)
    p = np.where(ns == 1, 0.3, np.where((ns == 2) | (ns == 3), 0.1, 0.5 / (len(N_SET) - 3)))
    hist = np.concatenate([rad * rad, rng.choice(np.array(N_SET, F), size=(h, w), p=p)[..., None]], -1).astype(F)
    hist = np.ascontiguousarray(hist)
    return hist, random_moments(hist, seed + 8000), hits


def not_vacuous(hist, mom, hits, iterations, min_history):
    """At least 20% of the hit pixels take the 49-tap branch (none with
    min_history 1), at least 20% are filtered in some pass, every pass count
    0..iterations occurs, and the moments hold every kind of variance."""
    live, k = A.pass_counts(hist, hits, iterations)
    hit = hits["tri"] >= 0
    spatial = []
    rec = V.estimate(hist, mom, hits, min_history=min_history, spatial=spatial)
    if min_history > 1:
        assert spatial[0][hit].mean() >= 0.2, float(spatial[0][hit].mean())
    else:
        assert not spatial[0].any()
    assert (k[hit] > 0).mean() >= 0.2, float((k[hit] > 0).mean())
    for j in range(iterations + 1):
        assert (k[hit] == j).any(), (iterations, j)
    d = mom[..., 1] - mom[..., 0] * mom[..., 0]
    assert (d[live] > 0).any() and (d[live] == 0).any() and (d[live] < 0).any() and (d[live] > 1e5).any()
    assert (rec[..., 3][live] == 0).any() and (rec[..., 3][~live] == -1).all()


def run(r, hist, mom, hits, params=None, form=0, rgba=True, radiance=True):
    """rt_denoise_variance_device on host arrays through guarded device buffers:
    (rgba or None, radiance or None); asserts that nothing outside the outputs
    and the workspace was written and that the inputs are unchanged."""
    import torch
    h, w = hist.shape[:2]
    hist, mom = np.ascontiguousarray(hist, F), np.ascontiguousarray(mom, F)
    hits = np.ascontiguousarray(hits)
    d_hist, d_mom, d_hit = Guarded(w * h * 16, hist), Guarded(w * h * 8, mom), Guarded(w * h * 32, hits)
    d_ws = Guarded(r.denoise_workspace_bytes(w, h))
    o_rgba = Guarded(w * h * 4) if rgba else None
    o_rad = Guarded(w * h * 12) if radiance else None
    r.set_option("denoise_kernel", form)
    try:
        r.denoise_variance_device(w, h, d_hist.ptr, d_mom.ptr, d_hit.ptr, d_ws.ptr, o_rgba.ptr if rgba else None,
                                  o_rad.ptr if radiance else None, params, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    finally:
        r.set_option("denoise_kernel", 0)
    for b in (d_hist, d_mom, d_hit, d_ws, o_rgba, o_rad):
        assert b is None or b.guards_intact()
    assert d_hist.host(np.uint8, -1).tobytes() == hist.tobytes()            # the inputs are never written
    assert d_mom.host(np.uint8, -1).tobytes() == mom.tobytes()
    assert d_hit.host(np.uint8, -1).tobytes() == hits.tobytes()
    return (o_rgba.host(np.uint8, (h, w, 4)) if rgba else None,
            o_rad.host(np.float32, (h, w, 3)) if radiance else None)


def check(r, hist, mom, hits, kw, forms=FORMS):
    import rtamd
    kw = {**V.DEFAULTS, **kw}
    want_rad, want_rgba = V.denoise_variance(hist, mom, hits, **kw)
    params = rtamd.VarianceParams(**kw)
    for form in forms:
        rgba, out = run(r, hist, mom, hits, params, form)
        diff = bits(out) != bits(want_rad)
        assert not diff.any(), (form, kw, int(diff.sum()), np.argwhere(diff)[:4].tolist())
        assert np.array_equal(rgba, want_rgba), (form, kw)
    return want_rad


@pytest.fixture(scope="module")
def frames():
    return {(w, h): variance_frame(h, w, seed=w * 1000 + h) for w, h in SIZES}


@pytest.mark.parametrize("iterations", [1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("size", SIZES)
def test_mixed_histories_equal_the_reference(r, frames, size, iterations):
    hist, mom, hits = frames[size]
    not_vacuous(hist, mom, hits, iterations, 4)
    check(r, hist, mom, hits, {"iterations": iterations})
    # wide sigmas and power 0: every tap carries weight (at 6 passes the step reaches 32: past 37x23's height)
    out = check(r, hist, mom, hits, {"iterations": iterations, "normal_power_log2": 0, "sigma_depth": 50.0,
                                     "sigma_lum": 1.5})
    live, k = A.pass_counts(hist, hits, iterations)
    raw = np.sqrt(hist[..., :3])
    assert (out[live & (k > 0)] != raw[live & (k > 0)]).any()
    assert np.array_equal(bits(out[k == 0]), bits(raw[k == 0]))


@pytest.mark.parametrize("min_history", [1, 8])
@pytest.mark.parametrize("size", SIZES)
def test_min_history(r, frames, size, min_history):
    hist, mom, hits = frames[size]
    not_vacuous(hist, mom, hits, 4, min_history)
    check(r, hist, mom, hits, {"min_history": min_history})
    check(r, hist, mom, hits, {"min_history": min_history, "iterations": 6, "normal_power_log2": 0, "sigma_depth": 50.0,
                               "sigma_lum": 0.5})


@pytest.mark.parametrize("w,h", [(1, 1), (3, 70), (70, 3)])
def test_degenerate_sizes(r, w, h):
    hist, mom, hits = variance_frame(h, w, seed=w * 100 + h)
    hits["tri"][0, 0], hist[0, 0, 3] = 5, 1.0       # at least one pixel that is filtered
    for kw in ({}, {"iterations": 6}, {"iterations": 1, "normal_power_log2": 0, "sigma_depth": 50.0, "min_history": 8}):
        check(r, hist, mom, hits, kw)


def test_odd_sample_counts_and_moments(r):
    """n and moments that rt_temporal_moments_device never writes: NaN, infinity, fractions, negatives."""
    hist, mom, hits = variance_frame(23, 37, seed=77)
    rng = np.random.default_rng(78)
    odd = np.array([np.nan, np.inf, -np.inf, 0.5, 1.5, -4.0, 0.99999994, 2.5e38, 1e-40], F)
    pick = rng.random((23, 37)) < 0.3
    hist[..., 3][pick] = rng.choice(odd, size=int(pick.sum()))
    pick = rng.random((23, 37, 2)) < 0.1
    mom[pick] = rng.choice(np.array([np.nan, np.inf, -np.inf, -1.0, 3e38, 1e-42], F), size=int(pick.sum()))
    check(r, hist, mom, hits, {"normal_power_log2": 0, "sigma_depth": 50.0})
    check(r, hist, mom, hits, {"min_history": 8})


@pytest.mark.parametrize("form", [1, 2])
def test_single_outputs_and_default_params(r, frames, form):
    hist, mom, hits = frames[(37, 23)]
    want_rad, want_rgba = V.denoise_variance(hist, mom, hits)
    rgba, none = run(r, hist, mom, hits, None, form, rgba=True, radiance=False)
    assert none is None and np.array_equal(rgba, want_rgba)
    none, out = run(r, hist, mom, hits, None, form, rgba=False, radiance=True)
    assert none is None and np.array_equal(bits(out), bits(want_rad))


@pytest.mark.parametrize("iterations", [1, 4, 6])
def test_a_long_history_everywhere_is_the_identity(r, iterations):
    import rtamd
    hist, mom, hits = variance_frame(65, 129, seed=42)
    rng = np.random.default_rng(43)
    hist[..., 3] = rng.choice(np.array([1 << iterations, (1 << iterations) + 1, 1024], F), size=(65, 129))
    want = np.sqrt(hist[..., :3])
    params = rtamd.VarianceParams(iterations=iterations, normal_power_log2=0, sigma_depth=50.0, min_history=1024)
    for form in FORMS:
        rgba, out = run(r, hist, mom, hits, params, form)
        assert np.array_equal(bits(out), bits(want)), form
        assert np.array_equal(rgba, D.unorm8(want)), form


def test_argument_errors(r):
    import torch
    import rtamd
    from rtamd import RtError
    w, h = 16, 8
    n = w * h
    buf = lambda nbytes: torch.zeros(nbytes + 64, dtype=torch.uint8, device="cuda:0")   # noqa: E731
    hist, mom, hit, ws, o1, o2 = buf(n * 16), buf(n * 8), buf(n * 32), buf(n * 32), buf(n * 4), buf(n * 12)
    good = dict(width=w, height=h, d_hist=hist.data_ptr(), d_mom=mom.data_ptr(), d_hits=hit.data_ptr(),
                d_workspace=ws.data_ptr(), d_out_rgba=o1.data_ptr(), d_out_radiance=o2.data_ptr(), params=None)
    r.denoise_variance_device(**good)               # the baseline is accepted
    torch.cuda.synchronize()
    P = rtamd.VarianceParams
    bad = [
        dict(d_hist=None), dict(d_mom=None), dict(d_hits=None), dict(d_workspace=None),
        dict(d_out_rgba=None, d_out_radiance=None),
        dict(width=0), dict(height=-3), dict(width=1 << 16, height=1 << 16),
        dict(params=P(iterations=0)), dict(params=P(iterations=7)),
        dict(params=P(normal_power_log2=-1)), dict(params=P(normal_power_log2=11)),
        dict(params=P(sigma_depth=0.0)), dict(params=P(sigma_depth=float("nan"))),
        dict(params=P(sigma_lum=-1.0)), dict(params=P(sigma_lum=0.0)), dict(params=P(sigma_lum=float("inf"))),
        dict(params=P(min_history=0)), dict(params=P(min_history=1025)),
        dict(d_hits=hit.data_ptr() + 8), dict(d_workspace=ws.data_ptr() + 4), dict(d_hist=hist.data_ptr() + 4),
        dict(d_mom=mom.data_ptr() + 4), dict(d_out_rgba=o1.data_ptr() + 2), dict(d_out_radiance=o2.data_ptr() + 1),
        dict(d_out_rgba=hist.data_ptr()), dict(d_out_radiance=hit.data_ptr() + 16), dict(d_out_rgba=mom.data_ptr()),
        dict(d_out_radiance=mom.data_ptr() + 8),
        dict(d_out_rgba=ws.data_ptr() + n * 16), dict(d_out_radiance=o1.data_ptr()),
        dict(d_workspace=hit.data_ptr()), dict(d_workspace=hist.data_ptr()), dict(d_workspace=mom.data_ptr()),
    ]
    for kw in bad:
        with pytest.raises(RtError, match="INVALID_ARG.*rt_denoise_variance_device") as ei:
            r.denoise_variance_device(**{**good, **kw})
        assert ei.value.code == -1, kw
    null = C.c_void_p()
    assert rtamd.lib().rt_denoise_variance_device(null, w, h, hist.data_ptr(), mom.data_ptr(), hit.data_ptr(), None,
                                                  ws.data_ptr(), o1.data_ptr(), None, None, None) == -1
    for v in (1, -2):
        with pytest.raises(RtError, match="INVALID_ARG"):
            r.set_option("variance_stage", v)
    assert r.get_option("variance_stage") == -1
    assert r.get_option("denoise_kernel") == 0 and r.get_option("denoise_pass") == -1


def test_the_estimate_alone_writes_no_output(r, frames):
    """Option variance_stage 0 (the timing tool's): the estimate's records land in
    the workspace's first half, the outputs stay as they were."""
    import torch
    hist, mom, hits = frames[(37, 23)]
    h, w = hist.shape[:2]
    d_hist, d_mom, d_hit = Guarded(w * h * 16, hist), Guarded(w * h * 8, mom), Guarded(w * h * 32, hits)
    d_ws, o_rad = Guarded(r.denoise_workspace_bytes(w, h)), Guarded(w * h * 12)
    r.set_option("variance_stage", 0)
    try:
        r.denoise_variance_device(w, h, d_hist.ptr, d_mom.ptr, d_hit.ptr, d_ws.ptr, None, o_rad.ptr, None,
                                  torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    finally:
        r.set_option("variance_stage", -1)
    assert (o_rad.host(np.uint8, -1) == 0xEE).all() and d_ws.guards_intact()
    rec = d_ws.host(F, (2, h, w, 4))[0]
    assert np.array_equal(bits(rec), bits(V.estimate(hist, mom, hits)))


@pytest.mark.parametrize("form", [1, 2])
def test_lone_passes_on_one_workspace(r, frames, form):
    """Option denoise_pass: the estimate alone (option variance_stage 0: a lone
    pass skips it), then passes 0, 1 and 2 of a 3-pass filter, each enqueued alone
    on one workspace (steps 1, 2 and 4), leave what the whole filter leaves; a
    pass that is not the last writes neither output."""
    import torch
    import rtamd
    hist, mom, hits = frames[(37, 23)]
    h, w = hist.shape[:2]
    hist, mom, hits = np.ascontiguousarray(hist, F), np.ascontiguousarray(mom, F), np.ascontiguousarray(hits)
    kw = {**V.DEFAULTS, "iterations": 3}
    params = rtamd.VarianceParams(**kw)
    want_rad, want_rgba = V.denoise_variance(hist, mom, hits, **kw)
    whole_rgba, whole_rad = run(r, hist, mom, hits, params, form)
    d_hist, d_mom, d_hit = Guarded(w * h * 16, hist), Guarded(w * h * 8, mom), Guarded(w * h * 32, hits)
    d_ws, o_rgba, o_rad = Guarded(r.denoise_workspace_bytes(w, h)), Guarded(w * h * 4), Guarded(w * h * 12)
    r.set_option("denoise_kernel", form)
    try:
        for i in (-1, 0, 1, 2):                     # -1: the estimate
            r.set_option("variance_stage", 0 if i < 0 else -1)
            r.set_option("denoise_pass", i)
            r.denoise_variance_device(w, h, d_hist.ptr, d_mom.ptr, d_hit.ptr, d_ws.ptr, o_rgba.ptr, o_rad.ptr, params,
                                      torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            if i < 2:
                assert (o_rgba.host(np.uint8, -1) == 0xEE).all() and (o_rad.host(np.uint8, -1) == 0xEE).all(), i
    finally:
        r.set_option("variance_stage", -1)
        r.set_option("denoise_pass", -1)
        r.set_option("denoise_kernel", 0)
    for b in (d_hist, d_mom, d_hit, d_ws, o_rgba, o_rad):
        assert b.guards_intact()
    rgba, out = o_rgba.host(np.uint8, (h, w, 4)), o_rad.host(np.float32, (h, w, 3))
    assert np.array_equal(bits(out), bits(whole_rad)) and np.array_equal(rgba, whole_rgba)
    assert np.array_equal(bits(out), bits(want_rad)) and np.array_equal(rgba, want_rgba)


# ---- rt_render_temporal_variance ----------------------------------------------------

def composed_frame(rr, w, h, cam, prev, tp, vp):
    """One frame through the four device calls on caller-owned buffers:
    rt_render_tile_device with option new_sample, rt_render_hits_device,
    rt_temporal_moments_device (no display output), rt_denoise_variance_device.
    prev = (camera, history, hits, moments tensors) or None.  Returns (rgba,
    radiance, stats of the render, (camera, history, hits, moments tensors))."""
    import torch
    s = torch.cuda.current_stream().cuda_stream
    new = lambda *shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device="cuda:0")   # noqa: E731
    d_rad, d_hits, d_hist, d_mom, d_ws = new(h, w, 3), new(h, w, 8), new(h, w, 4), new(h, w, 2), new(2, h, w, 4)
    o_rgba, o_rad = new(h, w, 4, dtype=torch.uint8), new(h, w, 3)
    rr.set_option("new_sample", 1)
    try:
        st = rr.render_tile_device(cam, w, h, BOUNCES, 0, 0, w, h, None, d_rad.data_ptr(), s, stats=True)
    finally:
        rr.set_option("new_sample", 0)
    rr.render_hits_device(cam, w, h, 0, 0, w, h, d_hits.data_ptr(), s)
    rr.temporal_moments_device(w, h, cam, d_rad.data_ptr(), d_hits.data_ptr(), d_hist.data_ptr(), d_mom.data_ptr(),
                               prev[0] if prev else None, prev[1].data_ptr() if prev else None,
                               prev[2].data_ptr() if prev else None, prev[3].data_ptr() if prev else None,
                               None, None, tp, s)
    rr.denoise_variance_device(w, h, d_hist.data_ptr(), d_mom.data_ptr(), d_hits.data_ptr(), d_ws.data_ptr(),
                               o_rgba.data_ptr(), o_rad.data_ptr(), vp, s)
    torch.cuda.synchronize()
    return o_rgba.cpu().numpy(), o_rad.cpu().numpy(), st, (cam, d_hist, d_hits, d_mom)


def orbit(w, h, k):
    cam = camera(w, h, orbit=1.0 * k)
    cam.ubo.frame_count = k
    return cam


@pytest.mark.parametrize("accel", [8, 0])
def test_render_temporal_variance_is_the_four_calls(accel):
    if not has_gpu():
        pytest.skip("no GPU")
    import torch
    import rtamd
    from rtamd import configs
    w, h = 64, 40
    tp = rtamd.TemporalParams(max_history=8, plane_tol=0.01, normal_min=0.8)
    vp = rtamd.VarianceParams(iterations=3, normal_power_log2=5, sigma_depth=0.02, sigma_lum=1.5, min_history=3)
    with rtamd.Renderer((0,)) as rr:
        rr.set_option("accel", accel)
        rr.upload_scene(configs.config2().build())
        cam0 = camera(w, h)
        rgba0, rad0, _ = rr.render(cam0, w, h, BOUNCES, radiance=True)
        for t_par, v_par in ((None, True), (tp, vp)):
            prev = None
            for k in range(4):
                cam = orbit(w, h, k)
                want_rgba, want_rad, st0, prev = composed_frame(rr, w, h, cam, prev, t_par,
                                                                None if v_par is True else v_par)
                rgba, rad, st = rr.render_temporal(cam, w, h, BOUNCES, t_par, reset=(k == 0), radiance=True,
                                                   stats=True, variance=v_par)
                assert np.array_equal(bits(rad), bits(want_rad)), (accel, k)
                assert np.array_equal(rgba, want_rgba), (accel, k)
                for key in ("segments", "node_visits", "tri_tests", "mat_reads", "pixels"):
                    assert st[key] == st0[key], key
                assert st["ms"] > 0
            # the composition is the numpy reference's too, and the filter did something to the last frame
            hist, mom = prev[1].cpu().numpy(), prev[3].cpu().numpy()
            hits = prev[2].cpu().numpy().view(D.HIT_DTYPE).reshape(h, w)
            kw = dict(V.DEFAULTS) if v_par is True else dict(iterations=3, normal_power_log2=5, sigma_depth=0.02,
                                                             sigma_lum=1.5, min_history=3)
            ref_rad, ref_rgba = V.denoise_variance(hist, mom, hits, **kw)
            assert np.array_equal(bits(rad), bits(ref_rad)) and np.array_equal(rgba, ref_rgba)
            assert (hist[..., 3] > 1).any() and (rad != np.sqrt(hist[..., :3])).any()
        # RGBA only, no stats
        got = rr.render_temporal(orbit(w, h, 4), w, h, BOUNCES, tp, variance=vp)
        assert got[1] is None and got[2] is None
        # a call that wrote no moments advanced the history: the next variance call starts a new sequence
        prev = None
        for k in range(4):
            cam = orbit(w, h, k)
            if k == 2:
                rr.render_temporal(cam, w, h, BOUNCES, tp)
                prev = None                                     # what the context must do as well
                continue
            want_rgba, want_rad, _, prev = composed_frame(rr, w, h, cam, prev, tp, vp)
            rgba, rad, _ = rr.render_temporal(cam, w, h, BOUNCES, tp, reset=(k == 0), radiance=True, variance=vp)
            assert np.array_equal(bits(rad), bits(want_rad)) and np.array_equal(rgba, want_rgba), k
            n = prev[1].cpu().numpy()[..., 3]
            hit = prev[2].cpu().numpy().view(D.HIT_DTYPE).reshape(h, w)["tri"] >= 0
            assert (n[hit] == (2 if k == 1 else 1)).mean() > (0.5 if k == 1 else 0.999), k   # n = 1 again at k = 3
        # ... and the same after the adaptive call; the other two calls still share their history
        rr.render_temporal(orbit(w, h, 4), w, h, BOUNCES, tp, adaptive=True)
        want_rgba, want_rad, _, _ = composed_frame(rr, w, h, orbit(w, h, 5), None, tp, vp)
        rgba, rad, _ = rr.render_temporal(orbit(w, h, 5), w, h, BOUNCES, tp, radiance=True, variance=vp)
        assert np.array_equal(bits(rad), bits(want_rad)) and np.array_equal(rgba, want_rgba)
        # the render state is an ordinary render's: the same frame afterwards
        rgba1, rad1, _ = rr.render(cam0, w, h, BOUNCES, radiance=True)
        assert np.array_equal(rgba1, rgba0) and np.array_equal(bits(rad1), bits(rad0))
        assert rr.get_option("extensions") == 0 and rr.get_option("new_sample") == 0
        # plain_kernels counts the render's kernels only: a warmed variance frame adds what a warmed tile adds
        d_rad = torch.empty((h, w, 3), dtype=torch.float32, device="cuda:0")
        for _ in range(3):
            rr.render_temporal(cam0, w, h, BOUNCES, fixed_seed=True, variance=True)
        k0 = rr.get_option("plain_kernels")
        rr.render_tile_device(cam0, w, h, BOUNCES, 0, 0, w, h, None, d_rad.data_ptr(), None)
        torch.cuda.synchronize()
        k1 = rr.get_option("plain_kernels")
        rr.render_temporal(cam0, w, h, BOUNCES, fixed_seed=True, variance=True)
        k2 = rr.get_option("plain_kernels")
        assert k1 - k0 >= 1 and k2 - k1 == k1 - k0


def test_render_temporal_variance_refusals(r):
    import rtamd
    from rtamd import RtError, configs
    w, h = 64, 40
    cam = configs.Camera.default(w, h)
    r.render_temporal(cam, w, h, BOUNCES, variance=True)
    for kw in (dict(params=rtamd.TemporalParams(max_history=0)), dict(params=rtamd.TemporalParams(plane_tol=-1.0)),
               dict(variance=rtamd.VarianceParams(iterations=9)), dict(variance=rtamd.VarianceParams(sigma_lum=0.0)),
               dict(variance=rtamd.VarianceParams(min_history=0))):
        with pytest.raises(RtError, match="INVALID_ARG.*rt_render_temporal_variance"):
            r.render_temporal(cam, w, h, BOUNCES, **{"variance": True, **kw})
    with pytest.raises(RtError, match="INVALID_ARG"):
        r.render_temporal(cam, 0, h, BOUNCES, variance=True)
    with pytest.raises(ValueError):
        r.render_temporal(cam, w, h, BOUNCES, variance=True, adaptive=True)
    out = np.zeros((h, w, 4), np.uint8)
    L = rtamd.lib()
    ubo = C.byref(cam.ubo)
    assert L.rt_render_temporal_variance(r._ctx, ubo, w, h, BOUNCES, None, None, 0, None, None, None) == -1
    assert L.rt_render_temporal_variance(None, ubo, w, h, BOUNCES, None, None, 0, out.ctypes.data, None, None) == -1
    assert L.rt_render_temporal_variance(r._ctx, ubo, w, h, BOUNCES, None, None, 4, out.ctypes.data, None, None) == -1
    assert b"rt_render_temporal_variance: unknown flags" in L.rt_last_error()
    r.set_option("extensions", 4)
    try:
        with pytest.raises(RtError, match="INVALID_ARG.*rt_render_temporal_variance.*bit 4"):
            r.render_temporal(cam, w, h, BOUNCES, variance=True)
    finally:
        r.set_option("extensions", 0)
    r.upload_spheres([[0.0, 5.0, 0.0, 4.0, 0.9, 0.2, 0.2, 0.0]])
    try:
        r.render_temporal(cam, w, h, BOUNCES, variance=True)     # bit 8 off: triangles only, accepted
        r.set_option("extensions", 8)
        with pytest.raises(RtError, match="INVALID_ARG.*rt_render_temporal_variance.*spheres"):
            r.render_temporal(cam, w, h, BOUNCES, variance=True)
    finally:
        r.set_option("extensions", 0)
        r.upload_spheres(np.zeros((0, 8), np.float32))
    with rtamd.Renderer((0, 0)) as rr:               # the same ordinal twice serves as two devices
        rr.upload_scene(configs.config2().build())
        with pytest.raises(RtError, match="INVALID_ARG.*devices"):
            rr.render_temporal(cam, w, h, BOUNCES, variance=True)
