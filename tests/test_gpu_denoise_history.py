"""rt_denoise_history_device / rt_render_temporal_adaptive on the GPU: radiance
bits and RGBA8 equal tests/denoise_history_ref.py (the numpy restatement of
DESIGN.md §4i) on synthetic guides whose history lengths put both sides of every
pass-count boundary into one wave and one LDS tile, at ragged and degenerate
sizes, for every pass count, in all three dispatches (option denoise_kernel);
the two identities of the contract, the first against rt_denoise_device on the
GPU; guard bytes, an untouched history, argument errors;
rt_render_temporal_adaptive = render + render_hits + temporal + this filter,
shares its history with rt_render_temporal and leaves the render state as an
ordinary render does; HipEngine with the switch on."""
import ctypes as C

import numpy as np
import pytest

import denoise_history_ref as A
import denoise_ref as D
import temporal_ref as T
from conftest import has_gpu
from test_denoise_ref import random_frame
from test_gpu_denoise import Guarded
from test_gpu_denoise import run as run_fixed
from test_gpu_temporal import BOUNCES, camera

pytestmark = pytest.mark.gpu

F = np.float32
FORMS = (0, 1, 2)     # option denoise_kernel: the shipped choice, plain, tiled
N_SET = (0, 1, 2, 3, 4, 7, 8, 15, 16, 31, 32, 1024)


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


def history_frame(h, w, seed):
    """random_frame's guides and a history record per pixel: c = g * g, n drawn
    per pixel from N_SET, n = 1 with probability 0.3 (the only filtered count at
    1 pass) and the others evenly."""
    rad, hits = random_frame(h, w, seed=seed, nan_normals=3)
    rng = np.random.default_rng(seed + 7000)
    p = np.where(np.array(N_SET) == 1, 0.3, 0.7 / (len(N_SET) - 1))
    hist = np.concatenate([rad * rad, rng.choice(np.array(N_SET, F), size=(h, w), p=p)[..., None]], -1).astype(F)
    return np.ascontiguousarray(hist), hits


def not_vacuous(hist, hits, iterations):
    """At least 20% of the hit pixels are filtered in some pass, and every pass
    count 0..iterations occurs."""
    live, k = A.pass_counts(hist, hits, iterations)
    hit = hits["tri"] >= 0
    assert (k[hit] > 0).mean() >= 0.2, float((k[hit] > 0).mean())
    for j in range(iterations + 1):
        assert (k[hit] == j).any(), (iterations, j)


def run(r, hist, hits, params=None, form=0, rgba=True, radiance=True):
    """rt_denoise_history_device on host arrays through guarded device buffers:
    (rgba or None, radiance or None); asserts that nothing outside the outputs
    and the workspace was written and that the inputs are unchanged."""
    import torch
    h, w = hist.shape[:2]
    hist = np.ascontiguousarray(hist, F)
    hits = np.ascontiguousarray(hits)
    d_hist, d_hit = Guarded(w * h * 16, hist), Guarded(w * h * 32, hits)
    d_ws = Guarded(r.denoise_workspace_bytes(w, h))
    o_rgba = Guarded(w * h * 4) if rgba else None
    o_rad = Guarded(w * h * 12) if radiance else None
    r.set_option("denoise_kernel", form)
    try:
        r.denoise_history_device(w, h, d_hist.ptr, d_hit.ptr, d_ws.ptr, o_rgba.ptr if rgba else None,
                                 o_rad.ptr if radiance else None, params, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    finally:
        r.set_option("denoise_kernel", 0)
    for b in (d_hist, d_hit, d_ws, o_rgba, o_rad):
        assert b is None or b.guards_intact()
    assert d_hist.host(np.uint8, -1).tobytes() == hist.tobytes()            # d_hist is never written
    assert d_hit.host(np.uint8, -1).tobytes() == hits.tobytes()
    return (o_rgba.host(np.uint8, (h, w, 4)) if rgba else None,
            o_rad.host(np.float32, (h, w, 3)) if radiance else None)


def check(r, hist, hits, kw, forms=FORMS):
    import rtamd
    want_rad, want_rgba = A.denoise_history(hist, hits, **{**D.DEFAULTS, **kw})
    params = rtamd.DenoiseParams(**{**D.DEFAULTS, **kw})
    for form in forms:
        rgba, out = run(r, hist, hits, params, form)
        diff = out.view(np.uint32) != want_rad.view(np.uint32)
        assert not diff.any(), (form, kw, int(diff.sum()), np.argwhere(diff)[:4].tolist())
        assert np.array_equal(rgba, want_rgba), (form, kw)
    return want_rad


@pytest.fixture(scope="module")
def frames():
    return {(w, h): history_frame(h, w, seed=w * 1000 + h) for w, h in ((129, 65), (37, 23))}


@pytest.mark.parametrize("iterations", [1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("size", [(129, 65), (37, 23)])
def test_mixed_histories_equal_the_reference(r, frames, size, iterations):
    hist, hits = frames[size]
    not_vacuous(hist, hits, iterations)
    check(r, hist, hits, {"iterations": iterations})
    # wide sigmas and power 0: every live tap carries weight (at 6 passes the step reaches 32: past 37x23's height)
    out = check(r, hist, hits, {"iterations": iterations, "normal_power_log2": 0, "sigma_depth": 50.0,
                                "sigma_color": 4.0})
    live, k = A.pass_counts(hist, hits, iterations)
    ok = np.isfinite(hits["normal"]).all(-1)
    raw = np.sqrt(hist[..., :3])
    assert (out[live & (k > 0) & ok] != raw[live & (k > 0) & ok]).mean() > 0.9
    assert np.array_equal(out[k == 0].view(np.uint32), raw[k == 0].view(np.uint32))


@pytest.mark.parametrize("w,h", [(1, 1), (3, 70), (70, 3)])
def test_degenerate_sizes(r, w, h):
    hist, hits = history_frame(h, w, seed=w * 100 + h)
    hits["tri"][0, 0], hist[0, 0, 3] = 5, 1.0       # at least one pixel that is filtered
    for kw in ({}, {"iterations": 6}, {"iterations": 1, "normal_power_log2": 0, "sigma_depth": 50.0}):
        check(r, hist, hits, kw)


def test_odd_sample_counts(r):
    """n that rt_temporal_device never writes: NaN, infinity, fractions, negatives."""
    hist, hits = history_frame(23, 37, seed=77)
    rng = np.random.default_rng(78)
    odd = np.array([np.nan, np.inf, -np.inf, 0.5, 1.5, -4.0, 0.99999994, 2.5e38, 1e-40], F)
    pick = rng.random((23, 37)) < 0.3
    hist[..., 3][pick] = rng.choice(odd, size=int(pick.sum()))
    check(r, hist, hits, {"normal_power_log2": 0, "sigma_depth": 50.0, "sigma_color": 4.0})


@pytest.mark.parametrize("form", [1, 2])
def test_single_outputs_and_default_params(r, frames, form):
    hist, hits = frames[(37, 23)]
    want_rad, want_rgba = A.denoise_history(hist, hits)
    rgba, none = run(r, hist, hits, None, form, rgba=True, radiance=False)
    assert none is None and np.array_equal(rgba, want_rgba)
    none, out = run(r, hist, hits, None, form, rgba=False, radiance=True)
    assert none is None and np.array_equal(out.view(np.uint32), want_rad.view(np.uint32))


@pytest.mark.parametrize("form", [1, 2])
def test_lone_passes_on_one_workspace(r, frames, form):
    """Option denoise_pass: passes 0, 1 and 2 of a 3-pass filter, each enqueued
    alone on one workspace (steps 1, 2 and 4; at 37x23 a step-4 residue class
    ends inside the first tile), leave what the whole filter leaves; a pass
    that is not the last writes neither output."""
    import torch
    import rtamd
    hist, hits = frames[(37, 23)]
    h, w = hist.shape[:2]
    hist, hits = np.ascontiguousarray(hist, F), np.ascontiguousarray(hits)
    kw = {**D.DEFAULTS, "iterations": 3}
    params = rtamd.DenoiseParams(**kw)
    want_rad, want_rgba = A.denoise_history(hist, hits, **kw)
    whole_rgba, whole_rad = run(r, hist, hits, params, form)
    d_hist, d_hit = Guarded(w * h * 16, hist), Guarded(w * h * 32, hits)
    d_ws, o_rgba, o_rad = Guarded(r.denoise_workspace_bytes(w, h)), Guarded(w * h * 4), Guarded(w * h * 12)
    r.set_option("denoise_kernel", form)
    try:
        for i in range(3):
            r.set_option("denoise_pass", i)
            r.denoise_history_device(w, h, d_hist.ptr, d_hit.ptr, d_ws.ptr, o_rgba.ptr, o_rad.ptr, params,
                                     torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            if i < 2:
                assert (o_rgba.host(np.uint8, -1) == 0xEE).all() and (o_rad.host(np.uint8, -1) == 0xEE).all(), i
    finally:
        r.set_option("denoise_pass", -1)
        r.set_option("denoise_kernel", 0)
    for b in (d_hist, d_hit, d_ws, o_rgba, o_rad):
        assert b.guards_intact()
    rgba, out = o_rgba.host(np.uint8, (h, w, 4)), o_rad.host(np.float32, (h, w, 3))
    assert np.array_equal(out.view(np.uint32), whole_rad.view(np.uint32)) and np.array_equal(rgba, whole_rgba)
    assert np.array_equal(out.view(np.uint32), want_rad.view(np.uint32)) and np.array_equal(rgba, want_rgba)


@pytest.mark.parametrize("iterations", [1, 4, 6])
def test_one_sample_everywhere_is_rt_denoise_device(r, iterations):
    """n = 1 on every hit pixel and c = g * g: the fixed filter's bits, from the GPU."""
    import rtamd
    g, hits = random_frame(65, 129, seed=41, nan_normals=3)
    hist = np.concatenate([g * g, np.where(hits["tri"] >= 0, F(1.0), F(0.0))[..., None]], -1).astype(F)
    for kw in ({"iterations": iterations},
               {"iterations": iterations, "normal_power_log2": 0, "sigma_depth": 50.0, "sigma_color": 4.0}):
        params = rtamd.DenoiseParams(**{**D.DEFAULTS, **kw})
        want_rgba, want_rad = run_fixed(r, g, hits, params, 0)
        assert (want_rad != g).any()
        for form in FORMS:
            rgba, out = run(r, hist, hits, params, form)
            assert np.array_equal(out.view(np.uint32), want_rad.view(np.uint32)), (form, kw)
            assert np.array_equal(rgba, want_rgba), (form, kw)


@pytest.mark.parametrize("iterations", [1, 4, 6])
def test_a_long_history_everywhere_is_the_identity(r, iterations):
    import rtamd
    hist, hits = history_frame(65, 129, seed=42)
    rng = np.random.default_rng(43)
    hist[..., 3] = rng.choice(np.array([1 << iterations, (1 << iterations) + 1, 1024], F), size=(65, 129))
    want = np.sqrt(hist[..., :3])
    params = rtamd.DenoiseParams(iterations=iterations, normal_power_log2=0, sigma_depth=50.0, sigma_color=4.0)
    for form in FORMS:
        rgba, out = run(r, hist, hits, params, form)
        assert np.array_equal(out.view(np.uint32), want.view(np.uint32)), form
        assert np.array_equal(rgba, D.unorm8(want)), form


def test_argument_errors(r):
    import torch
    import rtamd
    from rtamd import RtError
    w, h = 16, 8
    n = w * h
    buf = lambda nbytes: torch.zeros(nbytes + 64, dtype=torch.uint8, device="cuda:0")   # noqa: E731
    hist, hit, ws, o1, o2 = buf(n * 16), buf(n * 32), buf(n * 32), buf(n * 4), buf(n * 12)
    good = dict(width=w, height=h, d_hist=hist.data_ptr(), d_hits=hit.data_ptr(), d_workspace=ws.data_ptr(),
                d_out_rgba=o1.data_ptr(), d_out_radiance=o2.data_ptr(), params=None)
    r.denoise_history_device(**good)                # the baseline is accepted
    torch.cuda.synchronize()
    P = rtamd.DenoiseParams
    bad = [
        dict(d_hist=None), dict(d_hits=None), dict(d_workspace=None),
        dict(d_out_rgba=None, d_out_radiance=None),
        dict(width=0), dict(height=-3), dict(width=1 << 16, height=1 << 16),
        dict(params=P(iterations=0)), dict(params=P(iterations=7)),
        dict(params=P(normal_power_log2=-1)), dict(params=P(normal_power_log2=11)),
        dict(params=P(sigma_depth=0.0)), dict(params=P(sigma_depth=float("nan"))),
        dict(params=P(sigma_color=-1.0)), dict(params=P(sigma_color=float("inf"))),
        dict(d_hits=hit.data_ptr() + 8), dict(d_workspace=ws.data_ptr() + 4), dict(d_hist=hist.data_ptr() + 4),
        dict(d_out_rgba=o1.data_ptr() + 2), dict(d_out_radiance=o2.data_ptr() + 1),
        dict(d_out_rgba=hist.data_ptr()), dict(d_out_radiance=hit.data_ptr() + 16),
        dict(d_out_rgba=ws.data_ptr() + n * 16), dict(d_out_radiance=o1.data_ptr()),
        dict(d_workspace=hit.data_ptr()), dict(d_workspace=hist.data_ptr()),
    ]
    for kw in bad:
        with pytest.raises(RtError, match="INVALID_ARG.*rt_denoise_history_device") as ei:
            r.denoise_history_device(**{**good, **kw})
        assert ei.value.code == -1, kw
    null = C.c_void_p()
    assert rtamd.lib().rt_denoise_history_device(null, w, h, hist.data_ptr(), hit.data_ptr(), None, ws.data_ptr(),
                                                 o1.data_ptr(), None, None, None) == -1
    assert r.get_option("denoise_kernel") == 0 and r.get_option("denoise_pass") == -1


# ---- rt_render_temporal_adaptive -----------------------------------------------

def composed_frame(rr, w, h, cam, prev, tp, dp):
    """One frame through the four device calls on caller-owned buffers:
    rt_render_tile_device with option new_sample, rt_render_hits_device,
    rt_temporal_device (no display output), rt_denoise_history_device.
    prev = (camera, history tensor, hits tensor) or None.  Returns (rgba,
    radiance, stats of the render, (camera, history tensor, hits tensor))."""
    import torch
    s = torch.cuda.current_stream().cuda_stream
    new = lambda *shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device="cuda:0")   # noqa: E731
    d_rad, d_hits, d_hist, d_ws = new(h, w, 3), new(h, w, 8), new(h, w, 4), new(2, h, w, 4)
    o_rgba, o_rad = new(h, w, 4, dtype=torch.uint8), new(h, w, 3)
    rr.set_option("new_sample", 1)
    try:
        st = rr.render_tile_device(cam, w, h, BOUNCES, 0, 0, w, h, None, d_rad.data_ptr(), s, stats=True)
    finally:
        rr.set_option("new_sample", 0)
    rr.render_hits_device(cam, w, h, 0, 0, w, h, d_hits.data_ptr(), s)
    rr.temporal_device(w, h, cam, d_rad.data_ptr(), d_hits.data_ptr(), d_hist.data_ptr(),
                       prev[0] if prev else None, prev[1].data_ptr() if prev else None,
                       prev[2].data_ptr() if prev else None, None, None, tp, s)
    rr.denoise_history_device(w, h, d_hist.data_ptr(), d_hits.data_ptr(), d_ws.data_ptr(), o_rgba.data_ptr(),
                              o_rad.data_ptr(), dp, s)
    torch.cuda.synchronize()
    return o_rgba.cpu().numpy(), o_rad.cpu().numpy(), st, (cam, d_hist, d_hits)


def orbit(w, h, k):
    cam = camera(w, h, orbit=1.0 * k)
    cam.ubo.frame_count = k
    return cam


@pytest.mark.parametrize("accel", [8, 0])
def test_render_temporal_adaptive_is_the_four_calls(accel):
    if not has_gpu():
        pytest.skip("no GPU")
    import torch
    import rtamd
    from rtamd import configs
    w, h = 64, 40
    tp = rtamd.TemporalParams(max_history=8, plane_tol=0.01, normal_min=0.8)
    dp = rtamd.DenoiseParams(iterations=3, normal_power_log2=5, sigma_depth=0.02, sigma_color=1.0)
    with rtamd.Renderer((0,)) as rr:
        rr.set_option("accel", accel)
        rr.upload_scene(configs.config2().build())
        cam0 = camera(w, h)
        rgba0, rad0, _ = rr.render(cam0, w, h, BOUNCES, radiance=True)
        for t_par, d_par in ((None, None), (tp, dp)):
            prev, last = None, None
            for k in range(4):
                cam = orbit(w, h, k)
                want_rgba, want_rad, st0, prev = composed_frame(rr, w, h, cam, prev, t_par, d_par)
                rgba, rad, st = rr.render_temporal(cam, w, h, BOUNCES, t_par, d_par, reset=(k == 0), radiance=True,
                                                   stats=True, adaptive=True)
                assert np.array_equal(rad.view(np.uint32), want_rad.view(np.uint32)), (accel, k)
                assert np.array_equal(rgba, want_rgba), (accel, k)
                for key in ("segments", "node_visits", "tri_tests", "mat_reads", "pixels"):
                    assert st[key] == st0[key], key
                assert st["ms"] > 0
                last = (prev[1].cpu().numpy(), prev[2].cpu().numpy().view(D.HIT_DTYPE).reshape(h, w))
            # the composition is the numpy reference's too, and the filter did something to the last frame
            hist, hits = last
            kw = dict(D.DEFAULTS) if d_par is None else dict(iterations=3, normal_power_log2=5, sigma_depth=0.02,
                                                             sigma_color=1.0)
            ref_rad, ref_rgba = A.denoise_history(hist, hits, **kw)
            assert np.array_equal(rad.view(np.uint32), ref_rad.view(np.uint32)) and np.array_equal(rgba, ref_rgba)
            assert (hist[..., 3] > 1).any() and (rad != np.sqrt(hist[..., :3])).any()
        # RGBA only, no stats
        got = rr.render_temporal(orbit(w, h, 4), w, h, BOUNCES, tp, dp, adaptive=True)
        assert got[1] is None and got[2] is None
        # a sequence that alternates the two calls keeps one history
        prev = None
        for k in range(4):
            cam = orbit(w, h, k)
            want_rgba, want_rad, _, prev = composed_frame(rr, w, h, cam, prev, tp, dp)
            if k % 2:
                rgba, rad, _ = rr.render_temporal(cam, w, h, BOUNCES, tp, dp, radiance=True, adaptive=True)
                assert np.array_equal(rad.view(np.uint32), want_rad.view(np.uint32)), k
                assert np.array_equal(rgba, want_rgba), k
            else:
                rgba, rad, _ = rr.render_temporal(cam, w, h, BOUNCES, tp, reset=(k == 0), radiance=True)
                assert np.array_equal(rad.view(np.uint32), np.sqrt(prev[1].cpu().numpy()[..., :3]).view(np.uint32)), k
        assert (prev[1].cpu().numpy()[..., 3] == 4).any()
        # the render state is an ordinary render's: the same frame afterwards
        rgba1, rad1, _ = rr.render(cam0, w, h, BOUNCES, radiance=True)
        assert np.array_equal(rgba1, rgba0) and np.array_equal(rad1.view(np.uint32), rad0.view(np.uint32))
        assert rr.get_option("extensions") == 0 and rr.get_option("new_sample") == 0
        # plain_kernels counts the render's kernels only: a warmed adaptive frame adds what a warmed tile adds
        d_rad = torch.empty((h, w, 3), dtype=torch.float32, device="cuda:0")
        for _ in range(3):
            rr.render_temporal(cam0, w, h, BOUNCES, fixed_seed=True, adaptive=True)
        k0 = rr.get_option("plain_kernels")
        rr.render_tile_device(cam0, w, h, BOUNCES, 0, 0, w, h, None, d_rad.data_ptr(), None)
        torch.cuda.synchronize()
        k1 = rr.get_option("plain_kernels")
        rr.render_temporal(cam0, w, h, BOUNCES, fixed_seed=True, adaptive=True)
        k2 = rr.get_option("plain_kernels")
        assert k1 - k0 >= 1 and k2 - k1 == k1 - k0


def test_render_temporal_adaptive_refusals(r):
    import rtamd
    from rtamd import RtError, configs
    w, h = 64, 40
    cam = configs.Camera.default(w, h)
    r.render_temporal(cam, w, h, BOUNCES, adaptive=True)
    for kw in (dict(params=rtamd.TemporalParams(max_history=0)), dict(params=rtamd.TemporalParams(plane_tol=-1.0)),
               dict(denoise=rtamd.DenoiseParams(iterations=9))):
        with pytest.raises(RtError, match="INVALID_ARG.*rt_render_temporal_adaptive"):
            r.render_temporal(cam, w, h, BOUNCES, adaptive=True, **kw)
    with pytest.raises(RtError, match="INVALID_ARG"):
        r.render_temporal(cam, 0, h, BOUNCES, adaptive=True)
    out = np.zeros((h, w, 4), np.uint8)
    L = rtamd.lib()
    ubo = C.byref(cam.ubo)
    assert L.rt_render_temporal_adaptive(r._ctx, ubo, w, h, BOUNCES, None, None, 0, None, None, None) == -1
    assert L.rt_render_temporal_adaptive(None, ubo, w, h, BOUNCES, None, None, 0, out.ctypes.data, None, None) == -1
    assert L.rt_render_temporal_adaptive(r._ctx, ubo, w, h, BOUNCES, None, None, 4, out.ctypes.data, None, None) == -1
    assert b"rt_render_temporal_adaptive: unknown flags" in L.rt_last_error()
    r.set_option("extensions", 4)
    try:
        with pytest.raises(RtError, match="INVALID_ARG.*rt_render_temporal_adaptive.*bit 4"):
            r.render_temporal(cam, w, h, BOUNCES, adaptive=True)
    finally:
        r.set_option("extensions", 0)
    r.upload_spheres([[0.0, 5.0, 0.0, 4.0, 0.9, 0.2, 0.2, 0.0]])
    try:
        r.render_temporal(cam, w, h, BOUNCES, adaptive=True)     # bit 8 off: triangles only, accepted
        r.set_option("extensions", 8)
        with pytest.raises(RtError, match="INVALID_ARG.*rt_render_temporal_adaptive.*spheres"):
            r.render_temporal(cam, w, h, BOUNCES, adaptive=True)
    finally:
        r.set_option("extensions", 0)
        r.upload_spheres(np.zeros((0, 8), np.float32))
    with rtamd.Renderer((0, 0)) as rr:               # the same ordinal twice serves as two devices
        rr.upload_scene(configs.config2().build())
        with pytest.raises(RtError, match="INVALID_ARG.*devices"):
            rr.render_temporal(cam, w, h, BOUNCES, adaptive=True)


def test_engine_with_the_adaptive_filter():
    """HipEngine(adaptive=True) publishes rt_render_temporal_adaptive's frames, frame k with frame_count k."""
    if not has_gpu():
        pytest.skip("no GPU")
    import time
    import rtamd
    from rtamd import configs
    w, h = 96, 54
    built = configs.config2().build()
    cam = configs.Camera.default(w, h)
    want, plain = [], []
    with rtamd.Renderer((0,)) as rr:
        rr.upload_scene(built)
        for k in range(3):
            cam.ubo.frame_count = k
            want.append(rr.render_temporal(cam, w, h, BOUNCES, adaptive=True)[0])
        for k in range(3):
            cam.ubo.frame_count = k
            plain.append(rr.render_temporal(cam, w, h, BOUNCES, reset=(k == 0))[0])
    cam.ubo.frame_count = 0
    assert (want[2] != plain[2]).any()               # the switch changes what is shown

    class Recording(rtamd.AtomicReference):
        def __init__(self):
            super().__init__()
            self.frames = []

        def set(self, v):
            self.frames.append(v)
            super().set(v)

    q = Recording()
    eng = rtamd.HipEngine(q, w, h, BOUNCES, adaptive=True)
    assert not eng.pipelined and eng.temporal is not None
    eng.start()
    try:
        eng.submit_scene(built)
        eng.submit_camera_update(cam)
        deadline = time.time() + 30.0
        while len(q.frames) < 3 and eng.error is None and time.time() < deadline:
            time.sleep(0.005)
    finally:
        eng.stop()
    assert eng.error is None, eng.error
    assert len(q.frames) >= 3 and eng.temporal_frames >= 3
    for k in range(3):
        assert np.array_equal(q.frames[k].pixel_data, want[k]), k
