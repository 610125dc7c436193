"""rt_denoise_device / rt_render_denoised on the GPU: radiance bits and RGBA8
equal tests/denoise_ref.py (the numpy restatement of DESIGN.md §4g) on rendered
and on synthetic guides, at ragged sizes, for every pass count, with both
kernel forms forced (option denoise_kernel); buffers past the outputs stay
untouched; argument errors; rt_render_denoised = render + render_hits + filter
and leaves the render state as an ordinary render does."""
import ctypes as C

import numpy as np
import pytest

import denoise_ref as D
from conftest import has_gpu
from test_denoise_ref import random_frame

pytestmark = pytest.mark.gpu

GUARD = 256           # bytes around every device buffer (keeps the 16-byte alignment)
FORMS = (0, 1, 2)     # option denoise_kernel: the shipped choice, plain, tiled


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


class Guarded:
    """A device buffer of n bytes with GUARD bytes of 0xEE before and after."""

    def __init__(self, n, fill=None):
        import torch
        self.n = n
        self.t = torch.full((n + 2 * GUARD,), 0xEE, dtype=torch.uint8, device="cuda:0")
        if fill is not None:
            self.t[GUARD:GUARD + n] = torch.from_numpy(np.frombuffer(fill.tobytes(), np.uint8).copy()).cuda()
        self.ptr = self.t.data_ptr() + GUARD
        assert self.ptr % 16 == 0

    def host(self, dtype, shape):
        return self.t[GUARD:GUARD + self.n].cpu().numpy().view(dtype).reshape(shape)

    def guards_intact(self):
        h = self.t.cpu().numpy()
        return bool((h[:GUARD] == 0xEE).all() and (h[GUARD + self.n:] == 0xEE).all())


def run(r, rad, hits, params=None, form=0, rgba=True, radiance=True):
    """rt_denoise_device on host arrays through guarded device buffers:
    (rgba or None, radiance or None); asserts that nothing outside the outputs
    and the workspace was written and that the inputs are unchanged."""
    import torch
    h, w = rad.shape[:2]
    rad = np.ascontiguousarray(rad, np.float32)
    hits = np.ascontiguousarray(hits)
    d_rad, d_hit = Guarded(w * h * 12, rad), Guarded(w * h * 32, hits)
    d_ws = Guarded(r.denoise_workspace_bytes(w, h))
    o_rgba = Guarded(w * h * 4) if rgba else None
    o_rad = Guarded(w * h * 12) if radiance else None
    r.set_option("denoise_kernel", form)
    try:
        r.denoise_device(w, h, d_rad.ptr, d_hit.ptr, d_ws.ptr, o_rgba.ptr if rgba else None,
                         o_rad.ptr if radiance else None, params, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    finally:
        r.set_option("denoise_kernel", 0)
    for b in (d_rad, d_hit, d_ws, o_rgba, o_rad):
        assert b is None or b.guards_intact()
    assert d_rad.host(np.uint8, -1).tobytes() == rad.tobytes() and d_hit.host(np.uint8, -1).tobytes() == hits.tobytes()
    return (o_rgba.host(np.uint8, (h, w, 4)) if rgba else None,
            o_rad.host(np.float32, (h, w, 3)) if radiance else None)


def check(r, rad, hits, kw, forms=FORMS):
    import rtamd
    want_rad, want_rgba = D.denoise(rad, hits, **{**D.DEFAULTS, **kw})
    params = rtamd.DenoiseParams(**{**D.DEFAULTS, **kw})
    for form in forms:
        rgba, out = run(r, rad, hits, params, form)
        diff = out.view(np.uint32) != want_rad.view(np.uint32)
        assert not diff.any(), (form, kw, int(diff.sum()), np.argwhere(diff)[:4].tolist())
        assert np.array_equal(rgba, want_rgba), (form, kw)
    return want_rad


@pytest.fixture(scope="module")
def rendered(r):
    """Config 2 on the GPU at two ragged sizes: radiance and first-hit records."""
    from rtamd import configs
    out = {}
    for w, h in ((37, 23), (129, 65)):
        cam = configs.Camera.default(w, h)
        _, rad, _ = r.render(cam, w, h, 4, radiance=True)
        hits = r.render_hits(cam, w, h)
        assert (hits["tri"] >= 0).any() and (hits["tri"] < 0).any()
        out[(w, h)] = (rad, hits)
    return out


@pytest.mark.parametrize("size", [(37, 23), (129, 65)])
def test_rendered_frames_equal_the_reference(r, rendered, size):
    rad, hits = rendered[size]
    for kw in ({}, {"iterations": 6}):              # at 6 passes the step reaches 32: past 37x23's height
        out = check(r, rad, hits, kw)
        assert (out != rad).any()                   # the filter changed hit pixels
        sky = hits["tri"] < 0
        assert np.array_equal(out[sky].view(np.uint32), rad[sky].view(np.uint32))


@pytest.mark.parametrize("w,h", [(1, 1), (3, 70), (70, 3)])
def test_degenerate_sizes(r, w, h):
    rad, hits = random_frame(h, w, seed=w * 100 + h, nan_normals=1)
    hits["tri"][0, 0] = 5                           # at least one pixel with a hit
    for kw in ({}, {"iterations": 6}, {"iterations": 1, "normal_power_log2": 0, "sigma_depth": 50.0}):
        check(r, rad, hits, kw)


@pytest.fixture(scope="module")
def synthetic():
    return random_frame(41, 67, seed=2024, nan_normals=5)


@pytest.mark.parametrize("iterations", [1, 2, 3, 4, 5, 6])
def test_every_pass_count_on_synthetic_guides(r, synthetic, iterations):
    rad, hits = synthetic
    check(r, rad, hits, {"iterations": iterations})
    # wide sigmas and power 0: every tap with a hit carries weight
    out = check(r, rad, hits, {"iterations": iterations, "normal_power_log2": 0, "sigma_depth": 50.0,
                               "sigma_color": 4.0})
    hit = (hits["tri"] >= 0) & np.isfinite(hits["normal"]).all(-1)
    assert (out[hit] != rad[hit]).mean() > 0.9


def test_default_params_are_the_null_pointer(r, synthetic):
    rad, hits = synthetic
    want_rad, want_rgba = D.denoise(rad, hits)
    rgba, out = run(r, rad, hits, None)
    assert np.array_equal(out.view(np.uint32), want_rad.view(np.uint32)) and np.array_equal(rgba, want_rgba)
    import rtamd
    q = rtamd.DenoiseParams(1, 1, 1.0, 1.0)
    rtamd.lib().rt_denoise_default_params(C.byref(q))
    assert (q.iterations, q.normal_power_log2, q.sigma_depth, q.sigma_color) == (4, 7, np.float32(0.005), 0.5)
    assert rtamd.lib().rt_denoise_workspace_bytes(67, 41) == 2 * 67 * 41 * 16
    assert rtamd.lib().rt_denoise_workspace_bytes(0, 41) == 0 and rtamd.lib().rt_denoise_workspace_bytes(67, -1) == 0
    assert rtamd.lib().rt_denoise_workspace_bytes(1 << 16, 1 << 16) == 0


@pytest.mark.parametrize("form", [1, 2])
def test_single_outputs(r, synthetic, form):
    rad, hits = synthetic
    want_rad, want_rgba = D.denoise(rad, hits)
    rgba, none = run(r, rad, hits, None, form, rgba=True, radiance=False)
    assert none is None and np.array_equal(rgba, want_rgba)
    none, out = run(r, rad, hits, None, form, rgba=False, radiance=True)
    assert none is None and np.array_equal(out.view(np.uint32), want_rad.view(np.uint32))


@pytest.mark.parametrize("form", [1, 2])
def test_lone_passes_on_one_workspace(r, rendered, form):
    """Option denoise_pass: passes 0, 1 and 2 of a 3-pass filter, each enqueued
    alone on one workspace (steps 1, 2 and 4; at 37x23 a step-4 residue class
    ends inside the first tile), leave what the whole filter leaves; a pass
    that is not the last writes neither output."""
    import torch
    import rtamd
    rad, hits = rendered[(37, 23)]
    h, w = rad.shape[:2]
    rad, hits = np.ascontiguousarray(rad, np.float32), np.ascontiguousarray(hits)
    kw = {**D.DEFAULTS, "iterations": 3}
    params = rtamd.DenoiseParams(**kw)
    want_rad, want_rgba = D.denoise(rad, hits, **kw)
    whole_rgba, whole_rad = run(r, rad, hits, params, form)
    d_rad, d_hit = Guarded(w * h * 12, rad), Guarded(w * h * 32, hits)
    d_ws, o_rgba, o_rad = Guarded(r.denoise_workspace_bytes(w, h)), Guarded(w * h * 4), Guarded(w * h * 12)
    r.set_option("denoise_kernel", form)
    try:
        for i in range(3):
            r.set_option("denoise_pass", i)
            r.denoise_device(w, h, d_rad.ptr, d_hit.ptr, d_ws.ptr, o_rgba.ptr, o_rad.ptr, params,
                             torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            if i < 2:
                assert (o_rgba.host(np.uint8, -1) == 0xEE).all() and (o_rad.host(np.uint8, -1) == 0xEE).all(), i
    finally:
        r.set_option("denoise_pass", -1)
        r.set_option("denoise_kernel", 0)
    for b in (d_rad, d_hit, d_ws, o_rgba, o_rad):
        assert b.guards_intact()
    rgba, out = o_rgba.host(np.uint8, (h, w, 4)), o_rad.host(np.float32, (h, w, 3))
    assert np.array_equal(out.view(np.uint32), whole_rad.view(np.uint32)) and np.array_equal(rgba, whole_rgba)
    assert np.array_equal(out.view(np.uint32), want_rad.view(np.uint32)) and np.array_equal(rgba, want_rgba)


def test_host_array_form(r, rendered):
    rad, hits = rendered[(37, 23)]
    want_rad, want_rgba = D.denoise(rad, hits)
    rgba, out = r.denoise(rad, hits)
    assert np.array_equal(out.view(np.uint32), want_rad.view(np.uint32)) and np.array_equal(rgba, want_rgba)


def test_argument_errors(r):
    import torch
    import rtamd
    from rtamd import RtError
    w, h = 16, 8
    n = w * h
    buf = lambda nbytes: torch.zeros(nbytes + 64, dtype=torch.uint8, device="cuda:0")   # noqa: E731
    rad, hit, ws, o1, o2 = buf(n * 12), buf(n * 32), buf(n * 32), buf(n * 4), buf(n * 12)
    good = dict(width=w, height=h, d_radiance=rad.data_ptr(), d_hits=hit.data_ptr(), d_workspace=ws.data_ptr(),
                d_out_rgba=o1.data_ptr(), d_out_radiance=o2.data_ptr(), params=None)
    r.denoise_device(**good)                        # the baseline is accepted
    torch.cuda.synchronize()
    P = rtamd.DenoiseParams
    bad = [
        dict(d_radiance=None), dict(d_hits=None), dict(d_workspace=None),
        dict(d_out_rgba=None, d_out_radiance=None),
        dict(width=0), dict(height=-3), dict(width=1 << 16, height=1 << 16),
        dict(params=P(iterations=0)), dict(params=P(iterations=7)),
        dict(params=P(normal_power_log2=-1)), dict(params=P(normal_power_log2=11)),
        dict(params=P(sigma_depth=0.0)), dict(params=P(sigma_depth=float("nan"))),
        dict(params=P(sigma_color=-1.0)), dict(params=P(sigma_color=float("inf"))),
        dict(d_hits=hit.data_ptr() + 8), dict(d_workspace=ws.data_ptr() + 4), dict(d_radiance=rad.data_ptr() + 2),
        dict(d_out_rgba=rad.data_ptr()), dict(d_out_radiance=hit.data_ptr() + 16),
        dict(d_out_rgba=ws.data_ptr() + n * 16), dict(d_out_radiance=o1.data_ptr()),
        dict(d_workspace=hit.data_ptr()),
    ]
    for kw in bad:
        with pytest.raises(RtError, match="INVALID_ARG.*rt_denoise_device") as ei:
            r.denoise_device(**{**good, **kw})
        assert ei.value.code == -1, kw
    null = C.c_void_p()
    assert rtamd.lib().rt_denoise_device(null, w, h, rad.data_ptr(), hit.data_ptr(), None, ws.data_ptr(),
                                         o1.data_ptr(), None, None, None) == -1
    for name, v in (("denoise_kernel", 3), ("denoise_kernel", -1), ("denoise_pass", 6)):
        with pytest.raises(RtError, match="INVALID_ARG"):
            r.set_option(name, v)
    assert r.get_option("denoise_kernel") == 0 and r.get_option("denoise_pass") == -1


# ---- rt_render_denoised ------------------------------------------------------

@pytest.mark.parametrize("accel", [8, 0])
def test_render_denoised_is_render_hits_and_filter(accel):
    if not has_gpu():
        pytest.skip("no GPU")
    import torch
    import rtamd
    from rtamd import configs
    w, h, bounces = 129, 65, 4
    cam = configs.Camera.default(w, h)
    with rtamd.Renderer((0,)) as rr:
        rr.set_option("accel", accel)
        rr.upload_scene(configs.config2().build())
        rgba0, rad0, st0 = rr.render(cam, w, h, bounces, radiance=True, stats=True)
        hits = rr.render_hits(cam, w, h)
        want_rad, want_rgba = D.denoise(rad0, hits)
        rgba, rad, st = rr.render_denoised(cam, w, h, bounces, radiance=True, stats=True)
        assert np.array_equal(rad.view(np.uint32), want_rad.view(np.uint32)) and np.array_equal(rgba, want_rgba)
        for k in ("segments", "node_visits", "tri_tests", "mat_reads", "pixels"):
            assert st[k] == st0[k], k
        assert st["ms"] > 0
        # other parameters, RGBA only, no stats
        p = rtamd.DenoiseParams(iterations=2, normal_power_log2=3, sigma_depth=0.02, sigma_color=1.0)
        rgba2, none, none2 = rr.render_denoised(cam, w, h, bounces, p)
        assert none is None and none2 is None
        assert np.array_equal(rgba2, D.denoise(rad0, hits, 2, 3, 0.02, 1.0)[1])
        # the render state is an ordinary render's: the same frame afterwards, synchronously and pipelined
        rgba1, rad1, _ = rr.render(cam, w, h, bounces, radiance=True)
        assert np.array_equal(rgba1, rgba0) and np.array_equal(rad1.view(np.uint32), rad0.view(np.uint32))
        from rtamd.engine import PinnedFrame
        frame = PinnedFrame(h, w)
        try:
            rr.wait(rr.render_async(cam, w, h, bounces, frame))
            assert np.array_equal(frame.array, rgba0)
        finally:
            frame.close()
        # plain_kernels counts the render's kernels only: a warmed denoised frame adds what a warmed tile adds
        d_rad = torch.empty((h, w, 3), dtype=torch.float32, device="cuda:0")
        for _ in range(3):
            rr.render_denoised(cam, w, h, bounces)
        k0 = rr.get_option("plain_kernels")
        rr.render_tile_device(cam, w, h, bounces, 0, 0, w, h, None, d_rad.data_ptr(), None)
        torch.cuda.synchronize()
        k1 = rr.get_option("plain_kernels")
        rr.render_denoised(cam, w, h, bounces)
        k2 = rr.get_option("plain_kernels")
        assert k1 - k0 >= 1 and k2 - k1 == k1 - k0
        # a smaller and a larger frame through the same context buffers
        for ww, hh in ((37, 23), (160, 90)):
            c2 = configs.Camera.default(ww, hh)
            _, r2, _ = rr.render(c2, ww, hh, bounces, radiance=True)
            got = rr.render_denoised(c2, ww, hh, bounces, radiance=True)
            assert np.array_equal(got[1].view(np.uint32), D.denoise(r2, rr.render_hits(c2, ww, hh))[0].view(np.uint32))


def test_render_denoised_refusals(r):
    import rtamd
    from rtamd import RtError, configs
    w, h = 64, 40
    cam = configs.Camera.default(w, h)
    with pytest.raises(RtError, match="INVALID_ARG.*rt_render_denoised"):
        r.render_denoised(cam, w, h, 4, rtamd.DenoiseParams(iterations=9))
    with pytest.raises(RtError, match="INVALID_ARG"):
        r.render_denoised(cam, 0, h, 4)
    out = np.zeros((h, w, 4), np.uint8)
    assert rtamd.lib().rt_render_denoised(r._ctx, C.byref(cam.ubo), w, h, 4, None, None, None, None) == -1
    assert rtamd.lib().rt_render_denoised(None, C.byref(cam.ubo), w, h, 4, None, out.ctypes.data, None, None) == -1
    # spheres: refused only while they are uploaded AND the extension is on
    r.upload_spheres([[0.0, 5.0, 0.0, 4.0, 0.9, 0.2, 0.2, 0.0]])
    try:
        r.render_denoised(cam, w, h, 4)             # bit 8 off: triangles only, accepted
        r.set_option("extensions", 8)
        with pytest.raises(RtError, match="INVALID_ARG.*spheres"):
            r.render_denoised(cam, w, h, 4)
        r.upload_spheres(np.zeros((0, 8), np.float32))
        r.render_denoised(cam, w, h, 4)             # bit 8 on, none uploaded: accepted
    finally:
        r.set_option("extensions", 0)
        r.upload_spheres(np.zeros((0, 8), np.float32))


def test_render_denoised_with_accumulation(r):
    """Extension bit 4 is allowed: the filter takes the accumulated radiance."""
    from rtamd import configs
    w, h = 67, 41
    cam = configs.Camera.default(w, h)
    hits = r.render_hits(cam, w, h)
    r.set_option("extensions", 4)
    try:
        for f in range(2):
            cam.ubo.frame_count = f
            _, rad, _ = r.render(cam, w, h, 4, radiance=True)
        for f in range(2):
            cam.ubo.frame_count = f
            got = r.render_denoised(cam, w, h, 4, radiance=True)
    finally:
        r.set_option("extensions", 0)
    want_rad, want_rgba = D.denoise(rad, hits)
    assert np.array_equal(got[1].view(np.uint32), want_rad.view(np.uint32)) and np.array_equal(got[0], want_rgba)


def test_render_denoised_refused_on_two_devices():
    import torch
    if not has_gpu() or torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    import rtamd
    from rtamd import RtError, configs
    w, h = 64, 40
    with rtamd.Renderer((0, 1)) as rr:
        rr.upload_scene(configs.config2().build())
        with pytest.raises(RtError, match="INVALID_ARG.*devices"):
            rr.render_denoised(configs.Camera.default(w, h), w, h, 4)


def test_engine_with_denoise():
    """HipEngine(denoise=...) publishes render_denoised's frames."""
    if not has_gpu():
        pytest.skip("no GPU")
    import time
    import rtamd
    from rtamd import configs
    w, h, bounces = 96, 54, 4
    built = configs.config2().build()
    cam = configs.Camera.default(w, h)
    with rtamd.Renderer((0,)) as rr:
        rr.upload_scene(built)
        want = rr.render_denoised(cam, w, h, bounces)[0]
    q = rtamd.AtomicReference()
    eng = rtamd.HipEngine(q, w, h, bounces, denoise=rtamd.DenoiseParams())
    assert not eng.pipelined
    eng.start()
    try:
        eng.submit_scene(built)
        eng.submit_camera_update(cam)
        deadline = time.time() + 30.0
        while q.get() is None and eng.error is None and time.time() < deadline:
            time.sleep(0.005)
    finally:
        eng.stop()
    assert eng.error is None, eng.error
    assert q.get() is not None and np.array_equal(q.get().pixel_data, want)
