"""Temporal accumulation on the GPU: option new_sample (a new sample per
frame_count and nothing else) equals the oracle's frames through rt_render,
rt_render_tile_device and rt_render_async; rt_temporal_device's history,
radiance bits and RGBA8 equal tests/temporal_ref.py (the numpy restatement of
DESIGN.md §4h) on rendered camera pairs and on synthetic guides, at ragged
sizes, with both lane mappings forced (option temporal_tile); buffers past the
outputs stay untouched; argument errors; rt_render_temporal = render +
render_hits + temporal (+ filter), its history resets, its refusals, and it
leaves the render state as an ordinary render does."""
import ctypes as C

import numpy as np
import pytest

import denoise_ref as D
import temporal_ref as T
from conftest import has_gpu
from test_denoise_ref import random_frame
from test_gpu_denoise import GUARD, Guarded
from test_temporal_ref import look_at, random_camera_pair, random_history

pytestmark = pytest.mark.gpu

F = np.float32
FORMS = (0, 1, 2)     # option temporal_tile: the shipped choice, 64 x 1 waves, 16 x 4 tiles
SIZES = ((37, 23), (129, 65))
BOUNCES = 4


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


def camera(w, h, orbit=0.0, dolly=1.0, vup=(0.0, 1.0, 0.0), away=False):
    """The default camera turned `orbit` degrees about the vertical axis through
    the origin, moved to `dolly` times its distance, rolled by vup, or turned
    to look away from the scene."""
    from rtamd import configs
    a = np.radians(orbit)
    x, y, z = -25.0, 30.0, 140.0
    o = np.array([x * np.cos(a) + z * np.sin(a), y, -x * np.sin(a) + z * np.cos(a)]) * dolly
    return configs.Camera(tuple(o), tuple(2.0 * o) if away else (0.0, 0.0, 0.0), vup, 20.0, float(w) / float(h))


# ---- option new_sample ---------------------------------------------------------

def oracle_sample(built, cam, w, h, k):
    """Frame k's sample by the oracle: extension 4 with a zeroed sum leaves the
    sample's linear colour in it.  (radiance, rgba, counts)."""
    from oracle import oracle_lib
    cam.ubo.frame_count = k
    acc = np.zeros((h, w, 3), F)
    _, _, cnt = oracle_lib.render(built.model_vertex_data, built.model_material_data, built.flat_bvh_data,
                                  cam.ubo_bytes(), w, h, BOUNCES, ext=oracle_lib.EXT_ACCUMULATE, accum=acc)
    rad = np.sqrt(acc)
    return rad, D.unorm8(rad), cnt


@pytest.mark.parametrize("accel", [8, 0])
def test_new_sample_per_frame_count(accel):
    if not has_gpu():
        pytest.skip("no GPU")
    import torch
    import rtamd
    from rtamd import configs
    from rtamd.engine import PinnedFrame
    built = configs.config2().build()
    with rtamd.Renderer((0,)) as rr:
        rr.set_option("accel", accel)
        rr.upload_scene(built)
        for w, h in SIZES:
            cam = configs.Camera.default(w, h)
            plain = rr.render(cam, w, h, BOUNCES, radiance=True, stats=True)
            frame = PinnedFrame(h, w)
            d_rgba = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda:0")
            d_rad = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0")
            rr.set_option("new_sample", 1)
            try:
                for k in (0, 1, 5):
                    want_rad, want_rgba, cnt = oracle_sample(built, cam, w, h, k)
                    cam.ubo.frame_count = k
                    rgba, rad, st = rr.render(cam, w, h, BOUNCES, radiance=True, stats=True)
                    assert np.array_equal(rad.view(np.uint32), want_rad.view(np.uint32)), (accel, w, h, k)
                    assert np.array_equal(rgba, want_rgba), (accel, w, h, k)
                    assert st["segments"] == cnt["segments"] and st["mat_reads"] == cnt["mat_reads"], (accel, w, h, k)
                    if k == 0:                      # frame_count 0 is the reference's frame
                        assert np.array_equal(rgba, plain[0]) and np.array_equal(rad.view(np.uint32), plain[1].view(np.uint32))
                        assert st["segments"] == plain[2]["segments"] and st["mat_reads"] == plain[2]["mat_reads"]
                    else:
                        assert (rgba != plain[0]).any()
                    st2 = rr.render_tile_device(cam, w, h, BOUNCES, 0, 0, w, h, d_rgba.data_ptr(), d_rad.data_ptr(),
                                                torch.cuda.current_stream().cuda_stream, stats=True)
                    torch.cuda.synchronize()
                    assert np.array_equal(d_rgba.cpu().numpy(), want_rgba)
                    assert np.array_equal(d_rad.cpu().numpy().view(np.uint32), want_rad.view(np.uint32))
                    assert st2["segments"] == cnt["segments"] and st2["mat_reads"] == cnt["mat_reads"]
                    rr.wait(rr.render_async(cam, w, h, BOUNCES, frame))
                    assert np.array_equal(frame.array, want_rgba), (accel, w, h, k)
            finally:
                rr.set_option("new_sample", 0)
                frame.close()
            cam.ubo.frame_count = 5                 # the option off: frame_count is ignored again
            assert np.array_equal(rr.render(cam, w, h, BOUNCES)[0], plain[0])


def test_bit_4_with_new_sample_is_bit_4(r):
    from rtamd import configs
    w, h = 67, 41
    cam = configs.Camera.default(w, h)
    frames = {}
    try:
        for ext in (4, 20):                         # 20: bit 4 with option new_sample (the kernels' bit 16)
            r.set_option("extensions", 4)
            r.set_option("new_sample", ext >> 4)
            assert r.get_option("extensions") == 4 and r.get_option("new_sample") == ext >> 4
            out = []
            for f in range(3):
                cam.ubo.frame_count = f
                rgba, rad, _ = r.render(cam, w, h, BOUNCES, radiance=True)
                out.append((rgba, rad))
            frames[ext] = out
    finally:
        r.set_option("extensions", 0)
        r.set_option("new_sample", 0)
    for (a_rgba, a_rad), (b_rgba, b_rad) in zip(frames[4], frames[20]):
        assert np.array_equal(a_rgba, b_rgba) and np.array_equal(a_rad.view(np.uint32), b_rad.view(np.uint32))
    assert (frames[4][2][0] != frames[4][0][0]).any()


def test_new_sample_takes_one_frame_per_launch(r):
    """A launch carries one frame_count: like bit 4, new_sample is refused with several frames."""
    import torch
    from rtamd import RtError, configs
    import rtamd
    w, h = 64, 32
    cams = (rtamd.CameraUBO * 2)(configs.Camera.default(w, h).ubo, configs.Camera.default(w, h).ubo)
    d = torch.zeros((2, h, w, 4), dtype=torch.uint8, device="cuda:0")
    args = (r._ctx, cams, 2, w, h, BOUNCES, 16, None, 0, d.data_ptr(), None, None, None)
    assert rtamd.lib().rt_render_batch_device(*args) == 0
    torch.cuda.synchronize()
    r.set_option("new_sample", 1)
    try:
        assert rtamd.lib().rt_render_batch_device(*args) == -1
        assert b"one frame per launch" in rtamd.lib().rt_last_error()
        assert rtamd.lib().rt_render_batch_device(r._ctx, cams, 1, w, h, BOUNCES, 16, None, 0, d.data_ptr(), None, None,
                                                  None) == 0
        torch.cuda.synchronize()
    finally:
        r.set_option("new_sample", 0)
    for v in (2, -1):
        with pytest.raises(RtError, match="INVALID_ARG"):
            r.set_option("new_sample", v)
    assert r.get_option("new_sample") == 0


# ---- rt_temporal_device -------------------------------------------------------

def run(r, rad, hits, cam, prev=None, params=None, form=0, rgba=True, radiance=True):
    """rt_temporal_device on host arrays through guarded device buffers; prev =
    (camera bytes, history, hit records) or None.  Returns (history, rgba or
    None, radiance or None); asserts that nothing outside the outputs was
    written and that the inputs are unchanged."""
    import torch
    h, w = rad.shape[:2]
    rad = np.ascontiguousarray(rad, F)
    hits = np.ascontiguousarray(hits)
    d_rad, d_hit = Guarded(w * h * 12, rad), Guarded(w * h * 32, hits)
    ins = [(d_rad, rad), (d_hit, hits)]
    d_hp = d_hq = None
    if prev is not None:
        hist_prev, hits_prev = np.ascontiguousarray(prev[1], F), np.ascontiguousarray(prev[2])
        d_hp, d_hq = Guarded(w * h * 16, hist_prev), Guarded(w * h * 32, hits_prev)
        ins += [(d_hp, hist_prev), (d_hq, hits_prev)]
    o_hist = Guarded(w * h * 16)
    o_rgba = Guarded(w * h * 4) if rgba else None
    o_rad = Guarded(w * h * 12) if radiance else None
    r.set_option("temporal_tile", form)
    try:
        r.temporal_device(w, h, cam, d_rad.ptr, d_hit.ptr, o_hist.ptr, prev[0] if prev is not None else None,
                          d_hp.ptr if d_hp else None, d_hq.ptr if d_hq else None, o_rgba.ptr if rgba else None,
                          o_rad.ptr if radiance else None, params, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    finally:
        r.set_option("temporal_tile", 0)
    for b in (d_rad, d_hit, d_hp, d_hq, o_hist, o_rgba, o_rad):
        assert b is None or b.guards_intact()
    for buf, host in ins:
        assert buf.host(np.uint8, -1).tobytes() == host.tobytes()
    return (o_hist.host(F, (h, w, 4)), o_rgba.host(np.uint8, (h, w, 4)) if rgba else None,
            o_rad.host(F, (h, w, 3)) if radiance else None)


def check(r, rad, hits, cam, prev=None, kw=None, forms=FORMS):
    """Every form equals the reference bit for bit; returns the reference's (history, reused mask)."""
    import rtamd
    kw = {**T.DEFAULTS, **(kw or {})}
    p = prev if prev is not None else (None, None, None)
    want_hist, want_rad, want_rgba, reused = T.temporal(rad, hits, cam, p[0], p[1], p[2], **kw)
    params = rtamd.TemporalParams(**kw)
    for form in forms:
        hist, rgba, out = run(r, rad, hits, cam, prev, params, form)
        diff = hist.view(np.uint32) != want_hist.view(np.uint32)
        assert not diff.any(), (form, kw, int(diff.sum()), np.argwhere(diff)[:4].tolist())
        assert np.array_equal(out.view(np.uint32), want_rad.view(np.uint32)), (form, kw)
        assert np.array_equal(rgba, want_rgba), (form, kw)
    return want_hist, reused


@pytest.fixture(scope="module")
def rendered(r):
    """Config 2 on the GPU at two ragged sizes: the default camera's frame, its
    first-hit records and its first-frame history."""
    out = {}
    for w, h in SIZES:
        cam = camera(w, h)
        _, rad, _ = r.render(cam, w, h, BOUNCES, radiance=True)
        hits = r.render_hits(cam, w, h)
        assert (hits["tri"] >= 0).any() and (hits["tri"] < 0).any()
        hist, _ = check(r, rad, hits, cam.ubo_bytes())          # null prev_*: a first frame
        assert np.array_equal(hist[..., 3], np.where(hits["tri"] >= 0, 1.0, 0.0))
        out[(w, h)] = (cam.ubo_bytes(), hist, hits)
    return out


PAIRS = {"orbit1": dict(orbit=1.0), "orbit3": dict(orbit=3.0), "dolly": dict(dolly=0.93),
         "roll": dict(vup=(0.12, 1.0, 0.0)), "identical": dict()}


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("pair", sorted(PAIRS))
def test_rendered_camera_pairs_equal_the_reference(r, rendered, size, pair):
    w, h = size
    prev = rendered[size]
    cam = camera(w, h, **PAIRS[pair])
    cam.ubo.frame_count = 1
    r.set_option("new_sample", 1)
    try:
        _, rad, _ = r.render(cam, w, h, BOUNCES, radiance=True)
    finally:
        r.set_option("new_sample", 0)
    hits = r.render_hits(cam, w, h)
    hist, reused = check(r, rad, hits, cam.ubo_bytes(), prev)
    hit = hits["tri"] >= 0
    share = float(reused[hit].mean())
    print(f"{pair} {w}x{h}: {share:.3f} of the hit pixels reuse history")
    if pair == "orbit1":
        assert share >= 0.5                                     # the gather path is really compared
    if pair == "identical":
        assert reused[hit].all() and (hist[..., 3][hit] == 2).all()
    assert (hist[..., 3][~hit] == 0).all()


@pytest.mark.parametrize("size", SIZES)
def test_a_previous_camera_turned_away_reuses_nothing(r, rendered, size):
    w, h = size
    cam_bytes, hist_prev, hits = rendered[size]
    rad = np.random.default_rng(w).uniform(0.0, 1.2, size=(h, w, 3)).astype(F)
    away = camera(w, h, away=True).ubo_bytes()
    hist, reused = check(r, rad, hits, cam_bytes, (away, hist_prev, hits))
    assert not reused.any()
    assert np.array_equal(hist[..., :3].view(np.uint32), (rad * rad).view(np.uint32))


def synthetic_pair(h, w, seed):
    """Random guides of two frames that mostly see the same surfaces, a random
    history with a third of its records empty, a random camera pair."""
    rng = np.random.default_rng(seed)
    rad, hits = random_frame(h, w, seed=seed, nan_normals=5)
    _, hits_prev = random_frame(h, w, seed=seed + 1000, nan_normals=5)
    same = rng.random((h, w)) < 0.6
    hits_prev["normal"][same] = hits["normal"][same]
    hits_prev["pos"][same] = hits["pos"][same] + rng.normal(size=(int(same.sum()), 3)).astype(F) * F(1e-3)
    cam, prev_cam = random_camera_pair(rng)
    return rad, hits, cam, (prev_cam, random_history(h, w, rng), hits_prev)


@pytest.mark.parametrize("kw", [dict(), dict(max_history=1), dict(max_history=2, plane_tol=50.0, normal_min=-1.0),
                                dict(max_history=1024, plane_tol=0.5, normal_min=0.0)],
                         ids=["defaults", "history1", "history2-wide", "history1024"])
def test_synthetic_guides(r, kw):
    reused_any = 0
    for seed in (2024, 2025):
        rad, hits, cam, prev = synthetic_pair(41, 67, seed)
        hist, reused = check(r, rad, hits, cam, prev, kw)
        reused_any += int(reused.sum())
        if kw.get("max_history") == 1:
            assert (hist[..., 3][reused] == 1).all()
    assert reused_any > 40


@pytest.mark.parametrize("w,h", [(1, 1), (3, 70), (70, 3)])
def test_degenerate_sizes(r, w, h):
    rad, hits, cam, prev = synthetic_pair(h, w, seed=w * 100 + h)
    hits["tri"][0, 0] = 5                           # at least one pixel with a hit
    check(r, rad, hits, cam)
    check(r, rad, hits, cam, prev)
    check(r, rad, hits, cam, prev, dict(max_history=2, plane_tol=50.0, normal_min=-1.0))
    # an unmoved camera on its own guides: every valid pixel reuses its own record
    cam0 = look_at((3.0, 4.0, 40.0))
    _, reused = check(r, rad, hits, cam0, (cam0, prev[1], hits))
    ok = (hits["tri"] >= 0) & np.isfinite(hits["normal"]).all(-1) & (prev[1][..., 3] > 0)
    assert np.array_equal(reused, ok)


@pytest.mark.parametrize("form", [1, 2])
def test_single_outputs_and_default_params(r, form):
    rad, hits, cam, prev = synthetic_pair(41, 67, seed=77)
    want_hist, want_rad, want_rgba, _ = T.temporal(rad, hits, cam, *prev)
    hist, rgba, none = run(r, rad, hits, cam, prev, None, form, rgba=True, radiance=False)     # params NULL
    assert none is None and np.array_equal(rgba, want_rgba)
    assert np.array_equal(hist.view(np.uint32), want_hist.view(np.uint32))
    hist, none, out = run(r, rad, hits, cam, prev, None, form, rgba=False, radiance=True)
    assert none is None and np.array_equal(out.view(np.uint32), want_rad.view(np.uint32))
    hist, none, none2 = run(r, rad, hits, cam, prev, None, form, rgba=False, radiance=False)
    assert none is None and none2 is None and np.array_equal(hist.view(np.uint32), want_hist.view(np.uint32))


def test_host_array_form(r, rendered):
    w, h = 37, 23
    prev = rendered[(w, h)]
    cam = camera(w, h, orbit=1.0)
    _, rad, _ = r.render(cam, w, h, BOUNCES, radiance=True)
    hits = r.render_hits(cam, w, h)
    want = T.temporal(rad, hits, cam.ubo_bytes(), *prev)
    hist, rgba, out = r.temporal(rad, hits, cam, *prev)
    assert np.array_equal(hist.view(np.uint32), want[0].view(np.uint32))
    assert np.array_equal(out.view(np.uint32), want[1].view(np.uint32)) and np.array_equal(rgba, want[2])
    first = r.temporal(rad, hits, cam)
    assert np.array_equal(first[0].view(np.uint32), T.temporal(rad, hits)[0].view(np.uint32))


@pytest.mark.parametrize("form", FORMS)
def test_a_four_frame_chain_through_ping_ponged_buffers(r, form):
    """Two history / hit buffer pairs on the device take turns, as rt_render_temporal's do."""
    import torch
    import rtamd
    w, h = 129, 65
    d_hist = [Guarded(w * h * 16), Guarded(w * h * 16)]
    d_hits = [Guarded(w * h * 32), Guarded(w * h * 32)]
    o_rad = Guarded(w * h * 12)
    params = rtamd.TemporalParams(max_history=3)
    want = prev_cam = prev_hits = None
    r.set_option("temporal_tile", form)
    try:
        for k in range(4):
            cam = camera(w, h, orbit=1.0 * k)
            cam.ubo.frame_count = k
            _, rad, _ = r.render(cam, w, h, BOUNCES, radiance=True)
            hits = r.render_hits(cam, w, h)
            cur = k & 1
            d_rad = Guarded(w * h * 12, rad)
            d_hits[cur].t[GUARD:GUARD + w * h * 32] = torch.from_numpy(np.frombuffer(hits.tobytes(), np.uint8).copy()).cuda()
            r.temporal_device(w, h, cam, d_rad.ptr, d_hits[cur].ptr, d_hist[cur].ptr, prev_cam,
                              d_hist[1 - cur].ptr if k else None, d_hits[1 - cur].ptr if k else None, None, o_rad.ptr,
                              params, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            want = T.temporal(rad, hits, cam.ubo_bytes(), prev_cam, want[0] if want else None, prev_hits, max_history=3)
            got = d_hist[cur].host(F, (h, w, 4))
            assert np.array_equal(got.view(np.uint32), want[0].view(np.uint32)), (form, k)
            assert np.array_equal(o_rad.host(F, (h, w, 3)).view(np.uint32), want[1].view(np.uint32)), (form, k)
            prev_cam, prev_hits = cam.ubo_bytes(), hits
            for b in d_hist + d_hits + [o_rad, d_rad]:
                assert b.guards_intact()
    finally:
        r.set_option("temporal_tile", 0)
    n = want[0][..., 3]
    assert n.max() == 3 and (n == 2).any()                  # min(n' + 1, max_history) was reached


def test_argument_errors(r):
    import torch
    import rtamd
    from rtamd import RtError, configs
    w, h = 16, 8
    n = w * h
    buf = lambda nbytes: torch.zeros(nbytes + 64, dtype=torch.uint8, device="cuda:0")   # noqa: E731
    rad, hit, hp, hq, oh, o1, o2 = buf(n * 12), buf(n * 32), buf(n * 16), buf(n * 32), buf(n * 16), buf(n * 4), buf(n * 12)
    cam = configs.Camera.default(w, h)
    good = dict(width=w, height=h, camera=cam, d_radiance=rad.data_ptr(), d_hits=hit.data_ptr(),
                d_hist_out=oh.data_ptr(), prev_camera=cam, d_hist_prev=hp.data_ptr(), d_hits_prev=hq.data_ptr(),
                d_out_rgba=o1.data_ptr(), d_out_radiance=o2.data_ptr(), params=None)
    r.temporal_device(**good)                       # the baseline is accepted
    r.temporal_device(**{**good, "prev_camera": None, "d_hist_prev": None, "d_hits_prev": None,
                         "d_out_rgba": None, "d_out_radiance": None})
    torch.cuda.synchronize()
    P = rtamd.TemporalParams
    bad = [
        dict(camera=None), dict(d_radiance=None), dict(d_hits=None), dict(d_hist_out=None),
        dict(prev_camera=None), dict(d_hist_prev=None), dict(d_hits_prev=None),
        dict(prev_camera=None, d_hist_prev=None), dict(d_hist_prev=None, d_hits_prev=None),
        dict(width=0), dict(height=-3), dict(width=1 << 16, height=1 << 16),
        dict(params=P(max_history=0)), dict(params=P(max_history=1025)),
        dict(params=P(plane_tol=0.0)), dict(params=P(plane_tol=float("nan"))), dict(params=P(plane_tol=float("inf"))),
        dict(params=P(normal_min=1.5)), dict(params=P(normal_min=-2.0)), dict(params=P(normal_min=float("nan"))),
        dict(d_hits=hit.data_ptr() + 8), dict(d_hits_prev=hq.data_ptr() + 8), dict(d_hist_prev=hp.data_ptr() + 4),
        dict(d_hist_out=oh.data_ptr() + 8), dict(d_radiance=rad.data_ptr() + 2), dict(d_out_rgba=o1.data_ptr() + 1),
        dict(d_out_radiance=o2.data_ptr() + 2),
        dict(d_hist_out=hp.data_ptr()), dict(d_hist_out=hp.data_ptr() + 16), dict(d_hist_out=hit.data_ptr()),
        dict(d_hist_out=hq.data_ptr() + n * 16), dict(d_hist_out=rad.data_ptr()),
        dict(d_out_rgba=rad.data_ptr()), dict(d_out_rgba=hp.data_ptr()), dict(d_out_radiance=hit.data_ptr() + 16),
        dict(d_out_radiance=hq.data_ptr()), dict(d_out_rgba=oh.data_ptr()), dict(d_out_radiance=oh.data_ptr() + 4),
        dict(d_out_radiance=o1.data_ptr()),
    ]
    for kw in bad:
        with pytest.raises(RtError, match="INVALID_ARG.*rt_temporal_device") as ei:
            r.temporal_device(**{**good, **kw})
        assert ei.value.code == -1, kw
    null = C.c_void_p()
    assert rtamd.lib().rt_temporal_device(null, w, h, C.byref(cam.ubo), rad.data_ptr(), hit.data_ptr(), None, None, None,
                                          None, oh.data_ptr(), None, None, None, None) == -1
    assert b"rt_temporal_device" in rtamd.lib().rt_last_error()
    for v in (3, -1):
        with pytest.raises(RtError, match="INVALID_ARG"):
            r.set_option("temporal_tile", v)
    assert r.get_option("temporal_tile") == 0


# ---- rt_render_temporal -------------------------------------------------------

def orbit_frames(rr, w, h, n, new_sample):
    """The n frames of a 1-degree orbit as ordinary renders with option
    new_sample as given (frame k with frame_count k): [(camera, radiance, rgba, stats, hits)]."""
    out = []
    rr.set_option("new_sample", new_sample)
    try:
        for k in range(n):
            cam = camera(w, h, orbit=1.0 * k)
            cam.ubo.frame_count = k
            rgba, rad, st = rr.render(cam, w, h, BOUNCES, radiance=True, stats=True)
            out.append((cam, rad, rgba, st))
    finally:
        rr.set_option("new_sample", 0)
    return [f + (rr.render_hits(f[0], w, h),) for f in out]


@pytest.mark.parametrize("accel", [8, 0])
def test_render_temporal_is_render_hits_and_temporal(accel):
    if not has_gpu():
        pytest.skip("no GPU")
    import torch
    import rtamd
    from rtamd import configs
    from rtamd.engine import PinnedFrame
    w, h = 129, 65
    built = configs.config2().build()
    tp = rtamd.TemporalParams(max_history=3, plane_tol=0.01, normal_min=0.8)
    tkw = dict(max_history=3, plane_tol=0.01, normal_min=0.8)
    dp = rtamd.DenoiseParams(iterations=2)
    with rtamd.Renderer((0,)) as rr:
        rr.set_option("accel", accel)
        rr.upload_scene(built)
        cam0 = camera(w, h)
        rgba0, rad0, _ = rr.render(cam0, w, h, BOUNCES, radiance=True)
        frame = PinnedFrame(h, w)
        try:
            rr.wait(rr.render_async(cam0, w, h, BOUNCES, frame))
            assert np.array_equal(frame.array, rgba0)
            new_sample, fixed = orbit_frames(rr, w, h, 4, 1), orbit_frames(rr, w, h, 4, 0)
            assert (new_sample[2][1] != fixed[2][1]).any()
            for frames, kwargs, t_kw, t_par in ((new_sample, {}, T.DEFAULTS, None), (new_sample, dict(denoise=dp), tkw, tp),
                                                (fixed, dict(fixed_seed=True), tkw, tp)):
                hist = prev_cam = prev_hits = None
                for k, (cam, rad, _, st0, hits) in enumerate(frames):
                    hist, want_rad, want_rgba, reused = T.temporal(rad, hits, cam.ubo_bytes(), prev_cam, hist, prev_hits,
                                                                   **t_kw)
                    if "denoise" in kwargs:                 # the filter follows; the history stays unfiltered
                        want_rad, want_rgba = D.denoise(want_rad, hits, iterations=2)
                    rgba, out, st = rr.render_temporal(cam, w, h, BOUNCES, t_par, reset=(k == 0), radiance=True,
                                                       stats=True, **kwargs)
                    assert np.array_equal(out.view(np.uint32), want_rad.view(np.uint32)), (accel, kwargs, k)
                    assert np.array_equal(rgba, want_rgba), (accel, kwargs, k)
                    for key in ("segments", "node_visits", "tri_tests", "mat_reads", "pixels"):
                        assert st[key] == st0[key], key
                    assert st["ms"] > 0
                    if k:
                        assert reused.any() and (out != rad).any()
                    prev_cam, prev_hits = cam.ubo_bytes(), hits
            # RGBA only, no stats: the frame after the last sequence's, then a reset by the flag
            cam, rad, rgba_raw, _, hits = fixed[3]
            got = rr.render_temporal(cam, w, h, BOUNCES, tp, fixed_seed=True)
            assert got[1] is None and got[2] is None
            assert np.array_equal(got[0], T.temporal(rad, hits, cam.ubo_bytes(), prev_cam, hist, prev_hits, **tkw)[2])
            assert (got[0] != rgba_raw).any()
            assert np.array_equal(rr.render_temporal(cam, w, h, BOUNCES, tp, fixed_seed=True, reset=True)[0], rgba_raw)
            # ... by a scene upload (the history then holds another sample: keeping it would show)
            assert (rr.render_temporal(cam, w, h, BOUNCES, tp)[0] != rgba_raw).any()
            rr.upload_scene(built)
            assert np.array_equal(rr.render_temporal(cam, w, h, BOUNCES, tp, fixed_seed=True)[0], rgba_raw)
            # ... and by another frame size (a smaller and a larger frame through the same context buffers)
            for ww, hh in ((37, 23), (w, h), (160, 90)):
                c2 = camera(ww, hh, orbit=3.0)
                raw = rr.render(c2, ww, hh, BOUNCES, radiance=True)
                got = rr.render_temporal(c2, ww, hh, BOUNCES, fixed_seed=True, radiance=True)
                assert np.array_equal(got[0], raw[0]) and np.array_equal(got[1].view(np.uint32), raw[1].view(np.uint32))
                got = rr.render_temporal(c2, ww, hh, BOUNCES, fixed_seed=True, radiance=True)
                h2 = rr.render_hits(c2, ww, hh)
                first = T.temporal(raw[1], h2)[0]
                want = T.temporal(raw[1], h2, c2.ubo_bytes(), c2.ubo_bytes(), first, h2)
                assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
            # a sequence that gains a filter keeps its history (the buffers grow under it)
            got = rr.render_temporal(c2, ww, hh, BOUNCES, denoise=dp, fixed_seed=True, radiance=True)
            want3 = T.temporal(raw[1], h2, c2.ubo_bytes(), c2.ubo_bytes(), want[0], h2)
            assert np.array_equal(got[1].view(np.uint32), D.denoise(want3[1], h2, iterations=2)[0].view(np.uint32))
            # the render state is an ordinary render's: the same frame afterwards, synchronously and pipelined
            rgba1, rad1, _ = rr.render(cam0, w, h, BOUNCES, radiance=True)
            assert np.array_equal(rgba1, rgba0) and np.array_equal(rad1.view(np.uint32), rad0.view(np.uint32))
            rr.wait(rr.render_async(cam0, w, h, BOUNCES, frame))
            assert np.array_equal(frame.array, rgba0)
            assert rr.get_option("extensions") == 0 and rr.get_option("new_sample") == 0
        finally:
            frame.close()
        # plain_kernels counts the render's kernels only: a warmed temporal frame adds what a warmed tile adds
        d_rad = torch.empty((h, w, 3), dtype=torch.float32, device="cuda:0")
        for _ in range(3):
            rr.render_temporal(cam0, w, h, BOUNCES, fixed_seed=True)
        k0 = rr.get_option("plain_kernels")
        rr.render_tile_device(cam0, w, h, BOUNCES, 0, 0, w, h, None, d_rad.data_ptr(), None)
        torch.cuda.synchronize()
        k1 = rr.get_option("plain_kernels")
        rr.render_temporal(cam0, w, h, BOUNCES, fixed_seed=True)
        k2 = rr.get_option("plain_kernels")
        rr.render_temporal(cam0, w, h, BOUNCES, denoise=dp, fixed_seed=True)
        k3 = rr.get_option("plain_kernels")
        assert k1 - k0 >= 1 and k2 - k1 == k1 - k0 and k3 - k2 == k1 - k0


def test_render_temporal_refusals(r):
    import rtamd
    from rtamd import RtError, configs
    w, h = 64, 40
    cam = configs.Camera.default(w, h)
    r.render_temporal(cam, w, h, BOUNCES)
    for kw in (dict(params=rtamd.TemporalParams(max_history=0)), dict(params=rtamd.TemporalParams(plane_tol=-1.0)),
               dict(denoise=rtamd.DenoiseParams(iterations=9))):
        with pytest.raises(RtError, match="INVALID_ARG.*rt_render_temporal"):
            r.render_temporal(cam, w, h, BOUNCES, **kw)
    with pytest.raises(RtError, match="INVALID_ARG"):
        r.render_temporal(cam, 0, h, BOUNCES)
    out = np.zeros((h, w, 4), np.uint8)
    L = rtamd.lib()
    assert L.rt_render_temporal(r._ctx, C.byref(cam.ubo), w, h, BOUNCES, None, None, 0, None, None, None) == -1
    assert L.rt_render_temporal(None, C.byref(cam.ubo), w, h, BOUNCES, None, None, 0, out.ctypes.data, None, None) == -1
    assert L.rt_render_temporal(r._ctx, C.byref(cam.ubo), w, h, BOUNCES, None, None, 4, out.ctypes.data, None, None) == -1
    assert b"rt_render_temporal: unknown flags" in L.rt_last_error()
    # extensions bit 4 would average twice
    for ns in (0, 1):
        r.set_option("extensions", 4)
        r.set_option("new_sample", ns)
        try:
            with pytest.raises(RtError, match="INVALID_ARG.*rt_render_temporal.*bit 4"):
                r.render_temporal(cam, w, h, BOUNCES)
        finally:
            r.set_option("extensions", 0)
            r.set_option("new_sample", 0)
    # the other bits pass through to the render
    r.set_option("extensions", 3)
    try:
        r.render_temporal(cam, w, h, BOUNCES)
        assert r.get_option("extensions") == 3
    finally:
        r.set_option("extensions", 0)
    # spheres: refused only while they are uploaded AND the extension is on
    r.upload_spheres([[0.0, 5.0, 0.0, 4.0, 0.9, 0.2, 0.2, 0.0]])
    try:
        r.render_temporal(cam, w, h, BOUNCES)       # bit 8 off: triangles only, accepted
        r.set_option("extensions", 8)
        with pytest.raises(RtError, match="INVALID_ARG.*spheres"):
            r.render_temporal(cam, w, h, BOUNCES)
    finally:
        r.set_option("extensions", 0)
        r.upload_spheres(np.zeros((0, 8), np.float32))
    # rt_upload_spheres drops the history
    raw = r.render(cam, w, h, BOUNCES)[0]
    cam.ubo.frame_count = 3
    assert (r.render_temporal(cam, w, h, BOUNCES, reset=True)[0] != raw).any()      # another sample in the history
    assert (r.render_temporal(cam, w, h, BOUNCES, fixed_seed=True)[0] != raw).any()
    r.render_temporal(cam, w, h, BOUNCES)
    r.upload_spheres(np.zeros((0, 8), np.float32))
    assert np.array_equal(r.render_temporal(cam, w, h, BOUNCES, fixed_seed=True)[0], raw)


def test_render_temporal_refused_on_two_devices():
    """Two devices of one context (the same ordinal twice serves): whole frames of one device only."""
    if not has_gpu():
        pytest.skip("no GPU")
    import rtamd
    from rtamd import RtError, configs
    w, h = 64, 40
    with rtamd.Renderer((0, 0)) as rr:
        rr.upload_scene(configs.config2().build())
        with pytest.raises(RtError, match="INVALID_ARG.*devices"):
            rr.render_temporal(configs.Camera.default(w, h), w, h, BOUNCES)


def test_engine_with_temporal():
    """HipEngine(temporal=...) publishes render_temporal's frames, frame k with frame_count k."""
    if not has_gpu():
        pytest.skip("no GPU")
    import time
    import rtamd
    from rtamd import configs
    w, h = 96, 54
    built = configs.config2().build()
    cam = configs.Camera.default(w, h)
    tp = rtamd.TemporalParams(max_history=4)
    want = []
    with rtamd.Renderer((0,)) as rr:
        rr.upload_scene(built)
        for k in range(3):
            cam.ubo.frame_count = k
            want.append(rr.render_temporal(cam, w, h, BOUNCES, tp)[0])
    cam.ubo.frame_count = 0
    assert (want[1] != want[0]).any()

    class Recording(rtamd.AtomicReference):
        def __init__(self):
            super().__init__()
            self.frames = []

        def set(self, v):
            self.frames.append(v)
            super().set(v)

    q = Recording()
    eng = rtamd.HipEngine(q, w, h, BOUNCES, temporal=tp)
    assert not eng.pipelined
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
