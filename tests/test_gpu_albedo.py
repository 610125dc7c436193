"""rt_albedo_device, rt_denoise_albedo_device and rt_render_denoised with option
denoise_albedo on the GPU: the albedo records and the filtered
radiance bits and RGBA8 equal tests/albedo_ref.py on the checker's rendered
frames and on synthetic guides, at ragged and degenerate sizes, for every pass
count, with both kernel forms forced; guards around every device buffer stay
untouched; argument errors; the frame-level option is the composition made by
hand, and nothing of it moves the colour filter or the render state."""
import dataclasses

import numpy as np
import pytest

import albedo_ref as A
import denoise_ref as D
from conftest import has_gpu
from test_albedo_ref import special_materials
from test_denoise_ref import random_frame
from test_gpu_denoise import FORMS, Guarded
from test_gpu_denoise import run as run_colour
from test_temporal_motion_ref import checker_built

pytestmark = pytest.mark.gpu

F, U = np.float32, np.uint32
SIZES = ((37, 23), (67, 19), (129, 65))


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, F).view(U), np.ascontiguousarray(b, F).view(U))


def camera(w, h):
    """test_temporal_motion_ref.quality_camera() at the frame's own aspect: floor, cube and sky."""
    from rtamd import configs
    return configs.Camera((-10.0, 16.0, 30.0), (0.0, 2.0, 0.0), (0.0, 1.0, 0.0), 30.0, float(w) / float(h))


@pytest.fixture(scope="module")
def r():
    if not has_gpu():
        pytest.skip("no GPU")
    import rtamd
    rr = rtamd.Renderer((0,))
    rr.set_option("accel", 8)
    rr.upload_scene(checker_built()[0])
    yield rr
    rr.close()


@pytest.fixture(scope="module")
def mats():
    return np.asarray(checker_built()[0].model_material_data, F).reshape(-1, 4)


@pytest.fixture(scope="module")
def rendered(r, mats):
    """The checker on the GPU at three ragged sizes: RGBA8, radiance, first-hit
    records and the reference's albedo records, each computed once."""
    out = {}
    for w, h in SIZES:
        cam = camera(w, h)
        rgba, rad, _ = r.render(cam, w, h, 4, radiance=True)
        hits = r.render_hits(cam, w, h)
        alb = A.albedo(hits, mats)
        hit = hits["tri"] >= 0
        assert (hit & (alb[..., 3] == 0.0)).any() and (hit & (alb[..., 3] != 0.0)).any() and (~hit).any(), (w, h)
        out[(w, h)] = (rad, hits, alb, rgba)
    return out


def synthetic_albedo(h, w, seed):
    """An albedo buffer of everything rt_albedo_device can write: ordinary
    albedos, 1 (what every albedo outside [2^-10, 2^10] becomes), the two
    bounds and their neighbours inside; (1, 1, 1) without a hit; the fourth
    word, which the filter must not read, NaN or huge."""
    rng = np.random.default_rng(seed)
    alb = rng.uniform(0.05, 1.0, size=(h, w, 4)).astype(F)
    special = np.array([1.0, 2.0 ** -10, np.nextafter(F(2.0 ** -10), F(1)), np.nextafter(F(2.0 ** 10), F(0)), 2.0 ** 10,
                        0.5, 3.0], F)
    pick = rng.random((h, w, 3)) < 0.25
    alb[..., :3][pick] = rng.choice(special, size=int(pick.sum()))
    alb[..., 3] = np.where(rng.random((h, w)) < 0.5, np.nan, 3e38)
    return alb


def synthetic_frame(h, w, seed, nan_normals=5):
    rad, hits = random_frame(h, w, seed=seed, nan_normals=nan_normals)
    alb = synthetic_albedo(h, w, seed + 1)
    alb[..., :3][hits["tri"] < 0] = 1.0
    return rad, hits, alb


def run_albedo(r, hits):
    """rt_albedo_device on a host hit buffer through guarded device buffers: float32 [H, W, 4]."""
    import torch
    hits = np.ascontiguousarray(hits)
    h, w = hits.shape
    d_hit, o_alb = Guarded(w * h * 32, hits), Guarded(w * h * 16)
    r.albedo_device(w, h, d_hit.ptr, o_alb.ptr, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert d_hit.guards_intact() and o_alb.guards_intact()
    assert d_hit.host(np.uint8, -1).tobytes() == hits.tobytes()
    return o_alb.host(F, (h, w, 4))


def run(r, rad, hits, alb, params=None, form=0, rgba=True, radiance=True):
    """rt_denoise_albedo_device on host arrays through guarded device buffers:
    (rgba or None, radiance or None); nothing outside the outputs and the
    workspace is written and the inputs are unchanged."""
    import torch
    h, w = rad.shape[:2]
    rad, hits, alb = np.ascontiguousarray(rad, F), np.ascontiguousarray(hits), np.ascontiguousarray(alb, F)
    d_rad, d_hit, d_alb = Guarded(w * h * 12, rad), Guarded(w * h * 32, hits), Guarded(w * h * 16, alb)
    d_ws = Guarded(r.denoise_workspace_bytes(w, h))
    o_rgba = Guarded(w * h * 4) if rgba else None
    o_rad = Guarded(w * h * 12) if radiance else None
    r.set_option("denoise_kernel", form)
    try:
        r.denoise_device(w, h, d_rad.ptr, d_hit.ptr, d_ws.ptr, o_rgba.ptr if rgba else None,
                         o_rad.ptr if radiance else None, params, torch.cuda.current_stream().cuda_stream,
                         d_albedo=d_alb.ptr)
        torch.cuda.synchronize()
    finally:
        r.set_option("denoise_kernel", 0)
    for b in (d_rad, d_hit, d_alb, d_ws, o_rgba, o_rad):
        assert b is None or b.guards_intact()
    assert d_rad.host(np.uint8, -1).tobytes() == rad.tobytes() and d_hit.host(np.uint8, -1).tobytes() == hits.tobytes()
    assert d_alb.host(np.uint8, -1).tobytes() == alb.tobytes()
    return (o_rgba.host(np.uint8, (h, w, 4)) if rgba else None, o_rad.host(F, (h, w, 3)) if radiance else None)


def check(r, rad, hits, alb, kw, forms=FORMS):
    import rtamd
    want_rad, want_rgba = A.denoise_albedo(rad, hits, alb, **{**D.DEFAULTS, **kw})
    params = rtamd.DenoiseParams(**{**D.DEFAULTS, **kw})
    for form in forms:
        rgba, out = run(r, rad, hits, alb, params, form)
        diff = out.view(U) != want_rad.view(U)
        assert not diff.any(), (form, kw, int(diff.sum()), np.argwhere(diff)[:4].tolist())
        assert np.array_equal(rgba, want_rgba), (form, kw)
    return want_rad


# ---- rt_albedo_device -----------------------------------------------------------

@pytest.mark.parametrize("size", [(67, 19), (129, 65)])
def test_albedo_of_rendered_hits(r, rendered, size):
    rad, hits, want, rgba0 = rendered[size]
    w, h = size
    k0 = r.get_option("plain_kernels")
    got = run_albedo(r, hits)
    assert same_bits(got, want)
    assert same_bits(r.albedo(hits), want)                            # the host-array form
    assert r.get_option("plain_kernels") == k0
    rgba1, rad1, _ = r.render(camera(w, h), w, h, 4, radiance=True)   # the render state is untouched
    assert np.array_equal(rgba1, rgba0) and same_bits(rad1, rad)


def test_albedo_of_foreign_indices(r, mats):
    n = len(mats)
    assert r.scene_info()["n_tris"] == n
    _, hits = random_frame(5, 13, seed=1)
    tri = np.array([-1, -2, n - 1, n, 1 << 29, 0, n + 1, -(1 << 31), (1 << 31) - 1, 1, n // 2, -3, n - 2], np.int32)
    hits["tri"][:] = tri[None, :]
    hits["tri"][1] = tri[::-1]
    got = run_albedo(r, hits)
    assert same_bits(got, A.albedo(hits, mats))
    assert same_bits(got[0, 2], [*mats[n - 1, :3], mats[n - 1, 3]])
    for x in (0, 1, 3, 4, 6, 7, 8, 11):
        assert same_bits(got[0, x], [1, 1, 1, -1]), x


def test_albedo_of_special_materials_and_an_empty_scene():
    """Materials whose albedos run through every special value (never rendered),
    and a scene without triangles."""
    import rtamd
    from rtamd import build_buffers
    built = checker_built()[0]
    n = len(built.model_material_data) // 4
    special = special_materials(n, seed=3)
    hits = np.zeros((7, 64), D.HIT_DTYPE)
    hits["tri"] = (np.arange(7 * 64).reshape(7, 64) % (n + 2)) - 1            # -1 .. n
    with rtamd.Renderer((0,)) as rr:
        with pytest.raises(rtamd.RtError, match="NO_SCENE.*rt_albedo_device"):
            run_albedo(rr, hits)
        rr.upload_scene(dataclasses.replace(built, model_material_data=special.reshape(-1)))
        got = run_albedo(rr, hits)
        assert same_bits(got, A.albedo(hits, special))
        assert np.isfinite(got[..., :3]).all() and (got[..., :3] == 1.0).any() and (got[..., :3] == F(2.0 ** 10)).any()
        rr.upload_scene(build_buffers(np.zeros((0, 9)), np.zeros((0, 4), F)))
        got = run_albedo(rr, hits)
        assert same_bits(got, np.broadcast_to(np.array([1, 1, 1, -1], F), got.shape))


def test_albedo_argument_errors(r):
    import torch
    import rtamd
    from rtamd import RtError
    w, h = 16, 8
    n = w * h
    hit = torch.zeros(n * 32 + 64, dtype=torch.uint8, device="cuda:0")
    alb = torch.zeros(n * 16 + 64, dtype=torch.uint8, device="cuda:0")
    good = dict(width=w, height=h, d_hits=hit.data_ptr(), d_albedo=alb.data_ptr())
    r.albedo_device(**good)
    assert r.albedo_device(**good, ms=True) >= 0.0
    torch.cuda.synchronize()
    bad = [dict(d_hits=None), dict(d_albedo=None), dict(d_hits=hit.data_ptr() + 8), dict(d_albedo=alb.data_ptr() + 4),
           dict(width=0), dict(height=-3), dict(width=1 << 16, height=1 << 16),
           dict(d_albedo=hit.data_ptr()), dict(d_albedo=hit.data_ptr() + n * 32 - 16)]
    for kw in bad:
        with pytest.raises(RtError, match="INVALID_ARG.*rt_albedo_device") as ei:
            r.albedo_device(**{**good, **kw})
        assert ei.value.code == -1, kw
    assert rtamd.lib().rt_albedo_device(None, w, h, hit.data_ptr(), alb.data_ptr(), None, None) == -1


# ---- rt_denoise_albedo_device ---------------------------------------------------

@pytest.mark.parametrize("size", SIZES)
def test_rendered_frames_equal_the_reference(r, rendered, size):
    """37x23 and 129x65; 67x19 is two tiled workgroups across and three down at step 1, ragged both ways."""
    rad, hits, alb, _ = rendered[size]
    assert same_bits(run_albedo(r, hits), alb)
    for kw in ({}, {"iterations": 6}):
        out = check(r, rad, hits, alb, kw)
        sky = hits["tri"] < 0
        assert same_bits(out[sky], rad[sky])
        floor = (hits["tri"] >= 0) & (alb[..., 3] == 0.0)
        assert (out[floor] != D.denoise(rad, hits, **{**D.DEFAULTS, **kw})[0][floor]).any()


@pytest.mark.parametrize("w,h", [(1, 1), (3, 70), (70, 3)])
def test_degenerate_sizes(r, w, h):
    rad, hits, alb = synthetic_frame(h, w, seed=w * 100 + h, nan_normals=1)
    hits["tri"][0, 0] = 5
    for kw in ({}, {"iterations": 6}, {"iterations": 1, "normal_power_log2": 0, "sigma_depth": 50.0}):
        check(r, rad, hits, alb, kw)


@pytest.fixture(scope="module")
def synthetic():
    return synthetic_frame(65, 129, seed=2025)


@pytest.mark.parametrize("iterations", [1, 2, 3, 4, 5, 6])
def test_every_pass_count_on_synthetic_guides(r, synthetic, iterations):
    """Steps up to 32 on a 129 x 65 frame, an albedo buffer with the special values."""
    rad, hits, alb = synthetic
    check(r, rad, hits, alb, {"iterations": iterations})
    out = check(r, rad, hits, alb, {"iterations": iterations, "normal_power_log2": 0, "sigma_depth": 50.0,
                                    "sigma_color": 4.0})
    hit = (hits["tri"] >= 0) & np.isfinite(hits["normal"]).all(-1)
    assert (out[hit] != rad[hit]).mean() > 0.9
    assert np.isfinite(out).all()


def test_default_params_are_the_null_pointer(r, synthetic):
    rad, hits, alb = synthetic
    want_rad, want_rgba = A.denoise_albedo(rad, hits, alb)
    rgba, out = run(r, rad, hits, alb, None)
    assert same_bits(out, want_rad) and np.array_equal(rgba, want_rgba)
    rgba, out = r.denoise(rad, hits, albedo=alb)                      # the host-array form
    assert same_bits(out, want_rad) and np.array_equal(rgba, want_rgba)


@pytest.mark.parametrize("form", [1, 2])
def test_single_outputs(r, synthetic, form):
    rad, hits, alb = synthetic
    want_rad, want_rgba = A.denoise_albedo(rad, hits, alb)
    rgba, none = run(r, rad, hits, alb, None, form, rgba=True, radiance=False)
    assert none is None and np.array_equal(rgba, want_rgba)
    none, out = run(r, rad, hits, alb, None, form, rgba=False, radiance=True)
    assert none is None and same_bits(out, want_rad)


@pytest.mark.parametrize("form", [1, 2])
def test_lone_passes_on_one_workspace(r, rendered, form):
    """Option denoise_pass: passes 0, 1 and 2 of a 3-pass filter, each enqueued
    alone on one workspace, leave what the whole filter leaves; a pass that is
    not the last writes neither output."""
    import torch
    import rtamd
    rad, hits, alb, _ = rendered[(37, 23)]
    h, w = rad.shape[:2]
    rad, hits = np.ascontiguousarray(rad, F), np.ascontiguousarray(hits)
    kw = {**D.DEFAULTS, "iterations": 3}
    params = rtamd.DenoiseParams(**kw)
    want_rad, want_rgba = A.denoise_albedo(rad, hits, alb, **kw)
    d_rad, d_hit, d_alb = Guarded(w * h * 12, rad), Guarded(w * h * 32, hits), Guarded(w * h * 16, alb)
    d_ws, o_rgba, o_rad = Guarded(r.denoise_workspace_bytes(w, h)), Guarded(w * h * 4), Guarded(w * h * 12)
    r.set_option("denoise_kernel", form)
    try:
        for i in range(3):
            r.set_option("denoise_pass", i)
            r.denoise_device(w, h, d_rad.ptr, d_hit.ptr, d_ws.ptr, o_rgba.ptr, o_rad.ptr, params,
                             torch.cuda.current_stream().cuda_stream, d_albedo=d_alb.ptr)
            torch.cuda.synchronize()
            if i < 2:
                assert (o_rgba.host(np.uint8, -1) == 0xEE).all() and (o_rad.host(np.uint8, -1) == 0xEE).all(), i
    finally:
        r.set_option("denoise_pass", -1)
        r.set_option("denoise_kernel", 0)
    for b in (d_rad, d_hit, d_alb, d_ws, o_rgba, o_rad):
        assert b.guards_intact()
    rgba, out = o_rgba.host(np.uint8, (h, w, 4)), o_rad.host(F, (h, w, 3))
    assert same_bits(out, want_rad) and np.array_equal(rgba, want_rgba)


def test_ones_are_the_colour_filter_which_does_not_move(r, synthetic, rendered):
    """An all-ones albedo buffer gives rt_denoise_device's bits; rt_denoise_device
    gives the same bits before and after the albedo calls, which are not counted
    in plain_kernels."""
    import rtamd
    rad, hits, alb = synthetic
    ones = np.ones_like(alb)
    ones[..., 3] = np.nan
    for kw in ({}, {"iterations": 1}, {"iterations": 6}):
        params = rtamd.DenoiseParams(**{**D.DEFAULTS, **kw})
        for form in FORMS:
            before = run_colour(r, rad, hits, params, form)
            k0 = r.get_option("plain_kernels")
            got = run(r, rad, hits, ones, params, form)
            other = run(r, rad, hits, alb, params, form)
            run_albedo(r, hits)
            assert r.get_option("plain_kernels") == k0
            after = run_colour(r, rad, hits, params, form)
            assert same_bits(got[1], before[1]) and np.array_equal(got[0], before[0]), (kw, form)
            assert same_bits(after[1], before[1]) and np.array_equal(after[0], before[0]), (kw, form)
            assert not same_bits(other[1], before[1])
    rad, hits, _, _ = rendered[(129, 65)]
    got, before = run(r, rad, hits, np.ones((65, 129, 4), F)), run_colour(r, rad, hits)
    assert same_bits(got[1], before[1]) and np.array_equal(got[0], before[0])


def test_argument_errors(r):
    import torch
    import rtamd
    from rtamd import RtError
    w, h = 16, 8
    n = w * h
    buf = lambda nbytes: torch.zeros(nbytes + 64, dtype=torch.uint8, device="cuda:0")   # noqa: E731
    rad, hit, alb, ws, o1, o2 = buf(n * 12), buf(n * 32), buf(n * 16), buf(n * 32), buf(n * 4), buf(n * 12)
    good = dict(width=w, height=h, d_radiance=rad.data_ptr(), d_hits=hit.data_ptr(), d_workspace=ws.data_ptr(),
                d_out_rgba=o1.data_ptr(), d_out_radiance=o2.data_ptr(), params=None, d_albedo=alb.data_ptr())
    r.denoise_device(**good)
    torch.cuda.synchronize()
    P = rtamd.DenoiseParams
    bad = [
        dict(d_albedo=alb.data_ptr() + 8), dict(d_albedo=alb.data_ptr() + 4),
        dict(d_out_rgba=alb.data_ptr()), dict(d_out_radiance=alb.data_ptr() + 16), dict(d_workspace=alb.data_ptr()),
        dict(d_albedo=ws.data_ptr() + n * 16), dict(d_albedo=o2.data_ptr()),
        dict(d_radiance=None), dict(d_hits=None), dict(d_workspace=None), dict(d_out_rgba=None, d_out_radiance=None),
        dict(width=0), dict(width=1 << 16, height=1 << 16), dict(params=P(iterations=7)), dict(params=P(sigma_color=0.0)),
        dict(d_hits=hit.data_ptr() + 8), dict(d_out_rgba=rad.data_ptr()), dict(d_out_radiance=o1.data_ptr()),
    ]
    for kw in bad:
        with pytest.raises(RtError, match="INVALID_ARG.*rt_denoise_albedo_device") as ei:
            r.denoise_device(**{**good, **kw})
        assert ei.value.code == -1, kw
    L = rtamd.lib()
    assert L.rt_denoise_albedo_device(r._ctx, w, h, rad.data_ptr(), hit.data_ptr(), None, None, ws.data_ptr(),
                                      o1.data_ptr(), None, None, None) == -1          # a null d_albedo
    assert L.rt_denoise_albedo_device(None, w, h, rad.data_ptr(), hit.data_ptr(), alb.data_ptr(), None, ws.data_ptr(),
                                      o1.data_ptr(), None, None, None) == -1
    for v in (2, -1):
        with pytest.raises(RtError, match="INVALID_ARG"):
            r.set_option("denoise_albedo", v)
    with pytest.raises(RtError, match="INVALID_ARG"):
        r.set_option("denoise_albedo_used", 1)
    assert r.get_option("denoise_albedo") == 0


# ---- rt_render_denoised with option denoise_albedo -------------------------------

@pytest.mark.parametrize("accel", [8, 0])
def test_render_denoised_with_the_option(accel):
    if not has_gpu():
        pytest.skip("no GPU")
    import rtamd
    from rtamd import RtError
    w, h, bounces = 129, 65, 4
    cam = camera(w, h)
    built = checker_built()[0]
    mats = np.asarray(built.model_material_data, F).reshape(-1, 4)
    with rtamd.Renderer((0,)) as rr:
        rr.set_option("accel", accel)
        rr.upload_scene(built)
        assert rr.get_option("denoise_albedo") == 0 and rr.get_option("denoise_albedo_used") == 0
        rgba0, rad0, st0 = rr.render(cam, w, h, bounces, radiance=True, stats=True)
        hits = rr.render_hits(cam, w, h)
        alb = rr.albedo(hits)
        assert same_bits(alb, A.albedo(hits, mats))
        hand_rgba, hand_rad = rr.denoise(rad0, hits, albedo=alb)
        want_rad, want_rgba = A.denoise_albedo(rad0, hits, alb)
        assert same_bits(hand_rad, want_rad) and np.array_equal(hand_rgba, want_rgba)
        colour_rgba, colour_rad = rr.denoise(rad0, hits)
        # 0: today's composition
        rgba, rad, _ = rr.render_denoised(cam, w, h, bounces, radiance=True)
        assert same_bits(rad, colour_rad) and np.array_equal(rgba, colour_rgba)
        assert rr.get_option("denoise_albedo_used") == 0
        # 1: hit buffer, albedo buffer, the filter on the illumination
        rr.set_option("denoise_albedo", 1)
        rgba, rad, st = rr.render_denoised(cam, w, h, bounces, radiance=True, stats=True)
        assert same_bits(rad, hand_rad) and np.array_equal(rgba, hand_rgba)
        assert not same_bits(rad, colour_rad)
        assert rr.get_option("denoise_albedo_used") == 1
        for k in ("segments", "node_visits", "tri_tests", "mat_reads", "pixels"):
            assert st[k] == st0[k], k
        assert st["ms"] > 0
        # other parameters, RGBA only; a smaller and a larger frame through the same context buffers
        p = rtamd.DenoiseParams(iterations=2, normal_power_log2=3, sigma_depth=0.02, sigma_color=1.0)
        rgba2, none, none2 = rr.render_denoised(cam, w, h, bounces, p)
        assert none is None and none2 is None
        assert np.array_equal(rgba2, A.denoise_albedo(rad0, hits, alb, 2, 3, 0.02, 1.0)[1])
        for ww, hh in ((37, 23), (160, 90)):
            c2 = camera(ww, hh)
            _, r2, _ = rr.render(c2, ww, hh, bounces, radiance=True)
            h2 = rr.render_hits(c2, ww, hh)
            got = rr.render_denoised(c2, ww, hh, bounces, radiance=True)
            assert same_bits(got[1], A.denoise_albedo(r2, h2, A.albedo(h2, mats))[0]), (ww, hh)
        # the refusals stay, and a refused call leaves the flag
        with pytest.raises(RtError, match="INVALID_ARG.*rt_render_denoised"):
            rr.render_denoised(cam, w, h, bounces, rtamd.DenoiseParams(iterations=9))
        with pytest.raises(RtError, match="INVALID_ARG"):
            rr.render_denoised(cam, 0, h, bounces)
        rr.upload_spheres([[0.0, 5.0, 0.0, 4.0, 0.9, 0.2, 0.2, 0.0]])
        try:
            rr.set_option("extensions", 8)
            with pytest.raises(RtError, match="INVALID_ARG.*spheres"):
                rr.render_denoised(cam, w, h, bounces)
        finally:
            rr.set_option("extensions", 0)
            rr.upload_spheres(np.zeros((0, 8), F))
        assert rr.get_option("denoise_albedo_used") == 1
        # back to 0: the colour filter again; a plain render afterwards is unchanged
        rr.set_option("denoise_albedo", 0)
        rgba, rad, _ = rr.render_denoised(cam, w, h, bounces, radiance=True)
        assert same_bits(rad, colour_rad) and np.array_equal(rgba, colour_rgba)
        assert rr.get_option("denoise_albedo_used") == 0
        rgba1, rad1, _ = rr.render(cam, w, h, bounces, radiance=True)
        assert np.array_equal(rgba1, rgba0) and same_bits(rad1, rad0)

