"""The temporal history across a geometry update on the GPU (include/rtamd.h
"temporal history across an update"): rt_temporal_motion_device's
history, moments, radiance bits and RGBA8 equal tests/temporal_motion_ref.py on
translated, slid, jittered and squashed scenes, under a moving camera and on
synthetic guides with foreign triangle indices, with every lane mapping, with
and without moments, at ragged and degenerate sizes and through a ping-ponged
chain; with NULL vertex buffers it is rt_temporal_device and
rt_temporal_moments_device; its refusals leave the outputs alone; and with
option temporal_motion 1 rt_update_geometry keeps the context's history, the
next rt_render_temporal* call equals the explicit composition with the test's
own vertex buffers, and every state that dropped the history still does."""
import numpy as np
import pytest

import denoise_history_ref as DH
import refit_ref as R
import temporal_motion_ref as M
import temporal_ref as T
import variance_ref as V
from conftest import has_gpu
from test_denoise_ref import random_frame
from test_gpu_denoise import GUARD, Guarded
from test_temporal_motion_ref import camera, checker_built, moved_buffers, quality_camera, same_bits
from test_temporal_ref import random_camera_pair, random_history

pytestmark = pytest.mark.gpu

F = np.float32
FORMS = (0, 1, 2)
SIZES = ((37, 23), (129, 65))
BOUNCES = 3


@pytest.fixture(scope="module")
def r():
    if not has_gpu():
        pytest.skip("no GPU")
    import rtamd
    rr = rtamd.Renderer((0,))
    rr.set_option("accel", 8)
    rr.set_option("refit", 1)
    yield rr
    rr.close()


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def run(r, rad, hits, cam, prev, vc, vp, n_tris, mom_prev=None, moments=False, params=None, form=0):
    """rt_temporal_motion_device on host arrays through guarded device buffers;
    prev = (camera bytes, history, hit records); vc / vp None = NULL vertex
    buffers.  Returns (history, rgba, radiance, moments or None); asserts that
    nothing outside the outputs was written and that the inputs are unchanged."""
    import torch
    h, w = rad.shape[:2]
    host = [np.ascontiguousarray(rad, F), np.ascontiguousarray(hits), np.ascontiguousarray(prev[1], F),
            np.ascontiguousarray(prev[2])]
    sizes = [w * h * 12, w * h * 32, w * h * 16, w * h * 32]
    if vc is not None:
        host += [np.ascontiguousarray(vc, F), np.ascontiguousarray(vp, F)]
        sizes += [host[-2].nbytes, host[-1].nbytes]
    if moments:
        host.append(np.ascontiguousarray(mom_prev, F))
        sizes.append(w * h * 8)
    dev = [Guarded(n, a) for n, a in zip(sizes, host)]
    d_vc, d_vp = (dev[4], dev[5]) if vc is not None else (None, None)
    d_mp = dev[-1] if moments else None
    o_hist, o_rgba, o_rad = Guarded(w * h * 16), Guarded(w * h * 4), Guarded(w * h * 12)
    o_mom = Guarded(w * h * 8) if moments else None
    r.set_option("temporal_tile", form)
    try:
        r.temporal_motion_device(w, h, cam, dev[0].ptr, dev[1].ptr, o_hist.ptr, prev[0], dev[2].ptr, dev[3].ptr,
                                 d_vc.ptr if d_vc else None, d_vp.ptr if d_vp else None, n_tris,
                                 d_mp.ptr if d_mp else None, o_mom.ptr if o_mom else None, o_rgba.ptr, o_rad.ptr, params,
                                 stream())
        torch.cuda.synchronize()
    finally:
        r.set_option("temporal_tile", 0)
    for b in dev + [o_hist, o_rgba, o_rad] + ([o_mom] if moments else []):
        assert b.guards_intact()
    for b, a in zip(dev, host):
        assert b.host(np.uint8, -1).tobytes() == a.tobytes()
    return (o_hist.host(F, (h, w, 4)), o_rgba.host(np.uint8, (h, w, 4)), o_rad.host(F, (h, w, 3)),
            o_mom.host(F, (h, w, 2)) if moments else None)


def check(r, rad, hits, cam, prev, vc, vp, n_tris=None, mom_prev=None, kw=None, forms=FORMS):
    """Every lane mapping, with and without moments, equals the reference bit
    for bit; returns the reference's (history, reused mask, moments)."""
    import rtamd
    kw = {**T.DEFAULTS, **(kw or {})}
    n = len(np.asarray(vc).reshape(-1, 12)) if n_tris is None else n_tris
    want = M.temporal_motion(rad, hits, cam, prev[0], prev[1], prev[2], vc, vp, n, mom_prev=mom_prev, **kw)
    params = rtamd.TemporalParams(**kw)
    for form in forms:
        for moments in (False, True):
            hist, rgba, out, mom = run(r, rad, hits, cam, prev, vc, vp, n, mom_prev, moments, params, form)
            diff = hist.view(np.uint32) != want[0].view(np.uint32)
            assert not diff.any(), (form, moments, int(diff.sum()), np.argwhere(diff)[:4].tolist())
            assert same_bits(out, want[1]) and np.array_equal(rgba, want[2]), (form, moments)
            if moments:
                assert same_bits(mom, want[4]), form
    return want[0], want[3], want[4]


def render_pair(r, prev, cur, prev_cam, cam, w, h, seed):
    """The GPU's guides of both states of a scene (uploaded, then updated), the
    new frame's radiance, a random history and random moments."""
    rng = np.random.default_rng(seed)
    r.upload_scene(prev)
    hits_prev = r.render_hits(prev_cam, w, h)
    r.update_geometry(cur)
    hits = r.render_hits(cam, w, h)
    _, rad, _ = r.render(cam, w, h, BOUNCES, radiance=True)
    hist = random_history(h, w, rng)
    mom = rng.uniform(0.0, 1.0, (h, w, 2)).astype(F)
    return rad, hits, hits_prev, hist, mom


def scene_pairs(name):
    """[(previous buffers, current buffers, previous camera, camera factory)] of a named case."""
    from rtamd import build_buffers, configs, refit_buffers
    if name == "checker":
        built, tv, part = checker_built()
        c = quality_camera()
        cam = lambda w, h: configs.Camera(c.origin, c.look_at, c.v_up, c.vfov, w / h)   # noqa: E731
        return [(moved_buffers(built, tv, part, (-0.45, 0.0, -0.3)), built, cam, cam)]
    scene, kind = {"translate": ("config2", "translate"), "orbit": ("config2", "translate"),
                   "jitter": ("config2", "jitter"), "squash": ("tris5", "squash")}[name]
    tv, mats, seed, part, c0 = R.scene(scene)
    built = build_buffers(tv, mats, seed)
    states = [built] + [refit_buffers(built, s) for s in R.deform(kind, tv, part)]
    if scene == "config2":
        prev_cam = lambda w, h: camera(w, h)                                            # noqa: E731
        cam = (lambda w, h: camera(w, h, orbit=1.0)) if name == "orbit" else prev_cam    # noqa: E731
    else:
        prev_cam = cam = lambda w, h: configs.Camera(c0.origin, c0.look_at, c0.v_up, c0.vfov, w / h)   # noqa: E731
    return [(a, b, prev_cam, cam) for a, b in zip(states[:-1], states[1:])]


# ---- 8. rt_temporal_motion_device against the reference ----------------------------------

@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("name", ["translate", "checker", "jitter", "squash", "orbit"])
def test_moved_scenes_equal_the_reference(r, name, size):
    w, h = size
    moved_reused = 0
    for step, (prev, cur, prev_cam, cam) in enumerate(scene_pairs(name)):
        pc, c = prev_cam(w, h), cam(w, h)
        rad, hits, hits_prev, hist, mom = render_pair(r, prev, cur, pc, c, w, h, seed=w + step)
        vc, vp = cur.model_vertex_data, prev.model_vertex_data
        _, reused, _ = check(r, rad, hits, c.ubo_bytes(), (pc.ubo_bytes(), hist, hits_prev), vc, vp, mom_prev=mom)
        moved = M.previous_points(hits, vc, vp)[3]
        moved_reused += int((reused & moved).sum())
        print(f"{name} {w}x{h} step {step}: {int(moved.sum())} pixels on moved triangles, {int((reused & moved).sum())} "
              f"of them reuse history")
    assert moved_reused > 5                          # the moved path's gather is really compared


def synthetic_case(h, w, seed, n_tris=64):
    """Random guides of two frames that mostly see the same surfaces, random
    vertex records of which a third are unmoved, a few foreign indices."""
    rng = np.random.default_rng(seed)
    rad, hits = random_frame(h, w, seed=seed, nan_normals=5)
    _, hits_prev = random_frame(h, w, seed=seed + 1000, nan_normals=5)
    hit = hits["tri"] >= 0
    hits["tri"][hit] = rng.integers(0, n_tris, size=int(hit.sum()))
    vc = np.zeros((n_tris, 3, 4), F)
    vc[:, :, :3] = rng.normal(size=(n_tris, 3, 3)) * 3.0
    vc[:, :, 3] = rng.normal(size=(n_tris, 3))                   # w is ignored
    vp = vc.copy()
    moved = rng.random(n_tris) < 2.0 / 3.0
    vp[moved, :, :3] += rng.normal(size=(int(moved.sum()), 1, 3)).astype(F) * F(0.01)
    vp[:, :, 3] = rng.normal(size=(n_tris, 3))
    # the hit points on their triangles, the previous frame's near where they lay before
    k = np.maximum(hits["tri"], 0)
    b = rng.uniform(0.0, 0.5, size=(h, w, 2)).astype(F)
    on = lambda v: v[k, 0, :3] + b[..., :1] * (v[k, 1, :3] - v[k, 0, :3]) + b[..., 1:] * (v[k, 2, :3] - v[k, 0, :3])   # noqa: E731
    hits["pos"] = on(vc)
    same = rng.random((h, w)) < 0.7
    hits_prev["normal"][same] = hits["normal"][same]
    hits_prev["pos"][same] = on(vp)[same]
    flat = hits["tri"].reshape(-1)
    for i, t in enumerate((-1, -2, n_tris - 1, n_tris, 1 << 30)):
        if i < flat.size - 1:
            flat[1 + i] = t
    cam, prev_cam = random_camera_pair(rng)
    hist = random_history(h, w, rng)
    mom = rng.uniform(0.0, 1.0, (h, w, 2)).astype(F)
    return rad, hits, cam, (prev_cam, hist, hits_prev), vc.reshape(-1), vp.reshape(-1), mom


@pytest.mark.parametrize("kw", [dict(), dict(max_history=2, plane_tol=50.0, normal_min=-1.0)], ids=["defaults", "wide"])
def test_synthetic_guides_with_foreign_indices(r, kw):
    reused_any = 0
    for seed in (31, 32):
        rad, hits, cam, prev, vc, vp, mom = synthetic_case(41, 67, seed)
        assert {-1, -2, 63, 64, 1 << 30} <= set(hits["tri"].reshape(-1).tolist())
        hist, reused, _ = check(r, rad, hits, cam, prev, vc, vp, mom_prev=mom, kw=kw)
        foreign = hits["tri"] >= 64
        assert foreign.sum() >= 2 and not reused[foreign].any() and (hist[..., 3][foreign] == 1).all()
        reused_any += int(reused.sum())
    if kw:
        assert reused_any > 40


# ---- 9. NULL vertex buffers ----------------------------------------------------------------

@pytest.mark.parametrize("form", FORMS)
def test_null_vertex_buffers_are_the_static_calls(r, form):
    import torch
    h, w = 41, 67
    rad, hits, cam, prev, _, _, mom = synthetic_case(h, w, 33)
    got = run(r, rad, hits, cam, prev, None, None, 0, form=form)
    got_m = run(r, rad, hits, cam, prev, None, None, 7, mom, True, form=form)
    d = [Guarded(a.nbytes, a) for a in (np.ascontiguousarray(rad, F), np.ascontiguousarray(hits),
                                        np.ascontiguousarray(prev[1], F), np.ascontiguousarray(prev[2]), mom)]
    o_hist, o_rgba, o_rad, o_mom = Guarded(w * h * 16), Guarded(w * h * 4), Guarded(w * h * 12), Guarded(w * h * 8)
    r.set_option("temporal_tile", form)
    try:
        r.temporal_device(w, h, cam, d[0].ptr, d[1].ptr, o_hist.ptr, prev[0], d[2].ptr, d[3].ptr, o_rgba.ptr, o_rad.ptr,
                          None, stream())
        torch.cuda.synchronize()
        plain = (o_hist.host(F, (h, w, 4)).copy(), o_rgba.host(np.uint8, (h, w, 4)).copy(), o_rad.host(F, (h, w, 3)).copy())
        r.temporal_moments_device(w, h, cam, d[0].ptr, d[1].ptr, o_hist.ptr, o_mom.ptr, prev[0], d[2].ptr, d[3].ptr,
                                  d[4].ptr, o_rgba.ptr, o_rad.ptr, None, stream())
        torch.cuda.synchronize()
    finally:
        r.set_option("temporal_tile", 0)
    with_m = (o_hist.host(F, (h, w, 4)), o_rgba.host(np.uint8, (h, w, 4)), o_rad.host(F, (h, w, 3)), o_mom.host(F, (h, w, 2)))
    for a, b in zip(got[:3], plain):
        assert a.tobytes() == b.tobytes()
    for a, b in zip(got_m, with_m):
        assert a.tobytes() == b.tobytes()
    assert got[3] is None


# ---- 10. degenerate sizes ------------------------------------------------------------------

@pytest.mark.parametrize("w,h", [(1, 1), (3, 70), (70, 3)])
def test_degenerate_sizes(r, w, h):
    rad, hits, cam, prev, vc, vp, mom = synthetic_case(h, w, seed=w * 100 + h)
    hits["tri"][0, 0] = 5
    check(r, rad, hits, cam, prev, vc, vp, mom_prev=mom)
    check(r, rad, hits, cam, prev, vc, vp, mom_prev=mom, kw=dict(max_history=2, plane_tol=50.0, normal_min=-1.0))


# ---- 11. a chain ---------------------------------------------------------------------------

def test_a_four_frame_chain_with_a_move_between_every_pair(r):
    """Two history / hit buffer pairs on the device take turns, as rt_render_temporal's do; the cube moves
    between every two frames and the camera orbits."""
    import torch
    import rtamd
    from rtamd import build_buffers
    w, h = 129, 65
    tv, mats, seed, part, _ = R.scene("config2")
    built = build_buffers(tv, mats, seed)
    d_hist = [Guarded(w * h * 16), Guarded(w * h * 16)]
    d_hits = [Guarded(w * h * 32), Guarded(w * h * 32)]
    o_rad = Guarded(w * h * 12)
    params = rtamd.TemporalParams(max_history=3)
    want = prev_cam = prev_hits = prev_state = None
    r.upload_scene(built)
    on_cube = 0
    for k in range(4):
        state = moved_buffers(built, tv, part, (0.4 * k, 0.0, 0.2 * k))
        r.update_geometry(state)
        cam = camera(w, h, orbit=1.0 * k)
        cam.ubo.frame_count = k
        r.set_option("new_sample", 1)
        try:
            _, rad, _ = r.render(cam, w, h, BOUNCES, radiance=True)
        finally:
            r.set_option("new_sample", 0)
        hits = r.render_hits(cam, w, h)
        cur = k & 1
        d_rad = Guarded(w * h * 12, rad)
        d_hits[cur].t[GUARD:GUARD + w * h * 32] = torch.from_numpy(np.frombuffer(hits.tobytes(), np.uint8).copy()).cuda()
        d_vc = Guarded(state.model_vertex_data.nbytes, state.model_vertex_data)
        if k:
            d_vp = Guarded(prev_state.model_vertex_data.nbytes, prev_state.model_vertex_data)
            r.temporal_motion_device(w, h, cam, d_rad.ptr, d_hits[cur].ptr, d_hist[cur].ptr, prev_cam, d_hist[1 - cur].ptr,
                                     d_hits[1 - cur].ptr, d_vc.ptr, d_vp.ptr, state.triangle_count, None, None, None,
                                     o_rad.ptr, params, stream())
            torch.cuda.synchronize()
            want = M.temporal_motion(rad, hits, cam.ubo_bytes(), prev_cam, want[0], prev_hits, state.model_vertex_data,
                                     prev_state.model_vertex_data, max_history=3)
            moved = M.previous_points(hits, state.model_vertex_data, prev_state.model_vertex_data)[3]
            on_cube += int((want[3] & moved).sum())
        else:
            r.temporal_motion_device(w, h, cam, d_rad.ptr, d_hits[cur].ptr, d_hist[cur].ptr, d_out_radiance=o_rad.ptr,
                                     params=params, stream=stream())
            torch.cuda.synchronize()
            want = T.temporal(rad, hits, max_history=3)
        assert same_bits(d_hist[cur].host(F, (h, w, 4)), want[0]), k
        assert same_bits(o_rad.host(F, (h, w, 3)), want[1]), k
        for b in d_hist + d_hits + [o_rad, d_rad, d_vc]:
            assert b.guards_intact()
        prev_cam, prev_hits, prev_state = cam.ubo_bytes(), hits, state
    n = want[0][..., 3]
    assert n.max() == 3 and on_cube > 50


# ---- 12. argument errors -------------------------------------------------------------------

def test_argument_errors_leave_the_outputs_untouched(r):
    import torch
    from rtamd import RtError, configs
    w, h, n_tris = 16, 8, 10
    n = w * h
    buf = lambda nbytes: torch.full((nbytes + 64,), 0x5A, dtype=torch.uint8, device="cuda:0")   # noqa: E731
    rad, hit, hp, hq, mp = buf(n * 12), buf(n * 32), buf(n * 16), buf(n * 32), buf(n * 8)
    outs = [buf(n * 16), buf(n * 4), buf(n * 12), buf(n * 8)]
    oh, o1, o2, om = outs
    vc, vp = buf(n_tris * 48), buf(n_tris * 48)
    cam = configs.Camera.default(w, h)
    good = dict(width=w, height=h, camera=cam, d_radiance=rad.data_ptr(), d_hits=hit.data_ptr(),
                d_hist_out=oh.data_ptr(), prev_camera=cam, d_hist_prev=hp.data_ptr(), d_hits_prev=hq.data_ptr(),
                d_verts_cur=vc.data_ptr(), d_verts_prev=vp.data_ptr(), n_tris=n_tris, d_mom_prev=mp.data_ptr(),
                d_mom_out=om.data_ptr(), d_out_rgba=o1.data_ptr(), d_out_radiance=o2.data_ptr(), params=None)
    no_prev = dict(prev_camera=None, d_hist_prev=None, d_hits_prev=None, d_mom_prev=None)
    bad = [
        dict(d_verts_cur=None), dict(d_verts_prev=None),                                # one without the other
        no_prev,                                                                         # vertex buffers without a previous frame
        dict(d_verts_cur=vc.data_ptr() + 8), dict(d_verts_prev=vp.data_ptr() + 4),       # alignment
        dict(n_tris=0), dict(n_tris=(1 << 29) + 1),
        dict(d_hist_out=vc.data_ptr()), dict(d_out_rgba=vp.data_ptr() + 16), dict(d_out_radiance=vc.data_ptr() + 32),
        dict(d_mom_out=vp.data_ptr()), dict(d_verts_cur=oh.data_ptr()),                  # overlaps with an output
        dict(d_mom_out=None), dict(d_mom_prev=None),                                     # half a moments pair
        dict(camera=None), dict(d_radiance=None), dict(d_hist_out=None), dict(width=0),  # rt_temporal_device's own
    ]
    for kw in bad:
        with pytest.raises(RtError, match="INVALID_ARG.*rt_temporal_motion_device") as ei:
            r.temporal_motion_device(**{**good, **kw})
        assert ei.value.code == -1, kw
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o == 0x5A).all())
    r.temporal_motion_device(**good)                                                     # the baseline is accepted
    r.temporal_motion_device(**{**good, "n_tris": 1 << 29, "d_verts_cur": None, "d_verts_prev": None})
    r.temporal_motion_device(**{**good, **no_prev, "d_verts_cur": None, "d_verts_prev": None})
    torch.cuda.synchronize()
    assert not bool((oh[:n * 16] == 0x5A).all())


# ---- 13 - 17. the context form -------------------------------------------------------------

W, H = 129, 65


class Composition:
    """rt_render_temporal's frame put together from its parts on a context of
    its own: render_tile_device with option new_sample, render_hits_device and
    the temporal call, through ping-ponged device buffers; with verts_prev the
    temporal call is temporal_motion_device on the test's own vertex buffers."""

    def __init__(self, accel, built, moments=False):
        import torch
        import rtamd
        self.r = rtamd.Renderer((0,))
        self.r.set_option("accel", accel)
        self.r.set_option("refit", 1)
        self.r.upload_scene(built)
        z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device="cuda:0")     # noqa: E731
        self.rad, self.hist, self.hits = z(H, W, 3), [z(H, W, 4), z(H, W, 4)], [z(H, W, 8), z(H, W, 8)]
        self.mom = [z(H, W, 2), z(H, W, 2)] if moments else None
        self.o_rad, self.o_rgba = z(H, W, 3), z(H, W, 4, dt=torch.uint8)
        self.k, self.prev_cam = 0, None

    def close(self):
        self.r.close()

    def frame(self, cam, frame_count, verts=None, verts_prev=None, params=None):
        """One frame; returns (rgba, radiance, history, hit records, moments or None) on the host."""
        import torch
        import rtamd
        r, cur = self.r, self.k & 1
        ubo = rtamd.CameraUBO.from_buffer_copy(cam.ubo_bytes())
        ubo.frame_count = frame_count
        r.set_option("new_sample", 1)
        try:
            r.render_tile_device(ubo, W, H, BOUNCES, 0, 0, W, H, None, self.rad.data_ptr(), stream())
        finally:
            r.set_option("new_sample", 0)
        r.render_hits_device(ubo, W, H, 0, 0, W, H, self.hits[cur].data_ptr(), stream())
        first = self.prev_cam is None
        ptr = lambda t: None if first else t[1 - cur].data_ptr()                       # noqa: E731
        d_vc = d_vp = None
        if verts_prev is not None:
            d_vc = torch.from_numpy(np.ascontiguousarray(verts, F)).cuda()
            d_vp = torch.from_numpy(np.ascontiguousarray(verts_prev, F)).cuda()
        r.temporal_motion_device(W, H, ubo, self.rad.data_ptr(), self.hits[cur].data_ptr(), self.hist[cur].data_ptr(),
                                 self.prev_cam, ptr(self.hist), ptr(self.hits),
                                 d_vc.data_ptr() if d_vc is not None else None,
                                 d_vp.data_ptr() if d_vp is not None else None,
                                 d_vc.numel() // 12 if d_vc is not None else 0,
                                 ptr(self.mom) if self.mom else None, self.mom[cur].data_ptr() if self.mom else None,
                                 self.o_rgba.data_ptr(), self.o_rad.data_ptr(), params, stream())
        torch.cuda.synchronize()
        self.prev_cam, self.k = ubo, self.k + 1
        hits = self.hits[cur].cpu().numpy().view(T.HIT_DTYPE).reshape(H, W)
        return (self.o_rgba.cpu().numpy(), self.o_rad.cpu().numpy(), self.hist[cur].cpu().numpy(), hits,
                self.mom[cur].cpu().numpy() if self.mom else None)

    def reset(self):
        self.k, self.prev_cam = 0, None


def context(accel, built, motion=1):
    import rtamd
    rr = rtamd.Renderer((0,))
    rr.set_option("accel", accel)
    rr.set_option("refit", 1)
    rr.set_option("temporal_motion", motion)
    rr.upload_scene(built)
    return rr


def config2_states():
    from rtamd import build_buffers
    tv, mats, seed, part, _ = R.scene("config2")
    built = build_buffers(tv, mats, seed)
    return built, [moved_buffers(built, tv, part, (2.0 * k, 0.0, 1.0 * k)) for k in (1, 2)], part


def frame_of(rr, cam, k, **kw):
    cam.ubo.frame_count = k
    rgba, rad, _ = rr.render_temporal(cam, W, H, BOUNCES, radiance=True, **kw)
    return rgba, rad


def same_frame(got, want, what):
    assert np.array_equal(got[0], want[0]), f"{what}: RGBA8 differs"
    assert same_bits(got[1], want[1]), f"{what}: radiance differs"


@pytest.mark.parametrize("accel", [8, 0])
def test_an_update_keeps_the_history(accel):
    """Check 13, and 14 behind it: three frames, an update, a frame; then two updates and a frame."""
    if not has_gpu():
        pytest.skip("no GPU")
    built, (s1, s2), part = config2_states()
    rr, comp = context(accel, built), Composition(accel, built)
    try:
        assert rr.get_option("temporal_motion") == 1 and rr.get_option("temporal_motion_used") == 0
        for k in range(3):
            cam = camera(W, H, orbit=1.0 * k)
            same_frame(frame_of(rr, cam, k, reset=(k == 0)), comp.frame(cam, k), f"frame {k}")
            assert rr.get_option("temporal_motion_used") == 0
        rr.update_geometry(s1)
        comp.r.update_geometry(s1)
        cam = camera(W, H, orbit=3.0)
        want = comp.frame(cam, 3, s1.model_vertex_data, built.model_vertex_data)
        same_frame(frame_of(rr, cam, 3), want, "the frame after the update")
        assert rr.get_option("temporal_motion_used") == 1
        moved = np.isin(np.asarray(built.flat_source)[np.maximum(want[3]["tri"], 0)], part) & (want[3]["tri"] >= 0)
        assert moved.sum() > 50 and (want[2][..., 3][moved] > 1).sum() > 0.5 * moved.sum()
        # a frame with no update since the last one: the static kernel again
        same_frame(frame_of(rr, cam, 4), comp.frame(cam, 4), "the frame after that")
        assert rr.get_option("temporal_motion_used") == 0
        # check 14: two updates between two frames reproject from the last frame's state, not the intermediate one
        back = moved_buffers(built, *config2_tv_part(), (-1.0, 0.0, 0.5))
        for st in (back, s2):
            rr.update_geometry(st)
            comp.r.update_geometry(st)
        got = frame_of(rr, cam, 5)
        prev_cam = comp.prev_cam
        want = comp.frame(cam, 5, s2.model_vertex_data, s1.model_vertex_data)
        same_frame(got, want, "the frame after two updates")
        comp.k, comp.prev_cam = comp.k - 1, prev_cam            # the same frame again, from the intermediate state
        other = comp.frame(cam, 5, s2.model_vertex_data, back.model_vertex_data)
        assert not same_bits(other[1], want[1])                 # the two states are told apart
    finally:
        rr.close()
        comp.close()


def config2_tv_part():
    tv, _, _, part, _ = R.scene("config2")
    return tv, part


def test_what_drops_the_history_and_what_keeps_it():
    """Check 15."""
    if not has_gpu():
        pytest.skip("no GPU")
    import copy
    from rtamd import RtError
    built, (s1, _), _ = config2_states()
    rr, fresh, never = context(8, built), context(8, built), context(8, built)
    try:
        cam = camera(W, H)
        for k in range(2):
            frame_of(rr, cam, k)
            frame_of(never, cam, k)
        # a refused update: the history, the copy and the mark stay
        broken = copy.copy(s1)
        broken.model_vertex_data = s1.model_vertex_data[:-12]
        with pytest.raises(RtError, match="BAD_SCENE"):
            rr.update_geometry(broken)
        same_frame(frame_of(rr, cam, 2), frame_of(never, cam, 2), "after a refused update")
        assert rr.get_option("temporal_motion_used") == 0
        # an update, then reset=True: a fresh sequence on the moved scene
        rr.update_geometry(s1)
        fresh.upload_scene(s1)
        same_frame(frame_of(rr, cam, 3, reset=True), frame_of(fresh, cam, 3, reset=True), "an update and a reset")
        assert rr.get_option("temporal_motion_used") == 0
        same_frame(frame_of(rr, cam, 4), frame_of(fresh, cam, 4), "the frame after it")
        # an update, then an upload: dropped as ever
        rr.update_geometry(built)
        rr.upload_scene(s1)
        same_frame(frame_of(rr, cam, 5), frame_of(fresh, cam, 5, reset=True), "an update and an upload")
        assert rr.get_option("temporal_motion_used") == 0
        # an update, then another frame size
        frame_of(rr, cam, 6)
        rr.update_geometry(built)
        fresh.upload_scene(built)
        c2 = camera(37, 23)
        c2.ubo.frame_count = 7
        a = rr.render_temporal(c2, 37, 23, BOUNCES, radiance=True)
        b = fresh.render_temporal(c2, 37, 23, BOUNCES, radiance=True, reset=True)
        same_frame(a, b, "an update and another size")
        assert rr.get_option("temporal_motion_used") == 0
    finally:
        for c in (rr, fresh, never):
            c.close()


@pytest.mark.parametrize("kind", ["adaptive", "variance"])
def test_the_filtered_calls_follow_the_same_rule(kind):
    """Check 16: the composition's history (and moments) through the numpy filters, which the GPU's equal bit
    for bit (tests/test_gpu_denoise_history.py, tests/test_gpu_variance.py)."""
    if not has_gpu():
        pytest.skip("no GPU")
    built, (s1, _), _ = config2_states()
    rr, comp = context(8, built), Composition(8, built, moments=(kind == "variance"))
    kw = dict(adaptive=True) if kind == "adaptive" else dict(variance=True)
    try:
        for k in range(4):
            cam = camera(W, H, orbit=1.0 * k)
            if k == 3:
                rr.update_geometry(s1)
                comp.r.update_geometry(s1)
                _, _, hist, hits, mom = comp.frame(cam, k, s1.model_vertex_data, built.model_vertex_data)
            else:
                _, _, hist, hits, mom = comp.frame(cam, k)
            want = DH.denoise_history(hist, hits) if kind == "adaptive" else V.denoise_variance(hist, mom, hits)
            got = frame_of(rr, cam, k, reset=(k == 0), **kw)
            assert same_bits(got[1], want[0]) and np.array_equal(got[0], want[1]), (kind, k)
            assert rr.get_option("temporal_motion_used") == (1 if k == 3 else 0)
        # a change of history kind after an update drops the history and the copy
        rr.update_geometry(built)
        other = dict(variance=True) if kind == "adaptive" else dict(adaptive=True)
        got = frame_of(rr, cam, 4, **other)
        if kind == "adaptive":                       # moments that are not the history's: a new sequence
            assert rr.get_option("temporal_motion_used") == 0
            fresh = context(8, built)
            try:
                same_frame(got, frame_of(fresh, cam, 4, reset=True, **other), "a change of kind")
            finally:
                fresh.close()
    finally:
        rr.close()
        comp.close()


def test_with_the_option_off_an_update_starts_over():
    """Check 17."""
    if not has_gpu():
        pytest.skip("no GPU")
    built, (s1, _), _ = config2_states()
    rr, fresh, comp = context(8, built, motion=0), context(8, s1, motion=0), Composition(8, built)
    try:
        cam = camera(W, H)
        assert rr.get_option("temporal_motion") == 0
        # an unmoved scene's temporal frames are rt_temporal_device's
        for k in range(2):
            same_frame(frame_of(rr, cam, k), comp.frame(cam, k), f"unmoved frame {k}")
        rr.update_geometry(s1)
        same_frame(frame_of(rr, cam, 2), frame_of(fresh, cam, 2, reset=True), "the first frame after an update")
        assert rr.get_option("temporal_motion_used") == 0
        # turned on after the upload: a scene's first update still starts over (the uploaded records were not
        # staged), the second one keeps the history
        late = context(8, built, motion=0)
        try:
            frame_of(late, cam, 0)
            late.set_option("temporal_motion", 1)
            late.update_geometry(s1)
            same_frame(frame_of(late, cam, 3), frame_of(fresh, cam, 3, reset=True), "turned on after the upload")
            assert late.get_option("temporal_motion_used") == 0
            late.update_geometry(built)
            frame_of(late, cam, 4)
            assert late.get_option("temporal_motion_used") == 1
        finally:
            late.close()
        rr.set_option("temporal_motion", 1)
        frame_of(rr, cam, 5)
        # kept by an update, then the option turned off: the frame drops it
        rr.update_geometry(built)
        rr.set_option("temporal_motion", 0)
        fresh.upload_scene(built)
        same_frame(frame_of(rr, cam, 6), frame_of(fresh, cam, 6, reset=True), "the option turned off")
        assert rr.get_option("temporal_motion_used") == 0
        for v in (2, -1):
            with pytest.raises(Exception, match="INVALID_ARG"):
                rr.set_option("temporal_motion", v)
    finally:
        for c in (rr, fresh):
            c.close()
        comp.close()


# ---- 19. the engine ------------------------------------------------------------------------

def test_engine_with_motion():
    if not has_gpu():
        pytest.skip("no GPU")
    import time
    import rtamd
    built, (s1, s2), _ = config2_states()
    w, h = 96, 54
    q = rtamd.AtomicReference()
    eng = rtamd.HipEngine(q, w, h, BOUNCES, temporal=rtamd.TemporalParams(max_history=8), motion=True)
    eng.start()
    try:
        eng.submit_scene(built)
        eng.submit_camera_update(camera(w, h))
        seen = []
        for upd in (s1, s2):
            n0 = eng.frames_rendered
            deadline = time.time() + 30.0
            while eng.frames_rendered < n0 + 2 and eng.error is None and time.time() < deadline:
                time.sleep(0.002)
            seen.append(eng.frames_rendered)
            eng.submit_geometry_update(upd)
        deadline = time.time() + 30.0
        while ((eng.geometry_updates < 2 or eng.frames_rendered < seen[-1] + 2) and eng.error is None
               and time.time() < deadline):
            time.sleep(0.002)
    finally:
        eng.stop()
    assert eng.error is None, eng.error
    assert eng.geometry_updates == 2 and eng.frames_rendered >= seen[-1] + 2 > seen[0] >= 2
    assert q.get() is not None
