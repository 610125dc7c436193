"""rt_update_geometry_device on the GPU (include/rtamd.h): moved
triangles that already live on the device must leave the scene bit for bit as
the host path does (rt_refit_scene, then rt_update_geometry).

Two contexts, both uploaded with option refit 1: A also with refit_device 1 and
updated from a tensor, B updated from refit_buffers' host buffers.  After every
update the six record arrays, frames, counters, first-hit buffers, picks and
ray queries of A are B's.  The scenes and deformations are tests/refit_ref.py's."""
import functools
import re

import numpy as np
import pytest

import query_ref as Q
import refit_ref as R
from conftest import has_gpu

pytestmark = pytest.mark.gpu

W, H, BOUNCES = 64, 48, 3
MODES = [(8, 2), (1, 1), (0, 2), (0, 1)]           # (option accel, option leaf_align)
ARRAYS = range(6)                                  # rt_scene_copy_records' which
COUNTERS = ("segments", "mat_reads", "node_visits", "tri_tests")


@pytest.fixture(scope="module")
def ctx():
    """(A: the device path, B: the host path, a third context for fresh uploads)"""
    if not has_gpu():
        pytest.skip("no GPU")
    import rtamd
    rs = [rtamd.Renderer((0,)) for _ in range(3)]
    yield rs
    for r in rs:
        r.close()


def _upload(r, built, mode, device, refit=1, half=0):
    accel, align = mode
    r.set_option("accel_half", half)
    r.set_option("accel_wide", 0)
    r.set_option("accel", accel)
    r.set_option("leaf_align", align)
    r.set_option("refit", refit)
    r.set_option("refit_device", device)
    r.upload_scene(built)
    assert r.get_option("accel_used") == accel
    assert r.get_option("refit_device_used") == (1 if device and refit and not half else 0)


def _frame(r, cam, stats=False):
    return r.render(cam, W, H, BOUNCES, radiance=True, stats=stats)


def _same_frame(a, b, what):
    assert np.array_equal(a[0], b[0]), f"{what}: RGBA8 differs"
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), f"{what}: radiance differs"


def _arrays(r):
    return [r.copy_records(w) for w in ARRAYS]


def _same_arrays(a, b, what, skip=()):
    for w in ARRAYS:
        if w in skip:
            continue
        assert a[w].size == b[w].size, (what, w)
        assert np.array_equal(a[w], b[w]), f"{what}: array {w} differs in {int((a[w] != b[w]).sum())} of {a[w].size} words"


def _cuda(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _source(built):
    src = built.flat_source if built.flat_source is not None else []       # an empty scene has none
    return _cuda(np.asarray(src).astype(np.int32))


@functools.lru_cache(maxsize=None)
def _scene(name):
    from rtamd import build_buffers
    tv, mats, seed, part, cam = R.scene(name)
    return build_buffers(tv, mats, seed), cam


def _same_scene(a, b, cam, what, skip=()):
    """Everything the contract names: arrays, a frame with its counters, first hits, picks, a ray batch."""
    _same_arrays(_arrays(a), _arrays(b), what, skip)
    fa, fb = _frame(a, cam, stats=True), _frame(b, cam, stats=True)
    _same_frame(fa, fb, what)
    for k in COUNTERS:
        assert fa[2][k] == fb[2][k], (what, k, fa[2][k], fb[2][k])
    assert a.render_hits(cam, W, H).tobytes() == b.render_hits(cam, W, H).tobytes(), f"{what}: first hits differ"
    for x, y in ((W // 2, H // 2), (3, H - 2)):
        assert a.pick(cam, W, H, x, y).tobytes() == b.pick(cam, W, H, x, y).tobytes(), f"{what}: pick differs"
    if a.copy_records(2).size:
        rays = Q.primary_rays(cam.ubo_bytes(), W, H)[::5]
        assert a.query_rays(rays).tobytes() == b.query_rays(rays).tobytes(), f"{what}: ray batch differs"


# ------------------------------------------------------------------ 1. bit parity --

@pytest.mark.parametrize("kind", R.DEFORMATIONS)
@pytest.mark.parametrize("name", R.SCENES)
def test_device_update_is_the_host_update(ctx, name, kind):
    from rtamd import RtError, refit_buffers
    A, B, _ = ctx
    built, cam = _scene(name)
    tv, _, _, part, _ = R.scene(name)
    src = _source(built)
    states = [(moved, refit_buffers(built, moved)) for moved in R.deform(kind, tv, part)]
    for mode in MODES:
        what = f"{name} {kind} accel {mode[0]} leaf_align {mode[1]}"
        _upload(A, built, mode, 1)
        _upload(B, built, mode, 0)
        for r in (A, B):
            _frame(r, cam)                  # a plain launch learns a tile order; the next one uses it
        last = _frame(A, cam)
        for moved, new in states:
            try:
                B.update_geometry(new)
                refused = False
            except RtError as e:            # broken duplicates: only the accel build drops any
                assert mode[0] and re.search("BAD_SCENE.*dropped", str(e)), (what, str(e))
                refused = True
            if refused:
                with pytest.raises(RtError, match="BAD_SCENE.*dropped"):
                    A.update_geometry_device(_cuda(moved), src)
                _same_frame(_frame(A, cam), last, what + " after the refusal")
                continue
            ms = A.update_geometry_device(_cuda(moved), src, ms=True)
            assert ms >= 0.0
            _same_scene(A, B, cam, what)
            last = _frame(A, cam)


# ------------------------------------------------------------ 2. both input forms --

@pytest.mark.parametrize("mode", [(8, 2), (0, 1)])
@pytest.mark.parametrize("name", ["random1", "config2", "tris5"])
def test_float32_and_flattened_inputs(ctx, name, mode):
    A, B, _ = ctx
    built, cam = _scene(name)
    tv, _, _, part, _ = R.scene(name)
    moved = R.deform("jitter", tv, part)[0].astype(np.float32)      # float-representable vertices
    src = np.asarray(built.flat_source).astype(np.int64)
    _upload(A, built, mode, 1)
    _upload(B, built, mode, 1)
    B.update_geometry_device(_cuda(moved.astype(np.float64)), _source(built))
    want = _arrays(B)
    A.update_geometry_device(_cuda(moved), _source(built))
    _same_arrays(_arrays(A), want, f"{name} {mode}: float32 input")
    _upload(A, built, mode, 1)
    A.update_geometry_device(_cuda(moved.astype(np.float64)[src]))  # already in flattened order
    _same_arrays(_arrays(A), want, f"{name} {mode}: source=None")
    _upload(A, built, mode, 1)
    A.update_geometry_device(_cuda(moved[src]))                     # both at once
    _same_arrays(_arrays(A), want, f"{name} {mode}: float32, source=None")
    _same_frame(_frame(A, cam), _frame(B, cam), f"{name} {mode}")


# --------------------------------------------------------- 3. designed vertices --

F32_MAX = 3.4028234e38


def _designed(n):
    """A soup of n triangles, the first ones overwritten with designed vertices."""
    rng = np.random.default_rng(7 + n)
    tv = (rng.uniform(-20, 20, (n, 1, 3)) + rng.normal(size=(n, 3, 3)) * 3.0)
    d = [
        # signed zeros, a float subnormal, double subnormals that cast to signed float zeros
        [[-0.0, 0.0, 1e-40], [1e-320, -1e-320, 5.0], [3.0, -0.0, -1e-40]],
        [[1e-320, 1e-320, -1e-320], [-4.0, 6.0, -0.0], [-1e-320, 0.0, 2.0]],
        # zero extent on z only; the largest x is -0.0, which the z pad's + 0.0 turns into +0.0
        [[-1.0, 0.0, 1.0], [-0.0, 2.0, 1.0], [-0.5, -3.0, 1.0]],
        # zero extent on y and z (a segment); the largest x is -0.0 again
        [[-3.0, 1.0, 1.0], [-1.0, 1.0, 1.0], [-0.0, 1.0, 1.0]],
        # zero extent on all three (a point at -0.0)
        [[-0.0, -0.0, -0.0]] * 3,
        # extents just below (x) and just above (y) 1e-4
        [[2.0, 2.0, 0.0], [2.0 + 0.99e-4, 2.0 + 1.01e-4, 1.0], [2.0, 2.0, 3.0]],
        # the largest float
        [[F32_MAX, 1.0, 1.0], [0.0, 0.0, 0.0], [1.0, 0.0, 1.0]],
    ]
    at = np.linspace(0, n - 1, len(d)).astype(int)          # the first, the last, and between
    tv[at] = np.array(d, dtype=np.float64)
    return tv.reshape(n, 9), at


@pytest.mark.parametrize("n", [256, 300])
def test_designed_vertices(ctx, n):
    from rtamd import build_buffers, configs, refit_buffers
    A, B, _ = ctx
    rng = np.random.default_rng(n)
    base = (rng.uniform(-20, 20, (n, 1, 3)) + rng.normal(size=(n, 3, 3)) * 3.0).reshape(n, 9)
    mats = np.concatenate([rng.uniform(0.1, 0.9, (n, 3)), rng.integers(0, 3, (n, 1))], 1).astype(np.float32)
    built = build_buffers(base, mats, 2)
    flat = built.triangle_count
    assert flat == 256 if n == 256 else (flat > 256 and flat % 256 != 0), flat     # one exact, one ragged last workgroup
    moved, at = _designed(n)
    # on the CPU first: every pad branch and the + 0.0 rule are in the input
    v = moved.reshape(n, 3, 3)
    raw_lo, raw_hi = v.min(1), v.max(1)
    pads = ((raw_hi - raw_lo) < R.EPS).sum(1)
    assert {1, 2, 3} <= set(pads[at].tolist()) and 0 in pads[at]
    lo, hi = R.tri_boxes(moved)
    jhi = R._jmax(v[:, 0], R._jmax(v[:, 1], v[:, 2]))                              # before the pads
    turned = np.signbit(jhi) & (jhi == 0) & ~np.signbit(hi) & (hi == 0)
    assert turned.any(), "no -0.0 maximum that a pad's + 0.0 turns into +0.0"
    ext = (raw_hi - raw_lo)[at]
    assert ((ext > 0.9e-4) & (ext < R.EPS)).any() and ((ext > R.EPS) & (ext < 1.1e-4)).any()
    assert np.isfinite(moved.astype(np.float32)).all() and (moved.astype(np.float32) == np.float32(F32_MAX)).any()
    f32 = moved.astype(np.float32)
    assert ((f32 == 0) & (moved != 0)).any() and ((f32 != 0) & (np.abs(f32) < 1.1754944e-38)).any()
    cam = configs.Camera.default(W, H)
    new = refit_buffers(built, moved)
    for mode in MODES:
        _upload(A, built, mode, 1)
        _upload(B, built, mode, 0)
        B.update_geometry(new)
        A.update_geometry_device(_cuda(moved), _source(built))
        _same_scene(A, B, cam, f"designed {n} {mode}")


# ------------------------------------------------------------------ 4. refusals --

def _raw(r, ptr, n_tris, src_ptr, n_flat, flags):
    from rtamd._lib import check, lib
    check(lib().rt_update_geometry_device(r._ctx, ptr, n_tris, src_ptr, n_flat, flags, None))


@pytest.mark.parametrize("mode", [(8, 2), (0, 1)])
def test_refusals(ctx, mode):
    import torch
    import rtamd
    from rtamd import RtError, refit_buffers
    A, B, _ = ctx
    built, cam = _scene("config2")
    tv, _, _, part, _ = R.scene("config2")
    moved = R.deform("translate", tv, part)[0]
    src_np = np.asarray(built.flat_source).astype(np.int32)
    src = _cuda(src_np)
    flat, n = built.triangle_count, len(moved)
    good = _cuda(moved)

    def refused(status, match, call):
        before = _frame(A, cam)
        arrays = _arrays(A)
        with pytest.raises(RtError, match=f"{status}.*{match}"):
            call()
        _same_frame(_frame(A, cam), before, f"after {status} {match}")
        _same_arrays(_arrays(A), arrays, f"after {status} {match}")

    # scenes without the device tables
    _upload(A, built, mode, 1, refit=0)
    refused("INVALID_ARG", "refit_device", lambda: A.update_geometry_device(good, src))
    _upload(A, built, mode, 0)
    refused("INVALID_ARG", "refit_device", lambda: A.update_geometry_device(good, src))
    if mode[0]:
        _upload(A, built, mode, 1, half=1)
        assert A.get_option("accel_half_used") == 1 and A.get_option("refit_used") == 0
        refused("INVALID_ARG", "half", lambda: A.update_geometry_device(good, src))
    with rtamd.Renderer((0,)) as empty:
        empty.set_option("refit", 1)
        empty.set_option("refit_device", 1)
        with pytest.raises(RtError, match="NO_SCENE"):
            empty.update_geometry_device(good, src)

    _upload(A, built, mode, 1)
    _upload(B, built, mode, 0)
    # the first flattened copy of an input triangle, at a first, a middle and a last flattened index
    where = [0, flat // 2, flat - 1]
    for bad in (np.nan, np.inf, 3.5e38):
        x = moved.copy()
        for f in where:
            x[src_np[f], 4] = bad
        lowest = min(int(np.flatnonzero(src_np == src_np[f])[0]) for f in where)
        assert lowest == 0
        refused("BAD_SCENE", r"triangle 0 has a vertex that is not finite", lambda: A.update_geometry_device(_cuda(x), src))
        for f in where[1:]:                                  # one triangle alone: its lowest flattened copy is named
            y = moved.copy()
            y[src_np[f], 8] = bad
            low = int(np.flatnonzero(src_np == src_np[f])[0])
            refused("BAD_SCENE", rf"triangle {low} has a vertex", lambda: A.update_geometry_device(_cuda(y), src))
    for f in (flat - 1, flat // 2):
        s = src_np.copy()
        s[f] = n
        s[flat - 1] = n
        refused("BAD_SCENE", rf"flattened triangle {f} copies", lambda: A.update_geometry_device(good, _cuda(s)))
    refused("INVALID_ARG", "n_flat", lambda: A.update_geometry_device(good, _cuda(np.append(src_np, 0).astype(np.int32))))
    refused("INVALID_ARG", "n_flat", lambda: A.update_geometry_device(good))                   # the method's n_flat = n_tris
    refused("INVALID_ARG", "flattened order", lambda: _raw(A, good.data_ptr(), n, None, flat, 0))   # n_tris != n_flat
    refused("INVALID_ARG", "n_tris 0", lambda: A.update_geometry_device(good[:0], src))
    refused("INVALID_ARG", "unknown flags", lambda: _raw(A, good.data_ptr(), n, src.data_ptr(), flat, 2))
    refused("INVALID_ARG", "null input", lambda: _raw(A, None, n, src.data_ptr(), flat, 0))
    room = torch.zeros(9 * n + 1, dtype=torch.float64, device="cuda")
    refused("INVALID_ARG", "aligned", lambda: _raw(A, room.data_ptr() + 4, n, src.data_ptr(), flat, 0))
    refused("INVALID_ARG", "aligned", lambda: _raw(A, good.data_ptr(), n, src.data_ptr() + 2, flat, 0))
    host = np.zeros(9 * n)                                    # refused before any kernel would read it
    refused("INVALID_ARG", "not device memory", lambda: _raw(A, host.ctypes.data, n, src.data_ptr(), flat, 0))
    if mode[0]:                                               # one copy of a doubled triangle moved alone
        f = int(np.flatnonzero(src_np[1:] == src_np[:-1])[0])
        alone = moved[src_np]
        alone[f + 1, 0] += 0.5
        refused("BAD_SCENE", "dropped", lambda: A.update_geometry_device(_cuda(alone)))
        host_alone = refit_buffers(built, moved)
        v = host_alone.model_vertex_data.copy()
        v[12 * (f + 1)] += np.float32(0.5)
        with pytest.raises(RtError, match="BAD_SCENE.*dropped"):    # the host form's wording, as above
            B.update_geometry(rtamd.BuiltCpuData(v, host_alone.model_material_data, host_alone.flat_bvh_data,
                                                 host_alone.triangle_count, host_alone.flat_source))
    # the staging arrays were not touched: a host update and a device update still behave
    new = refit_buffers(built, moved)
    A.update_geometry(new)
    B.update_geometry(new)
    _same_scene(A, B, cam, f"{mode}: a host update after the refusals")
    back = refit_buffers(built, tv)
    B.update_geometry(back)
    A.update_geometry_device(_cuda(tv), src)
    _same_scene(A, B, cam, f"{mode}: a device update after the refusals")


def test_refuses_a_context_of_two_devices():
    import torch
    import rtamd
    from rtamd import RtError
    if not has_gpu() or torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    built, _ = _scene("config2")
    tv = R.scene("config2")[0]
    with rtamd.Renderer((0, 1)) as r:
        r.set_option("refit", 1)
        r.set_option("refit_device", 1)
        r.upload_scene(built)
        with pytest.raises(RtError, match="INVALID_ARG.*2 devices"):
            r.update_geometry_device(_cuda(tv), _source(built))


# ----------------------------------------------------------------- 5. sequences --

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["random1", "config2"])
def test_updates_in_a_row(ctx, name, mode):
    from rtamd import refit_buffers
    A, B, fresh = ctx
    built, cam = _scene(name)
    tv, _, _, part, _ = R.scene(name)
    src = _source(built)
    one, two = R.deform("translate", tv, part)[0], R.deform("jitter", tv, part)[0]
    final = refit_buffers(built, two)
    _upload(fresh, final, mode, 0, refit=0)
    skip = (0,) if mode[0] else ()              # a fresh upload builds another accel tree
    for first, second in (("device", "device"), ("device", "host"), ("host", "device")):
        _upload(A, built, mode, 1)
        _upload(B, built, mode, 0)
        for how, moved in ((first, one), (second, two)):
            if how == "device":
                A.update_geometry_device(_cuda(moved), src)
            else:
                A.update_geometry(refit_buffers(built, moved))
            B.update_geometry(refit_buffers(built, moved))
        what = f"{name} {mode}: {first} then {second}"
        _same_scene(A, B, cam, what)
        _same_arrays(_arrays(A), _arrays(fresh), what + " (fresh upload)", skip)
        _same_frame(_frame(A, cam), _frame(fresh, cam), what + " (fresh upload)")


@pytest.mark.parametrize("mode", [(8, 2), (0, 2)])
def test_temporal_history_and_samples_sum(ctx, mode):
    from rtamd import RtError, configs, refit_buffers
    A, B, _ = ctx
    w, h = 64, 40
    built, cam0 = _scene("config2")
    tv, _, _, part, _ = R.scene("config2")
    moved = R.deform("translate", tv, part)[0]
    cam = configs.Camera(cam0.origin, cam0.look_at, cam0.v_up, cam0.vfov, w / h)
    out = []
    for r in (A, B):
        r.set_option("temporal_motion", 1)
    try:
        for r, device in ((A, 1), (B, 0)):
            _upload(r, built, mode, device)
            cam.frame_count = cam.ubo.frame_count = 0
            r.render_temporal(cam, w, h, BOUNCES, reset=True)
            r.render_samples(cam, w, h, BOUNCES, n_samples=4)
            if device:
                r.update_geometry_device(_cuda(moved), _source(built))
            else:
                r.update_geometry(refit_buffers(built, moved))
            cam.frame_count = cam.ubo.frame_count = 4
            with pytest.raises(RtError, match="INVALID_ARG.*holds 0 samples"):
                r.render_samples(cam, w, h, BOUNCES, n_samples=2)
            cam.frame_count = cam.ubo.frame_count = 1
            out.append(r.render_temporal(cam, w, h, BOUNCES, radiance=True))
            assert r.get_option("temporal_motion_used") == 1
    finally:
        for r in (A, B):
            r.set_option("temporal_motion", 0)
    _same_frame(out[0], out[1], f"{mode}: the temporal frame after the update")


# ------------------------------------------------- 6. the option leaves the rest --

@pytest.mark.parametrize("mode", MODES)
def test_option_changes_nothing_else(ctx, mode):
    A, B, _ = ctx
    for name in ("random2", "config2"):
        built, cam = _scene(name)
        _upload(A, built, mode, 1)
        _upload(B, built, mode, 0)
        nodes = built.n_nodes
        extra = A.get_option("refit_bytes") - B.get_option("refit_bytes")
        assert B.get_option("refit_bytes") > 0 and B.get_option("refit_device_used") == 0
        # 4 B per node, 16 B per dropped pair and the status words, each section rounded up to 16 B
        assert 4 * nodes + 16 <= extra <= 4 * nodes + 16 * nodes + 48, (extra, nodes)
        assert A.walk_bytes() == B.walk_bytes()
        _same_scene(A, B, cam, f"{name} {mode}: before any update")
        pk = [x.get_option("plain_kernels") for x in (A, B)]
        _same_frame(_frame(A, cam), _frame(B, cam), f"{name} {mode}")
        assert A.get_option("plain_kernels") - pk[0] == B.get_option("plain_kernels") - pk[1]
