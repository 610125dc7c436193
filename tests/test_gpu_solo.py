"""GPU parity of option solo_lanes (rt_trace.hip solo_walk):
the format-0 accel walk's last lanes finished one ray at a time from records
read through the scalar cache.

Bar, as in test_gpu_accel.py (no tolerance anywhere): RGBA8 and the radiance
bits equal the CPU oracle's, segments and material reads the oracle's, node
visits and triangle tests the accel model's; and every launch is compared with
the same launch at solo_lanes 0 (the lockstep walk alone).  solo_lanes 64
sends every step of every ray through solo_walk.  Each case runs the learning
launch (the diag build), a counting launch and a plain launch.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import query_ref as Q
from conftest import has_gpu
from test_gpu_accel import HALF8, WIDE, _check, _oracle, _upload

pytestmark = pytest.mark.gpu

SOLO = (1, 2, 64)


@pytest.fixture(scope="module")
def solo():
    if not has_gpu():
        pytest.skip("no GPU")
    import rtamd
    r = rtamd.Renderer((0,))
    yield r
    r.close()


@functools.lru_cache(maxsize=None)
def _built(name):
    from rtamd import build_buffers, configs, triangles_of
    if name in ("c2", "c3"):
        return configs.get({"c2": 2, "c3": 3}[name]).build()
    if name.startswith("tri"):
        verts, mats = triangles_of(configs.config2().scene)
        n = int(name[3:])
        return build_buffers(verts[:n], mats[:n])
    if name == "slivers":
        from test_gpu_accel import _adversarial
        verts, mats, _, _ = _adversarial().SCENES["slivers"](0.3)
        return build_buffers(verts, mats, 1)
    from test_accel_model import _tie_scenes
    return _tie_scenes()[name]


@functools.lru_cache(maxsize=None)
def _records(name, nl):
    from rtamd import _lib
    return _lib.accel_records(_built(name), nl)


def _model(name, cam, w, h, b, nl):
    """The accel model's frame and counts (the scene's records built once)."""
    from oracle import oracle_lib
    built = _built(name)
    rec, info = _records(name, nl)
    return oracle_lib.render_accel(built.model_vertex_data, built.model_material_data, built.flat_bvh_data,
                                   cam.ubo_bytes(), w, h, b, rec, info)


def _frames(r, name, cam, w, h, b, nl, solos, what):
    """Renders at solo_lanes 0 and at each of `solos`: every launch against the
    oracle and the model, and against the launch at solo_lanes 0."""
    built = _built(name)
    ref = _oracle(built, cam, w, h, b)
    model = _model(name, cam, w, h, b, nl)
    base = {}
    try:
        for s in (0,) + tuple(solos):
            r.set_option("solo_lanes", s)
            for i, stats in enumerate((False, True, False)):
                rgba, rad, st = r.render(cam, w, h, b, radiance=True, stats=stats)
                tag = f"{what} {w}x{h} b{b} layouts {nl} solo_lanes {s} launch {i}"
                assert r.get_option("solo_lanes_used") == s, tag
                _check(rgba, rad, st, ref, model, tag)
                if s == 0:
                    base[i] = (rgba, rad, st)
                else:
                    assert np.array_equal(rgba, base[i][0]), tag
                    assert np.array_equal(rad.view(np.uint32), base[i][1].view(np.uint32)), tag
                    if stats:
                        assert {k: st[k] for k in ("segments", "node_visits", "tri_tests", "mat_reads")} == \
                               {k: base[i][2][k] for k in ("segments", "node_visits", "tri_tests", "mat_reads")}, tag
    finally:
        r.set_option("solo_lanes", -1)


# (a) ------------------------------------------------------------------------
@pytest.mark.parametrize("nl", [1, 8])
@pytest.mark.parametrize("name", ["c2", "c3"])
def test_solo_small_frames(solo, name, nl):
    """1x1; 17x1 (the second 16x4 wave tile holds one pixel: solo from the
    first record); one full tile; 33x5 and 64x36 (partial tiles, several
    waves); 1 and 4 bounces."""
    from rtamd import configs
    _upload(solo, _built(name), nl)
    for (w, h) in [(1, 1), (17, 1), (16, 4), (33, 5), (64, 36)]:
        cam = configs.Camera.default(w, h)
        for b in (1, 4):
            _frames(solo, name, cam, w, h, b, nl, SOLO, name)


# (b) ------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2, 3])
def test_solo_empty_and_tiny_scenes(solo, n):
    """No record at all, a root that is a leaf (root_leaf), and roots whose
    walk starts inside them (root_enter)."""
    from rtamd import configs
    for nl in (1, 8):
        _upload(solo, _built(f"tri{n}"), nl)
        for (w, h, b) in [(37, 23, 3), (1, 1, 1)]:
            _frames(solo, f"tri{n}", configs.Camera.default(w, h), w, h, b, nl, (1, 64), f"{n} triangles")


# (c) ------------------------------------------------------------------------
@pytest.mark.parametrize("nl", [1, 8])
@pytest.mark.parametrize("name", ["twins", "grid", "cube_both_diagonals", "slivers"])
def test_solo_ties_fallback_and_forced_records(solo, name, nl):
    """The tie scenes (hits before their own box's t_enter: incons, then the
    reference-order re-walk) and the slivers (forced records), every step
    through solo_walk."""
    from rtamd import configs
    _upload(solo, _built(name), nl)
    if name == "slivers":
        from test_gpu_accel import _adversarial
        _, _, (eye, at), vfov = _adversarial().SCENES["slivers"](0.3)
        w, h, b = 120, 68, 4
        cam = configs.Camera(eye, at, (0.0, 1.0, 0.0), vfov, w / h)
        _frames(solo, name, cam, w, h, b, nl, (64,), name)
    else:
        for (w, h, b) in [(80, 45, 3), (97, 61, 10)]:
            _frames(solo, name, configs.Camera.default(w, h), w, h, b, nl, (64,), name)


# (d) ------------------------------------------------------------------------
@pytest.mark.parametrize("nl", [1, 8])
def test_solo_queries(solo, nl):
    """rt_query_rays, closest and any-hit, 1 ray and 65 rays (one full wave and
    a wave of one ray), with a finite t_max on some rays and a non-unit
    direction (never walked by solo_walk: the reference-order re-walk)."""
    from test_gpu_query import _same, _ties, _adversarial
    for c in (_ties()["cube_both_diagonals"], _adversarial("slivers")):
        _upload(solo, c.built, nl)
        hit = np.nonzero(c.ref["tri"] >= 0)[0]
        # 65 rays, hits and misses mixed
        pick = np.concatenate([hit[:: max(1, len(hit) // 40)][:40], np.nonzero(c.ref["tri"] < 0)[0][:25]])[:65]
        assert len(pick) == 65
        rays = c.rays[pick].copy()
        k = np.arange(65) % 6
        rays["t_max"] = np.where(k == 1, c.ref["t"][pick] * np.float32(1.5),
                                 np.where(k == 3, c.ref["t"][pick] * np.float32(0.5), Q.T_MAX)).astype(np.float32)
        rays["dir"][7] *= np.float32(3.0)
        rays["dir"][63] *= np.float32(0.5)
        for n in (1, 65):
            batch = rays[:n]
            want, _, _ = c.hits_of(batch)
            base = {}
            try:
                for s in (0, 1, 2, 64):
                    solo.set_option("solo_lanes", s)
                    got, st = solo.query_rays(batch, stats=True)
                    assert solo.get_option("solo_lanes_used") == s
                    _same(got, want, f"closest, {n} rays, layouts {nl}, solo_lanes {s}")
                    _same(solo.query_rays(batch), want, f"closest (plain), {n} rays, solo_lanes {s}")
                    anyh, sa = solo.query_rays(batch, any_hit=True, stats=True)
                    assert np.array_equal(anyh["tri"] >= 0, want["tri"] >= 0)
                    miss = anyh["tri"] < 0
                    _same(anyh[miss], want[miss], "any-hit misses")
                    tm = np.where(batch["t_max"] < Q.T_MAX, batch["t_max"], Q.T_MAX).astype(np.float32)
                    idx, ok, t, _ = Q.oracle_triangle_hits(c.built.model_vertex_data, batch, anyh, tm)
                    assert ok.all() and np.array_equal(t.view(np.uint32), anyh["t"][idx].view(np.uint32))
                    if s == 0:
                        base = (got, st, anyh, sa)
                    else:
                        _same(got, base[0], f"closest vs solo_lanes 0 ({s})")
                        _same(anyh, base[2], f"any-hit vs solo_lanes 0 ({s})")
                        for key in ("segments", "node_visits", "tri_tests", "mat_reads"):
                            assert st[key] == base[1][key] and sa[key] == base[3][key], (key, s)
            finally:
                solo.set_option("solo_lanes", -1)


# (e) ------------------------------------------------------------------------
def _launch_both(r, case, nl, what):
    """The case's launch at solo_lanes 0 and 1 (learning, counting, plain): each
    verified against the oracle and the model, and the two outputs equal."""
    import torch
    from rtamd._lib import Stats, check
    from test_gpu_edges import _Guarded, _verify
    s = torch.cuda.current_stream().cuda_stream
    outs = {}
    try:
        for sl in (0, 1):
            r.set_option("solo_lanes", sl)
            for i, stats in enumerate((False, True, False)):
                out = _Guarded(case.rows, case.width)
                st = Stats(*([0xAB] * 4), 171.0, 0xAB) if stats else None
                check(case.launch(out.rgba_ptr, out.rad_ptr, C.byref(st) if st is not None else None, s))
                torch.cuda.synchronize()
                assert r.get_option("solo_lanes_used") == sl
                _verify(case, out, st, nl, f"{what} solo_lanes {sl} launch {i}")
                rgba, rad = out.read()
                if sl == 0:
                    outs[i] = (rgba.copy(), rad.copy())
                else:
                    assert np.array_equal(rgba, outs[i][0]) and np.array_equal(rad.view(np.uint32),
                                                                               outs[i][1].view(np.uint32)), what
    finally:
        r.set_option("solo_lanes", -1)


def test_solo_batch_paths(solo):
    """One 2-frame rt_render_batch_device launch with a band list, and one
    rt_render_batch_lists_device launch with -1 padding rows (config 3's
    scene, 65 x 9: partial tiles)."""
    import test_gpu_edges as E
    _upload(solo, E._scene("c3"), 8)
    w, h = 65, 9
    _launch_both(solo, E.case_batch(solo, "c3", w, h, 2, band_h=3, bands=[0, 2]), 8, "batch with a band list")
    _launch_both(solo, E.case_lists(solo, "c3", w, h, 3, [[0, 1, 2], [1], []]), 8, "per-frame lists")


# (f) ------------------------------------------------------------------------
def _diag_records(r):
    from rtamd import lib
    from rtamd._lib import check
    n = C.c_size_t()
    check(lib().rt_diag_copy(r._ctx, None, 0, C.byref(n)))
    buf = np.zeros(max(8, n.value), np.uint64)
    check(lib().rt_diag_copy(r._ctx, buf.ctypes.data, n.value, C.byref(n)))
    return buf[: n.value // 8 * 8].reshape(-1, 8)


def test_solo_learning_replay_and_diag(solo):
    """A learning launch and its replay with solo_lanes 1: the frames are the
    oracle's; a diag launch's records keep their meaning (a lane's steps, the
    longest lane's, their sum: drec[7] <= 64 * drec[4]) and equal the records
    at solo_lanes 0 word for word (a ray's steps do not depend on who walks
    them)."""
    from rtamd import configs
    name, w, h, b = "c3", 128, 72, 4
    built = _built(name)
    cam = configs.Camera.default(w, h)
    ref = _oracle(built, cam, w, h, b)
    _upload(solo, built, 8)
    recs = {}
    try:
        for s in (0, 1):
            solo.set_option("solo_lanes", s)
            for i in range(2):                                   # the learning launch, then its replay
                rgba, rad, _ = solo.render(cam, w, h, b, radiance=True)
                _check(rgba, rad, None, ref, None, f"solo_lanes {s} launch {i}")
                assert solo.get_option("solo_lanes_used") == s
            # (no learned order: the records of both settings then lie in raster order)
            solo.set_option("heavy_first", 0)
            solo.set_option("diag", 1)
            try:
                rgba, rad, _ = solo.render(cam, w, h, b, radiance=True)
                _check(rgba, rad, None, ref, None, f"solo_lanes {s} diag launch")
                rec = _diag_records(solo)
            finally:
                solo.set_option("diag", 0)
                solo.set_option("heavy_first", 1)
            assert (rec[:, 4] > 0).any()
            assert (rec[:, 7] <= 64 * rec[:, 4]).all()
            recs[s] = rec[:, [4, 5, 7]].copy()
        assert np.array_equal(recs[0], recs[1])
    finally:
        solo.set_option("solo_lanes", -1)


@pytest.mark.parametrize("nl", [0, HALF8, WIDE])
def test_solo_does_not_apply(solo, nl):
    """The reference's tree and the half and wide formats: solo_lanes_used
    reads 0 whatever the option says, and the frames are unchanged."""
    from rtamd import configs
    built = _built("c2")
    w, h, b = 64, 36, 4
    cam = configs.Camera.default(w, h)
    ref = _oracle(built, cam, w, h, b)
    if nl == 0:
        solo.set_option("accel", 0)
        solo.upload_scene(built)
        assert solo.get_option("accel_used") == 0
    else:
        _upload(solo, built, nl)
    try:
        for s in (0, 1, 64):
            solo.set_option("solo_lanes", s)
            for stats in (False, True, False):
                rgba, rad, st = solo.render(cam, w, h, b, radiance=True, stats=stats)
                _check(rgba, rad, st, ref, None, f"layouts {nl} solo_lanes {s}")
                assert solo.get_option("solo_lanes_used") == 0
    finally:
        solo.set_option("solo_lanes", -1)
        solo.set_option("accel", 8)


def test_solo_with_cooperative_tail_or_extensions(solo):
    """A launch that runs the cooperative tail, or extensions, is not touched."""
    from rtamd import configs
    built = _built("c2")
    w, h, b = 64, 36, 4
    cam = configs.Camera.default(w, h)
    ref = _oracle(built, cam, w, h, b)
    _upload(solo, built, 8)
    try:
        solo.set_option("solo_lanes", 2)
        solo.set_option("coop_lanes", 8)
        rgba, rad, st = solo.render(cam, w, h, b, radiance=True, stats=True)
        _check(rgba, rad, st, ref, None, "coop_lanes 8")
        assert solo.get_option("solo_lanes_used") == 0
        solo.set_option("coop_lanes", -1)
        rgba, rad, st = solo.render(cam, w, h, b, radiance=True, stats=True)
        assert solo.get_option("solo_lanes_used") == 2
    finally:
        solo.set_option("solo_lanes", -1)
        solo.set_option("coop_lanes", -1)
