"""Ray queries on the GPU (rt_query_rays*, rt_render_hits_device, rt_pick;
include/rtamd.h "queries"), bit for bit against
tests/query_ref.py (the reference's closest hit in numpy, pinned to the CPU
oracle by tests/test_query_ref.py).

Ray sources here are the rays of jittered perspective cameras: primary rays
and the per-bounce rays oracle/shader_np.py hands out (their origins lie on
surfaces, so T_MIN matters), over random soups, the tie scenes and the
adversarial scenes of the accel model's tests.  Such rays almost never have a
zero, negative-zero or denormal component, an origin in a box plane, a hit
exactly on an edge or a t_max equal to a hit's t: those are the rays of
tests/designed_rays.py, queried in tests/test_gpu_designed_rays.py.  Every
test runs on the accel tree in 8 layouts and in 1, and on the reference's own
tree (accel 0).
"""
import functools
import os
import sys

import numpy as np
import pytest

import query_ref as Q
from conftest import has_gpu

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
MODES = [8, 1, 0]
ALL_MODES = MODES + ["half", "wide"]


@pytest.fixture(scope="module")
def qr():
    if not has_gpu():
        pytest.skip("no GPU")
    import rtamd
    r = rtamd.Renderer((0,))
    yield r
    r.close()


def _upload(r, built, mode):
    """mode: option accel (8, 1, 0), or "half" / "wide": accel 8 in that record format."""
    r.set_option("accel_half", 1 if mode == "half" else 0)
    r.set_option("accel_wide", 1 if mode == "wide" else 0)
    r.set_option("accel", mode if isinstance(mode, int) else 8)
    r.upload_scene(built)
    if isinstance(mode, int):
        assert r.get_option("accel_used") == mode
    else:
        assert r.get_option(f"accel_{mode}_used") == 1


def _same(got, want, what=""):
    """Hit records equal bit for bit (NaN-free by construction; -0.0 != 0.0 matters)."""
    if got.tobytes() == want.tobytes():
        return
    bad = np.nonzero(got.view(np.uint32).reshape(len(got), 8) != want.view(np.uint32).reshape(len(want), 8))[0]
    i = int(bad[0])
    raise AssertionError(f"{what}: {len(np.unique(bad))} of {len(got)} records differ; first {i}: "
                         f"got {got[i]} want {want[i]}")


class Case:
    """A scene, its rays (bounce by bounce) and the reference's hits of them."""

    def __init__(self, built, cam, w, h, b):
        self.built, self.cam, self.w, self.h = built, cam, w, h
        self.rays = Q.segment_rays(built.model_vertex_data, built.model_material_data, built.flat_bvh_data,
                                   cam.ubo_bytes(), w, h, b)
        self.ref, self.nv, self.nt = self.hits_of(self.rays)

    def hits_of(self, rays):
        return Q.closest_hits(self.built.model_vertex_data, self.built.flat_bvh_data, rays)


@functools.lru_cache(maxsize=None)
def _soup(seed):
    from rtamd import build_buffers, configs
    from test_accel_model import random_scene
    verts, mats, (eye, at), vfov = random_scene(seed)
    w, h = 64, 48
    return Case(build_buffers(verts, mats, 1 + seed % 3), configs.Camera(eye, at, (0.0, 1.0, 0.0), vfov, w / h),
                w, h, 3)


@functools.lru_cache(maxsize=None)
def _ties():
    from rtamd import configs
    from test_accel_model import _tie_scenes
    w, h = 97, 61
    return {name: Case(built, configs.Camera.default(w, h), w, h, 3) for name, built in _tie_scenes().items()}


@functools.lru_cache(maxsize=None)
def _adversarial(name):
    from rtamd import build_buffers, configs
    tools = os.path.join(os.path.dirname(HERE), "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import accel_adversarial
    verts, mats, (eye, at), vfov = accel_adversarial.SCENES[name](0.3)
    w, h = 120, 68
    return Case(build_buffers(verts, mats, 1), configs.Camera(eye, at, (0.0, 1.0, 0.0), vfov, w / h), w, h, 3)


def _group(name):
    if name == "soups":
        return {f"soup{s}": _soup(s) for s in (0, 3, 5, 11, 17, 22)}
    if name == "ties":
        return _ties()
    return {name: _adversarial(name)}


GROUPS = ["soups", "ties", "slivers", "grazing", "far_origin_1e6_near"]


# (accel_half / accel_wide scenes are queried over their reference records: the soups only)
@pytest.mark.parametrize("group,mode", [(g, m) for g in GROUPS for m in MODES] + [("soups", "half"), ("soups", "wide")])
def test_closest_hits(qr, group, mode):
    """Every ray of every bounce: t, tri, normal and pos are the reference's."""
    for name, c in _group(group).items():
        _upload(qr, c.built, mode)
        got, st = qr.query_rays(c.rays, stats=True)
        _same(got, c.ref, f"{name} accel {mode}")
        assert st["pixels"] == len(c.rays) and st["segments"] == len(c.rays) and st["mat_reads"] == 0
        if mode in (0, "half", "wide"):                      # the reference's records: the reference DFS's counts
            assert st["node_visits"] == int(c.nv.sum()) and st["tri_tests"] == int(c.nt.sum()), name
        assert (c.ref["tri"] >= 0).any() and (c.ref["tri"] < 0).any(), name


@pytest.mark.parametrize("mode", MODES)
def test_ragged_counts(qr, mode):
    """The first n rays of a batch; lanes past n_rays neither load nor store."""
    import torch
    c = _ties()["grid"]
    assert len(c.rays) > 4097
    _upload(qr, c.built, mode)
    d_rays = torch.from_numpy(c.rays.view(np.float32).reshape(-1, 8).copy()).to("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    for n in (1, 63, 64, 65, 4097):
        d_hits = torch.full((n + 192, 8), -7.5, dtype=torch.float32, device="cuda:0")
        assert qr.query_rays_device(d_rays.data_ptr(), n, d_hits.data_ptr(), stream=stream) is None
        torch.cuda.synchronize()
        out = d_hits.cpu().numpy()
        _same(out[:n].view(Q.HIT_DTYPE)[:, 0], c.ref[:n], f"first {n} rays, accel {mode}")
        assert (out[n:] == np.float32(-7.5)).all(), f"{n} rays: bytes past the records were written"
        _same(qr.query_rays(c.rays[:n]), c.ref[:n], f"host form, first {n} rays")


def test_query_argument_checks(qr):
    import torch
    from rtamd import RtError
    c = _ties()["grid"]
    _upload(qr, c.built, 8)
    d = torch.zeros((64, 8), dtype=torch.float32, device="cuda:0")
    for args in [(d.data_ptr(), 0, d.data_ptr()), (d.data_ptr(), (1 << 26) + 1, d.data_ptr()),
                 (d.data_ptr() + 4, 8, d.data_ptr()), (d.data_ptr(), 8, d.data_ptr() + 8), (None, 8, d.data_ptr())]:
        with pytest.raises(RtError, match="INVALID_ARG"):
            qr.query_rays_device(*args)
    with pytest.raises(RtError, match="INVALID_ARG"):
        qr.query_rays(np.zeros((0, 8), np.float32))
    cam = c.cam
    for tile in [(0, 0, 98, 61), (-1, 0, 4, 4), (96, 60, 2, 1), (0, 0, 0, 4)]:
        with pytest.raises(RtError, match="INVALID_ARG"):
            qr.render_hits(cam, 97, 61, tile=tile)
    for (x, y) in [(-1, 0), (97, 0), (0, 61)]:
        with pytest.raises(RtError, match="INVALID_ARG"):
            qr.pick(cam, 97, 61, x, y)


@pytest.mark.parametrize("mode", MODES)
def test_t_max(qr, mode):
    """closest_t starts at the ray's t_max: the compare is strict, t_max <=
    T_MIN cannot hit, NaN and >= T_MAX are T_MAX; on accel 0 the walk's counts
    are the reference's for that t_max, so t_max really culls."""
    c = _ties()["cube_both_diagonals"]
    _upload(qr, c.built, mode)
    hit = c.ref["tri"] >= 0
    t0 = c.ref["t"]
    inf = np.float32(np.inf)
    variants = {
        "t0": np.where(hit, t0, Q.T_MAX),
        "above t0": np.where(hit, np.nextafter(t0, inf), Q.T_MAX),
        "t0 / 2": np.where(hit, t0 / np.float32(2), Q.T_MAX),
        "T_MIN": np.full(len(t0), 0.001),
        "below T_MIN": np.where(np.arange(len(t0)) % 2 == 0, 0.0005, -1.0),
        "NaN": np.full(len(t0), np.nan),
        "2e4": np.full(len(t0), 2.0e4),
        "inf": np.where(np.arange(len(t0)) % 2 == 0, np.inf, -np.inf),
    }
    visits = {}
    for name, tm in variants.items():
        rays = c.rays.copy()
        rays["t_max"] = tm.astype(np.float32)
        want, nv, nt = c.hits_of(rays)
        got, st = qr.query_rays(rays, stats=True)
        _same(got, want, f"t_max = {name}, accel {mode}")
        assert st["segments"] == len(rays)
        visits[name] = st["node_visits"]
        if mode == 0:
            assert st["node_visits"] == int(nv.sum()) and st["tri_tests"] == int(nt.sum()), name
        # what the reference says of each variant
        if name == "t0":           # strict: the same triangle at the same t is no hit
            assert (~hit | (want["tri"] != c.ref["tri"]) | (want["t"] < t0)).all()
            assert (want["tri"][hit] == -1).mean() > 0.9
        elif name == "above t0":   # the same hit, unless it lies before its own leaf box's t_enter
            lost = np.nonzero(hit & (want != c.ref))[0]
            assert len(lost) <= hit.sum() // 100
            assert not Q.leaf_box_entered(c.built.flat_bvh_data, rays[lost], c.ref["tri"][lost],
                                          rays["t_max"][lost]).any()
        elif name == "t0 / 2":     # a miss or a nearer hit
            assert (~hit | (want["tri"] == -1) | (want["t"] < t0)).all()
        elif name in ("T_MIN", "below T_MIN"):
            assert (want["tri"] == -1).all() and np.array_equal(want["t"], tm.astype(np.float32))
        elif name in ("NaN", "2e4"):
            _same(want, c.ref, name)
        elif name == "inf":
            even = np.arange(len(t0)) % 2 == 0
            _same(want[even], c.ref[even], name)
            assert (want["tri"][~even] == -1).all() and (want["t"][~even] == -inf).all()
    if mode == 0:
        assert visits["t0 / 2"] < visits["2e4"] and visits["T_MIN"] < visits["t0 / 2"]


@pytest.mark.parametrize("mode", MODES)
def test_non_unit_directions(qr, mode):
    """Half the batch with directions scaled by 0.5 and by 3: used as given
    (the accel tree hands such rays to the reference-order walk)."""
    for c in (_soup(5), _ties()["twins"]):
        _upload(qr, c.built, mode)
        rays = c.rays.copy()
        k = np.arange(len(rays)) % 4
        rays["dir"][k == 1] *= np.float32(0.5)
        rays["dir"][k == 3] *= np.float32(3.0)
        want, _, _ = c.hits_of(rays)
        _same(qr.query_rays(rays), want, f"scaled directions, accel {mode}")
        # the scaled rays hit what the unit rays hit, at t / scale (up to rounding)
        assert np.array_equal(want["tri"][k % 2 == 0], c.ref["tri"][k % 2 == 0])
        assert (want["tri"][k == 3] == c.ref["tri"][k == 3]).mean() > 0.9
        # ... with a finite t_max as well: the re-walk starts from the ray's own
        hitk = (want["tri"] >= 0)
        rays["t_max"] = np.where(hitk, want["t"] * np.float32(0.75), 5.0).astype(np.float32)
        want2, _, _ = c.hits_of(rays)
        _same(qr.query_rays(rays), want2, f"scaled directions with t_max, accel {mode}")


@pytest.mark.parametrize("mode", MODES)
def test_invalid_rays(qr, mode):
    """NaN, inf or an all-zero direction: tri = -2, t = 0, not walked; the
    other lanes of the wave are unaffected."""
    c = _ties()["grid"]
    _upload(qr, c.built, mode)
    rays = c.rays[:256].copy()
    rays["origin"][5, 1] = np.nan
    rays["dir"][70, 0] = np.inf
    rays["dir"][130] = 0.0
    rays["origin"][131, 2] = -np.inf
    rays["dir"][255, 2] = np.nan
    rays["dir"][17, 0] = 0.0                                # one zero component is a valid ray
    bad = np.zeros(256, bool)
    bad[[5, 70, 130, 131, 255]] = True
    want, _, _ = c.hits_of(rays)
    got, st = qr.query_rays(rays, stats=True)
    _same(got, want, f"invalid rays, accel {mode}")
    assert (got["tri"][bad] == -2).all() and not got["t"][bad].any() and not got["pos"][bad].any()
    keep = ~bad
    keep[17] = False
    _same(got[keep], c.ref[:256][keep], "neighbours of invalid rays")
    assert st["segments"] == 256 - 5 and st["pixels"] == 256


@pytest.mark.parametrize("mode", MODES)
def test_any_hit(qr, mode):
    """RT_QUERY_ANY: hit exactly where closest mode hits; every reported hit is
    a true intersection of its ray with T_MIN < t < t_max."""
    for c in (_soup(11), _ties()["cube_both_diagonals"], _adversarial("slivers")):
        _upload(qr, c.built, mode)
        rays = c.rays.copy()
        hit = c.ref["tri"] >= 0
        # a finite t_max on a third of the rays: beyond, at, and before the closest hit
        k = np.arange(len(rays)) % 6
        rays["t_max"] = np.where(k == 1, c.ref["t"] * np.float32(1.5),
                                 np.where(k == 3, c.ref["t"] * np.float32(0.5), Q.T_MAX)).astype(np.float32)
        want, _, _ = c.hits_of(rays)
        closest = qr.query_rays(rays)
        _same(closest, want, f"closest mode, accel {mode}")
        got, st = qr.query_rays(rays, any_hit=True, stats=True)
        assert np.array_equal(got["tri"] >= 0, want["tri"] >= 0)
        assert st["segments"] == len(rays)
        miss = got["tri"] < 0
        _same(got[miss], want[miss], "any-hit misses")
        tm = np.where(rays["t_max"] < Q.T_MAX, rays["t_max"], Q.T_MAX).astype(np.float32)
        idx, ok, t, nrm = Q.oracle_triangle_hits(c.built.model_vertex_data, rays, got, tm)
        assert ok.all()                                       # T_MIN < t < t_max, inside the triangle
        assert np.array_equal(t.view(np.uint32), got["t"][idx].view(np.uint32))
        assert np.array_equal(nrm.view(np.uint32), got["normal"][idx].view(np.uint32))
        pos = (rays["origin"][idx] + rays["dir"][idx] * got["t"][idx, None]).astype(np.float32)
        assert np.array_equal(pos.view(np.uint32), got["pos"][idx].view(np.uint32))
        assert (got["t"][idx] >= want["t"][idx]).all()        # never nearer than the closest hit
        # the device form of a first-hit buffer takes the flag too
        a = qr.render_hits(c.cam, c.w, c.h, any_hit=True)
        b = qr.render_hits(c.cam, c.w, c.h)
        assert np.array_equal(a["tri"] >= 0, b["tri"] >= 0)


@functools.lru_cache(maxsize=None)
def _config2():
    from rtamd import configs
    cfg = configs.config2()
    return cfg, cfg.build(), configs.Camera.default(160, 90)


@pytest.mark.parametrize("mode", MODES)
def test_render_hits(qr, mode):
    """The first-hit buffer: every pixel's own primary ray (:164-173), row-major."""
    cfg, built, cam = _config2()
    w, h = 160, 90
    _upload(qr, built, mode)
    _, rad, _ = qr.render(cam, w, h, 1, radiance=True)
    black = (rad == 0).all(-1)                                # a 1-bounce hit is black, the sky never is
    for tile in (None, (3, 5, 61, 37), (159, 89, 1, 1)):
        x0, y0, tw, th = tile or (0, 0, w, h)
        rays = Q.primary_rays(cam.ubo_bytes(), w, h, tile)
        want, nv, nt = Q.closest_hits(built.model_vertex_data, built.flat_bvh_data, rays)
        got, st = qr.render_hits(cam, w, h, tile=tile, stats=True)
        assert got.shape == (th, tw)
        _same(got.reshape(-1), want, f"render_hits tile {tile}, accel {mode}")
        _same(qr.query_rays(rays), want, f"query_rays of the primary rays, tile {tile}")
        assert np.array_equal(got["tri"] >= 0, black[y0:y0 + th, x0:x0 + tw])
        assert st["pixels"] == tw * th and st["segments"] == tw * th and st["mat_reads"] == 0
        if mode == 0:
            assert st["node_visits"] == int(nv.sum()) and st["tri_tests"] == int(nt.sum())
    assert black.any() and not black.all()


@pytest.mark.parametrize("mode", MODES)
def test_pick(qr, mode):
    import rtamd
    cfg, built, cam = _config2()
    w, h = 160, 90
    _upload(qr, built, mode)
    buf = qr.render_hits(cam, w, h)
    for (x, y) in [(0, 0), (159, 89), (80, 45), (37, 61), (81, 44)]:
        p = qr.pick(cam, w, h, x, y)
        assert p.tobytes() == buf[y, x].tobytes(), (x, y)
    centre = qr.pick(cam, w, h, w // 2, h // 2)
    assert centre["tri"] >= 0
    assert rtamd.instance_of(cfg.scene, built, int(centre["tri"])).display_name == "Cube"
    ground = qr.pick(cam, w, h, 5, 85)
    assert rtamd.instance_of(cfg.scene, built, int(ground["tri"])).display_name == "Ground Plane"
    assert qr.pick(cam, w, h, 5, 2)["tri"] == -1              # the sky


@pytest.mark.parametrize("ext", [0, 8])
@pytest.mark.parametrize("mode", MODES)
def test_render_state_untouched(qr, mode, ext):
    """A render, then queries, then the same render: identical frames, and
    plain_kernels (by which a profiler trace is cut) counts the renders only.
    With the sphere extension on, queries still see triangles only."""
    import torch
    cfg, built, cam = _config2()
    w, h = 160, 90
    _upload(qr, built, mode)
    qr.set_option("extensions", ext)
    try:
        if ext:
            qr.upload_spheres(np.array([[0.0, 6.0, 0.0, 6.0, 0.9, 0.2, 0.2, 0.0]], np.float32))
        d = torch.empty((h, w, 4), dtype=torch.uint8, device="cuda:0")
        stream = torch.cuda.current_stream().cuda_stream

        def frame():
            qr.render_tile_device(cam, w, h, 4, 0, 0, w, h, d.data_ptr(), None, stream)
            torch.cuda.synchronize()
            return d.cpu().numpy().copy()

        before = [frame() for _ in range(3)]                  # (the first may be a learning launch)
        pk0 = qr.get_option("plain_kernels")
        used0 = (qr.get_option("heavy_pixels_used"), qr.get_option("heavy_tiles_used"))
        rays = Q.primary_rays(cam.ubo_bytes(), w, h)
        want, _, _ = Q.closest_hits(built.model_vertex_data, built.flat_bvh_data, rays)
        _same(qr.query_rays(rays), want, f"query between renders, extensions {ext}")
        _same(qr.render_hits(cam, w, h).reshape(-1), want, f"render_hits between renders, extensions {ext}")
        qr.query_rays(rays, any_hit=True, stats=True)
        qr.pick(cam, w, h, 80, 45)
        assert qr.get_option("plain_kernels") == pk0
        assert (qr.get_option("heavy_pixels_used"), qr.get_option("heavy_tiles_used")) == used0
        after = [frame() for _ in range(2)]
        assert pk0 < qr.get_option("plain_kernels") <= pk0 + 4     # one or two kernels per frame
        for f in before[1:] + after:
            assert np.array_equal(f, before[0])
        if ext:                                               # the sphere is in the frame, not in the queries
            qr.set_option("extensions", 0)
            assert not np.array_equal(frame(), before[0])
    finally:
        qr.set_option("extensions", 0)
        qr.upload_spheres(np.zeros((0, 8), np.float32))


@pytest.mark.parametrize("mode", MODES)
def test_empty_and_one_triangle_scenes(qr, mode):
    from raw_bvh import raw_bvh_scene
    from rtamd import build_buffers, configs, triangles_of
    verts, mats = triangles_of(configs.config2().scene)
    w, h = 48, 32
    cam = configs.Camera.default(w, h)
    rays = Q.primary_rays(cam.ubo_bytes(), w, h)
    # an empty scene: all misses
    empty = build_buffers(verts[:0], mats[:0])
    qr.set_option("accel_half", 0)
    qr.set_option("accel_wide", 0)
    qr.set_option("accel", mode)
    qr.upload_scene(empty)
    got, st = qr.query_rays(rays, stats=True)
    assert (got["tri"] == -1).all() and (got["t"] == Q.T_MAX).all() and not got["pos"].any()
    assert st["segments"] == len(rays) and st["node_visits"] == 0 and st["tri_tests"] == 0
    assert (qr.render_hits(cam, w, h)["tri"] == -1).all()
    assert qr.pick(cam, w, h, 24, 16)["tri"] == -1
    # one triangle: the builder's root with the triangle twice (the accel tree's
    # root is a leaf), and a hand-built tree whose root is the leaf
    for name, built in [("built", build_buffers(verts[:1], mats[:1])), ("raw", raw_bvh_scene(1, "random", 4)),
                        ("two", build_buffers(verts[:2], mats[:2]))]:
        qr.upload_scene(built)
        want, nv, nt = Q.closest_hits(built.model_vertex_data, built.flat_bvh_data, rays)
        got, st = qr.query_rays(rays, stats=True)
        _same(got, want, f"{name} one-triangle scene, accel {mode}")
        _same(qr.render_hits(cam, w, h).reshape(-1), want, f"{name}: render_hits")
        assert (want["tri"] >= 0).any(), name
        if mode == 0:
            assert st["node_visits"] == int(nv.sum()) and st["tri_tests"] == int(nt.sum())
