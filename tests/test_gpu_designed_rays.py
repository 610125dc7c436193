"""The designed rays and cameras of tests/designed_rays.py on the GPU: zero,
negative-zero and denormal direction components, origins in box planes (NaN
slab products), hits on edges and vertices, tied hits, origins on a triangle,
t_max equal to a hit's own t.  tests/test_designed_rays.py shows on the CPU that
the battery and the cameras reach those inputs and that tests/query_ref.py
and the accel model equal the oracle on them.

Bar (no tolerance anywhere): hit records equal tests/query_ref.py's bit for
bit; frames (RGBA8 and radiance bits) equal the oracle's; counters the
oracle's on the reference's tree and the accel model's on the accel tree.
Every copy of the slab / triangle arithmetic in rt_trace.hip is walked: the
lockstep walk (walk 0 and 2), the cooperative tail (the reference's tree), the
wide tree's packed slab, the solo walk (solo_lanes 1) and split kernel 2.
"""
import functools

import numpy as np
import pytest

import designed_rays as D
import query_ref as Q
from conftest import has_gpu
from test_designed_rays import B, H, W, _oracle_frame
from test_gpu_accel import HALF8, WIDE, _check, _model
from test_gpu_accel import _upload as _upload_layouts
from test_gpu_query import ALL_MODES, _same, _upload
from test_gpu_split_pack import _options

pytestmark = pytest.mark.gpu

SOLO = [0, 1]
INF = np.float32(np.inf)


@pytest.fixture(scope="module")
def dr():
    if not has_gpu():
        pytest.skip("no GPU")
    import rtamd
    r = rtamd.Renderer((0,))
    yield r
    r.close()


def _hits_of(rays):
    s = D.scene()
    return Q.closest_hits(s.model_vertex_data, s.flat_bvh_data, rays)


@functools.lru_cache(maxsize=None)
def _battery_ref():
    """The battery, the reference's hits of it and its walk's counts."""
    rays, tags = D.battery()
    return (rays, tags) + _hits_of(rays)


@functools.lru_cache(maxsize=None)
def _t_max_variants():
    """{name: (rays, hits, node visits, triangle tests)}: the battery under each t_max."""
    rays, _, ref, _, _ = _battery_ref()
    hit = ref["tri"] >= 0
    t0 = np.where(hit, ref["t"], Q.T_MAX).astype(np.float32)
    out = {}
    for name, tm in (("t0", t0), ("above t0", np.where(hit, np.nextafter(t0, INF), Q.T_MAX)),
                     ("T_MIN", np.full(len(rays), Q.T_MIN)),
                     ("above T_MIN", np.full(len(rays), np.nextafter(Q.T_MIN, INF)))):
        r = rays.copy()
        r["t_max"] = tm.astype(np.float32)
        out[name] = (r,) + _hits_of(r)
    # what the reference says of them (the contract, not the kernel under test)
    want = out["t0"][1]
    assert (~hit | (want["tri"] != ref["tri"]) | (want["t"] < t0)).all()     # strict: the same hit is gone
    assert (out["T_MIN"][1]["tri"] == -1).all() and (out["above T_MIN"][1]["tri"] == -1).all()
    assert (out["above t0"][1]["tri"][hit] >= 0).mean() > 0.9
    return out


@functools.lru_cache(maxsize=None)
def _primary_ref(name):
    return _hits_of(Q.primary_rays(D.cameras()[name], W, H))


@functools.lru_cache(maxsize=None)
def _model_frame(name, nl):
    return _model(D.scene(), D.cameras()[name], W, H, B, nl)


def _solo_used(mode, solo):
    """solo_lanes walks format-0 accel records only."""
    return solo if mode in (1, 8) else 0


# ------------------------------------------------------------- the battery --

@pytest.mark.parametrize("solo", SOLO)
@pytest.mark.parametrize("mode", ALL_MODES)
def test_battery_closest_hits(dr, mode, solo):
    """Every battery ray's record is the reference's; on the reference's
    records (accel 0; half and wide scenes are queried over them) so are the
    node and triangle counts."""
    rays, tags, ref, nv, nt = _battery_ref()
    _upload(dr, D.scene(), mode)
    with _options(dr, solo_lanes=solo):
        got, st = dr.query_rays(rays, stats=True)
        assert dr.get_option("solo_lanes_used") == _solo_used(mode, solo)
    for c in D.CLASSES:                                       # (names the class of the first difference)
        _same(got[tags == c], ref[tags == c], f"class {c}, accel {mode}, solo_lanes {solo}")
    assert st["pixels"] == len(rays) and st["segments"] == len(rays) and st["mat_reads"] == 0
    if mode in (0, "half", "wide"):
        assert (st["node_visits"], st["tri_tests"]) == (int(nv.sum()), int(nt.sum()))


@pytest.mark.parametrize("solo", SOLO)
@pytest.mark.parametrize("mode", ALL_MODES)
def test_battery_t_max(dr, mode, solo):
    """closest_t starting at the hit's own t (strict: that hit is gone, a tied
    twin too), one ulp above it, at T_MIN and one ulp above T_MIN."""
    _upload(dr, D.scene(), mode)
    with _options(dr, solo_lanes=solo):
        for name, (rays, want, nv, nt) in _t_max_variants().items():
            got, st = dr.query_rays(rays, stats=True)
            _same(got, want, f"t_max = {name}, accel {mode}, solo_lanes {solo}")
            assert st["segments"] == len(rays)
            if mode in (0, "half", "wide"):
                assert (st["node_visits"], st["tri_tests"]) == (int(nv.sum()), int(nt.sum())), name


@pytest.mark.parametrize("solo", SOLO)
@pytest.mark.parametrize("mode", ALL_MODES)
def test_battery_any_hit(dr, mode, solo):
    """RT_QUERY_ANY: a hit exactly where closest mode hits, and every reported
    hit a true intersection by the contract's hit_triangle."""
    s = D.scene()
    rays, _, want, _, _ = _battery_ref()
    _upload(dr, s, mode)
    with _options(dr, solo_lanes=solo):
        got, st = dr.query_rays(rays, any_hit=True, stats=True)
    assert np.array_equal(got["tri"] >= 0, want["tri"] >= 0)
    assert st["segments"] == len(rays)
    miss = got["tri"] < 0
    _same(got[miss], want[miss], "any-hit misses")
    idx, ok, t, nrm = Q.oracle_triangle_hits(s.model_vertex_data, rays, got, np.full(len(rays), Q.T_MAX))
    assert ok.all()
    assert np.array_equal(t.view(np.uint32), got["t"][idx].view(np.uint32))
    assert np.array_equal(nrm.view(np.uint32), got["normal"][idx].view(np.uint32))
    pos = (rays["origin"][idx] + rays["dir"][idx] * got["t"][idx, None]).astype(np.float32)
    assert np.array_equal(pos.view(np.uint32), got["pos"][idx].view(np.uint32))
    assert (got["t"][idx] >= want["t"][idx]).all()


@pytest.mark.parametrize("mode", ALL_MODES)
def test_battery_device_form(dr, mode):
    """The device form with a ragged last wave: the records are the
    reference's and the rows past them are untouched."""
    import torch
    rays, _, ref, _, _ = _battery_ref()
    n = len(rays)
    assert n % 64 not in (0, 63)
    _upload(dr, D.scene(), mode)
    d_rays = torch.from_numpy(rays.view(np.float32).reshape(-1, 8).copy()).to("cuda:0")
    d_hits = torch.full((n + 192, 8), -7.5, dtype=torch.float32, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    assert dr.query_rays_device(d_rays.data_ptr(), n, d_hits.data_ptr(), stream=stream) is None
    torch.cuda.synchronize()
    out = d_hits.cpu().numpy()
    _same(out[:n].view(Q.HIT_DTYPE)[:, 0], ref, f"device form, accel {mode}")
    assert (out[n:] == np.float32(-7.5)).all(), "bytes past the records were written"


# ------------------------------------------------------------- the cameras --

# (layouts of test_gpu_accel._upload, option walk): the accel tree in its four
# formats, and the reference's own tree with both lockstep walks
RENDER_MODES = [(1, 2), (8, 2), (HALF8, 2), (WIDE, 2), (0, 0), (0, 2)]


@pytest.mark.parametrize("solo", SOLO)
@pytest.mark.parametrize("nl,walk", RENDER_MODES)
def test_render_designed_cameras(dr, nl, walk, solo):
    """A learning, a counting and a plain launch of every designed camera:
    frames and radiance bits the oracle's, counters the model's (accel) or the
    oracle's (the reference's tree)."""
    s = D.scene()
    _upload_layouts(dr, s, nl)
    with _options(dr, solo_lanes=solo, walk=walk):
        for name, cam in D.cameras().items():
            ref = _oracle_frame(name)
            model = _model_frame(name, nl) if nl else ref
            for stats in (False, True, False):
                rgba, rad, st = dr.render(cam, W, H, B, radiance=True, stats=stats)
                _check(rgba, rad, st, ref, model, f"{name} layouts {nl} walk {walk} solo_lanes {solo} stats {stats}")
        assert dr.get_option("solo_lanes_used") == (solo if nl in (1, 8) else 0)


@pytest.mark.parametrize("solo", SOLO)
@pytest.mark.parametrize("split", [1, 2])
@pytest.mark.parametrize("nl", [1, 8])
def test_split_designed_cameras(dr, nl, split, solo):
    """Split kernel 2 re-reads origin and direction from its queue: the split
    frame is the unsplit one and the oracle's, with room for every path."""
    s = D.scene()
    _upload_layouts(dr, s, nl)
    with _options(dr, solo_lanes=solo, heavy_first=0, split_pixels=0, split_bounce=0, split_capacity=1024):
        dr.get_option("split_overflow")
        for name, cam in D.cameras().items():
            ref = _oracle_frame(name)
            dr.set_option("split_bounce", 0)
            base = dr.render(cam, W, H, B, radiance=True)
            assert dr.get_option("split_bounce_used") == 0
            dr.set_option("split_bounce", split)
            rgba, rad, _ = dr.render(cam, W, H, B, radiance=True)
            assert dr.get_option("split_bounce_used") == split, name
            tag = f"{name} layouts {nl} split {split} solo_lanes {solo}"
            _check(base[0], base[1], None, ref, None, tag + " (unsplit)")
            _check(rgba, rad, None, ref, None, tag)
            assert np.array_equal(rgba, base[0]) and np.array_equal(rad.view(np.uint32), base[1].view(np.uint32)), tag
        assert dr.get_option("split_overflow") == 0


@pytest.mark.parametrize("mode", ALL_MODES)
def test_render_hits_and_pick(dr, mode):
    """The first-hit buffer of every designed camera is query_ref's closest hit
    of its primary rays, and pick returns its records."""
    _upload(dr, D.scene(), mode)
    for name, cam in D.cameras().items():
        want, nv, nt = _primary_ref(name)
        got, st = dr.render_hits(cam, W, H, stats=True)
        _same(got.reshape(-1), want, f"render_hits {name}, accel {mode}")
        assert st["pixels"] == W * H and st["segments"] == W * H
        if mode == 0:
            assert (st["node_visits"], st["tri_tests"]) == (int(nv.sum()), int(nt.sum())), name
        for (x, y) in [(0, 0), (W - 1, H - 1), (W // 2, H // 2), (17, 3)]:
            assert dr.pick(cam, W, H, x, y).tobytes() == got[y, x].tobytes(), (name, x, y)
