"""The designed rays and cameras of tests/designed_rays.py on the CPU: they reach
the inputs they were designed for (conditions asserted on the reference
alone), and on them tests/query_ref.py and the accel walk's model
(oracle/rt_accel_model.c) equal the oracle (oracle/rt_oracle.c).

The inputs: direction components exactly +0.0, -0.0 or denormal, origins in
box planes (a NaN slab product, dropped by fmin / fmax), hits exactly on an
edge or vertex, hits that tie, origins on a triangle.  The GPU's walks meet
the same rays and cameras in tests/test_gpu_designed_rays.py.
"""
import functools

import numpy as np
import pytest

import designed_rays as D
import query_ref as Q
from oracle import oracle_lib

W, H, B = 64, 8, 4


@functools.lru_cache(maxsize=None)
def _battery_stats():
    rays, tags = D.battery()
    return rays, tags, D.stats(D.scene(), rays)


@functools.lru_cache(maxsize=None)
def _oracle_frame(name, b=B):
    s = D.scene()
    return oracle_lib.render(s.model_vertex_data, s.model_material_data, s.flat_bvh_data, D.cameras()[name], W, H, b)


# -------------------------------------------------------------- conditions --

def test_battery_conditions():
    """What the battery must reach, measured on the reference's own walk."""
    rays, tags, st = _battery_stats()
    assert set(tags) == set(D.CLASSES)
    n2 = (rays["dir"].astype(np.float64) ** 2).sum(1)
    unit = np.abs(n2 - 1.0) <= 2.0 ** -10
    assert unit[tags != "half"].all() and not unit[tags == "half"].any()
    assert (rays["dir"][tags == "axis"] ** 2).sum(1).tolist() == [1.0] * int((tags == "axis").sum())
    for c in D.CLASSES:
        m = tags == c
        share = st["hit"][m].mean()
        print(f"{c}: {int(m.sum())} rays, hit share {share:.3f}, NaN share {st['nan'][m].mean():.3f}, "
              f"edge hits {int(st['edge'][m].sum())}, tied hits {int(st['tie'][m].sum())}")
        if c != "surface":
            assert share >= 0.30 and 1.0 - share >= 0.30, (c, share)
        if c in ("axis", "plane", "diag"):
            assert st["nan"][m].mean() >= 0.95, (c, st["nan"][m].mean())
    print(f"all: {len(rays)} rays, edge hits {int(st['edge'].sum())}, tied hits {int(st['tie'].sum())}")
    assert st["edge"].sum() >= 200
    assert st["tie"].sum() >= 200
    # the signed zeros and the denormals are in the records as designed
    d = rays["dir"]
    assert ((d == 0) & np.signbit(d)).any(1)[tags == "axis"].mean() == 0.75
    assert ((d == 0) & ~np.signbit(d)).any(1)[tags == "axis"].mean() == 0.75
    assert ((d != 0) & (np.abs(d) < np.finfo(np.float32).tiny)).any(1)[tags == "denorm"].all()
    # surface origins: t == 0 on their own triangle, which T_MIN rejects
    hits, _, _ = Q.closest_hits(D.scene().model_vertex_data, D.scene().flat_bvh_data, rays[tags == "surface"])
    assert (hits["t"] > Q.T_MIN).all()


def test_camera_conditions():
    """Every designed camera sees the mesh, its primary rays have the component
    its kind promises, and no NaN reaches the oracle's radiance."""
    s = D.scene()
    cams = D.cameras()
    assert {n.split("_")[0] for n in cams} == set(D.KINDS)
    tiny = np.finfo(np.float32).tiny
    for name, u in cams.items():
        rays = Q.primary_rays(u, W, H)
        hits, _, _ = Q.closest_hits(s.model_vertex_data, s.flat_bvh_data, rays)
        d = rays["dir"]
        assert ((hits["tri"] >= 0).mean()) >= 0.25, name
        kind = name.split("_")[0]
        if kind in ("plane", "axis"):
            assert ((d == 0) & ~np.signbit(d)).any(1).all(), name
        if kind == "axis":
            assert (d == d[0]).all() and (np.abs(d[0]) == 1).sum() == 1 and (d[0] == 0).sum() == 2, name
        if kind == "diag":
            nz = np.abs(d[0][d[0] != 0])
            assert (d == d[0]).all() and len(nz) >= 2 and (np.isin(nz / nz.min(), (1.0, 2.0))).all(), name
        if kind == "negzero":
            assert ((d == 0) & np.signbit(d)).any(1).all(), name
        if kind == "denorm":
            assert ((d != 0) & (np.abs(d) < tiny)).any(1).mean() > 0.9, name
        _, rad, cnt = _oracle_frame(name)
        assert not np.isnan(rad).any(), name
        assert cnt["segments"] > W * H or kind in ("axis", "diag"), name         # paths go on past the first hit


# ------------------------------------------------------- query_ref = oracle --

def test_query_ref_is_the_oracle_on_designed_cameras():
    from test_query_ref import assert_is_the_oracle
    for name, u in D.cameras().items():
        assert_is_the_oracle(name, D.scene(), u, W, H, mixed=False)


@functools.lru_cache(maxsize=None)
def _one_ray_frames():
    """[(index in the battery, its one-ray camera)] for the axis and diag rays
    that a viewport can produce bit for bit (designed_rays.frame_of)."""
    rays, tags, _ = _battery_stats()
    out = []
    for i in np.nonzero((tags == "axis") | (tags == "diag"))[0]:
        u = D.frame_of(rays[i])
        if u is not None:
            out.append((int(i), u))
    return out


def test_battery_rays_are_the_oracles():
    """Battery rays as 1 x 1 frames of the oracle: query_ref's hit mask and
    node / triangle counts of each ray are the oracle's; and for every hit of
    the whole battery the contract's hit_triangle gives query_ref's t and
    normal bits."""
    s = D.scene()
    rays, tags, _ = _battery_stats()
    hits, nv, nt = Q.closest_hits(s.model_vertex_data, s.flat_bvh_data, rays)
    frames = _one_ray_frames()
    # the axis rays with two +0.0 and those with a -0.0 on an axis where the origin is 0; most diagonals
    assert sum(tags[i] == "axis" for i, _ in frames) >= (tags == "axis").sum() // 4 + 40
    assert sum(bool(((rays["dir"][i] == 0) & np.signbit(rays["dir"][i])).any()) for i, _ in frames) >= 40
    assert sum(tags[i] == "diag" for i, _ in frames) >= 0.9 * (tags == "diag").sum()
    for i, u in frames:
        _, rad, cnt = oracle_lib.render(s.model_vertex_data, s.model_material_data, s.flat_bvh_data, u, 1, 1, 1)
        assert bool((rad == 0).all()) == bool(hits["tri"][i] >= 0), i
        assert (cnt["segments"], cnt["node_visits"], cnt["tri_tests"]) == (1, nv[i], nt[i]), i
    idx, ok, t, nrm = Q.oracle_triangle_hits(s.model_vertex_data, rays, hits, np.full(len(rays), Q.T_MAX))
    assert ok.all()
    assert np.array_equal(t.view(np.uint32), hits["t"][idx].view(np.uint32))
    assert np.array_equal(nrm.view(np.uint32), hits["normal"][idx].view(np.uint32))


# ----------------------------------------------------------- model = oracle --

@pytest.mark.parametrize("nl,half", [(1, False), (8, False), (8, True), (8, "wide")])
def test_model_matches_oracle_on_designed_cameras(nl, half):
    from test_accel_model import _assert_frames_equal, _records
    s = D.scene()
    rec, info = _records(s, nl, half)
    for name, u in D.cameras().items():
        acc = oracle_lib.render_accel(s.model_vertex_data, s.model_material_data, s.flat_bvh_data, u, W, H, B,
                                      rec, info)
        _assert_frames_equal(_oracle_frame(name), acc, f"{name} layouts {nl} half {half}")


@pytest.mark.parametrize("nl,half", [(1, False), (8, False), (8, True), (8, "wide")])
def test_model_matches_oracle_on_battery_rays(nl, half):
    """The battery's axis and diag rays as 1 x 1 frames of 2 bounces: the
    model's frame is the oracle's.  (Rays through box corners and along box
    edges, where t_exit == t_enter, come from this class, not from a fan.)"""
    from test_accel_model import _assert_frames_equal, _records
    s = D.scene()
    rec, info = _records(s, nl, half)
    args = (s.model_vertex_data, s.model_material_data, s.flat_bvh_data)
    for i, u in _one_ray_frames():
        ref = oracle_lib.render(*args, u, 1, 1, 2)
        acc = oracle_lib.render_accel(*args, u, 1, 1, 2, rec, info)
        _assert_frames_equal(ref, acc, f"battery ray {i} layouts {nl} half {half}")
