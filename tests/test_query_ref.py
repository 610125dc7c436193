"""tests/query_ref.py (the numpy closest hit the GPU query tests compare with)
pinned to the CPU oracle, so it cannot drift: on primary rays its hit mask, its
node / triangle counts and every hit's t and normal are oracle/rt_oracle.c's."""
import numpy as np
import pytest

import query_ref as Q
from oracle import oracle_lib


def _cases():
    from rtamd import configs
    out = [(f"config{k}", k, 96, 64) for k in (1, 2)]
    out += [(f"soup{seed}", -seed, 64, 48) for seed in (0, 5, 11, 17)]
    return out


def _scene(k, w, h):
    from rtamd import build_buffers, configs
    if k > 0:
        cfg = configs.get(k)
        return cfg.build(), configs.Camera.default(w, h)
    from test_accel_model import random_scene
    verts, mats, (eye, at), vfov = random_scene(-k)
    return build_buffers(verts, mats, 1 + (-k) % 3), configs.Camera(eye, at, (0.0, 1.0, 0.0), vfov, w / h)


@pytest.mark.parametrize("name,k,w,h", _cases())
def test_query_ref_is_the_oracle(name, k, w, h):
    built, cam = _scene(k, w, h)
    assert_is_the_oracle(name, built, cam.ubo_bytes(), w, h, mixed=k != 1)


def assert_is_the_oracle(name, built, ubo, w, h, mixed=True):
    """query_ref on the primary rays of the camera `ubo` against a 1-bounce
    oracle frame; mixed: the frame must hold both hits and sky."""
    rays = Q.primary_rays(ubo, w, h)
    hits, nv, nt = Q.closest_hits(built.model_vertex_data, built.flat_bvh_data, rays)
    _, rad, cnt = oracle_lib.render(built.model_vertex_data, built.model_material_data, built.flat_bvh_data,
                                    ubo, w, h, 1)
    # a 1-bounce hit is always black (:229-231) and the sky never is (:81-85)
    black = (rad.reshape(-1, 3) == 0).all(1)
    assert np.array_equal(hits["tri"] >= 0, black), name
    assert (hits["tri"] >= -1).all()
    assert cnt["segments"] == len(rays)
    assert int(nv.sum()) == cnt["node_visits"] and int(nt.sum()) == cnt["tri_tests"], name
    if mixed:
        assert black.any() and not black.all(), name
    # every hit: the contract's hit_triangle on (ray, tri) gives the same t and normal bits
    idx, ok, t, nrm = Q.oracle_triangle_hits(built.model_vertex_data, rays, hits, np.full(len(rays), Q.T_MAX))
    assert ok.all()
    assert np.array_equal(t.view(np.uint32), hits["t"][idx].view(np.uint32))
    assert np.array_equal(nrm.view(np.uint32), hits["normal"][idx].view(np.uint32))
    # pos = origin + dir * t, unfused (:77-79); a miss: t_max and zeros
    want = (rays["origin"][idx] + rays["dir"][idx] * hits["t"][idx, None]).astype(np.float32)
    assert np.array_equal(want.view(np.uint32), hits["pos"][idx].view(np.uint32))
    miss = hits["tri"] == -1
    assert (hits["t"][miss] == Q.T_MAX).all() and not hits["normal"][miss].any() and not hits["pos"][miss].any()


def test_query_ref_t_max_and_invalid_rays():
    """t_max: strict compare, clamping, and the rays that are not walked."""
    from rtamd import configs
    cfg = configs.get(2)
    built, w, h = cfg.build(), 48, 32
    rays = Q.primary_rays(configs.Camera.default(w, h).ubo_bytes(), w, h)
    base, nv0, _ = Q.closest_hits(built.model_vertex_data, built.flat_bvh_data, rays)
    hit = base["tri"] >= 0
    assert hit.any()
    r = rays.copy()
    r["t_max"][hit] = base["t"][hit]                       # t < closest_t is strict: the same triangle is a miss
    got, nv1, _ = Q.closest_hits(built.model_vertex_data, built.flat_bvh_data, r)
    assert ((got["tri"] != base["tri"]) | ~hit).all()
    assert (nv1 <= nv0).all()
    r["t_max"][hit] = np.nextafter(base["t"][hit], np.float32(np.inf))
    got, _, _ = Q.closest_hits(built.model_vertex_data, built.flat_bvh_data, r)
    # just above t0 the hit is the same, except where it lies before its own leaf
    # box's t_enter: that box is entered only while closest_t is above its t_enter
    lost = np.nonzero(hit & (got != base))[0]
    assert len(lost) <= hit.sum() // 100
    assert not Q.leaf_box_entered(built.flat_bvh_data, r[lost], base["tri"][lost], r["t_max"][lost]).any()
    for tm in (np.nan, 2.0e4, np.inf):
        r["t_max"] = tm
        got, _, _ = Q.closest_hits(built.model_vertex_data, built.flat_bvh_data, r)
        assert got.tobytes() == base.tobytes()
    r["t_max"] = 0.001
    got, _, _ = Q.closest_hits(built.model_vertex_data, built.flat_bvh_data, r)
    assert (got["tri"] == -1).all() and (got["t"] == np.float32(0.001)).all()
    bad = rays[:4].copy()
    bad["origin"][0, 1] = np.nan
    bad["dir"][1, 0] = np.inf
    bad["dir"][2] = 0.0
    got, nv, nt = Q.closest_hits(built.model_vertex_data, built.flat_bvh_data, bad)
    assert list(got["tri"][:3]) == [-2, -2, -2] and not got["t"][:3].any() and not nv[:3].any()
    assert got[3].tobytes() == base[3].tobytes()
