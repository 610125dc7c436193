"""rt_build_scene_map (the input triangle of every flattened triangle),
rtamd.instance_of, and the query entry points' argument checks (no device)."""
import ctypes as C

import numpy as np
import pytest


def _soup(n, seed=3):
    rng = np.random.default_rng(seed + n)
    verts = rng.uniform(-10, 10, (n, 9))
    mats = np.concatenate([rng.uniform(0.1, 0.9, (n, 3)), rng.integers(0, 3, (n, 1))], 1).astype(np.float32)
    return verts, mats


@pytest.mark.parametrize("n", [1, 2, 3, 7, 1000])
def test_source_map(n):
    from rtamd import _lib, build_buffers
    verts, mats = _soup(n)
    built = build_buffers(verts, mats, 4)
    src = built.flat_source
    assert src is not None and src.dtype == np.uint32 and src.shape == (built.triangle_count,)
    # every flattened triangle is the float cast of its input (Vec3.store), every input appears
    flat = built.model_vertex_data.reshape(-1, 3, 4)[:, :, :3].reshape(-1, 9)
    assert np.array_equal(flat, verts[src].astype(np.float32))
    assert np.array_equal(built.model_material_data.reshape(-1, 4), mats[src])
    assert set(src.tolist()) == set(range(n))
    # (the flattener writes a triangle twice when a range holds one)
    assert built.triangle_count >= n and (n != 1 or list(src) == [0, 0])
    # the buffers are rt_build_scene's, byte for byte
    L = _lib.lib()
    v = np.full(built.model_vertex_data.size, np.nan, np.float32)
    m = np.full(built.model_material_data.size, np.nan, np.float32)
    b = np.full(built.flat_bvh_data.size, 0xAB, np.uint8)
    fp, dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
    tv = np.ascontiguousarray(verts, np.float64)
    _lib.check(L.rt_build_scene(tv.ctypes.data_as(dp), mats.ctypes.data_as(fp), n, 4, 0, v.ctypes.data_as(fp),
                                m.ctypes.data_as(fp), b.ctypes.data_as(C.c_void_p)))
    assert v.tobytes() == built.model_vertex_data.tobytes()
    assert m.tobytes() == built.model_material_data.tobytes()
    assert b.tobytes() == built.flat_bvh_data.tobytes()
    # ... and with a NULL map, through the new entry point
    v2, m2, b2 = np.zeros_like(v), np.zeros_like(m), np.zeros_like(b)
    _lib.check(L.rt_build_scene_map(tv.ctypes.data_as(dp), mats.ctypes.data_as(fp), n, 4, 0, v2.ctypes.data_as(fp),
                                    m2.ctypes.data_as(fp), b2.ctypes.data_as(C.c_void_p), None))
    assert v2.tobytes() == v.tobytes() and m2.tobytes() == m.tobytes() and b2.tobytes() == b.tobytes()


def test_source_map_thread_independent():
    from rtamd import build_buffers
    verts, mats = _soup(40000, seed=9)
    a, b = build_buffers(verts, mats, 2, n_threads=1), build_buffers(verts, mats, 2, n_threads=8)
    assert np.array_equal(a.flat_source, b.flat_source)


def test_instance_of_config2():
    import rtamd
    from rtamd import configs
    cfg = configs.config2()
    built = cfg.build()
    names = [rtamd.instance_of(cfg.scene, built, t).display_name for t in range(built.triangle_count)]
    # the plane's 2 triangles and the cube's 12, wherever the flattener put them
    assert sorted(set(names)) == ["Cube", "Ground Plane"]
    mat_type = built.model_material_data.reshape(-1, 4)[:, 3]      # the plane is Lambertian, the cube metal
    for t, name in enumerate(names):
        assert (name == "Ground Plane") == (mat_type[t] == 0.0)
    assert names.count("Cube") >= 12 and names.count("Ground Plane") >= 2
    with pytest.raises(IndexError):
        rtamd.instance_of(cfg.scene, built, built.triangle_count)
    # a model that fails to load is skipped, as triangles_of skips it
    s = rtamd.Scene()
    s.add_instance(rtamd.ModelInstance("/nonexistent/model.obj", "Missing"))
    for inst in cfg.scene.get_instances():
        s.add_instance(inst)
    built2 = rtamd.SceneBuilder(1).build_scene(s)
    assert [rtamd.instance_of(s, built2, t).display_name for t in range(built2.triangle_count)] == names


def test_query_null_context_is_invalid_arg():
    """No device is touched before the arguments are checked."""
    from rtamd import _lib
    L = _lib.lib()
    rays = np.zeros((4, 8), np.float32)
    hits = np.zeros((4, 8), np.float32)
    assert L.rt_query_rays(None, rays.ctypes.data, 4, 0, hits.ctypes.data, None) == -1
    assert b"rt_query_rays" in L.rt_last_error()
    assert L.rt_query_rays_device(None, rays.ctypes.data, 4, 0, hits.ctypes.data, None, None) == -1
    cam = _lib.CameraUBO()
    hit = _lib.Hit()
    assert L.rt_pick(None, C.byref(cam), 64, 48, 1, 1, C.byref(hit)) == -1
    assert L.rt_render_hits_device(None, C.byref(cam), 64, 48, 0, 0, 64, 48, 0, hits.ctypes.data, None, None) == -1
    assert C.sizeof(_lib.Ray) == 32 and C.sizeof(_lib.Hit) == 32
