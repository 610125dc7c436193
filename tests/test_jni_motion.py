"""Option temporal_motion through the mock JNIEnv of tests/test_jni_shim.py
(DESIGN.md §4m): setOption("temporal_motion", 1), renderTemporal,
updateGeometry and renderTemporal of jni/HipNative.c give the frames of the
Python path, and the frame after the update ran the per-triangle kernel."""
import ctypes as C

import numpy as np
import pytest

from conftest import has_gpu
from test_jni_shim import PREFIX, Jvm
from test_jni_temporal import DEFAULTS


def _jvm():
    jvm = Jvm()
    f = getattr(jvm.L, PREFIX + "renderTemporal")
    f.restype = None
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float,
                  C.c_float, C.c_int32, C.c_int32, C.c_void_p]
    jvm.fn["renderTemporal"] = f
    f = getattr(jvm.L, PREFIX + "updateGeometry")
    f.restype = None
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    jvm.fn["updateGeometry"] = f
    return jvm


@pytest.mark.gpu
def test_an_update_keeps_the_history_through_the_shim():
    if not has_gpu():
        pytest.skip("no GPU")
    import rtamd
    from rtamd import build_buffers, configs, refit_buffers, triangles_of
    jvm = _jvm()
    tv, mats = triangles_of(configs.config2().scene)
    built = build_buffers(tv, mats, 1)
    moved = tv.reshape(-1, 3, 3).copy()
    moved[2:] += np.array([1.5, 0.25, -2.0])                    # the cube
    new = refit_buffers(built, moved)
    W, H, B = 160, 90, 4
    cams = []
    for k in range(3):
        cam = configs.Camera.default(W, H)
        cam.ubo.frame_count = k
        cams.append(cam)
    with rtamd.Renderer((0,)) as r:
        r.set_option("refit", 1)
        r.set_option("temporal_motion", 1)
        r.upload_scene(built)
        want = [r.render_temporal(c, W, H, B, reset=(k == 0))[0] for k, c in enumerate(cams[:2])]
        r.update_geometry(new)
        want.append(r.render_temporal(cams[2], W, H, B)[0])
        assert r.get_option("temporal_motion_used") == 1
        dropped = r.render_temporal(cams[2], W, H, B, reset=True)[0]
    assert (want[2] != dropped).any()                           # the kept history shows in the frame
    ctx = jvm.call("create", jvm.ints([0]))
    assert ctx != 0
    try:
        v = np.ascontiguousarray(built.model_vertex_data, dtype=np.float32)
        m = np.ascontiguousarray(built.model_material_data, dtype=np.float32)
        b = np.ascontiguousarray(built.flat_bvh_data, dtype=np.uint8)
        nv = np.ascontiguousarray(new.model_vertex_data, dtype=np.float32)
        nb = np.ascontiguousarray(new.flat_bvh_data, dtype=np.uint8)
        jvm.call("setOption", ctx, jvm.string("refit"), 1)
        jvm.call("setOption", ctx, jvm.string("temporal_motion"), 1)
        jvm.call("uploadScene", ctx, jvm.direct(v), v.size * 4, jvm.direct(m), m.size * 4, jvm.direct(b), b.size)
        out = np.zeros(W * H * 4, np.uint8)
        for k, c in enumerate(cams):
            if k == 2:
                jvm.call("updateGeometry", ctx, jvm.direct(nv), jvm.direct(nb))
            ubo = np.frombuffer(c.ubo_bytes(), dtype=np.uint8).copy()
            jvm.call("renderTemporal", ctx, jvm.direct(ubo), W, H, B, *DEFAULTS, 0, 1 if k == 0 else 0, jvm.direct(out))
            assert np.array_equal(out.reshape(H, W, 4), want[k]), k
            assert jvm.call("getOption", ctx, jvm.string("temporal_motion_used")) == (1 if k == 2 else 0)
    finally:
        jvm.call("destroy", ctx)
