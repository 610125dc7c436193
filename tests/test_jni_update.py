"""HipNative.updateGeometry (jni/HipNative.c) through the mock JNIEnv of
tests/test_jni_shim.py: the buffer checks and a null context throw
RuntimeException; on a GPU the frame after the shim's update is
Renderer.update_geometry's."""
import ctypes as C

import numpy as np
import pytest

from conftest import has_gpu
from test_jni_shim import PREFIX, JavaException, Jvm


def _jvm():
    jvm = Jvm()
    f = getattr(jvm.L, PREFIX + "updateGeometry")
    f.restype = None
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    jvm.fn["updateGeometry"] = f
    return jvm


def test_update_geometry_checks_buffers_and_context():
    jvm = _jvm()
    v = np.zeros(48 * 4, np.uint8)
    n = np.zeros(48 * 3, np.uint8)
    # heap buffers and null buffers: no rt_update_geometry call
    for a, b in [(jvm.L.mock_heap_buffer(), jvm.direct(n)), (jvm.direct(v), jvm.L.mock_heap_buffer()),
                 (None, jvm.direct(n)), (jvm.direct(v), None)]:
        with pytest.raises(JavaException, match="updateGeometry: need direct buffers") as ei:
            jvm.call("updateGeometry", 1, a, b)
        assert ei.value.cls == "java/lang/RuntimeException"
    # a null context: rt_update_geometry's status becomes the exception
    with pytest.raises(JavaException, match="rtamd error -1: rt_update_geometry: null context"):
        jvm.call("updateGeometry", 0, jvm.direct(v), jvm.direct(n))
    assert jvm.L.mock_outstanding() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("accel", [0, 8])
def test_update_geometry_through_the_shim(accel):
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
    cam = configs.Camera.default(W, H)
    with rtamd.Renderer((0,)) as r:
        r.set_option("accel", accel)
        r.set_option("refit", 1)
        r.upload_scene(built)
        before = r.render(cam, W, H, B)[0]
        r.update_geometry(new)
        want = r.render(cam, W, H, B)[0]
    assert (want != before).any()
    ctx = jvm.call("create", jvm.ints([0]))
    assert ctx != 0
    try:
        v = np.ascontiguousarray(built.model_vertex_data, dtype=np.float32)
        m = np.ascontiguousarray(built.model_material_data, dtype=np.float32)
        b = np.ascontiguousarray(built.flat_bvh_data, dtype=np.uint8)
        nv = np.ascontiguousarray(new.model_vertex_data, dtype=np.float32)
        nb = np.ascontiguousarray(new.flat_bvh_data, dtype=np.uint8)
        ubo = np.frombuffer(cam.ubo_bytes(), dtype=np.uint8).copy()
        out = np.zeros(W * H * 4, np.uint8)
        jvm.call("setOption", ctx, jvm.string("accel"), accel)
        jvm.call("uploadScene", ctx, jvm.direct(v), v.size * 4, jvm.direct(m), m.size * 4, jvm.direct(b), b.size)
        with pytest.raises(JavaException, match="rt_update_geometry: .*option refit"):
            jvm.call("updateGeometry", ctx, jvm.direct(nv), jvm.direct(nb))
        jvm.call("setOption", ctx, jvm.string("refit"), 1)
        jvm.call("uploadScene", ctx, jvm.direct(v), v.size * 4, jvm.direct(m), m.size * 4, jvm.direct(b), b.size)
        assert jvm.call("getOption", ctx, jvm.string("refit_used")) == 1
        jvm.call("render", ctx, jvm.direct(ubo), W, H, B, jvm.direct(out))
        assert np.array_equal(out.reshape(H, W, 4), before)
        jvm.call("updateGeometry", ctx, jvm.direct(nv), jvm.direct(nb))
        jvm.call("render", ctx, jvm.direct(ubo), W, H, B, jvm.direct(out))
        assert np.array_equal(out.reshape(H, W, 4), want)
        with pytest.raises(JavaException, match="rtamd error -4: rt_update_geometry"):
            jvm.call("updateGeometry", ctx, jvm.direct(nv[:-12]), jvm.direct(nb))
    finally:
        jvm.call("destroy", ctx)
