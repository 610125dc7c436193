"""HipNative.pick (jni/HipNative.c) through the mock JNIEnv of
tests/test_jni_shim.py: the buffer checks and a null context throw
RuntimeException; on a GPU the hit record is Renderer.pick's."""
import numpy as np
import pytest

from conftest import has_gpu
from test_jni_shim import PREFIX, JavaException, Jvm

import ctypes as C


def _jvm():
    jvm = Jvm()
    f = getattr(jvm.L, PREFIX + "pick")
    f.restype = None
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                  C.c_void_p]
    jvm.fn["pick"] = f
    return jvm


def test_pick_checks_buffers_and_context():
    jvm = _jvm()
    ubo = np.zeros(80, np.uint8)
    hit = np.zeros(32, np.uint8)
    # a short hit buffer, a short UBO buffer, a heap buffer, a null buffer: no rt_pick call is made
    for u, h in [(jvm.direct(ubo), jvm.direct(hit[:31])), (jvm.direct(ubo[:79]), jvm.direct(hit)),
                 (jvm.direct(ubo), jvm.L.mock_heap_buffer()), (jvm.L.mock_heap_buffer(), jvm.direct(hit)),
                 (None, jvm.direct(hit)), (jvm.direct(ubo), None)]:
        with pytest.raises(JavaException, match="pick: need direct buffers") as ei:
            jvm.call("pick", 1, u, 64, 48, 1, 1, h)
        assert ei.value.cls == "java/lang/RuntimeException"
    assert not hit.any()
    # a null context: rt_pick's status becomes the exception
    with pytest.raises(JavaException, match="rtamd error -1: rt_pick: null context or camera"):
        jvm.call("pick", 0, jvm.direct(ubo), 64, 48, 1, 1, jvm.direct(hit))
    assert jvm.L.mock_outstanding() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("accel", [0, 8])
def test_pick_through_the_shim(accel):
    if not has_gpu():
        pytest.skip("no GPU")
    import rtamd
    from rtamd import configs
    from rtamd.engine import HIT_DTYPE
    jvm = _jvm()
    cfg = configs.config2()
    built = cfg.build()
    W, H = 160, 90
    cam = configs.Camera.default(W, H)
    with rtamd.Renderer((0,)) as r:
        r.set_option("accel", accel)
        r.upload_scene(built)
        want = {(x, y): r.pick(cam, W, H, x, y) for (x, y) in [(80, 45), (5, 85), (5, 2), (159, 89)]}
    ctx = jvm.call("create", jvm.ints([0]))
    assert ctx != 0
    try:
        v = np.ascontiguousarray(built.model_vertex_data, dtype=np.float32)
        m = np.ascontiguousarray(built.model_material_data, dtype=np.float32)
        b = np.ascontiguousarray(built.flat_bvh_data, dtype=np.uint8)
        jvm.call("setOption", ctx, jvm.string("accel"), accel)
        jvm.call("uploadScene", ctx, jvm.direct(v), v.size * 4, jvm.direct(m), m.size * 4, jvm.direct(b), b.size)
        ubo = np.frombuffer(cam.ubo_bytes(), dtype=np.uint8).copy()
        for (x, y), w in want.items():
            out = np.full(40, 0xEE, np.uint8)                  # a larger buffer: only 32 bytes are written
            jvm.call("pick", ctx, jvm.direct(ubo), W, H, x, y, jvm.direct(out))
            assert out[:32].tobytes() == w.tobytes(), (x, y)
            assert (out[32:] == 0xEE).all()
        centre = np.frombuffer(want[(80, 45)].tobytes(), HIT_DTYPE)[0]
        assert rtamd.instance_of(cfg.scene, built, int(centre["tri"])).display_name == "Cube"
        with pytest.raises(JavaException, match="rt_pick: pixel"):
            jvm.call("pick", ctx, jvm.direct(ubo), W, H, W, 0, jvm.direct(np.zeros(32, np.uint8)))
    finally:
        jvm.call("destroy", ctx)
