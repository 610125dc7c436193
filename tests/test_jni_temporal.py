"""HipNative.renderTemporal (jni/HipNative.c) through the mock JNIEnv of
tests/test_jni_shim.py: the buffer checks and a null context throw
RuntimeException; on a GPU the frames are Renderer.render_temporal's."""
import ctypes as C

import numpy as np
import pytest

from conftest import has_gpu
from test_jni_shim import PREFIX, JavaException, Jvm


def _jvm():
    jvm = Jvm()
    f = getattr(jvm.L, PREFIX + "renderTemporal")
    f.restype = None
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float,
                  C.c_float, C.c_int32, C.c_int32, C.c_void_p]
    jvm.fn["renderTemporal"] = f
    return jvm


DEFAULTS = (32, 0.005, 0.9)       # rt_temporal_default_params


def test_render_temporal_checks_buffers_and_context():
    jvm = _jvm()
    w, h = 8, 4
    ubo = np.zeros(80, np.uint8)
    out = np.zeros(w * h * 4, np.uint8)
    # a short frame, a short UBO, heap buffers, null buffers, a frame size below 1: no rt_render_temporal call
    for u, o, ww, hh in [(jvm.direct(ubo), jvm.direct(out[:-1]), w, h), (jvm.direct(ubo[:79]), jvm.direct(out), w, h),
                         (jvm.direct(ubo), jvm.L.mock_heap_buffer(), w, h),
                         (jvm.L.mock_heap_buffer(), jvm.direct(out), w, h),
                         (None, jvm.direct(out), w, h), (jvm.direct(ubo), None, w, h),
                         (jvm.direct(ubo), jvm.direct(out), 0, h), (jvm.direct(ubo), jvm.direct(out), w, -1)]:
        with pytest.raises(JavaException, match="renderTemporal: need direct buffers") as ei:
            jvm.call("renderTemporal", 1, u, ww, hh, 4, *DEFAULTS, 0, 0, o)
        assert ei.value.cls == "java/lang/RuntimeException"
    assert not out.any()
    # a null context: rt_render_temporal's status becomes the exception
    with pytest.raises(JavaException, match="rtamd error -1: rt_render_temporal: null context or camera"):
        jvm.call("renderTemporal", 0, jvm.direct(ubo), w, h, 4, *DEFAULTS, 0, 0, jvm.direct(out))
    assert jvm.L.mock_outstanding() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("accel", [0, 8])
def test_render_temporal_through_the_shim(accel):
    if not has_gpu():
        pytest.skip("no GPU")
    import rtamd
    from rtamd import configs
    from test_gpu_temporal import camera
    jvm = _jvm()
    built = configs.config2().build()
    W, H, B = 160, 90, 4
    cams = []
    for k in range(3):
        cam = camera(W, H, orbit=1.0 * k)
        cam.ubo.frame_count = k
        cams.append(cam)
    other = (2, 0.02, 0.5)
    with rtamd.Renderer((0,)) as r:
        r.set_option("accel", accel)
        r.upload_scene(built)
        want = [r.render_temporal(c, W, H, B, reset=(k == 0))[0] for k, c in enumerate(cams)]
        want2 = [r.render_temporal(c, W, H, B, rtamd.TemporalParams(*other), rtamd.DenoiseParams(iterations=2),
                                   reset=(k == 0))[0] for k, c in enumerate(cams)]
        fixed = r.render_temporal(cams[2], W, H, B, fixed_seed=True, reset=True)[0]
        raw = r.render(cams[2], W, H, B)[0]
    assert (want[2] != raw).any() and (want2[2] != want[2]).any() and np.array_equal(fixed, raw)
    ctx = jvm.call("create", jvm.ints([0]))
    assert ctx != 0
    try:
        v = np.ascontiguousarray(built.model_vertex_data, dtype=np.float32)
        m = np.ascontiguousarray(built.model_material_data, dtype=np.float32)
        b = np.ascontiguousarray(built.flat_bvh_data, dtype=np.uint8)
        jvm.call("setOption", ctx, jvm.string("accel"), accel)
        jvm.call("uploadScene", ctx, jvm.direct(v), v.size * 4, jvm.direct(m), m.size * 4, jvm.direct(b), b.size)
        out = np.full(W * H * 4 + 16, 0xEE, np.uint8)            # a larger buffer: only the frame is written
        for k, c in enumerate(cams):
            ubo = np.frombuffer(c.ubo_bytes(), dtype=np.uint8).copy()
            jvm.call("renderTemporal", ctx, jvm.direct(ubo), W, H, B, *DEFAULTS, 0, 1 if k == 0 else 0, jvm.direct(out))
            assert np.array_equal(out[:W * H * 4].reshape(H, W, 4), want[k]), k
            assert (out[W * H * 4:] == 0xEE).all()
        for k, c in enumerate(cams):
            ubo = np.frombuffer(c.ubo_bytes(), dtype=np.uint8).copy()
            jvm.call("renderTemporal", ctx, jvm.direct(ubo), W, H, B, *other, 2, 1 if k == 0 else 0, jvm.direct(out))
            assert np.array_equal(out[:W * H * 4].reshape(H, W, 4), want2[k]), k
        jvm.call("renderTemporal", ctx, jvm.direct(ubo), W, H, B, *DEFAULTS, 0, 3, jvm.direct(out))   # reset | fixed seed
        assert np.array_equal(out[:W * H * 4].reshape(H, W, 4), fixed)
        with pytest.raises(JavaException, match="rt_render_temporal: max_history"):
            jvm.call("renderTemporal", ctx, jvm.direct(ubo), W, H, B, 0, 0.005, 0.9, 0, 0, jvm.direct(out))
        with pytest.raises(JavaException, match="rt_render_temporal: iterations"):
            jvm.call("renderTemporal", ctx, jvm.direct(ubo), W, H, B, *DEFAULTS, 9, 0, jvm.direct(out))
    finally:
        jvm.call("destroy", ctx)
