"""HipNative.renderDenoised (jni/HipNative.c) through the mock JNIEnv of
tests/test_jni_shim.py: the buffer checks and a null context throw
RuntimeException; on a GPU the frame is Renderer.render_denoised's."""
import ctypes as C

import numpy as np
import pytest

from conftest import has_gpu
from test_jni_shim import PREFIX, JavaException, Jvm


def _jvm():
    jvm = Jvm()
    f = getattr(jvm.L, PREFIX + "renderDenoised")
    f.restype = None
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                  C.c_float, C.c_float, C.c_void_p]
    jvm.fn["renderDenoised"] = f
    return jvm


DEFAULTS = (4, 7, 0.005, 0.5)


def test_render_denoised_checks_buffers_and_context():
    jvm = _jvm()
    w, h = 8, 4
    ubo = np.zeros(80, np.uint8)
    out = np.zeros(w * h * 4, np.uint8)
    # a short frame, a short UBO, heap buffers, null buffers, a frame size below 1: no rt_render_denoised call
    for u, o, ww, hh in [(jvm.direct(ubo), jvm.direct(out[:-1]), w, h), (jvm.direct(ubo[:79]), jvm.direct(out), w, h),
                         (jvm.direct(ubo), jvm.L.mock_heap_buffer(), w, h),
                         (jvm.L.mock_heap_buffer(), jvm.direct(out), w, h),
                         (None, jvm.direct(out), w, h), (jvm.direct(ubo), None, w, h),
                         (jvm.direct(ubo), jvm.direct(out), 0, h), (jvm.direct(ubo), jvm.direct(out), w, -1)]:
        with pytest.raises(JavaException, match="renderDenoised: need direct buffers") as ei:
            jvm.call("renderDenoised", 1, u, ww, hh, 4, *DEFAULTS, o)
        assert ei.value.cls == "java/lang/RuntimeException"
    assert not out.any()
    # a null context: rt_render_denoised's status becomes the exception
    with pytest.raises(JavaException, match="rtamd error -1: rt_render_denoised: null context or camera"):
        jvm.call("renderDenoised", 0, jvm.direct(ubo), w, h, 4, *DEFAULTS, jvm.direct(out))
    assert jvm.L.mock_outstanding() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("accel", [0, 8])
def test_render_denoised_through_the_shim(accel):
    if not has_gpu():
        pytest.skip("no GPU")
    import rtamd
    from rtamd import configs
    jvm = _jvm()
    cfg = configs.config2()
    built = cfg.build()
    W, H, B = 160, 90, 4
    cam = configs.Camera.default(W, H)
    other = (2, 3, 0.02, 1.0)
    with rtamd.Renderer((0,)) as r:
        r.set_option("accel", accel)
        r.upload_scene(built)
        want = r.render_denoised(cam, W, H, B)[0]
        want2 = r.render_denoised(cam, W, H, B, rtamd.DenoiseParams(*other))[0]
        raw = r.render(cam, W, H, B)[0]
    assert (want != raw).any() and (want2 != want).any()
    ctx = jvm.call("create", jvm.ints([0]))
    assert ctx != 0
    try:
        v = np.ascontiguousarray(built.model_vertex_data, dtype=np.float32)
        m = np.ascontiguousarray(built.model_material_data, dtype=np.float32)
        b = np.ascontiguousarray(built.flat_bvh_data, dtype=np.uint8)
        jvm.call("setOption", ctx, jvm.string("accel"), accel)
        jvm.call("uploadScene", ctx, jvm.direct(v), v.size * 4, jvm.direct(m), m.size * 4, jvm.direct(b), b.size)
        ubo = np.frombuffer(cam.ubo_bytes(), dtype=np.uint8).copy()
        out = np.full(W * H * 4 + 16, 0xEE, np.uint8)            # a larger buffer: only the frame is written
        jvm.call("renderDenoised", ctx, jvm.direct(ubo), W, H, B, *DEFAULTS, jvm.direct(out))
        assert np.array_equal(out[:W * H * 4].reshape(H, W, 4), want)
        assert (out[W * H * 4:] == 0xEE).all()
        jvm.call("renderDenoised", ctx, jvm.direct(ubo), W, H, B, *other, jvm.direct(out))
        assert np.array_equal(out[:W * H * 4].reshape(H, W, 4), want2)
        with pytest.raises(JavaException, match="rt_render_denoised: iterations"):
            jvm.call("renderDenoised", ctx, jvm.direct(ubo), W, H, B, 0, 7, 0.005, 0.5, jvm.direct(out))
    finally:
        jvm.call("destroy", ctx)
