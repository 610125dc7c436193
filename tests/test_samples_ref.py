"""The samples calls without a GPU: rt_samples_workspace_bytes, the bindings,
and tests/samples_ref.py's reference against the plain oracle frame."""
import numpy as np

import samples_ref as S


def test_workspace_bytes():
    from rtamd import Renderer
    ws = Renderer.samples_workspace_bytes
    assert ws(64, 48, 1) == 64 * 48 * 12
    assert ws(37, 23, 5) == 5 * 37 * 23 * 12
    assert ws(1, 1, 16) == 16 * 12
    assert ws(1920, 1080, 16) == 16 * 1920 * 1080 * 12
    assert ws(65536, 32768, 16) == 16 * (1 << 31) * 12           # the largest frame: past 2^32 bytes
    for w, h, f in ((0, 48, 1), (64, 0, 1), (-1, 48, 1), (64, 48, 0), (64, 48, 17), (64, 48, -3),
                    (65536, 32769, 1)):
        assert ws(w, h, f) == 0, (w, h, f)


def test_symbols_are_bound():
    from rtamd import Renderer, _lib
    L = _lib.lib()
    for name in ("rt_samples_workspace_bytes", "rt_render_samples_device", "rt_render_samples"):
        assert name in _lib.EXPORTED
        assert getattr(L, name).argtypes is not None
    assert len(L.rt_render_samples_device.argtypes) == 13 and len(L.rt_render_samples.argtypes) == 9
    for name in ("samples_workspace_bytes", "render_samples_device", "render_samples"):
        assert callable(getattr(Renderer, name))
    assert "csrc/rt_samples.hip" in _lib.BUILD_SOURCES


def test_one_sample_is_the_plain_frame():
    """The reference at n = 1: frame_count 0 is the reference's seed and the
    mean of one sample is the sample, so the sum is the frame's linear colour
    and radiance and RGBA8 are the plain oracle frame's bit for bit."""
    from oracle import oracle_lib
    from rtamd import configs
    w, h, b = 37, 23, 4
    built = S.config2_built()
    cam = configs.Camera.default(w, h)
    ref = S.config2_reference(w, h, b, 1)
    rgba, rad, cnt = oracle_lib.render(built.model_vertex_data, built.model_material_data, built.flat_bvh_data,
                                       cam.ubo_bytes(), w, h, b)
    assert np.array_equal(ref["rgba"], rgba)
    assert np.array_equal(ref["radiance"].view(np.uint32), rad.view(np.uint32))
    assert {k: ref["counts"][k] for k in S.COUNTERS} == {k: cnt[k] for k in S.COUNTERS}
    assert np.array_equal(np.sqrt(ref["sum"]).view(np.uint32), rad.view(np.uint32))


def test_reference_prefixes_and_order():
    """A prefix of the reference is the reference of fewer samples, and the
    sum after k samples is the sum after k - 1 plus one rounded add."""
    w, h, b = 37, 23, 4
    full = S.config2_reference(w, h, b, 5, prefixes=(2,))
    two = S.config2_reference(w, h, b, 2)
    for k in ("sum", "radiance", "rgba"):
        assert np.array_equal(full["at"][2][k], two[k])
    assert full["at"][2]["counts"] == two["counts"]
    assert (full["sum"] != two["sum"]).any()
    nf = np.float32(5.0)
    assert np.array_equal(np.sqrt(full["sum"] / nf).view(np.uint32), full["radiance"].view(np.uint32))
