"""Argument edges of the render entry points: what each refuses, and what it
accepts as "nothing to trace".

Every render launch is described once and enqueued through one function
(RenderLaunch / enqueue_render in rt_runtime.hip), and the entry points share
their checks where the text agrees.  The edges below differ from one entry
point to the next on purpose (an empty tile is refused, an empty rectangle is
not; a band rank without a band is fine, a band offset equal to the stride is
not), and the shared path must keep them apart:

* a refusal returns its code, and rt_last_error() starts with the name of the
  entry point that was called;
* a valid call with nothing to trace returns RT_OK, zeroes a pre-filled
  rt_stats and writes no byte of the outputs;
* the whole frame through rt_render_tile_device and through
  rt_render_batch_rect_device with one frame is the same launch: identical
  bytes and counters;
* rt_render_temporal leaves option new_sample as it found it, on a traced call
  and on a refused one.

One context, config 2's scene, a 40 x 24 frame at 2 bounces; most cases launch
no kernel.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import has_gpu

pytestmark = pytest.mark.gpu

W, H, B = 40, 24, 2
INVALID_ARG, NO_SCENE = -1, -5
RGBA_SENTINEL, RAD_SENTINEL = 7, -2.0
MAX_BATCH = 16


@pytest.fixture(scope="module")
def env():
    if not has_gpu():
        pytest.skip("no GPU")
    import rtamd
    from rtamd import _lib, configs
    r = rtamd.Renderer((0,))
    r.upload_scene(configs.get(2).build())
    cam = configs.Camera.default(W, H)
    cams = (_lib.CameraUBO * (MAX_BATCH + 1))(*([cam.ubo] * (MAX_BATCH + 1)))
    yield r, _lib.lib(), cam, cams
    r.close()


class _Out:
    """Device outputs of two frames, sentinel-filled, and a pre-filled rt_stats."""

    def __init__(self):
        import torch
        from rtamd import _lib
        self.rgba = torch.full((2 * H * W * 4,), RGBA_SENTINEL, dtype=torch.uint8, device="cuda:0")
        self.rad = torch.full((2 * H * W * 3,), RAD_SENTINEL, dtype=torch.float32, device="cuda:0")
        self.stats = _lib.Stats(11, 12, 13, 14, 15.0, 16)
        self.args = (self.rgba.data_ptr(), self.rad.data_ptr(), None, C.byref(self.stats))

    def untouched(self):
        import torch
        torch.cuda.synchronize()
        return bool((self.rgba == RGBA_SENTINEL).all()) and bool((self.rad == RAD_SENTINEL).all())


def _i32(*v):
    return (C.c_int32 * max(1, len(v)))(*v)


def _refused(L, rc, name, code=INVALID_ARG):
    assert rc == code, (name, rc, L.rt_last_error())
    msg = L.rt_last_error().decode()
    assert msg.startswith(name + ":"), (name, msg)


def _nothing(rc, out, name):
    assert rc == 0, (name, rc)
    assert out.stats.as_dict() == dict(segments=0, node_visits=0, tri_tests=0, mat_reads=0, ms=0.0, pixels=0), name
    assert out.untouched(), name


def _calls(L, ctx, cam, cams, out, n_frames=1):
    """Every device entry point on valid arguments (n_frames for the batch calls), by name."""
    lo, hi = _i32(*([0] * 17)), _i32(*([1] * 17))
    lists = _i32(*([0] * 17))
    return {
        "rt_render_tile_device": lambda: L.rt_render_tile_device(ctx, cam, W, H, B, 0, 0, W, H, *out.args),
        "rt_render_bands_device": lambda: L.rt_render_bands_device(ctx, cam, W, H, B, 8, 3, 0, *out.args),
        "rt_render_batch_device": lambda: L.rt_render_batch_device(ctx, cams, n_frames, W, H, B, 8, _i32(0), 1,
                                                                   *out.args),
        "rt_render_batch_rect_device": lambda: L.rt_render_batch_rect_device(ctx, cams, n_frames, W, H, B, 0, 0, W, 8,
                                                                             *out.args),
        "rt_render_batch_runs_device": lambda: L.rt_render_batch_runs_device(ctx, cams, n_frames, W, H, B, 8, lo, hi,
                                                                             *out.args),
        "rt_render_batch_lists_device": lambda: L.rt_render_batch_lists_device(ctx, cams, n_frames, W, H, B, 8, lists,
                                                                               1, *out.args),
    }


BATCH = ("rt_render_batch_device", "rt_render_batch_rect_device", "rt_render_batch_runs_device",
         "rt_render_batch_lists_device")


@pytest.mark.parametrize("tw,th", [(0, 8), (8, 0)])
def test_tile_refuses_an_empty_tile(env, tw, th):
    r, L, cam, _ = env
    out = _Out()
    _refused(L, L.rt_render_tile_device(r._ctx, cam.ubo, W, H, B, 4, 4, tw, th, *out.args), "rt_render_tile_device")
    assert out.untouched()


@pytest.mark.parametrize("tw,th", [(0, 8), (8, 0)])
def test_rect_takes_an_empty_rectangle(env, tw, th):
    r, L, _, cams = env
    out = _Out()
    _nothing(L.rt_render_batch_rect_device(r._ctx, cams, 2, W, H, B, 4, 4, tw, th, *out.args), out, "rect")


def test_rect_refuses_a_column_past_the_frame(env):
    r, L, _, cams = env
    out = _Out()
    _refused(L, L.rt_render_batch_rect_device(r._ctx, cams, 1, W, H, B, 1, 0, W, H, *out.args),
             "rt_render_batch_rect_device")
    assert out.untouched()


def test_bands_offset_and_rank_without_a_band(env):
    r, L, cam, _ = env
    out = _Out()
    _refused(L, L.rt_render_bands_device(r._ctx, cam.ubo, W, H, B, 8, 2, 2, *out.args), "rt_render_bands_device")
    assert out.untouched()
    # 24 rows in bands of 8 are bands 0..2: rank 4 of 5 has none
    _nothing(L.rt_render_bands_device(r._ctx, cam.ubo, W, H, B, 8, 5, 4, *out.args), out, "bands")


def test_batch_band_lists(env):
    r, L, _, cams = env
    out = _Out()
    _nothing(L.rt_render_batch_device(r._ctx, cams, 2, W, H, B, 8, _i32(0), 0, *out.args), out, "batch, empty list")
    out = _Out()
    _refused(L, L.rt_render_batch_device(r._ctx, cams, 2, W, H, B, 8, _i32(1, 1), 2, *out.args),
             "rt_render_batch_device")
    assert out.untouched()


def test_runs(env):
    r, L, _, cams = env
    out = _Out()
    _nothing(L.rt_render_batch_runs_device(r._ctx, cams, 2, W, H, B, 8, _i32(1, 2), _i32(1, 2), *out.args), out, "runs")
    out = _Out()
    _refused(L, L.rt_render_batch_runs_device(r._ctx, cams, 2, W, H, B, 7, _i32(0, 0), _i32(1, 1), *out.args),
             "rt_render_batch_runs_device")
    assert out.untouched()


def test_lists_refuse_a_value_after_the_padding(env):
    r, L, _, cams = env
    out = _Out()
    _refused(L, L.rt_render_batch_lists_device(r._ctx, cams, 2, W, H, B, 8, _i32(0, -1, 2, 0, 1, -1), 3, *out.args),
             "rt_render_batch_lists_device")
    assert out.untouched()


@pytest.mark.parametrize("n_frames", [0, MAX_BATCH + 1])
@pytest.mark.parametrize("name", BATCH)
def test_batch_frame_count(env, name, n_frames):
    r, L, _, cams = env
    out = _Out()
    _refused(L, _calls(L, r._ctx, cams, cams, out, n_frames)[name](), name)
    assert out.untouched()


def test_no_scene():
    """A fresh context refuses every entry point with NO_SCENE, which comes before the n_frames check."""
    if not has_gpu():
        pytest.skip("no GPU")
    import rtamd
    from rtamd import _lib, configs
    L = _lib.lib()
    cam = configs.Camera.default(W, H)
    cams = (_lib.CameraUBO * (MAX_BATCH + 1))(*([cam.ubo] * (MAX_BATCH + 1)))
    with rtamd.Renderer((0,)) as r:
        for n_frames in (1, 0):
            out = _Out()
            for name, call in _calls(L, r._ctx, cam.ubo, cams, out, n_frames).items():
                _refused(L, call(), name, NO_SCENE)
            assert out.untouched()
        host = np.full((H, W, 4), RGBA_SENTINEL, np.uint8)
        _refused(L, L.rt_render(r._ctx, cam.ubo, W, H, B, host.ctypes.data, None, None), "rt_render", NO_SCENE)
        assert (host == RGBA_SENTINEL).all()


def test_tile_and_one_frame_rectangle_are_the_same_launch(env):
    import torch
    r, L, cam, cams = env
    res = []
    for name in ("rt_render_tile_device", "rt_render_batch_rect_device"):
        out = _Out()
        if name == "rt_render_tile_device":
            rc = L.rt_render_tile_device(r._ctx, cam.ubo, W, H, B, 0, 0, W, H, *out.args)
        else:
            rc = L.rt_render_batch_rect_device(r._ctx, cams, 1, W, H, B, 0, 0, W, H, *out.args)
        assert rc == 0, (name, L.rt_last_error())
        torch.cuda.synchronize()
        rgba, rad = out.rgba.cpu().numpy(), out.rad.cpu().numpy().view(np.uint32)
        n = H * W
        # one frame written in full (alpha 255, radiance never negative), the second frame's room untouched
        assert (rgba[:4 * n].reshape(-1, 4)[:, 3] == 255).all() and (rgba[4 * n:] == RGBA_SENTINEL).all(), name
        assert (out.rad[:3 * n] >= 0).all() and (out.rad[3 * n:] == RAD_SENTINEL).all(), name
        st = out.stats.as_dict()
        assert st["pixels"] == n and st["segments"] >= n, (name, st)
        res.append((rgba, rad, {k: st[k] for k in ("segments", "node_visits", "tri_tests", "mat_reads", "pixels")}))
    assert np.array_equal(res[0][0], res[1][0]), "RGBA8 differs"
    assert np.array_equal(res[0][1], res[1][1]), "radiance differs"
    assert res[0][2] == res[1][2]


@pytest.mark.parametrize("value", [0, 1])
def test_render_temporal_leaves_new_sample_alone(env, value):
    r, L, cam, _ = env
    r.set_option("new_sample", value)
    try:
        rgba = np.empty((H, W, 4), np.uint8)
        # without RT_TEMPORAL_FIXED_SEED: the launch takes a new sample whatever the option says
        rc = L.rt_render_temporal(r._ctx, cam.ubo, W, H, B, None, None, 0, rgba.ctypes.data, None, None)
        assert rc == 0, L.rt_last_error()
        assert r.get_option("new_sample") == value
        _refused(L, L.rt_render_temporal(r._ctx, cam.ubo, W, H, B, None, None, 0x80, rgba.ctypes.data, None, None),
                 "rt_render_temporal")
        assert r.get_option("new_sample") == value
    finally:
        r.set_option("new_sample", 0)
