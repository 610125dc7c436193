"""rt_render_samples_device / rt_render_samples on the GPU: the
sum, the radiance and the RGBA8 of a samples call equal tests/samples_ref.py
(the CPU oracle's ORC_EXT_ACCUMULATE called sample by sample) bit for bit, at
sizes on and off the 16-byte grid, for every chunking the option and the
workspace can produce, on the accel walk and on the reference's tree; they
equal extension bit 4's frames on the GPU; a sum continues across calls;
extensions 1, 2 and 8 apply; the learning launch and the learned order give
the same bits; argument errors; the host form; and the render state stays as
it was."""

import numpy as np
import pytest

import samples_ref as S
from conftest import has_gpu
from test_gpu_denoise import Guarded

pytestmark = pytest.mark.gpu

B = 4                                                   # bounces
SIZES = ((64, 48), (37, 23), (129, 65), (1, 1))         # 37x23: 2553 floats per frame, slices off the 16-byte grid
N_MAX = 17
DEFAULT_FRAMES = 16                                     # option sample_frames as rt_create leaves it
PREFIXES = (1, 2, 3, 4, 5, 12, 16)
# (n_samples, sample_frames): one launch, a short last chunk, whole chunks, more samples than a launch holds
CHUNKS = ((1, 4), (2, 1), (2, 3), (5, 1), (5, 3), (5, 4), (16, 4), (16, 16), (17, 3), (17, 4), (17, 16))


def _renderer(accel):
    if not has_gpu():
        pytest.skip("no GPU")
    import rtamd
    rr = rtamd.Renderer((0,))
    rr.set_option("accel", accel)
    rr.upload_scene(S.config2_built())
    return rr


@pytest.fixture(scope="module")
def r():
    rr = _renderer(8)
    yield rr
    rr.close()


@pytest.fixture(scope="module")
def r0():
    rr = _renderer(0)
    yield rr
    rr.close()


def _cam(w, h, first=0, sky=None):
    from rtamd import configs
    cam = configs.Camera.default(w, h)
    cam.ubo.frame_count = first
    if sky is not None:
        cam.ubo.sky_enabled = sky
    return cam


def _ref(w, h, n):
    return S.config2_reference(w, h, B, N_MAX, prefixes=PREFIXES)["at"][n]


def run(r, cam, w, h, n, sample_frames=4, ws_frames=16, rgba=True, radiance=True, stats=True, d_sum=None, form=0):
    """rt_render_samples_device through guarded device buffers: a dict of sum,
    rgba, radiance (None where not asked for) and stats; asserts that nothing
    outside the buffers was written."""
    import torch
    d_ws = Guarded(w * h * 12 * ws_frames)
    d_sum = d_sum if d_sum is not None else Guarded(w * h * 12)
    o_rgba = Guarded(w * h * 4) if rgba else None
    o_rad = Guarded(w * h * 12) if radiance else None
    r.set_option("sample_frames", sample_frames)
    r.set_option("samples_kernel", form)
    try:
        st = r.render_samples_device(cam, w, h, B, n, d_ws.ptr, d_ws.n, d_sum.ptr, o_rgba.ptr if rgba else None,
                                     o_rad.ptr if radiance else None, torch.cuda.current_stream().cuda_stream, stats)
        torch.cuda.synchronize()
    finally:
        r.set_option("sample_frames", DEFAULT_FRAMES)
        r.set_option("samples_kernel", 0)
    for b in (d_ws, d_sum, o_rgba, o_rad):
        assert b is None or b.guards_intact()
    return {"sum": d_sum.host(np.float32, (h, w, 3)), "rgba": o_rgba.host(np.uint8, (h, w, 4)) if rgba else None,
            "radiance": o_rad.host(np.float32, (h, w, 3)) if radiance else None, "stats": st, "d_sum": d_sum}


def same(got, want, what=("sum", "radiance", "rgba"), note=None):
    for k in what:
        g, t = got[k], want[k]
        if g.dtype == np.float32:
            g, t = g.view(np.uint32), t.view(np.uint32)
        diff = g != t
        assert not diff.any(), (note, k, int(diff.sum()), np.argwhere(diff)[:4].tolist())


@pytest.mark.parametrize("accel", [8, 0])
@pytest.mark.parametrize("size", SIZES)
def test_parity_with_the_reference(r, r0, size, accel):
    """Every chunking of N samples gives the oracle's sum, radiance and RGBA8;
    segments and material reads are the oracle's sums, and on the reference's
    tree node visits and triangle tests too."""
    rr = r if accel else r0
    w, h = size
    cam = _cam(w, h)
    for n, sf in CHUNKS:
        want = _ref(w, h, n)
        got = run(rr, cam, w, h, n, sample_frames=sf)
        same(got, want, note=(n, sf))
        st = got["stats"]
        assert st["pixels"] == w * h * n and st["ms"] > 0.0
        for k in ("segments", "mat_reads") if accel else S.COUNTERS:
            assert st[k] == want["counts"][k], (n, sf, k, st[k], want["counts"][k])
    # the scalar resolve on every size, and a plain (non-counting) call
    same(run(rr, cam, w, h, 5, sample_frames=3, form=1), _ref(w, h, 5), note="scalar")
    same(run(rr, cam, w, h, 5, sample_frames=3, stats=False), _ref(w, h, 5), note="plain")


@pytest.mark.parametrize("size", [(37, 23), (64, 48)])
def test_workspace_limits_the_chunk(r, size):
    """A workspace of exactly one frame and of exactly two frames: the launch
    takes what the workspace holds, not what the option says."""
    w, h = size
    for ws_frames, n in ((1, 1), (1, 5), (2, 5), (2, 2), (2, 16)):
        same(run(r, _cam(w, h), w, h, n, sample_frames=4, ws_frames=ws_frames), _ref(w, h, n), note=(ws_frames, n))


def test_parity_with_bit_4_on_the_gpu(r):
    """The outputs equal N rt_render calls with extensions 4, and on the accel
    walk node visits and triangle tests are the sums over N single-frame
    new_sample launches."""
    w, h, n = 129, 65, 5
    got = run(r, _cam(w, h), w, h, n)
    try:
        r.set_option("extensions", 4)
        for k in range(n):
            rgba, rad, _ = r.render(_cam(w, h, k), w, h, B, radiance=True)
        r.set_option("extensions", 0)
        same(got, {"rgba": rgba, "radiance": rad}, what=("radiance", "rgba"))
        r.set_option("new_sample", 1)
        tot = dict.fromkeys(S.COUNTERS, 0)
        for k in range(n):
            st = r.render(_cam(w, h, k), w, h, B, stats=True)[2]
            for c in S.COUNTERS:
                tot[c] += st[c]
    finally:
        r.set_option("extensions", 0)
        r.set_option("new_sample", 0)
    assert {c: got["stats"][c] for c in S.COUNTERS} == tot


@pytest.mark.parametrize("size", SIZES)
def test_one_sample_at_frame_count_0_is_rt_render(r, size):
    w, h = size
    rgba, rad, _ = r.render(_cam(w, h), w, h, B, radiance=True)
    same(run(r, _cam(w, h), w, h, 1), {"rgba": rgba, "radiance": rad}, what=("radiance", "rgba"))


@pytest.mark.parametrize("size", [(64, 48), (37, 23)])
def test_continuation(r, size):
    """Samples [0, 5) then [5, 12) on one d_sum = one call of 12; the sum is
    not read when frame_count is 0 (it starts as NaN)."""
    w, h = size
    nan = np.full((h, w, 3), np.nan, np.float32)
    first = run(r, _cam(w, h), w, h, 5, d_sum=Guarded(w * h * 12, nan))
    same(first, _ref(w, h, 5))
    second = run(r, _cam(w, h, 5), w, h, 7, sample_frames=3, d_sum=first["d_sum"])
    whole = run(r, _cam(w, h), w, h, 12, d_sum=Guarded(w * h * 12, nan))
    same(second, whole)
    same(second, _ref(w, h, 12))
    assert second["stats"]["pixels"] == w * h * 7


def test_extensions_apply(r):
    """Extensions 2, 1 with sky_enabled 0, and 8 with two spheres: each equals
    the oracle called with the same bits."""
    from test_oracle_kat import SPHERES, _ext_scene
    w, h, n = 37, 23, 3
    cases = ((2, None, None, S.config2_built()), (2, None, None, _ext_scene()), (1, 0, None, S.config2_built()),
             (8, None, SPHERES[:2], S.config2_built()))
    try:
        for ext, sky, spheres, built in cases:
            r.upload_scene(built)
            r.upload_spheres(spheres if spheres is not None else np.zeros((0, 8), np.float32))
            r.set_option("extensions", ext)
            cam = _cam(w, h, 0, sky)
            want = S.accumulate(built, cam, w, h, B, n, ext=ext, spheres=spheres, sky_enabled=sky)
            got = run(r, cam, w, h, n, sample_frames=2)
            same(got, want, note=(ext, sky))
            for k in ("segments", "mat_reads"):
                assert got["stats"][k] == want["counts"][k], (ext, k)
            assert r.get_option("extensions") == ext
    finally:
        r.set_option("extensions", 0)
        r.upload_spheres(np.zeros((0, 8), np.float32))
        r.upload_scene(S.config2_built())
    assert not np.array_equal(want["rgba"], _ref(w, h, n)["rgba"])      # the spheres are in the frame


def test_learning_launch_then_learned_order():
    """Two plain calls of one launch each with one camera under the default
    heavy_first: the first is a learning launch, the second runs in the order
    it learned; same bits."""
    rr = _renderer(8)
    try:
        assert rr.get_option("heavy_first") == 1
        w, h, n = 129, 65, 4
        with pytest.raises(Exception, match="INVALID_ARG"):
            rr.learn_copy(records=False)                                # nothing learned yet
        a = run(rr, _cam(w, h), w, h, n, stats=False)
        s = rr.get_option("wave_tile_used")
        tiles = -(-w // (8 << s)) * -(-h // (8 >> s)) * n               # the wave tiles of the launch's 4 frames
        assert rr.learn_copy(records=False)["n_tiles"] == tiles
        b = run(rr, _cam(w, h), w, h, n, stats=False)
        info = rr.learn_copy(records=False)
        assert info["n_tiles"] == tiles and sorted(info["order"].tolist()) == list(range(tiles))
        same(a, _ref(w, h, n), note="learning")
        same(b, _ref(w, h, n), note="learned")
        # a later sample of the same camera runs in that order too (the order's key leaves the sample index out)
        same(run(rr, _cam(w, h, 4), w, h, 1, stats=False, d_sum=b["d_sum"]), _ref(w, h, 5), note="continued")
    finally:
        rr.close()


def test_output_combinations(r):
    w, h, n = 37, 23, 5
    want = _ref(w, h, n)
    only_rgba = run(r, _cam(w, h), w, h, n, radiance=False)
    same(only_rgba, want, what=("sum", "rgba"))
    only_rad = run(r, _cam(w, h), w, h, n, rgba=False)
    same(only_rad, want, what=("sum", "radiance"))
    same(run(r, _cam(w, h), w, h, n), want)


def test_refusals(r):
    import torch
    from rtamd import RtError
    w, h = 64, 48
    fb = w * h * 12
    ws, sm, o4, o12 = Guarded(2 * fb), Guarded(fb), Guarded(w * h * 4), Guarded(fb)
    stream = torch.cuda.current_stream().cuda_stream

    def call(cam=None, n=2, d_ws=ws.ptr, ws_bytes=2 * fb, d_sum=sm.ptr, d_rgba=o4.ptr, d_rad=o12.ptr, ctx=r):
        return ctx.render_samples_device(cam or _cam(w, h), w, h, B, n, d_ws, ws_bytes, d_sum, d_rgba, d_rad, stream)

    def refused(match, **kw):
        with pytest.raises(RtError, match=match) as e:
            call(**kw)
        assert e.value.code == -1                                   # RT_ERR_INVALID_ARG

    try:
        r.set_option("extensions", 4)
        refused("extensions bit 4 is set")
    finally:
        r.set_option("extensions", 0)
    refused(r"n_samples must be in \[1, 65536\], got 0", n=0)
    refused(r"n_samples must be in \[1, 65536\], got 65537", n=65537)
    refused("frame_count .* must be >= 0, got -1", cam=_cam(w, h, -1))
    refused(r"reach past 2\^24", cam=_cam(w, h, (1 << 24) - 1), n=2)
    refused("both outputs are null", d_rgba=None, d_rad=None)
    refused("d_sum is null", d_sum=None)
    refused("16-byte aligned", d_sum=sm.ptr + 4)
    refused("16-byte aligned", d_ws=ws.ptr + 8)
    refused("4-byte", d_rad=o12.ptr + 2)
    refused("cannot hold one frame", ws_bytes=fb - 1)
    refused("d_sum overlaps d_workspace", d_sum=ws.ptr + 16)
    refused("d_out_radiance overlaps d_sum", d_rad=sm.ptr)
    refused("d_out_rgba overlaps d_workspace", d_rgba=ws.ptr + 2 * fb - 4)
    import rtamd
    two = rtamd.Renderer((0, 1) if torch.cuda.device_count() >= 2 else (0, 0))
    try:
        two.upload_scene(S.config2_built())
        refused("the context has 2 devices", ctx=two)
        with pytest.raises(RtError, match="the context has 2 devices"):
            two.render_samples(_cam(w, h), w, h, B, 2)
    finally:
        two.close()
    torch.cuda.synchronize()
    for b in (ws, sm, o4, o12):                                     # a refused call writes nothing
        assert b.guards_intact() and (b.host(np.uint8, -1) == 0xEE).all()
    # the last sample index that fits: 2^24 - 1 (the divisor 2^24 is an exact float); nothing is compared
    call(cam=_cam(w, h, (1 << 24) - 1), n=1)
    torch.cuda.synchronize()


def test_render_samples_host_form(r):
    from rtamd import RtError
    w, h = 37, 23
    rgba, rad, st = r.render_samples(_cam(w, h), w, h, B, 5, radiance=True, stats=True)
    same({"rgba": rgba, "radiance": rad}, _ref(w, h, 5), what=("radiance", "rgba"))
    dev = run(r, _cam(w, h), w, h, 5)
    same({"rgba": rgba, "radiance": rad}, dev, what=("radiance", "rgba"))
    assert {k: st[k] for k in S.COUNTERS} == {k: dev["stats"][k] for k in S.COUNTERS} and st["pixels"] == w * h * 5
    # it continues across calls (a device call in between has its own sum), with more samples than before
    rgba, rad, _ = r.render_samples(_cam(w, h, 5), w, h, B, 7, radiance=True)
    same({"rgba": rgba, "radiance": rad}, _ref(w, h, 12), what=("radiance", "rgba"))
    with pytest.raises(RtError, match="holds 12 samples"):
        r.render_samples(_cam(w, h, 3), w, h, B, 2)
    rgba, _, _ = r.render_samples(_cam(w, h, 12), w, h, B, 4)       # a refused call keeps the sum
    same({"rgba": rgba}, _ref(w, h, 16), what=("rgba",))
    # a new scene drops the sum
    r.upload_scene(S.config2_built())
    with pytest.raises(RtError, match="holds 0 samples"):
        r.render_samples(_cam(w, h, 16), w, h, B, 1)
    rgba, rad, _ = r.render_samples(_cam(w, h), w, h, B, 2, radiance=True)
    same({"rgba": rgba, "radiance": rad}, _ref(w, h, 2), what=("radiance", "rgba"))
    # so does another frame size
    with pytest.raises(RtError, match="holds 0 samples"):
        r.render_samples(_cam(64, 48, 2), 64, 48, B, 1)
    rgba, rad, _ = r.render_samples(_cam(64, 48), 64, 48, B, 5, radiance=True)
    same({"rgba": rgba, "radiance": rad}, _ref(64, 48, 5), what=("radiance", "rgba"))
    with pytest.raises(RtError, match="holds 0 samples"):
        r.render_samples(_cam(w, h, 2), w, h, B, 1)
    # and new spheres
    r.render_samples(_cam(w, h), w, h, B, 2)
    r.upload_spheres(np.zeros((0, 8), np.float32))
    with pytest.raises(RtError, match="holds 0 samples"):
        r.render_samples(_cam(w, h, 2), w, h, B, 1)


def test_render_state_is_untouched(r):
    """rt_render and rt_render_async draw the frames they drew before the
    samples calls; extensions and new_sample read back unchanged; the batch
    entry point still refuses new_sample with two frames."""
    import torch
    from rtamd import CameraUBO, RtError, lib
    from rtamd.engine import PinnedFrame
    from rtamd._lib import check
    w, h = 129, 65
    cam = _cam(w, h)
    before_rgba, before_rad, before_st = r.render(cam, w, h, B, radiance=True, stats=True)
    assert r.get_option("extensions") == 0 and r.get_option("new_sample") == 0
    run(r, _cam(w, h), w, h, 5, stats=False)
    run(r, _cam(w, h, 5), w, h, 2)
    r.render_samples(_cam(w, h), w, h, B, 3)
    assert r.get_option("extensions") == 0 and r.get_option("new_sample") == 0
    assert r.get_option("sample_frames") == DEFAULT_FRAMES and r.get_option("samples_stage") == -1
    rgba, rad, st = r.render(cam, w, h, B, radiance=True, stats=True)
    same({"rgba": rgba, "radiance": rad}, {"rgba": before_rgba, "radiance": before_rad}, what=("radiance", "rgba"))
    assert {k: st[k] for k in S.COUNTERS} == {k: before_st[k] for k in S.COUNTERS}
    frame = PinnedFrame(h, w)
    try:
        r.wait(r.render_async(cam, w, h, B, frame))
        assert np.array_equal(frame.array, before_rgba)
    finally:
        frame.close()
    d = torch.empty((2, h, w, 4), dtype=torch.uint8, device="cuda:0")
    ubos = (CameraUBO * 2)(cam.ubo, cam.ubo)
    try:
        r.set_option("new_sample", 1)
        with pytest.raises(RtError, match="one frame per launch"):
            check(lib().rt_render_batch_device(r._ctx, ubos, 2, w, h, B, 0, None, 0, d.data_ptr(), None,
                                               torch.cuda.current_stream().cuda_stream, None))
    finally:
        r.set_option("new_sample", 0)
    for bad in (0, 17):
        with pytest.raises(RtError, match="INVALID_ARG"):
            r.set_option("sample_frames", bad)
