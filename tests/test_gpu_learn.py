"""The heavy-first learning on the GPU (csrc/rt_learn.hip; rt_runtime.hip
learn_order for the host path): every word of the tile order, the lane masks,
the heavy-pixel list and its count equals tests/learn_ref.py.

* Synthetic records through rt_learn_device (the inputs of
  tests/test_learn_ref.py cases(), whose properties are asserted there on the
  CPU): ties, both cost kinds, skipped records, every order_split, caps below /
  at / above the candidate count, no candidate and every pixel one, all-zero
  costs, costs past 2^32 and a wrapped duration, bars at which a pre-multiplied
  scale rounds to the other side of an integer, and the XCD grouping with
  partial last cycles of bands and tile counts it does not apply to.  Guard
  bytes around every buffer; inputs unchanged.
* Live learning launches of config 2 read back through rt_learn_copy: the
  result equals the model evaluated on the launch's own records and the
  parameters the runtime reports, on the device and the host path, and every
  frame stays the oracle's.
"""
import ctypes as C

import numpy as np
import pytest

import learn_ref as L
from conftest import has_gpu
from test_gpu_denoise import Guarded
from test_learn_ref import CASES, synth, want

pytestmark = pytest.mark.gpu

W, H, B = 128, 72, 4            # config 2: 144 wave tiles, a multiple of 8
UNTOUCHED = 0xEEEEEEEE          # Guarded's fill, as a 32-bit word


@pytest.fixture(scope="module")
def r():
    if not has_gpu():
        pytest.skip("no GPU")
    import rtamd
    rr = rtamd.Renderer((0,))
    yield rr
    rr.close()


def run_synth(r, case):
    """rt_learn_device on a case's arrays through guarded device buffers:
    (order, mask, hpix buffer, count)."""
    import torch
    n, kw = case["n"], case["kw"]
    cap = min(kw["cap"], 64 * n)
    rec, lane = np.ascontiguousarray(case["records"]), np.ascontiguousarray(case["lane"])
    d_rec, d_lane = Guarded(rec.nbytes, rec), Guarded(lane.nbytes, lane)
    d_order, d_mask, d_hpix, d_count = Guarded(4 * n), Guarded(8 * n), Guarded(4 * max(cap, 1)), Guarded(4)
    r.learn_device(d_rec.ptr, d_lane.ptr, n, d_order.ptr, d_mask.ptr, d_hpix.ptr, d_count.ptr,
                   torch.cuda.current_stream().cuda_stream, **kw)
    torch.cuda.synchronize()
    for b in (d_rec, d_lane, d_order, d_mask, d_hpix, d_count):
        assert b.guards_intact()
    assert d_rec.host(np.uint8, -1).tobytes() == rec.tobytes() and d_lane.host(np.uint8, -1).tobytes() == lane.tobytes()
    return (d_order.host(np.int32, -1), d_mask.host(np.uint64, -1), d_hpix.host(np.uint32, -1),
            int(d_count.host(np.int32, -1)[0]))


@pytest.mark.parametrize("name", sorted(CASES))
def test_synthetic_records_equal_the_model(r, name):
    case = synth(**CASES[name])
    order, mask, hpix, _ = want(case)
    g_order, g_mask, g_hpix, g_count = run_synth(r, case)
    assert g_count == len(hpix), (name, g_count, len(hpix), case["n_cand"], case["kw"])
    assert g_hpix[:g_count].tolist() == hpix, name
    assert (g_hpix[g_count:] == UNTOUCHED).all(), name                  # nothing past the count is written
    assert g_mask.tolist() == mask, name
    bad = np.flatnonzero(g_order != np.array(order, np.int32))
    assert bad.size == 0, (name, bad[:8].tolist(), g_order[bad[:8]].tolist(), [order[i] for i in bad[:8]])


def test_learn_device_argument_errors(r):
    from rtamd import RtError
    case = synth(8, 1)
    import torch
    d = torch.zeros(8 * 64 * 8, dtype=torch.uint8, device="cuda:0")
    p = d.data_ptr()
    for bad in (dict(n_tiles=0), dict(order_split=101), dict(learn_cost=2), dict(heavy_pixel_factor=0),
                dict(concurrent=0), dict(resident=0), dict(cap=-1), dict(rec_off=-1), dict(d_order=None)):
        kw = dict(case["kw"])
        args = dict(d_records=p, d_lanes=p, n_tiles=8, d_order=p, d_mask=p, d_hpix=p, d_count=p)
        for k, v in bad.items():
            (args if k in args else kw)[k] = v
        with pytest.raises(RtError, match="INVALID_ARG"):
            r.learn_device(**args, **kw)


# ---------------------------------------------------------------- live launches

@pytest.fixture(scope="module")
def scene():
    """Config 2, its camera at W x H and a second one, and the oracle's frames."""
    from oracle import oracle_lib
    from rtamd import configs
    built = configs.config2().build()

    def frame(cam, w=W, h=H):
        return oracle_lib.render(built.model_vertex_data, built.model_material_data, built.flat_bvh_data,
                                 cam.ubo_bytes(), w, h, B, radiance=False)[0]
    cam_a = configs.Camera.default(W, H)
    cam_b = configs.Camera((3.0, 2.5, 6.0), (0.0, 0.5, 0.0), (0.0, 1.0, 0.0), 40.0, W / H)
    cam_c = configs.Camera.default(104, H)
    return dict(built=built, cam_a=cam_a, ref_a=frame(cam_a), cam_b=cam_b, ref_b=frame(cam_b), cam_c=cam_c,
                ref_c=frame(cam_c, 104, H))


def options(r, **kw):
    base = dict(accel=0, learn_cost=0, learn_device=1, order_split=0, heavy_pixel_factor=50, heavy_cap=75,
                xcd_order=0, concurrent_launches=1)
    for k, v in {**base, **kw}.items():
        r.set_option(k, v)


def model_of(got):
    """The model on a readback's own records and reported parameters."""
    assert got["records_resident"] == 1 and got["records"] is not None
    kw = {k: got[k] for k in ("learn_cost", "order_split", "heavy_pixel_factor", "concurrent", "resident", "cap",
                              "xcd", "tiles_x", "tiles_y", "frames")}
    return L.learn(got["records"].tolist(), got["lanes"].tolist(), rec_off=0, **kw)     # records start at tile 0


def assert_equals_model(got, tag):
    order, mask, hpix, _ = model_of(got)
    n = got["n_tiles"]
    assert n == got["tiles_x"] * got["tiles_y"] * got["frames"], tag
    assert got["xcd_applied"] == int(bool(got["on_device"]) and L.xcd_applies(n, got["xcd"], got["tiles_x"],
                                                                             got["tiles_y"], got["frames"])), tag
    assert got["n_hpix"] == len(hpix), (tag, got["n_hpix"], len(hpix), got["cap"])
    assert got["hpix"].tolist() == hpix, tag
    assert got["mask"].tolist() == mask, tag
    assert got["order"].tolist() == order, tag
    return order, mask, hpix


def candidates(got):
    steps, _ = L.tile_costs(got["records"].tolist(), 0, got["learn_cost"])
    bar = L.heavy_bar(sum(steps), got["heavy_pixel_factor"], got["concurrent"], got["resident"])
    return int((got["lanes"].astype(np.float64) > bar).sum())


LIVE = [  # accel, learn_cost, learn_device, order_split, limit, xcd_order
    (0, 0, 1, 0, "bar", 0), (0, 0, 0, 0, "bar", 0), (0, 1, 1, 20, "cap", 1), (0, 1, 0, 20, "cap", 2),
    (0, 0, 1, 20, "cap", 2), (0, 0, 0, 20, "cap", 0), (0, 1, 1, 0, "bar", 2), (8, 1, 1, 0, "bar", 2),
    (8, 0, 1, 20, "cap", 1),
]


@pytest.mark.parametrize("accel,learn_cost,learn_device,order_split,limit,xcd", LIVE)
def test_live_learning_equals_the_model(r, scene, accel, learn_cost, learn_device, order_split, limit, xcd):
    """The learning launch of a whole frame, then the launch that runs in its
    order.  limit "bar": the bar decides the heavy pixels (fewer than the cap);
    "cap": a low bar and a cap of 1% of the resident waves, which cuts the list.
    Config 2 at this size has a few dozen pixels past 100 x the bulk estimate
    and every pixel past 1% of it."""
    tag = (accel, learn_cost, learn_device, order_split, limit, xcd)
    options(r, accel=accel, learn_cost=learn_cost, learn_device=learn_device, order_split=order_split, xcd_order=xcd,
            heavy_pixel_factor=10000 if limit == "bar" else 1, heavy_cap=75 if limit == "bar" else 1)
    r.upload_scene(scene["built"])                       # a new scene generation: nothing learned yet
    assert np.array_equal(r.render(scene["cam_a"], W, H, B)[0], scene["ref_a"]), tag      # the learning launch
    got = r.learn_copy()
    assert (got["on_device"], got["learn_cost"], got["order_split"], got["rec_off"], got["frames"]) == \
        (learn_device, learn_cost, order_split, 0, 1), tag
    assert got["n_tiles"] == 144 and got["xcd"] == (xcd if learn_device else 0), tag
    assert got["xcd_applied"] == int(learn_device == 1 and xcd > 0), tag    # a whole frame of 144 tiles is grouped
    assert got["cap"] == max(1, got["resident"] * (75 if limit == "bar" else 1) // 100), tag
    order, mask, hpix = assert_equals_model(got, tag)
    n_cand = candidates(got)
    print(f"live {tag}: {n_cand} candidates, cap {got['cap']}, {len(hpix)} heavy pixels, host heavy tiles {got['heavy']}")
    if limit == "bar":
        assert 0 < n_cand == len(hpix) < got["cap"], tag
    else:
        assert len(hpix) == got["cap"] < n_cand, tag
    assert np.array_equal(r.render(scene["cam_a"], W, H, B)[0], scene["ref_a"]), tag      # in the learned order
    # heavy pixels are split out of the reference-tree walk only (plan_order: splittable)
    assert r.get_option("heavy_pixels_used") == (len(hpix) if accel == 0 else 0), tag
    again = r.learn_copy()
    assert again["order"].tolist() == order and again["hpix"].tolist() == hpix, tag       # a use does not relearn


def test_device_and_host_paths_learn_the_same(r, scene):
    """learn_cost 0 (a deterministic cost) on a fresh scene generation: the
    same order, masks and heavy list, with and without order_split."""
    for split, factor, cap in ((0, 10000, 75), (20, 1, 1), (100, 30, 75)):
        got = {}
        for dev in (1, 0):
            options(r, learn_device=dev, order_split=split, heavy_pixel_factor=factor, heavy_cap=cap)
            r.upload_scene(scene["built"])
            assert np.array_equal(r.render(scene["cam_a"], W, H, B)[0], scene["ref_a"])
            got[dev] = r.learn_copy()
            assert got[dev]["on_device"] == dev
        assert np.array_equal(got[1]["records"][:, 4:6], got[0]["records"][:, 4:6])       # the same launch twice
        assert np.array_equal(got[1]["lanes"], got[0]["lanes"])
        for k in ("order", "mask", "hpix"):
            assert np.array_equal(got[1][k], got[0][k]), (split, k)
        assert got[1]["n_hpix"] == got[0]["n_hpix"] > 0


def test_second_learning_in_a_reused_order(r, scene):
    """A camera that moves reuses the order; its first repeat learns in that
    order, the heavy pixels' one-pixel waves recording ahead of the tiles
    (rec_off = their count)."""
    options(r, learn_cost=0, heavy_pixel_factor=1, heavy_cap=1, xcd_order=1)
    r.upload_scene(scene["built"])
    for _ in range(2):
        assert np.array_equal(r.render(scene["cam_a"], W, H, B)[0], scene["ref_a"])
    first = r.learn_copy()
    assert first["rec_off"] == 0 and first["n_hpix"] > 0
    assert np.array_equal(r.render(scene["cam_b"], W, H, B)[0], scene["ref_b"])          # moved: reuses, no learning
    assert r.get_option("heavy_pixels_used") == first["n_hpix"]
    assert r.learn_copy()["order"].tolist() == first["order"].tolist()
    assert np.array_equal(r.render(scene["cam_b"], W, H, B)[0], scene["ref_b"])          # stopped: learns in that order
    second = r.learn_copy()
    assert second["rec_off"] == first["n_hpix"] and second["on_device"] == 1 and second["xcd_applied"] == 1
    order, mask, hpix = assert_equals_model(second, "second")
    # a pixel traced by a one-pixel wave carries the mark, and stays heavy
    marked = np.flatnonzero(second["lanes"] == 0x3FFFFFFF)
    assert sorted(marked.tolist()) == sorted(first["hpix"].tolist()) and set(marked.tolist()) <= set(hpix)
    assert np.array_equal(r.render(scene["cam_b"], W, H, B)[0], scene["ref_b"])
    assert r.get_option("heavy_pixels_used") == len(hpix)


def _tile_shape(r):
    wt = r.get_option("wave_tile_used")
    return 8 << wt, 8 >> wt


def test_batch_band_and_ragged_launches_state_their_grouping(r, scene):
    """What xcd_order gets on the other launch shapes: a batch of 4 whole
    frames (576 tiles: grouped over the same rows of all frames), a band launch
    (grouped over its own packed rows) and a 104-pixel-wide frame (117 tiles, no multiple
    of 8: the plain order, reported as not applied)."""
    import torch
    from rtamd import lib
    from rtamd._lib import CameraUBO, check
    options(r, learn_cost=0, xcd_order=2, heavy_pixel_factor=1, heavy_cap=1)
    r.upload_scene(scene["built"])
    tw, th = _tile_shape(r)
    s = torch.cuda.current_stream().cuda_stream
    ubos = (CameraUBO * 4)(*[scene["cam_a"].ubo] * 4)
    d = torch.zeros((4 * H, W, 4), dtype=torch.uint8, device="cuda:0")
    for launch in range(2):
        check(lib().rt_render_batch_device(r._ctx, ubos, 4, W, H, B, 0, None, 0, d.data_ptr(), None, s, None))
        torch.cuda.synchronize()
        assert np.array_equal(d.cpu().numpy().reshape(4, H, W, 4), np.stack([scene["ref_a"]] * 4)), launch
        if launch == 0:
            got = r.learn_copy()
            assert (got["n_tiles"], got["frames"], got["tiles_x"] * tw, got["tiles_y"] * th) == (576, 4, W, H)
            assert got["xcd_applied"] == 1 and got["on_device"] == 1
            assert_equals_model(got, "batch")
    # bands 1, 4 and 7 of 8 rows: 24 packed rows
    rows = np.concatenate([np.arange(8 * b, 8 * b + 8) for b in (1, 4, 7)])
    d = torch.zeros((24, W, 4), dtype=torch.uint8, device="cuda:0")
    for launch in range(2):
        check(lib().rt_render_bands_device(r._ctx, C.byref(scene["cam_a"].ubo), W, H, B, 8, 3, 1, d.data_ptr(), None, s,
                                           None))
        torch.cuda.synchronize()
        assert np.array_equal(d.cpu().numpy(), scene["ref_a"][rows]), launch
        if launch == 0:
            got = r.learn_copy()
            assert (got["n_tiles"], got["frames"], got["tiles_x"] * tw, got["tiles_y"] * th) == (48, 1, W, 24)
            assert got["xcd_applied"] == 1                               # over the launch's own 24 rows
            assert_equals_model(got, "bands")
    for launch in range(2):
        assert np.array_equal(r.render(scene["cam_c"], 104, H, B)[0], scene["ref_c"]), launch
        if launch == 0:
            got = r.learn_copy()
            assert got["n_tiles"] == -(-104 // tw) * (H // th) and got["n_tiles"] % 8 != 0     # 117 tiles of 8 x 8
            assert got["xcd"] == 2 and got["xcd_applied"] == 0
            order = assert_equals_model(got, "ragged")[0]
            _, cost = L.tile_costs(got["records"].tolist(), 0, 0)
            assert order == L.cost_order(cost, 0)


def test_learn_copy_errors(r):
    import rtamd
    from rtamd import RtError
    with rtamd.Renderer((0,)) as fresh:
        with pytest.raises(RtError, match="INVALID_ARG.*no order"):
            fresh.learn_copy()
