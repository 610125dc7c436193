"""GPU parity of option rng_table (rt_trace.hip kFeatRng,
rt_rngtable.hip): below bounce K a path reads its scatter draw from a table
keyed by the frame size, built once per device by the first launch that needs
it.

Bar (no tolerance anywhere): the table's words equal a plain-Python
restatement of the chain (tests/rng_table_ref.py, pinned to the oracle's pcg);
RGBA8 and the radiance bits equal the CPU oracle's and the same launch with
the option at 0, whatever K, the split bounce, the launch path, the stream or
the table held before; rng_table_used says what the last launch read.
"""
import contextlib
import ctypes as C

import numpy as np
import pytest

from conftest import has_gpu
from test_gpu_accel import _check, _model, _oracle, _upload

pytestmark = pytest.mark.gpu

W, H = 203, 77


@pytest.fixture(scope="module")
def rt():
    if not has_gpu():
        pytest.skip("no GPU")
    import rtamd
    r = rtamd.Renderer((0,))
    r.set_option("rng_table_pixels", 0)        # the small frames here read the table too
    yield r
    r.close()


@contextlib.contextmanager
def _options(r, **kw):
    old = {k: r.get_option(k) for k in kw}
    try:
        for k, v in kw.items():
            r.set_option(k, v)
        yield
    finally:
        for k, v in old.items():
            r.set_option(k, v)


_BUILT = {}


def _built(k):
    if k not in _BUILT:
        from rtamd import configs
        _BUILT[k] = configs.get(k).build()
    return _BUILT[k]


def _same(a, b, what):
    assert np.array_equal(a[0], b[0]), f"{what}: RGBA8 differs from option 0"
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), f"{what}: radiance differs from option 0"


def _outputs(case):
    import torch
    from test_gpu_edges import _Guarded
    out = _Guarded(case.rows, case.width)
    torch.cuda.synchronize()
    return out


def _launch(case, stream, out):
    from rtamd._lib import check
    check(case.launch(out.rgba_ptr, out.rad_ptr, None, stream))


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------ the table --

def test_helper_pcg_is_the_oracles():
    import rng_table_ref as R
    from oracle import shader_np
    seeds = np.concatenate([np.arange(300, dtype=np.uint32), np.array([0x7FFFFFFF, 0x80000000, 0xFFFFFFFF], np.uint32),
                            (np.arange(300, dtype=np.uint64) * 2654435761 % (1 << 32)).astype(np.uint32)])
    want = shader_np.pcg(seeds)
    assert [R.pcg(int(s)) for s in seeds] == [int(x) for x in want]


def test_table_contents(rt):
    """Every word of the 37x19 table at K = 3, .w included."""
    import rng_table_ref as R
    from rtamd import configs
    w, h, k = 37, 19, 3
    _upload(rt, _built(2), 8)
    with _options(rt, rng_table=k, heavy_first=0):
        rt.render(configs.Camera.default(w, h), w, h, 4)
        assert rt.get_option("rng_table_used") == k
        words, tw, th, tk = rt.rng_table_copy()
    assert (tw, th, tk) == (w, h, k) and words.shape == (k, h, w, 4)
    want = R.table(w, h, k)
    bad = np.argwhere(words != want)
    assert bad.size == 0, f"{len(bad)} words differ, first (plane, y, x, word) {bad[:4].tolist()}"


def test_option_ranges(rt):
    from rtamd import RtError
    for name, bad in (("rng_table", -1), ("rng_table", 65), ("rng_table_mb", -1), ("rng_table_mb", (1 << 20) + 1),
                      ("rng_table_pixels", -1), ("rng_table_pixels", (1 << 30) + 1), ("rng_table_used", 1)):
        with pytest.raises(RtError):
            rt.set_option(name, bad)
    with _options(rt, rng_table=64, rng_table_mb=1 << 20):
        assert rt.get_option("rng_table") == 64 and rt.get_option("rng_table_mb") == 1 << 20
    with _options(rt, rng_table=0, rng_table_mb=0):
        assert rt.get_option("rng_table") == 0 and rt.get_option("rng_table_mb") == 0


# -------------------------------------------------------------------- frames --

def _frames_at(r, built, cam, w, h, b, ks, what):
    """The frame with the option at 0, then at each of ks: against the oracle
    and against option 0."""
    ref = _oracle(built, cam, w, h, b)
    with _options(r, rng_table=0, heavy_first=0):
        rgba, rad, _ = r.render(cam, w, h, b, radiance=True)
        assert r.get_option("rng_table_used") == 0
        _check(rgba, rad, None, ref, None, f"{what} K 0")
        base = (rgba, rad)
        for k in ks:
            r.set_option("rng_table", k)
            rgba, rad, _ = r.render(cam, w, h, b, radiance=True)
            tag = f"{what} {w}x{h} b{b} K {k}"
            assert r.get_option("rng_table_used") == k, tag
            _check(rgba, rad, None, ref, None, tag)
            _same((rgba, rad), base, tag)


@pytest.mark.parametrize("solo", [0, 1])
@pytest.mark.parametrize("cfg", [1, 2])
def test_frames_at_every_k(rt, cfg, solo):
    """1x1, 9x9 and 203x77 at 4 bounces with K = 1, 2, 3, max_bounces and
    max_bounces + 3 (and 0, the base)."""
    from rtamd import configs
    built = _built(cfg)
    _upload(rt, built, 8)
    b = 4
    with _options(rt, solo_lanes=solo):
        for (w, h) in [(1, 1), (9, 9), (W, H)]:
            _frames_at(rt, built, configs.Camera.default(w, h), w, h, b, (1, 2, 3, b, b + 3),
                       f"config {cfg} solo_lanes {solo}")


@pytest.mark.parametrize("nl", [1, 8])
def test_long_paths_cross_the_tables_end(rt, nl):
    """Config 2 at 10 bounces: with K = 10 the whole path is tabled, with K = 4
    a long path leaves the table and goes on with the seed it took from .w."""
    from rtamd import configs
    built = _built(2)
    _upload(rt, built, nl)
    w, h = 64, 36
    _frames_at(rt, built, configs.Camera.default(w, h), w, h, 10, (10, 4, 1), f"config 2 layouts {nl}")


def test_learned_order_at_the_defaults(rt):
    """heavy_first as shipped: the learning launch computes its draws, the
    launches in the learned order read the table; all three exact."""
    from rtamd import configs
    built = _built(2)
    _upload(rt, built, 8)
    cam = configs.Camera.default(W, H)
    ref = _oracle(built, cam, W, H, 4)
    with _options(rt, rng_table=2, heavy_first=1):
        used = []
        for i in range(3):
            rgba, rad, _ = rt.render(cam, W, H, 4, radiance=True)
            used.append(rt.get_option("rng_table_used"))
            _check(rgba, rad, None, ref, None, f"launch {i}")
        assert used[0] == 0 and used[1:] == [2, 2], used


# --------------------------------------------------------------------- split --

@pytest.mark.parametrize("solo", [0, 1])
def test_table_and_split(rt, solo):
    """Every pair of split_bounce in 1, 2, 3 and K in 1, 2, 3 on four 203x77
    frames per launch: the table ends before, at and after the split."""
    import torch
    import test_gpu_edges as E
    _upload(rt, E._scene("c3"), 8)
    case = E.case_batch(rt, "c3", W, H, 4)
    s = _stream()
    with _options(rt, solo_lanes=solo, heavy_first=0, rng_table=0, split_pixels=0, split_bounce=0, split_capacity=1024):
        out = _outputs(case)
        _launch(case, s, out)
        torch.cuda.synchronize()
        E._verify(case, out, None, 8, "unsplit, K 0")
        base = tuple(x.copy() for x in out.read())
        for split in (1, 2, 3):
            for k in (1, 2, 3):
                rt.set_option("split_bounce", split)
                rt.set_option("rng_table", k)
                out = _outputs(case)
                _launch(case, s, out)
                tag = f"solo_lanes {solo} split {split} K {k}"
                assert rt.get_option("split_bounce_used") == split and rt.get_option("rng_table_used") == k, tag
                torch.cuda.synchronize()
                E._verify(case, out, None, 8, tag)
                _same(out.read(), base, tag)
        assert rt.get_option("split_overflow") == 0


# -------------------------------------------------------------- launch paths --

def test_launch_paths_index_by_frame_coordinates(rt):
    """A tile with x0, y0 != 0, interleaved bands with an offset, one band list
    for every frame, per-frame lists with padding rows, a rectangle with
    x0 != 0 and packed runs: each against the same rows of the whole frame."""
    import torch
    import test_gpu_edges as E
    _upload(rt, E._scene("c3"), 8)
    s = _stream()
    cases = [E.case_tile(rt, "c3", W, H, (5, 3, 191, 70)), E.case_bands(rt, "c3", W, H, 3, 2, 1),
             E.case_bands(rt, "c3", W, H, 16, 2, 1), E.case_batch(rt, "c3", W, H, 2, band_h=7, bands=[1, 4, 10]),
             E.case_lists(rt, "c3", W, H, 7, E._lists_for(11)), E.case_rect(rt, "c3", W, H, (5, 3, 191, 70)),
             E.case_runs(rt, "c3", W, H, 11, E._runs_for(7))]
    with _options(rt, heavy_first=0, rng_table=2):
        for case in cases:
            out = _outputs(case)
            _launch(case, s, out)
            assert rt.get_option("rng_table_used") == 2, case.name
            torch.cuda.synchronize()
            E._verify(case, out, None, 8, case.name)


def test_counting_launches(rt):
    """Counting launches through the same paths with the option on: frames and
    counters are the oracle's and the model's (what option 0 gives)."""
    import test_gpu_edges as E
    _upload(rt, E._scene("c3"), 8)
    with _options(rt, heavy_first=0, rng_table=2):
        for case in (E.case_tile(rt, "c3", W, H, (5, 3, 191, 70)), E.case_lists(rt, "c3", W, H, 7, E._lists_for(11))):
            E._run(rt, case, 8, seq=(True,))
            assert rt.get_option("rng_table_used") == 2, case.name


def test_counters_equal_option_off(rt):
    from rtamd import configs
    built = _built(2)
    _upload(rt, built, 8)
    cam = configs.Camera.default(W, H)
    ref = _oracle(built, cam, W, H, 6)
    model = _model(built, cam, W, H, 6, 8)
    got = {}
    with _options(rt, heavy_first=0, rng_table=0):
        for k in (0, 3):
            rt.set_option("rng_table", k)
            rgba, rad, st = rt.render(cam, W, H, 6, radiance=True, stats=True)
            assert rt.get_option("rng_table_used") == k
            _check(rgba, rad, st, ref, model, f"K {k}")
            got[k] = {n: st[n] for n in ("segments", "node_visits", "tri_tests", "mat_reads")}
    assert got[0] == got[3], got


# ----------------------------------------------------- rebuilds and streams --

def test_two_resolutions_alternate(rt):
    """64x40, 203x77, 64x40 on one stream with no wait between the launches: a
    build, a rebuild while a launch on the old table is queued, and another."""
    import torch
    import test_gpu_edges as E
    _upload(rt, E._scene("c3"), 8)
    s = _stream()
    cases = [E.case_batch(rt, "c3", 64, 40, 1), E.case_batch(rt, "c3", W, H, 1), E.case_batch(rt, "c3", 64, 40, 1),
             E.case_batch(rt, "c3", 64, 40, 1)]
    with _options(rt, heavy_first=0, rng_table=2):
        outs = [_outputs(c) for c in cases]
        for c, o in zip(cases, outs):
            _launch(c, s, o)
            assert rt.get_option("rng_table_used") == 2
        assert rt.rng_table_copy()[1:] == (64, 40, 2)              # the last two launches share one table
        torch.cuda.synchronize()
        for i, (c, o) in enumerate(zip(cases, outs)):
            E._verify(c, o, None, 8, f"launch {i}: {c.name}")


def test_cold_start_on_four_streams():
    """A fresh context: the first four launches go out on four streams with
    nothing between them; none may read the table before it is complete."""
    import torch
    import rtamd
    import test_gpu_edges as E
    if not has_gpu():
        pytest.skip("no GPU")
    with rtamd.Renderer((0,)) as r:
        r.set_option("accel", 8)
        r.upload_scene(E._scene("c3"))
        for k, v in (("heavy_first", 0), ("rng_table", 3), ("rng_table_pixels", 0), ("concurrent_launches", 4)):
            r.set_option(k, v)
        cams = E._cams(W, H, 4)
        cases = [E.case_batch(r, "c3", W, H, 1, cams=[c]) for c in cams]
        outs = [_outputs(c) for c in cases]
        streams = [torch.cuda.Stream() for _ in range(4)]
        assert r.rng_table_copy()[3] == 0
        for c, o, st in zip(cases, outs, streams):
            _launch(c, st.cuda_stream, o)
            assert r.get_option("rng_table_used") == 3
        torch.cuda.synchronize()
        for j, (c, o) in enumerate(zip(cases, outs)):
            E._verify(c, o, None, 8, f"stream {j}")


def test_byte_cap(rt):
    """K = 64 on 203x77 is a 16 MB table: under a 1 MiB cap the launch computes
    its draws, and raising the cap brings the table in."""
    from rtamd import configs, lib
    built = _built(2)
    _upload(rt, built, 8)
    cam = configs.Camera.default(W, H)
    ref = _oracle(built, cam, W, H, 4)
    n = C.c_uint64()
    assert lib().rt_rng_table_bytes(W, H, 64, C.byref(n)) == 0 and n.value == W * H * 64 * 16 > 1 << 20
    with _options(rt, heavy_first=0, rng_table=64, rng_table_mb=1):
        for cap, want in ((1, 0), (512, 64), (0, 0)):
            rt.set_option("rng_table_mb", cap)
            rgba, rad, _ = rt.render(cam, W, H, 4, radiance=True)
            assert rt.get_option("rng_table_used") == want, cap
            _check(rgba, rad, None, ref, None, f"cap {cap} MiB")


# ------------------------------------------- launches that keep their draws --

def test_small_launches_compute_their_draws(rt):
    """Option rng_table_pixels counts the launch's pixels, all frames together:
    with the bar at two frames' worth a launch of one frame computes its draws,
    launches of two and of four frames read the table; all exact."""
    import torch
    import test_gpu_edges as E
    _upload(rt, E._scene("c3"), 8)
    s = _stream()
    with _options(rt, heavy_first=0, rng_table=2, rng_table_pixels=2 * W * H):
        for n, want in ((1, 0), (2, 2), (4, 2)):
            case = E.case_batch(rt, "c3", W, H, n)
            out = _outputs(case)
            _launch(case, s, out)
            assert rt.get_option("rng_table_used") == want, n
            torch.cuda.synchronize()
            E._verify(case, out, None, 8, f"{n} frame(s)")
        rt.set_option("rng_table_pixels", 2 * W * H + 1)
        case = E.case_batch(rt, "c3", W, H, 2)
        out = _outputs(case)
        _launch(case, s, out)
        assert rt.get_option("rng_table_used") == 0
        torch.cuda.synchronize()
        E._verify(case, out, None, 8, "one pixel short of the bar")



def test_new_sample_and_samples_launches_compute_their_draws(rt):
    from rtamd import configs
    built = _built(2)
    _upload(rt, built, 8)
    w, h, b = 64, 36, 4
    cam = configs.Camera.default(w, h)
    got = {}
    with _options(rt, heavy_first=0, rng_table=0, new_sample=0):
        for k in (0, 2):
            rt.set_option("rng_table", k)
            rt.set_option("new_sample", 1)
            cam.ubo.frame_count = 3
            a = rt.render(cam, w, h, b, radiance=True)
            assert rt.get_option("rng_table_used") == 0
            rt.set_option("new_sample", 0)
            cam.ubo.frame_count = 0
            s = rt.render_samples(cam, w, h, b, n_samples=3, radiance=True)
            assert rt.get_option("rng_table_used") == 0
            got[k] = (a, s)
    _same(got[2][0], got[0][0], "new_sample")
    _same(got[2][1], got[0][1], "samples")
    # and frame_count 0 of a new_sample launch is still the reference's frame
    ref = _oracle(built, cam, w, h, b)
    with _options(rt, heavy_first=0, rng_table=2, new_sample=1):
        rgba, rad, _ = rt.render(cam, w, h, b, radiance=True)
        _check(rgba, rad, None, ref, None, "new_sample at frame_count 0")
