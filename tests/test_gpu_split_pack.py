"""GPU parity of the split launch's packed queues (rt_trace.hip
kFeatQ1 / kFeatQ2): kernel 1's waves claim queue entries for the paths alive at
the split bounce, kernel 2 finishes them 64 to a wave, a wave whose claim does
not fit finishes its own, and the queues are reset by kernel 2 itself.

Bar (no tolerance anywhere): RGBA8 and the radiance bits equal the CPU oracle's
and the same launch unsplit, on 1 and 8 layouts with solo_lanes 0 and 1;
split_bounce_used says whether the launch split, and split_overflow how many
waves kept their paths.
"""
import contextlib

import numpy as np
import pytest

from conftest import has_gpu
from test_gpu_accel import _check, _oracle, _upload

pytestmark = pytest.mark.gpu

LAYOUTS = [1, 8]
SOLO = [0, 1]


@pytest.fixture(scope="module")
def sp():
    if not has_gpu():
        pytest.skip("no GPU")
    import rtamd
    r = rtamd.Renderer((0,))
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


def _built(name):
    import test_gpu_solo as S
    return S._built(name)


def _same(a, b, what):
    assert np.array_equal(a[0], b[0]), f"{what}: RGBA8 differs from the unsplit launch"
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), f"{what}: radiance differs from the unsplit launch"


def _frames(r, built, cam, w, h, b, splits, what, capacity=None):
    """The frame unsplit, then split at each of `splits` (three launches each:
    the learning launch stays one kernel, the next two run in the learned
    order): every launch against the oracle, the split ones against the
    unsplit one; returns the overflows read after each split."""
    ref = _oracle(built, cam, w, h, b)
    over = []
    with _options(r, split_bounce=0, split_pixels=0):
        rgba, rad, _ = r.render(cam, w, h, b, radiance=True)
        assert r.get_option("split_bounce_used") == 0
        _check(rgba, rad, None, ref, None, f"{what} unsplit")
        base = (rgba, rad)
        r.get_option("split_overflow")
        for split in splits:
            cap = capacity(split) if capacity else r.get_option("split_capacity")
            with _options(r, split_bounce=split, split_capacity=cap):
                for i in range(3):
                    rgba, rad, _ = r.render(cam, w, h, b, radiance=True)
                    tag = f"{what} {w}x{h} b{b} split {split} launch {i}"
                    _check(rgba, rad, None, ref, None, tag)
                    _same((rgba, rad), base, tag)
                assert r.get_option("split_bounce_used") == (split if split < b else 0), tag
                over.append(r.get_option("split_overflow"))
    return over


# ------------------------------------------------------------- frame shapes --

@pytest.mark.parametrize("solo", SOLO)
@pytest.mark.parametrize("nl", LAYOUTS)
def test_frame_shapes(sp, nl, solo):
    """1x1 (fewer waves than queues), 17x1 (a wave of one pixel), 16x4 (one
    full tile), 33x5 (partial tiles) and 203x77 (several queues, ragged last
    packs), 4 bounces, split at 1, 2 and 3.  Seven paths in ten are alive at
    bounce 1, so that split gets room for every pixel; 2 and 3 run at the
    default capacity.  Nothing overflows: the packed path is what ran."""
    from rtamd import configs
    built = _built("c3")
    _upload(sp, built, nl)
    with _options(sp, solo_lanes=solo):
        for (w, h) in [(1, 1), (17, 1), (16, 4), (33, 5), (203, 77)]:
            cam = configs.Camera.default(w, h)
            over = _frames(sp, built, cam, w, h, 4, (1, 2, 3), f"layouts {nl} solo_lanes {solo}",
                           capacity=lambda s: 1024 if s == 1 else 64)
            assert over == [0, 0, 0], (w, h, over)


@pytest.mark.parametrize("solo", SOLO)
@pytest.mark.parametrize("nl", LAYOUTS)
def test_config2_ten_bounces(sp, nl, solo):
    """Config 2's scene (cube faces: ties and the fallback walk) at 64x36 and
    10 bounces, split at 1, 2, 5 and 9, with room for every pixel (nothing
    overflows) and at the default capacity (whatever overflows stays exact)."""
    from rtamd import configs
    built = _built("c2")
    _upload(sp, built, nl)
    w, h, b = 64, 36, 10
    cam = configs.Camera.default(w, h)
    with _options(sp, solo_lanes=solo):
        over = _frames(sp, built, cam, w, h, b, (1, 2, 5, 9), f"config 2 layouts {nl} solo_lanes {solo}",
                       capacity=lambda s: 1024)
        assert over == [0, 0, 0, 0], over
        _frames(sp, built, cam, w, h, b, (1, 2, 5, 9), f"config 2 layouts {nl} solo_lanes {solo} default capacity")


# -------------------------------------------------------------- batch paths --

def _outputs(case):
    """Fresh guarded outputs for the case, their sentinel fill complete (it runs
    on torch's stream, the launches on theirs)."""
    import torch
    from test_gpu_edges import _Guarded
    out = _Guarded(case.rows, case.width)
    torch.cuda.synchronize()
    return out


def _launch(case, stream, out=None):
    """One plain launch of the case into guarded outputs (not waited for)."""
    from rtamd._lib import check
    out = out or _outputs(case)
    check(case.launch(out.rgba_ptr, out.rad_ptr, None, stream))
    return out


def _split_and_not(r, case, nl, what, launches=3, **split_opts):
    """The case's plain launches unsplit, then with split_opts: each verified
    against the oracle (guards and untouched rows included), the split ones
    equal to the unsplit ones and split at bounce 2."""
    import torch
    from test_gpu_edges import _verify
    s = torch.cuda.current_stream().cuda_stream
    base = None
    for opts, want in (({"split_bounce": 0, "split_pixels": 0}, 0), (split_opts, 2)):
        with _options(r, **opts):
            for i in range(launches):
                out = _launch(case, s)
                torch.cuda.synchronize()
                tag = f"{what} {opts} launch {i}"
                _verify(case, out, None, nl, tag)
            # (the first launch of a shape may be the learning launch: one kernel)
            assert r.get_option("split_bounce_used") == want, tag
            got = out.read()
            if base is None:
                base = (got[0].copy(), got[1].copy())
            else:
                _same(got, base, tag)


@pytest.mark.parametrize("solo", SOLO)
@pytest.mark.parametrize("nl", LAYOUTS)
def test_batch_paths_split_by_the_pixel_rule(sp, nl, solo):
    """split_bounce 0 with split_pixels lowered to 1: four 203x77 frames in one
    launch, per-frame band lists with padding rows, packed runs and a
    rectangle of 3 frames all split at bounce 2 by the automatic rule."""
    import test_gpu_edges as E
    w, h = 203, 77
    _upload(sp, E._scene("c3"), nl)
    with _options(sp, solo_lanes=solo):
        for case in (E.case_batch(sp, "c3", w, h, 4), E.case_lists(sp, "c3", w, h, 7, E._lists_for(11)),
                     E.case_runs(sp, "c3", w, h, 11, E._runs_for(7)), E.case_rect(sp, "c3", w, h, (5, 3, 191, 70))):
            _split_and_not(sp, case, nl, case.name, split_bounce=0, split_pixels=1)


# -------------------------------------------------------------- queue reset --

@pytest.mark.parametrize("solo", SOLO)
@pytest.mark.parametrize("nl", LAYOUTS)
def test_queue_reset_between_launches(sp, nl, solo):
    """Three plain launches in a row on one stream with three cameras and no
    wait between them, then the same on 4 streams at once: a queue that
    kernel 2 did not reset, or reset too early, shows as another launch's
    pixels (or as missing ones).  No learned order, so every launch splits."""
    import torch
    import test_gpu_edges as E
    w, h = 203, 77
    _upload(sp, E._scene("c3"), nl)
    cams = E._cams(w, h, 4)
    cases = [E.case_batch(sp, "c3", w, h, 1, cams=[c]) for c in cams]
    with _options(sp, solo_lanes=solo, heavy_first=0, split_bounce=0, split_pixels=1, concurrent_launches=4):
        sp.get_option("split_overflow")
        s0 = torch.cuda.current_stream().cuda_stream
        outs = [(cases[k], _outputs(cases[k])) for k in (0, 1, 2)]     # allocated first: no wait between launches
        for case, out in outs:
            _launch(case, s0, out)
            assert sp.get_option("split_bounce_used") == 2
        torch.cuda.synchronize()
        for case, out in outs:
            E._verify(case, out, None, nl, f"one stream, {case.name}")
        streams = [torch.cuda.Stream() for _ in range(4)]
        outs = [(j, cases[(k + j) % 4], _outputs(cases[(k + j) % 4])) for k in (0, 1, 2) for j in range(4)]
        for j, case, out in outs:
            _launch(case, streams[j].cuda_stream, out)
            assert sp.get_option("split_bounce_used") == 2
        torch.cuda.synchronize()
        for j, case, out in outs:
            E._verify(case, out, None, nl, f"stream {j} of 4, {case.name}")
        assert sp.get_option("split_overflow") == 0


# ----------------------------------------------------------------- capacity --

@pytest.mark.parametrize("solo", SOLO)
@pytest.mark.parametrize("nl", LAYOUTS)
def test_capacity(sp, nl, solo):
    """Four 203x77 frames split by the pixel rule: at the default capacity no
    claim fails; with one queue at the smallest capacity (one entry per 1024
    pixels: two packs for about 1800 survivors) some do and the frames are
    still exact; with no entries at all every wave with a survivor keeps its
    paths, no fewer waves than before."""
    import test_gpu_edges as E
    w, h = 203, 77
    _upload(sp, E._scene("c3"), nl)
    case = E.case_batch(sp, "c3", w, h, 4)
    with _options(sp, solo_lanes=solo, heavy_first=0):
        sp.get_option("split_overflow")
        _split_and_not(sp, case, nl, "default capacity", launches=1, split_bounce=0, split_pixels=1)
        assert sp.get_option("split_overflow") == 0
        _split_and_not(sp, case, nl, "smallest capacity", launches=1, split_bounce=0, split_pixels=1,
                       split_queues=1, split_capacity=1)
        some = sp.get_option("split_overflow")
        assert some > 0
        _split_and_not(sp, case, nl, "no capacity", launches=1, split_bounce=0, split_pixels=1, split_capacity=0)
        every = sp.get_option("split_overflow")
        assert every >= some and sp.get_option("split_overflow") == 0
        # and the queues are usable again afterwards
        _split_and_not(sp, case, nl, "default capacity again", launches=1, split_bounce=0, split_pixels=1)
        assert sp.get_option("split_overflow") == 0


# ------------------------------------------------------------- no survivors --

@pytest.mark.parametrize("n", [0, 1])
def test_no_survivors(sp, n):
    """An empty scene and a 1-triangle scene: no path is alive at bounce 2, so
    kernel 2 finds every queue empty (and resets it: the second launch)."""
    from rtamd import configs
    built = _built(f"tri{n}")
    w, h, b = 37, 23, 3
    cam = configs.Camera.default(w, h)
    ref = _oracle(built, cam, w, h, b)
    for nl in LAYOUTS:
        _upload(sp, built, nl)
        for solo in SOLO:
            with _options(sp, solo_lanes=solo, heavy_first=0, split_bounce=0, split_pixels=1):
                for i in range(2):
                    rgba, rad, _ = sp.render(cam, w, h, b, radiance=True)
                    assert sp.get_option("split_bounce_used") == 2
                    _check(rgba, rad, None, ref, None, f"{n} triangles layouts {nl} solo_lanes {solo} launch {i}")
                assert sp.get_option("split_overflow") == 0


def test_launches_that_stay_one_kernel(sp):
    """The pixel rule needs 3 bounces; counting, learning and extension
    launches never split."""
    from rtamd import configs
    built = _built("c3")
    w, h = 64, 36
    cam = configs.Camera.default(w, h)
    _upload(sp, built, 8)
    with _options(sp, split_bounce=0, split_pixels=1):
        with _options(sp, heavy_first=0):
            for b, want in ((1, 0), (2, 0), (3, 2), (4, 2)):
                rgba, rad, _ = sp.render(cam, w, h, b, radiance=True)
                assert sp.get_option("split_bounce_used") == want, b
                _check(rgba, rad, None, _oracle(built, cam, w, h, b), None, f"b{b}")
            ref = _oracle(built, cam, w, h, 4)
            rgba, rad, st = sp.render(cam, w, h, 4, radiance=True, stats=True)      # a counting launch
            assert sp.get_option("split_bounce_used") == 0
            _check(rgba, rad, st, ref, None, "counting")
            with _options(sp, split_pixels=w * h + 1):                               # a launch below the threshold
                sp.render(cam, w, h, 4)
                assert sp.get_option("split_bounce_used") == 0
            with _options(sp, split_pixels=w * h):
                sp.render(cam, w, h, 4)
                assert sp.get_option("split_bounce_used") == 2
            with _options(sp, extensions=1):                                         # an extensions launch
                sp.render(cam, w, h, 4)
                assert sp.get_option("split_bounce_used") == 0
        # a learning launch (the first plain launch of a new shape with heavy_first), then its replay
        _upload(sp, built, 8)
        w2, h2 = 80, 45
        cam2 = configs.Camera.default(w2, h2)
        ref2 = _oracle(built, cam2, w2, h2, 4)
        rgba, rad, _ = sp.render(cam2, w2, h2, 4, radiance=True)
        assert sp.get_option("split_bounce_used") == 0
        _check(rgba, rad, None, ref2, None, "learning")
        for i in range(2):
            rgba, rad, _ = sp.render(cam2, w2, h2, 4, radiance=True)
            _check(rgba, rad, None, ref2, None, f"replay {i}")
        assert sp.get_option("split_bounce_used") == 2
