"""GPU parity at ragged frame, band and batch shapes, on every launch path.

The hand-written part of trace_simple and of enqueue_render / plan_order maps
a lane to a pixel, a local row to a frame row, a workgroup to a tile and a
frame to an output row.  The other GPU suites run that mapping almost only
where nothing is partial; here every entry point runs at widths and heights
that leave partial wave tiles, band heights that are no multiple of the
tile's rows, per-frame band lists of unequal length, 1 to 16 frames per
launch, every tile shape, every accel format and the split launch.

Bar (no tolerance anywhere): RGBA8 and float radiance bit-exact against the
CPU oracle's frame of the same camera; on counting launches segments and
material reads equal the oracle's sums over exactly the traced pixels, node
visits and triangle tests the oracle's (accel 0) or the accel model's (accel
walks), and `pixels` the traced count.

Every output is allocated with 4096 bytes of guard before and after the
region the library is given, all of it filled with a sentinel (RGBA bytes 7,
so alpha != 255; radiance -2.0): after each launch the guards and every row
the launch must not write still hold the sentinel, and no traced pixel does.

Each case runs a plain launch (it learns the order), a counting launch and a
plain launch in the learned order; all are checked.
"""
import ctypes as C
from dataclasses import dataclass, field

import numpy as np
import pytest

from conftest import has_gpu
from test_gpu_accel import HALF8, WIDE, _model, _upload
from test_gpu_parity import COUNTERS, DEFAULT_OPTS, WALKS, _assert_same, _oracle

pytestmark = pytest.mark.gpu

B = 4
SHAPES = [(203, 77), (65, 9), (37, 23), (64, 1), (8, 8), (1, 1)]
SHAPE_IDS = [f"{w}x{h}" for w, h in SHAPES]
GUARD = 4096                       # bytes before and after every output region
RGBA_SENTINEL = 7                  # every byte: alpha 7, never a frame's 255
RAD_SENTINEL = -2.0                # the radiance is a square root: never negative

_MODE = {"accel": 0, "scene": None}


def _defaults(accel):
    d = dict(DEFAULT_OPTS)
    if accel:
        d["coop_lanes"] = -1
    d["split_bounce"] = 0
    return d


def _restore(r, accel):
    for k, v in _defaults(accel).items():
        r.set_option(k, v)


@pytest.fixture(scope="module", params=WALKS, ids=lambda a: f"accel{a}")
def renderer(request):
    """One context per walk for the module."""
    if not has_gpu():
        pytest.skip("no GPU")
    import rtamd
    r = rtamd.Renderer((0,))
    r.set_option("accel", request.param)
    _MODE["accel"] = request.param
    _MODE["scene"] = None
    _restore(r, request.param)
    yield r
    r.close()


@pytest.fixture(scope="module")
def acc():
    """A context of its own for the tests that choose the accel format."""
    if not has_gpu():
        pytest.skip("no GPU")
    import rtamd
    r = rtamd.Renderer((0,))
    yield r
    r.close()


# ------------------------------------------------------------ scenes, oracle --

_SCENES = {}


def _scene(name):
    """Config 3's scene (50k triangles: a deep SAH tree, all 8 layouts, thin
    records, fallback segments) and config 2's (cube faces: ties and the
    fallback), built once per module."""
    if name not in _SCENES:
        from rtamd import configs
        _SCENES[name] = configs.get({"c3": 3, "c2": 2}[name]).build()
    return _SCENES[name]


def _use_scene(r, name):
    """Uploads the scene unless the module's context already holds it (an
    upload drops the learned orders)."""
    if _MODE["scene"] != name:
        r.upload_scene(_scene(name))
        _MODE["scene"] = name


def _cams(w, h, n):
    """n distinct cameras; the first is the app's default."""
    from rtamd import configs
    return [configs.Camera.default(w, h) if k == 0 else
            configs.Camera((-25.0 + 5 * k, 30.0, 140.0 - 6 * k), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 20.0, w / h)
            for k in range(n)]


@dataclass
class _Frame:
    """The oracle's frame of one (scene, camera, W, H, bounces), its counts
    row by row, and per accel format the model's counts pixel by pixel."""
    scene: str
    cam: object
    w: int
    h: int
    b: int
    rgba: np.ndarray
    rad: np.ndarray
    rows: np.ndarray                          # int64 [H, 4]: COUNTERS of each row
    rects: dict = field(default_factory=dict)
    model: dict = field(default_factory=dict)

    def counts(self, ys, x0, tw, nl):
        """COUNTERS over the pixels rows ys x columns [x0, x0 + tw)."""
        built = _scene(self.scene)
        if x0 == 0 and tw == self.w:
            c = self.rows[ys].sum(0) if len(ys) else np.zeros(4, np.int64)
        else:                                 # a rectangle: the oracle on it as a tile
            y0, th = int(ys[0]), len(ys)
            assert list(ys) == list(range(y0, y0 + th))
            key = (x0, y0, tw, th)
            if key not in self.rects:
                cnt = _oracle(built, self.cam.ubo_bytes(), self.w, self.h, self.b, accel=0, tile=key,
                              radiance=False)[2]
                self.rects[key] = np.array([cnt[k] for k in COUNTERS], np.int64)
            c = self.rects[key]
        out = dict(zip(COUNTERS, (int(x) for x in c)))
        if nl:
            if nl not in self.model:
                m = _model(built, self.cam, self.w, self.h, self.b, nl, profile=True)
                prof = m[3].astype(np.int64)
                node, tri = (prof & 0xFFFFF).sum(-1), (prof >> 20).sum(-1)
                # the per-pixel profile packs two counts in a word: it must add up to the model's totals
                assert int(node.sum()) == m[2]["node_visits"] and int(tri.sum()) == m[2]["tri_tests"]
                assert np.array_equal(m[0], self.rgba)
                self.model[nl] = (node, tri)
            node, tri = self.model[nl]
            ys = np.asarray(ys, np.int64)
            out["node_visits"] = int(node[ys, x0:x0 + tw].sum())
            out["tri_tests"] = int(tri[ys, x0:x0 + tw].sum())
        return out


_FRAMES = {}


def _frame(scene, cam, w, h, b=B):
    key = (scene, cam.ubo_bytes(), w, h, b)
    if key not in _FRAMES:
        built = _scene(scene)
        rgba, rad, _ = _oracle(built, cam.ubo_bytes(), w, h, b, accel=0)
        rows = np.zeros((h, 4), np.int64)
        for y in range(h):
            cnt = _oracle(built, cam.ubo_bytes(), w, h, b, accel=0, tile=(0, y, w, 1), radiance=False)[2]
            rows[y] = [cnt[k] for k in COUNTERS]
        _FRAMES[key] = _Frame(scene, cam, w, h, b, rgba, rad, rows)
    return _FRAMES[key]


# ---------------------------------------------------------- guarded outputs --

class _Guarded:
    """The outputs of one launch, each one allocation with GUARD bytes before
    and after the region the library is given, all filled with the sentinel.
    host: pageable host memory (rt_render), else device memory."""

    def __init__(self, rows, width, rgba=True, rad=True, host=False):
        self.rows, self.width, self.host = rows, width, host
        self.n_rgba = rows * width * 4 if rgba else None
        self.n_rad = rows * width * 3 if rad else None
        self.t_rgba = self.t_rad = None
        if host:
            if rgba:
                self.t_rgba = np.full(2 * GUARD + self.n_rgba, RGBA_SENTINEL, np.uint8)
            if rad:
                self.t_rad = np.full(2 * (GUARD // 4) + self.n_rad, RAD_SENTINEL, np.float32)
        else:
            import torch
            if rgba:
                self.t_rgba = torch.full((2 * GUARD + self.n_rgba,), RGBA_SENTINEL, dtype=torch.uint8, device="cuda:0")
            if rad:
                self.t_rad = torch.full((2 * (GUARD // 4) + self.n_rad,), RAD_SENTINEL, dtype=torch.float32,
                                        device="cuda:0")

    def _base(self, t):
        return t.ctypes.data if self.host else t.data_ptr()

    @property
    def rgba_ptr(self):
        return self._base(self.t_rgba) + GUARD if self.t_rgba is not None else None

    @property
    def rad_ptr(self):
        return self._base(self.t_rad) + GUARD if self.t_rad is not None else None

    def read(self):
        """(rgba[rows, width, 4] or None, radiance[rows, width, 3] or None)
        after checking both guards of each."""
        out = []
        for t, n, sentinel, g, shape in ((self.t_rgba, self.n_rgba, RGBA_SENTINEL, GUARD, (self.rows, self.width, 4)),
                                         (self.t_rad, self.n_rad, RAD_SENTINEL, GUARD // 4,
                                          (self.rows, self.width, 3))):
            if t is None:
                out.append(None)
                continue
            a = t if self.host else t.cpu().numpy()
            assert (a[:g] == sentinel).all(), "the guard before the output was written"
            assert (a[g + n:] == sentinel).all(), "the guard after the output was written"
            out.append(a[g:g + n].reshape(shape))
        return tuple(out)


@dataclass
class _Case:
    """One launch shape: `launch(rgba_ptr, rad_ptr, stats_ref, stream)` writes
    `pieces` (output row, frame, the frame's rows ys, columns [x0, x0 + tw))
    into buffers of rows x width pixels and must leave every other row alone."""
    name: str
    rows: int
    width: int
    pieces: list
    launch: object
    host: bool = False
    rgba_required: bool = False


MODES = {"both": (True, True), "rgba": (True, False), "rad": (False, True)}


def _verify(case, out, st, nl, what):
    rgba, rad = out.read()
    traced = np.zeros(case.rows, bool)
    want = {k: 0 for k in COUNTERS}
    pixels = 0
    for row0, fr, ys, x0, tw in case.pieces:
        n = len(ys)
        if n == 0:
            continue
        assert tw == case.width and not traced[row0:row0 + n].any()
        traced[row0:row0 + n] = True
        ys = np.asarray(ys, np.int64)
        ref_rgba, ref_rad = fr.rgba[ys, x0:x0 + tw], fr.rad[ys, x0:x0 + tw]
        try:
            if rgba is not None:
                got = rgba[row0:row0 + n]
                assert (got[..., 3] == 255).all(), "a traced pixel still holds the sentinel"
                _assert_same(got, None, None, ref_rgba, None, None)
            if rad is not None:
                got = rad[row0:row0 + n]
                assert (got != RAD_SENTINEL).all(), "a traced pixel's radiance still holds the sentinel"
                assert np.array_equal(got.view(np.uint32), ref_rad.view(np.uint32)), "radiance bits differ"
        except AssertionError as e:
            raise AssertionError(f"{what}, piece at output row {row0} ({n} rows): {e}")
        if st is not None:
            for k, v in fr.counts(ys, x0, tw, nl).items():
                want[k] += v
            pixels += n * tw
    if rgba is not None:
        assert (rgba[~traced] == RGBA_SENTINEL).all(), f"{what}: a row the launch must not write was written (RGBA)"
    if rad is not None:
        assert (rad[~traced] == RAD_SENTINEL).all(), f"{what}: a row the launch must not write was written (radiance)"
    if st is not None:
        sd = st.as_dict()
        for k in COUNTERS:
            assert sd[k] == want[k], (what, k, sd[k], want[k])
        assert sd["pixels"] == pixels, (what, sd["pixels"], pixels)


def _run(r, case, nl, modes=("both",), seq=(False, True, False), heavy=None, stream=None):
    """The launch sequence of one case (plain: it learns; counting; plain in
    the learned order), once per output mode; every launch checked.  heavy:
    True = the last plain launch must have traced heavy pixels one per wave,
    False = none."""
    import torch
    from rtamd._lib import Stats, check
    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    for mode in modes:
        want_rgba, want_rad = MODES[mode]
        if case.rgba_required and not want_rgba:
            continue
        for i, stats in enumerate(seq):
            out = _Guarded(case.rows, case.width, want_rgba, want_rad, case.host)
            st = Stats(*([0xAB] * 4), 171.0, 0xAB) if stats else None     # junk the call must overwrite
            check(case.launch(out.rgba_ptr, out.rad_ptr, C.byref(st) if st is not None else None, s))
            torch.cuda.synchronize()
            _verify(case, out, st, nl, f"{case.name} [{mode}, launch {i}{' counting' if stats else ''}]")
        if heavy is not None and any(len(p[2]) for p in case.pieces):
            used = r.get_option("heavy_pixels_used")
            assert (used > 0) == heavy, (case.name, mode, used)


# ----------------------------------------------------------- the entry points --

def _ubos(cams):
    from rtamd import CameraUBO
    return (CameraUBO * len(cams))(*[c.ubo for c in cams])


def _i32(xs):
    return (C.c_int32 * max(1, len(xs)))(*xs)


def case_render(r, scene, w, h, b=B):
    from rtamd import lib
    cam = _cams(w, h, 1)[0]
    fr = _frame(scene, cam, w, h, b)
    return _Case(f"rt_render {w}x{h}", h, w, [(0, fr, np.arange(h), 0, w)],
                 lambda pr, pf, st, s: lib().rt_render(r._ctx, C.byref(cam.ubo), w, h, b, pr, pf, st),
                 host=True, rgba_required=True)


def case_tile(r, scene, w, h, rect, b=B):
    from rtamd import lib
    x0, y0, tw, th = rect
    cam = _cams(w, h, 1)[0]
    fr = _frame(scene, cam, w, h, b)
    return _Case(f"rt_render_tile_device {w}x{h} {rect}", th, tw, [(0, fr, np.arange(y0, y0 + th), x0, tw)],
                 lambda pr, pf, st, s: lib().rt_render_tile_device(r._ctx, C.byref(cam.ubo), w, h, b, x0, y0, tw, th,
                                                                  pr, pf, s, st))


def case_rect(r, scene, w, h, rect, n=3, b=B):
    from rtamd import lib
    x0, y0, tw, th = rect
    cams = _cams(w, h, n)
    ubos = _ubos(cams)
    pieces = [(f * th, _frame(scene, c, w, h, b), np.arange(y0, y0 + th), x0, tw) for f, c in enumerate(cams)]
    return _Case(f"rt_render_batch_rect_device {w}x{h} {rect} x{n}", n * th, tw, pieces,
                 lambda pr, pf, st, s: lib().rt_render_batch_rect_device(r._ctx, ubos, n, w, h, b, x0, y0, tw, th,
                                                                        pr, pf, s, st))


def case_bands(r, scene, w, h, band_h, stride, off, b=B):
    from rtamd import lib
    cam = _cams(w, h, 1)[0]
    fr = _frame(scene, cam, w, h, b)
    ys = np.array([y for y in range(h) if (y // band_h) % stride == off], np.int64)
    assert lib().rt_band_rows(h, band_h, stride, off) == len(ys)
    # (no row to trace: the call returns at once; a few rows show that nothing is written)
    return _Case(f"rt_render_bands_device {w}x{h} ({band_h},{stride},{off})", max(len(ys), 2), w,
                 [(0, fr, ys, 0, w)],
                 lambda pr, pf, st, s: lib().rt_render_bands_device(r._ctx, C.byref(cam.ubo), w, h, b, band_h, stride,
                                                                   off, pr, pf, s, st))


def case_batch(r, scene, w, h, n, band_h=0, bands=None, b=B, cams=None):
    """rt_render_batch_device: whole frames (bands None) or one band list for
    every frame (the last band may be partial; an empty list traces nothing)."""
    from rtamd import lib
    cams = cams or _cams(w, h, n)
    ubos = _ubos(cams)
    if bands is None:
        ys, arr, nb = np.arange(h), None, 0
    else:
        ys = np.array([y for bnd in bands for y in range(bnd * band_h, min(h, (bnd + 1) * band_h))], np.int64)
        arr, nb = _i32(bands), len(bands)
        assert lib().rt_band_list_rows(h, band_h, arr, nb) == len(ys)
    R = len(ys)
    pieces = [(f * R, _frame(scene, c, w, h, b), ys, 0, w) for f, c in enumerate(cams)]
    return _Case(f"rt_render_batch_device {w}x{h} x{n} band_h {band_h} bands {bands}", max(n * R, 2), w, pieces,
                 lambda pr, pf, st, s: lib().rt_render_batch_device(r._ctx, ubos, n, w, h, b, band_h, arr, nb, pr, pf,
                                                                   s, st))


def _lists_for(nb):
    """Per-frame band lists of unequal length over nb bands: the whole frame,
    a list from band 0, an empty list, a list ending at the last band."""
    return [list(range(nb)), sorted({0, 2 % nb, 5 % nb}), [], sorted({1 % nb, nb - 1})]


def case_lists(r, scene, w, h, band_h, lists, b=B):
    """rt_render_batch_lists_device: frame f's list, -1 padded to the longest;
    list position k is written at rows f * R + k * band_h; padding rows stay
    untouched (they share wave tiles with real rows where band_h is no
    multiple of the tile's rows)."""
    from rtamd import lib
    assert h % band_h == 0
    n = len(lists)
    n_per = max(1, max(len(x) for x in lists))
    flat = np.full((n, n_per), -1, np.int32)
    for f, x in enumerate(lists):
        flat[f, :len(x)] = x
    arr = flat.ctypes.data_as(C.POINTER(C.c_int32))
    R = lib().rt_band_lists_rows(h, band_h, arr, n, n_per)
    assert R == n_per * band_h
    cams = _cams(w, h, n)
    ubos = _ubos(cams)
    pieces = []
    for f, (c, x) in enumerate(zip(cams, lists)):
        ys = np.array([y for bnd in x for y in range(bnd * band_h, (bnd + 1) * band_h)], np.int64)
        pieces.append((f * R, _frame(scene, c, w, h, b), ys, 0, w))
    case = _Case(f"rt_render_batch_lists_device {w}x{h} band_h {band_h} {lists}", n * R, w, pieces,
                 lambda pr, pf, st, s: lib().rt_render_batch_lists_device(r._ctx, ubos, n, w, h, b, band_h, arr, n_per,
                                                                         pr, pf, s, st))
    case.keep = flat
    return case


def _runs_for(nb):
    """A run ending at the last band, the whole frame, an empty run, a run from band 0."""
    return [(max(0, nb - 3), nb), (0, nb), (min(4, nb), min(4, nb)), (0, min(2, nb))]


def case_runs(r, scene, w, h, band_h, runs, b=B, tail=3):
    """rt_render_batch_runs_device: frame f's rows follow frame f - 1's; the
    rows past the packed total (`tail` of them here) stay untouched."""
    from rtamd import lib
    assert h % band_h == 0
    n = len(runs)
    lo, hi = _i32([a for a, _ in runs]), _i32([z for _, z in runs])
    cams = _cams(w, h, n)
    ubos = _ubos(cams)
    pieces, row = [], 0
    for c, (a, z) in zip(cams, runs):
        ys = np.arange(a * band_h, z * band_h)
        pieces.append((row, _frame(scene, c, w, h, b), ys, 0, w))
        row += len(ys)
    return _Case(f"rt_render_batch_runs_device {w}x{h} band_h {band_h} {runs}", row + tail, w, pieces,
                 lambda pr, pf, st, s: lib().rt_render_batch_runs_device(r._ctx, ubos, n, w, h, b, band_h, lo, hi,
                                                                        pr, pf, s, st))


RECTS = {(203, 77): [(5, 3, 191, 70), (0, 0, 1, 77)], (65, 9): [(1, 1, 63, 7), (64, 0, 1, 9)],
         (37, 23): [(3, 5, 31, 13), (0, 22, 37, 1)], (64, 1): [(7, 0, 50, 1), (63, 0, 1, 1)],
         (8, 8): [(1, 1, 6, 6), (0, 0, 8, 8)], (1, 1): [(0, 0, 1, 1)]}
BANDS = [(1, 3, 2), (3, 2, 1), (5, 4, 0), (7, 1, 0), (16, 2, 1)]
# band heights that divide the height (the lists and runs entry points need
# it) and, where the height allows, are no multiple of the tiles' 2/4/8 rows
LIST_BAND_H = {77: (7, 11), 9: (3,), 23: (1,), 1: (1,), 8: (2,)}


def _heavy(w, h):
    """The default schedule's expectation at the 203 x 77 shapes: heavy pixels
    on the reference tree (the fused one-pixel waves and the tile masks then
    run on partial tiles), none on the accel walks (by design)."""
    if (w, h) != (203, 77):
        return None
    return not _MODE["accel"]


ENTRIES = ("render", "tile", "rect", "bands", "batch", "lists", "runs")


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("entry", ENTRIES)
def test_entry_points_at_ragged_shapes(renderer, entry, shape):
    """Every entry point at every shape, default schedule: rectangles that
    start and end off tile boundaries, band heights 1, 3, 5, 7 and 16 at
    several strides, a band list with the partial last band, an empty list,
    per-frame lists and runs of unequal length.  The first case of each id
    also runs with RGBA only and with radiance only."""
    r, nl = renderer, _MODE["accel"]
    w, h = shape
    _use_scene(r, "c3")
    if entry == "render":
        cases = [case_render(r, "c3", w, h)]
    elif entry == "tile":
        cases = [case_tile(r, "c3", w, h, rect) for rect in RECTS[shape]]
    elif entry == "rect":
        cases = [case_rect(r, "c3", w, h, rect) for rect in RECTS[shape]]
    elif entry == "bands":
        cases = [case_bands(r, "c3", w, h, *bnd) for bnd in BANDS]
    elif entry == "batch":
        nb = (h + 4) // 5
        cases = [case_batch(r, "c3", w, h, 3, 5, sorted({0, 3 % nb, nb - 1})),    # with the partial last band
                 case_batch(r, "c3", w, h, 2),
                 case_batch(r, "c3", w, h, 2, 5, [])]
    elif entry == "lists":
        cases = [case_lists(r, "c3", w, h, bh, _lists_for(h // bh)) for bh in LIST_BAND_H[h]]
    else:
        cases = [case_runs(r, "c3", w, h, bh, _runs_for(h // bh)) for bh in LIST_BAND_H[h]]
    for i, case in enumerate(cases):
        _run(r, case, nl, modes=("both", "rgba", "rad") if i == 0 else ("both",), heavy=_heavy(w, h))


def test_reference_bounces_through_lists(renderer):
    """Config 2 at the reference's 10 bounces through the per-frame lists."""
    r, nl = renderer, _MODE["accel"]
    _use_scene(r, "c2")
    w, h = 203, 77
    _run(r, case_lists(r, "c2", w, h, 7, _lists_for(11), b=10), nl)
    _run(r, case_runs(r, "c2", w, h, 11, _runs_for(7), b=10), nl)


# ------------------------------------------------------- frames per launch --

@pytest.mark.parametrize("order_frames", [0, 1])
@pytest.mark.parametrize("n", [1, 3, 4, 16])
def test_frames_per_launch(renderer, n, order_frames):
    """1, 3, 4 and 16 (the most a launch takes) whole frames of 203 x 77 with
    distinct cameras in one rt_render_batch_device launch, the order's rows
    frame by frame and interleaved across the frames (order_frames)."""
    r, nl = renderer, _MODE["accel"]
    _use_scene(r, "c3")
    try:
        r.set_option("order_frames", order_frames)
        _run(r, case_batch(r, "c3", 203, 77, n), nl, heavy=_heavy(203, 77))
    finally:
        _restore(r, nl)


def test_bench_shape_four_frames_on_four_streams(renderer):
    """bench.py's N = 1 shape at a ragged frame: 4 launches in flight on 4
    streams (concurrent_launches 4), each 4 whole frames into its own slot,
    through rtamd.dist.ShareTracer; a plain round, a counting round, a plain
    round."""
    import torch
    from rtamd._lib import Stats
    from rtamd.dist import ShareTracer
    r, nl = renderer, _MODE["accel"]
    _use_scene(r, "c3")
    w, h, D, F = 203, 77, 4, 4
    cams = _cams(w, h, D * F)
    tracer = ShareTracer(r._ctx, w, h, B, "whole")
    streams = [torch.cuda.Stream() for _ in range(D)]
    cases = []
    for j in range(D):
        mine = cams[j * F:(j + 1) * F]
        pieces = [(f * h, _frame("c3", c, w, h), np.arange(h), 0, w) for f, c in enumerate(mine)]
        cases.append((_Case(f"ShareTracer stream {j}", F * h, w, pieces, None), _ubos(mine)))
    try:
        r.set_option("concurrent_launches", D)
        for rnd, stats in enumerate((False, True, False)):
            torch.cuda.synchronize()
            outs = [_Guarded(F * h, w) for _ in range(D)]
            sts = [Stats() if stats else None for _ in range(D)]
            torch.cuda.synchronize()
            for j, (case, ubos) in enumerate(cases):
                tracer.launch(ubos, j * F, F, streams[j].cuda_stream, outs[j].rgba_ptr, outs[j].rad_ptr, sts[j])
            torch.cuda.synchronize()
            for j, (case, _) in enumerate(cases):
                _verify(case, outs[j], sts[j], nl, f"{case.name} round {rnd}")
    finally:
        _restore(r, nl)


# ------------------------------------------------ schedules at ragged shapes --

SCHEDULES = [{"wave_tile": s, "block_waves": bw} for s in (0, 1, 2, 3) for bw in (1, 4)] + \
            [{"coop_lanes": c} for c in (0, 8, 64)]


@pytest.mark.parametrize("opts", SCHEDULES, ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()))
def test_schedules_at_ragged_shapes(renderer, opts):
    """Every tile shape (8x8 to 64x1) with one and four waves per workgroup,
    and the cooperative tail at 0, 8 and 64 lanes, through the strided bands
    (band_h 5) and the per-frame lists (band_h 7 at 77 rows; 3 at 9 rows, the
    heights' divisors that are no multiple of the tiles' rows) at 203 x 77 and
    65 x 9."""
    r, nl = renderer, _MODE["accel"]
    _use_scene(r, "c3")
    try:
        for k, v in opts.items():
            r.set_option(k, v)
        for (w, h), bh in (((203, 77), 7), ((65, 9), 3)):
            _run(r, case_bands(r, "c3", w, h, 5, 4, 0), nl)
            _run(r, case_lists(r, "c3", w, h, bh, _lists_for(h // bh)[:3]), nl)
    finally:
        _restore(r, nl)


# ------------------------------ accel formats and the split launch, batched --

@pytest.mark.parametrize("nl", [1, 8, HALF8, WIDE])
def test_accel_formats_through_batch_paths(acc, nl):
    """1 and 8 layouts, the half-precision boxes and the 4-wide tree through
    the per-frame lists, the packed runs and the rectangle of 3 frames at
    203 x 77."""
    w, h = 203, 77
    _upload(acc, _scene("c3"), nl)
    _run(acc, case_lists(acc, "c3", w, h, 7, _lists_for(11)[:3]), nl)
    _run(acc, case_runs(acc, "c3", w, h, 11, _runs_for(7)[:3]), nl)
    _run(acc, case_rect(acc, "c3", w, h, (5, 3, 191, 70)), nl)


@pytest.mark.parametrize("split", [1, 3])
def test_split_launch_through_batch_paths(acc, split):
    """Option split_bounce with accel 8 through 4 whole frames, the per-frame
    lists and the packed runs: kernel 2 rebuilds a path's output row and
    column from lyo * tw + lx, here with per-frame row offsets, padding rows
    and a 203-pixel row.  The learning and counting launches stay one kernel,
    so two plain launches follow them."""
    w, h = 203, 77
    _upload(acc, _scene("c3"), 8)
    seq = (False, True, False, False)
    try:
        acc.set_option("split_bounce", split)
        _run(acc, case_batch(acc, "c3", w, h, 4), 8, seq=seq)
        _run(acc, case_lists(acc, "c3", w, h, 7, _lists_for(11)), 8, seq=seq)
        _run(acc, case_runs(acc, "c3", w, h, 11, _runs_for(7)), 8, seq=seq)
        _run(acc, case_rect(acc, "c3", w, h, (5, 3, 191, 70)), 8, seq=seq)
    finally:
        acc.set_option("split_bounce", 0)


# ----------------------------------------------------- multi-device context --

@pytest.mark.parametrize("accel", WALKS)
def test_multi_device_context_at_ragged_shapes(accel):
    """rt_create with the same GPU twice: rt_render's multi-device band path
    at 203 x 77, 65 x 9 and 1 x 1 equals the oracle."""
    if not has_gpu():
        pytest.skip("no GPU")
    import rtamd
    with rtamd.Renderer((0, 0)) as r2:
        r2.set_option("accel", accel)
        r2.upload_scene(_scene("c3"))
        assert r2.get_option("accel_used") == accel
        for (w, h) in [(203, 77), (65, 9), (1, 1)]:
            _run(r2, case_render(r2, "c3", w, h), accel, modes=("both", "rgba"))


# ------------------------------------------------------------ cache turnover --

def test_band_list_cache_turnover(renderer):
    """300 distinct band lists (band_h 1 of a 24 x 40 frame, 2 frames per
    launch): past 256 the runtime drops every device band list, and past 16
    learned orders the oldest; then the first list again."""
    r, nl = renderer, _MODE["accel"]
    _use_scene(r, "c2")
    w, h = 24, 40
    lists = [[i * 4 + k % 4 for i in range(10) if ((k // 4 + 1) >> i) & 1] for k in range(300)]
    assert len({tuple(x) for x in lists}) == 300
    for x in lists + lists[:1]:
        _run(r, case_batch(r, "c2", w, h, 2, 1, x), nl, seq=(False,))
    _run(r, case_batch(r, "c2", w, h, 2, 1, lists[0]), nl)


def test_learned_order_turnover(renderer):
    """20 cameras of one frame geometry, three launches each (a camera's
    repeat learns its own order: more than the 16 the runtime keeps), then
    the first camera again."""
    from rtamd import configs
    r, nl = renderer, _MODE["accel"]
    _use_scene(r, "c2")
    w, h = 24, 40
    cams = [configs.Camera((-25.0 + 2 * k, 30.0, 140.0 - 3 * k), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 20.0, w / h)
            for k in range(20)]
    for c in cams + cams[:1]:
        _run(r, case_batch(r, "c2", w, h, 1, cams=[c]), nl)


def test_frame_geometry_turnover(renderer):
    """70 frame geometries (heights 1 to 70) once each, more than the 64 the
    runtime remembers the last camera of, then the first again."""
    r, nl = renderer, _MODE["accel"]
    _use_scene(r, "c2")
    for hh in list(range(1, 71)) + [1]:
        _run(r, case_batch(r, "c2", 24, hh, 1), nl, seq=(False,))
    _run(r, case_batch(r, "c2", 24, 1, 1), nl)
