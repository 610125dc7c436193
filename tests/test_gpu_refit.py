"""rt_update_geometry on the GPU (include/rtamd.h "refit"): a
scene uploaded with option refit 1 whose triangles move must afterwards
render, count, answer queries and hold records exactly as a fresh context that
uploaded the moved buffers, on the accel tree in 8 layouts and in 1 and on the
reference's own tree, with and without pad slots (leaf_align).

The scenes and deformations are tests/refit_ref.py's (the CPU side checks them
in tests/test_refit_ref.py).  A deformation that pulls apart two triangles the
accel build merged as byte-identical copies (a twin of the tie scenes whose
colour is its own complement) is refused on the accel tree, and must leave the
scene as it was."""
import functools

import numpy as np
import pytest

import query_ref as Q
import refit_ref as R
from conftest import has_gpu

pytestmark = pytest.mark.gpu

W, H, BOUNCES = 64, 48, 3
# (option accel, option leaf_align): leaf_align 1 puts pad slots into the reference's walk records, which
# are the walk's own on accel 0 and the fallback's beside the accel records
MODES = [(8, 2), (1, 1), (0, 2), (0, 1)]
ARRAYS = range(6)                         # rt_scene_copy_records' which


@pytest.fixture(scope="module")
def ctx():
    """(the context under test, a second one for fresh uploads of the moved buffers)"""
    if not has_gpu():
        pytest.skip("no GPU")
    import rtamd
    r, f = rtamd.Renderer((0,)), rtamd.Renderer((0,))
    yield r, f
    r.close()
    f.close()


def _upload(r, built, mode, refit):
    accel, align = mode
    r.set_option("accel_half", 0)
    r.set_option("accel_wide", 0)
    r.set_option("accel", accel)
    r.set_option("leaf_align", align)
    r.set_option("refit", refit)
    r.upload_scene(built)
    assert r.get_option("accel_used") == accel
    assert r.get_option("refit_used") == refit


def _frame(r, cam, stats=False):
    rgba, rad, st = r.render(cam, W, H, BOUNCES, radiance=True, stats=stats)
    return rgba, rad, st


def _same_frame(a, b, what):
    assert np.array_equal(a[0], b[0]), f"{what}: RGBA8 differs"
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), f"{what}: radiance differs"


@functools.lru_cache(maxsize=None)
def _case(name, kind):
    """The scene, and for every state of the deformation: the moved buffers,
    the oracle's frame and counts, the accel model's counts over the
    host-refitted records, the segment rays and their closest hits."""
    from oracle import oracle_lib as O
    from rtamd import _lib, build_buffers, refit_buffers
    tv, mats, seed, part, cam = R.scene(name)
    built = build_buffers(tv, mats, seed)
    recs = {nl: _lib.accel_records(built, nl) for nl in (1, 8)}
    states = []
    for moved in R.deform(kind, tv, part):
        new = refit_buffers(built, moved)
        args = (new.model_vertex_data, new.model_material_data, new.flat_bvh_data, cam.ubo_bytes(), W, H, BOUNCES)
        st = {"new": new, "ref": O.render(*args), "words": {}, "model": {}, "refused": False}
        for nl in (1, 8):
            rec, info = recs[nl]
            if R.broken_duplicates(rec, nl, new.model_vertex_data, new.flat_bvh_data):
                st["refused"] = True
                continue
            st["words"][nl] = _lib.accel_refit_records(rec, nl, new)
            st["model"][nl] = O.render_accel(*args, st["words"][nl], info)[2]
        if built.triangle_count:
            st["rays"] = Q.segment_rays(*args)
            st["hits"] = Q.closest_hits(new.model_vertex_data, new.flat_bvh_data, st["rays"])[0]
        states.append(st)
    return built, cam, recs, states


def _check_queries(r, fresh, st, cam, what):
    """Check 3: ray queries against the numpy reference, first-hit buffer and pick against the fresh context."""
    if "rays" in st:
        rays, want = st["rays"], st["hits"]
        got = r.query_rays(rays)
        assert got.tobytes() == want.tobytes(), f"{what}: closest hits differ"
        # any-hit as tests/test_gpu_query.py checks it: hit exactly where closest mode hits, every
        # reported hit a true intersection (the oracle's hit_triangle) no nearer than the closest
        any_ = r.query_rays(rays, any_hit=True)
        assert np.array_equal(any_["tri"] >= 0, want["tri"] >= 0), what
        miss = any_["tri"] < 0
        assert any_[miss].tobytes() == want[miss].tobytes(), what
        tm = np.full(len(rays), Q.T_MAX, np.float32)
        idx, ok, t, nrm = Q.oracle_triangle_hits(st["new"].model_vertex_data, rays, any_, tm)
        assert ok.all(), what
        assert np.array_equal(t.view(np.uint32), any_["t"][idx].view(np.uint32)), what
        assert np.array_equal(nrm.view(np.uint32), any_["normal"][idx].view(np.uint32)), what
        assert (any_["t"][idx] >= want["t"][idx]).all(), what
    assert r.render_hits(cam, W, H).tobytes() == fresh.render_hits(cam, W, H).tobytes(), f"{what}: first hits differ"
    for x, y in ((W // 2, H // 2), (3, H - 2)):
        assert r.pick(cam, W, H, x, y).tobytes() == fresh.pick(cam, W, H, x, y).tobytes(), f"{what}: pick differs"


@pytest.mark.parametrize("kind", R.DEFORMATIONS)
@pytest.mark.parametrize("name", R.SCENES)
def test_update_matches_fresh_upload(ctx, name, kind):
    """Checks 1-3 for every scene, deformation and mode."""
    from rtamd import RtError
    r, fresh = ctx
    built, cam, recs, states = _case(name, kind)
    for mode in MODES:
        accel = mode[0]
        what = f"{name} {kind} accel {accel} leaf_align {mode[1]}"
        _upload(r, built, mode, 1)
        if accel:                           # a fresh upload's accel records are rt_accel_records'
            assert np.array_equal(r.copy_records(0), recs[accel][0]), what
        _frame(r, cam)                      # a plain launch learns a tile order; the next one uses it
        last = _frame(r, cam)
        for st in states:
            if accel and st["refused"]:
                with pytest.raises(RtError, match="BAD_SCENE.*dropped"):
                    r.update_geometry(st["new"])
                _same_frame(_frame(r, cam), last, what + " after the refusal")
                continue
            r.update_geometry(st["new"])
            f1 = _frame(r, cam)
            f2 = _frame(r, cam, stats=True)
            last = f1
            ref = st["ref"]
            _same_frame(f1, ref, what + " (first frame)")
            _same_frame(f2, ref, what + " (second frame)")
            want = dict(ref[2]) if not accel else {**ref[2], "node_visits": st["model"][accel]["node_visits"],
                                                   "tri_tests": st["model"][accel]["tri_tests"]}
            for k in ("segments", "mat_reads", "node_visits", "tri_tests"):
                assert f2[2][k] == want[k], (what, k, f2[2][k], want[k])
            # 2. the records
            _upload(fresh, st["new"], mode, 0)
            if accel:
                assert np.array_equal(r.copy_records(0), st["words"][accel]), what + ": accel records"
            for which in ARRAYS:
                if accel and which == 0:
                    continue                # a fresh upload builds another tree
                a, b = r.copy_records(which), fresh.copy_records(which)
                assert np.array_equal(a, b), f"{what}: array {which} differs in {int((a != b).sum())} of {a.size} words"
            held = [w for w in ARRAYS if r.copy_records(w).size]
            if built.triangle_count:
                assert held == ([0, 1, 2] if accel else [0, 2, 3, 4, 5]), (what, held)
            _check_queries(r, fresh, st, cam, what)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["random1", "config2", "tris1", "tris5"])
def test_updates_in_a_row_and_identity(ctx, name, mode):
    """Check 4: translate, then jitter of the original, equal one fresh upload
    of the jittered buffers; the identity update leaves every array as it is."""
    r, fresh = ctx
    built, cam, _, states = _case(name, "identity")
    _upload(r, built, mode, 1)
    before = [r.copy_records(w) for w in ARRAYS]
    f0 = _frame(r, cam)
    r.update_geometry(states[0]["new"])
    for w in ARRAYS:
        assert np.array_equal(r.copy_records(w), before[w]), (name, mode, w)
    _same_frame(_frame(r, cam), f0, "identity")
    r.update_geometry(_case(name, "translate")[3][0]["new"])
    final = _case(name, "jitter")[3][0]
    r.update_geometry(final["new"])
    _upload(fresh, final["new"], mode, 0)
    _same_frame(_frame(r, cam), final["ref"], f"{name} {mode}")
    _same_frame(_frame(fresh, cam), final["ref"], f"{name} {mode} (fresh)")
    for w in ARRAYS:
        if mode[0] and w == 0:
            assert np.array_equal(r.copy_records(0), final["words"][mode[0]])
        else:
            assert np.array_equal(r.copy_records(w), fresh.copy_records(w)), (name, mode, w)


def _doubled(built):
    """(f, f + 1): two flattened copies of one input triangle."""
    src = np.asarray(built.flat_source)
    f = int(np.flatnonzero(src[1:] == src[:-1])[0])
    return f, f + 1


@pytest.mark.parametrize("mode", [(8, 2), (0, 1)])
def test_refusals(ctx, mode):
    """Check 5: every refusal names its status, and the scene stays as it was."""
    import rtamd
    from rtamd import BuiltCpuData, RtError
    r, _ = ctx
    built, cam, _, states = _case("config2", "translate")
    new = states[0]["new"]

    def with_(v=None, n=None):
        return BuiltCpuData(new.model_vertex_data if v is None else v, new.model_material_data,
                            new.flat_bvh_data if n is None else n, new.triangle_count, new.flat_source)

    def refused(status, match, data):
        before = _frame(r, cam)
        arrays = [r.copy_records(w) for w in ARRAYS]
        with pytest.raises(RtError, match=f"{status}.*{match}"):
            r.update_geometry(data)
        _same_frame(_frame(r, cam), before, f"after {status} {match}")
        for w in ARRAYS:
            assert np.array_equal(r.copy_records(w), arrays[w])

    _upload(r, built, mode, 0)
    refused("INVALID_ARG", "refit", new)
    if mode[0]:
        for fmt in ("half", "wide"):
            r.set_option(f"accel_{fmt}", 1)
            r.set_option("refit", 1)
            r.upload_scene(built)
            r.set_option(f"accel_{fmt}", 0)
            assert r.get_option(f"accel_{fmt}_used") == 1 and r.get_option("refit_used") == 0
            refused("INVALID_ARG", fmt, new)
    with rtamd.Renderer((0,)) as empty:
        empty.set_option("refit", 1)
        with pytest.raises(RtError, match="NO_SCENE"):
            empty.update_geometry(new)
    _upload(r, built, mode, 1)
    link = new.flat_bvh_data.copy()
    link[36] ^= 1                                     # the root's right child
    refused("BAD_SCENE", "outside its boxes", with_(n=link))
    pad = new.flat_bvh_data.copy()
    pad[48 + 12] = 1                                  # a pad byte between the boxes
    refused("BAD_SCENE", "outside its boxes", with_(n=pad))
    refused("BAD_SCENE", "bytes", with_(v=new.model_vertex_data[:-12]))
    refused("BAD_SCENE", "bytes", with_(n=new.flat_bvh_data[:-48]))
    nan = new.model_vertex_data.copy()
    nan[12 * 3 + 5] = np.nan
    refused("BAD_SCENE", "not finite", with_(v=nan))
    inf = new.flat_bvh_data.copy()
    inf.view(np.float32)[12 * 2 + 4] = np.inf
    refused("BAD_SCENE", "not finite", with_(n=inf))
    if mode[0]:                                       # one copy of a doubled triangle edited alone
        f, g = _doubled(built)
        alone = new.model_vertex_data.copy()
        alone[12 * g] += 0.5
        refused("BAD_SCENE", "dropped", with_(v=alone))
    # and after all of them the update itself still works
    r.update_geometry(new)
    _same_frame(_frame(r, cam), states[0]["ref"], "after the refusals")


@pytest.mark.parametrize("mode", [(8, 2), (0, 2)])
def test_sequences_start_over(ctx, mode):
    """Check 6: the temporal history and the samples sum are dropped."""
    from rtamd import RtError, configs
    r, fresh = ctx
    built, cam0, _, states = _case("config2", "translate")
    new = states[0]["new"]
    cam = configs.Camera(cam0.origin, cam0.look_at, cam0.v_up, cam0.vfov, cam0.aspect_ratio)
    _upload(r, built, mode, 1)
    _upload(fresh, new, mode, 0)
    for k in range(3):                                # a history of three frames, a sum of four samples
        cam.frame_count = cam.ubo.frame_count = k
        r.render_temporal(cam, W, H, BOUNCES, reset=(k == 0))
    cam.frame_count = cam.ubo.frame_count = 0
    r.render_samples(cam, W, H, BOUNCES, n_samples=4)
    r.update_geometry(new)
    cam.frame_count = cam.ubo.frame_count = 4
    with pytest.raises(RtError, match="INVALID_ARG.*holds 0 samples"):
        r.render_samples(cam, W, H, BOUNCES, n_samples=2)
    cam.frame_count = cam.ubo.frame_count = 3
    a = r.render_temporal(cam, W, H, BOUNCES, radiance=True)
    b = fresh.render_temporal(cam, W, H, BOUNCES, radiance=True)
    _same_frame(a, b, "the first temporal frame after the update")
    cam.frame_count = cam.ubo.frame_count = 0
    a = r.render_samples(cam, W, H, BOUNCES, n_samples=3, radiance=True)
    b = fresh.render_samples(cam, W, H, BOUNCES, n_samples=3, radiance=True)
    _same_frame(a, b, "the first samples call after the update")


@pytest.mark.parametrize("mode", MODES)
def test_refit_option_changes_nothing_else(ctx, mode):
    """Check 7: before any update a refit 1 scene is a refit 0 scene: frames,
    counters, walk_bytes, the records, and what a launch enqueues."""
    r, other = ctx
    for name in ("random2", "config2"):
        built, cam, _, _ = _case(name, "identity")
        _upload(r, built, mode, 1)
        _upload(other, built, mode, 0)
        assert r.get_option("refit_bytes") > 0 and other.get_option("refit_bytes") == 0
        assert r.walk_bytes() == other.walk_bytes()
        for k in ("leaf_align_used", "wave_tile_used", "coop_window_used"):
            assert r.get_option(k) == other.get_option(k)
        for w in ARRAYS:
            assert np.array_equal(r.copy_records(w), other.copy_records(w))
        pk = [x.get_option("plain_kernels") for x in (r, other)]
        frames = [[_frame(x, cam), _frame(x, cam), _frame(x, cam, stats=True)] for x in (r, other)]
        for a, b in zip(*frames):
            _same_frame(a, b, f"{name} {mode}")
        sa, sb = frames[0][2][2], frames[1][2][2]
        assert {k: v for k, v in sa.items() if k != "ms"} == {k: v for k, v in sb.items() if k != "ms"}
        assert r.get_option("plain_kernels") - pk[0] == other.get_option("plain_kernels") - pk[1]
