"""The refit on the CPU: rt_refit_scene and
rt_accel_refit_records against their numpy restatement (tests/refit_ref.py),
against a fresh build of the moved triangles, and the frame of the refitted
records (oracle/rt_accel_model.c) against the reference-order oracle's."""
import ctypes as C

import numpy as np
import pytest

import refit_ref as R

W, H, BOUNCES = 64, 48, 4


def _built(name):
    from rtamd import build_buffers
    tv, mats, seed, part, cam = R.scene(name)
    return build_buffers(tv, mats, seed), tv, mats, seed, part, cam


def _validate(b):
    from rtamd import lib
    from rtamd._lib import check
    v, m, n = (np.ascontiguousarray(x) for x in (b.model_vertex_data, b.model_material_data, b.flat_bvh_data))
    check(lib().rt_scene_validate(v.ctypes.data, v.nbytes, m.ctypes.data, m.nbytes, n.ctypes.data, n.nbytes, None, None))


def _boxes(b):
    f = np.ascontiguousarray(b.flat_bvh_data, dtype=np.uint8).view(np.uint32).reshape(-1, 12)
    return f[:, [0, 1, 2, 4, 5, 6]]


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


@pytest.mark.parametrize("name", R.SCENES)
def test_identity_is_the_builders_bytes(name):
    """Check 1: unchanged triangles give rt_build_scene_map's bytes back, and
    (check 4) the identity refit leaves rt_accel_records' words alone."""
    from rtamd import _lib, refit_buffers
    built, tv, *_ = _built(name)
    again = refit_buffers(built, tv)
    assert _same_bits(again.model_vertex_data, built.model_vertex_data)
    assert _same_bits(again.flat_bvh_data, built.flat_bvh_data)
    for nl in (1, 8):
        rec, _ = _lib.accel_records(built, nl)
        assert np.array_equal(_lib.accel_refit_records(rec, nl, again), rec)
        assert np.array_equal(R.refit_records(rec, nl, again.model_vertex_data, again.flat_bvh_data), rec)


@pytest.mark.parametrize("kind", R.DEFORMATIONS)
@pytest.mark.parametrize("name", R.SCENES)
def test_deformed(name, kind):
    """Checks 2, 3 and 5 for every state a deformation goes through.

    One kind of state cannot be refitted and is checked for its refusal
    instead: the twins scenes hold pairs of coincident triangles, and where a
    twin's colour is its own complement (the ground's 0.5 grey) the pair is
    byte-identical, so the accel build kept one of the two.  The jitter moves
    the two apart; the records hold no slot for the second, and
    rt_accel_refit_records answers RT_ERR_BAD_SCENE as rt_update_geometry does
    for a dropped duplicate that is no longer one."""
    from oracle import oracle_lib as O
    from rtamd import RtError, _lib, build_buffers, refit_buffers
    built, tv, mats, seed, part, cam = _built(name)
    recs = {nl: _lib.accel_records(built, nl) for nl in (1, 8)}
    before = {nl: R.leaf_bits(recs[nl][0], nl) for nl in (1, 8)}
    states = R.deform(kind, tv, part)
    for step, moved in enumerate(states):
        new = refit_buffers(built, moved)
        # 2. the vertex records and leaf boxes of a fresh build, triangle by triangle; the numpy unions
        fresh = build_buffers(moved, mats, seed)
        if built.triangle_count:
            def by_source(b):
                data, count = R.node_fields(b.flat_bvh_data)
                leaves = np.flatnonzero(count < 0)
                flat = -(data[leaves] + 1)
                src = np.asarray(b.flat_source)[flat]
                v = np.ascontiguousarray(b.model_vertex_data).view(np.uint32).reshape(-1, 12)
                return {(int(s), tuple(v[f]), tuple(_boxes(b)[k])) for s, f, k in zip(src, flat, leaves)}
            assert by_source(new) == by_source(fresh)
            ref_v, ref_n = R.refit_scene(built, moved)
            assert _same_bits(new.model_vertex_data, ref_v)
            assert _same_bits(new.flat_bvh_data, ref_n)
        _validate(new)
        assert new.flat_source is built.flat_source and new.model_material_data is built.model_material_data
        # 3. the accel records, word for word; 5. their frame is the reference's of the new buffers
        args = (new.model_vertex_data, new.model_material_data, new.flat_bvh_data, cam.ubo_bytes(), W, H, BOUNCES)
        ref = O.render(*args)
        for nl in (1, 8):
            rec, info = recs[nl]
            if R.broken_duplicates(rec, nl, new.model_vertex_data, new.flat_bvh_data):
                # the build dropped a byte-identical copy (a twin in its own colour, 1 - 0.5) that the
                # deformation moved away from its keeper: not a scene these records can stand for
                with pytest.raises(RtError, match="BAD_SCENE.*dropped"):
                    _lib.accel_refit_records(rec, nl, new)
                continue
            got = _lib.accel_refit_records(rec, nl, new)
            want = R.refit_records(rec, nl, new.model_vertex_data, new.flat_bvh_data)
            assert np.array_equal(got, want), (name, kind, nl, np.flatnonzero(got != want)[:8])
            rgba, rad, cnt = O.render_accel(*args, got, info)
            assert np.array_equal(rgba, ref[0]) and np.array_equal(rad.view(np.uint32), ref[1].view(np.uint32))
            assert cnt["segments"] == ref[2]["segments"] and cnt["mat_reads"] == ref[2]["mat_reads"]
            if kind == "squash" and built.triangle_count:
                bits, root = R.leaf_bits(got, nl)
                if step == 0:               # needles everywhere: force bits go on
                    assert any(bits.values()) and root
                else:                       # and off again: none that was clear before is set now
                    assert not any(v and not before[nl][0][t] for t, v in bits.items())
                    assert root == before[nl][1]
                    assert np.array_equal(got, rec)


def test_refit_records_errors():
    """Check 6: every refusal of rt_accel_refit_records."""
    from rtamd import RtError, _lib, lib
    built = _built("config2")[0]
    rec, _ = _lib.accel_records(built, 8)
    v = np.ascontiguousarray(built.model_vertex_data)
    n = np.ascontiguousarray(built.flat_bvh_data)

    def call(words, n_words, nl, vb=v, nb=n, v_bytes=None, n_bytes=None):
        p = words.ctypes.data_as(C.POINTER(C.c_uint32)) if words is not None else None
        _lib.check(lib().rt_accel_refit_records(p, n_words, nl, vb.ctypes.data, vb.nbytes if v_bytes is None else v_bytes,
                                                nb.ctypes.data, nb.nbytes if n_bytes is None else n_bytes))
    w = rec.copy()
    call(w, w.size, 8)
    assert np.array_equal(w, rec)
    with pytest.raises(RtError, match="INVALID_ARG"):
        call(None, rec.size, 8)
    with pytest.raises(RtError, match="INVALID_ARG.*1 or 8"):
        call(rec.copy(), rec.size, 3)
    with pytest.raises(RtError, match="INVALID_ARG"):
        call(rec.copy(), rec.size - 8, 8)               # not 8 x layouts x slots + 16
    with pytest.raises(RtError, match="INVALID_ARG"):
        call(rec.copy(), 8, 8)
    with pytest.raises(RtError, match="BAD_SCENE.*multiple of 48"):
        call(rec.copy(), rec.size, 8, n_bytes=n.nbytes - 8)
    with pytest.raises(RtError, match="BAD_SCENE.*outside"):
        call(rec.copy(), rec.size, 8, v_bytes=48 * 3)   # leaves name triangles past the vertices
    # two leaves that name one triangle
    two = n.copy()
    f = two.view(np.int32).reshape(-1, 12)
    leaves = np.flatnonzero(f[:, 9] < 0)
    f[leaves[1], 8] = f[leaves[0], 8]
    with pytest.raises(RtError, match="BAD_SCENE.*both name triangle"):
        call(rec.copy(), rec.size, 8, nb=two)
    # words that are no records: a skip that leaves its layout, a triangle no leaf names, a lost leaf bit
    bad = rec.copy()
    bad[3] = (bad[3] & ~np.uint32(R.IDX)) | np.uint32(R.IDX)
    with pytest.raises(RtError, match="BAD_SCENE"):
        call(bad, bad.size, 8)
    bad = rec.copy()
    s = next(k for k in range(0, 64) if (int(bad[8 * k + 3]) >> 30) & 1)
    bad[8 * s + 3] = (bad[8 * s + 3] & ~np.uint32(R.IDX)) | np.uint32(built.triangle_count + 7)
    with pytest.raises(RtError, match="BAD_SCENE"):
        call(bad, bad.size, 8)
    bad = rec.copy()
    bad[8 * s + 3] &= ~np.uint32(1 << 30)
    with pytest.raises(RtError, match="BAD_SCENE"):
        call(bad, bad.size, 8)
    # a one-layout buffer read as 8 layouts cannot divide
    one, _ = _lib.accel_records(built, 1)
    with pytest.raises(RtError, match="INVALID_ARG|BAD_SCENE"):
        call(one.copy(), one.size, 8)


def test_refit_scene_errors():
    from rtamd import RtError, lib
    from rtamd._lib import check
    built, tv, *_ = _built("config2")
    src = np.ascontiguousarray(built.flat_source, dtype=np.uint32)
    v = np.empty(src.size * 12, np.float32)
    nodes = built.flat_bvh_data.copy()
    L = lib()

    def call(tvp, n_tris, srcp, n_flat, nb):
        check(L.rt_refit_scene(tvp, n_tris, srcp, n_flat, v.ctypes.data_as(C.POINTER(C.c_float)),
                               nb.ctypes.data_as(C.c_void_p), nb.size // 48))
    dp = tv.ctypes.data_as(C.POINTER(C.c_double))
    sp = src.ctypes.data_as(C.POINTER(C.c_uint32))
    call(dp, len(tv), sp, src.size, nodes)
    with pytest.raises(RtError, match="INVALID_ARG"):
        call(None, len(tv), sp, src.size, nodes)
    with pytest.raises(RtError, match="BAD_SCENE.*input triangle"):
        call(dp, 3, sp, src.size, nodes)                # source names triangles past the inputs
    with pytest.raises(RtError, match="BAD_SCENE.*outside"):
        call(dp, len(tv), sp, 4, nodes)                 # leaves name triangles past the flattened
    bad = nodes.copy()
    bad.view(np.int32).reshape(-1, 12)[0, 8] = 0        # a child that is not a later node
    with pytest.raises(RtError, match="BAD_SCENE.*later"):
        call(dp, len(tv), sp, src.size, bad)
