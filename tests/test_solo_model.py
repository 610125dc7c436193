"""tools/solo_model.py: the share of lockstep wave steps that
serve at most k lanes, on a hand-made visits array and on a small profile of
the accel walk's CPU model."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import solo_model as S  # noqa: E402


def test_shares_by_hand():
    # one wave of 4 lanes, two bounces.  Bounce 0: visits 5, 3, 3, 0 -> steps
    # 0-2 have 3 lanes walking, steps 3-4 one lane.  Bounce 1: 2, 0, 0, 7 ->
    # steps 0-1 two lanes, steps 2-6 one lane.
    T = np.array([[[5, 2], [3, 0], [3, 0], [0, 7]]])
    st = S.steps_by_lanes(T)
    assert st.shape == (5, 2)
    assert st[:, 0].tolist() == [0, 2, 0, 3, 0]
    assert st[:, 1].tolist() == [0, 5, 2, 0, 0]
    assert int(st.sum()) == 5 + 7                               # the wave's steps: its longest lane's, per bounce
    sh = S.shares(T)
    assert np.allclose(sh, [7 / 12, 9 / 12, 1.0, 1.0])
    # a second wave whose 4 lanes all walk 6 steps: 6 more steps, none below 4 lanes
    T2 = np.concatenate([T, np.array([[[6, 0]] * 4])])
    assert np.allclose(S.shares(T2), [7 / 18, 9 / 18, 12 / 18, 1.0])
    # nothing walks at all
    assert S.shares(np.zeros((2, 4, 1), int)).tolist() == [1.0] * 4


def test_wave_tiles_order():
    vis = np.arange(8 * 32).reshape(8, 32, 1)
    T = S.wave_tiles(vis, 16, 4)
    assert T.shape == (4, 64, 1)
    assert T[1, :, 0].tolist() == [y * 32 + x for y in range(4) for x in range(16, 32)]
    assert T[2, 0, 0] == 4 * 32
    assert S.wave_tiles(np.zeros((9, 33, 2)), 16, 4).shape == (4, 64, 2)   # partial tiles are left out


def test_shares_on_config2_profile():
    """A 64 x 36 frame of config 2's scene: the shares are non-decreasing and
    end at 1, and the steps add up to each wave's longest lane."""
    sys.path[:0] = [os.path.join(ROOT, "3d-ray-tracer-vulkan_amd"), ROOT]
    from rtamd import configs, _lib
    from oracle import oracle_lib as O
    cfg = configs.config2()
    b = cfg.build()
    w, h = 64, 36
    cam = configs.Camera.default(w, h)
    rec, info = _lib.accel_records(b, 8)
    prof = O.render_accel(b.model_vertex_data, b.model_material_data, b.flat_bvh_data, cam.ubo_bytes(), w, h,
                          cfg.max_bounces, rec, info, profile=True)[3]
    T = S.wave_tiles((prof & 0xFFFFF).astype(np.int64), 16, 4)
    assert T.shape[:2] == (36, 64) and T.sum() > 0
    sh = S.shares(T)
    assert len(sh) == 64 and (np.diff(sh) >= 0).all() and sh[0] > 0 and abs(sh[-1] - 1.0) < 1e-12
    assert int(S.steps_by_lanes(T).sum()) == int(T.max(axis=1).sum())
