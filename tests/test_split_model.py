"""tools/split_model.py's packing function on small synthetic visit arrays
(no scene, no GPU): T[waves, lanes, bounces] node visits, 0 = the lane does not
walk in that bounce."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import split_model as S  # noqa: E402


def _random(waves=37, lanes=64, bounces=4, seed=5):
    """Paths that thin out bounce by bounce: a lane walks bounce b only if it
    walked bounce b - 1."""
    rng = np.random.default_rng(seed)
    T = rng.integers(1, 60, (waves, lanes, bounces))
    live = np.ones((waves, lanes), bool)
    for b in range(bounces):
        live &= rng.random((waves, lanes)) < (1.0, 0.7, 0.1, 0.5)[b]
        T[:, :, b] *= live
    return T


def _unsplit(T):
    return int(T.max(axis=1).sum())


def test_paths_are_conserved():
    T = _random()
    for split in (1, 2, 3):
        survivors = int((T[:, :, split] > 0).sum())
        visits = int(T[:, :, split:][T[:, :, split] > 0].sum())
        for nq, how in ((1, "modulo"), (5, "modulo"), (5, "blocks"), (64, "modulo"), (T.shape[0], "wave")):
            r = S.pack(T, split, S.deal(T.shape[0], nq, how))
            assert r["paths"] == survivors == int(r["entries"].sum()), (split, nq, how)
            assert r["visits"] == visits, (split, nq, how)
            assert (r["packs"] == (r["entries"] + 63) // 64).all()
            assert r["k1_steps"] == int(T[:, :, :split].max(axis=1).sum())


def test_one_full_queue_by_hand():
    """Four waves of 64 lanes, 16 survivors each with visits (wave + 1) x 10 at
    bounce 1 and, for the first 4 lanes of each wave, 7 at bounce 2: one queue
    holds 64 paths, exactly one full pack."""
    T = np.zeros((4, 64, 3), np.int64)
    T[:, :, 0] = 5
    T[2, 9, 0] = 11                                     # one long lane: wave 2 walks 11 steps at bounce 0
    for w in range(4):
        T[w, 8 * w:8 * w + 16, 1] = (w + 1) * 10
        T[w, 8 * w:8 * w + 4, 2] = 7
    r = S.pack(T, 1, S.deal(4, 1, "modulo"))
    assert r["paths"] == 64 and list(r["packs"]) == [1] and r["fill"] == 1.0
    assert r["k1_steps"] == 5 + 5 + 11 + 5
    assert r["k2_steps"] == 40 + 7                      # the pack's longest lane per bounce
    assert r["chain"] == 47
    # unsplit, every wave pays its own longest lane: 10 + 20 + 30 + 40 and 4 x 7
    assert _unsplit(T) == 26 + 100 + 28
    # two queues dealt modulo: waves 0, 2 and waves 1, 3; half-full packs
    r2 = S.pack(T, 1, S.deal(4, 2, "modulo"))
    assert list(r2["entries"]) == [32, 32] and r2["fill"] == 0.5
    assert r2["k2_steps"] == (30 + 7) + (40 + 7)


def test_a_queue_per_wave_is_the_unsplit_frame():
    T = _random(waves=23, seed=11)
    for split in (1, 2, 3):
        r = S.pack(T, split, S.deal(T.shape[0], T.shape[0], "wave"))
        assert r["k1_steps"] + r["k2_steps"] == _unsplit(T), split
        assert r["packs"].max() <= 1


def test_deal():
    assert list(S.deal(7, 3, "modulo")) == [0, 1, 2, 0, 1, 2, 0]
    assert list(S.deal(7, 3, "blocks")) == [0, 0, 0, 1, 1, 2, 2]
    assert list(S.deal(3, 3, "wave")) == [0, 1, 2]
