"""How many lockstep wave steps serve few lanes (analysis aid for option
solo_lanes; not part of the product).  From the accel
walk's CPU model (oracle/rt_accel_model.c profile: node visits per pixel and
bounce), replayed in lockstep wave tiles as tools/compact_model.py does: a
wave's steps in a bounce are the most visits of its lanes, and at step j the
lanes still walking are those with more than j visits.  Prints the wave
steps, lane visits and lane utilisation, the share of wave steps with at most
k lanes walking, and per bounce the one-lane steps and all steps.
Usage: solo_model.py CONFIG [TILE_W TILE_H]   (default 16 4; config 5: rows 0-539)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def wave_tiles(vis, tw, th):
    """vis[H, W, B] -> [tiles, tw * th, B]: whole tw x th wave tiles, raster order."""
    H, W, B = vis.shape
    v = vis[:H // th * th, :W // tw * tw]
    return v.reshape(H // th, th, W // tw, tw, B).transpose(0, 2, 1, 3, 4).reshape(-1, tw * th, B)


def steps_by_lanes(T):
    """T[tiles, lanes, B] visits (0 = the lane does not walk in that bounce) ->
    steps[lanes + 1, B]: steps[m, b] = the lockstep wave steps of bounce b
    during which exactly m lanes are still walking (steps[0] is all zero)."""
    T = np.asarray(T, np.int64)
    n, lanes, B = T.shape
    S = -np.sort(-T, axis=1)                                   # most visits first
    S = np.concatenate([S, np.zeros((n, 1, B), np.int64)], axis=1)
    out = np.zeros((lanes + 1, B), np.int64)
    out[1:] = (S[:, :-1] - S[:, 1:]).sum(axis=0)               # the m-th longest outlives the (m+1)-th by this
    return out


def shares(T):
    """The share of wave steps with at most k lanes walking, k = 1..lanes."""
    st = steps_by_lanes(T).sum(axis=1)
    total = st.sum()
    return np.cumsum(st[1:]) / total if total else np.ones(len(st) - 1)


def profile(k, nl=8):
    sys.path[:0] = [os.path.join(ROOT, "3d-ray-tracer-vulkan_amd"), ROOT]
    from rtamd import configs, _lib
    from oracle import oracle_lib as O
    cfg = configs.get(k)
    b = cfg.build()
    rec, info = _lib.accel_records(b, nl)
    tile = (0, 0, cfg.width, 540) if k == 5 else None
    prof = O.render_accel(b.model_vertex_data, b.model_material_data, b.flat_bvh_data, cfg.camera().ubo_bytes(),
                          cfg.width, cfg.height, cfg.max_bounces, rec, info, profile=True, tile=tile)[3]
    return (prof & 0xFFFFF).astype(np.int64)


def main():
    k = int(sys.argv[1])
    tw, th = (int(sys.argv[2]), int(sys.argv[3])) if len(sys.argv) > 3 else (16, 4)
    T = wave_tiles(profile(k), tw, th)
    st = steps_by_lanes(T)
    steps, visits = int(T.max(axis=1).sum()), int(T.sum())
    assert steps == int(st.sum())
    print(f"config {k} tiles {tw}x{th}: wave steps {steps} lane visits {visits} "
          f"lane utilisation {visits / (tw * th * steps):.3f}")
    sh = shares(T)
    print("share of wave steps with <= k lanes walking:",
          " ".join(f"k={j}: {sh[j - 1]:.3f}" for j in (1, 2, 3, 4, 8, 16, 32)))
    for bb in range(T.shape[2]):
        if st[:, bb].sum():
            print(f"  bounce {bb}: one-lane steps {int(st[1, bb])} of {int(st[:, bb].sum())}")


if __name__ == "__main__":
    main()
