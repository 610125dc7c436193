"""What packing the paths alive at a split bounce into full waves saves
(analysis aid for the split launch; not part of the product).
From the accel walk's CPU model (tools/solo_model.py profile: node visits per
pixel and bounce), replayed in lockstep wave tiles: kernel 1 walks the bounces
below the split in the frame's own tiles; the paths still walking at the split
bounce are appended, wave by wave in dispatch order and lane order, to the
queue their wave is dealt to, and kernel 2 walks every queue 64 paths to a
wave.  Prints per bounce the segments, live waves and lockstep steps, then for
each queue layout the steps of kernel 2, its lane fill, packs per queue, the
longest chain of steps one kernel-2 wave walks, and the fullest queue's
entries as a share of the launch's pixels (what a queue's capacity must hold).
Usage: split_model.py CONFIG [SPLIT [FRAMES]]   (default split 2, 4 frames per
launch: the frame repeated; config 5: rows 0-539)
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from solo_model import profile, wave_tiles  # noqa: E402

QUEUE_COUNTS = (1, 8, 32, 64, 256)


def deal(n_waves, nq, how):
    """The queue of each wave: by dispatch index modulo nq ("modulo"), in nq
    contiguous blocks ("blocks"), or one queue per wave ("wave")."""
    k = np.arange(n_waves)
    if how == "modulo":
        return k % nq
    if how == "blocks":
        return k * nq // max(n_waves, 1)
    if how == "wave":
        return k
    raise ValueError(how)


def pack(T, split, queue):
    """T[waves, lanes, B] visits (0 = the lane does not walk in that bounce),
    queue[waves] = the queue each wave appends to.  Returns a dict:
    k1_steps: lockstep steps of the bounces below the split;
    k2_steps: lockstep steps of the packed waves (64 paths each, per queue);
    paths, visits: the survivors and their node visits from the split on;
    packs: packs per queue (array over the queues that exist);
    entries: entries per queue; chain: the most steps one packed wave walks;
    fill: paths / (64 x packs)."""
    T = np.asarray(T, np.int64)
    queue = np.asarray(queue)
    n, lanes, B = T.shape
    k1 = int(T[:, :, :split].max(axis=1).sum()) if split > 0 else 0
    live = T[:, :, split] > 0                                    # [waves, lanes]
    w_idx, l_idx = np.nonzero(live)                              # dispatch order, then lane order
    tails = T[w_idx, l_idx, split:]                              # [paths, B - split]
    q_of = queue[w_idx]
    order = np.argsort(q_of, kind="stable")
    tails, q_of = tails[order], q_of[order]
    nq = int(queue.max()) + 1 if n else 0
    entries = np.bincount(q_of, minlength=nq)
    packs = (entries + 63) // 64
    k2, chain = 0, 0
    start = np.concatenate([[0], np.cumsum(entries)])
    for q in range(nq):
        t = tails[start[q]:start[q + 1]]
        if not len(t):
            continue
        pad = (-len(t)) % 64
        t = np.concatenate([t, np.zeros((pad, t.shape[1]), np.int64)])
        per_pack = t.reshape(-1, 64, t.shape[1]).max(axis=1).sum(axis=1)   # a pack's steps over its bounces
        k2 += int(per_pack.sum())
        chain = max(chain, int(per_pack.max()))
    n_paths = len(tails)
    return {"k1_steps": k1, "k2_steps": k2, "paths": n_paths, "visits": int(tails.sum()), "packs": packs,
            "entries": entries, "chain": chain, "fill": n_paths / (64.0 * packs.sum()) if packs.sum() else 1.0}


def bounce_table(T):
    rows = []
    for b in range(T.shape[2]):
        live = T[:, :, b] > 0
        rows.append((b, int(live.sum()), int(live.any(axis=1).sum()), int(T[:, :, b].max(axis=1).sum())))
    return rows


def main():
    k = int(sys.argv[1])
    split = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    frames = int(sys.argv[3]) if len(sys.argv) > 3 else 4
    T1 = wave_tiles(profile(k), 16, 4)
    print(f"config {k}: {T1.shape[0]} waves of 16x4 per frame, {T1.shape[2]} bounces, split at {split}, "
          f"{frames} frame(s) per launch")
    print("| bounce | segments | waves with a live lane | lockstep wave steps |")
    print("|---|---|---|---|")
    for b, seg, lw, st in bounce_table(T1):
        print(f"| {b} | {seg:,} | {lw:,} | {st:,} |")
    one = int(T1.max(axis=1).sum())
    if split >= T1.shape[2] or not (T1[:, :, split] > 0).any():
        print(f"no path walks at bounce {split}: nothing to pack")
        return
    late = int(T1[:, :, split:].max(axis=1).sum())
    lanes = (T1[:, :, split:] > 0).sum(axis=1)
    lw = lanes[lanes > 0]
    print(f"bounces >= {split}: {late:,} of {one:,} wave steps ({100.0 * late / one:.1f}%), "
          f"{lw.mean():.1f} lanes per live wave and bounce")
    T = np.concatenate([T1] * frames)
    n = T.shape[0]
    pixels = n * 64
    total1 = one * frames
    share = (T[:, :, split] > 0).sum() / pixels
    print(f"survivors: {100.0 * share:.2f}% of the launch's pixels")
    print("| queues | dealt | kernel-2 wave steps | lane fill | packs per queue (min-max) | longest chain | "
          "fullest queue, share of pixels / queues | total steps vs one kernel |")
    print("|---|---|---|---|---|---|---|---|")
    layouts = [(1, "modulo")] + [(q, how) for q in QUEUE_COUNTS[1:] for how in ("modulo", "blocks")]
    layouts.append((max(1, n // 64), "blocks"))                  # queues of 64 neighbouring tile waves
    for nq, how in layouts:
        r = pack(T, split, deal(n, nq, how))
        fullest = r["entries"].max() / (pixels / nq)
        print(f"| {nq} | {how} | {r['k2_steps']:,} | {r['fill']:.2f} | {r['packs'].min()}-{r['packs'].max()} | "
              f"{r['chain']} | {100.0 * fullest:.2f}% | {(r['k1_steps'] + r['k2_steps']) / total1:.3f}x |")
    r = pack(T, split, deal(n, n, "wave"))
    assert r["k1_steps"] + r["k2_steps"] == total1               # a queue per wave is the unsplit frame
    print(f"| {n} | wave | {r['k2_steps']:,} | {r['fill']:.2f} | - | {r['chain']} | - | 1.000x |")


if __name__ == "__main__":
    main()
