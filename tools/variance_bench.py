#!/usr/bin/env python3
"""Times of the variance-guided filter and of the accumulation that feeds it
(rt_denoise_variance_device, rt_temporal_moments_device; options denoise_kernel,
denoise_pass, variance_stage and temporal_tile) on three histories, beside
rt_denoise_history_device and rt_temporal_device in the same session.

On one config and one stream, the histories are accumulated on the GPU
(rt_render_tile_device with option new_sample, rt_render_hits_device,
rt_temporal_moments_device), each ending at the config's camera:

  n1       after 1 frame: every live pixel has n = 1, takes the 49-tap estimate
           and is filtered in every pass (the cost ceiling)
  static8  after 8 frames of an unmoved camera
  orbit8   after 8 frames of a camera orbiting 1 degree per frame

After warm-up, windows of --launches back-to-back launches each, timed with
device events, every kind alternated --rounds times.  Per history <h>:

  <h>.temporal / <h>.moments   the last frame's accumulation by rt_temporal_device
                               / rt_temporal_moments_device (n1: no previous frame)
  <h>.estimate                 the variance estimate alone (variance_stage 0)
  <h>.plain<i> / <h>.tiled0    pass i alone in the plain form / pass 0 in the tiled
  <h>.plain / .tiled / .auto   the whole filter, one form forced / as shipped
  <h>.adaptive                 rt_denoise_history_device as shipped on the same
                               history: the yardstick

A pass timed alone reads what a whole run of the filter on the same history left
in the workspace (enqueued before each window, outside the events).  Before
timing, the three dispatches' outputs and the two lane mappings' moments are
compared per history: they must be equal bit for bit.  Prints one JSON line and
appends it to --out (default profiles/variance/variance_bench.jsonl): per kind
the median, fastest and slowest window in ms per launch, per history the share
of hit pixels the estimate's 49-tap branch and each pass take, the faster form
at step 1 and the whole filter's time over the adaptive filter's.

Usage: python tools/variance_bench.py [--config 3] [--launches 100] [--rounds 5] [--iterations 4]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "3d-ray-tracer-vulkan_amd"), ROOT]

HISTORIES = ("n1", "static8", "orbit8")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=3)
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iterations", type=int, default=4)
    ap.add_argument("--accel", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "variance", "variance_bench.jsonl"))
    args = ap.parse_args()
    import rtamd  # first: sets GPU_MAX_HW_QUEUES before torch loads HIP
    import torch

    from rtamd import configs

    if not torch.cuda.is_available():
        sys.exit("variance_bench.py needs a GPU (there is no CPU path to time)")
    cfg = configs.get(args.config)
    built = cfg.build()
    W, H, B = cfg.width, cfg.height, cfg.max_bounces
    n_px = W * H
    vparams = rtamd.VarianceParams(iterations=args.iterations)
    dparams = rtamd.DenoiseParams(iterations=args.iterations)

    def orbit(deg):
        cam = cfg.camera()
        a = np.radians(deg)
        x, y, z = cam.origin
        cam.set_origin((x * np.cos(a) + z * np.sin(a), y, -x * np.sin(a) + z * np.cos(a)))
        return cam

    with rtamd.Renderer((0,)) as r:
        r.set_option("accel", args.accel)
        r.upload_scene(built)
        stream = torch.cuda.current_stream().cuda_stream
        new = lambda *shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device="cuda:0")   # noqa: E731
        d_ws, o_rgba, o_rad = new(2, n_px, 4), new(H, W, 4, dtype=torch.uint8), new(H, W, 3)
        t_hist, t_mom = new(n_px, 4), new(n_px, 2)            # the timed accumulations' outputs

        def accumulate(frames, step_deg):
            """After `frames` frames ending at the config's camera: the last frame's (camera, radiance, hit
            records, history, moments) and the previous frame's (camera, history, hit records, moments) or None."""
            prev = last = None
            r.set_option("new_sample", 1)
            try:
                for k in range(frames):
                    cam = orbit(-step_deg * (frames - 1 - k))
                    cam.ubo.frame_count = k
                    d_rad, d_hits, d_hist, d_mom = new(H, W, 3), new(n_px, 8), new(n_px, 4), new(n_px, 2)
                    r.render_tile_device(cam, W, H, B, 0, 0, W, H, None, d_rad.data_ptr(), stream)
                    r.render_hits_device(cam, W, H, 0, 0, W, H, d_hits.data_ptr(), stream)
                    r.temporal_moments_device(W, H, cam, d_rad.data_ptr(), d_hits.data_ptr(), d_hist.data_ptr(),
                                              d_mom.data_ptr(), prev[0] if prev else None,
                                              prev[1].data_ptr() if prev else None,
                                              prev[2].data_ptr() if prev else None,
                                              prev[3].data_ptr() if prev else None, None, None, None, stream)
                    torch.cuda.synchronize()
                    last = ((cam, d_rad, d_hits, d_hist, d_mom), prev)
                    prev = (cam, d_hist, d_hits, d_mom)
            finally:
                r.set_option("new_sample", 0)
            return last

        hists = {"n1": accumulate(1, 0.0), "static8": accumulate(8, 0.0), "orbit8": accumulate(8, 1.0)}

        def accum(h, moments, mapping=0):
            (cam, d_rad, d_hits, _, _), prev = hists[h]
            p = [prev[0], prev[1].data_ptr(), prev[2].data_ptr()] if prev else [None, None, None]

            def f():
                r.set_option("temporal_tile", mapping)
                if moments:
                    r.temporal_moments_device(W, H, cam, d_rad.data_ptr(), d_hits.data_ptr(), t_hist.data_ptr(),
                                              t_mom.data_ptr(), p[0], p[1], p[2], prev[3].data_ptr() if prev else None,
                                              None, None, None, stream)
                else:
                    r.temporal_device(W, H, cam, d_rad.data_ptr(), d_hits.data_ptr(), t_hist.data_ptr(), p[0], p[1],
                                      p[2], None, None, None, stream)
            return f

        def filt(h, form, only=-1, stage=-1, adaptive=False):
            _, _, d_hits, d_hist, d_mom = hists[h][0]

            def f():
                r.set_option("denoise_kernel", form)
                r.set_option("denoise_pass", only)
                r.set_option("variance_stage", stage)
                if adaptive:
                    r.denoise_history_device(W, H, d_hist.data_ptr(), d_hits.data_ptr(), d_ws.data_ptr(),
                                             o_rgba.data_ptr(), o_rad.data_ptr(), dparams, stream)
                else:
                    r.denoise_variance_device(W, H, d_hist.data_ptr(), d_mom.data_ptr(), d_hits.data_ptr(),
                                              d_ws.data_ptr(), o_rgba.data_ptr(), o_rad.data_ptr(), vparams, stream)
            return f

        same, shares, mean_n = {}, {}, {}
        for h in HISTORIES:
            outs = {}
            for name, form in (("auto", 0), ("plain", 1), ("tiled", 2)):
                filt(h, form)()
                torch.cuda.synchronize()
                outs[name] = (o_rgba.clone(), o_rad.clone())
            same[h] = all(bool((outs[k][0] == outs["plain"][0]).all()) and
                          bool((outs[k][1].view(torch.int32) == outs["plain"][1].view(torch.int32)).all())
                          for k in ("auto", "tiled"))
            moms = []
            for mapping in (1, 2):
                accum(h, True, mapping)()
                torch.cuda.synchronize()
                moms.append((t_hist.clone(), t_mom.clone()))
            accum(h, False)()
            torch.cuda.synchronize()
            same[h] = (same[h] and all(bool((a.view(torch.int32) == b.view(torch.int32)).all())
                                       for a, b in zip(moms[0], moms[1]))
                       and bool((t_hist.view(torch.int32) == moms[0][0].view(torch.int32)).all())
                       and bool((moms[0][0].view(torch.int32) == hists[h][0][3].view(torch.int32)).all())
                       and bool((moms[0][1].view(torch.int32) == hists[h][0][4].view(torch.int32)).all()))
            n = hists[h][0][3][:, 3].cpu().numpy()
            hit = hists[h][0][2][:, 1].cpu().numpy().view(np.int32) >= 0
            live = hit & (n >= 1)
            e = ((n.view(np.uint32) >> 23) & 0xFF).astype(np.int64) - 127
            k = np.where(live, np.maximum(0, args.iterations - e), 0)
            shares[h] = {"estimate_49_taps": round(float((live & (n < vparams.min_history))[hit].mean()), 4),
                         "filtered_per_pass": [round(float((k[hit] > i).mean()), 4) for i in range(args.iterations)]}
            mean_n[h] = round(float(n[hit].mean()), 3)

        kinds = {}
        for h in HISTORIES:
            kinds[f"{h}.temporal"] = (h, accum(h, False))
            kinds[f"{h}.moments"] = (h, accum(h, True))
            kinds[f"{h}.estimate"] = (h, filt(h, 0, stage=0))
            for name, form in (("auto", 0), ("plain", 1), ("tiled", 2)):
                kinds[f"{h}.{name}"] = (h, filt(h, form))
            kinds[f"{h}.adaptive"] = (h, filt(h, 0, adaptive=True))
            for i in range(args.iterations):
                kinds[f"{h}.plain{i}"] = (h, filt(h, 1, i))
            kinds[f"{h}.tiled0"] = (h, filt(h, 2, 0))
        for _, f in kinds.values():                           # warm-up: every shape of the timed windows
            for _ in range(10):
                f()
        torch.cuda.synchronize()
        ms = {k: [] for k in kinds}
        for _ in range(args.rounds):
            for k, (h, f) in kinds.items():
                filt(h, 0)()                                  # the workspace holds this history's records
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.launches):
                    f()
                e1.record()
                e1.synchronize()
                ms[k].append(e0.elapsed_time(e1) / args.launches)
        r.set_option("denoise_kernel", 0)
        r.set_option("denoise_pass", -1)
        r.set_option("variance_stage", -1)
        r.set_option("temporal_tile", 0)
        med = {k: statistics.median(v) for k, v in ms.items()}
        out = {"config": cfg.name, "accel_used": r.get_option("accel_used"), "width": W, "height": H,
               "max_bounces": B, "iterations": args.iterations, "launches": args.launches, "rounds": args.rounds,
               "ms": {k: {"median": round(med[k], 5), "min": round(min(v), 5), "max": round(max(v), 5)}
                      for k, v in ms.items()},
               "faster_form_at_step_1": {h: "tiled" if med[f"{h}.tiled0"] < med[f"{h}.plain0"] else "plain"
                                         for h in HISTORIES},
               "variance_over_adaptive": {h: round(med[f"{h}.auto"] / med[f"{h}.adaptive"], 3) for h in HISTORIES},
               "moments_over_temporal": {h: round(med[f"{h}.moments"] / med[f"{h}.temporal"], 3) for h in HISTORIES},
               "share_of_hit_pixels": shares, "mean_n_of_hit_pixels": mean_n, "forms_bit_identical": same}
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
