#!/usr/bin/env python3
"""Per-pass times of the history-adaptive filter's two kernel forms
(rt_denoise_history_device, options denoise_kernel and denoise_pass) on three
histories, beside rt_denoise_device's same passes in the same session.

On one config and one stream, the histories are accumulated on the GPU
(rt_render_tile_device with option new_sample, rt_render_hits_device,
rt_temporal_device), each ending at the config's camera:

  n1       after 1 frame: every live pixel has n = 1, every pass filters every
           hit pixel (the cost ceiling)
  static8  after 8 frames of an unmoved camera
  orbit8   after 8 frames of a camera orbiting 1 degree per frame

After warm-up, windows of --launches back-to-back launches each, timed with
device events, every kind alternated --rounds times.  Per history <h>:

  <h>.plain<i> / <h>.tiled<i>  pass i alone in the plain / the tiled form
  <h>.plain / .tiled / .auto   the whole filter, one form forced / as shipped
  old.*                        rt_denoise_device on the n1 frame's radiance: the
                               same kinds, the baseline the new passes are
                               compared with

A pass timed alone reads what a whole run of the same filter on the same
history left in the workspace (enqueued before each window, outside the events).
Before timing, the three dispatches' outputs are compared per history: they
must be equal bit for bit.  Prints one JSON line and appends it to --out
(default profiles/adaptive/adaptive_bench.jsonl): per kind the median, fastest
and slowest window in ms per launch, per history the share of hit pixels each
pass filters and the faster form per pass.

Usage: python tools/adaptive_bench.py [--config 3] [--launches 100] [--rounds 5] [--iterations 4]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "3d-ray-tracer-vulkan_amd"), ROOT]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=3)
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iterations", type=int, default=4)
    ap.add_argument("--accel", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adaptive", "adaptive_bench.jsonl"))
    args = ap.parse_args()
    import rtamd  # first: sets GPU_MAX_HW_QUEUES before torch loads HIP
    import torch

    from rtamd import configs

    if not torch.cuda.is_available():
        sys.exit("adaptive_bench.py needs a GPU (there is no CPU path to time)")
    cfg = configs.get(args.config)
    built = cfg.build()
    W, H, B = cfg.width, cfg.height, cfg.max_bounces
    n_px = W * H
    params = rtamd.DenoiseParams(iterations=args.iterations)

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

        def accumulate(frames, step_deg):
            """(history, hit records, radiance) on the device after `frames` frames ending at the config's camera."""
            prev = None
            r.set_option("new_sample", 1)
            try:
                for k in range(frames):
                    cam = orbit(-step_deg * (frames - 1 - k))
                    cam.ubo.frame_count = k
                    d_rad, d_hits, d_hist, t_rad = new(H, W, 3), new(n_px, 8), new(n_px, 4), new(H, W, 3)
                    r.render_tile_device(cam, W, H, B, 0, 0, W, H, None, d_rad.data_ptr(), stream)
                    r.render_hits_device(cam, W, H, 0, 0, W, H, d_hits.data_ptr(), stream)
                    r.temporal_device(W, H, cam, d_rad.data_ptr(), d_hits.data_ptr(), d_hist.data_ptr(),
                                      prev[0] if prev else None, prev[1].data_ptr() if prev else None,
                                      prev[2].data_ptr() if prev else None, None, t_rad.data_ptr(), None, stream)
                    torch.cuda.synchronize()
                    prev = (cam, d_hist, d_hits)
            finally:
                r.set_option("new_sample", 0)
            return d_hist, d_hits, t_rad

        hists = {"n1": accumulate(1, 0.0), "static8": accumulate(8, 0.0), "orbit8": accumulate(8, 1.0)}

        def filt(h, form, only=-1):
            d_hist, d_hits, t_rad = hists["n1" if h == "old" else h]

            def f():
                r.set_option("denoise_kernel", form)
                r.set_option("denoise_pass", only)
                if h == "old":
                    r.denoise_device(W, H, t_rad.data_ptr(), d_hits.data_ptr(), d_ws.data_ptr(), o_rgba.data_ptr(),
                                     o_rad.data_ptr(), params, stream)
                else:
                    r.denoise_history_device(W, H, d_hist.data_ptr(), d_hits.data_ptr(), d_ws.data_ptr(),
                                             o_rgba.data_ptr(), o_rad.data_ptr(), params, stream)
            return f

        same, filtered_share, mean_n = {}, {}, {}
        for h in ("old", "n1", "static8", "orbit8"):
            outs = {}
            for name, form in (("auto", 0), ("plain", 1), ("tiled", 2)):
                filt(h, form)()
                torch.cuda.synchronize()
                outs[name] = (o_rgba.clone(), o_rad.clone())
            same[h] = all(bool((outs[k][0] == outs["plain"][0]).all()) and
                          bool((outs[k][1].view(torch.int32) == outs["plain"][1].view(torch.int32)).all())
                          for k in ("auto", "tiled"))
            if h != "old":
                n = hists[h][0][:, 3].cpu().numpy()
                hit = hists[h][1][:, 1].cpu().numpy().view(np.int32) >= 0
                live = hit & (n >= 1)
                e = ((n.view(np.uint32) >> 23) & 0xFF).astype(np.int64) - 127
                k = np.where(live, np.maximum(0, args.iterations - e), 0)
                filtered_share[h] = [round(float((k[hit] > i).mean()), 4) for i in range(args.iterations)]
                mean_n[h] = round(float(n[hit].mean()), 3)
        filt("old", 0)()                                      # one sample everywhere: the fixed filter's bits
        torch.cuda.synchronize()
        old_out = o_rad.clone()
        filt("n1", 0)()
        torch.cuda.synchronize()
        n1_is_old = bool((o_rad.view(torch.int32) == old_out.view(torch.int32)).all())

        kinds = {}
        for h in ("old", "n1", "static8", "orbit8"):
            for name, form in (("auto", 0), ("plain", 1), ("tiled", 2)):
                kinds[f"{h}.{name}"] = (h, filt(h, form))
            for i in range(args.iterations):
                kinds[f"{h}.plain{i}"] = (h, filt(h, 1, i))
                kinds[f"{h}.tiled{i}"] = (h, filt(h, 2, i))
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
        med = {k: statistics.median(v) for k, v in ms.items()}
        faster = {h: ["tiled" if med[f"{h}.tiled{i}"] < med[f"{h}.plain{i}"] else "plain"
                      for i in range(args.iterations)] for h in ("old", "n1", "static8", "orbit8")}
        out = {"config": cfg.name, "accel_used": r.get_option("accel_used"), "width": W, "height": H,
               "max_bounces": B, "iterations": args.iterations, "launches": args.launches, "rounds": args.rounds,
               "ms": {k: {"median": round(med[k], 5), "min": round(min(v), 5), "max": round(max(v), 5)}
                      for k, v in ms.items()},
               "faster_form_per_pass": faster, "filtered_share_of_hit_pixels_per_pass": filtered_share,
               "mean_n_of_hit_pixels": mean_n, "forms_bit_identical": same, "n1_equals_rt_denoise_device": n1_is_old}
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
