#!/usr/bin/env python3
"""Ray-query throughput (rt_render_hits_device, rt_query_rays_device) against the
render it shares its walks with.

On one config and one stream, after warm-up, windows of --launches back-to-back
launches each, timed with device events, the four kinds alternated --rounds times:

  hits    rt_render_hits_device of the whole frame (the first-hit buffer)
  render  rt_render_tile_device of the same frame at max_bounces = 1, option
          heavy_first 0: the same walks, shading instead of the hit record
  copy    a device-to-device copy of 32 x n_rays bytes (what the hit records
          add to the 4 bytes per pixel the render writes)
  batch   rt_query_rays_device of one incoherent batch: the rays leaving the
          primary hits along their normals, in pixel order

Prints one JSON line and appends it to --out (default profiles/query/query_bench.jsonl):
per kind the median, fastest and slowest window in ms per launch, rays/s of hits
and batch, the render's window-to-window spread, and the speed bar's verdict:
hits <= render + copy + spread (medians).

Usage: python tools/query_bench.py [--config 3] [--launches 200] [--rounds 5] [--accel 8]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "3d-ray-tracer-vulkan_amd"), ROOT]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=3)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--accel", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "query", "query_bench.jsonl"))
    args = ap.parse_args()
    import rtamd  # first: sets GPU_MAX_HW_QUEUES before torch loads HIP
    import torch
    from rtamd import configs

    if not torch.cuda.is_available():
        sys.exit("query_bench.py needs a GPU (there is no CPU path to time)")
    cfg = configs.get(args.config)
    built = cfg.build()
    cam = cfg.camera()
    W, H = cfg.width, cfg.height
    n_px = W * H
    with rtamd.Renderer((0,)) as r:
        r.set_option("accel", args.accel)
        r.set_option("heavy_first", 0)
        r.upload_scene(built)
        stream = torch.cuda.current_stream().cuda_stream
        d_rgba = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda:0")
        d_hits = torch.empty((n_px, 8), dtype=torch.float32, device="cuda:0")
        d_copy = torch.empty_like(d_hits)

        def hits():
            r.render_hits_device(cam, W, H, 0, 0, W, H, d_hits.data_ptr(), stream)

        def render():
            r.render_tile_device(cam, W, H, 1, 0, 0, W, H, d_rgba.data_ptr(), None, stream)

        def copy():
            d_copy.copy_(d_hits)

        # the incoherent batch, built on the device from the first-hit buffer
        hits()
        torch.cuda.synchronize()
        tri = d_hits[:, 1].view(torch.int32)
        hit = tri >= 0
        n_batch = int(hit.sum())
        d_rays = torch.zeros((max(n_batch, 1), 8), dtype=torch.float32, device="cuda:0")
        d_rays[:n_batch, 0:3] = d_hits[hit, 5:8]             # origin = pos
        d_rays[:n_batch, 3] = 1.0e4                          # t_max = T_MAX
        d_rays[:n_batch, 4:7] = d_hits[hit, 2:5]             # dir = normal
        d_bhits = torch.empty((max(n_batch, 1), 8), dtype=torch.float32, device="cuda:0")

        def batch():
            r.query_rays_device(d_rays.data_ptr(), max(n_batch, 1), d_bhits.data_ptr(), stream=stream)

        # the two passes agree on what is hit: a 1-bounce hit is black, the sky never is
        render()
        torch.cuda.synchronize()
        black = (d_rgba[..., :3] == 0).all(-1).reshape(-1)
        same_mask = bool((black == hit).all())

        kinds = {"hits": hits, "render": render, "copy": copy, "batch": batch}
        for f in kinds.values():                              # warm-up: every shape of the timed windows
            for _ in range(20):
                f()
        torch.cuda.synchronize()
        ms = {k: [] for k in kinds}
        for _ in range(args.rounds):
            for k, f in kinds.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.launches):
                    f()
                e1.record()
                e1.synchronize()
                ms[k].append(e0.elapsed_time(e1) / args.launches)
        med = {k: statistics.median(v) for k, v in ms.items()}
        spread = max(ms["render"]) - min(ms["render"])
        out = {"config": cfg.name, "accel_used": r.get_option("accel_used"), "width": W, "height": H,
               "launches": args.launches, "rounds": args.rounds, "n_rays_hits": n_px, "n_rays_batch": n_batch,
               "ms": {k: {"median": round(med[k], 5), "min": round(min(v), 5), "max": round(max(v), 5)}
                      for k, v in ms.items()},
               "hits_mrays_s": round(n_px / med["hits"] / 1e3, 1),
               "batch_mrays_s": round(n_batch / med["batch"] / 1e3, 1),
               "render_spread_ms": round(spread, 5),
               "bar_ms": round(med["render"] + med["copy"] + spread, 5),
               "hits_within_bar": bool(med["hits"] <= med["render"] + med["copy"] + spread),
               "hit_mask_equals_render": same_mask}
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
