#!/usr/bin/env python3
"""Times of the filter on the illumination (rt_albedo_device,
rt_denoise_albedo_device) beside the colour filter's
(rt_denoise_device), with tools/denoise_bench.py's protocol.

On one config and one stream, after warm-up, windows of --launches back-to-back
launches each, timed with device events, every kind alternated --rounds times.
`c_` is the colour filter as shipped, `a_` the albedo form:

  albedo                      rt_albedo_device of the frame's hit buffer
  c_plain0 / a_plain0, c_tiled0 / a_tiled0
                              pass 0 of the 4-pass filter alone (option
                              denoise_pass), in each form: the pass that divides
  c_plain3 / a_plain3, c_tiled3 / a_tiled3
                              its last pass alone, in each form: the pass that
                              multiplies and writes the outputs
  c_auto4 / a_auto4           the whole 4-pass filter as dispatched by default
  c_auto6 / a_auto6           the whole 6-pass filter

Before timing, the albedo form's outputs in the three dispatches (option
denoise_kernel 0 / 1 / 2) are compared bit for bit, for 4 and for 6 passes, and
so are the colour filter's.  Prints one JSON line and appends it to --out
(default profiles/albedo/albedo_bench.jsonl): per kind the median, fastest and
slowest window in ms per launch, and per pair the albedo form's median as a
share of the colour filter's.

Usage: python tools/albedo_bench.py [--config 3] [--launches 100] [--rounds 5]
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
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--accel", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "albedo", "albedo_bench.jsonl"))
    args = ap.parse_args()
    import rtamd  # first: sets GPU_MAX_HW_QUEUES before torch loads HIP
    import torch
    from rtamd import configs

    if not torch.cuda.is_available():
        sys.exit("albedo_bench.py needs a GPU (there is no CPU path to time)")
    cfg = configs.get(args.config)
    built = cfg.build()
    cam = cfg.camera()
    W, H, B = cfg.width, cfg.height, cfg.max_bounces
    n_px = W * H
    params = {n: rtamd.DenoiseParams(iterations=n) for n in (4, 6)}
    with rtamd.Renderer((0,)) as r:
        r.set_option("accel", args.accel)
        r.upload_scene(built)
        stream = torch.cuda.current_stream().cuda_stream
        d_rad = torch.empty((H, W, 3), dtype=torch.float32, device="cuda:0")
        d_hits = torch.empty((n_px, 8), dtype=torch.float32, device="cuda:0")
        d_alb = torch.empty((n_px, 4), dtype=torch.float32, device="cuda:0")
        d_ws = torch.empty((2, n_px, 4), dtype=torch.float32, device="cuda:0")
        o_rgba = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda:0")
        o_rad = torch.empty((H, W, 3), dtype=torch.float32, device="cuda:0")

        def albedo():
            r.albedo_device(W, H, d_hits.data_ptr(), d_alb.data_ptr(), stream)

        def filt(alb, n, form=0, only=-1):
            def f():
                r.set_option("denoise_kernel", form)
                r.set_option("denoise_pass", only)
                r.denoise_device(W, H, d_rad.data_ptr(), d_hits.data_ptr(), d_ws.data_ptr(), o_rgba.data_ptr(),
                                 o_rad.data_ptr(), params[n], stream, d_albedo=d_alb.data_ptr() if alb else 0)
            return f

        for _ in range(3):                                    # the order is learned, the radiance is there
            r.render_tile_device(cam, W, H, B, 0, 0, W, H, None, d_rad.data_ptr(), stream)
        r.render_hits_device(cam, W, H, 0, 0, W, H, d_hits.data_ptr(), stream)
        albedo()
        torch.cuda.synchronize()
        same, outs = True, {}
        for alb in (False, True):
            for n in (4, 6):
                for form in (0, 1, 2):
                    filt(alb, n, form)()
                    torch.cuda.synchronize()
                    outs[form] = (o_rgba.clone(), o_rad.clone())
                same = same and all(bool((outs[k][0] == outs[1][0]).all()) and
                                    bool((outs[k][1].view(torch.int32) == outs[1][1].view(torch.int32)).all())
                                    for k in (0, 2))
                if n == 4:
                    outs["a" if alb else "c"] = outs[0][1]
        differ = float((outs["a"] != outs["c"]).any(-1).float().mean())
        divided = float((d_alb[:, :3] != 1).any(-1).float().mean())     # pixels with some d != 1

        kinds = {"albedo": albedo}
        for tag, alb in (("c", False), ("a", True)):
            for i in (0, 3):
                kinds[f"{tag}_plain{i}"] = filt(alb, 4, 1, i)
                kinds[f"{tag}_tiled{i}"] = filt(alb, 4, 2, i)
            kinds[f"{tag}_auto4"] = filt(alb, 4)
            kinds[f"{tag}_auto6"] = filt(alb, 6)
        for f in kinds.values():                              # warm-up: every shape of the timed windows
            for _ in range(10):
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
        r.set_option("denoise_kernel", 0)
        r.set_option("denoise_pass", -1)
        med = {k: statistics.median(v) for k, v in ms.items()}
        out = {"config": cfg.name, "accel_used": r.get_option("accel_used"), "width": W, "height": H,
               "max_bounces": B, "launches": args.launches, "rounds": args.rounds,
               "ms": {k: {"median": round(med[k], 5), "min": round(min(v), 5), "max": round(max(v), 5)}
                      for k, v in ms.items()},
               "albedo_share_of_colour": {k[2:]: round(med["a_" + k[2:]] / med[k], 4) for k in med if k.startswith("c_")},
               "pass_bytes": n_px * 64, "albedo_bytes_per_pass": n_px * 16,
               "forms_bit_identical": same, "pixels_differing_from_colour_share": round(differ, 4),
               "pixels_divided_share": round(divided, 4)}
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
