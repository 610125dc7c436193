#!/usr/bin/env python3
"""Per-pass times of the denoiser's two kernel forms (rt_denoise_device, options
denoise_kernel and denoise_pass) beside the render they follow.

On one config and one stream, after warm-up, windows of --launches back-to-back
launches each, timed with device events, every kind alternated --rounds times:

  plain<i> / tiled<i>  pass i alone (option denoise_pass i) in the plain / the
                       tiled form, for each pass of the --iterations-pass filter
  plain / tiled / auto the whole filter with one form forced, and as shipped
                       (per step size the form that measured faster)
  copy                 a device-to-device copy of a pass's compulsory bytes:
                       48 B read and 16 B written per pixel
  render               rt_render_tile_device of the frame (radiance only)
  hits                 rt_render_hits_device of the frame

Before timing, the three whole-filter outputs are compared: they must be equal
bit for bit.  Prints one JSON line and appends it to --out (default
profiles/denoise/denoise_bench.jsonl): per kind the median, fastest and slowest
window in ms per launch, which form was faster per pass, and whether the
shipped dispatch is no slower than the plain form on the whole filter.

Usage: python tools/denoise_bench.py [--config 3] [--launches 100] [--rounds 5] [--iterations 4]
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
    ap.add_argument("--iterations", type=int, default=4)
    ap.add_argument("--accel", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise", "denoise_bench.jsonl"))
    args = ap.parse_args()
    import rtamd  # first: sets GPU_MAX_HW_QUEUES before torch loads HIP
    import torch
    from rtamd import configs

    if not torch.cuda.is_available():
        sys.exit("denoise_bench.py needs a GPU (there is no CPU path to time)")
    cfg = configs.get(args.config)
    built = cfg.build()
    cam = cfg.camera()
    W, H, B = cfg.width, cfg.height, cfg.max_bounces
    n_px = W * H
    params = rtamd.DenoiseParams(iterations=args.iterations)
    with rtamd.Renderer((0,)) as r:
        r.set_option("accel", args.accel)
        r.upload_scene(built)
        stream = torch.cuda.current_stream().cuda_stream
        d_rad = torch.empty((H, W, 3), dtype=torch.float32, device="cuda:0")
        d_hits = torch.empty((n_px, 8), dtype=torch.float32, device="cuda:0")
        d_ws = torch.empty((2, n_px, 4), dtype=torch.float32, device="cuda:0")
        o_rgba = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda:0")
        o_rad = torch.empty((H, W, 3), dtype=torch.float32, device="cuda:0")
        c_src = torch.empty((n_px, 12), dtype=torch.float32, device="cuda:0")     # 48 B per pixel
        c_dst = torch.empty((n_px, 4), dtype=torch.float32, device="cuda:0")      # 16 B per pixel
        c_sink = torch.empty((n_px, 8), dtype=torch.float32, device="cuda:0")

        def render():
            r.render_tile_device(cam, W, H, B, 0, 0, W, H, None, d_rad.data_ptr(), stream)

        def hits():
            r.render_hits_device(cam, W, H, 0, 0, W, H, d_hits.data_ptr(), stream)

        def filt(form, only=-1):
            def f():
                r.set_option("denoise_kernel", form)
                r.set_option("denoise_pass", only)
                r.denoise_device(W, H, d_rad.data_ptr(), d_hits.data_ptr(), d_ws.data_ptr(), o_rgba.data_ptr(),
                                 o_rad.data_ptr(), params, stream)
            return f

        def copy():
            # 48 B read and 16 B written per pixel: 16 B copied, 32 B more read into a sink that stays in place
            c_dst.copy_(c_src[:, :4])
            c_sink.copy_(c_src[:, 4:])

        def copy64():
            # the same bytes as one contiguous copy: 32 B read + 32 B written per pixel
            c_sink.copy_(d_hits)

        for _ in range(3):                                    # the order is learned, the radiance is there
            render()
        hits()
        torch.cuda.synchronize()
        outs = {}
        for name, form in (("auto", 0), ("plain", 1), ("tiled", 2)):
            filt(form)()
            torch.cuda.synchronize()
            outs[name] = (o_rgba.clone(), o_rad.clone())
        same = all(bool((outs[k][0] == outs["plain"][0]).all()) and
                   bool((outs[k][1].view(torch.int32) == outs["plain"][1].view(torch.int32)).all())
                   for k in ("auto", "tiled"))
        changed = float((outs["auto"][1] != d_rad).any(-1).float().mean())

        kinds = {"render": render, "hits": hits, "copy": copy, "copy64": copy64,
                 "auto": filt(0), "plain": filt(1), "tiled": filt(2)}
        for i in range(args.iterations):
            kinds[f"plain{i}"] = filt(1, i)
            kinds[f"tiled{i}"] = filt(2, i)
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
        faster = ["tiled" if med[f"tiled{i}"] < med[f"plain{i}"] else "plain" for i in range(args.iterations)]
        out = {"config": cfg.name, "accel_used": r.get_option("accel_used"), "width": W, "height": H,
               "max_bounces": B, "iterations": args.iterations, "launches": args.launches, "rounds": args.rounds,
               "ms": {k: {"median": round(med[k], 5), "min": round(min(v), 5), "max": round(max(v), 5)}
                      for k, v in ms.items()},
               "faster_form_per_pass": faster,
               "pass_bytes": n_px * 64,
               "auto_no_slower_than_plain": bool(med["auto"] <= med["plain"] + (max(ms["plain"]) - min(ms["plain"]))),
               "forms_bit_identical": same, "pixels_changed_share": round(changed, 4)}
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
