#!/usr/bin/env python3
"""Times of the temporal accumulation (rt_temporal_device, option temporal_tile)
beside the render it follows, its compulsory memory traffic, and the whole
rt_render_temporal pipeline.

On one config, camera orbiting 1 degree per frame about its look-at point, after
warm-up, windows of --launches back-to-back launches each, every kind alternated
--rounds times; device events on the launch stream, except the synchronous
whole-pipeline kinds, which are timed by the host clock around the calls:

  rows / tiles / auto   rt_temporal_device of one camera pair (frame 1 against
                        frame 0) with a wave on 64 pixels of a row / on a 16x4
                        tile, and as shipped
  first                 the same without history (null prev_*)
  copy_strided / copy   a device-to-device copy of the kernel's compulsory bytes
                        (124 B per pixel: 92 read, 32 written), as a strided
                        slice of wider records and as one contiguous copy
  render0 / render16    rt_render_tile_device of the orbit's frames (radiance
                        only) with option new_sample 0 and 1: the cost of the
                        extension kernels it selects
  hits                  rt_render_hits_device of a frame
  temporal / temporal_f2   rt_render_temporal whole (into host memory), without a
                        spatial filter and with a 2-pass one

Before timing, the three forms' outputs (history, radiance, RGBA8) are compared:
they must be equal bit for bit.  Prints one JSON line and appends it to --out
(default profiles/temporal/temporal_bench.jsonl): per kind the median, fastest
and slowest window in ms per launch, the faster form, and the kernel's time over
the copies'.

Usage: python tools/temporal_bench.py [--config 3] [--launches 100] [--rounds 5]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "3d-ray-tracer-vulkan_amd"), ROOT]

BYTES_PER_PIXEL = 124       # own 12 + 32, one coherent tap 48 (the other three hit the same lines), written 16 + 12 + 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=3)
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--accel", type=int, default=8)
    ap.add_argument("--orbit-frames", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal", "temporal_bench.jsonl"))
    args = ap.parse_args()
    import rtamd  # first: sets GPU_MAX_HW_QUEUES before torch loads HIP
    import torch
    from rtamd import configs

    if not torch.cuda.is_available():
        sys.exit("temporal_bench.py needs a GPU (there is no CPU path to time)")
    cfg = configs.get(args.config)
    built = cfg.build()
    base = cfg.camera()
    W, H, B = cfg.width, cfg.height, cfg.max_bounces
    n_px = W * H

    def orbit(k):
        a = math.radians(1.0 * k)
        ox, oy, oz = (base.origin[i] - base.look_at[i] for i in range(3))
        o = (base.look_at[0] + ox * math.cos(a) + oz * math.sin(a), base.look_at[1] + oy,
             base.look_at[2] - ox * math.sin(a) + oz * math.cos(a))
        cam = configs.Camera(o, base.look_at, base.v_up, base.vfov, base.aspect_ratio)
        cam.ubo.frame_count = k
        return cam

    cams = [orbit(k) for k in range(args.orbit_frames)]
    with rtamd.Renderer((0,)) as r:
        r.set_option("accel", args.accel)
        r.upload_scene(built)
        stream = torch.cuda.current_stream().cuda_stream
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device="cuda:0")   # noqa: E731
        d_rad = [f32(H, W, 3), f32(H, W, 3)]
        d_hits = [f32(n_px, 8), f32(n_px, 8)]
        d_hist = [f32(n_px, 4), f32(n_px, 4)]
        o_rgba = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda:0")
        o_rad = f32(H, W, 3)
        c_src = f32(n_px, 23)                       # 92 B per pixel
        c_dst = f32(n_px, 8)                        # 32 B per pixel
        c_a, c_b = torch.empty((2, n_px * 62), dtype=torch.uint8, device="cuda:0")
        state = {"k": 0}

        def render(new_sample):
            def f():
                r.set_option("new_sample", new_sample)
                k = state["k"] = (state["k"] + 1) % len(cams)
                r.render_tile_device(cams[k], W, H, B, 0, 0, W, H, None, d_rad[1].data_ptr(), stream)
            return f

        def hits():
            r.render_hits_device(cams[1], W, H, 0, 0, W, H, d_hits[1].data_ptr(), stream)

        def temporal(form, history=True):
            def f():
                r.set_option("temporal_tile", form)
                r.temporal_device(W, H, cams[1], d_rad[1].data_ptr(), d_hits[1].data_ptr(), d_hist[1].data_ptr(),
                                  cams[0] if history else None, d_hist[0].data_ptr() if history else None,
                                  d_hits[0].data_ptr() if history else None, o_rgba.data_ptr(), o_rad.data_ptr(), None,
                                  stream)
            return f

        def copy_strided():
            c_dst.copy_(c_src[:, :8])               # 32 B of every 92-B record: the lines of all 92 are fetched

        def copy():
            c_b.copy_(c_a)                          # 62 B read + 62 B written per pixel

        def whole(denoise):
            def f():
                k = state["k"] = (state["k"] + 1) % len(cams)
                r.render_temporal(cams[k], W, H, B, denoise=denoise)
            return f

        # frames 0 and 1 of the orbit as new samples, their hit buffers, frame 0's history
        r.set_option("new_sample", 1)
        for k in (0, 1):
            for _ in range(3):                                # the order is learned
                r.render_tile_device(cams[k], W, H, B, 0, 0, W, H, None, d_rad[k].data_ptr(), stream)
            r.render_hits_device(cams[k], W, H, 0, 0, W, H, d_hits[k].data_ptr(), stream)
        r.set_option("new_sample", 0)
        r.temporal_device(W, H, cams[0], d_rad[0].data_ptr(), d_hits[0].data_ptr(), d_hist[0].data_ptr(),
                          stream=stream)
        torch.cuda.synchronize()
        outs = {}
        for name, form in (("auto", 0), ("rows", 1), ("tiles", 2)):
            temporal(form)()
            torch.cuda.synchronize()
            outs[name] = (d_hist[1].clone(), o_rad.clone(), o_rgba.clone())
        same = all(bool((outs[k][0].view(torch.int32) == outs["rows"][0].view(torch.int32)).all()) and
                   bool((outs[k][1].view(torch.int32) == outs["rows"][1].view(torch.int32)).all()) and
                   bool((outs[k][2] == outs["rows"][2]).all()) for k in ("auto", "tiles"))
        n_out = outs["rows"][0][:, 3]
        hit_share = float((n_out > 0).float().mean())
        reuse_share = float((n_out > 1).float().sum() / max(1.0, float((n_out > 0).float().sum())))

        dev_kinds = {"rows": temporal(1), "tiles": temporal(2), "auto": temporal(0), "first": temporal(0, False),
                     "copy_strided": copy_strided, "copy": copy, "render0": render(0), "render16": render(1),
                     "hits": hits}
        host_kinds = {"temporal": whole(None), "temporal_f2": whole(rtamd.DenoiseParams(iterations=2))}
        # warm-up: every shape of the timed windows, and every camera of the orbit often enough that its
        # order is learned (a camera's first repeat learns: option reuse_order)
        for f in list(dev_kinds.values()) + list(host_kinds.values()):
            for _ in range(3 * len(cams) + 2):
                f()
        r.set_option("new_sample", 0)
        torch.cuda.synchronize()
        ms = {k: [] for k in list(dev_kinds) + list(host_kinds)}
        host_launches = max(1, args.launches // 4)
        for _ in range(args.rounds):
            for k, f in dev_kinds.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.launches):
                    f()
                e1.record()
                e1.synchronize()
                ms[k].append(e0.elapsed_time(e1) / args.launches)
            r.set_option("new_sample", 0)
            for k, f in host_kinds.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(host_launches):
                    f()
                ms[k].append((time.perf_counter() - t0) * 1e3 / host_launches)
        r.set_option("temporal_tile", 0)
        med = {k: statistics.median(v) for k, v in ms.items()}
        out = {"config": cfg.name, "accel_used": r.get_option("accel_used"), "width": W, "height": H,
               "max_bounces": B, "launches": args.launches, "host_launches": host_launches, "rounds": args.rounds,
               "orbit_frames": len(cams),
               "ms": {k: {"median": round(med[k], 5), "min": round(min(v), 5), "max": round(max(v), 5)}
                      for k, v in ms.items()},
               "faster_form": "tiles" if med["tiles"] < med["rows"] else "rows",
               "kernel_bytes": n_px * BYTES_PER_PIXEL,
               "auto_over_copy_strided": round(med["auto"] / med["copy_strided"], 3),
               "auto_over_copy": round(med["auto"] / med["copy"], 3),
               "render16_over_render0": round(med["render16"] / med["render0"], 3),
               "forms_bit_identical": same, "hit_pixels_share": round(hit_share, 4),
               "hit_pixels_reusing_history": round(reuse_share, 4)}
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
