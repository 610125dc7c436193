#!/usr/bin/env python3
"""Device time per sample of rt_render_samples_device (option sample_frames 1,
2, 4, 8 and 16), of its resolve and its trace launches alone
(option samples_stage), and of the way to the same image without it: N
rt_render_tile_device launches with extensions 4 on one stream.

One config, one stream, N samples per call into a workspace of 16 frames.
Before timing, every kind's RGBA8 and radiance are compared with the serial
bit-4 frames': they must be equal bit for bit.  After warm-up (every kind's
launches, so every launch shape has its learned order), windows of --calls
back-to-back calls each, timed with device events, every kind alternated
--rounds times:

  sf<k>        a whole call at sample_frames k
  trace<k>     its trace launches alone (samples_stage 0)
  resolve<k>   its resolves alone (samples_stage 1; on what the workspace holds)
  scalar4      a whole call at sample_frames 4 with the scalar resolve
  bit4         N launches with extensions 4, frame_count 0 .. N - 1

Prints one JSON line and appends it to --out (default
profiles/samples/samples_bench.jsonl): per kind the median, fastest and slowest
window in ms per SAMPLE, the fastest sample_frames, and each kind's time over
bit4's.

Usage: python tools/samples_bench.py [--config 3] [--samples 16] [--calls 10] [--rounds 5]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "3d-ray-tracer-vulkan_amd"), ROOT]

FRAMES = (1, 2, 4, 8, 16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=3)
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--accel", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "samples", "samples_bench.jsonl"))
    args = ap.parse_args()
    import rtamd  # first: sets GPU_MAX_HW_QUEUES before torch loads HIP
    import torch

    from rtamd import configs

    if not torch.cuda.is_available():
        sys.exit("samples_bench.py needs a GPU (there is no CPU path to time)")
    cfg = configs.get(args.config)
    built = cfg.build()
    W, H, B, N = cfg.width, cfg.height, cfg.max_bounces, args.samples
    n_px = W * H

    with rtamd.Renderer((0,)) as r:
        r.set_option("accel", args.accel)
        r.upload_scene(built)
        stream = torch.cuda.current_stream().cuda_stream
        new = lambda *shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device="cuda:0")   # noqa: E731
        ws_bytes = r.samples_workspace_bytes(W, H, 16)
        d_ws, d_sum = new(ws_bytes // 4), new(n_px * 3)
        o_rgba, o_rad = new(H, W, 4, dtype=torch.uint8), new(H, W, 3)
        cams = []
        for k in range(N):
            cam = cfg.camera()
            cam.ubo.frame_count = k
            cams.append(cam)

        def samples(frames, stage=-1, form=0):
            def f():
                r.set_option("sample_frames", frames)
                r.set_option("samples_stage", stage)
                r.set_option("samples_kernel", form)
                r.render_samples_device(cams[0], W, H, B, N, d_ws.data_ptr(), ws_bytes, d_sum.data_ptr(),
                                        o_rgba.data_ptr(), o_rad.data_ptr(), stream)
            return f

        def bit4():
            r.set_option("extensions", 4)
            for cam in cams:
                r.render_tile_device(cam, W, H, B, 0, 0, W, H, o_rgba.data_ptr(), o_rad.data_ptr(), stream)
            r.set_option("extensions", 0)

        kinds = {"bit4": bit4}
        for k in FRAMES:
            kinds[f"sf{k}"] = samples(k)
            kinds[f"trace{k}"] = samples(k, stage=0)
            kinds[f"resolve{k}"] = samples(k, stage=1)
        kinds["scalar4"] = samples(4, form=1)

        def outputs(f):
            f()
            torch.cuda.synchronize()
            return o_rgba.clone(), o_rad.clone()

        want = outputs(bit4)
        same = {}
        for name in [f"sf{k}" for k in FRAMES] + ["scalar4"]:
            got = outputs(kinds[name])
            same[name] = bool((got[0] == want[0]).all()) and \
                bool((got[1].view(torch.int32) == want[1].view(torch.int32)).all())
        for f in kinds.values():                              # warm-up: every shape of the timed windows, three times
            for _ in range(3):                                #   (a launch shape's first plain launch learns its order)
                f()
        torch.cuda.synchronize()
        ms = {k: [] for k in kinds}
        for _ in range(args.rounds):
            for k, f in kinds.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.calls):
                    f()
                e1.record()
                e1.synchronize()
                ms[k].append(e0.elapsed_time(e1) / (args.calls * N))
        r.set_option("sample_frames", 16)
        r.set_option("samples_stage", -1)
        r.set_option("samples_kernel", 0)
        med = {k: statistics.median(v) for k, v in ms.items()}
        best = min(FRAMES, key=lambda k: med[f"sf{k}"])
        out = {"config": cfg.name, "accel_used": r.get_option("accel_used"), "width": W, "height": H,
               "max_bounces": B, "samples": N, "calls": args.calls, "rounds": args.rounds,
               "ms_per_sample": {k: {"median": round(med[k], 5), "min": round(min(v), 5), "max": round(max(v), 5)}
                                 for k, v in ms.items()},
               "fastest_sample_frames": best,
               "over_bit4": {k: round(med[k] / med["bit4"], 3) for k in ms if k != "bit4"},
               "equal_to_bit4": same}
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
