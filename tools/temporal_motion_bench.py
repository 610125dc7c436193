#!/usr/bin/env python3
"""Times of the temporal accumulation across a geometry update
(rt_temporal_motion_device, option temporal_motion) beside the
unmoved-scene kernel, and of a whole rt_render_temporal frame after an update
beside one without.  Not part of bench.py.

On one config with the light cube (the scene's last 12 input triangles)
translated as tools/refit_bench.py does, a still camera, after warm-up, windows
of --launches back-to-back launches each, every kind alternated --rounds times;
device events on the launch stream (the kinds' order rotates from round to
round), except the whole-frame kinds, which are timed by the host clock around
the calls:

  static         rt_temporal_device of the frame after the update against the
                 frame before it (the unchanged kernel, which misses the move)
  parent_static  the same call into another build of the library (--parent-lib:
                 the parent commit's librtamd.so), in the same session
  null           rt_temporal_motion_device with NULL vertex buffers
  same           the MOTION kernel with the current records given twice: every
                 triangle unmoved, two record reads per hit pixel and no more
  cube           the MOTION kernel, light cube moved
  all            the MOTION kernel with every triangle translated: every hit
                 pixel takes the binary64 block
  frame_static   rt_render_temporal, no update since the last frame
  frame_update   rt_render_temporal after an rt_update_geometry (the update is
                 outside the timed region), and update_frame with it inside

Before timing, `null` is compared with `static` and `same` with `static` bit for
bit (an unmoved triangle is the static contract).  Prints one JSON line and
appends it to --out (default profiles/temporal_motion/temporal_motion_bench.jsonl).

Usage: python tools/temporal_motion_bench.py [--config 3] [--parent-lib PATH]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "3d-ray-tracer-vulkan_amd"), ROOT]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=3)
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--accel", type=int, default=8)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal_motion", "temporal_motion_bench.jsonl"))
    args = ap.parse_args()
    import numpy as np
    import rtamd  # first: sets GPU_MAX_HW_QUEUES before torch loads HIP
    import torch
    from rtamd import build_buffers, configs, refit_buffers, triangles_of

    if not torch.cuda.is_available():
        sys.exit("temporal_motion_bench.py needs a GPU (there is no CPU path to time)")
    cfg = configs.get(args.config)
    tv, mats = triangles_of(cfg.scene)
    built = build_buffers(tv, mats, 1)
    moved = tv.reshape(-1, 3, 3).copy()
    moved[-12:] += np.array([1.5, 0.25, -2.0])
    new = refit_buffers(built, moved.reshape(-1, 9))
    W, H, B = cfg.width, cfg.height, cfg.max_bounces
    n_px, n_tris = W * H, built.triangle_count
    cams = []
    for k in range(2):
        cam = cfg.camera()
        cam.ubo.frame_count = k
        cams.append(cam)

    parent = parent_ctx = None
    if args.parent_lib:
        parent = C.CDLL(os.path.abspath(args.parent_lib))
        vp = C.c_void_p
        parent.rt_create.argtypes = [C.POINTER(C.c_int), C.c_int, C.POINTER(vp)]
        parent.rt_temporal_device.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        parent.rt_destroy.argtypes = [vp]
        parent_ctx = vp()
        if parent.rt_create((C.c_int * 1)(0), 1, C.byref(parent_ctx)) != 0:
            sys.exit("the parent library's rt_create failed")

    with rtamd.Renderer((0,)) as r:
        r.set_option("accel", args.accel)
        r.set_option("refit", 1)
        r.set_option("temporal_motion", 1)
        r.upload_scene(built)
        stream = torch.cuda.current_stream().cuda_stream
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device="cuda:0")   # noqa: E731
        d_rad = [f32(H, W, 3), f32(H, W, 3)]
        d_hits = [f32(n_px, 8), f32(n_px, 8)]
        d_hist = [f32(n_px, 4), f32(n_px, 4)]
        o_rgba = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda:0")
        o_rad = f32(H, W, 3)
        v_prev = torch.from_numpy(np.ascontiguousarray(built.model_vertex_data, np.float32)).cuda()
        v_cur = torch.from_numpy(np.ascontiguousarray(new.model_vertex_data, np.float32)).cuda()
        v_all = v_cur.clone().view(-1, 4)
        v_all[:, :3] -= torch.tensor([0.5, 0.0, 0.25], device="cuda:0")          # every triangle's previous place
        v_all = v_all.view(-1)

        # frame 0 of the scene at rest, frame 1 after the update; frame 0's history
        r.set_option("new_sample", 1)
        for k in (0, 1):
            if k:
                r.update_geometry(new)
            for _ in range(3):                                                   # the order is learned
                r.render_tile_device(cams[k], W, H, B, 0, 0, W, H, None, d_rad[k].data_ptr(), stream)
            r.render_hits_device(cams[k], W, H, 0, 0, W, H, d_hits[k].data_ptr(), stream)
        r.set_option("new_sample", 0)
        r.temporal_device(W, H, cams[0], d_rad[0].data_ptr(), d_hits[0].data_ptr(), d_hist[0].data_ptr(), stream=stream)
        torch.cuda.synchronize()

        def static():
            r.temporal_device(W, H, cams[1], d_rad[1].data_ptr(), d_hits[1].data_ptr(), d_hist[1].data_ptr(), cams[0],
                              d_hist[0].data_ptr(), d_hits[0].data_ptr(), o_rgba.data_ptr(), o_rad.data_ptr(), None, stream)

        def parent_static():
            rc = parent.rt_temporal_device(parent_ctx, W, H, C.addressof(cams[1].ubo), d_rad[1].data_ptr(),
                                           d_hits[1].data_ptr(), C.addressof(cams[0].ubo), d_hist[0].data_ptr(),
                                           d_hits[0].data_ptr(), None, d_hist[1].data_ptr(), o_rgba.data_ptr(),
                                           o_rad.data_ptr(), stream, None)
            assert rc == 0, rc

        def motion(prev, cur=v_cur):
            def f():
                r.temporal_motion_device(W, H, cams[1], d_rad[1].data_ptr(), d_hits[1].data_ptr(), d_hist[1].data_ptr(),
                                         cams[0], d_hist[0].data_ptr(), d_hits[0].data_ptr(),
                                         cur.data_ptr() if prev is not None else None,
                                         prev.data_ptr() if prev is not None else None, n_tris, None, None,
                                         o_rgba.data_ptr(), o_rad.data_ptr(), None, stream)
            return f

        def snapshot(f):
            f()
            torch.cuda.synchronize()
            return d_hist[1].clone(), o_rad.clone(), o_rgba.clone()

        def equal(a, b):
            return all(bool((x.view(torch.uint8) == y.view(torch.uint8)).all()) for x, y in zip(a, b))

        s_static = snapshot(static)
        null_is_static = equal(snapshot(motion(None)), s_static)
        same_is_static = equal(snapshot(motion(v_cur)), s_static)
        parent_is_static = equal(snapshot(parent_static), s_static) if parent else None
        s_cube = snapshot(motion(v_prev))
        tri = d_hits[1][:, 1].contiguous().view(torch.int32)
        on_cube = tri >= 0
        flat_src = torch.from_numpy(np.asarray(built.flat_source, np.int64)).cuda()
        on_cube = on_cube & (flat_src[tri.clamp(min=0).long()] >= len(tv) - 12)
        n_cube = int(on_cube.sum())
        reuse = lambda s: float((s[0][:, 3][on_cube] > 1).float().mean()) if n_cube else None   # noqa: E731

        dev_kinds = {"static": static, "null": motion(None), "same": motion(v_cur), "cube": motion(v_prev),
                     "all": motion(v_all)}
        if parent:
            dev_kinds["parent_static"] = parent_static
        states = [built, new]
        frame = {"k": 1, "n": 2}

        def frame_static():
            cams[1].ubo.frame_count = frame["n"] = frame["n"] + 1
            r.render_temporal(cams[1], W, H, B)

        for f in dev_kinds.values():
            for _ in range(10):
                f()
        for _ in range(5):
            frame_static()
        torch.cuda.synchronize()
        ms = {k: [] for k in list(dev_kinds) + ["frame_static", "frame_update", "update_frame", "update"]}
        host_launches = max(1, args.launches // 4)
        used = []
        for rnd in range(args.rounds):
            order = list(dev_kinds.items())
            order = order[rnd % len(order):] + order[:rnd % len(order)]      # no kind keeps a place in the round
            for k, f in order:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.launches):
                    f()
                e1.record()
                e1.synchronize()
                ms[k].append(e0.elapsed_time(e1) / args.launches)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(host_launches):
                frame_static()
            ms["frame_static"].append((time.perf_counter() - t0) * 1e3 / host_launches)
            t_frame = t_update = 0.0
            for _ in range(host_launches):
                frame["k"] ^= 1
                t0 = time.perf_counter()
                r.update_geometry(states[frame["k"]])
                t1 = time.perf_counter()
                frame_static()
                t2 = time.perf_counter()
                used.append(r.get_option("temporal_motion_used"))
                t_update += t1 - t0
                t_frame += t2 - t1
            ms["frame_update"].append(t_frame * 1e3 / host_launches)
            ms["update"].append(t_update * 1e3 / host_launches)
            ms["update_frame"].append((t_frame + t_update) * 1e3 / host_launches)
        med = {k: statistics.median(v) for k, v in ms.items()}
        out = {"config": cfg.name, "accel_used": r.get_option("accel_used"), "width": W, "height": H, "max_bounces": B,
               "flat_triangles": n_tris, "launches": args.launches, "host_launches": host_launches, "rounds": args.rounds,
               "ms": {k: {"median": round(med[k], 5), "min": round(min(v), 5), "max": round(max(v), 5)}
                      for k, v in ms.items()},
               "cube_over_static": round(med["cube"] / med["static"], 3),
               "same_over_static": round(med["same"] / med["static"], 3),
               "all_over_static": round(med["all"] / med["static"], 3),
               "cube_over_parent_static": round(med["cube"] / med["parent_static"], 3) if parent else None,
               "static_over_parent_static": round(med["static"] / med["parent_static"], 3) if parent else None,
               "frame_update_over_frame_static": round(med["frame_update"] / med["frame_static"], 3),
               "null_is_static": null_is_static, "same_is_static": same_is_static, "parent_is_static": parent_is_static,
               "motion_used_after_every_update": all(u == 1 for u in used),
               "hit_pixels_share": round(float((tri >= 0).float().mean()), 4), "pixels_on_the_cube": n_cube,
               "cube_pixels_reusing_history": {"static": reuse(s_static), "motion": reuse(s_cube)}}
    if parent:
        parent.rt_destroy(parent_ctx)
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
