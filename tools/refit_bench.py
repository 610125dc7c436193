#!/usr/bin/env python3
"""What rt_update_geometry costs against the upload it replaces, and what a
refitted tree costs the walk.  Not part of bench.py.

Default (needs a GPU): for each config (3 and 5), the light cube is translated
by (1.5, 0.25, -2) (tests/refit_ref.py's deformation (b)) and, in one process:

  update_wall_ms   host wall time of rt_update_geometry, the median of --calls
                   calls (>= 9) after one warm-up, alternating between the moved
                   and the original buffers so that every call moves something
  update_ms        its `ms`: the refit kernels' device time on device 0
  upload_wall_ms   rt_upload_scene of the same moved buffers (option refit 1, as
                   the scene under test; --uploads of them)
  ratio            upload_wall_ms / update_wall_ms
  refit_bytes      the extra device memory of option refit 1

and for config 3 the default render (plain launches of whole frames on one
stream, device events, windows of --frames frames) before and after an
identity update: the records are byte-identical, so the two must agree within
the windows' own spread.

--device (needs a GPU): rt_update_geometry_device beside the
path it replaces, for each config, in one process, the same translated cube,
the median of --calls calls after one warm-up of each, alternating between the
moved and the original triangles:

  old_wall_ms      host wall time of rt_refit_scene (rtamd.refit_buffers) followed
                   by rt_update_geometry from pageable memory; old_refit_scene_ms
                   and old_update_wall_ms are its two parts, old_update_ms the
                   update's `ms`
  device_wall_ms   host wall time of rt_update_geometry_device on a float64
                   tensor (and the source map) already resident on the device
  device_ms        its `ms`: the device time of all its kernels
  same_records     every device array after the last device update equals the
                   arrays after the host path's update of the same triangles

--upload (needs a GPU): for each config, the host wall time of --uploads calls of
rt_upload_scene after one warm-up, with option refit 0 and then 1, and the
library's build id (RTAMD_LIB_PATH chooses the library: profiles/scene_plan
alternates two of them).

--quality (CPU only): node visits per segment of the accel walk's CPU model
(oracle/rt_accel_model.c) over config 3 after deformations (b), (c) and (f),
on the refitted records and on a fresh rt_accel_records of the moved scene:
what a host weighs when it decides to rebuild instead of refitting.

Prints one JSON line per measurement and appends it to --out
(profiles/refit/refit_bench.jsonl).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "3d-ray-tracer-vulkan_amd"), ROOT, os.path.join(ROOT, "tests")]


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "a") as f:
        f.write(line + "\n")


def moved_cube(tv):
    """Deformation (b): the last instance (the light cube, 12 triangles) translated."""
    import numpy as np
    out = tv.reshape(-1, 3, 3).copy()
    out[-12:] += np.array([1.5, 0.25, -2.0])
    return out.reshape(-1, 9)


def bench_config(k, args):
    import numpy as np
    import rtamd
    import torch
    from rtamd import build_buffers, configs, refit_buffers, triangles_of
    cfg = configs.get(k)
    tv, mats = triangles_of(cfg.scene)
    t0 = time.perf_counter()
    built = build_buffers(tv, mats, 1)
    build_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    new = refit_buffers(built, moved_cube(tv))
    refit_scene_ms = (time.perf_counter() - t0) * 1e3
    W, H, B = cfg.width, cfg.height, cfg.max_bounces
    cam = cfg.camera()
    with rtamd.Renderer((0,)) as r:
        r.set_option("accel", args.accel)
        r.set_option("refit", 1)
        r.upload_scene(built)
        rec = {"what": "update_vs_upload", "config": k, "accel_used": r.get_option("accel_used"),
               "flat_triangles": built.triangle_count, "nodes": built.n_nodes, "walk_bytes": r.walk_bytes(),
               "refit_bytes": r.get_option("refit_bytes"), "build_buffers_s": round(build_s, 3),
               "rt_refit_scene_ms": round(refit_scene_ms, 3)}
        rec["refit_bytes_per_flat_triangle"] = round(rec["refit_bytes"] / built.triangle_count, 1)
        d_rgba = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda:0")
        stream = torch.cuda.current_stream().cuda_stream

        def frames(n):
            for _ in range(n):
                r.render_tile_device(cam, W, H, B, 0, 0, W, H, d_rgba.data_ptr(), None, stream)

        def windows(rounds):
            out = []
            for _ in range(rounds):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                frames(args.frames)
                e1.record()
                e1.synchronize()
                out.append(e0.elapsed_time(e1) / args.frames)
            return out

        if k == 3:
            frames(4)                       # the learning launch and its first uses
            torch.cuda.synchronize()
            before = windows(args.rounds)
            first = d_rgba.cpu().numpy().copy()
            r.update_geometry(built)        # the identity update
            after = windows(args.rounds)
            same = bool(np.array_equal(first, d_rgba.cpu().numpy()))
            emit({"what": "render_before_after_identity", "config": k, "frames_per_window": args.frames,
                  "before_ms": [round(x, 4) for x in before], "after_ms": [round(x, 4) for x in after],
                  "before_median_ms": round(statistics.median(before), 4),
                  "after_median_ms": round(statistics.median(after), 4), "same_frame": same}, args.out)
        r.update_geometry(new)              # warm-up
        wall, dev = [], []
        for i in range(args.calls):
            data = built if i % 2 == 0 else new
            t0 = time.perf_counter()
            ms = r.update_geometry(data, ms=True)
            wall.append((time.perf_counter() - t0) * 1e3)
            dev.append(ms)
        up = []
        for _ in range(args.uploads):
            t0 = time.perf_counter()
            r.upload_scene(new)
            up.append((time.perf_counter() - t0) * 1e3)
        rec.update({"calls": args.calls, "update_wall_ms": round(statistics.median(wall), 3),
                    "update_wall_min_max_ms": [round(min(wall), 3), round(max(wall), 3)],
                    "update_ms": round(statistics.median(dev), 4),
                    "update_ms_min_max": [round(min(dev), 4), round(max(dev), 4)],
                    "uploads": args.uploads, "upload_wall_ms": round(statistics.median(up), 1),
                    "upload_wall_min_max_ms": [round(min(up), 1), round(max(up), 1)]})
        rec["ratio"] = round(rec["upload_wall_ms"] / rec["update_wall_ms"], 1)
        emit(rec, args.out)


def bench_device(k, args):
    import numpy as np
    import rtamd
    import torch
    from rtamd import build_buffers, configs, refit_buffers, triangles_of
    cfg = configs.get(k)
    tv, mats = triangles_of(cfg.scene)
    tv = np.ascontiguousarray(tv, dtype=np.float64).reshape(-1, 9)
    built = build_buffers(tv, mats, 1)
    states = [moved_cube(tv), tv]
    with rtamd.Renderer((0,)) as r:
        r.set_option("accel", args.accel)
        r.set_option("refit", 1)
        r.upload_scene(built)
        plain_bytes = r.get_option("refit_bytes")
        r.set_option("refit_device", 1)
        r.upload_scene(built)
        assert r.get_option("refit_device_used") == 1
        rec = {"what": "device_vs_host_update", "config": k, "accel_used": r.get_option("accel_used"),
               "flat_triangles": built.triangle_count, "nodes": built.n_nodes, "input_triangles": len(tv),
               "refit_bytes": r.get_option("refit_bytes"), "refit_device_bytes": r.get_option("refit_bytes") - plain_bytes,
               "calls": args.calls}
        # the old path: rt_refit_scene on one host thread, then the update from pageable memory
        r.update_geometry(refit_buffers(built, states[0]))
        refit_ms, upd_ms, old_ms, old_dev = [], [], [], []
        for i in range(args.calls):
            t0 = time.perf_counter()
            new = refit_buffers(built, states[(i + 1) % 2])
            t1 = time.perf_counter()
            old_dev.append(r.update_geometry(new, ms=True))
            t2 = time.perf_counter()
            refit_ms.append((t1 - t0) * 1e3)
            upd_ms.append((t2 - t1) * 1e3)
            old_ms.append((t2 - t0) * 1e3)
        last = (args.calls) % 2                  # the state the last call left
        want = [r.copy_records(w) for w in range(6)]
        # the new path: the triangles and the source map already live on the device
        d_states = [torch.from_numpy(x).cuda() for x in states]
        d_src = torch.from_numpy(np.asarray(built.flat_source).astype(np.int32)).cuda()
        torch.cuda.synchronize()
        r.update_geometry_device(d_states[0], d_src)
        wall, dev = [], []
        for i in range(args.calls):
            t0 = time.perf_counter()
            ms = r.update_geometry_device(d_states[(i + 1) % 2], d_src, ms=True)
            wall.append((time.perf_counter() - t0) * 1e3)
            dev.append(ms)
        same = all(np.array_equal(r.copy_records(w), want[w]) for w in range(6))
        med = statistics.median

        def mm(x, nd=3):
            return [round(min(x), nd), round(max(x), nd)]
        rec.update({"old_wall_ms": round(med(old_ms), 3), "old_wall_min_max_ms": mm(old_ms),
                    "old_refit_scene_ms": round(med(refit_ms), 3), "old_update_wall_ms": round(med(upd_ms), 3),
                    "old_update_ms": round(med(old_dev), 4),
                    "device_wall_ms": round(med(wall), 3), "device_wall_min_max_ms": mm(wall),
                    "device_ms": round(med(dev), 4), "device_ms_min_max": mm(dev, 4),
                    "last_state": last, "same_records": bool(same)})
        rec["ratio"] = round(rec["old_wall_ms"] / rec["device_wall_ms"], 1)
        emit(rec, args.out)


def bench_upload(k, args):
    """--upload: the wall time of rt_upload_scene alone, with option refit 0 and 1."""
    import rtamd
    from rtamd import build_buffers, configs, triangles_of
    tv, mats = triangles_of(configs.get(k).scene)
    built = build_buffers(tv, mats, 1)
    with rtamd.Renderer((0,)) as r:
        r.set_option("accel", args.accel)
        for refit in (0, 1):
            r.set_option("refit", refit)
            r.upload_scene(built)               # warm-up
            up = []
            for _ in range(args.uploads):
                t0 = time.perf_counter()
                r.upload_scene(built)
                up.append((time.perf_counter() - t0) * 1e3)
            emit({"what": "upload_wall", "library": rtamd.lib().rt_build_id().decode(), "config": k,
                  "accel_used": r.get_option("accel_used"), "refit": refit, "flat_triangles": built.triangle_count,
                  "upload_ms": [round(x, 2) for x in up], "upload_median_ms": round(statistics.median(up), 2)}, args.out)


def quality(args):
    import numpy as np
    import refit_ref as R
    from oracle import oracle_lib as O
    from rtamd import _lib, build_buffers, configs, refit_buffers, triangles_of
    cfg = configs.get(3)
    tv, mats = triangles_of(cfg.scene)
    built = build_buffers(tv, mats, 1)
    cam = cfg.camera()
    W, H, B = cfg.width, cfg.height, cfg.max_bounces
    part = np.arange(len(tv) - 12, len(tv))
    rec, info = _lib.accel_records(built, 8)

    def visits(b, words, inf):
        c = O.render_accel(b.model_vertex_data, b.model_material_data, b.flat_bvh_data, cam.ubo_bytes(), W, H, B,
                           words, inf, row_step=args.row_step)[2]
        return round(c["node_visits"] / c["segments"], 3), round(c["tri_tests"] / c["segments"], 3)
    rows = [("original", tv.reshape(-1, 9))]
    rows += [(k, R.deform(k, tv, part)[0]) for k in ("translate", "jitter", "swap")]
    small = tv.reshape(-1, 3, 3) + np.random.default_rng(11).uniform(-1, 1, (len(tv), 3, 3)) * 0.05
    rows.append(("jitter_0.05_units", small.reshape(-1, 9)))
    for name, moved in rows:
        new = refit_buffers(built, moved)
        fresh_rec, fresh_info = _lib.accel_records(new, 8)
        a = visits(new, _lib.accel_refit_records(rec, 8, new), info)
        f = visits(new, fresh_rec, fresh_info)
        emit({"what": "tree_quality", "config": 3, "deformation": name, "row_step": args.row_step,
              "refit_visits_per_segment": a[0], "refit_tri_tests_per_segment": a[1],
              "fresh_visits_per_segment": f[0], "fresh_tri_tests_per_segment": f[1],
              "visits_ratio": round(a[0] / f[0], 2)}, args.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="3,5")
    ap.add_argument("--calls", type=int, default=11)
    ap.add_argument("--uploads", type=int, default=3)
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--accel", type=int, default=8)
    ap.add_argument("--quality", action="store_true")
    ap.add_argument("--device", action="store_true", help="time rt_update_geometry_device beside the host path")
    ap.add_argument("--upload", action="store_true", help="time rt_upload_scene alone, with option refit 0 and 1")
    ap.add_argument("--row-step", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refit", "refit_bench.jsonl"))
    args = ap.parse_args()
    if args.quality:
        return quality(args)
    if args.calls < 9:
        sys.exit("--calls must be at least 9")
    import rtamd  # noqa: F401  first: sets GPU_MAX_HW_QUEUES before torch loads HIP
    import torch
    if not torch.cuda.is_available():
        sys.exit("refit_bench.py needs a GPU for the timings (--quality runs without one)")
    for k in (int(x) for x in args.configs.split(",")):
        (bench_upload if args.upload else bench_device if args.device else bench_config)(k, args)


if __name__ == "__main__":
    main()
