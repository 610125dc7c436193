#!/usr/bin/env python3
"""What rt_upload_scene puts on the device for the small refit scenes, as counts
and hashes: tests/golden/upload_records.json.

Run on a GPU with the library whose bytes are to be pinned (the file was written
with the library as it was before the upload's layout moved into
csrc/scene_plan.cpp):

  python tools/upload_records.py --write

uploads every scene of SCENES in every mode of MODES with option refit 0 and 1
and records, for every `which` of rt_scene_copy_records, the word count and the
64-bit FNV-1a hash of the words' little-endian bytes, and rt_scene_info's three
numbers.  tests/test_gpu_upload_records.py repeats the uploads on the tree under
test, and tests/test_scene_plan.py compares the same file with what the host-only
planner (tools/scene_plan_check.cpp) lays out, without a GPU.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (os.path.join(ROOT, "3d-ray-tracer-vulkan_amd"), ROOT, os.path.join(ROOT, "tests"))
                if p not in sys.path]

GOLDEN = os.path.join(ROOT, "tests", "golden", "upload_records.json")
# tests/refit_ref.py's: tris2 under leaf_align 1 is the smallest scene with a pad slot (its second leaf
# would start at slot 3), twins has the duplicates the accel build drops
SCENES = ("tris0", "tris1", "tris2", "tris3", "tris5", "twins", "grid", "random0", "config2")
MODES = ((8, 2), (1, 1), (0, 2), (0, 1))        # (option accel, option leaf_align): tests/test_gpu_refit.py MODES
ARRAYS = range(6)                               # rt_scene_copy_records' which


def fnv1a64(data: bytes) -> str:
    h = 0xCBF29CE484222325
    for b in data:
        h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return f"{h:016x}"


def key(name, mode, refit) -> str:
    return f"{name} accel={mode[0]} leaf_align={mode[1]} refit={refit}"


def cases():
    for name in SCENES:
        for mode in MODES:
            for refit in (0, 1):
                yield name, mode, refit


def built_scene(name):
    import refit_ref as R
    from rtamd import build_buffers
    tv, mats, seed, _, _ = R.scene(name)
    return build_buffers(tv, mats, seed)


def upload(r, built, mode, refit):
    """One upload on Renderer r; what the golden file holds for it."""
    import numpy as np
    r.set_option("accel_half", 0)
    r.set_option("accel_wide", 0)
    r.set_option("accel", mode[0])
    r.set_option("leaf_align", mode[1])
    r.set_option("refit", refit)
    r.upload_scene(built)
    info = r.scene_info()
    recs = []
    for which in ARRAYS:
        w = np.ascontiguousarray(r.copy_records(which), dtype="<u4")
        recs.append([int(w.size), fnv1a64(w.tobytes())])
    return {"info": [info["n_nodes"], info["n_tris"], info["max_depth"]], "records": recs}


def dump(doc, path):
    """One case per line."""
    with open(path, "w") as f:
        f.write('{"hash": %s,\n "library": %s,\n "cases": {\n' % (json.dumps(doc["hash"]), json.dumps(doc["library"])))
        f.write(",\n".join(f"  {json.dumps(k)}: {json.dumps(v)}" for k, v in doc["cases"].items()))
        f.write("\n }}\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--write", action="store_true", help=f"write {os.path.relpath(GOLDEN, ROOT)} (else compare with it)")
    args = ap.parse_args()
    import rtamd
    out = {}
    with rtamd.Renderer((0,)) as r:
        for name, mode, refit in cases():
            out[key(name, mode, refit)] = upload(r, built_scene(name), mode, refit)
    doc = {"hash": "64-bit FNV-1a of the words' little-endian bytes", "library": rtamd.lib().rt_build_id().decode(),
           "cases": out}
    if args.write:
        dump(doc, GOLDEN)
        print(f"wrote {len(out)} cases to {GOLDEN}")
        return 0
    with open(GOLDEN) as f:
        want = json.load(f)["cases"]
    bad = [k for k in want if out.get(k) != want[k]]
    print(f"{len(want) - len(bad)} of {len(want)} cases as recorded" + (f"; differ: {bad}" if bad else ""))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
