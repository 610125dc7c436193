"""The host-only scene plan (csrc/scene_plan.cpp: everything rt_upload_scene
puts on a device, laid out without one) through tools/scene_plan_check.cpp,
compiled with plain g++: the plan's arrays must be, word count for word count
and hash for hash, what the library put on the device before the layout moved
out of the runtime (tests/golden/upload_records.json, which
tests/test_gpu_upload_records.py checks on the GPU), and the program itself
checks the layout's invariants on every plan: slots, alignment, pad slots and
their bits, skips, the refit blob's sections and tables, and the refusals."""
import importlib.util
import json
import os
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("upload_records", os.path.join(ROOT, "tools", "upload_records.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def planned(tmp_path_factory):
    """The program's output over the golden file's scenes: {case: (info, records)}, and its last line."""
    U = _tool()
    tmp = tmp_path_factory.mktemp("scene_plan")
    exe = tmp / "scene_plan_check"
    pkg = os.path.join(ROOT, "3d-ray-tracer-vulkan_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-pthread", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(pkg, "csrc"), os.path.join(ROOT, "tools", "scene_plan_check.cpp"),
                    os.path.join(pkg, "csrc", "scene_plan.cpp"), os.path.join(pkg, "csrc", "accel_build.cpp"),
                    "-o", str(exe)], check=True)
    args = []
    for name in U.SCENES:
        built = U.built_scene(name)
        bufs = [np.ascontiguousarray(built.model_vertex_data, dtype=np.float32).tobytes(),
                np.ascontiguousarray(built.model_material_data, dtype=np.float32).tobytes(),
                np.ascontiguousarray(built.flat_bvh_data, dtype=np.uint8).tobytes()]
        path = tmp / f"{name}.scene"
        path.write_bytes(struct.pack("<3Q", *(len(b) for b in bufs)) + b"".join(bufs))
        args.append(f"{name}={path}")
    run = subprocess.run([str(exe)] + args, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr + run.stdout
    lines = run.stdout.splitlines()
    out = {}
    for line in lines[:-1]:
        case, info, recs = line.split("\t")
        r = recs.split()
        out[case] = {"info": [int(x) for x in info.split()], "records": [[int(r[2 * w]), r[2 * w + 1]] for w in range(6)]}
    return U, out, lines[-1]


def test_invariants_and_refusals(planned):
    """Every plan passed the program's own checks (it stops at the first that fails)."""
    assert planned[2].startswith("scene_plan_check: OK"), planned[2]


def test_plans_hold_the_recorded_bytes(planned):
    U, out, _ = planned
    with open(U.GOLDEN) as f:
        want = json.load(f)["cases"]
    assert sorted(want) == sorted(U.key(*c) for c in U.cases()) and len(want) == 72
    assert sorted(out) == sorted(want)
    for case in want:
        assert out[case] == want[case], case
