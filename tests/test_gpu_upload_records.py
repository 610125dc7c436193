"""rt_upload_scene on the GPU against tests/golden/upload_records.json: the word
counts and hashes of every device array rt_scene_copy_records shows, and
rt_scene_info's numbers, as the library put them there before the upload's
layout moved into csrc/scene_plan.cpp (tools/upload_records.py wrote the file
with that library).  The small refit scenes in tests/test_gpu_refit.py's modes,
with option refit 0 and 1."""
import importlib.util
import json
import os

import pytest

from conftest import has_gpu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("upload_records", os.path.join(ROOT, "tools", "upload_records.py"))
U = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(U)

with open(U.GOLDEN) as _f:
    WANT = json.load(_f)["cases"]


@pytest.fixture(scope="module")
def ctx():
    if not has_gpu():
        pytest.skip("no GPU")
    import rtamd
    r = rtamd.Renderer((0,))
    yield r
    r.close()


def test_file_covers_the_cases():
    assert sorted(WANT) == sorted(U.key(*c) for c in U.cases()) and len(WANT) == 72


@pytest.mark.parametrize("name", U.SCENES)
def test_upload_holds_the_recorded_bytes(ctx, name):
    built = U.built_scene(name)
    for mode in U.MODES:
        for refit in (0, 1):
            got = U.upload(ctx, built, mode, refit)
            assert ctx.get_option("accel_used") == mode[0] and ctx.get_option("refit_used") == refit
            assert got == WANT[U.key(name, mode, refit)], U.key(name, mode, refit)
