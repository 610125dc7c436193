"""The library's source list is written twice, in the Makefile (SRC_ALL, hashed
into rt_build_id) and in rtamd/_lib.py (BUILD_SOURCES, hashed by source_hash()
to tell whether a built library belongs to this tree): the two agree, and no
source file on disk is missing from them."""
import glob
import os
import subprocess

from rtamd import _lib


def test_makefile_and_binding_hash_the_same_sources():
    out = subprocess.run(["make", "-s", "-C", _lib.PKG_ROOT, "src-id"], check=True, capture_output=True, text=True)
    assert out.stdout.strip() == _lib.source_hash()


def test_every_source_on_disk_is_listed():
    on_disk = {f"csrc/{os.path.basename(p)}" for ext in ("hip", "cpp", "h")
               for p in glob.glob(os.path.join(_lib.PKG_ROOT, "csrc", f"*.{ext}"))}
    assert on_disk and on_disk <= set(_lib.BUILD_SOURCES), sorted(on_disk - set(_lib.BUILD_SOURCES))
