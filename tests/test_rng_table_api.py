"""Option rng_table without a GPU (include/rtamd.h): the names
and ranges as the option table declares them, the size computation through the
library and through tools/rng_table_check.cpp (csrc/rng_table_host.h alone,
edges and overflow), the launch key, and the plain-Python chain of
tests/rng_table_ref.py against the oracle's numpy restatement.  The ranges are
exercised through rt_set_option in tests/test_gpu_rng_table.py: a context needs
a device."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "3d-ray-tracer-vulkan_amd")


def test_option_rows_and_header_names():
    src = open(os.path.join(PKG, "csrc", "rt_runtime.hip")).read()
    host = open(os.path.join(PKG, "csrc", "rng_table_host.h")).read()
    hdr = open(os.path.join(ROOT, "include", "rtamd.h")).read()
    assert 'in_range("rng_table", &rt_ctx::rng_table, 0, kRngTableMaxK)' in src
    assert 'in_range("rng_table_mb", &rt_ctx::rng_table_mb, 0, kRngTableMaxMb)' in src
    assert 'in_range("rng_table_pixels", &rt_ctx::rng_table_pixels, 0, 1 << 30)' in src
    assert 'is("rng_table_used")' in src
    assert "constexpr int kRngTableMaxK = 64;" in host and "constexpr int kRngTableMaxMb = 1 << 20;" in host
    for name in ('"rng_table"', '"rng_table_mb"', '"rng_table_pixels"', '"rng_table_used"', "rt_rng_table_bytes", "rt_rng_table_copy",
                 "rt_rng_table_launch_key"):
        assert name in hdr, name


def test_null_arguments_are_refused():
    from rtamd import lib
    L = lib()
    assert L.rt_rng_table_bytes(4, 4, 1, None) == -1                     # RT_ERR_INVALID_ARG
    assert L.rt_rng_table_copy(None, None, 0, None, None, None) == -1
    assert L.rt_rng_table_launch_key(None, 0, None, 0, None) == -1
    n = C.c_size_t()
    assert L.rt_rng_table_launch_key(None, 0, None, 4, C.byref(n)) == -1   # room for words and nowhere to put them


def _bytes(w, h, k):
    from rtamd import lib
    n = C.c_uint64(12345)
    assert lib().rt_rng_table_bytes(w, h, k, C.byref(n)) == 0
    return n.value


def test_size_computation():
    i_max, i_min = 2 ** 31 - 1, -2 ** 31
    assert _bytes(1920, 1080, 2) == 1920 * 1080 * 2 * 16 == 66355200
    assert _bytes(3840, 2160, 2) == 265420800
    assert _bytes(1, 1, 1) == 16 and _bytes(37, 19, 3) == 37 * 19 * 3 * 16
    for w, h, k in ((0, 5, 1), (5, 0, 1), (5, 5, 0), (-1, 5, 1), (5, -1, 1), (5, 5, -1), (5, 5, 65)):
        assert _bytes(w, h, k) == 0, (w, h, k)
    assert _bytes(5, 5, 64) == 5 * 5 * 64 * 16
    # the pixel cap (2^27) from both sides; products past 32 and 63 bits
    assert _bytes(1 << 14, 1 << 13, 64) == (1 << 27) * 64 * 16
    assert _bytes((1 << 14) + 1, 1 << 13, 1) == 0
    assert _bytes(1 << 16, 1 << 16, 1) == 0
    assert _bytes(i_max, i_max, 64) == 0 and _bytes(i_max, 1, 1) == 0 and _bytes(i_min, i_min, i_min) == 0


def test_size_header_on_the_host_alone(tmp_path):
    """csrc/rng_table_host.h compiled into tools/rng_table_check.cpp, which
    checks the same edges and the rng_table_mb cap."""
    exe = tmp_path / "rng_table_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-I", os.path.join(PKG, "csrc"),
                    os.path.join(ROOT, "tools", "rng_table_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    assert "rng_table_check: OK" in out, out


def _key(table, k):
    from rtamd import lib
    n = C.c_size_t()
    assert lib().rt_rng_table_launch_key(table, k, None, 0, C.byref(n)) == 0
    words = (C.c_uint64 * n.value)()
    assert lib().rt_rng_table_launch_key(table, k, words, n.value, C.byref(n)) == 0
    return list(words)


def test_launch_key_tells_tables_apart():
    base = _key(None, 0)
    assert len(base) > 40 and base == _key(None, 0)
    a, b = _key(0x7000_0000_1000, 2), _key(0x7000_0000_2000, 2)
    assert a == _key(0x7000_0000_1000, 2)
    assert len({tuple(base), tuple(a), tuple(b), tuple(_key(0x7000_0000_1000, 3))}) == 4
    # a short buffer is filled as far as it goes
    from rtamd import lib
    n, two = C.c_size_t(), (C.c_uint64 * 2)()
    assert lib().rt_rng_table_launch_key(None, 0, two, 2, C.byref(n)) == 0
    assert n.value == len(base) and list(two) == base[:2]


def test_helper_agrees_with_the_oracles_restatement():
    """tests/rng_table_ref.py against oracle/shader_np.py: pcg on a few hundred
    seeds, and whole rows of the chain (draws, discards, rejection tries)."""
    import rng_table_ref as R
    from oracle import shader_np
    seeds = np.concatenate([np.arange(300, dtype=np.uint32), np.array([0x7FFFFFFF, 0x80000000, 0xFFFFFFFF], np.uint32),
                            (np.arange(300, dtype=np.uint64) * 2654435761 % (1 << 32)).astype(np.uint32)])
    assert [R.pcg(int(s)) for s in seeds] == [int(x) for x in shader_np.pcg(seeds)]
    w, h, k = 16, 4, 3
    want = R.table(w, h, k)
    seed = np.arange(w * h, dtype=np.uint32)
    seed, _ = shader_np.random_float(seed)
    seed, _ = shader_np.random_float(seed)
    for j in range(k):
        seed, px, py, pz = shader_np.random_in_unit_sphere(seed)
        got = np.stack([px.view(np.uint32), py.view(np.uint32), pz.view(np.uint32), seed], -1).reshape(h, w, 4)
        assert np.array_equal(got, want[j]), j
