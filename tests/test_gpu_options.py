"""rt_set_option / rt_get_option (include/rtamd.h): which values every option
takes, that a rejected value leaves the stored one alone, and which names
are read-only.  No scene and no render: the options live in the context.

Defaults are not asserted: rt_create reads them from RTAMD_* variables."""
import pytest

from conftest import has_gpu

pytestmark = pytest.mark.gpu

# name: an inclusive (lo, hi) range, or the set of allowed values
RANGES = {
    "coop_lanes": (-1, 64), "extensions": (0, 15), "heavy_tiles": (-1, 1 << 20), "heavy_factor": (10, 100000),
    "heavy_pixel_factor": (1, 100000), "heavy_cap": (1, 100), "async_slots": (1, 8),
    "concurrent_launches": (1, 64), "order_split": (0, 100), "xcd_order": (0, 4096), "accel_octants": (0, 7),
    "leaf_align": (0, 2), "split_bounce": (0, 64), "heavy_stream": (0, 2), "wave_tile": (-1, 3),
}
SETS = {
    "walk": {0, 2}, "coop_window": {0, 32, 64}, "coop_walk": {0, 1}, "block_waves": {1, 4}, "heavy_first": {0, 1},
    "heavy_pixels": {0, 1}, "reuse_order": {0, 1}, "copy_streams": {1, 2}, "learn_cost": {0, 1},
    "order_frames": {0, 1}, "learn_alone": {0, 1}, "learn_device": {0, 1}, "accel": {0, 1, 8},
    "accel_half": {0, 1}, "accel_wide": {0, 1}, "graph": {0, 1}, "diag": {0, 1},
}
ARCHIVED = ("shade_min", "blocks_per_cu", "seg_limit", "heavy_budget", "prio_after")
READ_ONLY = ("wave_tile_used", "coop_window_used", "accel_half_used", "accel_wide_used", "accel_used", "walk_bytes",
             "leaf_align_used", "heavy_pixels_used", "heavy_tiles_used", "plain_kernels", "hw_queues", "queues_short")


@pytest.fixture(scope="module")
def r():
    if not has_gpu():
        pytest.skip("no GPU")
    import rtamd
    r = rtamd.Renderer((0,))
    yield r
    r.close()


def _rejected(r, name, value):
    from rtamd import RtError
    with pytest.raises(RtError) as e:
        r.set_option(name, value)
    assert e.value.code == -1 and name in str(e.value), (name, value, str(e.value))


def _check(r, name, good, bad):
    for v in good:
        r.set_option(name, v)
        assert r.get_option(name) == v, (name, v)
    for v in bad:
        _rejected(r, name, v)
        assert r.get_option(name) == good[-1], (name, v)


def test_table_covers_every_settable_option():
    assert len(RANGES) + len(SETS) == 32 and not set(RANGES) & set(SETS)


@pytest.mark.parametrize("name", sorted(RANGES))
def test_range_option(r, name):
    lo, hi = RANGES[name]
    _check(r, name, [lo, hi, (lo + hi) // 2], [lo - 1, hi + 1, 1 << 32, -(1 << 32)])


@pytest.mark.parametrize("name", sorted(SETS))
def test_set_option(r, name):
    allowed = sorted(SETS[name])
    between = [v for v in range(allowed[0], allowed[-1]) if v not in SETS[name]][:1]   # walk 1, accel 2 ...
    _check(r, name, allowed, between + [allowed[0] - 1, allowed[-1] + 1, (1 << 32) + allowed[-1]])


def test_accel_between_members(r):
    _check(r, "accel", [8], [4])


def test_unknown_and_archived_names(r):
    from rtamd import RtError
    for name in ("no_such_option",) + ARCHIVED:
        _rejected(r, name, 0)
        with pytest.raises(RtError) as e:
            r.get_option(name)
        assert e.value.code == -1 and name in str(e.value)


def test_kernel(r):
    r.set_option("kernel", 0)
    assert r.get_option("kernel") == 0
    _rejected(r, "kernel", 1)
    assert r.get_option("kernel") == 0


@pytest.mark.parametrize("name", READ_ONLY)
def test_read_only(r, name):
    before = r.get_option(name)
    for v in (0, 1, before):
        _rejected(r, name, v)
    assert r.get_option(name) == before
