"""GPU parity of the hand-over between the format-0 lockstep loop and solo_walk
(rt_trace.hip): the loop's one exit counts the lanes still
walking against solo_lanes, so the frames here put 1, 2, 3 and 4 pixels in a
wave (17x1 .. 20x1: the second 16x4 wave tile) and solo_lanes at 0 .. 3, on both
sides of every count at which a latch off by one would hand over a lane too
early, too late or never.

Bar, as in test_gpu_solo.py (no tolerance anywhere): RGBA8 and the radiance
bits equal the CPU oracle's, segments and material reads the oracle's, node
visits and triangle tests the accel model's, and every launch equals the same
launch at solo_lanes 0.  Each case runs the learning launch, a counting launch
and a plain launch.  The same frames also run split at bounce 1, so the split
launch's second kernel walks them too.
"""
import pytest

import test_gpu_solo as S
import test_gpu_split_pack as P
from conftest import has_gpu
from test_gpu_accel import _upload

pytestmark = pytest.mark.gpu

FRAMES = [(17, 1), (18, 1), (19, 1), (20, 1)]
SOLO = (1, 2, 3)                      # S._frames adds solo_lanes 0, the launch the others are compared with
SCENES = ["c2", "tri3"]


@pytest.fixture(scope="module")
def r():
    if not has_gpu():
        pytest.skip("no GPU")
    import rtamd
    r = rtamd.Renderer((0,))
    yield r
    r.close()


@pytest.mark.parametrize("nl", [1, 8])
@pytest.mark.parametrize("name", SCENES)
def test_handover_lane_counts(r, name, nl):
    """1 to 4 pixels in the second wave tile, 1 and 4 bounces, solo_lanes 0 to 3."""
    from rtamd import configs
    _upload(r, S._built(name), nl)
    for (w, h) in FRAMES:
        cam = configs.Camera.default(w, h)
        for b in (1, 4):
            S._frames(r, name, cam, w, h, b, nl, SOLO, f"hand-over {name}")


@pytest.mark.parametrize("nl", [1, 8])
@pytest.mark.parametrize("name", SCENES)
def test_handover_in_a_split_launch(r, name, nl):
    """The same frames split at bounce 1 (split_pixels lowered, room for every
    pixel): kernel 1 hands its first segments over, kernel 2 every later one."""
    from rtamd import configs
    built = S._built(name)
    _upload(r, built, nl)
    for s in (0,) + SOLO:
        with P._options(r, solo_lanes=s):
            for (w, h) in FRAMES:
                cam = configs.Camera.default(w, h)
                over = P._frames(r, built, cam, w, h, 4, (1,), f"split hand-over {name} layouts {nl} solo_lanes {s}",
                                 capacity=lambda split: 1024)
                assert over == [0], (w, h, s, over)
