"""The expected bits of rt_render_samples_device, from the CPU
oracle: ORC_EXT_ACCUMULATE called for frame_count 0 .. n - 1 on one sum is the
contract (s = c_0, s = s + c_k in increasing k, sqrt(s / n)), so its sum, its
last frame and its summed counters are what a samples call must give."""
import functools

import numpy as np

from oracle import oracle_lib

COUNTERS = ("segments", "node_visits", "tri_tests", "mat_reads")


def camera_bytes(cam, frame_count, sky_enabled=None):
    """The 80 UBO bytes of cam with another frame_count (and sky_enabled)."""
    from rtamd import CameraUBO
    u = CameraUBO.from_buffer_copy(cam.ubo_bytes() if hasattr(cam, "ubo_bytes") else bytes(cam))
    u.frame_count = frame_count
    if sky_enabled is not None:
        u.sky_enabled = sky_enabled
    return bytes(u)


def accumulate(built, cam, w, h, bounces, n, ext=0, spheres=None, sky_enabled=None, prefixes=()):
    """Samples 0 .. n - 1 of a frame: {"sum": float32 [h, w, 3], "radiance",
    "rgba": the last call's outputs, "counts": the counters summed over the
    calls}; with prefixes (sample counts below n) also the same dict after
    that many samples, under its count in "at"."""
    acc = np.zeros((h, w, 3), np.float32)
    tot = dict.fromkeys(COUNTERS, 0)
    at = {}
    rgba = rad = None
    for k in range(n):
        rgba, rad, cnt = oracle_lib.render(built.model_vertex_data, built.model_material_data, built.flat_bvh_data,
                                           camera_bytes(cam, k, sky_enabled), w, h, bounces,
                                           ext=oracle_lib.EXT_ACCUMULATE | ext, accum=acc, spheres=spheres)
        for c in COUNTERS:
            tot[c] += cnt[c]
        if k + 1 in prefixes or k + 1 == n:
            at[k + 1] = {"sum": acc.copy(), "radiance": rad, "rgba": rgba, "counts": dict(tot)}
    return {**at[n], "at": at}


@functools.lru_cache(maxsize=None)
def config2_built():
    from rtamd import configs
    return configs.config2().build()


@functools.lru_cache(maxsize=None)
def config2_reference(w, h, bounces, n, prefixes=()):
    """accumulate() of config 2's scene through the default camera of the
    size, computed once per test session and never modified."""
    from rtamd import configs
    ref = accumulate(config2_built(), configs.Camera.default(w, h), w, h, bounces, n, prefixes=prefixes)
    for d in ref["at"].values():
        for a in (d["sum"], d["radiance"], d["rgba"]):
            a.setflags(write=False)
    return ref
