"""ctypes binding of the C ABI (include/rtamd.h) — the Python stand-in for the
JNI shim a Java host would use.

The library is the in-tree lib/librtamd.so built by __graft_entry__.build()
(or `make -C 3d-ray-tracer-vulkan_amd`).  There is no fallback: if it is
missing or fails to load, every call raises.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

PKG_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("RTAMD_LIB_PATH") or os.path.join(PKG_ROOT, "lib", "librtamd.so")   # override: experiments

RT_OK = 0
RT_ERR = {
    -1: "RT_ERR_INVALID_ARG",
    -2: "RT_ERR_NO_DEVICE",
    -3: "RT_ERR_HIP",
    -4: "RT_ERR_BAD_SCENE",
    -5: "RT_ERR_NO_SCENE",
    -6: "RT_ERR_OOM",
    -7: "RT_ERR_IO",
}

# Every symbol include/rtamd.h declares (checked by tests/test_abi.py).
ABI_VERSION = 6           # include/rtamd.h RT_ABI_VERSION

EXPORTED = (
    "rt_create", "rt_upload_scene", "rt_render", "rt_render_tile_device", "rt_destroy",
    "rt_last_error", "rt_scene_info", "rt_bvh_layout_size", "rt_build_scene",
    "rt_camera_from_lookat", "rt_mesh_load_obj", "rt_mesh_tri_count", "rt_mesh_transform",
    "rt_mesh_free", "rt_mesh_procedural", "rt_render_bands_device", "rt_band_rows",
    "rt_scene_validate", "rt_set_option", "rt_get_option", "rt_diag_copy",
    "rt_host_alloc", "rt_host_free", "rt_render_async", "rt_render_wait", "rt_upload_spheres",
    "rt_render_batch_device", "rt_band_list_rows", "rt_render_batch_lists_device", "rt_band_lists_rows",
    "rt_render_poll", "rt_accel_records", "rt_abi_version", "rt_pack_rgb", "rt_unpack_rgb",
    "rt_build_id", "rt_render_batch_rect_device", "rt_render_batch_runs_device",
    "rt_query_rays_device", "rt_query_rays", "rt_render_hits_device", "rt_pick", "rt_build_scene_map",
    "rt_denoise_default_params", "rt_denoise_workspace_bytes", "rt_denoise_device", "rt_render_denoised",
    "rt_albedo_device", "rt_denoise_albedo_device",
    "rt_temporal_default_params", "rt_temporal_camera_basis", "rt_temporal_device", "rt_render_temporal",
    "rt_denoise_history_device", "rt_render_temporal_adaptive",
    "rt_temporal_moments_device", "rt_variance_default_params", "rt_denoise_variance_device",
    "rt_render_temporal_variance", "rt_temporal_motion_device",
    "rt_learn_device", "rt_learn_copy",
    "rt_samples_workspace_bytes", "rt_render_samples_device", "rt_render_samples",
    "rt_update_geometry", "rt_refit_scene", "rt_accel_refit_records", "rt_scene_copy_records",
    "rt_update_geometry_device",
    "rt_rng_table_bytes", "rt_rng_table_copy", "rt_rng_table_launch_key",
)

# The library's sources in the Makefile's SRC_ALL order: rt_build_id's
# "src=" field is the first 16 hex digits of SHA-256 over them concatenated.
BUILD_SOURCES = ("csrc/rt_trace.hip", "csrc/rt_runtime.hip", "csrc/rt_learn.hip", "csrc/rt_wire.hip",
                 "csrc/rt_filter.hip", "csrc/rt_temporal.hip", "csrc/rt_samples.hip", "csrc/rt_refit.hip", "csrc/rt_rngtable.hip",
                 "csrc/scene_build.cpp", "csrc/accel_build.cpp", "csrc/scene_plan.cpp", "csrc/rt_internal.h", "csrc/rt_pixel.h",
                 "csrc/accel_build.h", "csrc/temporal_motion_host.h", "csrc/refit_levels_host.h", "csrc/rt_rng.h",
                 "csrc/rng_table_host.h", "csrc/scene_plan.h", "../include/rtamd.h")


def source_hash() -> str:
    """SHA-256 (16 hex digits) of the library's sources as they are in this tree."""
    import hashlib
    h = hashlib.sha256()
    for f in BUILD_SOURCES:
        with open(os.path.join(PKG_ROOT, f), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def file_build_id(path: str = LIB_PATH) -> str | None:
    """The build id embedded in a built library, read from the file (no load)."""
    import re
    try:
        with open(path, "rb") as fh:
            m = re.search(rb"RTAMD_BUILD_ID:(src=[0-9a-f]{16} git=[0-9a-z]+)", fh.read())
    except OSError:
        return None
    return m.group(1).decode() if m else None


def build_matches_tree(path: str = LIB_PATH) -> bool:
    """True when the library at path was built from this tree's sources."""
    bid = file_build_id(path)
    return bid is not None and bid.startswith(f"src={source_hash()} ")


class RtError(RuntimeError):
    """A non-zero status from the C ABI (the JNI shim throws RuntimeException)."""

    def __init__(self, code: int, message: str):
        super().__init__(f"{RT_ERR.get(code, code)}: {message}")
        self.code = code


class CameraUBO(C.Structure):
    _fields_ = [
        ("origin", C.c_float * 4),
        ("lower_left", C.c_float * 4),
        ("horizontal", C.c_float * 4),
        ("vertical", C.c_float * 4),
        ("frame_count", C.c_int32),
        ("sky_enabled", C.c_int32),
        ("pad", C.c_int32 * 2),
    ]


class Stats(C.Structure):
    _fields_ = [
        ("segments", C.c_uint64),
        ("node_visits", C.c_uint64),
        ("tri_tests", C.c_uint64),
        ("mat_reads", C.c_uint64),
        ("ms", C.c_double),
        ("pixels", C.c_uint64),
    ]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


class Ray(C.Structure):                 # rt_ray
    _fields_ = [("origin", C.c_float * 3), ("t_max", C.c_float), ("dir", C.c_float * 3), ("reserved", C.c_uint32)]


class Hit(C.Structure):                 # rt_hit
    _fields_ = [("t", C.c_float), ("tri", C.c_int32), ("normal", C.c_float * 3), ("pos", C.c_float * 3)]


class DenoiseParams(C.Structure):       # rt_denoise_params; the defaults are rt_denoise_default_params's
    _fields_ = [("iterations", C.c_int32), ("normal_power_log2", C.c_int32), ("sigma_depth", C.c_float),
                ("sigma_color", C.c_float)]

    def __init__(self, iterations: int = 4, normal_power_log2: int = 7, sigma_depth: float = 0.005,
                 sigma_color: float = 0.5):
        super().__init__(iterations, normal_power_log2, sigma_depth, sigma_color)


class TemporalParams(C.Structure):      # rt_temporal_params; the defaults are rt_temporal_default_params's
    _fields_ = [("max_history", C.c_int32), ("plane_tol", C.c_float), ("normal_min", C.c_float),
                ("reserved", C.c_int32)]

    def __init__(self, max_history: int = 32, plane_tol: float = 0.005, normal_min: float = 0.9):
        super().__init__(max_history, plane_tol, normal_min, 0)


class VarianceParams(C.Structure):      # rt_variance_params; the defaults are rt_variance_default_params's
    _fields_ = [("iterations", C.c_int32), ("normal_power_log2", C.c_int32), ("sigma_depth", C.c_float),
                ("sigma_lum", C.c_float), ("min_history", C.c_int32), ("reserved", C.c_int32 * 3)]

    def __init__(self, iterations: int = 4, normal_power_log2: int = 7, sigma_depth: float = 0.005,
                 sigma_lum: float = 1.0, min_history: int = 4):
        super().__init__(iterations, normal_power_log2, sigma_depth, sigma_lum, min_history)


class LearnParams(C.Structure):         # rt_learn_params
    _fields_ = [(k, C.c_int32) for k in ("rec_off", "learn_cost", "order_split", "heavy_pixel_factor", "concurrent",
                                         "resident", "cap", "xcd", "tiles_x", "tiles_y", "frames", "reserved")]


class LearnInfo(C.Structure):           # rt_learn_info
    _fields_ = [(k, C.c_int32) for k in ("n_tiles", "n_hpix", "heavy", "on_device", "xcd_applied",
                                         "records_resident")] + [("params", LearnParams)]


RT_QUERY_ANY = 1
RT_GEOM_F32 = 1                 # rt_update_geometry_device's flags
RT_TEMPORAL_RESET = 1           # rt_render_temporal's flags
RT_TEMPORAL_FIXED_SEED = 2

assert C.sizeof(CameraUBO) == 80
assert C.sizeof(Ray) == 32 and C.sizeof(Hit) == 32 and C.sizeof(DenoiseParams) == 16
assert C.sizeof(TemporalParams) == 16 and C.sizeof(VarianceParams) == 32
assert C.sizeof(LearnParams) == 48 and C.sizeof(LearnInfo) == 72

_lock = threading.Lock()
_lib = None


def lib() -> C.CDLL:
    global _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise RtError(-3, f"{LIB_PATH} is missing: run __graft_entry__.build() "
                                  "(there is no non-HIP fallback)")
            # torch bundles its own libamdhip64.so.7 (same soname as ROCm's).  The
            # first one loaded serves the whole process, and torch only works
            # with its own; load it first so torch tensors and this library
            # share one HIP runtime.
            try:
                import torch  # noqa: F401
            except ImportError:
                pass
            L = C.CDLL(LIB_PATH)
            vp, sz, i32, u64, dp, fp = C.c_void_p, C.c_size_t, C.c_int, C.c_uint64, C.POINTER(C.c_double), C.POINTER(C.c_float)
            sig = {
                "rt_create": (i32, [C.POINTER(C.c_int), i32, C.POINTER(vp)]),
                "rt_upload_scene": (i32, [vp, vp, sz, vp, sz, vp, sz]),
                "rt_upload_spheres": (i32, [vp, vp, i32]),
                "rt_render": (i32, [vp, C.POINTER(CameraUBO), i32, i32, i32, vp, vp, C.POINTER(Stats)]),
                "rt_render_tile_device": (i32, [vp, C.POINTER(CameraUBO), i32, i32, i32, i32, i32, i32, i32,
                                                vp, vp, vp, C.POINTER(Stats)]),
                "rt_destroy": (i32, [vp]),
                "rt_last_error": (C.c_char_p, []),
                "rt_scene_info": (i32, [vp, C.POINTER(sz), C.POINTER(sz), C.POINTER(i32)]),
                "rt_bvh_layout_size": (i32, [sz, C.POINTER(sz), C.POINTER(sz)]),
                "rt_build_scene": (i32, [dp, fp, sz, u64, i32, fp, fp, vp]),
                "rt_camera_from_lookat": (i32, [dp, dp, dp, C.c_double, C.c_double, C.POINTER(CameraUBO)]),
                "rt_mesh_load_obj": (i32, [C.c_char_p, C.POINTER(vp)]),
                "rt_mesh_tri_count": (sz, [vp]),
                "rt_mesh_transform": (i32, [vp, dp, dp, dp]),
                "rt_mesh_free": (i32, [vp]),
                "rt_mesh_procedural": (i32, [sz, u64, dp, dp, dp]),
                "rt_render_bands_device": (i32, [vp, C.POINTER(CameraUBO), i32, i32, i32, i32, i32, i32,
                                                 vp, vp, vp, C.POINTER(Stats)]),
                "rt_band_rows": (i32, [i32, i32, i32, i32]),
                "rt_render_batch_device": (i32, [vp, C.POINTER(CameraUBO), i32, i32, i32, i32, i32,
                                                 C.POINTER(C.c_int32), i32, vp, vp, vp, C.POINTER(Stats)]),
                "rt_band_list_rows": (i32, [i32, i32, C.POINTER(C.c_int32), i32]),
                "rt_render_batch_lists_device": (i32, [vp, C.POINTER(CameraUBO), i32, i32, i32, i32, i32,
                                                       C.POINTER(C.c_int32), i32, vp, vp, vp, C.POINTER(Stats)]),
                "rt_band_lists_rows": (i32, [i32, i32, C.POINTER(C.c_int32), i32, i32]),
                "rt_render_batch_rect_device": (i32, [vp, C.POINTER(CameraUBO), i32, i32, i32, i32, i32, i32, i32,
                                                      i32, vp, vp, vp, C.POINTER(Stats)]),
                "rt_render_batch_runs_device": (i32, [vp, C.POINTER(CameraUBO), i32, i32, i32, i32, i32,
                                                      C.POINTER(C.c_int32), C.POINTER(C.c_int32), vp, vp, vp,
                                                      C.POINTER(Stats)]),
                "rt_scene_validate": (i32, [vp, sz, vp, sz, vp, sz, C.POINTER(sz), C.POINTER(i32)]),
                "rt_set_option": (i32, [vp, C.c_char_p, C.c_int64]),
                "rt_get_option": (i32, [vp, C.c_char_p, C.POINTER(C.c_int64)]),
                "rt_diag_copy": (i32, [vp, vp, sz, C.POINTER(sz)]),
                "rt_host_alloc": (vp, [sz]),
                "rt_host_free": (None, [vp]),
                "rt_render_async": (i32, [vp, C.POINTER(CameraUBO), i32, i32, i32, vp, C.POINTER(u64)]),
                "rt_render_wait": (i32, [vp, u64]),
                "rt_render_poll": (i32, [vp, u64, C.POINTER(i32)]),
                "rt_accel_records": (i32, [vp, sz, vp, sz, vp, sz, i32, C.POINTER(C.c_uint32), sz, C.POINTER(sz),
                                           C.POINTER(C.c_int32)]),
                "rt_abi_version": (i32, [C.POINTER(sz), C.POINTER(sz)]),
                "rt_build_id": (C.c_char_p, []),
                "rt_pack_rgb": (i32, [vp, vp, sz, vp]),
                "rt_unpack_rgb": (i32, [vp, vp, sz, vp]),
                "rt_query_rays_device": (i32, [vp, vp, sz, C.c_uint32, vp, vp, C.POINTER(Stats)]),
                "rt_query_rays": (i32, [vp, vp, sz, C.c_uint32, vp, C.POINTER(Stats)]),
                "rt_render_hits_device": (i32, [vp, C.POINTER(CameraUBO), i32, i32, i32, i32, i32, i32, C.c_uint32,
                                                vp, vp, C.POINTER(Stats)]),
                "rt_pick": (i32, [vp, C.POINTER(CameraUBO), i32, i32, i32, i32, C.POINTER(Hit)]),
                "rt_build_scene_map": (i32, [dp, fp, sz, u64, i32, fp, fp, vp, C.POINTER(C.c_uint32)]),
                "rt_denoise_default_params": (None, [C.POINTER(DenoiseParams)]),
                "rt_denoise_workspace_bytes": (sz, [i32, i32]),
                "rt_denoise_device": (i32, [vp, i32, i32, vp, vp, C.POINTER(DenoiseParams), vp, vp, vp, vp, dp]),
                "rt_render_denoised": (i32, [vp, C.POINTER(CameraUBO), i32, i32, i32, C.POINTER(DenoiseParams), vp, vp,
                                             C.POINTER(Stats)]),
                "rt_albedo_device": (i32, [vp, i32, i32, vp, vp, vp, dp]),
                "rt_denoise_albedo_device": (i32, [vp, i32, i32, vp, vp, vp, C.POINTER(DenoiseParams), vp, vp, vp, vp,
                                                   dp]),
                "rt_temporal_default_params": (None, [C.POINTER(TemporalParams)]),
                "rt_temporal_camera_basis": (i32, [C.POINTER(CameraUBO), fp]),
                "rt_temporal_device": (i32, [vp, i32, i32, C.POINTER(CameraUBO), vp, vp, C.POINTER(CameraUBO), vp, vp,
                                             C.POINTER(TemporalParams), vp, vp, vp, vp, dp]),
                "rt_render_temporal": (i32, [vp, C.POINTER(CameraUBO), i32, i32, i32, C.POINTER(TemporalParams),
                                             C.POINTER(DenoiseParams), C.c_uint32, vp, vp, C.POINTER(Stats)]),
                "rt_denoise_history_device": (i32, [vp, i32, i32, vp, vp, C.POINTER(DenoiseParams), vp, vp, vp, vp, dp]),
                "rt_render_temporal_adaptive": (i32, [vp, C.POINTER(CameraUBO), i32, i32, i32, C.POINTER(TemporalParams),
                                                      C.POINTER(DenoiseParams), C.c_uint32, vp, vp, C.POINTER(Stats)]),
                "rt_temporal_moments_device": (i32, [vp, i32, i32, C.POINTER(CameraUBO), vp, vp, C.POINTER(CameraUBO), vp,
                                                     vp, C.POINTER(TemporalParams), vp, vp, vp, vp, dp, vp, vp]),
                "rt_temporal_motion_device": (i32, [vp, i32, i32, C.POINTER(CameraUBO), vp, vp, C.POINTER(CameraUBO), vp,
                                                    vp, C.POINTER(TemporalParams), vp, vp, vp, vp, dp, vp, vp, vp, vp,
                                                    sz]),
                "rt_variance_default_params": (None, [C.POINTER(VarianceParams)]),
                "rt_denoise_variance_device": (i32, [vp, i32, i32, vp, vp, vp, C.POINTER(VarianceParams), vp, vp, vp, vp,
                                                     dp]),
                "rt_render_temporal_variance": (i32, [vp, C.POINTER(CameraUBO), i32, i32, i32, C.POINTER(TemporalParams),
                                                      C.POINTER(VarianceParams), C.c_uint32, vp, vp, C.POINTER(Stats)]),
                "rt_learn_device": (i32, [vp, vp, vp, i32, C.POINTER(LearnParams), vp, vp, vp, vp, vp]),
                "rt_learn_copy": (i32, [vp, C.POINTER(LearnInfo), vp, vp, vp, vp, vp]),
                "rt_samples_workspace_bytes": (sz, [i32, i32, i32]),
                "rt_render_samples_device": (i32, [vp, C.POINTER(CameraUBO), i32, i32, i32, i32, vp, sz, vp, vp, vp, vp,
                                                   C.POINTER(Stats)]),
                "rt_render_samples": (i32, [vp, C.POINTER(CameraUBO), i32, i32, i32, i32, vp, vp, C.POINTER(Stats)]),
                "rt_update_geometry": (i32, [vp, vp, sz, vp, sz, dp]),
                "rt_update_geometry_device": (i32, [vp, vp, sz, vp, sz, C.c_uint32, dp]),
                "rt_refit_scene": (i32, [dp, sz, C.POINTER(C.c_uint32), sz, fp, vp, sz]),
                "rt_accel_refit_records": (i32, [C.POINTER(C.c_uint32), sz, i32, vp, sz, vp, sz]),
                "rt_scene_copy_records": (i32, [vp, i32, C.POINTER(C.c_uint32), sz, C.POINTER(sz)]),
                "rt_rng_table_bytes": (i32, [i32, i32, i32, C.POINTER(C.c_uint64)]),
                "rt_rng_table_copy": (i32, [vp, vp, sz, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
                "rt_rng_table_launch_key": (i32, [vp, i32, C.POINTER(C.c_uint64), sz, C.POINTER(sz)]),
            }
            for name, (res, args) in sig.items():
                f = getattr(L, name)
                f.restype = res
                f.argtypes = args
            # the structs this binding lays out must be the library's
            sb, cb = C.c_size_t(), C.c_size_t()
            ver = L.rt_abi_version(C.byref(sb), C.byref(cb))
            if ver != ABI_VERSION or sb.value != C.sizeof(Stats) or cb.value != C.sizeof(CameraUBO):
                raise RtError(-1, f"{LIB_PATH}: ABI version {ver} (rt_stats {sb.value} B, camera {cb.value} B); "
                                  f"this binding expects {ABI_VERSION} ({C.sizeof(Stats)} B, {C.sizeof(CameraUBO)} B)")
            _lib = L
        return _lib


def check(rc: int) -> None:
    if rc != RT_OK:
        msg = lib().rt_last_error()
        raise RtError(rc, msg.decode() if msg else "")


RT_ACCEL_FORMAT_HALF = 0x100
RT_ACCEL_FORMAT_WIDE = 0x200


def accel_records(built, n_layouts: int = 8, half: bool = False, wide: bool = False):
    """Option accel's records for a BuiltCpuData (rt_accel_records): returns
    (uint32[slots_total * 8] (half: * 4, option accel_half's format; wide: *
    16, option accel_wide's 64-B records), info dict).  Host-only; no device
    needed."""
    import numpy as np
    L = lib()
    bufs = [np.ascontiguousarray(np.frombuffer(bytes(x), dtype=np.uint8)) if isinstance(x, (bytes, bytearray))
            else np.ascontiguousarray(x) for x in (built.model_vertex_data, built.model_material_data,
                                                   built.flat_bvh_data)]
    args = []
    for b in bufs:
        args += [b.ctypes.data, b.nbytes]
    n = C.c_size_t(0)
    info = (C.c_int32 * 8)()
    nl = n_layouts | (RT_ACCEL_FORMAT_HALF if half else 0) | (RT_ACCEL_FORMAT_WIDE if wide else 0)
    check(L.rt_accel_records(*args, nl, None, 0, C.byref(n), info))
    out = np.zeros(n.value, dtype=np.uint32)
    check(L.rt_accel_records(*args, nl, out.ctypes.data_as(C.POINTER(C.c_uint32)), out.size, C.byref(n), info))
    keys = ("n_layouts", "slots", "root_leaf", "n_prims", "n_inputs", "depth", "max_class", "n_thin")
    d = dict(zip(keys, list(info)))
    d["format"] = 1 if half else (2 if wide else 0)
    return out, d


def accel_refit_records(records, n_layouts: int, built):
    """rt_accel_refit_records: a refitted copy of format-0 accel records
    (accel_records' words for n_layouts 1 or 8) for the moved vertices and the
    new boxes of `built`.  Host-only."""
    import numpy as np
    out = np.array(records, dtype=np.uint32, copy=True)
    v = np.ascontiguousarray(built.model_vertex_data)
    b = np.ascontiguousarray(built.flat_bvh_data)
    check(lib().rt_accel_refit_records(out.ctypes.data_as(C.POINTER(C.c_uint32)), out.size, n_layouts,
                                       v.ctypes.data, v.nbytes, b.ctypes.data, b.nbytes))
    return out
