"""Render side of the host API.

Renderer   — a synchronous wrapper of one rt_ctx (the C ABI).
HipEngine  — a mirror of the reference's VulkanEngine public API
             (src/dev/demir/vulkan/engine/VulkanEngine.java:120-185): a render
             thread fed through queues that are drained to their latest value
             (handleCommands :277-313), rendering frames as long as a scene and
             a camera are present (mainLoop :244-271) and publishing each one to
             an AtomicReference-like slot (:264).
FrameData  — FrameData.java:9-16 (+ the render statistics its TODO asks for).
"""
from __future__ import annotations

import ctypes as C
import queue
import threading
import time
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple, Union

import numpy as np

from ._lib import (RT_GEOM_F32, RT_QUERY_ANY, RT_TEMPORAL_FIXED_SEED, RT_TEMPORAL_RESET, CameraUBO, DenoiseParams, Hit,
                   LearnInfo, LearnParams, RtError, Stats, TemporalParams, VarianceParams, check, lib)
from .scene import BuiltCpuData, Camera

REFERENCE_WIDTH = 1280          # VulkanEngine.java:45
REFERENCE_HEIGHT = 720          # VulkanEngine.java:46
REFERENCE_MAX_BOUNCES = 10      # compute_dynamic_ray.comp:44

# rt_ray / rt_hit (include/rtamd.h) as numpy records, 32 bytes each
RAY_DTYPE = np.dtype([("origin", "<f4", (3,)), ("t_max", "<f4"), ("dir", "<f4", (3,)), ("reserved", "<u4")])
HIT_DTYPE = np.dtype([("t", "<f4"), ("tri", "<i4"), ("normal", "<f4", (3,)), ("pos", "<f4", (3,))])
assert RAY_DTYPE.itemsize == 32 and HIT_DTYPE.itemsize == 32


def _rays(rays) -> np.ndarray:
    """Rays as contiguous RAY_DTYPE records: from such records, or from
    float32 (n, 8) rows (origin.xyz, t_max, dir.xyz, reserved)."""
    r = np.asarray(rays)
    if r.dtype == RAY_DTYPE:
        return np.ascontiguousarray(r).reshape(-1)
    if r.dtype.fields is None and r.ndim == 2 and r.shape[1] == 8:
        return np.ascontiguousarray(r, dtype=np.float32).view(RAY_DTYPE).reshape(-1)
    raise TypeError("rays must be RAY_DTYPE records or a float32 (n, 8) array")


def _ubo(cam: Union[Camera, CameraUBO, bytes]) -> CameraUBO:
    if isinstance(cam, Camera):
        return cam.ubo
    if isinstance(cam, CameraUBO):
        return cam
    if isinstance(cam, (bytes, bytearray)) and len(cam) == 80:
        return CameraUBO.from_buffer_copy(cam)
    raise TypeError("camera must be a Camera, a CameraUBO or 80 UBO bytes")


class Renderer:
    """One context on one or more HIP devices (rt_create / rt_destroy)."""

    def __init__(self, device_ids: Sequence[int] = (0,)):
        ids = (C.c_int * len(device_ids))(*device_ids)
        self._ctx = C.c_void_p()
        check(lib().rt_create(ids, len(device_ids), C.byref(self._ctx)))
        self.device_ids = tuple(device_ids)

    def close(self) -> None:
        if self._ctx:
            lib().rt_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_option(self, name: str, value: int) -> None:
        """Schedule options (rt_set_option; the list is in include/rtamd.h):
        "walk", "coop_lanes", "solo_lanes", "heavy_first", "concurrent_launches", ...
        Results do not depend on them."""
        check(lib().rt_set_option(self._ctx, name.encode(), int(value)))

    def get_option(self, name: str) -> int:
        v = C.c_int64()
        check(lib().rt_get_option(self._ctx, name.encode(), C.byref(v)))
        return v.value

    def walk_bytes(self) -> int:
        """Bytes of the records one ray walks (option walk_bytes)."""
        return self.get_option("walk_bytes")

    def upload_scene(self, data: BuiltCpuData) -> None:
        """internalSwapScene (VulkanEngine.java:318-373); deep copy."""
        v = np.ascontiguousarray(data.model_vertex_data, dtype=np.float32)
        m = np.ascontiguousarray(data.model_material_data, dtype=np.float32)
        b = np.ascontiguousarray(data.flat_bvh_data, dtype=np.uint8)
        check(lib().rt_upload_scene(self._ctx, v.ctypes.data, v.nbytes, m.ctypes.data, m.nbytes,
                                    b.ctypes.data, b.nbytes))

    def update_geometry(self, built: BuiltCpuData, ms: bool = False):
        """rt_update_geometry: the scene's triangles moved, in the tree it was
        uploaded with (option "refit" 1 at that upload).  built: the moved
        vertex records and the uploaded nodes with new boxes
        (rtamd.refit_buffers).  Returns the refit kernels' device time in ms
        with ms=True, else None."""
        v = np.ascontiguousarray(built.model_vertex_data, dtype=np.float32)
        b = np.ascontiguousarray(built.flat_bvh_data, dtype=np.uint8)
        t = C.c_double()
        check(lib().rt_update_geometry(self._ctx, v.ctypes.data, v.nbytes, b.ctypes.data, b.nbytes,
                                       C.byref(t) if ms else None))
        return t.value if ms else None

    def update_geometry_device(self, tri_verts, source=None, ms: bool = False):
        """rt_update_geometry_device: update_geometry from a tensor that
        already lives on the context's device (a one-device context, options
        "refit" and "refit_device" 1 at the upload).  tri_verts: a contiguous
        float64 or float32 torch tensor of 9 * n_tris elements (v0, v1, v2 of
        each input triangle, as build_buffers took them); source: the built
        scene's flat_source as an int32 tensor on the same device, or None
        for input that is already in flattened order.  Synchronous: the
        device is drained first, so whatever stream produced the tensors has
        finished.  Returns the device time of its kernels in ms with ms=True,
        else None.  ValueError (before the library is called) for anything
        but such tensors."""
        import torch
        dev = torch.device("cuda", self.device_ids[0])

        def on_device(t, what, dtypes):
            if not isinstance(t, torch.Tensor):
                raise ValueError(f"{what} must be a torch tensor on {dev}, not {type(t).__name__}")
            if t.device != dev:
                raise ValueError(f"{what} is on {t.device}, the context renders on {dev}")
            if t.dtype not in dtypes:
                raise ValueError(f"{what} is {t.dtype}, expected one of {[str(d) for d in dtypes]}")
            if not t.is_contiguous():
                raise ValueError(f"{what} must be contiguous")
            return t

        tv = on_device(tri_verts, "tri_verts", (torch.float64, torch.float32))
        if tv.numel() % 9:
            raise ValueError(f"tri_verts has {tv.numel()} elements, not 9 per triangle")
        n_tris = tv.numel() // 9
        if source is None:
            n_flat, src_ptr = n_tris, None
        else:
            src = on_device(source, "source", (torch.int32,))
            n_flat, src_ptr = src.numel(), src.data_ptr() or None
        flags = RT_GEOM_F32 if tv.dtype == torch.float32 else 0
        t = C.c_double()
        check(lib().rt_update_geometry_device(self._ctx, tv.data_ptr() or None, n_tris, src_ptr, n_flat, flags,
                                              C.byref(t) if ms else None))
        return t.value if ms else None

    def copy_records(self, which: int) -> np.ndarray:
        """rt_scene_copy_records: one of the scene's device arrays as uint32
        words (0 walk, 1 walk_ref, 2 shading, 3 nodes, 4 leafs, 5 pairs; empty
        when the scene holds none).  A diagnostic: it waits for the device."""
        n = C.c_size_t()
        check(lib().rt_scene_copy_records(self._ctx, which, None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=np.uint32)
        if n.value:
            check(lib().rt_scene_copy_records(self._ctx, which, out.ctypes.data_as(C.POINTER(C.c_uint32)), out.size,
                                              C.byref(n)))
        return out

    def upload_spheres(self, spheres) -> None:
        """Extension (option "extensions" bit 8; no reference counterpart):
        float32[n, 8] = (centre.xyz, radius, albedo.rgb, type); n = 0 removes
        them.  Deep copy; independent of upload_scene."""
        s = np.ascontiguousarray(np.asarray(spheres, dtype=np.float32).reshape(-1, 8))
        check(lib().rt_upload_spheres(self._ctx, s.ctypes.data if len(s) else None, len(s)))

    def upload_raw(self, vertices: bytes, materials: bytes, nodes: bytes) -> None:
        check(lib().rt_upload_scene(self._ctx, vertices, len(vertices), materials, len(materials),
                                    nodes, len(nodes)))

    def scene_info(self) -> dict:
        nn, nt, d = C.c_size_t(), C.c_size_t(), C.c_int()
        check(lib().rt_scene_info(self._ctx, C.byref(nn), C.byref(nt), C.byref(d)))
        return {"n_nodes": nn.value, "n_tris": nt.value, "max_depth": d.value}

    def render(self, camera, width: int, height: int, max_bounces: int = REFERENCE_MAX_BOUNCES,
               radiance: bool = False, stats: bool = False):
        """renderFrame (VulkanEngine.java:401-431).  Returns (rgba[H,W,4] uint8,
        radiance[H,W,3] float32 or None, stats dict or None)."""
        rgba = np.empty((height, width, 4), dtype=np.uint8)
        rad = np.empty((height, width, 3), dtype=np.float32) if radiance else None
        st = Stats() if stats else None
        check(lib().rt_render(self._ctx, C.byref(_ubo(camera)), width, height, max_bounces,
                              rgba.ctypes.data, rad.ctypes.data if rad is not None else None,
                              C.byref(st) if st is not None else None))
        return rgba, rad, (st.as_dict() if st is not None else None)

    def render_async(self, camera, width: int, height: int, max_bounces: int, out: "PinnedFrame") -> int:
        """Enqueue a whole frame into a pinned host frame and return its ticket
        (rt_render_async); the frame is complete after wait(ticket)."""
        if out.shape != (height, width, 4):
            raise ValueError(f"frame buffer is {out.shape}, need {(height, width, 4)}")
        t = C.c_uint64()
        check(lib().rt_render_async(self._ctx, C.byref(_ubo(camera)), width, height, max_bounces,
                                    out.ptr, C.byref(t)))
        return t.value

    def wait(self, ticket: int) -> None:
        check(lib().rt_render_wait(self._ctx, ticket))

    def poll(self, ticket: int) -> bool:
        """True when the frame of `ticket` is complete (rt_render_poll; never blocks)."""
        done = C.c_int32()
        check(lib().rt_render_poll(self._ctx, ticket, C.byref(done)))
        return bool(done.value)

    def render_tile_device(self, camera, width: int, height: int, max_bounces: int,
                           x0: int, y0: int, tile_w: int, tile_h: int,
                           d_rgba: Optional[int], d_radiance: Optional[int] = None,
                           stream: Optional[int] = None, stats: bool = False):
        """Enqueue one tile into device buffers (raw device pointers, e.g.
        torch tensor data_ptr()) on a HIP stream handle."""
        st = Stats() if stats else None
        check(lib().rt_render_tile_device(self._ctx, C.byref(_ubo(camera)), width, height, max_bounces,
                                          x0, y0, tile_w, tile_h, d_rgba, d_radiance, stream,
                                          C.byref(st) if st is not None else None))
        return st.as_dict() if st is not None else None

    # --- ray queries (include/rtamd.h "queries") ---
    def query_rays(self, rays, any_hit: bool = False, stats: bool = False):
        """Closest hits (any_hit: any hit, RT_QUERY_ANY) of a batch of rays in
        host memory (rt_query_rays): RAY_DTYPE records or float32 (n, 8) rows
        in, HIT_DTYPE records out; with stats, (hits, stats dict)."""
        r = _rays(rays)
        hits = np.empty(len(r), dtype=HIT_DTYPE)
        st = Stats() if stats else None
        check(lib().rt_query_rays(self._ctx, r.ctypes.data, len(r), RT_QUERY_ANY if any_hit else 0,
                                  hits.ctypes.data, C.byref(st) if st is not None else None))
        return (hits, st.as_dict()) if st is not None else hits

    def query_rays_device(self, d_rays: int, n_rays: int, d_hits: int, any_hit: bool = False,
                          stream: Optional[int] = None, stats: bool = False):
        """The same between device buffers (raw 16-byte aligned device
        pointers) on a HIP stream handle (rt_query_rays_device); asynchronous
        unless stats."""
        st = Stats() if stats else None
        check(lib().rt_query_rays_device(self._ctx, d_rays, n_rays, RT_QUERY_ANY if any_hit else 0, d_hits,
                                         stream, C.byref(st) if st is not None else None))
        return st.as_dict() if st is not None else None

    def render_hits_device(self, camera, width: int, height: int, x0: int, y0: int, tile_w: int, tile_h: int,
                           d_hits: int, stream: Optional[int] = None, any_hit: bool = False, stats: bool = False):
        """Enqueue the first-hit buffer of a tile into a device buffer of
        tile_h x tile_w rt_hit records (a raw 16-byte aligned device pointer)
        on a HIP stream handle (rt_render_hits_device); asynchronous unless stats."""
        st = Stats() if stats else None
        check(lib().rt_render_hits_device(self._ctx, C.byref(_ubo(camera)), width, height, x0, y0, tile_w, tile_h,
                                          RT_QUERY_ANY if any_hit else 0, d_hits, stream,
                                          C.byref(st) if st is not None else None))
        return st.as_dict() if st is not None else None

    def render_hits(self, camera, width: int, height: int, tile: Optional[Tuple[int, int, int, int]] = None,
                    any_hit: bool = False, stats: bool = False):
        """The first-hit buffer of the frame render() draws: HIT_DTYPE records
        [tile_h, tile_w] of the tile (x0, y0, tile_w, tile_h), default the
        whole frame; with stats, (hits, stats dict)."""
        import torch
        x0, y0, tw, th = tile if tile is not None else (0, 0, width, height)
        with torch.cuda.device(self.device_ids[0]):
            d = torch.empty((max(th, 0), max(tw, 0), 8), dtype=torch.float32, device="cuda")
            st = self.render_hits_device(camera, width, height, x0, y0, tw, th, d.data_ptr(),
                                         torch.cuda.current_stream().cuda_stream, any_hit, stats)
            hits = d.cpu().numpy().view(HIT_DTYPE)[..., 0]
        return (hits, st) if stats else hits

    def pick(self, camera, width: int, height: int, x: int, y: int) -> np.ndarray:
        """The hit record (a HIT_DTYPE scalar) of pixel (x, y)'s primary ray
        (rt_pick); rtamd.instance_of names its instance."""
        h = Hit()
        check(lib().rt_pick(self._ctx, C.byref(_ubo(camera)), width, height, x, y, C.byref(h)))
        return np.frombuffer(bytes(h), dtype=HIT_DTYPE)[0]

    # --- denoiser (include/rtamd.h "denoise") ---
    @staticmethod
    def denoise_workspace_bytes(width: int, height: int) -> int:
        """Bytes of denoise_device's workspace (rt_denoise_workspace_bytes)."""
        return lib().rt_denoise_workspace_bytes(width, height)

    def denoise_device(self, width: int, height: int, d_radiance: int, d_hits: int, d_workspace: int,
                       d_out_rgba: Optional[int] = None, d_out_radiance: Optional[int] = None,
                       params: Optional[DenoiseParams] = None, stream: Optional[int] = None, ms: bool = False,
                       d_albedo: int = 0):
        """Enqueue the edge-avoiding filter of one whole frame between device
        buffers (raw device pointers; rt_denoise_device) on a HIP stream
        handle; asynchronous unless ms, which waits and returns the passes'
        device time in milliseconds.  A non-zero d_albedo (albedo_device's
        buffer) filters the illumination instead (rt_denoise_albedo_device)."""
        t = C.c_double() if ms else None
        q = C.byref(params) if params is not None else None
        if d_albedo:
            check(lib().rt_denoise_albedo_device(self._ctx, width, height, d_radiance, d_hits, d_albedo, q, d_workspace,
                                                 d_out_rgba, d_out_radiance, stream,
                                                 C.byref(t) if t is not None else None))
        else:
            check(lib().rt_denoise_device(self._ctx, width, height, d_radiance, d_hits, q, d_workspace, d_out_rgba,
                                          d_out_radiance, stream, C.byref(t) if t is not None else None))
        return t.value if t is not None else None

    def denoise(self, radiance, hits, params: Optional[DenoiseParams] = None, albedo=None):
        """The filter on host arrays: radiance float32 [H, W, 3] (render()'s)
        and HIT_DTYPE records [H, W] (render_hits()'s) in, (rgba uint8
        [H, W, 4], radiance float32 [H, W, 3]) out.  With albedo (float32
        [H, W, 4], albedo()'s) the illumination is filtered."""
        import torch
        rad = np.ascontiguousarray(radiance, dtype=np.float32)
        h, w = rad.shape[:2]
        hit = np.ascontiguousarray(hits, dtype=HIT_DTYPE).reshape(h, w)
        with torch.cuda.device(self.device_ids[0]):
            d_rad = torch.from_numpy(rad).cuda()
            d_hit = torch.from_numpy(hit.view(np.float32).reshape(h, w, 8)).cuda()
            d_alb = None
            if albedo is not None:
                d_alb = torch.from_numpy(np.ascontiguousarray(albedo, dtype=np.float32).reshape(h, w, 4)).cuda()
            d_ws = torch.empty((2, h, w, 4), dtype=torch.float32, device="cuda")
            o_rgba = torch.empty((h, w, 4), dtype=torch.uint8, device="cuda")
            o_rad = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
            self.denoise_device(w, h, d_rad.data_ptr(), d_hit.data_ptr(), d_ws.data_ptr(), o_rgba.data_ptr(),
                                o_rad.data_ptr(), params, torch.cuda.current_stream().cuda_stream,
                                d_albedo=d_alb.data_ptr() if d_alb is not None else 0)
            return o_rgba.cpu().numpy(), o_rad.cpu().numpy()

    def albedo_device(self, width: int, height: int, d_hits: int, d_albedo: int, stream: Optional[int] = 0,
                      ms: bool = False):
        """Enqueue the first-hit albedo buffer of a frame's hit records between
        device buffers (raw 16-byte aligned device pointers; rt_albedo_device)
        on a HIP stream handle: 4 floats per pixel, (d.rgb, type), (1, 1, 1,
        -1) without a hit.  Asynchronous unless ms, which waits and returns the
        kernel's device time in milliseconds."""
        t = C.c_double() if ms else None
        check(lib().rt_albedo_device(self._ctx, width, height, d_hits, d_albedo, stream,
                                     C.byref(t) if t is not None else None))
        return t.value if t is not None else None

    def albedo(self, hits) -> np.ndarray:
        """The albedo buffer of HIT_DTYPE records [H, W] (render_hits()'s) on
        host arrays: float32 [H, W, 4]."""
        import torch
        hit = np.ascontiguousarray(hits, dtype=HIT_DTYPE)
        h, w = hit.shape
        with torch.cuda.device(self.device_ids[0]):
            d_hit = torch.from_numpy(hit.view(np.float32).reshape(h, w, 8)).cuda()
            d_alb = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
            self.albedo_device(w, h, d_hit.data_ptr(), d_alb.data_ptr(), torch.cuda.current_stream().cuda_stream)
            return d_alb.cpu().numpy()

    def render_denoised(self, camera, width: int, height: int, max_bounces: int = REFERENCE_MAX_BOUNCES,
                        params: Optional[DenoiseParams] = None, radiance: bool = False, stats: bool = False):
        """render() followed by the filter (rt_render_denoised): (rgba, radiance
        or None, stats dict or None); stats are the render's, ms with the
        filter's time added.  One device, no active spheres."""
        rgba = np.empty((height, width, 4), dtype=np.uint8)
        rad = np.empty((height, width, 3), dtype=np.float32) if radiance else None
        st = Stats() if stats else None
        check(lib().rt_render_denoised(self._ctx, C.byref(_ubo(camera)), width, height, max_bounces,
                                       C.byref(params) if params is not None else None, rgba.ctypes.data,
                                       rad.ctypes.data if rad is not None else None,
                                       C.byref(st) if st is not None else None))
        return rgba, rad, (st.as_dict() if st is not None else None)

    def denoise_history_device(self, width: int, height: int, d_hist: int, d_hits: int, d_workspace: int,
                               d_out_rgba: Optional[int] = None, d_out_radiance: Optional[int] = None,
                               params: Optional[DenoiseParams] = None, stream: Optional[int] = None,
                               ms: bool = False):
        """Enqueue the history-adaptive filter of one whole frame between
        device buffers (raw device pointers; rt_denoise_history_device,
        DESIGN.md §4i) on a HIP stream handle: d_hist is a history buffer as
        temporal_device writes it (never written), the workspace is
        denoise_workspace_bytes bytes.  Asynchronous unless ms, which waits and
        returns the passes' device time in milliseconds."""
        t = C.c_double() if ms else None
        check(lib().rt_denoise_history_device(self._ctx, width, height, d_hist, d_hits,
                                              C.byref(params) if params is not None else None, d_workspace,
                                              d_out_rgba, d_out_radiance, stream,
                                              C.byref(t) if t is not None else None))
        return t.value if t is not None else None

    # --- temporal accumulation (include/rtamd.h "temporal") ---
    def temporal_device(self, width: int, height: int, camera, d_radiance: int, d_hits: int, d_hist_out: int,
                        prev_camera=None, d_hist_prev: Optional[int] = None, d_hits_prev: Optional[int] = None,
                        d_out_rgba: Optional[int] = None, d_out_radiance: Optional[int] = None,
                        params: Optional[TemporalParams] = None, stream: Optional[int] = None, ms: bool = False):
        """Enqueue one frame of the accumulation between device buffers (raw
        device pointers; rt_temporal_device) on a HIP stream handle: the new
        frame's radiance, hit records and camera, the previous frame's camera,
        history and hit records (all None: a first frame), the new history and
        the optional display outputs.  Asynchronous unless ms, which waits and
        returns the kernel's device time in milliseconds."""
        t = C.c_double() if ms else None
        check(lib().rt_temporal_device(self._ctx, width, height, C.byref(_ubo(camera)) if camera is not None else None,
                                       d_radiance, d_hits,
                                       C.byref(_ubo(prev_camera)) if prev_camera is not None else None, d_hist_prev,
                                       d_hits_prev, C.byref(params) if params is not None else None, d_hist_out,
                                       d_out_rgba, d_out_radiance, stream, C.byref(t) if t is not None else None))
        return t.value if t is not None else None

    def temporal_moments_device(self, width: int, height: int, camera, d_radiance: int, d_hits: int, d_hist_out: int,
                                d_mom_out: int, prev_camera=None, d_hist_prev: Optional[int] = None,
                                d_hits_prev: Optional[int] = None, d_mom_prev: Optional[int] = None,
                                d_out_rgba: Optional[int] = None, d_out_radiance: Optional[int] = None,
                                params: Optional[TemporalParams] = None, stream: Optional[int] = None,
                                ms: bool = False):
        """temporal_device with luminance moments (rt_temporal_moments_device,
        DESIGN.md §4j): d_mom_out receives (m1, m2) per pixel, 8 bytes each;
        d_mom_prev is the previous frame's, None exactly when the other
        previous-frame inputs are.  The history and the display outputs are
        temporal_device's bit for bit."""
        t = C.c_double() if ms else None
        check(lib().rt_temporal_moments_device(
            self._ctx, width, height, C.byref(_ubo(camera)) if camera is not None else None, d_radiance, d_hits,
            C.byref(_ubo(prev_camera)) if prev_camera is not None else None, d_hist_prev, d_hits_prev,
            C.byref(params) if params is not None else None, d_hist_out, d_out_rgba, d_out_radiance, stream,
            C.byref(t) if t is not None else None, d_mom_prev, d_mom_out))
        return t.value if t is not None else None

    def temporal_motion_device(self, width: int, height: int, camera, d_radiance: int, d_hits: int, d_hist_out: int,
                               prev_camera=None, d_hist_prev: Optional[int] = None, d_hits_prev: Optional[int] = None,
                               d_verts_cur: Optional[int] = None, d_verts_prev: Optional[int] = None, n_tris: int = 0,
                               d_mom_prev: Optional[int] = None, d_mom_out: Optional[int] = None,
                               d_out_rgba: Optional[int] = None, d_out_radiance: Optional[int] = None,
                               params: Optional[TemporalParams] = None, stream: Optional[int] = None,
                               ms: bool = False):
        """temporal_device across a geometry update (rt_temporal_motion_device,
        DESIGN.md §4m): d_verts_cur and d_verts_prev are the vertex records (48
        bytes per flattened triangle) as the new and the previous frame's hit
        records saw them, n_tris the triangles both hold; the history is
        gathered where each pixel's point of its triangle lay before the
        update.  Both None: temporal_device, or with the moments buffers
        temporal_moments_device, bit for bit."""
        t = C.c_double() if ms else None
        check(lib().rt_temporal_motion_device(
            self._ctx, width, height, C.byref(_ubo(camera)) if camera is not None else None, d_radiance, d_hits,
            C.byref(_ubo(prev_camera)) if prev_camera is not None else None, d_hist_prev, d_hits_prev,
            C.byref(params) if params is not None else None, d_hist_out, d_out_rgba, d_out_radiance, stream,
            C.byref(t) if t is not None else None, d_mom_prev, d_mom_out, d_verts_cur, d_verts_prev, n_tris))
        return t.value if t is not None else None

    def denoise_variance_device(self, width: int, height: int, d_hist: int, d_mom: int, d_hits: int, d_workspace: int,
                                d_out_rgba: Optional[int] = None, d_out_radiance: Optional[int] = None,
                                params: Optional[VarianceParams] = None, stream: Optional[int] = None,
                                ms: bool = False):
        """Enqueue the variance-guided filter of one whole frame between device
        buffers (raw device pointers; rt_denoise_variance_device, DESIGN.md
        §4j) on a HIP stream handle: d_hist and d_mom as
        temporal_moments_device writes them (never written), the workspace is
        denoise_workspace_bytes bytes.  Asynchronous unless ms, which waits and
        returns the device time of the estimate and the passes in milliseconds."""
        t = C.c_double() if ms else None
        check(lib().rt_denoise_variance_device(self._ctx, width, height, d_hist, d_mom, d_hits,
                                               C.byref(params) if params is not None else None, d_workspace,
                                               d_out_rgba, d_out_radiance, stream,
                                               C.byref(t) if t is not None else None))
        return t.value if t is not None else None

    def temporal(self, radiance, hits, camera, prev_camera=None, hist_prev=None, hits_prev=None,
                 params: Optional[TemporalParams] = None):
        """The accumulation on host arrays: radiance float32 [H, W, 3] and
        HIT_DTYPE records [H, W] of the new frame and its camera; the previous
        frame's camera, history float32 [H, W, 4] and hit records, or None for
        a first frame.  Returns (history float32 [H, W, 4], rgba uint8
        [H, W, 4], radiance float32 [H, W, 3])."""
        import torch
        rad = np.ascontiguousarray(radiance, dtype=np.float32)
        h, w = rad.shape[:2]
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.float32).reshape(h, w, -1)).cuda()  # noqa: E731
        with torch.cuda.device(self.device_ids[0]):
            d_rad = torch.from_numpy(rad).cuda()
            d_hit = dev(np.ascontiguousarray(hits, dtype=HIT_DTYPE))
            d_hp = dev(np.ascontiguousarray(hist_prev, dtype=np.float32)) if hist_prev is not None else None
            d_hq = dev(np.ascontiguousarray(hits_prev, dtype=HIT_DTYPE)) if hits_prev is not None else None
            o_hist = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
            o_rgba = torch.empty((h, w, 4), dtype=torch.uint8, device="cuda")
            o_rad = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
            self.temporal_device(w, h, camera, d_rad.data_ptr(), d_hit.data_ptr(), o_hist.data_ptr(), prev_camera,
                                 d_hp.data_ptr() if d_hp is not None else None,
                                 d_hq.data_ptr() if d_hq is not None else None, o_rgba.data_ptr(), o_rad.data_ptr(),
                                 params, torch.cuda.current_stream().cuda_stream)
            return o_hist.cpu().numpy(), o_rgba.cpu().numpy(), o_rad.cpu().numpy()

    def render_temporal(self, camera, width: int, height: int, max_bounces: int = REFERENCE_MAX_BOUNCES,
                        params: Optional[TemporalParams] = None, denoise: Optional[DenoiseParams] = None,
                        reset: bool = False, fixed_seed: bool = False, radiance: bool = False, stats: bool = False,
                        adaptive: bool = False, variance=None):
        """One frame of a temporally accumulated sequence (rt_render_temporal):
        render with a new sample per camera.frame_count (fixed_seed: the
        context's extensions as they are), first-hit buffer, reprojection of
        the context's history of the previous call, and with `denoise` the
        spatial filter after it.  adaptive: the history-adaptive filter runs on
        the new history record instead (rt_render_temporal_adaptive; `denoise`
        None = its defaults); the two kinds of call share one history.
        variance (True = the defaults, or a VarianceParams): the
        variance-guided filter on a history with luminance moments instead
        (rt_render_temporal_variance; not with `denoise` or
        adaptive); a call after one of the other kinds starts a new sequence.
        reset drops the history first.  Returns
        (rgba, radiance or None, stats dict or None); ms = render + temporal
        (+ filter).  One device, no active spheres, extensions bit 4 off."""
        rgba = np.empty((height, width, 4), dtype=np.uint8)
        rad = np.empty((height, width, 3), dtype=np.float32) if radiance else None
        st = Stats() if stats else None
        flags = (RT_TEMPORAL_RESET if reset else 0) | (RT_TEMPORAL_FIXED_SEED if fixed_seed else 0)
        if variance is not None and variance is not False:
            if adaptive or denoise is not None:
                raise ValueError("render_temporal: variance excludes adaptive and denoise")
            call, denoise = lib().rt_render_temporal_variance, (None if variance is True else variance)
        else:
            call = lib().rt_render_temporal_adaptive if adaptive else lib().rt_render_temporal
        check(call(self._ctx, C.byref(_ubo(camera)), width, height, max_bounces,
                   C.byref(params) if params is not None else None,
                   C.byref(denoise) if denoise is not None else None, flags, rgba.ctypes.data,
                   rad.ctypes.data if rad is not None else None, C.byref(st) if st is not None else None))
        return rgba, rad, (st.as_dict() if st is not None else None)

    # --- samples (include/rtamd.h "samples") ---
    @staticmethod
    def samples_workspace_bytes(width: int, height: int, frames: int) -> int:
        """Bytes of render_samples_device's workspace for `frames` sample
        frames per launch (rt_samples_workspace_bytes; 0 for bad arguments)."""
        return lib().rt_samples_workspace_bytes(width, height, frames)

    def render_samples_device(self, camera, width: int, height: int, max_bounces: int, n_samples: int,
                              d_workspace: Optional[int], workspace_bytes: int, d_sum: Optional[int],
                              d_out_rgba: Optional[int] = None, d_out_radiance: Optional[int] = None,
                              stream: Optional[int] = None, stats: bool = False):
        """Enqueue samples camera.frame_count .. + n_samples - 1 of one whole
        frame and their resolve between device buffers (raw device pointers;
        rt_render_samples_device) on a HIP stream handle: d_sum keeps the
        running sum of the linear colour (overwritten when frame_count is 0,
        continued otherwise), the outputs receive sqrt(sum / samples) as
        extension bit 4 would show it.  Asynchronous unless stats (the totals
        over the samples)."""
        st = Stats() if stats else None
        check(lib().rt_render_samples_device(self._ctx, C.byref(_ubo(camera)), width, height, max_bounces, n_samples,
                                             d_workspace, workspace_bytes, d_sum, d_out_rgba, d_out_radiance, stream,
                                             C.byref(st) if st is not None else None))
        return st.as_dict() if st is not None else None

    def render_samples(self, camera, width: int, height: int, max_bounces: int = REFERENCE_MAX_BOUNCES,
                       n_samples: int = 1, radiance: bool = False, stats: bool = False):
        """n_samples samples per pixel in one call (rt_render_samples), into the
        context's own sum: camera.frame_count 0 starts it over, k > 0 continues
        a sum of exactly k samples.  Returns (rgba, radiance or None, stats
        dict or None).  One device, extensions bit 4 off."""
        rgba = np.empty((height, width, 4), dtype=np.uint8)
        rad = np.empty((height, width, 3), dtype=np.float32) if radiance else None
        st = Stats() if stats else None
        check(lib().rt_render_samples(self._ctx, C.byref(_ubo(camera)), width, height, max_bounces, n_samples,
                                      rgba.ctypes.data, rad.ctypes.data if rad is not None else None,
                                      C.byref(st) if st is not None else None))
        return rgba, rad, (st.as_dict() if st is not None else None)

    # --- heavy-first learning diagnostics (include/rtamd.h rt_learn_device, rt_learn_copy) ---
    def learn_device(self, d_records: int, d_lanes: int, n_tiles: int, d_order: int, d_mask: int, d_hpix: int,
                     d_count: int, stream: Optional[int] = None, **params) -> None:
        """The device learning on a caller's device buffers (raw pointers;
        rt_learn_device): params are rt_learn_params's fields.  Waits for the
        stream."""
        lp = LearnParams(**params)
        check(lib().rt_learn_device(self._ctx, d_records, d_lanes, n_tiles, C.byref(lp), d_order, d_mask, d_hpix,
                                    d_count, stream))

    def learn_copy(self, records: bool = True) -> dict:
        """The newest learned order of device 0 (rt_learn_copy): a dict of
        rt_learn_info's fields, with params flattened into it, and the arrays
        order, mask, hpix and, with records while they are resident, the
        learning launch's records [n, 8] and lanes [64 n].  Not for timing runs."""
        info = LearnInfo()
        check(lib().rt_learn_copy(self._ctx, C.byref(info), None, None, None, None, None))
        n = info.n_tiles
        out = {k: getattr(info, k) for k, _ in LearnInfo._fields_ if k != "params"}
        out.update({k: getattr(info.params, k) for k, _ in LearnParams._fields_ if k != "reserved"})
        order, mask = np.empty(n, np.int32), np.empty(n, np.uint64)
        hpix = np.empty(info.n_hpix, np.int32)
        rec = lanes = None
        if records and info.records_resident:
            rec, lanes = np.empty((n, 8), np.uint64), np.empty(64 * n, np.uint32)
        check(lib().rt_learn_copy(self._ctx, C.byref(info), order.ctypes.data, mask.ctypes.data, hpix.ctypes.data,
                                  rec.ctypes.data if rec is not None else None,
                                  lanes.ctypes.data if lanes is not None else None))
        out.update(order=order, mask=mask, hpix=hpix, records=rec, lanes=lanes)
        return out

    # --- option rng_table's table (include/rtamd.h rt_rng_table_copy) ---
    def rng_table_copy(self):
        """Device 0's table of scatter draws as (words, width, height, k): words
        is uint32 [k, height, width, 4], a float's bits in .x .y .z and the seed
        in .w; (None, 0, 0, 0) when the device holds none.  Not for timing runs."""
        w, h, k = C.c_int32(), C.c_int32(), C.c_int32()
        check(lib().rt_rng_table_copy(self._ctx, None, 0, C.byref(w), C.byref(h), C.byref(k)))
        if k.value == 0:
            return None, 0, 0, 0
        words = np.empty((k.value, h.value, w.value, 4), np.uint32)
        check(lib().rt_rng_table_copy(self._ctx, words.ctypes.data, words.nbytes, None, None, None))
        return words, w.value, h.value, k.value


class PinnedFrame:
    """An RGBA8 frame in pinned host memory (rt_host_alloc), as a numpy view."""

    def __init__(self, height: int, width: int):
        n = height * width * 4
        self.ptr = lib().rt_host_alloc(n)
        if not self.ptr:
            raise RtError(-6, lib().rt_last_error().decode())   # RT_ERR_OOM
        self.array = np.ctypeslib.as_array((C.c_uint8 * n).from_address(self.ptr)).reshape(height, width, 4)
        self.shape = self.array.shape

    def close(self) -> None:
        if self.ptr:
            self.array = None
            lib().rt_host_free(self.ptr)
            self.ptr = None

    def __del__(self):
        self.close()


@dataclass
class FrameData:
    """FrameData.java: RGBA8 pixels of one frame, row 0 = top."""
    pixel_data: np.ndarray
    stats: Optional[dict] = None


class AtomicReference:
    """The java.util.concurrent.atomic.AtomicReference the UI shares with the engine."""

    def __init__(self, value=None):
        self._v = value
        self._lock = threading.Lock()

    def set(self, v) -> None:
        with self._lock:
            self._v = v

    def get(self):
        with self._lock:
            return self._v

    def get_and_set(self, v):
        with self._lock:
            old, self._v = self._v, v
            return old


class HipEngine:
    """Drop-in for VulkanEngine: same public methods, a render thread that owns
    the rt_ctx (single-thread affinity, VulkanEngine.java:194-206)."""

    def __init__(self, frame_queue: AtomicReference, width: int = REFERENCE_WIDTH,
                 height: int = REFERENCE_HEIGHT, max_bounces: int = REFERENCE_MAX_BOUNCES,
                 device_ids: Sequence[int] = (0,), collect_stats: bool = False, pipelined: bool = True,
                 inflight: int = 4, denoise: Optional[DenoiseParams] = None,
                 temporal: Optional[TemporalParams] = None, adaptive: bool = False, variance=None,
                 motion: bool = False):
        self.frame_queue = frame_queue
        # pipelined: `inflight` frames in flight (rt_render_async, one slot and
        # trace stream each), so the frames' traces overlap each other and
        # their readbacks; the reference waits for each frame
        # (VulkanEngine.java:410-429).  Stats need the synchronous path.
        # denoise: every frame goes through render_denoised, which is synchronous.
        # temporal: every frame goes through render_temporal (synchronous as well), frame k of the
        # engine with frame_count k, so that every frame is a new sample; with denoise too, the
        # filter runs after the accumulation.
        # adaptive: the temporal path with the history-adaptive filter (render_temporal's adaptive=;
        # temporal None = the default parameters, denoise = the filter's parameters or None for its defaults).
        # variance (True or a VarianceParams): the temporal path with the variance-guided filter
        # (render_temporal's variance=; temporal None = the default parameters).
        # motion: scenes are uploaded with options refit and temporal_motion 1, so that a geometry update
        # (submit_geometry_update) keeps the temporal history and the next frame reprojects it per triangle;
        # refit_device 1 as well, so that the update may come as a tensor on the device.
        self.motion = bool(motion)
        self.denoise = denoise
        self.variance = None if variance is False else variance
        self.temporal = TemporalParams() if (adaptive or self.variance is not None) and temporal is None else temporal
        self.adaptive = bool(adaptive)
        self.temporal_frames = 0
        self.geometry_updates = 0
        self.pipelined = pipelined and not collect_stats and denoise is None and self.temporal is None
        self.inflight = max(1, min(8, int(inflight)))
        self.width, self.height, self.max_bounces = width, height, max_bounces
        self.device_ids = tuple(device_ids)
        self.collect_stats = collect_stats
        self._scene_q: "queue.Queue[tuple]" = queue.Queue()     # (BuiltCpuData, True for a geometry update)
        self._camera_q: "queue.Queue[Camera]" = queue.Queue()
        self._sky_q: "queue.Queue[bool]" = queue.Queue()
        self._running = False
        self._thread = threading.Thread(target=self._run, name="HIP-Engine-Thread", daemon=True)
        self.is_sky_enabled = 1
        self.frames_rendered = 0
        self.frames_submitted = 0
        self.error: Optional[BaseException] = None

    # --- public API (UI thread) ---
    def start(self) -> None:
        self._running = True
        self._thread.start()

    def stop(self) -> None:
        self._running = False
        self._thread.join(5.0)          # 5 s graceful window, VulkanEngine.java:145

    def submit_scene(self, scene_data: BuiltCpuData) -> None:
        self._scene_q.put((scene_data, False))

    def submit_geometry_update(self, built, source=None) -> None:
        """The current scene's triangles moved (rtamd.refit_buffers of the
        submitted scene): queued like a scene and applied on the render thread
        through Renderer.update_geometry, after the frames in flight.  The
        engine must have been made with motion=True, which uploads scenes with
        the refit tables.  built may also be a torch tensor of the moved input
        triangles on the engine's device (with source, the scene's flat_source
        as an int32 tensor there, or None for flattened order): applied
        through Renderer.update_geometry_device; the caller keeps both tensors
        unchanged until the update has been applied (geometry_updates)."""
        self._scene_q.put((built if isinstance(built, BuiltCpuData) else (built, source), True))

    def submit_camera_update(self, camera: Camera) -> None:
        self._camera_q.put(camera)

    def submit_sky_toggle(self, is_sky_on: bool) -> None:
        self._sky_q.put(bool(is_sky_on))

    # --- render thread ---
    def _run(self) -> None:
        renderer = None
        slots, pending = None, []
        try:
            renderer = Renderer(self.device_ids)
            renderer.set_option("async_slots", self.inflight)
            if self.motion:
                renderer.set_option("refit", 1)
                renderer.set_option("refit_device", 1)
                renderer.set_option("temporal_motion", 1)
            have_scene, camera = False, None
            while self._running:
                try:                                        # one scene per pass (:281-285)
                    scene, update = self._scene_q.get_nowait()
                    while pending:                          # frames of the old scene first
                        self._finish(renderer, slots, pending.pop(0))
                    if update:
                        if isinstance(scene, BuiltCpuData):
                            renderer.update_geometry(scene)
                        else:
                            renderer.update_geometry_device(*scene)
                        self.geometry_updates += 1
                    else:
                        renderer.upload_scene(scene)
                        have_scene = True
                except queue.Empty:
                    pass
                while True:                                 # drain to the latest camera (:288-298)
                    try:
                        camera = self._camera_q.get_nowait()
                    except queue.Empty:
                        break
                while True:                                 # latest sky state (:300-312)
                    try:
                        self.is_sky_enabled = 1 if self._sky_q.get_nowait() else 0
                    except queue.Empty:
                        break
                if not have_scene or camera is None:
                    time.sleep(0.016)
                    continue
                ubo = CameraUBO.from_buffer_copy(bytes(camera.ubo))
                ubo.sky_enabled = self.is_sky_enabled        # written, ignored by the shader
                if not self.pipelined:
                    if self.temporal is not None:
                        ubo.frame_count = self.temporal_frames
                        rgba, _, st = renderer.render_temporal(ubo, self.width, self.height, self.max_bounces,
                                                               self.temporal, self.denoise, stats=self.collect_stats,
                                                               adaptive=self.adaptive, variance=self.variance)
                        self.temporal_frames += 1
                    elif self.denoise is not None:
                        rgba, _, st = renderer.render_denoised(ubo, self.width, self.height, self.max_bounces,
                                                               self.denoise, stats=self.collect_stats)
                    else:
                        rgba, _, st = renderer.render(ubo, self.width, self.height, self.max_bounces,
                                                      stats=self.collect_stats)
                    self._publish(FrameData(rgba, st))
                    continue
                if slots is None:
                    slots = [PinnedFrame(self.height, self.width) for _ in range(self.inflight)]
                k = self.frames_submitted % self.inflight
                pending.append((renderer.render_async(ubo, self.width, self.height, self.max_bounces, slots[k]), k))
                self.frames_submitted += 1
                if len(pending) == self.inflight:
                    self._finish(renderer, slots, pending.pop(0))
            while pending:                                  # drain on stop
                self._finish(renderer, slots, pending.pop(0))
        except BaseException as e:                          # FATAL (VRT) path, :197-201
            self.error = e
            self._running = False
        finally:
            if renderer is not None:
                renderer.close()
            for f in slots or ():
                f.close()

    def _finish(self, renderer, slots, item) -> None:
        ticket, k = item
        renderer.wait(ticket)
        # a fresh buffer per frame, as the reference publishes (:416-429)
        self._publish(FrameData(slots[k].array.copy()))

    def _publish(self, frame: "FrameData") -> None:
        self.frame_queue.set(frame)
        self.frames_rendered += 1
