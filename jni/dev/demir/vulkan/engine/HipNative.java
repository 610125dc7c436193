package dev.demir.vulkan.engine;

import java.nio.ByteBuffer;

/** JNI entry points of jni/HipNative.c over librtamd.so (include/rtamd.h). */
final class HipNative {
    static { System.loadLibrary("hipnative"); }
    static native long create(int[] deviceIds);
    static native void uploadScene(long ctx, ByteBuffer v, long vBytes, ByteBuffer m, long mBytes,
                                   ByteBuffer bvh, long bvhBytes);
    static native void render(long ctx, ByteBuffer ubo80, int w, int h, int maxBounces, ByteBuffer outRgba);
    static native void destroy(long ctx);
    static native ByteBuffer allocFrame(long bytes);            // pinned (rt_host_alloc)
    static native void freeFrame(ByteBuffer frame);
    static native long renderAsync(long ctx, ByteBuffer ubo80, int w, int h, int maxBounces, ByteBuffer pinnedOut);
    static native void waitFrame(long ctx, long ticket);
    static native boolean pollFrame(long ctx, long ticket);       // rt_render_poll: never blocks
    static native void uploadSpheres(long ctx, float[] spheres8n);   // extension (option "extensions" bit 8)
    static native void setOption(long ctx, String name, long value);
    static native long getOption(long ctx, String name);
    /** rt_pick: the hit record of pixel (x, y) into outHit (direct, >= 32 bytes, native order: float t, int tri,
     *  float normal[3], float pos[3]); tri < 0 = nothing hit.  On the thread that owns ctx. */
    static native void pick(long ctx, ByteBuffer ubo80, int w, int h, int x, int y, ByteBuffer outHit);
    /** rt_render_denoised: one frame rendered and filtered by the edge-avoiding denoiser (rt_denoise_params:
     *  defaults 4, 7, 0.005f, 0.5f) into outRgba (direct, >= w * h * 4 bytes).  Synchronous; on the thread that
     *  owns ctx; one device, no active spheres. */
    static native void renderDenoised(long ctx, ByteBuffer ubo80, int w, int h, int maxBounces, int iterations,
                                      int normalPowerLog2, float sigmaDepth, float sigmaColor, ByteBuffer outRgba);
    /** rt_render_temporal: one frame of a temporally accumulated sequence (rt_temporal_params: defaults 32, 0.005f,
     *  0.9f) into outRgba (direct, >= w * h * 4 bytes); the caller advances the UBO's frame_count per frame.
     *  filterIterations 0 = no spatial filter, 1..6 = the denoiser's defaults with that many passes; flags: 1 = drop
     *  the history first, 2 = keep the context's extensions (no new sample per frame).  Synchronous; on the thread
     *  that owns ctx; one device, no active spheres, extensions bit 4 off. */
    static native void renderTemporal(long ctx, ByteBuffer ubo80, int w, int h, int maxBounces, int maxHistory,
                                      float planeTol, float normalMin, int filterIterations, int flags,
                                      ByteBuffer outRgba);
    /** rt_update_geometry: the uploaded scene's triangles moved, in the tree it was uploaded with (the upload must
     *  follow setOption(ctx, "refit", 1)).  Direct buffers whose capacities are the byte sizes: the moved vertex
     *  records in the uploaded order, and the uploaded nodes with new boxes (rt_refit_scene writes both).
     *  Synchronous; on the thread that owns ctx. */
    static native void updateGeometry(long ctx, ByteBuffer vertices, ByteBuffer nodes);
}
