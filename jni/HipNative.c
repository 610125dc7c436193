/*
 * HipNative.c — JNI shim between the Java host (dev.demir.vulkan.engine.HipEngine)
 * and the C ABI of librtamd.so (include/rtamd.h).  It replaces the LWJGL-Vulkan
 * calls VulkanEngine makes for the render path (VulkanEngine.java:120-185,
 * 318-431): direct buffers go to the C ABI as plain pointers, a non-zero
 * status becomes a RuntimeException carrying rt_last_error(), as the
 * reference's Vulkan errors are (e.g. VulkanEngine.java:596-598).
 *
 * Build (a host with a JDK; none exists in this repo's build image):
 *   make -C jni JAVA_HOME=/path/to/jdk
 */
#include <jni.h>
#include <stdint.h>
#include <stdio.h>
#include "rtamd.h"

static void throw_rt(JNIEnv* env, int rc) {
    jclass ex = (*env)->FindClass(env, "java/lang/RuntimeException");
    char msg[1200];
    snprintf(msg, sizeof msg, "rtamd error %d: %s", rc, rt_last_error());
    (*env)->ThrowNew(env, ex, msg);
}

/* long create(int[] deviceIds) */
JNIEXPORT jlong JNICALL Java_dev_demir_vulkan_engine_HipNative_create(JNIEnv* env, jclass c, jintArray ids) {
    /* the library must have this shim's struct layouts (rtamd.h RT_ABI_VERSION) */
    size_t sb = 0, cb = 0;
    if (rt_abi_version(&sb, &cb) != RT_ABI_VERSION || sb != sizeof(rt_stats) || cb != sizeof(rt_camera_ubo)) {
        jclass ex = (*env)->FindClass(env, "java/lang/RuntimeException");
        if (ex) (*env)->ThrowNew(env, ex, "librtamd ABI version differs from the shim's (include/rtamd.h)");
        return 0;
    }
    jsize n = (*env)->GetArrayLength(env, ids);
    jint* p = (*env)->GetIntArrayElements(env, ids, NULL);
    rt_ctx* ctx = NULL;
    int rc = rt_create((const int*)p, (int)n, &ctx);
    (*env)->ReleaseIntArrayElements(env, ids, p, JNI_ABORT);
    if (rc) { throw_rt(env, rc); return 0; }
    return (jlong)(intptr_t)ctx;
}

/* void uploadScene(long ctx, ByteBuffer v, long vBytes, ByteBuffer m, long mBytes, ByteBuffer bvh, long bvhBytes)
 * Direct buffers only (LWJGL memAllocFloat / ByteBuffer.allocateDirect, as SceneBuilder makes them).
 * Byte counts are remaining()*4 / remaining(), as VulkanEngine.java:337,345,353 computes them. */
JNIEXPORT void JNICALL Java_dev_demir_vulkan_engine_HipNative_uploadScene(JNIEnv* env, jclass c, jlong ctx,
        jobject v, jlong vb, jobject m, jlong mb, jobject bvh, jlong bb) {
    int rc = rt_upload_scene((rt_ctx*)(intptr_t)ctx,
                             (*env)->GetDirectBufferAddress(env, v), (size_t)vb,
                             (*env)->GetDirectBufferAddress(env, m), (size_t)mb,
                             (*env)->GetDirectBufferAddress(env, bvh), (size_t)bb);
    if (rc) throw_rt(env, rc);
}

/* void render(long ctx, ByteBuffer ubo80, int w, int h, int maxBounces, ByteBuffer outRgba) */
JNIEXPORT void JNICALL Java_dev_demir_vulkan_engine_HipNative_render(JNIEnv* env, jclass c, jlong ctx,
        jobject ubo, jint w, jint h, jint maxBounces, jobject out) {
    int rc = rt_render((rt_ctx*)(intptr_t)ctx, (const rt_camera_ubo*)(*env)->GetDirectBufferAddress(env, ubo),
                       w, h, maxBounces, (uint8_t*)(*env)->GetDirectBufferAddress(env, out), NULL, NULL);
    if (rc) throw_rt(env, rc);
}

/* Pipelined frames: pinned frame buffers the copy stream writes asynchronously. */
JNIEXPORT jobject JNICALL Java_dev_demir_vulkan_engine_HipNative_allocFrame(JNIEnv* env, jclass c, jlong bytes) {
    void* p = rt_host_alloc((size_t)bytes);
    if (!p) { throw_rt(env, RT_ERR_OOM); return NULL; }
    return (*env)->NewDirectByteBuffer(env, p, bytes);
}
JNIEXPORT void JNICALL Java_dev_demir_vulkan_engine_HipNative_freeFrame(JNIEnv* env, jclass c, jobject buf) {
    rt_host_free((*env)->GetDirectBufferAddress(env, buf));
}
/* long renderAsync(long ctx, ByteBuffer ubo80, int w, int h, int maxBounces, ByteBuffer pinnedOut) */
JNIEXPORT jlong JNICALL Java_dev_demir_vulkan_engine_HipNative_renderAsync(JNIEnv* env, jclass c, jlong ctx,
        jobject ubo, jint w, jint h, jint maxBounces, jobject out) {
    uint64_t t = 0;
    int rc = rt_render_async((rt_ctx*)(intptr_t)ctx, (const rt_camera_ubo*)(*env)->GetDirectBufferAddress(env, ubo),
                             w, h, maxBounces, (uint8_t*)(*env)->GetDirectBufferAddress(env, out), &t);
    if (rc) throw_rt(env, rc);
    return (jlong)t;
}
JNIEXPORT void JNICALL Java_dev_demir_vulkan_engine_HipNative_waitFrame(JNIEnv* env, jclass c, jlong ctx, jlong t) {
    int rc = rt_render_wait((rt_ctx*)(intptr_t)ctx, (uint64_t)t);
    if (rc) throw_rt(env, rc);
}
/* boolean pollFrame(long ctx, long ticket): true when the frame is complete (never blocks) */
JNIEXPORT jboolean JNICALL Java_dev_demir_vulkan_engine_HipNative_pollFrame(JNIEnv* env, jclass c, jlong ctx, jlong t) {
    int done = 0;
    int rc = rt_render_poll((rt_ctx*)(intptr_t)ctx, (uint64_t)t, &done);
    if (rc) { throw_rt(env, rc); return JNI_FALSE; }
    return done ? JNI_TRUE : JNI_FALSE;
}

/* Extension: void uploadSpheres(long ctx, float[] spheres8n) — centre.xyz, radius, albedo.rgb, type per sphere.
 * Then setOption(ctx, "extensions", 8) turns them on. */
JNIEXPORT void JNICALL Java_dev_demir_vulkan_engine_HipNative_uploadSpheres(JNIEnv* env, jclass c, jlong ctx,
        jfloatArray s) {
    jsize n = (*env)->GetArrayLength(env, s);
    jfloat* p = (*env)->GetFloatArrayElements(env, s, NULL);
    int rc = rt_upload_spheres((rt_ctx*)(intptr_t)ctx, (const float*)p, (int)(n / 8));
    (*env)->ReleaseFloatArrayElements(env, s, p, JNI_ABORT);
    if (rc) throw_rt(env, rc);
}

/* void setOption(long ctx, String name, long value) — schedule and extension options (rtamd.h rt_set_option) */
JNIEXPORT void JNICALL Java_dev_demir_vulkan_engine_HipNative_setOption(JNIEnv* env, jclass c, jlong ctx,
        jstring name, jlong value) {
    const char* n = (*env)->GetStringUTFChars(env, name, NULL);
    int rc = rt_set_option((rt_ctx*)(intptr_t)ctx, n, (int64_t)value);
    (*env)->ReleaseStringUTFChars(env, name, n);
    if (rc) throw_rt(env, rc);
}

/* long getOption(long ctx, String name) — e.g. "queues_short": 1 when the async slots lack hardware queues */
JNIEXPORT jlong JNICALL Java_dev_demir_vulkan_engine_HipNative_getOption(JNIEnv* env, jclass c, jlong ctx,
        jstring name) {
    const char* n = (*env)->GetStringUTFChars(env, name, NULL);
    int64_t v = 0;
    int rc = rt_get_option((rt_ctx*)(intptr_t)ctx, n, &v);
    (*env)->ReleaseStringUTFChars(env, name, n);
    if (rc) throw_rt(env, rc);
    return (jlong)v;
}

/* void pick(long ctx, ByteBuffer ubo80, int w, int h, int x, int y, ByteBuffer outHit32)
 * The hit record of pixel (x, y)'s primary ray (rtamd.h rt_pick, rt_hit: float t, int tri, float normal[3],
 * float pos[3], native byte order) into a direct buffer of at least 32 bytes; tri < 0: nothing under the
 * cursor.  Call it on the thread that owns ctx (the render thread): a context is single-thread-affine. */
JNIEXPORT void JNICALL Java_dev_demir_vulkan_engine_HipNative_pick(JNIEnv* env, jclass c, jlong ctx,
        jobject ubo, jint w, jint h, jint x, jint y, jobject outHit) {
    /* a heap (non-direct) buffer has capacity -1 */
    if (!ubo || !outHit || (*env)->GetDirectBufferCapacity(env, ubo) < (jlong)sizeof(rt_camera_ubo) ||
        (*env)->GetDirectBufferCapacity(env, outHit) < (jlong)sizeof(rt_hit)) {
        jclass ex = (*env)->FindClass(env, "java/lang/RuntimeException");
        if (ex) (*env)->ThrowNew(env, ex, "pick: need direct buffers of >= 80 bytes (camera UBO) and >= 32 bytes (hit)");
        return;
    }
    int rc = rt_pick((rt_ctx*)(intptr_t)ctx, (const rt_camera_ubo*)(*env)->GetDirectBufferAddress(env, ubo),
                     w, h, x, y, (rt_hit*)(*env)->GetDirectBufferAddress(env, outHit));
    if (rc) throw_rt(env, rc);
}

/* void renderDenoised(long ctx, ByteBuffer ubo80, int w, int h, int maxBounces, int iterations, int normalPowerLog2,
 *                     float sigmaDepth, float sigmaColor, ByteBuffer outRgba)
 * One frame rendered and filtered by the edge-avoiding denoiser (rtamd.h rt_render_denoised; the parameters are
 * rt_denoise_params, whose defaults are 4, 7, 0.005f, 0.5f) into a direct buffer of at least w * h * 4 bytes.
 * Synchronous; on the thread that owns ctx. */
JNIEXPORT void JNICALL Java_dev_demir_vulkan_engine_HipNative_renderDenoised(JNIEnv* env, jclass c, jlong ctx,
        jobject ubo, jint w, jint h, jint maxBounces, jint iterations, jint normalPowerLog2, jfloat sigmaDepth,
        jfloat sigmaColor, jobject out) {
    /* a heap (non-direct) buffer has capacity -1; the size check needs a sane frame size first */
    if (!ubo || !out || w < 1 || h < 1 || (*env)->GetDirectBufferCapacity(env, ubo) < (jlong)sizeof(rt_camera_ubo) ||
        (*env)->GetDirectBufferCapacity(env, out) < (jlong)w * (jlong)h * 4) {
        jclass ex = (*env)->FindClass(env, "java/lang/RuntimeException");
        if (ex) (*env)->ThrowNew(env, ex, "renderDenoised: need direct buffers of >= 80 bytes (camera UBO) and >= w * h * 4 "
                                          "bytes (frame), w and h >= 1");
        return;
    }
    rt_denoise_params p;
    p.iterations = iterations;
    p.normal_power_log2 = normalPowerLog2;
    p.sigma_depth = sigmaDepth;
    p.sigma_color = sigmaColor;
    int rc = rt_render_denoised((rt_ctx*)(intptr_t)ctx, (const rt_camera_ubo*)(*env)->GetDirectBufferAddress(env, ubo),
                                w, h, maxBounces, &p, (uint8_t*)(*env)->GetDirectBufferAddress(env, out), NULL, NULL);
    if (rc) throw_rt(env, rc);
}

/* void renderTemporal(long ctx, ByteBuffer ubo80, int w, int h, int maxBounces, int maxHistory, float planeTol,
 *                     float normalMin, int filterIterations, int flags, ByteBuffer outRgba)
 * One frame of a temporally accumulated sequence (rtamd.h rt_render_temporal; the parameters are
 * rt_temporal_params, whose defaults are 32, 0.005f, 0.9f) into a direct buffer of at least w * h * 4 bytes.  The
 * host advances the UBO's frame_count per frame.  filterIterations 0 = no spatial filter, 1..6 = the denoiser's
 * default parameters with that many passes after the accumulation; flags = RT_TEMPORAL_RESET (1) |
 * RT_TEMPORAL_FIXED_SEED (2).  Synchronous; on the thread that owns ctx. */
JNIEXPORT void JNICALL Java_dev_demir_vulkan_engine_HipNative_renderTemporal(JNIEnv* env, jclass c, jlong ctx,
        jobject ubo, jint w, jint h, jint maxBounces, jint maxHistory, jfloat planeTol, jfloat normalMin,
        jint filterIterations, jint flags, jobject out) {
    /* a heap (non-direct) buffer has capacity -1; the size check needs a sane frame size first */
    if (!ubo || !out || w < 1 || h < 1 || (*env)->GetDirectBufferCapacity(env, ubo) < (jlong)sizeof(rt_camera_ubo) ||
        (*env)->GetDirectBufferCapacity(env, out) < (jlong)w * (jlong)h * 4) {
        jclass ex = (*env)->FindClass(env, "java/lang/RuntimeException");
        if (ex) (*env)->ThrowNew(env, ex, "renderTemporal: need direct buffers of >= 80 bytes (camera UBO) and >= w * h * 4 "
                                          "bytes (frame), w and h >= 1");
        return;
    }
    rt_temporal_params t;
    t.max_history = maxHistory;
    t.plane_tol = planeTol;
    t.normal_min = normalMin;
    t.reserved = 0;
    rt_denoise_params d;
    rt_denoise_default_params(&d);
    d.iterations = filterIterations;
    int rc = rt_render_temporal((rt_ctx*)(intptr_t)ctx, (const rt_camera_ubo*)(*env)->GetDirectBufferAddress(env, ubo),
                                w, h, maxBounces, &t, filterIterations != 0 ? &d : NULL, (uint32_t)flags,
                                (uint8_t*)(*env)->GetDirectBufferAddress(env, out), NULL, NULL);
    if (rc) throw_rt(env, rc);
}

/* void updateGeometry(long ctx, ByteBuffer vertices, ByteBuffer nodes)
 * The scene's triangles moved, in the tree it was uploaded with (rtamd.h rt_update_geometry; the scene must have
 * been uploaded after setOption(ctx, "refit", 1)).  Direct buffers whose capacities are the byte sizes: the moved
 * vertex records in the uploaded order and the uploaded nodes with new boxes.  Synchronous; on the thread that
 * owns ctx. */
JNIEXPORT void JNICALL Java_dev_demir_vulkan_engine_HipNative_updateGeometry(JNIEnv* env, jclass c, jlong ctx,
        jobject vertices, jobject nodes) {
    /* a heap (non-direct) buffer has capacity -1 */
    if (!vertices || !nodes || (*env)->GetDirectBufferCapacity(env, vertices) < 0 ||
        (*env)->GetDirectBufferCapacity(env, nodes) < 0) {
        jclass ex = (*env)->FindClass(env, "java/lang/RuntimeException");
        if (ex) (*env)->ThrowNew(env, ex, "updateGeometry: need direct buffers (the vertex records and the nodes)");
        return;
    }
    int rc = rt_update_geometry((rt_ctx*)(intptr_t)ctx,
                                (*env)->GetDirectBufferAddress(env, vertices),
                                (size_t)(*env)->GetDirectBufferCapacity(env, vertices),
                                (*env)->GetDirectBufferAddress(env, nodes),
                                (size_t)(*env)->GetDirectBufferCapacity(env, nodes), NULL);
    if (rc) throw_rt(env, rc);
}

JNIEXPORT void JNICALL Java_dev_demir_vulkan_engine_HipNative_destroy(JNIEnv* env, jclass c, jlong ctx) {
    rt_destroy((rt_ctx*)(intptr_t)ctx);
}
