package dev.demir.vulkan.engine;

import dev.demir.vulkan.renderer.BuiltCpuData;
import dev.demir.vulkan.renderer.FrameData;
import dev.demir.vulkan.scene.Camera;
import java.nio.ByteBuffer;
import java.nio.ByteOrder;
import java.util.concurrent.ConcurrentLinkedQueue;
import java.util.concurrent.atomic.AtomicReference;
import static org.lwjgl.system.MemoryUtil.memFree;

/**
 * Drop-in for VulkanEngine (VulkanEngine.java:120-185): the same public API and
 * render thread, rendering through jni/HipNative.c into librtamd.so.
 */
public class HipEngine implements Runnable {
    private static final int WIDTH = 1280, HEIGHT = 720, MAX_BOUNCES = 10;   // VulkanEngine.java:45-46, .comp:44
    private volatile boolean isRunning = true;
    private final Thread thread;
    private final AtomicReference<FrameData> frameQueue;
    private final ConcurrentLinkedQueue<BuiltCpuData> sceneQueue = new ConcurrentLinkedQueue<>();
    private final ConcurrentLinkedQueue<Camera> cameraQueue = new ConcurrentLinkedQueue<>();
    private final ConcurrentLinkedQueue<Boolean> skyToggleQueue = new ConcurrentLinkedQueue<>();
    private final ByteBuffer ubo = ByteBuffer.allocateDirect(80).order(ByteOrder.nativeOrder());
    private final ByteBuffer hit = ByteBuffer.allocateDirect(32).order(ByteOrder.nativeOrder());   // rt_hit
    private final ConcurrentLinkedQueue<Object[]> pickQueue = new ConcurrentLinkedQueue<>();
    private final ConcurrentLinkedQueue<ByteBuffer[]> geometryQueue = new ConcurrentLinkedQueue<>();
    private volatile boolean refit = false;                               // setRefit: uploads keep the refit tables
    private volatile boolean temporalMotion = false;                      // setTemporalMotion: updates keep the history
    private long ctx = 0;
    private boolean haveScene = false;
    private ByteBuffer[] slots = null;
    private static final int IN_FLIGHT = 4;                               // rt option async_slots (default 4)
    private final long[] tickets = new long[IN_FLIGHT];
    private long submitted = 0;
    private Camera currentCamera = null;
    private int isSkyEnabled = 1;
    private volatile boolean denoise = false;                             // setDenoise: filter every frame
    private int dnIterations = 4, dnNormalPowerLog2 = 7;                  // rt_denoise_default_params
    private float dnSigmaDepth = 0.005f, dnSigmaColor = 0.5f;
    private volatile boolean denoiseAlbedo = false;                       // setDenoiseAlbedo: filter the illumination
    private volatile boolean temporal = false;                            // setTemporal: accumulate across frames
    private int tpMaxHistory = 32;                                        // rt_temporal_default_params
    private float tpPlaneTol = 0.005f, tpNormalMin = 0.9f;
    private int temporalFrames = 0;                                       // the frame_count of the next temporal frame

    public HipEngine(AtomicReference<FrameData> frameQueue) {
        this.frameQueue = frameQueue;
        this.thread = new Thread(this, "HIP-Engine-Thread");
        this.thread.setDaemon(true);
    }
    public void start() { isRunning = true; thread.start(); }
    public void stop() {
        isRunning = false;
        try { thread.join(5000); } catch (InterruptedException e) { Thread.currentThread().interrupt(); }
    }
    public void submitScene(BuiltCpuData d) { sceneQueue.add(d); }
    public void submitCameraUpdate(Camera c) { cameraQueue.add(c); }
    public void submitSkyToggle(boolean on) { skyToggleQueue.add(on); }
    /** Scenes submitted from now on keep what submitGeometryUpdate needs (rt option "refit"). */
    public void setRefit(boolean on) { refit = on; }
    /** With setTemporal and setRefit: a geometry update keeps the temporal history, and the next frame gathers it
     *  where each pixel's point of its triangle lay before the update (rt option "temporal_motion").  Takes
     *  effect with the next submitted scene, like setRefit. */
    public void setTemporalMotion(boolean on) { temporalMotion = on; }
    /** The current scene's triangles moved (an object dragged): the moved vertex records in the uploaded order and
     *  the uploaded nodes with new boxes, as direct buffers whose capacities are their byte sizes (rt_refit_scene
     *  writes both).  Applied on the render thread before its next frame (rt_update_geometry); only the newest
     *  of several pending updates is applied.  The scene must have been submitted after setRefit(true). */
    public void submitGeometryUpdate(ByteBuffer vertices, ByteBuffer nodes) {
        geometryQueue.add(new ByteBuffer[]{vertices, nodes});
    }
    /** The flattened triangle under pixel (x, y) of the current camera (negative: nothing), handed to onHit
     *  on the render thread, which owns the context (rt_pick; a context is single-thread-affine). */
    public void submitPick(int x, int y, java.util.function.IntConsumer onHit) {
        pickQueue.add(new Object[]{x, y, onHit});
    }

    /** Filter every frame with the edge-avoiding denoiser (rt_render_denoised, its default parameters): the
     *  frames are then rendered synchronously, one at a time, instead of IN_FLIGHT at once. */
    public void setDenoise(boolean on) { denoise = on; }
    /** With setDenoise: divide each frame by its first-hit albedo before the filter and multiply it back after
     *  (rt option "denoise_albedo"), so that a surface's per-triangle albedos are not blurred with the noise. */
    public void setDenoiseAlbedo(boolean on) { denoiseAlbedo = on; }
    /** One denoised frame of the given UBO into a direct RGBA8 buffer; on the render thread. */
    private void renderDenoised(ByteBuffer cameraUbo, ByteBuffer outRgba) {
        HipNative.setOption(ctx, "denoise_albedo", denoiseAlbedo ? 1 : 0);
        HipNative.renderDenoised(ctx, cameraUbo, WIDTH, HEIGHT, MAX_BOUNCES, dnIterations, dnNormalPowerLog2,
                                 dnSigmaDepth, dnSigmaColor, outRgba);
    }

    /** Accumulate samples across frames, following the camera (rt_render_temporal, its default parameters; with
     *  setDenoise too, a 2-pass spatial filter after the accumulation): synchronous frames, like setDenoise. */
    public void setTemporal(boolean on) { temporal = on; }
    /** One temporal frame of the given UBO into a direct RGBA8 buffer; on the render thread.  Every frame gets a
     *  frame_count of its own, so that it is a new sample. */
    private void renderTemporal(ByteBuffer cameraUbo, ByteBuffer outRgba) {
        cameraUbo.putInt(64, temporalFrames++);
        HipNative.renderTemporal(ctx, cameraUbo, WIDTH, HEIGHT, MAX_BOUNCES, tpMaxHistory, tpPlaneTol, tpNormalMin,
                                 denoise ? 2 : 0, 0, outRgba);
    }

    @Override public void run() {
        try {
            ctx = HipNative.create(new int[]{0});
            if (HipNative.getOption(ctx, "queues_short") != 0)             // rtamd.h: async_slots + 2 > hw_queues
                System.err.println("WARN (HIP): GPU_MAX_HW_QUEUES=" + HipNative.getOption(ctx, "hw_queues")
                                   + " is too few for " + IN_FLIGHT + " frames in flight: start the JVM with "
                                   + "GPU_MAX_HW_QUEUES=16, or the frames' traces run one after another");
            while (isRunning) {
                BuiltCpuData d = sceneQueue.poll();                       // one scene per pass (:281-285)
                if (d != null) {
                    geometryQueue.clear();                                // updates of the scene this one replaces
                    HipNative.setOption(ctx, "refit", refit ? 1 : 0);
                    HipNative.setOption(ctx, "temporal_motion", temporalMotion ? 1 : 0);
                    HipNative.uploadScene(ctx, memByteBufferOf(d.modelVertexData), d.modelVertexData.remaining() * 4L,
                                          memByteBufferOf(d.modelMaterialData), d.modelMaterialData.remaining() * 4L,
                                          d.flatBvhData, d.flatBvhData.remaining());
                    memFree(d.modelVertexData);                           // as VulkanEngine.java:343,351
                    memFree(d.modelMaterialData);
                    haveScene = true;
                }
                ByteBuffer[] g, moved = null;                             // drain to the latest, like the cameras
                while ((g = geometryQueue.poll()) != null) moved = g;
                if (moved != null && haveScene) {
                    for (int j = 0; j < IN_FLIGHT; j++)                   // frames in flight read the old records
                        if (tickets[j] != 0) { HipNative.waitFrame(ctx, tickets[j]); tickets[j] = 0; }
                    submitted = 0;
                    HipNative.updateGeometry(ctx, moved[0], moved[1]);
                }
                Camera c, latest = null;                                  // drain to the latest (:288-298)
                while ((c = cameraQueue.poll()) != null) latest = c;
                if (latest != null) currentCamera = latest;
                Boolean s, sky = null;
                while ((s = skyToggleQueue.poll()) != null) sky = s;
                if (sky != null) isSkyEnabled = sky ? 1 : 0;
                if (!haveScene || currentCamera == null) { Thread.sleep(16); continue; }
                currentCamera.getOrigin().store(0, ubo);                  // same bytes as :387-395
                currentCamera.getLowerLeft().store(16, ubo);
                currentCamera.getHorizontal().store(32, ubo);
                currentCamera.getVertical().store(48, ubo);
                ubo.putInt(64, currentCamera.getFrameCount());
                ubo.putInt(68, isSkyEnabled);
                Object[] pk;                                              // picks see the camera of this pass
                while ((pk = pickQueue.poll()) != null) {
                    HipNative.pick(ctx, ubo, WIDTH, HEIGHT, (Integer) pk[0], (Integer) pk[1], hit);
                    ((java.util.function.IntConsumer) pk[2]).accept(hit.getInt(4));   // rt_hit.tri
                }
                if (denoise || temporal) {                                // synchronous: render, hits, filter, copy
                    for (int j = 0; j < IN_FLIGHT; j++)                   // frames the pipelined loop left in flight
                        if (tickets[j] != 0) { HipNative.waitFrame(ctx, tickets[j]); tickets[j] = 0; }   // (tickets are >= 1)
                    submitted = 0;
                    ByteBuffer px = ByteBuffer.allocateDirect(WIDTH * HEIGHT * 4);
                    if (temporal) renderTemporal(ubo, px); else renderDenoised(ubo, px);
                    frameQueue.set(new FrameData(px));
                    continue;
                }
                // IN_FLIGHT (= the library's async_slots, default 4) frames in
                // flight, each tracing on its own stream: the frames' traces
                // overlap each other and every readback overlaps later traces.
                // Start the JVM with GPU_MAX_HW_QUEUES=16 so each stream gets a
                // hardware queue of its own (HIP's default is 4 per process).
                if (slots == null) {
                    slots = new ByteBuffer[IN_FLIGHT];
                    for (int i = 0; i < IN_FLIGHT; i++) slots[i] = HipNative.allocFrame(WIDTH * HEIGHT * 4L);
                }
                int k = (int)(submitted++ % IN_FLIGHT);
                tickets[k] = HipNative.renderAsync(ctx, ubo, WIDTH, HEIGHT, MAX_BOUNCES, slots[k]);
                if (submitted >= IN_FLIGHT) {
                    int j = (int)(submitted % IN_FLIGHT);                 // the oldest frame in flight
                    HipNative.waitFrame(ctx, tickets[j]);
                    ByteBuffer px = ByteBuffer.allocateDirect(WIDTH * HEIGHT * 4);   // a fresh buffer per frame (:421)
                    px.put(slots[j].duplicate()).flip();
                    frameQueue.set(new FrameData(px));
                }
            }
        } catch (Exception e) {
            System.err.println("FATAL (HIP): HipEngine thread crashed!");
            e.printStackTrace();
            isRunning = false;
        } finally {
            if (ctx != 0) HipNative.destroy(ctx);                         // waits for frames in flight
            if (slots != null) for (ByteBuffer b : slots) HipNative.freeFrame(b);
        }
    }

    private static ByteBuffer memByteBufferOf(java.nio.FloatBuffer f) {
        return org.lwjgl.system.MemoryUtil.memByteBuffer(f);
    }
}
