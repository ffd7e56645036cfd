/*
 * hip_raytrace.h -- C ABI of libhip_raytrace.so (MI355X / gfx950).
 *
 * Drop-in boundary for ONE path of NullandKale/ILGPU_Raytracing: the two ILGPU kernel
 * launches inside RTRenderer.RenderDirectToPbo and the device buffers they touch.
 * Plain pointers and sizes only; no C++ or torch types.  The reference-side binding a
 * maintainer adds (C# [DllImport]) is shown in INTEGRATION.md.
 *
 *   entry point            replaces in the reference (ILGPU_Raytracing/Engine/...)
 *   ---------------------  -----------------------------------------------------------
 *   hrt_create             Context.Create + CreateCudaAccelerator + DefaultStream,
 *                          LoadAutoGroupedStreamKernel x2        RTRenderer.cs:66-68,85-86
 *   hrt_scene_upload       Scene.UploadAll (15 Allocate1D H2D copies, empty -> 1 zeroed
 *                          element)                              Scene.cs:258-279,370-377
 *                          reached through SceneManager.Commit / BvhManager.BuildOrRefit
 *                                                                SceneManager.cs:23, BvhManager.cs:27
 *   hrt_render_frame       GBuffer.EnsureLength / Framebuffer.EnsureLength /
 *                          EnsureLowResBuffers                   RTRenderer.cs:118-120,265-279
 *                          _primaryKernel(Index1D(inLen), gp)    RTRenderer.cs:152-153
 *                          Framebuffer.GetReservoirPair(0,frame) RTRenderer.cs:164, Framebuffer.cs:127-146
 *                          _integratorKernel(Index1D(inLen), ip, SpecializedValue(maxDepth))
 *                                                                RTRenderer.cs:181-205
 *                          _cuda.Synchronize()                   RTRenderer.cs:233
 *                          Framebuffer.DownloadToCpu (the unused read-back hook)
 *                                                                Framebuffer.cs:148-160
 *   hrt_present            pbo.MapCuda + RTTaa.ResolveUpsample | BlitKernel | BilinearUpsampleKernel
 *                                                                RTRenderer.cs:208-231,281-345; RTTaa.cs:34-171
 *                          HRT_PRESENT_TAAU_REPROJECT / hrt_motion_vectors: the reprojection the reference declares and
 *                          leaves out                            RTTaa.cs:49-57,82-84; RTRay.cs:339-360
 *   hrt_synchronize        _cuda.Synchronize() when frames were enqueued without it  RTRenderer.cs:233
 *   hrt_device_buffers     GpuFramebuffer / GpuGBuffer views handed to the post kernels
 *                          (TAAU, blit) without leaving the device  RTRenderer.cs:155-161,208-231
 *   hrt_reset_history      Framebuffer.EnsureLength re-allocation on resize (fresh
 *                          reservoirs)                           Framebuffer.cs:60-97
 *   hrt_trace_rays         SceneDeviceViews.TraceClosest / ShadowOcclusion over caller rays
 *                                                                SceneDeviceViews.cs:30-121
 *   hrt_trace_hits         the k nearest accepted hits along caller rays (ShadowOcclusion's walk, TraceClosest's records)
 *                                                                SceneDeviceViews.cs:30-237
 *   hrt_trace_paths        PathTraceKernel over caller rays in place of camera rays
 *                                                                RTRay.cs:187-199,203-325
 *   hrt_denoise            nothing: the reference shows its 2 spp frame (RTRenderer.cs:43-49) through TAAU alone.  An edge-avoiding
 *                          a-trous filter over the frame's radiance, guided by its G-buffer
 *   hrt_destroy            RTRenderer.Dispose                    RTRenderer.cs:347-363
 *   hrt_last_error         the exception message of CudaException / Argument*Exception
 *
 * Behavioural contract kept from the reference:
 *   - frame parity picks the reservoir pair: even frame -> prev = B, cur = A
 *     (Framebuffer.cs:132-145); reservoirs are zero-initialised when (re)allocated
 *     (the reference leaves them uninitialised; zero makes frame 0 well defined:
 *      m == 0 rejects every import, RTRay.cs:417).
 *   - per-pixel buffers are re-allocated only when width*height changes.
 *   - RNG and ReSTIR hashing key on the GLOBAL pixel index, so tiling never changes a
 *     pixel's value (RTUtils.cs:108-113, RTRay.cs:488).
 *   - hrt_render_frame blocks until the frame is complete; one call at a time per ctx.
 *
 * Multi-GPU: a ctx created on n devices cuts the image into 8-row strips and deals them
 * round-robin to its devices (device slot i renders strips s with s % n == i: sky rows are
 * cheap, geometry rows expensive, interleaving balances the tiles without knowing the image).
 * The scene is replicated, there is no collective; every device's strips are gathered into the
 * caller's host framebuffer by strided hipMemcpy2DAsync copies issued from one host thread per
 * device.  Page-lock the framebuffer once with hrt_host_register and those copies are
 * asynchronous DMA.  One-process-per-GPU hosts instead create one ctx per process and restrict
 * it to a row range / strip set with hrt_render_opts.  With ReSTIR reuse enabled a multi-device ctx
 * exchanges G-buffer and reservoir tiles between its devices (device-to-device copies); partial tiles of a
 * one-process-per-GPU host are refused while reuse is on.
 *
 * Status codes: 0 = ok, negative = error (message via hrt_last_error).
 *
 * Caller memory: an entry point writes exactly the bytes its contract names in caller memory (host or device), at the stated
 * minimum alignment and no more, and never modifies an input array (tests/test_guard_bands_gpu.py holds every entry point to it).
 */
#ifndef HIP_RAYTRACE_H
#define HIP_RAYTRACE_H

#include "hrt_types.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hrt_ctx hrt_ctx;

enum hrt_status {
    HRT_OK                = 0,
    HRT_ERR_INVALID_ARG   = -1,   /* ArgumentNullException / ArgumentOutOfRangeException */
    HRT_ERR_INVALID_STATE = -2,   /* InvalidOperationException (e.g. render before upload) */
    HRT_ERR_HIP           = -3,   /* CudaException analogue: a HIP runtime call failed     */
    HRT_ERR_NO_DEVICE     = -4,
    HRT_ERR_OUT_OF_MEMORY = -5
};

enum hrt_render_flags {
    HRT_FLAG_COUNTERS     = 1u << 0,  /* run the counting build of both kernels, fill hrt_stats.k[] */
    HRT_FLAG_SKIP_PRIMARY = 1u << 1,  /* bench/profiling only: reuse the resident G-buffer          */
    HRT_FLAG_REFERENCE_LAYOUT = 1u << 2, /* walk the reference's own arrays (TracerRef) instead of the device-private
                                         repack: identical results, A/B baseline and fallback for scenes beyond the
                                         packed encoding (leaf count > 15)                                      */
    HRT_FLAG_MEGAKERNEL   = 1u << 4,  /* force the path-trace launch to run as ONE one-pixel-per-lane kernel      */
    HRT_FLAG_STREAMED     = 1u << 5,  /* force the streamed init/shade/walk/finish/resolve pipeline.  Neither flag:
                                         the library picks by scene size (tiny BVH -> fused).  Identical results.  */
    HRT_FLAG_NO_SYNC      = 1u << 3,  /* enqueue only (outputs must be NULL); collect with hrt_synchronize.
                                         Up to 128 frames may be in flight; the 129th call drains first.  The
                                         times and the count of the frames drained there are not reported by
                                         the next hrt_synchronize (nor by hrt_frame_times): it reports the frames
                                         enqueued since, kernel_ms and frames alike.                            */
    /* One process per GPU with ReSTIR reuse ON: a tile needs the current G-buffer (worldPos, normalWS, objId) and the
     * previous reservoirs of the WHOLE image (RTRay.cs:339-374, 488-515).  The host then renders a frame in two calls
     * with an all-gather after each (ilgpu_raytracing_amd/tiling.py, RCCL through torch.distributed):
     *   1. HRT_FLAG_PRIMARY_ONLY            launch 1 on this tile           -> all-gather the 3 G-buffer arrays
     *   2. HRT_FLAG_SKIP_PRIMARY|EXCHANGED  path-trace launch on this tile  -> all-gather the 7 arrays of resCur
     * through the device pointers of hrt_device_buffers.  EXCHANGED is the caller's statement that both all-gathers of
     * the protocol are done; without it a reuse frame on a partial tile is refused (HRT_ERR_INVALID_STATE).        */
    HRT_FLAG_PRIMARY_ONLY = 1u << 6,
    HRT_FLAG_EXCHANGED    = 1u << 7,
    HRT_FLAG_TREELETS     = 1u << 8   /* streamed production frames of scenes with big triangle meshes (>= 4096 BLAS nodes): walk them with the
                                         LDS-staged, treelet-queued walker (csrc/hrt_walker_tl.hpp) instead of the persistent-wave walker.
                                         Identical results; measured SLOWER on every BASELINE config (profiles/r03_treelet_walker.md),
                                         hence opt-in.  Ignored where no treelets exist (sphere scenes, small meshes, after a vertex update).  */
};

/* Host destinations of one frame; any pointer may be NULL (not copied).  Arrays hold
 * width*height elements in the reference's layout (row 0 = bottom row, RTRay.cs:122).
 * With a row range only rows [row_begin,row_end) of each array are written. */
typedef struct hrt_outputs {
    /* GpuFramebuffer, RTRay.cs:51-56 */
    int32_t*    color;        /* packed 0xFFRRGGBB                              */
    float*      depth;
    int32_t*    objectId;
    int32_t*    cameraId;     /* 1 element                                      */
    /* pre-pack Lout (RTRay.cs:323), 3 floats per pixel: the 1e-4 parity target */
    hrt_float3* radiance;
    /* GpuGBuffer, RTRay.cs:80-87 */
    hrt_float3* gb_worldPos;
    hrt_float3* gb_normalWS;
    hrt_float3* gb_baseColor;
    int32_t*    gb_matId;
    int32_t*    gb_objId;
    int32_t*    gb_hitMask;
    /* resCur of this frame, GpuReservoirSoA RTRay.cs:23-31 */
    hrt_float3* res_L;
    hrt_float3* res_wi;
    float*      res_pdf;
    float*      res_w;
    float*      res_wSum;
    int32_t*    res_m;
    int32_t*    res_lightId;
} hrt_outputs;

typedef struct hrt_render_opts {
    uint32_t flags;           /* hrt_render_flags                                   */
    int32_t  row_begin;       /* rows [row_begin,row_end) of the global image;      */
    int32_t  row_end;         /* 0,0 = all rows                                     */
    int32_t  strip_n;         /* > 1: the range is cut into 8-row strips and this   */
    int32_t  strip_i;         /* call renders strips s with s % strip_n == strip_i  */
                              /* (load-balanced tiling for one-process-per-GPU hosts) */
} hrt_render_opts;
/* Strips are counted from row_begin, not from row 0: strip s holds rows row_begin + 8 s .. row_begin + 8 s + 7, the last one only
 * the rows below row_end.  A range that begins off a multiple of 8 therefore has strips off the 8-row grid of the image, and its
 * last strip may be ragged although row_end is not the image's height.
 * A call may own no strip (strip_i >= S, S = (row_end - row_begin + 7) / 8 the number of strips of the range): it returns HRT_OK,
 * renders nothing and writes nothing to `outputs`.
 * A context over nd device slots deals the call's strips again among its slots: slot j renders, and gathers into `outputs`, the
 * strips s with s % (strip_n * nd) == strip_i + strip_n * j, which is what hrt_device_views of slot j reports as strip_n, strip_i.
 * A slot may own no strip either.  Row y of [row_begin, row_end) thus belongs to slot j of the call iff
 * ((y - row_begin) / 8) % (strip_n * nd) == strip_i + strip_n * j.  cameraId (one element, in no row) is delivered by the call
 * and slot that own strip 0 of a range beginning at row 0. */

/* Device-resident views of the current frame on device slot `dev` (for on-device
 * consumers such as the TAAU/blit kernels or a torch tensor wrapper).  Pointers stay
 * valid until the next hrt_render_frame with a different size, or hrt_destroy.
 * Every array spans the whole image (global pixel index); only the strips this device
 * owns (rows [row_begin,row_end), strips s % strip_n == strip_i) hold this frame. */
typedef struct hrt_device_views {
    int32_t row_begin, row_end, strip_n, strip_i, width, height, device_id, reserved;
    void *color, *depth, *objectId, *radiance;
    void *gb_worldPos, *gb_normalWS, *gb_baseColor, *gb_matId, *gb_objId, *gb_hitMask;
    void *present_color;                      /* display-size RGBA8 of the last hrt_present (NULL before) */
    int32_t present_width, present_height;
    /* reservoir sets A and B (GpuReservoirSoA, RTRay.cs:23-48): L, wi (float3), pdf, w, wSum (float), m, lightId (int).
     * Frame f writes resCur = A and reads resPrev = B when f is even, the other way round when odd (Framebuffer.cs:132-145) */
    void *res_a[7], *res_b[7];
} hrt_device_views;

/* Presentation step of RenderDirectToPbo after the two launches (RTRenderer.cs:208-231): the last frame
 * rendered at (width,height) = (inW,inH) is resolved to the display size. */
enum hrt_present_mode {
    HRT_PRESENT_RESAMPLE = 0,   /* _enableTAAU == false: BlitKernel when sizes match, else BilinearUpsampleKernel
                                   (RTRenderer.cs:225-231,281-345)                                              */
    HRT_PRESENT_TAAU     = 1,   /* RTTaa.ResolveUpsample (RTTaa.cs:49-171): history kept per display size,
                                   first frame after (re)allocation or hrt_reset_history ignores it             */
    HRT_PRESENT_TAAU_REPROJECT = 2  /* the same resolve, with the history read where the camera's motion puts it (below) */
};
/* HRT_PRESENT_TAAU_REPROJECT finishes what the reference declares and ignores: ResolveUpsample(..., prevCam, curCam) never reads its
 * cameras and motionScaleX / Y are 0 ("No motion vectors (engine-side)", RTTaa.cs:49-57,82-84,110-111).
 * History camera: the context records, on slot 0, the cam of the frame a TAAU present (mode 1 or 2) last resolved into the history,
 *   and reprojects from THAT camera, not from the caller's params.prevCam: the history stays right when the host skips a present,
 *   presents twice or keeps prevCam for ReSTIR only.  The record goes wherever the history goes (hrt_reset_history, a new display
 *   size, hrt_destroy).  hrt_render_progressive frames count as frames.
 * Per output pixel idx = (px, py), float32 under the contract of hrt_math.h, statement order as written:
 *   1. cur, nmin, nmax, the nearest low-res pixel (ix, iy) and objId as TaaResolveKernel computes them (RTTaa.cs:117-160).
 *   2. P = gb_worldPos[iy * inW + ix] (a miss holds origin + dir * 1e6f: sky reprojects as a far point).
 *   3. proj(C, P) = ReprojectToPrevPixel (RTRay.cs:339-355) with camera C for prevCam and outW, outH for width, height, stopped before
 *      the (int) casts: p = P - C.origin; x, y, z = Dot(p, C.right / up / forward); ok = z > 1e-4f; t = hrt_tan(0.5f * C.fovYRadians);
 *      fx = 0.5f * (x / (z * t * C.aspect) + 1f) * outW; fy = 0.5f * (y / (z * t) + 1f) * outH.
 *   4. (okh, hx, hy) = proj(historyCam, P), (okc, cx, cy) = proj(cam of the frame, P); qx = (float)px + (hx - cx), qy = (float)py +
 *      (hy - cy).  Both run the same expressions: a bitwise equal camera gives qx == px, qy == py exactly.  No snapping threshold.
 *   5. valid = okh && okc && qx >= 0 && qx <= outW - 1 && qy >= 0 && qy <= outH - 1 (a NaN fails every comparison).
 *   6. valid: x0 = floor(qx), fx = qx - x0, x1 = min(x0 + 1, outW - 1), likewise y; hist = (c00*(1-fx) + c10*fx)*(1-fy) +
 *      (c01*(1-fx) + c11*fx)*fy over the four history texels unpacked with UnpackSRGB; histObj = historyObjId at the tap with the
 *      larger weight (fx < 0.5f ? x0 : x1, same for y).  Not valid: the taps of (qx, qy) = (px, py); the value cannot reach the output.
 *   7. reset = isFirstFrame || !valid || histObj != objId; from here on (clamp, blend, sharpen, PackSRGB) TaaResolveKernel unchanged.
 *      The packed result goes to the output and to the history at idx, objId to historyObjId[idx].
 * A lane reads history texels other lanes write, so slot 0 holds a second colour / objId pair (8 B per display pixel, allocated by
 * the first mode-2 present) and swaps after each mode-2 resolve; mode 1 resolves in place on whichever pair is current, so modes 0, 1
 * and 2 may alternate from frame to frame on one history.
 * Static camera: with fx = fy = 0 step 6 returns c00 exactly, so where the history camera is bitwise the frame's, mode 2 writes what
 * mode 1 writes, bit for bit, on every pixel whose P passes ok.
 * Out of scope: object motion (instances moved by hrt_scene_update_* are handled as in mode 1, by the objId test and the clamp;
 * every sphere carries objId -1, so there disocclusion rests on `valid` and the clamp), sub-pixel jitter, any depth plane in the history. */
typedef struct hrt_present_params {
    int32_t out_width, out_height;
    int32_t mode;                              /* hrt_present_mode */
    float feedback, sharpness, clampK;         /* TAAU tunables; <= 0 selects the reference's 0.075 / 0.10 / 1.25 (RTTaa.cs:77-79) */
} hrt_present_params;

int  hrt_create(const int* device_ids, int n_dev, hrt_ctx** out);
void hrt_destroy(hrt_ctx* ctx);
const char* hrt_last_error(hrt_ctx* ctx);      /* ctx may be NULL: last error of hrt_create */

int  hrt_scene_upload(hrt_ctx* ctx, const hrt_scene_desc* scene);

/* ---- moving instances of the committed scene: BvhManager.BuildOrRefit(scene, policy) (BvhManager.cs:13-27).
 * The reference declares the policy and ignores it: Commit re-runs RebuildTLAS on the host (Scene.cs:358-368)
 * and re-uploads all fifteen arrays (Scene.cs:258-279).  Here the scene stays on the device:
 *   - objectToWorld of instance instance_ids[k] becomes objectToWorld[k]; worldToObject, uniformScale and the
 *     world bounds are derived from it exactly as Scene.cs does (InvertRigidOrUniform :616-638, TransformAABB
 *     :560-580 of the box of the instance's BLAS root node); instance_ids must be distinct;
 *   - HRT_REBUILD_FORCE_REFIT keeps the TLAS topology and recomputes every box bottom-up;
 *   - HRT_REBUILD_FORCE_REBUILD builds a new TLAS over ALL instances (as RebuildTLAS does) with a Morton-order
 *     LBVH, leaves of <= 2 instances;
 *   - HRT_REBUILD_AUTO rebuilds a tree that was uploaded (once: the device-built tree costs about as much as a refit
 *     and walks faster than the reference's median split), afterwards refits, and rebuilds again if the boxes of the
 *     refitted tree have grown, in the geometric mean
 *     over all nodes, to more than 1.5 x the surface area they had when the tree was last built (uploaded or
 *     rebuilt): a measure neither one far-flung instance nor one huge instance dominates.
 * The rebuilt topology is a function of the instance records alone (tests/lbvh_ref.py restates it): the centroid of an
 * item is 0.5f * (worldBoundsMin + worldBoundsMax); the centroid bounds are the per-axis min / max over the centroids that are
 * not NaN, in every layout of the ids (an axis without one has no extent); every axis is cut into 1024 cells with the pitch
 * of the longest extent, a centroid at or beyond lo + ext lands in cell 1023, one that is NaN or not above lo in cell 0; the
 * 30-bit Morton keys (x in the highest lane) are sorted stably, equal keys keep id order and are told apart by sorted
 * position in Karras' construction; a subtree of <= 2 instances whose parent holds more is one leaf; nodes are numbered in
 * walk order.
 * n may be 0 (re-derive / rebuild only).  Blocking; every device of the context is updated.  The TLAS of a scene
 * updated this way is numbered in walk order; hrt_scene_download_tlas returns it in the reference's layout.
 * A different tree visits the same primitives in another order: results change only where two primitives are
 * hit at bit-equal distance (DESIGN.md "inner nodes only accelerate"). */
enum hrt_rebuild_policy { HRT_REBUILD_AUTO = 0, HRT_REBUILD_FORCE_REFIT = 1, HRT_REBUILD_FORCE_REBUILD = 2,
                          HRT_REBUILD_BLAS = 16 /* flag for hrt_scene_update_positions, see there */ };

typedef struct hrt_bvh_update_stats {
    int32_t action;           /* HRT_REBUILD_FORCE_REFIT or HRT_REBUILD_FORCE_REBUILD: what was done          */
    int32_t tlas_nodes;       /* nodes of the TLAS now in use                                                  */
    int32_t tlas_slots;       /* entries of its instance index list                                            */
    int32_t general_instances;/* 1 if a leaf slot holds an instance that needs the ray transform               */
    float   growth_refit;     /* after the refit: geometric mean over the nodes of area / area at the last build (0: no refit) */
    float   growth_final;     /* the same for the tree now in use (1 after a rebuild)                          */
    float   sah_cost;         /* of the tree now in use: sum(area x (leaf ? count : 1)) / area(root)            */
    float   device_ms;        /* HIP-event time of the device work on device slot 0 (tree in use; the library's second tree
                                 over many one-sphere instances is refitted after it, about as long again)    */
    int32_t blas_action;      /* hrt_scene_update_positions: what happened to the mesh BLASes (0 none, refit, rebuild) */
    float   blas_growth;      /* ... and the growth of their node boxes after the refit (0: not measured)       */
} hrt_bvh_update_stats;

int  hrt_scene_update_instances(hrt_ctx* ctx, const int32_t* instance_ids, int32_t n, const hrt_affine3x4* objectToWorld,
                                int32_t policy, hrt_bvh_update_stats* stats /* may be NULL */);

/* ---- deforming meshes: meshPositions[first_vertex, first_vertex + n) := positions (n may be 0).
 * The reference has no counterpart (its Commit rebuilds every BLAS on the host, Scene.cs:405-467, and re-uploads): here
 * every triangle-mesh BLAS keeps its topology and gets its triangle records and boxes recomputed bottom-up on the device
 * (BoundsOfTriangle over the items of each node, Scene.cs:423-429,597-605), the world bounds of the mesh instances are
 * re-derived from the new root boxes (TransformAABB, Scene.cs:560-580), and the TLAS is refitted / rebuilt per `policy`
 * as in hrt_scene_update_instances; with HRT_REBUILD_AUTO the mesh BLASes are rebuilt too when their boxes have grown, in the
 * geometric mean, to more than 1.5 x their area at the last build.  policy | HRT_REBUILD_BLAS first gives every triangle-mesh BLAS a new topology for the
 * new positions: a Morton-order LBVH over its triangles with leaves of <= 4 like the reference's BLAS, built on the device
 * into the node range and the leaf region of triPrimIdx the mesh already owns (blasNodeCount of its instance shrinks to
 * the new node count).  The construction is the TLAS's (see hrt_scene_update_instances) over the triangle centroids
 * ((a + b) + c) / 3.f, items always read from the instance's own item list triPrimIdx[primIndexFirst ...], with the smallest
 * leaf size in 4..14 whose tree (2 leaves - 1 nodes) fits the node range; nodes of the range behind the tree are zeroed, links -1.
 * Meshes are rebuilt in instance order and each reads its item list as it is at its turn (the reference's builder gives a later
 * mesh an item window inside an earlier mesh's leaf region, Scene.cs:398-403: its items are what that rebuild left there).
 * A mesh whose tree does not fit its node range even with leaves of 14 (the range an upload accepts only guarantees room for
 * FULL leaves) keeps the topology, leaf region and triPrimIdx it has and is refitted; the call succeeds, the other meshes are
 * rebuilt, and blas_action says rebuild only if at least one mesh got a new topology.  Another BLAS visits triangles in another order: pixels where two triangles are hit at bit-equal
 * distance (shared edges) may change, exactly as they would under a different host builder.
 * Sphere BLASes are untouched.  Blocking; every device of the context is updated. */
int  hrt_scene_update_positions(hrt_ctx* ctx, int64_t first_vertex, int64_t n, const hrt_float3* positions,
                                int32_t policy, hrt_bvh_update_stats* stats /* may be NULL */);

/* ---- moving / resizing / recolouring spheres: spheres[first, first + n) := spheres (n may be 0).  Every sphere-set BLAS
 * keeps its topology and gets its boxes recomputed bottom-up on the device (centre -+ radius per sphere of a leaf,
 * Scene.cs:331-336,386-390), the world bounds of the sphere-set instances are re-derived from the new root boxes, and the
 * TLAS is refitted / rebuilt per `policy` as in hrt_scene_update_instances.  Single-sphere instances with an identity
 * transform stay on the walkers' fast path (a moved INSTANCE would leave it: its ray transform must then be evaluated).
 * Note: the boxes are the unions of the spheres each node really holds; the reference's own builder indexes its
 * pre-computed bounds by array position (Scene.cs:386-395,413-419), which for more than four spheres per instance
 * yields other (wrong) boxes on a rebuild.  Blocking; every device of the context is updated. */
int  hrt_scene_update_spheres(hrt_ctx* ctx, int64_t first_sphere, int64_t n, const hrt_sphere* spheres,
                              int32_t policy, hrt_bvh_update_stats* stats /* may be NULL */);

/* Copies scene array `array` (0..14, in the order of hrt_scene_desc / SceneDeviceViews.cs:13-27) as it is now on device
 * slot `dev` back to the host: what TracerRef walks after updates.  *count (may be NULL) receives the element count;
 * dst may be NULL to query it; cap = capacity of dst in elements. */
int  hrt_scene_download_array(hrt_ctx* ctx, int dev, int array, void* dst, int64_t cap, int64_t* count);

/* Copies the TLAS in use on device slot `dev`, in the reference's layout, and the instance records to the host
 * (any pointer may be NULL).  counts[3] (may be NULL) receives the element counts {tlasNodes, tlasInstanceIndices,
 * instances}; an array is copied only if its capacity (in elements) is large enough, else HRT_ERR_INVALID_ARG. */
int  hrt_scene_download_tlas(hrt_ctx* ctx, int dev, hrt_bvh_node* tlasNodes, int64_t cap_nodes,
                             int32_t* tlasInstanceIndices, int64_t cap_indices, hrt_instance* instances, int64_t cap_instances,
                             int64_t* counts);

int  hrt_render_frame(hrt_ctx* ctx, const hrt_frame_params* params,
                      const hrt_render_opts* opts,      /* may be NULL */
                      const hrt_outputs* outputs,       /* may be NULL: leave results on device */
                      hrt_stats* stats);                /* may be NULL */

/* ---- progressive frames: one frame refined over several calls, bit-exact.
 * Renders samples [sample_begin, params->spp) of the frame `params` describes.  On return every output
 * (host `outputs`, hrt_device_views, resCur) holds exactly what hrt_render_frame(params) would: the frame at
 * params->spp samples.
 *   - sample_begin == 0 starts a progressive frame: primary visibility, then samples [0, spp).  params->spp >= 1.
 *   - sample_begin > 0 continues the progressive frame last rendered on this ctx, without primary visibility.  It needs
 *     params bitwise identical to the previous call's except spp, sample_begin == the previous call's spp, and the same
 *     row range, strips and path-selecting flags (REFERENCE_LAYOUT, MEGAKERNEL, STREAMED, TREELETS); otherwise, or after
 *     an hrt_render_frame, hrt_scene_upload, hrt_scene_update_*, hrt_reset_history or resize in between, it returns
 *     HRT_ERR_INVALID_STATE with a message naming what differs.  params->spp <= sample_begin: HRT_ERR_INVALID_ARG.
 *   - hrt_present (the preview), hrt_trace_rays, hrt_device_buffers, hrt_frame_times and hrt_synchronize may run in between.
 *   - flags: REFERENCE_LAYOUT, MEGAKERNEL, STREAMED, TREELETS and NO_SYNC (outputs must then be NULL, as for frames; several
 *     continuations may be enqueued back to back).  COUNTERS, PRIMARY_ONLY, SKIP_PRIMARY and EXCHANGED: HRT_ERR_INVALID_ARG
 *     (the one-process-per-GPU reuse protocol is not progressive).
 *   - ReSTIR reuse: legal wherever a reuse frame is (a full image; one ctx over several device slots), exact in the same sense.
 *   - a refused call changes no device state: a following valid continuation is unaffected.
 * Exact because the sample sum is one in-order f32 sum carried between calls unscaled, the random stream of a sample depends
 * only on (pixel, frame, lock, sample index), and resCur keeps its last writer.  The carried sum is a per-device plane of
 * 12 B per pixel (99.5 MB at 3840x2160), allocated by the first progressive call and freed by hrt_destroy (or a resize). */
int  hrt_render_progressive(hrt_ctx* ctx, const hrt_frame_params* params, const hrt_render_opts* opts,
                            int32_t sample_begin, const hrt_outputs* outputs, hrt_stats* stats);

/* Waits for every frame enqueued with HRT_FLAG_NO_SYNC.  stats (may be NULL): kernel_ms[]
 * = per-launch HIP-event time summed over those frames (max over devices), frames = their
 * number.  A blocking hrt_render_frame is enqueue + hrt_synchronize. */
int  hrt_synchronize(hrt_ctx* ctx, hrt_stats* stats);

/* out_color_host: out_width*out_height packed 0xFFRRGGBB, may be NULL (result stays in hrt_device_views.present_color).
 * The last frame must have been a full-image render.  The resolve runs on device slot 0; a multi-device ctx first
 * brings the colour / objectId strips of its other devices there (device-to-device copies). */
int  hrt_present(hrt_ctx* ctx, const hrt_present_params* params, int32_t* out_color_host);
/* HIP-event time (ms) of the kernel of the last successful hrt_present (the resolve, blit or upsample alone: no strip or host
 * copies); 0 before the first. */
int  hrt_present_time(hrt_ctx* ctx, float* ms);

/* The camera motion vectors of the last full-image frame, for hosts with a temporal filter of their own: mv[i] for internal pixel i =
 * (hx - cx, hy - cy) of step 4 above with outW, outH = the frame's width, height, P = gb_worldPos[i] and from_cam as the history
 * camera (NULL: the frame's params.prevCam), in pixels; (NaN, NaN) where okh && okc is false.  The same device function as the
 * mode-2 resolve.
 * dev < 0: mv is a host array of width * height; every device slot computes the strips it rendered, gathered as frame outputs are.
 * dev == 0: mv is device memory of slot 0, 8-byte aligned (other slots' gb_worldPos strips are brought over first, as hrt_present
 *   brings colour).  Any other dev, NULL mv, the wrong memory kind: HRT_ERR_INVALID_ARG.  No frame yet or a partial tile:
 *   HRT_ERR_INVALID_STATE.
 * Blocking.  device_ms (may be NULL): HIP-event time of the kernel (max over slots).  Frame state, present history and a pending
 * progressive frame are untouched. */
int  hrt_motion_vectors(hrt_ctx* ctx, const hrt_camera* from_cam, hrt_float2* mv, int32_t dev, float* device_ms);

/* Per-frame HIP-event times (ms) of the frames the last hrt_synchronize (or blocking hrt_render_frame) collected on device
 * slot `dev`: launch 0 = primary visibility, 1 = the path-trace stage.  *n (may be NULL) receives their number; at most
 * cap values are written to ms (may be NULL). */
int  hrt_frame_times(hrt_ctx* ctx, int dev, int launch, float* ms, int cap, int* n);

/* Page-locks (hipHostRegister, portable) a host range the caller will pass as hrt_outputs destination, e.g. the C# host's
 * pinned framebuffer arrays (GCHandle.Alloc(..., Pinned)): gathers into it are asynchronous DMA instead of staged copies.
 * The range must stay mapped until hrt_host_unregister / hrt_destroy.  Replaces nothing in the reference, whose frame never
 * leaves the GPU (CudaGlInteropIndexBuffer.cs:37-194). */
int  hrt_host_register(hrt_ctx* ctx, void* ptr, int64_t bytes);
int  hrt_host_unregister(hrt_ctx* ctx, void* ptr);

/* Caps a path-state workspace of the streamed pipeline at max_resident_paths paths (324 bytes each; 0 = the default of
 * 2^25 paths = 10.9 GB): frames whose width*height*spp exceeds it run in several sample batches, with identical results.
 * Two sample batches are in flight at a time, each in a workspace of its own, so up to twice that much memory is held.
 * Counterpart of sizing MemoryBuffer1D allocations in the reference (Framebuffer.cs:60-97). */
int  hrt_set_workspace_limit(hrt_ctx* ctx, int64_t max_resident_paths);

int  hrt_device_buffers(hrt_ctx* ctx, int dev, hrt_device_views* out);

/* ---- ray queries on the scene now on the device (hrt_ray / hrt_ray_hit in hrt_types.h).
 * HRT_QUERY_CLOSEST: SceneDeviceViews.TraceClosest(ray, out ...) (SceneDeviceViews.cs:30-86): closestT starts at 1e30 with the
 *   fixed 0.001 epsilon (no tMax); result i = hrt_ray_hit of ray i, plus the instance record and primitive that won.
 * HRT_QUERY_OCCLUDED: ShadowOcclusion(ray, ray.tMax) (SceneDeviceViews.cs:89-121) with the any-hit alpha cut-outs (:270-327);
 *   result i = 1 if ray i is occluded, else 0.  Any float tMax is legal (0, negative, NaN, +-inf: what the slab and t tests make of it).
 * results: hrt_ray_hit[n] (CLOSEST) or int32_t[n] (OCCLUDED).
 * dev < 0: rays / results are host memory; the rays are split into contiguous chunks over every device slot, each slot works in
 *   fixed-size chunks through its own pinned staging (or straight from / to a range registered with hrt_host_register).
 * dev >= 0: rays / results are device memory of device slot `dev` (checked; host memory -> HRT_ERR_INVALID_ARG), 16-byte aligned.
 * Blocking.  device_ms (may be NULL): HIP-event time of the device work (max over slots), copies excluded.
 * Queries leave frame state alone (G-buffer, reservoirs, present history, hrt_frame_times, hrt_device_views pointers); they run on
 * the device streams after any frames enqueued with HRT_FLAG_NO_SYNC, whose accounting stays with hrt_synchronize.
 * n == 0 launches nothing. */
enum hrt_ray_query { HRT_QUERY_CLOSEST = 0, HRT_QUERY_OCCLUDED = 1 };
#define HRT_QUERY_CHUNK (1 << 21)      /* rays per walk: a device slot works through its rays in chunks of at most this many */
int  hrt_trace_rays(hrt_ctx* ctx, int32_t query, const hrt_ray* rays, int64_t n, void* results,
                    int32_t dev, float* device_ms);

/* ---- multi-hit queries: the k nearest accepted primitive tests along each caller ray, on the scene now on the device.
 * Defined by an unpruned walk of the uploaded tree with ShadowOcclusion's limits and TraceClosest's per-hit records:
 *   - TLAS: IntersectAABB(ray, box, 0.001f, ray.tMax); every leaf entry reached transforms the ray (TransformRay(worldToObject)),
 *     scale = uniformScale > 0 ? uniformScale : 1, tMaxObj = tMax * scale (SceneDeviceViews.cs:89-121).
 *   - BLAS: IntersectAABB(rayObj, box, 0.001f, tMaxObj).  A primitive test is accepted when the intersection routine reports a hit
 *     with t > 0.001f && t < tMaxObj; a triangle must also pass TraceClosest's alpha rule, linear mask sample >= AlphaCutoff
 *     (:206-221; not AnyHit's point/band rule).
 *   - One record per accepted test: the hrt_ray_hit CLOSEST would return if that hit won (:65-86, :146-159, :196-227): t = tObj / scale,
 *     normal = Normalize(TransformVector(objectToWorld, nObj)) with the TwoSided flip in object space, the sphere albedo rules (Kd or
 *     albedo, texture by atan2/acos) or the triangle's Kd or diffuse texture, objId (triangle index, -1 for a sphere), shade, ior
 *     (s.ior > 0 ? s.ior : 1; 1 for triangles), instance = the instance record, prim = the sphere or triangle index.
 *   - Order: ascending t as IEEE totalOrder (t >= +0 or NaN: the unsigned bit pattern), then instance, then prim.  A tree that lists
 *     a primitive or an instance twice gives identical duplicate records, side by side.
 * hits: n * k records, hits[i * k + j]; slots j >= counts[i] hold CLOSEST's miss record (t = 1e30, normal 0, albedo 1, ior 1,
 *   objId -1, shade 0, instance -1, prim -1).  counts[i] = min(k, totals[i]).  Hits at t >= 1e29 are hits.
 * totals (may be NULL): every accepted test of ray i, saturating at INT32_MAX.  No box test is cut at the k-th distance (no such
 *   cut is provably exact in float arithmetic), so results with and without totals are the same bit for bit.
 * Any float tMax is legal (0, negative, NaN, +-inf): what the slab and t tests make of it.  hrt_ray.pad is ignored.
 * HRT_ERR_INVALID_ARG: k < 1 or k > HRT_HITS_MAX, n < 0, NULL rays, hits or counts with n > 0, a bad slot or memory kind,
 *   misalignment.  HRT_ERR_INVALID_STATE: no scene uploaded.  n == 0 launches nothing.
 * dev, device_ms, blocking and frame state: as hrt_trace_rays.  dev < 0 chunks by hit slots (at most HRT_QUERY_CHUNK of n * k per
 *   chunk); dev >= 0 takes device memory of that slot, rays and hits 16-byte aligned, counts and totals 4-byte aligned.  The query
 *   works in a private workspace freed by hrt_destroy and leaves the frame's state and a pending progressive frame alone. */
#define HRT_HITS_MAX 16
int  hrt_trace_hits(hrt_ctx* ctx, const hrt_ray* rays, int64_t n, int32_t k,
                    hrt_ray_hit* hits, int32_t* counts, int32_t* totals,
                    int32_t dev, float* device_ms);

/* ---- radiance queries: PathTraceKernel (RTRay.cs:203-325) along caller rays on the scene now on the device.
 * Ray i (0 <= i < n) has key j = first_key + i and RNG pixel (px, py) = (j % params->width, j / params->width).  It is shaded as
 * that pixel of a frame with reuse off, with two substitutions:
 *   - primary vertex: TraceClosest(ray) replaces the camera ray (RTRay.cs:187-199).  No tMax: hrt_ray.tMax and pad are ignored,
 *     dir is used as given.  The vertex takes the frame's G-buffer encoding (packedMat = shade | FloatToI16(ior) << 16, so ior is
 *     quantised as in a frame); a miss stores worldPos = origin + dir * 1e6f and objId = -1 (StoreMiss).
 *   - camera-derived values take the ray's own origin and direction: ViewDirFromCam(pos) is normalize(pos - ray.origin), the miss
 *     colour SkyWeighted(PrimaryRayDir(index)) is SkyWeighted(ray.dir) (added spp times, in order), DistanceFromCamera is
 *     |worldPos - ray.origin|.
 * Everything else is the frame's: frame, rngLockNoise, spp (max(1, spp)), maxDepth, the sun and sky tints, the RNG salt, the bounce
 * loop, Russian roulette, the ReSTIR candidate stream with reuse off, SafeColor, the in-order sum and the final 1/spp scale.
 * cam, prevCam, height and debugCamSeq are ignored; resCur and cameraId are not written.
 * Camera rays in pixel order (o = cam.origin, d = normalize(lowerLeft + horizontal*u + vertical*v - origin)) with first_key = 0,
 * the frame's width and reuse off give results[p] == the frame's radiance[p], color[p], depth[p], objectId[p], bit for bit.
 *   - flags: HRT_FLAG_REFERENCE_LAYOUT, MEGAKERNEL, STREAMED, TREELETS only (any other bit: HRT_ERR_INVALID_ARG).  REFERENCE_LAYOUT
 *     selects TracerRef as for a frame.  MEGAKERNEL, STREAMED and TREELETS are accepted and ignored: every query runs the fused
 *     path-trace organisation (a frame forced to it with MEGAKERNEL costs the same; scenes whose frames stream are several times
 *     slower as queries).  Results do not depend on the organisation.
 *   - HRT_ERR_INVALID_ARG: enableTemporalReuse or enableSpatialReuse nonzero, width <= 0, maxDepth < 0, first_key < 0,
 *     first_key + n > 2^31 - 1, NULL rays or results with n > 0.  HRT_ERR_INVALID_STATE: no scene uploaded.  n == 0 launches nothing.
 *   - dev, device_ms: as hrt_trace_rays (dev < 0: host arrays over every device slot in bounded chunks through pinned staging or a
 *     range registered with hrt_host_register; dev >= 0: device memory of that slot, 16-byte aligned).
 *   - Blocking; runs on the device streams after any HRT_FLAG_NO_SYNC frames.  Frame state is left alone (G-buffer, reservoirs,
 *     present history, hrt_frame_times, hrt_device_views pointers, a pending progressive frame): the query works in a private
 *     per-chunk workspace freed by hrt_destroy. */
int  hrt_trace_paths(hrt_ctx* ctx, const hrt_frame_params* params, uint32_t flags,
                     const hrt_ray* rays, int64_t n, int64_t first_key,
                     hrt_path_result* results, int32_t dev, float* device_ms);
int  hrt_reset_history(hrt_ctx* ctx);           /* zero both reservoir sets */

/* ---- spatial denoiser: an edge-avoiding a-trous filter over the radiance of the last full-image frame, guided by its G-buffer.
 * The filter, float32 under hrt_math.h, no contraction, statement order as written.  W, H = the frame's size, idx = y * W + x,
 * dot(a, b) = a.x*b.x + a.y*b.y + a.z*b.z left to right, n = gb_normalWS, P = gb_worldPos:
 *   1. Prepare, per pixel: hit = gb_hitMask[idx] != 0.  a = (1, 1, 1) when HRT_DENOISE_NO_DEMODULATE is set or !hit, else per channel
 *      hrt_fmax(gb_baseColor, 0.01f).  c = radiance / a per channel (IEEE divide).
 *      kx = 1.0f / (sigma_plane * sigma_plane * hrt_fmax(depth * depth, 1e-12f)).  Uniform: kn = 1.0f / (sigma_normal * sigma_normal).
 *   2. Iteration i = 0 .. iterations-1: s = 1 << i, sc = sigma_color * 2^-i (exact), kc = 1.0f / (sc * sc).  It reads the plane
 *      iteration i-1 wrote and writes another.  A pixel with !hit is copied.  For a hit pixel p, taps dy = -2..2 outer, dx = -2..2
 *      inner, q = (x + dx*s, y + dy*s):
 *        - skipped if q is outside the image or q is not a hit;
 *        - dn = dot(n_p - n_q, n_p - n_q); d = dot(P_q - P_p, n_p); dc = dot(c_p - c_q, c_p - c_q);
 *        - e = dn * kn + d * d * kx + dc * kc (kx of p); w = (h[dx] * h[dy]) * hrt_exp(-e), h = (1/16, 1/4, 3/8, 1/4, 1/16);
 *        - skipped unless w > 0.0f (a NaN fails); else per channel acc += w * c_q (multiply, then add) and ws += w;
 *      result: ws > 0.0f ? acc / ws : c_p per channel (IEEE divide).  A pixel whose own guides are NaN keeps its value.
 *   3. Finish: out = c * a per channel -> the denoised radiance; pack_rgba8(out) (RTRay.cs:66-76, as the frame packs) -> the
 *      denoised colour.
 * Misses (sky) are noise-free and stay bit-equal to the frame's radiance.  Samples are SafeColor-clamped to +-1e6, so every c is
 * finite; hostile guides (NaN / infinite normals or positions) fall to the w > 0 rule.
 *   - Works on the last full-image frame (hrt_render_frame, or any call of hrt_render_progressive: a preview may be denoised between
 *     refinements).  No frame yet, or a partial tile: HRT_ERR_INVALID_STATE, as hrt_present.
 *   - Blocking; runs on device slot 0 after any HRT_FLAG_NO_SYNC frames.  A multi-device ctx first brings the other slots' strips of
 *     radiance, normalWS, worldPos, baseColor, depth and hitMask to slot 0, as hrt_present brings colour.
 *   - Writes two private planes on slot 0 (denoised radiance, float3; denoised colour, packed 0xFFRRGGBB) and works in a private
 *     workspace (80 bytes per pixel in all), allocated on first use, re-allocated for a new frame size, freed by hrt_destroy.  Frame
 *     state is untouched: radiance, colour, G-buffer, reservoirs, present history, hrt_frame_times, a pending progressive frame.
 *   - out_radiance_host / out_color_host (either may be NULL): width * height elements, row 0 = bottom row as hrt_outputs.
 *   - device_ms (may be NULL): HIP-event time of the denoise kernels alone (no strip or host copies).
 *   - HRT_ERR_INVALID_ARG: NULL params, iterations < 0 or > 8, an unknown flag bit.
 * The denoised planes belong to the frame they were made from: hrt_present with HRT_PRESENT_DENOISED in its mode resolves the
 * denoised colour in place of the frame's (modes 0, 1 and 2 otherwise unchanged: objectId and gb_worldPos stay the frame's), and
 * returns HRT_ERR_INVALID_STATE after a newer frame, scene upload or resize until hrt_denoise has run again.
 * Out of scope: denoising at display resolution, object motion; temporal accumulation and variance guidance are hrt_denoise_temporal's. */
enum hrt_denoise_flags { HRT_DENOISE_NO_DEMODULATE = 1u << 0 };
typedef struct hrt_denoise_params {
    int32_t  iterations;      /* 1..8; 0 selects 5.  Iteration i uses tap step 1 << i                         */
    uint32_t flags;           /* hrt_denoise_flags; any other bit: HRT_ERR_INVALID_ARG                        */
    float    sigma_color, sigma_normal, sigma_plane;   /* <= 0 selects 4.0, 0.5, 0.02; a NaN goes through, as in hrt_present */
} hrt_denoise_params;
int  hrt_denoise(hrt_ctx* ctx, const hrt_denoise_params* params, hrt_float3* out_radiance_host /* may be NULL */,
                 int32_t* out_color_host /* may be NULL */, float* device_ms /* may be NULL */);
/* slot 0 device pointers of the denoised radiance (hrt_float3) and colour (int32) planes; NULL before the first hrt_denoise.  Valid
 * until an hrt_denoise at another frame size, or hrt_destroy. */
int  hrt_denoised_buffers(hrt_ctx* ctx, void** radiance, void** color);
#define HRT_PRESENT_DENOISED 0x100   /* OR into hrt_present_params.mode: resolve the denoised colour instead of the frame's */

/* ---- temporal denoiser: hrt_denoise's filter with the demodulated radiance and its luminance moments accumulated over frames (in
 * float, at internal resolution, read where the camera's motion puts each surface point) and with the colour term of the a-trous
 * passes driven by a per-pixel variance instead of a constant (SVGF-shaped).  It writes the same two result planes as hrt_denoise
 * and stamps them with the frame: hrt_denoised_buffers and HRT_PRESENT_DENOISED serve whichever of the two ran last on the frame.
 * float32 under hrt_math.h, no contraction, statement order as written.  W, H, idx, dot, n, P as for hrt_denoise;
 * lum(v) = 0.2126f*v.x + 0.7152f*v.y + 0.0722f*v.z, left to right.  Parameters after their defaults; the host also replaces an
 * alpha > 1 by 1 (a NaN goes through).  A "record" is four floats; history records are kept for the next call.
 *   1. Prepare, per pixel: hit, a, c, kx, kn as steps 1 of hrt_denoise (HRT_DENOISE_T_NO_DEMODULATE for its flag).  The guide values
 *      (n, kx, P, hit) are kept in one of two sets; the other set holds the previous call's: the geometry of the history.
 *   2. Temporal, per pixel p = (px, py).  !hit: colour record (c, 0), moment record (0, 0, 0, 0).  hit:
 *      - m = (okh && okc, hx - cx, hy - cy) of step 4 of HRT_PRESENT_TAAU_REPROJECT with P = P_p, outW, outH = W, H and for historyCam
 *        the cam of the frame this entry point last accumulated (recorded on slot 0, never params.prevCam).  qx = (float)px + m.dx,
 *        qy = (float)py + m.dy; valid = step 5 there, and false while the history is empty.
 *      - hn = 0.  valid: x0 = floor(qx), fx = qx - x0, x1 = min(x0 + 1, W - 1), likewise y.  Taps t in the order (x0, y0), (x1, y0),
 *        (x0, y1), (x1, y1) with weights wt = (1-fx)*(1-fy), fx*(1-fy), (1-fx)*fy, fx*fy.  A tap is accepted when wt > 0.0f, it was a hit
 *        in the previous guides, dot(n_p, n_t) >= normal_cos_min and hrt_abs(dot(P_t - P_p, n_p)) <= plane_tol * depth_p (n_t, P_t from
 *        the previous guides, depth_p the frame's depth; a NaN fails).  Accepted: ws += wt; hc += wt * C_t per channel, hm1 += wt * M1_t,
 *        hm2 += wt * M2_t, hs += wt * N_t (multiply, then add; all start at 0; C_t, M1_t, M2_t, N_t = the history records of t).
 *        ws > 0.0f: hc, hm1, hm2 are divided by ws and hn = hs / ws.
 *      - l = lum(c).  !(hn > 0.0f) (no history): C = c, M1 = l, M2 = l * l, N = 1, taken as they are.  Else N = hrt_fmin(hn + 1.0f,
 *        (float)max_history), r = 1.0f / N, ac = hrt_fmax(r, alpha_color), am = hrt_fmax(r, alpha_moments), C = hc + (c - hc) * ac per
 *        channel, M1 = hm1 + (l - hm1) * am, M2 = hm2 + (l * l - hm2) * am.
 *      - colour record (C, 0), moment record (M1, M2, N, 0).  The history is a pair of record planes each, swapped per call: a lane
 *        reads records other lanes write.
 *      A camera bitwise equal to the history camera gives fx = fy = 0: one tap of weight 1, and x * 1 / 1 is exact, so a static camera
 *      reads its own pixel's history unresampled.
 *   3. Variance v, the fourth word of the colour record (a kernel of its own).  !hit: 0.  N >= 4.0f: v = hrt_fmax(M2 - M1 * M1, 0.0f).
 *      Else over the 7x7 window, dy = -3..3 outer, dx = -3..3 inner, q = (x + dx, y + dy) inside the image and a hit: dn, d as hrt_denoise,
 *      w = hrt_exp(-(dn * kn + d * d * kx)); w > 0.0f: S1 += w * M1_q, S2 += w * M2_q, sw += w.  sw > 0.0f: S1 = S1 / sw, S2 = S2 / sw,
 *      v = hrt_fmax(S2 - S1 * S1, 0.0f) * (4.0f / N); else the moment formula.
 *   4. A-trous, iteration i = 0 .. iterations-1, s = 1 << i, on records (c, v); a pixel with !hit is copied.  Hit pixel p:
 *      - vs = gs = 0; dy = -1..1 outer, dx = -1..1 inner, q = (x + dx*s, y + dy*s) inside the image and a hit: g = k[dx] * k[dy],
 *        k = (1/4, 1/2, 1/4); vs += g * v_q; gs += g.  vf = vs / gs.  kl = 1.0f / (sigma_lum * hrt_sqrt(vf) + 1e-6f).  (The taps lie on
 *        the step-s lattice, not on adjacent pixels: the one deviation from SVGF's prefilter.)
 *      - the 25 taps of hrt_denoise step 2 with e = dn * kn + d * d * kx + hrt_abs(lum(c_p) - lum(c_q)) * kl and, where w > 0.0f,
 *        acc += w * c_q, va += (w * w) * v_q, ws += w.  ws > 0.0f: c' = acc / ws per channel, v' = va / (ws * ws); else (c_p, v_p).
 *      - iteration 0 also writes its (c', v') records (copies of misses included) to the history colour plane: what the next call sees.
 *      - the last iteration finishes as hrt_denoise step 3.
 *   5. HRT_DENOISE_T_NO_SPATIAL: steps 3 and 4 are skipped; out = C * a, the history colour record is (C, 0).
 * Misses stay bit-equal to the frame's radiance.  On an empty history with NO_SPATIAL the output is (radiance / a) * a.
 *   - Preconditions, blocking, slot 0, the strips of a multi-device ctx, out_*_host, device_ms: as hrt_denoise.
 *   - HRT_ERR_INVALID_ARG: NULL params, iterations < 0 or > 8, an unknown flag bit.  HRT_ERR_INVALID_STATE: no frame yet, a partial
 *     tile, or a frame this entry point has already accumulated (one call per frame serial; the refused call changes nothing).
 *   - History: private to slot 0 (two guide sets, two colour and two moment record planes: 128 bytes per pixel beside
 *     hrt_denoise's 80-byte workspace, whose colour and result planes it shares), allocated on first use, freed by hrt_destroy.  hrt_reset_history, hrt_scene_upload, a new frame size
 *     and HRT_DENOISE_T_RESET empty it; hrt_scene_update_* does not.  Frame state, reservoirs, the present history, hrt_frame_times, a
 *     pending progressive frame and hrt_denoise's own behaviour are untouched.
 * Out of scope: object motion (a moved surface fails the plane test and restarts), sub-pixel jitter, filtering at display resolution,
 * specular / diffuse separation. */
enum hrt_denoise_temporal_flags { HRT_DENOISE_T_NO_DEMODULATE = 1u << 0, HRT_DENOISE_T_NO_SPATIAL = 1u << 1, HRT_DENOISE_T_RESET = 1u << 2 };
typedef struct hrt_denoise_temporal_params {
    int32_t  iterations;                          /* 1..8; 0 selects 5 (as hrt_denoise)                                  */
    uint32_t flags;                               /* hrt_denoise_temporal_flags; any other bit: HRT_ERR_INVALID_ARG      */
    float    alpha_color, alpha_moments;          /* <= 0 selects 0.2, 0.2 (SVGF): the floor of the blend factor         */
    float    sigma_lum, sigma_normal, sigma_plane;   /* <= 0 selects 0.7, 0.5, 0.02; a NaN goes through.  sigma_lum is not SVGF's
                                                     4: v is the variance of one frame's sample, not of the accumulated mean,
                                                     and a band of 4 deviations of it blurs real detail     */
    float    normal_cos_min, plane_tol;           /* history tap acceptance; <= 0 selects 0.9, 0.02                      */
    int32_t  max_history;                         /* frames; <= 0 selects 64                                              */
} hrt_denoise_temporal_params;
int  hrt_denoise_temporal(hrt_ctx* ctx, const hrt_denoise_temporal_params* params, hrt_float3* out_radiance_host /* may be NULL */,
                          int32_t* out_color_host /* may be NULL */, float* device_ms /* may be NULL */);
/* slot 0 device pointers of the current history (all NULL, sizes 0 while it is empty): records of four floats per pixel.
 * color[4 i .. 4 i + 2] = the accumulated (after iteration 0: filtered) demodulated colour, variance = color + 3;
 * moments[4 i], [4 i + 1] = M1, M2, length = moments + 2; stride = 4 floats between pixels.  Valid until the next
 * hrt_denoise_temporal (the planes swap) or anything that empties the history. */
typedef struct hrt_denoise_history_views {
    const float *color, *moments, *length, *variance;
    int32_t width, height, stride, reserved;
} hrt_denoise_history_views;
int  hrt_denoise_history(hrt_ctx* ctx, hrt_denoise_history_views* out);
/* The same two record planes copied to the host, for hosts without a device path of their own: color_host and moments_host (either
 * may be NULL) receive width * height records of four floats, laid out as above.  Blocking, on slot 0's stream.  An empty history:
 * HRT_ERR_INVALID_STATE. */
int  hrt_denoise_history_read(hrt_ctx* ctx, float* color_host, float* moments_host);

/* Test hooks (math probes, host-side builders of derived trees) are declared in hrt_test_hooks.h and exist only in
 * libhip_raytrace_test.so, the -DHRT_TEST_HOOKS build of the same sources; the shipped library exports none of them. */
int  hrt_device_count(void);                    /* visible HIP devices, <0 on error */
const char* hrt_version(void);

#ifdef __cplusplus
}
#endif
#endif /* HIP_RAYTRACE_H */
