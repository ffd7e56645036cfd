// HipRaytrace.cs -- P/Invoke surface of libhip_raytrace.so for the reference's C# host (drop into Engine/).
// Mirrors include/hip_raytrace.h and include/hrt_host.h one to one; the Engine structs (Float3, Affine3x4, Sphere,
// MaterialRecord, TLASNode, BLASNode, InstanceRecord, MeshTri, MeshTriUV, Float2, RGBA32, TexInfo, Camera) are already
// sequential blittable value types with the layouts of include/hrt_types.h, so they cross the boundary unchanged.
// Not compiled in this repository (no .NET toolchain in the build image); the same entry points are exercised through
// the Python ctypes mirror (ilgpu_raytracing_amd/engine.py) by the test-suite.
using System;
using System.Runtime.InteropServices;

namespace ILGPU_Raytracing.Engine
{
    [StructLayout(LayoutKind.Sequential)]
    public unsafe struct HrtSceneDesc            // hrt_scene_desc: 15 x (pointer, Int64 count), order of SceneDeviceViews.cs:13-27
    {
        public TLASNode* tlasNodes;            public long n_tlasNodes;
        public int* tlasInstanceIndices;       public long n_tlasInstanceIndices;
        public InstanceRecord* instances;      public long n_instances;
        public BLASNode* blasNodes;            public long n_blasNodes;
        public int* spherePrimIdx;             public long n_spherePrimIdx;
        public Sphere* spheres;                public long n_spheres;
        public int* triPrimIdx;                public long n_triPrimIdx;
        public Float3* meshPositions;          public long n_meshPositions;
        public MeshTri* meshTris;              public long n_meshTris;
        public Float2* meshTexcoords;          public long n_meshTexcoords;
        public MeshTriUV* meshTriUVs;          public long n_meshTriUVs;
        public int* triMatIndex;               public long n_triMatIndex;
        public MaterialRecord* materials;      public long n_materials;
        public RGBA32* texels;                 public long n_texels;
        public TexInfo* texInfos;              public long n_texInfos;
    }

    [StructLayout(LayoutKind.Sequential)]
    public struct HrtFrameParams                 // hrt_frame_params: scalar fields of GBufferParams / IntegratorParams + maxDepth
    {
        public int width, height, frame;
        public Camera cam, prevCam;
        public Float3 dirLightDir, dirLightRadiance, skyTintTop, skyTintBottom;
        public int debugCamSeq, enableTemporalReuse, enableSpatialReuse, rngLockNoise, spp, maxDepth;
    }

    [Flags]
    public enum HrtFlags : uint
    {
        None = 0, Counters = 1, SkipPrimary = 2, ReferenceLayout = 4, NoSync = 8, Megakernel = 16, Streamed = 32,
        PrimaryOnly = 64, Exchanged = 128,
        Treelets = 256      // opt-in LDS-staged treelet walker: same pictures, slower than the default (DESIGN.md 5.4)
    }

    [StructLayout(LayoutKind.Sequential)]
    public struct HrtRenderOpts { public uint flags; public int row_begin, row_end, strip_n, strip_i; }

    [StructLayout(LayoutKind.Sequential)]
    public struct HrtPresentParams { public int out_width, out_height, mode; public float feedback, sharpness, clampK; }   // mode: HrtPresentMode
    public enum HrtPresentMode { Resample = 0, Taau = 1, TaauReproject = 2 }   // hrt_present_mode: blit / bilinear, TAAU, TAAU with camera reprojection
    // hrt_denoise_params: iterations 1..8 (0: 5), flags HrtDenoiseFlags, sigmas <= 0: 4.0 / 0.5 / 0.02
    [StructLayout(LayoutKind.Sequential)]
    public struct HrtDenoiseParams { public int iterations; public uint flags; public float sigma_color, sigma_normal, sigma_plane; }
    [Flags] public enum HrtDenoiseFlags : uint { None = 0, NoDemodulate = 1 }
    // hrt_denoise_temporal_params: values <= 0 select the defaults of include/hip_raytrace.h
    [StructLayout(LayoutKind.Sequential)]
    public struct HrtDenoiseTemporalParams
    {
        public int iterations; public uint flags;
        public float alpha_color, alpha_moments, sigma_lum, sigma_normal, sigma_plane, normal_cos_min, plane_tol;
        public int max_history;
    }
    [Flags] public enum HrtDenoiseTemporalFlags : uint { None = 0, NoDemodulate = 1, NoSpatial = 2, Reset = 4 }
    // hrt_denoise_history_views: slot 0 device pointers of the temporal denoiser's history, records of `stride` floats per pixel
    [StructLayout(LayoutKind.Sequential)]
    public struct HrtDenoiseHistoryViews { public IntPtr color, moments, length, variance; public int width, height, stride, reserved; }

    [StructLayout(LayoutKind.Sequential)]
    public unsafe struct HrtOutputs               // host destinations of one frame, any may be null
    {
        public int* color; public float* depth; public int* objectId; public int* cameraId;
        public Float3* radiance;
        public Float3* gb_worldPos, gb_normalWS, gb_baseColor; public int* gb_matId, gb_objId, gb_hitMask;
        public Float3* res_L, res_wi; public float* res_pdf, res_w, res_wSum; public int* res_m, res_lightId;
    }

    [StructLayout(LayoutKind.Sequential)]
    public unsafe struct HrtStats
    {
        public fixed ulong counters[20];          // 2 x hrt_kernel_counters (launch 1, launch 2)
        public fixed double kernel_ms[2]; public double d2h_ms;
        public int n_devices, counters_valid, frames, reserved;
    }

    [StructLayout(LayoutKind.Sequential)]
    public struct HrtBvhUpdateStats
    {
        public int action, tlas_nodes, tlas_slots, general_instances;
        public float growth_refit, growth_final, sah_cost, device_ms;
        public int blas_action; public float blas_growth;
    }

    [StructLayout(LayoutKind.Sequential)]
    public struct HrtRay                         // hrt_ray (32 bytes): Ray (RTUtils.cs:6-10) without invDir, plus ShadowOcclusion's tMaxWorld
    {
        public Float3 origin; public float tMax;   // tMax: occlusion queries only
        public Float3 dir; public float pad;       // dir as given, not normalised
    }

    [StructLayout(LayoutKind.Sequential)]
    public struct HrtRayHit                      // hrt_ray_hit (48 bytes): TraceClosest's out parameters (SceneDeviceViews.cs:30-86) + what was hit
    {
        public float t; public Float3 normal;      // miss: t = 1e30, normal = 0
        public Float3 albedo; public float ior;    // miss: albedo = 1, ior = 1
        public int objId, shade;                   // bestObjId / bestShade (miss: -1 / 0)
        public int instance, prim;                 // instance record; sphere or triangle index (miss: -1 / -1)
    }

    [StructLayout(LayoutKind.Sequential)]
    public struct HrtPathResult                  // hrt_path_result (32 bytes): PathTraceKernel (RTRay.cs:203-325) along a caller ray
    {
        public Float3 radiance;                    // Lout: mean over spp of SafeColor(Li), pre-pack
        public int color;                          // PackRGBA8(radiance)
        public float depth;                        // |worldPos - ray.origin|
        public int objId;                          // primary hit, -1 on a miss
        public int reserved0, reserved1;           // 0
    }

    internal static unsafe class HipRaytrace
    {
        const string Lib = "hip_raytrace";        // libhip_raytrace.so

        [DllImport(Lib)] public static extern int hrt_create(int* deviceIds, int nDev, out IntPtr ctx);
        [DllImport(Lib)] public static extern void hrt_destroy(IntPtr ctx);
        [DllImport(Lib)] public static extern IntPtr hrt_last_error(IntPtr ctx);
        [DllImport(Lib)] public static extern int hrt_scene_upload(IntPtr ctx, HrtSceneDesc* scene);
        // BvhManager.BuildOrRefit(scene, policy) for moved instances: policy = (int)RebuildPolicy (Auto 0, ForceRefit 1, ForceRebuild 2);
        // hrt_scene_update_positions also takes policy | HRT_REBUILD_BLAS (16): new BLAS topology for every mesh
        public const int HRT_REBUILD_BLAS = 16;
        [DllImport(Lib)] public static extern int hrt_scene_update_instances(IntPtr ctx, int* instanceIds, int n, Affine3x4* objectToWorld, int policy, HrtBvhUpdateStats* stats);
        [DllImport(Lib)] public static extern int hrt_scene_update_positions(IntPtr ctx, long firstVertex, long n, Float3* positions, int policy, HrtBvhUpdateStats* stats);
        [DllImport(Lib)] public static extern int hrt_scene_update_spheres(IntPtr ctx, long firstSphere, long n, Sphere* spheres, int policy, HrtBvhUpdateStats* stats);
        [DllImport(Lib)] public static extern int hrt_scene_download_array(IntPtr ctx, int dev, int array, void* dst, long cap, long* count);
        [DllImport(Lib)] public static extern int hrt_scene_download_tlas(IntPtr ctx, int dev, TLASNode* nodes, long capNodes, int* indices, long capIndices, InstanceRecord* instances, long capInstances, long* counts);
        [DllImport(Lib)] public static extern int hrt_render_frame(IntPtr ctx, HrtFrameParams* p, HrtRenderOpts* opts, HrtOutputs* outputs, HrtStats* stats);
        // progressive frames: samples [sampleBegin, p->spp) of the frame p describes; afterwards every output equals hrt_render_frame(p).
        // sampleBegin 0 starts a frame, > 0 continues the last one (same params except spp, sampleBegin = its spp; hrt_present may run between)
        [DllImport(Lib)] public static extern int hrt_render_progressive(IntPtr ctx, HrtFrameParams* p, HrtRenderOpts* opts, int sampleBegin, HrtOutputs* outputs, HrtStats* stats);
        [DllImport(Lib)] public static extern int hrt_present(IntPtr ctx, HrtPresentParams* p, int* outColorHost);
        [DllImport(Lib)] public static extern int hrt_present_time(IntPtr ctx, float* ms);
        public const int HRT_PRESENT_DENOISED = 0x100;   // OR into HrtPresentParams.mode: resolve the denoised colour of the last hrt_denoise
        // a-trous denoiser over the last full-image frame; either host destination may be null (the planes stay on device slot 0)
        [DllImport(Lib)] public static extern int hrt_denoise(IntPtr ctx, HrtDenoiseParams* p, Float3* outRadianceHost, int* outColorHost, float* deviceMs);
        [DllImport(Lib)] public static extern int hrt_denoised_buffers(IntPtr ctx, IntPtr* radiance, IntPtr* color);
        // the temporal, variance-guided denoiser: one call per frame, the same result planes as hrt_denoise
        [DllImport(Lib)] public static extern int hrt_denoise_temporal(IntPtr ctx, HrtDenoiseTemporalParams* p, Float3* outRadianceHost, int* outColorHost, float* deviceMs);
        [DllImport(Lib)] public static extern int hrt_denoise_history(IntPtr ctx, HrtDenoiseHistoryViews* views);
        [DllImport(Lib)] public static extern int hrt_denoise_history_read(IntPtr ctx, float* colorHost, float* momentsHost);   // 4 floats per pixel each, either may be null
        // camera motion vectors of the last full-image frame, in pixels; fromCam null: the frame's prevCam; dev < 0 host memory, 0 device memory of slot 0
        [DllImport(Lib)] public static extern int hrt_motion_vectors(IntPtr ctx, Camera* fromCam, Float2* mv, int dev, float* deviceMs);
        [DllImport(Lib)] public static extern int hrt_synchronize(IntPtr ctx, HrtStats* stats);
        [DllImport(Lib)] public static extern int hrt_reset_history(IntPtr ctx);
        // page-lock the managed framebuffer arrays once (GCHandle.Alloc(array, GCHandleType.Pinned).AddrOfPinnedObject()): gathers
        // into them become asynchronous DMA; keep the handles alive until hrt_host_unregister / hrt_destroy
        [DllImport(Lib)] public static extern int hrt_host_register(IntPtr ctx, void* ptr, long bytes);
        [DllImport(Lib)] public static extern int hrt_host_unregister(IntPtr ctx, void* ptr);
        [DllImport(Lib)] public static extern int hrt_frame_times(IntPtr ctx, int dev, int launch, float* ms, int cap, int* n);
        [DllImport(Lib)] public static extern int hrt_set_workspace_limit(IntPtr ctx, long maxResidentPaths);
        [DllImport(Lib)] public static extern int hrt_device_count();
        // SceneDeviceViews.TraceClosest / ShadowOcclusion over caller rays: query 0 = closest (results: HrtRayHit[n]), 1 = occluded
        // (results: int[n] of 0/1).  dev < 0: host arrays, split over every device slot; dev >= 0: device pointers of that slot.  Blocking.
        public const int HRT_QUERY_CLOSEST = 0, HRT_QUERY_OCCLUDED = 1;
        [DllImport(Lib)] public static extern int hrt_trace_rays(IntPtr ctx, int query, HrtRay* rays, long n, void* results, int dev, float* deviceMs);
        // the k nearest accepted hits along each ray (k <= HRT_HITS_MAX): hits[i * k + j] for j < counts[i], CLOSEST's miss record after;
        // totals (may be null): every accepted test of ray i.  Arguments, devices and blocking as hrt_trace_rays.
        public const int HRT_HITS_MAX = 16;
        [DllImport(Lib)] public static extern int hrt_trace_hits(IntPtr ctx, HrtRay* rays, long n, int k, HrtRayHit* hits, int* counts, int* totals, int dev, float* deviceMs);
        [DllImport(Lib)] public static extern int hrt_trace_paths(IntPtr ctx, HrtFrameParams* p, uint flags, HrtRay* rays, long n, long firstKey, HrtPathResult* results, int dev, float* deviceMs);

        // native asset loader (optional: a C# host may keep MeshLoaderOBJ)
        [DllImport(Lib)] public static extern IntPtr hrth_scene_new();
        [DllImport(Lib)] public static extern void hrth_scene_free(IntPtr scene);
        [DllImport(Lib)] public static extern int hrth_scene_load_obj_instance(IntPtr scene, [MarshalAs(UnmanagedType.LPUTF8Str)] string objPath, Affine3x4* objectToWorld, float uniformScale);
        [DllImport(Lib)] public static extern void hrth_scene_get_desc(IntPtr scene, HrtSceneDesc* desc);
        [DllImport(Lib)] public static extern IntPtr hrth_last_error();

        /// <summary>Turns a negative hrt_status into the exception type the reference's own classes throw.</summary>
        public static void Check(IntPtr ctx, int rc)
        {
            if (rc >= 0) return;
            string msg = Marshal.PtrToStringAnsi(hrt_last_error(ctx)) ?? "hip_raytrace error";
            throw rc switch
            {
                -1 => new ArgumentException(msg),              // HRT_ERR_INVALID_ARG   (ArgumentNull/OutOfRange in Framebuffer.cs:62,101-102)
                -2 => new InvalidOperationException(msg),      // HRT_ERR_INVALID_STATE
                -5 => new OutOfMemoryException(msg),           // HRT_ERR_OUT_OF_MEMORY
                _ => new Exception(msg),                       // HRT_ERR_HIP / HRT_ERR_NO_DEVICE: CudaException analogue
            };
        }
    }
}
