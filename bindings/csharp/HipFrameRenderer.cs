// HipFrameRenderer.cs -- what RTRenderer's device side becomes when the two ILGPU kernel launches and the presentation
// kernels are replaced by libhip_raytrace.so.  RTRenderer keeps its camera controller, sun animation, TAAU switch and
// render scale and calls Render() where it used to launch _primaryKernel / _integratorKernel / _taa (RTRenderer.cs:105-237);
// Scene.UploadAll calls Upload() with its pinned host lists.  Shipped as source; see INTEGRATION.md.
using System;
using System.Runtime.InteropServices;

namespace ILGPU_Raytracing.Engine
{
    public sealed unsafe class HipFrameRenderer : IDisposable
    {
        private IntPtr _ctx;
        private int[] _display = Array.Empty<int>();      // RGBA8 display image (what the PBO received)

        /// <param name="deviceIds">one id: one GPU; several ids: one frame row-tiled over the GPUs of the node.</param>
        public HipFrameRenderer(params int[] deviceIds)
        {
            if (deviceIds == null || deviceIds.Length == 0) deviceIds = new[] { 0 };
            fixed (int* ids = deviceIds)
                HipRaytrace.Check(IntPtr.Zero, HipRaytrace.hrt_create(ids, deviceIds.Length, out _ctx));
        }

        /// <summary>Scene.UploadAll: the 15 host lists, pinned by the caller for the duration of the call (empty list: null, 0).</summary>
        public void Upload(in HrtSceneDesc scene)
        {
            fixed (HrtSceneDesc* p = &scene)
                HipRaytrace.Check(_ctx, HipRaytrace.hrt_scene_upload(_ctx, p));
        }

        /// <summary>One RenderDirectToPbo: both launches at (inW, inH), then TAAU or blit/bilinear to (outW, outH).
        /// Returns the display image (row 0 = bottom row, 0xAARRGGBB), valid until the next call.</summary>
        public ReadOnlySpan<int> Render(in HrtFrameParams frame, int outW, int outH, bool taau)
        {
            fixed (HrtFrameParams* fp = &frame)
                HipRaytrace.Check(_ctx, HipRaytrace.hrt_render_frame(_ctx, fp, null, null, null));      // blocking, results stay on the device
            return Present(outW, outH, taau);
        }

        /// <summary>Render with the present mode spelled out: HrtPresentMode.TaauReproject reads the TAAU history where the camera's
        /// motion since the last resolved frame puts it (the reprojection RTTaa.ResolveUpsample declares and leaves out).</summary>
        public ReadOnlySpan<int> Render(in HrtFrameParams frame, int outW, int outH, HrtPresentMode mode)
        {
            fixed (HrtFrameParams* fp = &frame)
                HipRaytrace.Check(_ctx, HipRaytrace.hrt_render_frame(_ctx, fp, null, null, null));
            return Present(outW, outH, mode);
        }

        /// <summary>One step of a progressive frame: samples [sampleBegin, frame.spp) of the frame, then the same presentation as
        /// Render.  sampleBegin 0 starts the frame; a later step passes the same frame with a larger spp and sampleBegin = the spp of
        /// the step before.  The returned preview is what Render(frame) would return at frame.spp samples, and the last step's is the
        /// finished frame.  Throws InvalidOperationException when the step does not continue the last one.</summary>
        public ReadOnlySpan<int> RenderProgressive(in HrtFrameParams frame, int sampleBegin, int outW, int outH, bool taau)
        {
            fixed (HrtFrameParams* fp = &frame)
                HipRaytrace.Check(_ctx, HipRaytrace.hrt_render_progressive(_ctx, fp, null, sampleBegin, null, null));   // blocking, results stay on the device
            return Present(outW, outH, taau);
        }

        private ReadOnlySpan<int> Present(int outW, int outH, bool taau) => Present(outW, outH, taau ? HrtPresentMode.Taau : HrtPresentMode.Resample);

        /// <summary>Presents the last frame again (or for the first time) with the given mode; the history follows the frames that
        /// were actually resolved, so skipping or repeating a present is safe in every mode.</summary>
        public ReadOnlySpan<int> Present(int outW, int outH, HrtPresentMode mode, bool denoised = false)
        {
            if (_display.Length != outW * outH) _display = new int[outW * outH];
            var pp = new HrtPresentParams { out_width = outW, out_height = outH, mode = (int)mode | (denoised ? HipRaytrace.HRT_PRESENT_DENOISED : 0) };   // tunables <= 0: the reference's 0.075 / 0.10 / 1.25
            fixed (int* dst = _display)
                HipRaytrace.Check(_ctx, HipRaytrace.hrt_present(_ctx, &pp, dst));
            return _display;
        }

        /// <summary>Edge-avoiding a-trous denoiser over the radiance of the last full-image frame, guided by its G-buffer (hrt_denoise).
        /// The frame is left as it is; Present(..., denoised: true) resolves the denoised colour until the next frame.  radiance / color
        /// (internal size, either may be empty) receive the denoised planes.  Returns the HIP-event time of the kernels in ms.</summary>
        public float Denoise(Span<Float3> radiance = default, Span<int> color = default, int iterations = 0, bool demodulate = true,
                             float sigmaColor = 0f, float sigmaNormal = 0f, float sigmaPlane = 0f)
        {
            var dp = new HrtDenoiseParams { iterations = iterations, flags = (uint)(demodulate ? HrtDenoiseFlags.None : HrtDenoiseFlags.NoDemodulate),
                                            sigma_color = sigmaColor, sigma_normal = sigmaNormal, sigma_plane = sigmaPlane };
            float ms = 0f;
            fixed (Float3* r = radiance)
            fixed (int* c = color)
                HipRaytrace.Check(_ctx, HipRaytrace.hrt_denoise(_ctx, &dp, radiance.IsEmpty ? null : r, color.IsEmpty ? null : c, &ms));
            return ms;
        }

        /// <summary>The temporal denoiser (hrt_denoise_temporal): accumulates the demodulated radiance and its luminance moments of the last
        /// full-image frame into a history reprojected with the camera's motion, then filters with a-trous passes guided by the per-pixel
        /// variance.  Call it once per frame; Present(..., denoised: true) resolves the result.  p null: every default.  Returns the
        /// HIP-event time of the kernels in ms.</summary>
        public float DenoiseTemporal(Span<Float3> radiance = default, Span<int> color = default, HrtDenoiseTemporalParams? p = null)
        {
            var tp = p ?? default;
            float ms = 0f;
            fixed (Float3* r = radiance)
            fixed (int* c = color)
                HipRaytrace.Check(_ctx, HipRaytrace.hrt_denoise_temporal(_ctx, &tp, radiance.IsEmpty ? null : r, color.IsEmpty ? null : c, &ms));
            return ms;
        }

        /// <summary>Camera motion vectors of the last full-image frame (hrt_motion_vectors), one per internal pixel, in pixels: where the
        /// pixel's surface point was in fromCam's image minus where it is now; NaN where the point is behind either camera.
        /// fromCam null: the frame's prevCam.</summary>
        public void MotionVectors(Span<Float2> mv, Camera? fromCam = null)
        {
            Camera cam = fromCam.GetValueOrDefault();
            fixed (Float2* dst = mv)
                HipRaytrace.Check(_ctx, HipRaytrace.hrt_motion_vectors(_ctx, fromCam.HasValue ? &cam : null, dst, -1, null));
        }

        /// <summary>Picking: the closest hit under pixel (x, y) of a width x height frame (row 0 = bottom row) seen through `cam`, the
        /// camera the frame was rendered with.  The ray is the primary-visibility launch's pixel-centre ray (RTRay.cs:120-126,
        /// Ray.GenerateRay RTUtils.cs:13-17), so the hit is what the G-buffer holds at that pixel.</summary>
        public HrtRayHit Pick(in Camera cam, int width, int height, int x, int y)
        {
            float u = (x + 0.5f) / Math.Max(1, width), v = (y + 0.5f) / Math.Max(1, height);
            Ray r = Ray.GenerateRay(cam, u, v);
            var ray = new HrtRay { origin = r.origin, dir = r.dir, tMax = 1e30f };
            HrtRayHit hit;
            HipRaytrace.Check(_ctx, HipRaytrace.hrt_trace_rays(_ctx, HipRaytrace.HRT_QUERY_CLOSEST, &ray, 1, &hit, -1, null));
            return hit;
        }

        /// <summary>The k nearest hits along each ray (hrt_trace_hits): hits[i * k + j], j &lt; counts[i], in ascending (t, instance, prim);
        /// the remaining slots hold the miss record.  totals (optional, one per ray): every accepted hit of the ray.  Returns rays.Length.</summary>
        public int TraceHits(ReadOnlySpan<HrtRay> rays, int k, Span<HrtRayHit> hits, Span<int> counts, Span<int> totals = default)
        {
            if (k < 1 || k > HipRaytrace.HRT_HITS_MAX) throw new ArgumentOutOfRangeException(nameof(k));
            if (hits.Length < (long)rays.Length * k) throw new ArgumentException("hits is shorter than rays.Length * k");
            if (counts.Length < rays.Length) throw new ArgumentException("counts is shorter than rays");
            if (!totals.IsEmpty && totals.Length < rays.Length) throw new ArgumentException("totals is shorter than rays");
            fixed (HrtRay* r = rays) fixed (HrtRayHit* h = hits) fixed (int* c = counts) fixed (int* t = totals)
                HipRaytrace.Check(_ctx, HipRaytrace.hrt_trace_hits(_ctx, r, rays.Length, k, h, c, totals.IsEmpty ? null : t, -1, null));
            return rays.Length;
        }

        /// <summary>Picking through surfaces: the k nearest hits under pixel (x, y), nearest first, on the ray Pick casts.</summary>
        public HrtRayHit[] PickAll(in Camera cam, int width, int height, int x, int y, int k)
        {
            float u = (x + 0.5f) / Math.Max(1, width), v = (y + 0.5f) / Math.Max(1, height);
            Ray r = Ray.GenerateRay(cam, u, v);
            var ray = new HrtRay { origin = r.origin, dir = r.dir, tMax = float.PositiveInfinity };
            var hits = new HrtRayHit[k];
            var counts = new int[1];
            TraceHits(new ReadOnlySpan<HrtRay>(&ray, 1), k, hits, counts);
            return hits.AsSpan(0, counts[0]).ToArray();
        }

        /// <summary>Radiance along caller rays (hrt_trace_paths): ray i is path-traced as pixel key firstKey + i of the frame `p`
        /// describes (reuse off), with its own origin and direction in place of the camera's.  Panoramas, probes, custom cameras.
        /// The frame's own camera rays in pixel order give the frame's colour, radiance, depth and objectId bit for bit.</summary>
        public void TracePaths(in HrtFrameParams p, ReadOnlySpan<HrtRay> rays, Span<HrtPathResult> results, long firstKey = 0, uint flags = 0)
        {
            if (results.Length < rays.Length) throw new ArgumentException("results is shorter than rays");
            HrtFrameParams pp = p;
            fixed (HrtRay* r = rays) fixed (HrtPathResult* o = results)
                HipRaytrace.Check(_ctx, HipRaytrace.hrt_trace_paths(_ctx, &pp, flags, r, rays.Length, firstKey, o, -1, null));
        }

        /// <summary>Framebuffer.EnsureLength / RTTaa.Ensure side effect the host may want explicitly (camera cut).</summary>
        public void ResetHistory() => HipRaytrace.Check(_ctx, HipRaytrace.hrt_reset_history(_ctx));

        public void Dispose()
        {
            if (_ctx != IntPtr.Zero) { HipRaytrace.hrt_destroy(_ctx); _ctx = IntPtr.Zero; }
        }
    }
}
