// hrt_denoise_temporal.hpp -- launch interface of the temporal denoiser (hrt_denoise_temporal; kernels in hrt_denoise_temporal.hip).
//
// A translation unit of its own, as hrt_denoise.hip: the frame's kernels in hrt_runtime.hip and hrt_denoise's keep their code.  The
// filter is defined in include/hip_raytrace.h; what is here is its data layout.  Everything a tap reads is a 16-byte record:
//   guide[2 i]     = (n.x, n.y, n.z, kx)           as hrt_denoise.hpp; two sets, this call's and the previous call's (the history's geometry)
//   guide[2 i + 1] = (P.x, P.y, P.z, bits(hit))
//   colour[i]      = (c.x, c.y, c.z, v)            demodulated colour and its variance: work planes, ping-ponged by the a-trous passes
//   hcol[i]        = (C.x, C.y, C.z, v)            history colour: what iteration 0 wrote (NO_SPATIAL: what the temporal step wrote)
//   hmom[i]        = (M1, M2, N, 0)                luminance moments and history length
// hcol and hmom are pairs (read: the previous call's, written: this call's), swapped by the host after every call.
#pragma once
#include "hrt_device.hpp"
#include "hrt_post.hpp"

struct DenoiseTemporalLaunch {
    int width, height;
    int iterations;           // 1..8
    bool demodulate, spatial, haveHistory;
    float kn, sp2;            // 1 / (sigma_normal * sigma_normal), sigma_plane * sigma_plane
    float sigma_lum, alpha_color, alpha_moments, normal_cos_min, plane_tol, max_history;
    hrt::ProjCam histCam, curCam;
    // the frame (read only)
    const hrt_float3 *radiance, *normalWS, *worldPos, *baseColor;
    const float* depth;
    const int32_t* hitMask;
    // history and workspace, width * height records each (guide: 2 per pixel)
    float4* guideCur;
    const float4 *guidePrev, *hcolPrev, *hmomPrev;
    float4 *hcolNew, *hmomNew, *work[2];
    hrt_float3* outRadiance;
    int32_t* outColor;
};

// enqueues the temporal step, the variance estimate and the iterations on st
hipError_t denoise_temporal_launch(const DenoiseTemporalLaunch& L, hipStream_t st);
