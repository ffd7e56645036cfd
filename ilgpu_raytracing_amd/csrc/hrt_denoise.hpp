// hrt_denoise.hpp -- launch interface of the edge-avoiding a-trous denoiser (hrt_denoise; kernels in hrt_denoise.hip).
//
// The kernels live in a translation unit of their own, as the queries' do (hrt_paths.hpp, hrt_hits.hpp), so the frame's kernels in
// hrt_runtime.hip keep their code.  The filter is defined in include/hip_raytrace.h; what is here is its data layout.
//
// A tap reads three aligned 16-byte words of the neighbour instead of seven scattered arrays:
//   guide[2 i]     = (n.x, n.y, n.z, kx)           kx = 1 / (sigma_plane^2 * max(depth^2, 1e-12)), used for the CENTRE pixel only
//   guide[2 i + 1] = (P.x, P.y, P.z, bits(hit))    hit = gb_hitMask[i] != 0
//   colour[i]      = (c.x, c.y, c.z, 0)            the demodulated radiance, ping-ponged between two planes
// The prepare kernel writes guide and colour plane 0; iteration i reads plane i & 1 and writes the other; the last iteration
// multiplies the albedo back and writes the denoised radiance and its packed colour instead.
#pragma once
#include "hrt_device.hpp"

struct DenoiseLaunch {
    int width, height;
    int iterations;           // 1..8
    bool demodulate;
    float sigma_color;        // iteration i: sc = sigma_color * 2^-i, kc = 1 / (sc * sc), evaluated by denoise_launch
    float kn;                 // 1 / (sigma_normal * sigma_normal)
    float sp2;                // sigma_plane * sigma_plane
    // the frame (read only)
    const hrt_float3 *radiance, *normalWS, *worldPos, *baseColor;
    const float* depth;
    const int32_t* hitMask;
    // workspace and results, width * height elements each (guide: 2 float4 per pixel)
    float4 *guide, *colour[2];
    hrt_float3* outRadiance;
    int32_t* outColor;
};

// enqueues prepare and the iterations on st
hipError_t denoise_launch(const DenoiseLaunch& L, hipStream_t st);
