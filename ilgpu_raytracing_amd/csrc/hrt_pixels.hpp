// hrt_pixels.hpp -- the pixel <-> lane mapping and the occupancy of the fused path-trace kernels, shared by the frame's kernels
// (hrt_runtime.hip) and the radiance queries' (hrt_paths.hip).
#pragma once
#include "hrt_trace_packed.hpp"

using namespace hrt;

// ---------------------------------------------------------------------------------------
// Pixel <-> lane mapping.  A 256-thread workgroup shades a 32x8 pixel tile: each of its 4
// waves owns one 8x8 sub-tile (lane l -> (l&7, l>>3)), so the 64 rays of a wave leave the
// camera through a compact square and walk nearly the same BVH nodes.  Workgroup ids are
// dealt round-robin over the 8 XCDs by the dispatcher; remap() hands every XCD one
// contiguous band of tiles so each private 4 MiB L2 caches one region of the BVH instead
// of all of it (bijective form of the T1 remap, cdna_hip_programming.md).  Frames of a small scene (<= kSmallSceneNodes, hrt_scene.hip, in
// the fused kernels) skip the remap (band = 0): their BVH is a few cache lines, and the identity map gives every XCD tiles from
// the whole image (60 tiles per row is not a multiple of 8), so no XCD waits on the heaviest band of rows.
// ---------------------------------------------------------------------------------------
struct TileMap { int tilesX, tilesY, nTiles, wpb, band; };      // wpb: waves (8x8 pixel tiles) per workgroup, side by side

__device__ __forceinline__ bool tile_pixel(const TileMap& tm, const FrameK& k, int& x, int& y, int orig)
{
    int tile = orig;
    if (tm.band)
    {
        int q = tm.nTiles >> 3, r = tm.nTiles & 7;
        int xcd = orig & 7, seq = orig >> 3;
        tile = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + seq;
    }
    int ty = tile / tm.tilesX, tx = tile - ty * tm.tilesX;
    int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    x = (tx * tm.wpb + wave) * 8 + (lane & 7);
    y = k.row_begin + (ty * k.strip_n + k.strip_i) * 8 + (lane >> 3);   // 8-row strips dealt round-robin over tiles
    return x < k.width && y < k.row_end;
}

#ifndef HRT_PT_WAVES
#define HRT_PT_WAVES 4   // 128-VGPR cap: 4 waves/SIMD hide the dependent node loads better than 2 at 204 VGPRs (measured)
#endif
// The leaf-sweep tracer is the exception: at 5 waves/SIMD (102 VGPRs, 112 bytes of scratch per lane) the fused kernel of
// config 2 is 2 % faster than at 4 (VALU-bound: one more wave to issue from is worth the spill traffic); 6 and 3 lose 12 %.
// Every other tracer spills two to four times as much there and keeps 4.
template <class TR> struct PtWaves { static constexpr int value = HRT_PT_WAVES; };
#ifndef HRT_PT_WAVES_FLAT
#define HRT_PT_WAVES_FLAT (HRT_PT_WAVES + 1)
#endif
template <> struct PtWaves<TracerFlat> { static constexpr int value = HRT_PT_WAVES_FLAT; };
