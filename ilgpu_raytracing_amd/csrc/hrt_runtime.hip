// hrt_runtime.hip -- libhip_raytrace.so: kernels' entry points + the part of the C ABI of
// include/hip_raytrace.h that launches them (context, frame render, multi-device row tiling,
// presentation, motion vectors, queries, denoisers) + the test hooks.  The scene entry points
// are hrt_scene.hip's; what the host units share is hrt_ctx.hpp.  Host code that launches no
// kernel of this unit does not belong here.
//
// Replaces the ILGPU accelerator / kernel-launch layer of the reference
// (Engine/RTRenderer.cs:66-68,85-86,118-120,152-153,164,181-205,233; Engine/Scene.cs:258-279,
//  370-377; Engine/Framebuffer.cs:60-97,127-146,228-253).  HIP runtime only: no torch, no
// CPU fallback -- every entry point fails with HRT_ERR_NO_DEVICE / HRT_ERR_HIP when no
// MI355X is usable.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <functional>
#include <new>
#include <string>
#include <thread>
#include <vector>
#include <cmath>
#include <cfloat>
#include <utility>
#include "hrt_ctx.hpp"
#include "hrt_device.hpp"
#include "hrt_trace_packed.hpp"
#include "hrt_wavefront.hpp"
#include "hrt_walker_tl.hpp"
#include "hrt_bvh.hpp"
#include "hrt_post.hpp"
#include "hrt_query.hpp"
#include "hrt_paths.hpp"
#include "hrt_hits.hpp"
#include "hrt_denoise.hpp"
#include "hrt_denoise_temporal.hpp"
#include "../../include/hip_raytrace.h"
#ifdef HRT_TEST_HOOKS
#include "hrt_scene_pack.hpp"          // the host-only hooks call the scene validator and the second tree's host code
#include "../../include/hrt_test_hooks.h"
#endif

using namespace hrt;
using namespace hrt::detail;


#include "hrt_pixels.hpp"

// TR = TracerPacked (fast, device-private layout) or TracerRef (the reference's array layout);
// COUNT = work-counter build.
template <class TR, bool COUNT>
__global__ void __launch_bounds__(256)
hrt_primary_kernel(TR tr, FrameK k, DGBuffer gb, TileMap tm, unsigned long long* counters)
{
    Cnt<COUNT> C;
    int x, y;
    if (tile_pixel(tm, k, x, y, blockIdx.x)) primary_pixel<TR, COUNT>(tr, k, gb, y * k.width + x, C);
    C.flush(counters);
}

template <class TR, bool COUNT, bool REUSE = true>
__global__ void __launch_bounds__(256, PtWaves<TR>::value)
hrt_path_trace_kernel(TR tr, FrameK k, DGBuffer gb, DFramebuffer fb, DReservoir resPrev, DReservoir resCur,
                      long long nPix, TileMap tm, unsigned long long* counters)
{
    Cnt<COUNT> C;
    int x, y;
    if (tile_pixel(tm, k, x, y, blockIdx.x)) path_trace_pixel<TR, COUNT, false, REUSE>(tr, k, gb, fb, resPrev, resCur, nPix, y * k.width + x, C);
    C.flush(counters);
}

// Small tiles (a rank's share of a frame tiled over 4 or 8 GPUs, small images): one wave per 8x8 pixels running all samples
// fills the machine for about one round, and the launch lasts as long as its slowest wave.  The samples of a pixel are
// independent up to the ordered sum and the last-writer reservoir, so the launch is cut into sample groups (workgroup =
// tile x group) and a resolve pass puts the pixel together in sample order: same values, several rounds of shorter waves.
template <class TR, bool REUSE = true>
__global__ void __launch_bounds__(256, PtWaves<TR>::value)
hrt_path_trace_split_kernel(TR tr, FrameK k, DGBuffer gb, DFramebuffer fb, DReservoir resPrev, DReservoir resCur,
                            long long nPix, TileMap tm, hrt_float3* li, float* stage, int nGroups, int perGroup)
{
    Cnt<false> C;
    const int g = blockIdx.x / tm.nTiles;
    SplitK sk;
    sk.li = li; sk.stage = stage; sk.group = g; sk.nGroups = nGroups;
    sk.sBegin = g * perGroup; sk.sEnd = min(sk.sBegin + perGroup, max(1, k.spp));
    const int tileBlock = blockIdx.x - g * tm.nTiles;
    sk.local = tileBlock * (int)blockDim.x + (int)threadIdx.x; sk.nLocal = tm.nTiles * (int)blockDim.x;
    int x, y;
    if (tile_pixel(tm, k, x, y, tileBlock)) path_trace_pixel<TR, false, true, REUSE>(tr, k, gb, fb, resPrev, resCur, nPix, y * k.width + x, C, &sk);
}

__global__ void __launch_bounds__(256)
hrt_split_resolve_kernel(FrameK k, DGBuffer gb, DFramebuffer fb, DReservoir resCur, long long nPix, TileMap tm, const hrt_float3* li, const float* stage, int nGroups)
{
    int x, y;
    if (tile_pixel(tm, k, x, y, blockIdx.x)) split_resolve_pixel(k, gb, fb, resCur, y * k.width + x, li, stage, nGroups,
                                                                 (int)(blockIdx.x * blockDim.x + threadIdx.x), tm.nTiles * (int)blockDim.x);
}

// ---------------------------------------------------------------------------------------
// Streamed path-trace stage (hrt_wavefront.hpp): one wave per range of kRange path slots.
// Ranges are handed to workgroups through the same per-XCD contiguous remap as pixel tiles,
// so neighbouring ranges (neighbouring screen regions) share an L2.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ int wf_range(int nRanges)
{
    int nBlocks = gridDim.x, orig = blockIdx.x;
    int q = nBlocks >> 3, r = nBlocks & 7;
    int xcd = orig & 7, seq = orig >> 3;
    int blk = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + seq;
    int range = blk * 4 + (threadIdx.x >> 6);
    return range < nRanges ? range : -1;
}

// FIRST: depth 0, vertices straight from the G-buffer (every wave takes part in the workgroup's packing of the live paths)
template <bool COUNT, bool FIRST>
__global__ void __launch_bounds__(256)
hrt_wf_shade_kernel(FrameK k, WfGeom g, DGBuffer gb, DReservoir resPrev, long long nPix, WfBuffers W, int vsel, int depth, unsigned long long* counters)
{
    Cnt<COUNT> C;
    int range = wf_range(W.nRanges);
    if (FIRST || range >= 0) wf_shade_wave<COUNT, FIRST>(k, g, gb, resPrev, nPix, W, vsel ? W.B : W.A, depth, range, C);
    C.flush(counters);
}

#ifndef HRT_WALK_BLOCKS_PER_CU
#define HRT_WALK_BLOCKS_PER_CU 4               // persistent workgroups per CU of a chained walk launch: 16 of the 32 wave slots a CU has at <= 64 VGPRs.
                                               // Fewer rays in flight, but their tree nodes stay in L1 / L2: 3 / 4 / 5 / 6 / 8 / 12 measured
#endif
constexpr int kWalkBlocksPerCU = HRT_WALK_BLOCKS_PER_CU;
#ifndef HRT_WALK_BLOCKS_PER_CU_2LANES
#define HRT_WALK_BLOCKS_PER_CU_2LANES 2        // ... per lane when two sample batches are in flight: 2 / 3 / 4 / 6 measured on configs 4 / 5 at 64 / 256 spp:
                                               // 314 / 322 / 328 / 342 ms and 1287 / 1298 / 1318 / 1387 ms
#endif
constexpr int kWalkBlocksPerCU2 = HRT_WALK_BLOCKS_PER_CU_2LANES;
// Walk launches either give every wave one path range (static) or let persistent waves pull ranges until none is
// left (chained, RangeGrab).  Measured, path stage of configs 3 / 4 / 5: static 33.5 / 56.4 / 32.8 ms, chained
// 36.2 / 37.2 / 21.7 ms: the triangle scenes gain 1.5x from full lanes, the sphere-instance scene is bound by L1
// accesses (more live lanes do not help it) and loses the L1 sharing of four neighbouring ranges per workgroup.
#ifndef HRT_WF_TRACE_WAVES
#define HRT_WF_TRACE_WAVES 4
#endif
template <class TR, bool COUNT>
__global__ void __launch_bounds__(256, HRT_WF_TRACE_WAVES)
hrt_wf_shadow_kernel(TR tr, WfBuffers W, int vsel, int depth, unsigned long long* counters)
{
    Cnt<COUNT> C;
    int range = wf_range(W.nRanges);
    if (range >= 0) wf_shadow_wave<TR, COUNT>(tr, W, vsel ? W.B : W.A, depth, range, C);
    C.flush(counters);
}

template <class TR, bool COUNT>
__global__ void __launch_bounds__(256, HRT_WF_TRACE_WAVES)
hrt_wf_closest_kernel(TR tr, FrameK k, WfBuffers W, int vsel, int depth, unsigned long long* counters)
{
    Cnt<COUNT> C;
    int range = wf_range(W.nRanges);
    if (range >= 0) wf_closest_wave<TR, COUNT>(tr, k, W, vsel ? W.B : W.A, vsel ? W.A : W.B, depth, range, C);
    C.flush(counters);
}

// persistent-wave walk kernels (packed layout only) + the finish kernel that shades the winners
// ALT: `tr` walks the device-built tree over the same fast-sphere instances (boolean queries do not depend on the tree,
// hrt_walker.hpp); `exact` is the uploaded tree, for rays whose slab arithmetic is not finite
template <int FEAT, bool COUNT, bool ALT = false, int LT = 2>
__global__ void __launch_bounds__(256, HRT_WF_TRACE_WAVES)
hrt_wf_walk_shadow_kernel(TracerPackedT<FEAT> tr, TracerPackedT<FEAT> exact, WfBuffers W, int vsel, int depth, int chained, unsigned long long* counters)
{
    Cnt<COUNT> C;
    int own = -1;
    if (!chained) { own = wf_range(W.nRanges); if (own < 0) own = W.nRanges; }
    W = W.at_depth(depth);
    wf_walk_shadow_wave<FEAT, COUNT, ALT, LT>(tr, exact, W, vsel ? W.B : W.A, depth, W.grab + (depth * 2 + 0) * 8, own, C);
    C.flush(counters);
}

// EXISTS: the closest-hit walk of the last bounce, where only hit-or-miss is used (hrt_walker.hpp)
template <int FEAT, bool COUNT, bool EXISTS = false, bool ALT = false, int LT = 2>
__global__ void __launch_bounds__(256, HRT_WF_TRACE_WAVES)
hrt_wf_walk_closest_kernel(TracerPackedT<FEAT> tr, TracerPackedT<FEAT> exact, WfBuffers W, int depth, int chained, unsigned long long* counters)
{
    Cnt<COUNT> C;
    int own = -1;
    if (!chained) { own = wf_range(W.nRanges); if (own < 0) own = W.nRanges; }
    W = W.at_depth(depth);
    wf_walk_closest_wave<FEAT, COUNT, EXISTS, ALT, LT>(tr, exact, W, depth, W.grab + (depth * 2 + 1) * 8, own, C);
    C.flush(counters);
}

// ---------------------------------------------------------------------------------------
// Treelet-queued walks (hrt_walker_tl.hpp): production frames of scenes with big triangle meshes.
// PHASE 0 fresh rays of the path ranges; PHASE 1 one round over the rays binned by treelet, a span of the binned list per
// workgroup, each treelet of the span staged once in LDS; PHASE 2 clean-up of what is still suspended, from global memory.
// ---------------------------------------------------------------------------------------
template <int FEAT, bool ANY, bool EXISTS, int LT, int PHASE>
__global__ void __launch_bounds__(256, PHASE == 1 ? 2 : 4)
hrt_tl_walk_kernel(TracerPackedT<FEAT> tr, DTreelets T, TlQueues Q, WfBuffers W, int depth, int histBins, int tlRegion, int round)
{
    const TlShared sh = tl_shared(tlRegion, T.redLds, histBins);
    W = W.at_depth(depth);
    {   // the top of the reduced tree stays in LDS for the whole kernel
        float4* red = const_cast<float4*>(sh.red);
        const float4* src = reinterpret_cast<const float4*>(T.red);
        for (int i = threadIdx.x; i < T.redLds * 2; i += 256) red[i] = src[i];
        for (int i = threadIdx.x; i < histBins; i += 256) sh.hist[i] = 0;
    }
    __syncthreads();
    auto fetch = [&](int i, Ray& r) {
        if (ANY)
        {
            const float4 qa = W.SQ.ld4(SQ_A, i), qb = W.SQ.ld4(SQ_B, i);
            r.o = mk3(qa.x, qa.y, qa.z); r.d = mk3(qa.w, qb.x, qb.y); r.inv = inv_dir(r.d);
            return true;
        }
        const float4 qa = W.R.ld4(RQ_A, i), qb = W.R.ld4(RQ_B, i);
        if (__float_as_int(qb.z) & RF_DEAD) return false;
        r.o = mk3(qa.x, qa.y, qa.z); r.d = mk3(qa.w, qb.x, qb.y); r.inv = inv_dir(r.d);
        return true;
    };
    auto done = [&](int i, const WalkResult& res) {
        if (ANY) { if (!res.occluded) W.SQ.sti(S_VIS, i, 1); }
        else W.R.st4(RQ_H, i, mkq(res.t, res.tObj, __int_as_float(res.slot), __int_as_float(res.prim)));
    };
    if (PHASE != 1)
    {
        RangeGrab G; G.init(PHASE == 0 ? W.grab + (depth * 2 + (ANY ? 0 : 1)) * 8 : Q.misc + 8, W.nRanges, -1);
        const int* cnt = (ANY ? W.cntS : W.cntA) + (size_t)depth * W.nRanges;
        walk_tl<FEAT, ANY, EXISTS, LT, PHASE>(tr, T, Q, sh, histBins, Treelet{},
            [&](int& base, int& n) { for (;;) { const int r = G.next(); if (r < 0) return false; n = cnt[r]; base = r * kRange; if (n > 0) return true; } },
            fetch, done, PHASE == 0 ? 0 : 7);
    }
    else
    {
        const int M = Q.misc[0];
        const int G = (int)gridDim.x;
        int span = (M + G - 1) / G;
        if (span < kTlSpanMin) span = kTlSpanMin;
        const long long p0 = (long long)blockIdx.x * span;
        const int p1 = (int)(p0 + span < (long long)M ? p0 + span : (long long)M);
        int p = p0 < M ? (int)p0 : M;
        while (p < p1)
        {
            int lo = 0, hi = T.nTl;                           // offs[lo] <= p < offs[hi]
            while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (Q.offs[mid] <= p) lo = mid; else hi = mid; }
            const Treelet tlc = T.tl[lo];
            const int segEnd = Q.offs[lo + 1] < p1 ? Q.offs[lo + 1] : p1;
            __syncthreads();                                   // every wave has left the treelet staged before
#ifdef HRT_TL_STATS
            const long long tStage0 = (long long)__builtin_readcyclecounter();
#endif
            {
                const int nN = 2 * (tlc.nodeHi - tlc.nodeLo), nT = 3 * (tlc.triHi - tlc.triLo);
                const float4* sn = reinterpret_cast<const float4*>(tr.P.blas + tlc.nodeLo);
                const float4* st = reinterpret_cast<const float4*>(tr.P.ftri + tlc.triLo);
                for (int i = threadIdx.x; i < nN; i += 256) sh.tl[i] = sn[i];
                for (int i = threadIdx.x; i < nT; i += 256) sh.tl[nN + i] = st[i];
                if (threadIdx.x == 0) sh.misc[0] = p;
            }
            __syncthreads();
#ifdef HRT_TL_STATS
            if ((threadIdx.x & 63) == 0) atomicAdd(&g_tl_stats[round < 6 ? round : 6][ANY ? 0 : 1][12], (unsigned long long)((long long)__builtin_readcyclecounter() - tStage0));
#endif
            walk_tl<FEAT, ANY, EXISTS, LT, 1>(tr, T, Q, sh, histBins, tlc,
                [&](int& base, int& n) {
                    int b = 0;
                    if ((threadIdx.x & 63) == 0) b = atomicAdd(&sh.misc[0], 64);
                    b = __builtin_amdgcn_readfirstlane(b);
                    if (b >= segEnd) return false;
                    base = b; n = segEnd - b < 64 ? segEnd - b : 64;
                    return true;
                },
                fetch, done, round < 6 ? round : 6);
            p = segEnd;
        }
    }
    __syncthreads();
    for (int b = threadIdx.x; b < histBins; b += 256) { const int v = sh.hist[b]; if (v) atomicAdd(&Q.hist[b], v); }
}

__global__ void __launch_bounds__(1024)
hrt_tl_scan_kernel(TlQueues Q, int nTl) { tl_scan_block(Q, nTl); }

__global__ void __launch_bounds__(256)
hrt_tl_scatter_kernel(TlQueues Q, int nTl, const int* cnt, int nRanges)
{
    tl_scatter_block(Q, nTl, cnt, nRanges, wf_range(nRanges));
}

template <int FEAT, bool COUNT>
__global__ void __launch_bounds__(256)
hrt_wf_finish_kernel(TracerPackedT<FEAT> tr, FrameK k, WfBuffers W, int vsel, int depth)
{
    int range = wf_range(W.nRanges);
    W = W.at_depth(depth);
    wf_finish_wave<FEAT, COUNT>(tr, k, W, vsel ? W.B : W.A, vsel ? W.A : W.B, depth, range);      // every wave: the four waves of a workgroup pack their survivors together
}

// finish of bounce `depth` + shade of bounce depth + 1 in one kernel (every bounce but the last): hrt_wavefront.hpp
template <int FEAT, bool COUNT>
__global__ void __launch_bounds__(256)
hrt_wf_finish_shade_kernel(TracerPackedT<FEAT> tr, FrameK k, WfGeom g, DGBuffer gb, DReservoir resPrev, long long nPix, WfBuffers W, int vsel, int depth, unsigned long long* counters)
{
    Cnt<COUNT> C;
    int range = wf_range(W.nRanges);
    W = W.at_depth(depth);
    wf_finish_shade_wave<FEAT, COUNT>(tr, k, g, gb, resPrev, nPix, W, vsel ? W.B : W.A, vsel ? W.A : W.B, depth, range, C);
    C.flush(counters);
}

__global__ void __launch_bounds__(256)
hrt_wf_resolve_kernel(FrameK k, WfGeom g, DGBuffer gb, DFramebuffer fb, DReservoir resCur, WfBuffers W)
{
    int ord = blockIdx.x * 256 + threadIdx.x;
    if (ord < g.nOrd) wf_resolve_pixel(k, g, gb, fb, resCur, W, ord);
}

// ---------------------------------------------------------------------------------------
// Progressive frames (hrt_render_progressive): the same pixel code with PROG set -- samples [sBegin, k.spp) of the frame, the
// raw sample sum carried in a per-pixel plane between calls.  Separate entry points, so the kernels of hrt_render_frame keep
// their code; production tracers only (no COUNT variants: counting frames cannot be progressive).
// ---------------------------------------------------------------------------------------
template <class TR, bool REUSE = true>
__global__ void __launch_bounds__(256, PtWaves<TR>::value)
hrt_path_trace_prog_kernel(TR tr, FrameK k, DGBuffer gb, DFramebuffer fb, DReservoir resPrev, DReservoir resCur,
                           long long nPix, TileMap tm, hrt_float3* carry, int sBegin)
{
    Cnt<false> C;
    ProgK pk; pk.carry = carry; pk.sBegin = sBegin;
    int x, y;
    if (tile_pixel(tm, k, x, y, blockIdx.x)) path_trace_pixel<TR, false, false, REUSE, true>(tr, k, gb, fb, resPrev, resCur, nPix, y * k.width + x, C, nullptr, &pk);
}

// groups of perGroup samples over [sBegin, k.spp): the split kernel's pixel code with the groups moved (the scratch planes are
// indexed by absolute sample, as in a one-shot frame of k.spp samples)
template <class TR, bool REUSE = true>
__global__ void __launch_bounds__(256, PtWaves<TR>::value)
hrt_path_trace_split_prog_kernel(TR tr, FrameK k, DGBuffer gb, DFramebuffer fb, DReservoir resPrev, DReservoir resCur,
                                 long long nPix, TileMap tm, hrt_float3* li, float* stage, int nGroups, int perGroup, int sBegin)
{
    Cnt<false> C;
    const int g = blockIdx.x / tm.nTiles;
    SplitK sk;
    sk.li = li; sk.stage = stage; sk.group = g; sk.nGroups = nGroups;
    sk.sBegin = sBegin + g * perGroup; sk.sEnd = min(sk.sBegin + perGroup, k.spp);
    const int tileBlock = blockIdx.x - g * tm.nTiles;
    sk.local = tileBlock * (int)blockDim.x + (int)threadIdx.x; sk.nLocal = tm.nTiles * (int)blockDim.x;
    int x, y;
    if (tile_pixel(tm, k, x, y, tileBlock)) path_trace_pixel<TR, false, true, REUSE>(tr, k, gb, fb, resPrev, resCur, nPix, y * k.width + x, C, &sk);
}

__global__ void __launch_bounds__(256)
hrt_split_resolve_prog_kernel(FrameK k, DGBuffer gb, DFramebuffer fb, DReservoir resCur, long long nPix, TileMap tm, const hrt_float3* li, const float* stage,
                              int nGroups, hrt_float3* carry, int sBegin)
{
    int x, y;
    if (tile_pixel(tm, k, x, y, blockIdx.x)) split_resolve_pixel<true>(k, gb, fb, resCur, y * k.width + x, li, stage, nGroups,
                                                                       (int)(blockIdx.x * blockDim.x + threadIdx.x), tm.nTiles * (int)blockDim.x, carry, sBegin);
}

__global__ void __launch_bounds__(256)
hrt_wf_resolve_prog_kernel(FrameK k, WfGeom g, DGBuffer gb, DFramebuffer fb, DReservoir resCur, WfBuffers W, hrt_float3* carry)
{
    int ord = blockIdx.x * 256 + threadIdx.x;
    if (ord < g.nOrd) wf_resolve_pixel<true>(k, g, gb, fb, resCur, W, ord, carry);
}


// ---------------------------------------------------------------------------------------
// Presentation kernels (hrt_post.hpp)
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
hrt_taa_resolve_kernel(TaaK p)
{
    __shared__ float lut[256];                       // sRGB byte -> linear, same expression as UnpackSRGB
    lut[threadIdx.x] = srgb_to_linear_byte((int)threadIdx.x);
    __syncthreads();
    const int total = p.outW * p.outH;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) taa_resolve_pixel<false>(lut, p, nullptr, idx);
}

// HRT_PRESENT_TAAU_REPROJECT: the REPROJECT instantiation of the same resolve; reads the history pair in r, writes the pair in p
__global__ void __launch_bounds__(256)
hrt_taa_resolve_reproject_kernel(TaaK p, TaaReprojK r)
{
    __shared__ float lut[256];
    lut[threadIdx.x] = srgb_to_linear_byte((int)threadIdx.x);
    __syncthreads();
    const int total = p.outW * p.outH;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) taa_resolve_pixel<true>(lut, p, &r, idx);
}

// hrt_motion_vectors: one lane per pixel of the nRows rows a device slot owns (8-row strips s of [rowBegin, rowEnd) with
// s % stripN == stripI, in order); mv is indexed by the global pixel index like every per-pixel array
__global__ void __launch_bounds__(256)
hrt_motion_vectors_kernel(const hrt_float3* worldPos, ProjCam from, ProjCam cur, int width, int height,
                          int rowBegin, int rowEnd, int stripN, int stripI, int nRows, hrt_float2* mv)
{
    long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= (long long)nRows * width) return;
    int lr = (int)(j / width), x = (int)(j % width);
    int row = rowBegin + ((lr >> 3) * stripN + stripI) * 8 + (lr & 7);
    if (row < rowEnd) motion_vector_pixel(worldPos, from, cur, width, height, mv, row * width + x);
}

__global__ void __launch_bounds__(256)
hrt_blit_kernel(const int32_t* src, long long srcLen, int32_t* dst, long long dstLen)     // RTRenderer.cs:281-285
{
    long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= dstLen || i >= srcLen) return;
    dst[i] = src[i];
}

__global__ void __launch_bounds__(256)
hrt_bilinear_upsample_kernel(const int32_t* src, int srcW, int srcH, int32_t* dst, int dstW, int dstH)
{
    int i = blockIdx.x * 256 + threadIdx.x;
    if (i < dstW * dstH) bilinear_upsample_pixel(src, srcW, srcH, dst, dstW, dstH, i);
}

#ifdef HRT_TEST_HOOKS
// exactness probe: evaluates include/hrt_math.h on the device (tests compare with the oracle's bits)
__global__ void hrt_math_probe_kernel(int fn, int n, const float* x, const float* y, float* out)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float a = x[i], b = y ? y[i] : 0.f, r = 0.f;
    switch (fn) {
    case 0: r = hrt_sin(a); break;   case 1: r = hrt_cos(a); break;   case 2: r = hrt_tan(a); break;
    case 3: r = hrt_atan(a); break;  case 4: r = hrt_atan2(a, b); break; case 5: r = hrt_acos(a); break;
    case 6: r = hrt_asin(a); break;  case 7: r = hrt_rsqrt(a); break; case 8: r = hrt_sqrt(a); break;
    case 9: r = hrt_fmin(a, b); break; case 10: r = hrt_fmax(a, b); break;
    case 11: r = hrt_floor(a); break; case 12: r = hrt_round(a); break;
    case 13: { int v = hrt_f2i(a); r = __int_as_float(v); } break;
    case 14: r = 1.0f / a; break;    case 15: r = a / b; break;
    case 16: r = a * b + a; break;   // must NOT be contracted
    case 17: r = hrt_log(a); break;  case 18: r = hrt_exp(a); break;  case 19: r = hrt_pow(a, b); break;
    case 20: { float s, c; hrt_sincos(a, &s, &c); r = s; } break;
    case 21: { float s, c; hrt_sincos(a, &s, &c); r = c; } break;
    case 22: r = sqrt_normal_range(a); break;
    case 23: r = rsqrt_clamped(a); break;
    case 24: { float s, c; hrt_sincos_nonneg(a, &s, &c); r = s; } break;
    case 25: { float s, c; hrt_sincos_nonneg(a, &s, &c); r = c; } break;
    case 26: r = sqrt_normal_range<true>(a); break;
    case 27: r = rsqrt_clamped<true>(a); break;
    case 28: r = rcp_normal_range(a); break;
    case 29: r = div_by(a, recip_of(b)); break;
    case 30: r = inv_dir(mk3(a, b, 0.5f)).x; break;             // guarded: a wave with a out of rcp_domain takes 1.0f / a
    case 31: {                                                  // TracerFlat's sphere step: Recip or IEEE divide by a ballot on 2a
        Ray ray; ray.o = mk3(0.f, 0.f, 0.f); ray.d = mk3(0.f, 0.f, b); ray.inv = ray.d;
        const float sa = dot(ray.d, ray.d);
        const F3 c = mk3(0.25f, 0.f, a);
        float t = -1.f;
        const bool h = __builtin_amdgcn_ballot_w64(!recip_domain(2.f * sa)) == 0 ? hit_sphere_q(ray, sa, recip_of(2.f * sa), c, 1.f, t)
                                                                                  : hit_sphere_q(ray, sa, 2.f * sa, c, 1.f, t);
        r = h ? t : -1.f;
    } break;
    }
    out[i] = r;
}

// exhaustive device-side comparison of a trimmed function with its IEEE definition over every float of its domain:
// which 0: rsqrt_clamped(x) vs hrt_rsqrt(x) for x in [1e-20, +inf]; 1: sqrt_normal_range(x) vs hrt_sqrt(x) for x = +0, x in [2^-96, +inf];
// 2: rcp_normal_range(x) vs 1.0f / x for every x in rcp_domain (both signs);
// 3: div_by(n, recip_of(d)) vs n / d for EVERY float n and 1028 denominators d in [1, 4): each 2^14-th float from 1.0 and the
//    neighbours of 1, 2 and 4;  4: the same for 2^34 hashed pairs (n any float, d any float in [1, 4)).
// For 3 and 4 a pair counts as a mismatch unless the bits agree (|n| >= 2^-100, finite), |div_by| < 2^-98 (|n| < 2^-100) or
// div_by is NaN (n infinite or NaN): the contract of div_by (hrt_device.hpp).
HRT_D bool div_by_ok(float n, float d)
{
    const float a = div_by(n, recip_of(d)), b = n / d;
    if (!hrt_isfinite(n)) return a != a;
    if (__builtin_fabsf(n) < 0x1p-100f) return __builtin_fabsf(a) < 0x1p-98f;
    return __float_as_uint(a) == __float_as_uint(b);
}
HRT_D float dense_denominator(int j)
{
    const unsigned edges[4] = {0x3F800001u, 0x3FFFFFFFu, 0x40000001u, 0x407FFFFFu};
    return __uint_as_float(j < 1024 ? 0x3F800000u + (unsigned)j * 0x4000u : edges[j - 1024]);
}
__global__ void hrt_math_exhaustive_kernel(int which, unsigned long long* mismatches, unsigned* firstBad)
{
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x, first = blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x;
    unsigned long long bad = 0;
    if (which <= 2)
    {
        const unsigned lo = which == 0 ? __float_as_uint(1e-20f) : which == 1 ? __float_as_uint(0x1p-96f) : __float_as_uint(0x1p-94f);
        const unsigned hi = which == 2 ? __float_as_uint(0x1p125f) : 0x7F800000u;            // inclusive
        const int signs = which == 2 ? 2 : 1;
        for (int sgn = 0; sgn < signs; sgn++)
            for (unsigned long long u = (unsigned long long)lo + first; u <= hi; u += stride)
            {
                const unsigned bits = (unsigned)u | (sgn ? 0x80000000u : 0u);
                const float x = __uint_as_float(bits);
                const float a = which == 0 ? rsqrt_clamped(x) : which == 1 ? sqrt_normal_range(x) : rcp_normal_range(x);
                const float b = which == 0 ? hrt_rsqrt(x) : which == 1 ? hrt_sqrt(x) : 1.0f / x;
                if (__float_as_uint(a) != __float_as_uint(b)) { bad++; atomicMin(firstBad, bits); }
            }
    }
    else if (which == 3)
    {
        for (unsigned long long u = first; u <= 0xFFFFFFFFull; u += stride)
            for (int j = 0; j < 1028; j++)
                if (!div_by_ok(__uint_as_float((unsigned)u), dense_denominator(j))) { bad++; atomicMin(firstBad, (unsigned)u); }
    }
    else
    {
        for (unsigned long long i = first; i < (1ull << 34); i += stride)
        {
            const unsigned hn = hash32((unsigned)i ^ hash32((unsigned)(i >> 32) + 0x9E3779B9u)), hd = hash32(hn ^ 0x85EBCA6Bu);
            const float d = __uint_as_float(0x3F800000u + hd % 0x01000000u);                  // [1, 4): 2^24 floats
            if (!div_by_ok(__uint_as_float(hn), d)) { bad++; atomicMin(firstBad, hn); }
        }
    }
    if (which == 1 && blockIdx.x == 0 && threadIdx.x == 0 && __float_as_uint(sqrt_normal_range(0.f)) != 0u) bad++;
    if (bad) atomicAdd(mismatches, bad);
}

#endif // HRT_TEST_HOOKS

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
namespace {

thread_local std::string g_create_error;       // the error text of calls without a context, per calling thread

} // namespace

namespace hrt { namespace detail {

int fail(hrt_ctx* c, int code, const std::string& msg)
{
    if (c) c->err = msg; else g_create_error = msg;
    return code;
}

// no exception crosses the C ABI: std::bad_alloc of the host-side vectors / strings -> HRT_ERR_OUT_OF_MEMORY, anything else -> HRT_ERR_HIP
int on_exception(hrt_ctx* c, const char* who) noexcept
{
    try
    {
        try { throw; }
        catch (const std::bad_alloc&) { return fail(c, HRT_ERR_OUT_OF_MEMORY, std::string(who) + ": out of host memory"); }
        catch (const std::exception& e) { return fail(c, HRT_ERR_HIP, std::string(who) + ": " + e.what()); }
        catch (...) { return fail(c, HRT_ERR_HIP, std::string(who) + ": unknown exception"); }
    }
    catch (...) { return HRT_ERR_OUT_OF_MEMORY; }      // not even the message could be stored
}

int Scratch::grow(hrt_ctx* c, size_t need, hipStream_t st, Drain drain, bool pinned)
{
    if (need <= bytes) return HRT_OK;
    if (p) { HIPCHK(c, drain == kDevice ? hipDeviceSynchronize() : hipStreamSynchronize(st)); release(pinned); }
    HIPCHK(c, pinned ? hipHostMalloc(&p, need, hipHostMallocPortable) : hipMalloc(&p, need));
    bytes = need;
    return HRT_OK;
}

void Scratch::release(bool pinned)
{
    if (p) (void)(pinned ? hipHostFree(p) : hipFree(p));
    p = nullptr; bytes = 0;
}

int for_each_slot(hrt_ctx* c, bool threads, const char* who, const char* what, const std::function<int(int, hrt_ctx*)>& fn)
{
    const int nd = (int)c->dev.size();
    if (!threads)
    {
        for (int i = 0; i < nd; i++) { int rc = fn(i, c); if (rc != HRT_OK) return rc; }
        return HRT_OK;
    }
    std::vector<int> rcs((size_t)nd, HRT_OK);
    std::vector<std::string> errs((size_t)nd);
    std::vector<std::thread> workers;
    for (int i = 0; i < nd; i++)
        workers.emplace_back([&, i]() {
            try { rcs[(size_t)i] = fn(i, nullptr); if (rcs[(size_t)i] != HRT_OK) errs[(size_t)i] = g_create_error; }
            catch (...) { rcs[(size_t)i] = HRT_ERR_OUT_OF_MEMORY; }
        });
    for (std::thread& t : workers) t.join();
    for (int i = 0; i < nd; i++)
        if (rcs[(size_t)i] != HRT_OK) return fail(c, rcs[(size_t)i], std::string(who) + ": " + what + "device slot " + std::to_string(i) + ": " + errs[(size_t)i]);
    return HRT_OK;
}

}} // namespace hrt::detail

namespace {

void free_pixels(DeviceState& d)
{
    void* ptrs[] = {d.gb.worldPos, d.gb.normalWS, d.gb.baseColor, d.gb.matId, d.gb.objId, d.gb.hitMask,
                    d.fb.color, d.fb.depth, d.fb.objectId, d.fb.cameraId, d.fb.radiance,
                    d.resA.L, d.resA.wi, d.resA.pdf, d.resA.w, d.resA.wSum, d.resA.m, d.resA.lightId,
                    d.resB.L, d.resB.wi, d.resB.pdf, d.resB.w, d.resB.wSum, d.resB.m, d.resB.lightId};
    for (void* p : ptrs) if (p) (void)hipFree(p);
    if (d.prog_carry) (void)hipFree(d.prog_carry);
    d.prog_carry = nullptr;
    d.gb = DGBuffer{}; d.fb = DFramebuffer{}; d.resA = DReservoir{}; d.resB = DReservoir{};
    d.nPix = 0;
}

// zero-fill is ordered on the device's own (non-blocking) stream: the null stream does not
// synchronise with it, so a hipMemset there could land after the first kernel's stores
template <class T> hipError_t dalloc(T*& p, int64_t n, hipStream_t stream)
{
    void* v = nullptr;
    hipError_t e = hipMalloc(&v, (size_t)n * sizeof(T));
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(v, 0, (size_t)n * sizeof(T), stream);
    if (e != hipSuccess) return e;
    p = static_cast<T*>(v);
    return hipSuccess;
}

hipError_t alloc_res(DReservoir& r, int64_t n, hipStream_t st)
{
    hipError_t e;
    if ((e = dalloc(r.L, n, st)) != hipSuccess) return e;
    if ((e = dalloc(r.wi, n, st)) != hipSuccess) return e;
    if ((e = dalloc(r.pdf, n, st)) != hipSuccess) return e;
    if ((e = dalloc(r.w, n, st)) != hipSuccess) return e;
    if ((e = dalloc(r.wSum, n, st)) != hipSuccess) return e;
    if ((e = dalloc(r.m, n, st)) != hipSuccess) return e;
    return dalloc(r.lightId, n, st);
}

// GBuffer.EnsureLength / Framebuffer.EnsureLength / EnsureLowResBuffers: realloc on size change only
int ensure_pixels(hrt_ctx* c, DeviceState& d, int64_t nPix)
{
    if (d.nPix == nPix) return HRT_OK;
    HIPCHK(c, hipSetDevice(d.device_id));
    free_pixels(d);
    HIPCHK(c, dalloc(d.gb.worldPos, nPix, d.stream));
    HIPCHK(c, dalloc(d.gb.normalWS, nPix, d.stream));
    HIPCHK(c, dalloc(d.gb.baseColor, nPix, d.stream));
    HIPCHK(c, dalloc(d.gb.matId, nPix, d.stream));
    HIPCHK(c, dalloc(d.gb.objId, nPix, d.stream));
    HIPCHK(c, dalloc(d.gb.hitMask, nPix, d.stream));
    HIPCHK(c, dalloc(d.fb.color, nPix, d.stream));
    HIPCHK(c, dalloc(d.fb.depth, nPix, d.stream));
    HIPCHK(c, dalloc(d.fb.objectId, nPix, d.stream));
    HIPCHK(c, dalloc(d.fb.cameraId, 1, d.stream));
    HIPCHK(c, dalloc(d.fb.radiance, nPix, d.stream));
    HIPCHK(c, alloc_res(d.resA, nPix, d.stream));
    HIPCHK(c, alloc_res(d.resB, nPix, d.stream));
    d.nPix = nPix;
    return HRT_OK;
}

void free_present(DeviceState& d)
{
    if (d.present_color) (void)hipFree(d.present_color);
    if (d.taa_hist_color) (void)hipFree(d.taa_hist_color);
    if (d.taa_hist_obj) (void)hipFree(d.taa_hist_obj);
    if (d.taa_spare_color) (void)hipFree(d.taa_spare_color);
    if (d.taa_spare_obj) (void)hipFree(d.taa_spare_obj);
    d.present_color = d.taa_hist_color = d.taa_hist_obj = d.taa_spare_color = d.taa_spare_obj = nullptr;
    d.present_w = d.present_h = 0; d.taa_history_valid = false;
}

void free_workspace(DeviceState& d)
{
    for (int j = 0; j < kMaxLanes; j++) for (Scratch* s : {&d.tlq_mem[j], &d.wf_mem[j], &d.wf_cnt[j]}) s->release();
    d.wf_accum.release();
    d.split_mem.release();
}

// copies the strips `owner` renders (rows [row_begin,row_end), strips s % strip_n == strip_i) of one per-pixel array
// from src to dst (same global indexing on both sides) on `stream`: device -> host gather, or device -> device exchange
template <class T>
int copy_strips(hrt_ctx* c, const DeviceState& owner, T* dst, const T* src, int width, hipMemcpyKind kind, hipStream_t stream)
{
    if (!dst || owner.n_strips == 0) return HRT_OK;
    const size_t rowElems = (size_t)width;
    if (owner.strip_n == 1)
    {   // one contiguous row block
        size_t off = (size_t)owner.row_begin * rowElems;
        size_t cnt = (size_t)(owner.row_end - owner.row_begin) * rowElems;
        HIPCHK(c, hipMemcpyAsync(dst + off, src + off, cnt * sizeof(T), kind, stream));
        return HRT_OK;
    }
    // interleaved 8-row strips: one strided 2-D copy for the full strips, one plain copy for a ragged last strip
    int lastStrip = owner.strip_i + (owner.n_strips - 1) * owner.strip_n;
    int lastRows = std::min(8, (owner.row_end - owner.row_begin) - lastStrip * 8);
    int fullStrips = lastRows == 8 ? owner.n_strips : owner.n_strips - 1;
    size_t first = ((size_t)owner.row_begin + (size_t)owner.strip_i * 8) * rowElems;
    if (fullStrips > 0)
        HIPCHK(c, hipMemcpy2DAsync(dst + first, (size_t)8 * rowElems * owner.strip_n * sizeof(T), src + first, (size_t)8 * rowElems * owner.strip_n * sizeof(T),
                                   (size_t)8 * rowElems * sizeof(T), (size_t)fullStrips, kind, stream));
    if (lastRows < 8 && lastRows > 0)
    {
        size_t off = ((size_t)owner.row_begin + (size_t)lastStrip * 8) * rowElems;
        HIPCHK(c, hipMemcpyAsync(dst + off, src + off, (size_t)lastRows * rowElems * sizeof(T), kind, stream));
    }
    return HRT_OK;
}
template <class T>
int gather_rows(hrt_ctx* c, DeviceState& d, T* host, const T* devp, int width)
{
    return copy_strips(c, d, host, devp, width, hipMemcpyDeviceToHost, d.stream);
}

// ---------------------------------------------------------------------------------------
// The path-trace launch of one device, either as the one-pixel-per-lane megakernel or as the
// streamed pipeline of hrt_wavefront.hpp (default).
// ---------------------------------------------------------------------------------------
constexpr long long kWfMaxPaths = 1ll << 25;      // paths resident per sample batch (320 B of workspace each)

// workspace of batch lane `lane` (0 / 1); growing one drains the device first (frames of earlier calls may still use it)
int ensure_workspace(hrt_ctx* c, DeviceState& d, int lane, long long cap, int nOrd, int nRanges, int maxDepth, WfBuffers& W, bool treelets = false)
{
    const size_t planes = 2 * V_PLANES + R_PLANES + S_PLANES + 3 + G_PLANES;
    const size_t bytes = (size_t)planes * (size_t)cap * sizeof(float);
    const size_t ints = (size_t)(2 * maxDepth + 2) * (size_t)nRanges + (size_t)maxDepth * 16;
    int rc;
    if ((rc = d.wf_mem[lane].grow(c, bytes, d.stream, Scratch::kDevice)) != HRT_OK) return rc;
    if ((rc = d.wf_cnt[lane].grow(c, ints * sizeof(int), d.stream, Scratch::kDevice)) != HRT_OK) return rc;
    if ((rc = d.wf_accum.grow(c, (size_t)3 * (size_t)nOrd * sizeof(float), d.stream, Scratch::kDevice)) != HRT_OK) return rc;
    if (d.tl_ok && treelets)
    {   // queues of the treelet walker (only for frames that ask for it: HRT_FLAG_TREELETS): per walk kind key / state / binned indices over the path slots, and the per-treelet counters
        const size_t nTl = (size_t)d.dtl.nTl;
        const size_t ints = ((nTl + 32 + nTl + 1 + nTl) + 63) & ~(size_t)63;
        const size_t per0 = (size_t)cap * (4 + 16 + 4) + ints * 4, per1 = (size_t)cap * (4 + 32 + 4) + ints * 4;
        const size_t need = ((per0 + 255) & ~(size_t)255) + per1;
        if ((rc = d.tlq_mem[lane].grow(c, need, d.stream, Scratch::kDevice)) != HRT_OK) return rc;
    }
    float* m = (float*)d.wf_mem[lane].p;
    int* cnt = (int*)d.wf_cnt[lane].p;
    auto take = [&](int nplanes, long long stride) { Planes pl; pl.base = m; pl.stride = stride; m += (size_t)nplanes * (size_t)stride; return pl; };
    W.A = take(V_PLANES, cap); W.B = take(V_PLANES, cap); W.R = take(R_PLANES, cap); W.SQ = take(S_PLANES, cap);
    static_assert(V_POS == 0 && V_LI >= R_PLANES && V_PID >= R_PLANES && R_PLANES >= S_PLANES, "the second request set aliases the vertex planes below V_LI");
    W.Rn = W.A; W.SQn = W.B; W.pingpong = 0;
    W.sampleLi = take(3, cap); W.stage = take(G_PLANES, cap);
    W.accum.base = (float*)d.wf_accum.p; W.accum.stride = nOrd;
    W.cntA = cnt; W.cntS = cnt + (size_t)(maxDepth + 1) * (size_t)nRanges;
    W.grab = cnt + (size_t)(2 * maxDepth + 2) * (size_t)nRanges;
    W.nRanges = nRanges;
    return HRT_OK;
}


// queues of the treelet walker for one batch lane and walk kind (0 shadow, 1 closest), carved from DeviceState::tlq_mem
TlQueues tl_queues(const DeviceState& d, int lane, int kind, long long cap)
{
    const size_t nTl = (size_t)d.dtl.nTl;
    const size_t ints = ((nTl + 32 + nTl + 1 + nTl) + 63) & ~(size_t)63;
    const size_t per0 = (size_t)cap * (4 + 16 + 4) + ints * 4;
    char* p = (char*)d.tlq_mem[lane].p + (kind ? ((per0 + 255) & ~(size_t)255) : 0);
    TlQueues Q;
    Q.state = (float4*)p; p += (size_t)cap * (kind ? 32 : 16);
    Q.key = (int*)p; p += (size_t)cap * 4;
    Q.sorted = (int*)p; p += (size_t)cap * 4;
    Q.hist = (int*)p; Q.misc = Q.hist + nTl; Q.offs = Q.misc + 32; Q.curs = Q.offs + nTl + 1;
    return Q;
}

#ifndef HRT_TL_ROUNDS
#define HRT_TL_ROUNDS 3
#endif
// One walk launch of the streamed pipeline through the treelet walker: fresh rays, HRT_TL_ROUNDS rounds over the binned rays, clean-up.
template <int F, bool ANY, bool EXISTS, int LT>
int launch_tl_walk(hrt_ctx* c, DeviceState& d, const TracerPackedT<F>& tr, const WfBuffers& W, int lane, long long cap, int depth, hipStream_t st, dim3 gridW, dim3 gridR)
{
    const DTreelets& T = d.dtl;
    const TlQueues Q = tl_queues(d, lane, ANY ? 0 : 1, cap);
    const int histBins = T.nTl <= kTlHistLds ? T.nTl : 0;
    const size_t lds0 = tl_shared_bytes(0, T.redLds, histBins), lds1 = tl_shared_bytes(T.tlBytesMax, T.redLds, histBins);
    if (lds1 > 65536) HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&hrt_tl_walk_kernel<F, ANY, EXISTS, LT, 1>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds1));
    const dim3 block(256), grid1((unsigned)(d.n_cu * 8));
    HIPCHK(c, hipMemsetAsync(Q.hist, 0, ((size_t)T.nTl + 32) * sizeof(int), st));
    const int* cnt = (ANY ? W.cntS : W.cntA) + (size_t)depth * W.nRanges;
    hipLaunchKernelGGL((hrt_tl_walk_kernel<F, ANY, EXISTS, LT, 0>), gridW, block, lds0, st, tr, T, Q, W, depth, histBins, 0, 0);
    for (int r = 0; r < HRT_TL_ROUNDS; r++)
    {
        hipLaunchKernelGGL(hrt_tl_scan_kernel, dim3(1), dim3(1024), 0, st, Q, T.nTl);
        hipLaunchKernelGGL(hrt_tl_scatter_kernel, gridR, block, 0, st, Q, T.nTl, cnt, W.nRanges);
        hipLaunchKernelGGL((hrt_tl_walk_kernel<F, ANY, EXISTS, LT, 1>), grid1, block, lds1, st, tr, T, Q, W, depth, histBins, T.tlBytesMax, r + 1);
    }
    hipLaunchKernelGGL((hrt_tl_walk_kernel<F, ANY, EXISTS, LT, 2>), gridW, block, lds0, st, tr, T, Q, W, depth, histBins, 0, 0);
    HIPCHK(c, hipGetLastError());
    return HRT_OK;
}

// Sample groups of the fused path stage: when a launch of `waves` waves gives the machine less than ~5 rounds of them, the sppCall
// samples it renders are spread over nGroups workgroups per tile, perGroup samples each; the per-sample radiance of all sppAll samples
// of the frame and the groups' staged reservoirs then go through scratchFloats floats per lane of the launch.  One group: no scratch.
// A frame (run_path_stage) and a radiance query (paths_slot) both ask here, which is what keeps them bit-equal on camera rays.
struct SampleGroups { int nGroups, perGroup; size_t scratchFloats; };
SampleGroups sample_groups(int sppCall, int sppAll, int maxDepth, long long waves, int n_cu)
{
    const long long slots = (long long)n_cu * 4 * HRT_PT_WAVES;
    SampleGroups g{1, sppCall, 0};
    if (maxDepth <= 64 && sppCall > 1 && waves < 5 * slots)
        g.nGroups = (int)std::min<long long>(std::min(sppCall, 8), (16 * slots + waves - 1) / waves);   // config 2 over N = 2 / 4 / 8 ranks: 4 groups each (1.111 -> 1.079, 0.593 -> 0.555, 0.296 ms)
    if (g.nGroups > 1)
    {
        g.perGroup = (sppCall + g.nGroups - 1) / g.nGroups;
        g.nGroups = (sppCall + g.perGroup - 1) / g.perGroup;
        g.scratchFloats = (size_t)sppAll * 3 + (size_t)g.nGroups * 12;
    }
    return g;
}

template <class TR> struct PackedFeat { static constexpr int value = -1; };
template <int F> struct PackedFeat<TracerPackedT<F>> { static constexpr int value = F; };

template <class TR>
// carry != nullptr: a progressive call (hrt_render_progressive) renders samples [sBegin, k.spp) and carries the raw sample sum in
// carry (per global pixel index) -- the organisation is chosen as for a frame of the k.spp - sBegin samples this call renders
int run_path_stage(hrt_ctx* c, DeviceState& d, const TR& tr, const FrameK& k, const TileMap& tm, int width,
                   const DReservoir& resPrev, const DReservoir& resCur, long long nPix, bool count, bool mega, bool treelets = false,
                   hrt_float3* carry = nullptr, int sBegin = 0)
{
    unsigned long long* cnt1 = d.counters + 10;
    if (tm.nTiles <= 0) return HRT_OK;
    const bool prog = carry != nullptr;
    if (!prog) sBegin = 0;
    if (mega || k.maxDepth > 64)
    {
        const dim3 grid(tm.nTiles), block(64 * tm.wpb);
        // frames without ReSTIR reuse: the leaf-sweep tracer's kernels with the import code compiled out (hrt_device.hpp, REUSE)
        const bool noReuse = std::is_same<TR, TracerFlat>::value && !count && k.enableTemporal == 0 && k.enableSpatial == 0;
        // sample groups when the tile gives the machine less than ~5 rounds of waves
        const int sppAll = k.spp > 1 ? k.spp : 1;
        const int sppN = sppAll - sBegin;                            // samples of this call
        const long long waves = (long long)tm.nTiles * tm.wpb;
        const SampleGroups sg = !count && waves > 0 ? sample_groups(sppN, sppAll, k.maxDepth, waves, d.n_cu) : SampleGroups{1, sppN, 0};
        const int nGroups = sg.nGroups, perGroup = sg.perGroup;
        if (nGroups > 1)
        {
            // scratch planes over the lanes of THIS launch's tiles (a rank's share of the frame), not over the image
            const size_t nLocal = (size_t)tm.nTiles * 64 * (size_t)tm.wpb;
            int rc = d.split_mem.grow(c, sg.scratchFloats * nLocal * sizeof(float), d.stream);
            if (rc != HRT_OK) return rc;
            hrt_float3* li = (hrt_float3*)d.split_mem.p;
            float* stage = (float*)d.split_mem.p + (size_t)sppAll * 3 * nLocal;
            if (prog)
            {
                if (noReuse) { if constexpr (std::is_same<TR, TracerFlat>::value) hipLaunchKernelGGL((hrt_path_trace_split_prog_kernel<TR, false>), dim3(tm.nTiles * nGroups), block, 0, d.stream, tr, k, d.gb, d.fb, resPrev, resCur, nPix, tm, li, stage, nGroups, perGroup, sBegin); }
                else hipLaunchKernelGGL((hrt_path_trace_split_prog_kernel<TR>), dim3(tm.nTiles * nGroups), block, 0, d.stream, tr, k, d.gb, d.fb, resPrev, resCur, nPix, tm, li, stage, nGroups, perGroup, sBegin);
                hipLaunchKernelGGL(hrt_split_resolve_prog_kernel, grid, block, 0, d.stream, k, d.gb, d.fb, resCur, nPix, tm, (const hrt_float3*)li, (const float*)stage, nGroups, carry, sBegin);
                HIPCHK(c, hipGetLastError());
                return HRT_OK;
            }
            if (noReuse) { if constexpr (std::is_same<TR, TracerFlat>::value) hipLaunchKernelGGL((hrt_path_trace_split_kernel<TR, false>), dim3(tm.nTiles * nGroups), block, 0, d.stream, tr, k, d.gb, d.fb, resPrev, resCur, nPix, tm, li, stage, nGroups, perGroup); }
            else hipLaunchKernelGGL((hrt_path_trace_split_kernel<TR>), dim3(tm.nTiles * nGroups), block, 0, d.stream, tr, k, d.gb, d.fb, resPrev, resCur, nPix, tm, li, stage, nGroups, perGroup);
            hipLaunchKernelGGL(hrt_split_resolve_kernel, grid, block, 0, d.stream, k, d.gb, d.fb, resCur, nPix, tm, (const hrt_float3*)li, (const float*)stage, nGroups);
            HIPCHK(c, hipGetLastError());
            return HRT_OK;
        }
        if (prog)
        {
            if (noReuse) { if constexpr (std::is_same<TR, TracerFlat>::value) hipLaunchKernelGGL((hrt_path_trace_prog_kernel<TR, false>), grid, block, 0, d.stream, tr, k, d.gb, d.fb, resPrev, resCur, nPix, tm, carry, sBegin); }
            else hipLaunchKernelGGL((hrt_path_trace_prog_kernel<TR>), grid, block, 0, d.stream, tr, k, d.gb, d.fb, resPrev, resCur, nPix, tm, carry, sBegin);
            HIPCHK(c, hipGetLastError());
            return HRT_OK;
        }
        if (count) hipLaunchKernelGGL((hrt_path_trace_kernel<TR, true>), grid, block, 0, d.stream, tr, k, d.gb, d.fb, resPrev, resCur, nPix, tm, cnt1);
        else if (noReuse) { if constexpr (std::is_same<TR, TracerFlat>::value) hipLaunchKernelGGL((hrt_path_trace_kernel<TR, false, false>), grid, block, 0, d.stream, tr, k, d.gb, d.fb, resPrev, resCur, nPix, tm, cnt1); }
        else       hipLaunchKernelGGL((hrt_path_trace_kernel<TR, false>), grid, block, 0, d.stream, tr, k, d.gb, d.fb, resPrev, resCur, nPix, tm, cnt1);
        HIPCHK(c, hipGetLastError());
        return HRT_OK;
    }
    WfGeom g;
    g.tilesX8 = (width + 7) / 8;
    g.nOrd = g.tilesX8 * d.n_strips * 64;
    const int spp = k.spp > 1 ? k.spp : 1;
    const int nS = spp - sBegin;                 // samples of this call: [sBegin, spp)
    long long maxPaths = kWfMaxPaths;
    if (c->max_resident_paths > 0) maxPaths = c->max_resident_paths;              // hrt_set_workspace_limit
    long long sb = maxPaths / g.nOrd;
    if (sb < 1) sb = 1;
    if (sb > nS) sb = nS;
    // Two sample batches in flight: the walks of one are latency-bound and leave the vector units idle most of the time, the
    // shade / finish / resolve kernels of the other fill them (measured first as two processes sharing the card: configs 4 / 5
    // -11 % / -7 %).  A frame that fits one batch is cut into two halves; only the ordered steps -- the per-pixel sample sum
    // and the last-writer reservoir in wf_resolve -- are chained by events, in batch order.
    // ... a frame that fits one batch is cut in two only while each half still fills the machine (measured: halves of 16.6 M paths
    // config 3 -5.5 %, config 4 +-0; halves of 8.3 M paths config 5 +13 %)
    constexpr long long kMinHalfBatchPaths = 12000000;
    const bool severalBatches = sb < nS;
    const bool halves = !severalBatches && nS >= 2 && (long long)((nS + 1) / 2) * g.nOrd >= kMinHalfBatchPaths;
    const int nBatchesNatural = (int)((nS + sb - 1) / sb);
    const int nLanes = severalBatches ? std::min(kBatchLanes, nBatchesNatural) : (halves ? std::min(kBatchLanes, 2) : 1);
    if (nLanes >= 2 && !severalBatches && sb > (nS + 1) / 2) sb = (nS + 1) / 2;
    const long long batchPaths = sb * (long long)g.nOrd;
    const int nRanges = (int)((batchPaths + kRange - 1) / kRange);
    const long long cap = (long long)nRanges * kRange;
    WfBuffers Wl[kMaxLanes];
    for (int j = 0; j < nLanes; j++) { int rc = ensure_workspace(c, d, j, cap, g.nOrd, nRanges, k.maxDepth, Wl[j], treelets); if (rc != HRT_OK) return rc; }
    hipStream_t laneMain[kMaxLanes], laneSide[kMaxLanes];
    laneMain[0] = d.stream; laneSide[0] = d.stream2;
    for (int j = 1; j < kMaxLanes; j++) { laneMain[j] = d.laneStream[j][0]; laneSide[j] = d.laneStream[j][1]; }
    if (nLanes >= 2)
    {   // the other lanes start behind everything enqueued so far (this frame's primary launch, the previous frame)
        HIPCHK(c, hipEventRecord(d.evStage, d.stream));
        for (int j = 1; j < nLanes; j++) HIPCHK(c, hipStreamWaitEvent(laneMain[j], d.evStage, 0));
    }
    const dim3 block(256), gridR((nRanges + 3) / 4), gridP((g.nOrd + 255) / 256);
    // walk launches are persistent: enough workgroups to fill every wave slot, each wave pulls ranges until none is left
    const dim3 gridW((unsigned)std::min<long long>((nRanges + 3) / 4, (long long)d.n_cu * (nLanes >= 2 ? kWalkBlocksPerCU2 : kWalkBlocksPerCU)));
    // finish of a bounce and shade of the next one as ONE kernel (the vertex never round-trips through its 22 planes): sphere-instance scenes
    // (config 3: path stage -3.6 %, HBM traffic 13.6 -> 11.7 GB per frame).  Triangle scenes keep the two kernels: their walks leave the vector
    // units to the other sample batch's shade / finish kernels, and the fused kernel (111 registers through the fetch-bound half) fills them
    // worse (config 5 +3 %, config 4 +-0.5 %: profiles/EXPERIMENTS.md)
    constexpr bool fuse = PackedFeat<TR>::value == 0;
    for (int j = 0; j < nLanes; j++) Wl[j].pingpong = fuse ? 1 : 0;
    int batch = 0;
    for (int b0 = sBegin; b0 < spp; b0 += (int)sb, batch++)
    {
        const int lane = batch % nLanes;
        const WfBuffers& W = Wl[lane];
        const hipStream_t sMain = laneMain[lane], sSide = laneSide[lane];
        if (k.maxDepth > 0) HIPCHK(c, hipMemsetAsync(W.grab, 0, (size_t)k.maxDepth * 16 * sizeof(int), sMain));
        g.batchStart = b0;
        g.batchCount = (int)std::min<long long>(sb, spp - b0);
        g.lastBatch = (b0 + g.batchCount >= spp) ? 1 : 0;
        for (int depth = 0; depth < k.maxDepth; depth++)
        {
            const int vsel = depth & 1;
            const bool lastBounce = depth + 1 >= k.maxDepth;        // its closest-hit walk only decides hit or miss
            constexpr int chained = PackedFeat<TR>::value > 0 ? 1 : 0;
            if (depth == 0)
            {
                if (count) hipLaunchKernelGGL((hrt_wf_shade_kernel<true, true>), gridR, block, 0, sMain, k, g, d.gb, resPrev, nPix, W, vsel, depth, cnt1);
                else       hipLaunchKernelGGL((hrt_wf_shade_kernel<false, true>), gridR, block, 0, sMain, k, g, d.gb, resPrev, nPix, W, vsel, depth, cnt1);
            }
            else if (fuse) { }                              // the vertices of this bounce were shaded by the fused finish + shade kernel of the last one
            else if (count) hipLaunchKernelGGL((hrt_wf_shade_kernel<true, false>), gridR, block, 0, sMain, k, g, d.gb, resPrev, nPix, W, vsel, depth, cnt1);
            else            hipLaunchKernelGGL((hrt_wf_shade_kernel<false, false>), gridR, block, 0, sMain, k, g, d.gb, resPrev, nPix, W, vsel, depth, cnt1);
            if constexpr (PackedFeat<TR>::value >= 0)
            {   // packed layout: persistent-wave walks + finish
                constexpr int F = PackedFeat<TR>::value;
                // production walks.  Boolean queries (shadow rays, the last bounce's hit-or-miss) of fast-sphere scenes walk the
                // device-built tree over the same instances when one was made at upload (hrt_walker.hpp, ALT)
                // scenes with big triangle meshes: the treelet-queued walker (hrt_walker_tl.hpp)
                const bool useTl = F != 0 && treelets && d.tl_ok && !count;
                int tlRc = HRT_OK;
                auto launch_shadow = [&](hipStream_t st) {
                    if constexpr (F != 0)
                        if (useTl)
                        {
                            const int rcT = d.dpacked.leafTris == 3 ? launch_tl_walk<F, true, false, 3>(c, d, tr, W, lane, cap, depth, st, gridW, gridR)
                                                                    : launch_tl_walk<F, true, false, 2>(c, d, tr, W, lane, cap, depth, st, gridW, gridR);
                            if (rcT != HRT_OK) tlRc = rcT;
                            return;
                        }
                    if constexpr (F == 0)
                        if (d.any_ok)
                        {
                            TR trAny = tr; trAny.P = d.dpackedAny;
                            hipLaunchKernelGGL((hrt_wf_walk_shadow_kernel<F, false, true>), chained ? gridW : gridR, block, 0, st, trAny, tr, W, vsel, depth, chained, cnt1);
                            return;
                        }
                    if (F != 0 && d.dpacked.leafTris == 3)
                        hipLaunchKernelGGL((hrt_wf_walk_shadow_kernel<F, false, false, (F != 0 ? 3 : 2)>), chained ? gridW : gridR, block, 0, st, tr, tr, W, vsel, depth, chained, cnt1);
                    else
                        hipLaunchKernelGGL((hrt_wf_walk_shadow_kernel<F, false>), chained ? gridW : gridR, block, 0, st, tr, tr, W, vsel, depth, chained, cnt1);
                };
                // with a second tree every production walk of the frame uses it, and so does the shading of their winners (leaf
                // slots are the second tree's)
                bool second = false;
                TR trFin = tr;
                if constexpr (F == 0) { second = d.any_ok && !count; if (second) trFin.P = d.dpackedAny; }
                auto launch_closest = [&](hipStream_t st) {
                    if constexpr (F != 0)
                        if (useTl)
                        {
                            const bool lt3 = d.dpacked.leafTris == 3;
                            const int rcT = lastBounce ? (lt3 ? launch_tl_walk<F, false, true, 3>(c, d, tr, W, lane, cap, depth, st, gridW, gridR)
                                                              : launch_tl_walk<F, false, true, 2>(c, d, tr, W, lane, cap, depth, st, gridW, gridR))
                                                       : (lt3 ? launch_tl_walk<F, false, false, 3>(c, d, tr, W, lane, cap, depth, st, gridW, gridR)
                                                              : launch_tl_walk<F, false, false, 2>(c, d, tr, W, lane, cap, depth, st, gridW, gridR));
                            if (rcT != HRT_OK) tlRc = rcT;
                            return;
                        }
                    if constexpr (F == 0)
                        if (lastBounce ? d.any_ok : second)
                        {
                            TR trAny = tr; trAny.P = d.dpackedAny;
                            if (lastBounce) hipLaunchKernelGGL((hrt_wf_walk_closest_kernel<F, false, true, true>), chained ? gridW : gridR, block, 0, st, trAny, tr, W, depth, chained, cnt1);
                            else            hipLaunchKernelGGL((hrt_wf_walk_closest_kernel<F, false, false, true>), chained ? gridW : gridR, block, 0, st, trAny, tr, W, depth, chained, cnt1);
                            return;
                        }
                    const bool lt3 = F != 0 && d.dpacked.leafTris == 3;
                    if (!lastBounce)
                    {
                        if (lt3) hipLaunchKernelGGL((hrt_wf_walk_closest_kernel<F, false, false, false, (F != 0 ? 3 : 2)>), chained ? gridW : gridR, block, 0, st, tr, tr, W, depth, chained, cnt1);
                        else     hipLaunchKernelGGL((hrt_wf_walk_closest_kernel<F, false>), chained ? gridW : gridR, block, 0, st, tr, tr, W, depth, chained, cnt1);
                        return;
                    }
                    if (lt3) hipLaunchKernelGGL((hrt_wf_walk_closest_kernel<F, false, true, false, (F != 0 ? 3 : 2)>), chained ? gridW : gridR, block, 0, st, tr, tr, W, depth, chained, cnt1);
                    else     hipLaunchKernelGGL((hrt_wf_walk_closest_kernel<F, false, true>), chained ? gridW : gridR, block, 0, st, tr, tr, W, depth, chained, cnt1);
                };
                // the winners' shading: on the last bounce the paths end (wf_finish); before it the fused kernel shades the next vertex
                auto launch_finish = [&](const TR& trF) {
                    if constexpr (fuse)
                        if (!lastBounce)
                        {
                            if (count) hipLaunchKernelGGL((hrt_wf_finish_shade_kernel<F, true>), gridR, block, 0, sMain, trF, k, g, d.gb, resPrev, nPix, W, vsel, depth, cnt1);
                            else       hipLaunchKernelGGL((hrt_wf_finish_shade_kernel<F, false>), gridR, block, 0, sMain, trF, k, g, d.gb, resPrev, nPix, W, vsel, depth, cnt1);
                            return;
                        }
                    if (count) hipLaunchKernelGGL((hrt_wf_finish_kernel<F, true>), gridR, block, 0, sMain, trF, k, W, vsel, depth);
                    else       hipLaunchKernelGGL((hrt_wf_finish_kernel<F, false>), gridR, block, 0, sMain, trF, k, W, vsel, depth);
                };
                if (count)
                {
                    hipLaunchKernelGGL((hrt_wf_walk_shadow_kernel<F, true>), chained ? gridW : gridR, block, 0, sMain, tr, tr, W, vsel, depth, chained, cnt1);
                    hipLaunchKernelGGL((hrt_wf_walk_closest_kernel<F, true>), chained ? gridW : gridR, block, 0, sMain, tr, tr, W, depth, chained, cnt1);
                    launch_finish(tr);
                }
                else if (chained)
                {   // the two walks of a bounce are independent (shadow requests vs bounce rays) and both are persistent
                    // launches that end in a drain: on two streams the second one's workgroups move into the wave slots
                    // the first one's drain frees, instead of waiting for its last ray
                    HIPCHK(c, hipEventRecord(d.evLane[lane][0], sMain));
                    HIPCHK(c, hipStreamWaitEvent(sSide, d.evLane[lane][0], 0));
                    launch_closest(sMain);
                    launch_shadow(sSide);
                    HIPCHK(c, hipEventRecord(d.evLane[lane][1], sSide));
                    HIPCHK(c, hipStreamWaitEvent(sMain, d.evLane[lane][1], 0));
                    launch_finish(trFin);
                }
                else
                {
                    launch_shadow(sMain);
                    launch_closest(sMain);
                    launch_finish(trFin);
                }
                if (tlRc != HRT_OK) return tlRc;
            }
            else
            {   // reference layout: one-ray-per-lane walks
                if (count)
                {
                    hipLaunchKernelGGL((hrt_wf_shadow_kernel<TR, true>), gridR, block, 0, sMain, tr, W, vsel, depth, cnt1);
                    hipLaunchKernelGGL((hrt_wf_closest_kernel<TR, true>), gridR, block, 0, sMain, tr, k, W, vsel, depth, cnt1);
                }
                else
                {
                    hipLaunchKernelGGL((hrt_wf_shadow_kernel<TR, false>), gridR, block, 0, sMain, tr, W, vsel, depth, cnt1);
                    hipLaunchKernelGGL((hrt_wf_closest_kernel<TR, false>), gridR, block, 0, sMain, tr, k, W, vsel, depth, cnt1);
                }
            }
        }
        // ordered part: Lframe is summed in sample order and resCur keeps its last writer, so a batch resolves after its predecessor
        if (batch > 0 && nLanes >= 2) HIPCHK(c, hipStreamWaitEvent(sMain, d.evLane[(batch - 1) % nLanes][2], 0));
        if (prog) hipLaunchKernelGGL(hrt_wf_resolve_prog_kernel, gridP, block, 0, sMain, k, g, d.gb, d.fb, resCur, W, carry);
        else      hipLaunchKernelGGL(hrt_wf_resolve_kernel, gridP, block, 0, sMain, k, g, d.gb, d.fb, resCur, W);
        HIPCHK(c, hipGetLastError());
        if (nLanes >= 2) HIPCHK(c, hipEventRecord(d.evLane[lane][2], sMain));
    }
    // the frame ends on the device's main stream: the resolves form one chain, so its last link covers every batch of both lanes
    if (nLanes >= 2 && batch > 1 && (batch - 1) % nLanes != 0) HIPCHK(c, hipStreamWaitEvent(d.stream, d.evLane[(batch - 1) % nLanes][2], 0));
    return HRT_OK;
}

// ---------------------------------------------------------------------------------------
// Ray queries (hrt_trace_rays, kernels in hrt_query.hpp).  Rays are walked in chunks of at most kQueryChunk, so the memory a query
// holds is bounded for any n; a 1920x1080 set of rays is one chunk.
// ---------------------------------------------------------------------------------------
constexpr int64_t kQueryChunk = HRT_QUERY_CHUNK;
constexpr size_t kQueryGrabBytes = 8 * kQueryGrabStride * sizeof(int);      // the hand-out counters of a packed walk
constexpr int kMaxQueryArgs = 4;

// One caller array of a query: `stride` bytes per ray; device pointers must be `align`-byte aligned (16 where the kernels read or write
// float4, 4 for ints), and the staged copy starts so.  args[0] holds the rays (read), the others are results (written); only an
// optional one (totals) may be null.
struct QueryArg { const void* p; size_t stride; unsigned align; bool optional; };

void free_query(DeviceState& d)
{
    d.q_dev.release();
    d.q_pin.release(true);
    d.mv_mem.release();
    d.dn_mem.release(); d.dn_pix = 0; d.dn_radiance = nullptr; d.dn_color = nullptr;
    d.dt_mem.release(); d.dt_w = d.dt_h = 0; d.dt_valid = false;
    for (hipEvent_t& e : d.q_ev) { if (e) (void)hipEventDestroy(e); e = nullptr; }
}

// p .. p + bytes lies in a range the caller page-locked (hrt_host_register): copies go straight to it, without pinned staging
bool registered(const hrt_ctx& cc, const void* p, size_t bytes)
{
    for (const auto& r : cc.pinned) if ((const char*)p >= r.first && (const char*)p + bytes <= r.first + r.second) return true;
    return false;
}

// The chunk sequence of a query on slot d's main stream (after any frame in flight), for rays [off, off + m) of the caller's arrays:
//   begin(): device workspace of workBytes (`work`) and the device addresses of the chunk's arrays (`dev`); H2D of the rays, first event
//   (the slot function enqueues its kernels)
//   end():   second event, one D2H per result array, synchronise, *ms += the events' time -- the kernels only
// dev_ptrs: the arrays are device memory of this slot: `dev` are the caller's own pointers, nothing is staged or allocated beyond `work`.
// Otherwise the arrays are carved behind the workspace in q_dev and, unless the caller registered their range, pass through q_pin.
// Both buffers grow only for a chunk that needs more than any before it.  The caller has made d's device current.
struct ChunkStager {
    hrt_ctx* c; const hrt_ctx& cc; DeviceState& d; const QueryArg* args; int nArgs; bool dev_ptrs;
    void* work = nullptr;
    void* dev[kMaxQueryArgs] = {};
    char* user[kMaxQueryArgs] = {}; char* pin[kMaxQueryArgs] = {}; size_t bytes[kMaxQueryArgs] = {};     // pin[i] == nullptr: no staging

    int begin(int64_t off, int64_t m, size_t workBytes)
    {
        size_t devNeed = (workBytes + 15) & ~(size_t)15, pinNeed = 0, devOff[kMaxQueryArgs] = {}, pinOff[kMaxQueryArgs] = {};
        for (int i = 0; i < nArgs; i++)
        {
            user[i] = args[i].p ? (char*)args[i].p + (size_t)off * args[i].stride : nullptr;
            bytes[i] = user[i] ? (size_t)m * args[i].stride : 0;
            if (dev_ptrs) continue;
            const size_t a = args[i].align - 1;
            devOff[i] = devNeed = (devNeed + a) & ~a; devNeed += bytes[i];
            pinOff[i] = pinNeed = (pinNeed + a) & ~a; pinNeed += bytes[i];
        }
        int rc;
        if ((rc = d.q_dev.grow(c, devNeed, d.stream)) != HRT_OK) return rc;
        if ((rc = d.q_pin.grow(c, pinNeed, d.stream, Scratch::kStream, true)) != HRT_OK) return rc;
        work = d.q_dev.p;
        for (int i = 0; i < nArgs; i++)
        {
            dev[i] = dev_ptrs || !user[i] ? (void*)user[i] : (void*)((char*)d.q_dev.p + devOff[i]);
            pin[i] = dev_ptrs || !user[i] || registered(cc, user[i], bytes[i]) ? nullptr : (char*)d.q_pin.p + pinOff[i];
        }
        if (!dev_ptrs)
        {
            if (pin[0]) std::memcpy(pin[0], user[0], bytes[0]);
            HIPCHK(c, hipMemcpyAsync(dev[0], pin[0] ? pin[0] : user[0], bytes[0], hipMemcpyHostToDevice, d.stream));
        }
        HIPCHK(c, hipEventRecord(d.q_ev[0], d.stream));
        return HRT_OK;
    }

    int end(float* ms)
    {
        HIPCHK(c, hipEventRecord(d.q_ev[1], d.stream));
        if (!dev_ptrs)
            for (int i = 1; i < nArgs; i++)
                if (user[i]) HIPCHK(c, hipMemcpyAsync(pin[i] ? pin[i] : user[i], dev[i], bytes[i], hipMemcpyDeviceToHost, d.stream));
        HIPCHK(c, hipStreamSynchronize(d.stream));
        float t = 0.f;
        HIPCHK(c, hipEventElapsedTime(&t, d.q_ev[0], d.q_ev[1]));
        *ms += t;
        for (int i = 1; i < nArgs; i++) if (pin[i]) std::memcpy(user[i], pin[i], bytes[i]);
        return HRT_OK;
    }
};

template <int F>
void launch_query_packed(const DeviceState& d, int query, const QueryK& q, hipStream_t st)
{
    TracerPackedT<F> tr; tr.P = d.dpacked; tr.S = d.dscene;
    const dim3 block(256), gridR((unsigned)((q.n + 255) / 256));
    const dim3 gridW((unsigned)std::min<long long>((q.nSegs + 3) / 4, (long long)d.n_cu * kWalkBlocksPerCU));     // persistent waves, as a chained walk
    const bool lt3 = F != 0 && d.dpacked.leafTris == 3;           // triangle records per leaf step, chosen at upload (DPacked::leafTris)
    if (query == HRT_QUERY_OCCLUDED)
    {
        if (lt3) hipLaunchKernelGGL((hrt_query_occluded_kernel<F, (F != 0 ? 3 : 2)>), gridW, block, 0, st, tr, q);
        else     hipLaunchKernelGGL((hrt_query_occluded_kernel<F, 2>), gridW, block, 0, st, tr, q);
        return;
    }
    if (lt3) hipLaunchKernelGGL((hrt_query_closest_kernel<F, (F != 0 ? 3 : 2)>), gridW, block, 0, st, tr, q);
    else     hipLaunchKernelGGL((hrt_query_closest_kernel<F, 2>), gridW, block, 0, st, tr, q);
    hipLaunchKernelGGL((hrt_query_finish_kernel<F>), gridR, block, 0, st, tr, q);
}

// rays with a non-finite origin or direction, which the packed walks leave out (hrt_query.hpp), on the reference's arrays
void launch_query_fixup(const DeviceState& d, int query, const QueryK& q, hipStream_t st)
{
    TracerRef t; t.S = d.dscene;
    const dim3 block(256), gridR((unsigned)((q.n + 255) / 256));
    if (query == HRT_QUERY_OCCLUDED) hipLaunchKernelGGL((hrt_query_ref_kernel<true, true>), gridR, block, 0, st, t, q);
    else                             hipLaunchKernelGGL((hrt_query_ref_kernel<false, true>), gridR, block, 0, st, t, q);
}

// the walk (+ finish) of q.n <= kQueryChunk rays already on the device; q.raw / q.grab point into d's staging
int launch_query(hrt_ctx* c, const hrt_ctx& cc, DeviceState& d, int query, const QueryK& q, hipStream_t st)
{
    if (cc.packed_ok)
    {
        HIPCHK(c, hipMemsetAsync(q.grab, 0, kQueryGrabBytes, st));
        if (cc.packed_feat == 0)      launch_query_packed<0>(d, query, q, st);
        else if (cc.packed_feat == 1) launch_query_packed<1>(d, query, q, st);
        else                          launch_query_packed<3>(d, query, q, st);
        launch_query_fixup(d, query, q, st);
    }
    else
    {
        TracerRef t; t.S = d.dscene;
        const dim3 block(256), gridR((unsigned)((q.n + 255) / 256));
        if (query == HRT_QUERY_OCCLUDED) hipLaunchKernelGGL((hrt_query_ref_kernel<true, false>), gridR, block, 0, st, t, q);
        else                             hipLaunchKernelGGL((hrt_query_ref_kernel<false, false>), gridR, block, 0, st, t, q);
    }
    HIPCHK(c, hipGetLastError());
    return HRT_OK;
}

// rays [begin, end) of one device slot, chunk by chunk (ChunkStager): walk, finish, fix-up.  The chunk's workspace is the raw winners of
// the walk (16 B per ray), then the 8 hand-out counters.
int query_slot(hrt_ctx* c, const hrt_ctx& cc, DeviceState& d, int query, const QueryArg* args, int64_t begin, int64_t end, bool dev_ptrs, float* ms)
{
    HIPCHK(c, hipSetDevice(d.device_id));
    ChunkStager s{c, cc, d, args, 2, dev_ptrs};
    for (int64_t off = begin; off < end; off += kQueryChunk)
    {
        const int64_t m = std::min<int64_t>(kQueryChunk, end - off);
        int rc = s.begin(off, m, (size_t)m * 16 + kQueryGrabBytes);
        if (rc != HRT_OK) return rc;
        QueryK q;
        q.raw = (float4*)s.work;
        q.grab = (int*)((char*)s.work + (size_t)m * 16);
        q.n = (int)m; q.nSegs = (int)((m + kQuerySeg - 1) / kQuerySeg);
        q.rays = (const float4*)s.dev[0];
        q.hits = (float4*)s.dev[1]; q.occ = (int32_t*)s.dev[1];
        if ((rc = launch_query(c, cc, d, query, q, d.stream)) != HRT_OK) return rc;
        if ((rc = s.end(ms)) != HRT_OK) return rc;
    }
    return HRT_OK;
}

// ---------------------------------------------------------------------------------------
// Multi-hit queries (hrt_trace_hits, kernels in hrt_hits.hip).  A chunk holds at most kQueryChunk hit slots (rays * k), so the staging
// does not grow with k.  The walk keeps each ray's candidates in the ray's own hit slots and the finish shades them in place: the
// device workspace is the 8 hand-out counters.
// ---------------------------------------------------------------------------------------
// rays [begin, end) of one device slot, chunk by chunk (ChunkStager): walk, finish, fix-up
int hits_slot(hrt_ctx* c, const hrt_ctx& cc, DeviceState& d, int k, const QueryArg* args, int64_t begin, int64_t end, bool dev_ptrs, float* ms)
{
    HIPCHK(c, hipSetDevice(d.device_id));
    ChunkStager s{c, cc, d, args, 4, dev_ptrs};
    const int64_t per = std::max<int64_t>(1, kQueryChunk / k);          // rays per chunk: at most kQueryChunk hit slots
    for (int64_t off = begin; off < end; off += per)
    {
        const int64_t m = std::min<int64_t>(per, end - off);
        int rc = s.begin(off, m, kQueryGrabBytes);
        if (rc != HRT_OK) return rc;
        HitsLaunch L;
        L.variant = cc.packed_ok ? cc.packed_feat : -1;
        L.lt3 = cc.packed_feat != 0 && d.dpacked.leafTris == 3;
        L.S = d.dscene; L.P = d.dpacked;
        HitsK& h = L.h;
        h.grab = (int*)s.work;
        h.n = (int)m; h.k = k; h.nSegs = (int)((m + kQuerySeg - 1) / kQuerySeg);
        L.gridW = (unsigned)std::min<long long>((h.nSegs + 3) / 4, (long long)d.n_cu * kWalkBlocksPerCU);     // persistent waves, as hrt_trace_rays
        h.rays = (const float4*)s.dev[0]; h.hits = (float4*)s.dev[1]; h.counts = (int32_t*)s.dev[2]; h.totals = (int32_t*)s.dev[3];
        HIPCHK(c, hits_launch(L, d.stream));
        if ((rc = s.end(ms)) != HRT_OK) return rc;
    }
    return HRT_OK;
}

// dev < 0 reads and writes through the host: device memory there would be dereferenced by the CPU
bool in_device_memory(const void* p)
{
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }       // unknown to HIP: pageable host memory
    return a.type == hipMemoryTypeDevice;
}

// dev >= 0 takes device memory of that slot only: a host pointer, another device's memory or a range that runs past its allocation is refused
bool on_device(const DeviceState& d, const void* p, size_t bytes)
{
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    if (a.type != hipMemoryTypeDevice || a.device != d.device_id) return false;
    hipDeviceptr_t lo = nullptr; size_t size = 0;
    if (hipMemGetAddressRange(&lo, &size, (hipDeviceptr_t)p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return (const char*)p >= (const char*)lo && (const char*)p + bytes <= (const char*)lo + size;
}

// What the three caller-ray queries share once an entry point has made its own checks.  The texts carry the function's words:
// `needed` the arrays a call with n > 0 must pass, `all` every array, `aligned` the alignment rule of device pointers.
struct QueryDoor { const char* who; const char* needed; const char* all; const char* aligned; bool sceneBeforeEmpty; };
using QuerySlotFn = std::function<int(hrt_ctx* ec, DeviceState& d, int64_t begin, int64_t end, bool dev_ptrs, float* ms)>;

// dev >= 0: the arrays are device memory of that slot, walked in place.  dev < 0: host memory, cut into one contiguous part per
// device slot; *device_ms is the largest of the slots' kernel times.
int run_query(hrt_ctx* c, const QueryDoor& q, const QueryArg* args, int nArgs, int64_t n, int32_t dev, float* device_ms, const QuerySlotFn& slot)
{
    const std::string who = std::string(q.who) + ": ";
    if (n < 0) return fail(c, HRT_ERR_INVALID_ARG, who + "n must be >= 0");
    for (int i = 0; i < nArgs; i++)
        if (n > 0 && !args[i].p && !args[i].optional) return fail(c, HRT_ERR_INVALID_ARG, who + q.needed + " are needed when n > 0");
    const int nd = (int)c->dev.size();
    if (dev >= nd) return fail(c, HRT_ERR_INVALID_ARG, who + "device slot out of range");
    if (n == 0 && !q.sceneBeforeEmpty) return HRT_OK;
    if (!c->scene_ready) return fail(c, HRT_ERR_INVALID_STATE, who + "no scene uploaded (call hrt_scene_upload first)");
    if (n == 0) return HRT_OK;
    if (dev >= 0)
    {
        DeviceState& d = c->dev[(size_t)dev];
        HIPCHK(c, hipSetDevice(d.device_id));
        for (int i = 0; i < nArgs; i++)
            if (args[i].p && !on_device(d, args[i].p, (size_t)n * args[i].stride))
                return fail(c, HRT_ERR_INVALID_ARG, who + "with dev >= 0, " + q.all + " must be device memory of that slot's device, large enough for n");
        for (int i = 0; i < nArgs; i++)
            if ((uintptr_t)args[i].p & (args[i].align - 1)) return fail(c, HRT_ERR_INVALID_ARG, who + "device " + q.aligned);
        float ms = 0.f;
        int rc = slot(c, d, 0, n, true, &ms);
        if (rc != HRT_OK) return rc;
        if (device_ms) *device_ms = ms;
        return HRT_OK;
    }
    for (int i = 0; i < nArgs; i++)
        if (args[i].p && in_device_memory(args[i].p))
            return fail(c, HRT_ERR_INVALID_ARG, who + "with dev < 0, " + q.all + " must be host memory (pass the slot of device pointers as dev)");
    std::vector<float> ms((size_t)nd, 0.f);
    int rc = for_each_slot(c, nd > 1, q.who, "", [&](int i, hrt_ctx* ec) {
        return slot(ec, c->dev[(size_t)i], n * i / nd, n * (i + 1) / nd, false, &ms[(size_t)i]);
    });
    if (rc != HRT_OK) return rc;
    if (device_ms) *device_ms = *std::max_element(ms.begin(), ms.end());
    return HRT_OK;
}

} // namespace

extern "C" {

const char* hrt_version(void)
{
#if defined(HRT_TEST_HOOKS)
    return "hip_raytrace 0.4 (gfx950) test-hooks";
#else
    return "hip_raytrace 0.4 (gfx950)";
#endif
}

int hrt_device_count(void)
try {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return -1;
    return n;
}
catch (...) { return on_exception(nullptr, "hrt_device_count"); }

const char* hrt_last_error(hrt_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int hrt_create(const int* device_ids, int n_dev, hrt_ctx** out)
try {
    if (!out) return fail(nullptr, HRT_ERR_INVALID_ARG, "hrt_create: out is NULL");
    *out = nullptr;
    int avail = 0;
    hipError_t e = hipGetDeviceCount(&avail);
    if (e != hipSuccess || avail <= 0)
        return fail(nullptr, HRT_ERR_NO_DEVICE, std::string("hrt_create: no HIP device (") + hipGetErrorString(e) + "); this library has no CPU path");
    std::vector<int> ids;
    if (device_ids && n_dev > 0) ids.assign(device_ids, device_ids + n_dev);
    else ids.push_back(0);
    for (int id : ids)
        if (id < 0 || id >= avail) return fail(nullptr, HRT_ERR_INVALID_ARG, "hrt_create: device id out of range");
    struct CtxGuard { hrt_ctx* p; ~CtxGuard() { if (p) hrt_destroy(p); } } guard{new hrt_ctx()};      // an exception below must not leak the context
    hrt_ctx* c = guard.p;
    c->dev.resize(ids.size());
    for (size_t i = 0; i < ids.size(); i++)
    {
        DeviceState& d = c->dev[i];
        d.device_id = ids[i];
        hipError_t err = hipSetDevice(d.device_id);
        if (err == hipSuccess) { int cu = 0; if (hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, d.device_id) == hipSuccess && cu > 0) d.n_cu = cu; }
        if (err == hipSuccess) { int lds = 0; if (hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, d.device_id) == hipSuccess && lds > 0) d.max_lds = lds; }
        if (err == hipSuccess) err = hipStreamCreateWithFlags(&d.stream, hipStreamNonBlocking);
        if (err == hipSuccess) err = hipStreamCreateWithFlags(&d.stream2, hipStreamNonBlocking);
        for (int j = 1; j < kBatchLanes && err == hipSuccess; j++)
            for (int e = 0; e < 2 && err == hipSuccess; e++) err = hipStreamCreateWithFlags(&d.laneStream[j][e], hipStreamNonBlocking);
        for (int j = 0; j < kMaxLanes && err == hipSuccess; j++)
            for (int e = 0; e < 3 && err == hipSuccess; e++) err = hipEventCreateWithFlags(&d.evLane[j][e], hipEventDisableTiming);
        if (err == hipSuccess) err = hipEventCreateWithFlags(&d.evStage, hipEventDisableTiming);
        for (int f = 0; f < DeviceState::kRing && err == hipSuccess; f++)
            for (int k = 0; k < 4 && err == hipSuccess; k++) err = hipEventCreate(&d.ev[f][k]);
        for (int e = 0; e < 2 && err == hipSuccess; e++) err = hipEventCreate(&d.q_ev[e]);
        if (err == hipSuccess) { void* p = nullptr; err = hipMalloc(&p, 20 * sizeof(unsigned long long)); d.counters = (unsigned long long*)p; }
        if (err != hipSuccess)
        {
            std::string m = std::string("hrt_create: ") + hipGetErrorString(err);
            return fail(nullptr, HRT_ERR_HIP, m);           // the guard destroys the half-made context
        }
    }
    for (size_t i = 0; i < ids.size(); i++)
        for (size_t j = 0; j < ids.size(); j++)
            if (ids[i] != ids[j])
            {   // tiles are exchanged device-to-device when ReSTIR reuse is on (xGMI peer copies)
                (void)hipSetDevice(ids[i]);
                hipError_t pe = hipDeviceEnablePeerAccess(ids[j], 0);
                if (pe != hipSuccess && pe != hipErrorPeerAccessAlreadyEnabled) (void)hipGetLastError();
            }
    guard.p = nullptr;
    *out = c;
    return HRT_OK;
}
catch (...) { return on_exception(nullptr, "hrt_create"); }

void hrt_destroy(hrt_ctx* c)
{
    if (!c) return;
    for (DeviceState& d : c->dev) if (d.device_id >= 0 && d.stream) { (void)hipSetDevice(d.device_id); (void)hipStreamSynchronize(d.stream); }
    for (const auto& r : c->pinned) (void)hipHostUnregister(r.first);
    c->pinned.clear();
    for (DeviceState& d : c->dev)
    {
        if (d.device_id < 0) continue;
        (void)hipSetDevice(d.device_id);
        if (d.stream) (void)hipStreamSynchronize(d.stream);
        free_pixels(d);
        free_scene(d);
        free_workspace(d);
        free_present(d);
        free_query(d);
        if (d.counters) (void)hipFree(d.counters);
        for (int f = 0; f < DeviceState::kRing; f++)
            for (int k = 0; k < 4; k++) if (d.ev[f][k]) (void)hipEventDestroy(d.ev[f][k]);
        if (d.stream2) { (void)hipStreamSynchronize(d.stream2); (void)hipStreamDestroy(d.stream2); }
        for (int j = 1; j < kMaxLanes; j++) for (int e = 0; e < 2; e++) if (d.laneStream[j][e]) { (void)hipStreamSynchronize(d.laneStream[j][e]); (void)hipStreamDestroy(d.laneStream[j][e]); }
        for (int j = 0; j < kMaxLanes; j++) for (int e = 0; e < 3; e++) if (d.evLane[j][e]) (void)hipEventDestroy(d.evLane[j][e]);
        if (d.evStage) (void)hipEventDestroy(d.evStage);
        if (d.stream) (void)hipStreamDestroy(d.stream);
    }
    delete c;
}

int hrt_synchronize(hrt_ctx* c, hrt_stats* stats)
try {
    if (!c) return HRT_ERR_INVALID_ARG;
    hrt_stats st; std::memset(&st, 0, sizeof(st));
    st.n_devices = (int)c->dev.size();
    for (DeviceState& d : c->dev)
    {
        HIPCHK(c, hipSetDevice(d.device_id));
        HIPCHK(c, hipStreamSynchronize(d.stream));        // _cuda.Synchronize(), RTRenderer.cs:233
        double k0 = 0, k1 = 0, dh = 0;
        if (d.ring_head > 0) { d.frame_ms[0].clear(); d.frame_ms[1].clear(); }
        for (int f = 0; f < d.ring_head; f++)
        {
            float ms;
            HIPCHK(c, hipEventElapsedTime(&ms, d.ev[f][0], d.ev[f][1])); k0 += ms; d.frame_ms[0].push_back(ms);
            HIPCHK(c, hipEventElapsedTime(&ms, d.ev[f][1], d.ev[f][2])); k1 += ms; d.frame_ms[1].push_back(ms);
            HIPCHK(c, hipEventElapsedTime(&ms, d.ev[f][2], d.ev[f][3])); dh += ms;
        }
        st.kernel_ms[0] = std::max(st.kernel_ms[0], k0);
        st.kernel_ms[1] = std::max(st.kernel_ms[1], k1);
        st.d2h_ms = std::max(st.d2h_ms, dh);
        st.frames = std::max(st.frames, d.ring_head);
        if (d.ring_counts)
        {
            unsigned long long h[20];
            HIPCHK(c, hipMemcpy(h, d.counters, sizeof(h), hipMemcpyDeviceToHost));
            for (int kk = 0; kk < 2; kk++)
            {
                uint64_t* dst = reinterpret_cast<uint64_t*>(&st.k[kk]);
                for (int i = 0; i < 10; i++) dst[i] += h[kk * 10 + i];
            }
            st.counters_valid = 1;
        }
        d.ring_head = 0;
        d.ring_counts = false;
    }
    if (stats) *stats = st;
    return HRT_OK;
}
catch (...) { return on_exception(c, "hrt_synchronize"); }

int hrt_reset_history(hrt_ctx* c)
try {
    if (!c) return HRT_ERR_INVALID_ARG;
    c->prog.valid = false;                     // a progressive frame cannot be continued across this call
    int rc = hrt_synchronize(c, nullptr);
    if (rc != HRT_OK) return rc;
    for (DeviceState& d : c->dev)
    {
        d.taa_history_valid = false;
        d.dt_valid = false;
        if (d.nPix == 0) continue;
        HIPCHK(c, hipSetDevice(d.device_id));
        DReservoir* rs[2] = {&d.resA, &d.resB};
        for (DReservoir* r : rs)
        {
            HIPCHK(c, hipMemsetAsync(r->L, 0, d.nPix * 12, d.stream)); HIPCHK(c, hipMemsetAsync(r->wi, 0, d.nPix * 12, d.stream));
            HIPCHK(c, hipMemsetAsync(r->pdf, 0, d.nPix * 4, d.stream)); HIPCHK(c, hipMemsetAsync(r->w, 0, d.nPix * 4, d.stream));
            HIPCHK(c, hipMemsetAsync(r->wSum, 0, d.nPix * 4, d.stream)); HIPCHK(c, hipMemsetAsync(r->m, 0, d.nPix * 4, d.stream));
            HIPCHK(c, hipMemsetAsync(r->lightId, 0, d.nPix * 4, d.stream));
        }
        HIPCHK(c, hipStreamSynchronize(d.stream));
    }
    return HRT_OK;
}
catch (...) { return on_exception(c, "hrt_reset_history"); }

// the kernels' frame constants of params (the row range and strips are the caller's)
static FrameK frame_consts(const hrt_frame_params* p)
{
    FrameK k;
    k.width = p->width; k.height = p->height; k.frame = p->frame;
    k.row_begin = 0; k.row_end = p->height; k.strip_n = 1; k.strip_i = 0;
    k.cam = p->cam; k.prevCam = p->prevCam;
    k.dirLightDir = p->dirLightDir; k.dirLightRadiance = p->dirLightRadiance;
    {   // Float3.Normalize(k.dirLightDir) (RTRay.cs:464) is the same for every vertex of the frame: evaluated here, by the contract's
        // host definitions (IEEE sqrt and division, maxNum: include/hrt_math.h), instead of at every diffuse vertex on the device
        const float x = p->dirLightDir.X, y = p->dirLightDir.Y, z = p->dirLightDir.Z;
        const float inv = hrt_rsqrt(hrt_fmax(1e-20f, x * x + y * y + z * z));
        k.dirLightN.X = x * inv; k.dirLightN.Y = y * inv; k.dirLightN.Z = z * inv;
    }
    k.skyTop = p->skyTintTop; k.skyBottom = p->skyTintBottom;
    k.debugCamSeq = p->debugCamSeq; k.enableTemporal = p->enableTemporalReuse; k.enableSpatial = p->enableSpatialReuse;
    k.rngLockNoise = p->rngLockNoise; k.spp = p->spp; k.maxDepth = p->maxDepth;
    return k;
}

// hrt_render_frame (progBegin < 0) and hrt_render_progressive (progBegin = sample_begin >= 0): one body, the progressive call renders
// samples [progBegin, spp) and carries the raw sample sum in DeviceState::prog_carry; a continuation (progBegin > 0) keeps the G-buffer
// of the call that started the frame instead of running primary visibility again.
static int render_impl(hrt_ctx* c, const hrt_frame_params* p, const hrt_render_opts* opts, const hrt_outputs* out, hrt_stats* stats,
                       const char* who, int progBegin)
{
    const bool prog = progBegin >= 0, cont = progBegin > 0;
    if (!prog) c->prog.valid = false;          // a one-shot frame ends any progressive one
    if (!p) return fail(c, HRT_ERR_INVALID_ARG, std::string(who) + ": params is NULL");
    if (!c->scene_ready) return fail(c, HRT_ERR_INVALID_STATE, std::string(who) + ": no scene uploaded (call hrt_scene_upload first)");
    if (p->width <= 0 || p->height <= 0) return fail(c, HRT_ERR_INVALID_ARG, std::string(who) + ": width/height must be positive");
    if ((int64_t)p->width * p->height > 0x7FFFFFFFLL) return fail(c, HRT_ERR_INVALID_ARG, std::string(who) + ": image too large for int pixel indices");
    if (p->maxDepth < 0) return fail(c, HRT_ERR_INVALID_ARG, std::string(who) + ": maxDepth must be >= 0");
    const uint32_t flags = opts ? opts->flags : 0u;
    int rb = opts ? opts->row_begin : 0, re = opts ? opts->row_end : 0;
    int sn = opts && opts->strip_n > 0 ? opts->strip_n : 1, si = opts ? opts->strip_i : 0;
    if (rb == 0 && re == 0) re = p->height;
    if (rb < 0 || re > p->height || rb > re) return fail(c, HRT_ERR_INVALID_ARG, std::string(who) + ": row range outside the image");
    if (si < 0 || si >= sn) return fail(c, HRT_ERR_INVALID_ARG, std::string(who) + ": strip_i must be in [0, strip_n)");
    const bool nosync = (flags & HRT_FLAG_NO_SYNC) != 0;
    if (nosync && out) return fail(c, HRT_ERR_INVALID_ARG, std::string(who) + ": HRT_FLAG_NO_SYNC frames cannot gather to host (outputs must be NULL)");
    const bool reuse = (p->enableTemporalReuse != 0 || p->enableSpatialReuse != 0);
    const int nd = (int)c->dev.size();
    const bool primaryOnly = (flags & HRT_FLAG_PRIMARY_ONLY) != 0;
    if (primaryOnly && (flags & HRT_FLAG_SKIP_PRIMARY)) return fail(c, HRT_ERR_INVALID_ARG, std::string(who) + ": PRIMARY_ONLY and SKIP_PRIMARY exclude each other");
    if (reuse && !primaryOnly && !(flags & HRT_FLAG_EXCHANGED) && (sn > 1 || rb != 0 || re != p->height))
        return fail(c, HRT_ERR_INVALID_STATE, std::string(who) + ": ReSTIR reuse needs every pixel's G-buffer and previous reservoir: render reuse frames as full images, "
                    "or exchange tiles between processes and say so (HRT_FLAG_PRIMARY_ONLY / HRT_FLAG_EXCHANGED; one ctx over several devices exchanges tiles itself)");
    if (reuse && nd > 1 && nosync) return fail(c, HRT_ERR_INVALID_ARG, std::string(who) + ": multi-device reuse frames cannot be enqueued with HRT_FLAG_NO_SYNC");
    const int64_t nPix = (int64_t)p->width * p->height;
    const bool count = (flags & HRT_FLAG_COUNTERS) != 0;
    constexpr uint32_t kPathFlags = HRT_FLAG_REFERENCE_LAYOUT | HRT_FLAG_MEGAKERNEL | HRT_FLAG_STREAMED | HRT_FLAG_TREELETS;
    if (prog)
    {   // every refusal comes before anything is enqueued or allocated: a refused call leaves the frame it would continue intact
        if (flags & (HRT_FLAG_COUNTERS | HRT_FLAG_PRIMARY_ONLY | HRT_FLAG_SKIP_PRIMARY | HRT_FLAG_EXCHANGED))
            return fail(c, HRT_ERR_INVALID_ARG, std::string(who) + ": HRT_FLAG_COUNTERS, PRIMARY_ONLY, SKIP_PRIMARY and EXCHANGED cannot be used with progressive frames");
        if (p->spp < 1) return fail(c, HRT_ERR_INVALID_ARG, std::string(who) + ": params->spp must be >= 1");
        if (p->spp <= progBegin) return fail(c, HRT_ERR_INVALID_ARG, std::string(who) + ": params->spp (" + std::to_string(p->spp) + ") must exceed sample_begin (" + std::to_string(progBegin) + ")");
        if (cont)
        {
            const auto& q = c->prog;
            if (!q.valid)
                return fail(c, HRT_ERR_INVALID_STATE, std::string(who) + ": no progressive frame to continue (start one with sample_begin = 0; hrt_render_frame, scene uploads / updates, "
                            "hrt_reset_history and resizes end it)");
            if (progBegin != q.p.spp)
                return fail(c, HRT_ERR_INVALID_STATE, std::string(who) + ": sample_begin (" + std::to_string(progBegin) + ") differs from the samples rendered so far (" + std::to_string(q.p.spp) + ")");
#define HRT_PROG_FIELD(f) { #f, offsetof(hrt_frame_params, f), sizeof(p->f) }
            static const struct { const char* name; size_t off, size; } kFields[] = {
                HRT_PROG_FIELD(width), HRT_PROG_FIELD(height), HRT_PROG_FIELD(frame), HRT_PROG_FIELD(cam), HRT_PROG_FIELD(prevCam),
                HRT_PROG_FIELD(dirLightDir), HRT_PROG_FIELD(dirLightRadiance), HRT_PROG_FIELD(skyTintTop), HRT_PROG_FIELD(skyTintBottom),
                HRT_PROG_FIELD(debugCamSeq), HRT_PROG_FIELD(enableTemporalReuse), HRT_PROG_FIELD(enableSpatialReuse), HRT_PROG_FIELD(rngLockNoise),
                HRT_PROG_FIELD(maxDepth)};
#undef HRT_PROG_FIELD
            for (const auto& f : kFields)        // bitwise: every field but spp
                if (std::memcmp((const char*)p + f.off, (const char*)&q.p + f.off, f.size) != 0)
                    return fail(c, HRT_ERR_INVALID_STATE, std::string(who) + ": params->" + f.name + " differs from the progressive frame being continued");
            if (rb != q.rb || re != q.re) return fail(c, HRT_ERR_INVALID_STATE, std::string(who) + ": the row range differs from the progressive frame being continued");
            if (sn != q.sn || si != q.si) return fail(c, HRT_ERR_INVALID_STATE, std::string(who) + ": strip_n / strip_i differ from the progressive frame being continued");
            if ((flags & kPathFlags) != q.pathFlags)
                return fail(c, HRT_ERR_INVALID_STATE, std::string(who) + ": the path-selecting flags (REFERENCE_LAYOUT, MEGAKERNEL, STREAMED, TREELETS) differ from the progressive frame being continued");
        }
        c->prog.valid = false;                 // until this call is enqueued
    }

    if (nPix != c->dev[0].nPix || c->dev[0].ring_head >= DeviceState::kRing)
    {   // resize (or a full event ring) drains the frames in flight first
        int rc = hrt_synchronize(c, nullptr);
        if (rc != HRT_OK) return rc;
    }
    for (DeviceState& d : c->dev)
    {
        int rc = ensure_pixels(c, d, nPix);
        if (rc != HRT_OK) return rc;
        if (prog && !d.prog_carry)
        {   // not initialised: the call that starts a frame (sample_begin 0) seeds its sums with zero and only stores
            void* v = nullptr;
            HIPCHK(c, hipSetDevice(d.device_id));
            HIPCHK(c, hipMalloc(&v, (size_t)nPix * sizeof(hrt_float3)));
            d.prog_carry = (hrt_float3*)v;
        }
    }
    c->width = p->width; c->height = p->height;
    c->frame_cam = p->cam; c->frame_prev_cam = p->prevCam;
    c->frame_serial++;

    // 8-row strips of [rb,re) are dealt round-robin: this call owns strips s % sn == si, and
    // device i of the ctx takes every nd-th of those (sky rows are cheap, geometry rows are
    // expensive: interleaving balances the tiles without knowing the image)
    const int S = (re - rb + 7) / 8;
    for (int i = 0; i < nd; i++)
    {
        DeviceState& d = c->dev[i];
        d.row_begin = rb; d.row_end = re;
        d.strip_n = sn * nd; d.strip_i = si + sn * i;
        d.n_strips = d.strip_i < S ? (S - d.strip_i + d.strip_n - 1) / d.strip_n : 0;
    }

    // Framebuffer.GetReservoirPair: even frame -> prev = B, cur = A (Framebuffer.cs:132-145)
    const bool even = (p->frame & 1) == 0;
    const bool exchange = reuse && nd > 1;      // ReSTIR reuse reads other tiles' G-buffer and previous reservoirs
    auto frame_k = [&](const DeviceState& d) {
        FrameK k = frame_consts(p);
        k.row_begin = d.row_begin; k.row_end = d.row_end; k.strip_n = d.strip_n; k.strip_i = d.strip_i;
        return k;
    };
    // pixel kernels: four waves per workgroup, each on an 8x8 tile, side by side (a 32x8 tile: the 256 lanes of the path-trace
    // kernels' launch bounds)
    const bool mega = (flags & HRT_FLAG_MEGAKERNEL) ? true : ((flags & HRT_FLAG_STREAMED) ? false : c->small_scene);
    constexpr int ptWaves = 4;
    auto tile_map = [&](const DeviceState& d) {
        TileMap tm;
        tm.wpb = ptWaves;
        tm.tilesX = (p->width + 8 * ptWaves - 1) / (8 * ptWaves);
        tm.tilesY = d.n_strips;
        tm.nTiles = tm.tilesX * tm.tilesY;
        tm.band = !(mega && c->small_scene);
        return tm;
    };
    // tracer variant: the smallest packed walker that covers the committed scene, or the reference layout
    const bool usePacked = c->packed_ok && !(flags & HRT_FLAG_REFERENCE_LAYOUT);
    const int variant = usePacked ? c->packed_feat : -1;
    // production frames of a tiny fast-sphere scene in the fused kernel: wave-uniform sweep over the TLAS leaves
    const bool flat = variant == 0 && mega && !count && c->flat_leaves > 0;
    auto with_tracer = [&](DeviceState& d, auto fn) -> int {
        if (flat) { TracerFlat t; t.tree.P = d.dpacked; t.tree.S = d.dscene; t.leaves = (const NodeQ*)d.packed[4]; t.nLeaves = c->flat_leaves; return fn(t); }
        if (variant == 0)      { TracerPackedT<0> t; t.P = d.dpacked; t.S = d.dscene; return fn(t); }
        else if (variant == 1) { TracerPackedT<1> t; t.P = d.dpacked; t.S = d.dscene; return fn(t); }
        else if (variant == 3) { TracerPackedT<3> t; t.P = d.dpacked; t.S = d.dscene; return fn(t); }
        TracerRef t; t.S = d.dscene; return fn(t);
    };
    // all-gather of per-pixel arrays between the devices of the ctx: every device receives the strips the others own.
    // Copies run on the RECEIVER's stream after it has waited for the owner's event, so no host synchronisation is needed.
    auto exchange_arrays = [&](int evIndex, auto get_arrays) -> int {
        for (int j = 0; j < nd; j++)
        {
            DeviceState& dst = c->dev[j];
            HIPCHK(c, hipSetDevice(dst.device_id));
            for (int i = 0; i < nd; i++)
            {
                if (i == j) continue;
                DeviceState& src = c->dev[i];
                HIPCHK(c, hipStreamWaitEvent(dst.stream, src.ev[src.ring_head][evIndex], 0));
                int rc = get_arrays(src, dst);
                if (rc != HRT_OK) return rc;
            }
        }
        return HRT_OK;
    };
    const int W = p->width;

    // ---- phase 1: primary visibility on every device
    for (DeviceState& d : c->dev)
    {
        HIPCHK(c, hipSetDevice(d.device_id));
        const FrameK k = frame_k(d);
        const TileMap tm = tile_map(d);
        if (count)
        {
            if (d.ring_head > 0 && !d.ring_counts) { int rc = hrt_synchronize(c, nullptr); if (rc != HRT_OK) return rc; HIPCHK(c, hipSetDevice(d.device_id)); }
            if (!d.ring_counts) HIPCHK(c, hipMemsetAsync(d.counters, 0, 20 * sizeof(unsigned long long), d.stream));
            d.ring_counts = true;
        }
        hipEvent_t* ev = d.ev[d.ring_head];
        HIPCHK(c, hipEventRecord(ev[0], d.stream));
        if (tm.nTiles > 0 && !(flags & HRT_FLAG_SKIP_PRIMARY) && !cont)
        {
            const dim3 grid(tm.nTiles), block(64 * tm.wpb);
            int rcs = with_tracer(d, [&](auto tr) -> int {
                using TR = decltype(tr);
                bool second = false;
                if constexpr (std::is_same<TR, TracerPackedT<0>>::value) second = !count && d.any_ok;
                if (second)
                {
                    if constexpr (std::is_same<TR, TracerPackedT<0>>::value)
                    {
                        TracerSecond t2; t2.second = tr; t2.second.P = d.dpackedAny; t2.uploaded = tr;
                        hipLaunchKernelGGL((hrt_primary_kernel<TracerSecond, false>), grid, block, 0, d.stream, t2, k, d.gb, tm, d.counters);
                    }
                }
                else if (count) hipLaunchKernelGGL((hrt_primary_kernel<TR, true>), grid, block, 0, d.stream, tr, k, d.gb, tm, d.counters);
                else            hipLaunchKernelGGL((hrt_primary_kernel<TR, false>), grid, block, 0, d.stream, tr, k, d.gb, tm, d.counters);
                HIPCHK(c, hipGetLastError());
                return HRT_OK;
            });
            if (rcs != HRT_OK) return rcs;
        }
        HIPCHK(c, hipEventRecord(ev[1], d.stream));
    }
    if (exchange && !cont)
    {   // SpatialCompatible reads objId / normalWS / worldPos of the CURRENT frame at other pixels (RTRay.cs:363-374)
        int rc = exchange_arrays(1, [&](DeviceState& src, DeviceState& dst) -> int {
            int r;
            if ((r = copy_strips(c, src, dst.gb.worldPos, (const hrt_float3*)src.gb.worldPos, W, hipMemcpyDeviceToDevice, dst.stream)) != HRT_OK) return r;
            if ((r = copy_strips(c, src, dst.gb.normalWS, (const hrt_float3*)src.gb.normalWS, W, hipMemcpyDeviceToDevice, dst.stream)) != HRT_OK) return r;
            return copy_strips(c, src, dst.gb.objId, (const int32_t*)src.gb.objId, W, hipMemcpyDeviceToDevice, dst.stream);
        });
        if (rc != HRT_OK) return rc;
    }

    // ---- phase 2: path trace + gather on every device
    for (DeviceState& d : c->dev)
    {
        HIPCHK(c, hipSetDevice(d.device_id));
        const FrameK k = frame_k(d);
        const TileMap tm = tile_map(d);
        DReservoir resPrev = even ? d.resB : d.resA;
        DReservoir resCur = even ? d.resA : d.resB;
        hipEvent_t* ev = d.ev[d.ring_head];
        int rcs = primaryOnly ? HRT_OK : with_tracer(d, [&](auto tr) -> int {
            return run_path_stage(c, d, tr, k, tm, p->width, resPrev, resCur, (long long)nPix, count, mega, (flags & HRT_FLAG_TREELETS) != 0,
                                  prog ? d.prog_carry : nullptr, prog ? progBegin : 0);
        });
        if (rcs != HRT_OK) return rcs;
        HIPCHK(c, hipEventRecord(ev[2], d.stream));
    }
    if (exchange && !primaryOnly)
    {   // next frame's resPrev must be complete on every device (temporal reprojection can land anywhere, RTRay.cs:339-360)
        int rc = exchange_arrays(2, [&](DeviceState& src, DeviceState& dst) -> int {
            const DReservoir& a = even ? src.resA : src.resB;
            const DReservoir& b = even ? dst.resA : dst.resB;
            int r;
            if ((r = copy_strips(c, src, b.L, (const hrt_float3*)a.L, W, hipMemcpyDeviceToDevice, dst.stream)) != HRT_OK) return r;
            if ((r = copy_strips(c, src, b.wi, (const hrt_float3*)a.wi, W, hipMemcpyDeviceToDevice, dst.stream)) != HRT_OK) return r;
            if ((r = copy_strips(c, src, b.pdf, (const float*)a.pdf, W, hipMemcpyDeviceToDevice, dst.stream)) != HRT_OK) return r;
            if ((r = copy_strips(c, src, b.w, (const float*)a.w, W, hipMemcpyDeviceToDevice, dst.stream)) != HRT_OK) return r;
            if ((r = copy_strips(c, src, b.wSum, (const float*)a.wSum, W, hipMemcpyDeviceToDevice, dst.stream)) != HRT_OK) return r;
            if ((r = copy_strips(c, src, b.m, (const int32_t*)a.m, W, hipMemcpyDeviceToDevice, dst.stream)) != HRT_OK) return r;
            return copy_strips(c, src, b.lightId, (const int32_t*)a.lightId, W, hipMemcpyDeviceToDevice, dst.stream);
        });
        if (rc != HRT_OK) return rc;
    }
    // ---- phase 3: per-tile gather into the caller's host framebuffer.  Each device's copies are issued by its own host
    // thread when the ctx spans several devices: a copy into pageable memory blocks its issuing thread, so one thread
    // would serialise the N gathers.  Into page-locked memory (hrt_host_register) the copies are asynchronous DMA anyway.
    auto gather_device = [&](DeviceState& d, hrt_ctx* ec) -> int {
        HIPCHK(ec, hipSetDevice(d.device_id));
        DReservoir resCur = even ? d.resA : d.resB;
        hipEvent_t* ev = d.ev[d.ring_head];
        if (out)
        {
            int rc;
#define G(hostp, devp) if ((rc = gather_rows(ec, d, hostp, devp, W)) != HRT_OK) return rc
            G(out->color, d.fb.color); G(out->depth, d.fb.depth); G(out->objectId, d.fb.objectId);
            G(out->radiance, d.fb.radiance);
            G(out->gb_worldPos, d.gb.worldPos); G(out->gb_normalWS, d.gb.normalWS); G(out->gb_baseColor, d.gb.baseColor);
            G(out->gb_matId, d.gb.matId); G(out->gb_objId, d.gb.objId); G(out->gb_hitMask, d.gb.hitMask);
            G(out->res_L, resCur.L); G(out->res_wi, resCur.wi); G(out->res_pdf, resCur.pdf); G(out->res_w, resCur.w);
            G(out->res_wSum, resCur.wSum); G(out->res_m, resCur.m); G(out->res_lightId, resCur.lightId);
#undef G
            if (out->cameraId && d.row_begin == 0 && d.strip_i == 0 && d.n_strips > 0)
                HIPCHK(ec, hipMemcpyAsync(out->cameraId, d.fb.cameraId, 4, hipMemcpyDeviceToHost, d.stream));
        }
        HIPCHK(ec, hipEventRecord(ev[3], d.stream));
        return HRT_OK;
    };
    int grc = for_each_slot(c, out && nd > 1, who, "gather of ", [&](int i, hrt_ctx* ec) { return gather_device(c->dev[(size_t)i], ec); });
    if (grc != HRT_OK) return grc;
    for (DeviceState& d : c->dev) d.ring_head++;
    if (prog)
    {
        c->prog.valid = true; c->prog.p = *p;
        c->prog.rb = rb; c->prog.re = re; c->prog.sn = sn; c->prog.si = si; c->prog.pathFlags = flags & kPathFlags;
    }
    if (nosync) { if (stats) std::memset(stats, 0, sizeof(*stats)); return HRT_OK; }
    return hrt_synchronize(c, stats);
}

int hrt_render_frame(hrt_ctx* c, const hrt_frame_params* p, const hrt_render_opts* opts, const hrt_outputs* out, hrt_stats* stats)
try {
    if (!c) return HRT_ERR_INVALID_ARG;
    return render_impl(c, p, opts, out, stats, "hrt_render_frame", -1);
}
catch (...) { return on_exception(c, "hrt_render_frame"); }

int hrt_render_progressive(hrt_ctx* c, const hrt_frame_params* p, const hrt_render_opts* opts, int32_t sample_begin, const hrt_outputs* out, hrt_stats* stats)
try {
    if (!c) return HRT_ERR_INVALID_ARG;
    if (sample_begin < 0) return fail(c, HRT_ERR_INVALID_ARG, "hrt_render_progressive: sample_begin must be >= 0");
    return render_impl(c, p, opts, out, stats, "hrt_render_progressive", sample_begin);
}
catch (...) { return on_exception(c, "hrt_render_progressive"); }

// the camera as the reprojection kernels take it: tan(0.5 * fovY) evaluated once, here (hrt_tan is bit-equal on host and device)
static ProjCam proj_cam(const hrt_camera& cam)
{
    ProjCam q;
    q.origin = cam.origin; q.right = cam.right; q.up = cam.up; q.forward = cam.forward;
    q.tanHalfFov = hrt_tan(0.5f * cam.fovYRadians); q.aspect = cam.aspect;
    return q;
}

int hrt_present(hrt_ctx* c, const hrt_present_params* pp, int32_t* out_color_host)
try {
    if (!c) return HRT_ERR_INVALID_ARG;
    if (!pp) return fail(c, HRT_ERR_INVALID_ARG, "hrt_present: params is NULL");
    if (pp->out_width <= 0 || pp->out_height <= 0 || (int64_t)pp->out_width * pp->out_height > 0x7FFFFFFFLL)
        return fail(c, HRT_ERR_INVALID_ARG, "hrt_present: output size must be positive");
    const bool denoised = (pp->mode & HRT_PRESENT_DENOISED) != 0;
    const int mode = pp->mode & ~HRT_PRESENT_DENOISED;
    if (mode != HRT_PRESENT_RESAMPLE && mode != HRT_PRESENT_TAAU && mode != HRT_PRESENT_TAAU_REPROJECT)
        return fail(c, HRT_ERR_INVALID_ARG, "hrt_present: unknown mode");
    const bool reproject = mode == HRT_PRESENT_TAAU_REPROJECT;
    const int nd = (int)c->dev.size();
    DeviceState& d = c->dev[0];
    if (d.nPix == 0 || c->width <= 0) return fail(c, HRT_ERR_INVALID_STATE, "hrt_present: no frame rendered yet");
    if (d.strip_n != nd || d.row_begin != 0 || d.row_end != c->height) return fail(c, HRT_ERR_INVALID_STATE, "hrt_present: the last frame was a partial tile");
    if (denoised && (!d.dn_color || c->dn_serial != c->frame_serial || d.dn_pix != d.nPix))
        return fail(c, HRT_ERR_INVALID_STATE, "hrt_present: HRT_PRESENT_DENOISED, but the denoised colour does not belong to the last frame "
                    "(call hrt_denoise after the frame, scene upload or resize)");
    const int32_t* lowColor = denoised ? d.dn_color : d.fb.color;      // the one thing the flag changes
    int rc = hrt_synchronize(c, nullptr);
    if (rc != HRT_OK) return rc;
    HIPCHK(c, hipSetDevice(d.device_id));
    for (int i = 1; i < nd; i++)
    {   // the resolve runs on device slot 0: bring the other devices' strips of colour and objectId over
        DeviceState& srcd = c->dev[i];
        if ((rc = copy_strips(c, srcd, d.fb.color, (const int32_t*)srcd.fb.color, c->width, hipMemcpyDeviceToDevice, d.stream)) != HRT_OK) return rc;
        if ((rc = copy_strips(c, srcd, d.fb.objectId, (const int32_t*)srcd.fb.objectId, c->width, hipMemcpyDeviceToDevice, d.stream)) != HRT_OK) return rc;
        if (reproject && (rc = copy_strips(c, srcd, d.gb.worldPos, (const hrt_float3*)srcd.gb.worldPos, c->width, hipMemcpyDeviceToDevice, d.stream)) != HRT_OK) return rc;
    }
    HIPCHK(c, hipSetDevice(d.device_id));
    const int outW = pp->out_width, outH = pp->out_height, inW = c->width, inH = c->height;
    const size_t outLen = (size_t)outW * outH;
    if (d.present_w != outW || d.present_h != outH)
    {   // RTTaa.Ensure (RTTaa.cs:34-47): new display size -> new history, invalid until written once
        free_present(d);
        HIPCHK(c, dalloc(d.present_color, (int64_t)outLen, d.stream));
        HIPCHK(c, dalloc(d.taa_hist_color, (int64_t)outLen, d.stream));
        HIPCHK(c, dalloc(d.taa_hist_obj, (int64_t)outLen, d.stream));
        d.present_w = outW; d.present_h = outH; d.taa_history_valid = false;
    }
    const int blocks = (int)((outLen + 255) / 256);
    HIPCHK(c, hipEventRecord(d.q_ev[0], d.stream));
    if (mode == HRT_PRESENT_TAAU || reproject)
    {
        TaaK k;
        k.outColor = d.present_color; k.inColorLow = lowColor; k.inObjIdLow = d.fb.objectId;
        k.historyColor = d.taa_hist_color; k.historyObjId = d.taa_hist_obj;
        k.outW = outW; k.outH = outH; k.inW = inW; k.inH = inH;
        k.feedback = pp->feedback <= 0.f ? 0.075f : pp->feedback;          // tunables of RTTaa.cs:77-79; "<= 0 selects the default" as the
        k.sharpness = pp->sharpness <= 0.f ? 0.10f : pp->sharpness;        // header says: a NaN is not <= 0 and goes through to the kernel,
        k.clampK = pp->clampK <= 0.f ? 1.25f : pp->clampK;                 // as a NaN written to the reference's public fields would
        k.isFirstFrame = d.taa_history_valid ? 0 : 1;
        if (!reproject)
            hipLaunchKernelGGL(hrt_taa_resolve_kernel, dim3(std::min(blocks, 256 * 16)), dim3(256), 0, d.stream, k);
        else
        {   // reads the current history pair at reprojected positions, writes the spare pair at the pixel's own: swapped afterwards
            if (!d.taa_spare_color) HIPCHK(c, dalloc(d.taa_spare_color, (int64_t)outLen, d.stream));
            if (!d.taa_spare_obj) HIPCHK(c, dalloc(d.taa_spare_obj, (int64_t)outLen, d.stream));
            TaaReprojK r;
            r.worldPos = d.gb.worldPos; r.prevColor = d.taa_hist_color; r.prevObjId = d.taa_hist_obj;
            k.historyColor = d.taa_spare_color; k.historyObjId = d.taa_spare_obj;
            r.curCam = proj_cam(c->frame_cam);
            r.histCam = proj_cam(d.taa_history_valid ? d.taa_hist_cam : c->frame_cam);      // no history: every pixel resets
            hipLaunchKernelGGL(hrt_taa_resolve_reproject_kernel, dim3(std::min(blocks, 256 * 16)), dim3(256), 0, d.stream, k, r);
            std::swap(d.taa_hist_color, d.taa_spare_color); std::swap(d.taa_hist_obj, d.taa_spare_obj);
        }
        d.taa_history_valid = true; d.taa_hist_cam = c->frame_cam;     // the camera the history now belongs to
    }
    else if (inW == outW && inH == outH)
        hipLaunchKernelGGL(hrt_blit_kernel, dim3(blocks), dim3(256), 0, d.stream, lowColor, (long long)d.nPix, d.present_color, (long long)outLen);
    else
        hipLaunchKernelGGL(hrt_bilinear_upsample_kernel, dim3(blocks), dim3(256), 0, d.stream, lowColor, inW, inH, d.present_color, outW, outH);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(d.q_ev[1], d.stream));
    if (out_color_host) HIPCHK(c, hipMemcpyAsync(out_color_host, d.present_color, outLen * 4, hipMemcpyDeviceToHost, d.stream));
    HIPCHK(c, hipStreamSynchronize(d.stream));
    HIPCHK(c, hipEventElapsedTime(&d.present_ms, d.q_ev[0], d.q_ev[1]));
    return HRT_OK;
}
catch (...) { return on_exception(c, "hrt_present"); }

int hrt_present_time(hrt_ctx* c, float* ms)
try {
    if (!c || !ms) return HRT_ERR_INVALID_ARG;
    *ms = c->dev[0].present_ms;
    return HRT_OK;
}
catch (...) { return on_exception(c, "hrt_present_time"); }

int hrt_motion_vectors(hrt_ctx* c, const hrt_camera* from_cam, hrt_float2* mv, int32_t dev, float* device_ms)
try {
    if (!c) return HRT_ERR_INVALID_ARG;
    if (device_ms) *device_ms = 0.f;
    if (!mv) return fail(c, HRT_ERR_INVALID_ARG, "hrt_motion_vectors: mv is NULL");
    if (dev > 0) return fail(c, HRT_ERR_INVALID_ARG, "hrt_motion_vectors: dev must be 0 (device memory of slot 0) or negative (host memory)");
    const int nd = (int)c->dev.size();
    DeviceState& d0 = c->dev[0];
    if (d0.nPix == 0 || c->width <= 0) return fail(c, HRT_ERR_INVALID_STATE, "hrt_motion_vectors: no frame rendered yet");
    if (d0.strip_n != nd || d0.row_begin != 0 || d0.row_end != c->height) return fail(c, HRT_ERR_INVALID_STATE, "hrt_motion_vectors: the last frame was a partial tile");
    const int W = c->width, Hh = c->height;
    const size_t bytes = (size_t)d0.nPix * sizeof(hrt_float2);
    if (dev == 0)
    {
        HIPCHK(c, hipSetDevice(d0.device_id));
        if (!on_device(d0, mv, bytes)) return fail(c, HRT_ERR_INVALID_ARG, "hrt_motion_vectors: with dev == 0, mv must be device memory of slot 0's device, large enough for the frame");
        if ((uintptr_t)mv & 7) return fail(c, HRT_ERR_INVALID_ARG, "hrt_motion_vectors: device mv must be 8-byte aligned");
    }
    else if (in_device_memory(mv)) return fail(c, HRT_ERR_INVALID_ARG, "hrt_motion_vectors: with dev < 0, mv must be host memory (pass 0 for device memory of slot 0)");
    int rc = hrt_synchronize(c, nullptr);
    if (rc != HRT_OK) return rc;
    const ProjCam from = proj_cam(from_cam ? *from_cam : c->frame_prev_cam), cur = proj_cam(c->frame_cam);
    auto launch = [&](DeviceState& d, hrt_float2* out, int stripN, int stripI, int nRows) -> int {
        HIPCHK(c, hipEventRecord(d.q_ev[0], d.stream));
        const long long lanes = (long long)nRows * W;
        if (lanes > 0)
            hipLaunchKernelGGL(hrt_motion_vectors_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, d.stream,
                               (const hrt_float3*)d.gb.worldPos, from, cur, W, Hh, 0, Hh, stripN, stripI, nRows, out);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipEventRecord(d.q_ev[1], d.stream));
        return HRT_OK;
    };
    auto elapsed = [&](DeviceState& d, float& best) -> int {
        HIPCHK(c, hipSetDevice(d.device_id));
        HIPCHK(c, hipStreamSynchronize(d.stream));
        float t = 0.f;
        HIPCHK(c, hipEventElapsedTime(&t, d.q_ev[0], d.q_ev[1]));
        best = std::max(best, t);
        return HRT_OK;
    };
    float ms = 0.f;
    if (dev == 0)
    {   // everything on slot 0: bring the other slots' strips of gb_worldPos over, as hrt_present brings colour
        for (int i = 1; i < nd; i++)
            if ((rc = copy_strips(c, c->dev[(size_t)i], d0.gb.worldPos, (const hrt_float3*)c->dev[(size_t)i].gb.worldPos, W, hipMemcpyDeviceToDevice, d0.stream)) != HRT_OK) return rc;
        if ((rc = launch(d0, mv, 1, 0, Hh)) != HRT_OK) return rc;
        if ((rc = elapsed(d0, ms)) != HRT_OK) return rc;
    }
    else
    {   // every slot computes the strips it rendered; gathered into the host array like a frame output
        for (DeviceState& d : c->dev)
        {
            HIPCHK(c, hipSetDevice(d.device_id));
            if ((rc = d.mv_mem.grow(c, bytes, d.stream)) != HRT_OK) return rc;
            if ((rc = launch(d, (hrt_float2*)d.mv_mem.p, d.strip_n, d.strip_i, d.n_strips * 8)) != HRT_OK) return rc;      // a ragged last strip: the kernel's row test
            if ((rc = gather_rows(c, d, mv, (const hrt_float2*)d.mv_mem.p, W)) != HRT_OK) return rc;
        }
        for (DeviceState& d : c->dev) if ((rc = elapsed(d, ms)) != HRT_OK) return rc;
    }
    if (device_ms) *device_ms = ms;
    return HRT_OK;
}
catch (...) { return on_exception(c, "hrt_motion_vectors"); }

namespace {

// what both denoisers do before their kernels: the frame checks, then everything on slot 0 (the other slots' strips of what the
// filters read are brought over, as hrt_present brings colour) and the workspace with the two result planes
int denoise_frame_check(hrt_ctx* c, const char* who)
{
    const int nd = (int)c->dev.size();
    DeviceState& d = c->dev[0];
    if (d.nPix == 0 || c->width <= 0) return fail(c, HRT_ERR_INVALID_STATE, std::string(who) + ": no frame rendered yet");
    if (d.strip_n != nd || d.row_begin != 0 || d.row_end != c->height) return fail(c, HRT_ERR_INVALID_STATE, std::string(who) + ": the last frame was a partial tile");
    return HRT_OK;
}

int denoise_gather(hrt_ctx* c)
{
    const int nd = (int)c->dev.size();
    DeviceState& d = c->dev[0];
    int rc = hrt_synchronize(c, nullptr);
    if (rc != HRT_OK) return rc;
    HIPCHK(c, hipSetDevice(d.device_id));
    const int W = c->width;
    for (int i = 1; i < nd; i++)
    {
        DeviceState& srcd = c->dev[(size_t)i];
        if ((rc = copy_strips(c, srcd, d.fb.radiance, (const hrt_float3*)srcd.fb.radiance, W, hipMemcpyDeviceToDevice, d.stream)) != HRT_OK) return rc;
        if ((rc = copy_strips(c, srcd, d.gb.normalWS, (const hrt_float3*)srcd.gb.normalWS, W, hipMemcpyDeviceToDevice, d.stream)) != HRT_OK) return rc;
        if ((rc = copy_strips(c, srcd, d.gb.worldPos, (const hrt_float3*)srcd.gb.worldPos, W, hipMemcpyDeviceToDevice, d.stream)) != HRT_OK) return rc;
        if ((rc = copy_strips(c, srcd, d.gb.baseColor, (const hrt_float3*)srcd.gb.baseColor, W, hipMemcpyDeviceToDevice, d.stream)) != HRT_OK) return rc;
        if ((rc = copy_strips(c, srcd, d.fb.depth, (const float*)srcd.fb.depth, W, hipMemcpyDeviceToDevice, d.stream)) != HRT_OK) return rc;
        if ((rc = copy_strips(c, srcd, d.gb.hitMask, (const int32_t*)srcd.gb.hitMask, W, hipMemcpyDeviceToDevice, d.stream)) != HRT_OK) return rc;
    }
    HIPCHK(c, hipSetDevice(d.device_id));
    const size_t nPix = (size_t)d.nPix;
    if (d.dn_pix != d.nPix)
    {   // a new frame size: new planes (the old pointers of hrt_denoised_buffers end here)
        HIPCHK(c, hipStreamSynchronize(d.stream));
        d.dn_mem.release(); d.dn_pix = 0; d.dn_radiance = nullptr; d.dn_color = nullptr; c->dn_serial = 0;
        if ((rc = d.dn_mem.grow(c, nPix * 80, d.stream)) != HRT_OK) return rc;
        d.dn_pix = d.nPix;
        d.dn_radiance = (hrt_float3*)((char*)d.dn_mem.p + nPix * 64);
        d.dn_color = (int32_t*)((char*)d.dn_mem.p + nPix * 76);
    }
    return HRT_OK;
}

// after the kernels were enqueued between q_ev[0] and q_ev[1]: the host copies, the wait and the time
int denoise_finish(hrt_ctx* c, hrt_float3* out_radiance_host, int32_t* out_color_host, float* device_ms)
{
    DeviceState& d = c->dev[0];
    const size_t nPix = (size_t)d.nPix;
    if (out_radiance_host) HIPCHK(c, hipMemcpyAsync(out_radiance_host, d.dn_radiance, nPix * sizeof(hrt_float3), hipMemcpyDeviceToHost, d.stream));
    if (out_color_host) HIPCHK(c, hipMemcpyAsync(out_color_host, d.dn_color, nPix * 4, hipMemcpyDeviceToHost, d.stream));
    HIPCHK(c, hipStreamSynchronize(d.stream));
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, d.q_ev[0], d.q_ev[1]));
    if (device_ms) *device_ms = ms;
    c->dn_serial = c->frame_serial;
    return HRT_OK;
}

} // namespace

int hrt_denoise(hrt_ctx* c, const hrt_denoise_params* dp, hrt_float3* out_radiance_host, int32_t* out_color_host, float* device_ms)
try {
    if (!c) return HRT_ERR_INVALID_ARG;
    if (device_ms) *device_ms = 0.f;
    if (!dp) return fail(c, HRT_ERR_INVALID_ARG, "hrt_denoise: params is NULL");
    if (dp->iterations < 0 || dp->iterations > 8) return fail(c, HRT_ERR_INVALID_ARG, "hrt_denoise: iterations must be 1..8 (0 selects 5)");
    if (dp->flags & ~(uint32_t)HRT_DENOISE_NO_DEMODULATE) return fail(c, HRT_ERR_INVALID_ARG, "hrt_denoise: unknown flag bit");
    int rc = denoise_frame_check(c, "hrt_denoise");
    if (rc != HRT_OK) return rc;
    if ((rc = denoise_gather(c)) != HRT_OK) return rc;
    DeviceState& d = c->dev[0];
    const size_t nPix = (size_t)d.nPix;
    DenoiseLaunch L;
    L.width = c->width; L.height = c->height;
    L.iterations = dp->iterations == 0 ? 5 : dp->iterations;
    L.demodulate = (dp->flags & HRT_DENOISE_NO_DEMODULATE) == 0;
    const float sn = dp->sigma_normal <= 0.f ? 0.5f : dp->sigma_normal, sp = dp->sigma_plane <= 0.f ? 0.02f : dp->sigma_plane;     // "<= 0 selects the
    L.sigma_color = dp->sigma_color <= 0.f ? 4.0f : dp->sigma_color;                                                              // default": a NaN goes through
    L.kn = 1.0f / (sn * sn); L.sp2 = sp * sp;
    L.radiance = d.fb.radiance; L.normalWS = d.gb.normalWS; L.worldPos = d.gb.worldPos; L.baseColor = d.gb.baseColor;
    L.depth = d.fb.depth; L.hitMask = d.gb.hitMask;
    L.guide = (float4*)d.dn_mem.p;
    L.colour[0] = (float4*)((char*)d.dn_mem.p + nPix * 32); L.colour[1] = (float4*)((char*)d.dn_mem.p + nPix * 48);
    L.outRadiance = d.dn_radiance; L.outColor = d.dn_color;
    c->dn_serial = 0;                          // until the kernels are enqueued
    HIPCHK(c, hipEventRecord(d.q_ev[0], d.stream));
    HIPCHK(c, denoise_launch(L, d.stream));
    HIPCHK(c, hipEventRecord(d.q_ev[1], d.stream));
    return denoise_finish(c, out_radiance_host, out_color_host, device_ms);
}
catch (...) { return on_exception(c, "hrt_denoise"); }

int hrt_denoise_temporal(hrt_ctx* c, const hrt_denoise_temporal_params* tp, hrt_float3* out_radiance_host, int32_t* out_color_host, float* device_ms)
try {
    if (!c) return HRT_ERR_INVALID_ARG;
    if (device_ms) *device_ms = 0.f;
    if (!tp) return fail(c, HRT_ERR_INVALID_ARG, "hrt_denoise_temporal: params is NULL");
    if (tp->iterations < 0 || tp->iterations > 8) return fail(c, HRT_ERR_INVALID_ARG, "hrt_denoise_temporal: iterations must be 1..8 (0 selects 5)");
    if (tp->flags & ~(uint32_t)(HRT_DENOISE_T_NO_DEMODULATE | HRT_DENOISE_T_NO_SPATIAL | HRT_DENOISE_T_RESET))
        return fail(c, HRT_ERR_INVALID_ARG, "hrt_denoise_temporal: unknown flag bit");
    int rc = denoise_frame_check(c, "hrt_denoise_temporal");
    if (rc != HRT_OK) return rc;
    if (c->dt_serial == c->frame_serial)
        return fail(c, HRT_ERR_INVALID_STATE, "hrt_denoise_temporal: this frame has already been accumulated into the history (one call per frame)");
    if ((rc = denoise_gather(c)) != HRT_OK) return rc;
    DeviceState& d = c->dev[0];
    const size_t nPix = (size_t)d.nPix;
    const int W = c->width, Hh = c->height;
    if (d.dt_w != W || d.dt_h != Hh)
    {   // a new frame size: a new, empty history
        HIPCHK(c, hipStreamSynchronize(d.stream));
        d.dt_mem.release(); d.dt_w = d.dt_h = 0; d.dt_valid = false;
        if ((rc = d.dt_mem.grow(c, nPix * 128, d.stream)) != HRT_OK) return rc;
        d.dt_w = W; d.dt_h = Hh; d.dt_cur = 0;
    }
    if (tp->flags & HRT_DENOISE_T_RESET) d.dt_valid = false;
    const int prev = d.dt_cur, cur = prev ^ 1;
    char* base = (char*)d.dt_mem.p;
    auto guide = [&](int k) { return (float4*)(base + nPix * 32 * (size_t)k); };
    auto hcol = [&](int k) { return (float4*)(base + nPix * 64 + nPix * 16 * (size_t)k); };
    auto hmom = [&](int k) { return (float4*)(base + nPix * 96 + nPix * 16 * (size_t)k); };
    DenoiseTemporalLaunch L;
    L.width = W; L.height = Hh;
    L.iterations = tp->iterations == 0 ? 5 : tp->iterations;
    L.demodulate = (tp->flags & HRT_DENOISE_T_NO_DEMODULATE) == 0;
    L.spatial = (tp->flags & HRT_DENOISE_T_NO_SPATIAL) == 0;
    L.haveHistory = d.dt_valid;
    const float sn = tp->sigma_normal <= 0.f ? 0.5f : tp->sigma_normal, sp = tp->sigma_plane <= 0.f ? 0.02f : tp->sigma_plane;     // "<= 0 selects the
    L.sigma_lum = tp->sigma_lum <= 0.f ? 0.7f : tp->sigma_lum;                                                                    // default": a NaN goes through
    L.kn = 1.0f / (sn * sn); L.sp2 = sp * sp;
    const float ac = tp->alpha_color <= 0.f ? 0.2f : tp->alpha_color, am = tp->alpha_moments <= 0.f ? 0.2f : tp->alpha_moments;
    L.alpha_color = ac > 1.0f ? 1.0f : ac; L.alpha_moments = am > 1.0f ? 1.0f : am;
    L.normal_cos_min = tp->normal_cos_min <= 0.f ? 0.9f : tp->normal_cos_min;
    L.plane_tol = tp->plane_tol <= 0.f ? 0.02f : tp->plane_tol;
    L.max_history = (float)(tp->max_history <= 0 ? 64 : tp->max_history);
    L.curCam = proj_cam(c->frame_cam);
    L.histCam = proj_cam(d.dt_valid ? d.dt_cam : c->frame_cam);
    L.radiance = d.fb.radiance; L.normalWS = d.gb.normalWS; L.worldPos = d.gb.worldPos; L.baseColor = d.gb.baseColor;
    L.depth = d.fb.depth; L.hitMask = d.gb.hitMask;
    L.guideCur = guide(cur); L.guidePrev = guide(prev);
    L.hcolPrev = hcol(prev); L.hmomPrev = hmom(prev); L.hcolNew = hcol(cur); L.hmomNew = hmom(cur);
    L.work[0] = (float4*)((char*)d.dn_mem.p + nPix * 32); L.work[1] = (float4*)((char*)d.dn_mem.p + nPix * 48);
    L.outRadiance = d.dn_radiance; L.outColor = d.dn_color;
    c->dn_serial = 0;                          // until the kernels are enqueued
    d.dt_valid = false;                        // ... and the history is whole again
    HIPCHK(c, hipEventRecord(d.q_ev[0], d.stream));
    HIPCHK(c, denoise_temporal_launch(L, d.stream));
    HIPCHK(c, hipEventRecord(d.q_ev[1], d.stream));
    if ((rc = denoise_finish(c, out_radiance_host, out_color_host, device_ms)) != HRT_OK) return rc;
    d.dt_cur = cur; d.dt_valid = true; d.dt_cam = c->frame_cam;
    c->dt_serial = c->frame_serial;
    return HRT_OK;
}
catch (...) { return on_exception(c, "hrt_denoise_temporal"); }

int hrt_denoise_history(hrt_ctx* c, hrt_denoise_history_views* out)
try {
    if (!c || !out) return HRT_ERR_INVALID_ARG;
    std::memset(out, 0, sizeof(*out));
    const DeviceState& d = c->dev[0];
    if (!d.dt_valid) return HRT_OK;
    const size_t nPix = (size_t)d.dt_w * (size_t)d.dt_h;
    const char* base = (const char*)d.dt_mem.p;
    out->color = (const float*)(base + nPix * 64 + nPix * 16 * (size_t)d.dt_cur);
    out->moments = (const float*)(base + nPix * 96 + nPix * 16 * (size_t)d.dt_cur);
    out->length = out->moments + 2; out->variance = out->color + 3;
    out->width = d.dt_w; out->height = d.dt_h; out->stride = 4;
    return HRT_OK;
}
catch (...) { return on_exception(c, "hrt_denoise_history"); }

int hrt_denoise_history_read(hrt_ctx* c, float* color_host, float* moments_host)
try {
    if (!c) return HRT_ERR_INVALID_ARG;
    DeviceState& d = c->dev[0];
    if (!d.dt_valid) return fail(c, HRT_ERR_INVALID_STATE, "hrt_denoise_history_read: the history is empty");
    const size_t bytes = (size_t)d.dt_w * (size_t)d.dt_h * 16;
    const char* base = (const char*)d.dt_mem.p;
    HIPCHK(c, hipSetDevice(d.device_id));
    if (color_host) HIPCHK(c, hipMemcpyAsync(color_host, base + bytes * 4 + bytes * (size_t)d.dt_cur, bytes, hipMemcpyDeviceToHost, d.stream));
    if (moments_host) HIPCHK(c, hipMemcpyAsync(moments_host, base + bytes * 6 + bytes * (size_t)d.dt_cur, bytes, hipMemcpyDeviceToHost, d.stream));
    HIPCHK(c, hipStreamSynchronize(d.stream));
    return HRT_OK;
}
catch (...) { return on_exception(c, "hrt_denoise_history_read"); }

int hrt_denoised_buffers(hrt_ctx* c, void** radiance, void** color)
try {
    if (!c) return HRT_ERR_INVALID_ARG;
    if (radiance) *radiance = c->dev[0].dn_radiance;
    if (color) *color = c->dev[0].dn_color;
    return HRT_OK;
}
catch (...) { return on_exception(c, "hrt_denoised_buffers"); }

int hrt_set_workspace_limit(hrt_ctx* c, int64_t max_resident_paths)
try {
    if (!c) return HRT_ERR_INVALID_ARG;
    if (max_resident_paths < 0) return fail(c, HRT_ERR_INVALID_ARG, "hrt_set_workspace_limit: the limit must be >= 0 (0 = default)");
    c->max_resident_paths = max_resident_paths;
    return HRT_OK;
}
catch (...) { return on_exception(c, "hrt_set_workspace_limit"); }

int hrt_host_register(hrt_ctx* c, void* ptr, int64_t bytes)
try {
    if (!c) return HRT_ERR_INVALID_ARG;
    if (!ptr || bytes <= 0) return fail(c, HRT_ERR_INVALID_ARG, "hrt_host_register: needs a pointer and a positive size");
    for (const auto& r : c->pinned) if (r.first == (char*)ptr) return fail(c, HRT_ERR_INVALID_STATE, "hrt_host_register: this range is registered already");
    HIPCHK(c, hipSetDevice(c->dev[0].device_id));
    HIPCHK(c, hipHostRegister(ptr, (size_t)bytes, hipHostRegisterPortable));
    c->pinned.emplace_back((char*)ptr, (size_t)bytes);
    return HRT_OK;
}
catch (...) { return on_exception(c, "hrt_host_register"); }

int hrt_host_unregister(hrt_ctx* c, void* ptr)
try {
    if (!c) return HRT_ERR_INVALID_ARG;
    for (size_t i = 0; i < c->pinned.size(); i++)
        if (c->pinned[i].first == (char*)ptr)
        {
            int rc = hrt_synchronize(c, nullptr);                 // no copy into the range may still be in flight
            if (rc != HRT_OK) return rc;
            c->pinned.erase(c->pinned.begin() + (long)i);
            HIPCHK(c, hipHostUnregister(ptr));
            return HRT_OK;
        }
    return fail(c, HRT_ERR_INVALID_ARG, "hrt_host_unregister: range was not registered through this context");
}
catch (...) { return on_exception(c, "hrt_host_unregister"); }

int hrt_frame_times(hrt_ctx* c, int dev, int launch, float* ms, int cap, int* n)
try {
    if (!c) return HRT_ERR_INVALID_ARG;
    if (dev < 0 || dev >= (int)c->dev.size() || launch < 0 || launch > 1 || cap < 0) return fail(c, HRT_ERR_INVALID_ARG, "hrt_frame_times: device slot or launch out of range");
    const std::vector<float>& v = c->dev[(size_t)dev].frame_ms[launch];
    if (n) *n = (int)v.size();
    if (ms) for (int i = 0; i < cap && i < (int)v.size(); i++) ms[i] = v[(size_t)i];
    return HRT_OK;
}
catch (...) { return on_exception(c, "hrt_frame_times"); }

int hrt_device_buffers(hrt_ctx* c, int dev, hrt_device_views* o)
try {
    if (!c || !o) return HRT_ERR_INVALID_ARG;
    if (dev < 0 || dev >= (int)c->dev.size()) return fail(c, HRT_ERR_INVALID_ARG, "hrt_device_buffers: device slot out of range");
    DeviceState& d = c->dev[dev];
    if (d.nPix == 0) return fail(c, HRT_ERR_INVALID_STATE, "hrt_device_buffers: no frame rendered yet");
    o->row_begin = d.row_begin; o->row_end = d.row_end; o->strip_n = d.strip_n; o->strip_i = d.strip_i;
    o->width = c->width; o->height = c->height; o->device_id = d.device_id; o->reserved = 0;
    o->color = d.fb.color; o->depth = d.fb.depth; o->objectId = d.fb.objectId; o->radiance = d.fb.radiance;
    o->gb_worldPos = d.gb.worldPos; o->gb_normalWS = d.gb.normalWS; o->gb_baseColor = d.gb.baseColor;
    o->gb_matId = d.gb.matId; o->gb_objId = d.gb.objId; o->gb_hitMask = d.gb.hitMask;
    o->present_color = d.present_color; o->present_width = d.present_w; o->present_height = d.present_h;
    const DReservoir* rs[2] = {&d.resA, &d.resB};
    void** dst[2] = {o->res_a, o->res_b};
    for (int i = 0; i < 2; i++)
    {
        dst[i][0] = rs[i]->L; dst[i][1] = rs[i]->wi; dst[i][2] = rs[i]->pdf; dst[i][3] = rs[i]->w;
        dst[i][4] = rs[i]->wSum; dst[i][5] = rs[i]->m; dst[i][6] = rs[i]->lightId;
    }
    return HRT_OK;
}
catch (...) { return on_exception(c, "hrt_device_buffers"); }

int hrt_trace_rays(hrt_ctx* c, int32_t query, const hrt_ray* rays, int64_t n, void* results, int32_t dev, float* device_ms)
try {
    if (!c) return HRT_ERR_INVALID_ARG;
    if (device_ms) *device_ms = 0.f;
    if (query != HRT_QUERY_CLOSEST && query != HRT_QUERY_OCCLUDED) return fail(c, HRT_ERR_INVALID_ARG, "hrt_trace_rays: unknown query");
    const size_t resBytes = query == HRT_QUERY_CLOSEST ? sizeof(hrt_ray_hit) : sizeof(int32_t);
    const QueryArg args[2] = {{rays, sizeof(hrt_ray), 16, false}, {results, resBytes, 16, false}};
    const QueryDoor door{"hrt_trace_rays", "rays and results", "rays and results", "rays and results must be 16-byte aligned", false};
    return run_query(c, door, args, 2, n, dev, device_ms, [&](hrt_ctx* ec, DeviceState& d, int64_t begin, int64_t end, bool dev_ptrs, float* ms) {
        return query_slot(ec, *c, d, query, args, begin, end, dev_ptrs, ms);
    });
}
catch (...) { return on_exception(c, "hrt_trace_rays"); }

int hrt_trace_hits(hrt_ctx* c, const hrt_ray* rays, int64_t n, int32_t k, hrt_ray_hit* hits, int32_t* counts, int32_t* totals,
                   int32_t dev, float* device_ms)
try {
    if (!c) return HRT_ERR_INVALID_ARG;
    if (device_ms) *device_ms = 0.f;
    if (k < 1 || k > HRT_HITS_MAX) return fail(c, HRT_ERR_INVALID_ARG, "hrt_trace_hits: k must be in [1, HRT_HITS_MAX]");
    const QueryArg args[4] = {{rays, sizeof(hrt_ray), 16, false}, {hits, (size_t)k * sizeof(hrt_ray_hit), 16, false},
                              {counts, sizeof(int32_t), 4, false}, {totals, sizeof(int32_t), 4, true}};
    const QueryDoor door{"hrt_trace_hits", "rays, hits and counts", "rays, hits, counts and totals",
                         "rays and hits must be 16-byte aligned, counts and totals 4-byte aligned", false};
    return run_query(c, door, args, 4, n, dev, device_ms, [&](hrt_ctx* ec, DeviceState& d, int64_t begin, int64_t end, bool dev_ptrs, float* ms) {
        return hits_slot(ec, *c, d, k, args, begin, end, dev_ptrs, ms);
    });
}
catch (...) { return on_exception(c, "hrt_trace_hits"); }

// hrt_trace_paths: rays [begin, end) of one device slot, chunk by chunk (ChunkStager): primary kernel into the chunk's private G-buffer,
// fused path stage writing the result records.  A chunk is whole rows of width keys (at most kQueryChunk slots), or a segment of at
// most kQueryChunk columns of one row when a row is wider.  Its workspace is the sample groups' scratch, then the G-buffer planes
// (48 B per slot).
static int paths_slot(hrt_ctx* c, const hrt_ctx& cc, DeviceState& d, const hrt_frame_params& p, uint32_t flags, const QueryArg* args,
                      int64_t begin, int64_t end, int64_t first_key, bool dev_ptrs, float* ms)
{
    HIPCHK(c, hipSetDevice(d.device_id));
    ChunkStager s{c, cc, d, args, 2, dev_ptrs};
    const int64_t W = p.width, K1 = first_key + end;
    // the frame's tracer for the scene (render_impl, with the fused path stage): TracerFlat for tiny sphere scenes, the smallest packed
    // walker otherwise (its primary over the second tree where one describes the scene), TracerRef for REFERENCE_LAYOUT
    const bool usePacked = cc.packed_ok && !(flags & HRT_FLAG_REFERENCE_LAYOUT);
    const int variant = usePacked ? cc.packed_feat : -1;
    PathsLaunch L;
    L.variant = variant;
    L.flat = variant == 0 && cc.flat_leaves > 0;
    L.second = variant == 0 && !L.flat && d.any_ok;
    L.S = d.dscene; L.P = d.dpacked; L.PAny = d.dpackedAny;
    L.leaves = (const NodeQ*)d.packed[4]; L.nLeaves = cc.flat_leaves;
    for (int64_t c0 = first_key + begin; c0 < K1; )
    {
        int64_t R = c0 / W, rows, x0, xw;
        if (W <= kQueryChunk) { x0 = 0; xw = W; rows = std::min<int64_t>(kQueryChunk / W, (K1 + W - 1) / W - R); }
        else { x0 = (c0 - R * W) / kQueryChunk * kQueryChunk; xw = std::min<int64_t>(kQueryChunk, W - x0); rows = 1; }
        const int64_t c1 = std::min<int64_t>(K1, (R + rows - 1) * W + x0 + xw);
        const int64_t slots = rows * xw;
        L.k = frame_consts(&p);
        L.k.row_begin = (int)R; L.k.row_end = (int)(R + rows); L.k.height = L.k.row_end;
        TileMap& tm = L.tm;
        tm.wpb = 4;
        tm.tilesX = (int)((xw + 31) / 32);
        tm.tilesY = (int)((rows + 7) / 8);
        tm.nTiles = tm.tilesX * tm.tilesY;
        tm.band = !cc.small_scene;
        // sample groups as a fused frame of this many tiles forms them
        const int spp = p.spp > 1 ? p.spp : 1;
        const SampleGroups sg = sample_groups(spp, spp, p.maxDepth, (long long)tm.nTiles * tm.wpb, d.n_cu);
        const size_t splitBytes = sg.scratchFloats * (size_t)tm.nTiles * 256 * sizeof(float);
        int rc = s.begin(c0 - first_key, c1 - c0, splitBytes + (size_t)slots * 48);
        if (rc != HRT_OK) return rc;
        L.split = (float*)s.work; L.nGroups = sg.nGroups; L.perGroup = sg.perGroup;
        DGBuffer& gb = L.gb;
        gb.worldPos = (hrt_float3*)((char*)s.work + splitBytes); gb.normalWS = gb.worldPos + slots; gb.baseColor = gb.normalWS + slots;
        gb.matId = (int32_t*)(gb.baseColor + slots); gb.objId = gb.matId + slots; gb.hitMask = gb.objId + slots;
        PathsK& q = L.q;
        q.k0 = (int)c0; q.k1 = (int)c1; q.base = (int)(R * W + x0); q.x0 = (int)x0; q.xw = (int)xw;
        q.rays = (const hrt_ray*)s.dev[0]; q.out = (hrt_path_result*)s.dev[1];
        HIPCHK(c, paths_launch(L, d.stream));
        if ((rc = s.end(ms)) != HRT_OK) return rc;
        c0 = c1;
    }
    return HRT_OK;
}

int hrt_trace_paths(hrt_ctx* c, const hrt_frame_params* p, uint32_t flags, const hrt_ray* rays, int64_t n, int64_t first_key,
                    hrt_path_result* results, int32_t dev, float* device_ms)
try {
    if (!c) return HRT_ERR_INVALID_ARG;
    if (device_ms) *device_ms = 0.f;
    if (!p) return fail(c, HRT_ERR_INVALID_ARG, "hrt_trace_paths: params is NULL");
    constexpr uint32_t kPathFlags = HRT_FLAG_REFERENCE_LAYOUT | HRT_FLAG_MEGAKERNEL | HRT_FLAG_STREAMED | HRT_FLAG_TREELETS;
    if (flags & ~kPathFlags)
        return fail(c, HRT_ERR_INVALID_ARG, "hrt_trace_paths: only the path-selecting flags (REFERENCE_LAYOUT, MEGAKERNEL, STREAMED, TREELETS) apply to radiance queries");
    if (p->enableTemporalReuse != 0 || p->enableSpatialReuse != 0)
        return fail(c, HRT_ERR_INVALID_ARG, "hrt_trace_paths: ReSTIR reuse needs a frame's reservoirs: set enableTemporalReuse and enableSpatialReuse to 0");
    if (p->width <= 0) return fail(c, HRT_ERR_INVALID_ARG, "hrt_trace_paths: params->width must be positive");
    if (p->maxDepth < 0) return fail(c, HRT_ERR_INVALID_ARG, "hrt_trace_paths: maxDepth must be >= 0");
    if (n < 0) return fail(c, HRT_ERR_INVALID_ARG, "hrt_trace_paths: n must be >= 0");      // here too: the key range below is tested on a valid n
    if (first_key < 0) return fail(c, HRT_ERR_INVALID_ARG, "hrt_trace_paths: first_key must be >= 0");
    if (first_key > 0x7FFFFFFFLL - n) return fail(c, HRT_ERR_INVALID_ARG, "hrt_trace_paths: first_key + n exceeds 2^31 - 1 (keys are int pixel indices)");
    const QueryArg args[2] = {{rays, sizeof(hrt_ray), 16, false}, {results, sizeof(hrt_path_result), 16, false}};
    const QueryDoor door{"hrt_trace_paths", "rays and results", "rays and results", "rays and results must be 16-byte aligned", true};
    return run_query(c, door, args, 2, n, dev, device_ms, [&](hrt_ctx* ec, DeviceState& d, int64_t begin, int64_t end, bool dev_ptrs, float* ms) {
        return paths_slot(ec, *c, d, *p, flags, args, begin, end, first_key, dev_ptrs, ms);
    });
}
catch (...) { return on_exception(c, "hrt_trace_paths"); }

#ifdef HRT_TEST_HOOKS
// test hook: evaluate hrt_math.h function `fn` on device 0 of ctx (see hrt_math_probe_kernel)
int hrt_math_probe(hrt_ctx* c, int fn, int n, const float* x, const float* y, float* out)
try {
    if (!c || !x || !out || n <= 0) return HRT_ERR_INVALID_ARG;
    DeviceState& d = c->dev[0];
    HIPCHK(c, hipSetDevice(d.device_id));
    float *dx = nullptr, *dy = nullptr, *dout = nullptr;
    HIPCHK(c, hipMalloc((void**)&dx, (size_t)n * 4));
    HIPCHK(c, hipMalloc((void**)&dout, (size_t)n * 4));
    HIPCHK(c, hipMemcpy(dx, x, (size_t)n * 4, hipMemcpyHostToDevice));
    if (y) { HIPCHK(c, hipMalloc((void**)&dy, (size_t)n * 4)); HIPCHK(c, hipMemcpy(dy, y, (size_t)n * 4, hipMemcpyHostToDevice)); }
    hipLaunchKernelGGL(hrt_math_probe_kernel, dim3((n + 255) / 256), dim3(256), 0, d.stream, fn, n, dx, dy, dout);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(d.stream));
    HIPCHK(c, hipMemcpy(out, dout, (size_t)n * 4, hipMemcpyDeviceToHost));
    (void)hipFree(dx); (void)hipFree(dout); if (dy) (void)hipFree(dy);
    return HRT_OK;
}
catch (...) { return on_exception(c, "hrt_math_probe"); }

// test hook: compares a trimmed device function with its IEEE definition over EVERY float of its stated domain, on the device
// (which: 0 rsqrt_clamped, 1 sqrt_normal_range, 2 rcp_normal_range, 3 and 4 div_by); *mismatches = number of differing bit patterns, *first_bad = the smallest one
int hrt_math_exhaustive(hrt_ctx* c, int which, uint64_t* mismatches, uint32_t* first_bad)
try {
    if (!c || !mismatches || which < 0 || which > 4) return HRT_ERR_INVALID_ARG;
    DeviceState& d = c->dev[0];
    HIPCHK(c, hipSetDevice(d.device_id));
    unsigned long long* dm = nullptr;
    HIPCHK(c, hipMalloc((void**)&dm, 16));
    const unsigned long long init[2] = {0ull, 0xFFFFFFFFull};
    HIPCHK(c, hipMemcpy(dm, init, 16, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(hrt_math_exhaustive_kernel, dim3(4096), dim3(256), 0, d.stream, which, dm, (unsigned*)(dm + 1));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(d.stream));
    unsigned long long h[2];
    HIPCHK(c, hipMemcpy(h, dm, 16, hipMemcpyDeviceToHost));
    (void)hipFree(dm);
    *mismatches = h[0];
    if (first_bad) *first_bad = (uint32_t)h[1];
    return HRT_OK;
}
catch (...) { return on_exception(c, "hrt_math_exhaustive"); }
#endif // HRT_TEST_HOOKS

} // extern "C"

#ifdef HRT_TEST_HOOKS
// test hooks of the treelet cut (include/hrt_test_hooks.h)
extern "C" int hrt_debug_set_treelet_limits(int bytes, int min_nodes, int min_blas_nodes)
{
    TreeletLimits& lim = treelet_limits();
    lim = TreeletLimits{};
    if (bytes > 0) { lim.bytes = bytes; lim.minNodes = min_nodes; lim.minBlasNodes = min_blas_nodes; }
    if (min_blas_nodes < 0) lim.minBlasNodes = 0x7FFFFFFF;
    return 0;
}

extern "C" int hrt_debug_treelet_count(hrt_ctx* c)
{
    if (!c || c->dev.empty()) return 0;
    return c->dev[0].tl_ok ? c->dev[0].dtl.nTl : 0;
}

extern "C" int hrt_debug_treelets(const hrt_scene_desc* s, int bytes, int min_nodes, int min_blas_nodes,
                                  float* blas, float* red, int32_t* red_orig, int32_t* treelets, int32_t* red_of_root, int64_t* counts)
try {
    if (!s || !counts) return HRT_ERR_INVALID_ARG;
    PackedHost ph;
    if (!validate_and_pack(s, ph).empty()) return HRT_ERR_INVALID_ARG;
    TreeletLimits lim;
    if (bytes > 0) { lim.bytes = bytes; lim.minNodes = min_nodes; lim.minBlasNodes = min_blas_nodes; }
    TreeletsHost th;
    if (ph.ok && (ph.feat & 1) && ph.blas_refit_ok && !ph.meshRanges.empty()) build_treelets(ph.blas, ph.bsubend, ph.meshRanges, lim, th);
    counts[0] = (int64_t)ph.blas.size(); counts[1] = (int64_t)th.red.size(); counts[2] = (int64_t)th.tl.size();
    if (blas) std::memcpy(blas, ph.blas.data(), ph.blas.size() * sizeof(NodeQ));
    if (red && !th.red.empty()) std::memcpy(red, th.red.data(), th.red.size() * sizeof(NodeQ));
    if (red_orig && !th.redOrig.empty()) std::memcpy(red_orig, th.redOrig.data(), th.redOrig.size() * sizeof(int32_t));
    if (treelets && !th.tl.empty()) std::memcpy(treelets, th.tl.data(), th.tl.size() * sizeof(Treelet));
    if (red_of_root && !th.redOfRoot.empty()) std::memcpy(red_of_root, th.redOfRoot.data(), th.redOfRoot.size() * sizeof(int32_t));
    return HRT_OK;
}
catch (...) { return on_exception(nullptr, "hrt_debug_treelets"); }

// host-only test hook of the scene validator (include/hrt_test_hooks.h): the text hrt_scene_upload would fail with
extern "C" int hrt_debug_validate_scene(const hrt_scene_desc* s, char* msg, int cap)
try {
    if (!s) return HRT_ERR_INVALID_ARG;
    if (msg && cap > 0) msg[0] = 0;
    PackedHost ph;
    const std::string verr = validate_and_pack(s, ph);
    if (verr.empty()) return HRT_OK;
    if (msg && cap > 0) { std::strncpy(msg, verr.c_str(), (size_t)cap - 1); msg[cap - 1] = 0; }
    return HRT_ERR_INVALID_ARG;
}
catch (...) { return on_exception(nullptr, "hrt_debug_validate_scene"); }
#endif // HRT_TEST_HOOKS

#ifdef HRT_TL_STATS
// variant builds only (tools/tl_stats.py): read and clear the treelet walker's statistics of the current device
extern "C" int hrt_debug_tl_stats(unsigned long long* out256)
{
    if (hipMemcpyFromSymbol(out256, HIP_SYMBOL(g_tl_stats), sizeof(g_tl_stats)) != hipSuccess) return -1;
    static const unsigned long long zero[8][2][16] = {};
    return hipMemcpyToSymbol(HIP_SYMBOL(g_tl_stats), zero, sizeof(g_tl_stats)) == hipSuccess ? 0 : -1;
}
#endif

#ifdef HRT_PT_STATS
// variant builds only (tools/pt_stats.py): read and clear the fused kernel's section statistics of the current device
extern "C" int hrt_debug_pt_stats(unsigned long long* out64)
{
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(out64, HIP_SYMBOL(g_pt_stats), sizeof(unsigned long long) * 64) != hipSuccess) return -1;
    unsigned long long z[64] = {};
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_pt_stats), z, sizeof z) != hipSuccess) return -1;
    return 0;
}
#endif

#ifdef HRT_TEST_HOOKS
// ---- host-only test hooks of the second tree (include/hrt_test_hooks.h; the code is hrt_scene_pack.hip's)
extern "C" {

int hrt_debug_second_tree_topology(const hrt_instance* instances, int32_t n, int32_t* order, int32_t* link, int32_t* skip, int32_t* count,
                                   int32_t* parent, int32_t* n_nodes)
try {
    if (!instances || n < 1 || !order || !link || !skip || !count || !parent || !n_nodes) return HRT_ERR_INVALID_ARG;
    std::vector<hrt_instance> inst(instances, instances + n);
    SahTopology t;
    host_sah_topology(inst, t);
    *n_nodes = (int32_t)t.nodes.size();
    std::memcpy(order, t.order.data(), (size_t)n * 4);
    for (size_t i = 0; i < t.nodes.size(); i++)
    {
        const int lo = __builtin_bit_cast(int, t.nodes[i].lo.w), hi = __builtin_bit_cast(int, t.nodes[i].hi.w);
        link[i] = lo; skip[i] = hi & kEnd; count[i] = (int32_t)((unsigned)hi >> 28); parent[i] = t.parent[i];
    }
    return HRT_OK;
}
catch (...) { return on_exception(nullptr, "hrt_debug_second_tree_topology"); }

int hrt_debug_second_tree_reorder(const float* records, int32_t n_records, const int32_t* sign, int32_t base, int32_t inlined, float* out_records, int32_t* from)
try {
    if (!records || n_records < 1 || !sign || !out_records || !from) return HRT_ERR_INVALID_ARG;
    std::vector<NodeQ> X((size_t)n_records), out((size_t)n_records);
    std::memcpy(X.data(), records, (size_t)n_records * sizeof(NodeQ));
    const int sg[3] = {sign[0], sign[1], sign[2]};
    if (!reorder_second_tree(X, sg, base, out.data(), from, inlined != 0)) return HRT_ERR_INVALID_ARG;
    std::memcpy(out_records, out.data(), (size_t)n_records * sizeof(NodeQ));
    return HRT_OK;
}
catch (...) { return on_exception(nullptr, "hrt_debug_second_tree_reorder"); }

} // extern "C"
#endif // HRT_TEST_HOOKS

#ifdef HRT_WALK_STATS
// variant builds only (tools/walk_stats.py): read and clear the walker's phase statistics of the current device
extern "C" int hrt_debug_walk_stats(unsigned long long* out48)
{
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(out48, HIP_SYMBOL(hrt::g_walk_stats), sizeof(unsigned long long) * 48) != hipSuccess) return -1;
    unsigned long long z[48] = {};
    if (hipMemcpyToSymbol(HIP_SYMBOL(hrt::g_walk_stats), z, sizeof z) != hipSuccess) return -1;
    return 0;
}
#endif
