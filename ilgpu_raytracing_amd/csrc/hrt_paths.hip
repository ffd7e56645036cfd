// hrt_paths.hip -- radiance queries (hrt_trace_paths): PathTraceKernel (RTRay.cs:203-325) along caller rays.
//
// The frame's two launches with the primary vertex taken from a caller ray: a primary kernel runs the frame's primary tracer for the
// scene on the ray buffer and writes a private G-buffer, and the fused path stage (path_trace_pixel with RAYS, hrt_device.hpp) runs
// the frame's bounce loop from it, in one kernel or in sample groups plus a resolve, as a frame of that size would.  Kernels of their
// own, in a translation unit of their own (hrt_paths.hpp), so the kernels of hrt_render_frame / hrt_render_progressive keep their code.
//
// Layout: a launch covers keys [k0, k1) laid out as rows of params->width keys (key j -> pixel (j % width, j / width)), walked in the
// frame's 8x8 tile order over the rows the keys touch (columns [x0, x0 + xw) when a row is wider than a chunk); lanes of other keys
// idle.  Camera rays in pixel order therefore run at the frame's coherence.
#include <hip/hip_runtime.h>
#include <type_traits>
#include "hrt_paths.hpp"
#include "hrt_query.hpp"

// key of the lane, or false for a lane outside the launch's keys
__device__ __forceinline__ bool paths_key(const TileMap& tm, const FrameK& k, const PathsK& q, int orig, int& key)
{
    int x, y;
    (void)tile_pixel(tm, k, x, y, orig);
    if (x >= q.xw || y >= k.row_end) return false;
    const long long j = (long long)y * k.width + q.x0 + x;
    if (j < q.k0 || j >= q.k1) return false;
    key = (int)j;
    return true;
}

// PrimaryVisibilityKernel (RTRay.cs:188-201) on the caller's ray of the key: TraceClosest(ray) with the frame's primary tracer, the
// G-buffer encoding of primary_pixel.  Rays with a non-finite origin or direction take TracerRef: the packed walkers' identity-instance
// shortcut is exact for finite rays only (hrt_query.hpp).
template <class TR>
__global__ void __launch_bounds__(256)
hrt_paths_primary_kernel(TR tr, TracerRef ref, FrameK k, DGBuffer gb, TileMap tm, PathsK q)
{
    Cnt<false> C;
    int j;
    if (!paths_key(tm, k, q, blockIdx.x, j)) return;
    Ray wray; wray.o = paths_origin(&q, j); wray.d = paths_dir(&q, j); wray.inv = inv_dir(wray.d);
    Hit h;
    bool hit;
    if (std::is_same<TR, TracerRef>::value || query_finite(wray)) hit = tr.template closest<false>(wray, h, C);
    else hit = ref.template closest<false>(wray, h, C);
    const int g = j - q.base;
    if (!hit)
    {   // StoreMiss :100-108
        gb.hitMask[g] = 0;
        gb.worldPos[g] = to3(wray.o + wray.d * 1e6f);
        gb.normalWS[g] = to3(mk3(0.f, 1.f, 0.f));
        gb.baseColor[g] = to3(mk3(0.f, 0.f, 0.f));
        gb.matId[g] = -1;
        gb.objId[g] = -1;
        return;
    }
    F3 posWS = wray.o + wray.d * h.t;
    int packedMat = (h.shade & 0xFFFF) | (float_to_i16(h.ior) << 16);
    gb.hitMask[g] = 1;
    gb.worldPos[g] = to3(posWS);
    gb.normalWS[g] = to3(h.n);
    gb.baseColor[g] = to3(h.albedo);
    gb.matId[g] = packedMat;
    gb.objId[g] = h.objId;
}

// the fused path stage, one key per lane (hrt_path_trace_kernel with reuse off)
template <class TR>
__global__ void __launch_bounds__(256, PtWaves<TR>::value)
hrt_paths_trace_kernel(TR tr, FrameK k, DGBuffer gb, TileMap tm, PathsK q)
{
    Cnt<false> C;
    int j;
    if (paths_key(tm, k, q, blockIdx.x, j))
        path_trace_pixel<TR, false, false, false, false, true>(tr, k, gb, DFramebuffer{}, DReservoir{}, DReservoir{}, 0, j, C, nullptr, nullptr, &q);
}

// ... in sample groups (hrt_path_trace_split_kernel): small key sets fill the machine as small tiles do
template <class TR>
__global__ void __launch_bounds__(256, PtWaves<TR>::value)
hrt_paths_split_kernel(TR tr, FrameK k, DGBuffer gb, TileMap tm, PathsK q, hrt_float3* li, float* stage, int nGroups, int perGroup)
{
    Cnt<false> C;
    const int g = blockIdx.x / tm.nTiles;
    SplitK sk;
    sk.li = li; sk.stage = stage; sk.group = g; sk.nGroups = nGroups;
    sk.sBegin = g * perGroup; sk.sEnd = min(sk.sBegin + perGroup, max(1, k.spp));
    const int tileBlock = blockIdx.x - g * tm.nTiles;
    sk.local = tileBlock * (int)blockDim.x + (int)threadIdx.x; sk.nLocal = tm.nTiles * (int)blockDim.x;
    int j;
    if (paths_key(tm, k, q, tileBlock, j))
        path_trace_pixel<TR, false, true, false, false, true>(tr, k, gb, DFramebuffer{}, DReservoir{}, DReservoir{}, 0, j, C, &sk, nullptr, &q);
}

// the ordered sample sum of split_resolve_pixel (:320-324) and the result record; no reservoir is kept
__global__ void __launch_bounds__(256)
hrt_paths_split_resolve_kernel(FrameK k, DGBuffer gb, TileMap tm, PathsK q, const hrt_float3* li)
{
    int j;
    if (!paths_key(tm, k, q, blockIdx.x, j)) return;
    const size_t local = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nLocal = (size_t)tm.nTiles * blockDim.x;
    const int spp = hrt_imax(1, k.spp);
    F3 Lframe = mk3(0.f, 0.f, 0.f);
    for (int s = 0; s < spp; s++) Lframe = Lframe + ld3(&li[(size_t)s * nLocal + local]);
    const F3 Lout = Lframe * (1.0f / (float)spp);
    const int g = j - q.base;
    paths_store(&q, j, Lout, ld3(&gb.worldPos[g]), gb.objId[g]);
}

template <class TR>
static void launch_stage(const PathsLaunch& L, const TR& tr, hipStream_t st)
{
    const dim3 grid(L.tm.nTiles), block(256);
    if (L.nGroups > 1)
    {
        const size_t nLocal = (size_t)L.tm.nTiles * 256;
        const int sppAll = L.k.spp > 1 ? L.k.spp : 1;
        hipLaunchKernelGGL((hrt_paths_split_kernel<TR>), dim3(L.tm.nTiles * L.nGroups), block, 0, st, tr, L.k, L.gb, L.tm, L.q,
                           (hrt_float3*)L.split, L.split + (size_t)sppAll * 3 * nLocal, L.nGroups, L.perGroup);
        hipLaunchKernelGGL(hrt_paths_split_resolve_kernel, grid, block, 0, st, L.k, L.gb, L.tm, L.q, (const hrt_float3*)L.split);
    }
    else hipLaunchKernelGGL((hrt_paths_trace_kernel<TR>), grid, block, 0, st, tr, L.k, L.gb, L.tm, L.q);
}

template <class TR>
static void launch_primary(const PathsLaunch& L, const TR& tr, hipStream_t st)
{
    TracerRef ref; ref.S = L.S;
    hipLaunchKernelGGL((hrt_paths_primary_kernel<TR>), dim3(L.tm.nTiles), dim3(256), 0, st, tr, ref, L.k, L.gb, L.tm, L.q);
}

hipError_t paths_launch(const PathsLaunch& L, hipStream_t st)
{
    if (L.tm.nTiles <= 0) return hipSuccess;
    if (L.flat)
    {
        TracerFlat t; t.tree.P = L.P; t.tree.S = L.S; t.leaves = L.leaves; t.nLeaves = L.nLeaves;
        launch_primary(L, t, st);
        launch_stage(L, t, st);
    }
    else if (L.variant == 0)
    {
        TracerPackedT<0> t; t.P = L.P; t.S = L.S;
        if (L.second) { TracerSecond t2; t2.second = t; t2.second.P = L.PAny; t2.uploaded = t; launch_primary(L, t2, st); }
        else launch_primary(L, t, st);
        launch_stage(L, t, st);
    }
    else if (L.variant == 1) { TracerPackedT<1> t; t.P = L.P; t.S = L.S; launch_primary(L, t, st); launch_stage(L, t, st); }
    else if (L.variant == 3) { TracerPackedT<3> t; t.P = L.P; t.S = L.S; launch_primary(L, t, st); launch_stage(L, t, st); }
    else { TracerRef t; t.S = L.S; launch_primary(L, t, st); launch_stage(L, t, st); }
    return hipGetLastError();
}
