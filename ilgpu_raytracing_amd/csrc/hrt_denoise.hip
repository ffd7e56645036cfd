// hrt_denoise.hip -- edge-avoiding a-trous denoiser guided by the G-buffer (hrt_denoise).
//
// Definition (include/hip_raytrace.h, "The filter"): a prepare pass demodulates the radiance by the albedo and packs what a tap reads
// into aligned records (hrt_denoise.hpp); `iterations` passes of a 5x5 B3-spline stencil with tap step 1 << i weight every hit
// neighbour by exp(-(normal term + plane-distance term + colour term)); the last pass multiplies the albedo back and packs.  Misses
// are copied.  float32 under include/hrt_math.h, no contraction, statement order of the contract: every pass is one tap() per
// neighbour in dy-outer, dx-inner order, whichever way the records reach the lane.
//
// Two shapes of the iteration pass, selected at build time (make variant DEFS=-DHRT_DENOISE_SHAPE=...; profiles/EXPERIMENTS.md):
//   1  sub-lattice tile in LDS.  The taps of step s stay inside the sub-lattice of pixels with equal (x mod s, y mod s), where they
//      are dense.  A 256-lane workgroup owns a 32x8 tile OF ONE SUB-LATTICE, stages its 36x12 records (three float4 planes, 20736 B)
//      and reads its 25 taps with ds_read_b128.  A lane's 32-lane half reads 32 consecutive 16-byte slots of one row: the two
//      16-lane groups of a ds_read_b128 inside a half ({0-3, 12-15, 20-27} and {4-11, 16-19, 28-31}) then cover 16 distinct slots
//      of the 256-byte bank row each, whatever the row stride and the tap offset, so the image needs no padding or swizzle.
//   0  one pixel per lane (64x4 per workgroup), 25 taps of three global 16-byte loads each through L1 / L2.
#include <hip/hip_runtime.h>
#include <cmath>
#include "hrt_denoise.hpp"

#ifndef HRT_DENOISE_SHAPE
#define HRT_DENOISE_SHAPE 1
#endif

using namespace hrt;

namespace {

struct DnK {
    int W, H, s;
    float kn, kc;
    int demod;
    const float4* guide;
    const float4* cin;
    float4* cout;                       // every pass but the last
    const hrt_float3* baseColor;        // the last pass: albedo, denoised radiance, packed colour
    hrt_float3* outRadiance;
    int32_t* outColor;
};

HRT_D F3 albedo_of(const hrt_float3* baseColor, int idx, bool hit, bool demod)
{
    if (!demod || !hit) return mk3(1.f, 1.f, 1.f);
    const F3 b = ld3(&baseColor[idx]);
    return mk3(hrt_fmax(b.x, 0.01f), hrt_fmax(b.y, 0.01f), hrt_fmax(b.z, 0.01f));
}

struct Centre { F3 n, P, c; float kx; };

// one neighbour q of the hit pixel p; hw = h[dx] * h[dy]
HRT_D void tap(const Centre& p, float4 g0, float4 g1, float4 cq, float hw, float kn, float kc, F3& acc, float& ws)
{
    if (__float_as_uint(g1.w) == 0u) return;                    // q is not a hit (or lies outside the image)
    const F3 nd = p.n - mk3(g0.x, g0.y, g0.z);
    const float dn = dot(nd, nd);
    const float d = dot(mk3(g1.x, g1.y, g1.z) - p.P, p.n);
    const F3 cd = p.c - mk3(cq.x, cq.y, cq.z);
    const float dc = dot(cd, cd);
    const float e = dn * kn + d * d * p.kx + dc * kc;
    const float w = hw * hrt_exp(-e);
    if (w > 0.0f)                                               // a NaN fails
    {
        acc.x = acc.x + w * cq.x; acc.y = acc.y + w * cq.y; acc.z = acc.z + w * cq.z;
        ws = ws + w;
    }
}

HRT_D F3 resolve(const Centre& p, F3 acc, float ws)
{
    return ws > 0.0f ? mk3(acc.x / ws, acc.y / ws, acc.z / ws) : p.c;
}

template <bool FINISH>
HRT_D void emit(const DnK& k, int idx, bool hit, F3 c)
{
    if (FINISH)
    {
        const F3 out = c * albedo_of(k.baseColor, idx, hit, k.demod != 0);
        k.outRadiance[idx] = to3(out);
        k.outColor[idx] = pack_rgba8(out);
    }
    else
        k.cout[idx] = make_float4(c.x, c.y, c.z, 0.f);
}

__device__ constexpr float kH[5] = {1.f / 16.f, 1.f / 4.f, 3.f / 8.f, 1.f / 4.f, 1.f / 16.f};

__global__ void __launch_bounds__(256)
hrt_denoise_prepare_kernel(DenoiseLaunch L)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)L.width * L.height) return;
    const int idx = (int)i;
    const bool hit = L.hitMask[idx] != 0;
    const F3 a = albedo_of(L.baseColor, idx, hit, L.demodulate);
    const F3 r = ld3(&L.radiance[idx]);
    const float dep = L.depth[idx];
    const float kx = 1.0f / (L.sp2 * hrt_fmax(dep * dep, 1e-12f));
    const F3 n = ld3(&L.normalWS[idx]), P = ld3(&L.worldPos[idx]);
    L.guide[2 * (size_t)idx] = make_float4(n.x, n.y, n.z, kx);
    L.guide[2 * (size_t)idx + 1] = make_float4(P.x, P.y, P.z, __uint_as_float(hit ? 1u : 0u));
    L.colour[0][idx] = make_float4(r.x / a.x, r.y / a.y, r.z / a.z, 0.f);
}

#if HRT_DENOISE_SHAPE == 1

constexpr int kTileW = 32, kTileH = 8, kHalo = 2, kLdsW = kTileW + 2 * kHalo, kLdsH = kTileH + 2 * kHalo;

// blockIdx.z = the sub-lattice (oy * s + ox), blockIdx.x / y = its 32x8 tile
template <bool FINISH>
__global__ void __launch_bounds__(256)
hrt_denoise_iter_kernel(DnK k)
{
    __shared__ float4 sG0[kLdsW * kLdsH], sG1[kLdsW * kLdsH], sC[kLdsW * kLdsH];
    const int s = k.s;
    const int oy = (int)blockIdx.z / s, ox = (int)blockIdx.z - oy * s;
    const int nx = (k.W - ox + s - 1) / s, ny = (k.H - oy + s - 1) / s;      // pixels of this sub-lattice (<= 0: none)
    const int bx = (int)blockIdx.x * kTileW, by = (int)blockIdx.y * kTileH;
    if (bx >= nx || by >= ny) return;                                        // the whole workgroup
    for (int r = threadIdx.x; r < kLdsW * kLdsH; r += 256)
    {
        const int ry = r / kLdsW, rx = r - ry * kLdsW;
        const int u = bx + rx - kHalo, v = by + ry - kHalo;
        float4 g0 = make_float4(0.f, 0.f, 0.f, 0.f), g1 = g0, c = g0;        // outside the image: not a hit
        if (u >= 0 && u < nx && v >= 0 && v < ny)
        {
            const size_t q = (size_t)(oy + v * s) * k.W + (ox + u * s);
            g0 = k.guide[2 * q]; g1 = k.guide[2 * q + 1]; c = k.cin[q];
        }
        sG0[r] = g0; sG1[r] = g1; sC[r] = c;
    }
    __syncthreads();
    const int lx = threadIdx.x & (kTileW - 1), ly = threadIdx.x / kTileW;
    const int u = bx + lx, v = by + ly;
    if (u >= nx || v >= ny) return;
    const int idx = (oy + v * s) * k.W + (ox + u * s);
    const int r0 = (ly + kHalo) * kLdsW + lx + kHalo;
    const float4 g0 = sG0[r0], g1 = sG1[r0], c0 = sC[r0];
    Centre p; p.n = mk3(g0.x, g0.y, g0.z); p.P = mk3(g1.x, g1.y, g1.z); p.c = mk3(c0.x, c0.y, c0.z); p.kx = g0.w;
    const bool hit = __float_as_uint(g1.w) != 0u;
    F3 res = p.c;
    if (hit)
    {
        F3 acc = mk3(0.f, 0.f, 0.f); float ws = 0.f;
#pragma unroll
        for (int dy = -2; dy <= 2; dy++)
#pragma unroll
            for (int dx = -2; dx <= 2; dx++)
            {
                const int r = r0 + dy * kLdsW + dx;
                tap(p, sG0[r], sG1[r], sC[r], kH[dx + 2] * kH[dy + 2], k.kn, k.kc, acc, ws);
            }
        res = resolve(p, acc, ws);
    }
    emit<FINISH>(k, idx, hit, res);
}

static void launch_iter(const DnK& k, bool finish, hipStream_t st)
{
    const int s = k.s, mx = (k.W + s - 1) / s, my = (k.H + s - 1) / s;       // the largest sub-lattice
    const dim3 grid((unsigned)((mx + kTileW - 1) / kTileW), (unsigned)((my + kTileH - 1) / kTileH), (unsigned)(s * s));
    if (finish) hipLaunchKernelGGL(hrt_denoise_iter_kernel<true>, grid, dim3(256), 0, st, k);
    else hipLaunchKernelGGL(hrt_denoise_iter_kernel<false>, grid, dim3(256), 0, st, k);
}

#else

template <bool FINISH>
__global__ void __launch_bounds__(256)
hrt_denoise_iter_kernel(DnK k)
{
    const int x = (int)blockIdx.x * 64 + (threadIdx.x & 63), y = (int)blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= k.W || y >= k.H) return;
    const int idx = y * k.W + x;
    const float4 g0 = k.guide[2 * (size_t)idx], g1 = k.guide[2 * (size_t)idx + 1], c0 = k.cin[idx];
    Centre p; p.n = mk3(g0.x, g0.y, g0.z); p.P = mk3(g1.x, g1.y, g1.z); p.c = mk3(c0.x, c0.y, c0.z); p.kx = g0.w;
    const bool hit = __float_as_uint(g1.w) != 0u;
    F3 res = p.c;
    if (hit)
    {
        F3 acc = mk3(0.f, 0.f, 0.f); float ws = 0.f;
#pragma unroll
        for (int dy = -2; dy <= 2; dy++)
        {
            const int qy = y + dy * k.s;
#pragma unroll
            for (int dx = -2; dx <= 2; dx++)
            {
                const int qx = x + dx * k.s;
                if (qx < 0 || qx >= k.W || qy < 0 || qy >= k.H) continue;
                const size_t q = (size_t)qy * k.W + qx;
                tap(p, k.guide[2 * q], k.guide[2 * q + 1], k.cin[q], kH[dx + 2] * kH[dy + 2], k.kn, k.kc, acc, ws);
            }
        }
        res = resolve(p, acc, ws);
    }
    emit<FINISH>(k, idx, hit, res);
}

static void launch_iter(const DnK& k, bool finish, hipStream_t st)
{
    const dim3 grid((unsigned)((k.W + 63) / 64), (unsigned)((k.H + 3) / 4));
    if (finish) hipLaunchKernelGGL(hrt_denoise_iter_kernel<true>, grid, dim3(256), 0, st, k);
    else hipLaunchKernelGGL(hrt_denoise_iter_kernel<false>, grid, dim3(256), 0, st, k);
}

#endif

} // namespace

hipError_t denoise_launch(const DenoiseLaunch& L, hipStream_t st)
{
    const long long n = (long long)L.width * L.height;
    hipLaunchKernelGGL(hrt_denoise_prepare_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, L);
    for (int i = 0; i < L.iterations; i++)
    {
        DnK k;
        k.W = L.width; k.H = L.height; k.s = 1 << i;
        const float sc = L.sigma_color * std::ldexp(1.0f, -i);           // exact scaling
        k.kn = L.kn; k.kc = 1.0f / (sc * sc);
        k.demod = L.demodulate ? 1 : 0;
        k.guide = L.guide; k.cin = L.colour[i & 1]; k.cout = L.colour[(i + 1) & 1];
        k.baseColor = L.baseColor; k.outRadiance = L.outRadiance; k.outColor = L.outColor;
        launch_iter(k, i == L.iterations - 1, st);
    }
    return hipGetLastError();
}
