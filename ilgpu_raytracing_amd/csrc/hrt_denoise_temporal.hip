// hrt_denoise_temporal.hip -- temporal accumulation, variance estimate and variance-guided a-trous passes (hrt_denoise_temporal).
//
// Definition: include/hip_raytrace.h, "temporal denoiser".  float32 under include/hrt_math.h, no contraction, statement order of the
// contract.  Three kinds of kernel, records as laid out in hrt_denoise_temporal.hpp:
//   temporal   one pixel per lane: prepares the pixel's guides and demodulated colour (step 1), reprojects it into the history with
//              camera_motion (hrt_post.hpp, the function of the mode-2 present), gathers four history taps of three records each
//              and blends (step 2).  The previous guides and history are read only, the new ones written only.
//   variance   a 32x8 tile per 256-lane workgroup.  Pixels with N >= 4 need their own moments alone; a workgroup where some pixel has
//              a shorter history (the first frames, a disoccluded strip) stages guides and moments of its tile with halo 3 in LDS
//              (38x14 records of 40 B: 21536 B as the compiler lays the three arrays out) and those pixels run the 7x7 window.  The
//              vote is one __syncthreads_or, so a converged image pays a moments load and a 4-byte store per pixel.
//   iteration  hrt_denoise's sub-lattice tile (hrt_denoise.hip, shape 1: 36x12 records of three planes, 20736 B, rows of 32 consecutive
//              16-byte slots per half-wave, so ds_read_b128 is conflict-free without padding).  The variance rides in the fourth
//              word of the colour record that is staged anyway; its 3x3 prefilter reads the lattice neighbours out of the same tile.
#include <hip/hip_runtime.h>
#include <cmath>
#include "hrt_denoise_temporal.hpp"

using namespace hrt;

namespace {

HRT_D F3 albedo_of(const hrt_float3* baseColor, int idx, bool hit, bool demod)
{
    if (!demod || !hit) return mk3(1.f, 1.f, 1.f);
    const F3 b = ld3(&baseColor[idx]);
    return mk3(hrt_fmax(b.x, 0.01f), hrt_fmax(b.y, 0.01f), hrt_fmax(b.z, 0.01f));
}

HRT_D float lum(F3 v) { return 0.2126f * v.x + 0.7152f * v.y + 0.0722f * v.z; }
HRT_D F3 xyz(float4 v) { return mk3(v.x, v.y, v.z); }

struct Hist { F3 c; float m1, m2, n, ws; };

// one bilinear tap t of the history of the hit pixel with normal n, position P
HRT_D void history_tap(const DenoiseTemporalLaunch& L, int t, float wt, F3 n, F3 P, float tol, Hist& h)
{
    if (!(wt > 0.0f)) return;
    const float4 g0 = L.guidePrev[2 * (size_t)t], g1 = L.guidePrev[2 * (size_t)t + 1];
    if (__float_as_uint(g1.w) == 0u) return;
    if (!(dot(n, xyz(g0)) >= L.normal_cos_min)) return;
    if (!(hrt_abs(dot(xyz(g1) - P, n)) <= tol)) return;
    const float4 hc = L.hcolPrev[t], hm = L.hmomPrev[t];
    h.ws = h.ws + wt;
    h.c.x = h.c.x + wt * hc.x; h.c.y = h.c.y + wt * hc.y; h.c.z = h.c.z + wt * hc.z;
    h.m1 = h.m1 + wt * hm.x; h.m2 = h.m2 + wt * hm.y; h.n = h.n + wt * hm.z;
}

__global__ void __launch_bounds__(256)
hrt_denoise_temporal_kernel(DenoiseTemporalLaunch L)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)L.width * L.height) return;
    const int idx = (int)i, W = L.width, H = L.height;
    const bool hit = L.hitMask[idx] != 0;
    const F3 a = albedo_of(L.baseColor, idx, hit, L.demodulate);
    const F3 r = ld3(&L.radiance[idx]);
    const float dep = L.depth[idx];
    const float kx = 1.0f / (L.sp2 * hrt_fmax(dep * dep, 1e-12f));
    const F3 n = ld3(&L.normalWS[idx]), P = ld3(&L.worldPos[idx]);
    L.guideCur[2 * (size_t)idx] = make_float4(n.x, n.y, n.z, kx);
    L.guideCur[2 * (size_t)idx + 1] = make_float4(P.x, P.y, P.z, __uint_as_float(hit ? 1u : 0u));
    const F3 c = mk3(r.x / a.x, r.y / a.y, r.z / a.z);
    F3 C = c;
    float4 mrec = make_float4(0.f, 0.f, 0.f, 0.f);
    if (hit)
    {
        float hn = 0.f;
        Hist h; h.c = mk3(0.f, 0.f, 0.f); h.m1 = 0.f; h.m2 = 0.f; h.n = 0.f; h.ws = 0.f;
        if (L.haveHistory)
        {
            const int px = idx % W, py = idx / W;
            const Motion m = camera_motion(L.histCam, L.curCam, P, (float)W, (float)H);
            const float qx = (float)px + m.dx, qy = (float)py + m.dy;
            const bool valid = m.ok && qx >= 0.f && qx <= (float)(W - 1) && qy >= 0.f && qy <= (float)(H - 1);   // a NaN fails every comparison
            if (valid)
            {   // 0 <= x0 <= W - 1 and x1 is clamped: every tap lies inside the image
                const float x0f = hrt_floor(qx), y0f = hrt_floor(qy);
                const float fx = qx - x0f, fy = qy - y0f;
                const int x0 = hrt_f2i(x0f), y0 = hrt_f2i(y0f);
                const int x1 = hrt_imin(x0 + 1, W - 1), y1 = hrt_imin(y0 + 1, H - 1);
                const float tol = L.plane_tol * dep;
                history_tap(L, y0 * W + x0, (1.f - fx) * (1.f - fy), n, P, tol, h);
                history_tap(L, y0 * W + x1, fx * (1.f - fy), n, P, tol, h);
                history_tap(L, y1 * W + x0, (1.f - fx) * fy, n, P, tol, h);
                history_tap(L, y1 * W + x1, fx * fy, n, P, tol, h);
                if (h.ws > 0.0f)
                {
                    h.c = mk3(h.c.x / h.ws, h.c.y / h.ws, h.c.z / h.ws);
                    h.m1 = h.m1 / h.ws; h.m2 = h.m2 / h.ws;
                    hn = h.n / h.ws;
                }
            }
        }
        const float l = lum(c);
        if (!(hn > 0.0f))
            mrec = make_float4(l, l * l, 1.0f, 0.f);
        else
        {
            const float N = hrt_fmin(hn + 1.0f, L.max_history);
            const float rN = 1.0f / N;
            const float ac = hrt_fmax(rN, L.alpha_color), am = hrt_fmax(rN, L.alpha_moments);
            C = mk3(h.c.x + (c.x - h.c.x) * ac, h.c.y + (c.y - h.c.y) * ac, h.c.z + (c.z - h.c.z) * ac);
            mrec = make_float4(h.m1 + (l - h.m1) * am, h.m2 + (l * l - h.m2) * am, N, 0.f);
        }
    }
    L.hmomNew[idx] = mrec;
    const float4 crec = make_float4(C.x, C.y, C.z, 0.f);
    if (L.spatial)
        L.work[0][idx] = crec;
    else
    {
        L.hcolNew[idx] = crec;
        const F3 out = C * a;
        L.outRadiance[idx] = to3(out);
        L.outColor[idx] = pack_rgba8(out);
    }
}

// ---- variance

constexpr int kTileW = 32, kTileH = 8;
constexpr int kVarHalo = 3, kVarW = kTileW + 2 * kVarHalo, kVarH = kTileH + 2 * kVarHalo;

struct VarK { int W, H; float kn; const float4* guide; const float4* mom; float4* colour; };

__global__ void __launch_bounds__(256)
hrt_denoise_variance_kernel(VarK k)
{
    __shared__ float4 sG0[kVarW * kVarH], sG1[kVarW * kVarH];
    __shared__ float2 sM[kVarW * kVarH];
    const int bx = (int)blockIdx.x * kTileW, by = (int)blockIdx.y * kTileH;
    const int lx = threadIdx.x & (kTileW - 1), ly = threadIdx.x / kTileW;
    const int x = bx + lx, y = by + ly;
    const bool inside = x < k.W && y < k.H;
    const int idx = inside ? y * k.W + x : 0;
    float4 mo = make_float4(0.f, 0.f, 0.f, 0.f);
    bool hit = false;
    if (inside)
    {
        mo = k.mom[idx];
        hit = __float_as_uint(k.guide[2 * (size_t)idx + 1].w) != 0u;
    }
    float v = hit ? hrt_fmax(mo.y - mo.x * mo.x, 0.0f) : 0.0f;
    const bool window = hit && !(mo.z >= 4.0f);
    if (__syncthreads_or(window ? 1 : 0))                                   // uniform over the workgroup
    {
        for (int r = threadIdx.x; r < kVarW * kVarH; r += 256)
        {
            const int ry = r / kVarW, rx = r - ry * kVarW;
            const int u = bx + rx - kVarHalo, w = by + ry - kVarHalo;
            float4 g0 = make_float4(0.f, 0.f, 0.f, 0.f), g1 = g0;             // outside the image: not a hit
            float2 m = make_float2(0.f, 0.f);
            if (u >= 0 && u < k.W && w >= 0 && w < k.H)
            {
                const size_t q = (size_t)w * k.W + u;
                g0 = k.guide[2 * q]; g1 = k.guide[2 * q + 1];
                const float4 mq = k.mom[q];
                m = make_float2(mq.x, mq.y);
            }
            sG0[r] = g0; sG1[r] = g1; sM[r] = m;
        }
        __syncthreads();
        if (window)
        {
            const int r0 = (ly + kVarHalo) * kVarW + lx + kVarHalo;
            const float4 g0 = sG0[r0], g1 = sG1[r0];
            const F3 n = xyz(g0), P = xyz(g1);
            float S1 = 0.f, S2 = 0.f, sw = 0.f;
            for (int dy = -kVarHalo; dy <= kVarHalo; dy++)
#pragma unroll
                for (int dx = -kVarHalo; dx <= kVarHalo; dx++)
                {
                    const int r = r0 + dy * kVarW + dx;
                    const float4 q0 = sG0[r], q1 = sG1[r];
                    if (__float_as_uint(q1.w) == 0u) continue;
                    const F3 nd = n - xyz(q0);
                    const float dn = dot(nd, nd);
                    const float d = dot(xyz(q1) - P, n);
                    const float w = hrt_exp(-(dn * k.kn + d * d * g0.w));
                    if (w > 0.0f)                                           // a NaN fails
                    {
                        const float2 m = sM[r];
                        S1 = S1 + w * m.x; S2 = S2 + w * m.y; sw = sw + w;
                    }
                }
            if (sw > 0.0f)
            {
                S1 = S1 / sw; S2 = S2 / sw;
                v = hrt_fmax(S2 - S1 * S1, 0.0f) * (4.0f / mo.z);
            }
        }
    }
    if (inside) reinterpret_cast<float*>(k.colour)[4 * (size_t)idx + 3] = v;
}

// ---- the a-trous passes

struct ItK {
    int W, H, s;
    float kn, sigma_lum;
    int demod;
    const float4* guide;
    const float4* cin;
    float4* cout;                       // every pass but the last
    float4* hist;                       // iteration 0: the history colour plane as well; else null
    const hrt_float3* baseColor;        // the last pass: albedo, denoised radiance, packed colour
    hrt_float3* outRadiance;
    int32_t* outColor;
};

constexpr int kHalo = 2, kLdsW = kTileW + 2 * kHalo, kLdsH = kTileH + 2 * kHalo;
__device__ constexpr float kH[5] = {1.f / 16.f, 1.f / 4.f, 3.f / 8.f, 1.f / 4.f, 1.f / 16.f};
__device__ constexpr float kG[3] = {1.f / 4.f, 1.f / 2.f, 1.f / 4.f};

// blockIdx.z = the sub-lattice (oy * s + ox), blockIdx.x / y = its 32x8 tile
template <bool FINISH>
__global__ void __launch_bounds__(256)
hrt_denoise_temporal_iter_kernel(ItK k)
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
    const F3 n = xyz(g0), P = xyz(g1), cp = xyz(c0);
    const bool hit = __float_as_uint(g1.w) != 0u;
    F3 res = cp;
    float vres = c0.w;
    if (hit)
    {
        float vs = 0.f, gs = 0.f;
#pragma unroll
        for (int dy = -1; dy <= 1; dy++)
#pragma unroll
            for (int dx = -1; dx <= 1; dx++)
            {
                const int r = r0 + dy * kLdsW + dx;
                if (__float_as_uint(sG1[r].w) == 0u) continue;
                const float g = kG[dx + 1] * kG[dy + 1];
                vs = vs + g * sC[r].w; gs = gs + g;
            }
        const float vf = vs / gs;
        const float kl = 1.0f / (k.sigma_lum * hrt_sqrt(vf) + 1e-6f);
        const float lp = lum(cp);
        F3 acc = mk3(0.f, 0.f, 0.f);
        float va = 0.f, ws = 0.f;
#pragma unroll
        for (int dy = -2; dy <= 2; dy++)
#pragma unroll
            for (int dx = -2; dx <= 2; dx++)
            {
                const int r = r0 + dy * kLdsW + dx;
                const float4 q1 = sG1[r];
                if (__float_as_uint(q1.w) == 0u) continue;                  // q is not a hit (or lies outside the image)
                const float4 q0 = sG0[r], cq = sC[r];
                const F3 nd = n - xyz(q0);
                const float dn = dot(nd, nd);
                const float d = dot(xyz(q1) - P, n);
                const float e = dn * k.kn + d * d * g0.w + hrt_abs(lp - lum(xyz(cq))) * kl;
                const float w = (kH[dx + 2] * kH[dy + 2]) * hrt_exp(-e);
                if (w > 0.0f)                                               // a NaN fails
                {
                    acc.x = acc.x + w * cq.x; acc.y = acc.y + w * cq.y; acc.z = acc.z + w * cq.z;
                    va = va + (w * w) * cq.w;
                    ws = ws + w;
                }
            }
        if (ws > 0.0f)
        {
            res = mk3(acc.x / ws, acc.y / ws, acc.z / ws);
            vres = va / (ws * ws);
        }
    }
    const float4 rec = make_float4(res.x, res.y, res.z, vres);
    if (k.hist) k.hist[idx] = rec;
    if (FINISH)
    {
        F3 a = mk3(1.f, 1.f, 1.f);
        if (k.demod != 0 && hit)
        {
            const F3 b = ld3(&k.baseColor[idx]);
            a = mk3(hrt_fmax(b.x, 0.01f), hrt_fmax(b.y, 0.01f), hrt_fmax(b.z, 0.01f));
        }
        const F3 out = res * a;
        k.outRadiance[idx] = to3(out);
        k.outColor[idx] = pack_rgba8(out);
    }
    else
        k.cout[idx] = rec;
}

} // namespace

hipError_t denoise_temporal_launch(const DenoiseTemporalLaunch& L, hipStream_t st)
{
    const long long n = (long long)L.width * L.height;
    hipLaunchKernelGGL(hrt_denoise_temporal_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, L);
    if (!L.spatial) return hipGetLastError();
    VarK vk;
    vk.W = L.width; vk.H = L.height; vk.kn = L.kn; vk.guide = L.guideCur; vk.mom = L.hmomNew; vk.colour = L.work[0];
    hipLaunchKernelGGL(hrt_denoise_variance_kernel, dim3((unsigned)((L.width + kTileW - 1) / kTileW), (unsigned)((L.height + kTileH - 1) / kTileH)),
                       dim3(256), 0, st, vk);
    for (int i = 0; i < L.iterations; i++)
    {
        ItK k;
        k.W = L.width; k.H = L.height; k.s = 1 << i;
        k.kn = L.kn; k.sigma_lum = L.sigma_lum;
        k.demod = L.demodulate ? 1 : 0;
        k.guide = L.guideCur; k.cin = L.work[i & 1]; k.cout = L.work[(i + 1) & 1];
        k.hist = i == 0 ? L.hcolNew : nullptr;
        k.baseColor = L.baseColor; k.outRadiance = L.outRadiance; k.outColor = L.outColor;
        const int s = k.s, mx = (k.W + s - 1) / s, my = (k.H + s - 1) / s;   // the largest sub-lattice
        const dim3 grid((unsigned)((mx + kTileW - 1) / kTileW), (unsigned)((my + kTileH - 1) / kTileH), (unsigned)(s * s));
        if (i == L.iterations - 1) hipLaunchKernelGGL(hrt_denoise_temporal_iter_kernel<true>, grid, dim3(256), 0, st, k);
        else hipLaunchKernelGGL(hrt_denoise_temporal_iter_kernel<false>, grid, dim3(256), 0, st, k);
    }
    return hipGetLastError();
}
