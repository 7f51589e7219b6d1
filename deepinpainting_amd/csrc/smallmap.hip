// smallmap.hip — small maps.  The inner levels of both U-Nets and netF (512-1024 channels on 8x8 ... 1x1: models/networks.py:220-259, 404-432,
// 510-515) are ~85 convolution calls per training step whose arithmetic is a skinny GEMM between a 9-33 MB weight tensor and
// a handful of activations: MIOpen spends 45-150 us on each (layout transposes, zero fills, tiles made for large maps).
// Here the weight tensor Wm = [R][Q] (R = its first channel dimension, Q = second channel dimension x taps, contiguous: Conv2d
// [Cout][(Cin,t)], ConvTranspose2d [Cin][(Cout,t)]) is STREAMED ONCE from where it lies, 16 bytes per lane straight into
// MFMA operands — no LDS, no packing — and the P = B*Ho*Wo <= 1024 positions ride on the 32-wide N side of 32x32x2 MFMAs:
//   DATA (Conv2d backward-data, ConvTranspose2d forward)   Mcol[q][p] = sum_r Wm[r][q] * in[r][p],  then col2im over the taps
//   FWD  (Conv2d forward, ConvTranspose2d backward-data)    y[r][p]    = sum_q Wm[r][q] * col(fine)[q][p]
//   WRW  (weight gradient of either)                        dW[r][q]   = sum_p coarse[r][p] * col(fine)[q][p]   (native layout, one pass)
// p runs over the grid on R's side ("coarse": the conv's output side), "fine" is the grid on Q's side.  The row / column labels
// of an MFMA tile are free, so a lane's float4 of four consecutive q feeds four MFMAs whose tiles are q = q0 + 4m + j: every
// weight byte is fetched by exactly one coalesced 16-byte load.  The streams are bandwidth bound (16.8 MB in ~5 us); the
// reduction is cut over workgroups into slabs that the tiny post-pass (col2im / layout) adds in order (deterministic).
//
// The small operand (in, col(fine), coarse) is GATHERED by the main kernels from the NCHW tensor itself: its position (b, oy, ox)
// or its (channel, tap) is a lane's own for the whole loop, the tensors are 64 KB - 1 MB and sit in L2, and a position >= P, a tap
// outside the map or the padding row of Pp is a load the hardware drops (see "operands of the main kernels").  The pre-pass kernels
// (sm_to_cn, sm_im2col_cn, sm_to_nc, sm_im2col_nt) that lay the same values out as images in the workspace remain — "staged": the
// weight gradient above 32 positions (sm_staged), and everything under ipsr_debug_set_option(3, 1); the values fed to the
// MFMAs are the same numbers in the same order either way, so the results are the same bits.  The plan and the workspace size do
// not depend on the form: gathered calls leave the image slices of the workspace unused.
// Each stream is software-pipelined over three register sets (sm_stream): two groups of loads are in flight beyond the one whose
// MFMAs run.
// A second regime, asked for by a flag bit of `op` (SM_TILED), runs DATA and FWD from 33 positions up as LDS-tiled split-K GEMMs on the same
// weights in place (sm_tiled_kernel, "the tiled regime" below): from 256 positions up it is ahead of the streams.
#include <algorithm>

#include "ipsr_common.h"

namespace ipsr {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4v __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(256) sm_to_cn_kernel(const float* __restrict__ x, int B, int C, int HW, int Tp, float* __restrict__ out)
{
    const int n = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y;
    if (n >= Tp) return;
    float v = 0.0f;
    if (n < B * HW) { const int b = n / HW, p = n - b * HW; v = x[((size_t)b * C + c) * HW + p]; }
    out[(size_t)c * Tp + n] = v;
}

__global__ void __launch_bounds__(256) sm_to_nc_kernel(const float* __restrict__ x, int B, int C, int HW, float* __restrict__ out)
{
    const int c = blockIdx.x * 256 + threadIdx.x, n = blockIdx.y;              // rows n >= B*HW are zero padding of the reduction
    if (c >= C) return;
    float v = 0.0f;
    if (n < B * HW) { const int b = n / HW, p = n - b * HW; v = x[((size_t)b * C + c) * HW + p]; }
    out[(size_t)n * C + c] = v;
}

__device__ __forceinline__ float sm_tap(const float* __restrict__ f, int B, int C, int Hf, int Wf, int Ho, int Wo, int k, int st, int pad, int dil,
                                        int n, int col)
{
    if (n >= B * Ho * Wo) return 0.0f;
    const int kk = k * k;
    const int c = col / kk, t = col - c * kk, r = t / k, q = t - r * k;
    const int b = n / (Ho * Wo), o = n - b * Ho * Wo, oy = o / Wo, ox = o - oy * Wo;
    const int fy = oy * st - pad + r * dil, fx = ox * st - pad + q * dil;
    return ((unsigned)fy < (unsigned)Hf && (unsigned)fx < (unsigned)Wf) ? f[(((size_t)b * C + c) * Hf + fy) * Wf + fx] : 0.0f;
}

// V[n][(c,t)] = fine[b][c][oy*s - pad + r*dil][ox*s - pad + q*dil]  (0 outside; rows n >= B*Ho*Wo zero)
__global__ void __launch_bounds__(256) sm_im2col_nt_kernel(const float* __restrict__ f, int B, int C, int Hf, int Wf, int Ho, int Wo,
                                                           int k, int st, int pad, int dil, float* __restrict__ out)
{
    const int col = blockIdx.x * 256 + threadIdx.x, n = blockIdx.y;
    const int ncol = C * k * k;
    if (col >= ncol) return;
    out[(size_t)n * ncol + col] = sm_tap(f, B, C, Hf, Wf, Ho, Wo, k, st, pad, dil, n, col);
}

// the same as [(c,t)][n] with row length Tp (columns n >= B*Ho*Wo zero)
__global__ void __launch_bounds__(256) sm_im2col_cn_kernel(const float* __restrict__ f, int B, int C, int Hf, int Wf, int Ho, int Wo,
                                                           int k, int st, int pad, int dil, int Tp, float* __restrict__ out)
{
    const int n = blockIdx.x * 256 + threadIdx.x, col = blockIdx.y;
    if (n >= Tp) return;
    out[(size_t)col * Tp + n] = sm_tap(f, B, C, Hf, Wf, Ho, Wo, k, st, pad, dil, n, col);
}

// out[b][c][fy][fx] = sum_{slabs} sum_{(r,q): fy = oy*s - pad + r*dil, fx = ox*s - pad + q*dil} M[(c,t)][(b,oy,ox)]
__global__ void __launch_bounds__(256) sm_col2im_kernel(const float* __restrict__ M, int nslab, size_t slab_stride, int B, int C, int Hf, int Wf,
                                                        int Ho, int Wo, int k, int st, int pad, int dil, int Tp, float* __restrict__ out)
{
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t total = (size_t)B * C * Hf * Wf;
    if (idx >= total) return;
    const int fx = (int)(idx % Wf), fy = (int)((idx / Wf) % Hf), c = (int)((idx / ((size_t)Wf * Hf)) % C), b = (int)(idx / ((size_t)Wf * Hf * C));
    float acc = 0.0f;
    for (int r = 0; r < k; ++r) {
        const int ny = fy + pad - r * dil;
        if (ny < 0 || ny % st) continue;
        const int oy = ny / st;
        if (oy >= Ho) continue;
        for (int q = 0; q < k; ++q) {
            const int nx = fx + pad - q * dil;
            if (nx < 0 || nx % st) continue;
            const int ox = nx / st;
            if (ox >= Wo) continue;
            const size_t off = (size_t)(c * k * k + r * k + q) * Tp + ((size_t)b * Ho + oy) * Wo + ox;
            for (int sl = 0; sl < nslab; ++sl) acc += M[(size_t)sl * slab_stride + off];
        }
    }
    out[idx] = acc;
}

// The same sums in the same order with every load issued before the first add: all K x K taps x up to SL slabs of a thread are
// independent buffer loads (a tap that reaches no position and a slab >= nslab are dropped by the descriptor's bounds check and add
// +0.0f, which changes no bit), where the loop above waits an L2 round trip per term.
template <int K, int SL>
__global__ void __launch_bounds__(256) sm_col2im_wide_kernel(const float* __restrict__ M, int nslab, unsigned slab_bytes, unsigned m_bytes, int B, int C, int Hf, int Wf,
                                                             int Ho, int Wo, int st, int pad, int dil, int Tp, float* __restrict__ out)
{
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t total = (size_t)B * C * Hf * Wf;
    if (idx >= total) return;
    const int fx = (int)(idx % Wf), fy = (int)((idx / Wf) % Hf), c = (int)((idx / ((size_t)Wf * Hf)) % C), b = (int)(idx / ((size_t)Wf * Hf * C));
    const __amdgpu_buffer_rsrc_t mrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(M), 0, (int)m_bytes, 0x00020000);
    float v[K * K][SL];
#pragma unroll
    for (int r = 0; r < K; ++r) {
        const int ny = fy + pad - r * dil, oy = ny / st;
        const bool yok = ny >= 0 && ny % st == 0 && oy < Ho;
#pragma unroll
        for (int q = 0; q < K; ++q) {
            const int nx = fx + pad - q * dil, ox = nx / st;
            const bool ok = yok && nx >= 0 && nx % st == 0 && ox < Wo;
            const unsigned off = (unsigned)((c * K * K + r * K + q) * Tp + (b * Ho + oy) * Wo + ox) * 4u;
#pragma unroll
            for (int sl = 0; sl < SL; ++sl)
                v[r * K + q][sl] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(mrs, (ok && sl < nslab) ? off + (unsigned)sl * slab_bytes : 0x80000000u, 0, 0));
        }
    }
    float acc = 0.0f;
#pragma unroll
    for (int t = 0; t < K * K; ++t)
#pragma unroll
        for (int sl = 0; sl < SL; ++sl) acc += v[t][sl];
    out[idx] = acc;
}

// out[b][r][o] = sum_{slabs} Y[slab][r][(b,o)]
__global__ void __launch_bounds__(256) sm_sum_to_nchw_kernel(const float* __restrict__ Y, int nslab, size_t slab_stride, int B, int R, int HW, int Tp,
                                                             float* __restrict__ out)
{
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)B * R * HW) return;
    const int o = (int)(idx % HW), r = (int)((idx / HW) % R), b = (int)(idx / ((size_t)HW * R));
    const size_t off = (size_t)r * Tp + (size_t)b * HW + o;
    float acc = 0.0f;
    for (int sl = 0; sl < nslab; ++sl) acc += Y[(size_t)sl * slab_stride + off];
    out[idx] = acc;
}

// In-workgroup reduction of the four waves' partial tiles (each wave took a quarter of the slab's reduction range): waves 1..3
// park a tile in LDS, wave 0 adds them in order.  Deterministic; 4x fewer slabs for the same number of waves in flight.
template <int NB>
__device__ __forceinline__ void sm_reduce4(f32x16 (&acc)[NB], float* lds, int wave, int lane)
{
    if (wave > 0) {
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int e = 0; e < 16; ++e) lds[(((wave - 1) * NB + nb) * 16 + e) * 64 + lane] = acc[nb][e];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int w = 0; w < 3; ++w)
#pragma unroll
            for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[nb][e] += lds[((w * NB + nb) * 16 + e) * 64 + lane];
    }
    __syncthreads();
}

// ---- operands of the main kernels ------------------------------------------------------------------------------------------------------
// Every load of a main kernel goes through a buffer descriptor that covers exactly the tensor it reads (all operands are below 2 GiB:
// launch_smallmap checks), with a 32-bit byte offset.  A load that is predicated off — a partly filled or empty group, a prefetch
// past the wave's range, a position >= P, a tap outside the map — has bit 31 of its offset set (sm_off), which is past every
// descriptor: the hardware drops it (no memory access) and the destination reads +0.0f, the value the pre-passes write for the
// same element.  No load is under a branch, so the loads of a group sit in one basic block and the compiler's wait counts let group
// g's MFMAs start while the groups after it are in flight.
constexpr unsigned SM_OFF = 0x80000000u;
__device__ __forceinline__ unsigned sm_off(unsigned off, unsigned on) { return off | (((on & 1u) - 1u) & SM_OFF); }     // on = 1: off, on = 0: dropped
__device__ __forceinline__ int cdiv_dev(int a, int b) { return (a + b - 1) / b; }

__device__ __forceinline__ __amdgpu_buffer_rsrc_t sm_rsrc(const float* p, unsigned bytes)
{
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p), 0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ float sm_ld(__amdgpu_buffer_rsrc_t rs, unsigned off) { return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, off, 0, 0)); }
__device__ __forceinline__ f32x4v sm_ld4(__amdgpu_buffer_rsrc_t rs, unsigned off)
{
    return __builtin_bit_cast(f32x4v, __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0));
}

// the convolution's geometry, for the kernels that gather from the NCHW tensors: coarse [B][R][Ho][Wo], fine [B][C][Hf][Wf]
struct SmGeo { int P, R, C, Ho, Wo, Hf, Wf, k, st, pad, dil; };

// One position p = (b, oy, ox) of the coarse grid as the taps see it: the byte offset of fine[b][0][oy*s - pad][ox*s - pad] (modulo
// 2^32: the corner may lie outside the tensor, the taps that are loaded do not) and which kernel rows r / columns s fall inside the
// map (bit r of ymask, bit s of xmask).  A position >= P has no row inside.
struct SmPos {
    unsigned base, ymask, xmask;
    SmPos() = default;
    __device__ __forceinline__ SmPos(const SmGeo& g, int p)
    {
        const int HW = g.Ho * g.Wo, b = p / HW, o = p - b * HW, oy = o / g.Wo, ox = o - oy * g.Wo;
        const int iy0 = oy * g.st - g.pad, ix0 = ox * g.st - g.pad;
        base = (unsigned)((b * g.C * g.Hf + iy0) * g.Wf + ix0) * 4u;
        ymask = xmask = 0;
        for (int t = 0; t < g.k; ++t) {
            ymask |= (unsigned)(p < g.P && (unsigned)(iy0 + t * g.dil) < (unsigned)g.Hf) << t;
            xmask |= (unsigned)((unsigned)(ix0 + t * g.dil) < (unsigned)g.Wf) << t;
        }
    }
};

// Byte offset of col(fine)[q][p] — tap t = q % K^2 = (r, s) of channel c = q / K^2 at position `pos` — dropped where the tap falls
// outside the map (the zero sm_tap returns) or `on` is 0.
template <int K>
__device__ __forceinline__ unsigned sm_tap_off(const SmGeo& g, const SmPos& pos, unsigned q, unsigned on)
{
    const unsigned c = q / (K * K), t = q - c * (K * K), r = t / K, s = t - r * K;
    return sm_off(pos.base + (c * g.Hf * g.Wf + r * g.dil * g.Wf + s * g.dil) * 4u, (pos.ymask >> r) & (pos.xmask >> s) & on);
}

// The software pipeline of the three streams.  A group is G loads of 16 weight bytes per lane with the small-operand values that go
// with them; `load(set, g)` issues group g into a register set (a group past the wave's range loads nothing: every offset is
// SM_OFF), `mma(set)` runs its MFMAs.  Three sets rotate, so two groups beyond the one being consumed are in flight: 3 * G * 16 =
// 192 B per lane, 48 KiB per CU at one workgroup per CU, of weights alone.  The MFMAs run in group order, as a plain loop would.
// The instruction scheduler may not move anything across SM_KEEP_ORDER: without it, it sinks each load to its first use to save
// registers and the prefetch is gone.  Every set is either consumed unconditionally or carried round the loop, so that no load can be
// sunk into a conditional block either.
#define SM_KEEP_ORDER() __builtin_amdgcn_sched_barrier(0)

template <class Set, class Load, class Mma>
__device__ __forceinline__ void sm_stream(int ngroups, Load load, Mma mma)
{
    Set s0, s1, s2;
    load(s0, 0);
    load(s1, 1);
    int g = 0;
    if (ngroups >= 3) do {            // a bottom-tested loop: as a `for`, the sets were copied at the loop head, behind a wait for every load
        load(s2, g + 2);
        SM_KEEP_ORDER();
        mma(s0);
        SM_KEEP_ORDER();
        load(s0, g + 3);
        SM_KEEP_ORDER();
        mma(s1);
        SM_KEEP_ORDER();
        load(s1, g + 4);
        SM_KEEP_ORDER();
        mma(s2);
        SM_KEEP_ORDER();
        g += 3;
    } while (g + 3 <= ngroups);
    if (g < ngroups) mma(s0);
    if (g + 1 < ngroups) mma(s1);
}

// group depth: 4 as in the single-buffered loops these kernels had; 2 where four position blocks' accumulators and operands fill the registers
template <int NB> struct SmDepth { static constexpr int G = NB == 4 ? 2 : 4; };

// DATA: one workgroup (4 waves) = 128 columns q of Wm x the rows of its slab (a quarter per wave) x NB position blocks.
//   A (MFMA j, lane (m, h)) = Wm[r + h][q0 + 4m + j]   — component j of the lane's float4 at Wm[r + h][q0 + 4m]
//   B (lane (n, h))         = in[r + h][n0 + 32 nb + n]
// slab s = blockIdx.y: Mcol_s[q0 + 4*row + j][n] for the 32x32 tile rows `row` of MFMA j.
// in[r][n]: HW == 0: the [R][Tp] image sm_to_cn_kernel laid out at In;  HW > 0: In is the NCHW tensor, in[r][n] = In[(b*R + r)*HW + o]
// for n = b*HW + o < P and zero for the padding columns — (b, o) is the lane's own for the whole loop, only r advances.
template <int NB>
__global__ void __launch_bounds__(256) sm_data_kernel(const float* __restrict__ Wm, const float* __restrict__ In, int R, int Q, int Tp, int rows_per_wave,
                                                      int P, int HW, float* __restrict__ Mcol)
{
    __shared__ float red[3 * NB * 16 * 64];
    constexpr int G = SmDepth<NB>::G;                      // row pairs per group
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), m = lane & 31, h = lane >> 5;
    const int q0 = blockIdx.x * 128, n0 = blockIdx.z * (32 * NB);
    const int ra = min(R, (blockIdx.y * 4 + wave) * rows_per_wave), rb = min(R, ra + rows_per_wave);
    const __amdgpu_buffer_rsrc_t wrs = sm_rsrc(Wm, (unsigned)R * Q * 4u), irs = sm_rsrc(In, (unsigned)R * (HW ? P : Tp) * 4u);
    f32x16 acc[4][NB];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[j][nb][e] = 0.0f;
    const unsigned wlane = (unsigned)(h * Q + q0 + 4 * m) * 4u, wrow = (unsigned)Q * 4u, irow = (unsigned)(HW ? HW : Tp) * 4u;
    unsigned icol[NB];                                     // the lane's position in row 0 of `in`
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        const int n = n0 + 32 * nb + m;
        icol[nb] = !HW ? (unsigned)n * 4u : (n < P ? (unsigned)((n / HW) * R * HW + n % HW) * 4u : SM_OFF);
    }
    struct Set { f32x4v a[G]; float bv[G][NB]; };
    auto load = [&](Set& s, int grp) {
        const int r = ra + grp * 2 * G;
#pragma unroll
        for (int u = 0; u < G; ++u) {
            const unsigned ok = r + 2 * u < rb;           // R and rows_per_wave are even: a pair is in or out as a whole
            s.a[u] = sm_ld4(wrs, sm_off(wlane + (unsigned)(r + 2 * u) * wrow, ok));
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) s.bv[u][nb] = sm_ld(irs, sm_off(icol[nb] + (unsigned)(r + 2 * u + h) * irow, ok) | (icol[nb] & SM_OFF));
        }
    };
    auto mma = [&](const Set& s) {
#pragma unroll
        for (int u = 0; u < G; ++u)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) acc[j][nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(s.a[u][j], s.bv[u][nb], acc[j][nb], 0, 0, 0);
    };
    sm_stream<Set>(cdiv_dev(rb - ra, 2 * G), load, mma);
    float* out = Mcol + (size_t)blockIdx.y * Q * Tp;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        sm_reduce4<NB>(acc[j], red, wave, lane);
        if (wave == 0) {
#pragma unroll
            for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int row = (e & 3) + 8 * (e >> 2) + 4 * h;
                    out[(size_t)(q0 + 4 * row + j) * Tp + n0 + 32 * nb + m] = acc[j][nb][e];
                }
        }
    }
}

// FWD: one workgroup (4 waves) = 32 rows r of Wm x the columns of its slab (a quarter per wave) x NB position blocks.
//   A (MFMA j, lane (m, h)) = Wm[r0 + m][q + 4h + j]   — component j of the lane's float4 at Wm[r0 + m][q + 4h]
//   B (MFMA j, lane (n, h)) = col[q + 4h + j][n0 + 32 nb + n]
// col[q][n]: K == 0: the [Q][Tp] image sm_im2col_cn_kernel laid out at X;  K > 0: X is the fine NCHW tensor and col[q][n] its tap
// (sm_tap_off) — (b, oy, ox) is the lane's own for the whole loop, (c, tap) follows q.
template <int NB, int K>
__global__ void __launch_bounds__(256) sm_fwd_kernel(const float* __restrict__ Wm, const float* __restrict__ X, int R, int Q, int Tp, int cols_per_wave,
                                                     SmGeo g, float* __restrict__ Y)
{
    __shared__ float red[3 * NB * 16 * 64];
    constexpr int G = SmDepth<NB>::G, KS = K ? K : 1;      // groups of 8 columns per pipeline group
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), m = lane & 31, h = lane >> 5;
    const int r0 = blockIdx.x * 32, n0 = blockIdx.z * (32 * NB);
    const int qa = min(Q, (blockIdx.y * 4 + wave) * cols_per_wave), qb = min(Q, qa + cols_per_wave);
    const __amdgpu_buffer_rsrc_t wrs = sm_rsrc(Wm, (unsigned)R * Q * 4u);
    const __amdgpu_buffer_rsrc_t xrs = sm_rsrc(X, (K ? (unsigned)(g.P / (g.Ho * g.Wo)) * g.C * g.Hf * g.Wf : (unsigned)Q * Tp) * 4u);
    f32x16 acc[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[nb][e] = 0.0f;
    const unsigned wlane = (unsigned)((r0 + m) * Q + 4 * h) * 4u;
    SmPos pos[NB];                                         // the lane's positions (unused by the staged form)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) pos[nb] = SmPos(g, n0 + 32 * nb + m);
    struct Set { f32x4v a[G]; float bv[G][4][NB]; };
    auto load = [&](Set& s, int grp) {
        const int q = qa + grp * 8 * G;
#pragma unroll
        for (int u = 0; u < G; ++u) {
            const unsigned ok = q + 8 * u < qb;           // Q and cols_per_wave are multiples of 8
            s.a[u] = sm_ld4(wrs, sm_off(wlane + (unsigned)(q + 8 * u) * 4u, ok));
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) {
                    const unsigned qq = (unsigned)(q + 8 * u + 4 * h + j);
                    s.bv[u][j][nb] = sm_ld(xrs, K ? sm_tap_off<KS>(g, pos[nb], qq, ok) : sm_off((qq * Tp + n0 + 32 * nb + m) * 4u, ok));
                }
        }
    };
    auto mma = [&](const Set& s) {
#pragma unroll
        for (int u = 0; u < G; ++u)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) acc[nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(s.a[u][j], s.bv[u][j][nb], acc[nb], 0, 0, 0);
    };
    sm_stream<Set>(cdiv_dev(qb - qa, 8 * G), load, mma);
    sm_reduce4<NB>(acc, red, wave, lane);
    if (wave == 0) {
        float* out = Y + (size_t)blockIdx.y * R * Tp;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = (e & 3) + 8 * (e >> 2) + 4 * h;
                out[(size_t)(r0 + row) * Tp + n0 + 32 * nb + m] = acc[nb][e];
            }
    }
}

// WRW: one wave = the 32 x 128 block dW[r0 .. r0+31][q0 .. q0+127], reduction over all Pp (even, zero padded) positions.
//   A (lane (m, h)) = Ct[p + h][r0 + m]                      coarse tensor as [p][r]
//   B (MFMA j)      = component j of the float4 Vt[p + h][q0 + 4n]   im2col of the fine tensor as [p][(c,t)]  -> tile column n is q0 + 4n + j
// K == 0: Ct / Vt are the images sm_to_nc_kernel / sm_im2col_nt_kernel laid out.  K > 0: they are the NCHW tensors: Ct[p][r] =
// coarse[(b*R + r)*Ho*Wo + o], and the lane's four Vt values are four taps of position p.  q0 + 4n + j is the lane's own for the
// whole loop: its (c, tap) is taken apart once, per component (for K = 3 four consecutive q cross a kernel row and a channel).  p
// advances, and what a position contributes to an address — SmPos and its offset in `coarse` — is tabulated in LDS first (<= 1024
// positions; entry Pp stands for every position past the end), so the loop adds and compares only.
template <int K>
__global__ void __launch_bounds__(64) sm_wrw_kernel(const float* __restrict__ Ct, const float* __restrict__ Vt, int R, int Q, int Pp, SmGeo g, float* __restrict__ dW)
{
    constexpr int G = 4, KS = K ? K : 1;                   // position pairs per group
    __shared__ uint4 tab[K ? 1025 : 1];                    // (byte offset in coarse, SmPos) of every position
    const int lane = threadIdx.x, m = lane & 31, h = lane >> 5;
    const int q0 = blockIdx.x * 128, r0 = blockIdx.y * 32;
    const int HW = g.Ho * g.Wo;
    const __amdgpu_buffer_rsrc_t crs = sm_rsrc(Ct, (unsigned)(K ? g.P : Pp) * R * 4u);
    const __amdgpu_buffer_rsrc_t vrs = sm_rsrc(Vt, (K ? (unsigned)(g.P / HW) * g.C * g.Hf * g.Wf : (unsigned)Pp * Q) * 4u);
    f32x16 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[j][e] = 0.0f;
    unsigned tr[4], ts[4], toff[4];                        // the lane's four (c, tap): kernel row, column, byte offset from a position's corner
    const unsigned rlane = (unsigned)((r0 + m) * HW) * 4u;
    if constexpr (K != 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned q = q0 + 4 * m + j, c = q / (KS * KS), t = q - c * (KS * KS);
            tr[j] = t / KS; ts[j] = t - tr[j] * KS; toff[j] = (c * g.Hf * g.Wf + tr[j] * g.dil * g.Wf + ts[j] * g.dil) * 4u;
        }
        for (int p = lane; p <= Pp; p += 64) {
            const SmPos pos(g, p);
            const int b = p / HW;
            tab[p] = make_uint4(p < g.P ? (unsigned)(b * R * HW + p - b * HW) * 4u : SM_OFF, pos.base, pos.ymask, pos.xmask);
        }
        __syncthreads();
    }
    struct Set { float av[G]; f32x4v b[G]; };
    auto load = [&](Set& s, int grp) {
        const int p = grp * 2 * G;
#pragma unroll
        for (int u = 0; u < G; ++u) {
            const int pp = p + 2 * u + h;
            if constexpr (K == 0) {
                const unsigned ok = p + 2 * u < Pp;
                s.av[u] = sm_ld(crs, sm_off((unsigned)(pp * R + r0 + m) * 4u, ok));
                s.b[u] = sm_ld4(vrs, sm_off((unsigned)(pp * Q + q0 + 4 * m) * 4u, ok));
            } else {
                const uint4 e = tab[min(pp, Pp)];          // the same for the 32 lanes of a half-wave
                s.av[u] = sm_ld(crs, e.x + rlane);         // SM_OFF + rlane stays past the descriptor
#pragma unroll
                for (int j = 0; j < 4; ++j) s.b[u][j] = sm_ld(vrs, sm_off(e.y + toff[j], (e.z >> tr[j]) & (e.w >> ts[j])));
            }
        }
    };
    auto mma = [&](const Set& s) {
#pragma unroll
        for (int u = 0; u < G; ++u)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(s.av[u], s.b[u][j], acc[j], 0, 0, 0);
    };
    sm_stream<Set>(cdiv_dev(Pp, 2 * G), load, mma);
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int row = (e & 3) + 8 * (e >> 2) + 4 * h;
        *reinterpret_cast<f32x4v*>(dW + (size_t)(r0 + row) * Q + q0 + 4 * m) = f32x4v{acc[0][e], acc[1][e], acc[2][e], acc[3][e]};
    }
}

// ---- the tiled regime (op | SM_TILED): 33 .. 1024 positions -------------------------------------------------------------------------------
// From 128 positions up DATA and FWD are real GEMMs, and a stream that reloads every small-operand value per lane and MFMA and reads the
// weights once per 128 positions is bound by its loads.  Here both are the LDS-tiled fp32-MFMA GEMM of conv_gemm.hip: 256 threads, a
// 128 (rows of the result) x 128 (positions) tile, 2 x 2 sub-tiles of 32 x 32 per wave, 16-deep stages double-buffered in LDS (32 KiB: up to
// four workgroups per CU), one barrier per stage.  The weights are still read where they lie:
//   DATA  Mcol[q][p] = sum_r Wm[r][q] * in[r][p]     Wm is reduction-major with q contiguous — the [red][rows] LDS image itself: its rows go
//                                                     HBM -> LDS by 16-byte DMA, one stage ahead (R % 32 == 0, Q % 128 == 0: every piece is whole)
//   FWD   Y[r][p]    = sum_q Wm[r][q] * col[q][p]    Wm's rows are reduction-contiguous: a thread's float4 is four reduction steps of one row,
//                                                     loaded one stage ahead (range-checked: rows >= R read zero) and scattered into the same image
// The small operand is gathered from the NCHW tensor through registers into LDS once per workgroup and stage — a thread owns one position for
// the whole loop and eight of the stage's sixteen reduction rows — by the offsets of the streaming kernels (SmPos / sm_tap_off: bit 31 set =
// dropped by the descriptor, reads +0.0f).  The reduction is cut over workgroups (SmPlan::nslab splits of per_slab stages); every split writes
// its own partial tile [rows][Tp], and the post-passes of the streaming regime add them in order.
typedef const __attribute__((address_space(1))) void* sm_gptr_t;
typedef __attribute__((address_space(3))) void* sm_lptr_t;
constexpr int SMT_BM = 128, SMT_BN = 128, SMT_BK = 16, SMT_NBUF = 2, SMT_SLOT = 2 * SMT_BK * SMT_BM;

template <bool FWD, int K>
__global__ void __launch_bounds__(256, 4) sm_tiled_kernel(const float* __restrict__ Wm, const float* __restrict__ X, int R, int Q, int Tp, int m_tiles,
                                                          int ksplit, int stages_per_split, int nstage, SmGeo g, float* __restrict__ part)
{
    __shared__ __attribute__((aligned(16))) float lds[SMT_NBUF * SMT_SLOT];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1, r = lane & 31, h = lane >> 5;
    const int M = FWD ? R : Q;                                // rows of the result

    // m-tiles fastest (they share the gathered operand), then the splits, then the position tiles
    const unsigned L = xcd_remap(blockIdx.x, gridDim.x);
    const int mt = L % m_tiles, ks = (L / m_tiles) % ksplit, nt = L / (m_tiles * ksplit);
    const int m0 = mt * SMT_BM, n0 = nt * SMT_BN;
    const int s_lo = ks * stages_per_split;
    const int ns = min(nstage, s_lo + stages_per_split) - s_lo;            // stages of this workgroup (>= 1)

    // ---- the small operand: this thread's position, rows jj + 8*gpar of every stage
    const int gpar = wave >> 1, gn = n0 + (tid & 127);
    const int HW = g.Ho * g.Wo;
    const __amdgpu_buffer_rsrc_t xrs = sm_rsrc(X, (unsigned)(g.P / HW) * (FWD ? g.C * g.Hf * g.Wf : R * HW) * 4u);
    const SmPos pos(g, gn);                                   // FWD: the taps of this position
    const unsigned icol = gn < g.P ? (unsigned)((gn / HW) * R * HW + gn % HW) * 4u : SM_OFF;      // DATA: the position in row 0 of `in`
    float breg[8];
    auto gather = [&](int s) {
        const unsigned row0 = (unsigned)((s_lo + s) * SMT_BK + 8 * gpar);                       // wave-uniform
#pragma unroll
        for (int jj = 0; jj < 8; ++jj)
            breg[jj] = sm_ld(xrs, FWD ? sm_tap_off<K>(g, pos, row0 + jj, 1u) : icol + (row0 + jj) * (unsigned)HW * 4u);
    };
    auto store_b = [&](int s) {
        float* bt = lds + (s & (SMT_NBUF - 1)) * SMT_SLOT + SMT_BK * SMT_BM + (tid & 127);
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) bt[(jj + 8 * gpar) * SMT_BM] = breg[jj];
    };

    // ---- the weights.  DATA: DMA pieces of two rows x 128 columns, piece q of a stage belongs to wave q % 4
    const int dma_row = lane >> 5, dma_col = (lane & 31) * 4;
    const float* wbase = Wm + (size_t)s_lo * SMT_BK * Q + m0 + dma_col;
    auto dma_piece = [&](int s, int q) {
        const int slot = (s & (SMT_NBUF - 1)) * SMT_SLOT + q * 2 * SMT_BM;
        const float* src = wbase + ((size_t)s * SMT_BK + 2 * q + dma_row) * Q;
        __builtin_amdgcn_global_load_lds((sm_gptr_t)src, (sm_lptr_t)&lds[slot], 16, 0, 0);
    };
    auto dma_stage = [&](int s) {
        dma_piece(s, wave);
        dma_piece(s, wave + 4);
    };
    // FWD: float4 i of a thread = row (tid + 256 i) / 4 of the tile, reduction steps 4 kc .. 4 kc + 3 of the stage, kc = tid % 4
    const __amdgpu_buffer_rsrc_t wrs = sm_rsrc(Wm, (unsigned)R * Q * 4u);
    const int arow = tid >> 2, akc = tid & 3;
    unsigned aoff[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int row = m0 + arow + 64 * i;
        aoff[i] = sm_off((unsigned)(min(row, R - 1) * Q + s_lo * SMT_BK + 4 * akc) * 4u, row < R);
    }
    f32x4v areg[2];
    auto load_a = [&](int s) {
#pragma unroll
        for (int i = 0; i < 2; ++i) areg[i] = sm_ld4(wrs, aoff[i] + (unsigned)(s * SMT_BK) * 4u);
    };
    auto store_a = [&](int s) {
        float* at = lds + (s & (SMT_NBUF - 1)) * SMT_SLOT + 4 * akc * SMT_BM + arow;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) at[j * SMT_BM + 64 * i] = areg[i][j];
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;

    // ---- prologue: stage 0 in LDS
    if constexpr (FWD) load_a(0);
    else dma_stage(0);
    gather(0);
    if constexpr (FWD) store_a(0);
    store_b(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();

    for (int s = 0; s < ns; ++s) {
        const int cur = s & (SMT_NBUF - 1);
        const bool more = s + 1 < ns;
        if (more) {                                           // stage s+1: lands under this stage's MFMAs
            if constexpr (FWD) load_a(s + 1);
            gather(s + 1);
        }
        const float* ta = lds + cur * SMT_SLOT + h * SMT_BM + wm * 32 + r;
        const float* tb = lds + cur * SMT_SLOT + SMT_BK * SMT_BM + h * SMT_BM + wn * 32 + r;
        float fa0[3], fa1[3], fb0[3], fb1[3];
        fa0[0] = ta[0]; fa1[0] = ta[64]; fb0[0] = tb[0]; fb1[0] = tb[64];
#pragma unroll
        for (int kk = 0; kk < SMT_BK / 2; ++kk) {
            const int cs = kk % 3, nx = (kk + 1) % 3;
            if (kk + 1 < SMT_BK / 2) {
                const int ro = (kk + 1) * 2 * SMT_BM;
                fa0[nx] = ta[ro]; fa1[nx] = ta[ro + 64]; fb0[nx] = tb[ro]; fb1[nx] = tb[ro + 64];
            }
            // DATA: this wave's two weight pieces of stage s+1, into the other slot (last read in stage s-1, before the barrier)
            if (!FWD && more && kk < 2) dma_piece(s + 1, wave + 4 * kk);
            __builtin_amdgcn_sched_barrier(0);
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa0[cs], fb0[cs], acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa0[cs], fb1[cs], acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa1[cs], fb0[cs], acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa1[cs], fb1[cs], acc[1][1], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
        // Stage s+1 must be whole in LDS before anyone crosses the barrier: the registers loaded at the top of this stage and the pieces
        // issued in its first two k-steps, a stage of MFMAs ago.  A counted wait that leaves pieces of later stages in flight is not to be
        // had here: before a store to LDS the compiler waits for every LDS DMA in flight (it cannot tell the slots apart), so a deeper ring
        // bought nothing and two slots it is.
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (more) {
            if constexpr (FWD) store_a(s + 1);
            store_b(s + 1);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
    }

    // ---- this split's partial tile: [M][Tp], lane = position column, 16 rows per sub-tile in registers (n0 + 127 < Tp)
    float* dst = part + (size_t)ks * M * Tp;
#pragma unroll
    for (int jn = 0; jn < 2; ++jn) {
        const int n = n0 + wn * 32 + jn * 64 + r;
#pragma unroll
        for (int im = 0; im < 2; ++im) {
            const int mb = m0 + wm * 32 + im * 64;            // M % 32 == 0: a sub-tile's 32 rows are inside or outside as a whole (wave-uniform)
            if (mb >= M) continue;
#pragma unroll
            for (int e = 0; e < 16; ++e) dst[(size_t)(mb + (e & 3) + 8 * (e >> 2) + 4 * h) * Tp + n] = acc[im][jn][e];
        }
    }
}

// Which form a call takes.  Gathering wins wherever it was measured on the forward / data passes (<= 32 positions in the training
// step) and on the weight gradient up to 32 positions; from 128 positions up the weight gradient's four scalar tap loads per lane
// and position pair cost more than its two pre-pass launches, and it stays staged (profiles/smallmap_stream_layers.txt).
// Debug option 3 (A/B, the bit comparison of tests/test_gpu_smallmap_stream.py): 1 = staged everywhere, 2 = gathered everywhere.
constexpr int SM_WRW_GATHER_MAX_POS = 32;
static bool sm_staged(int op, int P)
{
    const int forced = debug_option(3);
    return forced == 1 || (forced != 2 && op == 1 && P > SM_WRW_GATHER_MAX_POS);
}

// The flag bit of `op` that asks for the tiled regime (ipsr_hip.h).  It changes DATA and FWD with k = 3 | 4 from SM_TILED_MIN_POS positions up; the
// weight gradient, other kernel sizes and fewer positions (where the streams win: one position block, nothing to share) run as without it.
// Debug option 5 (A/B): the flag is ignored.
constexpr int SM_TILED = 16, SM_TILED_MIN_POS = 33;
static bool sm_tiled(int op, int flags, int k, int P)
{
    return (flags & SM_TILED) && !debug_option(5) && (op == 0 || op == 2) && (k == 3 || k == 4) && P >= SM_TILED_MIN_POS;
}

// tiled: nslab = the splits of the reduction, per_slab = 16-deep stages per split, m_tiles x ngroups = the 128 x 128 tiles
struct SmPlan { int P, Tp, Pp, Q, nb, ngroups, nslab, per_slab, m_tiles, nstage; bool tiled; size_t a_floats, b_floats, m_floats, total_bytes; };

// op 0 (DATA): in [B][R][Ho][Wo], W [R][Cq][k][k] -> out [B][Cq][Hf][Wf].   op 1 (WRW): coarse [B][R][Ho][Wo], fine [B][Cq][Hf][Wf]
// -> dW [R][Cq][k][k].   op 2 (FWD): fine [B][Cq][Hf][Wf], W -> out [B][R][Ho][Wo].   (R = the weight's first channel dimension.)
static int sm_plan(int op, int B, int R, int Cq, int Ho, int Wo, int Hf, int Wf, int k, int st, int pad, int dil, SmPlan* p)
{
    const int flags = op & ~3;
    op &= 3;
    if ((flags & ~SM_TILED) || op > 2) return fail(IPSR_ERR_INVALID, "small-map convolution: op %d", op | flags);
    if (k < 1 || k > 4 || st < 1 || st > 2 || dil < 1 || pad < 0) return fail(IPSR_ERR_UNSUPPORTED, "small-map convolution: k%d s%d p%d d%d", k, st, pad, dil);
    if (Ho != (Hf + 2 * pad - dil * (k - 1) - 1) / st + 1 || Wo != (Wf + 2 * pad - dil * (k - 1) - 1) / st + 1)
        return fail(IPSR_ERR_INVALID, "small-map convolution: %dx%d is not the output grid of %dx%d under k%d s%d p%d d%d", Ho, Wo, Hf, Wf, k, st, pad, dil);
    p->P = B * Ho * Wo;
    p->Q = Cq * k * k;
    if (p->Q % 128 != 0) return fail(IPSR_ERR_UNSUPPORTED, "small-map convolution: %d x %d taps is not a multiple of 128", Cq, k * k);
    if (R % 32 != 0) return fail(IPSR_ERR_UNSUPPORTED, "small-map convolution: %d weight rows are not a multiple of 32", R);
    if (p->P > 1024) return fail(IPSR_ERR_UNSUPPORTED, "small-map convolution: %d positions (made for <= 1024)", p->P);
    const int blocks = (p->P + 31) / 32;                           // 32-wide position blocks
    p->nb = blocks >= 4 ? 4 : (blocks == 3 ? 4 : blocks);          // 1, 2 or 4 per wave
    if (op == 0 && p->nb == 4) p->nb = 2;                          // DATA keeps 4 accumulator tiles per position block: 2 blocks fill the registers
    p->ngroups = (blocks + p->nb - 1) / p->nb;
    p->Tp = p->ngroups * p->nb * 32;
    p->Pp = (p->P + 1) & ~1;
    p->a_floats = p->b_floats = p->m_floats = 0;
    p->nslab = 1; p->per_slab = 0;
    p->m_tiles = p->nstage = 0;
    p->tiled = sm_tiled(op, flags, k, p->P);
    if (p->tiled) {
        // About 2 workgroups per CU and at least 8 stages per split (the pipeline's prologue).  What a split costs is its partial tile, written
        // and read back once: FWD's is R x Tp, small next to its reduction, and 32 splits were the best or level with it on every step shape
        // from 128 to 1024 positions; DATA's is Q x Tp, k*k times the result, and more than 4 splits lost everywhere
        // (profiles/smallmap_tiled_layers.txt, the sweep).
        const int M = op == 0 ? p->Q : R, red = op == 0 ? R : p->Q;
        p->ngroups = (p->P + SMT_BN - 1) / SMT_BN;
        p->Tp = p->ngroups * SMT_BN;
        p->m_tiles = (M + SMT_BM - 1) / SMT_BM;
        p->nstage = red / SMT_BK;
        const int tiles = p->m_tiles * p->ngroups;
        int ks = std::max(1, std::min({op == 0 ? 4 : 32, p->nstage / 8, (512 + tiles - 1) / tiles}));
        if (debug_option(6) > 0) ks = std::min(debug_option(6), p->nstage);          // A/B: a split count of the caller's
        p->per_slab = (p->nstage + ks - 1) / ks;
        p->nslab = (p->nstage + p->per_slab - 1) / p->per_slab;
        p->m_floats = (size_t)p->nslab * M * p->Tp;
        p->total_bytes = align_up(p->m_floats * 4, 256) + 768;
        return IPSR_OK;
    }
    // waves in flight ~ 1024 (one per SIMD) when the slab count allows it: a slab costs its write + its read in the post-pass, so it is
    // capped where that traffic would pass half the weight stream
    const size_t w_bytes = (size_t)R * p->Q * 4;
    if (op == 0) {
        const int qb = p->Q / 128;
        const size_t slab_bytes = (size_t)p->Q * p->Tp * 4;
        const int cap = (int)std::max<size_t>(1, w_bytes / slab_bytes);
        int ns = std::max(1, std::min({R / 64, cap, (256 + qb * p->ngroups - 1) / (qb * p->ngroups)}));
        p->per_slab = (((R + 4 * ns - 1) / (4 * ns)) + 1) & ~1;                      // rows per WAVE (even)
        p->nslab = (R + 4 * p->per_slab - 1) / (4 * p->per_slab);
        p->b_floats = (size_t)R * p->Tp;
        p->m_floats = (size_t)p->nslab * p->Q * p->Tp;
    } else if (op == 2) {
        const int rb = R / 32;
        const size_t slab_bytes = (size_t)R * p->Tp * 4;
        const int cap = (int)std::max<size_t>(1, w_bytes / slab_bytes);
        int ns = std::max(1, std::min({p->Q / 256, cap, (256 + rb * p->ngroups - 1) / (rb * p->ngroups)}));
        p->per_slab = (((p->Q + 4 * ns - 1) / (4 * ns)) + 7) & ~7;                   // columns per WAVE (multiple of 8)
        p->nslab = (p->Q + 4 * p->per_slab - 1) / (4 * p->per_slab);
        p->b_floats = (size_t)p->Q * p->Tp;
        p->m_floats = (size_t)p->nslab * R * p->Tp;
    } else {
        p->a_floats = (size_t)p->Pp * R;
        p->b_floats = (size_t)p->Pp * p->Q;
    }
    p->total_bytes = align_up(p->a_floats * 4, 256) + align_up(p->b_floats * 4, 256) + align_up(p->m_floats * 4, 256) + 256;
    return IPSR_OK;
}

size_t smallmap_ws_bytes(int op, int B, int R, int Cq, int Ho, int Wo, int Hf, int Wf, int k, int st, int pad, int dil)
{
    SmPlan p;
    if (sm_plan(op, B, R, Cq, Ho, Wo, Hf, Wf, k, st, pad, dil, &p) != IPSR_OK) return 0;
    return p.total_bytes;
}

int launch_smallmap(int op, const float* a, const float* b2, float* out, int B, int R, int Cq, int Ho, int Wo, int Hf, int Wf,
                    int k, int st_, int pad, int dil, void* ws, size_t ws_bytes, hipStream_t st)
{
    SmPlan p;
    if (int rc = sm_plan(op, B, R, Cq, Ho, Wo, Hf, Wf, k, st_, pad, dil, &p)) return rc;
    if (ws_bytes < p.total_bytes) return fail(IPSR_ERR_WORKSPACE, "small-map convolution: workspace %zu < %zu", ws_bytes, p.total_bytes);
    Carver cv(ws, ws_bytes);
    float* A = cv.take<float>(p.a_floats);
    float* Bv = cv.take<float>(p.b_floats);
    float* Mo = cv.take<float>(p.m_floats);
    // the main kernels address every operand by 32-bit byte offsets below SM_OFF
    const size_t largest = 4 * std::max({(size_t)R * p.Q, (size_t)B * Cq * Hf * Wf, (size_t)R * p.Tp, (size_t)p.Q * p.Tp, (size_t)p.Pp * p.Q});
    if (largest >= SM_OFF) return fail(IPSR_ERR_UNSUPPORTED, "small-map convolution: an operand of %zu bytes (made for < 2 GiB)", largest);
    op &= 3;
    const bool staged = sm_staged(op, p.P);
    const SmGeo g = {p.P, R, Cq, Ho, Wo, Hf, Wf, k, st_, pad, dil};
    const unsigned tgrid = (unsigned)(p.m_tiles * p.nslab * p.ngroups);
    if (op == 0) {          // a = in, b2 = W
        if (p.tiled) {
            sm_tiled_kernel<false, 4><<<tgrid, 256, 0, st>>>(b2, a, R, p.Q, p.Tp, p.m_tiles, p.nslab, p.per_slab, p.nstage, g, Mo);
            if (int rc = check_launch("sm_tiled_kernel")) return rc;
        } else {
            if (staged) sm_to_cn_kernel<<<dim3(cdiv(p.Tp, 256), R), 256, 0, st>>>(a, B, R, Ho * Wo, p.Tp, Bv);
            const float* in = staged ? Bv : a;
            const int HW = staged ? 0 : Ho * Wo;
            const dim3 grid(p.Q / 128, p.nslab, p.ngroups);
            if (p.nb == 1) sm_data_kernel<1><<<grid, 256, 0, st>>>(b2, in, R, p.Q, p.Tp, p.per_slab, p.P, HW, Mo);
            else sm_data_kernel<2><<<grid, 256, 0, st>>>(b2, in, R, p.Q, p.Tp, p.per_slab, p.P, HW, Mo);
            if (int rc = check_launch("sm_data_kernel")) return rc;
        }
        const size_t total = (size_t)B * Cq * Hf * Wf;
        const unsigned cgrid = (unsigned)((total + 255) / 256);
        const size_t slab_bytes = (size_t)p.Q * p.Tp * 4, m_bytes = slab_bytes * p.nslab;
        const bool wide = !debug_option(4) && m_bytes < SM_OFF && (k == 3 || k == 4) && p.nslab <= 8;      // debug option 4 = the looping kernel
        if (wide && k == 3) sm_col2im_wide_kernel<3, 8><<<cgrid, 256, 0, st>>>(Mo, p.nslab, (unsigned)slab_bytes, (unsigned)m_bytes, B, Cq, Hf, Wf, Ho, Wo, st_, pad, dil, p.Tp, out);
        else if (wide && p.nslab <= 4) sm_col2im_wide_kernel<4, 4><<<cgrid, 256, 0, st>>>(Mo, p.nslab, (unsigned)slab_bytes, (unsigned)m_bytes, B, Cq, Hf, Wf, Ho, Wo, st_, pad, dil, p.Tp, out);
        else if (wide) sm_col2im_wide_kernel<4, 8><<<cgrid, 256, 0, st>>>(Mo, p.nslab, (unsigned)slab_bytes, (unsigned)m_bytes, B, Cq, Hf, Wf, Ho, Wo, st_, pad, dil, p.Tp, out);
        else sm_col2im_kernel<<<cgrid, 256, 0, st>>>(Mo, p.nslab, (size_t)p.Q * p.Tp, B, Cq, Hf, Wf, Ho, Wo, k, st_, pad, dil, p.Tp, out);
        return check_launch("sm_col2im_kernel");
    }
    const int K = staged ? 0 : k;                                  // the kernels' template argument: 0 = the staged images
    if (op == 2 && p.tiled) {
        if (k == 3) sm_tiled_kernel<true, 3><<<tgrid, 256, 0, st>>>(b2, a, R, p.Q, p.Tp, p.m_tiles, p.nslab, p.per_slab, p.nstage, g, Mo);
        else sm_tiled_kernel<true, 4><<<tgrid, 256, 0, st>>>(b2, a, R, p.Q, p.Tp, p.m_tiles, p.nslab, p.per_slab, p.nstage, g, Mo);
        if (int rc = check_launch("sm_tiled_kernel")) return rc;
        const size_t total = (size_t)B * R * Ho * Wo;
        sm_sum_to_nchw_kernel<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(Mo, p.nslab, (size_t)R * p.Tp, B, R, Ho * Wo, p.Tp, out);
        return check_launch("sm_sum_to_nchw_kernel");
    }
    if (op == 2) {          // a = fine, b2 = W
        if (staged) sm_im2col_cn_kernel<<<dim3(cdiv(p.Tp, 256), p.Q), 256, 0, st>>>(a, B, Cq, Hf, Wf, Ho, Wo, k, st_, pad, dil, p.Tp, Bv);
        const float* x = staged ? Bv : a;
        const dim3 grid(R / 32, p.nslab, p.ngroups);
#define SM_FWD_K(NB)                                                                                                                                   \
    switch (K) {                                                                                                                                       \
    case 0: sm_fwd_kernel<NB, 0><<<grid, 256, 0, st>>>(b2, x, R, p.Q, p.Tp, p.per_slab, g, Mo); break;                                                 \
    case 1: sm_fwd_kernel<NB, 1><<<grid, 256, 0, st>>>(b2, x, R, p.Q, p.Tp, p.per_slab, g, Mo); break;                                                 \
    case 2: sm_fwd_kernel<NB, 2><<<grid, 256, 0, st>>>(b2, x, R, p.Q, p.Tp, p.per_slab, g, Mo); break;                                                 \
    case 3: sm_fwd_kernel<NB, 3><<<grid, 256, 0, st>>>(b2, x, R, p.Q, p.Tp, p.per_slab, g, Mo); break;                                                 \
    default: sm_fwd_kernel<NB, 4><<<grid, 256, 0, st>>>(b2, x, R, p.Q, p.Tp, p.per_slab, g, Mo); break;                                                \
    }
        if (p.nb == 1) { SM_FWD_K(1) }
        else if (p.nb == 2) { SM_FWD_K(2) }
        else { SM_FWD_K(4) }
#undef SM_FWD_K
        if (int rc = check_launch("sm_fwd_kernel")) return rc;
        const size_t total = (size_t)B * R * Ho * Wo;
        sm_sum_to_nchw_kernel<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(Mo, p.nslab, (size_t)R * p.Tp, B, R, Ho * Wo, p.Tp, out);
        return check_launch("sm_sum_to_nchw_kernel");
    }
    // op 1: a = coarse, b2 = fine
    if (staged) {
        sm_to_nc_kernel<<<dim3(cdiv(R, 256), p.Pp), 256, 0, st>>>(a, B, R, Ho * Wo, A);
        sm_im2col_nt_kernel<<<dim3(cdiv(p.Q, 256), p.Pp), 256, 0, st>>>(b2, B, Cq, Hf, Wf, Ho, Wo, k, st_, pad, dil, Bv);
    }
    const float *ct = staged ? A : a, *vt = staged ? Bv : b2;
    const dim3 grid(p.Q / 128, R / 32);
    switch (K) {
    case 0: sm_wrw_kernel<0><<<grid, 64, 0, st>>>(ct, vt, R, p.Q, p.Pp, g, out); break;
    case 1: sm_wrw_kernel<1><<<grid, 64, 0, st>>>(ct, vt, R, p.Q, p.Pp, g, out); break;
    case 2: sm_wrw_kernel<2><<<grid, 64, 0, st>>>(ct, vt, R, p.Q, p.Pp, g, out); break;
    case 3: sm_wrw_kernel<3><<<grid, 64, 0, st>>>(ct, vt, R, p.Q, p.Pp, g, out); break;
    default: sm_wrw_kernel<4><<<grid, 64, 0, st>>>(ct, vt, R, p.Q, p.Pp, g, out); break;
    }
    return check_launch("sm_wrw_kernel");
}

}  // namespace ipsr

using namespace ipsr;

extern "C" {

size_t ipsr_conv_smallmap_workspace_bytes(int op, int B, int R, int Cq, int Ho, int Wo, int Hf, int Wf, int k, int stride, int pad, int dil)
{
    if (B < 1 || R < 1 || Cq < 1 || Ho < 1 || Wo < 1 || Hf < 1 || Wf < 1) return 0;
    return smallmap_ws_bytes(op, B, R, Cq, Ho, Wo, Hf, Wf, k, stride, pad, dil);
}

int ipsr_conv_smallmap(int op, const float* a, const float* b, float* out, int B, int R, int Cq, int Ho, int Wo, int Hf, int Wf,
                       int k, int stride, int pad, int dil, void* ws, size_t ws_bytes, void* stream)
{
    if (!a || !b || !out || !ws) return fail(IPSR_ERR_INVALID, "ipsr_conv_smallmap: null pointer");
    if (B < 1 || R < 1 || Cq < 1 || Ho < 1 || Wo < 1 || Hf < 1 || Wf < 1) return fail(IPSR_ERR_INVALID, "ipsr_conv_smallmap: bad argument");
    if ((reinterpret_cast<uintptr_t>(ws) & 15u) || (reinterpret_cast<uintptr_t>(out) & 15u) || (reinterpret_cast<uintptr_t>(a) & 15u) ||
        (reinterpret_cast<uintptr_t>(b) & 15u))
        return fail(IPSR_ERR_INVALID, "ipsr_conv_smallmap: operands / workspace must be 16-byte aligned");
    return launch_smallmap(op, a, b, out, B, R, Cq, Ho, Wo, Hf, Wf, k, stride, pad, dil, ws, ws_bytes, static_cast<hipStream_t>(stream));
}

}  // extern "C"
