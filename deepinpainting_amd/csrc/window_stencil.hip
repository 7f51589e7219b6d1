// window_stencil.hip — shift_sz > 1: the p x p diagonal stencil + arg-max of the window correlation, tiled through LDS.
//
//     S[k'][q'] = inv[k'] * sum_{dy,dx} R[(ky+dy)*w + kx+dx][(qy+dy)*w + qx+dx]            k' = ky*nW + kx, q' = qy*nW + qx
//
// For a fixed pair of window rows (ky, qy) all nW x nW results read exactly p square blocks of R: block dy is rows
// (ky+dy)*w + [0,w), columns (qy+dy)*w + [0,w), and inside a block the dx taps are a one-step diagonal.  The streaming kernel
// (window_corr_argmax_kernel, corr_argmax.hip) fetches every tap by a global load of its own: every element of R leaves L2 p*p
// times.  Here a workgroup owns (sample b, window row qy, a contiguous range of window rows ky); per ky it copies the p blocks
// into LDS (w*w floats each, dense: the rows of a block are w contiguous floats, hw floats apart, not 16-byte aligned when w is
// odd, hence dword LDS-DMA) and the nW inverse norms of row ky behind them, then forms the nW x nW sums from LDS.  Every element
// of R leaves L2 p times, the p*p reads per result are ds_read_b32 with the lanes along qx (consecutive addresses).
//
// Threads: tq = t % TQ runs along qx (TQ = 64, or the power of two >= nW below that), tk = t / TQ takes kx = tk, tk + TK, ...
// (TK = 256 / TQ); with nW > 64 a thread owns the columns tq, tq + 64, tq + 128 (WS_MAXQ: the envelope ends below 192).
//
// Same bits as the streaming kernel by the same expressions: acc = first ? v : acc + v over dy outer, dx inner; sv = inv[k'] * acc;
// a thread meets its candidates in ascending k' (ky outer, its kx ascending) and replaces on takes_over; the TK threads of a
// column and the k-row splits combine by `better`, the index-aware total order, so any partition of k' gives the same winner.
// Every partial carries a real candidate: a thread starts at (-inf, its first k'), and a thread with no candidate (tk >= nW)
// takes no part in the combine.  An all -inf column therefore resolves to the lowest k' of its range, k' = 0 after the merge.
//
// Two LDS buffers (the next ky's blocks are in flight while this one's are consumed: one barrier per step) where two such
// workgroups still fit a CU, one buffer and two barriers otherwise: a step is bound by the latency of its stage, and the
// workgroups sharing a CU hide it for each other (window_stencil_plan).  The partials [B][split][N'] go to the window plan's WS_RU
// slice (split <= its slice count); with split == 1 they are the merged values and no merge is launched.
#include "ipsr_common.h"

namespace ipsr {

namespace {

constexpr int WS_THREADS = 256;
constexpr int WS_MAXQ = 3;                    // columns per thread: nW <= 64 * WS_MAXQ
constexpr int WS_LDS_LIMIT = 160 * 1024;      // LDS a workgroup may have (gfx950)
constexpr int WS_MIN_KROWS = 8;               // a k-row range is at least this long (its first stage is not overlapped)
constexpr int WS_CHIP_WGS = 256;              // CUs
constexpr int WS_MAX_WGS_PER_CU = 8;          // 4 waves each

// The size rule inside the envelope (option 8 = 0): at least this many workgroup rows B * nH.  profiles/window_stencil_lds.txt: the
// tiled kernel won in every class measured, 32 x 32 and 64 x 64 maps at batch 1 (30 and 62 rows) and at batch 8 / 4, by 5 - 22 % of
// the layer forward against spreads of 0.1 - 0.8 %; nothing measured loses, so the rule admits the whole envelope
constexpr long WS_MIN_WG_ROWS = 1;

typedef const __attribute__((address_space(1))) void* ws_gptr_t;
typedef __attribute__((address_space(3))) void* ws_lptr_t;

// The blocks of window row ky (element e of the p*w*w: row r = e / w of the p*w, column j = e % w, block dy = r / w) and the
// inverse norms of its nW windows, one dword per lane straight into LDS.  `wmagic` = 2^32 / w + 1: mul-high divides by w exactly
// for e * w < 2^32.
__device__ __forceinline__ void ws_stage(float* buf, const float* __restrict__ Rq, const float* __restrict__ invb, int ky, int w, int hw,
                                         int nW, int blockwords, unsigned wmagic)
{
    const int total = blockwords + nW;
    const int lane = threadIdx.x & 63;
    for (int base = (int)(threadIdx.x & ~63u); base < total; base += WS_THREADS) {      // base: wave-uniform
        const int e = base + lane;
        if (e < total) {
            const float* src;
            if (e < blockwords) {
                const unsigned r = __umulhi((unsigned)e, wmagic), j = (unsigned)e - r * (unsigned)w, dy = __umulhi(r, wmagic);
                src = Rq + ((size_t)ky * w + r) * hw + dy * w + j;
            } else {
                src = invb + (size_t)ky * nW + (e - blockwords);
            }
            __builtin_amdgcn_global_load_lds((ws_gptr_t)src, (ws_lptr_t)&buf[base], 4, 0, 0);
        }
    }
}

// the p*p taps of one result from the staged blocks, in the streaming kernel's order (dy outer, dx inner, the first tap copied)
template <int P>
__device__ __forceinline__ float ws_taps(const float* tap, int w, int p)
{
    float acc = 0.0f;
    bool first = true;
    if constexpr (P > 0) {
#pragma unroll
        for (int dy = 0; dy < P; ++dy)
#pragma unroll
            for (int dx = 0; dx < P; ++dx) {
                const float v = tap[dy * w * w + dx * w + dx];
                acc = first ? v : acc + v;
                first = false;
            }
    } else {
        for (int dy = 0; dy < p; ++dy)
            for (int dx = 0; dx < p; ++dx) {
                const float v = tap[dy * w * w + dx * w + dx];
                acc = first ? v : acc + v;
                first = false;
            }
    }
    return acc;
}

// P = the patch size (0: any, from `patch`); NQ = columns per thread, cdiv(nW, 64).  Workgroup ids pass through xcd_remap with qy
// running fastest: the workgroups of neighbouring qy (same sample, same range of ky) share an L2, and what (ky, qy) staged as
// block dy is block dy - 1 of (ky + 1, qy + 1) one step later.
template <int P, int NQ>
__global__ void __launch_bounds__(WS_THREADS) window_stencil_lds_kernel(const float* __restrict__ R, const float* __restrict__ inv, int hw, int w,
                                                                        int nH, int nW, int patch, int split, int kper, int tq_log2, int nbuf,
                                                                        unsigned wmagic, float* __restrict__ pval, int32_t* __restrict__ pidx)
{
    extern __shared__ float lds[];
    const int p = P ? P : patch;
    const int wg = (int)xcd_remap(blockIdx.x, gridDim.x);
    const int qy = wg % nH, ks = (wg / nH) % split, b = wg / (nH * split);
    const int Np = nH * nW;
    const int blockwords = p * w * w, bufwords = blockwords + w;
    const int t = threadIdx.x;
    const int TQ = 1 << tq_log2, TK = WS_THREADS >> tq_log2;
    const int tq = t & (TQ - 1), tk = t >> tq_log2;
    const float* Rq = R + (size_t)b * hw * hw + (size_t)qy * w;       // column base of window row qy
    const float* invb = inv + (size_t)b * Np;
    const int ky_lo = ks * kper, ky_hi = min(nH, ky_lo + kper);

    float best[NQ];
    int bidx[NQ], qoff[NQ];
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
        best[j] = -INFINITY;
        bidx[j] = ky_lo * nW + tk;
        qoff[j] = min(tq + 64 * j, nW - 1);          // a column past nW repeats the last one (in bounds, never written out)
    }

    ws_stage(lds, Rq, invb, ky_lo, w, hw, nW, blockwords, wmagic);
    for (int ky = ky_lo; ky < ky_hi; ++ky) {
        float* cur = lds + (nbuf == 2 ? ((ky - ky_lo) & 1) * bufwords : 0);
        // the blocks of ky have landed; everybody is done with the other buffer (read in the step before)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (nbuf == 2 && ky + 1 < ky_hi) ws_stage(lds + (((ky - ky_lo) & 1) ^ 1) * bufwords, Rq, invb, ky + 1, w, hw, nW, blockwords, wmagic);
        const float* sinv = cur + blockwords;
#pragma unroll 4
        for (int kx = tk; kx < nW; kx += TK) {
            const float ik = sinv[kx];
            const int k = ky * nW + kx;
#pragma unroll
            for (int j = 0; j < NQ; ++j) {
                const float sv = ik * ws_taps<P>(cur + kx * w + qoff[j], w, p);
                // as selects (v_cndmask).  Written as `if (takes_over) { ... }` under a per-column branch, the first column of this
                // loop came out of hipcc with the NaN clause computed and then dropped: tests/test_gpu_window_stencil.py, "nan_inf"
                const bool take = takes_over(sv, best[j]);
                best[j] = take ? sv : best[j];
                bidx[j] = take ? k : bidx[j];
            }
        }
        if (nbuf == 1 && ky + 1 < ky_hi) {
            __syncthreads();
            ws_stage(lds, Rq, invb, ky + 1, w, hw, nW, blockwords, wmagic);
        }
    }

    // the TK threads of a column -> one partial (the scratch lies over the buffers: everybody is done reading them)
    __syncthreads();
    float* sval = lds;
    int32_t* sidx = reinterpret_cast<int32_t*>(lds + WS_THREADS * WS_MAXQ);
#pragma unroll
    for (int j = 0; j < NQ; ++j) { sval[j * WS_THREADS + t] = best[j]; sidx[j * WS_THREADS + t] = bidx[j]; }
    __syncthreads();
    if (tk == 0) {
        const int owners = min(TK, nW);               // threads tk' < nW own at least kx = tk'
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
            const int qx = tq + 64 * j;
            if (qx < nW) {
                float v = best[j];
                int i = bidx[j];
                for (int o = 1; o < owners; ++o) {
                    const float ov = sval[j * WS_THREADS + (o << tq_log2) + tq];
                    const int oi = sidx[j * WS_THREADS + (o << tq_log2) + tq];
                    const bool take = better(ov, oi, v, i);
                    v = take ? ov : v;
                    i = take ? oi : i;
                }
                const size_t at = ((size_t)b * split + ks) * Np + (size_t)qy * nW + qx;
                pval[at] = v;
                pidx[at] = i;
            }
        }
    }
}

}  // namespace

// What launch_window_corr_argmax runs for (B, h, w, patch) under option 8; `slices` = the slice count of the window plan, which
// sizes the partials' workspace
WindowStencilPlan window_stencil_plan(int B, int h, int w, int patch, int slices)
{
    WindowStencilPlan p = {};
    const int nH = h - patch + 1, nW = w - patch + 1;
    const int opt = debug_option(8);
    const long bufwords = (long)patch * w * w + w;
    const bool envelope = patch >= 2 && bufwords * 4 <= WS_LDS_LIMIT && nW <= 64 * WS_MAXQ;
    if (opt == 1 || !envelope) return p;                                                     // variant 0: the streaming kernel
    // two buffers only where two workgroups of them still share a CU: the workgroups of a CU hide each other's stages better than a
    // workgroup hides its own (profiles/window_stencil_lds.txt: 504 against 252 workgroups at 64 x 64, p = 2)
    const int nbuf = 2 * bufwords * 4 <= WS_LDS_LIMIT / 2 ? 2 : 1;
    const int lds_bytes = (int)(max(nbuf * bufwords, (long)2 * WS_THREADS * WS_MAXQ) * 4);
    if (opt != 2 && (long)B * nH < WS_MIN_WG_ROWS) return p;
    p.lds_tiled = true;
    const int rows = B * nH, per_cu = min(WS_LDS_LIMIT / lds_bytes, WS_MAX_WGS_PER_CU);
    int split = (WS_CHIP_WGS * per_cu + rows / 2) / rows;                                    // nearest: as many workgroups as the chip holds
    split = max(1, min(min(split, nH / WS_MIN_KROWS), slices));
    p.kper = cdiv(nH, split);
    p.split = cdiv(nH, p.kper);
    p.nbuf = nbuf;
    p.lds_bytes = lds_bytes;
    p.workgroups = rows * p.split;
    return p;
}

template <int P, int NQ>
static int ws_launch(const WindowStencilPlan& p, const float* R, const float* inv, int B, int h, int w, int patch, float* pval, int32_t* pidx, hipStream_t st)
{
    const int nH = h - patch + 1, nW = w - patch + 1;
    int tq_log2 = 4;
    while ((1 << tq_log2) < nW && tq_log2 < 6) ++tq_log2;
    // more dynamic LDS than the default limit: raised on every launch (the attribute is per device, a static flag would be per process)
    if (int rc = raise_dynamic_lds(reinterpret_cast<const void*>(&window_stencil_lds_kernel<P, NQ>), "window_stencil_lds_kernel", p.lds_bytes)) return rc;
    window_stencil_lds_kernel<P, NQ><<<(unsigned)p.workgroups, WS_THREADS, p.lds_bytes, st>>>(R, inv, h * w, w, nH, nW, patch, p.split, p.kper, tq_log2, p.nbuf,
                                                                                         (unsigned)(0x100000000ull / (unsigned)w) + 1u, pval, pidx);
    return check_launch("window_stencil_lds_kernel");
}

// partials [B][p.split][N'] of the window arg-max into pval / pidx; the caller has taken p from window_stencil_plan (p.lds_tiled)
int launch_window_stencil(const WindowStencilPlan& p, const float* R, const float* inv, int B, int h, int w, int patch, float* pval, int32_t* pidx,
                          hipStream_t st)
{
#define WS_CASE(PP)                                                                                                     \
    switch (cdiv(w - patch + 1, 64)) {                                                                                 \
        case 1: return ws_launch<PP, 1>(p, R, inv, B, h, w, patch, pval, pidx, st);                                    \
        case 2: return ws_launch<PP, 2>(p, R, inv, B, h, w, patch, pval, pidx, st);                                    \
        default: return ws_launch<PP, WS_MAXQ>(p, R, inv, B, h, w, patch, pval, pidx, st);                             \
    }
    switch (patch) {
        case 2: WS_CASE(2);
        case 3: WS_CASE(3);
        case 4: WS_CASE(4);
        default: WS_CASE(0);
    }
#undef WS_CASE
}

}  // namespace ipsr
