// loss_head.hip — the scalar loss heads of the training step: value AND gradients in one launch per call.
//
// The relativistic-average LSGAN loss (models/networks.py GANLoss) and the pair of L1 terms of the generator loss (models/IPSR.py)
// are a handful of means over small tensors; written as PyTorch expressions they queue ~14 element-wise / reduce launches per call in
// the forward and as many again from autograd.  Nobody reads the intermediates.  Here each head is one kernel that returns the loss
// and d loss / d input for a unit incoming gradient; the backward is then one multiply by the incoming DEVICE scalar
// (loss_grad_scale_kernel).  All sums are fp64 in a fixed order: two calls give the same bits.  No host synchronisation, no device
// state: everything runs on the caller's stream.
#include "ipsr_common.h"

namespace ipsr {

constexpr int RG_THREADS = 1024;
constexpr int RG_MAX_BLOCKS = 16;           // the step's predictions: [8,1,30,30] = 7200 numbers (netD), [8,512,4,4] = 65536 (netF)
constexpr int L1_THREADS = 256;
constexpr int L1_MAX_BLOCKS = 1024;

__device__ __forceinline__ double lh_wave_sum(double v)
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s);
    return v;
}

// Sums of the whole workgroup of two per-thread values, returned to every thread; waves folded in ascending order.
template <int THREADS>
__device__ __forceinline__ void lh_block_sum2(double& a, double& b, double (*lds)[2])
{
    a = lh_wave_sum(a);
    b = lh_wave_sum(b);
    __syncthreads();                                                     // the previous round's readers are done
    if ((threadIdx.x & 63) == 0) { lds[threadIdx.x >> 6][0] = a; lds[threadIdx.x >> 6][1] = b; }
    __syncthreads();
    a = 0.0; b = 0.0;
#pragma unroll
    for (int w = 0; w < THREADS / 64; ++w) { a += lds[w][0]; b += lds[w][1]; }
}

// loss = 1/2 [ mean((real - mf - s)^2) + mean((fake - mr + s)^2) ],  mf = mean(fake), mr = mean(real)
// d/d real_i = [(real_i - mf - s) - (mf - mr + s)] / n_real        d/d fake_j = [(fake_j - mr + s) - (mr - mf - s)] / n_fake
// (the second term is the path through the other side's mean).  Everything in fp64, rounded once on the way out.
//
// One launch of 1 .. RG_MAX_BLOCKS workgroups with no traffic between them: EVERY workgroup sums both inputs whole (the same loads in
// the same order: the same bits everywhere), then writes its own share of the gradients; workgroup 0 also writes the loss.  A
// workgroup streams from the L2 at ~150 GB/s, so the redundant pass costs what the first pass of a single workgroup would, and the
// gradient pass is cut nb ways: measured in the training step, one workgroup took 11.6 us on netD's [8,1,30,30] predictions and
// 68 us on netF's [8,512,4,4].  The loss comes from the moments of that first pass, taken about each input's first element so that
// nothing cancels when the values cluster far from zero:  sum (x - c)^2 = Q - 2 (c - x0) S + n (c - x0)^2  with
// S = sum (x - x0), Q = sum (x - x0)^2.
__device__ __forceinline__ void rg_moments(const float* __restrict__ x, int n, int vec, double x0, double& S, double& Q)
{
    const int n4 = vec ? n >> 2 : 0;
#pragma unroll 4
    for (size_t i = threadIdx.x; i < (size_t)n4; i += RG_THREADS) {
        const float4 v = reinterpret_cast<const float4*>(x)[i];
        const double d0 = (double)v.x - x0, d1 = (double)v.y - x0, d2 = (double)v.z - x0, d3 = (double)v.w - x0;
        S += d0; S += d1; S += d2; S += d3;
        Q += d0 * d0; Q += d1 * d1; Q += d2 * d2; Q += d3 * d3;
    }
    for (size_t i = (size_t)4 * n4 + threadIdx.x; i < (size_t)n; i += RG_THREADS) {
        const double d = (double)x[i] - x0;
        S += d; Q += d * d;
    }
}

// g[i] = (x[i] - sub + add) * inv over this workgroup's share of the elements
__device__ __forceinline__ void rg_gradient(const float* __restrict__ x, int n, int vec, double sub, double add, double inv, float* __restrict__ g)
{
    const size_t first = (size_t)blockIdx.x * RG_THREADS + threadIdx.x, stride = (size_t)gridDim.x * RG_THREADS;
    const int n4 = vec ? n >> 2 : 0;
    for (size_t i = first; i < (size_t)n4; i += stride) {
        const float4 v = reinterpret_cast<const float4*>(x)[i];
        float4 o;
        o.x = (float)(((double)v.x - sub + add) * inv); o.y = (float)(((double)v.y - sub + add) * inv);
        o.z = (float)(((double)v.z - sub + add) * inv); o.w = (float)(((double)v.w - sub + add) * inv);
        reinterpret_cast<float4*>(g)[i] = o;
    }
    for (size_t i = (size_t)4 * n4 + first; i < (size_t)n; i += stride) g[i] = (float)(((double)x[i] - sub + add) * inv);
}

__global__ void __launch_bounds__(RG_THREADS) ragan_loss_kernel(const float* __restrict__ fake, int n_fake, int vec_fake, const float* __restrict__ real,
                                                                int n_real, int vec_real, float s, float* __restrict__ loss,
                                                                float* __restrict__ grad_fake, float* __restrict__ grad_real)
{
    __shared__ double lds[RG_THREADS / 64][2];
    const double f0 = (double)fake[0], r0 = (double)real[0], sd = (double)s;
    double Sf = 0.0, Qf = 0.0, Sr = 0.0, Qr = 0.0;
    rg_moments(fake, n_fake, vec_fake, f0, Sf, Qf);
    rg_moments(real, n_real, vec_real, r0, Sr, Qr);
    lh_block_sum2<RG_THREADS>(Sf, Sr, lds);
    lh_block_sum2<RG_THREADS>(Qf, Qr, lds);
    const double inv_f = 1.0 / n_fake, inv_r = 1.0 / n_real;
    const double mf = f0 + Sf * inv_f, mr = r0 + Sr * inv_r;
    const double cross = mf - mr + sd;                                   // = mean(fake - mr + s) = -mean(real - mf - s)
    // real_i - mf - s - cross  and  fake_j - mr + s + cross
    if (grad_real) rg_gradient(real, n_real, vec_real, mf + sd, -cross, inv_r, grad_real);
    if (grad_fake) rg_gradient(fake, n_fake, vec_fake, mr - sd, cross, inv_f, grad_fake);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const double cr = mf + sd - r0, cf = mr - sd - f0;
        const double a = (Qr - 2.0 * cr * Sr) * inv_r + cr * cr, b = (Qf - 2.0 * cf * Sf) * inv_f + cf * cf;
        *loss = (float)(0.5 * (a + b));
    }
}

// One pass over a1, a2 and their shared target t: block partials of sum|a1 - t| + sum|a2 - t| (fp64; the difference itself is exact in
// fp64), and g = gconst * sign(a - t) for each (sign(0) = 0, a NaN stays a NaN).  `vec`: all pointers 16-byte aligned -> float4
// accesses over the first n / 4 * 4 elements; the last block's first threads take the 0 .. 3 left over.
__device__ __forceinline__ float l1_term(float a, float t, float gconst, double& acc)
{
    const double d = (double)a - (double)t;
    acc += fabs(d);
    return d != d ? (float)d : (a > t ? gconst : (a < t ? -gconst : 0.0f));
}

__global__ void __launch_bounds__(L1_THREADS) l1_pair_kernel(const float* __restrict__ a1, const float* __restrict__ a2, const float* __restrict__ t,
                                                             int n, int vec, float gconst, float* __restrict__ g1, float* __restrict__ g2,
                                                             double* __restrict__ partial)
{
    __shared__ double lds[L1_THREADS / 64][2];
    double s1 = 0.0, s2 = 0.0;
    const int stride = gridDim.x * L1_THREADS;
    const int first = blockIdx.x * L1_THREADS + threadIdx.x;
    const int n4 = vec ? n >> 2 : 0;
    for (size_t i = first; i < (size_t)n4; i += stride) {
        const float4 tv = reinterpret_cast<const float4*>(t)[i];
        const float4 x = reinterpret_cast<const float4*>(a1)[i];
        const float4 y = reinterpret_cast<const float4*>(a2)[i];
        float4 gx, gy;
        gx.x = l1_term(x.x, tv.x, gconst, s1); gx.y = l1_term(x.y, tv.y, gconst, s1);
        gx.z = l1_term(x.z, tv.z, gconst, s1); gx.w = l1_term(x.w, tv.w, gconst, s1);
        gy.x = l1_term(y.x, tv.x, gconst, s2); gy.y = l1_term(y.y, tv.y, gconst, s2);
        gy.z = l1_term(y.z, tv.z, gconst, s2); gy.w = l1_term(y.w, tv.w, gconst, s2);
        if (g1) reinterpret_cast<float4*>(g1)[i] = gx;
        if (g2) reinterpret_cast<float4*>(g2)[i] = gy;
    }
    // scalar elements: everything when !vec (grid-stride), else the tail [4 n4, n) on the last block
    const int lo = 4 * n4;
    const int sfirst = vec ? (blockIdx.x == gridDim.x - 1 ? lo + (int)threadIdx.x : n) : first;
    const int sstride = vec ? L1_THREADS : stride;
    for (size_t i = sfirst; i < (size_t)n; i += sstride) {
        const float gx = l1_term(a1[i], t[i], gconst, s1);
        const float gy = l1_term(a2[i], t[i], gconst, s2);
        if (g1) g1[i] = gx;
        if (g2) g2[i] = gy;
    }
    lh_block_sum2<L1_THREADS>(s1, s2, lds);
    if (threadIdx.x == 0) partial[blockIdx.x] = s1 + s2;
}

__global__ void __launch_bounds__(256) l1_pair_final_kernel(const double* __restrict__ partial, int nblocks, double scale_over_n, float* __restrict__ loss)
{
    __shared__ double lds[4][2];
    double acc = 0.0, unused = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += 256) acc += partial[i];
    lh_block_sum2<256>(acc, unused, lds);
    if (threadIdx.x == 0) *loss = (float)(acc * scale_over_n);
}

// out = g * (*gscale) for up to two saved gradients in one launch (blockIdx.y picks the tensor).
__global__ void __launch_bounds__(256) loss_grad_scale_kernel(const float* __restrict__ gscale, const float* __restrict__ g1, float* __restrict__ o1, int n1,
                                                              int vec1, const float* __restrict__ g2, float* __restrict__ o2, int n2, int vec2)
{
    const float sc = *gscale;
    const float* g = blockIdx.y ? g2 : g1;
    float* o = blockIdx.y ? o2 : o1;
    const int n = blockIdx.y ? n2 : n1, vec = blockIdx.y ? vec2 : vec1;
    const int stride = gridDim.x * 256;
    const int first = blockIdx.x * 256 + threadIdx.x;
    const int n4 = vec ? n >> 2 : 0;
    for (size_t i = first; i < (size_t)n4; i += stride) {
        float4 v = reinterpret_cast<const float4*>(g)[i];
        v.x *= sc; v.y *= sc; v.z *= sc; v.w *= sc;
        reinterpret_cast<float4*>(o)[i] = v;
    }
    for (size_t i = (size_t)4 * n4 + first; i < (size_t)n; i += stride) o[i] = g[i] * sc;
}

static inline bool lh_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// workgroups of 256 threads for n elements: two float4 per thread before another workgroup pays, at most `cap`
static int lh_blocks(int n, int cap)
{
    const long long nb = ((long long)n + 2047) / 2048;
    return nb < 1 ? 1 : (nb > cap ? cap : (int)nb);
}
static int l1_pair_blocks(int n) { return lh_blocks(n, L1_MAX_BLOCKS); }

}  // namespace ipsr

using namespace ipsr;

extern "C" {

int ipsr_ragan_loss(const float* fake, int n_fake, const float* real, int n_real, float s, float* loss, float* grad_fake, float* grad_real, void* stream)
{
    if (!fake || !real || !loss) return fail(IPSR_ERR_INVALID, "ipsr_ragan_loss: null pointer");
    if (n_fake < 1 || n_real < 1) return fail(IPSR_ERR_INVALID, "ipsr_ragan_loss: bad size n_fake=%d n_real=%d", n_fake, n_real);
    // a workgroup per 4096 elements of the larger input, at most RG_MAX_BLOCKS: more would only repeat the first pass more often
    const long long want = ((long long)(n_fake > n_real ? n_fake : n_real) + 4095) / 4096;
    const int nb = want > RG_MAX_BLOCKS ? RG_MAX_BLOCKS : (int)want;
    const int vec_fake = lh_aligned16(fake) && (!grad_fake || lh_aligned16(grad_fake));
    const int vec_real = lh_aligned16(real) && (!grad_real || lh_aligned16(grad_real));
    ragan_loss_kernel<<<nb, RG_THREADS, 0, static_cast<hipStream_t>(stream)>>>(fake, n_fake, vec_fake, real, n_real, vec_real, s, loss, grad_fake,
                                                                               grad_real);
    return check_launch("ragan_loss_kernel");
}

size_t ipsr_l1_pair_loss_workspace_bytes(int n)
{
    if (n < 1) { set_error("ipsr_l1_pair_loss_workspace_bytes: bad size n=%d", n); return 0; }
    return (size_t)l1_pair_blocks(n) * sizeof(double);
}

int ipsr_l1_pair_loss(const float* a1, const float* a2, const float* t, int n, float scale, float* loss, float* g1, float* g2,
                      void* ws, size_t ws_bytes, void* stream)
{
    if (!a1 || !a2 || !t || !loss || !ws) return fail(IPSR_ERR_INVALID, "ipsr_l1_pair_loss: null pointer");
    if (n < 1) return fail(IPSR_ERR_INVALID, "ipsr_l1_pair_loss: bad size n=%d", n);
    if (reinterpret_cast<uintptr_t>(ws) & 7u) return fail(IPSR_ERR_INVALID, "ipsr_l1_pair_loss: the workspace must be 8-byte aligned");
    const int nb = l1_pair_blocks(n);
    if (ws_bytes < (size_t)nb * sizeof(double)) return fail(IPSR_ERR_WORKSPACE, "ipsr_l1_pair_loss: workspace %zu < %zu", ws_bytes, (size_t)nb * sizeof(double));
    const int vec = lh_aligned16(a1) && lh_aligned16(a2) && lh_aligned16(t) && (!g1 || lh_aligned16(g1)) && (!g2 || lh_aligned16(g2));
    const hipStream_t st = static_cast<hipStream_t>(stream);
    double* partial = static_cast<double*>(ws);
    l1_pair_kernel<<<nb, L1_THREADS, 0, st>>>(a1, a2, t, n, vec, (float)((double)scale / n), g1, g2, partial);
    if (int rc = check_launch("l1_pair_kernel")) return rc;
    l1_pair_final_kernel<<<1, 256, 0, st>>>(partial, nb, (double)scale / n, loss);
    return check_launch("l1_pair_final_kernel");
}

int ipsr_loss_grad_scale(const float* gscale, const float* g1, float* out1, int n1, const float* g2, float* out2, int n2, void* stream)
{
    if (!gscale || !g1 || !out1 || (n2 > 0 && (!g2 || !out2))) return fail(IPSR_ERR_INVALID, "ipsr_loss_grad_scale: null pointer");
    if (n1 < 1 || n2 < 0) return fail(IPSR_ERR_INVALID, "ipsr_loss_grad_scale: bad size n1=%d n2=%d", n1, n2);
    const int nmax = n1 > n2 ? n1 : n2;
    const int nb = lh_blocks(nmax, 1024);
    const int vec1 = lh_aligned16(g1) && lh_aligned16(out1), vec2 = n2 > 0 && lh_aligned16(g2) && lh_aligned16(out2);
    loss_grad_scale_kernel<<<dim3(nb, n2 > 0 ? 2 : 1), 256, 0, static_cast<hipStream_t>(stream)>>>(gscale, g1, out1, n1, vec1, g2, out2, n2, vec2);
    return check_launch("loss_grad_scale_kernel");
}

}  // extern "C"
