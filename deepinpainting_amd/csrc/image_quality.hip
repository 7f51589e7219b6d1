// image_quality.hip — the evaluation path: per-image SSIM, mean (x - y)^2 and mean |x - y| of a batch, one main launch.
//
// What test.ipynb cell 3 computes per image with `IQA_pytorch.SSIM(channels=3)(real_B, fake_B, as_loss=False)` and
// `torch.mean((real_B - fake_B)**2)`, and what train.ipynb's validation loop needs of `get_loss()` (two mean absolute differences):
//     X, Y [B,C,H,W] fp32 NCHW  ->  out[b] = { mean SSIM map, mean (x - y)^2, mean |x - y| }   (float64, one row per image)
// SSIM as DESIGN.md "Image quality" defines it: an 11x11 Gaussian window `win` (sigma 1.5, rounded to float32, passed by the caller
// widened to double), depthwise, stride 1, NO padding -> (H-10) x (W-10) positions per channel;
//     mu1 = win*X, mu2 = win*Y, s1 = win*(X.X) - mu1^2, s2 = win*(Y.Y) - mu2^2, s12 = win*(X.Y) - mu1.mu2
//     cs = relu((2 s12 + C2) / (s1 + s2 + C2)),  map = ((2 mu1 mu2 + C1) / (mu1^2 + mu2^2 + C1)) . cs,   C1 = 0.01^2, C2 = 0.03^2
// and the score of an image is the mean of `map` over its C (H-10) (W-10) positions.  Values are taken as they are ([-1,1] in the
// notebooks, no rescaling): the score can be negative.
//
// Arithmetic: everything in fp64.  x.x, x.y, y.y of two floats are EXACT in fp64 (24 + 24 significant bits); the 121-tap window sums
// are fma chains in fp64 (written as fma in the source: the build's -ffp-contract=off is untouched), so a window sum carries at most
// ~121 * 2^-53 of values <= 1, and s = E[x^2] - mu^2 keeps ~1e-14 absolute against C2 = 9e-4 where fp32 loses 6e-5 on flat regions.
// The result is then within ~1e-11 of an fp64 evaluation in any tap or pixel order.  Cost: [16,3,256,256] is 1.8e9 fp64 fma.
//
// Shape of the work: one workgroup of 256 threads per (image, channel, output tile of IQ_T x IQ_T = 32 x 32 SSIM positions).
//   1. the tile's (IQ_T + 10)^2 input pixels of X and Y are read ONCE and staged in LDS as five fp64 planes x, y, xx, yy, xy (zeros
//      past the image); the same pass accumulates (x - y)^2 and |x - y| over the pixels the tile OWNS (below);
//   2. thread (tx, tg) computes the 4 positions (rows 4 tg .. 4 tg + 3, column tx) of the tile: for each window column dx it walks the
//      14 input rows once and feeds every loaded value to the up to 4 positions it belongs to (each LDS value is read 11 (4+10)/(4*11)
//      = 3.1 times fewer than position by position; a wave's 32 + 32 lanes read consecutive doubles: no bank conflicts); the 11
//      weights of the column are broadcast reads;
//   3. the three per-thread fp64 sums go through a fixed wave (shuffle) and LDS tree (as innercos.hip), one triple per workgroup into
//      the workspace; a second tiny launch folds each image's triples in a fixed order and divides by the counts.
// No atomics, no cross-workgroup traffic inside a launch; image b's result depends on nothing but image b (same grid, same order
// for every B and every position in the batch): two calls, or the image alone, give the same bits.
//
// OWNERSHIP of input pixels (the halos of neighbouring tiles overlap, the streaming sums must count every pixel exactly once):
// tile (ty, tx) of a plane, with origin (ty IQ_T, tx IQ_T), owns the input pixels of rows [ty IQ_T, (ty + 1) IQ_T) and columns
// [tx IQ_T, (tx + 1) IQ_T); the LAST tile row also owns every row from its origin to H - 1, the last tile column every column to
// W - 1.  (nty = ceil((H - 10) / IQ_T) gives (nty - 1) IQ_T + IQ_T + 10 >= H: the last tile's staged block reaches the edge.)  Every
// pixel thus belongs to exactly one tile, inside that tile's staged block.  Without the SSIM bit (IPSR_IQ_SSIM) the same kernel, grid,
// ownership and summation order run with step 2 and the halo loads left out, so the two streaming columns are bit-identical with and
// without it, and any H, W >= 1 is taken (below 11: one tile).  out[b][0] is then a quiet NaN: not computed.
#include "ipsr_common.h"

#include <limits>

namespace ipsr {

constexpr int IQ_T = 32;                    // output tile edge
constexpr int IQ_WIN = 11;                  // window edge
constexpr int IQ_IN = IQ_T + IQ_WIN - 1;    // staged block edge: 42
constexpr int IQ_THREADS = 256;
constexpr int IQ_ROWS = IQ_T * IQ_T / IQ_THREADS;   // positions per thread, consecutive rows of one column: 4
static_assert(IQ_T == 32 && IQ_ROWS * IQ_THREADS == IQ_T * IQ_T, "thread (tx, tg) = (t % 32, t / 32) covers the tile");

__device__ __forceinline__ double iq_wave_sum(double v)
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s);
    return v;
}

// the workgroup's sums of three per-thread values, valid on thread 0; waves folded in ascending order
__device__ __forceinline__ void iq_block_sum3(double& a, double& b, double& c, double (*lds)[3])
{
    a = iq_wave_sum(a); b = iq_wave_sum(b); c = iq_wave_sum(c);
    if ((threadIdx.x & 63) == 0) { lds[threadIdx.x >> 6][0] = a; lds[threadIdx.x >> 6][1] = b; lds[threadIdx.x >> 6][2] = c; }
    __syncthreads();
    a = 0.0; b = 0.0; c = 0.0;
#pragma unroll
    for (int w = 0; w < IQ_THREADS / 64; ++w) { a += lds[w][0]; b += lds[w][1]; c += lds[w][2]; }
}

struct IqPlan {
    int nty, ntx;            // tiles of a plane
    long long per_image;     // workgroups (= partial triples) per image: C * nty * ntx
};

static IqPlan iq_plan(int C, int H, int W)
{
    IqPlan p;
    p.nty = H > IQ_WIN - 1 ? cdiv(H - (IQ_WIN - 1), IQ_T) : 1;
    p.ntx = W > IQ_WIN - 1 ? cdiv(W - (IQ_WIN - 1), IQ_T) : 1;
    p.per_image = (long long)C * p.nty * p.ntx;
    return p;
}

// grid (C * nty * ntx, B).  partial[(b * gridDim.x + blockIdx.x) * 3 + {0, 1, 2}]
template <bool SSIM>
__global__ void __launch_bounds__(IQ_THREADS) image_quality_kernel(const float* __restrict__ X, const float* __restrict__ Y, int C, int H, int W,
                                                                   int nty, int ntx, const double* __restrict__ window, double* __restrict__ partial)
{
    __shared__ double pl[SSIM ? 5 : 1][SSIM ? IQ_IN * IQ_IN : 1];
    __shared__ double wl[IQ_WIN * IQ_WIN];
    __shared__ double red[IQ_THREADS / 64][3];
    const int t = threadIdx.x;
    const int tiles = nty * ntx;
    const int c = blockIdx.x / tiles, tile = blockIdx.x - c * tiles;
    const int ty = tile / ntx, tx = tile - ty * ntx;
    const int y0 = ty * IQ_T, x0 = tx * IQ_T;
    const size_t plane = ((size_t)blockIdx.y * C + c) * ((size_t)H * W);
    const bool last_y = ty == nty - 1, last_x = tx == ntx - 1;

    if (SSIM && t < IQ_WIN * IQ_WIN) wl[t] = window[t];
    double sq = 0.0, ab = 0.0;
    for (int i = t; i < IQ_IN * IQ_IN; i += IQ_THREADS) {
        const int ly = i / IQ_IN, lx = i - ly * IQ_IN;
        const int gy = y0 + ly, gx = x0 + lx;
        const bool inside = gy < H && gx < W;
        const bool owned = inside && (ly < IQ_T || last_y) && (lx < IQ_T || last_x);
        if (!SSIM && !owned) continue;                                  // the halo is only needed by the window sums
        double xv = 0.0, yv = 0.0;
        if (inside) {
            const size_t g = plane + (size_t)gy * W + gx;
            xv = (double)X[g];
            yv = (double)Y[g];
        }
        if (owned) {
            const double d = xv - yv;                                   // exact
            sq += d * d;
            ab += fabs(d);
        }
        if (SSIM) {
            pl[0][i] = xv; pl[1][i] = yv; pl[2][i] = xv * xv; pl[3][i] = yv * yv; pl[4][i] = xv * yv;     // exact products
        }
    }
    double ss = 0.0;
    if (SSIM) {
        __syncthreads();
        const int ox = t & (IQ_T - 1), oy = (t >> 5) * IQ_ROWS;
        double acc[IQ_ROWS][5];
#pragma unroll
        for (int o = 0; o < IQ_ROWS; ++o)
#pragma unroll
            for (int k = 0; k < 5; ++k) acc[o][k] = 0.0;
        for (int dx = 0; dx < IQ_WIN; ++dx) {
            double w[IQ_WIN];
#pragma unroll
            for (int dy = 0; dy < IQ_WIN; ++dy) w[dy] = wl[dy * IQ_WIN + dx];
#pragma unroll
            for (int iy = 0; iy < IQ_ROWS + IQ_WIN - 1; ++iy) {
                const int at = (oy + iy) * IQ_IN + ox + dx;             // row <= 31 + 10, column <= 31 + 10: inside the staged block
                double v[5];
#pragma unroll
                for (int k = 0; k < 5; ++k) v[k] = pl[k][at];
#pragma unroll
                for (int o = 0; o < IQ_ROWS; ++o) {
                    const int dy = iy - o;
                    if (dy >= 0 && dy < IQ_WIN) {
#pragma unroll
                        for (int k = 0; k < 5; ++k) acc[o][k] = fma(w[dy], v[k], acc[o][k]);
                    }
                }
            }
        }
        constexpr double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;
#pragma unroll
        for (int o = 0; o < IQ_ROWS; ++o) {
            if (y0 + oy + o < H - (IQ_WIN - 1) && x0 + ox < W - (IQ_WIN - 1)) {
                const double mu1 = acc[o][0], mu2 = acc[o][1];
                const double m11 = mu1 * mu1, m22 = mu2 * mu2, m12 = mu1 * mu2;
                const double s1 = acc[o][2] - m11, s2 = acc[o][3] - m22, s12 = acc[o][4] - m12;
                double cs = (2.0 * s12 + C2) / (s1 + s2 + C2);
                cs = cs < 0.0 ? 0.0 : cs;                               // relu; a NaN stays a NaN
                ss += ((2.0 * m12 + C1) / (m11 + m22 + C1)) * cs;
            }
        }
    }
    iq_block_sum3(ss, sq, ab, red);
    if (t == 0) {
        double* p = partial + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 3;
        p[0] = ss; p[1] = sq; p[2] = ab;
    }
}

// grid B: image b's triples folded in a fixed order (thread i takes i, i + 256, ...; then the wave and LDS tree), divided by the counts
__global__ void __launch_bounds__(IQ_THREADS) image_quality_final_kernel(const double* __restrict__ partial, int per_image, double n_ssim, double n_pix,
                                                                         int ssim, double* __restrict__ out)
{
    __shared__ double red[IQ_THREADS / 64][3];
    const double* p = partial + (size_t)blockIdx.x * per_image * 3;
    double a = 0.0, b = 0.0, c = 0.0;
    for (int i = threadIdx.x; i < per_image; i += IQ_THREADS) { a += p[3 * (size_t)i]; b += p[3 * (size_t)i + 1]; c += p[3 * (size_t)i + 2]; }
    iq_block_sum3(a, b, c, red);
    if (threadIdx.x == 0) {
        double* o = out + (size_t)blockIdx.x * 3;
        o[0] = ssim ? a / n_ssim : std::numeric_limits<double>::quiet_NaN();
        o[1] = b / n_pix;
        o[2] = c / n_pix;
    }
}

// every check that needs no pointer: IPSR_OK, or the status with the message set
static int iq_check_shape(const char* who, int B, int C, int H, int W, int flags, IqPlan* plan)
{
    if (B < 1 || C < 1 || H < 1 || W < 1) return fail(IPSR_ERR_INVALID, "%s: bad size B=%d C=%d H=%d W=%d", who, B, C, H, W);
    if (flags & ~IPSR_IQ_SSIM) return fail(IPSR_ERR_INVALID, "%s: unknown flag bits 0x%x", who, flags & ~IPSR_IQ_SSIM);
    if ((flags & IPSR_IQ_SSIM) && (H < IQ_WIN || W < IQ_WIN))
        return fail(IPSR_ERR_UNSUPPORTED, "%s: SSIM needs H, W >= %d (11x11 window, no padding), got %dx%d", who, IQ_WIN, H, W);
    const IqPlan p = iq_plan(C, H, W);
    // grid.x = workgroups per image (an int in the kernels), grid.y = B
    if (p.per_image > 0x7fffffffLL || B > 65535)
        return fail(IPSR_ERR_UNSUPPORTED, "%s: grid overflow (%lld workgroups per image, limit 2^31 - 1; B=%d, limit 65535)", who, p.per_image, B);
    if (plan) *plan = p;
    return IPSR_OK;
}

}  // namespace ipsr

using namespace ipsr;

extern "C" {

size_t ipsr_image_quality_workspace_bytes(int B, int C, int H, int W, int flags)
{
    IqPlan p;
    if (iq_check_shape("ipsr_image_quality_workspace_bytes", B, C, H, W, flags, &p)) return 0;
    return (size_t)B * (size_t)p.per_image * 3 * sizeof(double);
}

int ipsr_image_quality(const float* x, const float* y, int B, int C, int H, int W, int flags, const double* window121, double* out,
                       void* ws, size_t ws_bytes, void* stream)
{
    const bool ssim = (flags & IPSR_IQ_SSIM) != 0;
    IqPlan p;
    if (int rc = iq_check_shape("ipsr_image_quality", B, C, H, W, flags, &p)) return rc;      // the shape first: ops reports a refused shape by it
    if (!x || !y || !out || !ws || (ssim && !window121)) return fail(IPSR_ERR_INVALID, "ipsr_image_quality: null pointer");
    if (reinterpret_cast<uintptr_t>(ws) & 7u) return fail(IPSR_ERR_INVALID, "ipsr_image_quality: the workspace must be 8-byte aligned");
    const size_t need = (size_t)B * (size_t)p.per_image * 3 * sizeof(double);
    if (ws_bytes < need) return fail(IPSR_ERR_WORKSPACE, "ipsr_image_quality: workspace %zu < %zu", ws_bytes, need);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    double* partial = static_cast<double*>(ws);
    const dim3 grid((unsigned)p.per_image, (unsigned)B);
    if (ssim)
        image_quality_kernel<true><<<grid, IQ_THREADS, 0, st>>>(x, y, C, H, W, p.nty, p.ntx, window121, partial);
    else
        image_quality_kernel<false><<<grid, IQ_THREADS, 0, st>>>(x, y, C, H, W, p.nty, p.ntx, window121, partial);
    if (int rc = check_launch("image_quality_kernel")) return rc;
    const double n_pix = (double)C * (double)H * (double)W;
    const double n_ssim = ssim ? (double)C * (double)(H - (IQ_WIN - 1)) * (double)(W - (IQ_WIN - 1)) : 1.0;
    image_quality_final_kernel<<<B, IQ_THREADS, 0, st>>>(partial, (int)p.per_image, n_ssim, n_pix, ssim ? 1 : 0, out);
    return check_launch("image_quality_final_kernel");
}

}  // extern "C"
