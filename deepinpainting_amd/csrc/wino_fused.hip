// wino_fused.hip — F(4x4, 3x3) in ONE launch for the 3x3 stride-1 pad-1 data passes that produce at most 64 channels on large maps
// (VGG conv1_2, netG's outermost up convolution, the input gradient of its outermost down convolution).  On those layers the
// three-launch path of winograd.hip spends two thirds of its time writing the transformed windows V and the products M to HBM and
// reading them back (2.25x the activations each way); here they never leave the CU:
//
//   workgroup (256 threads, one per CU) = 32 output tiles (2 tile rows x 16 tile columns of one image) x all K <= 64 produced
//   channels x all 36 points.  Per 16-channel chunk of the reduction:
//     1. every thread transforms two 6x6 windows (16 channels x 32 tiles = 512) by B^T d B into LDS, V[xi][16 c][32 t] (72 KB);
//     2. wave w multiplies for its produced channels [16w, 16w + 16): per point 8 v_mfma_f32_16x16x4_f32 (two 16-tile halves x
//        four groups of 4 channels); A = U[xi][c][k], one float per lane straight from global memory / L2 (the transformed
//        filter of WinoFilter<0>, 36 x C x 64 floats, which every workgroup reads), fetched WF_PF points ahead; B = V from LDS;
//     3. the raw windows of the next chunk are requested before the multiplies, so that their latency lies under them.
//   The 36 x 2 x 4 accumulators of a lane (288 registers) are, by the 16x16 C/D layout (column = lane & 15 = tile, row =
//   4 (lane >> 4) + register = produced channel), ALL 36 points of 8 (channel, tile) pairs: A^T M A, bias, ReLU and the 2x2
//   max-pool are register arithmetic in the lane, and 16 lanes with consecutive tile columns store 256 contiguous bytes per row.
//
// The reduction runs in a fixed order (channels ascending inside each accumulator, no atomics, no split): deterministic.  Against
// the three-launch path only the order of the channel sum differs (there: pairs of channels on the 32x32x2 MFMA); both are k-ordered
// fp32 fma chains.
//
// LDS banking: a ds_read_b32 is served in two groups of 32 lanes over 32 banks, and the B fragment of a lane group is 2 rows
// (channels) x 16 tiles.  With rows 32 floats apart both rows would sit on banks 0-15, so odd channels keep their two 16-tile
// halves swapped (column ^ 16): conflict free, and a writing wave (32 tiles of one channel per lane group) stays so too.
#include "ipsr_common.h"
#include "wino_transforms.h"

namespace ipsr {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int WF_THREADS = 256;
constexpr int WF_TROWS = 2, WF_TCOLS = 16, WF_TILES = WF_TROWS * WF_TCOLS;     // tiles of a workgroup
constexpr int WF_CK = 16;                                                      // reduction channels per chunk
constexpr int WF_KP = 64;                                                      // produced channels (rows of U), padded
constexpr int WF_PF = 4;                                                       // points the A operand is fetched ahead
constexpr int WF_LDS_BYTES = 36 * WF_CK * WF_TILES * 4;                        // 73,728
// the size rule (profiles/wino_fused_layers.txt): shapes with at least this many tiles take the fused kernel
constexpr long WF_MIN_TILES = 8192;

// the 6x6 window at (y0, x0) of plane xp, zero outside the map; nothing is read for a tile that is not `live`
template <bool VEC>
__device__ __forceinline__ void wf_load_window(const float* __restrict__ xp, bool live, int y0, int x0, int H, int Wd, float (&d)[6][6])
{
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const int yy = y0 + i;
        const bool yok = live && (unsigned)yy < (unsigned)H;
        if (VEC) {                 // Wd % 4 == 0: the inner four columns are the tile's own, 16-byte aligned and inside the map
            const float* rp = xp + (size_t)(yok ? yy : 0) * Wd;
            const float4 mid = yok ? ld4(rp, (size_t)(x0 + 1) >> 2) : make_float4(0.f, 0.f, 0.f, 0.f);
            d[i][0] = (yok && x0 >= 0) ? rp[x0] : 0.0f;
            d[i][1] = mid.x; d[i][2] = mid.y; d[i][3] = mid.z; d[i][4] = mid.w;
            d[i][5] = (yok && x0 + 5 < Wd) ? rp[x0 + 5] : 0.0f;
        } else {
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                const int xx = x0 + j;
                d[i][j] = (yok && (unsigned)xx < (unsigned)Wd) ? xp[(size_t)yy * Wd + xx] : 0.0f;
            }
        }
    }
}

// V[(xi * 16 + c) * 32 + col] = (B^T d B)[xi]
__device__ __forceinline__ void wf_transform_store(const float (&d)[6][6], float* __restrict__ Vc)
{
    float w[6][6], v[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) {                 // columns: w[:,j] = B^T d[:,j]
        const float col[6] = {d[0][j], d[1][j], d[2][j], d[3][j], d[4][j], d[5][j]};
        float o[6];
        wino_bt(col, o);
#pragma unroll
        for (int i = 0; i < 6; ++i) w[i][j] = o[i];
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {                 // rows
        wino_bt(w[i], v);
#pragma unroll
        for (int j = 0; j < 6; ++j) Vc[(i * 6 + j) * WF_CK * WF_TILES] = v[j];
    }
}

// EPI as wino_output_kernel: 0 plain; 1 = + bias[k], ReLU; 2 = + bias[k], ReLU, 2x2 max-pool (y is [B,K,H/2,W/2]; H, W even).
// VEC: Wd % 4 == 0 (x and y 16-byte aligned: the entry point checks), rows move as float4.
// grid = B * nby * nbx workgroups; block id -> (image, block row of 2 tile rows, block column of 16 tile columns).
template <int EPI, bool VEC>
__global__ void __launch_bounds__(WF_THREADS, 1) wino_fused_kernel(const float* __restrict__ x, const float* __restrict__ U, const float* __restrict__ bias,
                                                                    float* __restrict__ y, int C, int K, int H, int Wd, int TY, int TX, int nbx, int nby)
{
    extern __shared__ __attribute__((aligned(16))) float V[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    unsigned id = blockIdx.x;
    const int bx = id % nbx;
    id /= nbx;
    const int by = id % nby, b = id / nby;
    const size_t HW = (size_t)H * Wd;

    // transform role: tile tl of the block, channels tc and tc + 8 of the chunk
    const int tl = tid & 31, tc = tid >> 5;
    const int wty = WF_TROWS * by + (tl >> 4), wtx = WF_TCOLS * bx + (tl & 15);
    const bool live = wty < TY && wtx < TX;
    const int wy0 = 4 * wty - 1, wx0 = 4 * wtx - 1;
    const float* xw = x + ((size_t)b * C + tc) * HW;
    float* Vw = V + tc * WF_TILES + (tl ^ ((tc & 1) << 4));          // (tc + 8) has tc's parity: the same column for both windows

    // multiply role: A[k = lane & 15][c = lane >> 4], B[c = lane >> 4][t = lane & 15]
    const int kq = lane >> 4, ln = lane & 15;
    const float* Ua = U + (size_t)kq * WF_KP + 16 * wave + ln;
    const float* Vb0 = V + kq * WF_TILES + (ln ^ ((kq & 1) << 4));            // tile row 0 of the block (4g + kq has kq's parity)
    const float* Vb1 = V + kq * WF_TILES + ((16 + ln) ^ ((kq & 1) << 4));     // tile row 1
    const size_t uplane = (size_t)C * WF_KP;

    f32x4 acc[36][2];
#pragma unroll
    for (int xi = 0; xi < 36; ++xi)
#pragma unroll
        for (int h = 0; h < 2; ++h) acc[xi][h] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    // VEC: a chunk's raw windows are requested one chunk ahead.  Maps whose rows are no whole vectors (no layer of the nets has one)
    // fetch each window right before its transform: 72 predicated scalar loads in flight beside the accumulators would spill.
    float raw[2][6][6];
    if (VEC) {
        wf_load_window<VEC>(xw, live, wy0, wx0, H, Wd, raw[0]);
        wf_load_window<VEC>(xw + 8 * HW, live, wy0, wx0, H, Wd, raw[1]);
    }

    const int nchunk = C / WF_CK;
    for (int ch = 0; ch < nchunk; ++ch) {
        const float* Uc = Ua + (size_t)ch * WF_CK * WF_KP;
        float ua[36][4];
        // the first points' A fragments travel while the windows are transformed
#pragma unroll
        for (int xi = 0; xi < WF_PF; ++xi)
#pragma unroll
            for (int g = 0; g < 4; ++g) ua[xi][g] = Uc[xi * uplane + g * 4 * WF_KP];

        const float* xc = xw + (size_t)ch * WF_CK * HW;
        if (!VEC) wf_load_window<VEC>(xc, live, wy0, wx0, H, Wd, raw[0]);
        wf_transform_store(raw[0], Vw);
        if (!VEC) wf_load_window<VEC>(xc + 8 * HW, live, wy0, wx0, H, Wd, raw[1]);
        wf_transform_store(raw[1], Vw + 8 * WF_TILES);
        __syncthreads();

        if (VEC && ch + 1 < nchunk) {              // the next chunk's windows: in flight under the multiplies
            wf_load_window<VEC>(xc + WF_CK * HW, live, wy0, wx0, H, Wd, raw[0]);
            wf_load_window<VEC>(xc + (WF_CK + 8) * HW, live, wy0, wx0, H, Wd, raw[1]);
        }

#pragma unroll
        for (int xi = 0; xi < 36; ++xi) {
            if (xi + WF_PF < 36) {
#pragma unroll
                for (int g = 0; g < 4; ++g) ua[xi + WF_PF][g] = Uc[(xi + WF_PF) * uplane + g * 4 * WF_KP];
            }
            float vb[4][2];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                vb[g][0] = Vb0[(xi * WF_CK + 4 * g) * WF_TILES];
                vb[g][1] = Vb1[(xi * WF_CK + 4 * g) * WF_TILES];
            }
#pragma unroll
            for (int g = 0; g < 4; ++g) {          // the two halves alternate: a dependent accumulator is two issues away
                acc[xi][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(ua[xi][g], vb[g][0], acc[xi][0], 0, 0, 0);
                acc[xi][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(ua[xi][g], vb[g][1], acc[xi][1], 0, 0, 0);
            }
        }
        __syncthreads();                           // V is rewritten by the next chunk
    }

    // ---- A^T M A in the lane: accumulator register r of half h = produced channel 16 wave + 4 kq + r, tile (2 by + h, 16 bx + ln) ----
    const int tx = WF_TCOLS * bx + ln;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int ty = WF_TROWS * by + h;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int k = 16 * wave + 4 * kq + r;
            float w[4][6], o[4][4];
#pragma unroll
            for (int j = 0; j < 6; ++j) {             // columns: w[:,j] = A^T m[:,j]
                const float col[6] = {acc[j][h][r], acc[6 + j][h][r], acc[12 + j][h][r], acc[18 + j][h][r], acc[24 + j][h][r], acc[30 + j][h][r]};
                float r4[4];
                wino_at(col, r4);
#pragma unroll
                for (int i = 0; i < 4; ++i) w[i][j] = r4[i];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) wino_at(w[i], o[i]);
            if (k >= K || ty >= TY || tx >= TX) continue;
            if (EPI >= 1) {
                const float bv = bias ? bias[k] : 0.0f;
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) { const float v = o[i][j] + bv; o[i][j] = v < 0.0f ? 0.0f : v; }
            }
            if (EPI == 2) {                            // H, W even (host-checked): the 4x4 tile pools to 2x2
                const int Hh = H >> 1, Wh = Wd >> 1;
                float* yp = y + ((size_t)b * K + k) * Hh * Wh;
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    float pm[2];
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        const float a0 = o[2 * i][2 * j], a1 = o[2 * i][2 * j + 1], a2 = o[2 * i + 1][2 * j], a3 = o[2 * i + 1][2 * j + 1];
                        const float m01 = (a0 > a1 || a0 != a0) ? a0 : a1, m23 = (a2 > a3 || a2 != a2) ? a2 : a3;
                        pm[j] = (m01 > m23 || m01 != m01) ? m01 : m23;
                    }
                    const int yy = 2 * ty + i, xx = 2 * tx;
                    if (yy >= Hh) continue;
                    if (VEC) {                         // Wh even: both pooled columns exist, 8-byte aligned
                        *reinterpret_cast<float2*>(yp + (size_t)yy * Wh + xx) = make_float2(pm[0], pm[1]);
                    } else {
                        if (xx < Wh) yp[(size_t)yy * Wh + xx] = pm[0];
                        if (xx + 1 < Wh) yp[(size_t)yy * Wh + xx + 1] = pm[1];
                    }
                }
                continue;
            }
            float* yp = y + ((size_t)b * K + k) * HW;
            const int y0 = 4 * ty, x0 = 4 * tx;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (y0 + i >= H) continue;
                if (VEC) {
                    st4(yp, ((size_t)(y0 + i) * Wd + x0) >> 2, make_float4(o[i][0], o[i][1], o[i][2], o[i][3]));
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (x0 + j < Wd) yp[(size_t)(y0 + i) * Wd + x0 + j] = o[i][j];
                }
            }
        }
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
// Which calls of launch_winograd take this kernel.  Envelope: fp32 arithmetic on fp32 tensors, at most 64 produced channels, the
// reduction in whole chunks.  Inside it the size rule decides; debug option 7: 1 = never, 2 = wherever the envelope allows.
bool wino_fused_admits(int math, bool in_bf16, bool out_bf16, int B, int C, int K, int H, int W)
{
    const int opt = debug_option(7);
    if (opt == 1 || math != 0 || in_bf16 || out_bf16 || K > WF_KP || C % WF_CK != 0) return false;
    if (opt == 2) return true;
    return (long)B * ((H + 3) / 4) * ((W + 3) / 4) >= WF_MIN_TILES;
}

template <int EPI, bool VEC>
static int wf_launch(const float* x, const float* U, const float* bias, float* y, int B, int C, int K, int H, int W, hipStream_t st)
{
    const int TY = (H + 3) / 4, TX = (W + 3) / 4;
    const int nbx = cdiv(TX, WF_TCOLS), nby = cdiv(TY, WF_TROWS);
    // more dynamic LDS than the default limit: raised on every launch (the attribute is per device, a static flag would be per process)
    if (int rc = raise_dynamic_lds(reinterpret_cast<const void*>(&wino_fused_kernel<EPI, VEC>), "wino_fused_kernel", WF_LDS_BYTES)) return rc;
    wino_fused_kernel<EPI, VEC><<<(unsigned)((size_t)B * nby * nbx), WF_THREADS, WF_LDS_BYTES, st>>>(x, U, bias, y, C, K, H, W, TY, TX, nbx, nby);
    return check_launch("wino_fused_kernel");
}

// y = conv3x3(x) from the transformed filter U[36][C][64] (WinoFilter<0> with Kp = 64); the caller has checked wino_fused_admits
int launch_wino_fused(const float* x, const float* U, const float* bias, float* y, int B, int C, int K, int H, int W, int epilogue, hipStream_t st)
{
    if ((size_t)B * cdiv((H + 3) / 4, WF_TROWS) * cdiv((W + 3) / 4, WF_TCOLS) > 0x7fffffffu)
        return fail(IPSR_ERR_UNSUPPORTED, "wino_fused_kernel: too many tile blocks");
    const bool vec = (W & 3) == 0;
    if (epilogue == 2) return vec ? wf_launch<2, true>(x, U, bias, y, B, C, K, H, W, st) : wf_launch<2, false>(x, U, bias, y, B, C, K, H, W, st);
    if (epilogue == 1) return vec ? wf_launch<1, true>(x, U, bias, y, B, C, K, H, W, st) : wf_launch<1, false>(x, U, bias, y, B, C, K, H, W, st);
    return vec ? wf_launch<0, true>(x, U, bias, y, B, C, K, H, W, st) : wf_launch<0, false>(x, U, bias, y, B, C, K, H, W, st);
}

}  // namespace ipsr
