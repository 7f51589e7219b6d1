// conv_bf16.hip — direct bf16 implicit-GEMM convolutions on v_mfma_f32_32x32x16_bf16, NCHW in and out, no layout passes.
//
// BASELINE config 5 ("256x256 bf16 mixed precision: CDNA4 bf16 MFMA for patch-corr + convs") runs the conv stacks of the four nets
// and of VGG16 (models/networks.py:220-259, 404-432, 470-495, 510-515; models/vgg16.py:9-21) on bf16 activations.  The split-bf16
// Winograd engines (winograd.hip) only win on the >= 512-channel <= 32x32 layers: their transformed operands stay fp32-wide
// (4.5x the bf16 activation bytes each way).  Everything else was MIOpen's (NCHW<->NHWC transposes + ~450 TF implicit GEMMs).
// This file is the direct form for those layers: bf16 operands, fp32 accumulation, ONE launch per pass.
//
//      out[b][k][oy][ox] = sum_{c, t} Wp[k][c][t] * in[b][c][oy + dy_t][ox + dx_t]            (zero outside the image)
//
// as a GEMM  M = produced channels k,  N = pixels,  reduction = (c, t).  Forward and input gradient of Conv2d / ConvTranspose2d
// (k3 s1 p1) are all this form: only the weight re-packing differs (index strides, tap flip), as in conv_gemm.hip / winograd.hip.
//
// The MFMA wants, per lane, 8 CONSECUTIVE reduction elements: 8 channels of ONE pixel — but NCHW has a channel's pixels contiguous.
//   * weights: re-packed once per call (cast to bf16 anyway) into the image the LDS wants, [k tile][c block 16][tap][c group 2][128 k][8 c]:
//     one stage's A tile is one contiguous block, copied by LDS-DMA, fragments by ds_read_b128;
//   * activations: a stage's tile (16 channels x the tile's rows + halo rows, full image width) comes in by LDS-DMA in its natural
//     [c][row][x] form, then crosses LDS once: ds_read_b64_tr_b16 reads 4 channels x 16 pixels and hands every lane 4 channels of ONE
//     pixel, which it stores to the POSITION-major image T[c group][row][x + halo][8 c].  From T a B fragment (8 channels of pixel
//     n shifted by any tap) is one aligned ds_read_b128 whose tap shift is a constant added to the address — consecutive lanes read
//     consecutive 16-byte slots (conflict free).  The transposition costs ~2 x 16 KB of LDS traffic per stage against ~290 KB of
//     fragment reads (nine taps reuse the tile).
// Workgroup = 512 threads = 8 waves (2 x 4), tile 128 channels x 256 pixels (R = 256 / W whole image rows), a wave owns 64 x 64
// (2 x 2 MFMA tiles); stage = 16 channels x all taps; A and the raw tile double-buffered by LDS-DMA one / two stages ahead, the
// transposition of stage s+1 runs inside stage s.  L2 -> LDS traffic: A 128 x 144 x 2 B + tile ~16 KB per 256 x 128 x 288 flop.
//
// Supported: image width W in {16, 32, 64, 128} (power of two), H a multiple of 256 / W, reduction channels a multiple of 16.
// Anything else -> IPSR_ERR_UNSUPPORTED (the dispatcher leaves it where it was).
#include "ipsr_common.h"
#include <initializer_list>

namespace ipsr {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(1))) void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;
typedef __attribute__((address_space(3))) s16x4* lds_s4_t;
// LDS reads that run beside an LDS-DMA use ext-vector types: a HIP_vector_type (uint4) load is a struct copy that reaches the back end
// without alias metadata, and hipcc then drains the DMA queue (s_waitcnt vmcnt(0)) in front of it — the prefetch stops overlapping.
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

constexpr int CB_K = 128, CB_P = 256, CB_C = 16, CB_THREADS = 512, CB_MAXTAP = 9;
// per-thread loop bounds of a stage, by pixels per tile (256 / 512): transposition blocks (4 channels x 16 pixels) per 16-lane group, and
// 16-byte raw-tile chunks per thread
constexpr int cb_tr_max(int ptile) { return ptile == 256 ? 6 : 10; }
constexpr int cb_xj(int ptile) { return ptile == 256 ? 3 : 5; }
constexpr int CB_LDS_MAX = 160 * 1024;
// LDS plan (per geometry, data_geometry): A[2] | T[2] | raw[2 or 1].  A stage = ntap x 4 KB ([tap][c group][128 k][8 c] bf16), raw = [16 c][raw
// rows][input width] bf16, T = [planes][2 c groups][positions][8 c].  k3 at W <= 128: 2 x (36 + 16 + 16.3) KB; stride 2: 2 x (32 + 20 + 20.4);
// k3 at W = 256 (one image row per tile): 2 x 36 + 2 x 24.3 + ONE raw buffer of 24 KB — the transposition then follows the stage's
// multiplications instead of running beside them (`raw1`).

// The three forms (all: out = sum over (channel, tap) of packed weight x shifted input; lanes = pixels of the LANE grid Hl x Wl):
//   S1   k3 s1 p1                     lane grid = image; 9 taps; raw tile = R + 2 rows of the image, T = [cg][R + 2][W + 2]
//   F2C  k4 s2 p1, fine -> coarse     (Conv2d forward, ConvTranspose2d input gradient) lane grid = COARSE output, in(2o - 1 + r).  A stage =
//        16 channels x the 8 taps whose input ROW parity is ey: raw tile = the R + 1 fine rows of that parity (full fine width), the
//        transposition splits them into the two COLUMN phases, T = [ex][cg][R + 1][Wl + 1] — every tap a unit-stride shift again.
//   C2F  k4 s2 p1, coarse -> fine     (ConvTranspose2d forward, Conv2d input gradient) lane grid = COARSE input; a workgroup produces the
//        fine rows of ONE row parity ey' and both column parities (two accumulator sets of 2 x 2 taps each: 8 taps per stage), raw / T as
//        S1 on the coarse image; the epilogue interleaves the two column phases into whole fine rows.
//   DF2C / DC2F  k4 s2 p3 d2 (ipsr_conv4x4s2_bf16_dil; on fp32 tensors conv_bf16x3_s2_kernel below, whose header has the geometry): a channel
//        block = two sub-stages of 8 taps, each on its own R + 1 rows, ONE plane T = [cg][R + 1][Wl + 3].  DF2C: lane grid = coarse output, raw tile =
//        the R + 1 ODD fine rows of the sub-stage at full fine width, the transposition stores the odd columns only.  DC2F: lane grid = coarse
//        input, raw / T on the coarse image, one accumulator set; the epilogue writes the whole fine tile ((0, v) pairs on the odd rows, zero rows).
enum { CB_S1 = 0, CB_F2C = 1, CB_C2F = 2, CB_DF2C = 3, CB_DC2F = 4 };

struct CbGeom {
    int B, C, K;                // C reduction channels (multiple of 16), K produced channels
    int Hin, Win;               // the tensor the kernel reads
    int Hl, Wl, wshift;         // lane grid (rows, width = power of two), log2 Wl
    int Hout, Wout;             // the tensor written
    int R, NR, PW, NPOS;        // lane-grid rows per tile (ptile / Wl), raw rows, padded width, positions NR * PW per (plane, c group)
    int ymul, rowstep, yoff[2]; // input row of raw row i of sub-stage e: ymul * y0 + yoff[e] + rowstep * i
    int nsub, nphase;           // stages per channel block (F2C: 2), output row phases = workgroups per (k tile, pixel tile) (C2F: 2)
    int ntap;
    int tapoff[2][CB_MAXTAP];   // per sub-stage (F2C) / row phase (C2F): plane * 2 * NPOS + drow * PW + dcol
    int ktiles, ptiles, nstage; // ceil(K / 128), B * Hl / R, (C / 16) * nsub
    int a_bytes, t_bytes, raw_bytes, raw1;      // LDS plan: stage sizes, one raw buffer instead of two
    int kt, ptile;              // produced channels per workgroup tile: 128, or 64 when K <= 64; pixels per tile: 256, or 512 (64-row kernel)
    int nsplit, sps;            // reduction split (small maps: too few tiles to fill the chip): runs of `sps` stages, fp32 partials added by a second launch
};

// packed weights: Wp[kt][phase][cb][sub][t][cg][k & 127][c & 7] bf16 (zero for k >= K); source element (k, c, tap) at w[c * sc + k * sk + srctap]
struct CbPack { int ntap, nsub, nphase, kt; int srctap[2][2][CB_MAXTAP]; };      // kt: rows per k tile (128 or 64); srctap[phase][sub][t]

// SPLIT (the fp32-activation kernel below): two such images, hi = bf16(w) and, `lo_plane` uint4 further on, lo = bf16(w - hi) — the fp32
// residual w - hi is exact (hi keeps w's leading 8 significand bits), so hi + lo carries 16.
template <bool SPLIT>
__global__ void __launch_bounds__(256) cb_pack_weights_kernel(const float* __restrict__ w, int C, int K, long sc, long sk, CbPack pk,
                                                              uint4* __restrict__ Wp, uint4* __restrict__ zero_page, size_t lo_plane)
{
    if (blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && threadIdx.x < 4) zero_page[threadIdx.x] = make_uint4(0u, 0u, 0u, 0u);
    const int k = blockIdx.x * 256 + threadIdx.x;          // padded produced channel
    const int c8 = blockIdx.y;
    const int t = blockIdx.z % pk.ntap, ps = blockIdx.z / pk.ntap, sub = ps % pk.nsub, phase = ps / pk.nsub;
    const int ktiles = (K + pk.kt - 1) / pk.kt;
    if (k >= ktiles * pk.kt) return;
    const int tap = pk.srctap[phase][sub][t];
    unsigned short h[8], l[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int c = c8 * 8 + e;
        const float v = k < K ? w[(long)c * sc + (long)k * sk + tap] : 0.0f;
        h[e] = __builtin_bit_cast(unsigned short, (__bf16)v);
        if (SPLIT) l[e] = __builtin_bit_cast(unsigned short, (__bf16)(v - bf2f(h[e])));
    }
    uint4 o;
    o.x = h[0] | ((unsigned)h[1] << 16); o.y = h[2] | ((unsigned)h[3] << 16);
    o.z = h[4] | ((unsigned)h[5] << 16); o.w = h[6] | ((unsigned)h[7] << 16);
    const int kt = k / pk.kt, kl = k - kt * pk.kt, cb = c8 >> 1, cg = c8 & 1;
    const int ncb = C / CB_C;
    const size_t at = ((((((size_t)kt * pk.nphase + phase) * ncb + cb) * pk.nsub + sub) * pk.ntap + t) * 2 + cg) * pk.kt + kl;
    Wp[at] = o;
    if (SPLIT) {
        o.x = l[0] | ((unsigned)l[1] << 16); o.y = l[2] | ((unsigned)l[3] << 16);
        o.z = l[4] | ((unsigned)l[5] << 16); o.w = l[6] | ((unsigned)l[7] << 16);
        Wp[lo_plane + at] = o;
    }
}

// KT = produced channels per workgroup tile: 128 (waves 2 x 4, a wave 64 x 64), or 64 for layers that produce <= 64 channels (waves 1 x 8, a
// wave 64 x 32) — a 128-row tile on a 64-channel layer multiplies zeros half of the time (VGG conv1_2, the outermost U-Net levels).
template <int MODE, int KT, int P, typename TOUT>
__global__ void __launch_bounds__(CB_THREADS, 1) conv_bf16_kernel(const unsigned short* __restrict__ in, const uint4* __restrict__ Wp,
                                                                  const uint4* __restrict__ zero_page, CbGeom g, TOUT* __restrict__ out)
{
    constexpr int NTAP = MODE == CB_S1 ? 9 : 8;
    constexpr int NSET = MODE == CB_C2F ? 2 : 1;               // accumulator sets (C2F: the two column phases of the fine output)
    constexpr int TPSET = NTAP / NSET;
    constexpr bool SUB2 = MODE == CB_F2C || MODE == CB_DF2C || MODE == CB_DC2F;  // two sub-stages per channel block, each with its own input rows
    // P = pixels per tile: 256 under 128 produced channels; under 64 it is 512 where the map has the rows for it — a wave owns 64 x 64
    // either way (4 fragment reads per 4 MFMAs; on a 64 x 256 tile it is 64 x 32: 3 reads per 2 MFMAs = 192 B/clk/CU of the LDS's 256)
    static_assert((KT == 128 && P == 256) || (KT == 64 && (P == 256 || P == 512)), "tile");
    constexpr int WN = KT == 128 ? 4 : 8, NJ = P / 32 / WN;    // wave columns; 32-pixel MFMA tiles per wave
    constexpr int CB_TR_MAX = cb_tr_max(P);
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];          // 2 x (A | raw | T)
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = KT == 128 ? wave >> 2 : 0, wn = KT == 128 ? wave & 3 : wave;
    const int r = lane & 31, h = lane >> 5;

    // tile: all (k tile, row phase) workgroups of one pixel tile are neighbours (they share the activation tile in L2)
    const unsigned L = xcd_remap(blockIdx.x, gridDim.x);
    const int per_pt = g.ktiles * g.nphase * g.nsplit;
    const int pt = L / per_pt, kps = L - pt * per_pt;
    const int split = kps % g.nsplit, kp = kps / g.nsplit;
    const int kt = kp % g.ktiles, phase = kp / g.ktiles;
    const int s_lo = split * g.sps, s_hi = min(g.nstage, s_lo + g.sps);        // this workgroup's run of stages (the whole reduction unless split)
    out += (size_t)split * g.B * g.K * g.Hout * g.Wout;                         // split runs write their own fp32 partial
    const int tiles_per_img = g.Hl / g.R;
    const int b = pt / tiles_per_img, y0 = (pt - b * tiles_per_img) * g.R;

    // ---- stage-invariant addresses ------------------------------------------------------------------------------------------
    // raw tile DMA: chunk q (16 bytes = 8 pixels) = (c, row, seg), LDS image linear in q; per sub-stage its own row set
    const int segs = g.Win >> 3, nchunk = CB_C * g.NR * segs;
    constexpr int XJ = cb_xj(P);
    const unsigned short* gx[XJ][SUB2 ? 2 : 1];
    bool xlive[XJ];
#pragma unroll
    for (int j = 0; j < XJ; ++j) {
        const int q = tid + CB_THREADS * j;
        xlive[j] = q < nchunk;
        const int qq = xlive[j] ? q : 0;
        const int seg = qq % segs, row = (qq / segs) % g.NR, c = qq / (segs * g.NR);
#pragma unroll
        for (int e = 0; e < (SUB2 ? 2 : 1); ++e) {
            const int y = g.ymul * y0 + g.yoff[e] + g.rowstep * row;
            const bool inside = (unsigned)y < (unsigned)g.Hin;
            gx[j][e] = inside ? in + (((size_t)b * g.C + c) * g.Hin + y) * g.Win + seg * 8 : nullptr;
        }
    }
    const size_t xstride = (size_t)CB_C * g.Hin * g.Win;
    // A tile DMA: NTAP * 4 pieces of 1 KiB, piece = wave + 8 j; the stages of (kt, phase) are contiguous
    constexpr int NPIECE = NTAP * KT / 32, APW = (NPIECE + 7) / 8;
    const uint4* ga = Wp + ((size_t)(kt * g.nphase + phase) * g.nstage) * (NTAP * 2 * KT) + lane;
    // transposition: block u = (c quad, row, 16-pixel block); lane 4q+p of a 16-lane group supplies row q, pixels 4p..4p+3
    const int grp = tid >> 4, li = tid & 15;
    const int cb16s = g.Win >> 4, nblk = 4 * g.NR * cb16s;
    int tr_rd[CB_TR_MAX], tr_wr[CB_TR_MAX];
#pragma unroll
    for (int j = 0; j < CB_TR_MAX; ++j) {
        int u = grp + 32 * j;
        if (u >= nblk) u = nblk - 1;                       // duplicates the last block (same data to the same place): EXEC stays full
        const int cb16 = u % cb16s, row = (u / cb16s) % g.NR, cq = u / (cb16s * g.NR);
        tr_rd[j] = (((cq * 4 + (li >> 2)) * g.NR + row) * g.Win + cb16 * 16 + (li & 3) * 4) * 2;
        const int x = cb16 * 16 + li;
        int pos;
        if (MODE == CB_F2C) { const int ex = x & 1; pos = (ex * 2 + (cq >> 1)) * g.NPOS + row * g.PW + (x >> 1) + ex; }      // x = 2 j + ex; plane 1 starts at j = -1
        else if (MODE == CB_DF2C) pos = (cq >> 1) * g.NPOS + row * g.PW + (x >> 1) + 2;    // x = 2 n + 1 -> q column n at n + 2; the even x are not stored (tr_keep)
        else pos = (cq >> 1) * g.NPOS + row * g.PW + x + 1;
        tr_wr[j] = (pos * 8 + (cq & 1) * 4) * 2;
    }
    const int ntr = (nblk + 31) / 32;
    // DF2C: the raw rows carry every fine column, T takes the odd ones only: the lanes that hold an even column read (the transposing read wants
    // the whole 16-lane group) and store nothing
    const bool tr_keep = MODE != CB_DF2C || (li & 1);
    const int t_base = 2 * g.a_bytes, raw_base = t_base + 2 * g.t_bytes;
    // fragments: A rows wm*64 + {0,32} + r; B lane-grid pixels wn*64 + {0,32} + r
    const int a_off = (h * KT + wm * 64 + r) * 16;
    int b_off[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int p = wn * (32 * NJ) + j * 32 + r;
        b_off[j] = (h * g.NPOS + (p >> g.wshift) * g.PW + (p & (g.Wl - 1))) * 16;
    }

    f32x16 acc[NSET][2][NJ];
#pragma unroll
    for (int q = 0; q < NSET; ++q)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < NJ; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[q][i][j][e] = 0.0f;

    auto dma_a = [&](int buf, int stage) {
        const uint4* src = ga + (size_t)stage * (NTAP * 2 * KT);
#pragma unroll
        for (int j = 0; j < APW; ++j) {
            const int piece = wave + 8 * j;
            if (piece < NPIECE)
                __builtin_amdgcn_global_load_lds((gptr_t)(src + piece * 64), (lptr_t)(lds + buf * g.a_bytes + piece * 1024), 16, 0, 0);
        }
    };
    auto dma_x = [&](int buf, int stage) {
        const int cb = SUB2 ? stage >> 1 : stage, e = SUB2 ? stage & 1 : 0;
#pragma unroll
        for (int j = 0; j < XJ; ++j) {
            if (xlive[j]) {
                const unsigned short* base = (SUB2 && e) ? gx[j][SUB2 ? 1 : 0] : gx[j][0];
                const void* src = base ? static_cast<const void*>(base + (size_t)cb * xstride) : static_cast<const void*>(zero_page);
                __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(lds + raw_base + buf * g.raw_bytes + (wave * 64 + CB_THREADS * j) * 16), 16, 0, 0);
            }
        }
    };
    auto transpose = [&](int rbuf, int tbuf) {                 // raw[rbuf] -> T[tbuf]
        unsigned char* raw = lds + raw_base + rbuf * g.raw_bytes;
        unsigned char* T = lds + t_base + tbuf * g.t_bytes;
        s16x4 v[CB_TR_MAX];
#pragma unroll
        for (int j = 0; j < CB_TR_MAX; ++j)
            if (j < ntr) v[j] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4_t)(raw + tr_rd[j]));
#pragma unroll
        for (int j = 0; j < CB_TR_MAX; ++j)
            if (j < ntr && tr_keep) *reinterpret_cast<s16x4*>(T + tr_wr[j]) = v[j];
    };

    // both T images start as zeros: the halo columns are never written (tiles span the full image width).
    // The dilated forms keep T double-buffered like F2C (2 x 21 KB at most, DF2C at nw = 128 on the 512-pixel tile; the largest plan is 153 KB):
    // a transposition writes ALL R + 1 row slots of its buffer, the rows outside the image from the zero page, so a slot that lies outside the
    // image for one sub-stage and inside it for the other never keeps the other's row — nothing is rewritten apart from the transposition itself.
    for (int i = tid; i < 2 * (g.t_bytes / 16); i += CB_THREADS)
        *reinterpret_cast<uint4*>(lds + t_base + i * 16) = make_uint4(0u, 0u, 0u, 0u);
    // prologue: A[0], raw[0] <- stage 0; raw[1] <- stage 1 (two raw buffers)
    dma_a(0, s_lo);
    dma_x(0, s_lo);
    if (!g.raw1 && s_lo + 1 < s_hi) dma_x(1, s_lo + 1);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    transpose(0, 0);
    __syncthreads();

    for (int s = s_lo; s < s_hi; ++s) {
        const int cur = (s - s_lo) & 1, nxt = cur ^ 1;
        // The transposition goes first: hipcc drains every LDS-DMA in flight (s_waitcnt vmcnt(0)) before a ds_read_b64_tr_b16, so a
        // DMA issued ahead of it would be waited for here instead of behind the multiplications.
        if (!g.raw1 && s + 1 < s_hi) transpose(nxt, nxt);      // raw[nxt] (stage s+1) landed before the barrier that ended stage s-1
        if (s + 1 < s_hi) dma_a(nxt, s + 1);                   // A[nxt] was last read in stage s-1
        if (!g.raw1) {
            if (s + 2 < s_hi) dma_x(cur, s + 2);               // raw[cur] was transposed in stage s-1
        } else if (s + 1 < s_hi) {
            dma_x(0, s + 1);                                   // the one raw buffer was transposed at the end of stage s-1
        }
        const unsigned char* A = lds + cur * g.a_bytes + a_off;
        const unsigned char* T = lds + t_base + cur * g.t_bytes;
        const int* toff = g.tapoff[SUB2 ? (s & 1) : (MODE == CB_C2F ? phase : 0)];     // (two sub-stages: sps is even, a run starts on sub-stage 0)
        // software pipeline over the taps: the fragments of tap t + 1 are read while tap t multiplies (two register sets); the
        // sched_group_barriers pin that order — left alone the compiler issues a tap's reads right before its own multiplications and
        // every tap waits out the LDS latency (s_waitcnt lgkmcnt(0) in front of 4 MFMAs)
        bf16x8 fa[2][2], fb[2][NJ];
        auto load_tap = [&](int t, int set) {
            fa[set][0] = *reinterpret_cast<const bf16x8*>(A + (t * 2 * KT) * 16);
            fa[set][1] = *reinterpret_cast<const bf16x8*>(A + (t * 2 * KT + 32) * 16);
#pragma unroll
            for (int j = 0; j < NJ; ++j) fb[set][j] = *reinterpret_cast<const bf16x8*>(T + b_off[j] + toff[t] * 16);
        };
        load_tap(0, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 2 + NJ, 0);                              // tap 0's reads: the pipeline's fill
#pragma unroll
        for (int t = 0; t < NTAP; ++t) {
            const int q = t / TPSET, set = t & 1;
            if (t + 1 < NTAP) load_tap(t + 1, set ^ 1);
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                acc[q][0][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[set][0], fb[set][j], acc[q][0][j], 0, 0, 0);
                acc[q][1][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[set][1], fb[set][j], acc[q][1][j], 0, 0, 0);
            }
            if (t + 1 < NTAP) {
                // (with an LDS-DMA in flight hipcc only ever waits lgkmcnt(0), never a counted value: the reads must all be OLD when the next
                // tap's first multiplication asks for them, so they go right behind this tap's first one, not one per multiplication)
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                           // this tap's first MFMA
                __builtin_amdgcn_sched_group_barrier(0x100, 2 + NJ, 0);                      // the next tap's reads
                __builtin_amdgcn_sched_group_barrier(0x008, 2 * NJ - 1, 0);                  // the rest of this tap
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // this stage's DMAs are the next stage's operands
        __syncthreads();
        if (g.raw1 && s + 1 < s_hi) {                          // one raw buffer: the next stage's tile crosses LDS now, behind the multiplications
            transpose(0, nxt);
            __syncthreads();
        }
    }

    // epilogue: lane = lane-grid pixel, register = channel
    const size_t HWo = (size_t)g.Hout * g.Wout;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int p = wn * (32 * NJ) + j * 32 + r;
        const int py = y0 + (p >> g.wshift), px = p & (g.Wl - 1);
        if (MODE == CB_C2F) {
            // fine row 2 py + phase, fine columns 2 px and 2 px + 1 (the two accumulator sets): one 2-element store
            TOUT* op = out + (size_t)b * g.K * HWo + (size_t)(2 * py + phase) * g.Wout + 2 * px;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int k = kt * KT + wm * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
                    if (k < g.K) {
                        if (sizeof(TOUT) == 2) {
                            const unsigned pk = (unsigned)f2bf(acc[0][i][j][e]) | ((unsigned)f2bf(acc[NSET - 1][i][j][e]) << 16);
                            *reinterpret_cast<unsigned*>(op + (size_t)k * HWo) = pk;
                        } else {
                            *reinterpret_cast<float2*>(op + (size_t)k * HWo) = make_float2(acc[0][i][j][e], acc[NSET - 1][i][j][e]);
                        }
                    }
                }
        } else if (MODE == CB_DC2F) {
            // fine row 2 py + 1, fine columns 2 px and 2 px + 1: (0, v), one 4- / 8-byte store; the even fine rows follow below
            TOUT* op = out + (size_t)b * g.K * HWo + (size_t)(2 * py + 1) * g.Wout + 2 * px;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int k = kt * KT + wm * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
                    if (k < g.K) {
                        if (sizeof(TOUT) == 2) *reinterpret_cast<unsigned*>(op + (size_t)k * HWo) = (unsigned)f2bf(acc[0][i][j][e]) << 16;
                        else *reinterpret_cast<float2*>(op + (size_t)k * HWo) = make_float2(0.0f, acc[0][i][j][e]);
                    }
                }
        } else if (sizeof(TOUT) == 2) {
            // bf16 output: through LDS (free after the last stage's barrier) as [k][P pixels], so that the tile leaves as 16-byte rows
            // instead of 64 two-byte stores per lane
            unsigned short* L = reinterpret_cast<unsigned short*>(lds);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int kl = wm * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
                    L[kl * P + p] = f2bf(acc[0][i][j][e]);
                }
        } else {
            const bool live = py < g.Hout && px < g.Wout;      // (lane grid == output grid here)
            TOUT* op = out + (size_t)b * g.K * HWo + (size_t)py * g.Wout + px;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int k = kt * KT + wm * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
                    if (live && k < g.K) st1(op, (size_t)k * HWo, acc[0][i][j][e]);
                }
        }
    }
    if (MODE == CB_DC2F) {
        // the even fine rows 2 (y0 + i), i < R, of the tile's channels: whole rows of +0 as 16-byte vectors
        const int rchunks = g.Wout * (int)sizeof(TOUT) / 16, nz = KT * g.R * rchunks;
        for (int z = tid; z < nz; z += CB_THREADS) {
            const int seg = z % rchunks, i = (z / rchunks) % g.R, k = kt * KT + z / (rchunks * g.R);
            if (k < g.K) {
                TOUT* op = out + ((size_t)b * g.K + k) * HWo + (size_t)(2 * (y0 + i)) * g.Wout;
                reinterpret_cast<uint4*>(op)[seg] = make_uint4(0u, 0u, 0u, 0u);
            }
        }
    } else if (MODE != CB_C2F && sizeof(TOUT) == 2) {
        __syncthreads();
        const uint4* L4 = reinterpret_cast<const uint4*>(lds);
#pragma unroll
        for (int it = 0; it < KT * P * 2 / 16 / CB_THREADS; ++it) {
            const int chunk = tid + CB_THREADS * it;           // P / 8 chunks of 8 pixels per channel row
            const int kl = chunk / (P / 8), p0 = (chunk % (P / 8)) * 8;
            const int k = kt * KT + kl;
            if (k < g.K) {
                TOUT* op = out + ((size_t)b * g.K + k) * HWo + (size_t)(y0 + (p0 >> g.wshift)) * g.Wout + (p0 & (g.Wl - 1));
                *reinterpret_cast<uint4*>(op) = L4[chunk];
            }
        }
    }
}

// log2 of a lane-grid width; the planners admit powers of two from 16 up only
static int cb_wshift(int w) { return 31 - __builtin_clz((unsigned)w); }

// The run cut of the four weight-gradient planners: ONE round of one workgroup per CU — every run costs a partial slab written and read
// back (PMC, bf16 3x3 128 -> 128 @128x128: 512 runs = 151 MB each way against 134 MB of operands).  tiles = output tiles, groups = stages
// per image -> stages a workgroup reduces (a divisor of groups) and the number of runs.
static void cb_cut_runs(int tiles, int B, int groups, int* stages_per_wg, int* nsplit)
{
    int spw = (int)(((long)tiles * B * groups + 255) / 256);
    if (spw < 1) spw = 1;
    if (spw > groups) spw = groups;
    while (groups % spw) --spw;
    *stages_per_wg = spw;
    *nsplit = B * (groups / spw);
}

// dW[k][c][t] = sum_s slab[s][t][k][c], t = 0..NT-1, s ascending.  NT = 9: dW + 9 (k C + c) is only 4-byte aligned, scalar stores;
// NT = 16: four 16-byte vectors.
template <int NT>
__global__ void __launch_bounds__(256) cb_slab_reduce_kernel(const float* __restrict__ slabs, int nsplit, int K, int C, int Kp, int Cp,
                                                             float* __restrict__ dW)
{
    const int c = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y;
    if (c >= C) return;
    float o[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) o[t] = 0.0f;
    const size_t slab = (size_t)NT * Kp * Cp;
    for (int s = 0; s < nsplit; ++s)
#pragma unroll
        for (int t = 0; t < NT; ++t) o[t] += slabs[(size_t)s * slab + ((size_t)t * Kp + k) * Cp + c];
    float* d = dW + ((size_t)k * C + c) * NT;
    if constexpr (NT % 4 == 0) {
#pragma unroll
        for (int i = 0; i < NT / 4; ++i) reinterpret_cast<float4*>(d)[i] = make_float4(o[4 * i], o[4 * i + 1], o[4 * i + 2], o[4 * i + 3]);
    } else {
#pragma unroll
        for (int t = 0; t < NT; ++t) d[t] = o[t];
    }
}

// The reduction cut of the data-pass planner (data_geometry): fewer than 128 workgroups and >= 8 channel blocks -> up to four runs of whole channel
// blocks (`nsub` stages each).  wgs = workgroups without a cut -> the number of runs and the stages of a run.
static void cb_cut_reduction(int wgs, int nblocks, int nsub, int* nsplit, int* sps)
{
    int ns = 1;
    if (wgs < 128 && nblocks >= 8) ns = min(min(4, nblocks / 4), (256 + wgs - 1) / wgs);
    const int bps = (nblocks + ns - 1) / ns;              // channel blocks per run
    *nsplit = (nblocks + bps - 1) / bps;
    *sps = bps * nsub;
}

// fp32 partials of a split reduction, behind the packed weights
static size_t cb_partial_bytes(const CbGeom& g) { return g.nsplit > 1 ? align_up((size_t)g.nsplit * g.B * g.K * g.Hout * g.Wout * sizeof(float), 256) : 0; }

// out[i] = sum over the runs' partials, ascending
template <typename TOUT>
__global__ void __launch_bounds__(256) cb_split_reduce_kernel(const float* __restrict__ part, int nsplit, size_t n4, TOUT* __restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    float4 a = reinterpret_cast<const float4*>(part)[i];
    for (int sI = 1; sI < nsplit; ++sI) {
        const float4 v = reinterpret_cast<const float4*>(part)[(size_t)sI * n4 + i];
        a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
    }
    st4(out, i, a);
}

// Where a data-pass kernel writes: `out`, or under a reduction cut the runs' fp32 partials behind the `pack_bytes` of packed weights at Wp
static void* cb_run_dst(int nsplit, uint4* Wp, size_t pack_bytes, void* out)
{
    return nsplit > 1 ? reinterpret_cast<unsigned char*>(Wp) + align_up(pack_bytes, 256) : out;
}

// The tail of launch_data, behind the launch of `kernel` into cb_run_dst(): under a cut the ordered add of the partials `dst`
// into the n elements of `out` (a multiple of 4: the output width is), the profile stop, the launch check.
static int cb_launch_tail(const char* kernel, int nsplit, const void* dst, size_t n, void* out, int out_bf16, hipStream_t st, double work, double work2)
{
    if (nsplit > 1) {
        if (int rc = check_launch(kernel)) return rc;
        if (out_bf16) cb_split_reduce_kernel<bf16_t><<<(unsigned)cdiv(n / 4, 256), 256, 0, st>>>(static_cast<const float*>(dst), nsplit, n / 4, static_cast<bf16_t*>(out));
        else cb_split_reduce_kernel<float><<<(unsigned)cdiv(n / 4, 256), 256, 0, st>>>(static_cast<const float*>(dst), nsplit, n / 4, static_cast<float*>(out));
    }
    profile_mark_stop(st, 4, work, work2);
    return check_launch(nsplit > 1 ? "cb_split_reduce_kernel" : kernel);
}

// =====================================================================================================================================
// The same k3 s1 p1 form on FP32 tensors with SPLIT-bf16 operands ("direct_bf16x3", io code 2 of ipsr_conv3x3_bf16): every operand a is
// taken as hi + lo, hi = bf16(a), lo = bf16(a - hi) (round to nearest even; a - hi is exact in fp32), and every product as
// lo*hi + hi*lo + hi*hi on v_mfma_f32_32x32x16_bf16 — three MFMAs into the same fp32 accumulators, smallest terms first, lo*lo dropped.
// bf16 x bf16 is exact in fp32, so what is lost per product is lo*lo and the two residuals: <= 3 * 2^-18 |a||b|.  No transform amplifies
// it (the split-bf16 Winograd engines: ~1.4e-4 of the output scale; this: ~6e-6), there are no transform passes and no fp32-wide
// intermediates in HBM: one launch per pass, NCHW fp32 in and out.
//   * weights: the packing launch writes the image above twice (hi plane, lo plane); a stage's A tile is 2 x 18 KB, by LDS-DMA;
//   * activations: a stage's 16 channels x (R + 2 rows) x full width go global -> registers -> split -> T: a lane loads 4 pixels of each of
//     the 8 channels of a group as 16-byte vectors (32 registers in flight, issued ahead of the stage's multiplications), converts, and
//     stores 16 bytes per pixel and plane into the position-major images T[plane][c group][row][x + halo][8 c].  No raw buffer, no
//     ds_read_b64_tr_b16, no separate split pass; every tap's B fragment stays one aligned ds_read_b128 per plane.
// Workgroup = 512 threads = 8 waves (1 x 8), tile 64 channels x 256 pixels, a wave owns 64 x 32: per tap 4 A + 2 B fragment reads for
// 6 MFMAs.  LDS plan: A[2] = 2 x 36 KB (hi + lo, double-buffered) | T = ONE buffer of <= 48.4 KB (hi + lo; W = 256: 3 rows x 258 positions)
// = 120.4 KB at most.  T has one buffer at every width (two would not fit at W = 256): the registers are the second one — the loads of stage
// s + 1 fly during the multiplications of stage s, the conversion and the stores follow them between two barriers.
// Small maps: the reduction cut of the bf16 kernel (fp32 partials behind the packed weights + cb_split_reduce_kernel).
// Supported: W in {16 .. 256} a power of two, H a multiple of 256 / W, reduction channels a multiple of 16.
constexpr int CX_K = 64, CX_A_BYTES = 2 * 9 * 2 * CX_K * 16;

// This kernel's arguments: the fields of the shared plan (CbGeom, data_geometry) that it reads, packed by launch_data.  On the whole CbGeom
// the fields are no longer contiguous (a longer scalar prologue, same registers) and 7 of the step's 12 k3 passes measured 1.4 - 2.9 % slower,
// the three builds in one process on the same buffers (profiles/conv_bf16_data_refactor_ab.txt).
struct CxGeom {
    int B, C, K, H, W, wshift;
    int R, NR, PW, NPOS;        // image rows per tile, rows with halo, padded width, positions per (plane, c group)
    int ktiles, ptiles, nstage, nsplit, sps;
    int t_bytes;                // both planes
    int tapoff[9];
};

typedef float f32x4 __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(CB_THREADS, 1) conv_bf16x3_kernel(const float* __restrict__ in, const uint4* __restrict__ Wp, size_t lo_plane,
                                                                   CxGeom g, float* __restrict__ out)
{
    constexpr int KT = CX_K, NTAP = 9;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];          // A[2] | T
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;

    const unsigned L = xcd_remap(blockIdx.x, gridDim.x);
    const int per_pt = g.ktiles * g.nsplit;
    const int pt = L / per_pt, kps = L - pt * per_pt;
    const int split = kps % g.nsplit, kt = kps / g.nsplit;
    const int s_lo = split * g.sps, s_hi = min(g.nstage, s_lo + g.sps);
    out += (size_t)split * g.B * g.K * g.H * g.W;
    const int tiles_per_img = g.H / g.R;
    const int b = pt / tiles_per_img, y0 = (pt - b * tiles_per_img) * g.R;
    const size_t HW = (size_t)g.H * g.W;

    // ---- stage-invariant addresses ------------------------------------------------------------------------------------------
    // activation item = (c group, row, 4-pixel segment): at most 2 x 3 x 64 = 384 of them, one per thread
    const int segs = g.W >> 2, nitem = 2 * g.NR * segs;
    const int seg = tid % segs, row = (tid / segs) % g.NR, cg = min(tid / (segs * g.NR), 1);
    const int yin = y0 - 1 + row;
    const bool xlive = tid < nitem && (unsigned)yin < (unsigned)g.H;            // rows outside the image keep T's zeros
    const float* gx = in + (((size_t)b * g.C + cg * 8) * g.H + (xlive ? yin : 0)) * g.W + seg * 4;
    const size_t xstride = (size_t)CB_C * HW;
    const int t_base = 2 * CX_A_BYTES, t_plane = 2 * g.NPOS * 16;
    const int t_wr = t_base + (cg * g.NPOS + row * g.PW + seg * 4 + 1) * 16;
    // A tile DMA: 2 planes x 18 pieces of 1 KiB, piece = wave + 8 j
    constexpr int PPP = NTAP * KT / 32, NPIECE = 2 * PPP, APW = (NPIECE + 7) / 8;
    const uint4* ga = Wp + (size_t)kt * g.nstage * (NTAP * 2 * KT) + lane;
    const int a_off = (h * KT + r) * 16;
    const int p = wave * 32 + r;
    const int b_off = t_base + (h * g.NPOS + (p >> g.wshift) * g.PW + (p & (g.W - 1))) * 16;

    f32x16 acc[2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][e] = 0.0f;

    auto dma_a = [&](int buf, int stage) {
        const uint4* src = ga + (size_t)stage * (NTAP * 2 * KT);
#pragma unroll
        for (int j = 0; j < APW; ++j) {
            const int piece = wave + 8 * j;
            if (piece < NPIECE) {
                const uint4* s = piece < PPP ? src + piece * 64 : src + lo_plane + (piece - PPP) * 64;
                __builtin_amdgcn_global_load_lds((gptr_t)s, (lptr_t)(lds + buf * CX_A_BYTES + piece * 1024), 16, 0, 0);
            }
        }
    };
    f32x4 xr[8];
    auto load_x = [&](int stage) {
        if (xlive) {
            const float* src = gx + (size_t)stage * xstride;
#pragma unroll
            for (int c = 0; c < 8; ++c) xr[c] = *reinterpret_cast<const f32x4*>(src + (size_t)c * HW);
        }
    };
    auto split_store = [&]() {                                 // registers -> T (hi plane, lo plane)
        if (xlive) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                unsigned hi[8], lo[8];
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    const float v = xr[c][i];
                    hi[c] = __builtin_bit_cast(unsigned short, (__bf16)v);
                    lo[c] = __builtin_bit_cast(unsigned short, (__bf16)(v - __uint_as_float(hi[c] << 16)));
                }
                u32x4 vh, vl;
#pragma unroll
                for (int c = 0; c < 4; ++c) { vh[c] = hi[2 * c] | (hi[2 * c + 1] << 16); vl[c] = lo[2 * c] | (lo[2 * c + 1] << 16); }
                *reinterpret_cast<u32x4*>(lds + t_wr + i * 16) = vh;
                *reinterpret_cast<u32x4*>(lds + t_wr + t_plane + i * 16) = vl;
            }
        }
    };

    // T starts as zeros: the halo columns and the rows outside the image are never written
    for (int i = tid; i < g.t_bytes / 16; i += CB_THREADS) *reinterpret_cast<u32x4*>(lds + t_base + i * 16) = u32x4{0u, 0u, 0u, 0u};
    load_x(s_lo);
    dma_a(0, s_lo);
    __syncthreads();
    split_store();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    for (int s = s_lo; s < s_hi; ++s) {
        const int cur = (s - s_lo) & 1;
        if (s + 1 < s_hi) {
            load_x(s + 1);                                     // consumed behind this stage's multiplications
            dma_a(cur ^ 1, s + 1);                             // A[nxt] was last read in stage s-1
        }
        const unsigned char* A = lds + cur * CX_A_BYTES + a_off;
        const unsigned char* T = lds + b_off;
        // the tap pipeline of conv_bf16_kernel: the six fragments of tap t + 1 are read behind tap t's first multiplication
        bf16x8 fa[2][2][2], fb[2][2];                          // [set][plane][row tile], [set][plane]
        auto load_tap = [&](int t, int set) {
#pragma unroll
            for (int pl = 0; pl < 2; ++pl) {
                fa[set][pl][0] = *reinterpret_cast<const bf16x8*>(A + pl * (CX_A_BYTES / 2) + (t * 2 * KT) * 16);
                fa[set][pl][1] = *reinterpret_cast<const bf16x8*>(A + pl * (CX_A_BYTES / 2) + (t * 2 * KT + 32) * 16);
                fb[set][pl] = *reinterpret_cast<const bf16x8*>(T + pl * t_plane + g.tapoff[t] * 16);
            }
        };
        load_tap(0, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 6, 0);
#pragma unroll
        for (int t = 0; t < NTAP; ++t) {
            const int set = t & 1;
            if (t + 1 < NTAP) load_tap(t + 1, set ^ 1);
            // smallest terms first: lo(w) hi(x), hi(w) lo(x), hi(w) hi(x); the two row tiles alternate so that no MFMA waits for its predecessor
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[set][1][0], fb[set][0], acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[set][1][1], fb[set][0], acc[1], 0, 0, 0);
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[set][0][0], fb[set][1], acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[set][0][1], fb[set][1], acc[1], 0, 0, 0);
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[set][0][0], fb[set][0], acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[set][0][1], fb[set][0], acc[1], 0, 0, 0);
            if (t + 1 < NTAP) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x100, 6, 0);
                __builtin_amdgcn_sched_group_barrier(0x008, 5, 0);
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // this stage's DMA and loads are the next stage's operands
        __syncthreads();                                       // every wave is done reading T
        if (s + 1 < s_hi) {
            split_store();
            __syncthreads();
        }
    }

    // epilogue: lane = pixel, register = channel
    const int py = y0 + (p >> g.wshift), px = p & (g.W - 1);
    float* op = out + (size_t)b * g.K * HW + (size_t)py * g.W + px;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int k = kt * KT + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
            if (k < g.K) op[(size_t)k * HW] = acc[i][e];
        }
}

// =====================================================================================================================================
// The k4 s2 p1 forms (F2C / C2F above) on FP32 tensors with the same split-bf16 operands ("direct_bf16x3_s2", ipsr_conv4x4s2_bf16x3):
// conv_bf16x3_kernel's structure on the geometry, tap maps and source-tap tables of the bf16 stride-2 kernel (data_form, data_pack).
//   * weights: cb_pack_weights_kernel<true> writes the hi and lo planes of Wp[kt][phase][cb][sub][t][cg][64 k][8 c]; a stage's A tile is
//     2 x 16 KB by LDS-DMA, double-buffered;
//   * activations: global -> registers -> split -> T, one item (c group, input row, 4 floats) per thread, 8 channels each.
//     F2C: a stage = 16 channels x the R + 1 fine rows of ONE row parity, full fine width (up to 256 floats); the split store deals the four
//     floats of an item to the two column-phase planes, T[hi | lo][ex][cg][R + 1][nw + 1][8 c].  C2F: a stage = 16 channels x R + 2 coarse
//     rows, T[hi | lo][cg][R + 2][nw + 2][8 c]; a workgroup makes the fine rows of one parity, two accumulator sets hold the column parities
//     and a lane stores both as one 8-byte vector.
//   * T has ONE buffer, shared by the two F2C sub-stages.  A row slot outside the image for one row parity (slot 0 of the first tile under
//     the odd rows, slot R of the last tile under the even rows) lies inside it for the other, so rows outside the image are WRITTEN as
//     zeros every stage (conv_bf16x3_kernel's "they keep T's zeros" does not hold here); only the halo columns keep their initial zeros.
// Workgroup = 512 threads = 8 waves (1 x 8), tile 64 channels x 256 lane-grid pixels, a wave owns 64 x 32 (C2F: twice, the column parities):
// per tap 4 A + 2 B fragment reads for 6 MFMAs.  LDS: A[2] = 2 x 32 KB | T <= 48.5 KB (F2C at nw = 128: 8 planes x 3 rows x 129 positions).
// Small maps: the reduction cut of data_geometry (cb_cut_reduction), fp32 partials behind the packed planes, cb_split_reduce_kernel<float>.
// Supported: coarse width nw in {16, 32, 64, 128}, nh a multiple of 256 / nw, reduction channels a multiple of 16.
//
// The DILATED forms (k4 s2 p3 d2, netG's down convolution; modes 4 / 5 of ipsr_conv4x4s2_bf16x3).  y(oy, ox) reads x(2 oy - 3 + 2 r, 2 ox - 3 + 2 s):
// odd rows and odd columns only, so with q(m, n) = x(2 m + 1, 2 n + 1) the layer is the 16-tap stride-1 correlation y(oy, ox) = sum w(r, s)
// q(oy + r - 2, ox + s - 2) on the coarse grid: halo 2 in front, 1 behind.  Its input gradient is dq(m, n) = sum w(r, s) dy(m + 2 - r, n + 2 - s)
// (halo 1 / 2), dx = dq on the odd / odd positions and zero everywhere else.  Sixteen taps of A (2 x 64 KB double-buffered) do not fit
// beside T, so a channel block is two sub-stages of 8 taps, the weight-row pairs {0, 1} and {2, 3}, each on its own R + 1 rows:
//   DF2C fine -> coarse: sub-stage e reads the fine rows 2 (y0 + i + 2 e - 2) + 1, i = 0 .. R (the even rows are never loaded); an item is 4
//        floats of such a row of which the split store keeps the two ODD columns: ONE plane T[hi | lo][cg][R + 1][nw + 3], q column n at n + 2;
//        tap (ri, s) of either sub-stage = row slot + ri, position + s.
//   DC2F coarse -> fine: sub-stage e reads the coarse rows y0 + i + 1 - 2 e; T[hi | lo][cg][R + 1][nw + 3], column n at n + 1; tap (ri, s) = row
//        slot + 1 - ri, position + 3 - s.  One accumulator set; the epilogue writes the WHOLE fine tile: (0, v) pairs on the odd fine rows
//        and zero rows between them.  Under a reduction cut every run writes such a whole fine partial, so the ordered add needs nothing new.
// Both share T between the sub-stages like F2C (rows outside the image written as zeros every stage); the halo columns keep the initial zeros.
// LDS: A[2] = 2 x 32 KB | T <= 24.6 KB (nw = 128: 4 planes x 3 rows x 131 positions); items <= 384 (DF2C at nw = 128).
constexpr int C2_K = 64, C2_A_BYTES = 2 * 8 * 2 * C2_K * 16;

template <int MODE>
__global__ void __launch_bounds__(CB_THREADS, 1) conv_bf16x3_s2_kernel(const float* __restrict__ in, const uint4* __restrict__ Wp, size_t lo_plane,
                                                                      CbGeom g, float* __restrict__ out)
{
    static_assert(MODE == CB_F2C || MODE == CB_C2F || MODE == CB_DF2C || MODE == CB_DC2F, "form");
    constexpr int KT = C2_K, NTAP = 8, NSET = MODE == CB_C2F ? 2 : 1, TPSET = NTAP / NSET;
    constexpr bool SUB2 = MODE != CB_C2F;                      // two sub-stages per channel block, each with its own input rows
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];          // A[2] | T
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;

    const unsigned L = xcd_remap(blockIdx.x, gridDim.x);
    const int per_pt = g.ktiles * g.nphase * g.nsplit;
    const int pt = L / per_pt, kps = L - pt * per_pt;
    const int split = kps % g.nsplit, kp = kps / g.nsplit;
    const int kt = kp % g.ktiles, phase = kp / g.ktiles;
    const int s_lo = split * g.sps, s_hi = min(g.nstage, s_lo + g.sps);        // (two sub-stages: sps is even, a run starts on sub-stage 0)
    const size_t HWi = (size_t)g.Hin * g.Win, HWo = (size_t)g.Hout * g.Wout;
    out += (size_t)split * g.B * g.K * HWo;
    const int tiles_per_img = g.Hl / g.R;
    const int b = pt / tiles_per_img, y0 = (pt - b * tiles_per_img) * g.R;

    // ---- stage-invariant addresses ------------------------------------------------------------------------------------------
    // activation item = (c group, row slot, 4-float segment of the input row): at most 2 x 3 x 64 = 384, one per thread
    const int segs = g.Win >> 2, nitem = 2 * g.NR * segs;
    const bool item = tid < nitem;
    const int seg = tid % segs, row = (tid / segs) % g.NR, cg = min(tid / (segs * g.NR), 1);
    const int ya = g.ymul * y0 + g.yoff[0] + g.rowstep * row, yb = g.ymul * y0 + g.yoff[1] + g.rowstep * row;     // sub-stage 0 / 1 (F2C)
    const bool in_a = (unsigned)ya < (unsigned)g.Hin, in_b = (unsigned)yb < (unsigned)g.Hin;
    const float* gbase = in + ((size_t)b * g.C + cg * 8) * HWi + seg * 4;
    const float* gxa = gbase + (size_t)(in_a ? ya : 0) * g.Win;                 // a row outside the image reads row 0 and stores zeros
    const float* gxb = gbase + (size_t)(in_b ? yb : 0) * g.Win;
    const size_t xstride = (size_t)CB_C * HWi;
    const int t_base = 2 * C2_A_BYTES, t_plane = g.t_bytes / 2;
    // F2C: float i of the item is fine column 4 seg + i = 2 j + ex -> plane ex, position j + ex (plane 1 starts at j = -1)
    // DF2C: only the odd columns 4 seg + i = 2 n + 1 are kept, n = 2 seg + (i >> 1) at position n + 2
    const int t_wr = t_base + (cg * g.NPOS + row * g.PW + (MODE == CB_F2C ? 2 * seg : MODE == CB_DF2C ? 2 * seg + 2 : 4 * seg + 1)) * 16;
    const int t_ex = 2 * g.NPOS * 16;
    // A tile DMA: 2 planes x 16 pieces of 1 KiB, piece = wave + 8 j
    constexpr int PPP = NTAP * KT / 32, NPIECE = 2 * PPP, APW = NPIECE / 8;
    const uint4* ga = Wp + ((size_t)(kt * g.nphase + phase) * g.nstage) * (NTAP * 2 * KT) + lane;
    const int a_off = (h * KT + r) * 16;
    const int p = wave * 32 + r;
    const int b_off = t_base + (h * g.NPOS + (p >> g.wshift) * g.PW + (p & (g.Wl - 1))) * 16;

    f32x16 acc[NSET][2];
#pragma unroll
    for (int q = 0; q < NSET; ++q)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[q][i][e] = 0.0f;

    auto dma_a = [&](int buf, int stage) {
        const uint4* src = ga + (size_t)stage * (NTAP * 2 * KT);
#pragma unroll
        for (int j = 0; j < APW; ++j) {
            const int piece = wave + 8 * j;
            const uint4* s = piece < PPP ? src + piece * 64 : src + lo_plane + (piece - PPP) * 64;
            __builtin_amdgcn_global_load_lds((gptr_t)s, (lptr_t)(lds + buf * C2_A_BYTES + piece * 1024), 16, 0, 0);
        }
    };
    f32x4 xr[8];
    auto load_x = [&](int stage) {
        if (item) {
            const int cb = SUB2 ? stage >> 1 : stage;
            const float* src = ((SUB2 && (stage & 1)) ? gxb : gxa) + (size_t)cb * xstride;
#pragma unroll
            for (int c = 0; c < 8; ++c) xr[c] = *reinterpret_cast<const f32x4*>(src + (size_t)c * HWi);
        }
    };
    auto split_store = [&](int stage) {                        // registers -> T (hi planes, lo planes)
        if (item) {
            const bool inside = (SUB2 && (stage & 1)) ? in_b : in_a;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (MODE == CB_DF2C && !(i & 1)) continue;     // the even columns are loaded and dropped
                unsigned hi[8], lo[8];
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    const float v = inside ? xr[c][i] : 0.0f;
                    hi[c] = __builtin_bit_cast(unsigned short, (__bf16)v);
                    lo[c] = __builtin_bit_cast(unsigned short, (__bf16)(v - __uint_as_float(hi[c] << 16)));
                }
                u32x4 vh, vl;
#pragma unroll
                for (int c = 0; c < 4; ++c) { vh[c] = hi[2 * c] | (hi[2 * c + 1] << 16); vl[c] = lo[2 * c] | (lo[2 * c + 1] << 16); }
                const int at = t_wr + (MODE == CB_F2C ? (i & 1) * t_ex + ((i >> 1) + (i & 1)) * 16 : MODE == CB_DF2C ? (i >> 1) * 16 : i * 16);
                *reinterpret_cast<u32x4*>(lds + at) = vh;
                *reinterpret_cast<u32x4*>(lds + at + t_plane) = vl;
            }
        }
    };

    // T starts as zeros: the halo columns are never written
    for (int i = tid; i < g.t_bytes / 16; i += CB_THREADS) *reinterpret_cast<u32x4*>(lds + t_base + i * 16) = u32x4{0u, 0u, 0u, 0u};
    load_x(s_lo);
    dma_a(0, s_lo);
    __syncthreads();
    split_store(s_lo);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    for (int s = s_lo; s < s_hi; ++s) {
        const int cur = (s - s_lo) & 1;
        if (s + 1 < s_hi) {
            load_x(s + 1);                                     // consumed behind this stage's multiplications
            dma_a(cur ^ 1, s + 1);                             // A[nxt] was last read in stage s-1
        }
        const unsigned char* A = lds + cur * C2_A_BYTES + a_off;
        const unsigned char* T = lds + b_off;
        const int* toff = g.tapoff[SUB2 ? (s & 1) : phase];
        // the tap pipeline of conv_bf16x3_kernel: the six fragments of tap t + 1 are read behind tap t's first multiplication
        bf16x8 fa[2][2][2], fb[2][2];                          // [set][plane][row tile], [set][plane]
        auto load_tap = [&](int t, int set) {
#pragma unroll
            for (int pl = 0; pl < 2; ++pl) {
                fa[set][pl][0] = *reinterpret_cast<const bf16x8*>(A + pl * (C2_A_BYTES / 2) + (t * 2 * KT) * 16);
                fa[set][pl][1] = *reinterpret_cast<const bf16x8*>(A + pl * (C2_A_BYTES / 2) + (t * 2 * KT + 32) * 16);
                fb[set][pl] = *reinterpret_cast<const bf16x8*>(T + pl * t_plane + toff[t] * 16);
            }
        };
        load_tap(0, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 6, 0);
#pragma unroll
        for (int t = 0; t < NTAP; ++t) {
            const int q = t / TPSET, set = t & 1;
            if (t + 1 < NTAP) load_tap(t + 1, set ^ 1);
            // smallest terms first: lo(w) hi(x), hi(w) lo(x), hi(w) hi(x); the two row tiles alternate so that no MFMA waits for its predecessor
            acc[q][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[set][1][0], fb[set][0], acc[q][0], 0, 0, 0);
            acc[q][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[set][1][1], fb[set][0], acc[q][1], 0, 0, 0);
            acc[q][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[set][0][0], fb[set][1], acc[q][0], 0, 0, 0);
            acc[q][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[set][0][1], fb[set][1], acc[q][1], 0, 0, 0);
            acc[q][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[set][0][0], fb[set][0], acc[q][0], 0, 0, 0);
            acc[q][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[set][0][1], fb[set][0], acc[q][1], 0, 0, 0);
            if (t + 1 < NTAP) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x100, 6, 0);
                __builtin_amdgcn_sched_group_barrier(0x008, 5, 0);
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // this stage's DMA and loads are the next stage's operands
        __syncthreads();                                       // every wave is done reading T
        if (s + 1 < s_hi) {
            split_store(s + 1);
            __syncthreads();
        }
    }

    // epilogue: lane = lane-grid pixel, register = channel
    const int py = y0 + (p >> g.wshift), px = p & (g.Wl - 1);
    if (MODE == CB_C2F) {
        // fine row 2 py + phase, fine columns 2 px and 2 px + 1 (the two accumulator sets): one 8-byte store
        float* op = out + (size_t)b * g.K * HWo + (size_t)(2 * py + phase) * g.Wout + 2 * px;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int k = kt * KT + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
                if (k < g.K) *reinterpret_cast<float2*>(op + (size_t)k * HWo) = make_float2(acc[0][i][e], acc[NSET - 1][i][e]);
            }
    } else if (MODE == CB_DC2F) {
        // fine rows 2 py and 2 py + 1, fine columns 2 px and 2 px + 1: only (odd, odd) carries a value, the other three are zeros of the result
        float* op = out + (size_t)b * g.K * HWo + (size_t)(2 * py) * g.Wout + 2 * px;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int k = kt * KT + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
                if (k < g.K) {
                    *reinterpret_cast<float2*>(op + (size_t)k * HWo) = make_float2(0.0f, 0.0f);
                    *reinterpret_cast<float2*>(op + (size_t)k * HWo + g.Wout) = make_float2(0.0f, acc[0][i][e]);
                }
            }
    } else {
        float* op = out + (size_t)b * g.K * HWo + (size_t)py * g.Wout + px;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int k = kt * KT + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
                if (k < g.K) op[(size_t)k * HWo] = acc[0][i][e];
            }
    }
}

// ---- the host side of the four data-pass kernels: one planner, one byte count, one launcher over DATA_KINDS x DATA_FORMS ----
// What the kernels differ in as far as the host is concerned: one row per kernel, read by data_geometry, data_ws_bytes and launch_data.
// All four run on the one plan CbGeom (conv_bf16x3_kernel on the part of it that it reads, CxGeom).
// `split` decides the rest of the plan: bf16 tensors (conv_bf16_kernel) get the tile 128 x 256, or 64 produced channels x 512 / 256 pixels when
// K <= 64, LDS = A[2] | T[2] | raw[2 or 1], and a stage has to fit the transposition and DMA loops (cb_tr_max, cb_xj); fp32 tensors on split-bf16
// operands get the tile 64 x 256, two packed planes (hi | lo), LDS = A[2] | T (hi | lo), and one activation item (c group, row, 4 floats) per thread.
enum { DATA_K3 = 0, DATA_S2 = 1, DATA_K3_SPLIT = 2, DATA_S2_SPLIT = 3, DATA_S2_DIL = 4 };
struct DataKind {
    bool split;
    int wmax;                           // widest lane grid
    const char *who, *width_fmt;        // the messages, as each planner has always worded them
    const char* kernel;                 // the name check_launch reports
};
constexpr DataKind DATA_KINDS[5] = {
    {false, 256, "bf16 direct conv", "%s: grid width %d (16 .. 256, a power of two)", "conv_bf16_kernel"},
    {false, 256, "bf16 direct 4x4 stride-2 conv", "%s: grid width %d (16 .. 256, a power of two)", "conv_bf16_kernel"},
    {true, 256, "split-bf16 direct conv", "%s: width %d (16 .. 256, a power of two)", "conv_bf16x3_kernel"},
    {true, 128, "split-bf16 direct 4x4 stride-2 conv", "%s: coarse width %d (16 .. 128, a power of two)", "conv_bf16x3_s2_kernel"},
    // the dilated forms on bf16 tensors: DATA_S2's plan on the coarse widths whose stage fits the loop bounds (DF2C at nw = 128 fills them: 192
    // transposition blocks and 1536 raw chunks at 256 pixels, 320 and 2560 at 512); two raw buffers always fit (<= 153 KB), `raw1` never comes up
    {false, 128, "bf16 direct dilated 4x4 stride-2 conv", "%s: coarse width %d (16 .. 128, a power of two)", "conv_bf16_kernel"},
};

// What a form (CB_S1 .. CB_DC2F) fixes on any grid: which tensor is the fine one (2 Hl x 2 Wl), sub-stages per channel block, row phases, taps per
// stage, column-phase planes of T, and for the profile marks the taps per counted pixel (`coarse`: per lane-grid pixel whichever tensor is written).
struct DataForm { bool fine_in, fine_out; int nsub, nphase, ntap, planes; double taps; bool coarse; };
constexpr DataForm DATA_FORMS[5] = {
    {false, false, 1, 1, 9, 1,  9.0, false},        // S1
    {true,  false, 2, 1, 8, 2, 16.0, false},        // F2C: T keeps the two column phases
    {false, true,  1, 2, 8, 1,  4.0, false},        // C2F
    {true,  false, 2, 1, 8, 1, 16.0, true},         // DF2C
    {false, true,  2, 1, 8, 1, 16.0, true},         // DC2F
};

// A form on a lane grid already set (Hl x Wl, R rows per tile): tensors, halo rows, row map, tap offsets
static void data_form(int form, CbGeom* g)
{
    const DataForm& f = DATA_FORMS[form];
    const int nh = g->Hl, nw = g->Wl;
    g->Hin = f.fine_in ? 2 * nh : nh; g->Win = f.fine_in ? 2 * nw : nw;
    g->Hout = f.fine_out ? 2 * nh : nh; g->Wout = f.fine_out ? 2 * nw : nw;
    g->nsub = f.nsub; g->nphase = f.nphase; g->ntap = f.ntap;
    g->ymul = g->rowstep = f.fine_in ? 2 : 1;
    if (form == CB_S1 || form == CB_C2F) {
        g->NR = g->R + 2; g->PW = nw + 2; g->yoff[0] = g->yoff[1] = -1;
    } else if (form == CB_F2C) {
        g->NR = g->R + 1; g->PW = nw + 1; g->yoff[0] = 0; g->yoff[1] = -1;                  // sub-stage e = input row parity: rows 2 (y0 + i) + e - 2 e
    } else {
        g->NR = g->R + 1; g->PW = nw + 3;                                                   // sub-stage e = weight rows {2 e, 2 e + 1}
        g->yoff[0] = form == CB_DF2C ? -3 : 1; g->yoff[1] = form == CB_DF2C ? 1 : -1;
    }
    g->NPOS = g->NR * g->PW;
    // tapoff[e][t], e = sub-stage (F2C, dilated) or row phase (C2F):
    //   F2C   tap t = ri * 4 + s of sub-stage e: r = e ? {0, 2}[ri] : {1, 3}[ri]; input row 2 oy - 1 + r = 2 (oy + drow - (e ? 1 : 0)) + e  ->  drow = ri;
    //         column 2 ox - 1 + s: s even -> odd column (plane 1, j = ox - 1 + s / 2, stored at j + 1), s odd -> even column (plane 0, j = ox + s / 2)
    //   C2F   row phase ey' (workgroup), column phase ex' (accumulator set), taps (ai, bi): fine row 2 i + ey' takes coarse rows
    //         ey' = 0: {i (r = 1), i - 1 (r = 3)};  ey' = 1: {i + 1 (r = 0), i (r = 2)}  ->  raw row (i - y0) + 1 + d, d = ey' - ai
    //   dilated  tap (ri, s): conv_bf16x3_s2_kernel's header
    for (int e = 0; e < 2; ++e)
        for (int t = 0; t < f.ntap; ++t) {
            const int ri = t >> 2, sx = t & 3;
            const int ex = t >> 2, ai = (t >> 1) & 1, bi = t & 1;
            g->tapoff[e][t] = form == CB_S1 ? (t / 3) * g->PW + (t % 3)
                            : form == CB_F2C ? ((sx & 1) ? 0 : 1) * 2 * g->NPOS + ri * g->PW + (sx >> 1)
                            : form == CB_C2F ? (1 + e - ai) * g->PW + (1 + ex - bi)
                            : form == CB_DF2C ? ri * g->PW + sx : (1 - ri) * g->PW + (3 - sx);
        }
}

// Source taps of a form's packed image: srctap[phase][sub][t] = the tap of the module's kernel (S1: 3x3, flipped when `flip`; else r * 4 + s of its 4x4)
static CbPack data_pack(int form, int flip, int kt)
{
    const DataForm& f = DATA_FORMS[form];
    CbPack pk{};
    pk.ntap = f.ntap; pk.nsub = f.nsub; pk.nphase = f.nphase; pk.kt = kt;
    for (int phase = 0; phase < f.nphase; ++phase)
        for (int sub = 0; sub < f.nsub; ++sub)
            for (int t = 0; t < f.ntap; ++t) {
                const int ri = t >> 2, sx = t & 3;
                const int ex = t >> 2, ai = (t >> 1) & 1, bi = t & 1;
                pk.srctap[phase][sub][t] = form == CB_S1 ? (flip ? 8 - t : t)
                                         : form == CB_F2C ? (sub ? 2 * ri : 2 * ri + 1) * 4 + sx
                                         : form == CB_C2F ? (1 - phase + 2 * ai) * 4 + (1 - ex + 2 * bi)
                                         : (2 * sub + ri) * 4 + sx;                         // both dilated forms: weight row 2 e + ri, column s
            }
    return pk;
}

static size_t data_lds_bytes(const DataKind& k, const CbGeom& g)
{
    return 2 * (size_t)g.a_bytes + (k.split ? 1 : 2) * (size_t)g.t_bytes + (g.raw1 ? 1 : 2) * (size_t)g.raw_bytes;
}

// The limits, before any launch.  C reduction channels -> K produced; Hl x Wl = the lane grid (S1: the image; k4 s2: the coarse grid nh x nw, the fine
// tensor is [., ., 2nh, 2nw]).
static int data_geometry(int kind, int form, int B, int C, int K, int Hl, int Wl, CbGeom* g)
{
    const DataKind& k = DATA_KINDS[kind];
    if (C % CB_C != 0) return fail(IPSR_ERR_UNSUPPORTED, "%s: %d reduction channels are not a multiple of %d", k.who, C, CB_C);
    if (Wl != 16 && Wl != 32 && Wl != 64 && Wl != 128 && Wl != k.wmax) return fail(IPSR_ERR_UNSUPPORTED, k.width_fmt, k.who, Wl);
    g->B = B; g->C = C; g->K = K; g->Hl = Hl; g->Wl = Wl;
    g->wshift = cb_wshift(Wl);
    g->kt = k.split || K <= 64 ? 64 : CB_K;
    g->ktiles = (K + g->kt - 1) / g->kt;
    const auto tile = [&](int ptile) -> int {
        g->ptile = ptile; g->R = ptile / Wl;
        if (Hl % g->R != 0) return fail(IPSR_ERR_UNSUPPORTED, "%s: %d rows are not a multiple of the %d rows of a tile", k.who, Hl, g->R);
        data_form(form, g);
        g->ptiles = B * (Hl / g->R);
        g->nstage = (C / CB_C) * g->nsub;
        // Small maps leave the chip idle (a 16x16 map is ONE pixel tile per image: 64 workgroups at 512 produced channels and batch 16): the
        // reduction is cut into up to four runs of whole channel blocks, each run a workgroup of its own writing an fp32 partial.
        cb_cut_reduction(g->ktiles * g->nphase * g->ptiles, C / CB_C, g->nsub, &g->nsplit, &g->sps);
        const int nplane = k.split ? 2 : 1;                       // hi | lo
        g->a_bytes = nplane * g->ntap * 2 * g->kt * 16;
        g->t_bytes = (int)align_up((size_t)nplane * DATA_FORMS[form].planes * 2 * g->NPOS * 16, 256);
        g->raw_bytes = k.split ? 0 : (int)align_up((size_t)CB_C * g->NR * g->Win * 2, 1024);
        g->raw1 = !k.split && 2 * (g->a_bytes + g->t_bytes + g->raw_bytes) > CB_LDS_MAX;
        const bool fits = k.split ? 2 * g->NR * (g->Win / 4) <= CB_THREADS
                                  : 4 * g->NR * (g->Win / 16) <= 32 * cb_tr_max(ptile) && CB_C * g->NR * (g->Win / 8) <= cb_xj(ptile) * CB_THREADS;
        if (data_lds_bytes(k, *g) > (size_t)CB_LDS_MAX || !fits)
            return fail(IPSR_ERR_UNSUPPORTED, "%s: a tile of %d rows x %d does not fit the LDS plan", k.who, g->NR, g->Win);
        return IPSR_OK;
    };
    // bf16, <= 64 produced channels: the 512-pixel tile where the map and the LDS plan allow it, else 256
    if (!k.split && K <= 64 && tile(2 * CB_P) == IPSR_OK) return IPSR_OK;
    return tile(CB_P);
}

static size_t data_pack_bytes(const CbGeom& g) { return (size_t)g.ktiles * g.nphase * g.nstage * g.ntap * 2 * g.kt * 16; }      // one plane

// zero page | packed weights (split: hi plane | lo plane) | fp32 partials of a split reduction
static size_t data_ws_bytes(const DataKind& k, const CbGeom& g) { return 256 + align_up((k.split ? 2 : 1) * data_pack_bytes(g), 256) + cb_partial_bytes(g); }

// the workspace queries: 0 for a refused shape
static size_t data_ws_query(int kind, int form, int B, int C, int K, int Hl, int Wl)
{
    CbGeom g;
    return data_geometry(kind, form, B, C, K, Hl, Wl, &g) == IPSR_OK ? data_ws_bytes(DATA_KINDS[kind], g) : 0;
}

template <int MODE, int KT, int P, typename TOUT>
static int cb_launch_kernel(const CbGeom& g, const void* in, const uint4* Wp, const uint4* zero_page, void* out, unsigned grid, size_t smem, hipStream_t st)
{
    if (int rc = raise_dynamic_lds(reinterpret_cast<const void*>(&conv_bf16_kernel<MODE, KT, P, TOUT>), "conv_bf16_kernel", CB_LDS_MAX)) return rc;
    conv_bf16_kernel<MODE, KT, P, TOUT><<<grid, CB_THREADS, smem, st>>>(static_cast<const unsigned short*>(in), Wp, zero_page, g, static_cast<TOUT*>(out));
    return IPSR_OK;
}

// the bf16 kernel instance of a plan: tile (g.kt x g.ptile) and output type
template <int MODE, typename TOUT>
static int cb_launch_tile(const CbGeom& g, const void* in, const uint4* Wp, const uint4* zero_page, void* out, unsigned grid, size_t smem, hipStream_t st)
{
    if (g.kt == 64 && g.ptile == 2 * CB_P) return cb_launch_kernel<MODE, 64, 2 * CB_P, TOUT>(g, in, Wp, zero_page, out, grid, smem, st);
    if (g.kt == 64) return cb_launch_kernel<MODE, 64, CB_P, TOUT>(g, in, Wp, zero_page, out, grid, smem, st);
    return cb_launch_kernel<MODE, 128, CB_P, TOUT>(g, in, Wp, zero_page, out, grid, smem, st);
}

// in [B,C,Hin,Win] (bf16; the split kinds: fp32), weight fp32 with element (c, k, tap) at w[c*sc + k*sk + tap] (S1: taps flipped when `flip`),
// out [B,K,Hout,Wout] bf16 / fp32 (the split kinds: fp32).  pack_valid (S1 only): ws already holds this weight's packed image.
template <int KIND, int FORM>
static int launch_data(const void* in, const float* w, void* out, int B, int C, int K, int Hl, int Wl, long sc, long sk, int flip, int out_bf16,
                       void* ws, size_t ws_bytes, hipStream_t st, int pack_valid = 0)
{
    constexpr DataKind k = DATA_KINDS[KIND];
    constexpr DataForm f = DATA_FORMS[FORM];
    static_assert((FORM == CB_S1) == (KIND == DATA_K3 || KIND == DATA_K3_SPLIT) && (FORM < CB_DF2C || KIND == DATA_S2_SPLIT || KIND == DATA_S2_DIL) &&
                  (KIND != DATA_S2_DIL || FORM >= CB_DF2C), "no kernel of this kind has the form");
    CbGeom g;
    if (int rc = data_geometry(KIND, FORM, B, C, K, Hl, Wl, &g)) return rc;
    const size_t need = data_ws_bytes(k, g);
    if (ws_bytes < need) return fail(IPSR_ERR_WORKSPACE, "%s: workspace %zu < %zu", k.who, ws_bytes, need);
    uint4* zero_page = static_cast<uint4*>(ws);
    uint4* Wp = zero_page + 16;
    const size_t pack = data_pack_bytes(g), lo_plane = k.split ? pack / 16 : 0;
    if (!pack_valid) {
        cb_pack_weights_kernel<k.split><<<dim3(cdiv(g.ktiles * g.kt, 256), C / 8, f.ntap * f.nsub * f.nphase), 256, 0, st>>>(
            w, C, K, sc, sk, data_pack(FORM, flip, g.kt), Wp, zero_page, lo_plane);
        if (int rc = check_launch("cb_pack_weights_kernel")) return rc;
    }
    const unsigned grid = (unsigned)(g.ktiles * g.nphase * g.ptiles * g.nsplit);
    const size_t smem = data_lds_bytes(k, g);
    void* dst = cb_run_dst(g.nsplit, Wp, (k.split ? 2 : 1) * pack, out);
    profile_mark_start(st, 4);
    if constexpr (!k.split) {
        if (int rc = (out_bf16 && g.nsplit == 1) ? cb_launch_tile<FORM, bf16_t>(g, in, Wp, zero_page, dst, grid, smem, st)
                                                 : cb_launch_tile<FORM, float>(g, in, Wp, zero_page, dst, grid, smem, st)) return rc;
    } else if constexpr (KIND == DATA_K3_SPLIT) {
        if (int rc = raise_dynamic_lds(reinterpret_cast<const void*>(&conv_bf16x3_kernel), k.kernel, CB_LDS_MAX)) return rc;
        CxGeom x{B, C, K, Hl, Wl, g.wshift, g.R, g.NR, g.PW, g.NPOS, g.ktiles, g.ptiles, g.nstage, g.nsplit, g.sps, g.t_bytes, {}};
        for (int t = 0; t < 9; ++t) x.tapoff[t] = g.tapoff[0][t];
        conv_bf16x3_kernel<<<grid, CB_THREADS, smem, st>>>(static_cast<const float*>(in), Wp, lo_plane, x, static_cast<float*>(dst));
    } else {
        if (int rc = raise_dynamic_lds(reinterpret_cast<const void*>(&conv_bf16x3_s2_kernel<FORM>), k.kernel, CB_LDS_MAX)) return rc;
        conv_bf16x3_s2_kernel<FORM><<<grid, CB_THREADS, smem, st>>>(static_cast<const float*>(in), Wp, lo_plane, g, static_cast<float*>(dst));
    }
    const double outs = f.coarse ? (double)B * Hl * Wl : (double)B * g.Hout * g.Wout;
    return cb_launch_tail(k.kernel, g.nsplit, dst, (size_t)B * K * g.Hout * g.Wout, out, out_bf16, st,
                          (k.split ? 3.0 : 1.0) * 2.0 * f.taps * C * (double)(g.ktiles * g.kt) * outs, 2.0 * f.taps * C * (double)K * outs);
}

// The k4 s2 entries' operands: weight [Kc][Cf][4][4], fine [B,Cf,2nh,2nw], coarse [B,Kc,nh,nw]; a form that reads the fine tensor reduces Cf
template <int KIND, int FORM>
static int launch_data_s2(const void* in, const float* w, void* out, int B, int Kc, int Cf, int nh, int nw, int out_bf16, void* ws, size_t ws_bytes, hipStream_t st)
{
    constexpr bool f2c = DATA_FORMS[FORM].fine_in;
    const long skc = (long)Cf * 16, scf = 16;
    return launch_data<KIND, FORM>(in, w, out, B, f2c ? Cf : Kc, f2c ? Kc : Cf, nh, nw, f2c ? scf : skc, f2c ? skc : scf, 0, out_bf16, ws, ws_bytes, st);
}

// =====================================================================================================================================
// Weight gradient of the k3 s1 p1 layers on the bf16 matrix cores:
//      dW[ka][cb][t] = sum_{b, y, x}  a[b][ka][y][x] * w[b][cb][y + dy_t][x + dx_t]            (w zero outside the image)
// Conv2d: a = dy (Ka = Cout), w = x (Cb = Cin);  ConvTranspose2d: a = x (Ka = Cin), w = dy (Cb = Cout) — dW comes out in the module's
// own layout either way.  As a GEMM the reduction runs over PIXELS, which NCHW has contiguous: both operands' fragments are 8
// consecutive pixels of one channel, i.e. aligned 16-byte reads of the natural image — except the dx = +-1 taps, whose windows start
// one pixel (2 bytes) off.  A lane therefore reads its aligned chunk plus the dword before and after it and builds the two shifted
// fragments with five v_alignbit_b32 (the three taps of a row share them).
// Workgroup = 512 threads = 8 waves (4 x 2): 128 a-channels x 64 w-channels x 9 taps; a wave owns 32 x 32 x 9 = nine MFMA tiles.
// The pixel range is cut over workgroups (`nsplit` runs of whole image rows): every workgroup writes its partial [t][ka][cb] slab and
// a second small kernel adds the slabs in ascending order (deterministic) into dW[ka][cb][t].  Stage = 128 pixels (RS = 128 / W image
// rows): the a rows [128][128 px] double-buffered, the w rows in a ring of 2 RS + 2 image rows (a stage needs RS + 2, the next one's
// RS new rows arrive meanwhile), both by LDS-DMA with the 16-byte chunks of a row XOR-swizzled / the row pitch odd in 16-byte slots so
// that the 32 channels of a fragment read hit distinct banks.

// The plan of all six weight-gradient kernels (this one, its split-bf16 form, the two k4 s2 p1 kernels and the two dilated k4 s2 kernels
// further down; wrw_geometry).
// The a operand is the one whose channels index dW's rows (3x3: see above; k4 s2: the coarse tensor), w the one read through the taps
// (k4 s2: the fine tensor); H x W is the grid the reduction runs over (k4 s2: the coarse grid nh x nw, the fine tensor is 2H x 2W).
struct WrwGeom {
    int B, K, C, H, W, wshift;  // channels of a / of w; log2 W
    int RS, NRING, pitch;       // grid rows per stage; ring entries (3x3: image rows, k4 s2: pairs of fine rows); 16-byte slots per (w row, channel)
    int stages_per_wg, nsplit;  // stages of RS rows a workgroup reduces; B * H / (RS * stages_per_wg) runs
    int ktiles, ctiles;
    int ring_plane;             // bytes of the ring (split-bf16: of one of its two planes, hi | lo); read by the split-bf16 kernels only
};

// What the six kernels differ in as far as the host is concerned: one row per kernel, read by wrw_geometry, wrw_ws_bytes and launch_wrw.
// LDS of a launch = 2 x TK x PX x 2 bytes of a (bf16: two buffers; split: hi | lo) + the ring (bf16: one plane; split: two).
enum { WRW_3X3 = 0, WRW_3X3_SPLIT = 1, WRW_S2 = 2, WRW_S2_SPLIT = 3, WRW_DIL_SPLIT = 4, WRW_DIL = 5 };
struct WrwKind {
    int TK, TC, NT, PX;         // tile: a channels x w channels; taps (= NT of cb_slab_reduce_kernel); pixels per stage
    int ring_mul, ring_add;     // ring entries = ring_mul * RS + ring_add
    int wscale, wmax;           // a ring entry per grid row, both ways (k4 s2: 2 = rows per ring entry, pitch of 2 W pixels; dilated: 1, the
                                // ring holds the sampled rows q); widest grid
    int dma_add;                // ring by LDS-DMA: one round moves up to RS + dma_add ring entries, 5 slots per thread; -1: the ring is filled
                                // through registers (the split kinds, and the bf16 dilated kind, which samples q on the way)
    bool split;                 // fp32 tensors, split-bf16 operands: two planes, no zero page, three MFMAs per product
    const char *who, *width_fmt, *rows_fmt, *ring_fmt;      // the messages, as each planner has always worded them
    const char *kernel, *reduce;                             // the names check_launch reports
};
constexpr WrwKind WRW_KINDS[6] = {
    // TK  TC  NT   PX  ring   wscale wmax dma split
    {128, 64,  9, 128, 2, 2,  1,    128,  0, false, "bf16 weight gradient",
     "%s: image width %d (16, 32, 64 or 128)", "%s: %d rows are not a multiple of %d", "%s: the row ring of a %d-wide image does not fit the LDS plan",
     "conv_bf16_wrw_kernel", "conv_bf16_wrw_reduce_kernel"},
    {128, 32,  9, 128, 1, 2,  1,    128, -1, true, "split-bf16 weight gradient",
     "%s: image width %d (16, 32, 64 or 128)", "%s: %d rows are not a multiple of the %d rows of a stage", "%s: the row ring of a %d-wide image does not fit the LDS plan",
     "conv_bf16x3_wrw_kernel", "conv_bf16_wrw_reduce_kernel"},
    {128, 32, 16,  64, 2, 1,  2,     64,  1, false, "bf16 4x4 stride-2 weight gradient",
     "%s: coarse width %d (16, 32 or 64)", "%s: %d coarse rows are not a multiple of %d", "%s: row ring of a %d-wide grid",
     "conv_bf16_wrw_s2_kernel", "conv_bf16_wrw_s2_reduce_kernel"},
    {128, 32, 16,  64, 1, 1,  2,     64, -1, true, "split-bf16 4x4 stride-2 weight gradient",
     "%s: coarse width %d (16, 32 or 64)", "%s: %d coarse rows are not a multiple of the %d rows of a stage", "%s: the row ring of a %d-wide grid does not fit the LDS plan",
     "conv_bf16x3_wrw_s2_kernel", "conv_bf16_wrw_s2_reduce_kernel"},
    {128, 32, 16,  64, 1, 3,  1,    128, -1, true, "split-bf16 dilated 4x4 stride-2 weight gradient",
     "%s: coarse width %d (16, 32, 64 or 128)", "%s: %d coarse rows are not a multiple of the %d rows of a stage", "%s: the row ring of a %d-wide grid does not fit the LDS plan",
     "conv_bf16x3_wrw_dil_kernel", "conv_bf16_wrw_dil_reduce_kernel"},
    {128, 32, 16,  64, 1, 3,  1,    128, -1, false, "bf16 dilated 4x4 stride-2 weight gradient",
     "%s: coarse width %d (16, 32, 64 or 128)", "%s: %d coarse rows are not a multiple of the %d rows of a stage", "%s: the row ring of a %d-wide grid does not fit the LDS plan",
     "conv_bf16_wrw_dil_kernel", "conv_bf16_wrw_dil_reduce_kernel"},
};
constexpr int WB_K = WRW_KINDS[WRW_3X3].TK, WB_C = WRW_KINDS[WRW_3X3].TC, WB_PX = WRW_KINDS[WRW_3X3].PX, WB_THREADS = 512;
constexpr int WB_A_BYTES = WB_K * WB_PX * 2;                 // 32 KB per buffer; the w-row ring gets the other 96 KB (largest: W = 16 -> 18 rows x 64 c
                                                             // x 5 slots x 16 B = 92 KB)

// ---- what the six kernels share on the device ----
struct WrwRun { int kt, ct, split, b, ylo; };               // tile, run, and the run's image and first grid row

// workgroup -> (tile, run): the tiles of one run are neighbours
__device__ __forceinline__ WrwRun wrw_decode(const WrwGeom& g)
{
    const unsigned L = xcd_remap(blockIdx.x, gridDim.x);
    const int tiles = g.ktiles * g.ctiles;
    const int tile = L % tiles, split = L / tiles;
    const int kt = tile % g.ktiles, ct = tile / g.ktiles;
    const int rows_per_wg = g.RS * g.stages_per_wg;
    const int runs_per_img = g.H / rows_per_wg;
    const int b = split / runs_per_img, ylo = (split - b * runs_per_img) * rows_per_wg;
    return {kt, ct, split, b, ylo};
}

// The accumulator clear of the two split-bf16 kernels.  The two bf16 kernels keep theirs inline, and all four keep their slab store
// (slab[split][t][ka][cb], rows by the element map of the 32 x 32 MFMA) inline: hoisted, either one makes hipcc lay the kernel out
// differently (an inverted compare and branch, other register numbers) — the same work, but not the instruction stream that was measured.
template <int N>
__device__ __forceinline__ void wrw_clear(f32x16 (&acc)[N])
{
#pragma unroll
    for (int t = 0; t < N; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[t][e] = 0.0f;
}

__device__ __forceinline__ unsigned alignbit16(unsigned hi, unsigned lo) { return __builtin_amdgcn_alignbit(hi, lo, 16); }

// 3x3: the three column taps of 8 pixels at X (a lane's aligned 16-byte chunk of a ring row): the chunk itself and, from it and the dword
// before and after it, the windows one pixel to the left and to the right
__device__ __forceinline__ void wrw_shifted(const unsigned char* X, u32x4* left, u32x4* ctr, u32x4* right)
{
    const u32x4 c4 = *reinterpret_cast<const u32x4*>(X);    // ext-vector load (see u32x4)
    const unsigned prev = *reinterpret_cast<const unsigned*>(X - 4);
    const unsigned next = *reinterpret_cast<const unsigned*>(X + 16);
    const unsigned s0 = alignbit16(c4.x, prev), s1 = alignbit16(c4.y, c4.x), s2 = alignbit16(c4.z, c4.y), s3 = alignbit16(c4.w, c4.z),
                   s4 = alignbit16(next, c4.w);
    *ctr = c4; *left = u32x4{s0, s1, s2, s3}; *right = u32x4{s1, s2, s3, s4};
}

__device__ __forceinline__ unsigned pack_hi(unsigned x, unsigned y) { return __builtin_amdgcn_perm(y, x, 0x07060302u); }   // {x.hi16, y.hi16}
__device__ __forceinline__ unsigned pack_lo(unsigned x, unsigned y) { return __builtin_amdgcn_perm(y, x, 0x05040100u); }   // {x.lo16, y.lo16}

// k4 s2: the four column taps s of 8 coarse pixels from the 16 fine pixels at X (two aligned 16-byte chunks of a ring row) and the dword
// before and after them: every other fine pixel, starting at fine column 2 ox - 1 + s
__device__ __forceinline__ void wrw_pick_even_odd(const unsigned char* X, u32x4 (&f)[4])
{
    const u32x4 lo4 = *reinterpret_cast<const u32x4*>(X);
    const u32x4 hi4 = *reinterpret_cast<const u32x4*>(X + 16);
    const unsigned prev = *reinterpret_cast<const unsigned*>(X - 4);
    const unsigned next = *reinterpret_cast<const unsigned*>(X + 32);
    const unsigned d0 = lo4.x, d1 = lo4.y, d2 = lo4.z, d3 = lo4.w, d4 = hi4.x, d5 = hi4.y, d6 = hi4.z, d7 = hi4.w;
    f[0] = u32x4{pack_hi(prev, d0), pack_hi(d1, d2), pack_hi(d3, d4), pack_hi(d5, d6)};
    f[1] = u32x4{pack_lo(d0, d1), pack_lo(d2, d3), pack_lo(d4, d5), pack_lo(d6, d7)};
    f[2] = u32x4{pack_hi(d0, d1), pack_hi(d2, d3), pack_hi(d4, d5), pack_hi(d6, d7)};
    f[3] = u32x4{pack_lo(d1, d2), pack_lo(d3, d4), pack_lo(d5, d6), pack_lo(d7, next)};
}

__global__ void __launch_bounds__(WB_THREADS, 1) conv_bf16_wrw_kernel(const unsigned short* __restrict__ a, const unsigned short* __restrict__ w,
                                                                      const uint4* __restrict__ zero_page, WrwGeom g, float* __restrict__ slabs)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];          // A[2] | X ring
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wk = wave >> 1, wc = wave & 1;
    const int r = lane & 31, h = lane >> 5;

    const WrwRun run = wrw_decode(g);
    const int kt = run.kt, ct = run.ct, b = run.b, ylo = run.ylo, split = run.split;
    const size_t HW = (size_t)g.H * g.W;
    const int cpr = g.W >> 3;                                // 16-byte chunks per image row

    // ---- a rows: slot sigma = k * 16 + cs holds stage chunk c8 = cs ^ (k & 15) of channel k; c8 -> (row rs, chunk cx) -------------------
    const unsigned short* ga[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int sigma = (wave + 8 * j) * 64 + lane;
        const int k = sigma >> 4, c8 = (sigma & 15) ^ (k & 15);
        const int rs = c8 / cpr, cx = c8 - rs * cpr;
        const int ka = kt * WB_K + k;
        ga[j] = ka < g.K ? a + ((size_t)b * g.K + ka) * HW + (size_t)(ylo + rs) * g.W + cx * 8 : nullptr;
    }
    // ---- w rows: ring slot of image row y = (y + 1) mod NRING; per (ring row, channel): [halo][W / 8 chunks][halo][pad] = `pitch` slots ----
    // a group of RS rows = RS * 64 * pitch slots; slot q = (row rr, channel c, slot sl); 64 * pitch is a multiple of 64, so the 64 lanes of
    // one DMA instruction never straddle rows: wave-uniform LDS base, per-lane source
    const int xslots = g.RS * WB_C * g.pitch;
    const unsigned short* gxw[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const int q = tid + WB_THREADS * j;
        const int qq = q < xslots ? q : 0;
        const int sl = qq % g.pitch, c = (qq / g.pitch) % WB_C;
        const int cb = ct * WB_C + c;
        const bool data = sl >= 1 && sl <= cpr && cb < g.C;
        gxw[j] = data ? w + ((size_t)b * g.C + cb) * HW + (sl - 1) * 8 : nullptr;
    }
    const int ring_row_slots = WB_C * g.pitch, ring_row_bytes = ring_row_slots * 16;

    f32x16 acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[t][e] = 0.0f;

    auto dma_a = [&](int buf, int stage) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const void* src = ga[j] ? static_cast<const void*>(ga[j] + (size_t)stage * g.RS * g.W) : static_cast<const void*>(zero_page);
            __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(lds + buf * WB_A_BYTES + (wave + 8 * j) * 1024), 16, 0, 0);
        }
    };
    // image rows y_first .. y_first + RS - 1 into their ring slots (rows outside the image: zeros)
    auto dma_x = [&](int y_first) {
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const int q0 = wave * 64 + WB_THREADS * j;        // uniform: first slot of this wave's instruction
            if (q0 < xslots) {
                const int rr = q0 / ring_row_slots, within = q0 - rr * ring_row_slots;
                const int y = y_first + rr;
                int slot = (y + 1) % g.NRING;
                if (slot < 0) slot += g.NRING;
                const bool ok = gxw[j] != nullptr && (unsigned)y < (unsigned)g.H;
                const void* src = ok ? static_cast<const void*>(gxw[j] + (size_t)y * g.W) : static_cast<const void*>(zero_page);
                __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(lds + 2 * WB_A_BYTES + slot * ring_row_bytes + within * 16), 16, 0, 0);
            }
        }
    };

    // prologue: a stage 0; w rows ylo - 1 .. ylo + RS (at least)
    dma_a(0, 0);
    for (int y = ylo - 1; y <= ylo + g.RS; y += g.RS) dma_x(y);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    const int a_row = (wk * 32 + r);                          // a fragment: channel row
    const int bcol = wc * 32 + r;                             // w fragment: channel column
    for (int s = 0; s < g.stages_per_wg; ++s) {
        const int cur = s & 1;
        const int y0 = ylo + s * g.RS;
        if (s + 1 < g.stages_per_wg) {
            dma_a(cur ^ 1, s + 1);
            dma_x(y0 + g.RS + 1);                             // the RS rows the next stage adds: y0 + RS + 1 .. y0 + 2 RS
        }
        const unsigned char* A = lds + cur * WB_A_BYTES;
#pragma unroll
        for (int j = 0; j < 8; ++j) {                         // k-steps of 16 pixels
            const int c8 = 2 * j + h;
            const bf16x8 fa = *reinterpret_cast<const bf16x8*>(A + ((a_row << 4) + (c8 ^ (a_row & 15))) * 16);
            const int p0 = 16 * j;                            // stage pixel of the k-step
            const int rs = p0 >> g.wshift, px = (p0 & (g.W - 1)) + 8 * h;
#pragma unroll
            for (int dy = 0; dy < 3; ++dy) {
                int slot = (y0 + rs + dy) % g.NRING;          // image row y0 + rs + dy - 1 lives in ring slot (y + 1) mod NRING
                const unsigned char* X = lds + 2 * WB_A_BYTES + slot * ring_row_bytes + (bcol * g.pitch + 1 + (px >> 3)) * 16;
                u32x4 left, c4, right;
                wrw_shifted(X, &left, &c4, &right);
                acc[dy * 3 + 0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, __builtin_bit_cast(bf16x8, left), acc[dy * 3 + 0], 0, 0, 0);
                acc[dy * 3 + 1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, __builtin_bit_cast(bf16x8, c4), acc[dy * 3 + 1], 0, 0, 0);
                acc[dy * 3 + 2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, __builtin_bit_cast(bf16x8, right), acc[dy * 3 + 2], 0, 0, 0);
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }

    // partial result: slab[split][t][ka][cb] (lanes along cb: coalesced)
    const int Kp = g.ktiles * WB_K, Cp = g.ctiles * WB_C;
    float* out = slabs + (size_t)split * 9 * Kp * Cp;
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int ka = kt * WB_K + wk * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
            out[((size_t)t * Kp + ka) * Cp + ct * WB_C + bcol] = acc[t][e];
        }
}

// =====================================================================================================================================
// The same weight gradient on FP32 tensors with split-bf16 operands (forms 2 / 3 of ipsr_conv3x3_bf16_wrw; the opt-in arithmetic
// "direct_bf16x3_dw" of the fp32 nets).  Every operand v is taken as hi + lo, hi = bf16(v), lo = bf16(v - hi) (round to nearest even; the
// fp32 residual is exact), every product as lo*hi + hi*lo + hi*hi: per tap and k-step three MFMAs into the same fp32 accumulator,
// smallest terms first; lo*lo (2^-18 of the product) is dropped.  A plain pixel reduction amplifies nothing: the error is the 3 * 2^-18 per
// product of the split plus the fp32 accumulation.
// The structure is conv_bf16_wrw_kernel's: 8-pixel fragments, the dx = +-1 taps by five v_alignbit_b32 from the aligned chunk and its
// neighbouring dwords (now for a hi and a lo image), runs of whole image rows cut over workgroups, partial [t][ka][cb] slabs added in
// ascending order by cb_slab_reduce_kernel<9>.  What changed is the plan, because hi + lo images of both operands do not fit the old one:
//   * the split happens in the kernel, global -> registers -> v_cvt_pk_bf16_f32 -> LDS at the swizzled addresses (no pass over HBM, no
//     fp32-sized intermediates, no LDS-DMA): the REGISTERS are the second buffer — the loads of stage s + 1 (40 dwords per lane) fly during
//     the multiplications of stage s, the conversion and the stores follow between two barriers — so LDS holds ONE buffer of each image;
//   * tile = 128 a-channels x 32 w-channels x 9 taps, stage = 128 pixels (RS = 128 / W image rows).  8 waves = 4 (a-channels) x 2 (halves
//     of the stage's pixels): a wave owns 32 x 32 x 9 = nine MFMA tiles (9 x 16 accumulator registers, as before) over four of the eight
//     k-steps; the two halves are added through LDS (fixed order: first half + second half) before the slab is written;
//   * the w rows live in a ring of RS + 2 image rows (a stage reads RS + 2; the next stage's RS new rows replace the RS oldest after the
//     barrier); its halo slots and the rows outside the image are zeros.
// LDS: a hi | a lo = 2 x 32 KB; ring hi | ring lo = 2 x (RS + 2) x 32 c x (W / 8 + 3) slots x 16 B:
//      W = 16: 65536 + 51200 = 116736 B   W = 32: 65536 + 43008 = 108544 B   W = 64: 65536 + 45056 = 110592 B   W = 128: 65536 + 58368 = 123904 B
// Supported: W in {16, 32, 64, 128}, H a multiple of 128 / W.  Deterministic: no atomics, every sum in a fixed order.
constexpr int WX_K = WRW_KINDS[WRW_3X3_SPLIT].TK, WX_C = WRW_KINDS[WRW_3X3_SPLIT].TC, WX_PX = WRW_KINDS[WRW_3X3_SPLIT].PX;
constexpr int WX_A_PLANE = WX_K * WX_PX * 2;                 // 32 KB per plane

// 8 consecutive fp32 pixels -> their hi and lo bf16 images (16 bytes each)
__device__ __forceinline__ void wx_split8(const f32x4& v0, const f32x4& v1, u32x4* hi, u32x4* lo)
{
    unsigned h16[8], l16[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float v = i < 4 ? v0[i] : v1[i - 4];
        h16[i] = __builtin_bit_cast(unsigned short, (__bf16)v);
        l16[i] = __builtin_bit_cast(unsigned short, (__bf16)(v - __uint_as_float(h16[i] << 16)));
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) { (*hi)[i] = h16[2 * i] | (h16[2 * i + 1] << 16); (*lo)[i] = l16[2 * i] | (l16[2 * i + 1] << 16); }
}

__global__ void __launch_bounds__(WB_THREADS, 1) conv_bf16x3_wrw_kernel(const float* __restrict__ a, const float* __restrict__ w, WrwGeom g,
                                                                        float* __restrict__ slabs)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];          // a hi | a lo | ring hi | ring lo
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wk = wave >> 1, wp = wave & 1;
    const int r = lane & 31, h = lane >> 5;

    const WrwRun run = wrw_decode(g);
    const int kt = run.kt, ct = run.ct, b = run.b, ylo = run.ylo, split = run.split;
    const size_t HW = (size_t)g.H * g.W;
    const int cpr = g.W >> 3;                                // 16-byte bf16 chunks per image row
    unsigned char* const ring = lds + 2 * WX_A_PLANE;
    const int ring_row_bytes = WX_C * g.pitch * 16;

    // ---- a rows: a lane owns chunk c8 = tid & 15 (8 pixels; a stage's pixels are contiguous in NCHW) of the channels (tid >> 4) + 32 j; slot
    // k * 16 + (c8 ^ (k & 15)) as in the bf16 kernel (k & 15 is the same for the four j) ------------------------------------------------------
    const int c8 = tid & 15, k0 = tid >> 4;
    const float* ga[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int ka = kt * WX_K + k0 + 32 * j;
        ga[j] = ka < g.K ? a + ((size_t)b * g.K + ka) * HW + (size_t)ylo * g.W + c8 * 8 : nullptr;
    }
    const int a_wr = ((k0 << 4) + (c8 ^ (k0 & 15))) * 16;    // + j * 8192
    // ---- w rows: a lane owns chunk c8 (row rr, chunk cx of the stage's RS new rows) of channel tid >> 4 -------------------------------------
    const int rr = c8 / cpr, cx = c8 - rr * cpr;
    const int cbw = ct * WX_C + k0;
    const float* gw = cbw < g.C ? w + ((size_t)b * g.C + cbw) * HW + c8 * 8 : nullptr;
    const int w_wr = (k0 * g.pitch + 1 + cx) * 16;

    f32x16 acc[9];
    wrw_clear(acc);

    f32x4 ar[8], wr[2];
#pragma unroll
    for (int i = 0; i < 8; ++i) ar[i] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};           // channels past Ka stay zeros
    // stage s: its 128 pixels of a, and the RS rows y0 + 1 .. y0 + RS of w (the rows stage s needs beyond those of stage s - 1)
    auto load_stage = [&](int s) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (ga[j]) {
                const float* src = ga[j] + (size_t)s * WX_PX;
                ar[2 * j] = *reinterpret_cast<const f32x4*>(src);
                ar[2 * j + 1] = *reinterpret_cast<const f32x4*>(src + 4);
            }
        const int y1 = ylo + s * g.RS + 1;
        if (gw && y1 + rr < g.H) {
            const float* src = gw + (size_t)y1 * g.W;
            wr[0] = *reinterpret_cast<const f32x4*>(src);
            wr[1] = *reinterpret_cast<const f32x4*>(src + 4);
        } else {
            wr[0] = wr[1] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        }
    };
    auto store_stage = [&](int s) {
        u32x4 vh, vl;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            wx_split8(ar[2 * j], ar[2 * j + 1], &vh, &vl);
            *reinterpret_cast<u32x4*>(lds + a_wr + j * 8192) = vh;
            *reinterpret_cast<u32x4*>(lds + WX_A_PLANE + a_wr + j * 8192) = vl;
        }
        const int slot = (ylo + s * g.RS + 2 + rr) % g.NRING;                    // image row y lives in ring slot (y + 1) mod NRING
        wx_split8(wr[0], wr[1], &vh, &vl);
        *reinterpret_cast<u32x4*>(ring + slot * ring_row_bytes + w_wr) = vh;
        *reinterpret_cast<u32x4*>(ring + g.ring_plane + slot * ring_row_bytes + w_wr) = vl;
    };

    // prologue: the ring starts as zeros (its halo slots are never written); rows ylo - 1 and ylo, then stage 0
    for (int i = tid; i < 2 * g.ring_plane / 16; i += WB_THREADS) *reinterpret_cast<u32x4*>(ring + i * 16) = u32x4{0u, 0u, 0u, 0u};
    load_stage(0);
    __syncthreads();
    for (int i = tid; i < 2 * WX_C * cpr; i += WB_THREADS) {
        const int e = i / (WX_C * cpr), rem = i - e * (WX_C * cpr);
        const int c = rem / cpr, x8 = rem - c * cpr;
        const int y = ylo - 1 + e, cb = ct * WX_C + c;
        if (cb < g.C && y >= 0) {                            // else: the zeros stay
            const float* src = w + ((size_t)b * g.C + cb) * HW + (size_t)y * g.W + x8 * 8;
            u32x4 vh, vl;
            wx_split8(*reinterpret_cast<const f32x4*>(src), *reinterpret_cast<const f32x4*>(src + 4), &vh, &vl);
            const int off = ((y + 1) % g.NRING) * ring_row_bytes + (c * g.pitch + 1 + x8) * 16;
            *reinterpret_cast<u32x4*>(ring + off) = vh;
            *reinterpret_cast<u32x4*>(ring + g.ring_plane + off) = vl;
        }
    }
    store_stage(0);
    __syncthreads();

    const int a_row = wk * 32 + r;                            // a fragment: channel row; w fragment: channel column r
    for (int s = 0; s < g.stages_per_wg; ++s) {
        const int y0 = ylo + s * g.RS;
        if (s + 1 < g.stages_per_wg) load_stage(s + 1);       // consumed behind this stage's multiplications
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {                      // this wave's k-steps of 16 pixels
            const int j = 4 * wp + jj;
            const int f8 = 2 * j + h;
            const unsigned char* A = lds + ((a_row << 4) + (f8 ^ (a_row & 15))) * 16;
            const bf16x8 fah = *reinterpret_cast<const bf16x8*>(A), fal = *reinterpret_cast<const bf16x8*>(A + WX_A_PLANE);
            const int p0 = 16 * j;                            // stage pixel of the k-step
            const int rs = p0 >> g.wshift, px = (p0 & (g.W - 1)) + 8 * h;
#pragma unroll
            for (int dy = 0; dy < 3; ++dy) {
                const int slot = (y0 + rs + dy) % g.NRING;    // image row y0 + rs + dy - 1
                const unsigned char* X = ring + slot * ring_row_bytes + (r * g.pitch + 1 + (px >> 3)) * 16;
                u32x4 ctr[2], left[2], right[2];
#pragma unroll
                for (int pl = 0; pl < 2; ++pl) wrw_shifted(X + pl * g.ring_plane, &left[pl], &ctr[pl], &right[pl]);
                f32x16& a0 = acc[dy * 3 + 0];
                f32x16& a1 = acc[dy * 3 + 1];
                f32x16& a2 = acc[dy * 3 + 2];
                // smallest terms first: lo(a) hi(w), hi(a) lo(w), hi(a) hi(w); the three taps alternate so that no MFMA waits for its predecessor
                a0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fal, __builtin_bit_cast(bf16x8, left[0]), a0, 0, 0, 0);
                a1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fal, __builtin_bit_cast(bf16x8, ctr[0]), a1, 0, 0, 0);
                a2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fal, __builtin_bit_cast(bf16x8, right[0]), a2, 0, 0, 0);
                a0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fah, __builtin_bit_cast(bf16x8, left[1]), a0, 0, 0, 0);
                a1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fah, __builtin_bit_cast(bf16x8, ctr[1]), a1, 0, 0, 0);
                a2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fah, __builtin_bit_cast(bf16x8, right[1]), a2, 0, 0, 0);
                a0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fah, __builtin_bit_cast(bf16x8, left[0]), a0, 0, 0, 0);
                a1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fah, __builtin_bit_cast(bf16x8, ctr[0]), a1, 0, 0, 0);
                a2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fah, __builtin_bit_cast(bf16x8, right[0]), a2, 0, 0, 0);
            }
        }
        __syncthreads();                                       // every wave is done reading this stage
        if (s + 1 < g.stages_per_wg) {
            store_stage(s + 1);
            __syncthreads();
        }
    }

    // the two pixel halves of a tile: second half -> LDS (three taps at a time, 48 KB over the a images), first half adds and keeps the sum
    float* red = reinterpret_cast<float*>(lds);
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
        if (wp == 1) {
#pragma unroll
            for (int t = 0; t < 3; ++t)
#pragma unroll
                for (int e = 0; e < 16; ++e) red[((wk * 3 + t) * 16 + e) * 64 + lane] = acc[dy * 3 + t][e];
        }
        __syncthreads();
        if (wp == 0) {
#pragma unroll
            for (int t = 0; t < 3; ++t)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[dy * 3 + t][e] += red[((wk * 3 + t) * 16 + e) * 64 + lane];
        }
        __syncthreads();
    }
    if (wp != 0) return;

    // partial result: slab[split][t][ka][cb] (lanes along cb: coalesced)
    const int Kp = g.ktiles * WX_K, Cp = g.ctiles * WX_C;
    float* out = slabs + (size_t)split * 9 * Kp * Cp;
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int ka = kt * WX_K + wk * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
            out[((size_t)t * Kp + ka) * Cp + ct * WX_C + r] = acc[t][e];
        }
}

// =====================================================================================================================================
// Weight gradient of the k4 s2 p1 layers (Conv2d [Kc][Cf] and ConvTranspose2d [Kc][Cf] alike, in the coarse / fine terms above):
//      dW[kc][cf][r][s] = sum_{b, oy, ox}  coarse[b][kc][oy][ox] * fine[b][cf][2 oy - 1 + r][2 ox - 1 + s]
// The reduction runs over COARSE pixels: the coarse operand's fragments are aligned 16-byte reads as in the k3 kernel; the fine
// operand's 8 consecutive reduction elements are every OTHER pixel of a fine row: a lane reads the 16 fine pixels they span (two
// aligned 16-byte reads + the dword before and after) and picks the even / odd halves with four v_perm_b32 per column tap.
// Workgroup = 8 waves = 4 (kc) x 2 (row taps r in {0,1} / {2,3}): 128 kc x 32 cf x 16 taps, a wave 32 x 32 x 8 taps; stage = 64 coarse
// pixels (RS = 64 / nw coarse rows); the fine rows live in a ring of 4 RS + 2 image rows handled in PAIRS (row 2 i - 1 and 2 i:
// 64 x pitch slots, so a DMA instruction never straddles ring entries); runs of coarse rows are cut over workgroups, the partial
// [t][kc][cf] slabs added in order by the second launch.
// In WrwGeom's terms (both k4 s2 kernels): K = Kc, C = Cf, H x W = the coarse grid nh x nw, NRING = pairs of fine rows.
constexpr int W2_K = WRW_KINDS[WRW_S2].TK, W2_C = WRW_KINDS[WRW_S2].TC, W2_PX = WRW_KINDS[WRW_S2].PX;
constexpr int W2_A_BYTES = W2_K * W2_PX * 2;                 // 16 KB per buffer

__global__ void __launch_bounds__(512, 1) conv_bf16_wrw_s2_kernel(const unsigned short* __restrict__ coarse, const unsigned short* __restrict__ fine,
                                                                   const uint4* __restrict__ zero_page, WrwGeom g, float* __restrict__ slabs)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];          // A[2] | fine-row ring
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wk = wave >> 1, rh = wave & 1;
    const int r = lane & 31, h = lane >> 5;

    const WrwRun run = wrw_decode(g);
    const int kt = run.kt, ct = run.ct, b = run.b, ylo = run.ylo, split = run.split;
    const int Hf = 2 * g.H, Wf = 2 * g.W;
    const size_t HWc = (size_t)g.H * g.W, HWf = (size_t)Hf * Wf;
    const int cprc = g.W >> 3;                               // 16-byte chunks per coarse row
    const int cprf = Wf >> 3;                                // ... per fine row

    // ---- coarse rows: slot sigma = k * 8 + cs holds stage chunk c8 = cs ^ (k & 7) of channel k; c8 -> (coarse row rs, chunk cx) ----------
    const unsigned short* ga[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int sigma = (wave + 8 * j) * 64 + lane;
        const int k = sigma >> 3, c8 = (sigma & 7) ^ (k & 7);
        const int rs = c8 / cprc, cx = c8 - rs * cprc;
        const int kc = kt * W2_K + k;
        ga[j] = kc < g.K ? coarse + ((size_t)b * g.K + kc) * HWc + (size_t)(ylo + rs) * g.W + cx * 8 : nullptr;
    }
    // ---- fine rows: ring entry of the row pair (2 i - 1, 2 i) = i mod NRING; per (row, channel): [halo][Wf / 8 chunks][halo][pad] ---------
    const int pair_slots = 2 * W2_C * g.pitch;               // a multiple of 64
    const unsigned short* gf[5];
    int f_row[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const int q = tid + 512 * j;
        const int within = q % pair_slots;
        const int pr = within / (W2_C * g.pitch), rem = within - pr * (W2_C * g.pitch);
        const int c = rem / g.pitch, sl = rem - c * g.pitch;
        const int cf = ct * W2_C + c;
        f_row[j] = 2 * (q / pair_slots) + pr;                // fine row offset from the first row of the group
        const bool data = sl >= 1 && sl <= cprf && cf < g.C;
        gf[j] = data ? fine + ((size_t)b * g.C + cf) * HWf + (sl - 1) * 8 : nullptr;
    }
    const int pair_bytes = pair_slots * 16;

    f32x16 acc[8];
#pragma unroll
    for (int t = 0; t < 8; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[t][e] = 0.0f;

    auto dma_a = [&](int buf, int stage) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const void* src = ga[j] ? static_cast<const void*>(ga[j] + (size_t)stage * g.RS * g.W) : static_cast<const void*>(zero_page);
            __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(lds + buf * W2_A_BYTES + (wave + 8 * j) * 1024), 16, 0, 0);
        }
    };
    // `npairs` row pairs starting with the pair (2 i0 - 1, 2 i0)
    auto dma_f = [&](int i0, int npairs) {
        const int nslots = npairs * pair_slots;
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const int q0 = wave * 64 + 512 * j;              // uniform
            if (q0 < nslots) {
                const int pp = q0 / pair_slots, within = q0 - pp * pair_slots;
                int entry = (i0 + pp) % g.NRING;
                if (entry < 0) entry += g.NRING;
                const int yf = 2 * i0 - 1 + f_row[j];
                const bool ok = gf[j] != nullptr && (unsigned)yf < (unsigned)Hf;
                const void* src = ok ? static_cast<const void*>(gf[j] + (size_t)yf * Wf) : static_cast<const void*>(zero_page);
                __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(lds + 2 * W2_A_BYTES + entry * pair_bytes + within * 16), 16, 0, 0);
            }
        }
    };

    // a stage on coarse rows y0 .. y0 + RS - 1 reads the fine rows 2 y0 - 1 .. 2 (y0 + RS - 1) + 2 = the pairs y0 .. y0 + RS
    dma_a(0, 0);
    dma_f(ylo, g.RS + 1);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    const int a_row = wk * 32 + r;
    const int row_bytes = W2_C * g.pitch * 16;
    for (int s = 0; s < g.stages_per_wg; ++s) {
        const int cur = s & 1;
        const int y0 = ylo + s * g.RS;
        if (s + 1 < g.stages_per_wg) {
            dma_a(cur ^ 1, s + 1);
            dma_f(y0 + g.RS + 1, g.RS);                       // the pairs the next stage adds
        }
        const unsigned char* A = lds + cur * W2_A_BYTES;
#pragma unroll
        for (int j = 0; j < 4; ++j) {                         // k-steps of 16 coarse pixels
            const int c8 = 2 * j + h;
            const bf16x8 fa = *reinterpret_cast<const bf16x8*>(A + ((a_row << 3) + (c8 ^ (a_row & 7))) * 16);
            const int p0 = 16 * j;
            const int rs = p0 >> g.wshift, ox0 = (p0 & (g.W - 1)) + 8 * h;
#pragma unroll
            for (int ri = 0; ri < 2; ++ri) {
                // fine row 2 (y0 + rs) - 1 + (2 rh + ri) = row (1 - ...) of a pair: row index u = 2 (y0 + rs) + 2 rh + ri  ->  pair u / 2, member u & 1
                const int u = 2 * (y0 + rs) + 2 * rh + ri;    // = fine row + 1
                const int entry = (u >> 1) % g.NRING;
                const unsigned char* X = lds + 2 * W2_A_BYTES + entry * pair_bytes + (u & 1) * row_bytes + (r * g.pitch + 1 + (ox0 >> 2)) * 16;
                u32x4 f[4];                                  // [column tap]
                wrw_pick_even_odd(X, f);
#pragma unroll
                for (int t = 0; t < 4; ++t) acc[ri * 4 + t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, __builtin_bit_cast(bf16x8, f[t]), acc[ri * 4 + t], 0, 0, 0);
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }

    // partial result: slab[split][t = r * 4 + s][kc][cf] (lanes along cf)
    const int Kp = g.ktiles * W2_K, Cp = g.ctiles * W2_C;
    float* out = slabs + (size_t)split * 16 * Kp * Cp;
#pragma unroll
    for (int t = 0; t < 8; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int ka = kt * W2_K + wk * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
            out[((size_t)(rh * 8 + t) * Kp + ka) * Cp + ct * W2_C + r] = acc[t][e];
        }
}

// =====================================================================================================================================
// The same k4 s2 p1 weight gradient on FP32 tensors with split-bf16 operands (ipsr_conv4x4s2_bf16x3_wrw; the opt-in arithmetic
// "direct_bf16x3_s2_dw" of the fp32 nets).  Operands and products as in conv_bf16x3_wrw_kernel: v = hi + lo, hi = bf16(v),
// lo = bf16(v - hi), every product lo*hi + hi*lo + hi*hi into the same fp32 accumulator, smallest terms first, lo*lo dropped.
// Tile, wave layout, fragments (aligned 16-byte coarse reads; 16 consecutive fine pixels + the dword before and after, the even / odd
// halves by v_perm_b32 — now from a hi and a lo image), run cut and slab reduction are conv_bf16_wrw_s2_kernel's.  The plan is
// conv_bf16x3_wrw_kernel's, because two coarse buffers and a (2 RS + 1)-pair ring of hi + lo images do not fit:
//   * the split happens in the kernel, global -> registers -> v_cvt_pk_bf16_f32 -> LDS; the REGISTERS are the second buffer: the loads of
//     stage s + 1 (16 dwords of coarse, 16 of fine per lane) fly during the multiplications of stage s, conversion and stores follow between
//     two barriers, so LDS holds ONE coarse buffer and a ring of the RS + 1 row pairs a stage reads (pair i = fine rows 2 i - 1, 2 i in
//     entry i mod (RS + 1)); the next stage's RS new pairs — 2 RS consecutive fine rows, 256 contiguous floats per channel — replace the
//     RS oldest;
//   * a fine row outside the image (row -1: the ring's initial zeros, written before anything else; row 2 nh: zeros STORED by the stage
//     that would load it, so a slot that held data one stage earlier reads as zeros) and the channels past Cf are zeros; the halo slots
//     of every (row, channel) are zeroed once and never written.
// LDS: coarse hi | lo = 2 x 16 KB; ring hi | lo = 2 x (RS + 1) pairs x 2 rows x 32 cf x (2 nw / 8 + 3) slots x 16 B:
//      nw = 16: 32768 + 71680 = 104448 B     nw = 32: 32768 + 67584 = 100352 B     nw = 64: 32768 + 77824 = 110592 B
// nw = 128 is refused: a stage of 64 coarse pixels is half a coarse row, and a ring of whole fine rows costs 2 planes x 2 pairs x 2 rows x
// 32 cf x 35 slots x 16 B = 143360 B + 32768 = 176128 B > 160 KB of LDS.
// Supported: nw in {16, 32, 64}, nh a multiple of 64 / nw.  Deterministic: no atomics, every sum in a fixed order.
__global__ void __launch_bounds__(512, 1) conv_bf16x3_wrw_s2_kernel(const float* __restrict__ coarse, const float* __restrict__ fine, WrwGeom g,
                                                                     float* __restrict__ slabs)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];          // coarse hi | coarse lo | ring hi | ring lo
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wk = wave >> 1, rh = wave & 1;
    const int r = lane & 31, h = lane >> 5;

    const WrwRun run = wrw_decode(g);
    const int kt = run.kt, ct = run.ct, b = run.b, ylo = run.ylo, split = run.split;
    const int Hf = 2 * g.H, Wf = 2 * g.W;
    const size_t HWc = (size_t)g.H * g.W, HWf = (size_t)Hf * Wf;
    const int cprf = Wf >> 3;                                // 8-pixel chunks per fine row
    unsigned char* const ring = lds + 2 * W2_A_BYTES;
    const int row_bytes = W2_C * g.pitch * 16;
    const int pair_bytes = 2 * row_bytes;

    // ---- coarse rows: a stage's 64 pixels are contiguous in NCHW; a lane owns chunk c8 = tid & 7 of the channels (tid >> 3) + 64 j, slot
    // k * 8 + (c8 ^ (k & 7)) as in the bf16 kernel (k & 7 is the same for both j) --------------------------------------------------------------
    const int c8 = tid & 7, k0 = tid >> 3;
    const float* ga[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int kc = kt * W2_K + k0 + 64 * j;
        ga[j] = kc < g.K ? coarse + ((size_t)b * g.K + kc) * HWc + (size_t)ylo * g.W + c8 * 8 : nullptr;
    }
    const int a_wr = ((k0 << 3) + (c8 ^ (k0 & 7))) * 16;     // + j * 8192
    // ---- fine rows: the 2 RS new rows of a stage are 32 chunks per channel; a lane owns chunk fi = tid & 31 (row fr, chunk fx) of the
    // channels (tid >> 5) + 16 j ------------------------------------------------------------------------------------------------------------
    const int fi = tid & 31, c0 = tid >> 5;
    const int fr = fi / cprf, fx = fi - fr * cprf;
    const float* gf[2];                                      // channels past Cf: a valid address (the last channel), zeros are stored
    bool fok[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int cf = ct * W2_C + c0 + 16 * j;
        fok[j] = cf < g.C;
        gf[j] = fine + ((size_t)b * g.C + (fok[j] ? cf : g.C - 1)) * HWf + fi * 8;
    }
    const int f_wr = (c0 * g.pitch + 1 + fx) * 16;           // + j * 16 * pitch * 16

    f32x16 acc[8];
    wrw_clear(acc);

    f32x4 ar[4], fw[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) ar[i] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};           // channels past Kc stay zeros
    // stage s: its 64 coarse pixels, and the fine rows 2 y0 + 1 .. 2 y0 + 2 RS = the pairs y0 + 1 .. y0 + RS (what stage s reads beyond
    // the last pair of stage s - 1)
    auto load_stage = [&](int s) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
            if (ga[j]) {
                const float* src = ga[j] + (size_t)s * W2_PX;
                ar[2 * j] = *reinterpret_cast<const f32x4*>(src);
                ar[2 * j + 1] = *reinterpret_cast<const f32x4*>(src + 4);
            }
        // unconditional loads (no branch between the loads and the multiplications): the one row that can lie outside the image, row
        // 2 nh, reads row 2 nh - 1 instead and store_stage stores zeros for it
        const int yf0 = 2 * (ylo + s * g.RS) + 1;
        const int yld = yf0 + fr < Hf ? yf0 : yf0 - 1;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const float* src = gf[j] + (size_t)yld * Wf;
            fw[2 * j] = *reinterpret_cast<const f32x4*>(src);
            fw[2 * j + 1] = *reinterpret_cast<const f32x4*>(src + 4);
        }
    };
    auto store_stage = [&](int s) {
        u32x4 vh, vl;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            wx_split8(ar[2 * j], ar[2 * j + 1], &vh, &vl);
            *reinterpret_cast<u32x4*>(lds + a_wr + j * 8192) = vh;
            *reinterpret_cast<u32x4*>(lds + W2_A_BYTES + a_wr + j * 8192) = vl;
        }
        const int u = 2 * (ylo + s * g.RS) + 2 + fr;          // fine row + 1: pair u >> 1, member u & 1
        unsigned char* dst = ring + ((u >> 1) % g.NRING) * pair_bytes + (u & 1) * row_bytes + f_wr;
        const bool inside = u - 1 < Hf;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            wx_split8(fw[2 * j], fw[2 * j + 1], &vh, &vl);
            if (!(inside && fok[j])) vh = vl = u32x4{0u, 0u, 0u, 0u};           // row 2 nh / channel past Cf
            *reinterpret_cast<u32x4*>(dst + j * 16 * g.pitch * 16) = vh;
            *reinterpret_cast<u32x4*>(dst + g.ring_plane + j * 16 * g.pitch * 16) = vl;
        }
    };

    // prologue: the ring starts as zeros (halo slots and row -1 keep them); the pair ylo (rows 2 ylo - 1, 2 ylo), then stage 0
    for (int i = tid; i < 2 * g.ring_plane / 16; i += 512) *reinterpret_cast<u32x4*>(ring + i * 16) = u32x4{0u, 0u, 0u, 0u};
    load_stage(0);
    __syncthreads();
    for (int i = tid; i < 2 * W2_C * cprf; i += 512) {
        const int m = i / (W2_C * cprf), rem = i - m * (W2_C * cprf);
        const int c = rem / cprf, x8 = rem - c * cprf;
        const int y = 2 * ylo - 1 + m, cf = ct * W2_C + c;
        if (cf < g.C && y >= 0) {                            // else: the zeros stay
            const float* src = fine + ((size_t)b * g.C + cf) * HWf + (size_t)y * Wf + x8 * 8;
            u32x4 vh, vl;
            wx_split8(*reinterpret_cast<const f32x4*>(src), *reinterpret_cast<const f32x4*>(src + 4), &vh, &vl);
            const int off = (ylo % g.NRING) * pair_bytes + m * row_bytes + (c * g.pitch + 1 + x8) * 16;
            *reinterpret_cast<u32x4*>(ring + off) = vh;
            *reinterpret_cast<u32x4*>(ring + g.ring_plane + off) = vl;
        }
    }
    store_stage(0);
    __syncthreads();

    const int a_row = wk * 32 + r;
    for (int s = 0; s < g.stages_per_wg; ++s) {
        const int y0 = ylo + s * g.RS;
        if (s + 1 < g.stages_per_wg) load_stage(s + 1);       // consumed behind this stage's multiplications
#pragma unroll
        for (int j = 0; j < 4; ++j) {                         // k-steps of 16 coarse pixels
            const int f8 = 2 * j + h;
            const unsigned char* A = lds + ((a_row << 3) + (f8 ^ (a_row & 7))) * 16;
            const bf16x8 fah = *reinterpret_cast<const bf16x8*>(A), fal = *reinterpret_cast<const bf16x8*>(A + W2_A_BYTES);
            const int p0 = 16 * j;
            const int rs = p0 >> g.wshift, ox0 = (p0 & (g.W - 1)) + 8 * h;
#pragma unroll
            for (int ri = 0; ri < 2; ++ri) {
                const int u = 2 * (y0 + rs) + 2 * rh + ri;    // = fine row + 1 (tap row 2 rh + ri)
                const unsigned char* X = ring + ((u >> 1) % g.NRING) * pair_bytes + (u & 1) * row_bytes + (r * g.pitch + 1 + (ox0 >> 2)) * 16;
                u32x4 f[2][4];                               // [plane][column tap]
#pragma unroll
                for (int pl = 0; pl < 2; ++pl) wrw_pick_even_odd(X + pl * g.ring_plane, f[pl]);
                // smallest terms first: lo(coarse) hi(fine), hi(coarse) lo(fine), hi hi; the four taps alternate so that no MFMA waits for its predecessor
#pragma unroll
                for (int t = 0; t < 4; ++t) acc[ri * 4 + t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fal, __builtin_bit_cast(bf16x8, f[0][t]), acc[ri * 4 + t], 0, 0, 0);
#pragma unroll
                for (int t = 0; t < 4; ++t) acc[ri * 4 + t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fah, __builtin_bit_cast(bf16x8, f[1][t]), acc[ri * 4 + t], 0, 0, 0);
#pragma unroll
                for (int t = 0; t < 4; ++t) acc[ri * 4 + t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fah, __builtin_bit_cast(bf16x8, f[0][t]), acc[ri * 4 + t], 0, 0, 0);
            }
        }
        __syncthreads();                                       // every wave is done reading this stage
        if (s + 1 < g.stages_per_wg) {
            store_stage(s + 1);
            __syncthreads();
        }
    }

    // partial result: slab[split][t = r * 4 + s][kc][cf] (lanes along cf)
    const int Kp = g.ktiles * W2_K, Cp = g.ctiles * W2_C;
    float* out = slabs + (size_t)split * 16 * Kp * Cp;
#pragma unroll
    for (int t = 0; t < 8; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int ka = kt * W2_K + wk * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
            out[((size_t)(rh * 8 + t) * Kp + ka) * Cp + ct * W2_C + r] = acc[t][e];
        }
}

// =====================================================================================================================================
// Weight gradient of the dilated down convolution Conv2d(Cf, Kc, k4, stride 2, pad 3, dilation 2) on FP32 tensors with split-bf16 operands
// (ipsr_conv4x4s2_bf16x3_dil_wrw; the opt-in switch set_direct_dilated_dw of the fp32 nets).  With q(m, n) = fine(2 m + 1, 2 n + 1) the
// layer is a 16-tap stride-1 correlation on the coarse grid (the derivation of the dilated data passes above), so
//      dW[kc][cf][r][s] = sum_{b, oy, ox}  coarse[b][kc][oy][ox] * q[b][cf][oy + r - 2][ox + s - 2]            (q zero outside nh x nw)
// with a halo of 2 in front and 1 behind, in rows and columns; only odd fine rows and odd fine columns are ever read.
// Operands and products as in conv_bf16x3_wrw_kernel (hi + lo, lo*hi + hi*lo + hi*hi, smallest first).  Tile, wave layout (4 kc x 2 row-tap
// pairs), stage (64 coarse pixels), run cut and slab reduction are conv_bf16x3_wrw_s2_kernel's; the fragments are conv_bf16x3_wrw_kernel's:
// unit-stride 16-byte reads of a ring of whole q rows, the column taps s = 0..3 as the shifts -2, -1, 0, +1 of the aligned chunk and its
// neighbouring dwords (wrw_shifted plus the window two pixels to the left, which needs no alignbit).
//   * q is sampled at split time: a thread loads 8 consecutive floats of an odd fine row (two 16-byte loads), keeps the 4 odd ones, and
//     stores 8 bytes into the hi and the lo plane — no de-interleave on the read side.  512 threads x 8 floats = the 256 q chunks of a stage;
//   * q row y lives in ring slot (y + 2) mod NRING; a stage reads rows y0 - 2 .. y0 + RS, so NRING = RS + 3 and the next stage's RS new
//     rows replace the RS oldest.  Rows above the image are the ring's initial zeros (only the first stages of a run at ylo = 0 read them);
//     rows below it are zeros STORED by the stage that would load them (the slot held data a stage earlier), from a load of row nh - 1, so
//     that the loads stay unconditional; channels past Cf likewise.  The halo slots of every (row, channel) are zeroed once, never written;
//   * nw = 128 (WIDE): a stage is half a q row.  The ring is 4 whole rows, a new row (two 8-float loads per thread) arrives every second
//     stage, after the second half of the row above has been multiplied.  In WrwGeom's terms RS = 1 and stages_per_wg counts ROWS.
// LDS: coarse hi | lo = 2 x 16 KB; ring hi | lo = 2 x (RS + 3) rows x 32 cf x (nw / 8 + 3) slots x 16 B:
//      nw = 16: 32768 + 35840 = 68608 B    nw = 32: 32768 + 35840 = 68608 B    nw = 64: 32768 + 45056 = 77824 B    nw = 128: 32768 + 77824 = 110592 B
// Supported: nw in {16, 32, 64, 128}, nh a multiple of max(1, 64 / nw).  Deterministic: no atomics, every sum in a fixed order.

// 8 consecutive fp32 pixels of an odd fine row -> the hi and lo bf16 images (8 bytes each) of the 4 odd ones
__device__ __forceinline__ void wd_split4_odd(const f32x4& v0, const f32x4& v1, u32x2* hi, u32x2* lo)
{
    unsigned h16[4], l16[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float v = i < 2 ? v0[2 * i + 1] : v1[2 * i - 3];
        h16[i] = __builtin_bit_cast(unsigned short, (__bf16)v);
        l16[i] = __builtin_bit_cast(unsigned short, (__bf16)(v - __uint_as_float(h16[i] << 16)));
    }
    *hi = u32x2{h16[0] | (h16[1] << 16), h16[2] | (h16[3] << 16)};
    *lo = u32x2{l16[0] | (l16[1] << 16), l16[2] | (l16[3] << 16)};
}

// the four column taps s of 8 coarse pixels at X (a lane's aligned 16-byte chunk of a ring row): the windows starting at ox - 2 + s
__device__ __forceinline__ void wd_taps(const unsigned char* X, u32x4 (&f)[4])
{
    wrw_shifted(X, &f[1], &f[2], &f[3]);
    const unsigned prev = *reinterpret_cast<const unsigned*>(X - 4);
    f[0] = u32x4{prev, f[2].x, f[2].y, f[2].z};
}

template <bool WIDE>
__global__ void __launch_bounds__(512, 1) conv_bf16x3_wrw_dil_kernel(const float* __restrict__ coarse, const float* __restrict__ fine, WrwGeom g,
                                                                      float* __restrict__ slabs)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];          // coarse hi | coarse lo | ring hi | ring lo
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wk = wave >> 1, rh = wave & 1;
    const int r = lane & 31, h = lane >> 5;

    const WrwRun run = wrw_decode(g);
    const int kt = run.kt, ct = run.ct, b = run.b, ylo = run.ylo, split = run.split;
    const int Wf = 2 * g.W;
    const size_t HWc = (size_t)g.H * g.W, HWf = 4 * HWc;
    const int hpr = g.W >> 2;                                // 4-pixel half chunks per q row
    unsigned char* const ring = lds + 2 * W2_A_BYTES;
    const int row_bytes = W2_C * g.pitch * 16;

    // ---- coarse rows: as in conv_bf16x3_wrw_s2_kernel ---------------------------------------------------------------------------------------
    const int c8 = tid & 7, k0 = tid >> 3;
    const float* ga[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int kc = kt * W2_K + k0 + 64 * j;
        ga[j] = kc < g.K ? coarse + ((size_t)b * g.K + kc) * HWc + (size_t)ylo * g.W + c8 * 8 : nullptr;
    }
    const int a_wr = ((k0 << 3) + (c8 ^ (k0 & 7))) * 16;     // + j * 8192
    // ---- q rows: the new rows of a stage (WIDE: of a row) are 16 (32) half chunks per channel; a lane owns half chunk (tid & 15) + 16 j
    // (row fr, half chunk fx) of channel tid >> 4 -----------------------------------------------------------------------------------------
    constexpr int NQ = WIDE ? 2 : 1;
    const int c0 = tid >> 4;
    const bool fok = ct * W2_C + c0 < g.C;                   // channels past Cf: a valid address (the last channel), zeros are stored
    const float* gq = fine + ((size_t)b * g.C + (fok ? ct * W2_C + c0 : g.C - 1)) * HWf + Wf;        // q row 0 = fine row 1
    int fr[NQ], fx[NQ];
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
        const int hi = (tid & 15) + 16 * j;
        fr[j] = hi >> (g.wshift - 2); fx[j] = hi & (hpr - 1);
    }
    const int q_wr = (c0 * g.pitch + 1) * 16;                // + fx * 8

    f32x16 acc[8];
    wrw_clear(acc);

    f32x4 ar[4], fw[2 * NQ];
#pragma unroll
    for (int i = 0; i < 4; ++i) ar[i] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};           // channels past Kc stay zeros
    // step st: its 64 coarse pixels
    auto load_a = [&](int st) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
            if (ga[j]) {
                const float* src = ga[j] + (size_t)st * W2_PX;
                ar[2 * j] = *reinterpret_cast<const f32x4*>(src);
                ar[2 * j + 1] = *reinterpret_cast<const f32x4*>(src + 4);
            }
    };
    auto store_a = [&]() {
        u32x4 vh, vl;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            wx_split8(ar[2 * j], ar[2 * j + 1], &vh, &vl);
            *reinterpret_cast<u32x4*>(lds + a_wr + j * 8192) = vh;
            *reinterpret_cast<u32x4*>(lds + W2_A_BYTES + a_wr + j * 8192) = vl;
        }
    };
    // unit u (a stage; WIDE: a row): the q rows y0 + 1 .. y0 + RS, what it reads beyond the rows of unit u - 1.  Unconditional loads: a row
    // below the image reads row nh - 1 instead and store_q stores zeros for it
    auto load_q = [&](int u) {
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
            const int y = ylo + u * g.RS + 1 + fr[j];
            const float* src = gq + (size_t)(y < g.H ? y : g.H - 1) * (2 * Wf) + fx[j] * 8;
            fw[2 * j] = *reinterpret_cast<const f32x4*>(src);
            fw[2 * j + 1] = *reinterpret_cast<const f32x4*>(src + 4);
        }
    };
    auto store_q = [&](int u) {
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
            const int y = ylo + u * g.RS + 1 + fr[j];
            u32x2 vh, vl;
            wd_split4_odd(fw[2 * j], fw[2 * j + 1], &vh, &vl);
            if (!(y < g.H && fok)) vh = vl = u32x2{0u, 0u};                      // row below the image / channel past Cf
            unsigned char* dst = ring + ((y + 2) % g.NRING) * row_bytes + q_wr + fx[j] * 8;
            *reinterpret_cast<u32x2*>(dst) = vh;
            *reinterpret_cast<u32x2*>(dst + g.ring_plane) = vl;
        }
    };

    // prologue: the ring starts as zeros (halo slots and the rows above the image keep them); rows ylo - 2 .. ylo, then unit 0
    for (int i = tid; i < 2 * g.ring_plane / 16; i += 512) *reinterpret_cast<u32x4*>(ring + i * 16) = u32x4{0u, 0u, 0u, 0u};
    load_a(0);
    load_q(0);
    __syncthreads();
    for (int i = tid; i < 3 * W2_C * hpr; i += 512) {
        const int m = i / (W2_C * hpr), rem = i - m * (W2_C * hpr);
        const int c = rem / hpr, x4 = rem - c * hpr;
        const int y = ylo - 2 + m, cf = ct * W2_C + c;
        if (cf < g.C && y >= 0) {                            // else: the zeros stay
            const float* src = fine + ((size_t)b * g.C + cf) * HWf + (size_t)(2 * y + 1) * Wf + x4 * 8;
            u32x2 vh, vl;
            wd_split4_odd(*reinterpret_cast<const f32x4*>(src), *reinterpret_cast<const f32x4*>(src + 4), &vh, &vl);
            const int off = ((y + 2) % g.NRING) * row_bytes + (c * g.pitch + 1) * 16 + x4 * 8;
            *reinterpret_cast<u32x2*>(ring + off) = vh;
            *reinterpret_cast<u32x2*>(ring + g.ring_plane + off) = vl;
        }
    }
    store_a();
    store_q(0);
    __syncthreads();

    const int a_row = wk * 32 + r;
    const int nsteps = WIDE ? 2 * g.stages_per_wg : g.stages_per_wg;
    for (int st = 0; st < nsteps; ++st) {
        const int y0 = ylo + (WIDE ? st >> 1 : st * g.RS);
        const bool more = st + 1 < nsteps, new_rows = more && (!WIDE || (st & 1));
        if (more) load_a(st + 1);                             // consumed behind this step's multiplications
        if (new_rows) load_q(WIDE ? (st + 1) >> 1 : st + 1);
#pragma unroll
        for (int j = 0; j < 4; ++j) {                         // k-steps of 16 coarse pixels
            const int f8 = 2 * j + h;
            const unsigned char* A = lds + ((a_row << 3) + (f8 ^ (a_row & 7))) * 16;
            const bf16x8 fah = *reinterpret_cast<const bf16x8*>(A), fal = *reinterpret_cast<const bf16x8*>(A + W2_A_BYTES);
            const int p0 = 16 * j + (WIDE ? 64 * (st & 1) : 0);
            const int rs = WIDE ? 0 : p0 >> g.wshift, ox0 = (p0 & (g.W - 1)) + 8 * h;
#pragma unroll
            for (int ri = 0; ri < 2; ++ri) {
                const int slot = (y0 + rs + 2 * rh + ri) % g.NRING;             // q row y0 + rs + (tap row 2 rh + ri) - 2
                const unsigned char* X = ring + slot * row_bytes + (r * g.pitch + 1 + (ox0 >> 3)) * 16;
                u32x4 f[2][4];                               // [plane][column tap]
#pragma unroll
                for (int pl = 0; pl < 2; ++pl) wd_taps(X + pl * g.ring_plane, f[pl]);
                // smallest terms first: lo(coarse) hi(q), hi(coarse) lo(q), hi hi; the four taps alternate so that no MFMA waits for its predecessor
#pragma unroll
                for (int t = 0; t < 4; ++t) acc[ri * 4 + t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fal, __builtin_bit_cast(bf16x8, f[0][t]), acc[ri * 4 + t], 0, 0, 0);
#pragma unroll
                for (int t = 0; t < 4; ++t) acc[ri * 4 + t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fah, __builtin_bit_cast(bf16x8, f[1][t]), acc[ri * 4 + t], 0, 0, 0);
#pragma unroll
                for (int t = 0; t < 4; ++t) acc[ri * 4 + t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fah, __builtin_bit_cast(bf16x8, f[0][t]), acc[ri * 4 + t], 0, 0, 0);
            }
        }
        __syncthreads();                                       // every wave is done reading this step
        if (more) {
            store_a();
            if (new_rows) store_q(WIDE ? (st + 1) >> 1 : st + 1);
            __syncthreads();
        }
    }

    // partial result: slab[split][t = r * 4 + s][kc][cf] (lanes along cf)
    const int Kp = g.ktiles * W2_K, Cp = g.ctiles * W2_C;
    float* out = slabs + (size_t)split * 16 * Kp * Cp;
#pragma unroll
    for (int t = 0; t < 8; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int ka = kt * W2_K + wk * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
            out[((size_t)(rh * 8 + t) * Kp + ka) * Cp + ct * W2_C + r] = acc[t][e];
        }
}

// =====================================================================================================================================
// The same dilated weight gradient on BF16 tensors (ipsr_conv4x4s2_bf16_dil_wrw; the opt-in switch set_direct_dilated_bf16_dw under bf16
// activations): one plane and ONE MFMA per product.  Work split, slab store and reduction are conv_bf16_wrw_s2_kernel's, as is the coarse
// operand: double-buffered by LDS-DMA, 2 x 16 KB, XOR-swizzled chunks, channels past Kc from the zero page.  The q ring, its zero rows, the
// column-tap fragments (wd_taps) and the 128-wide form are conv_bf16x3_wrw_dil_kernel's with the one plane:
//   * q is sampled on the way in: a thread loads 16 bytes (8 bf16) of an odd fine row into registers behind the previous step's
//     multiplications, keeps the 4 odd pixels (two v_perm_b32) and stores 8 bytes.  No even fine row is loaded, no even fine column is stored;
//   * q row y lives in ring slot (y + 2) mod (RS + 3); rows -2 and -1 are the ring's initial zeros, a row at or past nh loads row nh - 1 and
//     stores zeros, channels past Cf store zeros, the halo slots (one in front of and one behind every (row, channel)) are zeroed once;
//   * nw = 128 (WIDE): a step is half a q row, RS = 1, stages_per_wg counts ROWS, the ring is 4 rows.
// A step that brings new rows has two barriers (every wave done reading the ring | the new rows stored, the coarse DMA landed); one otherwise.
// LDS: coarse 2 x 16 KB; ring (RS + 3) rows x 32 cf x (nw / 8 + 3) slots x 16 B:
//      nw = 16: 32768 + 17920 = 50688 B    nw = 32: 32768 + 17920 = 50688 B    nw = 64: 32768 + 22528 = 55296 B    nw = 128: 32768 + 38912 = 71680 B
// Supported: nw in {16, 32, 64, 128}, nh a multiple of max(1, 64 / nw).  Deterministic: no atomics, every sum in a fixed order.

// 8 consecutive bf16 pixels of an odd fine row -> the 4 odd ones
__device__ __forceinline__ u32x2 wd_pick4_odd(const u32x4& v) { return u32x2{pack_hi(v.x, v.y), pack_hi(v.z, v.w)}; }

template <bool WIDE>
__global__ void __launch_bounds__(512, 1) conv_bf16_wrw_dil_kernel(const unsigned short* __restrict__ coarse, const unsigned short* __restrict__ fine,
                                                                    const uint4* __restrict__ zero_page, WrwGeom g, float* __restrict__ slabs)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];          // A[2] | q-row ring
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wk = wave >> 1, rh = wave & 1;
    const int r = lane & 31, h = lane >> 5;

    const WrwRun run = wrw_decode(g);
    const int kt = run.kt, ct = run.ct, b = run.b, ylo = run.ylo, split = run.split;
    const int Wf = 2 * g.W;
    const size_t HWc = (size_t)g.H * g.W, HWf = 4 * HWc;
    const int hpr = g.W >> 2;                                // 4-pixel half chunks per q row
    unsigned char* const ring = lds + 2 * W2_A_BYTES;
    const int row_bytes = W2_C * g.pitch * 16;

    // ---- coarse rows: slot sigma = k * 8 + cs holds step chunk c8 = cs ^ (k & 7) of channel k; a step's 64 pixels are contiguous ------------
    const unsigned short* ga[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int sigma = (wave + 8 * j) * 64 + lane;
        const int k = sigma >> 3, c8 = (sigma & 7) ^ (k & 7);
        const int kc = kt * W2_K + k;
        ga[j] = kc < g.K ? coarse + ((size_t)b * g.K + kc) * HWc + (size_t)ylo * g.W + c8 * 8 : nullptr;
    }
    // ---- q rows: as in conv_bf16x3_wrw_dil_kernel: a lane owns half chunk (tid & 15) + 16 j (row fr, half chunk fx) of channel tid >> 4 -----
    constexpr int NQ = WIDE ? 2 : 1;
    const int c0 = tid >> 4;
    const bool fok = ct * W2_C + c0 < g.C;                   // channels past Cf: a valid address (the last channel), zeros are stored
    const unsigned short* gq = fine + ((size_t)b * g.C + (fok ? ct * W2_C + c0 : g.C - 1)) * HWf + Wf;          // q row 0 = fine row 1
    int fr[NQ], fx[NQ];
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
        const int hi = (tid & 15) + 16 * j;
        fr[j] = hi >> (g.wshift - 2); fx[j] = hi & (hpr - 1);
    }
    const int q_wr = (c0 * g.pitch + 1) * 16;                // + fx * 8

    f32x16 acc[8];
#pragma unroll
    for (int t = 0; t < 8; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[t][e] = 0.0f;

    auto dma_a = [&](int buf, int st) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const void* src = ga[j] ? static_cast<const void*>(ga[j] + (size_t)st * W2_PX) : static_cast<const void*>(zero_page);
            __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(lds + buf * W2_A_BYTES + (wave + 8 * j) * 1024), 16, 0, 0);
        }
    };
    u32x4 fw[NQ];
    // unit u (a stage; WIDE: a row): the q rows y0 + 1 .. y0 + RS, what it reads beyond the rows of unit u - 1.  Unconditional loads: a row
    // below the image reads row nh - 1 instead and store_q stores zeros for it
    auto load_q = [&](int u) {
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
            const int y = ylo + u * g.RS + 1 + fr[j];
            fw[j] = *reinterpret_cast<const u32x4*>(gq + (size_t)(y < g.H ? y : g.H - 1) * (2 * Wf) + fx[j] * 8);
        }
    };
    auto store_q = [&](int u) {
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
            const int y = ylo + u * g.RS + 1 + fr[j];
            u32x2 v = wd_pick4_odd(fw[j]);
            if (!(y < g.H && fok)) v = u32x2{0u, 0u};                            // row below the image / channel past Cf
            *reinterpret_cast<u32x2*>(ring + ((y + 2) % g.NRING) * row_bytes + q_wr + fx[j] * 8) = v;
        }
    };

    // prologue: the ring starts as zeros (halo slots and the rows above the image keep them); rows ylo - 2 .. ylo, then unit 0
    for (int i = tid; i < g.ring_plane / 16; i += 512) *reinterpret_cast<u32x4*>(ring + i * 16) = u32x4{0u, 0u, 0u, 0u};
    dma_a(0, 0);
    load_q(0);
    __syncthreads();
    for (int i = tid; i < 3 * W2_C * hpr; i += 512) {
        const int m = i / (W2_C * hpr), rem = i - m * (W2_C * hpr);
        const int c = rem / hpr, x4 = rem - c * hpr;
        const int y = ylo - 2 + m, cf = ct * W2_C + c;
        if (cf < g.C && y >= 0) {                            // else: the zeros stay
            const unsigned short* src = fine + ((size_t)b * g.C + cf) * HWf + (size_t)(2 * y + 1) * Wf + x4 * 8;
            *reinterpret_cast<u32x2*>(ring + ((y + 2) % g.NRING) * row_bytes + (c * g.pitch + 1) * 16 + x4 * 8) = wd_pick4_odd(*reinterpret_cast<const u32x4*>(src));
        }
    }
    store_q(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    const int a_row = wk * 32 + r;
    const int nsteps = WIDE ? 2 * g.stages_per_wg : g.stages_per_wg;
    for (int st = 0; st < nsteps; ++st) {
        const int cur = st & 1;
        const int y0 = ylo + (WIDE ? st >> 1 : st * g.RS);
        const bool more = st + 1 < nsteps, new_rows = more && (!WIDE || (st & 1));
        if (more) dma_a(cur ^ 1, st + 1);                     // lands behind this step's multiplications
        if (new_rows) load_q(WIDE ? (st + 1) >> 1 : st + 1);
        const unsigned char* A = lds + cur * W2_A_BYTES;
#pragma unroll
        for (int j = 0; j < 4; ++j) {                         // k-steps of 16 coarse pixels
            const int f8 = 2 * j + h;
            const bf16x8 fa = *reinterpret_cast<const bf16x8*>(A + ((a_row << 3) + (f8 ^ (a_row & 7))) * 16);
            const int p0 = 16 * j + (WIDE ? 64 * (st & 1) : 0);
            const int rs = WIDE ? 0 : p0 >> g.wshift, ox0 = (p0 & (g.W - 1)) + 8 * h;
#pragma unroll
            for (int ri = 0; ri < 2; ++ri) {
                const int slot = (y0 + rs + 2 * rh + ri) % g.NRING;             // q row y0 + rs + (tap row 2 rh + ri) - 2
                u32x4 f[4];                                  // [column tap]
                wd_taps(ring + slot * row_bytes + (r * g.pitch + 1 + (ox0 >> 3)) * 16, f);
#pragma unroll
                for (int t = 0; t < 4; ++t) acc[ri * 4 + t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, __builtin_bit_cast(bf16x8, f[t]), acc[ri * 4 + t], 0, 0, 0);
            }
        }
        if (new_rows) {
            __syncthreads();                                  // every wave is done reading the rows the new ones replace
            store_q(WIDE ? (st + 1) >> 1 : st + 1);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }

    // partial result: slab[split][t = r * 4 + s][kc][cf] (lanes along cf)
    const int Kp = g.ktiles * W2_K, Cp = g.ctiles * W2_C;
    float* out = slabs + (size_t)split * 16 * Kp * Cp;
#pragma unroll
    for (int t = 0; t < 8; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int ka = kt * W2_K + wk * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
            out[((size_t)(rh * 8 + t) * Kp + ka) * Cp + ct * W2_C + r] = acc[t][e];
        }
}

// ---- the host side of the six weight-gradient kernels: one planner, one byte count, one launcher over WRW_KINDS ----
static size_t wrw_lds_bytes(const WrwKind& k, const WrwGeom& g) { return 2 * (size_t)k.TK * k.PX * 2 + (k.split ? 2 : 1) * (size_t)g.ring_plane; }

// The limits, before any launch (3x3: K = Ka, C = Cb, the image H x W; k4 s2: K = Kc, C = Cf, the coarse grid nh x nw).
static int wrw_geometry(int kind, int B, int K, int C, int H, int W, WrwGeom* g)
{
    const WrwKind& k = WRW_KINDS[kind];
    if (kind == WRW_S2_SPLIT && W == 128)
        return fail(IPSR_ERR_UNSUPPORTED, "%s: coarse width 128: the ring of whole fine rows for a half-row stage needs 176128 bytes of LDS (16, 32 or 64)", k.who);
    if (W != 16 && W != 32 && W != 64 && W != k.wmax) return fail(IPSR_ERR_UNSUPPORTED, k.width_fmt, k.who, W);
    const int RS = k.PX >= W ? k.PX / W : 1;                  // the dilated kernel at W = 128: a stage is half a row, the cut is by rows
    if (H % RS != 0) return fail(IPSR_ERR_UNSUPPORTED, k.rows_fmt, k.who, H, RS);
    g->B = B; g->K = K; g->C = C; g->H = H; g->W = W;
    g->wshift = cb_wshift(W);
    g->RS = RS; g->NRING = k.ring_mul * RS + k.ring_add; g->pitch = k.wscale * W / 8 + 3;
    g->ktiles = (K + k.TK - 1) / k.TK; g->ctiles = (C + k.TC - 1) / k.TC;
    const int entry_slots = k.wscale * k.TC * g->pitch;       // 16-byte slots of a ring entry
    g->ring_plane = g->NRING * entry_slots * 16;
    if (wrw_lds_bytes(k, *g) > (size_t)CB_LDS_MAX || (k.dma_add >= 0 && (RS + k.dma_add) * entry_slots > 5 * WB_THREADS))
        return fail(IPSR_ERR_UNSUPPORTED, k.ring_fmt, k.who, W);
    cb_cut_runs(g->ktiles * g->ctiles, B, H / RS, &g->stages_per_wg, &g->nsplit);
    return IPSR_OK;
}

// [bf16: the zero page |] the partial slabs
static size_t wrw_ws_bytes(int kind, int B, int K, int C, int H, int W)
{
    const WrwKind& k = WRW_KINDS[kind];
    WrwGeom g;
    if (wrw_geometry(kind, B, K, C, H, W, &g) != IPSR_OK) return 0;
    return (k.split ? 0 : 256) + (size_t)g.nsplit * k.NT * g.ktiles * k.TK * g.ctiles * k.TC * 4;
}

// a [B,K,H,W], w [B,C,wscale H,wscale W] (the dilated kinds: [B,C,2H,2W]) (bf16, or fp32 for the split kinds) -> dW [K][C][NT] fp32
template <int KIND>
static int launch_wrw(const void* a, const void* w, float* dW, int B, int K, int C, int H, int W, void* ws, size_t ws_bytes, hipStream_t st)
{
    constexpr WrwKind k = WRW_KINDS[KIND];
    WrwGeom g;
    if (int rc = wrw_geometry(KIND, B, K, C, H, W, &g)) return rc;
    const size_t need = wrw_ws_bytes(KIND, B, K, C, H, W);
    if (ws_bytes < need) return fail(IPSR_ERR_WORKSPACE, "%s: workspace %zu < %zu", k.who, ws_bytes, need);
    const uint4* zero_page = static_cast<const uint4*>(ws);   // bf16 kinds: what the LDS-DMA reads outside the image and past the channels
    float* slabs = reinterpret_cast<float*>(static_cast<unsigned char*>(ws) + (k.split ? 0 : 256));
    if (!k.split && hipMemsetAsync(ws, 0, 64, st) != hipSuccess) return fail(IPSR_ERR_LAUNCH, "%s: hipMemsetAsync failed", k.who);
    const unsigned grid = (unsigned)(g.ktiles * g.ctiles * g.nsplit);
    const size_t smem = wrw_lds_bytes(k, g);
    const void* kernel;
    if constexpr (KIND == WRW_3X3) kernel = reinterpret_cast<const void*>(&conv_bf16_wrw_kernel);
    else if constexpr (KIND == WRW_3X3_SPLIT) kernel = reinterpret_cast<const void*>(&conv_bf16x3_wrw_kernel);
    else if constexpr (KIND == WRW_S2) kernel = reinterpret_cast<const void*>(&conv_bf16_wrw_s2_kernel);
    else if constexpr (KIND == WRW_S2_SPLIT) kernel = reinterpret_cast<const void*>(&conv_bf16x3_wrw_s2_kernel);
    else if constexpr (KIND == WRW_DIL_SPLIT)
        kernel = W == 128 ? reinterpret_cast<const void*>(&conv_bf16x3_wrw_dil_kernel<true>) : reinterpret_cast<const void*>(&conv_bf16x3_wrw_dil_kernel<false>);
    else {
        static_assert(KIND == WRW_DIL, "one branch per row of WRW_KINDS");
        kernel = W == 128 ? reinterpret_cast<const void*>(&conv_bf16_wrw_dil_kernel<true>) : reinterpret_cast<const void*>(&conv_bf16_wrw_dil_kernel<false>);
    }
    if (int rc = raise_dynamic_lds(kernel, k.kernel, CB_LDS_MAX)) return rc;
    profile_mark_start(st, 4);
    if constexpr (KIND == WRW_3X3)
        conv_bf16_wrw_kernel<<<grid, WB_THREADS, smem, st>>>(static_cast<const unsigned short*>(a), static_cast<const unsigned short*>(w), zero_page, g, slabs);
    else if constexpr (KIND == WRW_3X3_SPLIT)
        conv_bf16x3_wrw_kernel<<<grid, WB_THREADS, smem, st>>>(static_cast<const float*>(a), static_cast<const float*>(w), g, slabs);
    else if constexpr (KIND == WRW_S2)
        conv_bf16_wrw_s2_kernel<<<grid, WB_THREADS, smem, st>>>(static_cast<const unsigned short*>(a), static_cast<const unsigned short*>(w), zero_page, g, slabs);
    else if constexpr (KIND == WRW_S2_SPLIT)
        conv_bf16x3_wrw_s2_kernel<<<grid, WB_THREADS, smem, st>>>(static_cast<const float*>(a), static_cast<const float*>(w), g, slabs);
    else if constexpr (KIND == WRW_DIL_SPLIT) {
        if (W == 128) conv_bf16x3_wrw_dil_kernel<true><<<grid, WB_THREADS, smem, st>>>(static_cast<const float*>(a), static_cast<const float*>(w), g, slabs);
        else conv_bf16x3_wrw_dil_kernel<false><<<grid, WB_THREADS, smem, st>>>(static_cast<const float*>(a), static_cast<const float*>(w), g, slabs);
    } else {
        const unsigned short *ca = static_cast<const unsigned short*>(a), *fw = static_cast<const unsigned short*>(w);
        if (W == 128) conv_bf16_wrw_dil_kernel<true><<<grid, WB_THREADS, smem, st>>>(ca, fw, zero_page, g, slabs);
        else conv_bf16_wrw_dil_kernel<false><<<grid, WB_THREADS, smem, st>>>(ca, fw, zero_page, g, slabs);
    }
    const double px = (double)B * H * W;
    profile_mark_stop(st, 4, (k.split ? 3.0 : 1.0) * 2.0 * k.NT * (double)(g.ktiles * k.TK) * (g.ctiles * k.TC) * px, 2.0 * k.NT * (double)K * C * px);
    if (int rc = check_launch(k.kernel)) return rc;
    cb_slab_reduce_kernel<k.NT><<<dim3(cdiv(C, 256), K), 256, 0, st>>>(slabs, g.nsplit, K, C, g.ktiles * k.TK, g.ctiles * k.TC, dW);
    return check_launch(k.reduce);
}

}  // namespace ipsr

using namespace ipsr;

// The argument checks of the entries below; `who` = the entry's name as its messages have always spelled it, `what` = the pointers the
// kernels read and write as 16-byte vectors (uint4 rows of bf16, 4-element vectors of fp32).
static bool cb_dims_ok(bool code_ok, std::initializer_list<int> dims) { for (int d : dims) code_ok = code_ok && d >= 1; return code_ok; }
static int cb_bad_dims(const char* who, bool code_ok, std::initializer_list<int> dims) { return cb_dims_ok(code_ok, dims) ? IPSR_OK : fail(IPSR_ERR_INVALID, "%s: bad argument", who); }
static int cb_null(const char* who, std::initializer_list<const void*> ptrs)
{
    for (const void* p : ptrs) if (!p) return fail(IPSR_ERR_INVALID, "%s: null pointer", who);
    return IPSR_OK;
}
static int cb_misaligned(const char* who, const char* what, std::initializer_list<const void*> ptrs)
{
    for (const void* p : ptrs) if (reinterpret_cast<uintptr_t>(p) & 15u) return fail(IPSR_ERR_INVALID, "%s: %s must be 16-byte aligned", who, what);
    return IPSR_OK;
}

// modes of the k4 s2 entries: bit 0 = coarse -> fine, bit 2 = pad 3, dilation 2 (ipsr_conv4x4s2_bf16x3 only; ipsr_conv4x4s2_bf16_dil is the
// dilated layer on bf16 tensors with modes 0 / 1) -> the form
static bool c2_mode_ok(int mode) { return mode == 0 || mode == 1 || mode == 4 || mode == 5; }
static int c2_form(int mode) { return ((mode & 4) ? CB_DF2C : CB_F2C) + (mode & 1); }

extern "C" {

size_t ipsr_conv3x3_bf16_workspace_bytes(int op, int B, int Cin, int H, int W, int Cout)
{
    if (!cb_dims_ok(op >= 0 && op <= 3, {B, Cin, Cout, H, W})) return 0;
    const bool fwd = op == 0 || op == 2;
    return data_ws_query(DATA_K3, CB_S1, B, fwd ? Cin : Cout, fwd ? Cout : Cin, H, W);
}

size_t ipsr_conv3x3_bf16x3_workspace_bytes(int op, int B, int Cin, int H, int W, int Cout)
{
    if (cb_bad_dims("ipsr_conv3x3_bf16x3_workspace_bytes", op >= 0 && op <= 3, {B, Cin, Cout, H, W})) return 0;
    const bool fwd = op == 0 || op == 2;
    return data_ws_query(DATA_K3_SPLIT, CB_S1, B, fwd ? Cin : Cout, fwd ? Cout : Cin, H, W);
}

int ipsr_conv3x3_bf16(int op, const void* in, const float* weight, void* out, int B, int Cin, int H, int W, int Cout, int io,
                      void* ws, size_t ws_bytes, void* stream)
{
    return ipsr_conv3x3_bf16_packed(op, in, weight, out, B, Cin, H, W, Cout, io, 0, ws, ws_bytes, stream);
}

int ipsr_conv3x3_bf16_packed(int op, const void* in, const float* weight, void* out, int B, int Cin, int H, int W, int Cout, int io,
                             int pack_valid, void* ws, size_t ws_bytes, void* stream)
{
    if (int rc = cb_null("ipsr_conv3x3_bf16", {in, weight, out, ws})) return rc;
    if (int rc = cb_bad_dims("ipsr_conv3x3_bf16", op >= 0 && op <= 3, {B, Cin, Cout, H, W})) return rc;
    if (io < 0 || io > 2) return fail(IPSR_ERR_INVALID, "ipsr_conv3x3_bf16: io code %d (0 bf16 -> fp32, 1 bf16 -> bf16, 2 fp32 -> fp32 on split-bf16 operands)", io);
    if (int rc = cb_misaligned("ipsr_conv3x3_bf16", "in / out / workspace", {ws, in, out})) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool fwd = op == 0 || op == 2;
    const int C = fwd ? Cin : Cout, K = fwd ? Cout : Cin;      // reduction / produced channels
    // (sc, sk, flip) as in ipsr_conv3x3_winograd_mp: weight element (reduction channel c, produced channel k, tap) at w[c * sc + k * sk + tap]
    const long wc = (long)(op < 2 ? Cin : Cout) * 9;           // stride of the weight's first dimension
    const long sc = (op == 0 || op == 3) ? 9 : wc, sk = (op == 0 || op == 3) ? wc : 9;
    const int flip = op == 1 || op == 2;
    if (io == 2) return launch_data<DATA_K3_SPLIT, CB_S1>(in, weight, out, B, C, K, H, W, sc, sk, flip, 0, ws, ws_bytes, st, pack_valid);
    return launch_data<DATA_K3, CB_S1>(in, weight, out, B, C, K, H, W, sc, sk, flip, io, ws, ws_bytes, st, pack_valid);
}

size_t ipsr_conv4x4s2_bf16_workspace_bytes(int mode, int B, int Kc, int Cf, int nh, int nw)
{
    if (!cb_dims_ok(mode == 0 || mode == 1, {B, Kc, Cf, nh, nw})) return 0;
    return data_ws_query(DATA_S2, c2_form(mode), B, mode == 0 ? Cf : Kc, mode == 0 ? Kc : Cf, nh, nw);
}

int ipsr_conv4x4s2_bf16(int mode, const void* in, const float* weight, void* out, int B, int Kc, int Cf, int nh, int nw, int out_bf16,
                        void* ws, size_t ws_bytes, void* stream)
{
    if (int rc = cb_null("ipsr_conv4x4s2_bf16", {in, weight, out, ws})) return rc;
    if (int rc = cb_bad_dims("ipsr_conv4x4s2_bf16", mode == 0 || mode == 1, {B, Kc, Cf, nh, nw})) return rc;
    if (int rc = cb_misaligned("ipsr_conv4x4s2_bf16", "in / out / workspace", {ws, in, out})) return rc;
    // weight [Kc][Cf][4][4] in both modules (Conv2d: [Cout][Cin], ConvTranspose2d: [Cin][Cout]), as in ipsr_conv4x4s2_winograd
    const auto launch = mode == 0 ? launch_data_s2<DATA_S2, CB_F2C> : launch_data_s2<DATA_S2, CB_C2F>;
    return launch(in, weight, out, B, Kc, Cf, nh, nw, out_bf16, ws, ws_bytes, static_cast<hipStream_t>(stream));
}

size_t ipsr_conv4x4s2_bf16_dil_workspace_bytes(int mode, int B, int Kc, int Cf, int nh, int nw)
{
    if (!cb_dims_ok(mode == 0 || mode == 1, {B, Kc, Cf, nh, nw})) return 0;
    return data_ws_query(DATA_S2_DIL, c2_form(mode | 4), B, mode == 0 ? Cf : Kc, mode == 0 ? Kc : Cf, nh, nw);
}

int ipsr_conv4x4s2_bf16_dil(int mode, const void* in, const float* weight, void* out, int B, int Kc, int Cf, int nh, int nw, int out_bf16,
                            void* ws, size_t ws_bytes, void* stream)
{
    if (int rc = cb_null("ipsr_conv4x4s2_bf16_dil", {in, weight, out, ws})) return rc;
    if (int rc = cb_bad_dims("ipsr_conv4x4s2_bf16_dil", mode == 0 || mode == 1, {B, Kc, Cf, nh, nw})) return rc;
    if (int rc = cb_misaligned("ipsr_conv4x4s2_bf16_dil", "in / out / workspace", {ws, in, out})) return rc;
    const auto launch = mode == 0 ? launch_data_s2<DATA_S2_DIL, CB_DF2C> : launch_data_s2<DATA_S2_DIL, CB_DC2F>;
    return launch(in, weight, out, B, Kc, Cf, nh, nw, out_bf16, ws, ws_bytes, static_cast<hipStream_t>(stream));
}

size_t ipsr_conv4x4s2_bf16x3_workspace_bytes(int mode, int B, int Kc, int Cf, int nh, int nw)
{
    if (cb_bad_dims("ipsr_conv4x4s2_bf16x3_workspace_bytes", c2_mode_ok(mode), {B, Kc, Cf, nh, nw})) return 0;
    return data_ws_query(DATA_S2_SPLIT, c2_form(mode), B, (mode & 1) ? Kc : Cf, (mode & 1) ? Cf : Kc, nh, nw);
}

int ipsr_conv4x4s2_bf16x3(int mode, const float* in, const float* weight, float* out, int B, int Kc, int Cf, int nh, int nw,
                          void* ws, size_t ws_bytes, void* stream)
{
    if (int rc = cb_null("ipsr_conv4x4s2_bf16x3", {in, weight, out, ws})) return rc;
    if (!cb_dims_ok(c2_mode_ok(mode), {B, Kc, Cf, nh, nw}))
        return fail(IPSR_ERR_INVALID, "ipsr_conv4x4s2_bf16x3: bad argument (mode %d: 0 fine -> coarse, 1 coarse -> fine; 4, 5 the same with pad 3, dilation 2)", mode);
    if (int rc = cb_misaligned("ipsr_conv4x4s2_bf16x3", "in / out / workspace", {ws, in, out})) return rc;
    const auto launch = mode == 0 ? launch_data_s2<DATA_S2_SPLIT, CB_F2C> : mode == 1 ? launch_data_s2<DATA_S2_SPLIT, CB_C2F>
                      : mode == 4 ? launch_data_s2<DATA_S2_SPLIT, CB_DF2C> : launch_data_s2<DATA_S2_SPLIT, CB_DC2F>;
    return launch(in, weight, out, B, Kc, Cf, nh, nw, 0, ws, ws_bytes, static_cast<hipStream_t>(stream));
}

size_t ipsr_conv4x4s2_bf16_wrw_workspace_bytes(int B, int Kc, int Cf, int nh, int nw)
{
    if (!cb_dims_ok(true, {B, Kc, Cf, nh, nw})) return 0;
    return wrw_ws_bytes(WRW_S2, B, Kc, Cf, nh, nw);
}

int ipsr_conv4x4s2_bf16_wrw(const void* fine, const void* coarse, float* dw, int B, int Kc, int Cf, int nh, int nw, void* ws, size_t ws_bytes, void* stream)
{
    if (int rc = cb_null("ipsr_conv4x4s2_bf16_wrw", {fine, coarse, dw, ws})) return rc;
    if (int rc = cb_bad_dims("ipsr_conv4x4s2_bf16_wrw", true, {B, Kc, Cf, nh, nw})) return rc;
    if (int rc = cb_misaligned("ipsr_conv4x4s2_bf16_wrw", "operands / workspace", {ws, fine, coarse, dw})) return rc;
    return launch_wrw<WRW_S2>(coarse, fine, dw, B, Kc, Cf, nh, nw, ws, ws_bytes, static_cast<hipStream_t>(stream));
}

size_t ipsr_conv4x4s2_bf16x3_wrw_workspace_bytes(int B, int Kc, int Cf, int nh, int nw)
{
    if (cb_bad_dims("ipsr_conv4x4s2_bf16x3_wrw_workspace_bytes", true, {B, Kc, Cf, nh, nw})) return 0;
    return wrw_ws_bytes(WRW_S2_SPLIT, B, Kc, Cf, nh, nw);
}

int ipsr_conv4x4s2_bf16x3_wrw(const float* fine, const float* coarse, float* dw, int B, int Kc, int Cf, int nh, int nw, void* ws, size_t ws_bytes, void* stream)
{
    if (int rc = cb_null("ipsr_conv4x4s2_bf16x3_wrw", {fine, coarse, dw, ws})) return rc;
    if (int rc = cb_bad_dims("ipsr_conv4x4s2_bf16x3_wrw", true, {B, Kc, Cf, nh, nw})) return rc;
    if (int rc = cb_misaligned("ipsr_conv4x4s2_bf16x3_wrw", "operands / workspace", {ws, fine, coarse, dw})) return rc;
    return launch_wrw<WRW_S2_SPLIT>(coarse, fine, dw, B, Kc, Cf, nh, nw, ws, ws_bytes, static_cast<hipStream_t>(stream));
}

size_t ipsr_conv4x4s2_bf16x3_dil_wrw_workspace_bytes(int B, int Kc, int Cf, int nh, int nw)
{
    if (cb_bad_dims("ipsr_conv4x4s2_bf16x3_dil_wrw_workspace_bytes", true, {B, Kc, Cf, nh, nw})) return 0;
    return wrw_ws_bytes(WRW_DIL_SPLIT, B, Kc, Cf, nh, nw);
}

int ipsr_conv4x4s2_bf16x3_dil_wrw(const float* fine, const float* coarse, float* dw, int B, int Kc, int Cf, int nh, int nw, void* ws, size_t ws_bytes, void* stream)
{
    if (int rc = cb_null("ipsr_conv4x4s2_bf16x3_dil_wrw", {fine, coarse, dw, ws})) return rc;
    if (int rc = cb_bad_dims("ipsr_conv4x4s2_bf16x3_dil_wrw", true, {B, Kc, Cf, nh, nw})) return rc;
    if (int rc = cb_misaligned("ipsr_conv4x4s2_bf16x3_dil_wrw", "operands / workspace", {ws, fine, coarse, dw})) return rc;
    return launch_wrw<WRW_DIL_SPLIT>(coarse, fine, dw, B, Kc, Cf, nh, nw, ws, ws_bytes, static_cast<hipStream_t>(stream));
}

size_t ipsr_conv4x4s2_bf16_dil_wrw_workspace_bytes(int B, int Kc, int Cf, int nh, int nw)
{
    if (cb_bad_dims("ipsr_conv4x4s2_bf16_dil_wrw_workspace_bytes", true, {B, Kc, Cf, nh, nw})) return 0;
    return wrw_ws_bytes(WRW_DIL, B, Kc, Cf, nh, nw);
}

int ipsr_conv4x4s2_bf16_dil_wrw(const void* fine, const void* coarse, float* dw, int B, int Kc, int Cf, int nh, int nw, void* ws, size_t ws_bytes, void* stream)
{
    if (int rc = cb_null("ipsr_conv4x4s2_bf16_dil_wrw", {fine, coarse, dw, ws})) return rc;
    if (int rc = cb_bad_dims("ipsr_conv4x4s2_bf16_dil_wrw", true, {B, Kc, Cf, nh, nw})) return rc;
    if (int rc = cb_misaligned("ipsr_conv4x4s2_bf16_dil_wrw", "operands / workspace", {ws, fine, coarse, dw})) return rc;
    return launch_wrw<WRW_DIL>(coarse, fine, dw, B, Kc, Cf, nh, nw, ws, ws_bytes, static_cast<hipStream_t>(stream));
}

size_t ipsr_conv3x3_bf16_wrw_workspace_bytes(int transposed, int B, int Cin, int H, int W, int Cout)
{
    if (!cb_dims_ok(true, {B, Cin, Cout, H, W})) return 0;
    return transposed ? wrw_ws_bytes(WRW_3X3, B, Cin, Cout, H, W) : wrw_ws_bytes(WRW_3X3, B, Cout, Cin, H, W);
}

size_t ipsr_conv3x3_bf16x3_wrw_workspace_bytes(int transposed, int B, int Cin, int H, int W, int Cout)
{
    if (cb_bad_dims("ipsr_conv3x3_bf16x3_wrw_workspace_bytes", true, {B, Cin, Cout, H, W})) return 0;
    return transposed ? wrw_ws_bytes(WRW_3X3_SPLIT, B, Cin, Cout, H, W) : wrw_ws_bytes(WRW_3X3_SPLIT, B, Cout, Cin, H, W);
}

int ipsr_conv3x3_bf16_wrw(int form, const void* x, const void* dy, float* dw, int B, int Cin, int H, int W, int Cout,
                          void* ws, size_t ws_bytes, void* stream)
{
    if (form < 0 || form > 3)
        return fail(IPSR_ERR_INVALID, "ipsr_conv3x3_bf16_wrw: form code %d (0 Conv2d, 1 ConvTranspose2d on bf16 tensors; 2, 3 the same on fp32 tensors, split-bf16 operands)", form);
    if (int rc = cb_null("ipsr_conv3x3_bf16_wrw", {x, dy, dw, ws})) return rc;
    if (int rc = cb_bad_dims("ipsr_conv3x3_bf16_wrw", true, {B, Cin, Cout, H, W})) return rc;
    if (int rc = cb_misaligned("ipsr_conv3x3_bf16_wrw", "x / dy / workspace", {ws, x, dy})) return rc;          // dW leaves as scalars: 9 floats per (k, c)
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool transposed = form & 1;
    // Conv2d: dW[co][ci][t] = sum dy[co][p] x[ci][p + t];  ConvTranspose2d: dW[ci][co][t] = sum x[ci][p] dy[co][p + t]
    const auto launch = form >= 2 ? launch_wrw<WRW_3X3_SPLIT> : launch_wrw<WRW_3X3>;
    if (transposed) return launch(x, dy, dw, B, Cin, Cout, H, W, ws, ws_bytes, st);
    return launch(dy, x, dw, B, Cout, Cin, H, W, ws, ws_bytes, st);
}

}  // extern "C"
