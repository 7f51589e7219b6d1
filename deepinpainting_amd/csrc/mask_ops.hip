// mask_ops.hip — K1 feature-mask pyramid and K2 index prep, one mask per call or a batch of masks in one launch.
//
// Reference: util.cal_feat_mask (util/util.py:68-84) and util.cal_mask_given_mask_thred
// (util/util.py:88-161).  Both depend on the mask only, so the host caches their result per mask;
// they are byte/integer kernels far below any roofline (a 256x256 mask is 64 KB).
#include "ipsr_common.h"

namespace ipsr {

__host__ __device__ static inline int half_dim(int n) { return (n + 2 - 4) / 2 + 1; }

// One level of the pyramid: 4x4 box sum, stride 2, zero padding 1.  The reference does this in fp32
// with weights 1/16; the sums are count/16^level and exact, so integer counting gives the same bits.
// LAST: compare count * 16^-layers with the threshold and emit bytes.
// BINARY: the input is the 0/1 mask itself (any non-zero byte counts as 1), else a level of counts.
template <bool BINARY, typename TIn>
__device__ __forceinline__ uint32_t box4s2_at(const TIn* in, int h, int w, int y, int x)
{
    uint32_t s = 0;
#pragma unroll
    for (int dy = 0; dy < 4; ++dy) {
        const int yy = 2 * y - 1 + dy;
        if (yy < 0 || yy >= h) continue;
#pragma unroll
        for (int dx = 0; dx < 4; ++dx) {
            const int xx = 2 * x - 1 + dx;
            if (xx < 0 || xx >= w) continue;
            const TIn v = in[(size_t)yy * w + xx];
            s += BINARY ? (v ? 1u : 0u) : (uint32_t)v;
        }
    }
    return s;
}

template <typename TIn, bool LAST>
__global__ void __launch_bounds__(256) boxsum4s2_kernel(const TIn* __restrict__ in, int h, int w, int oh, int ow,
                                                        uint32_t* __restrict__ out_cnt, uint8_t* __restrict__ out_u8,
                                                        float scale, float threshold)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= oh * ow) return;
    const int y = idx / ow, x = idx - y * ow;
    const uint32_t s = box4s2_at<sizeof(TIn) == 1>(in, h, w, y, x);
    if (LAST) out_u8[idx] = ((float)s * scale > threshold) ? 1 : 0;
    else out_cnt[idx] = s;
}

int launch_feat_mask(const uint8_t* mask, int H, int W, int layers, float threshold, uint8_t* feat,
                     void* ws, size_t ws_bytes, hipStream_t st)
{
    const int h1 = half_dim(H), w1 = half_dim(W);
    const size_t lvl = align_up((size_t)h1 * w1 * sizeof(uint32_t), 256);
    if (layers > 1 && ws_bytes < 2 * lvl) return fail(IPSR_ERR_WORKSPACE, "ipsr_feat_mask: workspace %zu < %zu", ws_bytes, 2 * lvl);
    uint32_t* buf[2] = {reinterpret_cast<uint32_t*>(ws), reinterpret_cast<uint32_t*>(static_cast<char*>(ws) + lvl)};
    float scale = 1.0f;
    for (int l = 0; l < layers; ++l) scale *= (1.0f / 16.0f);
    int h = H, w = W;
    const void* cur = mask;
    for (int l = 0; l < layers; ++l) {
        const int oh = half_dim(h), ow = half_dim(w);
        if (oh < 1 || ow < 1) return fail(IPSR_ERR_INVALID, "ipsr_feat_mask: mask %dx%d too small for %d layers", H, W, layers);
        const bool last = (l == layers - 1);
        const int grid = cdiv(oh * ow, 256);
        uint32_t* dst = buf[l & 1];
        if (l == 0) {
            if (last) boxsum4s2_kernel<uint8_t, true><<<grid, 256, 0, st>>>((const uint8_t*)cur, h, w, oh, ow, nullptr, feat, scale, threshold);
            else boxsum4s2_kernel<uint8_t, false><<<grid, 256, 0, st>>>((const uint8_t*)cur, h, w, oh, ow, dst, nullptr, scale, threshold);
        } else {
            if (last) boxsum4s2_kernel<uint32_t, true><<<grid, 256, 0, st>>>((const uint32_t*)cur, h, w, oh, ow, nullptr, feat, scale, threshold);
            else boxsum4s2_kernel<uint32_t, false><<<grid, 256, 0, st>>>((const uint32_t*)cur, h, w, oh, ow, dst, nullptr, scale, threshold);
        }
        if (int rc = check_launch("boxsum4s2_kernel")) return rc;
        cur = dst;
        h = oh; w = ow;
    }
    return IPSR_OK;
}

// K2: raster scan -> flag[N], ordered compaction of the flagged positions.  One workgroup walks the N
// positions in chunks of 1024; order is kept by a ballot/popcount prefix inside each wave plus an LDS
// prefix over the 16 waves.
// The body is a device function: index_prep_kernel runs it on one feature mask, mask_index_kernel on the row its workgroup owns.
__device__ __forceinline__ void index_prep_row(const uint8_t* feat, int w, int patch, int stride, int mask_thred, int nW, int N,
                                               int32_t* __restrict__ flag, int32_t* __restrict__ mpi, int32_t* __restrict__ count)
{
    __shared__ int wave_tot[16];
    __shared__ int base_s;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid == 0) base_s = 0;
    __syncthreads();
    for (int i0 = 0; i0 < N; i0 += 1024) {
        const int i = i0 + tid;
        int f = 0;
        if (i < N) {
            const int py = i / nW, px = i - py * nW;
            int s = 0;
            for (int dy = 0; dy < patch; ++dy)
                for (int dx = 0; dx < patch; ++dx) s += feat[(size_t)(py * stride + dy) * w + px * stride + dx];
            f = (s >= mask_thred) ? 1 : 0;
            flag[i] = f;
        }
        const unsigned long long bal = __ballot(f);
        const int before = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wave_tot[wv] = __popcll(bal);
        __syncthreads();
        int off = base_s;
        for (int j = 0; j < wv; ++j) off += wave_tot[j];
        if (f) mpi[off + before] = i;
        __syncthreads();
        if (tid == 0) {
            int t = 0;
            for (int j = 0; j < 16; ++j) t += wave_tot[j];
            base_s += t;
        }
        __syncthreads();
    }
    const int M = base_s;
    for (int i = M + tid; i < N; i += 1024) mpi[i] = -1;
    if (tid == 0) *count = M;
}

__global__ void __launch_bounds__(1024) index_prep_kernel(const uint8_t* __restrict__ feat, int h, int w, int patch,
                                                          int stride, int mask_thred, int nW, int N,
                                                          int32_t* __restrict__ flag, int32_t* __restrict__ mpi,
                                                          int32_t* __restrict__ count)
{
    (void)h;
    index_prep_row(feat, w, patch, stride, mask_thred, nW, N, flag, mpi, count);
}

int launch_index_prep(const uint8_t* feat, int h, int w, int patch, int stride, int mask_thred,
                      int32_t* flag, int32_t* mask_point_idx, int32_t* count, hipStream_t st)
{
    const int nH = (h - patch) / stride + 1, nW = (w - patch) / stride + 1;
    index_prep_kernel<<<1, 1024, 0, st>>>(feat, h, w, patch, stride, mask_thred, nW, nH * nW, flag, mask_point_idx, count);
    return check_launch("index_prep_kernel");
}

// ---- K1 + K2 for a batch of masks in ONE launch ----------------------------------------------------------------------------------
// A workgroup owns mask row r from the first level to the -1 fill, so workgroup barriers are all the ordering there is.  The levels
// between the mask and the feature mask ping-pong between two buffers, in LDS where both fit and in the workgroup's slice of the
// workspace otherwise (mask_index_plan decides; the code is the same).  Buffer A holds level 1 as BYTES (a 4x4 box of 0/1 is <= 16)
// and then levels 3 and 5 as counts, buffer B levels 2 and 4: a 512x512 mask needs 64 + 64 KB, a 256x256 mask 16 + 16 KB.
constexpr int MI_THREADS = 1024;
constexpr size_t MI_LDS_MAX = 159 * 1024;       // of the CU's 160 KB: the index part keeps 17 words of its own

MaskIndexPlan mask_index_plan(int R, int H, int W, int layers)
{
    MaskIndexPlan p = {};
    int h = H, w = W;
    size_t a = 0, b = 0;
    for (int L = 1; L <= layers; ++L) {
        if (h < 2 || w < 2) return p;                                   // ok stays false: a level of one row or column has no half
        h = half_dim(h); w = half_dim(w);
        if (L == layers) break;                                          // the last level goes straight to `feat`
        const size_t bytes = (size_t)h * w * (L == 1 ? 1 : sizeof(uint32_t));
        if (L & 1) a = bytes > a ? bytes : a;
        else b = bytes > b ? bytes : b;
    }
    p.ok = true;
    p.h = h; p.w = w;
    p.off_b = align_up(a, 256);
    p.slice = p.off_b + align_up(b, 256);
    p.in_lds = p.slice <= MI_LDS_MAX;
    p.ws_bytes = 256 + (p.in_lds ? 0 : (size_t)R * p.slice);
    return p;
}

template <bool BINARY, typename TIn, typename TOut>
__device__ __forceinline__ void box_level(const TIn* in, int h, int w, int oh, int ow, TOut* out)
{
    for (int idx = threadIdx.x; idx < oh * ow; idx += MI_THREADS) {
        const int y = idx / ow, x = idx - y * ow;
        out[idx] = (TOut)box4s2_at<BINARY>(in, h, w, y, x);
    }
    __syncthreads();
}

// every byte of a word -> 1 where it is not zero (bit 0 of a byte collects the byte's 8 bits; what crosses in from the next byte
// lands in bits 4..7 and is masked away)
__device__ __forceinline__ uint32_t nonzero_bytes(uint32_t v)
{
    v |= v >> 4; v |= v >> 2; v |= v >> 1;
    return v & 0x01010101u;
}

// The same level from a BYTE input whose rows are whole 16-byte vectors (w % 16 == 0, `in` 16-byte aligned): a thread makes 8 adjacent
// outputs of a row from 4 vector loads and the two bytes beside them, instead of 128 byte loads.  The four rows are added as packed
// bytes first (<= 4 * 16: no carry between bytes), then every output is four neighbours of those 18 column sums.  Levels 1 and 2 of
// the 256x256 and 512x512 masks take this path; they hold 15/16 of the pyramid's loads.
template <bool BINARY, typename TOut>
__device__ __forceinline__ void box_level_bytes16(const uint8_t* in, int h, int w, int oh, int ow, TOut* out)
{
    const int segs = ow >> 3;
    for (int item = threadIdx.x; item < oh * segs; item += MI_THREADS) {
        const int y = item / segs, k = item - y * segs;
        uint32_t v[4] = {0u, 0u, 0u, 0u}, c[18];
        c[0] = c[17] = 0u;
#pragma unroll
        for (int dy = 0; dy < 4; ++dy) {
            const int yy = 2 * y - 1 + dy;
            if (yy < 0 || yy >= h) continue;
            const uint8_t* row = in + (size_t)yy * w + 16 * k;
            uint4 q = *reinterpret_cast<const uint4*>(row);
            uint32_t left = k > 0 ? row[-1] : 0u, right = 16 * k + 16 < w ? row[16] : 0u;
            if (BINARY) {
                q.x = nonzero_bytes(q.x); q.y = nonzero_bytes(q.y); q.z = nonzero_bytes(q.z); q.w = nonzero_bytes(q.w);
                left = left ? 1u : 0u; right = right ? 1u : 0u;
            }
            v[0] += q.x; v[1] += q.y; v[2] += q.z; v[3] += q.w;
            c[0] += left; c[17] += right;
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) c[1 + i] = (v[i >> 2] >> (8 * (i & 3))) & 0xffu;        // c[1 + m]: column 16k + m
        uint32_t o[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (c[2 * j] + c[2 * j + 1]) + (c[2 * j + 2] + c[2 * j + 3]);      // columns 2x-1 .. 2x+2, x = 8k + j
        TOut* dst = out + (size_t)y * ow + 8 * k;
        if (sizeof(TOut) == 1) {
            *reinterpret_cast<uint2*>(dst) = make_uint2(o[0] | (o[1] << 8) | (o[2] << 16) | (o[3] << 24), o[4] | (o[5] << 8) | (o[6] << 16) | (o[7] << 24));
        } else {
            reinterpret_cast<uint4*>(dst)[0] = make_uint4(o[0], o[1], o[2], o[3]);
            reinterpret_cast<uint4*>(dst)[1] = make_uint4(o[4], o[5], o[6], o[7]);
        }
    }
    __syncthreads();
}

template <bool BINARY, typename TIn>
__device__ __forceinline__ void box_last(const TIn* in, int h, int w, int oh, int ow, float scale, float threshold, uint8_t* feat)
{
    for (int idx = threadIdx.x; idx < oh * ow; idx += MI_THREADS) {
        const int y = idx / ow, x = idx - y * ow;
        feat[idx] = ((float)box4s2_at<BINARY>(in, h, w, y, x) * scale > threshold) ? 1 : 0;      // the compare of boxsum4s2_kernel
    }
    __syncthreads();                            // the index part reads what other threads of this workgroup stored
}

template <bool IN_LDS>
__global__ void __launch_bounds__(MI_THREADS) mask_index_kernel(const uint8_t* masks, int H, int W, int layers, float scale, float threshold,
                                                                int hf, int wf, int patch, int stride, int mask_thred, int nW, int N,
                                                                uint8_t* feat, int32_t* __restrict__ flag, int32_t* __restrict__ mpi,
                                                                int32_t* __restrict__ counts, char* ws, size_t slice, size_t off_b, int vec)
{
    extern __shared__ __align__(16) char mi_lds[];
    const size_t r = blockIdx.x;
    const uint8_t* mask = masks + r * (size_t)H * W;
    const uint8_t* fsrc = mask;                 // layers == 0: the input is the feature mask
    if (layers > 0) {
        uint8_t* frow = feat + r * (size_t)hf * wf;
        fsrc = frow;
        char* buf = IN_LDS ? mi_lds : ws + r * slice;
        uint8_t* l1 = reinterpret_cast<uint8_t*>(buf);
        int h = half_dim(H), w = half_dim(W);
        if (layers == 1) {
            box_last<true>(mask, H, W, h, w, scale, threshold, frow);
        } else {
            if (vec & 1) box_level_bytes16<true>(mask, H, W, h, w, l1);
            else box_level<true>(mask, H, W, h, w, l1);
            int oh = half_dim(h), ow = half_dim(w);
            if (layers == 2) {
                box_last<false>(l1, h, w, oh, ow, scale, threshold, frow);
            } else {
                uint32_t* cur = reinterpret_cast<uint32_t*>(buf + off_b);
                uint32_t* nxt = reinterpret_cast<uint32_t*>(buf);
                if (vec & 2) box_level_bytes16<false>(l1, h, w, oh, ow, cur);
                else box_level<false>(l1, h, w, oh, ow, cur);
                for (int L = 3; L < layers; ++L) {
                    h = oh; w = ow; oh = half_dim(h); ow = half_dim(w);
                    box_level<false>(cur, h, w, oh, ow, nxt);
                    uint32_t* t = cur; cur = nxt; nxt = t;
                }
                h = oh; w = ow; oh = half_dim(h); ow = half_dim(w);
                box_last<false>(cur, h, w, oh, ow, scale, threshold, frow);
            }
        }
    }
    index_prep_row(fsrc, wf, patch, stride, mask_thred, nW, N, flag + r * (size_t)N, mpi + r * (size_t)N, counts + r);
}

int launch_mask_index(const uint8_t* masks, int R, int H, int W, int layers, float threshold, int patch, int stride, int mask_thred,
                      uint8_t* feat, int32_t* flag, int32_t* mask_point_idx, int32_t* counts, void* ws, size_t ws_bytes, hipStream_t st)
{
    const MaskIndexPlan p = mask_index_plan(R, H, W, layers);
    if (!p.ok) return fail(IPSR_ERR_INVALID, "ipsr_mask_index: mask %dx%d too small for %d layers", H, W, layers);
    if (p.h < patch || p.w < patch) return fail(IPSR_ERR_INVALID, "ipsr_mask_index: patch %d does not fit the %dx%d feature mask", patch, p.h, p.w);
    if (!ws || ws_bytes < p.ws_bytes) return fail(IPSR_ERR_WORKSPACE, "ipsr_mask_index: workspace %zu < %zu", ws ? ws_bytes : (size_t)0, p.ws_bytes);
    float scale = 1.0f;
    for (int l = 0; l < layers; ++l) scale *= (1.0f / 16.0f);
    const int nH = (p.h - patch) / stride + 1, nW = (p.w - patch) / stride + 1;
    char* slices = static_cast<char*>(ws) + 256;
    // levels 1 and 2 by 16-byte loads where their input rows are whole aligned vectors (bit 0: the mask, bit 1: level 1)
    const bool aligned_in = (reinterpret_cast<uintptr_t>(masks) & 15u) == 0, aligned_ws = p.in_lds || (reinterpret_cast<uintptr_t>(ws) & 15u) == 0;
    const int vec = (W % 16 == 0 && aligned_in && aligned_ws ? 1 : 0) | (half_dim(W) % 16 == 0 && aligned_ws ? 2 : 0);
    if (p.in_lds) {
        if (p.slice > 48 * 1024)
            if (int rc = raise_dynamic_lds(reinterpret_cast<const void*>(&mask_index_kernel<true>), "mask_index_kernel", p.slice)) return rc;
        mask_index_kernel<true><<<R, MI_THREADS, p.slice, st>>>(masks, H, W, layers, scale, threshold, p.h, p.w, patch, stride, mask_thred, nW, nH * nW,
                                                                feat, flag, mask_point_idx, counts, slices, p.slice, p.off_b, vec);
    } else {
        mask_index_kernel<false><<<R, MI_THREADS, 0, st>>>(masks, H, W, layers, scale, threshold, p.h, p.w, patch, stride, mask_thred, nW, nH * nW,
                                                           feat, flag, mask_point_idx, counts, slices, p.slice, p.off_b, vec);
    }
    return check_launch("mask_index_kernel");
}

}  // namespace ipsr
