// Per-image pseudo-label refresh of the kidney and breast loops (include/aide_hip.h "per-image pseudo-label bank";
// trainkidney_proposed_mask1.py:373-434, trainbreast_dataset3_proposed_272cases25labeled.py:373-438): every training IMAGE is
// predicted and scored with Dice2d against a plane of the bank, all images are ranked and the worst int(update_percent * K)
// whose prediction is not empty get the prediction as their new label.  Four streaming / integer kernels: the fused
// epilogue of a forward batch (labels + exact sums), Dice / rank / write flags for up to 2^20 images, the rewrite of the
// flagged planes, and the loader's targets gathered from the bank.  Nothing here waits across workgroups, and the host reads
// nothing between prediction and update.
#include "common.h"

namespace {

constexpr int MAX_IMAGES = 1 << 20;
constexpr int CHUNK = 4096;          // pixels per workgroup of the epilogue: 256 threads x 4 groups of 4
constexpr int TILE = 4096;           // keys per LDS tile of the ranking
constexpr int OWN = 4;               // images ranked per thread

enum { SRC_LOGITS = 0, SRC_U8 = 1, SRC_I64 = 2 };

// prediction of pixel p of one image: the label rule of aide_label_map on logits, `label != 0` on ready label maps
template <int SRC>
__device__ __forceinline__ unsigned pred1(const void* src, long hw, long p) {
    if (SRC == SRC_LOGITS) {
        const float* z = static_cast<const float*>(src);
        return (unsigned)aide_label2(z[p], z[hw + p]);
    }
    if (SRC == SRC_U8) return static_cast<const unsigned char*>(src)[p] != 0;
    return static_cast<const long long*>(src)[p] != 0;
}

// ... of the four pixels p .. p + 3 (p % 4 == 0, 16-byte aligned rows), one byte each
template <int SRC>
__device__ __forceinline__ unsigned pred4(const void* src, long hw, long p) {
    if (SRC == SRC_LOGITS) {
        const float* z = static_cast<const float*>(src);
        const f32x4 a = ld4(z + p), b = ld4(z + hw + p);
        return (unsigned)aide_label2(a[0], b[0]) | (unsigned)aide_label2(a[1], b[1]) << 8 | (unsigned)aide_label2(a[2], b[2]) << 16 |
               (unsigned)aide_label2(a[3], b[3]) << 24;
    }
    if (SRC == SRC_U8) {
        const unsigned v = *reinterpret_cast<const unsigned*>(static_cast<const unsigned char*>(src) + p);
        return ((v & 0xffu) != 0) | ((v & 0xff00u) != 0) << 8 | ((v & 0xff0000u) != 0) << 16 | ((v & 0xff000000u) != 0) << 24;
    }
    const longlong2* q = reinterpret_cast<const longlong2*>(static_cast<const long long*>(src) + p);
    const longlong2 a = q[0], b = q[1];
    return (unsigned)(a.x != 0) | (unsigned)(a.y != 0) << 8 | (unsigned)(b.x != 0) << 16 | (unsigned)(b.y != 0) << 24;
}

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// workgroup b: chunk b % chunks of image b / chunks.  pred[k0 + n] = labels (uint8), sums[k0 + n] += (sum p*t, sum p, sum t)
// of the chunk with t = (score byte > 0) & gate[k0 + n]; the entry point has zeroed the rows, the totals are integers.
// VEC: hw % 16 == 0 and every row 16-byte aligned: 16-byte loads of the logits, 4 bytes of labels per thread and group.
template <int SRC, bool VEC>
__global__ __launch_bounds__(256) void image_eval_kernel(const void* __restrict__ src, long src_bs, int esize,
                                                         const unsigned char* __restrict__ score,
                                                         const unsigned char* __restrict__ gate, long hw, int chunks, long k0,
                                                         unsigned char* __restrict__ pred, long long* __restrict__ sums) {
    __shared__ int part[3];
    const long n = blockIdx.x / chunks;
    const long c0 = (long)(blockIdx.x - n * chunks) * CHUNK;
    const char* img = static_cast<const char*>(src) + n * src_bs * esize;
    const unsigned char* tgt = score + n * hw;
    unsigned char* out = pred + (k0 + n) * hw;
    const unsigned g = gate ? (gate[k0 + n] != 0) : 1u;
    if (threadIdx.x < 3) part[threadIdx.x] = 0;
    __syncthreads();
    int spt = 0, sp = 0, st = 0;
    if (VEC) {
#pragma unroll
        for (int j = 0; j < CHUNK / 1024; ++j) {
            const long p = c0 + (j * 256 + threadIdx.x) * 4;
            if (p < hw) {
                const unsigned pv = pred4<SRC>(img, hw, p);
                const unsigned tv = *reinterpret_cast<const unsigned*>(tgt + p);
                unsigned tb = ((tv & 0xffu) != 0) | ((tv & 0xff00u) != 0) << 8 | ((tv & 0xff0000u) != 0) << 16 |
                              ((tv & 0xff000000u) != 0) << 24;
                tb = g ? tb : 0u;
                *reinterpret_cast<unsigned*>(out + p) = pv;
                spt += __popc(pv & tb);
                sp += __popc(pv);
                st += __popc(tb);
            }
        }
    } else {
#pragma unroll 4
        for (int j = 0; j < CHUNK / 256; ++j) {
            const long p = c0 + j * 256 + threadIdx.x;
            if (p < hw) {
                const unsigned pv = pred1<SRC>(img, hw, p);
                const unsigned tb = (tgt[p] != 0) & g;
                out[p] = (unsigned char)pv;
                spt += pv & tb;
                sp += pv;
                st += tb;
            }
        }
    }
    // at most 1024 per wave and value: two of them share a register
    const int a = wave_sum_i(spt | sp << 16), b = wave_sum_i(st);
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&part[0], a & 0xffff);
        atomicAdd(&part[1], a >> 16);
        atomicAdd(&part[2], b);
    }
    __syncthreads();
    if (threadIdx.x < 3 && part[threadIdx.x])
        atomicAdd(reinterpret_cast<unsigned long long*>(sums + 4 * (k0 + n) + 1 + threadIdx.x), (unsigned long long)part[threadIdx.x]);
    if (threadIdx.x == 3 && c0 == 0) sums[4 * (k0 + n)] = hw;
}

// Dice2d (:131-141): 0.0 when sum p + sum t == 0, else the fp64 quotient rounded once to float32
__global__ __launch_bounds__(256) void image_dice_kernel(const long long* __restrict__ sums, int K, float* __restrict__ dice) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= K) return;
    const long long uni = sums[4 * k + 2] + sums[4 * k + 3];
    dice[k] = uni == 0 ? 0.0f : (float)((double)(2 * sums[4 * k + 1]) / (double)uni);
}

// a float as an unsigned whose order is the ranking's: ascending, -0 == +0, every NaN greatest (and equal to every other NaN)
__device__ __forceinline__ unsigned sort_key(float v) {
    if (v != v) return 0xffffffffu;
    const unsigned u = __float_as_uint(v + 0.0f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// rank[k] = |{j : key[j] < key[k], or key[j] == key[k] and j < k}|: a counting rank.  A workgroup owns the 1024 images
// [1024 b, 1024 b + 1024), four per thread, and walks all K keys through LDS tiles; a tile that lies wholly below / above the
// owned range needs one comparison per pair (<= / <), the one or two tiles that meet it the full rule.  The tail of the last
// tile is padded with the greatest key at indices >= K, which no image counts (an index above its own, never a smaller key).
__global__ __launch_bounds__(256) void image_rank_kernel(const float* __restrict__ dice, const long long* __restrict__ sums,
                                                         const unsigned char* __restrict__ labelled, int K, int n_select,
                                                         int* __restrict__ rank, unsigned char* __restrict__ written) {
    __shared__ __attribute__((aligned(16))) unsigned tile[TILE];
    const int base = blockIdx.x * (256 * OWN);
    unsigned mine[OWN];
    int idx[OWN], cnt[OWN];
#pragma unroll
    for (int i = 0; i < OWN; ++i) {
        idx[i] = base + i * 256 + threadIdx.x;
        mine[i] = idx[i] < K ? sort_key(dice[idx[i]]) : 0u;
        cnt[i] = 0;
    }
    for (int t0 = 0; t0 < K; t0 += TILE) {
        __syncthreads();
        for (int j = threadIdx.x; j < TILE; j += 256) tile[j] = t0 + j < K ? sort_key(dice[t0 + j]) : 0xffffffffu;
        __syncthreads();
        const int jn = min(TILE, (K - t0 + 3) & ~3);
        if (t0 + TILE <= base) {
            for (int j = 0; j < jn; j += 4) {
                const uint4 q = *reinterpret_cast<const uint4*>(&tile[j]);
#pragma unroll
                for (int i = 0; i < OWN; ++i) cnt[i] += (q.x <= mine[i]) + (q.y <= mine[i]) + (q.z <= mine[i]) + (q.w <= mine[i]);
            }
        } else if (t0 >= base + 256 * OWN) {
            for (int j = 0; j < jn; j += 4) {
                const uint4 q = *reinterpret_cast<const uint4*>(&tile[j]);
#pragma unroll
                for (int i = 0; i < OWN; ++i) cnt[i] += (q.x < mine[i]) + (q.y < mine[i]) + (q.z < mine[i]) + (q.w < mine[i]);
            }
        } else {
            for (int j = 0; j < jn; ++j) {
                const unsigned q = tile[j];
#pragma unroll
                for (int i = 0; i < OWN; ++i) cnt[i] += (q < mine[i]) | ((q == mine[i]) & (t0 + j < idx[i]));
            }
        }
    }
#pragma unroll
    for (int i = 0; i < OWN; ++i) {
        const int k = idx[i];
        if (k < K) {
            rank[k] = cnt[i];
            written[k] = (cnt[i] < n_select && sums[4 * k + 2] > 0 && !(labelled && labelled[k])) ? 1 : 0;
        }
    }
}

// plane[k] = pred[k] * scale for the written images; workgroup b: chunk b % chunks (span bytes) of image b / chunks
template <bool VEC>
__global__ __launch_bounds__(256) void image_update_kernel(const unsigned char* __restrict__ pred,
                                                           const unsigned char* __restrict__ written, long hw, int chunks,
                                                           long span, int scale, unsigned char* __restrict__ plane) {
    const long k = blockIdx.x / chunks;
    if (!written[k]) return;
    const long c0 = (long)(blockIdx.x - k * chunks) * span;
    const long c1 = min(c0 + span, hw);
    const unsigned char* src = pred + k * hw;
    unsigned char* dst = plane + k * hw;
    if (VEC) {
        for (long o = c0 + threadIdx.x * 16; o < c1; o += 256 * 16) {
            const uint4 a = *reinterpret_cast<const uint4*>(src + o);
            unsigned w[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                unsigned r = 0;
#pragma unroll
                for (int sh = 0; sh < 32; sh += 8) r |= ((((w[j] >> sh) & 255u) * (unsigned)scale) & 255u) << sh;
                w[j] = r;
            }
            *reinterpret_cast<uint4*>(dst + o) = make_uint4(w[0], w[1], w[2], w[3]);
        }
    } else {
        for (long o = c0 + threadIdx.x; o < c1; o += 256) dst[o] = (unsigned char)(src[o] * (unsigned)scale);
    }
}

// out[n][p] = (plane[idx[n]][p] > 0) & gate[idx[n]]; an index outside [0, K) gives zeros
__global__ __launch_bounds__(256) void image_targets_kernel(const unsigned char* __restrict__ plane, long K, long hw,
                                                            const long long* __restrict__ idx,
                                                            const unsigned char* __restrict__ gate, int chunks,
                                                            long long* __restrict__ out) {
    const long n = blockIdx.x / chunks;
    const long c0 = (long)(blockIdx.x - n * chunks) * CHUNK;
    const long long s = idx[n];
    const bool live = s >= 0 && s < K && (!gate || gate[s]);
#pragma unroll 4
    for (int j = 0; j < CHUNK / 256; ++j) {
        const long p = c0 + j * 256 + threadIdx.x;
        if (p < hw) out[n * hw + p] = (live && plane[s * hw + p] != 0) ? 1 : 0;
    }
}

// K images of H x W: every index that the kernels form stays below 2^31 blocks and 2^62 bytes
bool image_ok(int64_t K, int64_t H, int64_t W) {
    if (K < 0 || K > MAX_IMAGES || H < 0 || W < 0) return false;
    if (H == 0 || W == 0) return true;
    return H <= INT32_MAX && W <= INT32_MAX && H * W <= INT32_MAX;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <int SRC>
int launch_eval(const void* src, int64_t src_bs, int esize, const unsigned char* score, const unsigned char* gate, int64_t N,
                int64_t H, int64_t W, int64_t k0, int64_t K, unsigned char* pred, long long* sums, hipStream_t stream) {
    if (!image_ok(K, H, W) || N < 0 || k0 < 0 || k0 + N > K || src_bs < 0) return AIDE_ERR_ARG;
    const long hw = (long)(H * W);
    if (N == 0 || hw == 0) return 0;
    if (!src || !score || !pred || !sums || src_bs < (SRC == SRC_LOGITS ? 2 : 1) * hw) return AIDE_ERR_ARG;
    const long chunks = (hw + CHUNK - 1) / CHUNK;
    if (N * chunks > INT32_MAX) return AIDE_ERR_ARG;
    const hipError_t e = hipMemsetAsync(sums + 4 * k0, 0, (size_t)N * 4 * sizeof(long long), stream);
    if (e != hipSuccess) return (int)e;
    const bool vec = hw % 16 == 0 && aligned16(src) && (src_bs * esize) % 16 == 0 && aligned16(score) && aligned16(pred + k0 * hw);
    const dim3 grid((unsigned)(N * chunks)), block(256);
    const double bytes = (double)N * hw * ((SRC == SRC_LOGITS ? 2.0 : 1.0) * esize + 2.0);
    const auto kernel = vec ? image_eval_kernel<SRC, true> : image_eval_kernel<SRC, false>;
    AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, bytes, kernel, grid, block, 0, stream, src, (long)src_bs, esize, score, gate, hw, (int)chunks,
                      (long)k0, pred, sums);
    return aide_launch_status();
}

}  // namespace

extern "C" {

int aide_image_eval_logits(const float* logits, int64_t l_bs, const unsigned char* score_rows, const unsigned char* gate,
                           int64_t N, int64_t H, int64_t W, int64_t k0, int64_t K, unsigned char* pred, long long* sums,
                           hipStream_t stream) {
    return launch_eval<SRC_LOGITS>(logits, l_bs, 4, score_rows, gate, N, H, W, k0, K, pred, sums, stream);
}

int aide_image_eval_labels(const void* labels, int is_u8, const unsigned char* score_rows, const unsigned char* gate, int64_t N,
                           int64_t H, int64_t W, int64_t k0, int64_t K, unsigned char* pred, long long* sums,
                           hipStream_t stream) {
    if (H < 0 || W < 0) return AIDE_ERR_ARG;
    if (is_u8) return launch_eval<SRC_U8>(labels, H * W, 1, score_rows, gate, N, H, W, k0, K, pred, sums, stream);
    return launch_eval<SRC_I64>(labels, H * W, 8, score_rows, gate, N, H, W, k0, K, pred, sums, stream);
}

int aide_image_refresh_select(const long long* sums, const unsigned char* labelled, int64_t K, int64_t n_select, float* dice,
                              int* rank, unsigned char* written, hipStream_t stream) {
    if (K < 0 || K > MAX_IMAGES || n_select < 0) return AIDE_ERR_ARG;
    if (K == 0) return 0;
    if (!sums || !dice || !rank || !written) return AIDE_ERR_ARG;
    AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 0.0, image_dice_kernel, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, stream, sums, (int)K,
                      dice);
    AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 0.0, image_rank_kernel, dim3((unsigned)((K + 256 * OWN - 1) / (256 * OWN))), dim3(256), 0,
                      stream, dice, sums, labelled, (int)K, (int)min(n_select, (int64_t)MAX_IMAGES), rank, written);
    return aide_launch_status();
}

int aide_image_bank_update(const unsigned char* pred, const unsigned char* written, int64_t K, int64_t H, int64_t W, int scale,
                           unsigned char* plane, hipStream_t stream) {
    if (!image_ok(K, H, W) || scale < 0 || scale > 255) return AIDE_ERR_ARG;
    const long hw = (long)(H * W);
    if (K == 0 || hw == 0) return 0;
    if (!pred || !written || !plane) return AIDE_ERR_ARG;
    const bool vec = hw % 16 == 0 && aligned16(pred) && aligned16(plane);
    // 4096 bytes per workgroup, more where K * chunks would pass 2^30 workgroups
    long span = 4096, chunks = (hw + span - 1) / span;
    while (K * chunks > (1L << 30)) {
        span *= 2;
        chunks = (hw + span - 1) / span;
    }
    const dim3 grid((unsigned)(K * chunks)), block(256);
    const double bytes = 2.0 * (double)K * (double)hw;
    if (vec)
        AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, bytes, image_update_kernel<true>, grid, block, 0, stream, pred, written, hw, (int)chunks,
                          span, scale, plane);
    else
        AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, bytes, image_update_kernel<false>, grid, block, 0, stream, pred, written, hw, (int)chunks,
                          span, scale, plane);
    return aide_launch_status();
}

int aide_image_bank_targets(const unsigned char* plane, int64_t K, int64_t H, int64_t W, const long long* image_idx, int64_t N,
                            const unsigned char* gate, long long* out, hipStream_t stream) {
    if (!image_ok(K, H, W) || N < 0) return AIDE_ERR_ARG;
    const long hw = (long)(H * W);
    if (N == 0 || hw == 0) return 0;
    if (!image_idx || !out || (K > 0 && !plane)) return AIDE_ERR_ARG;
    const long chunks = (hw + CHUNK - 1) / CHUNK;
    if (N * chunks > INT32_MAX) return AIDE_ERR_ARG;
    AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, (double)N * hw * 9.0, image_targets_kernel, dim3((unsigned)(N * chunks)), dim3(256), 0, stream,
                      plane, (long)K, hw, image_idx, gate, (int)chunks, out);
    return aide_launch_status();
}

}  // extern "C"
