// Multi-class segmentation metrics on the device (include/aide_hip.h "multi-class metrics"): the per-image, per-class counts
// (sum i*t, sum i, sum t) behind MulticlassDice_fn / MulticlassIoU_fn / MulticlassTP_TN_FP_FN / MulticlassAccuracy_fn of
// utils/metrics2d.py:86-196, the same counts for two label volumes of a case, and the running sums of an epoch.
//
// Prediction = torch.argmax of the RAW logits (metrics2d.py:89): equal maxima go to the lowest class, a NaN counts as the
// greatest value and the first NaN wins.  (aide_label_map takes the soft-max first, whose rounding creates other ties.)
//
// Counting: every lane holds the class of its pixel in a register; per class a 64-lane ballot of (prediction == c) and one of
// (target has c) are popcounted -- their AND is the intersection -- into wave-uniform counters.  No per-thread counters and no
// shuffles.  The four waves of a block meet in LDS, and one 64-bit integer atomic per non-zero (class, count) and block adds
// to the output, which a memset node zeroed.  Integer sums: the result has the same bits whatever the order of the blocks.
#include "volume3d.h"

namespace {

constexpr int MAXC = 8;
enum { T_ONEHOT_F32 = 0, T_ONEHOT_I64 = 1, T_ONEHOT_U8 = 2, T_INDEX_I64 = 3 };

// class c beats the running best: greater, or the first NaN (nothing beats a NaN)
__device__ __forceinline__ bool beats(float z, float best) { return !(z <= best) && best == best; }

template <typename T, int V> struct Vec { T v[V]; };

// V consecutive elements; V == 4 only where the address is aligned to the natural 16 / 32 / 4 bytes (host-checked)
template <int V> __device__ __forceinline__ Vec<float, V> ldv(const float* p) {
    Vec<float, V> r;
    if (V == 4) { const f32x4 a = ld4(p); r.v[0] = a[0]; r.v[1] = a[1]; r.v[2] = a[2]; r.v[3] = a[3]; }
    else r.v[0] = *p;
    return r;
}
template <int V> __device__ __forceinline__ Vec<long long, V> ldv(const long long* p) {
    Vec<long long, V> r;
    if (V == 4) {
        const longlong2 a = *reinterpret_cast<const longlong2*>(p), b = *reinterpret_cast<const longlong2*>(p + 2);
        r.v[0] = a.x; r.v[1] = a.y; r.v[2] = b.x; r.v[3] = b.y;
    } else r.v[0] = *p;
    return r;
}
template <int V> __device__ __forceinline__ Vec<unsigned char, V> ldv(const unsigned char* p) {
    Vec<unsigned char, V> r;
    if (V == 4) {
        const unsigned a = *reinterpret_cast<const unsigned*>(p);
        r.v[0] = a & 255u; r.v[1] = (a >> 8) & 255u; r.v[2] = (a >> 16) & 255u; r.v[3] = a >> 24;
    } else r.v[0] = *p;
    return r;
}

// the block's wave counters -> counts[(n * C + c) * 3 + k]; acc[c][k] is wave-uniform
template <int C>
__device__ __forceinline__ void block_add(const unsigned (&acc)[C][3], unsigned (*sm)[C * 3], long long* __restrict__ out) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < C; ++c)
#pragma unroll
            for (int k = 0; k < 3; ++k) sm[wid][c * 3 + k] = acc[c][k];
    }
    __syncthreads();
    if (threadIdx.x < C * 3) {
        const unsigned long long s = (unsigned long long)sm[0][threadIdx.x] + sm[1][threadIdx.x] + sm[2][threadIdx.x] +
                                     sm[3][threadIdx.x];
        if (s) atomicAdd(reinterpret_cast<unsigned long long*>(out) + threadIdx.x, s);
    }
}

// grid (chunks of the plane, N): a block walks its image in steps of 256 * V pixels; every logit and target is read once
template <int C, int KIND, int V, typename TT>
__global__ __launch_bounds__(256) void counts_logits_kernel(const float* __restrict__ logits, long l_bs,
                                                            const TT* __restrict__ target, long t_bs, int HW,
                                                            long long* __restrict__ counts) {
    __shared__ unsigned sm[4][C * 3];
    const int n = blockIdx.y;
    const float* lg = logits + (long)n * l_bs;
    const TT* tg = target + (long)n * t_bs;
    unsigned acc[C][3];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c][0] = acc[c][1] = acc[c][2] = 0u;
    const long step = (long)gridDim.x * 256 * V;
    // the trip count is the block's: every wave reaches every ballot with all lanes, pixels past the plane are masked
    for (long base = (long)blockIdx.x * 256 * V; base < HW; base += step) {
        const long p = base + (long)threadIdx.x * V;
        const bool in = p < HW;                  // V == 4: HW % 4 == 0, so p < HW covers p + 3
        int pred[V];
        bool tc[C][V];
        if (in) {
            Vec<float, V> best = ldv<V>(lg + p);
#pragma unroll
            for (int j = 0; j < V; ++j) pred[j] = 0;
#pragma unroll
            for (int c = 1; c < C; ++c) {
                const Vec<float, V> z = ldv<V>(lg + (long)c * HW + p);
#pragma unroll
                for (int j = 0; j < V; ++j)
                    if (beats(z.v[j], best.v[j])) { best.v[j] = z.v[j]; pred[j] = c; }
            }
            if (KIND == T_INDEX_I64) {
                const Vec<TT, V> t = ldv<V>(tg + p);
#pragma unroll
                for (int c = 0; c < C; ++c)
#pragma unroll
                    for (int j = 0; j < V; ++j) tc[c][j] = t.v[j] == (TT)c;
            } else {
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const Vec<TT, V> t = ldv<V>(tg + (long)c * HW + p);
#pragma unroll
                    for (int j = 0; j < V; ++j) tc[c][j] = t.v[j] != (TT)0;
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < V; ++j) {
                pred[j] = -1;
#pragma unroll
                for (int c = 0; c < C; ++c) tc[c][j] = false;
            }
        }
#pragma unroll
        for (int c = 0; c < C; ++c)
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const unsigned long long bi = __ballot(pred[j] == c), bt = __ballot(tc[c][j]);
                acc[c][0] += (unsigned)__popcll(bi & bt);
                acc[c][1] += (unsigned)__popcll(bi);
                acc[c][2] += (unsigned)__popcll(bt);
            }
    }
    block_add<C>(acc, sm, counts + (long)n * C * 3);
}

// two label volumes with element strides; i_c = (p == c), t_c = (t == c); a value outside [0, C) belongs to no class
template <typename TP, typename TT>
__global__ __launch_bounds__(256) void counts_labels_kernel(Operand P, Operand T, int d1, int d2, int n, int C,
                                                            long long* __restrict__ counts) {
    __shared__ unsigned sm[4][MAXC * 3];
    unsigned acc[MAXC][3];
#pragma unroll
    for (int c = 0; c < MAXC; ++c) acc[c][0] = acc[c][1] = acc[c][2] = 0u;
    for (long base = (long)blockIdx.x * 256; base < n; base += (long)gridDim.x * 256) {
        const long u = base + threadIdx.x;
        long long a = -1, b = -1;
        if (u < n) {
            int i0, i1, i2;
            raster_decode((int)u, d1, d2, i0, i1, i2);
            a = P.at<TP>(P.off(i0, i1, i2));
            b = T.at<TT>(T.off(i0, i1, i2));
        }
#pragma unroll
        for (int c = 0; c < MAXC; ++c) {
            if (c < C) {                         // (uniform)
                const unsigned long long bi = __ballot(a == c), bt = __ballot(b == c);
                acc[c][0] += (unsigned)__popcll(bi & bt);
                acc[c][1] += (unsigned)__popcll(bi);
                acc[c][2] += (unsigned)__popcll(bt);
            }
        }
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
#pragma unroll
            for (int k = 0; k < 3; ++k) sm[wid][c * 3 + k] = acc[c][k];
    }
    __syncthreads();
    if ((int)threadIdx.x < C * 3) {
        const unsigned long long s = (unsigned long long)sm[0][threadIdx.x] + sm[1][threadIdx.x] + sm[2][threadIdx.x] +
                                     sm[3][threadIdx.x];
        if (s) atomicAdd(reinterpret_cast<unsigned long long*>(counts) + threadIdx.x, s);
    }
}

// one workgroup; thread c owns class c and walks the images in index order: the float64 sums are the sequence a host loop
// over the same images produces.  One division per term and nothing to contract around it.
__global__ __launch_bounds__(64) void metrics_accumulate_kernel(const long long* __restrict__ counts, int N, int C, long long HW,
                                                                long long* __restrict__ acc) {
    const int c = threadIdx.x;
    double* facc = reinterpret_cast<double*>(acc);
    if (c < C) {
        double dice = facc[c], iou = facc[MAXC + c];
        long long tp = 0, si = 0, st = 0;
        for (int n = 0; n < N; ++n) {
            const long long* q = counts + ((long)n * C + c) * 3;
            const long long a = q[0], b = q[1], d = q[2], uni = b + d;
            const double dn = (double)(2 * a), dd = (double)uni, in = (double)a, id = (double)(uni - a);
            const double dv = uni == 0 ? 1.0 : dn / dd;
            const double iv = uni == 0 ? 1.0 : in / id;
            dice += dv;
            iou += iv;
            tp += a; si += b; st += d;
        }
        facc[c] = dice;
        facc[MAXC + c] = iou;
        acc[2 * MAXC + c] += tp;
        acc[3 * MAXC + c] += si;
        acc[4 * MAXC + c] += st;
    }
    if (c == 63) {
        acc[5 * MAXC] += N;
        acc[5 * MAXC + 1] += (long long)N * HW;
    }
}

template <int C, int KIND, typename TT>
void launch_counts(bool vec, dim3 grid, hipStream_t stream, double bytes, const float* logits, long l_bs, const void* target,
                   long t_bs, int HW, long long* counts) {
    const TT* t = static_cast<const TT*>(target);
    if (vec)
        AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, bytes, (counts_logits_kernel<C, KIND, 4, TT>), grid, dim3(256), 0, stream, logits,
                          l_bs, t, t_bs, HW, counts);
    else
        AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, bytes, (counts_logits_kernel<C, KIND, 1, TT>), grid, dim3(256), 0, stream, logits,
                          l_bs, t, t_bs, HW, counts);
}

template <int C>
void launch_counts_kind(int kind, bool vec, dim3 grid, hipStream_t stream, double bytes, const float* logits, long l_bs,
                        const void* target, long t_bs, int HW, long long* counts) {
    switch (kind) {
        case T_ONEHOT_F32: launch_counts<C, T_ONEHOT_F32, float>(vec, grid, stream, bytes, logits, l_bs, target, t_bs, HW, counts); break;
        case T_ONEHOT_I64: launch_counts<C, T_ONEHOT_I64, long long>(vec, grid, stream, bytes, logits, l_bs, target, t_bs, HW, counts); break;
        case T_ONEHOT_U8: launch_counts<C, T_ONEHOT_U8, unsigned char>(vec, grid, stream, bytes, logits, l_bs, target, t_bs, HW, counts); break;
        default: launch_counts<C, T_INDEX_I64, long long>(vec, grid, stream, bytes, logits, l_bs, target, t_bs, HW, counts); break;
    }
}

}  // namespace

extern "C" {

int aide_mc_counts_logits(const float* logits, int64_t l_bs, const void* target, int t_kind, int64_t t_bs, int C, int64_t N,
                          int64_t HW, long long* counts, hipStream_t stream) {
    if (C < 2 || C > MAXC || t_kind < T_ONEHOT_F32 || t_kind > T_INDEX_I64 || N < 0 || N > 65535 || HW < 0 ||
        HW > INT32_MAX || (int64_t)C * HW > INT32_MAX)
        return AIDE_ERR_ARG;
    const int64_t t_img = t_kind == T_INDEX_I64 ? HW : (int64_t)C * HW;
    if (N > 1 && (l_bs < (int64_t)C * HW || t_bs < t_img)) return AIDE_ERR_ARG;   // images must not overlap
    if (N == 0) return 0;
    if (!counts) return AIDE_ERR_ARG;
    hipError_t e = hipMemsetAsync(counts, 0, (size_t)N * C * 3 * sizeof(long long), stream);
    if (e != hipSuccess) return (int)e;
    if (HW == 0) return 0;
    if (!logits || !target) return AIDE_ERR_ARG;
    const size_t tsz = t_kind == T_ONEHOT_F32 ? 4 : t_kind == T_ONEHOT_U8 ? 1 : 8;
    const bool vec = HW % 4 == 0 && l_bs % 4 == 0 && t_bs % 4 == 0 && (reinterpret_cast<uintptr_t>(logits) & 15) == 0 &&
                     (reinterpret_cast<uintptr_t>(target) & (4 * tsz - 1)) == 0;
    const long per = vec ? 1024 : 256;
    const long want = (HW + per - 1) / per, cap = max(1L, 2048L / N);
    const dim3 grid((unsigned)min(want, cap), (unsigned)N);
    const double bytes = (double)N * HW * (4.0 * C + (t_kind == T_INDEX_I64 ? 8.0 : (double)tsz * C));
#define L(CC) launch_counts_kind<CC>(t_kind, vec, grid, stream, bytes, logits, (long)l_bs, target, (long)t_bs, (int)HW, counts)
    switch (C) {
        case 2: L(2); break; case 3: L(3); break; case 4: L(4); break; case 5: L(5); break;
        case 6: L(6); break; case 7: L(7); break; default: L(8); break;
    }
#undef L
    return aide_launch_status();
}

int aide_mc_counts_labels(const void* p, int p_u8, int64_t p_s0, int64_t p_s1, int64_t p_s2, const void* t, int t_u8,
                          int64_t t_s0, int64_t t_s1, int64_t t_s2, int64_t d0, int64_t d1, int64_t d2, int C,
                          long long* counts, hipStream_t stream) {
    if (!dims_ok(d0, d1, d2) || !counts || C < 2 || C > MAXC || (p_u8 != 0 && p_u8 != 1) || (t_u8 != 0 && t_u8 != 1))
        return AIDE_ERR_ARG;
    const int n = (int)(d0 * d1 * d2);
    if (n > 0 && (!p || !t)) return AIDE_ERR_ARG;
    hipError_t e = hipMemsetAsync(counts, 0, (size_t)C * 3 * sizeof(long long), stream);
    if (e != hipSuccess) return (int)e;
    if (n == 0) return 0;
    const Operand P{p, (long)p_s0, (long)p_s1, (long)p_s2, p_u8}, T{t, (long)t_s0, (long)t_s1, (long)t_s2, t_u8};
    const dim3 grid((unsigned)min(((long)n + 1023) / 1024, 1024L)), block(256);
    const int e1 = (int)d1, e2 = (int)d2;
    if (p_u8 && t_u8)
        AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 2.0 * n, (counts_labels_kernel<unsigned char, unsigned char>), grid, block, 0, stream, P, T, e1, e2, n, C, counts);
    else if (p_u8)
        AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 9.0 * n, (counts_labels_kernel<unsigned char, long long>), grid, block, 0, stream, P, T, e1, e2, n, C, counts);
    else if (t_u8)
        AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 9.0 * n, (counts_labels_kernel<long long, unsigned char>), grid, block, 0, stream, P, T, e1, e2, n, C, counts);
    else
        AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 16.0 * n, (counts_labels_kernel<long long, long long>), grid, block, 0, stream, P, T, e1, e2, n, C, counts);
    return aide_launch_status();
}

int aide_mc_metrics_accumulate(const long long* counts, int64_t N, int C, int64_t HW, void* acc, hipStream_t stream) {
    if (C < 2 || C > MAXC || N < 0 || N > INT32_MAX || HW < 0 || HW > INT32_MAX || !acc ||
        (reinterpret_cast<uintptr_t>(acc) & 7) != 0)
        return AIDE_ERR_ARG;
    if (N == 0) return 0;
    if (!counts) return AIDE_ERR_ARG;
    AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 0.0, metrics_accumulate_kernel, dim3(1), dim3(64), 0, stream, counts, (int)N, C,
                      (long long)HW, static_cast<long long*>(acc));
    return aide_launch_status();
}

}  // extern "C"
