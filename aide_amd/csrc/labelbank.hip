// Pseudo-label refresh of the proposed loop (include/aide_hip.h "pseudo-label bank"): the case Dice values from the batched
// confusion sums, their ranking and the selection rule of trainchaos_proposed_30cases1labeled.py:528-575, the rewrite of the
// selected cases' planes in the device-resident bank, and the loader's one-hot targets gathered from the bank.  The host
// decides nothing between evaluation and update: `selected` is written and read on the device.
// The per-class form (multi-organ banks, C = 2 .. 8) does the same with a score that is the mean Dice of the organs present:
// per-case, per-class counts, the rule, bank = palette[prediction], and class-index targets.
#include "common.h"

namespace {

constexpr int MAX_CASES = 4096;

// a sorts before b: ascending, NaN greatest; equal values (two NaNs included) by the lower case index
__device__ __forceinline__ bool before(float a, int ia, float b, int ib) {
    const bool na = a != a, nb = b != b;
    if (na || nb) return na == nb ? ia < ib : nb;
    return a < b || (a == b && ia < ib);
}

// one workgroup: dice[k] = float(2 * sum p*t / (sum p + sum t)) with the division in fp64 (0 / 0 -> NaN), rank by counting
__global__ __launch_bounds__(256) void refresh_select_kernel(const long long* __restrict__ sums,
                                                             const unsigned char* __restrict__ labelled, int K, int n_select,
                                                             float* __restrict__ dice, int* __restrict__ rank,
                                                             unsigned char* __restrict__ selected) {
    __shared__ float d[MAX_CASES];
    for (int k = threadIdx.x; k < K; k += 256) {
        const double inter = (double)(2 * sums[4 * k + 1]), uni = (double)(sums[4 * k + 2] + sums[4 * k + 3]);
        const float v = (float)(inter / uni);
        d[k] = v;
        dice[k] = v;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < K; k += 256) {
        const float v = d[k];
        int r = 0;
        for (int j = 0; j < K; ++j) r += before(d[j], j, v, k) ? 1 : 0;
        rank[k] = r;
        selected[k] = (r < n_select && !(labelled && labelled[k])) ? 1 : 0;
    }
}

// bank[slices of k] = pred * scale for the selected cases; VEC: 16 bytes per thread (hw % 16 == 0, aligned)
template <bool VEC>
__global__ __launch_bounds__(256) void bank_update_kernel(const unsigned char* __restrict__ pred,
                                                          const unsigned char* __restrict__ selected,
                                                          const long long* __restrict__ start, int S_total, long hw, int scale,
                                                          unsigned char* __restrict__ bank) {
    const int k = blockIdx.y;
    if (!selected[k]) return;
    int s0, ns;
    case_range(start, k, S_total, s0, ns);
    const long n = ns * hw;
    const unsigned char* src = pred + s0 * hw;
    unsigned char* dst = bank + s0 * hw;
    if (VEC) {
        for (long o = ((long)blockIdx.x * 256 + threadIdx.x) * 16; o < n; o += (long)gridDim.x * 256 * 16) {
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
        for (long o = (long)blockIdx.x * 256 + threadIdx.x; o < n; o += (long)gridDim.x * 256)
            dst[o] = (unsigned char)(src[o] * (unsigned)scale);
    }
}

// out[n][c][p] = (bank[idx[n]][p] == palette[c]); a slice index outside the bank gives an all-zero image
__global__ __launch_bounds__(256) void bank_targets_kernel(const unsigned char* __restrict__ bank, int S_total, long hw,
                                                           const long long* __restrict__ idx, const int* __restrict__ palette,
                                                           int npal, long long* __restrict__ out) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= hw) return;
    const int n = blockIdx.y;
    const long long s = idx[n];
    const int v = (s >= 0 && s < S_total) ? (int)bank[s * hw + p] : -1;
    long long* o = out + (long)n * npal * hw + p;
    for (int c = 0; c < npal; ++c) o[c * hw] = palette[c] == v ? 1 : 0;
}

// ---- per-class form: C = 2 .. 8 organs, class c <-> bank byte palette[c] ----------------------------------------------------
constexpr int MAXC = 8;

// byte -> class (the lowest c with palette[c] == byte), `none` for a byte outside the palette; needs 256 threads
__device__ __forceinline__ void class_table(const int* __restrict__ palette, int C, int none, unsigned char* tbl) {
    int c = 0;
    while (c < C && palette[c] != (int)threadIdx.x) ++c;
    tbl[threadIdx.x] = (unsigned char)(c < C ? c : none);
    __syncthreads();
}

// eight 8-bit counters in one register, one per class: no per-thread array is indexed at run time.  Class 8 counts nowhere;
// a class in C .. 7 ("no class" when C < 8) counts into a byte that is never read.
__device__ __forceinline__ unsigned long long class_slot(unsigned c) { return c < 8u ? 1ull << (c * 8u) : 0ull; }

struct ClassCounts {
    unsigned long long i8, p8, t8;       // pending: at most 255 voxels since the last flush
    unsigned acc[3][MAXC];               // a thread sees fewer than 2^31 voxels
    __device__ __forceinline__ void add(unsigned f, unsigned cb, unsigned C) {
        const unsigned cf = f < C ? f : C;
        const unsigned long long s = class_slot(cf);
        p8 += s;
        t8 += class_slot(cb);
        i8 += cf == cb ? s : 0ull;
    }
    __device__ __forceinline__ void flush() {
#pragma unroll
        for (int c = 0; c < MAXC; ++c) {
            acc[0][c] += (unsigned)(i8 >> (8 * c)) & 255u;
            acc[1][c] += (unsigned)(p8 >> (8 * c)) & 255u;
            acc[2][c] += (unsigned)(t8 >> (8 * c)) & 255u;
        }
        i8 = p8 = t8 = 0;
    }
};

// out[k][c][0..2] += #(f == c && b == palette[c]), #(f == c), #(b == palette[c]) over the slices of case k (out zeroed before);
// VEC: 16 bytes per load (hw % 16 == 0, aligned)
template <bool VEC>
__global__ __launch_bounds__(256) void class_counts_batched_kernel(const unsigned char* __restrict__ p,
                                                                   const unsigned char* __restrict__ bank,
                                                                   const long long* __restrict__ start, int S_total, long hw,
                                                                   const int* __restrict__ palette, int C,
                                                                   long long* __restrict__ out) {
    __shared__ unsigned char tbl[256];
    __shared__ unsigned sm[4][3 * MAXC];
    class_table(palette, C, C, tbl);
    const int k = blockIdx.y;
    int s0, ns;
    case_range(start, k, S_total, s0, ns);
    const long n = ns * hw;
    const unsigned char* pp = p + s0 * hw;
    const unsigned char* bp = bank + s0 * hw;
    ClassCounts a = {};
    int pending = 0;
    if (VEC) {
        for (long o = ((long)blockIdx.x * 256 + threadIdx.x) * 16; o < n; o += (long)gridDim.x * 256 * 16) {
            const uint4 x = *reinterpret_cast<const uint4*>(pp + o);
            const uint4 y = *reinterpret_cast<const uint4*>(bp + o);
            const unsigned xw[4] = {x.x, x.y, x.z, x.w}, yw[4] = {y.x, y.y, y.z, y.w};
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int sh = 0; sh < 32; sh += 8) a.add((xw[j] >> sh) & 255u, tbl[(yw[j] >> sh) & 255u], (unsigned)C);
            if (++pending == 15) { a.flush(); pending = 0; }
        }
    } else {
        for (long o = (long)blockIdx.x * 256 + threadIdx.x; o < n; o += (long)gridDim.x * 256) {
            a.add(pp[o], tbl[bp[o]], (unsigned)C);
            if (++pending == 255) { a.flush(); pending = 0; }
        }
    }
    a.flush();
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int c = 0; c < MAXC; ++c) {
            unsigned v = a.acc[j][c];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
            if (lane == 0) sm[wid][c * 3 + j] = v;
        }
    __syncthreads();
    if ((int)threadIdx.x < 3 * C) {
        const unsigned long long s = (unsigned long long)sm[0][threadIdx.x] + sm[1][threadIdx.x] + sm[2][threadIdx.x] +
                                     sm[3][threadIdx.x];
        if (s) atomicAdd(reinterpret_cast<unsigned long long*>(out + (long)k * C * 3 + threadIdx.x), s);
    }
}

// one workgroup: class_dice[k][c] = float(2 I / (P + T)) with the division in fp64; dice[k] = float(the fp64 mean, summed in
// ascending c, of the foreground classes with P + T > 0), NaN without one; rank and selection as refresh_select_kernel
__global__ __launch_bounds__(256) void refresh_select_classes_kernel(const long long* __restrict__ counts,
                                                                     const unsigned char* __restrict__ labelled, int K, int C,
                                                                     int n_select, float* __restrict__ class_dice,
                                                                     float* __restrict__ dice, int* __restrict__ rank,
                                                                     unsigned char* __restrict__ selected) {
    __shared__ float d[MAX_CASES];
    for (int k = threadIdx.x; k < K; k += 256) {
        const long long* row = counts + (long)k * C * 3;
        double sum = 0.0;
        int present = 0;
        for (int c = 0; c < C; ++c) {
            const long long uni = row[3 * c + 1] + row[3 * c + 2];
            const double dc = (double)(2 * row[3 * c]) / (double)uni;
            class_dice[(long)k * C + c] = (float)dc;
            if (c > 0 && uni > 0) { sum += dc; ++present; }
        }
        const float v = (float)(sum / (double)present);        // no organ: 0 / 0, the NaN of refresh_select_kernel
        d[k] = v;
        dice[k] = v;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < K; k += 256) {
        const float v = d[k];
        int r = 0;
        for (int j = 0; j < K; ++j) r += before(d[j], j, v, k) ? 1 : 0;
        rank[k] = r;
        selected[k] = (r < n_select && !(labelled && labelled[k])) ? 1 : 0;
    }
}

// the palette bytes packed into one register: byte c = palette[c]
__device__ __forceinline__ unsigned long long pack_palette(const int* __restrict__ palette, int C) {
    unsigned long long pal = 0;
    for (int c = 0; c < C; ++c) pal |= (unsigned long long)(palette[c] & 255) << (8 * c);
    return pal;
}

__device__ __forceinline__ unsigned palette_byte(unsigned long long pal, unsigned v, unsigned C) {
    return (unsigned)(pal >> (8u * (v < C ? v : 0u))) & 255u;
}

// bank[slices of k] = palette[pred] (a value >= C: palette[0]) for the selected cases; VEC as bank_update_kernel
template <bool VEC>
__global__ __launch_bounds__(256) void bank_update_classes_kernel(const unsigned char* __restrict__ pred,
                                                                  const unsigned char* __restrict__ selected,
                                                                  const long long* __restrict__ start, int S_total, long hw,
                                                                  const int* __restrict__ palette, int C,
                                                                  unsigned char* __restrict__ bank) {
    const int k = blockIdx.y;
    if (!selected[k]) return;
    const unsigned long long pal = pack_palette(palette, C);
    int s0, ns;
    case_range(start, k, S_total, s0, ns);
    const long n = ns * hw;
    const unsigned char* src = pred + s0 * hw;
    unsigned char* dst = bank + s0 * hw;
    if (VEC) {
        for (long o = ((long)blockIdx.x * 256 + threadIdx.x) * 16; o < n; o += (long)gridDim.x * 256 * 16) {
            const uint4 a = *reinterpret_cast<const uint4*>(src + o);
            unsigned w[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                unsigned r = 0;
#pragma unroll
                for (int sh = 0; sh < 32; sh += 8) r |= palette_byte(pal, (w[j] >> sh) & 255u, (unsigned)C) << sh;
                w[j] = r;
            }
            *reinterpret_cast<uint4*>(dst + o) = make_uint4(w[0], w[1], w[2], w[3]);
        }
    } else {
        for (long o = (long)blockIdx.x * 256 + threadIdx.x; o < n; o += (long)gridDim.x * 256)
            dst[o] = (unsigned char)palette_byte(pal, src[o], (unsigned)C);
    }
}

// out[n][p] = the class of bank[idx[n]][p], `ignore` for a byte outside the palette or a slice index outside the bank
__global__ __launch_bounds__(256) void bank_targets_index_kernel(const unsigned char* __restrict__ bank, int S_total, long hw,
                                                                 const long long* __restrict__ idx,
                                                                 const int* __restrict__ palette, int C, long long ignore,
                                                                 long long* __restrict__ out) {
    __shared__ unsigned char tbl[256];
    class_table(palette, C, C, tbl);
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= hw) return;
    const int n = blockIdx.y;
    const long long s = idx[n];
    const int c = (s >= 0 && s < S_total) ? (int)tbl[bank[s * hw + p]] : C;
    out[(long)n * hw + p] = c < C ? (long long)c : ignore;
}

bool plane_ok(int64_t S_total, int64_t H, int64_t W) {
    if (S_total < 0 || H < 0 || W < 0) return false;
    if (S_total == 0 || H == 0 || W == 0) return true;
    return H <= INT32_MAX && W <= INT32_MAX && H * W <= INT32_MAX && S_total <= INT32_MAX && S_total * (H * W) <= INT32_MAX;
}

}  // namespace

extern "C" {

int aide_label_refresh_select(const long long* sums, const unsigned char* labelled, int64_t K, int64_t n_select, float* dice,
                              int* rank, unsigned char* selected, hipStream_t stream) {
    if (K < 0 || K > MAX_CASES || n_select < 0) return AIDE_ERR_ARG;
    if (K == 0) return 0;
    if (!sums || !dice || !rank || !selected) return AIDE_ERR_ARG;
    AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 0.0, refresh_select_kernel, dim3(1), dim3(256), 0, stream, sums, labelled, (int)K,
                      (int)min(n_select, (int64_t)MAX_CASES), dice, rank, selected);
    return aide_launch_status();
}

int aide_label_bank_update(const unsigned char* pred, const unsigned char* selected, const long long* slice_start, int64_t K,
                           int64_t S_total, int64_t H, int64_t W, int scale, unsigned char* bank_plane, hipStream_t stream) {
    if (!plane_ok(S_total, H, W) || K < 0 || K > 65535 || scale < 0 || scale > 255) return AIDE_ERR_ARG;
    const long hw = (long)(H * W);
    if (K == 0 || S_total * hw == 0) return 0;
    if (!pred || !selected || !slice_start || !bank_plane) return AIDE_ERR_ARG;
    const bool vec = hw % 16 == 0 && ((reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(bank_plane)) & 15) == 0;
    const long per = vec ? 4096 : 256;
    const dim3 grid((unsigned)max(1L, min((hw + per - 1) / per * 4, 1024L)), (unsigned)K), block(256);
    const double bytes = 2.0 * (double)S_total * (double)hw;
    if (vec)
        AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, bytes, bank_update_kernel<true>, grid, block, 0, stream, pred, selected, slice_start,
                          (int)S_total, hw, scale, bank_plane);
    else
        AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, bytes, bank_update_kernel<false>, grid, block, 0, stream, pred, selected, slice_start,
                          (int)S_total, hw, scale, bank_plane);
    return aide_launch_status();
}

int aide_label_bank_targets(const unsigned char* bank_plane, int64_t S_total, int64_t H, int64_t W, const long long* slice_idx,
                            int64_t N, const int* palette, int npal, long long* out, hipStream_t stream) {
    if (!plane_ok(S_total, H, W) || N < 0 || N > 65535 || npal < 1 || npal > 8) return AIDE_ERR_ARG;
    const long hw = (long)(H * W);
    if (N == 0 || hw == 0) return 0;
    if (!slice_idx || !palette || !out || (S_total > 0 && !bank_plane)) return AIDE_ERR_ARG;
    const dim3 grid((unsigned)((hw + 255) / 256), (unsigned)N), block(256);
    AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, (double)N * hw * (1.0 + 8.0 * npal), bank_targets_kernel, grid, block, 0, stream,
                      bank_plane, (int)S_total, hw, slice_idx, palette, npal, out);
    return aide_launch_status();
}

int aide_case_class_counts_batched(const unsigned char* pred, const unsigned char* bank_plane, const long long* slice_start,
                                   int64_t K, int64_t S_total, int64_t H, int64_t W, const int* palette, int C, long long* out,
                                   hipStream_t stream) {
    if (!plane_ok(S_total, H, W) || K < 0 || K > 65535 || C < 2 || C > MAXC) return AIDE_ERR_ARG;
    if (K == 0) return 0;
    if (!out || !slice_start || !palette) return AIDE_ERR_ARG;
    const long hw = (long)(H * W);
    if (S_total * hw > 0 && (!pred || !bank_plane)) return AIDE_ERR_ARG;
    hipError_t e = hipMemsetAsync(out, 0, (size_t)K * C * 3 * sizeof(long long), stream);
    if (e != hipSuccess) return (int)e;
    const bool vec = hw % 16 == 0 && ((reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(bank_plane)) & 15) == 0;
    const long per = vec ? 4096 : 256;
    const dim3 grid((unsigned)max(1L, min((hw + per - 1) / per * 4, 1024L)), (unsigned)K), block(256);
    const double bytes = 2.0 * (double)S_total * (double)hw;
    if (vec)
        AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, bytes, class_counts_batched_kernel<true>, grid, block, 0, stream, pred, bank_plane,
                          slice_start, (int)S_total, hw, palette, C, out);
    else
        AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, bytes, class_counts_batched_kernel<false>, grid, block, 0, stream, pred, bank_plane,
                          slice_start, (int)S_total, hw, palette, C, out);
    return aide_launch_status();
}

int aide_label_refresh_select_classes(const long long* counts, const unsigned char* labelled, int64_t K, int C, int64_t n_select,
                                      float* class_dice, float* dice, int* rank, unsigned char* selected, hipStream_t stream) {
    if (K < 0 || K > MAX_CASES || n_select < 0 || C < 2 || C > MAXC) return AIDE_ERR_ARG;
    if (K == 0) return 0;
    if (!counts || !class_dice || !dice || !rank || !selected) return AIDE_ERR_ARG;
    AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 0.0, refresh_select_classes_kernel, dim3(1), dim3(256), 0, stream, counts, labelled, (int)K,
                      C, (int)min(n_select, (int64_t)MAX_CASES), class_dice, dice, rank, selected);
    return aide_launch_status();
}

int aide_label_bank_update_classes(const unsigned char* pred, const unsigned char* selected, const long long* slice_start,
                                   int64_t K, int64_t S_total, int64_t H, int64_t W, const int* palette, int C,
                                   unsigned char* bank_plane, hipStream_t stream) {
    if (!plane_ok(S_total, H, W) || K < 0 || K > 65535 || C < 2 || C > MAXC) return AIDE_ERR_ARG;
    const long hw = (long)(H * W);
    if (K == 0 || S_total * hw == 0) return 0;
    if (!pred || !selected || !slice_start || !palette || !bank_plane) return AIDE_ERR_ARG;
    const bool vec = hw % 16 == 0 && ((reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(bank_plane)) & 15) == 0;
    const long per = vec ? 4096 : 256;
    const dim3 grid((unsigned)max(1L, min((hw + per - 1) / per * 4, 1024L)), (unsigned)K), block(256);
    const double bytes = 2.0 * (double)S_total * (double)hw;
    if (vec)
        AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, bytes, bank_update_classes_kernel<true>, grid, block, 0, stream, pred, selected,
                          slice_start, (int)S_total, hw, palette, C, bank_plane);
    else
        AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, bytes, bank_update_classes_kernel<false>, grid, block, 0, stream, pred, selected,
                          slice_start, (int)S_total, hw, palette, C, bank_plane);
    return aide_launch_status();
}

int aide_label_bank_targets_index(const unsigned char* bank_plane, int64_t S_total, int64_t H, int64_t W,
                                  const long long* slice_idx, int64_t N, const int* palette, int C, int64_t ignore_index,
                                  long long* out, hipStream_t stream) {
    if (!plane_ok(S_total, H, W) || N < 0 || N > 65535 || C < 2 || C > MAXC) return AIDE_ERR_ARG;
    const long hw = (long)(H * W);
    if (N == 0 || hw == 0) return 0;
    if (!slice_idx || !palette || !out || (S_total > 0 && !bank_plane)) return AIDE_ERR_ARG;
    const dim3 grid((unsigned)((hw + 255) / 256), (unsigned)N), block(256);
    AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, (double)N * hw * 9.0, bank_targets_index_kernel, grid, block, 0, stream, bank_plane,
                      (int)S_total, hw, slice_idx, palette, C, (long long)ignore_index, out);
    return aide_launch_status();
}

}  // extern "C"
