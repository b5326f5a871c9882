// Pseudo-label refresh of the proposed loop (include/aide_hip.h "pseudo-label bank"): the case Dice values from the batched
// confusion sums, their ranking and the selection rule of trainchaos_proposed_30cases1labeled.py:528-575, the rewrite of the
// selected cases' planes in the device-resident bank, and the loader's one-hot targets gathered from the bank.  The host
// decides nothing between evaluation and update: `selected` is written and read on the device.
#include "common.h"

namespace {

constexpr int MAX_CASES = 4096;

// slices [s0, s0 + ns) of case k, clamped into [0, S_total] (as in eval3d.hip)
__device__ __forceinline__ void case_range(const long long* start, int k, int S_total, int& s0, int& ns) {
    long long a = start[k], b = start[k + 1];
    a = a < 0 ? 0 : (a > S_total ? S_total : a);
    b = b < a ? a : (b > S_total ? S_total : b);
    s0 = (int)a;
    ns = (int)(b - a);
}

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

}  // extern "C"
