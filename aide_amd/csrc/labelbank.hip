// Pseudo-label refresh (include/aide_hip.h "pseudo-label bank" and "per-image pseudo-label bank").  Three banks share this file:
//   case bank      trainchaos_proposed_30cases1labeled.py:528-575: the case Dice from the batched confusion sums, the ranking, the
//                  rewrite of the selected cases' slices, and the loader's one-hot targets gathered from the bank;
//   per-class      the same for multi-organ banks (C = 2 .. 8) with the mean Dice of the organs present: per-case, per-class
//                  counts, bank = palette[prediction], class-index targets;
//   per-image      trainkidney_proposed_mask1.py:373-434, trainbreast_dataset3_proposed_272cases25labeled.py:373-438: every training
//                  IMAGE is scored with Dice2d against a plane of the bank (the fused epilogue of a forward batch: labels + exact
//                  sums) and the worst int(update_percent * K) whose prediction is not empty get it as their new label.
// What they share is stated once: score_kernel (a scoring rule per bank) -> rank_kernel (THE ranking rule) -> update_kernel (a
// byte map and a range source per bank).  The host decides nothing between evaluation and update: the flags are written and read
// on the device, and nothing here waits across workgroups.
#include "common.h"

namespace {

constexpr int MAX_CASES = 4096;
constexpr int MAX_IMAGES = 1 << 20;
constexpr int MAXC = 8;
constexpr int CHUNK = 4096;          // pixels per workgroup of the image epilogue: 256 threads x 4 groups of 4
constexpr int TILE = 4096;           // keys per LDS tile of the ranking
constexpr int OWN = 4;               // items ranked per thread

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

bool plane_ok(int64_t S_total, int64_t H, int64_t W) {
    if (S_total < 0 || H < 0 || W < 0) return false;
    if (S_total == 0 || H == 0 || W == 0) return true;
    return H <= INT32_MAX && W <= INT32_MAX && H * W <= INT32_MAX && S_total <= INT32_MAX && S_total * (H * W) <= INT32_MAX;
}

// K images of H x W: every index that the kernels form stays below 2^31 blocks and 2^62 bytes
bool image_ok(int64_t K, int64_t H, int64_t W) {
    if (K < 0 || K > MAX_IMAGES || H < 0 || W < 0) return false;
    if (H == 0 || W == 0) return true;
    return H <= INT32_MAX && W <= INT32_MAX && H * W <= INT32_MAX;
}

// ---- score: dice[k] and the item's eligibility -------------------------------------------------------------------------------------
// A rule is (k, eligible) -> dice[k]; it may clear `eligible`, which starts as !labelled[k].  Every rule is integer sums, fp64
// quotients and plain sums of quotients: no product next to a sum, so -ffp-contract=fast has nothing to contract.

// case bank, sums[K][4]: float(2 * sum p*t / (sum p + sum t)) with the division in fp64 (0 / 0 -> NaN)
struct BinaryScore {
    const long long* sums;
    __device__ float operator()(int k, bool&) const {
        return (float)((double)(2 * sums[4 * k + 1]) / (double)(sums[4 * k + 2] + sums[4 * k + 3]));
    }
};

// per-class bank, counts[K][C][3]: class_dice[k][c] = float(2 I / (P + T)) with the division in fp64; the score is float(the fp64
// mean, summed in ascending c, of the foreground classes with P + T > 0), without one the 0 / 0 NaN of BinaryScore
struct ClassScore {
    const long long* counts;
    int C;
    float* class_dice;
    __device__ float operator()(int k, bool&) const {
        const long long* row = counts + (long)k * C * 3;
        double sum = 0.0;
        int present = 0;
        for (int c = 0; c < C; ++c) {
            const long long uni = row[3 * c + 1] + row[3 * c + 2];
            const double dc = (double)(2 * row[3 * c]) / (double)uni;
            class_dice[(long)k * C + c] = (float)dc;
            if (c > 0 && uni > 0) { sum += dc; ++present; }
        }
        return (float)(sum / (double)present);
    }
};

// per-image bank, sums[K][4]: Dice2d (:131-141), 0.0 when sum p + sum t == 0, else the fp64 quotient rounded once to float32; an
// empty prediction is never written (:418 `if save_data.sum() > 0`)
struct ImageScore {
    const long long* sums;
    __device__ float operator()(int k, bool& eligible) const {
        const long long uni = sums[4 * k + 2] + sums[4 * k + 3];
        eligible = eligible && sums[4 * k + 2] > 0;
        return uni == 0 ? 0.0f : (float)((double)(2 * sums[4 * k + 1]) / (double)uni);
    }
};

template <class Score>
__global__ __launch_bounds__(256) void score_kernel(Score score, const unsigned char* __restrict__ labelled, int K,
                                                    float* __restrict__ dice, unsigned char* __restrict__ flag) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= K) return;
    bool eligible = !(labelled && labelled[k]);
    dice[k] = score(k, eligible);
    flag[k] = eligible ? 1 : 0;
}

// ---- rank: the one ranking rule -----------------------------------------------------------------------------------------------------
// Ascending score, NaN greatest, equal values to the lower index: j sorts before k when key[j] < key[k], or key[j] == key[k] and
// j < k.  The key is the float as an unsigned in that order: -0 == +0, and every NaN is the greatest key and equal to every other
// NaN, so two NaNs fall to the lower index like any other tie.  (Spelled on floats: neither NaN -> a < b || (a == b && ia < ib);
// one NaN -> the other sorts first; both -> ia < ib.)  This is this project's rule, not parity with the reference, whose sort is
// not stable.
__device__ __forceinline__ unsigned sort_key(float v) {
    if (v != v) return 0xffffffffu;
    const unsigned u = __float_as_uint(v + 0.0f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// rank[k] = |{j : j sorts before k}|, a counting rank, and flag[k] &= rank[k] < n_select.  A workgroup owns the 1024 items
// [1024 b, 1024 b + 1024), four per thread, and walks all K keys through LDS tiles; a tile that lies wholly below / above the
// owned range needs one comparison per pair (<= / <), the one or two tiles that meet it the full rule.  The tail of the last
// tile is padded with the greatest key at indices >= K, which no item counts (an index above its own, never a smaller key).
// No index depends on a key, so a NaN cannot send an access anywhere.
__global__ __launch_bounds__(256) void rank_kernel(const float* __restrict__ dice, int K, int n_select, int* __restrict__ rank,
                                                   unsigned char* __restrict__ flag) {
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
            flag[k] = (flag[k] && cnt[i] < n_select) ? 1 : 0;
        }
    }
}

// score then rank: dice, rank and flag[k] = rank[k] < n_select && eligible[k] for K items; two launches for any K
template <class Score>
int launch_select(Score score, const unsigned char* labelled, int64_t K, int64_t n_select, float* dice, int* rank,
                  unsigned char* flag, hipStream_t stream) {
    AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 0.0, score_kernel<Score>, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, stream, score,
                      labelled, (int)K, dice, flag);
    AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 0.0, rank_kernel, dim3((unsigned)((K + 256 * OWN - 1) / (256 * OWN))), dim3(256), 0, stream,
                      dice, (int)K, (int)min(n_select, K), rank, flag);
    return aide_launch_status();
}

// ---- update: the rewrite of the flagged items ------------------------------------------------------------------------------------------
// byte maps: load() runs once per thread before the loop
struct ScaleMap {                    // v * scale
    unsigned scale;
    __device__ void load() {}
    __device__ unsigned operator()(unsigned v) const { return (v * scale) & 255u; }
};

struct PaletteMap {                  // palette[v < C ? v : 0]; the palette bytes packed into one register: byte c = palette[c]
    const int* palette;
    unsigned C;
    unsigned long long pal;
    __device__ void load() {
        pal = 0;
        for (unsigned c = 0; c < C; ++c) pal |= (unsigned long long)(palette[c] & 255) << (8 * c);
    }
    __device__ unsigned operator()(unsigned v) const { return (unsigned)(pal >> (8u * (v < C ? v : 0u))) & 255u; }
};

// range sources: where item k's bytes lie, and how many workgroups share an item (vec: 16 bytes per thread, else one)
struct CaseRanges {                  // the slices [start[k], start[k + 1]) of hw bytes each, clamped to the bank
    const long long* start;
    int S_total;
    long hw;
    __device__ void operator()(long k, long& off, long& n) const {
        int s0, ns;
        case_range(start, (int)k, S_total, s0, ns);
        off = s0 * hw;
        n = ns * hw;
    }
    long chunks(bool vec) const { return min((hw + (vec ? 4095 : 255)) / (vec ? 4096 : 256) * 4, 1024L); }
};

struct Planes {                      // plane k of hw bytes; 4096 bytes per workgroup
    long hw;
    __device__ void operator()(long k, long& off, long& n) const {
        off = k * hw;
        n = hw;
    }
    long chunks(bool) const { return (hw + 4095) / 4096; }
};

// bank[bytes of item k] = map(pred[those bytes]) for the flagged items, the others are not touched.  Workgroup b is chunk
// b % chunks of item b / chunks (a 1-D grid: K may pass the 65535 of gridDim.y) and walks the item in steps of chunks * 256
// threads.  VEC: 16 bytes per thread (hw % 16 == 0, both planes 16-byte aligned).
template <class Map, class Range, bool VEC>
__global__ __launch_bounds__(256) void update_kernel(const unsigned char* __restrict__ pred, const unsigned char* __restrict__ flag,
                                                     Map map, Range range, int chunks, unsigned char* __restrict__ bank) {
    const long k = blockIdx.x / chunks;
    if (!flag[k]) return;
    map.load();
    long off, n;
    range(k, off, n);
    const unsigned char* src = pred + off;
    unsigned char* dst = bank + off;
    constexpr int B = VEC ? 16 : 1;
    for (long o = ((blockIdx.x - k * chunks) * 256 + threadIdx.x) * B; o < n; o += (long)chunks * 256 * B) {
        if (VEC) {
            const uint4 a = *reinterpret_cast<const uint4*>(src + o);
            unsigned w[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                unsigned r = 0;
#pragma unroll
                for (int sh = 0; sh < 32; sh += 8) r |= map((w[j] >> sh) & 255u) << sh;
                w[j] = r;
            }
            *reinterpret_cast<uint4*>(dst + o) = make_uint4(w[0], w[1], w[2], w[3]);
        } else {
            dst[o] = (unsigned char)map(src[o]);
        }
    }
}

// K >= 1 items of `bytes` bytes in all; at most 2^30 workgroups
template <class Map, class Range>
int launch_update(const unsigned char* pred, const unsigned char* flag, Map map, Range range, int64_t K, double bytes,
                  unsigned char* bank, hipStream_t stream) {
    const bool vec = range.hw % 16 == 0 && aligned16(pred) && aligned16(bank);
    const long chunks = max(1L, min(range.chunks(vec), (1L << 30) / (long)K));
    const auto kernel = vec ? update_kernel<Map, Range, true> : update_kernel<Map, Range, false>;
    AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 2.0 * bytes, kernel, dim3((unsigned)(K * chunks)), dim3(256), 0, stream, pred, flag, map, range,
                      (int)chunks, bank);
    return aide_launch_status();
}

// ---- case banks: targets and per-class counts --------------------------------------------------------------------------------------
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

// ---- per-image bank: the epilogue of a forward batch, and targets ---------------------------------------------------------------
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

// ---- case bank ----
int aide_label_refresh_select(const long long* sums, const unsigned char* labelled, int64_t K, int64_t n_select, float* dice,
                              int* rank, unsigned char* selected, hipStream_t stream) {
    if (K < 0 || K > MAX_CASES || n_select < 0) return AIDE_ERR_ARG;
    if (K == 0) return 0;
    if (!sums || !dice || !rank || !selected) return AIDE_ERR_ARG;
    return launch_select(BinaryScore{sums}, labelled, K, n_select, dice, rank, selected, stream);
}

int aide_label_bank_update(const unsigned char* pred, const unsigned char* selected, const long long* slice_start, int64_t K,
                           int64_t S_total, int64_t H, int64_t W, int scale, unsigned char* bank_plane, hipStream_t stream) {
    if (!plane_ok(S_total, H, W) || K < 0 || K > 65535 || scale < 0 || scale > 255) return AIDE_ERR_ARG;
    const long hw = (long)(H * W);
    if (K == 0 || S_total * hw == 0) return 0;
    if (!pred || !selected || !slice_start || !bank_plane) return AIDE_ERR_ARG;
    return launch_update(pred, selected, ScaleMap{(unsigned)scale}, CaseRanges{slice_start, (int)S_total, hw}, K,
                         (double)S_total * (double)hw, bank_plane, stream);
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

// ---- per-class bank ----
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
    const bool vec = hw % 16 == 0 && aligned16(pred) && aligned16(bank_plane);
    const long per = vec ? 4096 : 256;
    const dim3 grid((unsigned)max(1L, min((hw + per - 1) / per * 4, 1024L)), (unsigned)K), block(256);
    const double bytes = 2.0 * (double)S_total * (double)hw;
    const auto kernel = vec ? class_counts_batched_kernel<true> : class_counts_batched_kernel<false>;
    AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, bytes, kernel, grid, block, 0, stream, pred, bank_plane, slice_start, (int)S_total, hw, palette,
                      C, out);
    return aide_launch_status();
}

int aide_label_refresh_select_classes(const long long* counts, const unsigned char* labelled, int64_t K, int C, int64_t n_select,
                                      float* class_dice, float* dice, int* rank, unsigned char* selected, hipStream_t stream) {
    if (K < 0 || K > MAX_CASES || n_select < 0 || C < 2 || C > MAXC) return AIDE_ERR_ARG;
    if (K == 0) return 0;
    if (!counts || !class_dice || !dice || !rank || !selected) return AIDE_ERR_ARG;
    return launch_select(ClassScore{counts, C, class_dice}, labelled, K, n_select, dice, rank, selected, stream);
}

int aide_label_bank_update_classes(const unsigned char* pred, const unsigned char* selected, const long long* slice_start,
                                   int64_t K, int64_t S_total, int64_t H, int64_t W, const int* palette, int C,
                                   unsigned char* bank_plane, hipStream_t stream) {
    if (!plane_ok(S_total, H, W) || K < 0 || K > 65535 || C < 2 || C > MAXC) return AIDE_ERR_ARG;
    const long hw = (long)(H * W);
    if (K == 0 || S_total * hw == 0) return 0;
    if (!pred || !selected || !slice_start || !palette || !bank_plane) return AIDE_ERR_ARG;
    return launch_update(pred, selected, PaletteMap{palette, (unsigned)C, 0ull}, CaseRanges{slice_start, (int)S_total, hw}, K,
                         (double)S_total * (double)hw, bank_plane, stream);
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

// ---- per-image bank ----
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
    return launch_select(ImageScore{sums}, labelled, K, n_select, dice, rank, written, stream);
}

int aide_image_bank_update(const unsigned char* pred, const unsigned char* written, int64_t K, int64_t H, int64_t W, int scale,
                           unsigned char* plane, hipStream_t stream) {
    if (!image_ok(K, H, W) || scale < 0 || scale > 255) return AIDE_ERR_ARG;
    const long hw = (long)(H * W);
    if (K == 0 || hw == 0) return 0;
    if (!pred || !written || !plane) return AIDE_ERR_ARG;
    return launch_update(pred, written, ScaleMap{(unsigned)scale}, Planes{hw}, K, (double)K * (double)hw, plane, stream);
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
