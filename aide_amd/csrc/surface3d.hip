// Spacing-aware surface distances of a predicted volume P against its target T on the device: the raw sums behind RAVD, ASSD
// and MSSD (include/aide_hip.h "per-case evaluation"; the definitions are DESIGN.md section 4 "Surface distances").
//
// Foreground of an operand X: X != 0 (cls < 0) or X == cls.  Border: foreground with a face neighbour that is not foreground
// or lies outside the volume.  D_X(v) = the exact Euclidean distance, in fp64 and in units of the voxel spacing, from v to the
// nearest border voxel of X.  Launches (operand = blockIdx.y wherever both are handled):
//   1 surf_border   one thread per voxel of the two strided operands: the border maps as bytes in logical raster order,
//                   n_P, n_T, V_P, V_T with integer atomics (one per wave and counter).  From here on no stride is read.
//   2 surf_scan2    one thread per line along d2: g = integer distance to the nearest border voxel of the line, NONE when the
//                   line holds none (forward sweep, backward sweep)
//   3 surf_minplus<false>  along d1: f(i1) = min over j1 of (sp1 * (i1 - j1))^2 + (sp2 * g(j1))^2, +inf where g is NONE.
//                   A workgroup owns 64 neighbouring lines and walks them in chunks: 32 candidates in LDS, 32 results in
//                   registers (8 per thread); brute force, branch-free.
//   4 surf_minplus<true>   the same walk along d0 on the OTHER operand's f, kept only at the border voxels of this operand:
//                   sqrt, the optional distance map, and per workgroup one fp64 sum and one max, reduced in a fixed order and
//                   written to the workgroup's own slot
//   5 surf_finish   one workgroup adds the slots in slot order and writes S_PT, S_TP, M_PT, M_TP
// No workgroup waits for another, no floating-point atomic exists, every word of the workspace that is read was written by
// an earlier launch of the same call, and the order of every floating-point sum is fixed by the launch geometry: two calls on
// the same inputs give the same bytes.  "No border voxel" is the integer NONE after launch 2 and +inf after launch 3
// (inf + x = inf, min keeps the finite side, no product has an infinite factor: the spacings are finite); launch 4 takes a
// square root only of a finite minimum, which exists for every voxel as soon as the other operand has one border voxel.
// All indices come from integers.
//
// aide_surface3d_scores_select (percentiles of the distances and counts within a tolerance: HD95, NSD) runs the same launches
// with launch 4 as surf_minplus<true, true>, which also appends every distance to a per-operand list of uint64 keys, and then
// 8 x (sel_hist, sel_choose): an exact MSD radix select over those lists for all (set, rank) targets at once -- see there.
// Integer atomics only; the lists' order depends on the schedule and nothing computed from them does.
//
// aide_edt3d (the distance transform of one volume, every voxel evaluated) runs launches 2 and 3 on one operand whose
// candidates are its background voxels, between a launch that writes that map and edt_last, the walk along d0 with the square
// root -- see there.
#include "volume3d.h"

#include <cstring>

extern "C" size_t aide_surface3d_ws_bytes(int64_t nvox);

namespace {

constexpr int NONE = 0x7fffffff;   // surf_scan2: the line holds no border voxel (distances are < 2^31 - 1)
constexpr int COLS = 64;           // lines per workgroup = lanes of a wave: LDS rows are read without a bank conflict
constexpr int ROWS = 4;            // waves per workgroup, each owns R results of a chunk
constexpr int R = 8;
constexpr int OC = ROWS * R;       // results per chunk
constexpr int CH = 32;             // candidates per chunk in LDS: CH * COLS doubles = 16 KiB

__device__ __forceinline__ bool fg_at(const Operand& X, long off, int cls) {
    const long long v = X.at(off);
    return cls < 0 ? v != 0 : v == (long long)cls;
}

// -> 0: background, 1: inner foreground, 2: border
__device__ __forceinline__ int classify(const Operand& X, int i0, int i1, int i2, int d0, int d1, int d2, int cls) {
    const long off = X.off(i0, i1, i2);
    if (!fg_at(X, off, cls)) return 0;
    bool inner = i0 > 0 && i0 + 1 < d0 && i1 > 0 && i1 + 1 < d1 && i2 > 0 && i2 + 1 < d2;
    if (inner)
        inner = fg_at(X, off - X.s0, cls) && fg_at(X, off + X.s0, cls) && fg_at(X, off - X.s1, cls) &&
                fg_at(X, off + X.s1, cls) && fg_at(X, off - X.s2, cls) && fg_at(X, off + X.s2, cls);
    return inner ? 1 : 2;
}

// cnt[0..3] += n_P, n_T, V_P, V_T (zeroed by the launcher); bmap[2][n]
__global__ __launch_bounds__(256) void surf_border_kernel(Operand P, Operand T, int d0, int d1, int d2, int n, int cls,
                                                          unsigned char* __restrict__ bmap,
                                                          unsigned long long* __restrict__ cnt) {
    const unsigned u = blockIdx.x * 256u + threadIdx.x;
    int kp = 0, kt = 0;
    if (u < (unsigned)n) {
        const int i = (int)u;
        int i0, i1, i2;
        raster_decode(i, d1, d2, i0, i1, i2);
        kp = classify(P, i0, i1, i2, d0, d1, d2, cls);
        kt = classify(T, i0, i1, i2, d0, d1, d2, cls);
        bmap[i] = kp == 2;
        bmap[(size_t)n + i] = kt == 2;
    }
    const unsigned long long bp = __ballot(kp == 2), bt = __ballot(kt == 2), vp = __ballot(kp != 0), vt = __ballot(kt != 0);
    const int lane = threadIdx.x & 63;
    const unsigned long long mine = lane == 0 ? bp : lane == 1 ? bt : lane == 2 ? vp : vt;
    if (lane < 4 && mine) atomicAdd(cnt + lane, (unsigned long long)__popcll(mine));
}

// g[2][n]: one thread per line (i0, i1) of an operand
__global__ __launch_bounds__(256) void surf_scan2_kernel(const unsigned char* __restrict__ bmap, int lines, int d2, int n,
                                                         int* __restrict__ g) {
    const unsigned u = blockIdx.x * 256u + threadIdx.x;
    if (u >= (unsigned)lines) return;
    const size_t base = (size_t)blockIdx.y * n + (size_t)u * d2;
    const unsigned char* b = bmap + base;
    int* o = g + base;
    int last = -1;
    for (int i = 0; i < d2; ++i) {
        if (b[i]) last = i;
        o[i] = last >= 0 ? i - last : NONE;
    }
    int next = -1;
    for (int i = d2 - 1; i >= 0; --i) {
        if (b[i]) next = i;
        if (next >= 0) o[i] = min(o[i], next - i);
    }
}

// Lines of length L and element stride `stride`; line c of ncol starts at (c / inner) * outer + c % inner.
//   along d1: L = d1, stride = d2, inner = d2, outer = d1 * d2, ncol = d0 * d2
//   along d0: L = d0, stride = d1 * d2, inner = ncol = d1 * d2 (outer unused)
struct Lines {
    int L, stride, inner, outer, ncol, n;
    double sp;       // spacing along the line
    double sp_in;    // !LAST: spacing of the scanned dim (d2)
};

__host__ Lines lines_d1(int d0, int d1, int d2, int n, double sp1, double sp2) {
    return Lines{d1, d2, d2, d1 * d2, (int)((long)d0 * d2), n, sp1, sp2};
}
__host__ Lines lines_d0(int d0, int d1, int d2, int n, double sp0) { return Lines{d0, d1 * d2, d1 * d2, 0, d1 * d2, n, sp0, 0.0}; }

// The min-plus walk of one thread's R results first .. first + R - 1 of its line: best[r] = min over the candidates j < L of
// (sp * (first + r - j))^2 + load(j); load(j) = +inf: no candidate.  The workgroup walks the line in chunks of CH candidates
// in LDS (live: this thread's line exists); brute force, branch-free.
template <class Load>
__device__ __forceinline__ void minplus_walk(int L, double sp, bool live, int first, Load load, double (&best)[R]) {
    __shared__ double h[CH][COLS];
    const int col = threadIdx.x & 63, row = threadIdx.x >> 6;
    const double inf = __builtin_inf();
#pragma unroll
    for (int r = 0; r < R; ++r) best[r] = inf;
    for (int j0 = 0; j0 < L; j0 += CH) {
        __syncthreads();                         // the previous chunk is read to the end
#pragma unroll
        for (int k = 0; k < CH / ROWS; ++k) {
            const int jl = k * ROWS + row, j = j0 + jl;
            double v = inf;
            if (live && j < L) v = load(j);
            h[jl][col] = v;
        }
        __syncthreads();
        double dd = (double)(first - j0);        // result index - candidate index, exact
#pragma unroll 4
        for (int jl = 0; jl < CH; ++jl) {
            const double hv = h[jl][col];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const double t = sp * (dd + (double)r);
                best[r] = fmin(best[r], t * t + hv);
            }
            dd -= 1.0;
        }
    }
}

// {sum, max} over the 256 threads of the workgroup, folded pairwise in a fixed order; every thread gets the totals
__device__ __forceinline__ void fold_sum_max(double& sum, double& mx) {
    __shared__ double red[2][256];
    red[0][threadIdx.x] = sum;
    red[1][threadIdx.x] = mx;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            red[0][threadIdx.x] += red[0][threadIdx.x + s];
            red[1][threadIdx.x] = fmax(red[1][threadIdx.x], red[1][threadIdx.x + s]);
        }
        __syncthreads();
    }
    sum = red[0][0];
    mx = red[1][0];
}

// !LAST: f[op] from g[op].  LAST (blockIdx.y = op: 0 measures the border voxels of P against T, 1 the reverse):
// dist[op][i] = sqrt(min) at the border voxels of operand op against f[1 - op], -1 elsewhere; part[op][blockIdx.x] = {sum, max}
// KEYS (LAST only; aide_surface3d_scores_select): every distance is also appended to keys[op][kcnt[op]++] as its bit pattern,
// which orders like the non-negative double.  A wave takes the slots of the up to R * 64 distances of a chunk with one integer
// atomic (ballots, popcounts, lane prefix), so the order of the list depends on the schedule; the sum and the max do not.
template <bool LAST, bool KEYS = false>
__global__ __launch_bounds__(256) void surf_minplus_kernel(Lines q, const int* __restrict__ g, double* __restrict__ f,
                                                           const unsigned char* __restrict__ bmap,
                                                           double* __restrict__ dist, double* __restrict__ part,
                                                           unsigned long long* __restrict__ keys = nullptr,
                                                           unsigned* __restrict__ kcnt = nullptr) {
    const int op = blockIdx.y, col = threadIdx.x & 63, row = threadIdx.x >> 6;
    const long c = (long)blockIdx.x * COLS + col;
    const bool live = c < q.ncol;
    const int cc = live ? (int)c : 0;
    const size_t start = (size_t)(cc / q.inner) * q.outer + cc % q.inner;
    const size_t src = (size_t)(LAST ? 1 - op : op) * q.n + start, dst = (size_t)op * q.n + start;
    const double inf = __builtin_inf();
    double sum = 0.0, mx = 0.0;
    for (int o0 = 0; o0 < q.L; o0 += OC) {
        const int first = o0 + row * R;          // this thread's results: first .. first + R - 1
        double best[R];
        minplus_walk(q.L, q.sp, live, first, [&](int j) {
            if (LAST) return f[src + (size_t)j * q.stride];
            const int gi = g[src + (size_t)j * q.stride];
            if (gi == NONE) return inf;
            const double t = q.sp_in * (double)gi;
            return t * t;
        }, best);
        if (LAST) {
            double dk[R];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int i = first + r;
                double d = -1.0;
                if (live && i < q.L) {
                    const size_t at = dst + (size_t)i * q.stride;
                    if (bmap[at] && best[r] < inf) {
                        d = sqrt(best[r]);
                        sum += d;
                        mx = fmax(mx, d);
                    }
                    if (dist) dist[at] = d;
                }
                dk[r] = d;
            }
            if constexpr (KEYS) {                // whole waves arrive here: no thread has left the kernel
                unsigned long long has[R];
                unsigned total = 0;
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    has[r] = __ballot(dk[r] >= 0.0);
                    total += (unsigned)__popcll(has[r]);
                }
                if (total) {                     // wave-uniform
                    unsigned base = 0;
                    if (col == 0) base = atomicAdd(kcnt + op, total);
                    base = (unsigned)__builtin_amdgcn_readfirstlane((int)base);
                    const unsigned long long below = (1ull << col) - 1ull;
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const unsigned slot = base + (unsigned)__popcll(has[r] & below);
                        if (dk[r] >= 0.0 && slot < (unsigned)q.n)      // (at most n_op <= n distances exist)
                            keys[(size_t)op * q.n + slot] = (unsigned long long)__double_as_longlong(dk[r]);
                        base += (unsigned)__popcll(has[r]);
                    }
                }
            }
        } else {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int i = first + r;
                if (live && i < q.L) f[dst + (size_t)i * q.stride] = best[r];
            }
        }
    }
    if constexpr (LAST) {
        fold_sum_max(sum, mx);
        if (threadIdx.x == 0) {
            double* slot = part + 2 * ((size_t)op * gridDim.x + blockIdx.x);
            slot[0] = sum;
            slot[1] = mx;
        }
    }
}

// out[4], out[5] = S_PT, S_TP; out[6], out[7] = M_PT, M_TP from part[2][slots][2]: thread t adds the slots t, t + 256, ... in
// rising order, then the 256 partial sums fold pairwise
__global__ __launch_bounds__(256) void surf_finish_kernel(const double* __restrict__ part, int slots, double* __restrict__ out) {
    for (int op = 0; op < 2; ++op) {
        double sum = 0.0, mx = 0.0;
        for (int s = threadIdx.x; s < slots; s += 256) {
            const double* slot = part + 2 * ((size_t)op * slots + s);
            sum += slot[0];
            mx = fmax(mx, slot[1]);
        }
        __syncthreads();
        fold_sum_max(sum, mx);
        if (threadIdx.x == 0) {
            out[4 + op] = sum;
            out[6 + op] = mx;
        }
    }
}

// ---- exact selection over the key lists (aide_surface3d_scores_select) --------------------------------------------------------
// A target = (set, rank): set 0 = A (keys[0]), 1 = B (keys[1]), 2 = the multiset union; target index t = set * 8 + 2 * j + h for
// percentile j < nq, h = 0: rank lo, h = 1: rank hi.  MSD radix select, 8 passes of 8 bits: sel_hist counts, per target, the
// digits of the keys whose higher digits equal the target's prefix; sel_choose (one workgroup per target) walks the 256 bins,
// picks the digit that holds the rank, extends the prefix, reduces the rank to one inside that digit and clears the bins for
// the next pass.  After pass 7 the prefix is the key of that rank.  Equal keys share every digit: a run of ties is one bin.
constexpr int SEL_T = 24;          // targets: 3 sets x 4 percentiles x {lo, hi}
constexpr int SEL_WG = 512;        // workgroups per operand of sel_hist (grid-stride over the list)

struct SelState {
    unsigned long long prefix;     // the digits chosen so far, right-aligned
    unsigned long long rank;       // rank among the keys that carry the prefix
};

struct SelArgs {
    double q[4];
    unsigned long long tol[4];     // bit patterns of the tolerances
    int nq, nt;
};

// bins[d] += 1 for the active lanes of a wave.  The largest group of equal digits is the rule, not the exception (every key
// shares its exponent bits with most others; at unit spacing thousands of keys are equal), so the group of the first active
// lane goes as one add of its size; the others add one each.
__device__ __forceinline__ void sel_count(unsigned* bins, bool active, unsigned digit, int lane) {
    const unsigned long long m = __ballot(active);
    if (m) {
        const int lead = __ffsll((long long)m) - 1;
        const unsigned ld = (unsigned)__builtin_amdgcn_readlane((int)digit, lead);
        const unsigned long long grp = __ballot(active && digit == ld);
        if (lane == lead) atomicAdd(bins + ld, (unsigned)__popcll(grp));
        if (active && digit != ld) atomicAdd(bins + digit, 1u);
    }
}

// grid (SEL_WG, 2): blockIdx.y = the list.  PASS 0 also counts the keys <= tol[j] into out[8 + 2 * j + op].
template <int PASS>
__global__ __launch_bounds__(256) void sel_hist_kernel(SelArgs a, int n, const unsigned long long* __restrict__ keys,
                                                       const unsigned* __restrict__ kcnt, const SelState* __restrict__ st,
                                                       unsigned* __restrict__ hist, unsigned long long* __restrict__ out) {
    __shared__ unsigned h[SEL_T][256];
    __shared__ unsigned long long pre[SEL_T];
    const int op = blockIdx.y, lane = threadIdx.x & 63;
    const unsigned cnt = min(kcnt[op], (unsigned)n);
    if (blockIdx.x * 256u >= cnt) return;                                  // block-uniform: nothing of the list is mine
    const int nper = 2 * a.nq;                                             // targets per set
    for (int i = threadIdx.x; i < SEL_T * 256; i += 256) (&h[0][0])[i] = 0u;
    if (threadIdx.x < SEL_T) pre[threadIdx.x] = PASS ? st[threadIdx.x].prefix : 0ull;
    __syncthreads();
    constexpr int shift = 56 - 8 * PASS;
    const unsigned long long* list = keys + (size_t)op * n;
    unsigned within[4] = {0u, 0u, 0u, 0u};                                 // wave-uniform
    const unsigned rounds = (cnt + 255u) / 256u;                           // whole waves walk every round
    for (unsigned k = blockIdx.x; k < rounds; k += gridDim.x) {
        const unsigned i = k * 256u + threadIdx.x;
        const bool ok = i < cnt;
        const unsigned long long key = ok ? list[i] : 0ull;
        const unsigned digit = (unsigned)(key >> shift) & 255u;
        unsigned long long high = 0ull;                                    // the digits above this pass's
        if constexpr (PASS > 0) high = key >> (shift + 8);
        for (int s = op; s < 3; s += 2 - op) {                             // the sets this list belongs to: op and 2
            for (int j = 0; j < nper; ++j) {
                const int t = s * 8 + j;
                sel_count(h[t], ok && high == pre[t], digit, lane);
            }
        }
        if (PASS == 0) {
            for (int j = 0; j < a.nt; ++j) within[j] += (unsigned)__popcll(__ballot(ok && key <= a.tol[j]));
        }
    }
    __syncthreads();
    for (int s = op; s < 3; s += 2 - op) {
        for (int j = 0; j < nper; ++j) {
            const int t = s * 8 + j;
            const unsigned v = h[t][threadIdx.x];
            if (v) atomicAdd(hist + t * 256 + threadIdx.x, v);
        }
    }
    if (PASS == 0 && lane == 0) {
        for (int j = 0; j < a.nt; ++j)
            if (within[j]) atomicAdd(out + 8 + 2 * j + op, (unsigned long long)within[j]);
    }
}

// grid (SEL_T): one workgroup per target, thread d owns bin d.  PASS 0 derives the rank from n_P = out[0], n_T = out[1] and q
// (pos = (m - 1) * q / 100.0 left to right in fp64: a product and a quotient, nothing to contract) and writes lo; pass 7 writes
// the key.  A rank that no bin holds (a list shorter than its border count: include/aide_hip.h on overflow) takes digit 255.
template <int PASS>
__global__ __launch_bounds__(256) void sel_choose_kernel(SelArgs a, SelState* __restrict__ st, unsigned* __restrict__ hist,
                                                         unsigned long long* __restrict__ out) {
    __shared__ unsigned long long scan[256];
    __shared__ unsigned long long found[2];                                // digit, rank inside it
    const int t = blockIdx.x, s = t >> 3, j = (t & 7) >> 1, hi = t & 1, d = threadIdx.x;
    if (j >= a.nq) return;
    const long long n_p = (long long)out[0], n_t = (long long)out[1];
    const bool valid = n_p > 0 && n_t > 0;
    unsigned long long prefix = 0ull, rank = 0ull;
    if (PASS == 0) {
        if (valid) {
            const long long m = s == 0 ? n_p : s == 1 ? n_t : n_p + n_t;
            const double pos = (double)(m - 1) * a.q[j] / 100.0;
            const long long lo = (long long)floor(pos);
            rank = (unsigned long long)(hi ? (lo + 1 < m - 1 ? lo + 1 : m - 1) : lo);
            if (!hi && d == 0) out[16 + 3 * (s * 4 + j)] = (unsigned long long)lo;
        }
    } else {
        prefix = st[t].prefix;
        rank = st[t].rank;
    }
    const unsigned mine = hist[t * 256 + d];
    hist[t * 256 + d] = 0u;                                                // the next pass starts from cleared bins
    scan[d] = mine;
    if (d == 0) { found[0] = 255ull; found[1] = rank; }
    __syncthreads();
    for (int w = 1; w < 256; w <<= 1) {                                    // inclusive scan
        const unsigned long long add = d >= w ? scan[d - w] : 0ull;
        __syncthreads();
        scan[d] += add;
        __syncthreads();
    }
    const unsigned long long incl = scan[d], excl = incl - mine;
    if (excl <= rank && rank < incl) { found[0] = (unsigned long long)d; found[1] = rank - excl; }   // at most one thread
    __syncthreads();
    if (d == 0) {
        prefix = (prefix << 8) | found[0];
        st[t].prefix = prefix;
        st[t].rank = found[1];
        if (PASS == 7) out[16 + 3 * (s * 4 + j) + 1 + hi] = valid ? prefix : 0ull;
    }
}

// ---- the full distance transform of one volume (aide_edt3d) ---------------------------------------------------------------------
// Candidates are the voxels that are NOT foreground.  Launches: edt_bg (the candidate map as bytes in logical raster order; from
// here on no stride is read), surf_scan2 and surf_minplus<false> as above with one operand, edt_last.
__global__ __launch_bounds__(256) void edt_bg_kernel(Operand X, int d1, int d2, int n, int cls, unsigned char* __restrict__ bmap) {
    const unsigned u = blockIdx.x * 256u + threadIdx.x;
    if (u >= (unsigned)n) return;
    int i0, i1, i2;
    raster_decode((int)u, d1, d2, i0, i1, i2);
    bmap[u] = !fg_at(X, X.off(i0, i1, i2), cls);
}

// the walk of surf_minplus<true> along d0 on f of the same operand, evaluated at every voxel: dist = sqrt(min).  A candidate is
// its own nearest (min = 0, dist = 0 on the background); without any candidate every f is +inf and so is every dist.
__global__ __launch_bounds__(256) void edt_last_kernel(Lines q, const double* __restrict__ f, double* __restrict__ dist) {
    const int col = threadIdx.x & 63, row = threadIdx.x >> 6;
    const long c = (long)blockIdx.x * COLS + col;
    const bool live = c < q.ncol;
    const size_t start = live ? (size_t)c : 0;
    for (int o0 = 0; o0 < q.L; o0 += OC) {
        const int first = o0 + row * R;
        double best[R];
        minplus_walk(q.L, q.sp, live, first, [&](int j) { return f[start + (size_t)j * q.stride]; }, best);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int i = first + r;
            if (live && i < q.L) dist[start + (size_t)i * q.stride] = sqrt(best[r]);
        }
    }
}

// f [2][n] fp64 | g [2][n] int32 | bmap [2][n] bytes | slots [2][ceil(n / 64)][2] fp64 (d1 * d2 <= n: as many as any shape needs)
struct SurfaceWs {
    double* f;
    int* g;
    unsigned char* bmap;
    double* part;
    size_t bytes;
};
SurfaceWs surface_ws(void* ws, size_t n) {
    Carver c(ws);
    SurfaceWs w;
    w.f = c.take<double>(2 * n);
    w.g = c.take<int>(2 * n);
    w.bmap = c.take<unsigned char>(2 * n);
    w.part = c.take<double>(4 * ((n + COLS - 1) / COLS));
    w.bytes = c.used + 16;
    return w;
}

// f [n] fp64 | g [n] int32 | candidate map [n] bytes
struct EdtWs {
    double* f;
    int* g;
    unsigned char* bmap;
    size_t bytes;
};
EdtWs edt_ws(void* ws, size_t n) {
    Carver c(ws);
    EdtWs w;
    w.f = c.take<double>(n);
    w.g = c.take<int>(n);
    w.bmap = c.take<unsigned char>(n);
    w.bytes = c.used + 16;
    return w;
}

constexpr int SEL_WORDS = 52;      // out of aide_surface3d_scores_select, in words of 8 bytes
constexpr size_t SEL_CTRL_BYTES = 16 + SEL_T * sizeof(SelState) + SEL_T * 256 * sizeof(unsigned);

template <int PASS>
void sel_pass(const SelArgs& a, int n, const unsigned long long* keys, const unsigned* kcnt, SelState* state, unsigned* hist,
              unsigned long long* out, hipStream_t stream) {
    AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 0.0, sel_hist_kernel<PASS>, dim3(SEL_WG, 2), dim3(256), 0, stream, a, n, keys, kcnt,
                      (const SelState*)state, hist, out);
    AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 0.0, sel_choose_kernel<PASS>, dim3(SEL_T), dim3(256), 0, stream, a, state, hist, out);
}

// the launches of both entry points; sel = nullptr: aide_surface3d_scores
int surface_run(const void* p, int p_u8, int64_t p_s0, int64_t p_s1, int64_t p_s2, const void* t, int t_u8, int64_t t_s0,
                int64_t t_s1, int64_t t_s2, int64_t d0, int64_t d1, int64_t d2, double sp0, double sp1, double sp2, int cls,
                const SelArgs* sel, void* out, double* dist, void* ws, hipStream_t stream) {
    if (!dims_ok(d0, d1, d2) || !p || !t || !out || !ws || (reinterpret_cast<uintptr_t>(ws) & 15) != 0) return AIDE_ERR_ARG;
    if ((p_u8 != 0 && p_u8 != 1) || (t_u8 != 0 && t_u8 != 1)) return AIDE_ERR_ARG;
    const double sp[3] = {sp0, sp1, sp2};
    if (!spacing_ok(sp)) return AIDE_ERR_ARG;
    const int n = (int)(d0 * d1 * d2);
    const int plane = (int)(d1 * d2);
    const long cols1 = (long)d0 * d2, cols0 = plane;                        // lines along d1, along d0
    const long slots = (cols0 + COLS - 1) / COLS;
    hipError_t e = hipMemsetAsync(out, 0, (sel ? SEL_WORDS : 8) * sizeof(double), stream);
    if (e != hipSuccess) return (int)e;
    if (n == 0) return 0;
    const SurfaceWs w = surface_ws(ws, (size_t)n);
    double* f = w.f;
    int* g = w.g;
    unsigned char* bmap = w.bmap;
    double* part = w.part;
    const Operand P{p, (long)p_s0, (long)p_s1, (long)p_s2, p_u8}, T{t, (long)t_s0, (long)t_s1, (long)t_s2, t_u8};
    const unsigned nb = (unsigned)(((long)n + 255) / 256);
    const int lines = (int)(d0 * d1);
    const Lines a1 = lines_d1((int)d0, (int)d1, (int)d2, n, sp1, sp2), a0 = lines_d0((int)d0, (int)d1, (int)d2, n, sp0);
    const dim3 block(256);
    unsigned long long* keys = nullptr;
    unsigned* kcnt = nullptr;
    SelState* state = nullptr;
    unsigned* hist = nullptr;
    const double bytes_in = (double)n * ((p_u8 ? 1 : 8) + (t_u8 ? 1 : 8));
    AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, bytes_in + 2.0 * n, surf_border_kernel, dim3(nb), block, 0, stream, P, T, (int)d0, (int)d1,
                      (int)d2, n, cls, bmap, static_cast<unsigned long long*>(out));
    AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 10.0 * n, surf_scan2_kernel, dim3((unsigned)((lines + 255) / 256), 2), block, 0, stream,
                      (const unsigned char*)bmap, lines, (int)d2, n, g);
    AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 24.0 * n, surf_minplus_kernel<false>, dim3((unsigned)((cols1 + COLS - 1) / COLS), 2), block,
                      0, stream, a1, (const int*)g, f, (const unsigned char*)bmap, (double*)nullptr, (double*)nullptr,
                      (unsigned long long*)nullptr, (unsigned*)nullptr);
    if (!sel) {
        AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, (dist ? 34.0 : 18.0) * n, surf_minplus_kernel<true>, dim3((unsigned)slots, 2), block, 0,
                          stream, a0, (const int*)g, f, (const unsigned char*)bmap, dist, part, (unsigned long long*)nullptr,
                          (unsigned*)nullptr);
    } else {
        char* w2 = static_cast<char*>(ws) + w.bytes;
        keys = reinterpret_cast<unsigned long long*>(w2);
        w2 += 2 * (size_t)n * sizeof(unsigned long long);
        kcnt = reinterpret_cast<unsigned*>(w2);
        state = reinterpret_cast<SelState*>(w2 + 16);
        hist = reinterpret_cast<unsigned*>(w2 + 16 + SEL_T * sizeof(SelState));
        e = hipMemsetAsync(kcnt, 0, SEL_CTRL_BYTES, stream);
        if (e != hipSuccess) return (int)e;
        AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, (dist ? 34.0 : 18.0) * n, (surf_minplus_kernel<true, true>), dim3((unsigned)slots, 2),
                          block, 0, stream, a0, (const int*)g, f, (const unsigned char*)bmap, dist, part, keys, kcnt);
    }
    AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 0.0, surf_finish_kernel, dim3(1), block, 0, stream, (const double*)part, (int)slots,
                      static_cast<double*>(out));
    if (sel) {
        unsigned long long* o = static_cast<unsigned long long*>(out);
        sel_pass<0>(*sel, n, keys, kcnt, state, hist, o, stream);
        sel_pass<1>(*sel, n, keys, kcnt, state, hist, o, stream);
        sel_pass<2>(*sel, n, keys, kcnt, state, hist, o, stream);
        sel_pass<3>(*sel, n, keys, kcnt, state, hist, o, stream);
        sel_pass<4>(*sel, n, keys, kcnt, state, hist, o, stream);
        sel_pass<5>(*sel, n, keys, kcnt, state, hist, o, stream);
        sel_pass<6>(*sel, n, keys, kcnt, state, hist, o, stream);
        sel_pass<7>(*sel, n, keys, kcnt, state, hist, o, stream);
    }
    return aide_launch_status();
}

}  // namespace

extern "C" {

size_t aide_surface3d_ws_bytes(int64_t nvox) {
    if (nvox < 0 || nvox > INT32_MAX) return 0;
    return surface_ws(nullptr, (size_t)nvox).bytes;
}

int aide_surface3d_scores(const void* p, int p_u8, int64_t p_s0, int64_t p_s1, int64_t p_s2, const void* t, int t_u8,
                          int64_t t_s0, int64_t t_s1, int64_t t_s2, int64_t d0, int64_t d1, int64_t d2, double sp0, double sp1,
                          double sp2, int cls, void* out, double* dist, void* ws, hipStream_t stream) {
    return surface_run(p, p_u8, p_s0, p_s1, p_s2, t, t_u8, t_s0, t_s1, t_s2, d0, d1, d2, sp0, sp1, sp2, cls, nullptr, out, dist, ws,
                       stream);
}

// the workspace of aide_surface3d_scores | keys [2][n] uint64 | control: kcnt [2] uint32 (+ pad), state [24], bins [24][256]
size_t aide_surface3d_select_ws_bytes(int64_t nvox) {
    if (nvox < 0 || nvox > INT32_MAX) return 0;
    return aide_surface3d_ws_bytes(nvox) + 2 * (size_t)nvox * sizeof(unsigned long long) + SEL_CTRL_BYTES;
}

int aide_surface3d_scores_select(const void* p, int p_u8, int64_t p_s0, int64_t p_s1, int64_t p_s2, const void* t, int t_u8,
                                 int64_t t_s0, int64_t t_s1, int64_t t_s2, int64_t d0, int64_t d1, int64_t d2, double sp0,
                                 double sp1, double sp2, int cls, const double* q, int nq, const double* tol, int nt, void* out,
                                 double* dist, void* ws, hipStream_t stream) {
    if (nq < 0 || nq > 4 || nt < 0 || nt > 4 || (nq && !q) || (nt && !tol)) return AIDE_ERR_ARG;
    SelArgs a;
    a.nq = nq;
    a.nt = nt;
    for (int j = 0; j < 4; ++j) {
        a.q[j] = 0.0;
        a.tol[j] = 0ull;
    }
    for (int j = 0; j < nq; ++j) {
        if (!std::isfinite(q[j]) || q[j] < 0.0 || q[j] > 100.0) return AIDE_ERR_ARG;
        a.q[j] = q[j];
    }
    for (int j = 0; j < nt; ++j) {
        if (!std::isfinite(tol[j]) || tol[j] < 0.0) return AIDE_ERR_ARG;
        const double v = tol[j] + 0.0;                                      // -0.0 -> +0.0: the bits must order like the value
        memcpy(&a.tol[j], &v, sizeof v);
    }
    return surface_run(p, p_u8, p_s0, p_s1, p_s2, t, t_u8, t_s0, t_s1, t_s2, d0, d1, d2, sp0, sp1, sp2, cls, &a, out, dist, ws,
                       stream);
}

size_t aide_edt3d_ws_bytes(int64_t nvox) {
    if (nvox < 0 || nvox > INT32_MAX) return 0;
    return edt_ws(nullptr, (size_t)nvox).bytes;
}

int aide_edt3d(const void* v, int v_u8, int64_t d0, int64_t d1, int64_t d2, int64_t s0, int64_t s1, int64_t s2, int cls,
               const double* spacing, double* dist, void* ws, hipStream_t stream) {
    if (!dims_ok(d0, d1, d2) || !spacing || (v_u8 != 0 && v_u8 != 1)) return AIDE_ERR_ARG;
    if (!spacing_ok(spacing)) return AIDE_ERR_ARG;
    const int n = (int)(d0 * d1 * d2);
    if (n == 0) return 0;
    if (!v || !dist || !ws || (reinterpret_cast<uintptr_t>(ws) & 15) != 0 || (reinterpret_cast<uintptr_t>(dist) & 7) != 0 ||
        (!v_u8 && (reinterpret_cast<uintptr_t>(v) & 7) != 0))
        return AIDE_ERR_ARG;
    const int plane = (int)(d1 * d2), lines = (int)(d0 * d1);
    const long cols1 = (long)d0 * d2;
    const EdtWs w = edt_ws(ws, (size_t)n);
    const Operand X{v, (long)s0, (long)s1, (long)s2, v_u8};
    const Lines a1 = lines_d1((int)d0, (int)d1, (int)d2, n, spacing[1], spacing[2]),
                a0 = lines_d0((int)d0, (int)d1, (int)d2, n, spacing[0]);
    const dim3 block(256);
    AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, (double)n * (v_u8 ? 2 : 9), edt_bg_kernel, dim3((unsigned)(((long)n + 255) / 256)), block, 0,
                      stream, X, (int)d1, (int)d2, n, cls, w.bmap);
    AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 5.0 * n, surf_scan2_kernel, dim3((unsigned)((lines + 255) / 256), 1), block, 0, stream,
                      (const unsigned char*)w.bmap, lines, (int)d2, n, w.g);
    AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 12.0 * n, surf_minplus_kernel<false>, dim3((unsigned)((cols1 + COLS - 1) / COLS), 1), block,
                      0, stream, a1, (const int*)w.g, w.f, (const unsigned char*)nullptr, (double*)nullptr, (double*)nullptr,
                      (unsigned long long*)nullptr, (unsigned*)nullptr);
    AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 16.0 * n, edt_last_kernel, dim3((unsigned)((plane + COLS - 1) / COLS)), block, 0, stream, a0,
                      (const double*)w.f, dist);
    return aide_launch_status();
}

}  // extern "C"
