// Per-case evaluation on the device: the largest 3-D connected component of a label volume and the confusion sums of a
// predicted volume against its target (include/aide_hip.h "per-case evaluation").
//
// Largest component: union-find over the logical raster index i = (i0 * D1 + i1) * D2 + i2 of the foreground voxels
// (V != 0; face neighbours of EQUAL value are connected).  The root of a set is always its smallest index, so it IS the
// component's first voxel in raster order.  Invariant: parent[i] <= i, and after the launch that initialises it every
// global write to `parent` is an atomicMin -- parents only decrease, so every find and union loop ends, and no workgroup
// ever waits for another (no spin, no co-residency assumption).  Launches:
//   1 lcc_local   one workgroup per 4 x 16 x 16 tile: union-find in LDS; parent[i] = first voxel of i's blob inside the
//                 tile (-1 for background), area[i] = that blob's voxel count at its first voxel, 0 elsewhere
//   2 lcc_border  per tile, face-adjacent equal-valued pairs across its three lower faces joined with atomicMin; parent
//                 words other workgroups write are read with agent-scope relaxed atomic loads (no stale L1 / L2 line)
//   3 lcc_count   every tile-blob root that is no longer a root adds its area to its set's root (wave-aggregated atomics)
//   4 lcc_select  key = (area << 32) | (0x7fffffff - root), block max, one atomicMax per block; flags whether any root
//                 (hence any voxel) holds a positive value
//   5 lcc_write   out[i] = 1 where find(i) is the chosen root (nothing when no voxel is positive: the reference's
//                 `if mask.max() > 0`)
// Everything is integer and the result does not depend on the schedule.
//
// Batched form (aide_keep_largest_cc3d_batched, aide_case_confusion_batched): the label maps of K ragged cases concatenated
// as [S_total][H][W] with a device table slice_start[K + 1].  Case k's logical volume is [H][W][S_k]; its voxel (h, w, s) is
// node base_k + (h * W + w) * S_k + s with base_k = slice_start[k] * H * W, so a case owns a contiguous range of nodes whose
// order is its own raster order: the same invariants, the same tie rule, and a union never leaves the range because a tile
// never leaves its case.  Every launch has the grid (chunks of the plane, K): blockIdx.y is the case, the block walks the
// case's slices, and the number of launches is the per-case form's five whatever K is.
//
// Per-class form (aide_keep_largest_cc3d_classes[_batched]): blobs of different values are separate sets already, so launches
// 1 - 3 are shared as they are and only select and write differ: one key per class value 1 .. C - 1 (the value read at the
// root), out[i] = the voxel's own class where its root is that class's winner.  The 3 C control words per volume (keys, root
// counts, area sums) are cleared by one memset in front of launch 1: five launches and one memset whatever C and K are.
#include "common.h"

namespace {

constexpr int TX = 16, TY = 16, TZ = 4, TILE = TX * TY * TZ;   // tile of logical (i0, i1, i2) = (z, y, x)

struct Vol {
    const long long* v;
    long s0, s1, s2;   // element strides of the logical dims
    int d0, d1, d2;
    int tx, ty;        // tiles along i2, i1
};

__device__ __forceinline__ int ld_agent(const int* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// root of x with path splitting: every node passed points on to its grandparent (atomicMin: only lowers, and the
// grandparent is an ancestor in the same set)
__device__ int find_split(int* parent, int x) {
    int q = ld_agent(parent + x);
    while (q != x) {
        const int qq = ld_agent(parent + q);
        if (qq != q) atomicMin(parent + x, qq);
        x = q;
        q = qq;
    }
    return x;
}

// join the sets of a and b: link the larger root under the smaller.  If the atomicMin finds that the larger root was
// linked meanwhile (old != b), its old parent is carried on as b: the link it had is preserved through the next round
__device__ void unite(int* parent, int a, int b) {
    for (;;) {
        a = find_split(parent, a);
        b = find_split(parent, b);
        if (a == b) return;
        if (a > b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(parent + b, a);
        if (old == b) return;
        b = old;
    }
}

__device__ __forceinline__ int lds_find(volatile int* lp, int x) {
    int q = lp[x];
    while (q != x) { x = q; q = lp[x]; }
    return x;
}

__device__ __forceinline__ void lds_unite(int* lp, int a, int b) {
    volatile int* vp = lp;
    for (;;) {
        a = lds_find(vp, a);
        b = lds_find(vp, b);
        if (a == b) return;
        if (a > b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(lp + b, a);
        if (old == b) return;
        b = old;
    }
}

__device__ __forceinline__ void tile_origin(const Vol& g, int tile, int& z0, int& y0, int& x0) {
    const int tyx = g.tx * g.ty;
    const int tz = tile / tyx, r = tile - tz * tyx, ty = r / g.tx;
    z0 = tz * TZ; y0 = ty * TY; x0 = (r - ty * g.tx) * TX;
}

// thread t owns (y, x) = (t / 16, t % 16) of the tile at z = 0 .. 3: local index e = z * 256 + t
__global__ __launch_bounds__(256) void lcc_local_kernel(Vol g, long tiles, int* __restrict__ parent,
                                                        int* __restrict__ area, unsigned long long* __restrict__ ctrl) {
    __shared__ long long val[TILE];
    __shared__ int lp[TILE];
    __shared__ int cnt[TILE];
    const int t = threadIdx.x, y = t >> 4, x = t & 15;
    const int plane = g.d1 * g.d2;
    if (blockIdx.x == 0 && t == 0) { ctrl[0] = 0ull; ctrl[1] = 0ull; }
    for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        int z0, y0, x0;
        tile_origin(g, (int)tile, z0, y0, x0);
        const bool in_yx = y0 + y < g.d1 && x0 + x < g.d2;
        __syncthreads();                          // the previous tile's LDS is read to the end
#pragma unroll
        for (int z = 0; z < TZ; ++z) {
            const int e = z * 256 + t;
            long long v = 0;
            if (in_yx && z0 + z < g.d0) v = g.v[(long)(z0 + z) * g.s0 + (long)(y0 + y) * g.s1 + (long)(x0 + x) * g.s2];
            val[e] = v;
            lp[e] = v != 0 ? e : -1;
            cnt[e] = 0;
        }
        __syncthreads();
#pragma unroll
        for (int z = 0; z < TZ; ++z) {
            const int e = z * 256 + t;
            const long long v = val[e];
            if (v == 0) continue;                 // (out-of-volume voxels read as background)
            if (x > 0 && val[e - 1] == v) lds_unite(lp, e - 1, e);
            if (y > 0 && val[e - TX] == v) lds_unite(lp, e - TX, e);
            if (z > 0 && val[e - TX * TY] == v) lds_unite(lp, e - TX * TY, e);
        }
        __syncthreads();
        int root[TZ];
#pragma unroll
        for (int z = 0; z < TZ; ++z) {
            const int e = z * 256 + t;
            root[z] = val[e] != 0 ? lds_find(lp, e) : -1;
            if (root[z] >= 0) atomicAdd(&cnt[root[z]], 1);
        }
        __syncthreads();
        if (!in_yx) continue;
#pragma unroll
        for (int z = 0; z < TZ; ++z) {
            if (z0 + z >= g.d0) break;
            const int e = z * 256 + t;
            const int gi = (z0 + z) * plane + (y0 + y) * g.d2 + x0 + x;
            int gr = -1;
            if (root[z] >= 0) {   // local order (z, y, x) is raster order: the tile-blob's first voxel has the lowest index
                const int r = root[z], rz = r >> 8, ry = (r >> 4) & 15, rx = r & 15;
                gr = (z0 + rz) * plane + (y0 + ry) * g.d2 + x0 + rx;
            }
            parent[gi] = gr;
            area[gi] = cnt[e];
        }
    }
}

// the three lower faces of a tile: x face (TZ x TY pairs), y face (TZ x TX), z face (TY x TX)
__global__ __launch_bounds__(256) void lcc_border_kernel(Vol g, long tiles, int* __restrict__ parent) {
    const int plane = g.d1 * g.d2;
    for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        int z0, y0, x0;
        tile_origin(g, (int)tile, z0, y0, x0);
        for (int k = threadIdx.x; k < TZ * TY + TZ * TX + TY * TX; k += 256) {
            int z, y, x, dz = 0, dy = 0, dx = 0;
            if (k < TZ * TY) {
                if (x0 == 0) continue;
                z = k / TY; y = k % TY; x = 0; dx = 1;
            } else if (k < TZ * TY + TZ * TX) {
                if (y0 == 0) continue;
                const int j = k - TZ * TY;
                z = j / TX; x = j % TX; y = 0; dy = 1;
            } else {
                if (z0 == 0) continue;
                const int j = k - TZ * TY - TZ * TX;
                y = j / TX; x = j % TX; z = 0; dz = 1;
            }
            const int a0 = z0 + z, a1 = y0 + y, a2 = x0 + x;
            if (a0 >= g.d0 || a1 >= g.d1 || a2 >= g.d2) continue;
            const long off = (long)a0 * g.s0 + (long)a1 * g.s1 + (long)a2 * g.s2;
            const long long v = g.v[off];
            if (v == 0) continue;
            const long long w = g.v[off - dz * g.s0 - dy * g.s1 - dx * g.s2];
            if (w != v) continue;
            const int gi = a0 * plane + a1 * g.d2 + a2;
            unite(parent, gi - dz * plane - dy * g.d2 - dx, gi);
        }
    }
}

__device__ __forceinline__ int find_plain(const int* parent, int x) {
    int q = parent[x];
    while (q != x) { x = q; q = parent[x]; }
    return x;
}

// tile-blob roots that were joined to another set add their area to its root.  Lanes of one wave that add to the same
// root are summed first: one atomic per (wave, root)
__global__ __launch_bounds__(256) void lcc_count_kernel(int* __restrict__ parent, int* __restrict__ area, int n) {
    const int i = (int)min(blockIdx.x * 256u + threadIdx.x, (unsigned)n);
    int a = 0, r = -1;
    if (i < n) {
        a = area[i];
        if (a > 0) {
            r = find_plain(parent, i);
            if (r != i) atomicMin(parent + i, r);
            else a = 0;
        }
    }
    unsigned long long pending = __ballot(a > 0);
    while (pending) {
        const int leader = __ffsll((long long)pending) - 1;
        const int rl = __shfl(r, leader);
        const bool mine = a > 0 && r == rl;
        int s = mine ? a : 0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if ((int)(threadIdx.x & 63) == leader) atomicAdd(area + rl, s);
        if (mine) a = 0;
        pending &= ~__ballot(mine);
    }
}

__device__ __forceinline__ unsigned long long umax64(unsigned long long a, unsigned long long b) { return a > b ? a : b; }

// ctrl[0] = max key over the roots, ctrl[1] = 1 when some root (so some voxel) holds a positive value
__global__ __launch_bounds__(256) void lcc_select_kernel(Vol g, const int* __restrict__ parent, const int* __restrict__ area,
                                                         int n, unsigned long long* __restrict__ ctrl) {
    __shared__ unsigned long long sk[4];
    __shared__ int sp[4];
    unsigned long long key = 0;
    int pos = 0;
    const int plane = g.d1 * g.d2;
    for (unsigned u = blockIdx.x * 256u + threadIdx.x; u < (unsigned)n; u += gridDim.x * 256u) {
        const int i = (int)u;
        if (parent[i] != i) continue;
        key = umax64(key, ((unsigned long long)(unsigned)area[i] << 32) | (unsigned)(0x7fffffff - i));
        if (!pos) {
            const int i0 = i / plane, r = i - i0 * plane, i1 = r / g.d2, i2 = r - i1 * g.d2;
            pos = g.v[(long)i0 * g.s0 + (long)i1 * g.s1 + (long)i2 * g.s2] > 0;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        key = umax64(key, __shfl_xor(key, o));
        pos |= __shfl_xor(pos, o);
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) { sk[wid] = key; sp[wid] = pos; }
    __syncthreads();
    if (threadIdx.x == 0) {
        key = umax64(umax64(sk[0], sk[1]), umax64(sk[2], sk[3]));
        pos = sp[0] | sp[1] | sp[2] | sp[3];
        if (key) atomicMax(ctrl, key);
        if (pos) atomicMax(ctrl + 1, 1ull);
    }
}

__global__ __launch_bounds__(256) void lcc_write_kernel(const int* __restrict__ parent, int n,
                                                        const unsigned long long* __restrict__ ctrl,
                                                        unsigned char* __restrict__ out) {
    const unsigned u = blockIdx.x * 256u + threadIdx.x;
    if (u >= (unsigned)n) return;
    const int i = (int)u;
    const unsigned long long key = ctrl[0];
    const int best = ctrl[1] ? 0x7fffffff - (int)(unsigned)(key & 0xffffffffull) : -1;
    const int p = parent[i];
    out[i] = (best >= 0 && p >= 0 && find_plain(parent, p) == best) ? 1 : 0;
}

// ---- per-class form of select and write: one winner per class value 1 .. C - 1 (C <= MAXC) ----
// Control words of a volume (case k of K; K = 1, k = 0 for the single volume), all cleared by one memset before launch 1:
// ctrl[k * C + c] = max key over the roots of class c, ctrl[(K + k) * C + c] = number of roots (components) of class c,
// ctrl[(2 K + k) * C + c] = sum of their areas (voxels of class c).  Word c = 0 of every group stays zero.
constexpr int MAXC = 8;

// 1 .. C - 1, or 0 for a value that belongs to no class (0, negative, >= C)
__device__ __forceinline__ int class_of(long long v, int C) { return (v > 0 && v < C) ? (int)v : 0; }

struct ClassAcc {                                 // a thread's running key, root count and area sum per class: registers
    unsigned long long key[MAXC - 1];
    unsigned cnt[MAXC - 1], vox[MAXC - 1];        // a sum of areas of distinct roots never exceeds the voxel count < 2^31
};

template <bool STATS>
__device__ __forceinline__ void class_add(ClassAcc& a, int c, int i, int ar) {
    const unsigned long long key = ((unsigned long long)(unsigned)ar << 32) | (unsigned)(0x7fffffff - i);
#pragma unroll
    for (int j = 0; j < MAXC - 1; ++j)
        if (c == j + 1) {
            a.key[j] = umax64(a.key[j], key);
            if (STATS) { a.cnt[j] += 1u; a.vox[j] += (unsigned)ar; }
        }
}

// wave reduce with __shfl_xor, block reduce through LDS, then thread j commits class j + 1: at most one atomicMax (and, with
// STATS, two integer atomicAdd) per (block, class), none where the block saw no root of the class
template <bool STATS>
__device__ __forceinline__ void class_commit(ClassAcc& a, int C, unsigned long long* __restrict__ keys,
                                             unsigned long long* __restrict__ cnts, unsigned long long* __restrict__ voxs) {
    __shared__ unsigned long long sk[4][MAXC - 1];
    __shared__ unsigned sc[4][MAXC - 1], sv[4][MAXC - 1];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < MAXC - 1; ++j) {
        if (j >= C - 1) break;                    // uniform
        unsigned long long key = a.key[j];
        unsigned cn = a.cnt[j], vx = a.vox[j];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            key = umax64(key, __shfl_xor(key, o));
            if (STATS) { cn += __shfl_xor(cn, o); vx += __shfl_xor(vx, o); }
        }
        if (lane == 0) {
            sk[wid][j] = key;
            if (STATS) { sc[wid][j] = cn; sv[wid][j] = vx; }
        }
    }
    __syncthreads();
    const int j = threadIdx.x;
    if (j < C - 1) {
        const unsigned long long key = umax64(umax64(sk[0][j], sk[1][j]), umax64(sk[2][j], sk[3][j]));
        if (key) atomicMax(keys + j + 1, key);
        if (STATS) {
            const unsigned cn = sc[0][j] + sc[1][j] + sc[2][j] + sc[3][j], vx = sv[0][j] + sv[1][j] + sv[2][j] + sv[3][j];
            if (cn) atomicAdd(cnts + j + 1, (unsigned long long)cn);
            if (vx) atomicAdd(voxs + j + 1, (unsigned long long)vx);
        }
    }
}

// best[c] = the chosen root of class c, -1 where the class has no root (key 0) and for c = 0; then a block barrier
__device__ __forceinline__ void class_best(const unsigned long long* __restrict__ keys, int C, int* best) {
    const int c = threadIdx.x;
    if (c < MAXC) {
        const unsigned long long key = (c >= 1 && c < C) ? keys[c] : 0ull;
        best[c] = key ? 0x7fffffff - (int)(unsigned)(key & 0xffffffffull) : -1;
    }
    __syncthreads();
}

// stats[c][0..2] = components, voxels, voxels of the kept component of class c; row 0 zeros (threads 0 .. C - 1 of one block)
__device__ __forceinline__ void class_stats(const unsigned long long* __restrict__ keys,
                                            const unsigned long long* __restrict__ cnts,
                                            const unsigned long long* __restrict__ voxs, int C, long long* __restrict__ stats) {
    const int c = threadIdx.x;
    if (c >= C) return;
    stats[3 * c] = c ? (long long)cnts[c] : 0;
    stats[3 * c + 1] = c ? (long long)voxs[c] : 0;
    stats[3 * c + 2] = c ? (long long)(keys[c] >> 32) : 0;
}

// the value is read at the roots only, as in lcc_select_kernel
template <bool STATS>
__global__ __launch_bounds__(256) void lcc_select_classes_kernel(Vol g, const int* __restrict__ parent,
                                                                 const int* __restrict__ area, int n, int C,
                                                                 unsigned long long* __restrict__ ctrl) {
    ClassAcc a = {};
    const int plane = g.d1 * g.d2;
    for (unsigned u = blockIdx.x * 256u + threadIdx.x; u < (unsigned)n; u += gridDim.x * 256u) {
        const int i = (int)u;
        if (parent[i] != i) continue;
        const int i0 = i / plane, r = i - i0 * plane, i1 = r / g.d2, i2 = r - i1 * g.d2;
        const int c = class_of(g.v[(long)i0 * g.s0 + (long)i1 * g.s1 + (long)i2 * g.s2], C);
        if (c) class_add<STATS>(a, c, i, area[i]);
    }
    class_commit<STATS>(a, C, ctrl, ctrl + C, ctrl + 2 * C);
}

// out[i] = the voxel's own value v where v is a class and find(i) is the chosen root of that class, 0 elsewhere
__global__ __launch_bounds__(256) void lcc_write_classes_kernel(Vol g, const int* __restrict__ parent, int n, int C,
                                                                const unsigned long long* __restrict__ ctrl,
                                                                unsigned char* __restrict__ out, long long* __restrict__ stats) {
    __shared__ int best[MAXC];
    class_best(ctrl, C, best);
    if (stats && blockIdx.x == 0) class_stats(ctrl, ctrl + C, ctrl + 2 * C, C, stats);
    const unsigned u = blockIdx.x * 256u + threadIdx.x;
    if (u >= (unsigned)n) return;
    const int i = (int)u, p = parent[i];
    int o = 0;
    if (p >= 0) {
        const int plane = g.d1 * g.d2;
        const int i0 = i / plane, r = i - i0 * plane, i1 = r / g.d2, i2 = r - i1 * g.d2;
        const int c = class_of(g.v[(long)i0 * g.s0 + (long)i1 * g.s1 + (long)i2 * g.s2], C);
        if (c && best[c] >= 0 && find_plain(parent, p) == best[c]) o = c;
    }
    out[i] = (unsigned char)o;
}

// ---- confusion sums: out[0..3] = N, sum P*T, sum P, sum T (int64, order-independent atomics) ----
struct Operand {
    const void* p;
    long s0, s1, s2;
};

template <typename TP, typename TT>
__global__ __launch_bounds__(256) void confusion_kernel(Operand P, Operand T, int d1, int d2, int n,
                                                        long long* __restrict__ out) {
    __shared__ long long sm[3][4];
    const TP* pp = static_cast<const TP*>(P.p);
    const TT* tp = static_cast<const TT*>(T.p);
    const int plane = d1 * d2;
    long long spt = 0, sp = 0, st = 0;
    for (unsigned u = blockIdx.x * 256u + threadIdx.x; u < (unsigned)n; u += gridDim.x * 256u) {
        const int i = (int)u, i0 = i / plane, r = i - i0 * plane, i1 = r / d2, i2 = r - i1 * d2;
        const long long a = (long long)pp[(long)i0 * P.s0 + (long)i1 * P.s1 + (long)i2 * P.s2];
        const long long b = (long long)tp[(long)i0 * T.s0 + (long)i1 * T.s1 + (long)i2 * T.s2];
        spt += a * b; sp += a; st += b;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        spt += __shfl_xor(spt, o);
        sp += __shfl_xor(sp, o);
        st += __shfl_xor(st, o);
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) { sm[0][wid] = spt; sm[1][wid] = sp; sm[2][wid] = st; }
    __syncthreads();
    if (threadIdx.x < 3) {
        const long long s = sm[threadIdx.x][0] + sm[threadIdx.x][1] + sm[threadIdx.x][2] + sm[threadIdx.x][3];
        atomicAdd(reinterpret_cast<unsigned long long*>(out + 1 + threadIdx.x), (unsigned long long)s);
    }
    if (blockIdx.x == 0 && threadIdx.x == 3) atomicAdd(reinterpret_cast<unsigned long long*>(out), (unsigned long long)n);
}

bool dims_ok(int64_t d0, int64_t d1, int64_t d2) {
    if (d0 < 0 || d1 < 0 || d2 < 0) return false;
    if (d0 == 0 || d1 == 0 || d2 == 0) return true;
    return d0 <= INT32_MAX && d1 <= INT32_MAX && d2 <= INT32_MAX && d1 * d2 <= INT32_MAX && d0 * (d1 * d2) <= INT32_MAX;
}


// ---- batched over K ragged cases -------------------------------------------------------------------------------------
struct Cases {
    const long long* v;       // [S_total][H][W], contiguous
    const long long* start;   // [K + 1] first slice of every case (device)
    int S_total, H, W;
    int tw;                   // 16-wide tiles along w
};

// slices [s0, s0 + ns) of case k; a table entry outside [0, S_total] or below its predecessor is clamped, so that no
// address derived from it leaves the buffers
__device__ __forceinline__ void case_range(const long long* start, int k, int S_total, int& s0, int& ns) {
    long long a = start[k], b = start[k + 1];
    a = a < 0 ? 0 : (a > S_total ? S_total : a);
    b = b < a ? a : (b > S_total ? S_total : b);
    s0 = (int)a;
    ns = (int)(b - a);
}

// a 16 x 16 (h, w) tile of the plane per block, 4 slices at a time: thread t owns (h, w) = (t / 16, t % 16), local index
// e = t * 4 + z -- (h, w, s) order, the raster order of the case
__global__ __launch_bounds__(256) void lccb_local_kernel(Cases g, int* __restrict__ parent, int* __restrict__ area,
                                                         unsigned long long* __restrict__ ctrl) {
    __shared__ long long val[TILE];
    __shared__ int lp[TILE];
    __shared__ int cnt[TILE];
    const int k = blockIdx.y, t = threadIdx.x, hl = t >> 4, wl = t & 15;
    if (blockIdx.x == 0 && t == 0) { ctrl[2 * k] = 0ull; ctrl[2 * k + 1] = 0ull; }
    int s0, ns;
    case_range(g.start, k, g.S_total, s0, ns);
    const int h = (int)(blockIdx.x / g.tw) * 16 + hl, w = (int)(blockIdx.x % g.tw) * 16 + wl;
    const bool in_hw = h < g.H && w < g.W;
    const long hw = (long)g.H * g.W;
    const int base = (int)(s0 * hw), col = in_hw ? (h * g.W + w) * ns : 0;
    for (int sc = 0; sc < ns; sc += TZ) {
        __syncthreads();                          // the previous chunk's LDS is read to the end
#pragma unroll
        for (int z = 0; z < TZ; ++z) {
            const int e = t * TZ + z;
            long long v = 0;
            if (in_hw && sc + z < ns) v = g.v[(long)(s0 + sc + z) * hw + (long)h * g.W + w];
            val[e] = v;
            lp[e] = v != 0 ? e : -1;
            cnt[e] = 0;
        }
        __syncthreads();
#pragma unroll
        for (int z = 0; z < TZ; ++z) {
            const int e = t * TZ + z;
            const long long v = val[e];
            if (v == 0) continue;
            if (z > 0 && val[e - 1] == v) lds_unite(lp, e - 1, e);
            if (wl > 0 && val[e - TZ] == v) lds_unite(lp, e - TZ, e);
            if (hl > 0 && val[e - 16 * TZ] == v) lds_unite(lp, e - 16 * TZ, e);
        }
        __syncthreads();
        int root[TZ];
#pragma unroll
        for (int z = 0; z < TZ; ++z) {
            const int e = t * TZ + z;
            root[z] = val[e] != 0 ? lds_find(lp, e) : -1;
            if (root[z] >= 0) atomicAdd(&cnt[root[z]], 1);
        }
        __syncthreads();
        if (in_hw) {
#pragma unroll
            for (int z = 0; z < TZ; ++z) {
                if (sc + z >= ns) break;
                const int e = t * TZ + z;
                int gr = -1;
                if (root[z] >= 0) {               // the lowest local index of the tile-blob is its lowest node
                    const int r = root[z], rt = r / TZ, rh = rt >> 4, rw = rt & 15;
                    gr = base + ((h - hl + rh) * g.W + (w - wl + rw)) * ns + sc + (r - rt * TZ);
                }
                parent[base + col + sc + z] = gr;
                area[base + col + sc + z] = cnt[e];
            }
        }
    }
}

// lower faces of every 16 x 16 x 4 chunk: w face (4 x 16 pairs), h face (4 x 16), s face (16 x 16)
__global__ __launch_bounds__(256) void lccb_border_kernel(Cases g, int* __restrict__ parent) {
    const int k = blockIdx.y;
    int s0, ns;
    case_range(g.start, k, g.S_total, s0, ns);
    const int h0 = (int)(blockIdx.x / g.tw) * 16, w0 = (int)(blockIdx.x % g.tw) * 16;
    const long hw = (long)g.H * g.W;
    const int base = (int)(s0 * hw);
    for (int sc = 0; sc < ns; sc += TZ) {
        for (int q = threadIdx.x; q < 2 * TZ * 16 + 256; q += 256) {
            int z, hl, wl, dz = 0, dh = 0, dw = 0;
            if (q < TZ * 16) {
                if (w0 == 0) continue;
                z = q >> 4; hl = q & 15; wl = 0; dw = 1;
            } else if (q < 2 * TZ * 16) {
                if (h0 == 0) continue;
                const int j = q - TZ * 16;
                z = j >> 4; wl = j & 15; hl = 0; dh = 1;
            } else {
                if (sc == 0) continue;
                const int j = q - 2 * TZ * 16;
                hl = j >> 4; wl = j & 15; z = 0; dz = 1;
            }
            const int s = sc + z, h = h0 + hl, w = w0 + wl;
            if (s >= ns || h >= g.H || w >= g.W) continue;
            const long off = (long)(s0 + s) * hw + (long)h * g.W + w;
            const long long v = g.v[off];
            if (v == 0) continue;
            if (g.v[off - dz * hw - dh * g.W - dw] != v) continue;
            const int gi = base + (h * g.W + w) * ns + s;
            unite(parent, gi - dz - (dh * g.W + dw) * ns, gi);
        }
    }
}

// the nodes of 256 plane positions of a case are one contiguous run: (see lcc_count_kernel)
__global__ __launch_bounds__(256) void lccb_count_kernel(const long long* __restrict__ start, int S_total, int HW,
                                                         int* __restrict__ parent, int* __restrict__ area) {
    int s0, ns;
    case_range(start, blockIdx.y, S_total, s0, ns);
    const int p0 = (int)blockIdx.x * 256, np = min(256, HW - p0);
    const int first = (int)((long)s0 * HW) + p0 * ns, count = np * ns;
    for (int o = 0; o < count; o += 256) {        // whole waves: the trip count is the block's
        const int j = o + (int)threadIdx.x, i = first + j;
        int a = 0, r = -1;
        if (j < count) {
            a = area[i];
            if (a > 0) {
                r = find_plain(parent, i);
                if (r != i) atomicMin(parent + i, r);
                else a = 0;
            }
        }
        unsigned long long pending = __ballot(a > 0);
        while (pending) {
            const int leader = __ffsll((long long)pending) - 1;
            const int rl = __shfl(r, leader);
            const bool mine = a > 0 && r == rl;
            int s = mine ? a : 0;
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d);
            if ((int)(threadIdx.x & 63) == leader) atomicAdd(area + rl, s);
            if (mine) a = 0;
            pending &= ~__ballot(mine);
        }
    }
}

// thread = one plane position of the case, all its slices (consecutive nodes); ctrl[2k] = max key, ctrl[2k + 1] = positive flag
__global__ __launch_bounds__(256) void lccb_select_kernel(Cases g, const int* __restrict__ parent, const int* __restrict__ area,
                                                          unsigned long long* __restrict__ ctrl) {
    __shared__ unsigned long long sk[4];
    __shared__ int sp[4];
    const int k = blockIdx.y;
    int s0, ns;
    case_range(g.start, k, g.S_total, s0, ns);
    const long hw = (long)g.H * g.W;
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    unsigned long long key = 0;
    int pos = 0;
    if (p < hw) {
        const int first = (int)(s0 * hw + p * ns);
        for (int s = 0; s < ns; ++s) {
            const int i = first + s;
            if (parent[i] != i) continue;
            key = umax64(key, ((unsigned long long)(unsigned)area[i] << 32) | (unsigned)(0x7fffffff - i));
            if (!pos) pos = g.v[(long)(s0 + s) * hw + p] > 0;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        key = umax64(key, __shfl_xor(key, o));
        pos |= __shfl_xor(pos, o);
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) { sk[wid] = key; sp[wid] = pos; }
    __syncthreads();
    if (threadIdx.x == 0) {
        key = umax64(umax64(sk[0], sk[1]), umax64(sk[2], sk[3]));
        pos = sp[0] | sp[1] | sp[2] | sp[3];
        if (key) atomicMax(ctrl + 2 * k, key);
        if (pos) atomicMax(ctrl + 2 * k + 1, 1ull);
    }
}

__global__ __launch_bounds__(256) void lccb_write_kernel(const long long* __restrict__ start, int S_total, long hw,
                                                         const int* __restrict__ parent,
                                                         const unsigned long long* __restrict__ ctrl,
                                                         unsigned char* __restrict__ out) {
    const int k = blockIdx.y;
    int s0, ns;
    case_range(start, k, S_total, s0, ns);
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= hw) return;
    const int best = ctrl[2 * k + 1] ? 0x7fffffff - (int)(unsigned)(ctrl[2 * k] & 0xffffffffull) : -1;
    const int first = (int)(s0 * hw + p * ns);
    for (int s = 0; s < ns; ++s) {
        const int q = parent[first + s];
        out[(long)(s0 + s) * hw + p] = (best >= 0 && q >= 0 && find_plain(parent, q) == best) ? 1 : 0;
    }
}

// per-class forms (see lcc_select_classes_kernel): the control words of case k are the k-th group of C in each of the three
// runs of K * C words
template <bool STATS>
__global__ __launch_bounds__(256) void lccb_select_classes_kernel(Cases g, const int* __restrict__ parent,
                                                                  const int* __restrict__ area, int C,
                                                                  unsigned long long* __restrict__ ctrl) {
    const int k = blockIdx.y, K = gridDim.y;
    int s0, ns;
    case_range(g.start, k, g.S_total, s0, ns);
    const long hw = (long)g.H * g.W;
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    ClassAcc a = {};
    if (p < hw) {
        const int first = (int)(s0 * hw + p * ns);
        for (int s = 0; s < ns; ++s) {
            const int i = first + s;
            if (parent[i] != i) continue;
            const int c = class_of(g.v[(long)(s0 + s) * hw + p], C);
            if (c) class_add<STATS>(a, c, i, area[i]);
        }
    }
    class_commit<STATS>(a, C, ctrl + (long)k * C, ctrl + (long)(K + k) * C, ctrl + (long)(2 * K + k) * C);
}

__global__ __launch_bounds__(256) void lccb_write_classes_kernel(Cases g, const int* __restrict__ parent, int C,
                                                                 const unsigned long long* __restrict__ ctrl,
                                                                 unsigned char* __restrict__ out, long long* __restrict__ stats) {
    __shared__ int best[MAXC];
    const int k = blockIdx.y, K = gridDim.y;
    const unsigned long long* keys = ctrl + (long)k * C;
    class_best(keys, C, best);
    if (stats && blockIdx.x == 0)
        class_stats(keys, ctrl + (long)(K + k) * C, ctrl + (long)(2 * K + k) * C, C, stats + (long)k * C * 3);
    int s0, ns;
    case_range(g.start, k, g.S_total, s0, ns);
    const long hw = (long)g.H * g.W;
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= hw) return;
    const int first = (int)(s0 * hw + p * ns);
    for (int s = 0; s < ns; ++s) {
        const int q = parent[first + s];
        int o = 0;
        if (q >= 0) {
            const int c = class_of(g.v[(long)(s0 + s) * hw + p], C);
            if (c && best[c] >= 0 && find_plain(parent, q) == best[c]) o = c;
        }
        out[(long)(s0 + s) * hw + p] = (unsigned char)o;
    }
}

// out[k][0..3] = N, sum p*t, sum p, sum t with t = (target byte == match); VEC: 16 bytes per load (hw % 16 == 0, aligned)
template <bool VEC>
__global__ __launch_bounds__(256) void confusion_batched_kernel(const unsigned char* __restrict__ p,
                                                                const unsigned char* __restrict__ tg,
                                                                const long long* __restrict__ start, int S_total, long hw,
                                                                int match, long long* __restrict__ out) {
    __shared__ long long sm[3][4];
    const int k = blockIdx.y;
    int s0, ns;
    case_range(start, k, S_total, s0, ns);
    const long n = ns * hw;
    const unsigned char* pp = p + s0 * hw;
    const unsigned char* tp = tg + s0 * hw;
    long long spt = 0, sp = 0, st = 0;
    if (VEC) {
        for (long o = ((long)blockIdx.x * 256 + threadIdx.x) * 16; o < n; o += (long)gridDim.x * 256 * 16) {
            const uint4 a = *reinterpret_cast<const uint4*>(pp + o);
            const uint4 b = *reinterpret_cast<const uint4*>(tp + o);
            const unsigned aw[4] = {a.x, a.y, a.z, a.w}, bw[4] = {b.x, b.y, b.z, b.w};
            unsigned c0 = 0, c1 = 0, c2 = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int sh = 0; sh < 32; sh += 8) {
                    const unsigned x = (aw[j] >> sh) & 255u, m = ((bw[j] >> sh) & 255u) == (unsigned)match;
                    c0 += m ? x : 0u; c1 += x; c2 += m;
                }
            spt += c0; sp += c1; st += c2;
        }
    } else {
        for (long o = (long)blockIdx.x * 256 + threadIdx.x; o < n; o += (long)gridDim.x * 256) {
            const unsigned x = pp[o], m = tp[o] == (unsigned)match;
            spt += m ? x : 0u; sp += x; st += m;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        spt += __shfl_xor(spt, o);
        sp += __shfl_xor(sp, o);
        st += __shfl_xor(st, o);
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) { sm[0][wid] = spt; sm[1][wid] = sp; sm[2][wid] = st; }
    __syncthreads();
    if (threadIdx.x < 3) {
        const long long s = sm[threadIdx.x][0] + sm[threadIdx.x][1] + sm[threadIdx.x][2] + sm[threadIdx.x][3];
        if (s) atomicAdd(reinterpret_cast<unsigned long long*>(out + 4 * k + 1 + threadIdx.x), (unsigned long long)s);
    }
    if (blockIdx.x == 0 && threadIdx.x == 3) out[4 * k] = n;
}

// [S_total][H][W] with K cases: everything the grids and the node indices need fits an int
bool batch_ok(int64_t S_total, int64_t H, int64_t W, int64_t K) {
    if (S_total < 0 || H < 0 || W < 0 || K < 0 || K > 65535) return false;
    return dims_ok(S_total, H, W);
}

}  // namespace

extern "C" {

size_t aide_lcc3d_ws_bytes(int64_t nvox) {
    if (nvox < 0 || nvox > INT32_MAX) return 0;
    return (size_t)(2 * nvox) * sizeof(int) + 16 + 2 * sizeof(unsigned long long);
}

int aide_keep_largest_cc3d(const long long* v, int64_t d0, int64_t d1, int64_t d2, int64_t s0, int64_t s1, int64_t s2,
                           unsigned char* out, void* ws, hipStream_t stream) {
    if (!dims_ok(d0, d1, d2)) return AIDE_ERR_ARG;
    const int n = (int)(d0 * d1 * d2);
    if (n == 0) return 0;
    if (!v || !out || !ws) return AIDE_ERR_ARG;
    if ((reinterpret_cast<uintptr_t>(ws) & 15) != 0) return AIDE_ERR_ARG;
    int* parent = static_cast<int*>(ws);
    int* area = parent + n;
    unsigned long long* ctrl = reinterpret_cast<unsigned long long*>(
        (reinterpret_cast<uintptr_t>(area + n) + 15) & ~static_cast<uintptr_t>(15));
    Vol g;
    g.v = v; g.s0 = (long)s0; g.s1 = (long)s1; g.s2 = (long)s2;
    g.d0 = (int)d0; g.d1 = (int)d1; g.d2 = (int)d2;
    g.tx = (int)((d2 + TX - 1) / TX); g.ty = (int)((d1 + TY - 1) / TY);
    const long tiles = (long)g.tx * g.ty * ((d0 + TZ - 1) / TZ);
    const unsigned nb = (unsigned)(((long)n + 255) / 256);
    const unsigned ntile = (unsigned)min(tiles, 65536L);
    const unsigned nsel = (unsigned)min((long)nb, 1024L);
    const double bytes = 29.0 * n;   // algorithmic traffic: V 8 + parent / area 4 + 4 (local), count 4, select 4, write 4 + 1
    AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, bytes, lcc_local_kernel, dim3(ntile), dim3(256), 0, stream, g, tiles, parent, area, ctrl);
    AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 0.0, lcc_border_kernel, dim3(ntile), dim3(256), 0, stream, g, tiles, parent);
    AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 0.0, lcc_count_kernel, dim3(nb), dim3(256), 0, stream, parent, area, n);
    AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 0.0, lcc_select_kernel, dim3(nsel), dim3(256), 0, stream, g,
                      (const int*)parent, (const int*)area, n, ctrl);
    AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 0.0, lcc_write_kernel, dim3(nb), dim3(256), 0, stream, (const int*)parent, n,
                      (const unsigned long long*)ctrl, out);
    return aide_launch_status();
}

size_t aide_lcc3d_classes_ws_bytes(int64_t nvox, int num_classes) {
    if (nvox < 0 || nvox > INT32_MAX || num_classes < 2 || num_classes > MAXC) return 0;
    return (size_t)(2 * nvox) * sizeof(int) + 16 + (size_t)(3 * num_classes) * sizeof(unsigned long long);
}

// launches 1 - 3 are the binary form's, unchanged; one memset clears the 3 C control words before them
int aide_keep_largest_cc3d_classes(const long long* v, int64_t d0, int64_t d1, int64_t d2, int64_t s0, int64_t s1, int64_t s2,
                                   int num_classes, unsigned char* out, long long* stats, void* ws, hipStream_t stream) {
    if (num_classes < 2 || num_classes > MAXC || !dims_ok(d0, d1, d2)) return AIDE_ERR_ARG;
    const int n = (int)(d0 * d1 * d2), C = num_classes;
    if (n == 0) {
        if (!stats) return 0;
        return (int)hipMemsetAsync(stats, 0, (size_t)(3 * C) * sizeof(long long), stream);
    }
    if (!v || !out || !ws) return AIDE_ERR_ARG;
    if ((reinterpret_cast<uintptr_t>(ws) & 15) != 0) return AIDE_ERR_ARG;
    int* parent = static_cast<int*>(ws);
    int* area = parent + n;
    unsigned long long* ctrl = reinterpret_cast<unsigned long long*>(
        (reinterpret_cast<uintptr_t>(area + n) + 15) & ~static_cast<uintptr_t>(15));
    Vol g;
    g.v = v; g.s0 = (long)s0; g.s1 = (long)s1; g.s2 = (long)s2;
    g.d0 = (int)d0; g.d1 = (int)d1; g.d2 = (int)d2;
    g.tx = (int)((d2 + TX - 1) / TX); g.ty = (int)((d1 + TY - 1) / TY);
    const long tiles = (long)g.tx * g.ty * ((d0 + TZ - 1) / TZ);
    const unsigned nb = (unsigned)(((long)n + 255) / 256);
    const unsigned ntile = (unsigned)min(tiles, 65536L);
    const unsigned nsel = (unsigned)min((long)nb, 1024L);
    hipError_t e = hipMemsetAsync(ctrl, 0, (size_t)(3 * C) * sizeof(unsigned long long), stream);
    if (e != hipSuccess) return (int)e;
    const double bytes = 29.0 * n;
    AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, bytes, lcc_local_kernel, dim3(ntile), dim3(256), 0, stream, g, tiles, parent, area, ctrl);
    AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 0.0, lcc_border_kernel, dim3(ntile), dim3(256), 0, stream, g, tiles, parent);
    AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 0.0, lcc_count_kernel, dim3(nb), dim3(256), 0, stream, parent, area, n);
    if (stats)
        AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 0.0, lcc_select_classes_kernel<true>, dim3(nsel), dim3(256), 0, stream, g,
                          (const int*)parent, (const int*)area, n, C, ctrl);
    else
        AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 0.0, lcc_select_classes_kernel<false>, dim3(nsel), dim3(256), 0, stream, g,
                          (const int*)parent, (const int*)area, n, C, ctrl);
    AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 0.0, lcc_write_classes_kernel, dim3(nb), dim3(256), 0, stream, g, (const int*)parent, n, C,
                      (const unsigned long long*)ctrl, out, stats);
    return aide_launch_status();
}

int aide_case_confusion(const void* p, int p_u8, int64_t p_s0, int64_t p_s1, int64_t p_s2, const void* t, int t_u8,
                        int64_t t_s0, int64_t t_s1, int64_t t_s2, int64_t d0, int64_t d1, int64_t d2, long long* out,
                        hipStream_t stream) {
    if (!dims_ok(d0, d1, d2) || !out || (p_u8 != 0 && p_u8 != 1) || (t_u8 != 0 && t_u8 != 1)) return AIDE_ERR_ARG;
    const int n = (int)(d0 * d1 * d2);
    if (n > 0 && (!p || !t)) return AIDE_ERR_ARG;
    hipError_t e = hipMemsetAsync(out, 0, 4 * sizeof(long long), stream);
    if (e != hipSuccess) return (int)e;
    if (n == 0) return 0;
    const Operand P{p, (long)p_s0, (long)p_s1, (long)p_s2}, T{t, (long)t_s0, (long)t_s1, (long)t_s2};
    const dim3 grid((unsigned)min(((long)n + 1023) / 1024, 1024L)), block(256);
    const int e1 = (int)d1, e2 = (int)d2;
    if (p_u8 && t_u8)
        AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 2.0 * n, (confusion_kernel<unsigned char, unsigned char>), grid, block, 0, stream, P, T, e1, e2, n, out);
    else if (p_u8)
        AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 9.0 * n, (confusion_kernel<unsigned char, long long>), grid, block, 0, stream, P, T, e1, e2, n, out);
    else if (t_u8)
        AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 9.0 * n, (confusion_kernel<long long, unsigned char>), grid, block, 0, stream, P, T, e1, e2, n, out);
    else
        AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 16.0 * n, (confusion_kernel<long long, long long>), grid, block, 0, stream, P, T, e1, e2, n, out);
    return aide_launch_status();
}

size_t aide_lcc3d_batched_ws_bytes(int64_t nvox_total, int64_t K) {
    if (nvox_total < 0 || nvox_total > INT32_MAX || K < 0 || K > 65535) return 0;
    return (size_t)(2 * nvox_total) * sizeof(int) + 16 + (size_t)(2 * K) * sizeof(unsigned long long);
}

int aide_keep_largest_cc3d_batched(const long long* v, const long long* slice_start, int64_t K, int64_t S_total, int64_t H,
                                   int64_t W, unsigned char* out, void* ws, hipStream_t stream) {
    if (!batch_ok(S_total, H, W, K)) return AIDE_ERR_ARG;
    const int n = (int)(S_total * H * W);
    if (n == 0 || K == 0) return 0;
    if (!v || !slice_start || !out || !ws) return AIDE_ERR_ARG;
    if ((reinterpret_cast<uintptr_t>(ws) & 15) != 0) return AIDE_ERR_ARG;
    int* parent = static_cast<int*>(ws);
    int* area = parent + n;
    unsigned long long* ctrl = reinterpret_cast<unsigned long long*>(
        (reinterpret_cast<uintptr_t>(area + n) + 15) & ~static_cast<uintptr_t>(15));
    Cases g;
    g.v = v; g.start = slice_start; g.S_total = (int)S_total; g.H = (int)H; g.W = (int)W;
    g.tw = (int)((W + 15) / 16);
    const long tiles = (long)g.tw * ((H + 15) / 16), chunks = (H * W + 255) / 256;
    if (tiles > INT32_MAX) return AIDE_ERR_ARG;
    const dim3 gt((unsigned)tiles, (unsigned)K), gc((unsigned)chunks, (unsigned)K), block(256);
    const int hw = (int)(H * W);
    AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 29.0 * n, lccb_local_kernel, gt, block, 0, stream, g, parent, area, ctrl);
    AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 0.0, lccb_border_kernel, gt, block, 0, stream, g, parent);
    AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 0.0, lccb_count_kernel, gc, block, 0, stream, slice_start, (int)S_total, hw, parent, area);
    AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 0.0, lccb_select_kernel, gc, block, 0, stream, g, (const int*)parent, (const int*)area,
                      ctrl);
    AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 0.0, lccb_write_kernel, gc, block, 0, stream, slice_start, (int)S_total, (long)hw,
                      (const int*)parent, (const unsigned long long*)ctrl, out);
    return aide_launch_status();
}

size_t aide_lcc3d_classes_batched_ws_bytes(int64_t nvox_total, int64_t K, int num_classes) {
    if (nvox_total < 0 || nvox_total > INT32_MAX || K < 0 || K > 65535 || num_classes < 2 || num_classes > MAXC) return 0;
    return (size_t)(2 * nvox_total) * sizeof(int) + 16 + (size_t)(3 * K * num_classes) * sizeof(unsigned long long);
}

int aide_keep_largest_cc3d_classes_batched(const long long* v, const long long* slice_start, int64_t K, int64_t S_total,
                                           int64_t H, int64_t W, int num_classes, unsigned char* out, long long* stats,
                                           void* ws, hipStream_t stream) {
    if (num_classes < 2 || num_classes > MAXC || !batch_ok(S_total, H, W, K)) return AIDE_ERR_ARG;
    const int n = (int)(S_total * H * W), C = num_classes;
    if (n == 0 || K == 0) {
        if (!stats || K == 0) return 0;
        return (int)hipMemsetAsync(stats, 0, (size_t)(3 * K * C) * sizeof(long long), stream);
    }
    if (!v || !slice_start || !out || !ws) return AIDE_ERR_ARG;
    if ((reinterpret_cast<uintptr_t>(ws) & 15) != 0) return AIDE_ERR_ARG;
    int* parent = static_cast<int*>(ws);
    int* area = parent + n;
    unsigned long long* ctrl = reinterpret_cast<unsigned long long*>(
        (reinterpret_cast<uintptr_t>(area + n) + 15) & ~static_cast<uintptr_t>(15));
    Cases g;
    g.v = v; g.start = slice_start; g.S_total = (int)S_total; g.H = (int)H; g.W = (int)W;
    g.tw = (int)((W + 15) / 16);
    const long tiles = (long)g.tw * ((H + 15) / 16), chunks = (H * W + 255) / 256;
    if (tiles > INT32_MAX) return AIDE_ERR_ARG;
    const dim3 gt((unsigned)tiles, (unsigned)K), gc((unsigned)chunks, (unsigned)K), block(256);
    const int hw = (int)(H * W);
    hipError_t e = hipMemsetAsync(ctrl, 0, (size_t)(3 * K * C) * sizeof(unsigned long long), stream);
    if (e != hipSuccess) return (int)e;
    AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 29.0 * n, lccb_local_kernel, gt, block, 0, stream, g, parent, area, ctrl);
    AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 0.0, lccb_border_kernel, gt, block, 0, stream, g, parent);
    AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 0.0, lccb_count_kernel, gc, block, 0, stream, slice_start, (int)S_total, hw, parent, area);
    if (stats)
        AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 0.0, lccb_select_classes_kernel<true>, gc, block, 0, stream, g, (const int*)parent,
                          (const int*)area, C, ctrl);
    else
        AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 0.0, lccb_select_classes_kernel<false>, gc, block, 0, stream, g, (const int*)parent,
                          (const int*)area, C, ctrl);
    AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 0.0, lccb_write_classes_kernel, gc, block, 0, stream, g, (const int*)parent, C,
                      (const unsigned long long*)ctrl, out, stats);
    return aide_launch_status();
}

int aide_case_confusion_batched(const unsigned char* p, const unsigned char* t, const long long* slice_start, int64_t K,
                                int64_t S_total, int64_t H, int64_t W, int match, long long* out, hipStream_t stream) {
    if (!batch_ok(S_total, H, W, K) || match < 0 || match > 255) return AIDE_ERR_ARG;
    if (K == 0) return 0;
    if (!out || !slice_start) return AIDE_ERR_ARG;
    const long hw = (long)(H * W);
    if (S_total * hw > 0 && (!p || !t)) return AIDE_ERR_ARG;
    hipError_t e = hipMemsetAsync(out, 0, (size_t)K * 4 * sizeof(long long), stream);
    if (e != hipSuccess) return (int)e;
    const bool vec = hw % 16 == 0 && ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(t)) & 15) == 0;
    const long per = vec ? 4096 : 256;
    const dim3 grid((unsigned)max(1L, min((hw + per - 1) / per * 4, 1024L)), (unsigned)K), block(256);
    const double bytes = 2.0 * (double)S_total * (double)hw;
    if (vec)
        AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, bytes, confusion_batched_kernel<true>, grid, block, 0, stream, p, t, slice_start,
                          (int)S_total, hw, match, out);
    else
        AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, bytes, confusion_batched_kernel<false>, grid, block, 0, stream, p, t, slice_start,
                          (int)S_total, hw, match, out);
    return aide_launch_status();
}

}  // extern "C"
