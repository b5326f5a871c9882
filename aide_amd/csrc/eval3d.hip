// Per-case evaluation on the device: the largest 3-D connected component of a label volume and the confusion sums of a
// predicted volume against its target (include/aide_hip.h "per-case evaluation").
//
// Largest component: union-find over the logical raster index i = (i0 * D1 + i1) * D2 + i2 of the foreground voxels
// (V != 0; face neighbours of EQUAL value are connected).  The root of a set is always its smallest index, so it IS the
// component's first voxel in raster order.  Invariant: parent[i] <= i, and after the launch that initialises it every
// global write to `parent` is an atomicMin -- parents only decrease, so every find and union loop ends, and no workgroup
// ever waits for another (no spin, no co-residency assumption).  One pipeline of five launches:
//   1 local   one workgroup per 16 x 16 x 4 tile: union-find in LDS; parent[i] = first voxel of i's blob inside the tile
//             (-1 for background), area[i] = that blob's voxel count at its first voxel, 0 elsewhere
//   2 border  per tile, face-adjacent equal-valued pairs across its three lower faces joined with atomicMin; parent words
//             other workgroups write are read with agent-scope relaxed atomic loads (no stale L1 / L2 line)
//   3 count   every tile-blob root that is no longer a root adds its area to its set's root (wave-aggregated atomics)
//   4 select  key = (area << 32) | (0x7fffffff - root), block max, one atomicMax per block
//   5 write   out[i] = 1 (the voxel's class) where find(i) is the chosen root
// Everything is integer and the result does not depend on the schedule.
//
// Every stage is written once over a `View`: a strided volume with logical dims, element strides and the node index of
// its first voxel.  Two geometries supply views and index maps, nothing else:
//   Strided  (aide_keep_largest_cc3d[_classes]) the caller's volume itself, node base 0.  A thread of a tile walks the 4-deep
//            logical axis 0 and the 256 threads cover (i1, i2); the grid is strided over the tiles; lanes run along i2.
//   Ragged   (aide_keep_largest_cc3d[_classes]_batched) K cases concatenated as [S_total][H][W] with a device table
//            slice_start[K + 1]; blockIdx.y is the case.  Case k is the view with dims (H, W, S_k), strides (W, 1, H * W),
//            data offset and node base slice_start[k] * H * W: a case owns a contiguous range of nodes whose order is its own
//            raster order, a union never leaves the range because a tile never leaves its case, and nodes outside the
//            (clamped) case ranges are neither read nor written.  A thread walks the 4-deep logical axis 2 (slices), the 256
//            threads cover a 16 x 16 patch of (h, w), and a block walks its patch (its 256 plane positions in count, select
//            and write) through all the slices of the case; lanes run along w.
// In both, the local index inside a tile is raster order of the logical index, so a tile-blob's lowest local index is its
// first voxel.  The number of launches is five whatever K is.
//
// Modes: BINARY keeps the largest component of all values (nothing when no voxel is positive: the reference's
// `if mask.max() > 0`); control words per case: key, positive flag -- cleared by launch 1.  CLASSES: blobs of different
// values are separate sets already, so launches 1 - 3 are shared as they are and only select and write differ: one key per
// class value 1 .. C - 1 (the value read at the root), out[i] = the voxel's own class where its root is that class's winner.
// The 3 C control words per case (keys, root counts, area sums) are cleared by one memset in front of launch 1: five
// launches and one memset whatever C and K are.
//
// Case post-processing on the single volume reuses the pipeline (the invariant above holds for all of it: integers,
// atomicMin / atomicOr / atomicMax / atomicAdd only, nothing depends on the schedule, no workgroup waits for another):
//   k largest, size floor  (aide_keep_components3d) launches 1 - 3, one select pass per rank, and a write that compares
//                          key(find(i)) with the slot's threshold
//   holes                  (aide_fill_holes3d) launches 1 - 3 with the connectivity predicate "value == 0" (launches 1 - 2 take
//                          the predicate as a template parameter), one word per root that records what the blob touches, a
//                          write that fills where the word is exactly one class
//   labelled components    (aide_label_components3d) launches 1 - 3, then the rank of every root = the number of roots with a
//                          lower node index (roots are first voxels, so this is the blob's number in raster order): a prefix
//                          sum over the root flags in three launches -- per-block root counts, a scan of the block counts by
//                          ONE workgroup that loops over them (it is the only workgroup of its launch and reads what the
//                          launch before it wrote: nothing is looked back at, nothing is waited for), a per-block local scan
//                          plus the block's offset -- and one write: labels[i] = rank(find(i)) + 1, box and coordinate sums
//                          of the blobs below the cap with atomicMin / atomicMax / 64-bit atomicAdd, gathered per block in a
//                          table in LDS first.  Seven launches and at most one memset (the props table), whatever the
//                          volume, the class count and the cap are
//   lesion counts          (aide_lesion_counts3d) per volume A of (target, pred), B the other one: launches 1 - 3 on A, one
//                          launch that adds every voxel of A at which B agrees to cover[find(i)], one that reduces the roots
//                          into the six columns per class.  Both volumes go through the SAME three words per voxel one after
//                          the other (parent, area, cover).  Ten launches and three memsets (the table, cover twice).  The
//                          one non-integer operation of the file is its threshold: double(cover) >= overlap * double(area)
// In all of them no workgroup ever waits for another.
#include "volume3d.h"

namespace {

constexpr int TQ = 16, TZ = 4, TILE = TQ * TQ * TZ;   // a tile: 16 x 16 threads, each walking TZ voxels of the slab axis

struct View {
    const long long* v;   // voxel (0, 0, 0)
    long s0, s1, s2;      // element strides of the logical dims
    int d0, d1, d2;
    int base;             // node of voxel (0, 0, 0); node of (i0, i1, i2) = base + raster index
    __device__ __forceinline__ bool has(int i0, int i1, int i2) const { return i0 < d0 && i1 < d1 && i2 < d2; }
    __device__ __forceinline__ long off(int i0, int i1, int i2) const { return (long)i0 * s0 + (long)i1 * s1 + (long)i2 * s2; }
    __device__ __forceinline__ void decode(int i, int& i0, int& i1, int& i2) const { raster_decode(i, d1, d2, i0, i1, i2); }
    __device__ __forceinline__ long off_of(int i) const {   // of raster index i
        int i0, i1, i2;
        decode(i, i0, i1, i2);
        return off(i0, i1, i2);
    }
    __device__ __forceinline__ int node(int i0, int i1, int i2) const { return base + (i0 * d1 + i1) * d2 + i2; }
};

// Thread coordinates of a tile: z = 0 .. TZ - 1 along the slab axis, (p, q) = (t / 16, t % 16), q along the lanes.
// SLAB = 0: logical (z, p, q), tile extents 4 x 16 x 16.  SLAB = 2: logical (p, q, z), extents 16 x 16 x 4.
template <int SLAB>
__device__ __forceinline__ void to_logical(int z, int p, int q, int& l0, int& l1, int& l2) {
    if (SLAB == 0) { l0 = z; l1 = p; l2 = q; } else { l0 = p; l1 = q; l2 = z; }
}
// local index = raster order of the logical index inside the tile; the strides of logical axes 0 and 1 in it
template <int SLAB> constexpr int LS1 = SLAB == 0 ? TQ : TZ;
template <int SLAB> constexpr int LS0 = TQ * LS1<SLAB>;

struct Strided {
    static constexpr int SLAB = 0;
    View g;
    int t1, t2, tiles;    // tiles along i1 and i2, and in all
    __device__ View view() const { return g; }
    __device__ int tile_begin() const { return blockIdx.x; }
    __device__ int tile_end(const View&) const { return tiles; }
    __device__ int tile_step() const { return gridDim.x; }
    __device__ void tile_origin(int tile, int& o0, int& o1, int& o2) const {
        const int t12 = t1 * t2, a = tile / t12, r = tile - a * t12, b = r / t2;
        o0 = a * TZ; o1 = b * TQ; o2 = (r - b * t2) * TQ;
    }
    // count: the block's run of nodes
    __device__ void count_run(const View& g, int& first, int& count) const {
        const int b = (int)blockIdx.x * 256;
        first = g.base + b;
        count = min(256, g.d0 * g.d1 * g.d2 - b);
    }
    // A thread's nodes in select and write: f(node, offset of its value, index in `out`).  The offset is a callable: it is
    // decoded from the node only where it is needed.  Select is grid-strided over the nodes, write has one node per thread
    template <class F>
    __device__ void visit(const View& g, int i, F& f) const {
        f(g.base + i, [&] { return g.off_of(i); }, (long)i);
    }
    template <class F>
    __device__ void select_nodes(const View& g, F f) const {
        const unsigned n = (unsigned)(g.d0 * g.d1 * g.d2);
        for (unsigned u = blockIdx.x * 256u + threadIdx.x; u < n; u += gridDim.x * 256u) visit(g, (int)u, f);
    }
    template <class F>
    __device__ void write_nodes(const View& g, F f) const {
        const unsigned u = blockIdx.x * 256u + threadIdx.x;
        if (u < (unsigned)(g.d0 * g.d1 * g.d2)) visit(g, (int)u, f);
    }
};

struct Ragged {
    static constexpr int SLAB = 2;
    const long long* v;       // [S_total][H][W], contiguous
    const long long* start;   // [K + 1] first slice of every case (device)
    int S_total, H, W;
    int tw;                   // 16-wide tiles along w
    __device__ View view() const {
        int s0, ns;
        case_range(start, blockIdx.y, S_total, s0, ns);
        const long hw = (long)H * W;
        return View{v + s0 * hw, W, 1, hw, H, W, ns, (int)(s0 * hw)};
    }
    // the block's 16 x 16 patch of the plane, TZ slices at a time
    __device__ int tile_begin() const { return 0; }
    __device__ int tile_end(const View& g) const { return (g.d2 + TZ - 1) / TZ; }
    __device__ int tile_step() const { return 1; }
    __device__ void tile_origin(int tile, int& o0, int& o1, int& o2) const {
        o0 = (int)(blockIdx.x / tw) * TQ; o1 = (int)(blockIdx.x % tw) * TQ; o2 = tile * TZ;
    }
    // the nodes of 256 plane positions of a case are one contiguous run
    __device__ void count_run(const View& g, int& first, int& count) const {
        const int p0 = (int)blockIdx.x * 256;
        first = g.base + p0 * g.d2;
        count = min(256, g.d0 * g.d1 - p0) * g.d2;
    }
    // select and write: thread = one plane position p = h * W + w of the case, all its slices (consecutive nodes)
    template <class F>
    __device__ void select_nodes(const View& g, F f) const {
        const long p = (long)blockIdx.x * 256 + threadIdx.x;
        if (p >= (long)g.d0 * g.d1) return;
        const int first = g.base + (int)p * g.d2;
        for (int s = 0; s < g.d2; ++s) f(first + s, [&] { return s * g.s2 + p; }, g.base + s * g.s2 + p);
    }
    template <class F>
    __device__ void write_nodes(const View& g, F f) const { select_nodes(g, f); }
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

__device__ __forceinline__ int find_plain(const int* parent, int x) {
    int q = parent[x];
    while (q != x) { x = q; q = parent[x]; }
    return x;
}

// The connectivity predicate of launches 1 - 2: `at` maps the stored value to the value the union-find sees (0: the voxel is in
// no set; face neighbours of EQUAL non-zero mapped value join), `joins(axis)` says whether faces across a logical axis connect.
// Equal: the label itself, every axis -- the component filters.  Background<T>: 1 on the voxels whose stored value (T = int64
// or uint8) is exactly 0, so the sets are the blobs of background; axis `cut` (-1: none) does not connect: 2-D slices along it.
struct Equal {
    __device__ __forceinline__ long long at(const View& g, long off) const { return g.v[off]; }
    __device__ __forceinline__ bool joins(int) const { return true; }
};
template <typename T>
struct Background {
    int cut;
    __device__ __forceinline__ T raw(const View& g, long off) const { return reinterpret_cast<const T*>(g.v)[off]; }
    __device__ __forceinline__ long long at(const View& g, long off) const { return raw(g, off) == 0; }
    __device__ __forceinline__ bool joins(int axis) const { return axis != cut; }
};

// ---- 1 local: the tile at logical origin (o0, o1, o2); out-of-volume voxels read as background ----
// A thread's column: TZ voxels along the slab axis from the tile's voxel (c0, c1, c2), each step LZ local indices,
// slab_stride elements and slab_nodes nodes further on; `depth` of them lie inside the volume
template <int SLAB, class P>
__device__ __forceinline__ void tile_local(const View& g, const P& pred, int o0, int o1, int o2, int* __restrict__ parent,
                                           int* __restrict__ area, long long* val, int* lp, int* cnt) {
    constexpr int L0 = LS0<SLAB>, L1 = LS1<SLAB>, LZ = SLAB == 0 ? L0 : 1;
    const int t = threadIdx.x, p = t >> 4, q = t & 15;
    int c0, c1, c2;
    to_logical<SLAB>(0, p, q, c0, c1, c2);
    const int e0 = c0 * L0 + c1 * L1 + c2;
    const int depth = g.has(o0 + c0, o1 + c1, o2 + c2) ? (SLAB == 0 ? g.d0 - o0 : g.d2 - o2) : 0;
    const long off0 = g.off(o0 + c0, o1 + c1, o2 + c2), slab_stride = SLAB == 0 ? g.s0 : g.s2;
    const int node0 = depth ? g.node(o0 + c0, o1 + c1, o2 + c2) : 0, slab_nodes = SLAB == 0 ? g.d1 * g.d2 : 1;
    __syncthreads();                              // the previous tile's LDS is read to the end
#pragma unroll
    for (int z = 0; z < TZ; ++z) {
        const int e = e0 + z * LZ;
        long long v = 0;
        if (z < depth) v = pred.at(g, off0 + z * slab_stride);
        val[e] = v;
        lp[e] = v != 0 ? e : -1;
        cnt[e] = 0;
    }
    __syncthreads();
#pragma unroll
    for (int z = 0; z < TZ; ++z) {
        int l0, l1, l2;
        to_logical<SLAB>(z, p, q, l0, l1, l2);
        const int e = e0 + z * LZ;
        const long long v = val[e];
        if (v == 0) continue;
        if (l2 > 0 && pred.joins(2) && val[e - 1] == v) lds_unite(lp, e - 1, e);
        if (l1 > 0 && pred.joins(1) && val[e - L1] == v) lds_unite(lp, e - L1, e);
        if (l0 > 0 && pred.joins(0) && val[e - L0] == v) lds_unite(lp, e - L0, e);
    }
    __syncthreads();
    int root[TZ];
#pragma unroll
    for (int z = 0; z < TZ; ++z) {
        const int e = e0 + z * LZ;
        root[z] = val[e] != 0 ? lds_find(lp, e) : -1;
        if (root[z] >= 0) atomicAdd(&cnt[root[z]], 1);
    }
    __syncthreads();
#pragma unroll
    for (int z = 0; z < TZ; ++z) {
        if (z >= depth) break;
        int gr = -1;
        if (root[z] >= 0) {                       // the tile-blob's lowest local index is its first voxel: its lowest node
            const int r = root[z], r0 = r / L0, r1 = (r / L1) & (TQ - 1), r2 = r & (L1 - 1);
            gr = g.node(o0 + r0, o1 + r1, o2 + r2);
        }
        parent[node0 + z * slab_nodes] = gr;
        area[node0 + z * slab_nodes] = cnt[e0 + z * LZ];
    }
}

template <class G, class P>
__global__ __launch_bounds__(256) void lcc_local_kernel(G geo, P pred, int* __restrict__ parent, int* __restrict__ area,
                                                        unsigned long long* __restrict__ ctrl) {
    __shared__ long long val[TILE];
    __shared__ int lp[TILE];
    __shared__ int cnt[TILE];
    if (blockIdx.x == 0 && threadIdx.x == 0) { ctrl[2 * blockIdx.y] = 0ull; ctrl[2 * blockIdx.y + 1] = 0ull; }
    const View g = geo.view();
    for (int tile = geo.tile_begin(); tile < geo.tile_end(g); tile += geo.tile_step()) {
        int o0, o1, o2;
        geo.tile_origin(tile, o0, o1, o2);
        tile_local<G::SLAB>(g, pred, o0, o1, o2, parent, area, val, lp, cnt);
    }
}

// ---- 2 border: the three lower faces of a tile, in thread coordinates: q face (TZ x 16 pairs), p face (TZ x 16),
// z face (16 x 16) ----
template <int SLAB, class P>
__device__ __forceinline__ void tile_border(const View& g, const P& pred, int o0, int o1, int o2, int* __restrict__ parent) {
    for (int k = threadIdx.x; k < 2 * TZ * TQ + TQ * TQ; k += 256) {
        int z, p, q, dz = 0, dp = 0, dq = 0;
        if (k < TZ * TQ) {
            z = k >> 4; p = k & 15; q = 0; dq = 1;
        } else if (k < 2 * TZ * TQ) {
            const int j = k - TZ * TQ;
            z = j >> 4; q = j & 15; p = 0; dp = 1;
        } else {
            const int j = k - 2 * TZ * TQ;
            p = j >> 4; q = j & 15; z = 0; dz = 1;
        }
        int l0, l1, l2, e0, e1, e2;
        to_logical<SLAB>(z, p, q, l0, l1, l2);
        to_logical<SLAB>(dz, dp, dq, e0, e1, e2);
        const int a0 = o0 + l0, a1 = o1 + l1, a2 = o2 + l2;
        if (a0 < e0 || a1 < e1 || a2 < e2) continue;          // the face lies on the volume's edge
        if (!pred.joins(e0 ? 0 : e1 ? 1 : 2)) continue;
        if (!g.has(a0, a1, a2)) continue;
        const long off = g.off(a0, a1, a2);
        const long long v = pred.at(g, off);
        if (v == 0) continue;
        if (pred.at(g, off - g.off(e0, e1, e2)) != v) continue;
        unite(parent, g.node(a0 - e0, a1 - e1, a2 - e2), g.node(a0, a1, a2));
    }
}

template <class G, class P>
__global__ __launch_bounds__(256) void lcc_border_kernel(G geo, P pred, int* __restrict__ parent) {
    const View g = geo.view();
    for (int tile = geo.tile_begin(); tile < geo.tile_end(g); tile += geo.tile_step()) {
        int o0, o1, o2;
        geo.tile_origin(tile, o0, o1, o2);
        tile_border<G::SLAB>(g, pred, o0, o1, o2, parent);
    }
}

// ---- 3 count: tile-blob roots that were joined to another set add their area to its root.  Lanes of one wave that add
// to the same root are summed first: one atomic per (wave, root).  Whole waves: the trip count is the block's ----
template <class G>
__global__ __launch_bounds__(256) void lcc_count_kernel(G geo, int* __restrict__ parent, int* __restrict__ area) {
    const View g = geo.view();
    int first, count;
    geo.count_run(g, first, count);
    for (int o = 0; o < count; o += 256) {
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

// ---- 4 select, 5 write ----
// Control words of case k = blockIdx.y of K = gridDim.y (the single volume: k = 0, K = 1), by slot.
// BINARY, one slot: ctrl[2 k] = max key over the roots, ctrl[2 k + 1] = 1 when some root (so some voxel) holds a positive
// value.  CLASSES, slot j = class j + 1 <= C - 1 <= MAXC - 1: ctrl[k * C + c] = max key over the roots of class c,
// ctrl[(K + k) * C + c] = number of roots (components) of class c, ctrl[(2 K + k) * C + c] = sum of their areas (voxels of
// class c); word c = 0 of every group stays zero.  CLASSES_STATS: CLASSES that also fills the counts and the sums.
enum Mode { BINARY, CLASSES, CLASSES_STATS };
constexpr int MAXC = 8;
template <Mode M> constexpr int SLOTS = M == BINARY ? 1 : MAXC - 1;

struct Ctrl { long key, cnt, vox; };              // word of slot 0
template <Mode M>
__device__ __forceinline__ Ctrl ctrl_words(int C) {
    const long k = blockIdx.y, K = gridDim.y;
    if (M == BINARY) return Ctrl{2 * k, 2 * k + 1, 0};
    return Ctrl{k * C + 1, (K + k) * C + 1, (2 * K + k) * C + 1};
}

// 1 .. C - 1, or 0 for a value that belongs to no class (0, negative, >= C)
__device__ __forceinline__ int class_of(long long v, int C) { return (v > 0 && v < C) ? (int)v : 0; }

__device__ __forceinline__ unsigned long long umax64(unsigned long long a, unsigned long long b) { return a > b ? a : b; }

template <Mode M>
struct Acc {                                      // a thread's running key, root count and area sum per slot: registers
    unsigned long long key[SLOTS<M>];
    unsigned cnt[SLOTS<M>], vox[SLOTS<M>];        // a sum of areas of distinct roots never exceeds the voxel count < 2^31
};

// the key of root i of area ar: larger area first, then the lower root
__device__ __forceinline__ unsigned long long root_key(int i, int ar) {
    return ((unsigned long long)(unsigned)ar << 32) | (unsigned)(0x7fffffff - i);
}

// root i of area ar goes to `slot`
template <Mode M>
__device__ __forceinline__ void acc_add(Acc<M>& a, int slot, int i, int ar) {
    const unsigned long long key = root_key(i, ar);
#pragma unroll
    for (int j = 0; j < SLOTS<M>; ++j)
        if (slot == j) {
            a.key[j] = umax64(a.key[j], key);
            if (M == CLASSES_STATS) { a.cnt[j] += 1u; a.vox[j] += (unsigned)ar; }
        }
}

// wave reduce with __shfl_xor, block reduce through LDS, then thread j commits slot j: at most one atomicMax (and the flag's,
// or with the stats two integer atomicAdd) per (block, slot), none where the block saw no root of the slot
template <Mode M>
__device__ __forceinline__ void acc_commit(Acc<M>& a, int live, unsigned long long* __restrict__ ctrl, const Ctrl w) {
    __shared__ unsigned long long sk[4][SLOTS<M>];
    __shared__ unsigned sc[4][SLOTS<M>], sv[4][SLOTS<M>];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < SLOTS<M>; ++j) {
        if (j >= live) break;                     // uniform
        unsigned long long key = a.key[j];
        unsigned cn = a.cnt[j], vx = a.vox[j];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            key = umax64(key, __shfl_xor(key, o));
            if (M != CLASSES) cn += __shfl_xor(cn, o);
            if (M == CLASSES_STATS) vx += __shfl_xor(vx, o);
        }
        if (lane == 0) {
            sk[wid][j] = key;
            if (M != CLASSES) sc[wid][j] = cn;
            if (M == CLASSES_STATS) sv[wid][j] = vx;
        }
    }
    __syncthreads();
    const int j = threadIdx.x;
    if (j < live) {
        const unsigned long long key = umax64(umax64(sk[0][j], sk[1][j]), umax64(sk[2][j], sk[3][j]));
        if (key) atomicMax(ctrl + w.key + j, key);
        if (M != CLASSES) {
            const unsigned cn = sc[0][j] + sc[1][j] + sc[2][j] + sc[3][j];
            if (M == BINARY) { if (cn) atomicMax(ctrl + w.cnt + j, 1ull); }
            else if (cn) atomicAdd(ctrl + w.cnt + j, (unsigned long long)cn);
        }
        if (M == CLASSES_STATS) {
            const unsigned vx = sv[0][j] + sv[1][j] + sv[2][j] + sv[3][j];
            if (vx) atomicAdd(ctrl + w.vox + j, (unsigned long long)vx);
        }
    }
}

// the chosen root of a slot, -1 where it has none (key 0; BINARY: no positive voxel either)
template <Mode M>
__device__ __forceinline__ int chosen_root(const unsigned long long* __restrict__ ctrl, const Ctrl& w, int slot) {
    const unsigned long long key = ctrl[w.key + slot], flag = M == BINARY ? ctrl[w.cnt + slot] : 1ull;   // (one load for both)
    return (key && flag) ? 0x7fffffff - (int)(unsigned)(key & 0xffffffffull) : -1;
}

// voxel with tile-blob root p (-1: background) belongs to the component of root `best`
__device__ __forceinline__ bool kept(const int* __restrict__ parent, int p, int best) {
    return best >= 0 && p >= 0 && find_plain(parent, p) == best;
}

// the value is read at the roots only
template <class G, Mode M>
__global__ __launch_bounds__(256) void lcc_select_kernel(G geo, const int* __restrict__ parent, const int* __restrict__ area,
                                                         int C, unsigned long long* __restrict__ ctrl) {
    const View g = geo.view();
    Acc<M> a = {};
    geo.select_nodes(g, [&](int i, auto value_off, long) {
        if (parent[i] != i) return;
        if (M == BINARY) {
            acc_add(a, 0, i, area[i]);
            if (!a.cnt[0]) a.cnt[0] = g.v[value_off()] > 0;
        } else {
            const int c = class_of(g.v[value_off()], C);
            if (c) acc_add(a, c - 1, i, area[i]);
        }
    });
    acc_commit(a, M == BINARY ? 1 : C - 1, ctrl, ctrl_words<M>(C));
}

// BINARY: out[i] = 1 where find(i) is the chosen root.  CLASSES: out[i] = the voxel's own value v where v is a class and
// find(i) is the chosen root of that class; stats[k][c][0..2] = components, voxels, voxels of the kept component of class c,
// row 0 zeros (threads 0 .. C - 1 of the case's first block).  0 elsewhere
template <class G, Mode M>
__global__ __launch_bounds__(256) void lcc_write_kernel(G geo, const int* __restrict__ parent, int C,
                                                        const unsigned long long* __restrict__ ctrl,
                                                        unsigned char* __restrict__ out, long long* __restrict__ stats) {
    __shared__ int best[MAXC];
    const Ctrl w = ctrl_words<M>(C);
    const int c = threadIdx.x;
    int only = -1;
    if (M == BINARY) {
        only = chosen_root<M>(ctrl, w, 0);
    } else {
        if (c < MAXC) best[c] = (c >= 1 && c < C) ? chosen_root<M>(ctrl, w, c - 1) : -1;
        if (stats && blockIdx.x == 0 && c < C) {
            long long* st = stats + ((long)blockIdx.y * C + c) * 3;
            st[0] = c ? (long long)ctrl[w.cnt + c - 1] : 0;
            st[1] = c ? (long long)ctrl[w.vox + c - 1] : 0;
            st[2] = c ? (long long)(ctrl[w.key + c - 1] >> 32) : 0;
        }
        __syncthreads();
    }
    const View g = geo.view();
    geo.write_nodes(g, [&](int i, auto value_off, long at) {
        const int p = parent[i];
        int o;
        if (M == BINARY) {
            o = kept(parent, p, only);
        } else {
            const int cv = p >= 0 ? class_of(g.v[value_off()], C) : 0;
            o = (cv && kept(parent, p, best[cv])) ? cv : 0;
        }
        out[at] = (unsigned char)o;
    });
}

// ---- the k largest components with a size floor (aide_keep_components3d; the single volume) ----
// Launches 1 - 3, then one select pass per rank, then write.  Keys are unique per root, so "the first k of the order" is
// "key >= the k-th largest key of the slot": pass 0 is lcc_select_kernel itself (max key, and the flag or the stats sums), pass
// j >= 1 takes per slot the max key strictly below pass j - 1's (0 when the slot has no further root, and 0 from then on).
// Control words: 0 .. 3 MAXC - 1 are pass 0's as ctrl_words lays them out; the keys of pass j >= 1, slot s, are word
// 3 MAXC + (j - 1) MAXC + s.  One memset clears them all.
constexpr int MAXK = 8;
constexpr int KC_WORDS = 3 * MAXC + (MAXK - 1) * MAXC;

// per class value 1 .. C - 1 (BINARY: entry 1): top_k (0: every blob) and min_voxels << 32, a key no smaller blob reaches
struct Rule {
    int k[MAXC];
    unsigned long long floor[MAXC];
};

template <Mode M>
__device__ __forceinline__ long kc_keys(int pass, int C) {
    return pass == 0 ? ctrl_words<M>(C).key : 3 * MAXC + (long)(pass - 1) * MAXC;
}

template <class G, Mode M>                        // M: BINARY or CLASSES
__global__ __launch_bounds__(256) void kc_next_kernel(G geo, const int* __restrict__ parent, const int* __restrict__ area, int C,
                                                      int pass, unsigned long long* __restrict__ ctrl) {
    __shared__ unsigned long long bound[SLOTS<M>];
    const int live = M == BINARY ? 1 : C - 1;
    if ((int)threadIdx.x < live) bound[threadIdx.x] = ctrl[kc_keys<M>(pass - 1, C) + threadIdx.x];
    __syncthreads();
    const View g = geo.view();
    Acc<M> a = {};
    geo.select_nodes(g, [&](int i, auto value_off, long) {
        if (parent[i] != i) return;
        int slot = 0;
        if (M != BINARY) {
            const int c = class_of(g.v[value_off()], C);
            if (!c) return;
            slot = c - 1;
        }
        const unsigned long long key = root_key(i, area[i]);
#pragma unroll
        for (int j = 0; j < SLOTS<M>; ++j)
            if (slot == j && key < bound[j]) a.key[j] = umax64(a.key[j], key);
    });
    acc_commit(a, live, ctrl, Ctrl{kc_keys<M>(pass, C), 0, 0});   // (BINARY: the flag's count stays 0, no atomic for it)
}

// out[i] = 1 (the voxel's class) where key(find(i)) reaches its slot's threshold = max(k-th largest key, floor).  CLASSES
// with stats: rows (blobs, voxels) from pass 0's words by block 0, and every kept root adds its area to the row's third word
// (cleared before the launches): summed over the wave first, one atomic per (wave, class)
template <Mode M>                                 // M: BINARY or CLASSES
__global__ __launch_bounds__(256) void kc_write_kernel(Strided geo, const int* __restrict__ parent, const int* __restrict__ area,
                                                       int C, Rule rule, const unsigned long long* __restrict__ ctrl,
                                                       unsigned char* __restrict__ out, long long* __restrict__ stats) {
    __shared__ unsigned long long thr[MAXC];      // by class value; ~0: nothing of the class is kept
    const int c = threadIdx.x;
    if (c < MAXC) {
        unsigned long long t = ~0ull;
        if (c >= 1 && c < (M == BINARY ? 2 : C)) {
            const int k = rule.k[c];
            t = umax64(k ? ctrl[kc_keys<M>(k - 1, C) + c - 1] : 0ull, rule.floor[c]);
            if (M == BINARY && !ctrl[ctrl_words<M>(C).cnt]) t = ~0ull;      // no positive voxel: nothing
        }
        thr[c] = t;
        if (M != BINARY && stats && blockIdx.x == 0 && c < C) {
            const Ctrl w = ctrl_words<CLASSES_STATS>(C);
            stats[c * 3] = c ? (long long)ctrl[w.cnt + c - 1] : 0;
            stats[c * 3 + 1] = c ? (long long)ctrl[w.vox + c - 1] : 0;
        }
    }
    __syncthreads();
    const View g = geo.view();
    int kc = 0, ka = 0;                           // class and area of a kept root this thread holds
    geo.write_nodes(g, [&](int i, auto value_off, long at) {
        const int p = parent[i];
        int o = 0;
        if (p >= 0) {
            const int cv = M == BINARY ? 1 : class_of(g.v[value_off()], C);
            if (cv) {
                const int r = find_plain(parent, p), ar = area[r];
                if (root_key(r, ar) >= thr[cv]) {
                    o = cv;
                    if (r == i) { kc = cv; ka = ar; }
                }
            }
        }
        out[at] = (unsigned char)o;
    });
    if (M != BINARY && stats && __ballot(kc != 0)) {
        for (int cc = 1; cc < C; ++cc) {
            int s = kc == cc ? ka : 0;
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d);
            if ((threadIdx.x & 63) == 0 && s)
                atomicAdd(reinterpret_cast<unsigned long long*>(stats + cc * 3 + 2), (unsigned long long)s);
        }
    }
}

// ---- hole filling (aide_fill_holes3d; the single volume) ----
// Launches 1 - 3 under Background<T>: the sets are the face-connected blobs of the voxels that are exactly 0 (inside the slices
// along `cut` when there is one).  One 32-bit word per root, cleared by a memset, records what the blob touches:
//   flag   every background voxel ORs into word[find(i)]: bit 0 for a neighbour outside the volume (a face of the volume, or
//          an edge of the slice: the cut axis has no neighbours) or one holding a value outside 0 .. C - 1, bit c for a
//          neighbour of class c.  BINARY (C = 0): bit 0 only, no neighbour is read.  Bits are only ever added, so a word that
//          already shows them needs no atomic
//   write  a stored class keeps its value (BINARY: 1), a value outside 0 .. C - 1 gives 0, a background voxel gets c where its
//          root's word is exactly the one bit c >= 1 (BINARY: 1 where bit 0 is clear).  stats[c] += (1, area) at the root of a
//          filled blob, summed over the wave first
template <typename T>
__global__ __launch_bounds__(256) void holes_flag_kernel(Strided geo, Background<T> bg, const int* __restrict__ parent, int C,
                                                         unsigned* __restrict__ word) {
    const View g = geo.view();
    const unsigned u = blockIdx.x * 256u + threadIdx.x;
    if (u >= (unsigned)(g.d0 * g.d1 * g.d2)) return;
    const int i = (int)u, p = parent[i];
    if (p < 0) return;
    int x[3];
    g.decode(i, x[0], x[1], x[2]);
    const int d[3] = {g.d0, g.d1, g.d2};
    const long st[3] = {g.s0, g.s1, g.s2}, off = g.off(x[0], x[1], x[2]);
    unsigned bits = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (!bg.joins(a)) continue;
#pragma unroll
        for (int sg = -1; sg <= 1; sg += 2) {
            const int y = x[a] + sg;
            if (y < 0 || y >= d[a]) { bits |= 1u; continue; }
            if (C) {
                const long long nv = (long long)bg.raw(g, off + sg * st[a]);
                if (nv != 0) bits |= 1u << class_of(nv, C);       // (out of range: class 0, bit 0)
            }
        }
    }
    if (!bits) return;
    // A plain load: it may return an older value of the word, which holds a subset of the bits it holds now.  The atomic is
    // skipped where that already shows this thread's bits, or a word that no further bit can change the fate of (bit 0, or two
    // bits): the large open blobs stop drawing atomics -- and loads of one L2 line -- early.  What write reads of a word (bit 0,
    // exactly one bit c) is the same under every schedule
    unsigned* wp = word + find_plain(parent, p);
    const unsigned w = *wp;
    if (!(w & 1u) && !(w & (w - 1u)) && (w & bits) != bits) atomicOr(wp, bits);
}

template <typename T>
__global__ __launch_bounds__(256) void holes_write_kernel(Strided geo, Background<T> bg, const int* __restrict__ parent,
                                                          const int* __restrict__ area, int C, const unsigned* __restrict__ word,
                                                          unsigned char* __restrict__ out, long long* __restrict__ stats) {
    const View g = geo.view();
    const unsigned u = blockIdx.x * 256u + threadIdx.x;
    int fc = 0, fa = 0;                           // class and area of a filled blob whose root this thread holds
    if (u < (unsigned)(g.d0 * g.d1 * g.d2)) {
        const int i = (int)u;
        const long long v = (long long)bg.raw(g, g.off_of(i));
        int o;
        if (v != 0) {
            o = C ? class_of(v, C) : 1;
        } else {
            const int r = find_plain(parent, parent[i]);
            const unsigned w = word[r];
            o = C ? ((w > 1u && !(w & (w - 1u))) ? __ffs((int)w) - 1 : 0) : !(w & 1u);
            if (o && r == i) { fc = o; fa = area[i]; }
        }
        out[u] = (unsigned char)o;
    }
    if (stats && __ballot(fc != 0)) {
        const int rows = C ? C : 2;
        for (int cc = 1; cc < rows; ++cc) {
            int h = fc == cc, s = fc == cc ? fa : 0;
#pragma unroll
            for (int dd = 32; dd > 0; dd >>= 1) { h += __shfl_xor(h, dd); s += __shfl_xor(s, dd); }
            if ((threadIdx.x & 63) == 0 && h) {
                atomicAdd(reinterpret_cast<unsigned long long*>(stats + cc * 2), (unsigned long long)h);
                atomicAdd(reinterpret_cast<unsigned long long*>(stats + cc * 2 + 1), (unsigned long long)s);
            }
        }
    }
}

// ---- confusion sums: out[0..3] = N, sum P*T, sum P, sum T (int64, order-independent atomics) ----
// three block sums: thread j < 3 returns the block's j-th total, every other thread 0
__device__ __forceinline__ long long block_sum3(long long s0, long long s1, long long s2) {
    __shared__ long long sm[3][4];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s0 += __shfl_xor(s0, o);
        s1 += __shfl_xor(s1, o);
        s2 += __shfl_xor(s2, o);
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) { sm[0][wid] = s0; sm[1][wid] = s1; sm[2][wid] = s2; }
    __syncthreads();
    if (threadIdx.x >= 3) return 0;
    return sm[threadIdx.x][0] + sm[threadIdx.x][1] + sm[threadIdx.x][2] + sm[threadIdx.x][3];
}

template <typename TP, typename TT>
__global__ __launch_bounds__(256) void confusion_kernel(Operand P, Operand T, int d1, int d2, int n,
                                                        long long* __restrict__ out) {
    long long spt = 0, sp = 0, st = 0;
    for (unsigned u = blockIdx.x * 256u + threadIdx.x; u < (unsigned)n; u += gridDim.x * 256u) {
        int i0, i1, i2;
        raster_decode((int)u, d1, d2, i0, i1, i2);
        const long long a = P.at<TP>(P.off(i0, i1, i2)), b = T.at<TT>(T.off(i0, i1, i2));
        spt += a * b; sp += a; st += b;
    }
    const long long s = block_sum3(spt, sp, st);
    if (threadIdx.x < 3) atomicAdd(reinterpret_cast<unsigned long long*>(out + 1 + threadIdx.x), (unsigned long long)s);
    if (blockIdx.x == 0 && threadIdx.x == 3) atomicAdd(reinterpret_cast<unsigned long long*>(out), (unsigned long long)n);
}

// out[k][0..3] = N, sum p*t, sum p, sum t with t = (target byte == match); VEC: 16 bytes per load (hw % 16 == 0, aligned)
template <bool VEC>
__global__ __launch_bounds__(256) void confusion_batched_kernel(const unsigned char* __restrict__ p,
                                                                const unsigned char* __restrict__ tg,
                                                                const long long* __restrict__ start, int S_total, long hw,
                                                                int match, long long* __restrict__ out) {
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
    const long long s = block_sum3(spt, sp, st);
    if (threadIdx.x < 3 && s) atomicAdd(reinterpret_cast<unsigned long long*>(out + 4 * k + 1 + threadIdx.x), (unsigned long long)s);
    if (blockIdx.x == 0 && threadIdx.x == 3) out[4 * k] = n;
}

// ---- labelled components (aide_label_components3d; the single volume) ----
// After launches 1 - 3 under Equal every non-zero voxel has a root and every root its area.  A root is a MEMBER root when its
// value is a member (C = 0: any non-zero value; C >= 2: a class 1 .. C - 1): the blobs of other values exist in `parent` and
// get label 0.  The rank launches work on blocks of SCAN nodes: 256 threads x 4 nodes, node = block * SCAN + k * 256 + thread,
// so the order inside a block is (k, wave, lane).
constexpr int SCAN = 1024;
constexpr int PROPS = 12;                         // value, area, first, min0..2, max0..2 + 1, sum0..2

__device__ __forceinline__ long long node_value(const View& g, int i) { return g.v[g.off_of(i)]; }

// 0: node u is no root (or lies past the volume), 1: a member root, -1: the root of a blob of another value
__device__ __forceinline__ int root_kind(const View& g, const int* __restrict__ parent, unsigned u, unsigned n, int C) {
    if (u >= n || parent[u] != (int)u) return 0;
    if (!C) return 1;
    return class_of(node_value(g, (int)u), C) ? 1 : -1;
}

// 4 flag: blockcnt[b] = member roots among the block's SCAN nodes
__global__ __launch_bounds__(256) void lab_flag_kernel(Strided geo, const int* __restrict__ parent, int C,
                                                       int* __restrict__ blockcnt) {
    __shared__ int sm[4];
    const View g = geo.view();
    const unsigned n = (unsigned)(g.d0 * g.d1 * g.d2);
    int c = 0;
#pragma unroll
    for (int k = 0; k < SCAN / 256; ++k)
        c += root_kind(g, parent, blockIdx.x * (unsigned)SCAN + k * 256u + threadIdx.x, n, C) == 1;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) blockcnt[blockIdx.x] = sm[0] + sm[1] + sm[2] + sm[3];
}

// 5 scan: ONE workgroup turns the nb block counts into exclusive offsets in place, SCAN_T of them per trip with the running
// total carried in a register, and writes the number of blobs.  (a total is at most the voxel count < 2^31)
constexpr int SCAN_T = 1024;
__global__ __launch_bounds__(SCAN_T) void lab_scan_kernel(int* __restrict__ blockcnt, int nb, long long* __restrict__ count) {
    __shared__ int wsum[SCAN_T / 64];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    int carry = 0;
    for (int o = 0; o < nb; o += SCAN_T) {        // uniform trip count
        const int j = o + (int)threadIdx.x;
        const int c = j < nb ? blockcnt[j] : 0;
        int s = c;                                // inclusive scan of the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int t = __shfl_up(s, d);
            if (lane >= d) s += t;
        }
        if (lane == 63) wsum[wid] = s;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < SCAN_T / 64; ++w) {
            const int x = wsum[w];
            before += w < wid ? x : 0;
            total += x;
        }
        if (j < nb) blockcnt[j] = carry + before + s - c;
        carry += total;
        __syncthreads();                          // wsum is written again
    }
    if (threadIdx.x == 0) count[0] = carry;
}

// 6 rank: rank[i] = the block's offset + the member roots of the block in front of i, at every member root; -1 at the root of
// any other blob (no other node's word is ever read).  Blob j < cap gets its props row from its root's own thread: value, area,
// first index, and the box and the sums of the first voxel alone -- write adds the other voxels
__global__ __launch_bounds__(256) void lab_rank_kernel(Strided geo, const int* __restrict__ parent, const int* __restrict__ area,
                                                       int C, const int* __restrict__ blockoff, int* __restrict__ rank,
                                                       long long* __restrict__ props, int cap) {
    __shared__ int tot[SCAN / 256][4];
    const View g = geo.view();
    const unsigned n = (unsigned)(g.d0 * g.d1 * g.d2);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    int kind[SCAN / 256], pre[SCAN / 256], base[SCAN / 256];
#pragma unroll
    for (int k = 0; k < SCAN / 256; ++k) {
        kind[k] = root_kind(g, parent, blockIdx.x * (unsigned)SCAN + k * 256u + threadIdx.x, n, C);
        const unsigned long long b = __ballot(kind[k] == 1);
        pre[k] = __popcll(b & ((1ull << lane) - 1ull));
        if (lane == 0) tot[k][wid] = __popcll(b);
    }
    __syncthreads();
    int run = blockoff[blockIdx.x];
#pragma unroll
    for (int k = 0; k < SCAN / 256; ++k)
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            if (w == wid) base[k] = run;
            run += tot[k][w];
        }
#pragma unroll
    for (int k = 0; k < SCAN / 256; ++k) {
        if (kind[k] == 0) continue;
        const int i = (int)(blockIdx.x * (unsigned)SCAN + k * 256u + threadIdx.x);
        const int j = kind[k] == 1 ? base[k] + pre[k] : -1;
        rank[i] = j;
        if (props && j >= 0 && j < cap) {
            int i0, i1, i2;
            g.decode(i, i0, i1, i2);
            long long* row = props + (long)j * PROPS;
            row[0] = g.v[g.off(i0, i1, i2)]; row[1] = area[i]; row[2] = i;
            row[3] = i0; row[4] = i1; row[5] = i2;
            row[6] = i0 + 1; row[7] = i1 + 1; row[8] = i2 + 1;
            row[9] = i0; row[10] = i1; row[11] = i2;
        }
    }
}

// 7 write: labels[i] = rank(find(i)) + 1 (0: no member), WRITE_K x 256 consecutive nodes per block.  Props: every voxel but
// the first of a blob below the cap goes into its row, through a table of TBL slots in LDS per block.  Slot j % TBL belongs to
// the LOWEST blob number j the block holds there: the first pass over the nodes settles that with atomicMin (after a plain
// read: the word only decreases, so a value already at or below j needs no atomic) and keeps every voxel's blob in LDS.  The
// second pass, after a barrier: lanes of a wave that share a blob are reduced first (whole waves, as in count), and the leader
// adds the wave's part to the blob's slot, or straight to the row where another blob owns the slot.  The slots go to the rows
// at the end: one set of global atomics per (block, blob) for the owners, per (wave, blob) for the others.  Every part is a
// min, a max or a sum of integers: the same bytes whichever way a part takes
constexpr int WRITE_K = 16, TBL = 128;

// a part of blob j goes to its row: the six box words are lowered / raised after a plain load -- it may return an older
// value, which is no tighter than the word is now, so a coordinate inside it needs no atomic -- and the three sums added
__device__ __forceinline__ void props_commit(unsigned long long* __restrict__ props, int j, int lo0, int lo1, int lo2, int hi0,
                                             int hi1, int hi2, unsigned long long s0, unsigned long long s1,
                                             unsigned long long s2) {
    unsigned long long* row = props + (long)j * PROPS;
    if ((unsigned long long)lo0 < row[3]) atomicMin(row + 3, (unsigned long long)lo0);
    if ((unsigned long long)lo1 < row[4]) atomicMin(row + 4, (unsigned long long)lo1);
    if ((unsigned long long)lo2 < row[5]) atomicMin(row + 5, (unsigned long long)lo2);
    if ((unsigned long long)hi0 > row[6]) atomicMax(row + 6, (unsigned long long)hi0);
    if ((unsigned long long)hi1 > row[7]) atomicMax(row + 7, (unsigned long long)hi1);
    if ((unsigned long long)hi2 > row[8]) atomicMax(row + 8, (unsigned long long)hi2);
    atomicAdd(row + 9, s0);
    atomicAdd(row + 10, s1);
    atomicAdd(row + 11, s2);
}

__global__ __launch_bounds__(256) void lab_write_kernel(Strided geo, const int* __restrict__ parent, const int* __restrict__ rank,
                                                        int* __restrict__ labels, unsigned long long* __restrict__ props, int cap) {
    __shared__ int key[TBL];                      // the blob that owns the slot, INT32_MAX: none
    __shared__ int box[6][TBL];
    __shared__ unsigned long long sum[3][TBL];
    __shared__ int blob[WRITE_K][256];            // the blob a voxel adds to, -1: none
    const View g = geo.view();
    const unsigned n = (unsigned)(g.d0 * g.d1 * g.d2);
    const int lane = threadIdx.x & 63;
    if (props) {
        if (threadIdx.x < TBL) {
            const int e = threadIdx.x;
            key[e] = INT32_MAX;
            box[0][e] = box[1][e] = box[2][e] = INT32_MAX;
            box[3][e] = box[4][e] = box[5][e] = 0;
            sum[0][e] = sum[1][e] = sum[2][e] = 0ull;
        }
        __syncthreads();
    }
    for (int k = 0; k < WRITE_K; ++k) {
        const unsigned u = (blockIdx.x * (unsigned)WRITE_K + k) * 256u + threadIdx.x;
        const int i = (int)u;
        int j = -1, r = -1;
        if (u < n) {
            const int p = parent[i];
            if (p >= 0) {
                r = find_plain(parent, p);
                j = rank[r];
            }
            labels[i] = j + 1;
        }
        if (!props) continue;
        const bool add = j >= 0 && j < cap && r != i;
        blob[k][threadIdx.x] = add ? j : -1;
        if (add) {
            volatile int* owner = &key[j & (TBL - 1)];
            if (*owner > j) atomicMin(&key[j & (TBL - 1)], j);
        }
    }
    if (!props) return;
    __syncthreads();
    for (int k = 0; k < WRITE_K; ++k) {
        const int j = blob[k][threadIdx.x];
        const bool add = j >= 0;
        unsigned long long pending = __ballot(add);
        if (!pending) continue;
        int x0 = 0, x1 = 0, x2 = 0;
        if (add) g.decode((int)((blockIdx.x * (unsigned)WRITE_K + k) * 256u + threadIdx.x), x0, x1, x2);
        while (pending) {
            const int leader = __ffsll((long long)pending) - 1;
            const int jl = __shfl(j, leader);
            const bool mine = add && j == jl;
            int lo0 = mine ? x0 : INT32_MAX, lo1 = mine ? x1 : INT32_MAX, lo2 = mine ? x2 : INT32_MAX;
            int hi0 = mine ? x0 + 1 : 0, hi1 = mine ? x1 + 1 : 0, hi2 = mine ? x2 + 1 : 0;
            long long s0 = mine ? x0 : 0, s1 = mine ? x1 : 0, s2 = mine ? x2 : 0;
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) {
                lo0 = min(lo0, __shfl_xor(lo0, d)); lo1 = min(lo1, __shfl_xor(lo1, d)); lo2 = min(lo2, __shfl_xor(lo2, d));
                hi0 = max(hi0, __shfl_xor(hi0, d)); hi1 = max(hi1, __shfl_xor(hi1, d)); hi2 = max(hi2, __shfl_xor(hi2, d));
                s0 += __shfl_xor(s0, d); s1 += __shfl_xor(s1, d); s2 += __shfl_xor(s2, d);
            }
            if (lane == leader) {
                const int slot = jl & (TBL - 1);
                if (key[slot] == jl) {
                    atomicMin(&box[0][slot], lo0); atomicMin(&box[1][slot], lo1); atomicMin(&box[2][slot], lo2);
                    atomicMax(&box[3][slot], hi0); atomicMax(&box[4][slot], hi1); atomicMax(&box[5][slot], hi2);
                    atomicAdd(&sum[0][slot], (unsigned long long)s0);
                    atomicAdd(&sum[1][slot], (unsigned long long)s1);
                    atomicAdd(&sum[2][slot], (unsigned long long)s2);
                } else {
                    props_commit(props, jl, lo0, lo1, lo2, hi0, hi1, hi2, (unsigned long long)s0, (unsigned long long)s1,
                                 (unsigned long long)s2);
                }
            }
            pending &= ~__ballot(mine);
        }
    }
    __syncthreads();
    if (threadIdx.x < TBL && key[threadIdx.x] != INT32_MAX) {
        const int e = threadIdx.x;
        props_commit(props, key[e], box[0][e], box[1][e], box[2][e], box[3][e], box[4][e], box[5][e], sum[0][e], sum[1][e],
                     sum[2][e]);
    }
}

// ---- lesion counts (aide_lesion_counts3d; the single volume) ----
// After launches 1 - 3 on A.  cover: a voxel of A at which B agrees (C = 0: B != 0; C >= 2: A's value is a class and B holds
// it too) adds 1 to cover[find(i)].  COVER_K x 256 consecutive nodes per block and the table scheme of the labels' write launch:
// slot r % TBL of a table in LDS belongs to the lowest root r the block holds there (atomicMin in the first pass, which keeps
// every voxel's root in LDS); in the second pass the lanes of a wave with the same root are counted with one ballot and the
// leader adds the count to the root's slot, or straight to cover[r] where another root owns the slot; the slots go to cover at
// the end: one global atomicAdd per (block, root) for the owners, per (wave, root) for the others
constexpr int COVER_K = 16;
__global__ __launch_bounds__(256) void les_cover_kernel(Strided geo, Operand B, const int* __restrict__ parent, int C,
                                                        int* __restrict__ cover) {
    __shared__ int key[TBL];                      // the root that owns the slot, INT32_MAX: none
    __shared__ int cnt[TBL];
    __shared__ int root[COVER_K][256];            // the root a voxel adds to, -1: none
    const View g = geo.view();
    const unsigned n = (unsigned)(g.d0 * g.d1 * g.d2);
    const int lane = threadIdx.x & 63;
    if (threadIdx.x < TBL) { key[threadIdx.x] = INT32_MAX; cnt[threadIdx.x] = 0; }
    __syncthreads();
    for (int k = 0; k < COVER_K; ++k) {
        const unsigned u = (blockIdx.x * (unsigned)COVER_K + k) * 256u + threadIdx.x;
        int r = -1;
        if (u < n) {
            const int i = (int)u, p = parent[i];
            if (p >= 0) {
                int i0, i1, i2;
                g.decode(i, i0, i1, i2);
                const long long b = B.at<long long>(B.off(i0, i1, i2));
                bool agree = b != 0;
                if (C) {
                    const long long a = g.v[g.off(i0, i1, i2)];
                    agree = class_of(a, C) != 0 && b == a;
                }
                if (agree) r = find_plain(parent, p);
            }
        }
        root[k][threadIdx.x] = r;
        if (r >= 0) {
            volatile int* owner = &key[r & (TBL - 1)];
            if (*owner > r) atomicMin(&key[r & (TBL - 1)], r);
        }
    }
    __syncthreads();
    for (int k = 0; k < COVER_K; ++k) {
        const int r = root[k][threadIdx.x];
        unsigned long long pending = __ballot(r >= 0);
        while (pending) {
            const int leader = __ffsll((long long)pending) - 1;
            const int rl = __shfl(r, leader);
            const unsigned long long same = __ballot(r == rl);
            if (lane == leader) {
                const int slot = rl & (TBL - 1);
                if (key[slot] == rl) atomicAdd(&cnt[slot], __popcll(same));
                else atomicAdd(cover + rl, __popcll(same));
            }
            pending &= ~same;
        }
    }
    __syncthreads();
    if (threadIdx.x < TBL && key[threadIdx.x] != INT32_MAX) atomicAdd(cover + key[threadIdx.x], cnt[threadIdx.x]);
}

// reduce: the member roots of A into the columns of its side, per class row (C = 0: row 1).  side 0, A = target: blobs ->
// column 0, blobs that count -> 1, cover -> 4.  side 1, A = pred: blobs -> 2, blobs that count -> 3, the area of the blobs that
// do not count -> 5.  A blob counts when cover >= 1 and double(cover) >= overlap * double(area).  Roots are rare: LDS atomics
// per root, then one global atomicAdd per (block, word) that is not zero
__global__ __launch_bounds__(256) void les_reduce_kernel(Strided geo, const int* __restrict__ parent, const int* __restrict__ area,
                                                         const int* __restrict__ cover, int C, double overlap, int side,
                                                         long long* __restrict__ out) {
    __shared__ unsigned long long acc[MAXC][4];   // blobs, blobs that count, cover, area of the blobs that do not count
    if (threadIdx.x < MAXC * 4) (&acc[0][0])[threadIdx.x] = 0ull;
    __syncthreads();
    const View g = geo.view();
    geo.select_nodes(g, [&](int i, auto value_off, long) {
        if (parent[i] != i) return;
        int c = 1;
        if (C) {
            c = class_of(g.v[value_off()], C);
            if (!c) return;
        }
        const int ar = area[i], cv = cover[i];
        const bool counts = cv >= 1 && (double)cv >= overlap * (double)ar;
        atomicAdd(&acc[c][0], 1ull);
        if (counts) atomicAdd(&acc[c][1], 1ull);
        if (cv) atomicAdd(&acc[c][2], (unsigned long long)cv);
        if (!counts) atomicAdd(&acc[c][3], (unsigned long long)ar);
    });
    __syncthreads();
    if (threadIdx.x < MAXC * 4) {
        const int c = threadIdx.x >> 2, k = threadIdx.x & 3;
        const int col = side == 0 ? (k == 0 ? 0 : k == 1 ? 1 : k == 2 ? 4 : -1) : (k == 0 ? 2 : k == 1 ? 3 : k == 3 ? 5 : -1);
        const unsigned long long v = acc[c][k];
        if (v && col >= 0) atomicAdd(reinterpret_cast<unsigned long long*>(out + c * 6 + col), v);
    }
}

// ---- host ----
// [S_total][H][W] with K cases: everything the grids and the node indices need fits an int
bool batch_ok(int64_t S_total, int64_t H, int64_t W, int64_t K) {
    if (S_total < 0 || H < 0 || W < 0 || K < 0 || K > 65535) return false;
    return dims_ok(S_total, H, W);
}

bool classes_ok(int C) { return C >= 2 && C <= MAXC; }

// workspace: parent[n], area[n], then, 16-byte aligned, K groups of control words
size_t ws_bytes(int64_t nvox, int64_t K, int64_t words_per_case) {
    if (nvox < 0 || nvox > INT32_MAX || K < 0 || K > 65535) return 0;
    return (size_t)(2 * nvox) * sizeof(int) + 16 + (size_t)(K * words_per_case) * sizeof(unsigned long long);
}

struct Grids { dim3 tile, count, select, write; };   // launches 1 - 2, 3, 4, 5

Strided make_strided(const long long* v, int64_t d0, int64_t d1, int64_t d2, int64_t s0, int64_t s1, int64_t s2, Grids& gr) {
    Strided geo;
    geo.g = View{v, (long)s0, (long)s1, (long)s2, (int)d0, (int)d1, (int)d2, 0};
    geo.t1 = (int)((d1 + TQ - 1) / TQ); geo.t2 = (int)((d2 + TQ - 1) / TQ);
    geo.tiles = (int)((long)geo.t1 * geo.t2 * ((d0 + TZ - 1) / TZ));   // (<= the number of voxels)
    const long nb = (d0 * d1 * d2 + 255) / 256;
    gr.tile = dim3((unsigned)min((long)geo.tiles, 65536L));
    gr.count = gr.write = dim3((unsigned)nb);
    gr.select = dim3((unsigned)min(nb, 1024L));
    return geo;
}

Ragged make_ragged(const long long* v, const long long* slice_start, int64_t K, int64_t S_total, int64_t H, int64_t W,
                   Grids& gr) {
    Ragged geo;
    geo.v = v; geo.start = slice_start; geo.S_total = (int)S_total; geo.H = (int)H; geo.W = (int)W;
    geo.tw = (int)((W + 15) / 16);
    const long tiles = (long)geo.tw * ((H + 15) / 16), chunks = (H * W + 255) / 256;   // (tiles < H W / 256 + (H + W) / 16 + 2)
    gr.tile = dim3((unsigned)tiles, (unsigned)K);
    gr.count = gr.select = gr.write = dim3((unsigned)chunks, (unsigned)K);
    return geo;
}

// launches 1 - 3 under a connectivity predicate: every node gets a root, every root its area
template <class G, class P>
void label_launch(const G& geo, const P& pred, const Grids& gr, double bytes, int* parent, int* area, unsigned long long* ctrl,
                  hipStream_t stream) {
    const dim3 block(256);
    AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, bytes, (lcc_local_kernel<G, P>), gr.tile, block, 0, stream, geo, pred, parent, area, ctrl);
    AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 0.0, (lcc_border_kernel<G, P>), gr.tile, block, 0, stream, geo, pred, parent);
    AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 0.0, lcc_count_kernel<G>, gr.count, block, 0, stream, geo, parent, area);
}

// the five launches over n nodes and K cases; C = 0: BINARY, else the per-class form with one memset in front
template <class G>
int lcc_launch(const G& geo, const Grids& gr, int n, int64_t K, int C, unsigned char* out, long long* stats, void* ws,
               hipStream_t stream) {
    if ((reinterpret_cast<uintptr_t>(ws) & 15) != 0) return AIDE_ERR_ARG;
    Carver carver(ws);
    int* parent = carver.take<int>(2 * (size_t)n);
    int* area = parent + n;
    unsigned long long* ctrl = carver.take<unsigned long long>(0);
    const int* cparent = parent;
    const int* carea = area;
    const unsigned long long* cctrl = ctrl;
    const dim3 block(256);
    if (C) {
        hipError_t e = hipMemsetAsync(ctrl, 0, (size_t)(3 * K * C) * sizeof(unsigned long long), stream);
        if (e != hipSuccess) return (int)e;
    }
    const double bytes = 29.0 * n;   // algorithmic traffic: V 8 + parent / area 4 + 4 (local), count 4, select 4, write 4 + 1
    label_launch(geo, Equal{}, gr, bytes, parent, area, ctrl, stream);
    if (!C)
        AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 0.0, (lcc_select_kernel<G, BINARY>), gr.select, block, 0, stream, geo, cparent, carea, C, ctrl);
    else if (stats)
        AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 0.0, (lcc_select_kernel<G, CLASSES_STATS>), gr.select, block, 0, stream, geo, cparent, carea, C, ctrl);
    else
        AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 0.0, (lcc_select_kernel<G, CLASSES>), gr.select, block, 0, stream, geo, cparent, carea, C, ctrl);
    if (!C)
        AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 0.0, (lcc_write_kernel<G, BINARY>), gr.write, block, 0, stream, geo, cparent, C, cctrl, out, stats);
    else
        AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 0.0, (lcc_write_kernel<G, CLASSES>), gr.write, block, 0, stream, geo, cparent, C, cctrl, out, stats);
    return aide_launch_status();
}

// the workspace of the single-volume forms below: parent[n], area[n], then, 16-byte aligned, the control words
struct Carved {
    int *parent, *area;
    unsigned long long* ctrl;
};
Carved carve(void* ws, int n) {
    Carver c(ws);
    int* parent = c.take<int>(2 * (size_t)n);
    return Carved{parent, parent + n, c.take<unsigned long long>(0)};
}

// k largest with a floor: memset(s), launches 1 - 3, `passes` select passes, write; C = 0: BINARY
int kc_launch(const Strided& geo, const Grids& gr, int n, int C, const Rule& rule, int passes, unsigned char* out,
              long long* stats, void* ws, hipStream_t stream) {
    const Carved w = carve(ws, n);
    const int* cparent = w.parent;
    const int* carea = w.area;
    const unsigned long long* cctrl = w.ctrl;
    const dim3 block(256);
    hipError_t e = hipMemsetAsync(w.ctrl, 0, KC_WORDS * sizeof(unsigned long long), stream);
    if (e == hipSuccess && stats) e = hipMemsetAsync(stats, 0, (size_t)(3 * C) * sizeof(long long), stream);
    if (e != hipSuccess) return (int)e;
    label_launch(geo, Equal{}, gr, (25.0 + 4.0 * passes) * n, w.parent, w.area, w.ctrl, stream);
    if (!C)
        AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 0.0, (lcc_select_kernel<Strided, BINARY>), gr.select, block, 0, stream, geo, cparent, carea, C, w.ctrl);
    else if (stats)
        AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 0.0, (lcc_select_kernel<Strided, CLASSES_STATS>), gr.select, block, 0, stream, geo, cparent, carea, C, w.ctrl);
    else
        AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 0.0, (lcc_select_kernel<Strided, CLASSES>), gr.select, block, 0, stream, geo, cparent, carea, C, w.ctrl);
    for (int pass = 1; pass < passes; ++pass) {
        if (!C)
            AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 0.0, (kc_next_kernel<Strided, BINARY>), gr.select, block, 0, stream, geo, cparent, carea, C, pass, w.ctrl);
        else
            AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 0.0, (kc_next_kernel<Strided, CLASSES>), gr.select, block, 0, stream, geo, cparent, carea, C, pass, w.ctrl);
    }
    if (!C)
        AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 0.0, kc_write_kernel<BINARY>, gr.write, block, 0, stream, geo, cparent, carea, C, rule, cctrl, out, stats);
    else
        AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 0.0, kc_write_kernel<CLASSES>, gr.write, block, 0, stream, geo, cparent, carea, C, rule, cctrl, out, stats);
    return aide_launch_status();
}

// hole filling: the root words live behind the two control words launch 1 clears.  memset(s), launches 1 - 3 on the
// background, flag, write
template <typename T>
int holes_launch(const Strided& geo, const Grids& gr, int n, int C, int cut, unsigned char* out, long long* stats, void* ws,
                 hipStream_t stream) {
    const Carved w = carve(ws, n);
    unsigned* word = reinterpret_cast<unsigned*>(w.ctrl + 2);
    const int* cparent = w.parent;
    const int* carea = w.area;
    const unsigned* cword = word;
    const dim3 block(256);
    hipError_t e = hipMemsetAsync(word, 0, (size_t)n * sizeof(unsigned), stream);
    if (e == hipSuccess && stats) e = hipMemsetAsync(stats, 0, (size_t)(2 * (C ? C : 2)) * sizeof(long long), stream);
    if (e != hipSuccess) return (int)e;
    const Background<T> bg{cut};
    label_launch(geo, bg, gr, (30.0 + 2.0 * sizeof(T)) * n, w.parent, w.area, w.ctrl, stream);
    AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 0.0, holes_flag_kernel<T>, gr.write, block, 0, stream, geo, bg, cparent, C, word);
    AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 0.0, holes_write_kernel<T>, gr.write, block, 0, stream, geo, bg, cparent, carea, C, cword, out, stats);
    return aide_launch_status();
}

// workspace of the two pipelines below: three int words per voxel (parent, area, and rank or cover), then, 16-byte aligned, the
// two control words launch 1 clears and (labels) one int per block of SCAN nodes
struct Carved3 {
    int *parent, *area, *third;
    unsigned long long* ctrl;
    int* blockcnt;
};
Carved3 carve3(void* ws, int n) {
    Carver c(ws);
    int* parent = c.take<int>(3 * (size_t)n);
    unsigned long long* ctrl = c.take<unsigned long long>(2);
    return Carved3{parent, parent + n, parent + 2 * (size_t)n, ctrl, reinterpret_cast<int*>(ctrl + 2)};
}
size_t ws3_bytes(int64_t nvox, bool blocks) {
    if (nvox < 0 || nvox > INT32_MAX) return 0;
    return (size_t)(3 * nvox) * sizeof(int) + 16 + 2 * sizeof(unsigned long long) +
           (blocks ? (size_t)((nvox + SCAN - 1) / SCAN) * sizeof(int) : 0);
}

constexpr int64_t MAX_BLOBS = 1 << 20;

// labelled components: [memset of props,] launches 1 - 3, flag, scan, rank, write
int label_components_launch(const Strided& geo, const Grids& gr, int n, int C, int* labels, long long* count, long long* props,
                            int cap, void* ws, hipStream_t stream) {
    const Carved3 w = carve3(ws, n);
    const int* cparent = w.parent;
    const int* carea = w.area;
    const int* crank = w.third;
    const int* coff = w.blockcnt;
    const int nb = (int)(((long)n + SCAN - 1) / SCAN);
    const dim3 block(256), scan_grid((unsigned)nb);
    if (props) {
        hipError_t e = hipMemsetAsync(props, 0, (size_t)cap * PROPS * sizeof(long long), stream);
        if (e != hipSuccess) return (int)e;
    }
    // algorithmic traffic: V 8 + parent / area 4 + 4 (local), count 4, flag 4, rank 4, write 4 + 4 + 4
    label_launch(geo, Equal{}, gr, 40.0 * n, w.parent, w.area, w.ctrl, stream);
    AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 0.0, lab_flag_kernel, scan_grid, block, 0, stream, geo, cparent, C, w.blockcnt);
    AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 0.0, lab_scan_kernel, dim3(1), dim3(SCAN_T), 0, stream, w.blockcnt, nb, count);
    AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 0.0, lab_rank_kernel, scan_grid, block, 0, stream, geo, cparent, carea, C, coff, w.third, props, cap);
    const dim3 write_grid((unsigned)(((long)n + WRITE_K * 256 - 1) / (WRITE_K * 256)));
    AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 0.0, lab_write_kernel, write_grid, block, 0, stream, geo, cparent, crank, labels,
                      reinterpret_cast<unsigned long long*>(props), cap);
    return aide_launch_status();
}

// lesion counts of one side: memset of cover, launches 1 - 3 on A, cover, reduce
int lesion_side_launch(const Strided& geo, const Grids& gr, const Operand& other, int n, int C, double overlap, int side,
                       long long* out, void* ws, hipStream_t stream) {
    const Carved3 w = carve3(ws, n);
    const int* cparent = w.parent;
    const int* carea = w.area;
    const int* ccover = w.third;
    const dim3 block(256);
    hipError_t e = hipMemsetAsync(w.third, 0, (size_t)n * sizeof(int), stream);
    if (e != hipSuccess) return (int)e;
    // algorithmic traffic: V 8 + parent / area 4 + 4 (local), count 4, cover 4 + 8 (+ 8 with classes), reduce 4
    label_launch(geo, Equal{}, gr, (C ? 44.0 : 36.0) * n, w.parent, w.area, w.ctrl, stream);
    const dim3 cover_grid((unsigned)(((long)n + COVER_K * 256 - 1) / (COVER_K * 256)));
    AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 0.0, les_cover_kernel, cover_grid, block, 0, stream, geo, other, cparent, C, w.third);
    AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 0.0, les_reduce_kernel, gr.select, block, 0, stream, geo, cparent, carea, ccover, C, overlap,
                      side, out);
    return aide_launch_status();
}

}  // namespace

extern "C" {

size_t aide_label_components3d_ws_bytes(int64_t nvox) { return ws3_bytes(nvox, true); }

int aide_label_components3d(const long long* v, int64_t d0, int64_t d1, int64_t d2, int64_t s0, int64_t s1, int64_t s2,
                            int num_classes, int* labels, long long* count, long long* props, int64_t max_blobs, void* ws,
                            hipStream_t stream) {
    if ((num_classes != 0 && !classes_ok(num_classes)) || !dims_ok(d0, d1, d2) || !count) return AIDE_ERR_ARG;
    if (props && (max_blobs < 1 || max_blobs > MAX_BLOBS)) return AIDE_ERR_ARG;
    const int n = (int)(d0 * d1 * d2);
    if (n == 0) {
        hipError_t e = hipMemsetAsync(count, 0, sizeof(long long), stream);
        if (e == hipSuccess && props) e = hipMemsetAsync(props, 0, (size_t)max_blobs * PROPS * sizeof(long long), stream);
        return (int)e;
    }
    if (!v || !labels || !ws || (reinterpret_cast<uintptr_t>(ws) & 15) != 0) return AIDE_ERR_ARG;
    Grids gr;
    const Strided geo = make_strided(v, d0, d1, d2, s0, s1, s2, gr);
    return label_components_launch(geo, gr, n, num_classes, labels, count, props, props ? (int)max_blobs : 0, ws, stream);
}

size_t aide_lesion_counts3d_ws_bytes(int64_t nvox) { return ws3_bytes(nvox, false); }

int aide_lesion_counts3d(const long long* pred, int64_t p_s0, int64_t p_s1, int64_t p_s2, const long long* target, int64_t t_s0,
                         int64_t t_s1, int64_t t_s2, int64_t d0, int64_t d1, int64_t d2, int num_classes, double overlap,
                         long long* out, void* ws, hipStream_t stream) {
    if ((num_classes != 0 && !classes_ok(num_classes)) || !dims_ok(d0, d1, d2) || !out) return AIDE_ERR_ARG;
    if (!(overlap >= 0.0 && overlap <= 1.0)) return AIDE_ERR_ARG;   // (also a NaN)
    const int n = (int)(d0 * d1 * d2);
    if (n > 0 && (!pred || !target || !ws || (reinterpret_cast<uintptr_t>(ws) & 15) != 0)) return AIDE_ERR_ARG;
    hipError_t e = hipMemsetAsync(out, 0, (size_t)(6 * (num_classes ? num_classes : 2)) * sizeof(long long), stream);
    if (e != hipSuccess) return (int)e;
    if (n == 0) return 0;
    Grids gr;
    const Strided tgeo = make_strided(target, d0, d1, d2, t_s0, t_s1, t_s2, gr);
    const Operand P{pred, (long)p_s0, (long)p_s1, (long)p_s2, 0}, T{target, (long)t_s0, (long)t_s1, (long)t_s2, 0};
    if (int rc = lesion_side_launch(tgeo, gr, P, n, num_classes, overlap, 0, out, ws, stream)) return rc;
    const Strided pgeo = make_strided(pred, d0, d1, d2, p_s0, p_s1, p_s2, gr);
    return lesion_side_launch(pgeo, gr, T, n, num_classes, overlap, 1, out, ws, stream);
}

size_t aide_components3d_ws_bytes(int64_t nvox) { return ws_bytes(nvox, 1, KC_WORDS); }

int aide_keep_components3d(const long long* v, int64_t d0, int64_t d1, int64_t d2, int64_t s0, int64_t s1, int64_t s2,
                           int num_classes, const int* top_k, const long long* min_voxels, unsigned char* out, long long* stats,
                           void* ws, hipStream_t stream) {
    if ((num_classes != 0 && !classes_ok(num_classes)) || !dims_ok(d0, d1, d2) || !top_k || !min_voxels) return AIDE_ERR_ARG;
    if (stats && !num_classes) return AIDE_ERR_ARG;
    Rule rule = {};
    int passes = 1;
    for (int c = 1; c < (num_classes ? num_classes : 2); ++c) {
        if (top_k[c] < 0 || top_k[c] > MAXK || min_voxels[c] < 1) return AIDE_ERR_ARG;
        rule.k[c] = top_k[c];
        rule.floor[c] = (unsigned long long)std::min(min_voxels[c], 1ll << 31) << 32;   // (no blob has 2^31 voxels)
        passes = std::max(passes, top_k[c]);
    }
    const int n = (int)(d0 * d1 * d2);
    if (n == 0) {
        if (!stats) return 0;
        return (int)hipMemsetAsync(stats, 0, (size_t)(3 * num_classes) * sizeof(long long), stream);
    }
    if (!v || !out || !ws || (reinterpret_cast<uintptr_t>(ws) & 15) != 0) return AIDE_ERR_ARG;
    Grids gr;
    const Strided geo = make_strided(v, d0, d1, d2, s0, s1, s2, gr);
    return kc_launch(geo, gr, n, num_classes, rule, passes, out, stats, ws, stream);
}

size_t aide_fill_holes3d_ws_bytes(int64_t nvox) {
    const size_t base = ws_bytes(nvox, 1, 2);
    return base ? base + (size_t)nvox * sizeof(unsigned) : 0;
}

int aide_fill_holes3d(const void* v, int v_u8, int64_t d0, int64_t d1, int64_t d2, int64_t s0, int64_t s1, int64_t s2,
                      int num_classes, int slice_axis, unsigned char* out, long long* stats, void* ws, hipStream_t stream) {
    if ((num_classes != 0 && !classes_ok(num_classes)) || !dims_ok(d0, d1, d2) || (v_u8 != 0 && v_u8 != 1) || slice_axis < -1 ||
        slice_axis > 2)
        return AIDE_ERR_ARG;
    const int n = (int)(d0 * d1 * d2);
    if (n == 0) {
        if (!stats) return 0;
        return (int)hipMemsetAsync(stats, 0, (size_t)(2 * (num_classes ? num_classes : 2)) * sizeof(long long), stream);
    }
    if (!v || !out || !ws || (reinterpret_cast<uintptr_t>(ws) & 15) != 0) return AIDE_ERR_ARG;
    Grids gr;
    const Strided geo = make_strided(static_cast<const long long*>(v), d0, d1, d2, s0, s1, s2, gr);
    if (v_u8) return holes_launch<unsigned char>(geo, gr, n, num_classes, slice_axis, out, stats, ws, stream);
    return holes_launch<long long>(geo, gr, n, num_classes, slice_axis, out, stats, ws, stream);
}

size_t aide_lcc3d_ws_bytes(int64_t nvox) { return ws_bytes(nvox, 1, 2); }

size_t aide_lcc3d_classes_ws_bytes(int64_t nvox, int num_classes) {
    return classes_ok(num_classes) ? ws_bytes(nvox, 1, 3 * num_classes) : 0;
}

size_t aide_lcc3d_batched_ws_bytes(int64_t nvox_total, int64_t K) { return ws_bytes(nvox_total, K, 2); }

size_t aide_lcc3d_classes_batched_ws_bytes(int64_t nvox_total, int64_t K, int num_classes) {
    return classes_ok(num_classes) ? ws_bytes(nvox_total, K, 3 * num_classes) : 0;
}

int aide_keep_largest_cc3d(const long long* v, int64_t d0, int64_t d1, int64_t d2, int64_t s0, int64_t s1, int64_t s2,
                           unsigned char* out, void* ws, hipStream_t stream) {
    if (!dims_ok(d0, d1, d2)) return AIDE_ERR_ARG;
    const int n = (int)(d0 * d1 * d2);
    if (n == 0) return 0;
    if (!v || !out || !ws) return AIDE_ERR_ARG;
    Grids gr;
    const Strided geo = make_strided(v, d0, d1, d2, s0, s1, s2, gr);
    return lcc_launch(geo, gr, n, 1, 0, out, nullptr, ws, stream);
}

int aide_keep_largest_cc3d_classes(const long long* v, int64_t d0, int64_t d1, int64_t d2, int64_t s0, int64_t s1, int64_t s2,
                                   int num_classes, unsigned char* out, long long* stats, void* ws, hipStream_t stream) {
    if (!classes_ok(num_classes) || !dims_ok(d0, d1, d2)) return AIDE_ERR_ARG;
    const int n = (int)(d0 * d1 * d2);
    if (n == 0) {
        if (!stats) return 0;
        return (int)hipMemsetAsync(stats, 0, (size_t)(3 * num_classes) * sizeof(long long), stream);
    }
    if (!v || !out || !ws) return AIDE_ERR_ARG;
    Grids gr;
    const Strided geo = make_strided(v, d0, d1, d2, s0, s1, s2, gr);
    return lcc_launch(geo, gr, n, 1, num_classes, out, stats, ws, stream);
}

int aide_keep_largest_cc3d_batched(const long long* v, const long long* slice_start, int64_t K, int64_t S_total, int64_t H,
                                   int64_t W, unsigned char* out, void* ws, hipStream_t stream) {
    if (!batch_ok(S_total, H, W, K)) return AIDE_ERR_ARG;
    const int n = (int)(S_total * H * W);
    if (n == 0 || K == 0) return 0;
    if (!v || !slice_start || !out || !ws) return AIDE_ERR_ARG;
    Grids gr;
    const Ragged geo = make_ragged(v, slice_start, K, S_total, H, W, gr);
    return lcc_launch(geo, gr, n, K, 0, out, nullptr, ws, stream);
}

int aide_keep_largest_cc3d_classes_batched(const long long* v, const long long* slice_start, int64_t K, int64_t S_total,
                                           int64_t H, int64_t W, int num_classes, unsigned char* out, long long* stats,
                                           void* ws, hipStream_t stream) {
    if (!classes_ok(num_classes) || !batch_ok(S_total, H, W, K)) return AIDE_ERR_ARG;
    const int n = (int)(S_total * H * W);
    if (n == 0 || K == 0) {
        if (!stats || K == 0) return 0;
        return (int)hipMemsetAsync(stats, 0, (size_t)(3 * K * num_classes) * sizeof(long long), stream);
    }
    if (!v || !slice_start || !out || !ws) return AIDE_ERR_ARG;
    Grids gr;
    const Ragged geo = make_ragged(v, slice_start, K, S_total, H, W, gr);
    return lcc_launch(geo, gr, n, K, num_classes, out, stats, ws, stream);
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
    const Operand P{p, (long)p_s0, (long)p_s1, (long)p_s2, p_u8}, T{t, (long)t_s0, (long)t_s1, (long)t_s2, t_u8};
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
