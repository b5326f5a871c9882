// Spacing-aware resampling of a volume on the device (include/aide_hip.h "resampling"; the definition is the module docstring
// of aide_amd/resample.py): label volumes through the arg-max of the linearly interpolated class indicators, fp32 images, and
// [S,C,H,W] probabilities with the arg-max over their interpolated classes.
//
// Two launches per call:
//   1 resample_table  one thread per output index of every axis: (lo, hi, w1) of the half-pixel-centre map, in exact integers
//                     and one fp64 division, into the workspace (e0 + e1 + e2 entries of 16 bytes); order 0: the nearest index
//   2 resample        ONE gather body for the three sources (indicator / image value / probability), templated on the source
//                     and on the class count: the C fp64 accumulators live in registers, the eight corners are visited in the
//                     order 000, 001, .. 111 of the LOGICAL axes with the weight (w_a * w_b) * w_c, every product rounded on
//                     its own.  A thread owns VEC = 4 consecutive elements of the dense output IN ITS MEMORY ORDER (lanes run
//                     along the axis with the smallest output stride) and stores them as one word: 4 labels in 32 bits, 4
//                     floats or 2 x 2 int64 in 16 bytes.  No [C, ...] intermediate, no atomic, no workgroup waits for another.
#include "volume3d.h"

namespace {

constexpr int VEC = 4;

struct Entry { int lo, hi; double w1; };          // one output index of one axis; 16 bytes, read as one word
static_assert(sizeof(Entry) == 16, "table entry");

typedef long long i64x2 __attribute__((ext_vector_type(2)));

// a * b rounded to double before any use (the library builds with -ffp-contract=fast; the empty asm keeps the product out of a
// fused multiply-add, as in augment.hip)
__device__ __forceinline__ double mul_rn(double a, double b) {
    double p = a * b;
    asm volatile("" : "+v"(p));
    return p;
}

struct Geometry {
    int m0, m1, m2;            // the output dims in memory order, slowest first
    int at0, at1, at2;         // where the logical axes 0, 1, 2 stand in that order
    int n_out;                 // m0 * m1 * m2
    long total;                // batch * n_out
    const Entry *t0, *t1, *t2; // the tables of the logical axes
    long s0, s1, s2, sb;       // element strides of the input along the logical axes, and from one volume of a batch to the next
};

__global__ __launch_bounds__(256) void resample_table_kernel(Entry* __restrict__ tab, int d0, int d1, int d2, int e0, int e1,
                                                             int e2, int nearest) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    long o, n_in, n_out;
    if (i < e0) { o = i; n_in = d0; n_out = e0; }
    else if (i < (long)e0 + e1) { o = i - e0; n_in = d1; n_out = e1; }
    else if (i < (long)e0 + e1 + e2) { o = i - e0 - e1; n_in = d2; n_out = e2; }
    else return;
    const long den = 2 * n_out;
    Entry e;
    if (nearest) {
        e.lo = e.hi = (int)min(((2 * o + 1) * n_in) / den, n_in - 1);
        e.w1 = 0.0;
    } else {
        const long num = max((2 * o + 1) * n_in - n_out, 0L);
        const long lo = min(num / den, n_in - 1);
        e.lo = (int)lo;
        e.hi = (int)min(lo + 1, n_in - 1);
        e.w1 = (double)(num - lo * den) / (double)den;
    }
    tab[i] = e;
}

template <int C> struct Result { int label; float val[C]; };

// first index of the largest accumulator (strict >: a NaN never displaces an earlier class)
template <int C>
__device__ __forceinline__ int first_max(const double (&acc)[C]) {
    int best = 0;
    double top = acc[0];
#pragma unroll
    for (int c = 1; c < C; ++c)
        if (acc[c] > top) { top = acc[c]; best = c; }
    return best;
}

// ---- the three sources.  add: what a corner with weight w contributes; finish: accumulators -> result; nearest: order 0;
// store: `count` (VEC, or fewer at the very end) consecutive results from element `first` of the dense output
template <typename T>
struct LabelJob {
    Operand v;
    int classes;               // 0: v != 0
    unsigned char* out;
    __device__ __forceinline__ long long cls(long off) const {
        const long long x = v.at<T>(off);
        return classes ? x : (long long)(x != 0);
    }
    template <int C> __device__ __forceinline__ void add(double (&acc)[C], long off, double w) const {
        const long long x = cls(off);
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = (x == c) ? acc[c] + w : acc[c];
    }
    template <int C> __device__ __forceinline__ Result<C> finish(const double (&acc)[C]) const {
        Result<C> r;
        r.label = first_max<C>(acc);
        return r;
    }
    template <int C> __device__ __forceinline__ Result<C> nearest(long off) const {
        const long long x = cls(off);
        Result<C> r;
        r.label = (x >= 0 && x < (classes ? classes : 2)) ? (int)x : 0;
        return r;
    }
    template <int C> __device__ __forceinline__ void store(const Geometry&, long first, int count, const Result<C> (&r)[VEC]) const {
        if (count == VEC) {
            *reinterpret_cast<unsigned*>(out + first) = (unsigned)r[0].label | ((unsigned)r[1].label << 8) |
                                                        ((unsigned)r[2].label << 16) | ((unsigned)r[3].label << 24);
            return;
        }
#pragma unroll
        for (int j = 0; j < VEC - 1; ++j)
            if (j < count) out[first + j] = (unsigned char)r[j].label;
    }
};

struct ImageJob {
    const float* x;
    float* out;
    template <int C> __device__ __forceinline__ void add(double (&acc)[C], long off, double w) const {
        acc[0] += mul_rn(w, (double)x[off]);
    }
    template <int C> __device__ __forceinline__ Result<C> finish(const double (&acc)[C]) const {
        Result<C> r;
        r.val[0] = (float)acc[0];
        return r;
    }
    template <int C> __device__ __forceinline__ Result<C> nearest(long off) const {
        Result<C> r;
        r.val[0] = x[off];
        return r;
    }
    template <int C> __device__ __forceinline__ void store(const Geometry&, long first, int count, const Result<C> (&r)[VEC]) const {
        if (count == VEC) {
            st4(out + first, f32x4{r[0].val[0], r[1].val[0], r[2].val[0], r[3].val[0]});
            return;
        }
#pragma unroll
        for (int j = 0; j < VEC - 1; ++j)
            if (j < count) out[first + j] = r[j].val[0];
    }
};

struct ProbJob {
    const float* p;
    long cs;                   // class stride of the input
    long long* labels;         // [e0][e1][e2]
    float* probs;              // [e0][C][e1][e2], or null
    template <int C> __device__ __forceinline__ void add(double (&acc)[C], long off, double w) const {
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] += mul_rn(w, (double)p[off + c * cs]);
    }
    template <int C> __device__ __forceinline__ Result<C> finish(const double (&acc)[C]) const {
        Result<C> r;
        r.label = first_max<C>(acc);
#pragma unroll
        for (int c = 0; c < C; ++c) r.val[c] = (float)acc[c];
        return r;
    }
    template <int C> __device__ __forceinline__ Result<C> nearest(long) const { return Result<C>{}; }      // (not offered)
    template <int C> __device__ __forceinline__ void store(const Geometry& g, long first, int count, const Result<C> (&r)[VEC]) const {
        if (count == VEC) {
            i64x2* q = reinterpret_cast<i64x2*>(labels + first);
            q[0] = i64x2{r[0].label, r[1].label};
            q[1] = i64x2{r[2].label, r[3].label};
        } else {
#pragma unroll
            for (int j = 0; j < VEC - 1; ++j)
                if (j < count) labels[first + j] = r[j].label;
        }
        if (!probs) return;
        const int plane = g.m1 * g.m2;
        const int s = (int)(first / plane), po = (int)(first - (long)s * plane);
        if (count == VEC && po + VEC <= plane && (plane & 3) == 0) {       // one row of one class plane, 16-byte aligned
#pragma unroll
            for (int c = 0; c < C; ++c)
                st4(probs + ((long)s * C + c) * plane + po, f32x4{r[0].val[c], r[1].val[c], r[2].val[c], r[3].val[c]});
            return;
        }
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            if (j >= count) break;
            const int sj = (int)((first + j) / plane), pj = (int)(first + j - (long)sj * plane);
#pragma unroll
            for (int c = 0; c < C; ++c) probs[((long)sj * C + c) * plane + pj] = r[j].val[c];
        }
    }
};

// ---- the gather body: one output voxel at the logical index (o0, o1, o2) of volume b
template <class Job, int C, bool NEAREST>
__device__ __forceinline__ Result<C> gather(const Geometry& g, const Job& job, int b, int o0, int o1, int o2) {
    const Entry a0 = g.t0[o0], a1 = g.t1[o1], a2 = g.t2[o2];
    const long base = (long)b * g.sb;
    if constexpr (NEAREST) {
        return job.template nearest<C>(base + a0.lo * g.s0 + a1.lo * g.s1 + a2.lo * g.s2);
    } else {
        const double w0[2] = {1.0 - a0.w1, a0.w1}, w1[2] = {1.0 - a1.w1, a1.w1}, w2[2] = {1.0 - a2.w1, a2.w1};
        const long p0[2] = {a0.lo * g.s0, a0.hi * g.s0}, p1[2] = {a1.lo * g.s1, a1.hi * g.s1}, p2[2] = {a2.lo * g.s2, a2.hi * g.s2};
        double acc[C];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = 0.0;
#pragma unroll
        for (int ia = 0; ia < 2; ++ia)
#pragma unroll
            for (int ib = 0; ib < 2; ++ib) {
                const double wab = mul_rn(w0[ia], w1[ib]);
#pragma unroll
                for (int ic = 0; ic < 2; ++ic)
                    job.template add<C>(acc, base + p0[ia] + p1[ib] + p2[ic], mul_rn(wab, w2[ic]));
            }
        return job.template finish<C>(acc);
    }
}

__device__ __forceinline__ int pick3(int at, int i0, int i1, int i2) { return at == 0 ? i0 : at == 1 ? i1 : i2; }

template <class Job, int C, bool NEAREST>
__global__ __launch_bounds__(256) void resample_kernel(const Geometry g, const Job job) {
    const long first = ((long)blockIdx.x * 256 + threadIdx.x) * VEC;
    if (first >= g.total) return;
    const int count = (int)min((long)VEC, g.total - first);
    int b = (int)(first / g.n_out), i0, i1, i2;
    raster_decode((int)(first - (long)b * g.n_out), g.m1, g.m2, i0, i1, i2);
    Result<C> r[VEC] = {};
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
        if (j < count) {
            r[j] = gather<Job, C, NEAREST>(g, job, b, pick3(g.at0, i0, i1, i2), pick3(g.at1, i0, i1, i2), pick3(g.at2, i0, i1, i2));
            if (++i2 == g.m2) {
                i2 = 0;
                if (++i1 == g.m1) {
                    i1 = 0;
                    if (++i0 == g.m0) { i0 = 0; ++b; }
                }
            }
        }
    }
    job.template store<C>(g, first, count, r);
}

bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// what the three entry points check alike; 1: nothing to do, 0: go on
int common_args(int64_t batch, int64_t d0, int64_t d1, int64_t d2, int64_t e0, int64_t e1, int64_t e2, int order, const void* ws) {
    if (batch < 0 || !dims_ok(d0, d1, d2) || !dims_ok(e0, e1, e2) || (order != 0 && order != 1)) return AIDE_ERR_ARG;
    const int64_t n_in = d0 * d1 * d2, n_out = e0 * e1 * e2;
    if (batch > 0 && (n_in > INT32_MAX / batch || n_out > INT32_MAX / batch)) return AIDE_ERR_ARG;
    if (batch * n_out == 0) return 1;
    if (n_in == 0 || !ws || !aligned(ws, 16)) return AIDE_ERR_ARG;
    return 0;
}

// launch 1, and the part of the geometry that does not depend on the source; oa = the logical axes of the output from the
// slowest to the fastest in memory
Geometry prepare(int64_t batch, int64_t d0, int64_t d1, int64_t d2, int64_t e0, int64_t e1, int64_t e2, int order,
                 const int (&oa)[3], int64_t s0, int64_t s1, int64_t s2, int64_t sb, void* ws, hipStream_t stream) {
    Entry* tab = static_cast<Entry*>(ws);
    const long entries = (long)e0 + e1 + e2;
    AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 16.0 * entries, resample_table_kernel, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0,
                      stream, tab, (int)d0, (int)d1, (int)d2, (int)e0, (int)e1, (int)e2, order == 0);
    const int64_t e[3] = {e0, e1, e2};
    Geometry g;
    g.m0 = (int)e[oa[0]]; g.m1 = (int)e[oa[1]]; g.m2 = (int)e[oa[2]];
    int at[3];
    for (int k = 0; k < 3; ++k) at[oa[k]] = k;
    g.at0 = at[0]; g.at1 = at[1]; g.at2 = at[2];
    g.n_out = (int)(e0 * e1 * e2);
    g.total = (long)(batch * g.n_out);
    g.t0 = tab; g.t1 = tab + e0; g.t2 = tab + e0 + e1;
    g.s0 = (long)s0; g.s1 = (long)s1; g.s2 = (long)s2; g.sb = (long)sb;
    return g;
}

template <int C, bool NEAREST, class Job>
void launch(const Geometry& g, const Job& job, double bytes_per_voxel, hipStream_t stream) {
    const long threads = (g.total + VEC - 1) / VEC;
    AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, bytes_per_voxel * (double)g.total, (resample_kernel<Job, C, NEAREST>),
                      dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, g, job);
}

template <typename T>
void launch_labels(const Geometry& g, const LabelJob<T>& job, int order, hipStream_t stream) {
    const double bytes = 1.0 + (order ? 8.0 : 1.0) * sizeof(T);
    if (order == 0) return launch<2, true>(g, job, bytes, stream);
    aide_pick<2, 3, 4, 5, 6, 7, 8>(job.classes ? job.classes : 2, [&](auto c) { launch<decltype(c)::value, false>(g, job, bytes, stream); });
}

}  // namespace

extern "C" {

size_t aide_resample3d_ws_bytes(int64_t e0, int64_t e1, int64_t e2) {
    if (!dims_ok(e0, e1, e2)) return 0;
    return align16((size_t)(e0 + e1 + e2) * sizeof(Entry));
}

int aide_resample3d_labels(const void* v, int v_u8, int64_t d0, int64_t d1, int64_t d2, int64_t s0, int64_t s1, int64_t s2,
                           int64_t e0, int64_t e1, int64_t e2, int num_classes, int order, int oa0, int oa1, int oa2,
                           unsigned char* out, void* ws, hipStream_t stream) {
    if (v_u8 != 0 && v_u8 != 1) return AIDE_ERR_ARG;
    if (num_classes != 0 && (num_classes < 2 || num_classes > 8)) return AIDE_ERR_ARG;
    const int oa[3] = {oa0, oa1, oa2};
    if (oa0 < 0 || oa0 > 2 || oa1 < 0 || oa1 > 2 || oa2 < 0 || oa2 > 2 || oa0 == oa1 || oa0 == oa2 || oa1 == oa2) return AIDE_ERR_ARG;
    if (const int rc = common_args(1, d0, d1, d2, e0, e1, e2, order, ws)) return rc < 0 ? rc : 0;
    if (!v || !out || !aligned(out, 4) || (!v_u8 && !aligned(v, 8))) return AIDE_ERR_ARG;
    const Geometry g = prepare(1, d0, d1, d2, e0, e1, e2, order, oa, s0, s1, s2, 0, ws, stream);
    const Operand X{v, (long)s0, (long)s1, (long)s2, v_u8};
    if (v_u8) launch_labels(g, LabelJob<unsigned char>{X, num_classes, out}, order, stream);
    else launch_labels(g, LabelJob<long long>{X, num_classes, out}, order, stream);
    return aide_launch_status();
}

int aide_resample3d_image(const float* x, int64_t batch, int64_t xb, int64_t d0, int64_t d1, int64_t d2, int64_t s0, int64_t s1,
                          int64_t s2, int64_t e0, int64_t e1, int64_t e2, int order, float* out, void* ws, hipStream_t stream) {
    if (const int rc = common_args(batch, d0, d1, d2, e0, e1, e2, order, ws)) return rc < 0 ? rc : 0;
    if (!x || !out || !aligned(x, 4) || !aligned(out, 16)) return AIDE_ERR_ARG;
    const int oa[3] = {0, 1, 2};
    const Geometry g = prepare(batch, d0, d1, d2, e0, e1, e2, order, oa, s0, s1, s2, xb, ws, stream);
    const ImageJob job{x, out};
    if (order == 0) launch<1, true>(g, job, 8.0, stream);
    else launch<1, false>(g, job, 36.0, stream);
    return aide_launch_status();
}

int aide_resample3d_probs(const float* p, int num_classes, int64_t cs, int64_t d0, int64_t d1, int64_t d2, int64_t s0, int64_t s1,
                          int64_t s2, int64_t e0, int64_t e1, int64_t e2, int64_t* labels, float* probs_out, void* ws,
                          hipStream_t stream) {
    if (num_classes < 2 || num_classes > 8) return AIDE_ERR_ARG;
    if (const int rc = common_args(1, d0, d1, d2, e0, e1, e2, 1, ws)) return rc < 0 ? rc : 0;
    if (e0 * e1 * e2 > INT32_MAX / num_classes) return AIDE_ERR_ARG;
    if (!p || !labels || !aligned(p, 4) || !aligned(labels, 16) || !aligned(probs_out, 16)) return AIDE_ERR_ARG;
    const int oa[3] = {0, 1, 2};
    const Geometry g = prepare(1, d0, d1, d2, e0, e1, e2, 1, oa, s0, s1, s2, 0, ws, stream);
    const ProbJob job{p, (long)cs, reinterpret_cast<long long*>(labels), probs_out};
    const double bytes = 8.0 + num_classes * (32.0 + (probs_out ? 4.0 : 0.0));
    aide_pick<2, 3, 4, 5, 6, 7, 8>(num_classes, [&](auto c) { launch<decltype(c)::value, false>(g, job, bytes, stream); });
    return aide_launch_status();
}

}  // extern "C"
