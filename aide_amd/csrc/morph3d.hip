// Binary and per-class morphology with a ball in millimetres on the device: erosion, dilation, opening, closing
// (include/aide_hip.h "ball morphology"; the definitions are DESIGN.md section 4 "Ball morphology and the distance transform").
//
// Everything is one primitive, the thresholded and windowed form of the separable distance transform of surface3d.hip:
//   hit(v) = exists a candidate u with q(v - u) <= r * r,   q(o) = (sp0 * o0)^2 + ((sp1 * o1)^2 + (sp2 * o2)^2) in fp64.
//   dilate(X)          = hit with the candidates X
//   erode(X, outside)  = not hit with the candidates "not X"; outside = 0 adds the lattice points beyond the six faces, of which
//                        only the axis-aligned nearest can decide: one virtual candidate before and one after every line
// Along axis k only candidates within W_k = the largest w with (sp_k * w)^2 <= r * r can pass the threshold (every term of q is
// >= 0 and the rounded sum is monotone in each), so a primitive costs n * sum_k (2 W_k + 1) candidate evaluations.  Launches of
// one primitive, all with one thread per voxel in logical raster order, so that the lanes of a wave read along d2 in every pass:
//   1 morph_scan   along d2: g = the integer distance to the nearest candidate of the line within W_2 (the search walks outwards
//                  and stops at the first), NONE when there is none
//   2 morph_mid    along d1: f(i1) = min over |i1 - j1| <= W_1 of (sp1 * (i1 - j1))^2 + (sp2 * g(j1))^2, +inf where g is NONE
//   3 morph_last   along d0: the same min over f, compared with r * r; writes a byte plane for the next primitive, or merges the
//                  plane's answer into out
// The min of rounded sums is the rounded sum of the min (rounding is monotone), so hit is exactly "some offset of the ball, as
// this arithmetic evaluates q, leads to a candidate".  morph_classes (launch 0) reads the strided volume once and writes the class
// of every voxel as a byte (binary: v != 0); the planes X_c = (class == c) are never materialised, a candidate test is a compare.
// Opening and closing are two primitives with a byte plane in between; classes run one after the other in stream order.
// No workgroup waits for another, there is no atomic at all, every word of the workspace that is read was written by an
// earlier launch of the same call, and every thread writes only its own voxel: two calls give the same bytes.  All indices come
// from integers.
#include "volume3d.h"

namespace {

constexpr int NONE = 0x7fffffff;
constexpr unsigned char MIXED = 255;   // morph_last, merge mode: more than one class claims the voxel (class values are < 8)

enum { OP_ERODE0 = 0, OP_ERODE1 = 1, OP_DILATE = 2, OP_OPEN = 3, OP_CLOSE = 4 };
enum { TO_PLANE = 0, TO_OUT_SET = 1, TO_OUT_MERGE = 2 };

// cmap[i] = the class of voxel i: num_classes = 0: v != 0; C: v for 1 <= v < C, 0 otherwise.  out: nullptr, or a second copy
__global__ __launch_bounds__(256) void morph_classes_kernel(Operand X, int d1, int d2, int n, int num_classes,
                                                            unsigned char* __restrict__ cmap, unsigned char* __restrict__ out) {
    const unsigned u = blockIdx.x * 256u + threadIdx.x;
    if (u >= (unsigned)n) return;
    const int i = (int)u;
    int i0, i1, i2;
    raster_decode(i, d1, d2, i0, i1, i2);
    const long long v = X.at(X.off(i0, i1, i2));
    const unsigned char c = num_classes ? (v >= 1 && v < (long long)num_classes ? (unsigned char)v : (unsigned char)0)
                                        : (unsigned char)(v != 0);
    cmap[i] = c;
    if (out) out[i] = c;
}

// a candidate: map == val (eq) or map != val (!eq); faces: the positions -1 and d2 of every line are candidates too
__global__ __launch_bounds__(256) void morph_scan_kernel(const unsigned char* __restrict__ map, int val, int eq, int faces, int d2,
                                                         int n, int w2, int* __restrict__ g) {
    const unsigned u = blockIdx.x * 256u + threadIdx.x;
    if (u >= (unsigned)n) return;
    const int i = (int)u, i2 = i % d2;
    const unsigned char* line = map + (i - i2);
    int found = NONE;
    for (int k = 0; k <= w2; ++k) {
        const int lo = i2 - k, hi = i2 + k;
        const bool a = lo >= 0 ? ((int)line[lo] == val) == (eq != 0) : (faces && lo == -1);
        const bool b = hi < d2 ? ((int)line[hi] == val) == (eq != 0) : (faces && hi == d2);
        if (a || b) {
            found = k;
            break;
        }
        if (lo < -1 && hi > d2) break;           // beyond both ends: nothing is left
    }
    g[i] = found;
}

// f[i] from g along d1 (stride d2)
__global__ __launch_bounds__(256) void morph_mid_kernel(const int* __restrict__ g, int faces, int d1, int d2, int n, int w1,
                                                        double sp1, double sp2, double* __restrict__ f) {
    const unsigned u = blockIdx.x * 256u + threadIdx.x;
    if (u >= (unsigned)n) return;
    const int i = (int)u, i1 = (i / d2) % d1;
    const int jlo = max(0, i1 - w1), jhi = (int)min((long)d1 - 1, (long)i1 + w1);
    double best = __builtin_inf();
    for (int j = jlo; j <= jhi; ++j) {
        const int gi = g[i + (j - i1) * d2];
        if (gi != NONE) {
            const double s = sp2 * (double)gi, t = sp1 * (double)(i1 - j);
            best = fmin(best, t * t + s * s);
        }
    }
    if (faces) {
        if (i1 + 1 <= w1) { const double t = sp1 * (double)(i1 + 1); best = fmin(best, t * t + 0.0); }
        if (d1 - i1 <= w1) { const double t = sp1 * (double)(d1 - i1); best = fmin(best, t * t + 0.0); }
    }
    f[i] = best;
}

// hit = (min along d0 over f) <= r2; res = hit != invert.
//   TO_PLANE      dst[i] = res
//   TO_OUT_SET    dst[i] = cls where res (dst was cleared by the launcher; the planes of an erosion or opening are disjoint)
//   TO_OUT_MERGE  only where cmap[i] == 0 (dst started as a copy of cmap): a first claim writes cls, a second one MIXED; the
//                 last class turns MIXED into 0
__global__ __launch_bounds__(256) void morph_last_kernel(const double* __restrict__ f, int faces, int d0, int plane, int n, int w0,
                                                         double sp0, double r2, int invert, int mode, int cls, int last_class,
                                                         const unsigned char* __restrict__ cmap, unsigned char* __restrict__ dst) {
    const unsigned u = blockIdx.x * 256u + threadIdx.x;
    if (u >= (unsigned)n) return;
    const int i = (int)u, i0 = i / plane;
    const int jlo = max(0, i0 - w0), jhi = (int)min((long)d0 - 1, (long)i0 + w0);
    double best = __builtin_inf();
    for (int j = jlo; j <= jhi; ++j) {
        const double t = sp0 * (double)(i0 - j);
        best = fmin(best, t * t + f[(long)i + (long)(j - i0) * plane]);
    }
    if (faces) {
        if (i0 + 1 <= w0) { const double t = sp0 * (double)(i0 + 1); best = fmin(best, t * t + 0.0); }
        if (d0 - i0 <= w0) { const double t = sp0 * (double)(d0 - i0); best = fmin(best, t * t + 0.0); }
    }
    const bool res = (best <= r2 && best < __builtin_inf()) != (invert != 0);      // (r * r may overflow: +inf is still no candidate)
    if (mode == TO_PLANE) {
        dst[i] = res;
    } else if (mode == TO_OUT_SET) {
        if (res) dst[i] = (unsigned char)cls;
    } else if (cmap[i] == 0) {
        unsigned char o = dst[i];
        if (res) o = o == 0 ? (unsigned char)cls : MIXED;
        if (last_class && o == MIXED) o = 0;
        dst[i] = o;
    }
}

// the largest w in 0 .. d with (sp * w)^2 <= r2, in the arithmetic of the kernels (t * t + 0.0 is the rounded product, fused or not)
int window(double r, double sp, double r2, int64_t d) {
    const double q = std::floor(r / sp);
    int64_t w = q < (double)d ? (int64_t)q : d;
    while (w < d && (sp * (double)(w + 1)) * (sp * (double)(w + 1)) <= r2) ++w;
    while (w > 0 && (sp * (double)w) * (sp * (double)w) > r2) --w;
    return (int)w;
}

struct Geometry {
    int d0, d1, d2, n, plane, w0, w1, w2;
    double sp0, sp1, sp2, r2;
    int* g;
    double* f;
    hipStream_t stream;
};

// f [n] fp64 | g [n] int32 | class map [n] bytes | plane between the two primitives of an opening / closing [n] bytes
struct MorphWs {
    double* f;
    int* g;
    unsigned char *cmap, *mid;
    size_t bytes;
};
MorphWs morph_ws(void* ws, size_t n) {
    Carver c(ws);
    MorphWs w;
    w.f = c.take<double>(n);
    w.g = c.take<int>(n);
    w.cmap = c.take<unsigned char>(n);
    w.mid = c.take<unsigned char>(n);
    w.bytes = c.used + 16;
    return w;
}

// one primitive: candidates map == val (eq) or map != val; see morph_last_kernel for the rest
void primitive(const Geometry& q, const unsigned char* map, int val, int eq, int faces, int invert, int mode, int cls,
               int last_class, const unsigned char* cmap, unsigned char* dst) {
    const dim3 grid((unsigned)(((long)q.n + 255) / 256)), block(256);
    AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 5.0 * q.n, morph_scan_kernel, grid, block, 0, q.stream, map, val, eq, faces, q.d2, q.n, q.w2,
                      q.g);
    AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 12.0 * q.n, morph_mid_kernel, grid, block, 0, q.stream, (const int*)q.g, faces, q.d1, q.d2,
                      q.n, q.w1, q.sp1, q.sp2, q.f);
    AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 9.0 * q.n, morph_last_kernel, grid, block, 0, q.stream, (const double*)q.f, faces, q.d0,
                      q.plane, q.n, q.w0, q.sp0, q.r2, invert, mode, cls, last_class, cmap, dst);
}

}  // namespace

extern "C" {

size_t aide_morph3d_ws_bytes(int64_t nvox) {
    if (nvox < 0 || nvox > INT32_MAX) return 0;
    return morph_ws(nullptr, (size_t)nvox).bytes;
}

int aide_morph3d(const void* v, int v_u8, int64_t d0, int64_t d1, int64_t d2, int64_t s0, int64_t s1, int64_t s2,
                 int num_classes, int op, double radius, const double* spacing, unsigned char* out, void* ws,
                 hipStream_t stream) {
    if (!dims_ok(d0, d1, d2) || !spacing || (v_u8 != 0 && v_u8 != 1)) return AIDE_ERR_ARG;
    if (num_classes != 0 && (num_classes < 2 || num_classes > 8)) return AIDE_ERR_ARG;
    if (op < OP_ERODE0 || op > OP_CLOSE) return AIDE_ERR_ARG;
    if (!std::isfinite(radius) || radius < 0.0) return AIDE_ERR_ARG;
    if (!spacing_ok(spacing)) return AIDE_ERR_ARG;
    const int n = (int)(d0 * d1 * d2);
    if (n == 0) return 0;
    if (!v || !out || !ws || (reinterpret_cast<uintptr_t>(ws) & 15) != 0 || (!v_u8 && (reinterpret_cast<uintptr_t>(v) & 7) != 0))
        return AIDE_ERR_ARG;
    Geometry q;
    q.d0 = (int)d0; q.d1 = (int)d1; q.d2 = (int)d2; q.n = n; q.plane = (int)(d1 * d2);
    q.sp0 = spacing[0]; q.sp1 = spacing[1]; q.sp2 = spacing[2];
    q.r2 = radius * radius;
    q.w0 = window(radius, q.sp0, q.r2, d0);
    q.w1 = window(radius, q.sp1, q.r2, d1);
    q.w2 = window(radius, q.sp2, q.r2, d2);
    q.stream = stream;
    const MorphWs w = morph_ws(ws, (size_t)n);
    q.f = w.f;
    q.g = w.g;
    unsigned char *cmap = w.cmap, *mid = w.mid;
    const bool merge = op == OP_DILATE || op == OP_CLOSE;
    if (!merge) {
        const hipError_t e = hipMemsetAsync(out, 0, (size_t)n, stream);
        if (e != hipSuccess) return (int)e;
    }
    const Operand X{v, (long)s0, (long)s1, (long)s2, v_u8};
    AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, (double)n * (v_u8 ? 2 : 9), morph_classes_kernel, dim3((unsigned)(((long)n + 255) / 256)),
                      dim3(256), 0, stream, X, (int)d1, (int)d2, n, num_classes, cmap, merge ? out : (unsigned char*)nullptr);
    const int classes = num_classes ? num_classes : 2;
    for (int c = 1; c < classes; ++c) {
        const int last = c == classes - 1;
        switch (op) {
        case OP_ERODE0:
        case OP_ERODE1:
            primitive(q, cmap, c, 0, op == OP_ERODE0, 1, TO_OUT_SET, c, last, cmap, out);
            break;
        case OP_DILATE:
            primitive(q, cmap, c, 1, 0, 0, TO_OUT_MERGE, c, last, cmap, out);
            break;
        case OP_OPEN:
            primitive(q, cmap, c, 0, 1, 1, TO_PLANE, c, last, cmap, mid);
            primitive(q, mid, 1, 1, 0, 0, TO_OUT_SET, c, last, cmap, out);
            break;
        default:
            primitive(q, cmap, c, 1, 0, 0, TO_PLANE, c, last, cmap, mid);
            primitive(q, mid, 1, 0, 0, 1, TO_OUT_MERGE, c, last, cmap, out);
            break;
        }
    }
    return aide_launch_status();
}

}  // extern "C"
