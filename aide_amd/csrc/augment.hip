// Loader transforms of the proposed loaders on the device (include/aide_hip.h "loader transforms"): the chain
// Resize(BILINEAR) -> RandomRotate(BILINEAR) x augno -> RandomHorizontallyFlip x augno -> ToTensor -> Normalize of
// datasetchaos_proposed/transform.py (and the single-modal copies), for a whole batch, bit-exact where PIL is integer.
//
// The source of a plane is a grey u8 image or a raw u16 one (PIL's I;16 -> RGB conversion clamps to 255); the three RGB
// channels stay equal through every op, so one channel is computed and replicated on the store.  Launches:
//   1 la_resize   per plane: PIL's ImagingResample (horizontal pass, u8 clip, vertical pass; 22-bit fixed-point weights
//                 from the host tables) into the u8 base image, and per workgroup the integer sums of v and v^2
//   2 la_emit     per plane and view (0 = base, k = augmentation k): PIL's Image.rotate(angle, BILINEAR) of the base
//                 (inverse affine at pixel centres in double, 0 outside, clamped taps, truncation to u8; the exact
//                 transpose paths at multiples of 90 degrees), then the horizontal flip, then v / 255 normalised by the
//                 per-image mean / unbiased std (from the integer sums) or fixed per-channel values; 4 pixels per thread
//   3 la_mask     Resize(NEAREST) of the masks (host index tables: PIL's accumulated scale) + one-hot over a palette
// Everything but the final float normalisation is integer or exactly PIL's double arithmetic, with every product of the
// rotation rounded on its own (mul_rn): an FMA there moves values across the truncation and the `xin >= W` edge.
#include "common.h"

namespace {

// a * b rounded to double before any use.  (The library builds with -ffp-contract=fast, under which
// `#pragma clang fp contract(off)` is not honoured; the empty asm keeps the product out of a fused multiply-add.)
__device__ __forceinline__ double mul_rn(double a, double b) {
    double p = a * b;
    asm volatile("" : "+v"(p));
    return p;
}

constexpr int LA_PARTS = 256;        // resize workgroups per plane at most = partial sums per plane
constexpr int LA_DESC = 8;           // ints per plane descriptor

__device__ __forceinline__ int clip8(int v) { return v >= (1 << 30) ? 255 : v <= 0 ? 0 : (v >> 22); }

__device__ __forceinline__ int src_at(const unsigned char* __restrict__ src, int off, int u16, long idx) {
    if (u16) return min((int)reinterpret_cast<const unsigned short*>(src + off)[idx], 255);
    return src[off + idx];
}

// desc[p] = {byte offset, h, w, u16, x table, y table, kx, ky}; a table entry per output index: {first tap, taps, k weights}
__global__ __launch_bounds__(256) void la_resize_kernel(const unsigned char* __restrict__ src, const int* __restrict__ desc,
                                                        const int* __restrict__ tab, int S, unsigned char* __restrict__ base,
                                                        unsigned long long* __restrict__ part) {
    const int p = blockIdx.y;
    const int* d = desc + p * LA_DESC;
    const int off = d[0], h = d[1], w = d[2], u16 = d[3], kx = d[6], ky = d[7];
    const int* xt = tab + d[4];
    const int* yt = tab + d[5];
    const long npix = (long)S * S;
    unsigned long long s1 = 0, s2 = 0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < npix; i += (long)gridDim.x * 256) {
        const int oy = (int)(i / S), ox = (int)(i - (long)oy * S);
        const int* ex = xt + ox * (kx + 2);
        const int* ey = yt + oy * (ky + 2);
        const int x0 = ex[0], nx = ex[1], y0 = ey[0], ny = ey[1];
        int accv = 1 << 21;
        for (int j = 0; j < ny; ++j) {
            const long row = (long)min(y0 + j, h - 1) * w;
            int acch = 1 << 21;
            for (int t = 0; t < nx; ++t) acch += src_at(src, off, u16, row + min(x0 + t, w - 1)) * ex[2 + t];
            accv += clip8(acch) * ey[2 + j];
        }
        const int v = clip8(accv);
        base[p * npix + i] = (unsigned char)v;
        s1 += (unsigned)v;
        s2 += (unsigned)(v * v);
    }
    __shared__ unsigned long long r1[256], r2[256];
    r1[threadIdx.x] = s1;
    r2[threadIdx.x] = s2;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            r1[threadIdx.x] += r1[threadIdx.x + s];
            r2[threadIdx.x] += r2[threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        unsigned long long* q = part + ((long)p * LA_PARTS + blockIdx.x) * 2;
        q[0] = r1[0];
        q[1] = r2[0];
    }
}

// pixel (oy, ox) of view `m` (NULL: the base image) of an S x S u8 base plane b: flip after rotation
__device__ __forceinline__ int view_at(const unsigned char* __restrict__ b, const double* __restrict__ m, int S, int oy, int ox) {
    if (m == nullptr) return b[oy * S + ox];
    if (m[6] != 0.0) ox = S - 1 - ox;
    const int mode = (int)m[7];
    if (mode == 1) return b[(long)oy * S + ox];
    if (mode == 2) return b[(long)(S - 1 - oy) * S + (S - 1 - ox)];
    if (mode == 3) return b[(long)ox * S + (S - 1 - oy)];          // ROTATE_90
    if (mode == 4) return b[(long)(S - 1 - ox) * S + oy];          // ROTATE_270
    // Geometry.c affine_transform + bilinear_filter32RGB
    const double xin = mul_rn(m[0], ox + 0.5) + mul_rn(m[1], oy + 0.5) + m[2];
    const double yin = mul_rn(m[3], ox + 0.5) + mul_rn(m[4], oy + 0.5) + m[5];
    if (xin < 0.0 || xin >= (double)S || yin < 0.0 || yin >= (double)S) return 0;
    const double xi = xin - 0.5, yi = yin - 0.5;
    const double fx = floor(xi), fy = floor(yi);
    const double dx = xi - fx, dy = yi - fy;
    const int x0 = (int)fx, y0 = (int)fy;
    const int xc0 = min(max(x0, 0), S - 1), xc1 = min(max(x0 + 1, 0), S - 1);
    const int yc0 = min(max(y0, 0), S - 1);
    const double p00 = b[(long)yc0 * S + xc0], p01 = b[(long)yc0 * S + xc1];
    double v1 = p00 + mul_rn(p01 - p00, dx), v2 = v1;
    if (y0 + 1 >= 0 && y0 + 1 < S) {
        const double p10 = b[(long)(y0 + 1) * S + xc0], p11 = b[(long)(y0 + 1) * S + xc1];
        v2 = p10 + mul_rn(p11 - p10, dx);
    }
    v1 = v1 + mul_rn(v2 - v1, dy);
    return min(max((int)v1, 0), 255);
}

// grid.y = plane p (= n * M + m) x view v; out[m][v][n] is [3][S][S] float (or [S][S] u8 with out_u8)
__global__ __launch_bounds__(256) void la_emit_kernel(const unsigned char* __restrict__ base,
                                                      const unsigned long long* __restrict__ part, int nparts,
                                                      const double* __restrict__ par, const float* __restrict__ norm, int N,
                                                      int M, int S, int A, int out_u8, void* __restrict__ out) {
    const int v = blockIdx.y % (A + 1), p = blockIdx.y / (A + 1);
    const int n = p / M, m = p - n * M;
    const long npix = (long)S * S;
    const unsigned char* b = base + p * npix;
    const double* row = v == 0 ? nullptr : par + ((long)n * A + (v - 1)) * 8;
    const long oplane = ((long)m * (A + 1) + v) * N + n;
    const bool vec = (npix & 3) == 0;
    const int np = (int)npix;                     // (npix <= 2^30: the four pixels of a thread are indexed in 32 bits)
    // the u8 values of the 4 pixels q .. q + 3 (row and column from one 32-bit division; 0 past the plane)
    auto four = [&](int q, int* v) {
        int oy = (int)((unsigned)q / (unsigned)S), ox = q - oy * S;
        for (int e = 0; e < 4; ++e) {
            v[e] = q + e < np ? view_at(b, row, S, oy, ox) : 0;
            if (++ox == S) { ox = 0; ++oy; }
        }
    };
    if (out_u8) {
        unsigned char* o = static_cast<unsigned char*>(out) + oplane * npix;
        for (int q = ((int)blockIdx.x * 256 + (int)threadIdx.x) * 4; q < np; q += (int)gridDim.x * 1024) {
            int v4[4];
            four(q, v4);
            if (vec) {
                *reinterpret_cast<unsigned*>(o + q) = (unsigned)v4[0] | (unsigned)v4[1] << 8 | (unsigned)v4[2] << 16 |
                                                      (unsigned)v4[3] << 24;
            } else {
                for (int e = 0; e < 4 && q + e < np; ++e) o[q + e] = (unsigned char)v4[e];
            }
        }
        return;
    }
    float mean[3], sd[3];
    if (norm != nullptr) {
        for (int c = 0; c < 3; ++c) { mean[c] = norm[c]; sd[c] = norm[3 + c]; }
    } else {
        // ToTensor + Normalize(None): mean and unbiased std of the un-augmented resized image from exact integer sums
        __shared__ unsigned long long r1[256], r2[256];
        const unsigned long long* q = part + (long)p * LA_PARTS * 2;
        r1[threadIdx.x] = (int)threadIdx.x < nparts ? q[threadIdx.x * 2] : 0ull;
        r2[threadIdx.x] = (int)threadIdx.x < nparts ? q[threadIdx.x * 2 + 1] : 0ull;
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if ((int)threadIdx.x < s) {
                r1[threadIdx.x] += r1[threadIdx.x + s];
                r2[threadIdx.x] += r2[threadIdx.x + s];
            }
            __syncthreads();
        }
        const unsigned long long t1 = r1[0], t2 = r2[0], cnt = (unsigned long long)npix;
        const unsigned __int128 ss = (unsigned __int128)cnt * t2 - (unsigned __int128)t1 * t1;   // n^2 x biased variance, exact
        const double var = (double)ss / ((double)cnt * (double)(cnt - 1));
        const float mu = (float)((double)t1 / (255.0 * (double)cnt));
        const float s = (float)(sqrt(var) / 255.0);
        for (int c = 0; c < 3; ++c) { mean[c] = mu; sd[c] = s; }
    }
    float* o = static_cast<float*>(out) + oplane * 3 * npix;
    for (int q = ((int)blockIdx.x * 256 + (int)threadIdx.x) * 4; q < np; q += (int)gridDim.x * 1024) {
        int v4[4];
        four(q, v4);
        float f[4];
        for (int e = 0; e < 4; ++e) f[e] = (float)v4[e] / 255.0f;
        for (int c = 0; c < 3; ++c) {
            float* oc = o + c * npix + q;
            if (vec) {
                *reinterpret_cast<f32x4*>(oc) = f32x4{(f[0] - mean[c]) / sd[c], (f[1] - mean[c]) / sd[c],
                                                      (f[2] - mean[c]) / sd[c], (f[3] - mean[c]) / sd[c]};
            } else {
                for (int e = 0; e < 4 && q + e < np; ++e) oc[e] = (f[e] - mean[c]) / sd[c];
            }
        }
    }
}

// mdesc[q] = {byte offset, h, w, 0, x index table, y index table, 0, 0}; out[q] = [npal][S][S] int64
__global__ __launch_bounds__(256) void la_mask_kernel(const unsigned char* __restrict__ src, const int* __restrict__ mdesc,
                                                      const int* __restrict__ tab, const int* __restrict__ palette, int npal,
                                                      int S, long long* __restrict__ out) {
    const int qm = blockIdx.y;
    const int* d = mdesc + qm * LA_DESC;
    const int off = d[0], h = d[1], w = d[2];
    const int* xi = tab + d[4];
    const int* yi = tab + d[5];
    int pal[8];
    for (int c = 0; c < 8; ++c) pal[c] = c < npal ? palette[c] : -1;
    const long npix = (long)S * S;
    long long* o = out + (long)qm * npal * npix;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < npix; i += (long)gridDim.x * 256) {
        const int oy = (int)(i / S), ox = (int)(i - (long)oy * S);
        const int sy = min(max(yi[oy], 0), h - 1), sx = min(max(xi[ox], 0), w - 1);
        const int v = src[off + (long)sy * w + sx];
        for (int c = 0; c < npal; ++c) o[c * npix + i] = v == pal[c] ? 1 : 0;
    }
}

long la_ws_base(long nplanes, long npix) { return (nplanes * npix + 15) & ~15L; }

}  // namespace

extern "C" {

size_t aide_loader_aug_ws_bytes(int nplanes, int S) {
    if (nplanes <= 0 || S <= 0) return 0;
    return (size_t)(la_ws_base(nplanes, (long)S * S) + (long)nplanes * LA_PARTS * 2 * sizeof(unsigned long long));
}

int aide_loader_aug(const void* src, const int* desc, const int* tab, const double* par, const float* norm, int N, int M,
                    int S, int augno, int out_u8, void* out, void* ws, hipStream_t stream) {
    if (!src || !desc || !tab || !out || !ws) return AIDE_ERR_ARG;
    if (N <= 0 || M <= 0 || S <= 0 || augno < 0 || augno > 4) return AIDE_ERR_ARG;
    if (augno > 0 && !par) return AIDE_ERR_ARG;
    if ((reinterpret_cast<uintptr_t>(ws) & 15) != 0 || (!out_u8 && (reinterpret_cast<uintptr_t>(out) & 15) != 0))
        return AIDE_ERR_ARG;
    const long P = (long)N * M, npix = (long)S * S;
    if (P * (augno + 1) > 65535 || npix > (1L << 30)) return AIDE_ERR_ARG;
    unsigned char* base = static_cast<unsigned char*>(ws);
    unsigned long long* part = reinterpret_cast<unsigned long long*>(base + la_ws_base(P, npix));
    const int nparts = (int)min((npix + 255) / 256, (long)LA_PARTS);
    AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, (double)P * npix * 2.0, la_resize_kernel, dim3(nparts, (unsigned)P), dim3(256), 0,
                      stream, static_cast<const unsigned char*>(src), desc, tab, S, base, part);
    const unsigned nb = (unsigned)min((npix + 1023) / 1024, 65535L);
    AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, (double)P * (augno + 1) * npix * (out_u8 ? 1.0 : 12.0), la_emit_kernel,
                      dim3(nb, (unsigned)(P * (augno + 1))), dim3(256), 0, stream, base, part, nparts, par, norm, N, M, S,
                      augno, out_u8, out);
    return aide_launch_status();
}

int aide_loader_mask_onehot(const void* src, const int* desc, const int* tab, const int* palette, int nplanes, int S,
                            int npal, long long* out, hipStream_t stream) {
    if (!src || !desc || !tab || !palette || !out) return AIDE_ERR_ARG;
    if (nplanes <= 0 || nplanes > 65535 || S <= 0 || npal <= 0 || npal > 8) return AIDE_ERR_ARG;
    const long npix = (long)S * S;
    const unsigned nb = (unsigned)min((npix + 255) / 256, 4096L);
    AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, (double)nplanes * npix * (1.0 + 8.0 * npal), la_mask_kernel, dim3(nb, (unsigned)nplanes),
                      dim3(256), 0, stream, static_cast<const unsigned char*>(src), desc, tab, palette, npal, S, out);
    return aide_launch_status();
}

}  // extern "C"
