// Sliding-window inference on the device (gfx950): overlapping windows of an image, and the weighted blend of their soft-max maps.
//
// Along an axis of length `size` the windows of length `win` start at starts[0] = 0 < starts[1] < ... with every start in
// [0, max(0, size - win)], no gap between two starts above `win` and, when size > win, the last start at size - win: every pixel
// is covered and the windows that cover a pixel are a contiguous run of indices.  Window b = a_y * nx + a_x (raster order).
//   aide_window_stack   x[N][C][H][W] -> y[B][N][C][wh][ww], y[b][n][c][u][v] = x[n][c][min(sy + u, H - 1)][min(sx + v, W - 1)]
//   aide_window_blend   src[B][N][C][wh][ww] (logits or probabilities) -> for every output pixel, over its covering windows in
//                       increasing b: acc_c += w * p_c, den += w with w = g_h[u] * g_w[v]; labels = the first class of the
//                       largest acc_c, probs_c = acc_c / den.  No atomics, no workspace: the bytes repeat from call to call
// Both walk tiles of 8 rows x 128 columns with 256 threads: a thread owns four pixels of ONE row, 32 columns apart, so a wave
// reads and writes runs of 32 consecutive floats and the row terms (covering windows, g_h) are shared by a thread's pixels.
#include "common.h"

namespace {

constexpr int TH = 8;           // tile rows
constexpr int TW = 128;         // tile columns = 4 pixels per thread x 32 lanes
constexpr int PX = TW / 32;     // pixels per thread
constexpr int MAXC = 8;         // = aide_seg_max_classes()
constexpr int MAXS = 32;        // window starts per axis

struct Grid {
    int sy[MAXS], sx[MAXS];
    int ny, nx;
};

// A product rounded to fp32 on its own.  The library builds with -ffp-contract=fast and HIP's __fmul_rn / __fadd_rn are a
// plain product and sum that the compiler fuses after inlining; a product that has passed through the empty asm cannot be
// folded into the addition that consumes it, so a * b + c is two roundings as the host statement has them.
__device__ __forceinline__ float mul_rn(float a, float b) {
    float p = a * b;
    asm volatile("" : "+v"(p));
    return p;
}

// blk -> (plane, tile origin) for planes of tiles_i x tiles_j tiles
__device__ __forceinline__ void tile_origin(long blk, int tiles_i, int tiles_j, long& plane, int& i0, int& j0) {
    const long per = (long)tiles_i * tiles_j;
    plane = blk / per;
    const int t = (int)(blk - plane * per);
    i0 = (t / tiles_j) * TH;
    j0 = (t % tiles_j) * TW;
}

// one workgroup = one tile of one window plane (b, n, c)
__global__ __launch_bounds__(256) void window_stack_kernel(const float* __restrict__ x, long x_bs, float* __restrict__ y, long y_bs,
                                                           const Grid g, int N, int C, int H, int W, int wh, int ww, int tiles_i,
                                                           int tiles_j) {
    long plane;
    int u0, v0;
    tile_origin(blockIdx.x, tiles_i, tiles_j, plane, u0, v0);
    const long img = plane / C, c = plane - img * C;            // img = b * N + n
    const int b = (int)(img / N);
    const long n = img - (long)b * N;
    const int sy = g.sy[b / g.nx], sx = g.sx[b % g.nx];         // wave-uniform: scalar loads of the argument block
    const int u = u0 + (threadIdx.x >> 5);
    if (u >= wh) return;
    const float* xr = x + n * x_bs + c * ((long)H * W) + (long)min(sy + u, H - 1) * W;
    float* yr = y + img * y_bs + c * ((long)wh * ww) + (long)u * ww;
#pragma unroll
    for (int q = 0; q < PX; ++q) {
        const int v = v0 + (threadIdx.x & 31) + 32 * q;
        if (v < ww) yr[v] = xr[min(sx + v, W - 1)];
    }
}

struct BlendArgs {
    const float* src;
    const float* gh;
    const float* gw;
    long long* labels;
    float* probs;
    long src_bs, p_bs;
    int is_logits, N, H, W, wh, ww, tiles_i, tiles_j;
    Grid g;
};

// [lo, hi]: the windows of an axis that meet the pixels first .. last; wave-uniform when first / last are
__device__ __forceinline__ void cover_range(const int* starts, int count, int win, int first, int last, int& lo, int& hi) {
    lo = 0;
    hi = 0;
    for (int k = 0; k < count; ++k) {
        if (starts[k] + win <= first) lo = k + 1;
        if (starts[k] <= last) hi = k;
    }
}

// one workgroup = one tile of one output image; the per-class sums and the weight sum stay in registers across the windows
template <int C>
__global__ __launch_bounds__(256) void window_blend_kernel(const BlendArgs a) {
    long n;
    int i0, j0;
    tile_origin(blockIdx.x, a.tiles_i, a.tiles_j, n, i0, j0);
    const int H = a.H, W = a.W, wh = a.wh, ww = a.ww;
    const long whw = (long)wh * ww;
    const int i = i0 + (threadIdx.x >> 5);
    const int jb = j0 + (threadIdx.x & 31);
    // the covering windows of the TILE per axis (wave-uniform loop bounds: the start tables are read with scalar loads);
    // a thread's own pixels pick theirs out of these few by a range test
    int ylo, yhi, xlo, xhi;
    cover_range(a.g.sy, a.g.ny, wh, i0, min(i0 + TH, H) - 1, ylo, yhi);
    cover_range(a.g.sx, a.g.nx, ww, j0, min(j0 + TW, W) - 1, xlo, xhi);
    float acc[PX][C], den[PX];
#pragma unroll
    for (int q = 0; q < PX; ++q) {
        den[q] = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) acc[q][c] = 0.f;
    }
    for (int ky = ylo; ky <= yhi; ++ky) {
        const int u = i - a.g.sy[ky];
        if (i >= H || u < 0 || u >= wh) continue;
        const float gy = a.gh[u];
        for (int kx = xlo; kx <= xhi; ++kx) {
            const int sx = a.g.sx[kx];
            const float* sp = a.src + ((long)(ky * a.g.nx + kx) * a.N + n) * a.src_bs + (long)u * ww;
#pragma unroll
            for (int q = 0; q < PX; ++q) {
                const int j = jb + 32 * q, v = j - sx;
                if (j >= W || v < 0 || v >= ww) continue;
                float z[C], p[C], lse;
                if (a.is_logits) {
                    soft_terms<C>(sp + v, (int)whw, z, p, lse);
                } else {
#pragma unroll
                    for (int c = 0; c < C; ++c) p[c] = sp[c * whw + v];
                }
                const float w = mul_rn(gy, a.gw[v]);
#pragma unroll
                for (int c = 0; c < C; ++c) acc[q][c] = acc[q][c] + mul_rn(w, p[c]);    // two roundings: no FMA
                den[q] = den[q] + w;
            }
        }
    }
    if (i >= H) return;
    const long HW = (long)H * W;
#pragma unroll
    for (int q = 0; q < PX; ++q) {
        const int j = jb + 32 * q;
        if (j >= W) continue;
        const long off = (long)i * W + j;
        int best = 0;
        float sb = acc[q][0];
#pragma unroll
        for (int c = 1; c < C; ++c)
            if (acc[q][c] > sb) { sb = acc[q][c]; best = c; }
        a.labels[n * HW + off] = best;
        if (a.probs) {
#pragma unroll
            for (int c = 0; c < C; ++c) a.probs[n * a.p_bs + c * HW + off] = acc[q][c] / den[q];   // IEEE division
        }
    }
}

// the starts of one axis: 1 .. 32 of them, rising from 0, each in [0, max(0, size - win)], no pixel left uncovered
bool load_starts(const int* starts, int count, int size, int win, int* out) {
    if (!starts || count < 1 || count > MAXS || size < 1 || win < 1) return false;
    const int last = size > win ? size - win : 0;
    if (starts[0] != 0 || starts[count - 1] != last) return false;
    for (int k = 0; k < count; ++k) {
        if (starts[k] < 0 || starts[k] > last) return false;
        if (k && (starts[k] <= starts[k - 1] || starts[k] - starts[k - 1] > win)) return false;
        out[k] = starts[k];
    }
    for (int k = count; k < MAXS; ++k) out[k] = 0;
    return true;
}

bool load_grid(const int* starts_y, int ny, const int* starts_x, int nx, int H, int W, int wh, int ww, Grid& g) {
    if (!load_starts(starts_y, ny, H, wh, g.sy) || !load_starts(starts_x, nx, W, ww, g.sx)) return false;
    g.ny = ny;
    g.nx = nx;
    return true;
}

bool extent_ok(double n, int C, int H, int W) {
    return n >= 1 && C >= 1 && H >= 1 && W >= 1 && n * C * H * W < 2147483648.0;
}

}  // namespace

extern "C" {

int aide_window_stack(const float* x, int64_t x_bs, float* y, int64_t y_bs, int N, int C, int H, int W, int wh, int ww,
                      const int* starts_y, int ny, const int* starts_x, int nx, hipStream_t stream) {
    Grid g;
    if (!x || !y || !extent_ok(N, C, H, W) || !load_grid(starts_y, ny, starts_x, nx, H, W, wh, ww, g) ||
        !extent_ok((double)ny * nx * N, C, wh, ww))
        return AIDE_ERR_ARG;
    const int ti = (wh + TH - 1) / TH, tj = (ww + TW - 1) / TW;
    const long blocks = (long)ny * nx * N * C * ti * tj;           // <= B * N * C * wh * ww < 2^31
    AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 8.0 * ny * nx * N * C * wh * ww, window_stack_kernel, dim3((unsigned)blocks), dim3(256), 0,
                      stream, x, (long)x_bs, y, (long)y_bs, g, N, C, H, W, wh, ww, ti, tj);
    return aide_launch_status();
}

int aide_window_blend(const float* src, int src_is_logits, int64_t src_bs, int N, int C, int H, int W, int wh, int ww,
                      const int* starts_y, int ny, const int* starts_x, int nx, const float* g_h, const float* g_w,
                      long long* labels, float* probs, int64_t p_bs, hipStream_t stream) {
    BlendArgs a;
    if (!src || !g_h || !g_w || !labels || C < 2 || C > MAXC || !extent_ok(N, C, H, W) ||
        !load_grid(starts_y, ny, starts_x, nx, H, W, wh, ww, a.g) || !extent_ok((double)ny * nx * N, C, wh, ww))
        return AIDE_ERR_ARG;
    a.src = src; a.gh = g_h; a.gw = g_w; a.labels = labels; a.probs = probs;
    a.src_bs = (long)src_bs; a.p_bs = (long)p_bs; a.is_logits = src_is_logits != 0;
    a.N = N; a.H = H; a.W = W; a.wh = wh; a.ww = ww; a.tiles_i = (H + TH - 1) / TH; a.tiles_j = (W + TW - 1) / TW;
    const dim3 grid((unsigned)((long)N * a.tiles_i * a.tiles_j));
    // every window pixel inside the image is read once (at most B * N * C * wh * ww of them); labels and probabilities written once
    const double inside = (double)ny * nx * N * C * (wh < H ? wh : H) * (ww < W ? ww : W);
    const double bytes = 4.0 * inside + 8.0 * N * H * W + (probs ? 4.0 * N * C * H * W : 0.0);
    aide_pick<2, 3, 4, 5, 6, 7, 8>(C, [&](auto cc) {
        AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, bytes, window_blend_kernel<decltype(cc)::value>, grid, dim3(256), 0, stream, a);
    });
    return aide_launch_status();
}

}  // extern "C"
