// Test-time augmentation on the device (gfx950): the eight flips and quarter turns of an image as exact permutations.
//
// A view code is v = r + 4 f (r = 0 .. 3 quarter turns, f = 0 / 1 a flip of the last axis first):
//   view_v(x) = torch.rot90(torch.flip(x, [-1]) if f else x, r, (-2, -1)),
// so pixel (i, j) of the [H][W] input frame sits at `view_pos` in the view frame ([W][H] for odd r).
//   aide_view_stack     x[N][C][H][W] -> y[V][N][C][.][.], every view of the stack from one read of x
//   aide_ensemble_vote  K members' logits, each in its own view frame -> the mean soft-max in the input frame and its
//                       first-maximum label; members are added in the order given, so the bytes repeat from call to call
// Both walk 32 x 32 tiles of the input frame.  An unrotated member's rows are rows of the frame (read forwards or
// backwards); a rotated member's rows are its columns, so its tile goes through a padded LDS tile (33 floats per row:
// ds_write_b32 / ds_read_b32 bank = dword % 32, the transposed access touches 32 banks) and global memory is
// always walked along rows of whichever frame is being read or written.
#include "common.h"

namespace {

constexpr int TS = 32;          // tile edge
constexpr int TP = TS + 1;      // padded LDS row
constexpr int MAXC = 8;         // = aide_seg_max_classes()
constexpr int MAXM = 16;        // views of a stack / members of a vote

struct ViewPos { int a, b; };

// where pixel (i, j) of the [H][W] input frame lies in the frame of view `code`
__device__ __forceinline__ ViewPos view_pos(int code, int H, int W, int i, int j) {
    if (code & 4) j = W - 1 - j;
    switch (code & 3) {
        case 0: return {i, j};
        case 1: return {W - 1 - j, i};
        case 2: return {H - 1 - i, W - 1 - j};
        default: return {j, H - 1 - i};
    }
}

// Thread t of 256 and its q-th (0 .. 3) pixel of the tile at (i0, j0), ordered so that a wave walks a ROW of the frame
// of view `code`: lanes run along j for an unrotated view and along i for a rotated one.
//   ok: the pixel is inside the image; off: its offset in a plane of the view frame; lds: its slot in the padded tile
struct TileRef { bool ok; int off, lds; };
__device__ __forceinline__ TileRef tile_ref(int code, int H, int W, int i0, int j0, int q) {
    const int fast = threadIdx.x & (TS - 1), slow = (threadIdx.x >> 5) + 8 * q;
    const int li = (code & 1) ? fast : slow, lj = (code & 1) ? slow : fast;
    const int i = i0 + li, j = j0 + lj;
    const ViewPos p = view_pos(code, H, W, i, j);
    return {i < H && j < W, p.a * ((code & 1) ? H : W) + p.b, li * TP + lj};
}

struct Codes { int v[MAXM]; };

__device__ __forceinline__ void tile_origin(long blk, int tiles_i, int tiles_j, long& img, int& i0, int& j0) {
    const long per = (long)tiles_i * tiles_j;
    img = blk / per;
    const int t = (int)(blk - img * per);
    i0 = (t / tiles_j) * TS;
    j0 = (t % tiles_j) * TS;
}

// one workgroup = one tile of one plane (n, c): read once, written V times
__global__ __launch_bounds__(256) void view_stack_kernel(const float* __restrict__ x, long x_bs, float* __restrict__ y, long y_bs,
                                                         const Codes codes, int V, int N, int C, int H, int W, int tiles_i,
                                                         int tiles_j) {
    __shared__ float tile[TS * TP];
    long plane;
    int i0, j0;
    tile_origin(blockIdx.x, tiles_i, tiles_j, plane, i0, j0);
    const long n = plane / C, c = plane - n * C;
    const long HW = (long)H * W;
    const float* xp = x + n * x_bs + c * HW;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const TileRef t = tile_ref(0, H, W, i0, j0, q);
        if (t.ok) tile[t.lds] = xp[t.off];
    }
    __syncthreads();
    for (int v = 0; v < V; ++v) {
        const int code = codes.v[v];
        float* yp = y + ((long)v * N + n) * y_bs + c * HW;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const TileRef t = tile_ref(code, H, W, i0, j0, q);
            if (t.ok) yp[t.off] = tile[t.lds];
        }
    }
}

struct VoteArgs {
    const float* z[MAXM];
    int code[MAXM];
    int K, H, W, tiles_i, tiles_j;
    long l_bs, p_bs;
    float inv_k;
    long long* labels;
    float* probs;
};

// one workgroup = one tile of one image, four pixels per thread; the per-class sums stay in registers across the members
template <int C>
__global__ __launch_bounds__(256) void ensemble_vote_kernel(const VoteArgs a) {
    __shared__ float tile[C * TS * TP];
    long n;
    int i0, j0;
    tile_origin(blockIdx.x, a.tiles_i, a.tiles_j, n, i0, j0);
    const int H = a.H, W = a.W, HW = H * W;
    TileRef own[4];                                  // this thread's output pixels: the identity view's
#pragma unroll
    for (int q = 0; q < 4; ++q) own[q] = tile_ref(0, H, W, i0, j0, q);
    float sum[4][C];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int c = 0; c < C; ++c) sum[q][c] = 0.f;
    for (int k = 0; k < a.K; ++k) {
        const int code = a.code[k];
        const float* zn = a.z[k] + n * a.l_bs;
        float z[C], p[C], lse;
        if (code & 1) {                              // rotated: rows of the member -> padded tile -> this thread's pixels
            __syncthreads();                         // the reads of an earlier rotated member are over
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const TileRef t = tile_ref(code, H, W, i0, j0, q);
                if (t.ok) {
#pragma unroll
                    for (int c = 0; c < C; ++c) tile[c * TS * TP + t.lds] = zn[(long)c * HW + t.off];
                }
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (!own[q].ok) continue;
                soft_terms<C>(tile + own[q].lds, TS * TP, z, p, lse);
#pragma unroll
                for (int c = 0; c < C; ++c) sum[q][c] = __fadd_rn(sum[q][c], p[c]);     // never contracted with the soft-max
            }
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const TileRef t = tile_ref(code, H, W, i0, j0, q);
                if (!t.ok) continue;
                soft_terms<C>(zn + t.off, HW, z, p, lse);
#pragma unroll
                for (int c = 0; c < C; ++c) sum[q][c] = __fadd_rn(sum[q][c], p[c]);
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (!own[q].ok) continue;
        int best = 0;
        float sb = sum[q][0];
#pragma unroll
        for (int c = 1; c < C; ++c)
            if (sum[q][c] > sb) { sb = sum[q][c]; best = c; }
        a.labels[n * HW + own[q].off] = best;
        if (a.probs) {
#pragma unroll
            for (int c = 0; c < C; ++c) a.probs[n * a.p_bs + (long)c * HW + own[q].off] = __fmul_rn(sum[q][c], a.inv_k);
        }
    }
}

// codes 0 .. 7; a quarter turn (odd r) needs a square image
bool load_codes(const int* views, int count, int H, int W, int* out) {
    if (!views || count < 1 || count > MAXM) return false;
    for (int k = 0; k < count; ++k) {
        if (views[k] < 0 || views[k] > 7 || ((views[k] & 1) && H != W)) return false;
        out[k] = views[k];
    }
    return true;
}

bool extent_ok(int N, int C, int H, int W) {
    return N >= 1 && C >= 1 && H >= 1 && W >= 1 && (double)N * C * H * W < 2147483648.0;
}

}  // namespace

extern "C" {

int aide_view_stack(const float* x, int64_t x_bs, float* y, int64_t y_bs, const int* views, int V, int N, int C, int H, int W,
                    hipStream_t stream) {
    Codes codes;
    if (!x || !y || !extent_ok(N, C, H, W) || !load_codes(views, V, H, W, codes.v)) return AIDE_ERR_ARG;
    const int ti = (H + TS - 1) / TS, tj = (W + TS - 1) / TS;
    const long blocks = (long)N * C * ti * tj;                      // <= N * C * H * W < 2^31
    AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 4.0 * (1 + V) * N * C * H * W, view_stack_kernel, dim3((unsigned)blocks), dim3(256), 0, stream,
                      x, (long)x_bs, y, (long)y_bs, codes, V, N, C, H, W, ti, tj);
    return aide_launch_status();
}

int aide_ensemble_vote(const float* const* logits, const int* views, int K, int64_t l_bs, int N, int C, int H, int W,
                       long long* labels, float* probs, int64_t p_bs, hipStream_t stream) {
    VoteArgs a;
    if (!logits || !labels || C < 2 || C > MAXC || !extent_ok(N, C, H, W) || !load_codes(views, K, H, W, a.code))
        return AIDE_ERR_ARG;
    for (int k = 0; k < K; ++k) {
        if (!logits[k]) return AIDE_ERR_ARG;
        a.z[k] = logits[k];
    }
    a.K = K; a.H = H; a.W = W; a.tiles_i = (H + TS - 1) / TS; a.tiles_j = (W + TS - 1) / TS;
    a.l_bs = (long)l_bs; a.p_bs = (long)p_bs; a.inv_k = (float)(1.0 / K); a.labels = labels; a.probs = probs;
    const dim3 grid((unsigned)((long)N * a.tiles_i * a.tiles_j));
    const double bytes = 4.0 * K * N * C * H * W + 8.0 * N * H * W + (probs ? 4.0 * N * C * H * W : 0.0);
    aide_pick<2, 3, 4, 5, 6, 7, 8>(C, [&](auto cc) {
        AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, bytes, ensemble_vote_kernel<decltype(cc)::value>, grid, dim3(256), 0, stream, a);
    });
    return aide_launch_status();
}

}  // extern "C"
