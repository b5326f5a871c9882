// 3x3 / pad 1 convolution, Winograd F(2x2, 3x3) on fp32 MFMA (gfx950).  Forward and dgrad.
//
// Replaces the same reference ops as conv3x3.hip (nn.Conv2d(ci, co, 3, padding=1) forward and its
// autograd dgrad: models_twomodalinputs/netblocks.py:17,24,26) for the layers where it is faster.
//
//   Y = A^T [ sum_ci (G g G^T) (.) (B^T d B) ] A        d: 4x4 input tile, g: 3x3 filter, Y: 2x2 outputs
//
// 16 multiplies per (tile, ci, co) instead of 36: the direct kernels already sit at the power-limited
// MFMA ceiling (~130 TFLOP/s), so the only way to go faster in exact-fp32 arithmetic is to execute
// fewer MFMAs.  Per transform position p (16 of them) the contraction over input channels is a plain
// GEMM  M[p][co][tile] += U[p][ci][co] * V[p][ci][tile]  on v_mfma_f32_32x32x2_f32.
//   * workgroup = 4 waves = 64 output channels x 64 tiles (8x8 tiles = 16x16 pixels); a wave owns
//     32 co x 32 tiles x 16 positions = 16 accumulators (256 registers, one wave per SIMD);
//   * filters arrive pre-transformed (aide_conv3x3_wino_pack_multi: U[ci/8][16][co][8 ci]); the input transform runs
//     inside the kernel: raw halo tile -> LDS, each lane turns one (ci, tile) 4x4 patch into 16 values
//     (32 adds) and scatters them to V[p][tile][ci]; the output transform (24 adds per 2x2) is
//     per-lane on the accumulators, no cross-lane traffic;
//   * raw tile, V and the filters U[p][co][ci] are double buffered in LDS and issued in the shadow of the MFMAs (one MFMA
//     per slot).  The layouts are NOT conflict-free: the dword patch reads are 2-way (see RCS below), and so are the 16-byte
//     fragment reads of U and V (a lane's fragment starts 32 bytes after its neighbour's: the 16 lanes of a read group span
//     512 bytes = two bank rows).  Layouts without these conflicts, and filter fragments loaded global -> registers, were
//     built and measured: 1-4 % and a further 0-5 % off the kernel alone, nothing in the training step
//     (profiles/wino2_paths.md), so they are not here;
//   * the fixed part of a workgroup follows conv3x3_wino4.hip: accumulators zeroed by fenced instructions in the shadow of
//     the prologue's loads, bias and old outputs as batched buffer loads, outputs through one buffer descriptor per wave
//     whose range check is the only guard.
// fp32 F(2x2,3x3) has a forward error of a few ulp (|B|,|A| entries are 0/+-1, G has 1/2): the parity
// tests hold it to the same 2e-5 as the direct kernels.
#include "common.h"

namespace {

// buffer store with a 32-bit per-lane byte offset + scalar offset (the loads: common.h); voff = BUF_OOB drops the lane's store
__device__ __forceinline__ void buf_store_f32x2(f32x2 v, __amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, v), r, voff, soff, 0);
}

struct WinoArgs {
    const float* x;
    const float* u;      // [Cin_pad/8][16][Cout][8]
    const float* bias;
    float* y;
    long x_bs, y_bs, split_stride;
    int N, Cin, H, W, Cout;
    int tiles_w, tiles_h, n_co_tiles, splitk, chunks_total, accumulate;
};

constexpr int WCK = 8;                    // input channels per stage
constexpr int WTCO = 64;                  // output channels per workgroup
constexpr int RROWS = 18, RRS = 24;       // raw halo tile: 18 rows, row = [3 pad][-1][0..15][16][3 pad]
constexpr int RCS = RROWS * RRS + 8;      // raw channel stride 440 = 24 (mod 32): the 32 lanes (8 ci x 4 tj) of a half-wave read
                                          // banks 24 ci + 2 tj -- 16 distinct ones, ci and ci + 4 collide: 2-way
constexpr int RAWL = WCK * RCS;           // 3520 floats
constexpr int VL = 16 * 64 * WCK;         // V[p][tile][ci]   (ci minor: one ds_read_b128 = 4 k-steps)
constexpr int UL = 16 * WTCO * WCK;       // U[p][co][ci]
constexpr int WBUF = RAWL + VL + UL;      // one stage set (19904 floats = 79.6 KB)

__global__ __launch_bounds__(256, 1) void conv3x3_wino_kernel(const WinoArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];       // 2 * WBUF floats
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);         // wave-uniform (scalar) roles
    const int half = lane >> 5, j = lane & 31;
    const int wave_m = wid >> 1, wave_n = wid & 1;

    int b = xcd_remap(blockIdx.x, gridDim.x);
    const int co_tile = b % a.n_co_tiles; b /= a.n_co_tiles;
    const int split = b % a.splitk;       b /= a.splitk;
    const int tw = b % a.tiles_w;         b /= a.tiles_w;
    const int th = b % a.tiles_h;
    const int n = b / a.tiles_h;
    const int h0 = th * 16, w0 = tw * 16, co0 = co_tile * WTCO;
    const int HW = a.H * a.W;

    const int cps = (a.chunks_total + a.splitk - 1) / a.splitk;
    const int c_begin = split * cps;
    const int c_end = min(c_begin + cps, a.chunks_total);

    // ---- staging descriptors (tile-invariant per workgroup) ----
    // raw interior: CK x 18 rows x 4 float4 = 576 units; raw edges: CK x 18 x 2 dwords = 288 units
    constexpr int NRB = 3, NRC = 2, NU = UL / 4 / 256;      // 3 + 2 + 8 global loads per thread per chunk
    unsigned offB[NRB], ldsB[NRB], offC[NRC], ldsC[NRC], offU[NU];
#pragma unroll
    for (int e = 0; e < NRB; ++e) {
        int q = tid + e * 256;
        if (q >= WCK * RROWS * 4) q -= 256;                // spare lanes repeat a unit (same data, same slot):
        const int c = q / (RROWS * 4), rem = q - c * (RROWS * 4), r = rem / 4, s4 = rem - r * 4;   // no predicate
        const int ih = h0 - 1 + r, iw = w0 + 4 * s4;
        const bool ok = ih >= 0 && ih < a.H && iw < a.W;
        offB[e] = ok ? (unsigned)(c * HW + r * a.W + 1 + 4 * s4) * 4u : BUF_OOB;
        ldsB[e] = (unsigned)(c * RCS + r * RRS + 4 + 4 * s4);
    }
#pragma unroll
    for (int e = 0; e < NRC; ++e) {
        int q = tid + e * 256;
        if (q >= WCK * RROWS * 2) q -= 256;
        const int c = q / (RROWS * 2), rem = q - c * (RROWS * 2), r = rem / 2, side = rem - r * 2;
        const int ih = h0 - 1 + r, iw = side ? w0 + 16 : w0 - 1;
        const bool ok = ih >= 0 && ih < a.H && iw >= 0 && iw < a.W;
        offC[e] = ok ? (unsigned)(c * HW + r * a.W + (side ? 17 : 0)) * 4u : BUF_OOB;
        ldsC[e] = (unsigned)(c * RCS + r * RRS + (side ? 20 : 3));
    }
#pragma unroll
    for (int v = 0; v < NU; ++v) {
        const int f = tid + v * 256;                       // float4 index inside the [16][64 co][8 ci] block
        const int pp = f / (WTCO * WCK / 4), w4 = f - pp * (WTCO * WCK / 4);
        offU[v] = (unsigned)(pp * a.Cout * WCK + w4 * 4) * 4u;
    }
    const __amdgpu_buffer_rsrc_t xrs =
        make_rsrc(a.x + (long)n * a.x_bs + (long)h0 * a.W + w0 - (a.W + 1));
    const __amdgpu_buffer_rsrc_t urs = make_rsrc(a.u + (long)co0 * WCK);

    f32x4 rb[NRB], ru[NU];
    float rc[NRC];
    // Staging helpers carry NO vector-ALU work: the fp32 MFMA shares the VALU pipe, every v_* between
    // two MFMAs costs ~5 cycles plus ~13 for the first one in a slot (tools/ubench/mfma_shadow.hip),
    // whereas LDS, VMEM and scalar instructions issue in the MFMA's shadow.  Chunks past the end of
    // this split re-read the last chunk (scalar min); their data is stored but never consumed.
    auto fetch_raw = [&](int l, int chunk) {               // l < NRB + NRC, compile-time
        const unsigned xs = (unsigned)(min(chunk, c_end - 1) * WCK) * (unsigned)HW * 4u;
        if (l < NRB) rb[l] = buf_load_f32x4(xrs, offB[l], xs);
        else rc[l - NRB] = buf_load_f32(xrs, offC[l - NRB], xs);
    };
    auto put_raw = [&](int l, float* raw) {
        if (l < NRB) *reinterpret_cast<f32x4*>(raw + ldsB[l]) = rb[l];
        else raw[ldsC[l - NRB]] = rc[l - NRB];
    };
    auto fetch_u = [&](int v, int chunk) {
        const unsigned us = (unsigned)min(chunk, c_end - 1) * 16u * (unsigned)a.Cout * (unsigned)WCK * 4u;
        ru[v] = buf_load_f32x4(urs, offU[v], us);
    };
    auto put_u = [&](int v, float* ubuf) { *reinterpret_cast<f32x4*>(ubuf + (tid + v * 256) * 4) = ru[v]; };

    // Input transform B^T d B of the thread's two (ci, tile) items per chunk, 4x4 patch -> 16 values each.
    // The two items live in the two halves of f32x2 registers, so every add is one v_pk_add_f32
    // (32 VALU instructions per chunk instead of 64), and the adds are issued as ONE cluster:
    //   xf_read(i)  : td[i] <- raw patch element i of both items        (2 LDS reads, no VALU)
    //   xf_math()   : tt = B^T td ; to = tt B                           (32 packed adds)
    //   xf_store(o) : V[o] <- to[o] for both items                      (2 LDS stores, no VALU)
    // item e of this thread: input channel ci = lane & 7, tile (ti, tj) = (2 wid + e, lane >> 3): a wave
    // writes 64 consecutive floats of V[p][tile][ci] per position (conflict-free) and reads raw patches
    // at channel stride 440 (2-way: see RCS)
    f32x2 td[16], to[16];
    const int xci = lane & 7, xtj = lane >> 3;
    const int xr_off = xci * RCS + 4 * wid * RRS + 3 + 2 * xtj;           // item 0; item 1 is 2 rows down
    const int xw_off = (2 * wid * 8 + xtj) * WCK + xci;                   // item 0; item 1 is 8 tiles on
    auto xf_read = [&](int i, const float* raw) {
        td[i].x = raw[xr_off + (i / 4) * RRS + (i % 4)];
        td[i].y = raw[xr_off + (2 + i / 4) * RRS + (i % 4)];
    };
    auto xf_math = [&]() {
        f32x2 tt[16];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            tt[c] = td[c] - td[8 + c]; tt[4 + c] = td[4 + c] + td[8 + c];
            tt[8 + c] = td[8 + c] - td[4 + c]; tt[12 + c] = td[4 + c] - td[12 + c];
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            to[r * 4] = tt[r * 4] - tt[r * 4 + 2]; to[r * 4 + 1] = tt[r * 4 + 1] + tt[r * 4 + 2];
            to[r * 4 + 2] = tt[r * 4 + 2] - tt[r * 4 + 1]; to[r * 4 + 3] = tt[r * 4 + 1] - tt[r * 4 + 3];
        }
    };
    auto xf_store = [&](int o, float* vbuf) {
        vbuf[o * 64 * WCK + xw_off] = to[o].x;
        vbuf[o * 64 * WCK + xw_off + 8 * WCK] = to[o].y;
    };

    f32x16 acc[16];

    float* set0 = lds;
    float* set1 = lds + WBUF;
    // ---- prologue: raw[c0] + U[c0] -> set0, transform -> V0; raw[c0+1] -> set1.raw ----
#pragma unroll
    for (int l = 0; l < NRB + NRC; ++l) fetch_raw(l, c_begin);
#pragma unroll
    for (int v = 0; v < NU; ++v) fetch_u(v, c_begin);
    // The accumulators are zeroed HERE, in the shadow of the 13 loads just issued (nothing below can start before they
    // arrive).  Spelled as instructions and fenced, as in conv3x3_wino4.hip: plain assignments are free to sink behind the
    // prologue's last vector-memory wait, in front of the barrier that opens the main loop.
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int p = 0; p < 16; ++p) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float z;
            asm volatile("v_accvgpr_write_b32 %0, 0" : "=a"(z));
            acc[p][r] = z;
        }
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int l = 0; l < NRB + NRC; ++l) put_raw(l, set0);
#pragma unroll
    for (int v = 0; v < NU; ++v) put_u(v, set0 + RAWL + VL);
#pragma unroll
    for (int l = 0; l < NRB + NRC; ++l) fetch_raw(l, c_begin + 1);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 16; ++i) xf_read(i, set0);
    xf_math();
#pragma unroll
    for (int o = 0; o < 16; ++o) xf_store(o, set0 + RAWL);
#pragma unroll
    for (int l = 0; l < NRB + NRC; ++l) put_raw(l, set1);
    __syncthreads();

    // ---- main loop over channel chunks.  While the MFMAs consume (V, U) of set `cur`:
    //   * U[chunk+1] is fetched and stored into the other set,
    //   * raw[chunk+1] (already in the other set's raw area) is transformed into the other set's V,
    //   * raw[chunk+2] is fetched, and stored into THIS set's raw area (its contents were consumed by
    //     the transform of the previous iteration).
    int cur = 0;
    for (int chunk = c_begin; chunk < c_end; ++chunk) {
        float* sc = cur ? set1 : set0;
        float* sn = cur ? set0 : set1;
        const float* la = sc + RAWL + VL + (wave_m * 32 + j) * WCK + half * 4;     // U[p][co][ci]
        const float* lb = sc + RAWL + (wave_n * 32 + j) * WCK + half * 4;          // V[p][tile][ci]
        constexpr int STEPS = 16 * (WCK / 2);              // 16 positions x 4 channel pairs = 64 MFMAs
        // K order inside a chunk: step q pairs channel q (lanes 0-31) with channel q+4 (lanes 32-63), so
        // one ds_read_b128 per operand and position feeds four MFMAs (was: two ds_read_b32 per MFMA).
        // Two rotating fragment sets: position p+1 is requested while the four MFMAs of p run.
        // Consecutive MFMAs must not share an accumulator: with other instructions issued between
        // them, two dependent v_mfma_f32_32x32x2_f32 cost +43 cycles per pair (MI355X_MICROARCH.md,
        // "extra issue slot between two MFMAs on the SAME accumulator").  Positions are therefore
        // processed in pairs (p, p+1 alternating), which puts 128 cycles between dependent MFMAs.
        f32x4 a0A, b0A, a1A, b1A, a0B, b0B, a1B, b1B;
        auto frag = [&](int p, f32x4& af, f32x4& bf) {
            af = *reinterpret_cast<const f32x4*>(la + p * WTCO * WCK);
            bf = *reinterpret_cast<const f32x4*>(lb + p * 64 * WCK);
        };
        auto slot = [&](int st, const f32x4& a0c, const f32x4& b0c, const f32x4& a1c, const f32x4& b1c,
                        f32x4& a0n, f32x4& b0n, f32x4& a1n, f32x4& b1n) {
            const int g2 = st >> 3, k = st & 7, q = k >> 1;
            if (k == 0 && g2 + 1 < 8) { frag(2 * g2 + 2, a0n, b0n); frag(2 * g2 + 3, a1n, b1n); }
            if (k & 1) acc[2 * g2 + 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1c[q], b1c[q], acc[2 * g2 + 1], 0, 0, 0);
            else acc[2 * g2] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0c[q], b0c[q], acc[2 * g2], 0, 0, 0);
            // staging schedule (compile-time): only slot 24 carries vector-ALU work
            //   slots  0..12 : global fetches of U[chunk+1] (8) and raw[chunk+2] (5)
            //   slots  4..19 : patch reads (2 LDS reads each);  slot 24 : the 32 packed transform adds
            //   slots 26..41 : V stores (2 each);  44..51 : U[chunk+1] stores;  52..56 : raw[chunk+2] stores
            if (st < NU) fetch_u(st, chunk + 1);
            else if (st < NU + NRB + NRC) fetch_raw(st - NU, chunk + 2);
            if (st >= 4 && st < 20) xf_read(st - 4, sn);
            if (st == 24) xf_math();
            if (st >= 26 && st < 42) xf_store(st - 26, sn + RAWL);
            if (st >= 44 && st < 44 + NU) put_u(st - 44, sn + RAWL + VL);
            if (st >= 52 && st < 52 + NRB + NRC) put_raw(st - 52, sc);
            __builtin_amdgcn_sched_barrier(0);
        };
        frag(0, a0A, b0A); frag(1, a1A, b1A);
#pragma unroll
        for (int st = 0; st < STEPS; st += 16) {
#pragma unroll
            for (int k = 0; k < 8; ++k) slot(st + k, a0A, b0A, a1A, b1A, a0B, b0B, a1B, b1B);
#pragma unroll
            for (int k = 0; k < 8; ++k) slot(st + 8 + k, a0B, b0B, a1B, b1B, a0A, b0A, a1A, b1A);
        }
        __syncthreads();
        cur ^= 1;
    }

    // ---- output transform A^T M A per lane, + bias, store 2x2 pixels ----
    // Lane-derived values are retaken HERE from the lane id (v_mbcnt: two VALU) instead of being carried across the main loop.
    const int el = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    const int eh = el >> 5, ej = el & 31;
    // Outputs, old outputs and bias go through buffer descriptors built once per wave: a 32-bit per-lane offset plus a scalar
    // row offset instead of a 64-bit address per access, and every guard is a range check -- a lane whose 2x2 block lies
    // outside the plane carries BUF_OOB (stores dropped, loads read 0), "no bias" is a descriptor of zero length.  No
    // exec-masked branch and no select around a memory instruction.  (ez = 0, opaque to hipcc: the descriptors are built
    // here, behind the main loop, not ahead of it where their SGPRs would be live across it.)
    int ez;
    asm volatile("s_mov_b32 %0, 0" : "=s"(ez));
    const int cw = co0 + wave_m * 32 + ez;                 // first co of this wave (scalar); Cout % 64 == 0: always < Cout
    const bool add_bias = (a.bias != nullptr) && (split == 0);
    const __amdgpu_buffer_rsrc_t yrs = __builtin_amdgcn_make_buffer_rsrc(
        a.y + (long)split * a.split_stride + (long)n * a.y_bs + ez, 0, (int)BUF_OOB, 0x00020000);
    const __amdgpu_buffer_rsrc_t brs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(a.bias) + ez, 0, add_bias ? a.Cout * 4 : 0, 0x00020000);
    const int tile = wave_n * 32 + ej, ti = tile >> 3, tj = tile & 7;
    const int oh = h0 + 2 * ti, ow = w0 + 2 * tj;
    const bool pok = oh < a.H && ow < a.W;                 // H, W are even: the 2x2 block is in or out
    // byte offset of this lane's 2x2 block in row (r & 3) + 8 (r >> 2) of the wave's co block (host: planes < 2 GiB)
    const unsigned yoff = pok ? (unsigned)(4 * eh * HW + oh * a.W + ow) * 4u : BUF_OOB;
    const unsigned boff = (unsigned)eh * 16u;              // bias: co = cw + (r & 3) + 8 (r >> 2) + 4 half
    // (scalar row offsets, pinned: left to hipcc the products share a vector register with the lane offset above and every
    // access becomes a readfirstlane loop)
    const unsigned wrow = (unsigned)__builtin_amdgcn_readfirstlane(a.W * 4);
    const unsigned hw4 = (unsigned)__builtin_amdgcn_readfirstlane(HW * 4);
    const unsigned srow0 = (unsigned)__builtin_amdgcn_readfirstlane(cw * HW * 4);
    // the 16 bias values and (accumulate form) the 32 old output pairs are ONE batch of buffer loads ahead of the first
    // store, waited for once: next to their use each was a dependent load -> s_waitcnt vmcnt(0) that also waited for the
    // stores issued before it (stores count in vmcnt on gfx9)
    float bvs[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) bvs[r] = buf_load_f32(brs, boff, (unsigned)(cw + (r & 3) + 8 * (r >> 2)) * 4u);
    constexpr int RB = 8;                                  // output rows per batch of old-value loads
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int r0 = 0; r0 < 16; r0 += RB) {
        f32x2 olds[RB][2];
#pragma unroll
        for (int q = 0; q < RB; ++q) olds[q][0] = olds[q][1] = f32x2{0.f, 0.f};
        if (a.accumulate) {                                // wave-uniform
#pragma unroll
            for (int q = 0; q < RB; ++q) {
                const int r = r0 + q;
                const unsigned srow = srow0 + (unsigned)((r & 3) + 8 * (r >> 2)) * hw4;
#pragma unroll
                for (int i = 0; i < 2; ++i) olds[q][i] = buf_load_f32x2(yrs, yoff, srow + (unsigned)i * wrow);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int q = 0; q < RB; ++q) {
            const int r = r0 + q;
            const unsigned srow = srow0 + (unsigned)((r & 3) + 8 * (r >> 2)) * hw4;
            float s[2][4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float m0 = acc[c][r], m1 = acc[4 + c][r], m2 = acc[8 + c][r], m3 = acc[12 + c][r];
                s[0][c] = m0 + m1 + m2;
                s[1][c] = m1 - m2 - m3;
            }
            const float bv = bvs[r];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                f32x2 o;
                o.x = s[i][0] + s[i][1] + s[i][2] + bv;
                o.y = s[i][1] - s[i][2] - s[i][3] + bv;
                o.x += olds[q][i].x; o.y += olds[q][i].y;
                buf_store_f32x2(o, yrs, yoff, srow + (unsigned)i * wrow);
            }
            __builtin_amdgcn_sched_barrier(0);             // one row at a time
        }
    }
}

// y[n][c][p] (+)= bias[c] + sum_s slab[s][n][c][p]   (fixed summation order s = 0, 1, ...)
__global__ void wino_splitk_reduce_kernel(const float* __restrict__ slabs, long split_stride, int splitk,
                                          float* __restrict__ y, long y_bs, int C, int HW,
                                          const float* __restrict__ bias, int accumulate, long total) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (long)gridDim.x * blockDim.x) {
        const long chw = (long)C * HW;
        const long n = i / chw, rem = i - n * chw;
        float v = slabs[i];
        for (int s = 1; s < splitk; ++s) v += slabs[(long)s * split_stride + i];
        if (bias) v += bias[rem / HW];
        float* p = y + n * y_bs + rem;
        if (accumulate) v += *p;
        *p = v;
    }
}
// the same on 16-byte units (H * W, the batch stride and the slab stride multiples of 4), four slabs in flight per thread:
// the scalar loop above is a chain of dependent 4-byte loads -- 1.2 TB/s on the 16 .. 32 slabs of the 16x16 level (105 us for
// a 4 MB result in the C2 step); the additions keep their order, so the result is bit-identical
__global__ __launch_bounds__(256) void wino_splitk_reduce4_kernel(const float* __restrict__ slabs, long split_stride, int splitk,
                                                                  float* __restrict__ y, long y_bs, int C, int HW,
                                                                  const float* __restrict__ bias, int accumulate, long total4) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total4) return;
    const long chw4 = (long)C * HW / 4;
    const long n = i / chw4, rem = (i - n * chw4) * 4;
    const float* sp = slabs + i * 4;
    f32x4 v = *reinterpret_cast<const f32x4*>(sp);
    int s = 1;
    for (; s + 4 <= splitk; s += 4) {
        const f32x4 t0 = *reinterpret_cast<const f32x4*>(sp + (long)s * split_stride);
        const f32x4 t1 = *reinterpret_cast<const f32x4*>(sp + (long)(s + 1) * split_stride);
        const f32x4 t2 = *reinterpret_cast<const f32x4*>(sp + (long)(s + 2) * split_stride);
        const f32x4 t3 = *reinterpret_cast<const f32x4*>(sp + (long)(s + 3) * split_stride);
        v = (((v + t0) + t1) + t2) + t3;
    }
    for (; s < splitk; ++s) v += *reinterpret_cast<const f32x4*>(sp + (long)s * split_stride);
    if (bias) v += bias[rem / HW];
    float* p = y + n * y_bs + rem;
    if (accumulate) v += *reinterpret_cast<const f32x4*>(p);
    *reinterpret_cast<f32x4*>(p) = v;
}

// w[Co][Ci][3][3] -> uf[Ci_pad/8][16][Co][8] = G g G^T (forward) and ud[Co_pad/8][16][Ci][8] for the rotated,
// channel-transposed filter (dgrad).  One launch for all layers (descriptor table, like Adam).
struct WinoPackDesc {
    const float* w; float* uf; float* ud;
    int Co, Ci, ci_pad, co_pad;
    long block_start;
};

__device__ __forceinline__ void wino_g(const float g[9], float u[16]) {
    float t[12];                                           // G g : 4x3
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float g0 = g[c], g1 = g[3 + c], g2 = g[6 + c];
        t[c] = g0; t[3 + c] = 0.5f * (g0 + g1 + g2); t[6 + c] = 0.5f * (g0 - g1 + g2); t[9 + c] = g2;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {                          // (G g) G^T : 4x4
        const float a0 = t[r * 3], a1 = t[r * 3 + 1], a2 = t[r * 3 + 2];
        u[r * 4] = a0; u[r * 4 + 1] = 0.5f * (a0 + a1 + a2); u[r * 4 + 2] = 0.5f * (a0 - a1 + a2); u[r * 4 + 3] = a2;
    }
}

// One workgroup transforms a 32 co x 32 ci filter tile.  Every thread computes G g G^T for one (co, ci) pair per group
// (filters straight from global: the tile stays in L1 / L2) and the 16 transformed values go through LDS so that global stores are contiguous 1 KB runs of the packed
// layouts  uf [ci/8][16][Co][8 ci]  and  ud [co/8][16][Ci][8 co]  (4 groups of 8 channels each).
constexpr int WP_T = 32;
__global__ __launch_bounds__(256) void wino_pack_multi_kernel(const WinoPackDesc* __restrict__ descs, int n) {
    __shared__ __attribute__((aligned(16))) float ot[16 * 256];   // [p][256 pairs]
    const long blk = blockIdx.x;
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (descs[mid].block_start <= blk) lo = mid; else hi = mid - 1;
    }
    const WinoPackDesc d = descs[lo];
    const int tid = threadIdx.x;
    const int tiles_ci = (d.Ci + WP_T - 1) / WP_T;
    const int tb = (int)(blk - d.block_start);
    const int co0 = (tb / tiles_ci) * WP_T, ci0 = (tb % tiles_ci) * WP_T;
    const int nci = min(WP_T, d.Ci - ci0);               // valid input channels of this tile
    float g[9], u[16];
    const int lo3 = tid & 7, hi5 = tid >> 3;
    for (int grp = 0; grp < 8; ++grp) {
        const bool fwd = grp < 4;
        const int q = grp & 3;
        float* dst = fwd ? d.uf : d.ud;
        if (dst == nullptr) continue;                    // uniform
        // forward: 8 ci (group q) x 32 co, pair = (co = hi5, ci = 8q + lo3); dgrad: 8 co x 32 ci
        const int co = fwd ? hi5 : 8 * q + lo3, ci = fwd ? 8 * q + lo3 : hi5;
        const bool live = fwd ? (ci0 + 8 * q < d.ci_pad) : (co0 + 8 * q < d.co_pad);   // uniform
        if (!live) continue;
        {   // straight from global (zero outside [Co] x [Ci]): the tile is read by 8 groups and stays in L1 / L2
            const bool in = co0 + co < d.Co && ci < nci;
            const float* wp = d.w + ((long)(co0 + co) * d.Ci + ci0 + ci) * 9;
#pragma unroll
            for (int t = 0; t < 9; ++t) g[t] = in ? wp[fwd ? t : 8 - t] : 0.f;
        }
        wino_g(g, u);
#pragma unroll
        for (int p = 0; p < 16; ++p) ot[p * 256 + tid] = u[p];
        __syncthreads();
        // 16 runs of 256 floats: run p starts at ((group * 16 + p) * C + c0) * 8, C = Co (fwd) / Ci (dgrad)
        const int C = fwd ? d.Co : d.Ci, c0 = fwd ? co0 : ci0;
        const long gbase = (long)((fwd ? ci0 : co0) / 8 + q) * 16;
        const int nrun = min(WP_T, C - c0) * 8;          // floats per run that exist (multiple of 8)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int f = tid + k * 256, p = f >> 6, x4 = (f & 63) * 4;
            if (x4 < nrun)
                *reinterpret_cast<f32x4*>(dst + ((gbase + p) * C + c0) * 8 + x4) =
                    *reinterpret_cast<const f32x4*>(ot + p * 256 + x4);
        }
        __syncthreads();
    }
}

}  // namespace

extern "C" {

// The Winograd path needs even H and W, W % 4 == 0 (16-byte rows), Cout % 64 == 0 and Cin % 8 == 0.
int aide_conv3x3_wino_supported(int Cin, int H, int W, int Cout) {
    return (H % 2 == 0 && W % 4 == 0 && Cout % 64 == 0 && Cin % 8 == 0) ? 1 : 0;
}

// split-K factor chosen for a problem (>= 1); slabs need aide_conv3x3_ws_bytes(N,H,W,Cout,splitk).
int aide_conv3x3_wino_splitk(int N, int Cin, int H, int W, int Cout) {
    const long nb = (long)((H + 15) / 16) * ((W + 15) / 16) * N * (Cout / 64);
    const int chunks = Cin / 8;
    int s = 1;
    while (nb * s < 200 && s * 2 <= chunks / 4) s *= 2;
    return s;
}

// descs: DEVICE array of n 48-byte records {w, uf, ud (or 0), int32 Co, Ci, ci_pad, co_pad, int64
// block_start}; blocks per tensor = ceil((ci_pad*Co + co_pad*Ci) / 256).
int aide_conv3x3_wino_pack_blocks(int Co, int Ci) {
    return ((Co + WP_T - 1) / WP_T) * ((Ci + WP_T - 1) / WP_T);
}

int aide_conv3x3_wino_pack_multi(const void* descs, int n, int64_t total_blocks, hipStream_t stream) {
    if (!descs || n <= 0 || total_blocks <= 0) return AIDE_ERR_ARG;
    static_assert(sizeof(WinoPackDesc) == 48, "descriptor layout");
    AIDE_LAUNCH_TIMED(AIDE_KT_OTHER, 0.0, wino_pack_multi_kernel, dim3((unsigned)total_blocks), dim3(256), 0, stream,
                       (const WinoPackDesc*)descs, n);
    return aide_launch_status();
}

// y (+)= conv3x3(x) with Winograd-packed filters u [Cin_pad/8][16][Cout][8] (forward pack, or the dgrad pack
// with Cin/Cout swapped by the caller).  splitk from aide_conv3x3_wino_splitk (or 1); ws: split-K slabs.
int aide_conv3x3_wino(const float* x, int64_t x_bs, const float* u, const float* bias, float* y,
                      int64_t y_bs, int N, int Cin, int H, int W, int Cout, int accumulate, int splitk,
                      float* ws, hipStream_t stream) {
    if (!x || !u || !y || !aide_conv3x3_wino_supported(Cin, H, W, Cout) || x_bs % 4 || y_bs % 2)
        return AIDE_ERR_ARG;
    static AideLdsOptIn lds_opt;             // per device, status checked (common.h)
    if (int rc = lds_opt.ensure([] {
            return hipFuncSetAttribute((const void*)conv3x3_wino_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       2 * WBUF * (int)sizeof(float));
        })) return rc;
    WinoArgs a;
    a.x = x; a.u = u; a.x_bs = x_bs; a.N = N; a.Cin = Cin; a.H = H; a.W = W; a.Cout = Cout;
    a.tiles_w = (W + 15) / 16; a.tiles_h = (H + 15) / 16; a.n_co_tiles = Cout / WTCO;
    a.chunks_total = Cin / WCK;
    if (splitk < 1) splitk = 1;
    if (splitk > a.chunks_total) splitk = a.chunks_total;
    if (splitk > 1 && !ws) return AIDE_ERR_ARG;
    a.splitk = splitk;
    if (splitk > 1) {
        a.y = ws; a.y_bs = (long)Cout * H * W; a.split_stride = (long)N * Cout * H * W;
        a.bias = nullptr; a.accumulate = 0;
    } else {
        a.y = y; a.y_bs = y_bs; a.split_stride = 0; a.bias = bias; a.accumulate = (accumulate == 1);
    }
    const long nb = (long)a.tiles_w * a.tiles_h * N * a.n_co_tiles * splitk;
    AIDE_LAUNCH_TIMED(AIDE_KT_WINO2, AIDE_CONV_FLOPS(N, H, W, Cout, Cin), conv3x3_wino_kernel, dim3((unsigned)nb), dim3(256),
                      2 * WBUF * sizeof(float), stream, a);
    int rc = aide_launch_status();
    if (rc != 0) return rc;
    if (splitk > 1 && accumulate != 2) {           // accumulate == 2: the caller consumes the slabs itself
        const long total = (long)N * Cout * H * W;
        if ((H * W) % 4 == 0 && y_bs % 4 == 0) {
            AIDE_LAUNCH_TIMED(AIDE_KT_REDUCE, 0.0, wino_splitk_reduce4_kernel, dim3((unsigned)((total / 4 + 255) / 256)), dim3(256), 0, stream, ws,
                               total, splitk, y, (long)y_bs, Cout, H * W, bias, accumulate, total / 4);
        } else {
            const int blocks = (int)min((total + 255) / 256, (long)2048);
            AIDE_LAUNCH_TIMED(AIDE_KT_REDUCE, 0.0, wino_splitk_reduce_kernel, dim3(blocks), dim3(256), 0, stream, ws,
                               total, splitk, y, (long)y_bs, Cout, H * W, bias, accumulate, total);
        }
        rc = aide_launch_status();
    }
    return rc;
}

}  // extern "C"
