/* C ABI of libaide_hip.so — the MI355X (gfx950) drop-in for AIDE's FuseUNet/UNet training hot path.
 *
 * The reference (lich0031/AIDE) has no native code and no FFI: the replaceable seam is its Python
 * nn.Module / loss-module API.  Each entry point below is what a Python binding
 * for that seam calls; the "replaces" note cites the reference call site (path:line under the
 * reference tree).  Conventions:
 *   - plain pointers + sizes only; no torch types.  All pointers are DEVICE pointers unless noted.
 *   - tensors are NCHW fp32 planes; `*_bs` is the batch stride in ELEMENTS, so a tensor may be a
 *     channel slice of a larger concatenation buffer (this is how torch.cat is eliminated).
 *   - every call is asynchronous on `stream`, never allocates, never synchronises.
 *   - return value: 0 = ok, <0 = bad argument, >0 = hipError_t of the launch.
 */
#ifndef AIDE_HIP_H
#define AIDE_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* aide_stream_t; /* == hipStream_t */

/* ---- 3x3 convolution, pad 1 (MFMA implicit GEMM) -----------------------------------------------
 * replaces nn.Conv2d(ci, co, 3, padding=1): models_twomodalinputs/netblocks.py:17,24,26 and
 * models_singlemodalinput/UNet.py:12,19,21 (forward) and autograd's convolution_backward. */
int aide_conv3x3_chunk(int Cin);                                  /* channel padding granule */
int aide_conv3x3_pack_weights(const float* w /*[Co][Ci][3][3]*/, float* wf /*[ci_pad][9][Co]*/,
                              float* wd /*[co_pad][9][Ci] or NULL*/, int Co, int Ci, int ci_pad,
                              int co_pad, aide_stream_t stream);
/* all filters of a network in one launch; descs = DEVICE array of n 48-byte records
 * {const float* w; float* wf; float* wd; int32 Co, Ci, ci_pad, co_pad; int64 block_start} */
int aide_conv3x3_pack_weights_multi(const void* descs, int n, int64_t total_blocks, aide_stream_t stream);
int aide_conv3x3_plan(int N, int Cin, int H, int W, int Cout);    /* variant | splitk<<8 */
size_t aide_conv3x3_ws_bytes(int N, int H, int W, int Cout, int splitk);
int aide_conv3x3_igemm(const float* x, int64_t x_bs, const float* wp, int ldw, const float* bias,
                       float* y, int64_t y_bs, int N, int Cin, int H, int W, int Cout, int accumulate,
                       int plan, float* ws, const float* epi_scale, int epi_relu,
                       aide_stream_t stream);   /* forward and dgrad; any Cin, Cout, H, W (partial channel tiles / chunks are
                                                   masked).  epi_scale != NULL (non-split, accumulate = 0, bias given): the
                                                   epilogue writes y = relu?(acc * epi_scale[co] + bias[co]) -- eval-mode
                                                   BatchNorm folded into the convolution (aide_bn_eval_fold) */
/* Winograd F(2x2,3x3) variant of the same convolution (forward / dgrad) for even H, W % 4 == 0,
 * Cout % 64 == 0, Cin % 8 == 0.  Filters are pre-transformed (G g G^T), channel-blocked by 8:
 * uf [ci_pad/8][16][Co][8 ci], ud [co_pad/8][16][Ci][8 co] (the tensors are allocated as [pad][16][C]). */
int aide_conv3x3_wino_supported(int Cin, int H, int W, int Cout);
int aide_conv3x3_wino_splitk(int N, int Cin, int H, int W, int Cout);
/* Winograd F(4x4,3x3) variant for the large layers (36 multiplies per 16 outputs): H % 4 == 0, W % 4 == 0,
 * H >= 16, W >= 16, Cout % 32 == 0 (a trailing half block of 32 is computed and dropped), Cin % 8 == 0; W == 16 needs an even N
 * (two images per workgroup tile).  Workgroup tile = 32 slots of 4x4 outputs: 16 x 32 pixels, or a 20 x 20 canvas (25 slots used)
 * where that covers the plane with fewer tiles (20 x 20, 40 x 40, ... planes).  Filters: uf [Ci/4][36][Co][4 ci], ud [Co/4][36][Ci][4 co]
 * (allocated as [C][36][C']); pack descriptors as above with {w, uf|0, ud|0, Co, Ci, 0, 0, block_start}.
 * splitk must divide Cin / 8. */
int aide_conv3x3_wino4_supported(int Cin, int H, int W, int Cout);
int aide_conv3x3_wino4_splitk(int N, int Cin, int H, int W, int Cout);
int aide_conv3x3_wino4_pack_blocks(int Co, int Ci);
int aide_conv3x3_wino4_pack_multi(const void* descs, int n, int64_t total_blocks, aide_stream_t stream);
/* stats_parts (NULL, or parts[Cout][aide_conv3x3_wino4_stats_parts][2]; only a non-split launch with accumulate = 0 and
 * W >= 32, AIDE_ERR_ARG otherwise): the epilogue also writes, per output channel and workgroup tile, the fp32 sum and sum
 * of squares of its pre-bias outputs -- the BatchNorm statistics for aide_bn_train_fwd_parts (netblocks.py:25,27) without a
 * pass over z.  epi_scale (NULL, or [Cout]; accumulate = 0 and bias given): y = relu?(acc * epi_scale[co] + bias[co]), the
 * folded eval-mode BatchNorm of aide_bn_eval_fold (a split launch applies it in its slab reduce).
 * in_bn_tab (NULL, or [N / in_bn_group_images][Cin][2] = (scale, shift) per image group and INPUT channel; Cin <= 1024, not
 * for W == 16): x is the RAW output z of the layer before and the loader stages relu(x * scale + shift) -- that layer's
 * BatchNorm + ReLU applied on the way in (SURVEY 8b in_prologue{bn_relu}; netblocks.py:25-28), its normalised output never
 * written: the forward-only augmentation passes of the co-teaching loop (trainchaos_proposed_30cases1labeled.py:263-281)
 * keep nothing for a backward pass.  Channels that are already activations get (1, 0).  Table: aide_bn_finalize_groups.
 * All of these are plain arguments of THIS launch: the library keeps no state between calls. */
int aide_conv3x3_wino4(const float* x, int64_t x_bs, const float* u, const float* bias, float* y, int64_t y_bs,
                       int N, int Cin, int H, int W, int Cout, int accumulate, int splitk, float* ws,
                       float* stats_parts, const float* epi_scale, int epi_relu, const float* in_bn_tab,
                       int in_bn_group_images, aide_stream_t stream);
/* descs as above with {w, uf, ud}; an entry occupies aide_conv3x3_wino_pack_blocks(Co, Ci) workgroups */
int aide_conv3x3_wino_pack_blocks(int Co, int Ci);
int aide_conv3x3_wino_pack_multi(const void* descs, int n, int64_t total_blocks, aide_stream_t stream);
int aide_conv3x3_wino(const float* x, int64_t x_bs, const float* u, const float* bias, float* y,
                      int64_t y_bs, int N, int Cin, int H, int W, int Cout, int accumulate, int splitk,
                      float* ws, aide_stream_t stream);
int aide_conv3x3_wgrad_splits(int N, int Co, int Ci, int H, int W);
size_t aide_conv3x3_wgrad_ws_bytes(int N, int Co, int Ci, int H, int W);
/* every weight-gradient entry point: `queue` = NULL (the slab reduce into dw is launched behind the kernel) or a
 * caller-owned aide_wgrad_queue_* handle (the reduce is queued for the caller's batched launch; see below) */
int aide_conv3x3_wgrad(const float* dz, int64_t dz_bs, const float* a, int64_t a_bs,
                       float* dw /*[Co][Ci][3][3]*/, int N, int Co, int Ci, int H, int W, float* ws,
                       void* queue, aide_stream_t stream);

/* Winograd form of the weight gradient (16 instead of 36 MFMA-multiplies per tile, co, ci);
 * even H, W % 4 == 0, Co >= 64, Ci >= 64.  Same outputs as aide_conv3x3_wgrad. */
int aide_conv3x3_wgrad_wino_supported(int Co, int Ci, int H, int W);
int aide_conv3x3_wgrad_wino_splits(int N, int Co, int Ci, int H, int W);
size_t aide_conv3x3_wgrad_wino_ws_bytes(int N, int Co, int Ci, int H, int W);
int aide_conv3x3_wgrad_wino(const float* dz, int64_t dz_bs, const float* a, int64_t a_bs, float* dw, int N,
                            int Co, int Ci, int H, int W, float* ws, void* queue, aide_stream_t stream);
/* stem layers (Ci <= 3; H % 4 == 0, W % 64 == 0): the nine taps folded into the GEMM's N dimension, bound by reading dz once.
 * dz fp32 or bf16-stored (dz_bf16), x fp32; round_bf16: operands rounded to bf16 when staged (the bf16 mode's contract);
 * ws / splits as for aide_conv3x3_wgrad / aide_conv3x3_wgrad_bf16 (which dispatch here themselves).
 * Replaces autograd's weight gradient of nn.Conv2d(3, C, 3, padding=1) (netblocks.py:24 in modal*_downblock1, UNet.py:19). */
int aide_conv3x3_wgrad_stem_supported(int Co, int Ci, int H, int W);
int aide_conv3x3_wgrad_stem_splits(int N, int H, int W);
int aide_conv3x3_wgrad_stem(const void* dz, int dz_bf16, int64_t dz_bs, const float* x, int64_t x_bs, float* dw,
                            int N, int Co, int Ci, int H, int W, float* ws, int splits, int round_bf16,
                            void* queue, aide_stream_t stream);
/* transposed F(4x4,3x3) for the large layers: H % 4 == 0, W % 4 == 0, H >= 8, W >= 16, Co % 32 == 0 (a trailing half tile of 32
 * is computed and dropped), Ci % 32 == 0 */
int aide_conv3x3_wgrad_wino4_supported(int Co, int Ci, int H, int W);
int aide_conv3x3_wgrad_wino4_splits(int N, int Co, int Ci, int H, int W);
size_t aide_conv3x3_wgrad_wino4_ws_bytes(int N, int Co, int Ci, int H, int W);
/* dw [Co][Ci][3][3] = sum over images and pixels; the workgroup count of the launch is an argument (target_wgs <= 0: the
 * default, half of the chip -- the kernel normally shares it with the dependent chain of the backward pass; 256 for a launch
 * that has the chip alone); ws: aide_conv3x3_wgrad_wino4_ws_bytes_t() bytes; queue: NULL or a batched-reduce queue */
int aide_conv3x3_wgrad_wino4_splits_t(int N, int Co, int Ci, int H, int W, int target_wgs);
size_t aide_conv3x3_wgrad_wino4_ws_bytes_t(int N, int Co, int Ci, int H, int W, int target_wgs);
int aide_conv3x3_wgrad_wino4_t(const float* dz, int64_t dz_bs, const float* a, int64_t a_bs, float* dw, int N,
                               int Co, int Ci, int H, int W, float* ws, int target_wgs, void* queue,
                               aide_stream_t stream);

/* ---- bf16-MFMA mode of the same convolution (BASELINE config 5: "FuseUNet bf16 MFMA path") -------------------
 * replaces the same nn.Conv2d call sites (netblocks.py:17,24,26; UNet.py:12,19,21) when the engine runs with
 * precision='bf16': operands are rounded to bf16 (RNE) while they are staged into LDS, products accumulate in fp32
 * (v_mfma_f32_32x32x16_bf16); tensors in HBM, master weights, bias, BatchNorm statistics and the loss stay fp32.
 * Filters are pre-packed to bf16: uf [ceil(Ci/16)][9][2][Co][8], ud [ceil(Co/16)][9 reversed][2][Ci][8].
 * Supported: W % 32 == 0, Cout % 32 == 0 (forward / dgrad); Co % 32 == 0, W % 32 == 0, H % 4 == 0 (weight gradient;
 * a bf16-stored x operand additionally needs Ci % 8 == 0).  The engine keeps the fp32 kernels for every other layer. */
int aide_conv3x3_bf16_supported(int Cin, int H, int W, int Cout);
int aide_conv3x3_bf16_splitk(int N, int Cin, int H, int W, int Cout);
size_t aide_conv3x3_bf16_pack_elems(int Cout, int Cin);          /* bf16 elements of one direction's pack */
/* descs = DEVICE array of n 48-byte records {const float* w; uint16_t* uf (or 0); uint16_t* ud (or 0); int32 Co, Ci, 0, 0;
 * int64 block_start}; an entry occupies aide_conv3x3_bf16_pack_blocks(Co, Ci) workgroups (64 co x 16 ci blocks through LDS) */
int aide_conv3x3_bf16_pack_blocks(int Cout, int Cin);
int aide_conv3x3_bf16_pack_multi(const void* descs, int n, int64_t total_blocks, aide_stream_t stream);
/* forward and dgrad; x_bf16 / y_bf16 = 0: fp32 tensors; 1: bf16 STORAGE of the conv output z (forward: y_bf16) or of its
 * gradient dz (dgrad: x_bf16) -- the engine's precision='bf16' mode keeps z and dz in HBM as bf16 (they are only read by
 * BatchNorm / by these kernels) */
int aide_conv3x3_bf16_mixed(const void* x, int x_bf16, int64_t x_bs, const uint16_t* u, const float* bias, void* y,
                            int y_bf16, int64_t y_bs, int N, int Cin, int H, int W, int Cout, int accumulate, int splitk,
                            float* ws, aide_stream_t stream);
int aide_conv3x3_wgrad_bf16_supported(int Co, int Ci, int H, int W);
/* co_blocks: output-channel blocks of 32 per workgroup tile -- 1 (32 co x 64 ci, 2 waves, two workgroups per CU: the
 * 32-channel first-level layers), 2 (64 co x 64 ci, 4 waves), 4 (128 co x 64 ci, 8 waves; needs Co % 128 == 0, else 2 is
 * used) or 0 = the built-in rule (1 for Co <= 32, 4 from 150 GFLOP per launch); the split count depends on it */
int aide_conv3x3_wgrad_bf16_splits(int N, int Co, int Ci, int H, int W, int co_blocks);
size_t aide_conv3x3_wgrad_bf16_ws_bytes(int N, int Co, int Ci, int H, int W, int co_blocks);
int aide_conv3x3_wgrad_bf16_mixed(const void* dz, int dz_bf16, int64_t dz_bs, const void* a, int a_bf16, int64_t a_bs,
                                  float* dw, int N, int Co, int Ci, int H, int W, float* ws, int co_blocks, void* queue,
                                  aide_stream_t stream);

/* ---- ConvTranspose2d(k=2, s=2) (learned_bilinear=True up path) ---------------------------------
 * replaces nn.ConvTranspose2d: netblocks.py:12, UNet.py:7 */
int aide_convT2x2_fwd(const float* x, int64_t x_bs, const float* w /*[Ci][Co][2][2]*/, const float* b,
                      float* y, int64_t y_bs, int N, int Ci, int Co, int H, int W, aide_stream_t stream);
int aide_convT2x2_dgrad(const float* dy, int64_t dy_bs, const float* w, float* dx, int64_t dx_bs, int N,
                        int Ci, int Co, int H, int W, aide_stream_t stream);
size_t aide_convT2x2_wgrad_ws_bytes(int N, int Ci, int Co, int H, int W);
int aide_convT2x2_wgrad(const float* x, int64_t x_bs, const float* dy, int64_t dy_bs, float* dw, int N,
                        int Ci, int Co, int H, int W, float* ws, aide_stream_t stream);

/* ---- BatchNorm2d (+ReLU) -----------------------------------------------------------------------
 * replaces nn.BatchNorm2d + nn.ReLU: netblocks.py:25,27,28,18 ; UNet.py:20,22,23,13 */
/* Workspace of the training-mode calls below: ZERO-FILLED once by the caller (it holds the arrival counters of the one-pass
 * kernels, which every launch leaves at zero) and used by ONE stream at a time. */
size_t aide_bn_ws_bytes(int C);
/* 1: a channel of N * H * W values runs in the one-pass form -- S workgroups per channel hold the values in registers, exchange
 * fp64 partial sums through the workspace (summed in slot order: bit-reproducible) and normalise from the registers: forward
 * 8 B / element, backward 12, one launch each (units of 8 values when H * W and every batch stride are multiples of 8, whatever
 * the storage types: a bf16-stored call has the statistics of the fp32-stored call on the widened tensor, bit for bit).
 * 0: the two-pass fallbacks (planes that are no multiple of 4, channels of more than 2 M values). */
int aide_bn_one_pass(int N, int C, int H, int W);
/* Eval-mode BatchNorm folded into the convolution before it (the per-case inference loop,
 * trainchaos_comparison_1case.py:233-273: net.eval(), running statistics): aide_bn_eval_fold also writes
 * fbias = conv_bias * scale + shift; an aide_conv3x3_wino4 or aide_conv3x3_igemm launch given epi_scale = scale,
 * bias = fbias (accumulate = 0) writes y = relu?(acc * scale[co] + bias[co]) straight into the activation -- no separate
 * BatchNorm pass over the conv output (a split-K aide_conv3x3_wino4 launch applies it in its slab reduce;
 * aide_conv3x3_igemm only non-split).  A launch that cannot honour the epilogue returns AIDE_ERR_ARG. */
int aide_bn_eval_fold(int C, const float* gamma, const float* beta, const float* running_mean,
                      const float* running_var, float eps, const float* conv_bias, float* scale, float* shift,
                      float* fbias, aide_stream_t stream);
/* `done` (the three aide_bn_relu_bwd* calls): NULL, or an event of aide_event_create that is recorded when dz is complete --
 * attached to the call's last dispatch instead of a record packet of its own: aide_stream_wait_event(other, done) then
 * orders another stream behind dz at ~1.4 us of this queue's time (aide_stream_order: ~5 us; tools/ubench/handover_cost.hip) */
/* aide_bn_relu_bwd with dA still in the split-K slabs [splitk][N][C][H][W] (fp32, split_stride elements apart) of the
 * data-gradient convolution that produced it (aide_conv3x3_wino4 / aide_conv3x3_wino launched with accumulate = 2): the
 * kernel sums the slabs itself, in the order of the split reduce, so that launch and one pass over dA disappear.  One-pass
 * shapes only (aide_bn_one_pass(N, C, H, W) == 1); AIDE_ERR_ARG otherwise. */
int aide_bn_relu_bwd_slabs(const float* slabs, int splitk, int64_t split_stride, const float* z, int64_t z_bs, float* dz,
                           int64_t dz_bs, int N, int C, int H, int W, const float* mean, const float* rstd,
                           const float* scale, const float* shift, int relu, float* dgamma, float* dbeta, float* dbias,
                           void* ws, void* done, aide_stream_t stream);
/* Training-mode forward a = relu?(bn(z)) (batch statistics, running-statistics update; mean / rstd / scale / shift [C] are kept
 * by the caller for the backward), the plain apply a = relu?(z * scale + shift), and the backward dA -> dz, dgamma, dbeta (+ the
 * mathematically zero conv-bias gradient).  z_bf16 / a_bf16 / dz_bf16 give the element type behind the untyped pointers (0 = fp32;
 * 1 = bf16 STORAGE, precision='bf16'); the arithmetic (fp32 per element, fp64 reductions) is the same, widening is exact, dz is
 * narrowed RNE */
int aide_bn_train_fwd_mixed(const void* z, int z_bf16, int64_t z_bs, void* a, int a_bf16, int64_t a_bs, int N, int C,
                            int H, int W, const float* gamma, const float* beta, float eps, float momentum,
                            float* running_mean, float* running_var, long long* num_batches_tracked, float* mean,
                            float* rstd, float* scale, float* shift, int relu, void* ws, aide_stream_t stream);
/* BatchNorm(train)+ReLU fed directly by the split-K slabs of the convolution before it: a conv launched with
 * accumulate = 2 leaves its partial results in ws as [splitk][N][C][H][W] fp32 (no reduce launch); this entry sums them in
 * split order (+ bias), writes z for the backward pass and normalises -- one launch and one pass over z less per layer. */
int aide_bn_train_fwd_slabs(const float* slabs, int splitk, int64_t split_stride, const float* bias, void* z, int z_bf16,
                            int64_t z_bs, void* a, int a_bf16, int64_t a_bs, int N, int C, int H, int W,
                            const float* gamma, const float* beta, float eps, float momentum, float* running_mean,
                            float* running_var, long long* num_batches_tracked, float* mean, float* rstd, float* scale,
                            float* shift, int relu, void* ws, aide_stream_t stream);
/* BatchNorm statistics from the convolution's epilogue: a forward aide_conv3x3_wino4 launch given stats_parts writes, per
 * output channel and workgroup tile, the fp32 sum and sum of squares of its pre-bias outputs to parts[Cout][nparts][2]
 * (nparts = aide_conv3x3_wino4_stats_parts); aide_bn_train_fwd_parts then normalises with ONE pass over z (replaces the
 * statistics pass of nn.BatchNorm2d in train mode, netblocks.py:25,27).  aide_bn_two_pass: 1 for the planes where that pays
 * (more than 16384 values per channel, or fewer than 64 channels), 0 for the small deep-level planes. */
int aide_conv3x3_wino4_stats_parts(int N, int H, int W);
int aide_bn_two_pass(int N, int C, int H, int W);
/* the same for ONE group of a stacked batch (Engine.run_groups): `parts` points at the group's first entry of channel 0,
 * nparts counts the group's entries, parts_stride the entries per channel of the whole launch */
int aide_bn_train_fwd_parts_strided(const void* z, int z_bf16, int64_t z_bs, void* a, int a_bf16, int64_t a_bs, int N, int C,
                                    int H, int W, const float* parts, int nparts, int parts_stride, const float* conv_bias,
                                    const float* gamma, const float* beta, float eps, float momentum, float* running_mean,
                                    float* running_var, long long* num_batches_tracked, float* mean, float* rstd,
                                    float* scale, float* shift, int relu, aide_stream_t stream);
/* BatchNorm(train)+ReLU of a STACKED batch: `groups` independent batches of N images each, stacked along the batch dimension
 * (the four detached augmentation forwards of the co-teaching loop as one pass, trainchaos_proposed_30cases1labeled.py:265-269).
 * Every group is normalised with its own batch statistics; running statistics / num_batches_tracked are updated once per
 * group, in order -- what `groups` sequential train-mode forwards leave (bit for bit in the fused single-launch and the
 * conv-epilogue-parts forms; the two-pass form sums at most 96 / groups partials per channel instead of a launch's own split
 * count, so its statistics agree to rounding, <= 1e-6 relative) -- in ONE launch sequence; mean / rstd /
 * scale / shift receive the last group's values.  Input, one of: z as it is (slabs == parts == NULL); the split-K slabs
 * [splitk][N * groups][C][H][W] of the conv before it (as aide_bn_train_fwd_slabs; z is written); the conv epilogue's
 * statistics parts[C][parts_stride][2], group g's nparts entries at g * nparts (as aide_bn_train_fwd_parts). */
int aide_bn_train_fwd_groups(const void* z, int z_bf16, int64_t z_bs, void* a, int a_bf16, int64_t a_bs, int N, int groups,
                             int C, int H, int W, const float* slabs, int splitk, int64_t split_stride,
                             const float* slab_bias, const float* parts, int nparts, int parts_stride,
                             const float* conv_bias, const float* gamma, const float* beta, float eps, float momentum,
                             float* running_mean, float* running_var, long long* num_batches_tracked, float* mean,
                             float* rstd, float* scale, float* shift, int relu, void* ws, aide_stream_t stream);
/* BatchNorm(train) WITHOUT its pass over z: the conv epilogue's statistics of a stacked batch (parts / nparts / parts_stride /
 * conv_bias as above; N = images per group) become the per-group (scale, shift) entries [tab_c0, tab_c0 + C) of
 * tab[groups][tab_C][2] -- the table the consumer convolution's loader applies (in_bn_tab of aide_conv3x3_wino4) -- and the
 * running statistics / num_batches_tracked move once per group, in order. */
int aide_bn_finalize_groups(int N, int groups, int C, int H, int W, const float* parts, int nparts, int parts_stride,
                            const float* conv_bias, const float* gamma, const float* beta, float eps, float momentum,
                            float* running_mean, float* running_var, long long* num_batches_tracked, float* mean,
                            float* rstd, float* scale, float* shift, float* tab, int tab_C, int tab_c0, aide_stream_t stream);
int aide_bn_relu_apply_mixed(const void* z, int z_bf16, int64_t z_bs, void* a, int a_bf16, int64_t a_bs, int N, int C,
                             int H, int W, const float* scale, const float* shift, int relu, aide_stream_t stream);
/* Backward of relu?(bn(z)) of a layer whose activation ALSO fed an nn.MaxPool2d(2, 2) (fuseunet.py:13-31 / :51-78, UNet.py:114): dA is
 * the gradient from the activation's other readers (the decoder's skip path), pdy [N][C][H/2][W/2] (batch stride pdy_bs) the gradient of
 * the pooled tensor; the kernel routes pdy to the arg-max of every window (activation recomputed from z exactly as the forward pass
 * computed it; first maximum in row-major window order, as nn.MaxPool2d's backward) and adds it to dA on the way in -- bit-identical to
 * aide_maxpool2x2_bwd(accumulate = 1) followed by aide_bn_relu_bwd_mixed, without the pooling backward's pass.  fp32 storage, shapes of
 * aide_bn_relu_bwd_pool_supported (one-pass form with units of 8: H even, W % 8 == 0). */
int aide_bn_relu_bwd_pool_supported(int N, int C, int H, int W);
/* ... and the forward half: BatchNorm(train)+ReLU of such a layer writes the activation AND the pooled tensor [N * groups][C][H/2][W/2]
 * (at the layer's channel 0 of the pooled buffer) -- aide_maxpool2x2_fwd's pass does not run; `groups` as aide_bn_train_fwd_groups.  fp32,
 * z as it is, the shapes of aide_bn_relu_bwd_pool_supported(N, C, H, W) with N = images per group. */
int aide_bn_train_fwd_pool(const float* z, int64_t z_bs, float* a, int64_t a_bs, float* pooled, int64_t pooled_bs, int N, int groups,
                           int C, int H, int W, const float* gamma, const float* beta, float eps, float momentum,
                           float* running_mean, float* running_var, long long* num_batches_tracked, float* mean, float* rstd,
                           float* scale, float* shift, int relu, void* ws, aide_stream_t stream);
int aide_bn_relu_bwd_pool(const float* dA, int64_t d_bs, const float* pdy, int64_t pdy_bs, const float* z, int64_t z_bs, float* dz,
                          int64_t dz_bs, int N, int C, int H, int W, const float* mean, const float* rstd, const float* scale,
                          const float* shift, int relu, float* dgamma, float* dbeta, float* dbias, void* ws, void* done,
                          aide_stream_t stream);
/* Backward of relu?(bn(z)) of the layer whose activation feeds the 1x1 head (last_conv1: fuseunet.py:41 / :88, UNet.py:120): dA =
 * sum_k head_w[k][c] * dlogits[n][k][p] is formed inside the kernel (k ascending, fused multiply-adds: the sums of aide_head1x1_bwd's dx,
 * bit for bit) -- the head's data-gradient pass does not run.  fp32 storage, shapes of aide_bn_one_pass, 1 <= K <= 8. */
int aide_bn_relu_bwd_head(const float* dlogits, int64_t dl_bs, const float* head_w, int K, const float* z, int64_t z_bs, float* dz,
                          int64_t dz_bs, int N, int C, int H, int W, const float* mean, const float* rstd, const float* scale,
                          const float* shift, int relu, float* dgamma, float* dbeta, float* dbias, void* ws, void* done,
                          aide_stream_t stream);
int aide_bn_relu_bwd_mixed(const void* dA, int dA_bf16, int64_t d_bs, const void* z, int z_bf16, int64_t z_bs, void* dz,
                           int dz_bf16, int64_t dz_bs, int N, int C, int H, int W, const float* mean, const float* rstd,
                           const float* scale, const float* shift, int relu, float* dgamma, float* dbeta, float* dbias,
                           void* ws, void* done, aide_stream_t stream);

/* ---- MaxPool2d(2,2), bilinear x2 (align_corners=True) -------------------------------------------
 * replaces nn.MaxPool2d: fuseunet.py:13-31 (calls :51-78), UNet.py:114 ;
 *          nn.Upsample(scale_factor=2, mode='bilinear', align_corners=True): netblocks.py:16 */
int aide_maxpool2x2_fwd(const float* x, int64_t x_bs, float* y, int64_t y_bs, int N, int C, int H, int W,
                        aide_stream_t stream);
int aide_maxpool2x2_bwd(const float* x, int64_t x_bs, const float* dy, int64_t dy_bs, float* dx,
                        int64_t dx_bs, int N, int C, int H, int W, int accumulate, aide_stream_t stream);
int aide_upsample2x_bilinear_fwd(const float* x, int64_t x_bs, float* y, int64_t y_bs, int N, int C, int H,
                                 int W, aide_stream_t stream);
/* the same on bf16-stored activations and activation gradients (precision='bf16'); arithmetic in fp32 */
int aide_maxpool2x2_fwd_mixed(const void* x, int x_bf16, int64_t x_bs, void* y, int y_bf16, int64_t y_bs, int N, int C,
                              int H, int W, aide_stream_t stream);
int aide_maxpool2x2_bwd_mixed(const void* x, int x_bf16, int64_t x_bs, const void* dy, int dy_bf16, int64_t dy_bs, void* dx,
                              int dx_bf16, int64_t dx_bs, int N, int C, int H, int W, int accumulate, aide_stream_t stream);
int aide_upsample2x_bilinear_bwd_mixed(const void* dy, int dy_bf16, int64_t dy_bs, void* dx, int dx_bf16, int64_t dx_bs,
                                       int N, int C, int H, int W, int accumulate, aide_stream_t stream);
int aide_upsample2x_bilinear_fwd_mixed(const void* x, int x_bf16, int64_t x_bs, void* y, int y_bf16, int64_t y_bs, int N,
                                       int C, int H, int W, aide_stream_t stream);
int aide_upsample2x_bilinear_bwd(const float* dy, int64_t dy_bs, float* dx, int64_t dx_bs, int N, int C,
                                 int H, int W, int accumulate, aide_stream_t stream);
/* inverse augmentation of logit planes (flip + PIL-exact bilinear rotation); replaces the D2H -> PIL ->
 * H2D round trip of reverseaug(): train_files/trainchaos_proposed_30cases1labeled.py:81-95.
 * par: DEVICE [N][8] doubles {a,b,c,d,e,f (PIL inverse affine), flip, mode (0 affine,1 copy,2 r180,3 r90,4 r270)} */
int aide_reverse_aug(const float* x, int64_t x_bs, float* y, int64_t y_bs, const double* par, int N, int C,
                     int H, int W, aide_stream_t stream);
int aide_fill_zero(float* p, int64_t bs, int N, int C, int H, int W, aide_stream_t stream);

/* ---- loss-module branches off the hot path ----------------------------------------------------------------------
 * aide_onehot_argmax: targets given one-hot [N][C][HW] -> int64 class indices (utils/loss2d.py:11-12).
 * aide_dice_terms_{fwd,bwd}: per image sum_k w_k (1 - (2 sum p_k t_k + s) / (sum p_k + sum t_k + s)), reduction 0 mean
 * (/N), 1 sum, 2 none.  C = 1: DiceLoss on a PROBABILITY input x [N][HW] (loss2d.py:47-61); C = 2 .. aide_seg_max_classes():
 * MulticlassDiceLoss with one-hot targets t [N][C][HW] and class weights on logits x [N][C][HW] (loss2d.py:96-104; softmax
 * inside).  class_w: HOST array of C floats, NULL = ones.
 * ws: aide_dice_terms_ws_bytes (kept by the caller between fwd and bwd).  g: [1] or [N] upstream gradient. */
int aide_onehot_argmax(const float* t, int64_t t_bs, int N, int C, int HW, long long* idx, aide_stream_t stream);
size_t aide_dice_terms_ws_bytes(int N, int HW, int C);
int aide_dice_terms_fwd(const float* x, int64_t x_bs, const float* t, int64_t t_bs, int N, int HW, int C,
                        const float* class_w /* HOST */, float smooth, int reduction, double* ws, float* per_image,
                        float* out, aide_stream_t stream);
int aide_dice_terms_bwd(const float* x, int64_t x_bs, const float* t, int64_t t_bs, int N, int HW, int C,
                        const float* class_w /* HOST */, float smooth, int reduction, const double* ws, const float* g,
                        float* dx, int64_t dx_bs, aide_stream_t stream);

/* ---- stream ordering (host pointers): fork / join between the main stream and the weight-gradient stream as plain C
 * calls, so that a recorded launch sequence (aide_amd/tape.py) can re-issue them.  aide_stream_order(ev, from, to):
 * work enqueued on `to` afterwards waits for the work enqueued on `from` so far (hipEventRecord + hipStreamWaitEvent). */
int aide_event_create(void** ev);
int aide_event_destroy(void* ev);
int aide_stream_order(void* ev, aide_stream_t from, aide_stream_t to);
/* the two halves as separate calls (record first): the free-running second lane of the forward pass records an event
 * behind each of its pooling halves and the main stream waits for it only in front of the first reader */
int aide_event_record(void* ev, aide_stream_t from);
int aide_stream_wait_event(aide_stream_t to, void* ev);

/* ---- batched slab reduce of the weight gradients (host pointers) ---------------------------------------------------
 * Every aide_conv3x3_wgrad* call leaves per-split partial results ("slabs") in its workspace; with queue = NULL it reduces
 * them into dw with a small launch of its own.  Given a caller-owned queue (aide_wgrad_queue_create) the reduce is only
 * recorded there -- the call then needs a workspace region of its own that stays untouched until the flush -- and
 * aide_wgrad_queue_flush(queue, stream) runs ONE launch over everything recorded (<= 512 layers; fixed summation order per
 * element: deterministic, identical results) on `stream`, which must be ordered after the weight-gradient kernels.
 * aide_wgrad_queue_pending: entries recorded and not yet flushed.  aide_wgrad_queue_discard: error path, drops them (they
 * point into a pass that did not finish) and returns how many.  The queue is plain host memory owned by the caller: one
 * per launch sequence (the engine keeps one per plan); the library has no global state besides the kernel timer. */
int aide_wgrad_queue_create(void** queue);
int aide_wgrad_queue_destroy(void* queue);
int aide_wgrad_queue_pending(const void* queue);
int aide_wgrad_queue_flush(void* queue, aide_stream_t stream);
int aide_wgrad_queue_discard(void* queue);

/* ---- kernel timer (measurement only; bench.py `roofline`, `critical`, `streaming`) ----------------------------------
 * While armed for a family, every launch of that family's MAIN kernel carries a start / stop HIP event pair on its own
 * stream (hipExtLaunchKernelGGL): the pair records the dispatch's begin / end timestamps -- the duration rocprofv3
 * --kernel-trace reports -- without extra packets in the queue, so the two-stream schedule of the timed steps is
 * measured as it runs.  Families (bit ids of `family_mask`): 0 conv3x3_mfma_kernel, 1 conv3x3_wino_kernel,
 * 2 conv3x3_wino4_kernel, 3 conv3x3_wgrad_kernel, 4 conv3x3_wgrad_wino_kernel, 5 conv3x3_wgrad4_kernel,
 * 6 wgrad_stem_kernel, 7 conv3x3_bf16_kernel, 8 conv3x3_wgrad_bf16_kernel, 9 convT kernels (work = algorithmic
 * direct-convolution flop, 2 N H W Co Ci 9 per launch); the streaming families 10 BatchNorm forward, 11 BatchNorm backward,
 * 12 max-pooling, 13 bilinear up-sampling (work = algorithmic bytes of the launch: every operand read once, the result written
 * once), 14 split-K / slab reduces, 15 head, loss, Adam, filter packs (work 0).  A timed launch that also carries a hand-over
 * event (`done`) records that event with a packet of its own while the timer is armed.
 * aide_ktimer_start creates the events (call it outside the timed region); aide_ktimer_read / aide_ktimer_dump need an idle
 * device; aide_ktimer_read returns the number of launches that found no free slot (>= 0) or an error (< 0). */
int aide_ktimer_start(int family_mask, int capacity);
/* the launchers' own hook (not for callers): claims an event pair (hipEvent_t*) for one launch of `family` on `stream`; 0 = not armed */
int aide_ktimer_slot(int family, double work, aide_stream_t stream, void** e0, void** e1);
int aide_ktimer_stop(void);
int aide_ktimer_arm(int family_mask);        /* re-arm after a stop, keeping what was recorded */
int aide_ktimer_read(int family, int64_t* launches, double* ms, double* flops, double* max_ms);
/* every recorded launch in launch order: family, work, begin / end of the dispatch in ms after the begin of the first recorded
 * launch, launch stream (arrays of `capacity` entries) -> number of launches written, or an error (< 0) */
int aide_ktimer_dump(int capacity, int* family, double* work, double* begin_ms, double* end_ms, uint64_t* stream);

/* ---- Spatial_Attention branch of the attention variants (fuseunetsa / UNetsa) -----------------------------------
 * replaces Spatial_Attention.forward (models_twomodalinputs/netblocks.py:68-89, models_singlemodalinput/UNet.py:85-107)
 * and `y = sa(y) * y` (fuseunet.py:139-141, UNet.py:191-200) with their autograd backward:
 *   t1 = conv1x1(y; C -> R)   t2, t3 = dilated conv3x3 (R -> R, dilation = padding)   t4 = conv1x1(t3; R -> 1)
 *   gate = sigmoid(BatchNorm2d(1)(t4))   out[c] = gate * y[c]
 * Small-channel tensors (t1..t4, gate) are dense; C-channel tensors carry a batch stride (concat slices). */
int aide_pwconv_fwd(const float* x, int64_t x_bs, const float* w /*[R][C]*/, const float* b, float* y, int64_t y_bs,
                    int N, int C, int R, int HW, aide_stream_t stream);
/* dx (+)= gate * dout + W^T dt; gate [N][HW] and dout are both NULL for a plain 1x1 dgrad */
int aide_pwconv_dgrad(const float* dt, int64_t dt_bs, const float* w, const float* gate, const float* dout,
                      int64_t dout_bs, float* dx, int64_t dx_bs, int N, int C, int R, int HW, int accumulate,
                      aide_stream_t stream);
int aide_pwconv_wgrad(const float* dt, int64_t dt_bs, const float* x, int64_t x_bs, float* dw /*[R][C]*/,
                      float* db /*[R] or NULL*/, int N, int C, int R, int HW, aide_stream_t stream);
/* dilated 3x3 (padding = dilation), dense [N][C][H][W]; transposed != 0 computes the dgrad (x = dy, y = dx, b NULL) */
int aide_dconv3x3_small(const float* x, const float* w /*[Cout][Cin][3][3]*/, const float* b, float* y, int N, int Cin,
                        int Cout, int H, int W, int dilation, int transposed, aide_stream_t stream);
int aide_dconv3x3_small_wgrad(const float* dy, const float* x, float* dw, float* db, int N, int Cout, int Cin, int H,
                              int W, int dilation, aide_stream_t stream);
/* gate = sigmoid(bn(t4)) over M = N*H*W values of the single channel; stat[2] <- {mean, rstd} */
int aide_sa_gate_fwd(const float* t4, const float* gamma, const float* beta, float* running_mean, float* running_var,
                     int64_t* num_batches_tracked, float eps, float momentum, int training, float* stat, float* gate,
                     int64_t M, aide_stream_t stream);
int aide_sa_mul(const float* gate, const float* y, int64_t y_bs, float* out, int64_t out_bs, int N, int C, int HW,
                aide_stream_t stream);
/* dt4, dgamma, dbeta from dout (gradient of out) ; ws: N*HW floats + 16 bytes */
int aide_sa_gate_bwd(const float* dout, int64_t dout_bs, const float* y, int64_t y_bs, const float* gate,
                     const float* t4, const float* stat, const float* gamma, float* dgamma, float* dbeta, float* dt4,
                     int N, int C, int HW, float* ws, aide_stream_t stream);

/* ---- 1x1 head convolution -----------------------------------------------------------------------
 * replaces last_conv1 = nn.Conv2d(64, num_classes, 1): fuseunet.py:41,89 ; UNet.py:150,164.  K = num_classes, 1 .. 8 */
size_t aide_head1x1_ws_bytes(int C, int K);
/* x_bf16 / dx_bf16 = 1: the head on a bf16-stored feature map (precision='bf16'); logits and every gradient stay fp32 */
/* The head on the RAW output z of the conv layer under it (round 6): that layer's training-mode BatchNorm + ReLU
 * (netblocks.py:27-28 in front of last_conv1, fuseunet.py:88-89) is applied while z is read -- a = max(fma(z, scale[c], shift[c]), 0), the
 * expression of the BatchNorm apply kernels -- so the layer's normalising pass never runs and its activation is never stored.  in_scale /
 * in_shift [C]: e.g. from aide_bn_finalize_groups (statistics of the conv epilogue).  aide_head1x1_wgrad_bn: dw [K][C], db [K] from dlogits
 * and the recomputed activation; the data gradient belongs to aide_bn_relu_bwd_head.  fp32; ws: aide_head1x1_ws_bytes. */
int aide_head1x1_fwd_bn(const float* z, int64_t z_bs, const float* in_scale, const float* in_shift, const float* w, const float* b,
                        float* y, int64_t y_bs, int N, int C, int K, int H, int W, aide_stream_t stream);
int aide_head1x1_wgrad_bn(const float* dy, int64_t dy_bs, const float* z, int64_t z_bs, const float* in_scale, const float* in_shift,
                          float* dw, float* db, int N, int C, int K, int H, int W, void* ws, aide_stream_t stream);
int aide_head1x1_fwd_mixed(const void* x, int x_bf16, int64_t x_bs, const float* w, const float* b, float* y,
                           int64_t y_bs, int N, int C, int K, int H, int W, aide_stream_t stream);
int aide_head1x1_bwd_mixed(const float* dy, int64_t dy_bs, const void* x, int x_bf16, int64_t x_bs, const float* w,
                           void* dx, int dx_bf16, int64_t dx_bs, float* dw, float* db, int N, int C, int K, int H, int W,
                           void* ws, aide_stream_t stream);
/* ---- fused segmentation losses / co-teaching selection -----------------------------------------
 * replaces utils/loss2d.py:5-154, utils/coteach_loss.py:94-161, utils/metrics2d.py:8-29 and the
 * inline selection of train_files/trainchaos_proposed_30cases1labeled.py:274-321.
 * The reference's modules are written for any class count (fuseunet(num_classes=...), models_twomodalinputs/
 * fuseunet.py:7,41; nn.CrossEntropyLoss(weight), utils/loss2d.py:8; softmax(...)[:, 1] in every Dice form,
 * utils/loss2d.py:44-46,65-66,96,106; MulticlassMSELoss :115-117; sharpen, trainchaos_proposed_30cases1labeled.py:97-101;
 * argmax(softmax), trainchaos_comparison_1case.py:262-264); its shipped scripts run two.  Every operator has ONE entry
 * point that takes the class count C = 2 .. aide_seg_max_classes() and picks the kernel itself: two classes run kernels of
 * their own (one sigmoid of z1 - z0 per pixel), more classes the soft-max templates; any other C is AIDE_ERR_ARG and launches
 * nothing.  Logits / pseudo labels / gradients are [N][C][HW] planes, class_w is a HOST array of C floats (NULL = ones).
 * The statistics (partials, stats) have one layout for every C, so aide_seg_loss_finalize needs no C;
 * aide_coteach_finalize takes it for the mean of the consistency map. */
int aide_seg_max_classes(void);
int aide_seg_loss_blocks(int HW);
size_t aide_seg_loss_ws_bytes(int N, int HW);
int aide_seg_stats(const float* logits, int64_t l_bs, const long long* targets, int64_t t_bs,
                   const float* class_w /* HOST */, int C, int ignore_index, const float* pseudo, int64_t p_bs,
                   const float* wmap, int64_t w_bs, int N, int HW, double* partials, aide_stream_t stream);
int aide_seg_loss_finalize(const double* partials, int N, int HW, int reduction, float w_ce, float w_dice,
                           float smooth, double* stats, float* out, float* per_image, long long* idx,
                           float* coef, float* hard_dice, aide_stream_t stream);
int aide_coteach_finalize(const double* partials1, const double* partials2, int N, int HW, int C, int variant,
                          int keep, float w_ce, float w_dice, float smooth, float rate, float w_seg,
                          float w_cor, double* stats1, double* stats2, float* loss, float* per_image1,
                          float* per_image2, long long* idx1, long long* idx2, float* coef1, float* coef2,
                          float* hard_dice, aide_stream_t stream);
int aide_seg_loss_bwd(const float* logits, int64_t l_bs, const long long* targets, int64_t t_bs,
                      const float* class_w /* HOST */, int C, int ignore_index, const float* pseudo, int64_t p_bs,
                      const float* wmap, int64_t w_bs, int N, int HW, const double* stats, const float* coef,
                      float smooth, const float* gout, int g_stride, float* dlogits, int64_t d_bs,
                      aide_stream_t stream);
int aide_ce_map(const float* logits, int64_t l_bs, const long long* targets, int64_t t_bs,
                const float* class_w /* HOST */, int C, int ignore_index, int N, int HW, float* out,
                const float* gout, float* dlogits, int64_t d_bs, aide_stream_t stream);
int aide_mse_map(const float* logits, int64_t l_bs, const float* target, int64_t q_bs, int C, int N, int HW,
                 float* out, const float* gout, float* dlogits, int64_t d_bs, aide_stream_t stream);
int aide_pseudo_label(const float* const* logits /* HOST array of K device pointers */, int K, int C,
                      int64_t l_bs, int N, int HW, float temperature, float* pl, float* wm,
                      aide_stream_t stream);

/* ---- remaining co-teaching operators (utils/coteach_loss.py:85-92, 163-196, 198-254), C = 2 .. aide_seg_max_classes() ----
 * aide_kl_map: KLbidirection, out[n][p] = KL(p1||p2) + KL(p2||p1); with gout (per-pixel upstream gradient) also
 *   the gradients w.r.t. both logit tensors.
 * aide_region_ce_fwd/_bwd: the region cross entropy of Coteachingloss_dropregionce(scale), which pools logits (per class)
 *   and targets with MaxPool2d(kernel = stride = (KH, KW), ceil_mode=True), KH = int(H / int(H * scale)) (:171-179) --
 *   ceil(H / KH) x ceil(W / KW) regions, border windows clipped.  aux (opaque, aide_region_ce_aux_bytes, kept by the caller
 *   between fwd and bwd) holds the arg-max positions and the pooled target; bwd scatters coeff[0] * mask * dCE to those
 *   positions.  2x2 windows on even H and W have kernels of their own; the entry picks them.
 * aide_select_smallest: per segment of M values the k smallest candidates (all values, or only those > 0), ties
 *   by lower index (stable argsort, :180-186 / :228-232); k = *k_in | (int64)(rr * candidates) if rr >= 0 | k_host;
 *   mask[M] marks the selection, sums[seg] = fp64 sum of sum_vals over it, ks[seg] = k.
 * aide_droppixel_map/_bwd: v = target * (KL(z1, z2) + CE(z_which, target)) on the images idx[0..ndrop) (:221-227,
 *   :240-246) and its gradient w.r.t. both logit tensors for the selected pixels (g1, g2 pre-zeroed).  ignore_index acts
 *   for C > 2 only: the two-class kernels take every non-zero target as class 1 and do not read it.
 * (Pixelcoreg_Focalloss reads channels 0 and 1 only in the reference itself, utils/reg_loss.py:70-99: two classes.) */
int aide_kl_map(const float* z1, int64_t b1, const float* z2, int64_t b2, int C, int N, int HW, float* out,
                const float* gout, float* g1, int64_t gb1, float* g2, int64_t gb2, aide_stream_t stream);
size_t aide_region_ce_aux_bytes(int C, int N, int H, int W, int KH, int KW);      /* 0: arguments out of range */
int aide_region_ce_fwd(const float* z, int64_t zb, const long long* t, int64_t tb, int C, int N, int H, int W, int KH,
                       int KW, int ignore_index, float* loss, void* aux, aide_stream_t stream);
int aide_region_ce_bwd(const float* z, int64_t zb, const void* aux, const unsigned char* mask, const float* coeff, int C,
                       int N, int H, int W, int KH, int KW, float* dz, int64_t db, aide_stream_t stream);
int aide_select_smallest(const float* sel_vals, const float* sum_vals, int64_t seg_stride, int nseg, int M,
                         int64_t k_host, double rr, const long long* k_in, int only_positive, unsigned char* mask,
                         double* sums, long long* ks, aide_stream_t stream);
int aide_droppixel_map(const float* z1, int64_t b1, const float* z2, int64_t b2, const long long* t, int64_t tb,
                       const long long* idx, int ndrop, int C, int HW, int which, int ignore_index, float* v,
                       aide_stream_t stream);
int aide_droppixel_bwd(const float* z1, int64_t b1, const float* z2, int64_t b2, const long long* t, int64_t tb,
                       const long long* idx, int ndrop, int C, int HW, int which, int ignore_index,
                       const unsigned char* mask, const float* coeff, float* g1, float* g2, aide_stream_t stream);

/* Pixelcoreg_Focalloss / _twomodel (utils/reg_loss.py:58-193): per pixel key = (1-kd)(focal1 + focal2 [+ focal3]) +
 * kd KL(1,2) (focal: gamma 2, lossweight 1), val = focal3 with three nets (z3 != NULL), tf = target as float; the
 * per-image "k smallest keys" selection is aide_select_smallest; bwd: coeff[0] * mask * d val / d logits (two nets:
 * g1, g2 of the key; three nets: g3 only, as in the reference where the ranking is not differentiated). */
int aide_pixelcoreg_map(const float* z1, const float* z2, const float* z3, const long long* t, int64_t tb, int N,
                        int HW, float kd, float* key, float* val, float* tf, aide_stream_t stream);
int aide_pixelcoreg_bwd(const float* z1, const float* z2, const float* z3, const long long* t, int64_t tb, int N,
                        int HW, float kd, const unsigned char* mask, const float* coeff, float* g1, float* g2,
                        float* g3, aide_stream_t stream);

/* per-case inference (trainchaos_comparison_1case.py:262-264): labels[n][p] = argmax(softmax(logits[n][:,p])) for
 * C = 2 .. aide_seg_max_classes(), int64 like torch.argmax; ties (also those created by the softmax rounding) -> the
 * lowest class */
int aide_label_map(const float* logits, int64_t l_bs, int C, int N, int HW, long long* labels, aide_stream_t stream);

/* ---- per-case evaluation: largest 3-D connected component, confusion sums ----------------------
 * replaces the CPU post-processing of the per-case loop: keep_largest_connected_components (skimage
 * measure.label(connectivity=1) + regionprops + argmax(area), trainchaos_comparison_1case.py:67-77, called at
 * :267-268; trainchaos_proposed_30cases1labeled.py:103-112; evalchaos_comparison_1cases.py:232) and the scores
 * Dice3d_fn / IoU3d_fn / TP_TN_FP_FN3d (evalchaos_comparison_1cases.py:116-141, 238-242).
 * Volumes have a LOGICAL shape (d0, d1, d2) and element strides (s0, s1, s2): raster order is C order of the logical
 * index, so [S,H,W] labels passed as a permute(1, 2, 0) view are scanned in the reference's [H,W,S] order. */
/* workspace of aide_keep_largest_cc3d for nvox = d0 * d1 * d2 voxels (16-byte aligned); 0 for nvox >= 2^31 */
size_t aide_lcc3d_ws_bytes(int64_t nvox);
/* out[d0][d1][d2] (uint8, contiguous) = 1 on the largest blob of v, 0 elsewhere.  Foreground: v != 0; face neighbours
 * holding the SAME value are connected; ties in voxel count go to the blob whose first voxel comes first in raster
 * order; all zeros when the volume has no positive value.  d0 * d1 * d2 < 2^31 (AIDE_ERR_ARG otherwise). */
int aide_keep_largest_cc3d(const long long* v, int64_t d0, int64_t d1, int64_t d2, int64_t s0, int64_t s1, int64_t s2,
                           unsigned char* out, void* ws, aide_stream_t stream);
/* workspace of aide_keep_largest_cc3d_classes (16-byte aligned); 0 for nvox >= 2^31 or num_classes outside 2 .. 8 */
size_t aide_lcc3d_classes_ws_bytes(int64_t nvox, int num_classes);
/* The filter per class for multi-organ volumes, C = num_classes in 2 .. 8: for every class value c in 1 .. C - 1 the largest
 * blob of the voxels equal to c (face neighbours, ties to the blob whose first voxel comes first in raster order, the rule
 * above applied per class; classes never compete).  out[d0][d1][d2] (uint8, contiguous) = c on the kept blob of class c, 0
 * elsewhere; a value outside 1 .. C - 1 (0, negative, >= C) belongs to no class and gives 0; a class that does not occur
 * leaves nothing.  For C = 2 and values in {0, 1} the bytes are aide_keep_largest_cc3d's.
 * stats: NULL, or [C][3] int64: row c = {blobs of class c, voxels of class c, voxels of the kept blob}, row 0 zeros.
 * Five launches (the first three are aide_keep_largest_cc3d's) and one memset of the control words, whatever C is; integer
 * only, so two calls give the same bytes whatever the workspace held.  AIDE_ERR_ARG before any launch for a null v / out /
 * ws, a misaligned ws, d0 * d1 * d2 >= 2^31, num_classes outside 2 .. 8; an empty volume launches nothing (stats, when
 * given, is cleared). */
int aide_keep_largest_cc3d_classes(const long long* v, int64_t d0, int64_t d1, int64_t d2,
                                   int64_t s0, int64_t s1, int64_t s2, int num_classes,
                                   unsigned char* out, long long* stats /* NULL or [C][3] */,
                                   void* ws, aide_stream_t stream);
/* ---- case post-processing: the k largest blobs with a size floor, hole filling (the single volume) ---- */
/* workspace of aide_keep_components3d (16-byte aligned); 0 for nvox >= 2^31 */
size_t aide_components3d_ws_bytes(int64_t nvox);
/* The component rule of the two filters above with a rank and a size floor.  num_classes = 0: one slot over all non-zero
 * values, 1 written (nothing when no value is positive, as aide_keep_largest_cc3d); num_classes = C in 2 .. 8: one slot per
 * class value 1 .. C - 1, the class written.  Inside a slot blobs are ordered by voxel count, larger first, ties to the blob
 * whose first voxel comes first in raster order (the key (area << 32) | (0x7fffffff - root)); kept are the first top_k[c]
 * of that order (0: all of them), and of those the ones with at least min_voxels[c] voxels.  top_k and min_voxels are HOST
 * arrays of 8 entries read before the call returns, indexed by class value (num_classes = 0: entry 1; entry 0 is ignored);
 * top_k[c] in 0 .. 8, min_voxels[c] >= 1.  top_k = 1, min_voxels = 1 gives the bytes (and stats) of the two filters above.
 * stats: NULL, or with num_classes = C [C][3] int64: row c = {blobs of class c, voxels of class c, voxels kept}, row 0 zeros.
 * Launches: 4 + max(1, max top_k) and one or two memsets; integer only, no host read, the same bytes from call to call.
 * AIDE_ERR_ARG before any launch for num_classes outside {0, 2 .. 8}, an entry out of range, null top_k / min_voxels, stats with
 * num_classes = 0, d0 * d1 * d2 >= 2^31, a null v / out / ws or a misaligned ws; an empty volume launches nothing. */
int aide_keep_components3d(const long long* v, int64_t d0, int64_t d1, int64_t d2, int64_t s0, int64_t s1, int64_t s2,
                           int num_classes, const int* top_k /* host [8] */, const long long* min_voxels /* host [8] */,
                           unsigned char* out, long long* stats /* NULL or [C][3] */, void* ws, aide_stream_t stream);
/* workspace of aide_fill_holes3d (16-byte aligned); 0 for nvox >= 2^31 */
size_t aide_fill_holes3d_ws_bytes(int64_t nvox);
/* Background: the voxels whose value is exactly 0 (v is int64, v_u8 = 0, or uint8, v_u8 = 1, with element strides).  A hole: a
 * face-connected blob of background with no voxel on a face of the volume.  slice_axis = a in 0 .. 2 (-1: none): connectivity
 * is restricted to the 2-D slices along logical axis a and "face of the volume" reads "edge of the slice".
 * num_classes = 0: out = 1 where v != 0 or the voxel lies in a hole (scipy.ndimage.binary_fill_holes(v != 0), per slice with a
 * slice axis).  num_classes = C in 2 .. 8: a class value 1 .. C - 1 is kept, a value outside 0 .. C - 1 gives 0, and a hole gets
 * class c if and only if every non-background face neighbour of the hole holds c, 1 <= c <= C - 1: a hole between two classes
 * or next to an out-of-range value stays 0.
 * stats: NULL, or [max(C, 2)][2] int64: row c = {holes filled with c, voxels filled with c}, row 0 zeros (num_classes = 0: row 1).
 * The labelling launches of the filters on the background, one launch that ORs what each blob touches into a word per root,
 * one that writes; one or two memsets; integer atomics only, no host read, the same bytes from call to call.  AIDE_ERR_ARG
 * before any launch as for aide_keep_components3d, and for v_u8 outside {0, 1} or slice_axis outside -1 .. 2. */
int aide_fill_holes3d(const void* v, int v_u8, int64_t d0, int64_t d1, int64_t d2, int64_t s0, int64_t s1, int64_t s2,
                      int num_classes, int slice_axis, unsigned char* out, long long* stats /* NULL or [max(C, 2)][2] */,
                      void* ws, aide_stream_t stream);
/* ---- labelled components and lesion-wise counts (the single volume) ----
 * Members: num_classes = 0: every voxel whose value is not 0; num_classes = C in 2 .. 8: the values 1 .. C - 1.  Face neighbours
 * of EQUAL value are connected (skimage.measure.label(v, connectivity=1)).  The blobs of all values together are numbered
 * 1 .. n in raster order (C order of the logical index) of their first voxel. */
/* workspace of aide_label_components3d (16-byte aligned): three int words per voxel (parent, area, rank), the control words and
 * one int per 1024 voxels; 0 for nvox >= 2^31 */
size_t aide_label_components3d_ws_bytes(int64_t nvox);
/* labels[d0][d1][d2] (int32, contiguous) = the number of the voxel's blob, 0 for a voxel that is no member; count[0] (int64) =
 * the number of blobs, always the true one.  props: NULL, or [max_blobs][12] int64 with max_blobs in 1 .. 2^20: row j - 1
 * describes blob j as {value, area, raster index of the first voxel, min0, min1, min2, max0 + 1, max1 + 1, max2 + 1, sum i0,
 * sum i1, sum i2} (a half-open box; centroid = sum / area); the rows from count on are zero, and with count > max_blobs the
 * table holds the first max_blobs blobs while labels and count stay complete.
 * Seven launches whatever the volume is: the three labelling launches of aide_keep_largest_cc3d, the rank of every root as a
 * prefix sum over the root flags (per-block counts, a scan of the block counts by one workgroup, per-block ranks), one write;
 * one memset when props is given.  Integer atomics only, no workgroup waits for another, no host read, the same bytes from call
 * to call whatever the workspace held.  AIDE_ERR_ARG before any launch for num_classes outside {0, 2 .. 8}, d0 * d1 * d2 >= 2^31, a
 * null count, props with max_blobs out of range, a null v / labels / ws or a misaligned ws; an empty volume launches nothing
 * (count and props, when given, are cleared). */
int aide_label_components3d(const long long* v, int64_t d0, int64_t d1, int64_t d2, int64_t s0, int64_t s1, int64_t s2,
                            int num_classes, int* labels, long long* count /* [1] */,
                            long long* props /* NULL or [max_blobs][12] */, int64_t max_blobs, void* ws, aide_stream_t stream);
/* workspace of aide_lesion_counts3d (16-byte aligned): three int words per voxel (parent, area, cover) that the two volumes use
 * one after the other, and the control words; 0 for nvox >= 2^31 */
size_t aide_lesion_counts3d_ws_bytes(int64_t nvox);
/* Both volumes (int64, logical shape (d0, d1, d2), element strides each) are labelled by the rule above.  For a blob b of one
 * volume, cover(b) = the voxels of b at which the OTHER volume agrees: its voxel is not 0 (num_classes = 0), or equals b's value
 * (num_classes = C).  b counts if and only if cover(b) >= 1 and (double)cover(b) >= overlap * (double)area(b), overlap in [0, 1].
 * out[rows][6] int64, rows = C (row c: the blobs of value c) or 2 (num_classes = 0: row 1), row 0 zeros: {target blobs, target
 * blobs that count, pred blobs, pred blobs that count, sum of cover over the target blobs (= the voxel-wise TP of the class),
 * pred voxels in blobs that do not count}.  Swapping pred and target swaps columns 0 - 1 with 2 - 3.
 * Ten launches (per volume the three labelling launches, cover, reduce) and three memsets whatever the volumes are; integer
 * atomics, one double multiply and compare per blob, no host read.  AIDE_ERR_ARG before any launch for num_classes outside
 * {0, 2 .. 8}, overlap outside [0, 1], d0 * d1 * d2 >= 2^31, a null out, and on a volume that is not empty a null pred / target /
 * ws or a misaligned ws; an empty volume clears out and launches nothing. */
int aide_lesion_counts3d(const long long* pred, int64_t p_s0, int64_t p_s1, int64_t p_s2, const long long* target,
                         int64_t t_s0, int64_t t_s1, int64_t t_s2, int64_t d0, int64_t d1, int64_t d2, int num_classes,
                         double overlap, long long* out /* [max(C, 2)][6] */, void* ws, aide_stream_t stream);
/* out[4] (int64) = {N, sum p*t, sum p, sum t} over the logical volume; p / t are int64 (x_u8 = 0) or uint8 (x_u8 = 1)
 * with element strides.  TP = out[1], FP = out[2] - out[1], FN = out[3] - out[1], TN = N - out[2] - out[3] + out[1] */
int aide_case_confusion(const void* p, int p_u8, int64_t p_s0, int64_t p_s1, int64_t p_s2, const void* t, int t_u8,
                        int64_t t_s0, int64_t t_s1, int64_t t_s2, int64_t d0, int64_t d1, int64_t d2, long long* out,
                        aide_stream_t stream);

/* ---- surface distances in millimetres: the raw sums behind RAVD, ASSD and MSSD, the CHAOS challenge's other three scores.
 * The reference reads every case's PixelSpacing and SliceThickness into `voxelspacing`
 * (evalchaos_comparison_1cases.py:181, 192-194) and never uses them; its utils/metrics3d.py is four import lines.
 * Operands as in aide_case_confusion; (sp0, sp1, sp2) = edge lengths of a voxel along the logical dims.  Foreground of an
 * operand X: X != 0 (cls < 0) or X == cls.  Border: foreground with at least one of the six face neighbours not foreground or
 * outside the volume.  D_X(v) = min over u in border(X) of sqrt(sum_k (sp_k * (v_k - u_k))^2) in fp64: exact, no chamfer. */
/* workspace of aide_surface3d_scores for nvox = d0 * d1 * d2 voxels (16-byte aligned); 0 for nvox >= 2^31 */
size_t aide_surface3d_ws_bytes(int64_t nvox);
/* out = 8 words of 8 bytes: int64 n_P, n_T (border voxels), V_P, V_T (foreground voxels); double S_PT = sum over border(P)
 * of D_T, S_TP, M_PT = max of the same values, M_TP (sums and maxima 0 where an operand has no border: the caller decides
 * from n_P and n_T).  dist: NULL, or [2][d0 * d1 * d2] in logical raster order: dist[0] = D_T at the border voxels of P,
 * dist[1] = D_P at those of T, -1.0 everywhere else (everywhere when the other operand has no border).  Five launches, no
 * floating-point atomic: two calls on the same inputs give the same bytes, whatever the workspace held.  AIDE_ERR_ARG before
 * any launch for a null p / t / out / ws, a misaligned ws, d0 * d1 * d2 >= 2^31, a spacing that is not
 * positive and finite; an empty volume only clears out.  (sp_k * d_k)^2 must stay finite in fp64: a candidate whose squared
 * distance overflows counts as no candidate. */
int aide_surface3d_scores(const void* p, int p_u8, int64_t p_s0, int64_t p_s1, int64_t p_s2,
                          const void* t, int t_u8, int64_t t_s0, int64_t t_s1, int64_t t_s2,
                          int64_t d0, int64_t d1, int64_t d2, double sp0, double sp1, double sp2,
                          int cls, void* out, double* dist, void* ws, aide_stream_t stream);
/* ---- percentiles of the surface distances (HD95) and the surface Dice at a tolerance (NSD).  A = the multiset {D_T(v) : v in
 * border(P)} (n_P values), B = {D_P(v) : v in border(T)} (n_T values), A+B their multiset union.  Percentile q of a multiset
 * of m >= 1 values x[0] <= ... <= x[m-1]: pos = (m - 1) * q / 100.0 left to right in fp64, lo = floor(pos),
 * hi = min(lo + 1, m - 1), value = x[lo] + (x[hi] - x[lo]) * (pos - lo) (numpy's 'linear' up to the rounding of pos; q = 100
 * is the maximum exactly).  The entry point selects x[lo] and x[hi] exactly; the interpolation, the max of the two directions
 * and the NSD division stay with the caller, in fp64 on the host. */
/* workspace of aide_surface3d_scores_select: that of aide_surface3d_scores, two key lists of nvox uint64 and less than 64 KiB
 * of counters and bins (<= aide_surface3d_ws_bytes(nvox) + 16 * nvox + 65536); 0 for nvox >= 2^31 */
size_t aide_surface3d_select_ws_bytes(int64_t nvox);
/* The first 17 arguments, dist and ws (of the size above) as in aide_surface3d_scores.  q[nq], tol[nt]: HOST arrays, 0 .. 4
 * entries each, read before the call returns.  out = 52 words of 8 bytes:
 *   [0..7]    the words of aide_surface3d_scores, the same bytes
 *   [8 + 2*j + k]  int64: k = 0 |{a in A : a <= tol[j]}|, k = 1 the same for B; j < nt
 *   [16 + 3*(4*s + j) + {0, 1, 2}]  set s = 0: A, 1: B, 2: A+B, percentile j < nq: int64 lo, double x[lo], double x[hi]
 * Unused words, and the percentile words when n_P == 0 or n_T == 0, are 0.  dist is byte-equal to aide_surface3d_scores's.
 * Launches 1-3 and 5 of aide_surface3d_scores; launch 4 also appends every distance it produces to a per-operand list of
 * uint64 keys (the bit pattern of a non-negative double orders like the double), one integer atomic per wave and chunk, so
 * the order of a list depends on the schedule and nothing after it does: an MSD radix select, 8 passes of 8 bits, for all
 * targets (set, rank) at once -- per pass one launch that counts, per target, the digits of the keys that carry the target's
 * prefix (LDS bins, integer atomics into global bins; the first pass also counts key <= bits(tol)) and one launch of a
 * workgroup per target that picks the digit holding the rank and clears the bins.  The ranks come from out[0], out[1] and q
 * on the device.  21 launches and two memsets whatever nq, nt and the data are; no host read, no workgroup waits for another,
 * integer atomics only; the passes read the lists, never the volume; two calls on the same inputs give the same bytes in
 * every word whatever the workspace held.  nq = nt = 0 gives aide_surface3d_scores's result.  AIDE_ERR_ARG before any launch
 * for everything aide_surface3d_scores rejects, nq or nt outside 0 .. 4, a null array with a non-zero count, a q outside
 * [0, 100] or not finite, a tol that is negative or not finite. */
int aide_surface3d_scores_select(const void* p, int p_u8, int64_t p_s0, int64_t p_s1, int64_t p_s2,
                                 const void* t, int t_u8, int64_t t_s0, int64_t t_s1, int64_t t_s2,
                                 int64_t d0, int64_t d1, int64_t d2, double sp0, double sp1, double sp2,
                                 int cls, const double* q, int nq, const double* tol, int nt,
                                 void* out, double* dist, void* ws, aide_stream_t stream);

/* ---- the Euclidean distance transform of one volume, and ball morphology in millimetres.  v as in aide_fill_holes3d (int64,
 * v_u8 = 0, or uint8, v_u8 = 1; logical shape (d0, d1, d2), element strides); spacing = HOST array of the three edge lengths
 * of a voxel along the logical dims, read before the call returns.  Squared length of an integer offset o, in fp64 and in
 * exactly this association (the order in which the passes along d2, d1, d0 accumulate):
 *     q(o) = (sp0 * o0)^2 + ((sp1 * o1)^2 + (sp2 * o2)^2)
 * (sp_k * d_k)^2 must stay finite. */
/* workspace of aide_edt3d (16-byte aligned): f [n] fp64 | g [n] int32 | candidate map [n] bytes; 0 for nvox >= 2^31 */
size_t aide_edt3d_ws_bytes(int64_t nvox);
/* Foreground: v != 0 (cls < 0) or v == cls.  dist[d0][d1][d2] (fp64, contiguous) = 0 on the background and
 * sqrt(min over background u of q(v - u)) on the foreground (scipy.ndimage.distance_transform_edt(fg, sampling=spacing));
 * +inf everywhere when the volume has no background voxel.  Four launches: the background map in raster order, the scan
 * along d2 and the min-plus walk along d1 of aide_surface3d_scores, the walk along d0 with the square root at every voxel.
 * No atomic, no workgroup waits for another, every workspace word that is read was written by the same call.  AIDE_ERR_ARG
 * before any launch for d0 * d1 * d2 >= 2^31, a null spacing, a spacing that is not positive and finite, v_u8 outside {0, 1},
 * and on a volume that is not empty a null v / dist / ws, a ws off 16 bytes, a dist or an int64 v off 8 bytes; an empty volume
 * launches nothing. */
int aide_edt3d(const void* v, int v_u8, int64_t d0, int64_t d1, int64_t d2, int64_t s0, int64_t s1, int64_t s2, int cls,
               const double* spacing /* host [3] */, double* dist, void* ws, aide_stream_t stream);
/* workspace of aide_morph3d (16-byte aligned): f [n] fp64 | g [n] int32 | class map [n] bytes | the plane between the two
 * primitives of an opening or closing [n] bytes; 0 for nvox >= 2^31 */
size_t aide_morph3d_ws_bytes(int64_t nvox);
/* Ball B(r) = {o : q(o) <= radius * radius}.  op: 0 erosion with the outside of the volume as background, 1 erosion with the
 * outside as foreground, 2 dilation, 3 opening = dilate(erode0), 4 closing = erode1(dilate) (extensive).
 * num_classes = 0: X = (v != 0), out[d0][d1][d2] (uint8, contiguous) = 0 / 1.  num_classes = C in 2 .. 8: every plane
 * X_c = (v == c), c in 1 .. C - 1, is transformed on its own; erosion / opening: out = c where plane c survives, else 0;
 * dilation / closing: a voxel with v in 1 .. C - 1 keeps v, any other voxel becomes c when exactly one class claims it and 0
 * when none or several do.  A value outside 0 .. C - 1 belongs to no class.
 * Along axis k only the W_k = floor(radius / sp_k) nearest candidates on either side are evaluated.  Launches: one that reads
 * the strided volume into the class map, then per class 1 .. C - 1 (once for num_classes = 0) three (scan along d2, min-plus
 * along d1, min-plus along d0 with the compare) for op 0 - 2 and six for op 3 - 4; one memset (op 0, 1, 3).  One thread per
 * voxel in every launch, no atomic, no workgroup waits for another, no host read, every workspace word that is read was
 * written by the same call: two calls give the same bytes.  AIDE_ERR_ARG before any launch for num_classes outside
 * {0, 2 .. 8}, an unknown op, a radius that is negative or not finite, and everything aide_edt3d rejects (out for dist, no
 * alignment asked of out); an empty volume launches nothing. */
int aide_morph3d(const void* v, int v_u8, int64_t d0, int64_t d1, int64_t d2, int64_t s0, int64_t s1, int64_t s2,
                 int num_classes, int op, double radius, const double* spacing /* host [3] */, unsigned char* out, void* ws,
                 aide_stream_t stream);

/* ---- resampling: a volume of logical shape (d0, d1, d2) onto the grid (e0, e1, e2) over the same physical extent (the
 * definition: aide_amd/resample.py).  Per axis with n_in, n_out and output index o, in exact integers:
 *     num = max((2 o + 1) n_in - n_out, 0)   den = 2 n_out   lo = min(num / den, n_in - 1)   hi = min(lo + 1, n_in - 1)
 *     w1 = fp64(num - lo den) / fp64(den)  (one division)    w0 = 1 - w1
 * order 1: the eight corners in the order (a, b, c) = 000, 001, .. 111 (axis 0 slowest) with the weight (w_a * w_b) * w_c, every
 * product and every sum rounded to fp64 on its own (no fused multiply-add), accumulators starting at +0.  order 0: the voxel
 * at min(((2 o + 1) n_in) / (2 n_out), n_in - 1) per axis.  The largest accumulator is found with a strict > from class 0 on:
 * the first index wins a tie, and a NaN never displaces an earlier class.
 * Launches: TWO per call -- the table of (lo, hi, w1) for the e0 + e1 + e2 output indices into ws, then one gather in which
 * a thread computes four consecutive elements of the output in its memory order and stores them as one word.  No atomic, no
 * workgroup waits for another, no host read; every workspace word that is read was written by the same call: two calls give
 * the same bytes.  All three return AIDE_ERR_ARG before any launch for negative dims, more than 2^31 - 1 voxels (times the
 * batch) on either side, an order outside {0, 1}, and where the output is not empty an empty input, a null ws or one off 16
 * bytes; an empty output launches nothing. */
/* workspace (16-byte aligned): (e0 + e1 + e2) entries of 16 bytes; 0 for dims the entry points reject */
size_t aide_resample3d_ws_bytes(int64_t e0, int64_t e1, int64_t e2);
/* v as in aide_morph3d (int64 or uint8 through element strides).  num_classes = C in 2 .. 8: acc[c] += w for every corner
 * whose value is c (a value outside 0 .. C - 1 belongs to no class and its weight is dropped), out = the first index of the
 * largest acc; order 0: the nearest voxel's value, 0 when it is outside 0 .. C - 1.  num_classes = 0: the same with C = 2 on
 * (v != 0).  out: uint8, DENSE, its axes in the memory order (oa0, oa1, oa2) = the logical axes from the slowest to the fastest
 * (0, 1, 2: contiguous [e0][e1][e2]); the threads follow that order, the arithmetic the logical axes, so the values do not
 * depend on it.  AIDE_ERR_ARG also for v_u8 outside {0, 1}, num_classes outside {0, 2 .. 8}, (oa0, oa1, oa2) not a
 * permutation of (0, 1, 2), and on an output that is not empty a null v / out, an out off 4 bytes, an int64 v off 8 bytes. */
int aide_resample3d_labels(const void* v, int v_u8, int64_t d0, int64_t d1, int64_t d2, int64_t s0, int64_t s1, int64_t s2,
                           int64_t e0, int64_t e1, int64_t e2, int num_classes, int order, int oa0, int oa1, int oa2,
                           unsigned char* out, void* ws, aide_stream_t stream);
/* x: `batch` fp32 volumes xb elements apart, each read through the element strides (s0, s1, s2); out [batch][e0][e1][e2]
 * fp32, contiguous.  order 1: out = fp32(sum over the corners of w * fp64(x)), rounded once; order 0: the nearest voxel's
 * bits.  NaN and inf propagate as the arithmetic says (a corner of weight 0 is still multiplied).  AIDE_ERR_ARG also for a
 * negative batch and on an output that is not empty a null x / out, an x off 4 bytes, an out off 16 bytes. */
int aide_resample3d_image(const float* x, int64_t batch, int64_t xb, int64_t d0, int64_t d1, int64_t d2, int64_t s0, int64_t s1,
                          int64_t s2, int64_t e0, int64_t e1, int64_t e2, int order, float* out, void* ws, aide_stream_t stream);
/* p: fp32 probabilities of num_classes = C (2 .. 8) classes cs elements apart, each class a volume (d0, d1, d2) read through
 * (s0, s1, s2): [S][C][H][W] is passed as it lies, with cs = H W and (s0, s1, s2) = (C H W, W, 1).  Order 1 only:
 * acc[c] = sum over the corners of w * fp64(p[c]); labels [e0][e1][e2] int64 = the first index of the largest acc;
 * probs_out (or null) [e0][C][e1][e2] fp32 = fp32(acc).  AIDE_ERR_ARG also for num_classes outside 2 .. 8, C e0 e1 e2 >= 2^31,
 * and on an output that is not empty a null p / labels, a p off 4 bytes, labels or probs_out off 16 bytes. */
int aide_resample3d_probs(const float* p, int num_classes, int64_t cs, int64_t d0, int64_t d1, int64_t d2, int64_t s0, int64_t s1,
                          int64_t s2, int64_t e0, int64_t e1, int64_t e2, int64_t* labels, float* probs_out, void* ws,
                          aide_stream_t stream);

/* ---- the same for all cases of an epoch at once: K ragged cases concatenated as [S_total][H][W] (contiguous; what the
 * label map yields when fed all slices) with a DEVICE table slice_start[K + 1] (int64, non-decreasing, slice_start[0] >= 0,
 * slice_start[K] <= S_total; an entry outside that is clamped so that no access leaves the buffers).  Case k's logical
 * volume is the reference's [H][W][S_k] (np.stack(..., axis=-1)), raster order (h, w, s).  K <= 65535,
 * S_total * H * W < 2^31 (AIDE_ERR_ARG otherwise).  The number of launches does not depend on K. */
/* workspace of aide_keep_largest_cc3d_batched (16-byte aligned); 0 when the arguments are out of range */
size_t aide_lcc3d_batched_ws_bytes(int64_t nvox_total, int64_t K);
/* out[S_total][H][W] (uint8) = per case what aide_keep_largest_cc3d gives for that case alone: components never cross a
 * case boundary, one selection key per case, same tie rule within the case's raster order, all zeros for a case without
 * a positive value.  Slices that belong to no case are not written.  Five launches. */
int aide_keep_largest_cc3d_batched(const long long* v, const long long* slice_start, int64_t K, int64_t S_total, int64_t H,
                                   int64_t W, unsigned char* out, void* ws, aide_stream_t stream);
/* workspace of aide_keep_largest_cc3d_classes_batched (16-byte aligned); 0 when the arguments are out of range */
size_t aide_lcc3d_classes_batched_ws_bytes(int64_t nvox_total, int64_t K, int num_classes);
/* out[S_total][H][W] (uint8) = per case what aide_keep_largest_cc3d_classes gives for that case alone: one selection key per
 * (case, class), the tie rule within the case's raster order.  stats: NULL, or [K][C][3] int64, per case the rows of the
 * single-volume form (all zeros for an empty case).  Slices that belong to no case are not written.  Five launches and one
 * memset, whatever K and C are.  AIDE_ERR_ARG as for the two forms it combines. */
int aide_keep_largest_cc3d_classes_batched(const long long* v, const long long* slice_start, int64_t K,
                                           int64_t S_total, int64_t H, int64_t W, int num_classes,
                                           unsigned char* out, long long* stats /* NULL or [K][C][3] */,
                                           void* ws, aide_stream_t stream);
/* out[K][4] (int64) = {N, sum p*t, sum p, sum t} per case with t = (target byte == match): p is the uint8 prediction, target
 * a plane of the pseudo-label bank (match 63: the CHAOS liver plane mask[1] of the loader's palette one-hot).  One launch. */
int aide_case_confusion_batched(const unsigned char* p, const unsigned char* target, const long long* slice_start, int64_t K,
                                int64_t S_total, int64_t H, int64_t W, int match, long long* out, aide_stream_t stream);

/* ---- pseudo-label bank: the label self-correction of trainchaos_proposed_30cases1labeled.py:528-575 without its PNG round
 * trip.  The bank is [S_total][H][W] uint8 per network (the bytes of the `<mask>_netN.png` files the reference's loader
 * reads, datasetchaos_proposed/dataset.py:37-56). */
/* sums = aide_case_confusion_batched's out.  dice[k] = float32(2 * sums[k][1] / (sums[k][2] + sums[k][3])), the division in
 * fp64 and rounded once (a numpy float64 stored into a float32 tensor, :488; 0 / 0 -> NaN).  rank[k] = position of case k in
 * ascending order of dice, NaN greatest (torch's sort), equal values by the lower case index (this library's rule: the
 * reference's sort is not stable).  selected[k] = rank[k] < n_select && !labelled[k] (labelled may be NULL).  K <= 4096.
 * Two launches: the score, then the ranking that all three *_refresh_select* entry points share. */
int aide_label_refresh_select(const long long* sums, const unsigned char* labelled, int64_t K, int64_t n_select, float* dice,
                              int* rank, unsigned char* selected, aide_stream_t stream);
/* bank_plane[slices of k] = pred * scale (uint8; :548-551 with scale 63) for every case with selected[k] != 0, read on the
 * device.  One launch, a 1-D grid over (case, chunk): the rewrite kernel of all three *_bank_update* entry points. */
int aide_label_bank_update(const unsigned char* pred, const unsigned char* selected, const long long* slice_start, int64_t K,
                           int64_t S_total, int64_t H, int64_t W, int scale, unsigned char* bank_plane, aide_stream_t stream);
/* out[N][npal][H][W] (int64) = one_hot_mask of bank_plane[slice_idx[n]] over the palette (npal = 1 .. 8 device ints): the
 * loader's mask1 / mask2 (dataset.py:95-105).  A slice index outside [0, S_total) gives zeros.  N <= 65535.  One launch. */
int aide_label_bank_targets(const unsigned char* bank_plane, int64_t S_total, int64_t H, int64_t W, const long long* slice_idx,
                            int64_t N, const int* palette, int npal, long long* out, aide_stream_t stream);

/* ---- the same for multi-organ banks: C = 2 .. 8 classes, class c <-> bank byte palette[c] (C distinct device ints in
 * 0 .. 255; CHAOS: 0, 63, 126, 189, 252).  The reference refreshes the liver only; the rule below is this library's. */
/* out[K][C][3] (int64) = per case and class (#(pred == c && bank == palette[c]), #(pred == c), #(bank == palette[c])) over the
 * case's slices.  A predicted value >= C and a bank byte outside the palette belong to no class.  Integer atomics only: the
 * same bytes from call to call.  Limits as aide_case_confusion_batched.  One memset and one launch for any K and C. */
int aide_case_class_counts_batched(const unsigned char* pred, const unsigned char* bank_plane, const long long* slice_start,
                                   int64_t K, int64_t S_total, int64_t H, int64_t W, const int* palette, int C, long long* out,
                                   aide_stream_t stream);
/* counts = aide_case_class_counts_batched's out.  class_dice[k][c] = float32(2 I / (P + T)) for every c, the division in fp64
 * (0 / 0 -> NaN).  dice[k] = float32 of the fp64 mean of those fp64 quotients over the foreground classes c = 1 .. C - 1 with
 * P + T > 0, summed in ascending c and divided by their number; NaN when there is none.  An organ absent from prediction and
 * pseudo-label alike is left out, one present in only one of them scores 0.  With C = 2 the bits of aide_label_refresh_select.
 * rank, selected, labelled, the K <= 4096 limit and the two launches are that function's. */
int aide_label_refresh_select_classes(const long long* counts, const unsigned char* labelled, int64_t K, int C, int64_t n_select,
                                      float* class_dice, float* dice, int* rank, unsigned char* selected, aide_stream_t stream);
/* bank_plane[slices of k] = palette[pred] for every case with selected[k] != 0, read on the device; a predicted value >= C
 * writes palette[0].  Other cases are not touched.  One launch. */
int aide_label_bank_update_classes(const unsigned char* pred, const unsigned char* selected, const long long* slice_start,
                                   int64_t K, int64_t S_total, int64_t H, int64_t W, const int* palette, int C,
                                   unsigned char* bank_plane, aide_stream_t stream);
/* out[N][H][W] (int64) = the class index of every byte of bank_plane[slice_idx[n]]: the index targets the fused losses take.
 * A byte outside the palette gives ignore_index, a slice index outside [0, S_total) a plane of it.  N <= 65535.  One launch. */
int aide_label_bank_targets_index(const unsigned char* bank_plane, int64_t S_total, int64_t H, int64_t W,
                                  const long long* slice_idx, int64_t N, const int* palette, int C, int64_t ignore_index,
                                  long long* out, aide_stream_t stream);

/* ---- per-image pseudo-label bank: the label self-correction of trainkidney_proposed_mask{1,2,3}.py:373-434 and
 * trainbreast_dataset3_proposed_272cases25labeled.py:373-438.  Every training IMAGE k of K <= 2^20 is scored with Dice2d
 * (:131-141) and the worst int(update_percent * K) are rewritten.  Planes are [K][H][W] uint8, H * W < 2^31. */
/* Fused epilogue of a forward batch: logits [N][2][H*W] fp32 (image stride l_bs floats) of the images k0 .. k0 + N - 1.
 * pred[k0 + n] = the labels of aide_label_map on the same logits (bit-identical, equal logits and NaN included) as uint8;
 * sums[k0 + n] = (H*W, sum p*t, sum p, sum t) int64 with t = (score_rows[n] byte > 0) & gate[k0 + n] (gate: K bytes, or NULL
 * for 1).  score_rows: the N rows of the plane the network is scored against, [N][H*W].  Exact integers, whatever the order
 * of the workgroups.  16-byte loads when H*W % 16 == 0 and all rows are 16-byte aligned, else a scalar path.
 * One memset node and one launch. */
int aide_image_eval_logits(const float* logits, int64_t l_bs, const unsigned char* score_rows, const unsigned char* gate,
                           int64_t N, int64_t H, int64_t W, int64_t k0, int64_t K, unsigned char* pred, long long* sums,
                           aide_stream_t stream);
/* ... from ready label maps [N][H*W] (uint8 if is_u8, else int64) instead of logits: p = (label != 0). */
int aide_image_eval_labels(const void* labels, int is_u8, const unsigned char* score_rows, const unsigned char* gate, int64_t N,
                           int64_t H, int64_t W, int64_t k0, int64_t K, unsigned char* pred, long long* sums,
                           aide_stream_t stream);
/* dice[k] = 0 if sums[k][2] + sums[k][3] == 0, else float32(2 * sums[k][1] / (sums[k][2] + sums[k][3])) with the division in
 * fp64 (Dice2d stored into a float32 tensor, :392).  rank[k] = position of image k in ascending order of dice, equal values
 * by the lower image index (this library's rule: the reference's sort is not stable; NaN, which Dice2d cannot give, would
 * rank greatest).  written[k] = rank[k] < n_select && sums[k][2] > 0 && !labelled[k] (labelled may be NULL): the `if
 * save_data.sum() > 0` of :418.  Two launches for any K, the ranking being aide_label_refresh_select's. */
int aide_image_refresh_select(const long long* sums, const unsigned char* labelled, int64_t K, int64_t n_select, float* dice,
                              int* rank, unsigned char* written, aide_stream_t stream);
/* plane[k] = pred[k] * scale (uint8; 255 for the breast PNGs, 1 for the kidney volumes) for every image with written[k] != 0,
 * read on the device.  One launch, a 1-D grid over (image, chunk). */
int aide_image_bank_update(const unsigned char* pred, const unsigned char* written, int64_t K, int64_t H, int64_t W, int scale,
                           unsigned char* plane, aide_stream_t stream);
/* out[N][H][W] (int64) = (plane[image_idx[n]] > 0) & gate[image_idx[n]] (gate may be NULL): the loaders' mask1 / mask2 after
 * ToTensor.  An index outside [0, K) gives zeros.  One launch. */
int aide_image_bank_targets(const unsigned char* plane, int64_t K, int64_t H, int64_t W, const long long* image_idx, int64_t N,
                            const unsigned char* gate, long long* out, aide_stream_t stream);

/* ---- multi-class metrics (csrc/metrics_mc.hip): MulticlassDice_fn / MulticlassIoU_fn / MulticlassTP_TN_FP_FN /
 * MulticlassAccuracy_fn of utils/metrics2d.py:86-196, which copy the logits to the host on every call (:87-91) and count with
 * numpy.  Every one of them is a function of three integers per image and class: (sum i*t, sum i, sum t), i = one-hot of the
 * prediction, t = one-hot of the target.  C = 2 .. 8; integer sums, the same bits from run to run. */
/* counts[N][C][3] (int64) from logits [N][C][HW] fp32 (image stride l_bs floats, channels HW apart; N <= 65535, C * HW < 2^31).
 * Prediction = torch.argmax(logits, dim=1) of the RAW logits (:89): equal maxima -> the lowest class; NaN is the greatest
 * value and the first NaN wins.  (aide_label_map is argmax(softmax(.)): its rounding merges close logits, so it has other
 * ties.)  target (image stride t_bs elements), by t_kind: 0 one-hot [N][C][HW] float, 1 one-hot int64, 2 one-hot uint8 -- the
 * loaders' 0/1-valued masks: any non-zero value is read as 1, soft targets are outside the contract; 3 class index [N][HW]
 * int64 -- an index outside [0, C) belongs to no class, its pixel still counts in sum i.  counts need no zero-fill by the
 * caller.  16-byte loads along HW when HW, l_bs, t_bs are multiples of 4 and both bases are aligned, else a scalar path.
 * One memset node and one launch. */
int aide_mc_counts_logits(const float* logits, int64_t l_bs, const void* target, int t_kind, int64_t t_bs, int C, int64_t N,
                          int64_t HW, long long* counts, aide_stream_t stream);
/* counts[C][3] (int64) for two label volumes of a case, i_c = (p == c), t_c = (t == c): operands and conventions of
 * aide_case_confusion (int64 / uint8, logical dims with element strides, < 2^31 voxels); a label outside [0, C) belongs to no
 * class.  Replaces per-class loops of Dice3d_fn / IoU3d_fn / TP_TN_FP_FN3d over `generatedtarget == c`
 * (evalchaos_comparison_1cases.py:116-141).  One memset node and one launch. */
int aide_mc_counts_labels(const void* p, int p_u8, int64_t p_s0, int64_t p_s1, int64_t p_s2, const void* t, int t_u8,
                          int64_t t_s0, int64_t t_s1, int64_t t_s2, int64_t d0, int64_t d1, int64_t d2, int C,
                          long long* counts, aide_stream_t stream);
/* acc += the N images of counts[N][C][3] (HW pixels each), added in index order by one workgroup: the float64 sums are the
 * sequence the loops of metrics2d.py:124-133, 153-162 produce over the same images.  acc = 42 words of 8 bytes (8-byte
 * aligned; the caller zeroes it once per epoch):
 *   [0..7]   double  sum over images of Dice_c = 2 TP / (sum i + sum t), 1.0 when sum i + sum t == 0 (:130-131)
 *   [8..15]  double  sum over images of IoU_c = TP / (sum i + sum t - TP), 1.0 likewise (:159-160)
 *   [16..23] int64   sum TP_c      [24..31] int64 sum i_c      [32..39] int64 sum t_c
 *   [40]     int64   images        [41]     int64 pixels (N * HW)
 * classes >= C are not touched.  One fp64 division per term.  One launch. */
int aide_mc_metrics_accumulate(const long long* counts, int64_t N, int C, int64_t HW, void* acc, aide_stream_t stream);

/* ---- test-time augmentation (csrc/ensemble.hip): the eight flips and quarter turns of an image, exact permutations.
 * View code v = r + 4 f, r = 0 .. 3, f = 0 / 1: view_v(x) = torch.rot90(torch.flip(x, [-1]) if f else x, r, (-2, -1)); its
 * frame is [W][H] for odd r, which needs H == W.  views: HOST arrays of 1 .. 16 codes, duplicates allowed.  Both calls return
 * AIDE_ERR_ARG before any launch for a null pointer, a code outside 0 .. 7, an odd-r code with H != W, a count outside
 * 1 .. 16 or N * C * H * W >= 2^31; any H, W >= 1 (4-byte accesses: no alignment is asked of the pointers beyond a float's).
 * One launch each, no atomics, no workspace: the same bytes from call to call. */
/* y[V][N][C][.][.] (image stride y_bs floats, image v * N + n) with y[v][n] = view_views[v](x[n]), x[N][C][H][W] (image stride
 * x_bs); every tile of x is read once for all V views. */
int aide_view_stack(const float* x, int64_t x_bs, float* y, int64_t y_bs, const int* views /* HOST [V] */, int V,
                    int N, int C, int H, int W, aide_stream_t stream);
/* The soft vote of K members (C = 2 .. aide_seg_max_classes()): for output pixel (n, i, j) and member k = 0 .. K - 1 in order,
 * the C logits at the position views[k] maps (i, j) to, their fp32 soft-max as aide_label_map takes it for C > 2, added to a
 * per-class fp32 sum; probs (NULL, or [N][C][H][W] with image stride p_bs) = sum * (1 / K); labels[N][H][W] = the FIRST index
 * of the largest sum.  One member under view 0 gives the labels of aide_label_map. */
int aide_ensemble_vote(const float* const* logits /* HOST array of K device pointers, each [N][C][H][W] in its member's view frame */,
                       const int* views /* HOST [K] */, int K, int64_t l_bs, int N, int C, int H, int W,
                       long long* labels /* [N][H][W] */, float* probs /* NULL or [N][C][H][W] */, int64_t p_bs,
                       aide_stream_t stream);

/* ---- sliding-window inference (csrc/window.hip): overlapping windows of an image and the weighted blend of their soft-max
 * maps, for images that are not the training size.  Along an axis of length `size` the windows of length `win` start at the
 * HOST array starts[count], 1 <= count <= 32: starts[0] = 0, strictly increasing, every start in [0, max(0, size - win)], no
 * two neighbours more than `win` apart and, when size > win, the last start = size - win -- so every pixel is covered
 * (aide_amd/window.py `window_grid` makes such tables).  Window b = a_y * nx + a_x, B = ny * nx.  Both calls return
 * AIDE_ERR_ARG before any launch for a null pointer, a table that breaks one of these rules, a non-positive extent, or 2^31
 * or more elements in an operand (N * C * H * W, B * N * C * wh * ww).  One launch each, no atomics, no workspace: the same
 * bytes from call to call. */
/* y[B][N][C][wh][ww] (image stride y_bs floats, image b * N + n): y[b][n][c][u][v] = x[n][c][min(sy_b + u, H - 1)][min(sx_b + v,
 * W - 1)], x[N][C][H][W] (image stride x_bs); any C >= 1.  Replaces B slices `x[:, :, sy:sy + wh, sx:sx + ww]` and their
 * torch.stack (plus F.pad(mode='replicate') where the image is smaller than the window). */
int aide_window_stack(const float* x, int64_t x_bs, float* y, int64_t y_bs, int N, int C, int H, int W, int wh, int ww,
                      const int* starts_y /* HOST [ny] */, int ny, const int* starts_x /* HOST [nx] */, int nx,
                      aide_stream_t stream);
/* The weighted blend (C = 2 .. aide_seg_max_classes()): for output pixel (n, i, j) and the windows b that contain it, in
 * increasing b, with (u, v) = (i - sy_b, j - sx_b): p = the C values of src[b][n][.][u][v] (src_is_logits = 0) or their fp32
 * soft-max as aide_ensemble_vote takes it (src_is_logits != 0); w = g_h[u] * g_w[v]; acc_c = acc_c + w * p_c; den = den + w,
 * every product and sum rounded to fp32 on its own.  labels[N][H][W] = the FIRST index of the largest acc_c; probs (NULL, or
 * [N][C][H][W] with image stride p_bs) = acc_c / den.  Window pixels beyond the image are never read.  Replaces per window
 * F.softmax, a weighted `index_add_` / slice accumulation into [N][C][H][W], the division and torch.argmax. */
int aide_window_blend(const float* src /* [B][N][C][wh][ww], image stride src_bs */, int src_is_logits, int64_t src_bs,
                      int N, int C, int H, int W, int wh, int ww, const int* starts_y /* HOST [ny] */, int ny,
                      const int* starts_x /* HOST [nx] */, int nx, const float* g_h /* DEVICE [wh] */,
                      const float* g_w /* DEVICE [ww] */, long long* labels /* [N][H][W] */,
                      float* probs /* NULL or [N][C][H][W] */, int64_t p_bs, aide_stream_t stream);

/* ---- loader transforms of the proposed loaders: Resize(BILINEAR) -> RandomRotate(BILINEAR) -> RandomHorizontallyFlip
 * -> ToTensor -> Normalize (datasetchaos_proposed/transform.py; the single-modal copies of datasetkidney_proposed/ etc.), and
 * Resize(NEAREST) + one_hot_mask of the masks (datasetchaos_proposed/dataset.py).  Bit-exact with PIL where PIL is integer.
 * The tables come from aide_amd/utils/loader_aug.py: src = packed u8 / u16 planes; desc[p] = 8 ints {byte offset, h, w,
 * u16, x table, y table, kx, ky} (table offsets in ints into tab; an entry per output index {first tap, taps, kx / ky 22-bit
 * weights}) for the N * M source planes p = n * M + m; par[n][k] = {PIL inverse affine a..f, hflip, mode} of augmentation k
 * (mode 1 / 2 / 3 / 4: the 0 / 180 / 90 / 270 degree transpose paths); norm = {mean[3], std[3]} or NULL (per-image mean and
 * unbiased std of the resized base).  out[m][v][n]: v = 0 the base image, v = k the view of augmentation k, each [3][S][S]
 * float32, or [S][S] u8 with out_u8 (16-byte aligned when float).  ws: aide_loader_aug_ws_bytes(N * M, S), 16-byte aligned.
 * Two launches; augno 0 .. 4. */
size_t aide_loader_aug_ws_bytes(int nplanes, int S);
int aide_loader_aug(const void* src, const int* desc, const int* tab, const double* par, const float* norm, int N, int M,
                    int S, int augno, int out_u8, void* out, void* ws, aide_stream_t stream);
/* out[q] = [npal][S][S] int64 one-hot of mask plane q (u8) resized NEAREST; desc[q] = 8 ints {byte offset, h, w, 0, x index
 * table, y index table, 0, 0}; a value outside the palette (1 .. 8 entries, device ints) gives an all-zero row.  One launch. */
int aide_loader_mask_onehot(const void* src, const int* desc, const int* tab, const int* palette, int nplanes, int S,
                            int npal, long long* out, aide_stream_t stream);

/* ---- Adam(amsgrad), one launch for all parameter tensors ----------------------------------------
 * replaces torch.optim.Adam(net.parameters(), lr, amsgrad=True): trainchaos_comparison_1case.py:170 */
int aide_adam_amsgrad_multi(float* const* p, const float* const* g, float* const* m, float* const* v,
                            float* const* vmax, const int64_t* sizes, const int64_t* block_start,
                            int ntensors, int64_t total_blocks, float lr, float beta1, float beta2,
                            float eps, float weight_decay, int amsgrad, int64_t step,
                            aide_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* AIDE_HIP_H */
