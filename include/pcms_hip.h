/*
 * pcms_hip.h — C ABI of libpcms_hip.so, the MI355X (gfx950) kernels behind the drop-in
 * UNet3D / DiceLoss / BCEDiceLoss / Trainer.step of
 * qwertyhgb/Prostate-Cancer-Multimodal-Segmentation.
 *
 * The reference has no FFI: its hot path is PyTorch aten called from Python.  Each entry
 * point below replaces the aten op(s) named in its comment (paths relative to the
 * reference repo root).  The Python host layer (pcms_amd) binds these through ctypes.
 *
 * Conventions
 *   - dtype: 0 = fp32 storage (parity build), 1 = bf16 storage (performance build).
 *     Accumulation is always fp32; statistics are combined in fp64.
 *   - Activations are NDHWC, contiguous, channel pitch = channel count.
 *   - Pointers are device pointers; the caller owns every buffer (no allocation inside,
 *     except workspace passed in).  `s` is a hipStream_t; every call is stream-ordered and
 *     returns 0 on success, a hipError_t code, or a negative code for a bad argument.
 */
#ifndef PCMS_HIP_H
#define PCMS_HIP_H
#include <hip/hip_runtime.h>

#ifdef __cplusplus
extern "C" {
#endif

/* conv epilogue flags (pcms_conv3_fwd, pcms_split_epilogue, pcms_stem_fwd): ACCUMULATE
 * adds into y; RELU stores relu(conv + bias) -- eval mode with the BatchNorm folded into the
 * weights and bias (pcms_bn_fold), no statistics                                          */
#define PCMS_CONV_ACCUMULATE 1
#define PCMS_CONV_RELU 2
/* gradient writer flags (pcms_conv3_wgrad): STORE writes dw instead of adding into it -- the
 * first writer after zero_grad(set_to_none=True), so the gradient needs no zero fill       */
#define PCMS_GRAD_STORE 1
/* pcms_stem_fwd flag: the K-dense kernel (9 tap rows x 16 instead of 14 tap pairs x 16; the
 * pack's second form, valid for weights with cin_w <= 5)                                   */
#define PCMS_STEM_DENSE 16

/* ---- layout ---------------------------------------------------------------------- */
/* batch['image'] (N, Cin, D, H, W) fp32 NCDHW -> NDHWC, channels zero-padded to Cp.
 * Replaces the implicit layout of images.to(device) (utils/trainer.py:179).          */
int pcms_pack_input(int dtype, const float* in, void* out, int N, int Cin, long V, int Cp, hipStream_t s);

/* ---- Conv3d(k=3, padding=1): models/unet3d.py:29,35 ------------------------------- */
/* The conv3 entry points also take dtype 2 (PCMS_F32X3): fp32 data, bf16x3 arithmetic
 * (hi*hi + lo*hi + hi*lo, ~10x fp32 rounding error); dtype 0 there computes with bf16x6
 * (three bf16 parts per operand, fp32-grade: the parity build).                        */
int pcms_conv3_chunk(int dtype);                  /* input channels per K-chunk        */
/* elements (activation dtype) of one weight pack, J rows x Kdim input channels          */
int pcms_conv3_pack_elems(int dtype, int J, int Kdim);
int pcms_conv3_mblocks(int N, int D, int H, int W);/* general-kernel M blocks (an upper
                                                      bound on the BN partial rows)      */
/* BN partial rows an unsplit pcms_conv3_fwd over sources (c0, c1) writes: the persistent
 * big-box bf16 kernel (8x8x16 boxes, 16-channel chunks, >= pcms_conv3_big_min_boxes boxes)
 * writes one row per box slot (min(boxes, workgroups / (Cout / 64))), the general kernel
 * pcms_conv3_mblocks rows                                                               */
int pcms_conv3_fwd_rows(int dtype, int N, int D, int H, int W, int c0, int c1, int Cout);
int pcms_conv3_big_min_boxes(int v);               /* set (v > 0) / query; returns old */
int pcms_conv3_big_max_wgs(int v);                 /* persistent grid cap: set (v >= 0,
                                                      0 = one per CU) / query; old      */
/* general-kernel boxes of <= 256 voxels (level 4) on four waves of 2 M-tiles (1, default)
 * or two waves of 4 (0); v < 0 queries; returns the previous setting                   */
int pcms_conv3_small_box_mtw2(int v);
/* A/B switch: general forward / dgrad box volume, 512 or 256 voxels (v <= 0 queries) */
int pcms_conv3_fwd_box_vol(int v);
/* master W [Cout][Cin][3][3][3] fp32 -> kernel pack; flip=1 builds the dgrad pack      */
int pcms_conv3_pack(int dtype, const float* w, void* out, int Cout, int Cin, int flip, hipStream_t s);
// Both packs of one conv (forward and dgrad, as pcms_conv3_pack flip 0 / 1) from one read of w.
int pcms_conv3_pack2(int dtype, const float* w, void* fwd, void* dgrad, int Cout, int Cin, hipStream_t s);
/* Y = conv(X) + bias, X = channel-concat(x0[:, :c0], x1[:, :c1]) (Up3D cat, :156),
 * output channels [0, cy0) -> y0, [cy0, Cout) -> y1 (dgrad concat split).
 * stats: BN partials or NULL: [mblocks][Cout][2] fp32 (sum, M2 = sum of squared
 * deviations from the row's own mean) followed by [mblocks] fp32 row voxel counts
 * (numerically stable moments; consumed by pcms_bn_finalize).  splits > 1 (split-K over
 * input channels): every split stores its fp32 partial sums into its own slab of
 * yacc [pcms_conv3_splits(...)][Nvox][Cout] (plain stores, no zeroing, no atomics);
 * finish with pcms_split_epilogue, which adds the slabs in split order (deterministic).
 * Also used for dgrad with the flip pack.                                              */
int pcms_conv3_splits(int dtype, int Cin, int splits);  /* slabs a split-K launch uses   */
int pcms_conv3_fwd(int dtype, const void* x0, int c0, const void* x1, int c1,
                   const void* wpack, const float* bias, void* y0, void* y1, int cy0,
                   float* yacc, float* stats, int flags,
                   int N, int D, int H, int W, int Cout, int splits, hipStream_t s);
/* The conv of relu(x * isc + ish) (per input channel): the BatchNorm + ReLU of the layer
 * below (models/unet3d.py:31-35, bn -> relu -> conv) applied to the staged halo in LDS
 * instead of a separate HBM pass.  bf16, one source of <= 128 channels, the big-box shapes
 * (-5 otherwise); no split, no flags.  Measured against pcms_bn_relu + pcms_conv3_fwd in
 * DESIGN.md §0b (tests/tools/bnin_ab.py).                                                 */
int pcms_conv3_fwd_bnin(int dtype, const void* x, int cin, const float* isc, const float* ish, const void* wpack,
                        const float* bias, void* y, float* stats, int N, int D, int H, int W, int Cout,
                        hipStream_t s);
/* The weight gradient of that conv: x is the pre-BatchNorm input, relu(x * isc + ish) is
 * applied to the staged halo in LDS (bf16, one source, the LDS-DMA shapes; -5 otherwise).
 * pcms_conv3_bnin_ok: 1 when both pcms_conv3_fwd_bnin and this run the layer.              */
int pcms_conv3_wgrad_bnin(int dtype, const void* x, int cin, const float* isc, const float* ish, const void* dy,
                          float* dw, float* dwt, int N, int D, int H, int W, int Cout, int cin_w, int target_wgs,
                          int flags, hipStream_t s);
int pcms_conv3_bnin_ok(int N, int D, int H, int W, int cin, int Cout, int target_wgs);
/* dw [Cout][cin_w][27] fp32 += sum_v dy[v, co] * x[v + tap, ci] (ci < cin_w <= c0 + c1;
 * flags PCMS_GRAD_STORE: dw = ...);
 * dwt: pcms_conv3_wgrad_ws_floats(...) fp32 workspace (one partial row per voxel split,
 * summed in a fixed order: deterministic)                                               */
int pcms_conv3_wgrad_ws_floats(int dtype, int N, int D, int H, int W, int c0, int c1, int Cout, int target_wgs);
/* bf16 grids of at most v boxes split the taps over two workgroups (no partial rows) before
 * splitting the voxels; 0 never, v < 0 queries; returns the previous value              */
int pcms_conv3_wgrad_tg_maxbox(int v);
/* compile-time-box bf16 weight gradients (the LDS-DMA kernels of levels 0-4) on
 * v_mfma_f32_16x16x32_bf16 (1) or v_mfma_f32_32x32x16_bf16 (0, default); v < 0 queries;
 * returns the previous setting (A/B switch) */
int pcms_conv3_wgrad_k16(int v);
/* fp32 (bf16x6) weight gradient: boxes streamed by LDS-DMA into an fp32 staging buffer beside
 * the previous box's MFMAs (1) or staged synchronously through registers (0, default: measured
 * as fast); v < 0 queries; returns the previous setting (A/B switch) */
int pcms_conv3_wgrad_x6_dma(int v);
/* the weight gradient's per-split partial rows summed in one launch (1, default) or by the
 * group-sum + reduce pair (0); the sums are bit-identical; v < 0 queries; returns the previous
 * setting (A/B switch) */
int pcms_conv3_wgrad_reduce_fused(int v);
int pcms_conv3_wgrad(int dtype, const void* x0, int c0, const void* x1, int c1, const void* dy,
                     float* dw, float* dwt, int N, int D, int H, int W, int Cout, int cin_w,
                     int target_wgs, int flags, hipStream_t s);
/* The big-box convs on v_mfma_f32_16x16x32_bf16 (round 5): K = a pair of taps x 16 channels,
 * 8 M-tiles x 4 N-tiles per wave, one wave per box d-plane; boxes of 8 d-planes (levels 0-1,
 * the shapes of the 32x32x16 big-box path of pcms_conv3_fwd) or, where those leave CUs idle
 * and 4-deep boxes x 64-channel blocks fill them (level 2), of 4.  BN partial rows:
 * pcms_conv3_fwd16_rows (0: not a fwd16 shape).  Weights in the
 * pack16 layout: pcms_conv3_pack16 writes both directions of the convs of a table (int64 rows
 * {fp32 weight ptr, Cout, Cin, fwd16 ptr or 0, dgrad16 ptr or 0, first tile, 0, 0}, one tile
 * per 32 x 32 channels; fwd16 = rows Cout, k Cin; dgrad16 = rows Cin, k Cout, taps mirrored).
 * pcms_conv3_fwd16 takes isc / ish (the input's BatchNorm + ReLU, as pcms_conv3_fwd_bnin) or
 * NULL; flags 0 or PCMS_CONV_RELU; -5 where pcms_conv3_big16_ok is 0.                      */
int pcms_conv3_big16_ok(int N, int D, int H, int W, int c0, int c1, int Cout);
int pcms_conv3_fwd16_rows(int N, int D, int H, int W, int c0, int c1, int Cout);
/* 128-channel blocks (4-deep boxes, 8 N-tiles per wave: one staged halo feeds 128 output
 * channels) where Cout % 128 == 0 and they fill the CUs: 1 or 0 (default); v < 0 queries;
 * returns the previous setting (set before any workspace query)                          */
int pcms_conv3_b16_nt8(int v);
/* Level 3 (rows of 8 w): the same kernel on 4 d x 16 h x 8 w boxes, split over K into fp32
 * partial rows yacc[split][vox][Cout] (no bias / statistics; pcms_split_epilogue sums them in
 * split order).  _split_ok: the split count it uses for this conv, 0 where it does not apply. */
int pcms_conv3_fwd16_split_ok(int N, int D, int H, int W, int c0, int c1, int Cout);
int pcms_conv3_fwd16_split(const void* x0, int c0, const void* x1, int c1, const void* wpack16, float* yacc,
                           int N, int D, int H, int W, int Cout, int splits, hipStream_t s);
int pcms_conv3_pack16_elems(int J, int Kdim);
int pcms_conv3_pack16(const long long* table, int ntab, int ntiles, hipStream_t s);
int pcms_conv3_fwd16(const void* x0, int c0, const void* x1, int c1, const float* isc, const float* ish,
                     const void* wpack16, const float* bias, void* y0, void* y1, int cy0, float* stats, int flags,
                     int N, int D, int H, int W, int Cout, hipStream_t s);
/* Stem (inc.conv.0, bf16 build): input stored with 8 channels (n_modalities <= 8).
 * K packs two taps per MFMA k-step (14 x 16 = 224 instead of 27 x 32), or, with
 * PCMS_STEM_DENSE (cin_w <= 5), one (kd, kh) tap row of 3 kw x 5 channels per k-step (9 x 16);
 * pcms_stem_pack writes both forms.
 * pcms_stem_supported: bit 0 = pcms_stem_fwd runs this shape, bit 1 = pcms_stem_wgrad
 * does (other shapes: the general pcms_conv3_fwd / pcms_conv3_wgrad).                   */
int pcms_stem_supported(int N, int D, int H, int W);
int pcms_stem_pack_elems(void);
/* the stem weight gradient's MFMA columns: 0 (default) taps x 8 channels, 1 dense tap rows
 * x 16 for cin_w <= 5; v < 0 queries; returns the previous setting                        */
int pcms_stem_wgrad_dense(int v);
int pcms_stem_pack(const float* w, void* out, int cin_w, hipStream_t s);
/* y = stem conv(x) + bias; BatchNorm partial moments into stats, laid out as pcms_conv3_fwd
 * with rows = pcms_stem_fwd_rows(N, D, H, W) (one row per workgroup on the hot shapes)   */
int pcms_stem_fwd_rows(int N, int D, int H, int W);
int pcms_stem_fwd(const void* x, const void* wpack, const float* bias, void* y, float* stats,
                  int N, int D, int H, int W, int flags, hipStream_t s);
/* dw [64][cin_w][27] += stem weight gradient (streaming kernel: one partial row per
 * workgroup in ws, then a fixed-order sum), ws = pcms_stem_wgrad_ws_floats(...) floats.   */
int pcms_stem_wgrad_ws_floats(int N, int D, int H, int W, int cin_w);
int pcms_stem_wgrad(const void* x, const void* dy, float* dw, float* ws, int cin_w, int N, int D, int H,
                    int W, hipStream_t s);
/* Block fusion of the stem's BatchNorm + ReLU backward (models/unet3d.py:29-33) into its
 * weight gradient: da = gradient of the block's first ReLU output, y = the stem's pre-BN
 * output, scale / shift / mean / invstd = the forward's BN coefficients, coef = the apply
 * coefficients pcms_bn_relu_bwd(..., dy = NULL, ...) left; the stem's dy is formed in LDS
 * per box and never stored (the stem input needs no gradient).                          */
int pcms_stem_wgrad_bn(const void* x, const void* da, const void* y, const float* scale, const float* shift,
                       const float* mean, const float* invstd, const float* coef, float* dw, float* ws, int cin_w,
                       int N, int D, int H, int W, hipStream_t s);
/* The stem conv's input gradient (models/unet3d.py:29 inc.conv.0 under autograd: aten
 * convolution_backward's grad_input, which the reference forms whenever the model input
 * requires grad -- saliency, adversarial inputs, a differentiable pre-processing in front):
 *   dx[n][ci][d][h][w] = sum_{co, kd, kh, kw} dy[n][d+1-kd][h+1-kh][w+1-kw][co] W[co][ci][kd][kh][kw]
 * dy: NDHWC, 64 channels, storage type; dx: fp32 NCDHW [N][cin_w][D][H][W], every element
 * written exactly once with plain stores (no zero fill, no atomics, fp32 accumulation: two runs
 * are bit-identical).  wpack: pcms_stem_dgrad_pack of the fp32 master weight [64][cin_w][27]
 * (pcms_stem_dgrad_pack_elems(dtype) elements of the storage type).  Any N, D, H, W >= 1 with
 * dy below 2 GiB (-7 otherwise); cin_w <= 8.  bf16: v_mfma_f32_16x16x32_bf16, weights as the
 * A operand; fp32: plain fmaf.                                                            */
int pcms_stem_dgrad_pack_elems(int dtype);
int pcms_stem_dgrad_pack(int dtype, const float* w, void* out, int cin_w, hipStream_t s);
int pcms_stem_dgrad(int dtype, const void* dy, const void* wpack, float* dx, int N, int D, int H, int W, int cin_w,
                    hipStream_t s);
/* y = sum of the `splits` slabs of acc (in split order) + bias -> storage type; stats
 * layout as pcms_conv3_fwd with rows = pcms_split_epilogue_rows(nvox)                    */
int pcms_split_epilogue_rows(long nvox);
int pcms_split_epilogue(int dtype, const float* acc, int splits, const float* bias, void* y0, void* y1,
                        int cy0, float* stats, int C, long nvox, int flags, hipStream_t s);

/* ---- BatchNorm3d (train / eval) + ReLU(inplace): models/unet3d.py:31-39 ----------- */
/* part: the [rows][C][2] (sum, M2) partials + [rows] counts written by the conv / stem /
 * split-epilogue kernels; ws: pcms_bn_ws_doubles(C) fp64 workspace (two-stage fp64
 * column reduction, rows merged with Chan's parallel-variance formula)                  */
int pcms_bn_ws_doubles(int C);
int pcms_bn_finalize(const float* part, int rows, int C, double count, const float* gamma,
                     const float* beta, float* rmean, float* rvar, long long* nbt, float momentum,
                     float eps, float* scale, float* shift, float* mean, float* invstd, double* ws,
                     hipStream_t s);
/* Eval-mode BatchNorm folded into the conv before it (UNet3D.predict / .inference,
 * models/unet3d.py:298-344): wo = w * sc[co], bo = b * sc + sh (sc = gamma / sqrt(rvar +
 * eps), sh = beta - rmean * sc, in fp64); w [Cout][K] fp32 (K = Cin * 27), b may be NULL.
 * The folded conv with PCMS_CONV_RELU is conv -> BN -> ReLU in one pass.                  */
int pcms_bn_fold(const float* w, const float* b, const float* gamma, const float* beta, const float* rmean,
                 const float* rvar, float eps, int Cout, long K, float* wo, float* bo, hipStream_t s);
int pcms_bn_eval_coeffs(const float* gamma, const float* beta, const float* rmean, const float* rvar,
                        float eps, int C, float* scale, float* shift, hipStream_t s);
int pcms_bn_relu(int dtype, const void* y, void* a, const float* scale, const float* shift, int C,
                 long nvox, hipStream_t s);
/* Eval-mode BatchNorm3d + ReLU backward (models/unet3d.py:31-39 with the module in eval():
 * aten native_batch_norm_backward(train=False) + threshold_backward, as autograd runs them
 * for an input gradient): dy = da * scale[c] where y * scale[c] + shift[c] > 0 (the forward's
 * own fp32 expression, pcms_bn_relu), else 0; scale / shift from pcms_bn_eval_coeffs.  A pure
 * apply: running statistics are constants, so there is no reduction and no parameter
 * gradient.                                                                                */
int pcms_bn_relu_bwd_eval(int dtype, const void* da, const void* y, const float* scale, const float* shift,
                          void* dy, int C, long nvox, hipStream_t s);
/* A/B switch: block cap of the BN-backward reduce passes (their partial rows): 512 (default,
 * the one-launch finalize) or more (2048: the two-stage finalize); v <= 0 queries; returns the
 * previous value; set before the workspace queries */
int pcms_bn_bwd_rows_cap(int v);
/* Test switch: an extra block cap on every grid-stride launch and every row-count / workspace
 * query of the streaming kernels (BatchNorm + ReLU, pools, head, loss, Adam, clip, pack / unpack /
 * add): each uses min(its own cap, v), so a small v makes a test-sized input take the
 * many-trips-per-thread paths; default INT_MAX (no extra cap, the product); v <= 0 queries;
 * returns the previous value; set before the workspace queries */
int pcms_stream_grid_cap(int v);
int pcms_bn_bwd_rows(int dtype, int C, long nvox);
/* dy = BN+ReLU backward(da); dgamma/dbeta += ; part: rows*C*2 fp32; coef: 3*C fp32 (the
 * apply coefficients k1, k2, k3 per channel: dy = k1 g + k2 xhat + k3).  dy == NULL: no
 * apply pass (a fused consumer applies from coef: pcms_stem_wgrad_bn)                    */
int pcms_bn_relu_bwd(int dtype, const void* da, const void* y, const float* scale, const float* shift,
                     const float* mean, const float* invstd, const float* gamma, float* part, float* coef,
                     float* dgamma, float* dbeta, void* dy, int C, long nvox, double* ws, hipStream_t s);
/* the same without the reduction pass: ``part`` holds ``rows`` partial rows [rows][C][2] of
 * (sum g, sum g xhat) written by a fused producer (pcms_maxpool_bwd_bn)                  */
int pcms_bn_relu_bwd_finish(int dtype, const void* da, const void* y, const float* scale, const float* shift,
                            const float* mean, const float* invstd, const float* gamma, const float* part,
                            int rows, float* coef, float* dgamma, float* dbeta, void* dy, int C, long nvox,
                            double* ws, hipStream_t s);

/* ---- MaxPool3d(2): models/unet3d.py:80 ------------------------------------------- */
int pcms_maxpool_fwd(int dtype, const void* a, void* p, int N, int D, int H, int W, int C, hipStream_t s);
/* da[argmax] += dp (first max in d,h,w scan order wins, as PyTorch)                  */
int pcms_maxpool_bwd(int dtype, const void* a, const void* dp, void* da, int N, int D, int H, int W,
                     int C, hipStream_t s);
/* Block fusion at the encoder's Down3D boundary (a DoubleConv's second BatchNorm3d + ReLU,
 * models/unet3d.py:37-39, and the next MaxPool3d, :80).  Forward: a = relu(y scale + shift)
 * is stored (the block output, also the skip input) and pooled into p in the same pass.
 * Backward: da (the block output's gradient, holding the skip part) += dp at the argmax of a,
 * which is recomputed from y; the pass also writes the BatchNorm-backward partial rows
 * [rows][C][2] for pcms_bn_relu_bwd_finish (rows = pcms_maxpool_bwd_bn_rows(...)).       */
int pcms_bn_relu_pool(int dtype, const void* y, void* a, void* p, const float* scale, const float* shift,
                      int N, int D, int H, int W, int C, hipStream_t s);
int pcms_maxpool_bwd_bn_rows(int dtype, int N, int D, int H, int W, int C);
int pcms_maxpool_bwd_bn(int dtype, const void* y, const float* scale, const float* shift, const float* mean,
                        const float* invstd, const void* dp, void* da, float* part, int N, int D, int H, int W,
                        int C, hipStream_t s);
/* The same pair with da never written: pcms_maxpool_bwd_bn_sums writes only the partial rows
 * (da, holding the skip part, is read); after pcms_bn_relu_bwd_finish(..., dy = NULL) has
 * formed coef, pcms_maxpool_bn_apply forms da = da_skip + dp at the argmax again per 2x2x2 cell
 * (rounded as pcms_maxpool_bwd_bn stores it) and writes dy = k1 g + k2 xhat + k3 -- the same
 * dy bits as pcms_maxpool_bwd_bn + pcms_bn_relu_bwd_finish(dy), one tensor write and read
 * fewer (engine.pool_bn_apply_fused; measured +0.19 % per step, so the engine keeps the pair
 * above by default).                                                                      */
int pcms_maxpool_bwd_bn_sums(int dtype, const void* y, const float* scale, const float* shift, const float* mean,
                             const float* invstd, const void* dp, const void* da, float* part, int N, int D, int H,
                             int W, int C, hipStream_t s);
int pcms_maxpool_bn_apply(int dtype, const void* y, const float* scale, const float* shift, const float* mean,
                          const float* invstd, const float* coef, const void* dp, const void* da, void* dy, int N,
                          int D, int H, int W, int C, hipStream_t s);

/* ---- ConvTranspose3d(k=2, s=2) + F.pad: models/unet3d.py:120,139-151 --------------- */
/* the persistent bf16 forward used at Cin 128 / Cout 64 (level-0 Up3D): on (1) / off (0),
 * v < 0 queries; returns the previous setting (A/B and tests)                          */
int pcms_convt_fwd_stream(int v);
/* elements (activation dtype) of one pack: bf16 8 Cin Cout; fp32 (bf16x6 fragments) 3x that */
int pcms_convt_pack_elems(int dtype, int Cin, int Cout);
int pcms_convt_pack(int dtype, const float* w, void* out, int Cin, int Cout, int dgrad, hipStream_t s);
int pcms_convt_fwd(int dtype, const void* x, const void* wpack, const float* bias, void* out,
                   int N, int Din, int Hin, int Win, int Cin, int Cout, int Do, int Ho, int Wo, hipStream_t s);
/* the same with a K-split workspace for small grids (bf16; fp32 partials summed in a fixed
   order with the bias): ws = pcms_convt_fwd_ws_floats(...) floats (0: no split, ws may be NULL) */
int pcms_convt_fwd_ws_floats(int N, int Din, int Hin, int Win, int Cin, int Cout);
int pcms_convt_fwd_ws(int dtype, const void* x, const void* wpack, const float* bias, void* out, float* ws,
                      int N, int Din, int Hin, int Win, int Cin, int Cout, int Do, int Ho, int Wo, hipStream_t s);
int pcms_convt_dgrad(int dtype, const void* dout, const void* wpack_d, void* dx,
                     int N, int Din, int Hin, int Win, int Cin, int Cout, int Do, int Ho, int Wo, hipStream_t s);
/* the same with an fp32 workspace of pcms_convt_dgrad_ws_floats(...) floats (0: none needed):
 * small grids (the deepest levels) split the 8 Cout reduction into K slabs summed in a fixed
 * order; ws may be NULL (no split)                                                        */
int pcms_convt_dgrad_ws_floats(int N, int Din, int Hin, int Win, int Cin, int Cout);
int pcms_convt_dgrad_ws(int dtype, const void* dout, const void* wpack_d, void* dx, float* ws,
                        int N, int Din, int Hin, int Win, int Cin, int Cout, int Do, int Ho, int Wo, hipStream_t s);
/* dw += ConvTranspose3d weight gradient; ws: pcms_convt_wgrad_ws_floats(...) fp32 (one
 * [Cin][8][Cout] partial row per voxel split, summed in a fixed order)                   */
int pcms_convt_wgrad_ws_floats(int N, int Din, int Hin, int Win, int Cin, int Cout, int target_wgs);
/* A/B switch: taps per workgroup of the bf16 Cin % 128 == 0 weight gradient (8, 4 or 2; 0 =
   chosen by shape); returns the previous setting.  Process-wide. */
/* the ConvTranspose weight gradient's split rows and (bf16 128-channel path) bias rows summed
 * by one launch (1, default) or by the group-sum / reduce / bias-reduce launches (0); the sums
 * are bit-identical; v < 0 queries; returns the previous setting (A/B switch) */
int pcms_convt_reduce_fused(int v);
int pcms_convt_wgrad_taps(int tt);
int pcms_convt_wgrad(int dtype, const void* x, const void* dout, float* dw, float* ws,
                     int N, int Din, int Hin, int Win, int Cin, int Cout, int Do, int Ho, int Wo,
                     int target_wgs, hipStream_t s);
/* pcms_convt_wgrad + the bias gradient db[co] += sum of dout over the ConvT output box
 * (F.pad front offsets floor((Do - 2 Din) / 2), ...), taken from the weight gradient's own
 * read of dout where the kernel allows it (bf16, Cin % 128 == 0), else by
 * pcms_box_channel_sum after it (models/unet3d.py:118-122 ConvTranspose3d bias, autograd);
 * bws: pcms_convt_wgrad_bias_ws_floats(...) fp32                                         */
int pcms_convt_wgrad_bias_ws_floats(int dtype, int N, int Din, int Hin, int Win, int Cin, int Cout, int target_wgs);
int pcms_convt_wgrad_bias(int dtype, const void* x, const void* dout, float* dw, float* db, float* ws, float* bws,
                          int N, int Din, int Hin, int Win, int Cin, int Cout, int Do, int Ho, int Wo,
                          int target_wgs, hipStream_t s);
/* out[c] += sum over the sub-box of x (ConvTranspose3d bias gradient); ws:
 * pcms_box_channel_sum_ws_floats(...) fp32 (per-block partial rows, fixed-order sum)     */
int pcms_box_channel_sum_ws_floats(int dtype, int N, int C, int bd, int bh, int bw);
int pcms_box_channel_sum(int dtype, const void* x, float* out, float* ws, int N, int D, int H, int W, int C,
                         int z0, int y0, int x0, int bd, int bh, int bw, hipStream_t s);

/* ---- outc Conv3d(64, ncls, 1): models/unet3d.py:222,295 ---------------------------- */
/* act 0: logits; 1: sigmoid (UNet3D.predict, :298-318); 2: sigmoid > thr as 0 / 1 floats
 * (UNet3D.inference, :320-344)                                                           */
int pcms_head_fwd(int dtype, const void* a, const float* w, const float* b, float* out,
                  long nvox_per_n, int N, int ncls, int act, float thr, hipStream_t s);
/* da = dlogits . w (written); dw / db += (per-block partial rows in ws, fixed-order sum);
 * ws: pcms_head_bwd_ws_floats(...) fp32                                                  */
int pcms_head_bwd_ws_floats(long nvox_per_n, int N, int ncls);
int pcms_head_bwd(int dtype, const void* a, const float* dlogits, const float* w, void* da, float* dw,
                  float* db, float* ws, long nvox_per_n, int N, int ncls, hipStream_t s);
/* Block fusion of the decoder's last BatchNorm3d + ReLU (models/unet3d.py:37-39, up4's
 * DoubleConv) with the head (:222, :295).  Forward: the head reads that block's pre-BN conv
 * output y and applies BN + ReLU itself (scale / shift from pcms_bn_finalize or
 * pcms_bn_eval_coeffs); the ReLU output is never stored.  Backward: dw / db += the head's
 * gradients, dgamma / dbeta += the BatchNorm's, and dy = the gradient of y -- the head's input
 * gradient is recomputed per voxel from dlogits instead of being stored and read twice.
 * ws: pcms_head_bwd_ws_floats; bnpart: pcms_head_bn_bwd_rows(...) * 64 * 2 fp32; coef: 3*64
 * fp32; bnws: pcms_bn_ws_doubles(64) fp64.  C = 64 input channels.                      */
int pcms_head_bn_fwd(int dtype, const void* y, const float* scale, const float* shift, const float* w,
                     const float* b, float* out, long nvox_per_n, int N, int ncls, int act, float thr,
                     hipStream_t s);
int pcms_head_bn_bwd_rows(long nvox_per_n, int N);
int pcms_head_bn_bwd(int dtype, const void* y, const float* scale, const float* shift, const float* mean,
                     const float* invstd, const float* gamma, const float* dlogits, const float* w, float* dw,
                     float* db, float* ws, float* bnpart, float* coef, float* dgamma, float* dbeta, void* dy,
                     long nvox_per_n, int N, int ncls, double* bnws, hipStream_t s);
/* Eval-mode input-gradient backward of pcms_head_bn_fwd (models/unet3d.py:222, :295 outc and
 * :37-39 up4's last BatchNorm3d + ReLU in eval(), under autograd): dy[v][c] = (sum_k
 * dlogits[k][v] w[k][c]) * scale[c] where y * scale[c] + shift[c] > 0, else 0 -- the gradient of
 * the block's pre-BN conv output y in one pass; no parameter gradient is written.           */
int pcms_head_bn_bwd_eval(int dtype, const void* y, const float* scale, const float* shift, const float* dlogits,
                          const float* w, void* dy, long nvox_per_n, int N, int ncls, hipStream_t s);

/* ---- DiceLoss / BCEDiceLoss: utils/losses.py:44-92, 124-152 ------------------------ */
int pcms_loss_rows(long M);
int pcms_loss_fwd(const float* x, const float* t, long M, float smooth, float wb, float wd, float* part,
                  double* sums, float* loss, hipStream_t s);
int pcms_loss_bwd(const float* x, const float* t, long M, const double* sums, float smooth, float wb,
                  float wd, const float* gout, float* dx, hipStream_t s);

/* ---- Tversky / focal-Tversky region term + focal voxel term (csrc/losses.hip; not in the
 * reference, whose two losses above stay as they are) ------------------------------------
 * x (logits), t (targets): NCDHW fp32, groups * nvox elements.  A group is a contiguous run of
 * nvox elements: groups = 1, nvox = M for region sums over the batch; groups = N*C, nvox =
 * D*H*W for sums per sample and channel.  Per group, p = sigmoid(x):
 *   I = sum p t, P = sum p, T = sum t, D = (1-alpha-beta) I + alpha P + beta T + smooth,
 *   TI = (I + smooth) / D, region_g = max(1 - TI, 0)^gamma          (0 where D <= 0)
 * per voxel, ce = BCE-with-logits, p_t = p t + (1-p)(1-t):
 *   v_i = a_i (1 - p_t)^focal_gamma ce, a_i = focal_alpha t + (1-focal_alpha)(1-t), or 1 with
 *   use_focal_alpha == 0; focal_gamma == 0: v_i = a_i ce
 *   loss = w_region mean_g region_g + w_voxel (1/M) sum_i v_i
 * Forward, two launches: per-block fp32 rows [4] = (sum p t, sum p, sum t, sum v) into part
 * (groups * pcms_region_loss_rows(nvox, groups) * 4 floats; the row count follows
 * pcms_stream_grid_cap), then one block that sums each group's rows in fp64 in row order into
 * sums (groups * 4 doubles) and writes loss (one float) and coef (groups * 2 floats): the
 * backward's (cI, cP) per group, computed in fp64 and rounded once, the 1/groups mean and
 * w_region folded in, 0 where 1 - TI <= 0.
 * Backward, one launch: dx_i = gout [ (cI t_i + cP) p (1-p) + (w_voxel / M) a_i dv_i ], gout a
 * device float or NULL (1).  16-byte accesses on the groups whose base is 16-byte aligned,
 * scalar ones on the others.  Fixed-order sums: the same bits on every run.  No allocation, no
 * host synchronisation.  |x| of any size gives finite values; (1 - p_t) == 0 contributes 0.
 * Negative, no launch: a NULL or misaligned pointer, groups < 1 or > 65535, nvox < 1, groups *
 * nvox >= 2^31, alpha or beta or smooth < 0, gamma <= 0, focal_gamma neither 0 nor >= 1,
 * focal_alpha outside [0, 1] with use_focal_alpha, a non-finite parameter.
 * w_voxel == 0 evaluates no voxel term; focal_gamma == 0 and gamma == 1 evaluate no power.   */
int pcms_region_loss_rows(long nvox, int groups);
int pcms_region_loss_fwd(const float* x, const float* t, long nvox, int groups, float alpha, float beta, float gamma,
                         float smooth, float focal_gamma, int use_focal_alpha, float focal_alpha, float w_region,
                         float w_voxel, float* part, double* sums, float* coef, float* loss, hipStream_t s);
int pcms_region_loss_bwd(const float* x, const float* t, long nvox, int groups, float focal_gamma,
                         int use_focal_alpha, float focal_alpha, float w_voxel, const float* coef, const float* gout,
                         float* dx, hipStream_t s);

/* ---- torch.optim.Adam(lr, weight_decay=1e-5): utils/trainer.py:113-117 ------------- */
/* g_eff = s * g + wd * p, s = gscale * (*gmul if gmul != NULL): gscale = 1/world (the
 * data-parallel mean of summed gradients), *gmul = a device-side multiplier (gradient-clip
 * coefficient x AMP unscale, from pcms_grad_clip).  When s != 1, s * g is written back to g. */
int pcms_adam(float* p, float* g, float* m, float* v, long n, float step_size, float b1, float b2,
              float eps, float wd, float bc2_sqrt, float gscale, const float* gmul, hipStream_t s);
/* The same update split three ways so the weight packs come out of the same pass (bf16
 * build): conv weights by table rows int64[8] = {flat offset, Cout, Cin, fwd pack, dgrad
 * pack, first tile, fwd16 pack, dgrad16 pack} (one 32 x 32 tile per block, Cout % 32 ==
 * Cin % 32 == 0) writing each non-NULL pack: the pcms_conv3_pack2 pair and the
 * pcms_conv3_pack16 pair; ConvTranspose3d weights by rows {offset, Cin, Cout, fwd pack,
 * dgrad pack, first tile, 0, 0} writing both pcms_convt_pack packs; every other parameter
 * through [begin, end) element ranges (int64 pairs).  Identical per-element arithmetic.   */
int pcms_adam_pack_conv3(float* p, float* g, float* m, float* v, const long long* table, int ntab, int ntiles,
                         float step_size, float b1, float b2, float eps, float wd, float bc2_sqrt, float gscale,
                         const float* gmul, hipStream_t s);
int pcms_adam_pack_convt(float* p, float* g, float* m, float* v, const long long* table, int ntab, int ntiles,
                         float step_size, float b1, float b2, float eps, float wd, float bc2_sqrt, float gscale,
                         const float* gmul, hipStream_t s);
/* fp32 build: the same with the bf16x6 packs (pcms_conv3_pack / pcms_convt_pack dtype 0
 * layouts); conv tiles are 32 co x 16 ci (ntiles = sum Cout / 32 x Cin / 16), ConvT tiles
 * 32 x 32 as above.  Replaces the per-step repack of the fp32 build's weights.             */
int pcms_adam_pack_conv3_x6(float* p, float* g, float* m, float* v, const long long* table, int ntab, int ntiles,
                            float step_size, float b1, float b2, float eps, float wd, float bc2_sqrt, float gscale,
                            const float* gmul, hipStream_t s);
int pcms_adam_pack_convt_x6(float* p, float* g, float* m, float* v, const long long* table, int ntab, int ntiles,
                            float step_size, float b1, float b2, float eps, float wd, float bc2_sqrt, float gscale,
                            const float* gmul, hipStream_t s);
int pcms_adam_ranges(float* p, float* g, float* m, float* v, const long long* ranges, int nranges, long max_len,
                     float step_size, float b1, float b2, float eps, float wd, float bc2_sqrt, float gscale,
                     const float* gmul, hipStream_t s);

/* ---- torch.nn.utils.clip_grad_norm_(params, max_norm): train_bph.py:166,
 * train_bph_cv.py:311 ------------------------------------------------------------------
 * norm = gscale * ||g||_2 over the flat gradient (fp64 block partials, fixed-order sum);
 * mul = gscale * min(1, max_norm / (norm + 1e-6)) (max_norm <= 0: gscale) -> device floats;
 * apply != 0: g *= mul in place (else pass mul to pcms_adam as gmul).  A non-finite norm
 * flags inf/NaN gradients (GradScaler's found_inf).  ws: pcms_grad_clip_ws_doubles().      */
int pcms_grad_clip_ws_doubles(void);
/* p[b, e) = v for each int64 [b, e) pair of ranges (the gradient ranges no STORE writer
 * covers, zeroed before a backward into a fresh gradient)                                 */
int pcms_fill_ranges(float* p, const long long* ranges, int nranges, long max_len, float v, hipStream_t s);
int pcms_grad_clip(float* g, long n, float gscale, float max_norm, int apply, double* ws, float* norm_out,
                   float* mul_out, hipStream_t s);

/* ---- misc -------------------------------------------------------------------------- */
int pcms_add(int dtype, void* dst, const void* src, long n, hipStream_t s);
/* NDHWC (Cs stored channels) -> NCDHW fp32 (first C channels): the sub-module outputs
 * (DoubleConv3D / Down3D / Up3D called on their own, models/unet3d.py:42-158)          */
int pcms_unpack_output(int dtype, const void* in, float* out, int N, int C, int Cs, long V, hipStream_t s);

/* ---- loader: resample.resample on the device (script/data_loader.py:240-283, :379-409) --- */
/* One source volume -> one D x H x W fp32 plane (a channel of an NCDHW tensor), equal to
 * resample.resample of the decoded volume bit for bit.  src: the file's voxels in their native
 * type, little endian, (Di, Hi, Wi) with W fastest, aligned to the element size; datatype: the
 * NIfTI-1 code (2 u8, 4 i16, 8 i32, 16 f32, 64 f64, 256 i8, 512 u16, 768 u32, 1024 i64, 1280
 * u64).  A voxel's value is (float)((double)raw * slope + inter) when scl_slope is not 0 or 1
 * or scl_inter is not 0 (slope 0 meaning 1), else (float)raw.  Output index i of an axis
 * samples c = (double)i * ((double)n_in / n_out): neighbours floor(c), floor(c) + 1 clamped to
 * the volume, fp64 lerps a (1 - w) + b w over D, then H, then W (no FMA contraction), one
 * rounding to fp32; 0 where c >= n_in - 0.5 on any axis; an axis with n_in == n_out is copied.
 * An unknown datatype, a dimension < 1, a NULL or misaligned pointer: negative, no launch.  */
int pcms_resample_linear(const void* src, int datatype, int Di, int Hi, int Wi, double scl_slope, double scl_inter,
                         float* out, int D, int H, int W, hipStream_t s);
/* The label form: index k = floor((double)i * ratio + 0.5) per axis (identity when n_in ==
 * n_out), out = 0 where k >= n_in, else (value > 0 ? 1 : 0) with the value scaled in fp64 as
 * above and, as resample.resample returns fp32, rounded to fp32 before the comparison unless the
 * volume already has the target shape (ProstateDataset compares that one as read).        */
int pcms_resample_label(const void* src, int datatype, int Di, int Hi, int Wi, double scl_slope, double scl_inter,
                        float* out, int D, int H, int W, hipStream_t s);
/* Training-time augmentation (resample.resample_affine on the device, bit for bit): the same
 * gather under a 3x4 affine.  affine12: twelve HOST doubles, row-major A[3][3] then t[3],
 * copied into the kernel arguments.  Output index (d, h, w) samples source axis a at
 * c_a = ((A[a][0] d + A[a][1] h) + A[a][2] w) + t[a] in fp64, every product and sum rounded on
 * its own.  Linear: inside iff -0.5 <= c_a < n_a - 0.5 on all axes (decided on the doubles);
 * there i0 = floor(c), w = c - i0, neighbours i0 and i0 + 1 each clamped to [0, n - 1], the 8
 * corners lerped a (1 - w) + b w over D, then H, then W, one rounding to fp32, then -- unless
 * gain == 1 and bias == 0 -- fl32(fl32(r * gain) + bias); outside voxels are 0.  With
 * A = diag(n_in / n_out), t = 0 this is pcms_resample_linear's result.  Rejects what the plain
 * entry points reject, a NULL affine12 and any non-finite affine12 / gain / bias.          */
int pcms_resample_affine_linear(const void* src, int datatype, int Di, int Hi, int Wi, double scl_slope,
                                double scl_inter, const double* affine12, float gain, float bias, float* out, int D,
                                int H, int W, hipStream_t s);
/* The label form: k_a = floor(c_a + 0.5); 0 where any k_a < 0 or k_a >= n_a, else
 * ((float)value > 0 ? 1 : 0), the decoded value always rounded to fp32 first.             */
int pcms_resample_affine_label(const void* src, int datatype, int Di, int Hi, int Wi, double scl_slope,
                               double scl_inter, const double* affine12, float* out, int D, int H, int W,
                               hipStream_t s);
/* Elastic deformation in the same launch (resample.resample_deform on the device, bit for bit).
 * field: gd * gh * gw * 3 DEVICE doubles, the control grid P[gd][gh][gw][3] of a uniform cubic
 * B-spline over the output grid's index space, 8-byte aligned; each workgroup copies it into LDS.
 * For output index i of an axis of extent N with g control points: x = (double)i * ((double)
 * (g - 3) / (double)N), k = floor(x), s = x - k, r = 1 - s, s2 = s s, s3 = s2 s,
 * b0 = ((r r) r) / 6, b1 = ((3 s3 - 6 s2) + 4) / 6, b2 = ((((-3 s3) + 3 s2) + 3 s) + 1) / 6,
 * b3 = s3 / 6, and for component c in (D, H, W)
 * u_c = sum_jd bd[jd] (sum_jh bh[jh] (sum_jw bw[jw] P[kd + jd][kh + jh][kw + jw][c])), every sum
 * left to right from j = 0, every product, sum and IEEE division rounded on its own in fp64.
 * The voxel then samples the source at c_a = ((A[a][0] p_d + A[a][1] p_h) + A[a][2] p_w) + t[a]
 * with p_a = (double)index_a + u_a, and everything after the coordinate is
 * pcms_resample_affine_linear's; a zero field gives its result.  The field's values are not
 * checked (device memory): a non-finite displacement gives a NaN coordinate, which is outside.
 * Rejects what pcms_resample_affine_linear rejects, a NULL or misaligned field, any of gd / gh /
 * gw below 4 and gd * gh * gw above 512.                                                    */
int pcms_resample_deform_linear(const void* src, int datatype, int Di, int Hi, int Wi, double scl_slope,
                                double scl_inter, const double* affine12, const double* field, int gd, int gh, int gw,
                                float gain, float bias, float* out, int D, int H, int W, hipStream_t s);
/* The label form: pcms_resample_affine_label at the deformed position.                      */
int pcms_resample_deform_label(const void* src, int datatype, int Di, int Hi, int Wi, double scl_slope, double scl_inter,
                               const double* affine12, const double* field, int gd, int gh, int gw, float* out, int D,
                               int H, int W, hipStream_t s);

/* ---- case prediction: predict.py's host forms on the device (script/predict.py) ------ */
/* lohi[0] / lohi[1]: the minimum / maximum of the n decoded fp32 values of a volume (decoded
 * as pcms_resample_linear decodes a voxel, so a negative scl_slope is seen), what
 * intensity.normalise takes from numpy's min / max: a NaN anywhere gives NaN for both.  src
 * needs its element's alignment only.  Two launches, deterministic: per-workgroup partials in
 * work (pcms_volume_minmax_work_floats(n) floats, device memory), then one workgroup folds them.
 * An unknown datatype, n < 1, a NULL or misaligned pointer: negative, no launch.            */
int pcms_volume_minmax_work_floats(long n);
int pcms_volume_minmax(const void* src, int datatype, long n, double scl_slope, double scl_inter, float* lohi,
                       float* work, hipStream_t s);
/* pcms_resample_linear with every source voxel v replaced by intensity.normalise's value: with
 * lo = lohi[0], hi = lohi[1] (DEVICE floats, e.g. pcms_volume_minmax's) and den =
 * fl32((double)hi - (double)lo), the corner is fl32(fl32(v - lo) / den), or 0 when den == 0.
 * Equal to resample.resample(intensity.normalise(vol), (D, H, W)) bit for bit; with all three axes
 * identical a plain normalise.  Rejects what pcms_resample_linear rejects and a NULL lohi.    */
int pcms_resample_linear_norm(const void* src, int datatype, int Di, int Hi, int Wi, double scl_slope,
                              double scl_inter, const float* lohi, float* out, int D, int H, int W, hipStream_t s);
/* window.tta_mean: probs holds k contiguous D x H x W fp32 volumes, volume j computed from the
 * input flipped along the axes in flipmask[j] (bit 0: D, bit 1: H, bit 2: W; k HOST ints copied
 * into the kernel arguments).  out = (((p0 + flip(p1)) + flip(p2)) + ...) / (float)k, every fp32
 * sum and the quotient rounded on its own; out must not overlap probs.  1 <= k <= 8 (the
 * distinct flip sets), flipmask[0] == 0, every flipmask[j] in 0..7, else negative, no launch. */
int pcms_flip_mean(const float* probs, int k, const int* flipmask, float* out, int D, int H, int W, hipStream_t s);
/* predict.mask_on_grid in one launch: pcms_resample_linear's gather on an fp32 Dt x Ht x Wt
 * volume, onto the D x H x W grid; mask[i] = value > threshold ? 1 : 0 (strict; bytes), and the
 * fp32 value itself to prob_native unless that is NULL.  Zero (so background) where an axis is
 * sampled at or past n_in - 0.5.  A dimension < 1, a NULL prob or mask, a misaligned float
 * pointer: negative, no launch.                                                            */
int pcms_prob_to_mask(const float* prob, int Dt, int Ht, int Wt, float threshold, unsigned char* mask,
                      float* prob_native, int D, int H, int W, hipStream_t s);

/* ---- mask post-processing: components.py's label_components / postprocess on the device ---- */
/* Foreground is mask != 0 (mask == 0 with invert = 1), the flat index of a voxel is
 * (d H + h) W + w, connectivity is 6, 18 or 26 (offsets in {-1, 0, 1}, at most 1 / 2 / 3 of
 * them nonzero).  work: pcms_components_work_ints(D, H, W) int32 of device memory (negative for
 * a dimension < 1 or a volume too large for an int-sized workspace: more than 2^30 - 32 voxels).
 * Both entry points zero work[0] first and a kernel that runs into one of its iteration caps
 * stores a nonzero status there (it cannot, the caps are the proven bounds), so
 * work[0] must read 0 after the stream has run.  Everything is enqueued on s: no allocation,
 * no host synchronisation, no device-to-host read.  NULL or misaligned pointers, a connectivity
 * other than 6 / 18 / 26, keep_largest outside 0..8, min_voxels < 0, a bad dimension, out
 * overlapping mask: negative, no launch, outputs and work untouched.                        */
int pcms_components_work_ints(int D, int H, int W);
/* labels[i] = 0 on background, 1 + the smallest flat index of the voxel's component on
 * foreground (components.label_components): a function of the mask alone, deterministic.       */
int pcms_components_label(const unsigned char* mask, int invert, int connectivity, int* labels, int* work, int D,
                          int H, int W, hipStream_t s);
/* components.postprocess byte for byte: components ranked by (size descending, label ascending);
 * one stays iff size >= min_voxels and (keep_largest == 0 or rank < keep_largest); then, with
 * fill_holes != 0, every 6-connected background component that touches none of the six faces
 * of the volume becomes 1.  out holds 0 / 1 bytes.                                           */
int pcms_mask_postprocess(const unsigned char* mask, unsigned char* out, int* work, int keep_largest, int min_voxels,
                          int fill_holes, int connectivity, int D, int H, int W, hipStream_t s);

/* ---- surface distances: distance.py's surface / edt_sq / surface_metrics on the device ----- */
/* Volumes are (D, H, W) with W fastest; foreground / feature is byte != 0.  Every axis is at
 * most 2048 long (the H and D passes stage whole lines in LDS) and the volume at most
 * 2^30 - 4096 voxels; pcms_edt_work_bytes(D, H, W) is the bytes of device workspace all three
 * entry points accept (8-byte aligned), negative for a dimension < 1 or a volume past those
 * limits.  Everything is enqueued on s: no allocation, no host synchronisation.  A NULL or
 * misaligned pointer, a bad dimension, a spacing that is not finite and > 0, an output or the
 * workspace overlapping an input or one another: negative, no launch, outputs and work untouched. */
int pcms_edt_work_bytes(int D, int H, int W);
/* out[i] = 1 where voxel i is foreground and one of its six face neighbours is background or
 * lies outside the volume, else 0 (distance.surface).                                          */
int pcms_mask_surface(const unsigned char* mask, unsigned char* out, int D, int H, int W, hipStream_t s);
/* distance.edt_sq bit for bit: out[p] (fp64) = min over feature voxels q of
 * fl(Z(|pd-qd|) + fl(Y(|ph-qh|) + X(|pw-qw|))), X(k) = fl(fl(k sx) fl(k sx)) and Y, Z alike with
 * spacing = {sz, sy, sx}: three HOST doubles copied into the kernel arguments; +inf everywhere
 * when feat has no feature voxel.  Three launches (W, H, D passes), no atomics, every loop
 * bounded by an axis length.                                                                   */
int pcms_edt_sq(const unsigned char* feat, const double* spacing, double* out, void* work, int D, int H, int W,
                hipStream_t s);
/* One direction of distance.surface_metrics.  sq_b: pcms_edt_sq of b's surface.  sd_sq_out[i] =
 * sq_b[i] at the voxels of surface(mask_a) (computed here), -1.0 elsewhere.  stats (device, 24
 * bytes, 8-byte aligned): [0] the number of surface voxels as int64, [1] the maximum of
 * sd_sq_out as a double (-1.0 without a surface voxel), [2] the sum of sqrt(sd_sq_out) over the
 * surface voxels as a double: per-workgroup partials in work, folded by one workgroup in a fixed
 * order, so the sum is the same from run to run.  Two launches.                                */
int pcms_surface_distance_stats(const unsigned char* mask_a, const double* sq_b, double* sd_sq_out, void* stats,
                                void* work, int D, int H, int W, hipStream_t s);

/* ---- lesion analysis: lesions.py's component_table on the device ------------------------- */
/* labels: a canonical label volume (pcms_components_label's output: 0 on background, 1 + the
 * smallest flat index of the component elsewhere).  Voxel i is a root iff labels[i] == i + 1; the
 * row of a component is the number of roots below its own, so rows are in ascending label order.
 * table: pcms_component_table_bytes(capacity, prob != NULL) bytes of device memory, 8-byte
 * aligned, columns of `capacity` entries one after the other:
 *   byte  0 capacity  index_sum  int64 [capacity][3]  sums of d, h, w over the component
 *   byte 24 capacity  label      int32 [capacity]
 *   byte 28 capacity  voxels     int32 [capacity]
 *   byte 32 capacity  bbox       int32 [capacity][6]  dmin, dmax, hmin, hmax, wmin, wmax, inclusive
 * and with prob (fp32, the labels' shape) three more:
 *   byte 56 capacity  peak_key   uint64 [capacity]    (key << 32) | ~flat index of the peak voxel
 *   byte 64 capacity  peak       fp32  [capacity]     the component's maximum of prob
 *   byte 68 capacity  peak_index int32 [capacity]     the smallest flat index attaining it
 * The maximum is taken under the total order of key = bits ^ (sign ? 0xFFFFFFFF : 0x80000000):
 * -0.0 < +0.0 and a positive NaN is above +inf.  Every row of the table is written: a row at or
 * past the component count holds label 0, voxels 0, sums 0, box minima 2^31 - 1 and maxima -1,
 * peak_key 0, peak +0.0, peak_index -1.  header (two int32): [0] status, 0 or nonzero where some
 * label was not canonical (negative, past the volume or not naming a root: that voxel is
 * skipped, nothing is read or written out of bounds); [1] K, the number of components, also when
 * K > capacity -- rows at or past capacity are then written nowhere and the caller sizes a
 * second call from K.  work: pcms_component_table_work_bytes(D, H, W) bytes of device memory,
 * 4-byte aligned (negative for a dimension < 1 or a volume whose workspace does not fit an int:
 * about 2^29 voxels).  Integer atomics only, so the bytes are the same from run to run.
 * Everything is enqueued on s: no allocation, no host synchronisation.  A NULL (but for prob) or
 * misaligned pointer, a bad dimension, capacity < 1, table / header / work overlapping an input
 * or one another: negative, no launch, outputs and work untouched.                            */
int pcms_component_table_work_bytes(int D, int H, int W);
int pcms_component_table_bytes(int capacity, int with_prob);
int pcms_component_table(const int* labels, const float* prob, void* table, int capacity, int* header, void* work,
                         int D, int H, int W, hipStream_t s);

/* ---- sliding-window prediction: window.py's gather_windows / blend_windows on the device ----- */
/* A window is a wd x wh x ww box of a D x H x W volume (W fastest) at a start (sd, sh, sw): three
 * int32 of a DEVICE table; it may stick out past the volume.  flipmask: k HOST ints copied into
 * the kernel arguments, bit 0 / 1 / 2 = the window is mirrored along its D / H / W axis, 1 <= k
 * <= 8, flipmask[0] == 0, every entry in 0..7.  No window axis is longer than 512 (the blend
 * keeps the three weight tables in LDS).  Everything is enqueued on s: no allocation, no host
 * synchronisation, no atomics.  A NULL or misaligned pointer, a size < 1, k outside 1..8,
 * flipmask[0] != 0 or an entry outside 0..7, a window axis above 512, first_window < 0:
 * negative, no launch.                                                                        */
/* window.gather_windows for the B windows of starts[B][3]: out is (B k, C, wd, wh, ww) fp32, all
 * of it written; entry i k + j at (c, a, b, e) is x[c] at start_i + (a', b', e'), the primed index
 * mirrored (n - 1 - index) along the axes of flipmask[j], or 0.f where that lies outside the
 * volume (a start is not checked: whatever it is, nothing outside x is read).  One thread forms
 * four consecutive e; with ww % 4 == 0 and out 16-byte aligned it stores them as one vector.
 * x is (C, D, H, W) fp32 and must not overlap out.  B k C must fit an int.                     */
int pcms_window_gather(const float* x, int C, int D, int H, int W, const int* starts, int B, const int* flipmask, int k,
                       int wd, int wh, int ww, float* out, hipStream_t s);
/* window.blend_windows for windows first_window .. first_window + B - 1 of the whole table
 * starts (row = window index); probs is (B k, wd, wh, ww) fp32, the batch's probabilities in
 * pcms_window_gather's entry order.  wts: wd + wh + ww DEVICE floats, the three per-axis tables
 * one after the other.  One thread per voxel of the batch's bounding box (found on the device,
 * clipped to the volume) reads acc and wsum once, visits the batch's windows covering the voxel
 * in ascending index -- m = (((p_0 + p_1 at the mirrored index) + ...) / (float)k as
 * pcms_flip_mean forms it (no division for k == 1), wgt = fl(fl(wtd[a] wth[b]) wtw[e]),
 * acc = fl(acc + fl(wgt m)), wsum = fl(wsum + wgt) -- and writes each once.  The result is the
 * same bits however the windows are split into batches, as long as the batches are consecutive
 * index ranges sent in ascending order on one stream.  acc and wsum are D x H x W fp32, zeroed
 * by the caller before the first batch; nothing may overlap.                                   */
int pcms_window_blend(const float* probs, const int* starts, int first_window, int B, const int* flipmask, int k,
                      const float* wts, int wd, int wh, int ww, float* acc, float* wsum, int D, int H, int W,
                      hipStream_t s);
/* prob[i] = acc[i] / wsum[i] (correctly rounded fp32 division) for i < n; 16-byte loads and
 * stores where the three pointers share their offset within 16 bytes.  prob overlaps neither.  */
int pcms_window_finish(const float* acc, const float* wsum, float* prob, long n, hipStream_t s);

/* ---- patch training: data.py's pick_origins / resample_patch on the device ------------------ */
/* A patch is a wd x wh x ww box of a Gd x Gh x Gw grid (W fastest) at an origin: three int32.
 * Everything is enqueued on s: no allocation, no host synchronisation, no atomics, so the bytes
 * are the same from run to run.                                                                */
/* data.pick_origins: label is the grid's n = Gd Gh Gw DEVICE floats, foreground where > 0 (a NaN
 * is background), T their number.  rank_u: P DEVICE doubles; fallback: P x 3 DEVICE int32.  picks:
 * 3 P + 1 DEVICE int32, the P origins, then T.  Patch p takes its fallback row, each entry
 * clamped into [0, max(G_a - w_a, 0)], when rank_u[p] < 0 or T == 0.  Otherwise r = floor(rank_u[p]
 * (double)T) capped at T - 1 -- the test is !(r < T - 1), so a NaN or a rank of 1 or more gives
 * T - 1 -- v is the r-th foreground voxel in flat order (d Gh + h) Gw + w, and the origin is
 * min(max(v_a - w_a / 2, 0), max(G_a - w_a, 0)) per axis (integer division).  Neither table is
 * trusted: whatever they hold, nothing outside label is read and nothing outside picks written.
 * Three launches: workgroups count the foreground of chunks of pcms_foreground_pick_chunk()
 * consecutive voxels (16-byte loads when label is 16-byte aligned), one workgroup scans the counts
 * exclusively in place, one workgroup per patch finds its chunk by binary search, re-reads it and
 * locates the voxel by ballots.  work: pcms_foreground_pick_work_ints(n) DEVICE int32 (negative
 * for n < 1 or n >= 2^31).  P outside 1..64, n != Gd Gh Gw or n >= 2^31, a grid or patch axis
 * < 1, a NULL or misaligned pointer: negative, no launch.                                       */
int pcms_foreground_pick_chunk(void);
int pcms_foreground_pick_work_ints(long n);
int pcms_foreground_pick(const float* label, long n, int Gd, int Gh, int Gw, int wd, int wh, int ww,
                         const double* rank_u, const int* fallback, int P, int* picks, int* work, hipStream_t s);
/* data.resample_patch for the P patches at origins[P][3] (DEVICE int32, e.g. pcms_foreground_pick's
 * picks), bit for bit: out + p patch_stride (patch_stride counted in floats, >= D H W, so out can
 * be channel c of a (P, M, D, H, W) batch) is patch p, D x H x W fp32, all of it written.  Patch
 * index (a, b, e) stands for grid index q = (a, b, e) + origin_p, formed in 64-bit integers; the
 * voxel is 0.f where any q_a < 0 or q_a >= G_a, else pcms_resample_affine_linear's value at output
 * index q: c_a = ((A[a][0] q_d + A[a][1] q_h) + A[a][2] q_w) + t[a] and everything after the
 * coordinate.  An origin is not checked: the zero rule and the inside rule on the doubles mean
 * nothing outside src is read.  src, datatype, Di .. scl_inter, affine12 (twelve HOST doubles),
 * gain, bias: as pcms_resample_affine_linear takes them.  lohi: NULL, or two DEVICE floats (e.g.
 * pcms_volume_minmax's) that select pcms_resample_linear_norm's corner fl32(fl32(v - lo) / den),
 * den = fl32((double)hi - (double)lo), 0 when den == 0.  One thread forms four consecutive e of a
 * row and stores 16 bytes when W % 4 == 0 and out and patch_stride are 16-byte aligned, else up
 * to four scalars.  Rejects what pcms_resample_affine_linear rejects, a grid axis < 1, a NULL or
 * misaligned origins, a misaligned lohi, P outside 1..64, patch_stride < D H W and D H above
 * 2^31 - 1: negative, no launch.                                                              */
int pcms_patch_resample_linear(const void* src, int datatype, int Di, int Hi, int Wi, double scl_slope,
                               double scl_inter, const double* affine12, const float* lohi, float gain, float bias,
                               int Gd, int Gh, int Gw, const int* origins, int P, float* out, long patch_stride, int D,
                               int H, int W, hipStream_t s);

/* ---- percentile intensity window: intensity.py's intensity_window / normalise_window ------- */
/* intensity.intensity_window on the device, bit for bit: lohi[0] / lohi[1] (DEVICE floats) are the
 * values at ranks r_lo / r_hi of the ascending order of the selected voxels.  A voxel is decoded as
 * pcms_volume_minmax decodes it and replaced by v + 0.f (-0 becomes +0); the selected set is every
 * voxel, or with use_above != 0 the voxels with v > above (never a NaN); m is its size.  ppm_lo <
 * ppm_hi are the two percentiles in parts per million (0 .. 1000000) and r_lo = floor(ppm_lo
 * (m - 1) / 10^6), r_hi = ceil(ppm_hi (m - 1) / 10^6) in 64-bit integers, formed on the device.
 * NaNs order last (a selected NaN reads back as a quiet NaN); m == 0 gives (0, 0).  (0, 1000000)
 * gives pcms_volume_minmax's pair on a NaN-free volume.
 * Method: a most-significant-digit radix select of both ranks at once on the order-preserving
 * u32 image of the value (every NaN the top key), 8 bits per pass: one launch zeroes work, then
 * four times a histogram launch (16-byte loads on the aligned body, a grid capped through
 * pcms_stream_grid_cap; per workgroup a 2 x 256-bin LDS histogram whose adds are aggregated over
 * the wave's lanes that share a bin, then one integer atomic per non-empty bin into one of eight
 * copies of the rows in work) and a one-workgroup launch that sums the copies, scans the bins
 * and fixes the next digit and the rank left inside it.
 * Integer counts only: the same bits on every run.  Everything is enqueued on s: no allocation,
 * no host synchronisation; work is pcms_volume_window_work_bytes(n) bytes of DEVICE memory,
 * 8-byte aligned, in any state (negative for n < 1 or n >= 2^31).  src needs its element's
 * alignment only.  An unknown datatype, n < 1 or n >= 2^31, a NULL or misaligned pointer, ppm_lo
 * < 0, ppm_hi > 1000000, ppm_lo >= ppm_hi, a non-finite above with use_above: negative, no
 * launch.                                                                                      */
int pcms_volume_window_work_bytes(long n);
int pcms_volume_window(const void* src, int datatype, long n, double scl_slope, double scl_inter, int ppm_lo,
                       int ppm_hi, int use_above, float above, float* lohi, void* work, hipStream_t s);
/* pcms_resample_linear_norm with intensity.normalise_window's corner: with lo = lohi[0], hi =
 * lohi[1] (DEVICE floats, e.g. pcms_volume_window's) and den = fl32((double)hi - (double)lo), a
 * source voxel v becomes c = v < lo ? lo : v > hi ? hi : v (a NaN stays), then fl32(fl32(c - lo)
 * / den), or 0 when den == 0.  Equal to resample.resample(intensity.normalise_window(vol, lohi), (D, H,
 * W)) bit for bit.  Rejects what pcms_resample_linear_norm rejects.                            */
int pcms_resample_linear_window(const void* src, int datatype, int Di, int Hi, int Wi, double scl_slope,
                                double scl_inter, const float* lohi, float* out, int D, int H, int W, hipStream_t s);
/* pcms_patch_resample_linear with that corner: data.resample_patch of
 * intensity.normalise_window(vol, lohi), bit for bit.  lohi is required; every other argument, the
 * 16-byte / scalar store rule and the rejections are pcms_patch_resample_linear's, and a NULL
 * lohi is rejected too.                                                                        */
int pcms_patch_resample_window(const void* src, int datatype, int Di, int Hi, int Wi, double scl_slope,
                               double scl_inter, const double* affine12, const float* lohi, float gain, float bias,
                               int Gd, int Gh, int Gw, const int* origins, int P, float* out, long patch_stride, int D,
                               int H, int W, hipStream_t s);

/* ---- modality alignment: align.py's joint_histogram --------------------------------------- */
/* align.joint_histogram on the device, on the counts exactly: the joint intensity histogram of
 * a fixed and a moving raw volume under an affine, the table a mutual-information similarity is
 * formed from.  The lattice is every (sd, sh, sw)-th voxel of the fixed volume, q = (a sd, b sh,
 * e sw) with q inside (Df, Hf, Wf).  For a lattice voxel q: the moving coordinate is c_a =
 * ((A[a][0] q_d + A[a][1] q_h) + A[a][2] q_w) + t[a] (fp64, pcms_resample_affine_linear's); the
 * voxel counts iff -0.5 <= c_a < n_a - 0.5 on all three moving axes and neither value below is a
 * NaN.  f: the fixed voxel decoded as pcms_resample_linear decodes it, then
 * pcms_resample_linear_window's corner under flohi (clip to [lo, hi] by comparisons, fl32(fl32(c
 * - lo) / den), 0 when den == 0).  m: pcms_resample_affine_linear's 8-corner sample (gain 1, bias
 * 0) of the moving volume's corners treated the same way under mlohi.  The bin of a value v is
 * (int) of fl32(v * (float)bins) clamped to [0, bins - 1] -- min((int)fl32(v bins), bins - 1) for
 * v in [0, 1] -- and hist[bf * bins + bm] (bins * bins DEVICE uint32, all of it written) is the
 * number of counted voxels with that pair; the sum of the table is the overlap count.
 * flohi / mlohi: two DEVICE floats each (pcms_volume_minmax's or pcms_volume_window's), read on
 * the device.  affine12: twelve HOST doubles, row-major A then t, read during the call.
 * Method: one launch zeroes work; one thread per lattice voxel, grid-stride (a grid capped
 * through pcms_stream_grid_cap), counts into a 64 x 64 table of 32-bit counts in LDS by integer
 * atomics aggregated over the wave's lanes that share a bin, then one integer atomic per
 * non-empty bin and workgroup into one of eight copies of the table in work; a third launch sums
 * the copies into hist.  Integer counts only: the same bits on every run.  Everything is enqueued
 * on s: no allocation, no host synchronisation; work is pcms_joint_histogram_work_bytes(bins)
 * bytes of DEVICE memory, 4-byte aligned, in any state (negative for bins outside 2..64).  fix
 * and mov need their element's alignment only.  bins outside 2..64, a stride or an extent below
 * 1, a lattice of 2^31 voxels or more, a NULL or misaligned pointer, an unknown datatype, a
 * non-finite affine: negative, no launch.                                                     */
int pcms_joint_histogram_work_bytes(int bins);
int pcms_joint_histogram(const void* fix, int fdatatype, int Df, int Hf, int Wf, double fslope, double finter,
                         const float* flohi, const void* mov, int mdatatype, int Dm, int Hm, int Wm, double mslope,
                         double minter, const float* mlohi, const double* affine12, int sd, int sh, int sw, int bins,
                         unsigned* hist, void* work, hipStream_t s);

/* ---- mutually exclusive classes (csrc/classes.hip; classes.py has the host forms) ----------- */
/* SoftmaxDiceCELoss.  x: (N, C, nvox) fp32 logits, 2 <= C <= 8; target: the (N, nvox) class map,
 * fp32 (target_u8 == 0) or uint8, read as it is.  A voxel whose label is not an integer in [0, C)
 * is ignored: it enters no sum and its gradient is 0.  Per voxel p = softmax_c(x) (the maximum
 * subtracted, the sum in class order), y the one-hot label.  A group is the batch (per_sample ==
 * 0) or one sample; over its valid voxels
 *   I_c = sum p_c y_c, P_c = sum p_c, T_c = sum y_c, dice_c = (2 I_c + smooth) / (P_c + T_c + smooth)
 *   (1 where the denominator is not positive), region_g = mean_{c in K} (1 - dice_c), K = {1..C-1}
 *   or {0..C-1} with include_background;
 *   CE = sum_i w[y_i] (-log p_{y_i}) / sum_i w[y_i] over the batch's valid voxels, 0 without one;
 *   loss = ce_weight CE + dice_weight mean_g region_g.
 * class_weights: C HOST floats >= 0 read during the call, or NULL (ones).
 * Forward, two launches: per-block fp32 rows [3C + 2] = (I_c, P_c, T_c, CE numerator, sum w) into
 * part (N * pcms_softmax_loss_rows(nvox, N) * (3C + 2) floats, sample-major; the row count follows
 * pcms_stream_grid_cap), then one block that sums each group's rows in fp64 in a fixed order into
 * sums (groups * (3C + 2) doubles, groups = N or 1) and writes loss (one float) and coef (groups *
 * 2C + 1 floats): per group A_c then B_c with dL/dp_c = A_c y_c + B_c (fp64, rounded once,
 * dice_weight and both means folded in, 0 outside K), then one float ce_weight / sum w (0 without
 * a valid voxel).
 * Backward, one launch: dx_k = gout [ p_k (g_k - sum_j p_j g_j) + (ce_weight / sum w) w[y]
 * (p_k - y_k) ], g_c = A_c y_c + B_c; gout a device float or NULL (1).  Each thread reads its
 * voxels' C logits from the C planes, four voxels per 16-byte access where nvox % 4 == 0 and the
 * sample's bases allow it, scalar accesses otherwise.  Fixed-order sums: the same bits on every
 * run.  Finite results for finite logits of any size.  No allocation, no host synchronisation.
 * Negative, no launch: a NULL or misaligned pointer, C outside 2..8, N < 1 or > 65535, nvox < 1 or
 * >= 2^31, smooth < 0, a negative class weight, a non-finite parameter.                        */
int pcms_softmax_loss_rows(long nvox, int N);
int pcms_softmax_loss_fwd(const float* x, const void* target, int target_u8, long nvox, int N, int C, int per_sample,
                          int include_background, float smooth, float ce_weight, float dice_weight,
                          const float* class_weights, float* part, double* sums, float* coef, float* loss,
                          hipStream_t s);
int pcms_softmax_loss_bwd(const float* x, const void* target, int target_u8, long nvox, int N, int C, int per_sample,
                          const float* class_weights, const float* coef, const float* gout, float* dx,
                          hipStream_t s);
/* Class-map labels: pcms_resample_label's / pcms_resample_affine_label's nearest index rules and
 * decoding, bit for bit, with a table in place of `> 0`: out = j + 1 (fp32) for the first j with
 * fl32(decoded value) == class_values[j], else 0 (also outside the source).  class_values:
 * n_values (1..7) finite HOST floats copied into the kernel arguments.  Equal to
 * classes.classes_of(resample.resample(vol, target, nearest=True), class_values) and to the same
 * after resample.resample_affine(..., nearest=True), byte for byte.  Negative, no launch: the
 * label entry points' cases, a NULL table, n_values outside 1..7, a non-finite value.          */
int pcms_resample_classes(const void* src, int datatype, int Di, int Hi, int Wi, double scl_slope, double scl_inter,
                          const float* class_values, int n_values, float* out, int D, int H, int W, hipStream_t s);
int pcms_resample_affine_classes(const void* src, int datatype, int Di, int Hi, int Wi, double scl_slope,
                                 double scl_inter, const double* affine12, const float* class_values, int n_values,
                                 float* out, int D, int H, int W, hipStream_t s);
/* logits (B, C, n) fp32 -> probs (C, B, n), class-major, so that the B volumes of a class are
 * contiguous (pcms_flip_mean takes them as they are): m = max_c x_c, e_c = expf(x_c - m), s summed
 * in class order, p_c = e_c / s.  16-byte accesses where n % 4 == 0 and both bases allow it.
 * Negative, no launch: a NULL or misaligned pointer, overlapping buffers, B or n < 1, C outside
 * 2..8.                                                                                        */
int pcms_softmax_planes(const float* logits, int B, int C, long n, float* probs, hipStream_t s);
/* classes.labels_on_grid: probs (C, Dt, Ht, Wt) -> labels (D, H, W) uint8.  pcms_prob_to_mask's
 * linear gather runs on every class plane (the same bits); the label is the class of the largest
 * value, the first one winning (strict >), so a voxel outside the volume (all zeros) gets class
 * 0.  probs_native (C, D, H, W fp32) receives the gathered planes unless NULL.  Negative, no
 * launch: a NULL or misaligned pointer, C outside 1..8, an extent below 1.                     */
int pcms_probs_to_labels(const float* probs, int C, int Dt, int Ht, int Wt, unsigned char* labels, float* probs_native,
                         int D, int H, int W, hipStream_t s);
/* counts[3 c + (0, 1, 2)] = |pred == c|, |ref == c|, |pred == c and ref == c| for c < C over two
 * uint8 class maps of n voxels (counts: 3 C DEVICE int64, zeroed on s by the call).  Integer
 * atomics aggregated over the lanes of a wave that share a class: exact, the same on every run.
 * Negative, no launch: a NULL pointer, misaligned counts, n < 1, C outside 1..8.               */
int pcms_class_overlap(const unsigned char* pred, const unsigned char* ref, long n, int C, long* counts,
                       hipStream_t s);

/* ---- measurement (bench.py, not a training path) ----------------------------------- */
/* One launch of nblocks single-wave workgroups; block b writes {s_memtime, s_memrealtime,
 * XCC id} to out[3b .. 3b+2] (uint64).  Two probes around a stretch of work give each XCD's
 * average shader clock over it: d(memtime) / d(memrealtime) x 100 MHz.                    */
int pcms_clock_probe(void* out, int nblocks, hipStream_t s);
/* check of the probe: every block spins `cycles` shader cycles and writes its own {t0, r0,
 * t1, r1, XCC id} to out[5b ..] (tests/tools/clock_check.py)                              */
int pcms_clock_spin(void* out, int nblocks, long cycles, hipStream_t s);

#ifdef __cplusplus
}
#endif
#endif /* PCMS_HIP_H */
