/* vrnet_hip.h -- C ABI of libvrnet_hip.so: MI355X (gfx950) kernels for the ASY-VRNet fusion hot path.
 *
 * The drop-in boundary of this repository (DESIGN.md "Boundary").  Plain pointers and sizes only: no
 * torch types.  Every pointer is a DEVICE pointer unless stated; every function enqueues work on the HIP
 * stream `stream` (a hipStream_t passed as void*) and returns without synchronising:
 *   0 = ok, 1 = bad argument, 2 = launch failure, 3 = workspace too small; the message of the last
 *   failure on the calling thread is returned by vrnet_last_error().
 * Tensors are fp32, NHWC, addressed as rows of pixels: element (pixel r, channel c) of tensor t lives at
 * t[r * ld + c]; `ld` (row stride in floats) >= channel count lets a tensor be a channel slice of a wider
 * buffer (torch.cat is never materialised by a copy of the producer's output).  `accumulate` != 0 makes an
 * output `+=` instead of `=` (gradient fan-in).
 *
 * Each entry point names the reference code (GuanRunwei/ASY-VRNet, file:line) it replaces; the reference
 * is pure PyTorch, so "replaces" means the ATen op sequence the reference module executes there.
 * The reference-side binding a maintainer would add is a ctypes stub: see INTEGRATION.md.
 */
#ifndef VRNET_HIP_H
#define VRNET_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---- library ------------------------------------------------------------------------------------- */
int vrnet_abi_version(void);                 /* == 11 */
/* Kernel family the last vrnet_conv2d_f32 / vrnet_conv2d_wgrad_f32 call of this thread dispatched to: 1 fp32 MFMA
 * (register-staged), 2 fp32 MFMA (LDS-DMA ring), 3 bf16-rounded operands, 4 direct kernels for tiny channel counts,
 * 5 direct HBM-streaming kernels for 1x1 convs with <= 16 output channels over wide inputs (head predictions, seg logits),
 * 6 "x6": every fp32 product as six exact bf16 x bf16 products on the bf16 MFMA, fp32 accumulate;
 * 9: x6 with pre-split weights (vrnet_conv2d_f32 `w_planes`);
 * 7 / 8: the fused Mlp kernels (vrnet_mlp_fwd_f32 / vrnet_mlp_bwd_f32) at precision 2 (x6) / 1 (bf16-rounded operands);
 * 10 / 11: plane GEMM forward / data gradient (vrnet_gemm_planes_f32) with np = 3 / 1; 12 / 13: plane weight gradient. */
int vrnet_last_kernel(void);
/* Launches of kernel family `family` (same codes) issued by this process (all threads) since the library was loaded. */
long vrnet_kernel_launches(int family);
const char* vrnet_last_error(void);          /* host string, thread local */
/* Diagnostic: a one-thread kernel writes the device's constant-rate clock (wall_clock64, 100 MHz) to *dst in stream order:
 * section timelines of the captured step without a tracer attached (no reference counterpart). */
int vrnet_clock_stamp(long long* dst, void* stream);
/* 0 for the product library, which reads NO environment variable; 1 for the diagnostic build (make tuning:
 * libvrnet_hip_tuning.so, -DVR_TUNING) in which the VRNET_* dispatch knobs and the VRNET_ABLATE launch-skipping timing
 * ablation exist.  Benchmarks must refuse a library that answers 1. */
int vrnet_tuning_build(void);
int vrnet_device_arch(char* buf, int len);   /* host buffer <- e.g. "gfx950:sramecc+:xnack-" (synchronous) */

/* ---- dense convolution as implicit GEMM on the fp32 MFMA ------------------------------------------
 * Replaces nn.Conv2d forward / input-gradient for every dense conv of the path:
 *   Cluster fc1, fc_v, fc2 (backbone/fusion/vr_coc.py:145-147,156-157,191), Mlp fc1/fc2 (:205-207,217-223),
 *   PointRecuder.proj k1 / k4s4 / k3s2p1 (:83-102), BaseConv.conv (backbone/conv_utils/normal_conv.py:41,48),
 *   ASPP 1x1 + dilated 3x3 (neck/coc_fpn_dual.py:50-77), head stems / pconv / preds (head/decouplehead.py:21-40).
 * Geometry is always the FORWARD convolution's: input (B,H,W,Cin), output (B,OH,OW,Cout), kernel kh x kw.
 * w: weights packed [kh*kw][Cout][Cin] (vrnet_pack_weight_f32; for 1x1 this IS the OIHW tensor).
 * mode 0: y(B,OH,OW,Cout) = conv(a = x).   mode 1: y(B,H,W,Cin) = d/dx given a = dy(B,OH,OW,Cout).
 * Fused epilogue, in this order (each optional, NULL/0 = off):
 *   v = acc + bias[n];  v *= gelu'(aux[m,n]) (Mlp backward);  ypre[m,n] = v (pre-activation / branch output);
 *   act: 1 ReLU, 2 exact-erf GELU;  v = res[m,n] + res_scale[n] * v (layer-scale residual, vr_coc.py:266-271);
 *   store NHWC y[m*ldy+n] or NCHW y[b][out_coff+n][pix] of a (B,out_ctot,OH,OW) tensor (head cat, decouplehead.py:86).
 * kscale[k]: multiplies the contraction channels of `a` (layer scale folded into the data gradient).
 * precision: 2 = every fp32 product as six exact bf16 x bf16 products (operands split into three bf16 values each,
 *   a0b0 + a0b1 + a1b0 + a0b2 + a2b0 + a1b1 on v_mfma_f32_32x32x16_bf16, fp32 accumulate: fp32 rounding-level error,
 *   2.7x the matrix rate of the fp32 MFMA) on the LDS-DMA tile kernels where vrnet_conv2d_dma_tile() != 0, the fp32 MFMA
 *   elsewhere -- the default of the fp32 path; 3 = bf16-rounded operands on those tile kernels, standard weight layout;
 *   0 = fp32 operands on v_mfma_f32_32x32x2_f32 only; 1 = operands rounded to bf16 while staged,
 *   v_mfma_f32_32x32x16_bf16, fp32 accumulate and epilogue (BASELINE configs "bf16 with MFMA conv path"): needs
 *   16-byte rows, Cin % 4 == 0 (mode 0) / Cout % 4 == 0 (mode 1), > 32 GEMM columns, and in mode 1 `w` =
 *   vrnet_pack_weight_t_f32's [kh*kw][Cin][Cout] pack with kscale folded in (kscale itself must then be NULL).
 * stats (NULL = none; forward, NHWC, Cout > 32, OH*OW % 32 == 0): [ceil(M/32)][ceil(Cout/32)][2] fp64 (sum, sum of
 *   squares) of the STORED outputs per 32-row x 32-channel tile -- the GroupNorm statistics of the consumer
 *   (vrnet_gn_coef_from_pairs: OH*OW/32 * ceil(Cout/32) consecutive pairs per sample) without another pass over y.
 * Two-stream launch (pair_rows > 0): the image chain and the radar chain of a backbone stage run the same layer
 *   shapes on their own parameters (vr_coc.py:589-600: network[idx](x), network_radar[idx](x_radar)); with both
 *   streams stacked along the batch, GEMM rows < pair_rows use (w, bias, res_scale, kscale) and rows >= pair_rows use
 *   (w2, bias2, res_scale2, kscale2) -- one launch with twice the tiles instead of two.  pair_rows % 128 == 0. */
/* Tile the LDS-DMA x6 / bf16 kernels would use for a GEMM of `rows` x `cols` (mode 0: output pixels x Cout; mode 1: input
 * pixels x Cin): 22 (128 x 128), 21 (128 x 64) or 0 = no such kernel for the shape.  precision 2 falls back to the fp32
 * MFMA by itself; precision 3 (bf16-rounded operands with the STANDARD weight layout in both modes, kscale allowed) is only
 * accepted where this returns non-zero. */
int vrnet_conv2d_dma_tile(long rows, int cols);
/* Optional column statistics of the STORED outputs (NULL = none; NHWC vector epilogue, > 32 output channels, not for
 * stride-2 data gradients): what a separate pass over the output tensor would otherwise compute.
 *   partial[mb][n] = (sum_m v[m,n], sum_m v[m,n] * f[m,n]) over the 32 rows of row tile mb, f = x2 (row stride ldx2) or,
 *     with x2 == NULL, v itself: the chunk partials of train-mode BatchNorm statistics (vrnet_bn_coef_fwd_partial, forward
 *     conv of a BaseConv, normal_conv.py:45-49) and of GroupNorm's backward moments (data gradient of the conv behind a
 *     GroupNorm, x2 = the GroupNorm input; vr_coc.py:264-271), in the layout [row tile][channel][2] of the moments kernel;
 *   tile_totals[mb][n / 32] = the same two sums weighted by gamma[n] and added over the tile's 32 columns (GroupNorm
 *     backward: per-sample coefficients, vrnet_gn_apply_bwd_from_partials). */
typedef struct vrnet_conv_colstats {
  double* partial;
  const float* x2; long ldx2;
  const float* gamma;
  double* tile_totals;
} vrnet_conv_colstats;
int vrnet_conv2d_f32(const float* a, long lda, const float* w, const float* bias, float* y, long ldy,
                     int B, int H, int W, int Cin, int OH, int OW, int Cout, int kh, int kw, int stride, int pad,
                     int dil, int mode, int act, float* ypre, long ldypre, const float* res, long ldres,
                     const float* res_scale, const float* kscale, const float* aux, long ldaux, int out_nchw,
                     int out_ctot, int out_coff, int accumulate, double* stats, int precision, int pair_rows,
                     const float* w2, const float* bias2, const float* res_scale2, const float* kscale2,
                     const void* w_planes, const vrnet_conv_colstats* colstats, void* workspace, long workspace_bytes,
                     void* stream);
/* Split contraction (round 4): a 2048-row map (16 x 16 at batch 8) has 64-128 tiles of 128 x 64 for 256 CUs, so at
 * precision 2 such layers ran on 64 x 64 fp32-MFMA tiles at 40-70 TFLOP/s.  With a `workspace` of
 * vrnet_conv2d_splitk_workspace(rows, cols, ktot) bytes (rows x cols = the GEMM: B*OH*OW x Cout forward, B*H*W x Cin data
 * gradient; ktot = contraction length incl. taps; 0 = the shape is not split) the x6 tile kernels take them: `splits`
 * workgroups per tile each run a share of the K loop and leave raw accumulators in the workspace, a finishing launch adds
 * the slabs in order (deterministic) and runs the usual fused epilogue.  workspace NULL: never split.
 * vrnet_conv2d_dma_plan: the tile (as vrnet_conv2d_dma_tile, or 21 for a split launch) and *splits. */
long vrnet_conv2d_splitk_workspace(long rows, int cols, long ktot);
int vrnet_conv2d_dma_plan(long rows, int cols, long ktot, int* splits);
/* What vrnet_conv2d_f32 launches for a single-stream call (pair_rows = 0): a host-only query, answered by the function the
 * launcher itself dispatches on.  Geometry, mode, precision and the row strides lda, ldy as in vrnet_conv2d_f32;
 * workspace_bytes: the split workspace the call would be given (0: none).  flags, one bit per condition the dispatch reads:
 *      1 a      2 w      4 y        16-byte aligned bases
 *      8 bias  16 ypre  32 res  64 res_scale  128 aux    absent, or an aligned base and (ypre, res, aux) a row stride % 4 == 0
 *    256 kscale given           512 no fused epilogue operand: no ypre, res, kscale, aux, act
 *   1024 out_nchw              2048 stats given          4096 colstats given          8192 w_planes given
 * out[12]:
 *   0 family   what vrnet_last_kernel reports after the call
 *   1 kernel   0 igemm_kernel (tile 128032 / 128064 / 64064 = rows x columns per workgroup), 1 the fp32 LDS-DMA ring
 *              igemm_dma_kernel<mode, 3, 1, 1> (64064), 2 the x6 tile kernels (tile 22 = 128 x 128, 21 = 128 x 64), 3 the same
 *              tiles on bf16-rounded operands, 4 igemm_planes_kernel<TN, NST, KXK> on pre-split weights (22 / 21), 5 igemm_bf16_kernel
 *              (64064), 6 the tiny-channel kernels, 7 the narrow-output kernels, 8 the patch data gradient (6-8: the rest is 0)
 *   2 tile     3 S   splits of the contraction (> 1: igemm_splitk_finish_kernel follows)
 *   4 k_live   the contraction length that counts for the split: taps that reach the image for at least one row
 *   5 perm2    parity-major rows of a stride-2 data gradient
 *   6 a_vec    7 b_vec   16-byte loaders of the activation / weight operand      8 e_vec   vector epilogue
 *   9 grid x  10 grid y  11 workgroups of the finish kernel (0: none)
 * Returns non-zero where vrnet_conv2d_f32 refuses the call (precision 1 / 3 without a kernel for the shape or alignment,
 * statistics without the vector epilogue, bad geometry), with the launcher's message. */
int vrnet_conv2d_plan(int B, int H, int W, int Cin, int OH, int OW, int Cout, int kh, int kw, int stride, int pad, int dil,
                      int mode, int precision, long lda, long ldy, int flags, long workspace_bytes, int* out);
/* Pre-split weights for the x6 kernels (precision 2, 1x1 convs, contraction % 16 == 0): the six-product scheme spends its
 * VALU time on splitting fragments into bf16 planes; weights are the same for every row tile of a step, so they can be
 * split ONCE per step.  vrnet_conv_planes_pack_f32 does that for a whole table of weights in one launch (round-to-nearest-
 * even: w = p0 + p1 + p2 exactly), writing each as the LDS stage image of the kernel ([k16 step][64-column block][plane]
 * [lane half][64 columns] x 8 bf16); `w_planes` of vrnet_conv2d_f32 passes one such pack (NULL = split in the kernel).
 * mode 0: columns J = Cout, contraction K = Cin (source strides Cin, 1 for an OIHW 1x1 weight); mode 1: J = Cin, K = Cout
 * (strides 1, Cin) with kscale folded in through the table's scale address (the kscale argument is then ignored).
 * `w` is still required: shapes without a tile kernel (vrnet_conv2d_dma_tile == 0) use it.  Kernel family 9.
 * k x k convs (2 .. 32 taps, any stride / padding / dilation; the 128 x 64 tile, split or not): the pack is kh * kw such images
 * in ONE buffer of vrnet_conv_planes_bytes(J, kh * kw * K) bytes, tap t = ky * kw + kx at K16 steps [t * K / 16, (t + 1) * K / 16),
 * i.e. one table entry per tap on the OIHW weight: source w + t, destination + t * vrnet_conv_planes_bytes(J, K), and 2^32 added
 * to the entry's J: such an entry is split by truncation, into the planes igemm_dma_kernel makes of the weight fragments it
 * splits itself, so a k x k launch gives the same bits with planes as without (a 1x1 entry stays round-to-nearest-even); mode 0 strides
 * (Cin * kh * kw, kh * kw), mode 1 (kh * kw, Cin * kh * kw) with kscale as for 1x1.  A call whose plan (vrnet_conv2d_plan with
 * flag 8192) does not answer family 9 -- no tile, the 128 x 128 tile, K % 16 != 0, more than 32 taps -- runs as without
 * `w_planes` and reads `w`; a call that does answer 9 reads only the pack. */
long vrnet_conv_planes_bytes(int J, int K);
int vrnet_conv_planes_pack_f32(const long* table, int nentries, long total_blocks, void* stream);

/* ---- Plane GEMMs (round 4, csrc/pgemm.hip): the 1x1 convolutions of the ClusterBlocks (fc1 | fc_v, the Cluster's proj, the
 * Mlp's fc1 / fc2: backbone/fusion/vr_coc.py:145-147, 187, 205-207, neck variant backbone/vision/context_cluster.py:211-216)
 * and their data gradients on operands that ALREADY ARE bf16 planes in HBM, so that the GEMM main loop is LDS-DMA +
 * ds_read_b128 + MFMA with no VALU work on operands.
 *   plane tensor: element (r, k) of plane q at base[q * plane + r * ld + k], bf16; ld and plane multiples of 8, base 16-byte
 *   aligned.  np = 3: an fp32 tensor t split EXACTLY, t = p0 + p1 + p2 (round-to-nearest-even at each step; written by the
 *   producing kernel's epilogue, by vrnet_planes_split_f32 for the weights of a step, or by vrnet_planes_from_f32); products
 *   a0b0 + a0b1 + a1b0 + a0b2 + a2b0 + a1b1 accumulated in fp32 on v_mfma_f32_32x32x16_bf16 -- the x6 scheme of precision 2
 *   with the same error bound.  np = 1: bf16 tensors, one product (compute_dtype "bf16": bf16 activations in HBM).
 * vrnet_gemm_planes_f32: y[M][N] = epilogue(A[M][K] . B[N][K]^T); forward: A = activations, B = w[Cout][Cin]; data gradient:
 * A = dy, B = transposed weights with the layer scale folded in.  Epilogue as vrnet_conv2d_f32: bias, aux (x gelu'(aux)),
 * ypre, act (0 / 1 ReLU / 2 GELU), res (+ res_scale), accumulate, stats (fp64 (sum, sumsq) per 32 x 32 tile; stats_hw = rows
 * per sample), colstats.  The result goes to `y` (fp32; may be NULL) and / or to `yp` as planes (yp_np 3 or 1).
 * K % 32 == 0, N % 4 == 0; ask vrnet_gemm_planes_ok for shapes with too few 128 x 128 tiles.  half_side: bit 0 = `ypre` is a bf16
 * tensor (stored rounded), bit 1 = `aux` is a bf16 tensor (row strides in elements): the Mlp's pre-activation u in bf16 mode.
 * Kernel families 10 (np 3), 11 (np 1). */
int vrnet_gemm_planes_ok(long rows, int cols, int K);
int vrnet_gemm_planes_f32(const void* a, long lda, long a_plane, const void* b, long ldb, long b_plane, int np, long M, int N,
                          int K, const float* bias, float* y, long ldy, void* yp, long ldyp, long yp_plane, int yp_np, int act,
                          float* ypre, long ldypre, const float* res, long ldres, const float* res_scale, const float* aux,
                          long ldaux, int accumulate, double* stats, long stats_hw, const vrnet_conv_colstats* colstats,
                          int half_side, void* stream);
/* fp32 matrices -> planes in one launch for a table of matrices (the weights of a step).  Entry (10 longs): source address,
 * rows R, contraction K, source element strides (row, k), address of a scale per k or 0 (the layer scale of a data-gradient
 * pack), destination address, destination row stride, destination plane stride, first block (running sum of
 * vrnet_planes_split_blocks). */
long vrnet_planes_split_blocks(long R, long K);
int vrnet_planes_split_f32(const long* table, int nentries, long total_blocks, int np, void* stream);
/* One row-major fp32 matrix (R rows of K values, row stride lds) -> planes: conversion pass for an activation tensor whose
 * producer has no plane output. */
int vrnet_planes_from_f32(const float* src, long lds, long R, long K, void* dst, long ld, long plane, int np, void* stream);
/* Weight (+ bias, + layer-scale) gradient of a 1x1 conv on plane operands: dw[Cout][Cin] (+)= row_scale[n] * sum_m dy[m][n] *
 * x[m][c]; dbias, row_scale, accumulate, (w, bias, dls) as vrnet_conv2d_wgrad_f32 (autograd of vr_coc.py:145-147, 187, 205-207).
 * x: planes of the conv's input (M rows of Cin), dy: planes of the output gradient (M rows of Cout), same np.  The fragments
 * -- 8 consecutive rows of one column -- are read with ds_read_b64_tr_b16; no operand is split in the kernel (the in-kernel
 * split weight gradient splits four fragments per 24 MFMAs).  Channel counts multiples of 8.  Families 12 (np 3) / 13 (np 1). */
/* Optional bf16-plane output of a producing kernel: the tensor it hands to a plane GEMM.  plane q of element (row, c) at
 * p[q * plane + row * ld + c]; np = 3 exact split, 1 rounded to bf16. */
typedef struct vrnet_planes_out {
  void* p;
  long ld, plane;
  int np;
} vrnet_planes_out;
/* Producers with a plane output (same arguments as the functions they extend, plus the planes):
 *   vrnet_gn_apply_fwd_planes    GroupNorm(1, C) output (vr_coc.py:264, 268) -- y may be NULL (planes only);
 *   vrnet_gn_apply_bwd_planes    its input gradient: the block's outgoing gradient as the next GEMMs' dy operand;
 *   vrnet_cluster_fwd_planes_f32 the Cluster core's output (vr_coc.py:158-186), forced != 0 = the teacher-forced form; the fp32
 *     `out` may be NULL (planes only); in_bf16 != 0: f and v are bf16 tensors (ld in elements) -- what the reference's
 *     autocast hands its Cluster (train.py:345-350): the fc1 | fc_v GEMM then writes 2 bytes per element and nothing else;
 *   vrnet_cluster_bwd_planes_f32 [df | dv] as ONE plane tensor of 2 E D columns (df first); df / dv may both be NULL (planes
 *     only); in_bf16 != 0: f, v AND dout are bf16 tensors. */
int vrnet_gn_apply_fwd_planes(const float* x, long ldx, const double* pairs, long pairs_per_sample, const float* gamma,
                              const float* beta, float eps, int B, long HW, int C, float* y, long ldy, float* mean_rstd,
                              const vrnet_planes_out* yp, void* stream);
int vrnet_gn_apply_bwd_planes(const float* dy, long lddy, const float* x, long ldx, const float* mean_rstd, const float* gamma,
                              int B, long HW, int C, const float* add, long ldadd, float* out, long ldo, float* dgamma,
                              float* dbeta, int accumulate_params, const vrnet_planes_out* outp, void* workspace,
                              long workspace_bytes, void* stream);
/* Regions of more than 256 points (every backbone stage at 1 024 px, neck p3 at 512 px) run on a kernel that streams the
 * points in chunks; its backward re-read f four times and v three times.  `state` (vrnet_cluster_state_floats(...) floats, 0 for
 * the register-resident region sizes; NULL = not wanted): the forward leaves the region centres, aggregated values and
 * assignment counts there; the backward, given that state and the forward's similarity map `wgt_fwd` (both or neither), starts
 * at its third pass -- f twice, v once, the same bits (outp / dfvp may be NULL in both: no plane copies). */
long vrnet_cluster_state_floats(int B, int H, int W, int E, int fold);
int vrnet_cluster_fwd_planes_f32(const void* f, const void* v, long ld, int in_bf16, const float* alpha, const float* beta,
                                 float* out, long ldo, unsigned char* idx, float* wgt, int B, int H, int W, int E, int D,
                                 int fold, int forced, const vrnet_planes_out* outp, float* state, void* stream);
int vrnet_cluster_bwd_planes_f32(const void* f, const void* v, long ld, int in_bf16, const float* alpha, const float* beta,
                                 const unsigned char* idx, const void* dout, long lddo, float* df, float* dv, long lddf,
                                 float* dalpha, float* dbeta, int accumulate_ab, int B, int H, int W, int E, int D, int fold,
                                 const vrnet_planes_out* dfvp, const float* wgt_fwd, const float* state, void* workspace,
                                 long workspace_bytes, void* stream);
int vrnet_wgrad_planes_ok(long M, int Cin, int Cout);
long vrnet_wgrad_planes_workspace(long M, int Cin, int Cout);
/* What vrnet_wgrad_planes_f32 launches for M contraction rows at np = 3 or 1; a host-only query over the function the launcher
 * itself plans with.  n_tiles x c_tiles tiles of 128 (Cout) x 128 (Cin) channels, `splits` row splits of rows_per_split rows (a
 * multiple of 32; the last split may be shorter), one fp32 slab per split; the grid is 8 * ceil(splits / 8) * n_tiles * c_tiles
 * workgroups.  Returns non-zero on bad arguments. */
int vrnet_wgrad_planes_plan(long M, int Cin, int Cout, int np, int* n_tiles, int* c_tiles, int* splits, int* rows_per_split);
int vrnet_wgrad_planes_f32(const void* x, long ldx, long x_plane, const void* dy, long lddy, long dy_plane, int np, long M, int Cin,
                           int Cout, float* dw, float* dbias, const float* row_scale, int accumulate, const float* w,
                           const float* bias, float* dls, void* workspace, long workspace_bytes, void* stream);

/* Weight (+ bias) gradient of the same convolutions (autograd of nn.Conv2d): dw in OIHW layout
 * [Cout][Cin][kh][kw], dbias[Cout] (NULL = none), both scaled by row_scale[Cout] when given (layer scale).
 * Deterministic split over output pixels into fp32 slabs in `workspace` (size from ..._workspace).
 * ldx < Cin or lddy < Cout is refused ("conv2d_wgrad: row stride smaller than channel count"), as vrnet_conv2d_f32 refuses
 * lda / ldy below the contracted / produced channel count ("conv2d: row stride ..."), whichever kernel would serve the shape.
 * precision 1: dy and x rounded to bf16 while staged, v_mfma_f32_32x32x16_bf16 with transposing LDS reads, fp32
 * accumulate / slabs / bias sums (needs 16-byte rows, Cin, Cout multiples of 4 and > 32).
 * Two-stream launch (dw2 != NULL; workspace with pair = 1): samples [0, B/2) contribute to (dw, dbias, row_scale),
 * samples [B/2, B) to (dw2, dbias2, row_scale2).
 * dls (NULL = none; 1x1 convs): gradient of the layer scale behind this conv (vr_coc.py:266-271, x + ls * conv(h)):
 *   dls[n] (+)= sum_c w[n][c] * dw_raw[n][c] + bias[n] * db_raw[n]  (raw = before row_scale), which equals
 *   sum_m dy[m,n] * conv(h)[m,n] -- so the branch output is neither stored in the forward pass nor re-read. */
long vrnet_conv2d_wgrad_workspace(int B, int OH, int OW, int Cin, int Cout, int kh, int kw, int pair);
/* What vrnet_conv2d_wgrad_f32 launches on its MFMA path (the shapes that the tiny- and narrow-channel kernels, families 4
 * and 5, do not take) for `rows` = B*OH*OW output pixels PER STREAM and taps = kh * kw; a host-only query, taken from the
 * functions the launcher itself dispatches on.  ident: 1x1, stride 1, pad 0; vec: both operands have 16-byte rows (Cin, Cout,
 * ldx, lddy % 4 == 0, aligned bases); has_bias: dbias given; has_dls: dls given (dw and w 16-byte aligned).  out[8]:
 *   0 kernel   0 wgrad_kernel, 1 wgrad_dma_kernel, 2 wgrad_x6_kernel (precision 2: x6, 1: bf16-rounded operands), 3 the bf16
 *              kernel of igemm_bf16.hip.  0 / 1 at precision 2: no tile kernel for the shape, the fp32 path serves it.
 *   1 tile     64064 / 128128 / 128064 / 128032 (rows x columns of dW per workgroup), or the x6 cfg 22 / 21 / 12
 *   2 S        row splits = slabs per stream            3 rows_per_split (the last split may be shorter)
 *   4 xcd_group  1: all tiles of a row split run on one XCD (x6 kernels)
 *   5 reduce   0 wgrad_reduce_kernel<VEC, SL> (with has_dls followed by wgrad_rowdot_kernel), 1 wgrad_reduce_rows_kernel<SL>
 *   6 VEC      7 SL
 * Returns non-zero where vrnet_conv2d_wgrad_f32 refuses the call (precision 1 without a kernel, precision outside 0..2). */
int vrnet_conv2d_wgrad_plan(long rows, int Cin, int Cout, int taps, int ident, int vec, int precision, int has_bias,
                            int has_dls, int* out);
int vrnet_conv2d_wgrad_f32(const float* x, long ldx, const float* dy, long lddy, float* dw, float* dbias,
                           const float* row_scale, int B, int H, int W, int Cin, int OH, int OW, int Cout, int kh,
                           int kw, int stride, int pad, int dil, int accumulate, int precision, float* dw2,
                           float* dbias2, const float* row_scale2, const float* w, const float* bias, float* dls,
                           const float* w2, const float* bias2, float* dls2, void* workspace, long workspace_bytes,
                           void* stream);
int vrnet_pack_weight_f32(const float* w_oihw, float* w_tnc, int Cout, int Cin, int kh, int kw, void* stream);
/* [kh*kw][Cin][Cout] = w_oihw[n][c][t] * kscale[n] (kscale NULL = 1): the data-gradient operand of the bf16 path. */
int vrnet_pack_weight_t_f32(const float* w_oihw, const float* kscale, float* w_tcn, int Cout, int Cin, int kh, int kw,
                            void* stream);

/* ---- fused Mlp: fc1 -> GELU -> fc2 in ONE kernel per direction ---------------------------------------
 * Replaces Mlp.forward (backbone/fusion/vr_coc.py:217-223; neck variant backbone/vision/context_cluster.py) together with
 * the layer-scale residual around it (vr_coc.py:270-271: x + layer_scale_2 * mlp(norm2(x))) and their autograd: the
 * hidden activation (8x / 4x the block width) never makes a round trip through HBM.  Rows are pixels (M = B*H*W),
 * C = block width, HID = hidden width; kernels exist for C in {64, 128}, HID % 32 == 0, HID <= 2560, M % 32 == 0
 * (vrnet_mlp_fused_ok; callers keep the two vrnet_conv2d_f32 launches elsewhere).
 * Weights are consumed as bf16 PLANES in MFMA fragment order, written once per step by vrnet_mlp_pack_f32 from the
 * state_dict tensors w1 = fc1.weight [HID][C], w2 = fc2.weight [C][HID] (1x1 OIHW): precision 2 = three planes per weight,
 * w = p0 + p1 + p2 exactly (round-to-nearest-even splits), and every fp32 product is evaluated as the six bf16 x bf16
 * products p_i q_j with i + j <= 2 (exact in fp32), fp32 accumulate -- the "x6" arithmetic of vrnet_conv2d_f32 precision
 * 2; precision 1 = one plane, operands rounded to bf16.  Activations are split / rounded in registers.  vrnet_mlp_pack_bytes
 * = size of ONE direction's planes.
 * forward:  u = x w1^T + b1 (stored to upre when non-NULL: the backward pass needs it);  y = res + res_scale * (gelu(u) w2^T
 *   + b2)  (exact-erf GELU; res / res_scale / b1 / b2 optional);  stats as in vrnet_conv2d_f32 ([M/32][C/32][2] fp64).
 *   res_scale scales the Mlp's output only on its way onto a residual: given WITHOUT res it is ignored, y = gelu(u) w2^T + b2
 *   (pinned by tests/test_cluster_edges.py).
 * backward: given dy and the stored u:  du = gelu'(u) * ((dy * dy_scale) w2);  dx = du w1;  h = gelu(u) is recomputed.
 *   du and h are written once (operands of the two weight gradients, vrnet_conv2d_wgrad_f32), dx is the data gradient.
 * precision 4 (round 4): precision 1 with the hidden-sized tensors in bf16 -- `upre` (forward: written, backward: read), `h` and
 *   `du` are then addresses of bf16 elements (row strides in elements): half the bytes of the kernels' dominant traffic; h and
 *   du are what vrnet_wgrad_planes_f32 (np = 1) takes as they are.  The forward output does not change (u is rounded only on
 *   its way to memory); the backward pass evaluates gelu / gelu' at the rounded u.  Packs: those of precision 1.
 * x6 on non-finite / tiny operands (both here and in vrnet_conv2d_f32 precision 2): an operand of +-Inf splits into
 *   (Inf, NaN, NaN), so an Inf in the data yields NaN where fp32 arithmetic yields Inf; NaN stays NaN.  The low planes of an
 *   operand below 2^-110 in magnitude fall into the bf16 denormal range, which the matrix pipe flushes: such operands
 *   carry 8-16 instead of 24 significant bits (the product is below 2^-110 |other operand|).
 * x6 error: the three dropped products are each below 2^-21 |ab| (typically 2^-23); the activation operands are split by
 *   truncation in the kernels, so their share is a bias towards zero rather than zero-mean rounding; the pre-split
 *   weights round to nearest even.  Against an fp64 matmul the results are as close as the fp32 MFMA's
 *   (profiles/r03_x6_vs_fp32_mfma_gemm_probe.txt; tests hold 2e-5 of the output scale). */
int vrnet_mlp_fused_ok(int C, int HID, long M);
long vrnet_mlp_pack_bytes(int C, int HID, int precision);
int vrnet_mlp_pack_f32(const float* w1, const float* w2, int C, int HID, int precision, void* pack_fwd, void* pack_bwd,
                       void* stream);
int vrnet_mlp_fwd_f32(const float* x, long ldx, const void* pack_fwd, const float* b1, const float* b2, const float* res,
                      long ldres, const float* res_scale, float* y, long ldy, float* upre, long ldu, double* stats, long M,
                      int C, int HID, int precision, void* stream);
int vrnet_mlp_bwd_f32(const float* dy, long lddy, const float* dy_scale, const void* pack_bwd, const float* upre, long ldu,
                      float* h, long ldh, float* du, long lddu, float* dx, long lddx, long M, int C, int HID, int precision,
                      void* stream);
/* The backward kernel WITHOUT a stored pre-activation (round 5, ABI 9): u = W1 x + b1 is recomputed chunk by chunk from the forward's
 * input rows x (the normalised block input: fp32, row stride ldx) against pack = vrnet_mlp_pack_rc_f32's per-chunk
 * [fc2^T | fc1^T | fc1] planes; the forward (vrnet_mlp_fwd_f32 with upre = NULL) then writes no hidden-sized tensor and the
 * backward reads one less.  precision 2: fp32 h / du, bit-identical to vrnet_mlp_bwd_f32 on the stored u; 4: bf16-rounded
 * operands, bf16 h / du.  Hidden widths up to 1024 (C = 64) / 1536 (C = 128): vrnet_mlp_rc_ok (ABI 10) is the predicate the
 * pack and the kernel check, for callers that decide in the FORWARD pass whether to store u. */
int vrnet_mlp_rc_ok(int C, int HID, long M);
long vrnet_mlp_pack_rc_bytes(int C, int HID, int precision);
int vrnet_mlp_pack_rc_f32(const float* w1, const float* w2, int C, int HID, int precision, void* pack, void* stream);
int vrnet_mlp_bwd_rc_f32(const float* dy, long lddy, const float* dy_scale, const void* pack, const float* x, long ldx,
                         const float* b1, float* h, long ldh, float* du, long lddu, float* dx, long lddx, long M, int C, int HID,
                         int precision, void* stream);

/* ---- per-(sample, channel) moments in fp64 ---------------------------------------------------------
 * out[b][c] = { sum_p x, sum_p x*x }                    (x2 == NULL)
 *           = { sum_p xm, sum_p xm*x2 }, xm = mask>0 ? x : 0   (x2 given; mask optional)
 * Feeds GroupNorm(1,C) (vr_coc.py:105-111), train-mode BatchNorm2d (normal_conv.py:45; vr_coc.py:310,329),
 * ShuffleAttention's avg-pool / per-channel GroupNorm (shuffle_attention.py:57,62), ECA's avg-pool (eca.py:17),
 * ASPP's global mean (coc_fpn_dual.py:91-92) and the layer-scale / bias / norm-parameter gradients. */
long vrnet_moments_workspace(int B, long HW, int C);
int vrnet_moments_f32(const float* x, long ldx, const float* x2, long ldx2, const float* mask, long ldm, int B,
                      long HW, int C, double* out, void* workspace, long workspace_bytes, void* stream);

/* out = pre(A*(x1 - S1) + D1) + E*(x2 - S2) + D2; pre: 0 none, 1 ReLU, 2 keep where masky > 0.  Coefficients are
 * indexed [b*coef_bstride + c] (0 = per channel, C = per sample and channel); NULL A/E = 1, NULL D1/D2/S1/S2 = 0,
 * NULL x1/x2 = term absent.  The shifts keep normalisation in torch's (x - mean) * scale order: the algebraically
 * equal A*x + (beta - mean*A) cancels catastrophically when |mean| >> std.  The apply step of GroupNorm / BatchNorm(+ReLU, + residual) forward AND backward,
 * ECA gating (eca.py:22), global-feature broadcast (coc_fpn_dual.py:96).
 * Every tensor that is read or written (out; x1, x2 if given; masky when pre == 2; add if given) needs a row stride >= C:
 * a smaller one is refused ("affine: row stride smaller than channel count").  16-byte kernel when C % 4 == 0 and all of
 * them have strides % 4 == 0 and 16-byte aligned bases, one float per access otherwise. */
int vrnet_affine_f32(const float* x1, long ld1, const float* A, const float* D1, const float* S1, int pre,
                     const float* masky, long ldm, const float* x2, long ld2, const float* E, const float* D2,
                     const float* S2, long coef_bstride, float* out, long ldo, int B, long HW, int C, int accumulate,
                     const float* add, long ldadd, void* stream);   /* add: out-of-place addend (out = ... + add) */

/* Coefficient kernels: moments -> affine coefficients, saved statistics, parameter gradients. */
/* GroupNorm(1,C), eps 1e-5 (vr_coc.py:105-111): y = A*(x - S) + D with A,D,S [B][C]; mean_rstd [B][2]. */
int vrnet_gn_coef_fwd(const double* mom, const float* gamma, const float* beta, float eps, int B, long HW, int C,
                      float* A, float* D, float* S, float* mean_rstd, void* stream);
/* The same coefficients from (sum, sum of squares) pairs, pairs_per_sample consecutive pairs per sample (the `stats`
 * output of vrnet_conv2d_f32).  gamma2 / beta2 (NULL = none): two-stream launch, samples [B/2, B) use them. */
int vrnet_gn_coef_from_pairs(const double* pairs, long pairs_per_sample, const float* gamma, const float* beta, float eps,
                             int B, long HW, int C, float* A, float* D, float* S, float* mean_rstd,
                             const float* gamma2, const float* beta2, void* stream);
/* vrnet_moments_f32 + vrnet_gn_coef_fwd in two launches (the per-sample totals come straight from the chunk partials);
 * workspace as vrnet_moments_workspace. */
int vrnet_gn_stats_fwd(const float* x, long ldx, const float* gamma, const float* beta, float eps, int B, long HW, int C,
                       float* A, float* D, float* S, float* mean_rstd, const float* gamma2, const float* beta2,
                       void* workspace, long workspace_bytes, void* stream);
/* mom2 = moments(dy, x2 = x): dx = A*dy + E*(x - S) + D with A,E,D,S [B][C]; dgamma, dbeta [C].
 * gamma2 / dgamma2 / dbeta2 (NULL = none): two-stream launch, samples [B/2, B) belong to the second norm. */
int vrnet_gn_coef_bwd(const double* mom2, const float* mean_rstd, const float* gamma, int B, long HW, int C,
                      float* A, float* E, float* D, float* S, float* dgamma, float* dbeta, int accumulate,
                      const float* gamma2, float* dgamma2, float* dbeta2, void* stream);

/* GroupNorm(1, C) with the coefficient step INSIDE the apply kernels (vr_coc.py:105-111, 264-271: norm1 / norm2 of every
 * ClusterBlock sit on the critical chain of the step, so launches count).  C % 4 == 0, 16-byte rows.
 * vrnet_gn_apply_fwd: y = GN(x) in ONE launch from the (sum, sumsq) tile pairs the producing conv / fused Mlp left
 *   (`stats` of vrnet_conv2d_f32 / vrnet_mlp_fwd_f32: pairs_per_sample consecutive fp64 pairs per sample); every workgroup
 *   re-adds its sample's pairs in the same fixed order; mean_rstd [B][2] is written for the backward pass.
 * vrnet_gn_apply_bwd: TWO launches -- the moments kernel over (dy, dy * x), which also leaves gamma-weighted totals per
 *   chunk, then one kernel that finishes each sample's coefficients from those totals, writes out = dx (+ add) and, in an
 *   extra row of its grid, the parameter gradients dgamma / dbeta (+= when accumulate_params). */
int vrnet_gn_apply_fwd(const float* x, long ldx, const double* pairs, long pairs_per_sample, const float* gamma,
                       const float* beta, float eps, int B, long HW, int C, float* y, long ldy, float* mean_rstd, void* stream);
long vrnet_gn_bwd_workspace(int B, long HW, int C);
/* The apply step of vrnet_gn_apply_bwd alone (ONE launch) when the conv that produced dy already left its moments
 * (vrnet_conv_colstats with x2 = the GroupNorm input, gamma = the GroupNorm weight): partial [B*HW/32][C][2],
 * tile_totals [B*HW/32][ceil(C/32)][2]; HW % 32 == 0. */
int vrnet_gn_apply_bwd_from_partials(const float* dy, long lddy, const float* x, long ldx, const double* partial,
                                     const double* tile_totals, const float* mean_rstd, const float* gamma, int B, long HW,
                                     int C, const float* add, long ldadd, float* out, long ldo, float* dgamma, float* dbeta,
                                     int accumulate_params, void* stream);
/* Train-mode BatchNorm2d coefficients (y = A * (z - S) + D), running statistics and mean / rstd from the column partials
 * the producing conv left (vrnet_conv_colstats, x2 = NULL; partial [B*HW/32][C][2]; HW % 32 == 0): BaseConv's conv -> BN
 * (normal_conv.py:45-49) without a statistics pass over z. */
int vrnet_bn_coef_fwd_from_partials(const double* partial, const float* gamma, const float* beta, float eps, float momentum,
                                    float* running_mean, float* running_var, long long* num_batches_tracked, int B, long HW,
                                    int C, float* A, float* D, float* S, float* mean_rstd, void* stream);
int vrnet_gn_apply_bwd(const float* dy, long lddy, const float* x, long ldx, const float* mean_rstd, const float* gamma, int B,
                       long HW, int C, const float* add, long ldadd, float* out, long ldo, float* dgamma, float* dbeta,
                       int accumulate_params, void* workspace, long workspace_bytes, void* stream);
/* nn.BatchNorm2d: batch statistics + running-stat update (unbiased var, momentum) + num_batches_tracked += 1
 * when training, running statistics otherwise.  y = A*(z - S) + D with A,D,S [C]; mean_rstd [C][2]. */
int vrnet_bn_coef_fwd(const double* mom, const float* gamma, const float* beta, float eps, float momentum,
                      float* running_mean, float* running_var, long long* num_batches_tracked, int training, int B,
                      long HW, int C, float* A, float* D, float* S, float* mean_rstd, void* stream);
/* Train-mode BatchNorm in two launches instead of three: vrnet_moments_f32's first kernel over z, then ONE kernel that
 * adds the chunk partials per channel, updates the running statistics and writes the coefficients (no [B][C][2] table, no
 * separate reduce launch).  workspace as vrnet_moments_workspace.  The backward counterpart does the same for
 * moments(dy, x2 = z, mask). */
int vrnet_bn_stats_fwd(const float* x, long ldx, const float* gamma, const float* beta, float eps, float momentum,
                       float* running_mean, float* running_var, long long* num_batches_tracked, int B, long HW, int C,
                       float* A, float* D, float* S, float* mean_rstd, void* workspace, long workspace_bytes, void* stream);
int vrnet_bn_stats_bwd(const float* dy, long lddy, const float* z, long ldz, const float* mask, long ldm,
                       const float* mean_rstd, const float* gamma, int training, int B, long HW, int C, float* A, float* E,
                       float* D, float* S, float* dgamma, float* dbeta, int accumulate, void* workspace,
                       long workspace_bytes, void* stream);
/* BatchNorm backward of y = ReLU(BN(z)) WITHOUT reading y (round 4; BaseConv, normal_conv.py:36-49): the mask [y > 0] is
 * recomputed from z with the forward coefficients, fwd_A (z - fwd_S) + fwd_D evaluated as the single fused multiply-add
 * the forward apply used (same bits), which removes one of three tensor reads from the moments pass and from the apply
 * pass.  vrnet_bn_stats_bwd_zmask: as vrnet_bn_stats_bwd;  vrnet_bn_apply_bwd_zmask: dz = [mask] (A dy) + E (z - S) + D. */
int vrnet_bn_stats_bwd_zmask(const float* dy, long lddy, const float* z, long ldz, const float* fwd_A, const float* fwd_D,
                             const float* fwd_S, const float* mean_rstd, const float* gamma, int training, int B, long HW,
                             int C, float* A, float* E, float* D, float* S, float* dgamma, float* dbeta, int accumulate,
                             void* workspace, long workspace_bytes, void* stream);
int vrnet_bn_apply_bwd_zmask(const float* dy, long lddy, const float* z, long ldz, const float* fwd_A, const float* fwd_D,
                             const float* fwd_S, const float* A, const float* E, const float* D, const float* S, float* dz,
                             long lddz, int B, long HW, int C, void* stream);
/* mom2 = moments(dy, x2 = z, mask = relu output): dz = A*dy' + E*(z - S) + D with A,E,D,S [C]. */
int vrnet_bn_coef_bwd(const double* mom2, const float* mean_rstd, const float* gamma, int training, int B, long HW,
                      int C, float* A, float* E, float* D, float* S, float* dgamma, float* dbeta, int accumulate,
                      void* stream);
/* eca_block (backbone/attention_modules/eca.py:16-22): gate[b][c] = sigmoid(conv1d_k(mean_hw x)). */
int vrnet_eca_coef_fwd(const double* mom, const float* wk, int k, int B, long HW, int C, float* gate, void* stream);
/* mom2 = moments(dy, x2 = x): dx = gate*dy + F[b][c]; dwk [k].  F or dwk may be NULL (ABI 9): only the other half is computed
 * (dwk, the Conv1d weight gradient, is needed by nothing on the backward chain: a caller may issue it on a side stream). */
int vrnet_eca_coef_bwd(const double* mom2, const double* mom, const float* gate, const float* wk, int k, int B,
                       long HW, int C, float* F, float* dwk, int accumulate, void* stream);
/* Layer scale x + ls*o (vr_coc.py:266-271), mom2 = moments(dx, x2 = o): dls[c] = sum dx*o; dbias = ls * sum dx.
 * pair = 1: two-stream launch, samples [B/2, B) reduce into (dls2, dbias2) with ls2. */
int vrnet_ls_coef_bwd(const double* mom2, const float* ls, int B, int C, float* dls, float* dbias, int accumulate,
                      int pair, const float* ls2, float* dls2, float* dbias2, void* stream);
int vrnet_moments_to_float(const double* mom, float* out, long n, double scale, int which, void* stream);

/* ---- non-overlapping patch embedding as gather + GEMM ---------------------------------------------------
 * PointRecuder(patch_size=4, stride=4) over cat([x, fea_pos]) (backbone/fusion/vr_coc.py:83-102, 424-430, 583-586):
 * P[b,oy,ox,(ky*k+kx)*(C+CP)+c] = cat(x, pos)[b, oy*k+ky, ox*k+kx, c]  (pos: (H,W,CP) buffer shared by the batch,
 * NULL when CP == 0); the projection is then vrnet_conv2d_f32 with a 1x1 kernel over k*k*(C+CP) channels and the
 * weight in OHWI order (vrnet_weight_ohwi_f32 dir 0).  patch_scatter is the adjoint w.r.t. x;
 * vrnet_weight_ohwi_f32 dir 1 maps the OHWI weight gradient back to the parameter's OIHW layout. */
int vrnet_patch_gather_f32(const float* x, long ldx, const float* pos, float* out, int B, int H, int W, int C, int CP,
                           int k, void* stream);
int vrnet_patch_scatter_f32(const float* dp, float* dx, long lddx, int B, int H, int W, int C, int CP, int k,
                            int accumulate, void* stream);
int vrnet_weight_ohwi_f32(const float* src, float* dst, int Cout, int Cin, int kh, int kw, int dir, int accumulate,
                          void* stream);

/* ---- layout ---------------------------------------------------------------------------------------- */
/* dst[r*ldd + c*dcs] (+)= src[r*lds + c*scs]: torch.cat + shuffle_channels(groups=2) (vr_coc.py:70-80,
 * coc_fpn_dual.py:120-130) written straight into the consumer's buffer, and their adjoints. */
/* torch.cat([a, b], 1) (+ shuffle_channels(groups = 2) when interleave: channel 2 j = a_j, 2 j + 1 = b_j; vr_coc.py:70-80,
 * coc_fpn_dual.py:120-130) in ONE launch -- dir 0: cat (rows, Ca + Cb) = a | b -- and its adjoint -- dir 1: a (+)= its
 * channels of cat, b (+)= its channels (accumulate_a / accumulate_b; a or b NULL: that half is skipped). */
int vrnet_cat2_f32(float* a, long lda, int Ca, float* b, long ldb, int Cb, float* cat, long ldc, long rows, int interleave,
                   int dir, int accumulate_a, int accumulate_b, void* stream);
int vrnet_copy_channels_f32(const float* src, long lds, int scs, float* dst, long ldd, int dcs, long rows, int C,
                            int accumulate, void* stream);
int vrnet_nchw_to_nhwc_f32(const float* src, float* dst, long ldd, int B, int C, long HW, void* stream);
int vrnet_nhwc_to_nchw_f32(const float* src, long lds, float* dst, int B, int C, long HW, int accumulate, void* stream);
int vrnet_add_f32(float* dst, const float* src, long n, void* stream);
int vrnet_fill_f32(float* dst, float value, long n, void* stream);

/* ---- Context-Cluster core ---------------------------------------------------------------------------
 * Replaces Cluster.forward between fc1/fc_v and fc2 (vr_coc.py:158-190; pairwise_cos_sim :114-125) and its
 * autograd.  f, v, out: (B,H,W,E*D) NHWC; head e owns channels [e*D,(e+1)*D); regions are the fold x fold
 * tiles of the map (fold = 1: the whole map), D % 4 == 0, D <= 32.  Regions of <= 256 points (every backbone
 * stage at 512 px) stay in registers; larger ones (neck p3 at 512 px, everything at 1024 px) use a streaming kernel.
 * idx: (B,H,W,E) u8 hard assignment (first maximum, as torch.max(dim)); wgt: (B,H,W,E) similarity of the
 * assigned centre (optional for regions of <= 256 points, required above).  alpha, beta: device scalars (sim_alpha, sim_beta, :148-149).
 * alpha2 / beta2 (NULL = none): two-stream launch, samples [B/2, B) belong to a second Cluster module.
 * There are 16-byte kernels only: ld, ldo (backward: lddo, lddf) % 4 == 0 and 16-byte aligned f, v, out (dout, df, dv), else
 * the call is refused ("cluster_fwd: rows must be 16-byte aligned" / "cluster_bwd: ..."). */
int vrnet_cluster_fwd_f32(const float* f, const float* v, long ld, const float* alpha, const float* beta,
                          float* out, long ldo, unsigned char* idx, float* wgt, int B, int H, int W, int E, int D,
                          int fold, const float* alpha2, const float* beta2, void* stream);
/* the same forward with the assignment GIVEN (idx is read): parity work, where the numerically tied points of the arg-max
 * (vr_coc.py:173-176) must be decided the same way on both sides of a comparison */
int vrnet_cluster_fwd_forced_f32(const float* f, const float* v, long ld, const float* alpha, const float* beta,
                                 float* out, long ldo, const unsigned char* idx, float* wgt, int B, int H, int W, int E, int D,
                                 int fold, const float* alpha2, const float* beta2, void* stream);
/* What a launch on regions of N = (H / fold) (W / fold) points in blocks = B * E * fold^2 workgroups runs (host only; ABI 11;
 * bwd != 0: the backward): *T threads per workgroup and *npt points per lane group of the register kernel, or *T = 0, *npt = 0:
 * the streaming kernel.  Answered by the function the launchers dispatch on; an error code where they would refuse (N, blocks). */
int vrnet_cluster_plan(int N, long blocks, int bwd, int* T, int* npt);
long vrnet_cluster_bwd_workspace(int B, int E, int fold);                          /* regions of <= 256 points */
long vrnet_cluster_bwd_workspace2(int B, int H, int W, int E, int fold);            /* any region size */
/* Recomputes the forward from f, v with the saved assignment idx; df, dv share row stride lddf.
 * dalpha == dbeta == NULL (single-stream launches, also of vrnet_cluster_bwd_planes_f32; ABI 9): the per-workgroup (d alpha,
 * d beta) partials stay in the first 2 * B * E * fold^2 floats of `workspace` and no finishing launch runs -- the caller keeps
 * that workspace to itself and reduces a whole section's modules later with ONE vrnet_cluster_ab_reduce_multi. */
int vrnet_cluster_bwd_f32(const float* f, const float* v, long ld, const float* alpha, const float* beta,
                          const unsigned char* idx, const float* dout, long lddo, float* df, float* dv, long lddf,
                          float* dalpha, float* dbeta, int accumulate_ab, int B, int H, int W, int E, int D,
                          int fold, const float* alpha2, const float* beta2, float* dalpha2, float* dbeta2,
                          void* workspace, long workspace_bytes, void* stream);

/* (d alpha, d beta) of n Cluster modules (vr_coc.py:148-149: sim_alpha, sim_beta are shared by all regions and heads of a
 * module) from the partials their backward launches left (above): host arrays of n workspaces, their B * E * fold^2, the
 * gradient scalars (device) and accumulate flags; one launch per 32 modules. */
int vrnet_cluster_ab_reduce_multi(int n, const void* const* partial, const long* blocks, float* const* dalpha,
                                  float* const* dbeta, const int* accumulate, void* stream);

/* ---- depthwise 3x3, stride 1, pad 1 (DWConv.dconv, normal_conv.py:26-27; head towers decouplehead.py:23-34)
 * w: [C][3][3] (the OIHW tensor of a groups=C conv).  flip = 1 gives the input gradient.  ldx, ldy >= C, else the call is
 * refused ("dwconv3x3: row stride smaller than channel count"). */
int vrnet_dwconv3x3_f32(const float* x, long ldx, const float* w, float* y, long ldy, int B, int H, int W, int C,
                        int flip, int accumulate, void* stream);
long vrnet_dwconv3x3_wgrad_workspace(int B, int H, int W, int C);
int vrnet_dwconv3x3_wgrad_f32(const float* x, long ldx, const float* dy, long lddy, float* dw, int B, int H, int W,
                              int C, int accumulate, void* workspace, long workspace_bytes, void* stream);

/* ---- nn.Upsample(scale, 'bilinear', align_corners=True) (coc_fpn_dual.py:21) and its adjoint (gather form).
 * out_nchw / dy_nchw: the high-resolution side is a contiguous (B,C,OH,OW) tensor (the seg logits). */
int vrnet_upsample_bilinear_f32(const float* x, long ldx, float* y, long ldy, int B, int H, int W, int C, int scale,
                                int out_nchw, void* stream);
/* The same gather from the PRE-normalisation map z of CoCUpsample's 1x1 BaseConv (coc_fpn_dual.py:15-26): every tap is
 * ReLU(A (z - S) + D) evaluated on the fly (A, D, S per channel: the BatchNorm coefficients), so the low-resolution activation
 * is never stored.  Bit-identical to vrnet_affine_f32 (pre = 1) + vrnet_upsample_bilinear_f32. */
int vrnet_bn_relu_upsample_bilinear_f32(const float* z, long ldz, const float* A, const float* D, const float* S, float* y,
                                        long ldy, int B, int H, int W, int C, int scale, int out_nchw, void* stream);
int vrnet_upsample_bilinear_bwd_f32(const float* dy, long lddy, int dy_nchw, float* dx, long lddx, int B, int H, int W,
                                    int C, int scale, int accumulate, void* stream);
/* ---- the neck's up-path levels in one gather (csrc/spatial.hip) -- added within ABI 11: new symbols only.
 * vrnet_bn_relu_upsample_cat_f32, coc_fpn_dual.py:193-221: cat (B, sH, sW, C + Cs; row stride ldc) = torch.cat of the map
 *   vrnet_bn_relu_upsample_bilinear_f32 would write (A == D == S == NULL: of vrnet_upsample_bilinear_f32) and skip (B, sH, sW, Cs;
 *   row stride lds): [up | skip] if up_first, else [skip | up]; interleave (C == Cs): + the 2-group channel shuffle (column 2 j =
 *   first half's channel j, 2 j + 1 = second half's), the order of vrnet_cat2_f32.  The interpolated map is never stored; cat has
 *   the bits of the two calls.  Needs vrnet_up_cat_ok (C % 4 == Cs % 4 == 0, row strides % 4 == 0) and 16-byte aligned bases.
 *   stats 0: none.  stats 1: out (B, C + Cs, 2) fp64 = per-(sample, channel) (sum, sum of squares) of cat with the bits of
 *   vrnet_moments_f32 on it; workspace: vrnet_moments_workspace(B, sH sW, C + Cs).  stats 2: out (B, per, 2) fp64 = per-sample
 *   (sum, sum of squares) pairs, per = vrnet_up_cat_pairs(B, sH sW, C + Cs), the `pairs` of vrnet_gn_apply_fwd.  Fixed
 *   summation order, no atomics.
 * vrnet_upsample_bilinear_bwd_cat_f32: vrnet_upsample_bilinear_bwd_f32 reading its NHWC dy in place from the gradient of such a
 *   concatenation (row stride lddy): channel j at column coff + cstride j (cstride 1, or 2 with coff 0 / 1 for the shuffle). */
int vrnet_up_cat_ok(int C, int Cs, long ldz, long lds, long ldc, int interleave);
long vrnet_up_cat_pairs(int B, long HW, int Ct);
int vrnet_bn_relu_upsample_cat_f32(const float* z, long ldz, const float* A, const float* D, const float* S, const float* skip,
                                   long lds, float* cat, long ldc, int B, int H, int W, int C, int Cs, int scale, int up_first,
                                   int interleave, int stats, double* out, void* workspace, long workspace_bytes, void* stream);
int vrnet_upsample_bilinear_bwd_cat_f32(const float* dy, long lddy, int coff, int cstride, float* dx, long lddx, int B, int H,
                                        int W, int C, int scale, int accumulate, void* stream);

/* ---- ImageEnhanceByRadar gain (vr_coc.py:312-316) with data_normal (:59-67): batch-global min/max of the
 * ReLU'd radar projection p (contiguous, n elements), out = (1 + (p-min)/(max-min)) * x, and the backward
 * including the gradient through min and max (ties share it evenly, as torch's min()/max() backward). */
long vrnet_reduce_workspace(void);
int vrnet_minmax_f32(const float* p, long n, float* mm /* [2] */, void* workspace, long workspace_bytes, void* stream);
int vrnet_enhance_mul_f32(const float* p, const float* x, const float* mm, float* out, long n, void* stream);
/* vrnet_minmax_f32 + vrnet_enhance_mul_f32 in two launches instead of three (the final min / max step runs inside the apply
 * kernel); mm receives (min, max) for vrnet_enhance_bwd_f32.  workspace: vrnet_reduce_workspace() bytes.  (ABI 9) */
int vrnet_enhance_fwd_f32(const float* p, const float* x, float* mm, float* out, long n, void* workspace, long workspace_bytes,
                          void* stream);

/* ---- fused passes of the fusion blocks (csrc/fusion.hip, ABI 9): an elementwise pass that also leaves the partial sums the NEXT
 * reduction needs (contiguous NHWC tensors of n elements, row stride == C, C % 4 == 0, C <= 1024, 16-byte aligned).
 * vrnet_fusion_chunks(n, C): workgroups = entries of the column partials (0: shape not supported): colpart [chunks][C][2] fp64;
 * vrnet_fusion_fold_chunks(n, C): entries of mmpart [.][2] fp32 and sums4 [.][4] fp64.
 *   vrnet_bn_relu_minmax_f32     p = ReLU(A (z - S) + D) + the (min, max) partials of p         (vr_coc.py:308 + :59-67)
 *   vrnet_enhance_stats_f32      t = (1 + data_normal(p)) x + column (sum, sumsq) of t; mm <- (min, max)      (:314-315)
 *   vrnet_bn_relu_res_stats_f32  s = ReLU(A (z - S) + D) + res + column (sum, sumsq) of s                      (:355-357)
 *   vrnet_bn_bwd_enhance_f32     dt = A g + E (t - S) + D (BatchNorm backward apply) + the four sums of the gain's backward
 *   vrnet_enhance_bwd_stats_f32  dx (+)=, dp of the gain + column (sum dp', sum dp' z), dp' = dp [fA (z - fS) + fD > 0]
 * vrnet_bn_coef_{fwd,bwd}_from_chunks: the BatchNorm coefficient steps (vrnet_bn_coef_fwd_from_partials / the second half of
 * vrnet_bn_stats_bwd) from such column partials; count = values per channel (B * HW). */
int vrnet_fusion_chunks(long n, int C);
int vrnet_fusion_fold_chunks(long n, int C);      /* entries of mmpart / sums4 (folded again by every workgroup of the next kernel) */
int vrnet_bn_relu_minmax_f32(const float* z, const float* A, const float* D, const float* S, float* p, long n, int C, float* mmpart,
                             void* stream);
int vrnet_bn_relu_res_stats_f32(const float* z, const float* A, const float* D, const float* S, const float* res, float* s, long n,
                                int C, double* colpart, void* stream);
int vrnet_enhance_stats_f32(const float* p, const float* x, const float* mmpart, int nmm, float* mm, float* t, long n, int C,
                            double* colpart, void* stream);
int vrnet_bn_bwd_enhance_f32(const float* g, const float* t, const float* A, const float* E, const float* D, const float* S,
                             const float* x, const float* p, const float* mm, float* dt, long n, int C, double* sums4, void* stream);
int vrnet_enhance_bwd_stats_f32(const float* dt, const float* x, const float* p, const float* mm, const double* sums4, int nsums,
                                const float* z, const float* fA, const float* fD, const float* fS, float* dx, float* dp, long n, int C,
                                int accumulate_dx, double* colpart, void* stream);
/* ds = A g + E (s - S) + D (backward apply of a BatchNorm without ReLU) + column (sum ds', sum ds' z), ds' = ds [fA (z - fS) + fD > 0]:
 * the moments of the BatchNorm + ReLU in front of it (vr_coc.py:355-357 backwards) */
int vrnet_bn_bwd_next_stats_f32(const float* g, const float* s, const float* A, const float* E, const float* D, const float* S,
                                const float* z, const float* fA, const float* fD, const float* fS, float* ds, long n, int C,
                                double* colpart, void* stream);
int vrnet_bn_coef_fwd_from_chunks(const double* partial, int nchunks, long count, const float* gamma, const float* beta, float eps,
                                  float momentum, float* running_mean, float* running_var, long long* num_batches_tracked, int C,
                                  float* A, float* D, float* S, float* mean_rstd, void* stream);
int vrnet_bn_coef_bwd_from_chunks(const double* partial, int nchunks, long count, const float* mean_rstd, const float* gamma,
                                  int training, int C, float* A, float* E, float* D, float* S, float* dgamma, float* dbeta,
                                  int accumulate, void* stream);
int vrnet_enhance_bwd_f32(const float* dt, const float* x, const float* p, const float* mm, float* dx, float* dp,
                          long n, int accumulate_dx, void* workspace, long workspace_bytes, void* stream);

/* ---- ShuffleAttention (backbone/attention_modules/shuffle_attention.py:48-72) ---------------------------
 * mom = moments(x).  y[dst(q)] = x[q] * sigmoid(P[b][q]*(x[q] - Mn[b][q]) + Q[b][q]); dst() is the final 2-group channel
 * shuffle; the G-group split and the channel/spatial halves are index arithmetic on q.
 * Parameters: cweight, cbias, sweight, sbias, gn.weight, gn.bias, each [C/(2G)]. */
int vrnet_sa_coef_fwd(const double* mom, const float* cw, const float* cb, const float* sw, const float* sb,
                      const float* gnw, const float* gnb, int B, long HW, int C, int G, float* P, float* Q, float* Mn,
                      void* stream);
int vrnet_sa_apply_f32(const float* x, long ldx, const float* P, const float* Q, const float* Mn, float* y, long ldy,
                       int B, long HW, int C, void* stream);
/* cat = shuffle_channels(cat([ShuffleAttention(x), r], 1), 2) (vr_coc.py:343-349) and mom[b][c] = (sum of cat[b, :, c], 0) for the ECA
 * gate behind it (:350): vrnet_sa_apply_f32 + vrnet_cat2_f32 + the pass of vrnet_moments_f32 as one launch (+ the chunk reduce).
 * x, r: (B, HW, C); cat: (B, HW, 2 C); C % 4 == 0, C <= 512; workspace: vrnet_moments_workspace(B, HW, 2 C).  (ABI 9) */
int vrnet_sa_cat_sums_f32(const float* x, long ldx, const float* P, const float* Q, const float* Mn, const float* r, long ldr,
                          float* cat, long ldc, int B, long HW, int C, double* mom, void* workspace, long workspace_bytes,
                          void* stream);
long vrnet_sa_bwd_workspace(int B, long HW, int C);
int vrnet_sa_bwd_f32(const float* dy, long lddy, const float* x, long ldx, const float* P, const float* Q,
                     const float* Mn, const double* mom, const float* cw, const float* cb, const float* sw, const float* sb,
                     const float* gnw, const float* gnb, float* dx, long lddx, float* dcw, float* dcb, float* dsw,
                     float* dsb, float* dgnw, float* dgnb, float* EF /* [2][B][C] scratch */, int B, long HW, int C,
                     int G, int accumulate_dx, int accumulate_params, void* workspace, long workspace_bytes,
                     void* stream);

/* ---- training-step updates over ALL parameters in one launch ----------------------------------
 * Tensor table (device memory): addrs[k*n + t] = address of role k of tensor t, sizes[t] = element count; the work
 * list (chunk_tensor[c], chunk_index[c]) cuts every tensor into chunks of chunk_elems (multiple of 256) elements.
 * vrnet_mt_sgd_f32   roles {param, grad, momentum_buffer}: torch.optim.SGD(momentum, nesterov) as train.py:468-473
 *                    builds it; weight_decay[t] per tensor (group pg1 only, train.py:472); first_step = buffers unset.
 * vrnet_mt_adam_f32  roles {param, grad, exp_avg, exp_avg_sq}: torch.optim.Adam(betas=(momentum, 0.999)), step from 1.
 * vrnet_mt_ema_f32   roles {ema, model}: ModelEMA.update, nets/yolo_training.py:465-475 (v *= d; v += (1-d)*model). */
int vrnet_mt_sgd_f32(const long long* addrs, const long* sizes, const int* chunk_tensor, const int* chunk_index,
                     const float* weight_decay, int n_tensors, int n_chunks, int chunk_elems, float lr, float momentum,
                     int nesterov, int first_step, void* stream);
int vrnet_mt_adam_f32(const long long* addrs, const long* sizes, const int* chunk_tensor, const int* chunk_index,
                      const float* weight_decay, int n_tensors, int n_chunks, int chunk_elems, float lr, float beta1,
                      float beta2, float eps, int step, void* stream);
int vrnet_mt_ema_f32(const long long* addrs, const long* sizes, const int* chunk_tensor, const int* chunk_index,
                     int n_tensors, int n_chunks, int chunk_elems, float decay, void* stream);
/* roles {dst, src}: dst = src for every tensor of the table in one launch (the concatenated fc1 | fc_v weights of all
 * Cluster modules, vr_coc.py:145-147, so that both 1x1 convs of a block run as one GEMM). */
int vrnet_mt_copy_f32(const long long* addrs, const long* sizes, const int* chunk_tensor, const int* chunk_index,
                      int n_tensors, int n_chunks, int chunk_elems, void* stream);

/* The same three updates with the values that change from step to step read from DEVICE memory, for a captured hipGraph
 * (graph.TrainStep): a graph bakes launch scalars in, and lr (reset every epoch, nets/yolo_training.py:544-548), the EMA
 * decay ramp (yolo_training.py:466-468) and Adam's bias corrections change during a run.  The host writes one 16-byte
 * record per step, in stream order before the graph; momentum, betas, eps and nesterov stay launch constants.  The
 * per-element arithmetic is the scalar forms' own (shared device functions), so for the same values the results are the
 * same bits; vrnet_mt_sgd_dev_f32 is the first_step = 0 form (buffers exist and start at zero).
 * Added within ABI 11: new symbols only, no existing signature, layout or kernel behaviour changed; hip.py binds every
 * declared symbol at import, so a library older than this header fails to load there. */
typedef struct vrnet_step_scalars {
  float lr;             /* learning rate of this step */
  float ema_decay;      /* ModelEMA: decay * (1 - exp(-updates / tau)), rounded to float */
  float adam_bc1;       /* 1 - beta1^step           } as vrnet_adam_bias_correction returns them */
  float adam_bc2_sqrt;  /* sqrt(1 - beta2^step)     } */
} vrnet_step_scalars;
int vrnet_mt_sgd_dev_f32(const long long* addrs, const long* sizes, const int* chunk_tensor, const int* chunk_index,
                         const float* weight_decay, int n_tensors, int n_chunks, int chunk_elems,
                         const vrnet_step_scalars* s, float momentum, int nesterov, void* stream);
int vrnet_mt_adam_dev_f32(const long long* addrs, const long* sizes, const int* chunk_tensor, const int* chunk_index,
                          const float* weight_decay, int n_tensors, int n_chunks, int chunk_elems,
                          const vrnet_step_scalars* s, float beta1, float beta2, float eps, void* stream);
int vrnet_mt_ema_dev_f32(const long long* addrs, const long* sizes, const int* chunk_tensor, const int* chunk_index,
                         int n_tensors, int n_chunks, int chunk_elems, const vrnet_step_scalars* s, void* stream);
/* HOST helper, no launch: the bias corrections vrnet_mt_adam_f32 derives from `step` (>= 1) in double precision and
 * rounds to float -- bc1 = 1 - beta1^step, bc2_sqrt = sqrt(1 - beta2^step); bc1 and bc2_sqrt are HOST pointers. */
int vrnet_adam_bias_correction(float beta1, float beta2, int step, float* bc1, float* bc2_sqrt);

/* ---- box decode ----------------------------------------------------------------------------
 * decode_outputs, utils/utils_bbox.py:32-84: levels[l] = raw head map (B, C = 5+num_classes, hs[l], ws[l]) NCHW (the
 * hot path's det outputs); out (B, sum_l hs*ws, C): [cx/in_w, cy/in_h, w/in_w, h/in_h, sigmoid(obj), sigmoid(cls)...],
 * anchors level-major then row-major, stride_l = input_h / hs[l].  `levels`, `hs`, `ws` are HOST arrays. */
int vrnet_decode_outputs_f32(const float* const* levels, const int* hs, const int* ws, int n_levels, int B, int C,
                             float input_h, float input_w, float* out, void* stream);

/* ---- detection NMS (csrc/nms.hip, ABI 11) --------------------------------------------------------------------
 * vrnet_detect_select_f32, utils/utils_bbox.py:90-121 (non_max_suppression up to the batched_nms call): pred (B, A, C) =
 *   decode_outputs' result; per anchor class_conf / class_pred = max / first arg-max over channels 5 .. 5+num_classes-1,
 *   score = obj * class_conf (fp32), kept iff score >= conf_thres (a NaN fails).  The candidates of image b go to element
 *   k < counts[b] of rows (B, A, 7) = (x1, y1, x2, y2 = cx -+ w/2, cy -+ h/2, obj, class_conf, class_pred), scores (B, A),
 *   cls (B, A) and ids (B, A) = anchor index, in no particular order.  counts (B) is zeroed on `stream` first.
 * vrnet_nms_segmented_f32, torchvision.ops.boxes.batched_nms (called at utils_bbox.py:124) over `segments` independent
 *   segments: element k < counts[s] (counts NULL: all n_max) of segment s has the box (x1, y1, x2, y2) at
 *   rows[(s * stride + k) * ld], score scores[s * stride + k], class classes[s * stride + k] and tie-break id
 *   ids[s * stride + k] (ids NULL: k; the ids of a segment must be distinct).  Greedy NMS in the order (score descending,
 *   id ascending), suppressing a box of the same class whose IoU with a kept one is > iou_thres (torchvision's CPU
 *   expression in fp32, compared in double).  keep (segments, n_max) receives the k of the kept boxes in that order,
 *   kept (segments) their count; rows_out (segments, n_max, ld), if not NULL, the kept rows (all ld values).
 *   n_max <= 262 144; workspace: vrnet_nms_workspace_bytes(segments, n_max) bytes (the n_max^2 / 8-byte suppression
 *   mask of each segment dominates). */
int vrnet_detect_select_f32(const float* pred, int B, int A, int C, int num_classes, float conf_thres, float* rows,
                            float* scores, long long* cls, int* ids, int* counts, void* stream);
long vrnet_nms_workspace_bytes(int segments, int n_max);
int vrnet_nms_segmented_f32(const float* rows, int ld, const float* scores, const long long* classes, const int* ids,
                            const int* counts, int segments, long stride, int n_max, double iou_thres, void* workspace,
                            long workspace_bytes, int* keep, int* kept, float* rows_out, void* stream);
/* The same NMS with a FIXED capacity, for a captured graph (added within ABI 11: new symbols only; yolo.py:149 non_max_suppression inside predict.py's
 * `video` / `fps` loops, yolo.py:229-291 get_FPS):
 * vrnet_nms_capped_f32: vrnet_nms_segmented_f32 with device `counts` (required) and n_max = cap.  ALL min(counts[s],
 *   stride) candidates of a segment are ranked by (score descending, id ascending); only ranks < cap enter the NMS, so the
 *   result is the exact prefix of the uncapped result -- its kept boxes of rank < cap -- whatever order the candidate list
 *   has.  Bit 8 of *flag (int32, OR-ed in) is set when counts[s] > cap for some segment.  keep / kept / rows_out
 *   (segments, cap[, ld]); workspace: vrnet_nms_workspace_bytes(segments, cap).  stride < 2^31.
 * vrnet_detect_finish_f32, utils/utils_bbox.py:126-134 + 5-30 (yolo_correct_boxes) and yolo.py:164-208 (the box corners and
 *   class counts of detect_image): rows (B, cap, 7) / kept (B) = rows_out / kept of vrnet_nms_capped_f32 on
 *   vrnet_detect_select_f32's rows.  Per kept row: box_xy = (r[0:2] + r[2:4]) / 2, box_wh = r[2:4] - r[0:2] in fp32; then in
 *   fp64, per axis, centre = (centre - offset) * scale, size = size * scale, (centre -+ 0.5 size) * image size, rounded once
 *   to fp32.  The caller computes the shape-only scalars in float64: with a letterbox inner = round(image * min(input /
 *   image)), offset = 0.5 * (input - inner) / input, scale = input / inner; without one offset = 0, scale = 1 (exact
 *   identities).  rows_out (B, cap, 7) = top, left, bottom, right in pixels of the original image, obj, class_conf, class;
 *   rows k >= kept[b] are zero.  draw_rows (B * cap, 5) int32 = left, top, right, bottom, class with left = max(0,
 *   floor(left)), top = max(0, floor(top)), right = min(image_w, floor(right)), bottom = min(image_h, floor(bottom)), the
 *   images back to back (the rest zero); offsets (B + 1) int32 their prefix sums: what vrnet_render_u8 takes as boxes /
 *   box_offsets.  det_counts (B, num_classes) int64 = kept rows per class; a class id outside [0, num_classes) is not
 *   counted and sets bit 16 of *flag. */
int vrnet_nms_capped_f32(const float* rows, int ld, const float* scores, const long long* classes, const int* ids,
                         const int* counts, int segments, long stride, int cap, double iou_thres, void* workspace,
                         long workspace_bytes, int* keep, int* kept, float* rows_out, int* flag, void* stream);
int vrnet_detect_finish_f32(const float* rows, const int* kept, int B, int cap, int num_classes, int image_h, int image_w,
                            double offset_y, double offset_x, double scale_y, double scale_x, float* rows_out,
                            int* draw_rows, int* offsets, long long* det_counts, int* flag, void* stream);

/* ---- segmentation post-processing (csrc/segpost.hip, loss.hip) ------------------------------------------------
 * Added within ABI 11: new symbols only, no existing signature or layout changed; hip.py binds every declared symbol at
 * load time, so a library without them fails the import.
 * vrnet_seg_predict_f32, utils_seg/callbacks.py:140-157 (EvalCallback.get_miou_png) and deeplab.py:141-167 (detect_image):
 *   x (B, C, H, W) fp32 seg logits, C <= 32; the letterbox window rows top .. top+nh-1, columns left .. left+nw-1 (inside
 *   H x W) -> out (B, oh, ow) uint8 = per output pixel the arg-max over c of the bilinear resize of the window's softmax
 *   (softmax over C, crop, resize, arg-max: the reference's order; equal values -> the lower c, as numpy argmax).  The
 *   resize is OpenCV's INTER_LINEAR (cv2.resize at callbacks.py:153): per axis scale = src / dst, f = (d + 0.5) * scale - 0.5
 *   in fp32, s = floor(f), f -= s, s < 0 -> (0, 0), s >= src - 1 -> (src - 1, 0); horizontal taps blended first.
 *   workspace: vrnet_seg_predict_workspace(B, C, nh, nw) bytes (the window's softmax, (B, C, nh, nw) fp32).
 *   The kernels are those of vrnet_seg_predict_ragged_f32, given one record for every image in their arguments.
 * vrnet_confusion_hist, utils_seg/utils_metrics.py:35-44 (fast_hist, called per image at :102): hist (n, n) int64 +=
 *   counts of the pairs (label[i], pred[i]), i < N, row = label, column = pred; label / pred of label_bytes / pred_bytes
 *   = 1 (uint8) or 8 (int64) each; n <= 32.  A pair whose label or prediction is outside [0, n) is skipped (the reference
 *   skips such labels and would bin such a prediction into another cell).  Integer atomics: the same result on every run.
 * vrnet_seg_fscore_f32, utils_seg/utils_metrics.py:12-31 (f_score, utils/utils_fit.py:78,109,177): x (B, C, HW) fp32
 *   logits, onehot (B, HW, C+1) fp32, C <= 32; per class c < C over every pixel tp = sum t_c [p_c > threshold],
 *   sp = sum [p_c > threshold], st = sum t_c (p = softmax over C, t = onehot without its last channel; fp64 sums in a
 *   fixed order), fn = st - tp, fp = sp - tp; out[0] = mean over c of ((1+b^2) tp + smooth) / ((1+b^2) tp + b^2 fn + fp +
 *   smooth), b = beta.  counts (3C) fp64, if not NULL, receives tp[C], sp[C], st[C].  workspace:
 *   vrnet_seg_loss_workspace(B, C, HW) bytes. */
long vrnet_seg_predict_workspace(int B, int C, int nh, int nw);
int vrnet_seg_predict_f32(const float* x, int B, int C, int H, int W, int top, int left, int nh, int nw, int oh, int ow,
                          unsigned char* out, void* workspace, long workspace_bytes, void* stream);
int vrnet_confusion_hist(const void* label, int label_bytes, const void* pred, int pred_bytes, long N, int n,
                         long long* hist, void* stream);
int vrnet_seg_fscore_f32(const float* x, const float* onehot, int B, int C, long HW, float beta, float smooth,
                         float threshold, float* out, double* counts, void* workspace, long workspace_bytes, void* stream);

/* ---- detection mAP (csrc/detmap.hip) ---------------------------------------------------------------------------
 * Added within ABI 11: new symbols only, no existing signature or layout changed; hip.py binds every declared symbol at
 * load time, so a library without them fails the import.
 * vrnet_det_map_f64, utils/utils_map.py:276-798 (get_map, called at utils/callbacks.py:226; voc_ap :95-136,
 *   log_average_miss_rate :31-67) for T <= 16 IoU thresholds min_overlap (a HOST array) in the same launches.
 *   Detections, in input order (the reference's: files by sorted name, then lines): det_image / det_label (D) int,
 *   det_score (D) fp64 without NaN, det_box (D, 4) fp64 = left, top, right, bottom.  order (D): rank -> input index, ranks
 *   grouped by class ascending, inside a class by score descending with ties in input order (:416, a stable sort);
 *   det_offsets (num_classes + 1): the ranks of class c are det_offsets[c] .. det_offsets[c + 1] - 1.
 *   Ground truths, in input order: gt_box (G, 4) fp64, gt_difficult (G) bytes.  gt_perm (G): slot -> input index, slots
 *   grouped by image * num_classes + class with the input order kept inside a group; gt_offsets (n_images * num_classes
 *   + 1): the slots of a group.  Images and classes are indices in [0, n_images) and [0, num_classes).
 *   Match (:462-477): over the ground truths of the detection's image and class in input order, difficult ones included,
 *   iw = min(r) - max(l) + 1, ih likewise, and only if both > 0 ov = iw ih / (area_det + area_gt - iw ih), every extent
 *   with the + 1; the first strict maximum from ovmax = -1.  Per threshold (:482-498): ovmax >= min_overlap[t] on a
 *   difficult ground truth -> neither tp nor fp; on another one the lowest rank matched to it at t is the tp, every later
 *   one an fp; below the threshold an fp.  Per (t, class) (:554-599): ctp / cfp inclusive cumulative sums by rank,
 *   rec = ctp / max(n_gt, 1) (n_gt: non-difficult ground truths of the class), prec = ctp / max(ctp + cfp, 1); ap = voc_ap;
 *   recall, precision and f1 = 2 rec prec / (rec + prec, 1 where 0) at the last rank whose score >= score_threhold (0 if
 *   none); lamr = log_average_miss_rate(rec, cfp, n_img) (n_img: images with a non-difficult ground truth of the class) --
 *   the reference passes RECALL there.  All five are 0 for a class without detections and NaN for a class without a
 *   non-difficult ground truth, which the reference does not evaluate; map[t] = mean ap over the other classes in class
 *   order, 0 if there is none (:380-382, 652-656).  IEEE fp64, one rounding per operation, the reference's operand order.
 *   Outputs by rank: match (D) = input index of the matched ground truth or -1, ovmax (D), tp / fp (T, D) bytes, rec /
 *   prec (T, D) (both NULL = not wanted); per class: n_gt, n_img (num_classes) int, n_tp, ap, f1, recall, precision, lamr
 *   (T, num_classes); map (T).  D = 0 and G = 0 are valid.  Limits: D, G <= 2^24, num_classes <= 65535, n_images x
 *   num_classes <= 2^27.  Integer atomics and fixed-order fp64 sums: the same bits on every run.
 *   workspace: vrnet_det_map_workspace_bytes(D, G, T) bytes (first-claim ranks (T, G), cumulative counts 2 x (T, D)). */
long vrnet_det_map_workspace_bytes(int D, int G, int T);
int vrnet_det_map_f64(const int* det_image, const int* det_label, const double* det_score, const double* det_box,
                      const int* order, const int* det_offsets, int D, const double* gt_box,
                      const unsigned char* gt_difficult, const int* gt_perm, const int* gt_offsets, int G, int n_images,
                      int num_classes, const double* min_overlap, int T, double score_threhold, int* match, double* ovmax,
                      unsigned char* tp, unsigned char* fp, double* rec, double* prec, int* n_gt, int* n_img, int* n_tp,
                      double* ap, double* f1, double* recall, double* precision, double* lamr, double* map,
                      void* workspace, long workspace_bytes, void* stream);

/* ---- COCO detection metrics (csrc/cocomap.hip) -----------------------------------------------------------------
 * Added within ABI 11: new symbols only, no existing signature or layout changed; hip.py binds every declared symbol at
 * load time, so a library without them fails the import.
 * vrnet_coco_map_f64, utils/utils_map.py:894-923 (get_coco_map, called at utils/callbacks.py:224, fed by preprocess_gt /
 *   preprocess_dr :800-892): COCOeval(cocoGt, cocoDt, 'bbox') evaluate(), accumulate(), summarize() with its default
 *   parameters -- iou_thrs (10) = np.linspace(.5, .95, 10) and rec_thrs (101) = np.linspace(0, 1, 101) as DEVICE arrays of
 *   the doubles numpy gives, maxDets 1 / 10 / 100, area ranges [0, 1e10], [0, 1024], [1024, 9216], [9216, 1e10].
 *   Detections: det_box (D, 4) fp64 = left, top, right, bottom in input order.  order (D): slot -> input index, slots
 *   grouped by (image, class), inside a group by score descending with ties in input order; rank (D): a slot's position
 *   inside its group (slots of rank >= 100 are cut); group_start (n_groups + 1): the slots of group k, one group per
 *   (image, class) pair that has a detection; group_gt (n_groups, 2): the group's range lo, hi in gt_perm; class_slot (D):
 *   class order -> slot, classes ascending, inside a class score descending with ties by image index, then rank;
 *   det_offsets (num_classes + 1): the class-order positions of class c.  Ground truths in input order: gt_box (G, 4),
 *   gt_area (G) fp64, gt_crowd (G) bytes (ignore = iscrowd), gt_label (G); gt_perm (G): input indices grouped by (image,
 *   class), input order inside a group.  zero_id_gt: the input index of the ground truth that carries annotation id 0 (the
 *   reference numbers from 0, :865; COCOeval reads dtm == 0 as "unmatched": a detection matched to it consumes it and
 *   counts as a false positive, or as ignored if the ground truth is ignored or its own area is outside the range), -1:
 *   ids from 1.
 *   A box is x, y, w, h = l, t, r - l, b - t (no + 1); IoU: w = min(dx + dw, gx + gw) - max(dx, gx), h likewise, 0 unless
 *   both > 0, else w h / (dw dh [crowd] or dw dh + gw gh - w h).  Per group, threshold t and range: a ground truth is
 *   ignored if crowd or area outside the range; detections in slot order, each starting from iou = min(t, 1 - 1e-10) and
 *   taking, over the non-ignored ground truths in input order and then (only if none was taken) the ignored ones, the last
 *   one with IoU >= the running best that is not yet matched (a crowd may be matched again); an unmatched detection whose
 *   area w h is outside the range is ignored.  Per (class, range, maxDet M): the first M slots of every group in class
 *   order; tp / fp cumulative sums, rc = tp / npig, pr = tp / ((fp + tp) + 2^-52), the envelope from the back, precision[r]
 *   = pr at the first index with rc >= rec_thrs[r] (0: none), recall = rc[-1] (0: no detections); -1 where npig = 0.
 *   Outputs: dt_match (40, D) by slot, plane t * 4 + range: the matched ground truth's input index or -1; dt_code (40, D)
 *   bytes: 0 fp, 1 tp, 2 ignored, 3 cut; n_gt (num_classes, 4) int = npig; precision (10, 101, num_classes, 4, 3), recall
 *   (10, num_classes, 4, 3), stats (12) in COCOeval.stats order (-1: no entry > -1).  IEEE fp64, one rounding per
 *   operation; integer atomics only and fixed-order sums: the same bits on every run.  D = 0 and G = 0 are valid.
 *   A group keeps its IoUs (8 x min(n_det, 100) x n_gt bytes), 40 matched bit sets and a flag byte per ground truth --
 *   vrnet_coco_map_group_bytes(n_det, n_gt) bytes -- in LDS; lds_bytes (<= 65536) is the largest such figure over the
 *   groups that stay at or below 65536, and every other group k has group_ws[k] (a multiple of 8) as the offset of its
 *   slice in slice_bytes bytes of the workspace.
 *   workspace: vrnet_coco_map_workspace_bytes(D, slice_bytes) bytes.  Limits: D, G <= 2^24, num_classes <= 65535. */
long vrnet_coco_map_group_bytes(int n_det, int n_gt);
long vrnet_coco_map_workspace_bytes(int D, long slice_bytes);
int vrnet_coco_map_f64(const double* det_box, const int* order, const int* rank, const int* class_slot,
                       const int* det_offsets, int D, const int* group_start, const int* group_gt, const long* group_ws,
                       int n_groups, int lds_bytes, long slice_bytes, const double* gt_box, const double* gt_area,
                       const unsigned char* gt_crowd, const int* gt_label, const int* gt_perm, int G, int num_classes,
                       int zero_id_gt, const double* iou_thrs, const double* rec_thrs, int* dt_match,
                       unsigned char* dt_code, int* n_gt, double* precision, double* recall, double* stats,
                       void* workspace, long workspace_bytes, void* stream);

/* ---- input formats -----------------------------------------------------------------------------
 * What YoloDataset.__getitem__ / yolo_dataset_collate (utils/dataloader.py:88-107, 440-457) do to a letterboxed batch,
 * from BYTES: img (B, H, W, 3) u8 RGB -> images (B, 3, H, W) f32 = ((v / 255) - mean) / std evaluated in double and rounded
 * once (utils_seg/utils.py:43-47 preprocess_input on a float64 array, then FloatTensor: bit-identical); png (B, H, W) u8
 * labels -> png_out (B, H, W) int64 with labels >= num_classes_seg set to the ignore class num_classes_seg (:96-97) and
 * onehot (B, H, W, num_classes_seg + 1) f32 (:103-105).  img or png may be NULL (that half is skipped), as may png_out or
 * onehot. */
int vrnet_batch_formats_u8(const unsigned char* img, const unsigned char* png, int B, int H, int W, int num_classes_seg,
                           float* images, long long* png_out, float* onehot, void* stream);
/* vrnet_radar_normalise (added within ABI 11: a new symbol only), utils/utils.py:50-53 preprocess_input_radar as yolo.py:134 applies it to one frame's maps:
 * radar (B, frame_elems) float32 (is_f64 = 0) or float64 (1), frame_elems = 4 H W -> out (B, frame_elems) f32 =
 * (x - lo) / (hi - lo) + 1e-13 with lo / hi the frame's minimum / maximum over all its values, evaluated in the input's
 * type as numpy does and rounded to float32 (bit-identical; a constant frame gives NaN, as the reference's 0 / 0; a NaN in a
 * frame makes the whole frame NaN).  normalise = 0: the cast alone (deeplab.py and the dataloader feed the maps raw).  Two
 * launches (partials, apply), no atomics.  workspace (8-byte aligned): vrnet_radar_workspace_bytes(B) bytes. */
long vrnet_radar_workspace_bytes(int B);
int vrnet_radar_normalise(const void* radar, int is_f64, int B, long frame_elems, int normalise, float* out, void* workspace,
                          long workspace_bytes, void* stream);

/* ---- letterbox from raw bytes (csrc/letterbox.hip) --------------------------------------------------------------
 * Added within ABI 11: new symbols only, no existing signature or layout changed.
 * vrnet_letterbox_u8, utils/utils.py:19-32 and utils_seg/utils.py:19-31 (resize_image: detect_image, get_FPS, get_map_txt,
 *   both EvalCallbacks) and the random=False branch of get_random_data (utils/dataloader.py:131-146): img (B, ih, iw, 3) u8
 *   RGB frames of ONE original size and, optionally, label (B, ih, iw) u8 maps -> the frames resized to nw x nh with
 *   Pillow's Image.BICUBIC and pasted at column dx, row dy of a W x H canvas of 128, the labels resized with Image.NEAREST
 *   and pasted on a canvas of 0.  The caller computes (nw, nh, dx, dy): scale = min(W / iw, H / ih), nw = int(iw * scale),
 *   nh = int(ih * scale), dx = (W - nw) / 2, dy = (H - nh) / 2 (floor), or (W, H, 0, 0) for letterbox_image=False; required:
 *   0 < nw <= W, 0 < nh <= H and the window inside the canvas.  Outputs, any non-empty subset (NULL = not wanted):
 *   canvas (B, H, W, 3) u8; images (B, 3, H, W) f32 = the canvas normalised exactly as vrnet_batch_formats_u8 does it;
 *   label_out (B, H, W) u8 (needs label).
 *   EXACTNESS: the bytes are Pillow's, bit for bit (checked against Pillow 12.2).  Bicubic: Resample.c ImagingResample --
 *   per axis in -> out: scale = in / out, fs = max(scale, 1), support = 2 fs; per output index xx: center = (xx + 0.5) scale,
 *   xmin = max((int)(center - support + 0.5), 0), xmax = min((int)(center + support + 0.5), in), weights
 *   bicubic((x + xmin - center + 0.5) / fs) (a = -0.5) normalised by their sum, k = (int)(w 2^22 +- 0.5); out = clamp((2^21 +
 *   sum k v) >> 22, 0, 255) in int32; the horizontal pass first, its uint8 result feeding the vertical pass; a pass whose
 *   axis keeps its size is skipped.  Nearest: Geometry.c ImagingScaleAffine -- per axis a0 = in / out, xo = a0 / 2,
 *   idx[x] = (int)xo, xo += a0 (a running sum).  The tables are built on the device in double, one rounding per operation:
 *   no host table, no copy, no synchronisation; the call can be captured in a graph.
 *   workspace: vrnet_letterbox_workspace(B, ih, iw, nh, nw) bytes (the tables plus the horizontal pass's uint8 result). */
long vrnet_letterbox_workspace(int B, int ih, int iw, int nh, int nw);
int vrnet_letterbox_u8(const unsigned char* img, const unsigned char* label, int B, int ih, int iw, int H, int W, int nw,
                       int nh, int dx, int dy, unsigned char* canvas, float* images, unsigned char* label_out,
                       void* workspace, long workspace_bytes, void* stream);

/* ---- result rendering (csrc/render.hip) -------------------------------------------------------------------------
 * Added within ABI 11: new symbols only, no existing signature or layout changed; hip.py binds every declared symbol at
 * load time, so a library without them fails the import.
 * vrnet_render_u8, deeplab.py:169-222 (detect_image: the three mix_types and the pixel counts of :172-185) and yolo.py:221-222
 *   (the box outlines), in one launch: frames (B, ih, iw, 3) u8 RGB original frames -> out (B, ih, iw, 3) u8.  Every pointer
 *   but frames and out may be NULL.  Every output byte is exact.
 *   class_map (B, ih, iw) u8 (what vrnet_seg_predict_f32 writes) with palette (n_colors, 3) u8, 1 <= n_colors <= 256:
 *     mix_type 1 (deeplab.py:209)  out = palette[class];
 *     mix_type 2 (deeplab.py:216)  out = frame where class != 0, else 0 (a bool times float32, cast back); no palette needed;
 *     mix_type 0 (deeplab.py:193-201)  Image.blend(frame, palette[class], alpha), Pillow's ImagingBlend per byte:
 *       out = (uint8)((float)a + alpha * (float)((int)b - (int)a)), a the frame byte, b the palette byte, alpha a C float
 *       in [0, 1] (0.7f, not 0.7), each operation rounded to fp32 (no fused multiply-add), truncated towards zero;
 *       byte-identical to Pillow 12.2 on all 256 x 256 (a, b) pairs.
 *     No class_map: out = frame.  A class id >= n_colors (the reference raises IndexError) takes the last colour, is not
 *     counted, and sets bit 0 of *flag.
 *   counts (B, n_colors) int64, if not NULL (needs class_map; n_colors > 0 even without a palette): OVERWRITTEN with the
 *     pixels of each class per image (deeplab.py:172-185).  Integer atomics: the same result on every run.
 *   boxes (n_rows, 5) int32 rows left, top, right, bottom, colour index; box_offsets (B + 1) int32: the rows of image b
 *     are box_offsets[b] .. box_offsets[b + 1] - 1 (clamped into [0, n_rows]); box_palette (n_box_colors, 3) u8,
 *     1 <= n_box_colors <= 256; thickness >= 1.  Painted after the mix (yolo.py:221-222): for i = 0 .. thickness - 1 the
 *     ring [left+i, top+i, right-i, bottom-i] paints the perimeter pixels of that inclusive rectangle, clipped to the
 *     image, while left+i <= right-i and top+i <= bottom-i; where several rows of an image paint a pixel the LAST row
 *     wins (sequential drawing) -- decided per pixel, independent of scheduling.  Two differences from Pillow 12.2's
 *     ImageDraw.rectangle(outline=): Pillow paints a ring of one row (y0 == y1) two rows high ([5,5,5,5] paints (5,5) and
 *     (5,6)) and raises ValueError for x1 < x0; here a ring is its geometric perimeter and an empty ring paints nothing.
 *     At most 1024 rows per image: later rows of an image are ignored and set bit 2 of *flag; a colour index outside
 *     [0, n_box_colors) is clamped and sets bit 1.
 *   flag: one int32, if not NULL: the bits above are OR-ed into it (never cleared here), so a caller can read it when it
 *     next synchronises.
 *   out may BE frames when class_map is NULL (boxes drawn in place: only painted pixels are written); any other overlap of
 *   out with frames or class_map is rejected.  ih, iw <= 2^24, B ih iw < 2^31.  No workspace, no allocation, no host
 *   synchronisation; the call (a memset of counts, one kernel) can be captured in a graph. */
int vrnet_render_u8(const unsigned char* frames, const unsigned char* class_map, int B, int ih, int iw,
                    const unsigned char* palette, int n_colors, int mix_type, float alpha, const int* boxes,
                    const int* box_offsets, int n_rows, const unsigned char* box_palette, int n_box_colors, int thickness,
                    unsigned char* out, long long* counts, int* flag, void* stream);

/* ---- ragged batches: frames of mixed sizes through the four size-dependent entry points -----------------------------
 * Added within ABI 11: new symbols only, no existing signature, layout or kernel behaviour changed; hip.py binds every
 * declared symbol at load time, so a library without them fails the import.
 * LAYOUT.  Frames, label maps, class maps and rendered frames are padded buffers (B, ihm, iwm[, 3]); (ihm, iwm) is the
 *   capacity.  Image b occupies the top-left ih_b x iw_b corner of slot b, with row stride iwm.  Every OUTPUT pixel of a
 *   slot outside its image (class map, rendered frame) is written 0 on every call; input padding is never read into a
 *   result.
 * TABLE.  geom (B) records in DEVICE memory, one per image, built on the host per image by the same helpers that compute
 *   the launch scalars of the fixed entry points, and only read here:
 *     ih, iw                       the image's own size, 1 <= ih <= ihm, 1 <= iw <= iwm
 *     nw, nh, dx, dy               the letterbox window (vrnet_letterbox_u8's scalars)
 *     seg_top, seg_left, seg_nh, seg_nw   the window vrnet_seg_predict_f32 takes (utils_seg/utils.py:19-31; kept apart
 *                                  from the four above because yolo_correct_boxes rounds where resize_image truncates)
 *     thickness                    the outline thickness of yolo.py:164
 *     reserved                     0
 *     offset_y, offset_x, scale_y, scale_x   the float64 un-map scalars of vrnet_detect_finish_f32
 *   80 bytes, 8-byte aligned.  The kernels do not trust it: ih / iw are clamped to [0, ihm] / [0, iwm], a window to the
 *   canvas (sizes to [0, H] / [0, W], then the corner so that it fits), thickness to [1, 2^24], so no access leaves a slot;
 *   a record that had to be clamped, one with ih <= 0 or iw <= 0 -- or, in the letterbox, whose taps exceed max_taps and
 *   are truncated -- sets bit 256 (FLAG_GEOMETRY) of *flag (OR-ed in; flag may be NULL except in detect_finish).  An image
 *   or window clamped to nothing is all padding.
 * GRIDS are sized by the capacities, a whole number of workgroups per image (the image is grid dimension y, or
 *   blockIdx.x / blocks-per-image in seg_predict): a workgroup lies inside one image and reads one record.  All calls: no allocation, no host synchronisation, capturable in a graph.
 * vrnet_letterbox_ragged_u8: vrnet_letterbox_u8 per image -- img (B, ihm, iwm, 3), label (B, ihm, iwm) -> canvas (B, H, W, 3)
 *   / images (B, 3, H, W) / label_out (B, H, W), the same Pillow-exact bytes.  The tables of image b are built on the
 *   device in slot b of the workspace ((W + H) * (3 + max_taps) ints); the horizontal pass writes a (B, ihm, W, 3)
 *   intermediate; a pass whose axis keeps its size is skipped per image.  max_taps (>= 5): the tap capacity of a table
 *   entry; image b needs ksize = 2 * ceil(2 * max(in / out, 1)) + 1 per resized axis.
 *   workspace: vrnet_letterbox_ragged_workspace(B, ihm, iwm, H, W, max_taps) bytes.
 * vrnet_detect_finish_ragged_f32: vrnet_detect_finish_f32 with image_h, image_w and the four scalars of image b from geom[b].
 * vrnet_seg_predict_ragged_f32: vrnet_seg_predict_f32 with the window and the output size of image b from geom[b]; out is
 *   the padded (B, ihm, iwm) map, written by the same kernels.  workspace: vrnet_seg_predict_ragged_workspace(B, C, H, W) bytes.
 * vrnet_render_ragged_u8: vrnet_render_u8 on the padded frames / class_map / out with ih, iw, thickness of image b from
 *   geom[b]; boxes are clipped to the image's own size and counts cover its own pixels only.  out must not overlap frames
 *   (the padding is written): there is no in-place form. */
typedef struct vrnet_frame_geom {
  int ih, iw;
  int nw, nh, dx, dy;
  int seg_top, seg_left, seg_nh, seg_nw;
  int thickness;
  int reserved;
  double offset_y, offset_x, scale_y, scale_x;
} vrnet_frame_geom;
long vrnet_letterbox_ragged_workspace(int B, int ihm, int iwm, int H, int W, int max_taps);
int vrnet_letterbox_ragged_u8(const unsigned char* img, const unsigned char* label, const vrnet_frame_geom* geom, int B,
                              int ihm, int iwm, int H, int W, int max_taps, unsigned char* canvas, float* images,
                              unsigned char* label_out, int* flag, void* workspace, long workspace_bytes, void* stream);
int vrnet_detect_finish_ragged_f32(const float* rows, const int* kept, const vrnet_frame_geom* geom, int B, int cap,
                                   int num_classes, int ihm, int iwm, float* rows_out, int* draw_rows, int* offsets,
                                   long long* det_counts, int* flag, void* stream);
long vrnet_seg_predict_ragged_workspace(int B, int C, int H, int W);
int vrnet_seg_predict_ragged_f32(const float* x, const vrnet_frame_geom* geom, int B, int C, int H, int W, int ihm, int iwm,
                                 unsigned char* out, int* flag, void* workspace, long workspace_bytes, void* stream);
int vrnet_render_ragged_u8(const unsigned char* frames, const unsigned char* class_map, const vrnet_frame_geom* geom, int B,
                           int ihm, int iwm, const unsigned char* palette, int n_colors, int mix_type, float alpha,
                           const int* boxes, const int* box_offsets, int n_rows, const unsigned char* box_palette,
                           int n_box_colors, unsigned char* out, long long* counts, int* flag, void* stream);

/* ---- the targets of a training batch from raw label maps and boxes (csrc/traintargets.hip) ---------------------------
 * Added within ABI 11: new symbols only.  Both follow the ragged rules above: padded (B, ihm, iwm) slots, the geometry of
 * image b from geom[b], clamped on the device (bit 256 of *flag for a clamped record; flag may be NULL), grid y the image,
 * no workspace, no allocation, no host synchronisation, capturable in a graph.  Every output element is written on every
 * call.  With vrnet_letterbox_ragged_u8 (images only) they are the `random=False` dataset item of utils/dataloader.py
 * (:88-105, :129-183) for a batch of frames of mixed sizes, bit for bit.
 * vrnet_seg_targets_ragged_u8: label (B, ihm, iwm) -> png_out (B, H, W) int64 and onehot (B, H, W, ns + 1) fp32.  Inside the
 *   window (dx, dy, nw, nh) the source pixel is Pillow's Image.NEAREST pick (the index recurrence of the letterbox's
 *   label_out), outside it the label is 0; labels >= num_classes_seg become num_classes_seg, and the one-hot row is that of
 *   vrnet_batch_formats_u8.  0 < num_classes_seg < 255; (W + H) * 4 + 16 * W bytes of LDS must fit 64 KiB.
 * vrnet_box_targets_ragged_f32: boxes (B, max_gt, 5) int32 rows x1, y1, x2, y2, cls in pixels of the original image, counts
 *   (B) -> targets (B, max_gt, 5) fp32 rows cx, cy, w, h, cls on the canvas and counts_out (B): the buffers
 *   vrnet_yolo_loss_f32 reads.  Per coordinate, in fp64 as numpy evaluates dataloader.py:170-171: the 64-bit integer product
 *   x * nw, converted to double, / iw (IEEE division), + dx, truncated toward zero (y: nh, ih, dy); then x1, y1 < 0 -> 0,
 *   x2 > W -> W, y2 > H -> H; rows with x2 - x1 > 1 and y2 - y1 > 1 are kept and compacted IN INPUT ORDER (the reference's
 *   shuffle is omitted); w = x2 - x1, h = y2 - y1, cx = x1 + w / 2, cy = y1 + h / 2.  Rows at and beyond counts_out[b] are
 *   written 0.  A counts[b] outside [0, max_gt] is clamped and sets bit 512 of *flag.  One workgroup per image. */
int vrnet_seg_targets_ragged_u8(const unsigned char* label, const vrnet_frame_geom* geom, int B, int ihm, int iwm, int H,
                                int W, int num_classes_seg, long long* png_out, float* onehot, int* flag, void* stream);
int vrnet_box_targets_ragged_f32(const int* boxes, const int* counts, const vrnet_frame_geom* geom, int B, int max_gt,
                                 int ihm, int iwm, int H, int W, float* targets, int* counts_out, int* flag, void* stream);

/* ---- detection heat maps (csrc/heatmap.hip) ---------------------------------------------------------------------------
 * Added within ABI 11: new symbols only, no existing signature, layout or kernel behaviour changed.
 * vrnet_heatmap_f32, yolo.py:288-351 (detect_heatmap; predict.py's `heatmap` mode) for B images of one size ih x iw:
 *   p3, p4, p5: the raw detection maps (B, 5 + nc, H/8, W/8), (.., H/16, W/16), (.., H/32, W/32) fp32 NCHW of an H x W input
 *   (multiples of 32), nc >= 1.  Per level score = sigmoid(max_c cls_c) * sigmoid(obj) in fp32 (:339), resized to ih x iw
 *   with OpenCV's INTER_LINEAR rule (:340: the taps of vrnet_seg_predict_f32, horizontal blend first), times 255 and
 *   truncated to a byte (:341); mask (B, ih, iw) u8 = the max over the levels (:342).  minmax (B, 2) int32 = the (min, max)
 *   of each image's mask, the vmin / vmax of matplotlib's default normalisation (:344).
 *   window = 0: the reference's resize of the WHOLE level map, whatever letterbox made the input (dx, dy, nw, nh unused).
 *   window = 1: this project's aligned form: pixel x is mapped through the letterbox window (dx, dy, nw, nh) of the canvas,
 *     f = ((dx + ((x + 0.5) * nw) / iw) * w_l) / W - 0.5 in fp64, one rounding per operation, then the same floor and clamps,
 *     the fraction rounded to fp32; likewise in y.  The window must lie inside the canvas.
 *   out (B, ih, iw, 3) u8 or NULL (the mask only; frames and cmap may then be NULL): Image.blend(frame, cmap[index], alpha) per byte
 *     in the arithmetic of vrnet_render_u8's mix_type 0, with frames (B, ih, iw, 3) u8, cmap (256, 3) u8 (matplotlib's jet
 *     as bytes for the reference's picture) and index(m) = trunc(((m - vmin) / (vmax - vmin)) * 256) in fp64, one rounding
 *     per operation, 256 -> 255, and 0 for every m when vmax == vmin.  The picture has the frame's resolution: matplotlib's
 *     200-dpi figure with its margins is not reproduced.  out must not overlap frames or mask.  0 <= alpha <= 1.
 *   workspace: vrnet_heatmap_workspace(B, H, W) bytes (the score planes), 4-byte aligned.
 *   Three launches (two without out), no memset, integer atomics only (the same bytes on every run), no allocation, no
 *   host synchronisation, capturable in a graph.
 * vrnet_heatmap_ragged_f32: the same kernels on padded slots mask (B, ihm, iwm) / frames, out (B, ihm, iwm, 3), with ih, iw
 *   and the window (dx, dy, nw, nh) of image b from geom[b] (the ragged rules above: clamped on the device, bit 256 of *flag
 *   for a clamped record, flag may be NULL).  Every pixel of a slot outside its image is written 0; minmax[b] covers the
 *   image's own pixels and is (255, 0) for an image without pixels.  Image b equals vrnet_heatmap_f32 on that image alone.
 *   workspace: vrnet_heatmap_ragged_workspace(B, H, W) bytes. */
long vrnet_heatmap_workspace(int B, int H, int W);
int vrnet_heatmap_f32(const float* p3, const float* p4, const float* p5, int B, int nc, int H, int W, int ih, int iw,
                      int window, int dx, int dy, int nw, int nh, const unsigned char* frames, const unsigned char* cmap,
                      float alpha, unsigned char* mask, unsigned char* out, int* minmax, void* workspace,
                      long workspace_bytes, void* stream);
long vrnet_heatmap_ragged_workspace(int B, int H, int W);
int vrnet_heatmap_ragged_f32(const float* p3, const float* p4, const float* p5, const vrnet_frame_geom* geom, int B, int nc,
                             int H, int W, int ihm, int iwm, int window, const unsigned char* frames,
                             const unsigned char* cmap, float alpha, unsigned char* mask, unsigned char* out, int* minmax,
                             int* flag, void* workspace, long workspace_bytes, void* stream);

/* ---- the record arena of a validation pass (csrc/evalacc.hip) --------------------------------------------------------
 * Added within ABI 11: a new symbol only.
 * vrnet_eval_append_f32, utils/callbacks.py:151-170 (get_map_txt: the rows, scores and coordinates it writes per image)
 *   and :207-220 (the ground-truth file of on_epoch_end), for the B images of one batch, appended at the image slots
 *   *cursor .. *cursor + B - 1 of an arena of N slots; no host argument changes between the launches of a validation pass.
 *   rows (B, cap, 7) fp32 / kept (B) int32 = rows_out / kept of vrnet_detect_finish_f32 (top, left, bottom, right, obj,
 *   class_conf, class, in descending score order); gt (B, max_gt, 5) int32 = x1, y1, x2, y2, class with gt_count (B).
 *   Image b, slot s = *cursor + b, rows k < n = min(kept[b], max_boxes, cap):
 *     det_score (N, max_boxes) fp64 = float(str(score)[:6]) of score = obj * class_conf (one fp32 multiply): with
 *       x = (double)score, k4 = rint(x * 1e4), it is k4 / 1e4 if (float)(k4 / 1e4) == score, else floor(x * 1e4) / 1e4
 *       (exact for 1e-4 <= score <= 1, where numpy prints positionally);
 *     det_box (N, max_boxes, 4) fp64 = left, top, right, bottom, each (double)(int)value, truncated toward zero; a
 *       non-finite value or one outside int32 (Python raises there) is written as 0 and sets bit 128 of *flag;
 *     det_label (N, max_boxes) int32 = (int)class, under the same rule; det_count (N) int32 = n.
 *     Elements k >= n of a slot are not written.
 *   gt_label (N, max_gt) int32, gt_box (N, max_gt, 4) fp64, gt_n (N) int32: the first min(gt_count[b], max_gt) ground
 *   truths; gt_count[b] > max_gt sets bit 64.  If *cursor + B > N nothing is written, bit 32 is set and *cursor stays;
 *   otherwise a one-thread launch behind the append adds B to *cursor.  No atomics on the records: every element has one
 *   writer, the arena is bitwise the same on every run. */
int vrnet_eval_append_f32(const float* rows, const int* kept, int B, int cap, const int* gt, const int* gt_count,
                          int max_gt, int* cursor, int N, int max_boxes, int* det_label, double* det_score,
                          double* det_box, int* det_count, int* gt_label, double* gt_box, int* gt_n, int* flag,
                          void* stream);

/* ---- training losses on the path's outputs: value + gradient w.r.t. the head outputs ------------
 * vrnet_yolo_loss_f32: YOLOLoss (nets/yolo_training.py:60-427): decode (:99-111), SimOTA assignment per image
 *   (get_assignments :200-264, get_in_boxes_info :291-368, dynamic_k_matching :370-427), IoU / objectness / class
 *   losses (:113-198, IOUloss :13-57).  levels[l]: raw (B, C = 5+nc, hs[l], ws[l]) NCHW maps; grads[l]: same shapes,
 *   receives grad_scale * d loss / d levels[l] (grads or grads[l] NULL = value only); labels (B, max_gt, 5) =
 *   [cx, cy, w, h, class] in input pixels, counts[b] boxes valid in image b (0 allowed, :145-149).
 *   out[5] = {loss, num_fg, sum iou loss, sum obj loss, sum cls loss}; optional per-anchor assignment outputs
 *   fg_out (B,A) u8, matched_out (B,A) int (-1 = background), piou_out (B,A).  levels/grads/hs/ws/strides: HOST arrays.
 * vrnet_seg_loss_f32: CE_Loss (focal = 0), Focal_Loss (focal = 1) or no main term (focal = -1) (+ Dice_loss when dice = 1)
 *   (nets/deeplabv3_training.py:9-59; combination utils/utils_fit.py:96-103) on logits x (B, C, H, W) NCHW already at
 *   label size, png (B, H, W) int64 with ignore index C, onehot (B, H, W, C+1) float, weights[C] or NULL.
 *   out[3] = {main, dice, main + dice}; dx (NULL = value only) = grad_scale * d(main + dice)/dx. */
long vrnet_yolo_loss_workspace(int B, long n_anchors, int max_gt, int num_classes);
int vrnet_yolo_loss_f32(const float* const* levels, float* const* grads, const int* hs, const int* ws, const float* strides,
                        int n_levels, int B, int C, const float* labels, const int* counts, int max_gt, float grad_scale,
                        float* out, unsigned char* fg_out, int* matched_out, float* piou_out, void* workspace,
                        long workspace_bytes, void* stream);
long vrnet_seg_loss_workspace(int B, int C, long HW);
int vrnet_seg_loss_f32(const float* x, const long long* png, const float* onehot, const float* weights, int B, int C,
                       long HW, int focal, int dice, float alpha, float gamma, float beta, float smooth, float grad_scale,
                       float* out, float* dx, void* workspace, long workspace_bytes, void* stream);

/* ---- the synthetic backward driver: loss[0] = sum_k mean(t_k^2) over k <= 8 contiguous fp32 tensors -- the det maps
 * and the seg logits -- and its gradient grad_k = (2 g / n_k) t_k, g = upstream gradient of the scalar (device).  t, n, grad:
 * HOST arrays of device pointers / element counts.  Replaces the eager `sum((d * d).mean()) + (seg * seg).mean()` of the
 * reference's own smoke test (vr_coc.py:817-830 builds the same kind of scalar) and its autograd: ~27 launches -> 3. */
long vrnet_mean_square_workspace(int k, const long* n);
int vrnet_mean_square_f32(int k, const void* const* t, const long* n, float* loss, void* workspace, long workspace_bytes,
                          void* stream);
int vrnet_mean_square_bwd_f32(int k, const void* const* t, const long* n, const float* g, void* const* grad, void* stream);

/* ---- training augmentation on the device (csrc/augment.hip) -------------------------------------------------------------
 * Added within ABI 11: new symbols and one new record layout (vrnet_aug_rec) only, no existing signature, layout or kernel
 * behaviour changed; hip.py binds every declared symbol at import.
 * The random resize, placement, left-right flip and HSV jitter of utils/dataloader.py:187-247, applied consistently to the
 * frame, the label map (as utils_seg/dataloader.py:91-111), the boxes and the radar map of an image.  Nothing here draws a
 * random number: the host draws one record per image (data.augment_params) and the kernels apply it; they equal the host
 * functions data.augment_sample / augment_boxes / hsv_jitter bit for bit.  All four entry points follow the ragged rules
 * above: padded (B, ihm, iwm) slots, image index on grid y, the record of image b read and clamped on the device -- 0 <= ih
 * <= ihm, 0 <= iw <= iwm, 0 <= nw, nh <= 2 max(W, H), -nw <= dx <= W, -nh <= dy <= H, the letterbox window inside the canvas --
 * and bit 256 of *flag (VR_FLAG_GEOMETRY; flag may be NULL) set when something had to be clamped, when a size or window is
 * not positive, or when a resize needs more taps than max_taps.  An image whose record had to be clamped gets padding in
 * every output (grey canvas without the colour stage, label 0, no boxes, radar 0); the other images are unaffected.  No host
 * synchronisation; capturable.
 * The window (nw x nh pasted at (dx, dy)) may be larger than the canvas and start at negative offsets; what falls outside
 * is cropped, as Pillow's paste does.  flip mirrors the finished canvas (labels, boxes and radar alike).
 * vrnet_augment_frames_u8: img (B, ihm, iwm, 3) -> canvas (B, H, W, 3) uint8 and / or images (B, 3, H, W) fp32 normalised as
 *   vrnet_batch_formats_u8 does: Pillow's BICUBIC bytes (a pass whose size does not change is skipped), grey (128) padding,
 *   the flip, then -- color != 0 -- RGB -> HSV in OpenCV's 8-bit integer arithmetic, lut[0..2] on H, S, V, and HSV -> RGB in
 *   float32, over the whole canvas.  Three launches.  workspace: vrnet_letterbox_ragged_workspace(B, ihm, iwm, H, W,
 *   max_taps) bytes (tables and the horizontal result are indexed by visible column / row).
 * vrnet_augment_seg_targets_u8: label (B, ihm, iwm) -> png_out (B, H, W) int64 and onehot (B, H, W, ns + 1) fp32 as
 *   vrnet_seg_targets_ragged_u8 writes them: Pillow's NEAREST pick inside the window, 0 outside.
 * vrnet_augment_box_targets_f32: vrnet_box_targets_ragged_f32's arithmetic with the record's window, and x1, x2 = W - x2,
 *   W - x1 before the clip when flip is set; the same compaction, count clamp and VR_FLAG_BOX_COUNT.
 * vrnet_augment_radar_f32: radar (B, 4, H, W), aligned with the letterbox window (lb_*) of its frame -> out (B, 4, H, W): for
 *   canvas pixel (x, y), x' = flip ? W - 1 - x : x, wx = x' - dx, wy = y - dy; 0 outside 0 <= wx < nw, 0 <= wy < nh, else
 *   radar[c][lb_dy + ((2 wy + 1) lb_nh) / (2 nh)][lb_dx + ((2 wx + 1) lb_nw) / (2 nw)] (integer division).  out != radar; ihm,
 *   iwm only judge the record as the other three entry points do. */
typedef struct vrnet_aug_rec {
  int ih, iw;                        /* the image's own size inside its (ihm, iwm) slot */
  int nw, nh, dx, dy;                /* the resized frame and where it is pasted; may leave the canvas on every side */
  int flip, color;                   /* != 0: mirror the canvas left-right; run the colour stage */
  int lb_nw, lb_nh, lb_dx, lb_dy;    /* data.letterbox_geometry: the window the stored radar map is aligned with */
  unsigned char lut[3][256];         /* hue, saturation, value tables of the colour stage */
} vrnet_aug_rec;                     /* 816 bytes; the table must be 8-byte aligned */
int vrnet_augment_frames_u8(const unsigned char* img, const vrnet_aug_rec* aug, int B, int ihm, int iwm, int H, int W,
                            int max_taps, unsigned char* canvas, float* images, int* flag, void* workspace,
                            long workspace_bytes, void* stream);
int vrnet_augment_seg_targets_u8(const unsigned char* label, const vrnet_aug_rec* aug, int B, int ihm, int iwm, int H, int W,
                                 int num_classes_seg, long long* png_out, float* onehot, int* flag, void* stream);
int vrnet_augment_box_targets_f32(const int* boxes, const int* counts, const vrnet_aug_rec* aug, int B, int max_gt, int ihm,
                                  int iwm, int H, int W, float* targets, int* counts_out, int* flag, void* stream);
int vrnet_augment_radar_f32(const float* radar, const vrnet_aug_rec* aug, int B, int ihm, int iwm, int H, int W, float* out,
                            int* flag, void* stream);

/* ---- the blur and the rotation behind the augmentation (csrc/augment.hip) ---------------------------------------------------
 * Added within ABI 11: new symbols and one new record layout (vrnet_aug_post_rec) only; the four entry points above are
 * unchanged in signature and bytes; hip.py binds every declared symbol at import.
 * utils_seg/dataloader.py:113-131: cv2.GaussianBlur(image, (5, 5), 0) (:113-115) and a rotation about the canvas centre by a
 * whole angle in [-10, 10] (:117-131: cv2.warpAffine, INTER_CUBIC with a grey (128) border for the image, INTER_NEAREST with a 0
 * border for the label map), each with probability 0.25, between the flip and the colour stage.  The host draws one
 * vrnet_aug_post_rec per image (data.augment_post_params) and computes both matrices (data.rotation_matrices); the kernels walk
 * warpAffine's fixed-point coordinates (AB_BITS = 10, rint in double) from the twelve doubles and equal data.gaussian_blur5_u8,
 * rotate_canvas_u8, rotate_nearest and rotate_boxes bit for bit.  Those functions restate OpenCV's 8-bit paths from its public
 * sources; agreement with cv2's own bytes is UNMEASURED.  A record with a matrix entry that is not finite or with |angle| >
 * max_angle neither blurs nor rotates and sets bit 256 of *flag (VR_FLAG_GEOMETRY; flag may be NULL).  H, W >= 8; 0 <=
 * max_angle <= 45; the post table must be 8-byte aligned.  One launch each; no host synchronisation; capturable.
 * vrnet_augment_post_frames_u8: canvas (B, H, W, 3), what vrnet_augment_frames_u8 wrote with the colour stage OFF (the colour
 *   moves behind the rotation) -> images (B, 3, H, W) fp32 normalised and / or canvas_out (B, H, W, 3), canvas_out != canvas:
 *   the blur (weights {1, 4, 6, 4, 1} on both axes, BORDER_REFLECT_101, (S + 128) >> 8), the bicubic rotation (4 x 4 taps with
 *   int32 weights that sum to 32768, a tap outside the canvas reads 128, (sum + 16384) >> 15 clipped), then -- color != 0 in the
 *   image's vrnet_aug_rec -- the colour stage with its tables.  A workgroup owns a 32 x 8 output tile and stages the bounding
 *   box of its source pixels in LDS; the box is sized for max_angle (a tile whose box is larger reads grey beyond it and sets
 *   bit 256).  ihm, iwm only judge the vrnet_aug_rec as the entry points above do.
 * vrnet_augment_post_seg_targets_i64: png (B, H, W) int64, what vrnet_augment_seg_targets_u8 wrote -> png_out (B, H, W) int64,
 *   png_out != png, and onehot (B, H, W, ns + 1) fp32 of the rotated label canvas: the nearest walk, 0 outside.
 * vrnet_augment_post_box_targets_f32: vrnet_augment_box_targets_f32 with the rotation between the flip and the clip: the four
 *   corners through fwd in double, min and max per axis, truncated toward zero (this project's definition).
 * vrnet_augment_post_radar_f32: radar (B, 4, H, W), a finished radar input -> out (B, 4, H, W), out != radar: the nearest walk,
 *   0.0 outside (this project's definition). */
typedef struct vrnet_aug_post_rec {
  int blur, rotate;                  /* != 0: blur the canvas; rotate canvas, label map, radar map and boxes */
  int angle, reserved;               /* the reference's `rotation` in degrees, judged against max_angle */
  double inv[6], fwd[6];             /* data.rotation_matrices: the map warpAffine walks, and the one the boxes take */
} vrnet_aug_post_rec;                /* 112 bytes; the table must be 8-byte aligned */
int vrnet_augment_post_frames_u8(const unsigned char* canvas, const vrnet_aug_rec* aug, const vrnet_aug_post_rec* post, int B,
                                 int ihm, int iwm, int H, int W, int max_angle, unsigned char* canvas_out, float* images,
                                 int* flag, void* stream);
int vrnet_augment_post_seg_targets_i64(const long long* png, const vrnet_aug_post_rec* post, int B, int H, int W,
                                       int num_classes_seg, int max_angle, long long* png_out, float* onehot, int* flag,
                                       void* stream);
int vrnet_augment_post_box_targets_f32(const int* boxes, const int* counts, const vrnet_aug_rec* aug,
                                       const vrnet_aug_post_rec* post, int B, int max_gt, int ihm, int iwm, int H, int W,
                                       int max_angle, float* targets, int* counts_out, int* flag, void* stream);
int vrnet_augment_post_radar_f32(const float* radar, const vrnet_aug_post_rec* post, int B, int H, int W, int max_angle,
                                 float* out, int* flag, void* stream);

/* ---- Mosaic on the device (csrc/mosaic.hip) ----------------------------------------------------------------------------------
 * Added within ABI 11: new symbols and one new record layout (vrnet_mosaic_rec, with its vrnet_mosaic_tile) only, no existing
 * signature, layout or kernel behaviour changed; hip.py binds every declared symbol at import.
 * The four-tiles-into-one-canvas augmentation of utils/dataloader.py:251-426 (get_random_data_with_Mosaic, merge_bboxes),
 * applied consistently to the frames, the label maps, the boxes and the radar maps.  Nothing here draws a random number: the
 * host draws one record per OUTPUT image (data.mosaic_params) and the kernels apply it; they equal the host functions
 * data.mosaic_sample / mosaic_boxes / merge_boxes / hsv_jitter bit for bit.  Inputs are S source slots (padded (S, ihm, iwm)
 * frames and label maps, (S, max_gt, 5) boxes, (S, 4, H, W) radar maps), outputs B images; a tile names its source slot, and
 * several tiles, of one output image or of several, may name the same one.  Output image on grid y; its record is read and
 * clamped on the device, tile by tile as a vrnet_aug_rec is (src in -1 .. S - 1, 0 <= cutx <= W, 0 <= cuty <= H besides), and if
 * ANYTHING of it had to be clamped, or a size or window of a present tile is not positive, bit 256 of *flag
 * (VR_FLAG_GEOMETRY; flag may be NULL) is set and that output image is what an empty record gives in every output (grey
 * canvas without the colour stage, label 0, no boxes, radar 0); the other images are unaffected.  A resize that needs more
 * taps than max_taps sets the bit as well.  No host synchronisation; capturable.
 * Quadrants (dataloader.py:393-397): canvas pixel (x, y) belongs to tile 0 when x < cutx and y < cuty, tile 1 when x < cutx and
 * y >= cuty, tile 2 when x >= cutx and y >= cuty, tile 3 when x >= cutx and y < cuty.  With wx = x - dx, wy = y - dy of that tile
 * the pixel is inside when the tile is present (src >= 0) and 0 <= wx < nw, 0 <= wy < nh.  flip mirrors the SOURCE left-right
 * before the resize (:328-344) -- for every tile, where the reference flips only tiles that have boxes.
 * vrnet_mosaic_frames_u8: img (S, ihm, iwm, 3) -> canvas (B, H, W, 3) uint8 and / or images (B, 3, H, W) fp32 normalised as
 *   vrnet_batch_formats_u8 does: inside, Pillow's BICUBIC bytes of the (mirrored) source resized to nw x nh (a pass whose
 *   size does not change is skipped), grey (128) elsewhere; then -- color != 0 -- the colour stage of
 *   vrnet_augment_frames_u8 over the whole canvas (:404-419).  Three launches.  workspace:
 *   vrnet_mosaic_workspace_bytes(B, ihm, iwm, H, W, max_taps) bytes, twice vrnet_letterbox_ragged_workspace's: tables and the
 *   horizontal result are indexed by canvas column / row, one set for the top and one for the bottom half of the canvas
 *   (columns), one for the left and one for the right side (rows).
 * vrnet_mosaic_seg_targets_u8: label (S, ihm, iwm) -> png_out (B, H, W) int64 and onehot (B, H, W, ns + 1) fp32 as
 *   vrnet_seg_targets_ragged_u8 writes them: inside, Pillow's NEAREST pick of the (mirrored) source, 0 elsewhere.
 * vrnet_mosaic_box_targets_f32: boxes (S, max_gt, 5) int32 with counts (S) -> targets (B, max_gt, 5) rows [cx, cy, w, h, cls]
 *   and counts_out (B).  Tile by tile, the source's rows in their order: x1, x2 = iw - x2, iw - x1 when flip; x = x nw / iw +
 *   dx, y = y nh / ih + dy truncated toward zero (vrnet_augment_box_targets_f32's arithmetic); the clip to the canvas; kept
 *   when w > 1 and h > 1 (:371-382); merge_bboxes (:251-295) verbatim at the cut; kept when w > 1 and h > 1 again, which the
 *   reference does not ask.  Kept rows are compacted in that order; of more than max_gt the first max_gt stay and bit 512
 *   (VR_FLAG_BOX_COUNT) is set, as for a source count outside [0, max_gt] (clamped).
 * vrnet_mosaic_radar_f32: radar (S, 4, H, W), each aligned with the letterbox window (lb_*) of its source -> out (B, 4, H, W):
 *   inside, with wx' = flip ? nw - 1 - wx : wx, radar[src][c][lb_dy + ((2 wy + 1) lb_nh) / (2 nh)][lb_dx + ((2 wx' + 1) lb_nw) /
 *   (2 nw)] (integer division), 0 elsewhere.  out != radar; ihm, iwm only judge the record as the other three do. */
typedef struct vrnet_mosaic_tile {
  int src;                           /* the source slot, 0 .. S - 1; -1: no tile (the rest is then not looked at) */
  int ih, iw;                        /* that source's own size inside its (ihm, iwm) slot */
  int nw, nh, dx, dy;                /* the resized tile and where it is pasted; may leave the canvas on every side */
  int flip;                          /* != 0: mirror the SOURCE left-right before the resize */
  int lb_nw, lb_nh, lb_dx, lb_dy;    /* data.letterbox_geometry of the source: the window its stored radar map is aligned with */
} vrnet_mosaic_tile;                 /* 48 bytes */
typedef struct vrnet_mosaic_rec {
  int cutx, cuty;                    /* the cut: 0 <= cutx <= W, 0 <= cuty <= H */
  int color, reserved;               /* != 0: run the colour stage; 0 */
  vrnet_mosaic_tile tile[4];         /* in the reference's tile order (index of :349-360) */
  unsigned char lut[3][256];         /* hue, saturation, value tables of the colour stage */
} vrnet_mosaic_rec;                  /* 976 bytes; the table must be 8-byte aligned */
long vrnet_mosaic_workspace_bytes(int B, int ihm, int iwm, int H, int W, int max_taps);
int vrnet_mosaic_frames_u8(const unsigned char* img, int S, const vrnet_mosaic_rec* mosaic, int B, int ihm, int iwm, int H, int W,
                           int max_taps, unsigned char* canvas, float* images, int* flag, void* workspace,
                           long workspace_bytes, void* stream);
int vrnet_mosaic_seg_targets_u8(const unsigned char* label, int S, const vrnet_mosaic_rec* mosaic, int B, int ihm, int iwm, int H,
                                int W, int num_classes_seg, long long* png_out, float* onehot, int* flag, void* stream);
int vrnet_mosaic_box_targets_f32(const int* boxes, const int* counts, int S, const vrnet_mosaic_rec* mosaic, int B, int max_gt,
                                 int ihm, int iwm, int H, int W, float* targets, int* counts_out, int* flag, void* stream);
int vrnet_mosaic_radar_f32(const float* radar, int S, const vrnet_mosaic_rec* mosaic, int B, int ihm, int iwm, int H, int W,
                           float* out, int* flag, void* stream);

/* ---- the radar map from 4D radar points (csrc/radarmap.hip) ---------------------------------------------------------------
 * Added within ABI 11: new symbols and one new record layout (vrnet_radar_view) only, no existing signature, layout or kernel
 * behaviour changed; hip.py binds every declared symbol at import.
 * The step the reference's data instructions describe and ship no code for: "project 3D point clouds into 2D image plane,
 * then make a numpy matrix with 4 x 512 x 512".  The rule is this project's definition (host statement: data.radar_map), and
 * the kernels equal it bit for bit.  points (B, max_points, 7) fp32 rows x, y, z, f0, f1, f2, f3 -- the position in the radar's
 * frame and the four features in the order of the map's channels; rows at or past the record's count are never read.
 * views: one record per image.  P maps (x, y, z, 1) to homogeneous CONTINUOUS pixel coordinates of the original (ih, iw)
 * frame, source pixel (i, j) covering [i, i + 1) x [j, j + 1) (a calibration with pixel centres on integers adds half of row
 * 2 to rows 0 and 1).  The window nw x nh at (dx, dy) on the (H, W) canvas is the one the frame went through: the letterbox
 * window, the whole canvas, or the window of an augmentation record, which may be larger than the canvas and start at
 * negative offsets; flip mirrors the finished canvas.
 * Per point, in float32, every operation rounded on its own in this order, nothing contracted:
 *   hu = ((P00 x + P01 y) + P02 z) + P03, hv and hw likewise from rows 1 and 2
 *   kept when hw >= min_depth and hw, hu, hv are finite (a NaN anywhere rejects)
 *   u = hu / hw, v = hv / hw (correctly rounded); fx = (u float(nw)) / float(iw), fy = (v float(nh)) / float(ih)
 *   kept when 0 <= fx < nw and 0 <= fy < nh; ix = floor(fx), iy = floor(fy)
 *   X = flip ? W - 1 - dx - ix : dx + ix, Y = dy + iy
 * A kept point covers the pixels (X + ox, Y + oy), |ox|, |oy| <= radius (0..8), that lie inside the canvas and inside the
 * window's extent on the canvas (mirrored under flip); nothing is written outside the window.  Of the points covering a
 * pixel the one with the smallest hw wins, the lowest index among equal hw; out[b][c][Y][X] = f_c of the winner, copied bit
 * for bit, and 0 where no point lands.  out (B, 4, H, W) fp32.  The optional min-max normalisation of the prediction
 * scripts stays vrnet_radar_normalise, chained behind.
 * Three launches: keys (B, H, W) uint64 = ~0; one thread per point, a 64-bit atomic minimum of (bits(hw) << 32 | index) per
 * covered pixel; one thread per pixel resolving the key to the winner's features.  Integer atomics only: the same bytes on
 * every run; every call initialises its keys, so nothing carries over between calls.  No host synchronisation, no
 * allocation, no memset; capturable.  workspace: vrnet_radar_map_workspace(B, H, W) bytes, 8-byte aligned.
 * A record with ih, iw, nw or nh <= 0 gives a zero map for its image and sets bit 256 of *flag (VR_FLAG_GEOMETRY); a count
 * outside [0, max_points] is clamped and sets bit 1024 (VR_FLAG_POINT_COUNT).  flag may be NULL. */
typedef struct vrnet_radar_view {
  int ih, iw;                        /* the original frame the projection is calibrated for */
  int nw, nh, dx, dy;                /* the frame's window in the canvas; may leave the canvas on every side */
  int flip, count;                   /* != 0: mirror the canvas left-right; the image's points */
  float P[12];                       /* the (3, 4) projection, row-major */
} vrnet_radar_view;                  /* 80 bytes; the table must be 8-byte aligned */
long vrnet_radar_map_workspace(int B, int H, int W);
int vrnet_radar_map_f32(const float* points, int max_points, const vrnet_radar_view* views, int B, int H, int W, int radius,
                        float min_depth, float* out, int* flag, void* workspace, long workspace_bytes, void* stream);

/* ---- the radar map from points under a rotation (csrc/radarmap.hip; the record and its judgement: csrc/postrec.h) ----------------
 * Added within ABI 11: one new symbol only, no existing signature, layout or kernel behaviour changed -- vrnet_radar_map_f32
 * writes the bytes it wrote before; hip.py binds every declared symbol at import.
 * vrnet_radar_map_f32 with the rotation of the post stage inside the point pass (host statement: data.radar_map(..., post=)):
 * post is the (B) table of vrnet_aug_post_rec the vrnet_augment_post_* entry points read, 8-byte aligned, 0 <= max_angle <= 45.
 * Only the ROTATION of a record is looked at (a blur does not move a point), and only its forward matrix is applied.  For a
 * record that rotates, after the canvas pixel (X, Y) of a kept point has been computed as above, flip included -- in
 * float64, every operation rounded on its own, left to right as vrnet_augment_post_box_targets_f32 takes fwd, nothing contracted:
 *   rx = (fwd[0] X + fwd[1] Y) + fwd[2], ry = (fwd[3] X + fwd[4] Y) + fwd[5]
 *   X' = floor(rx + 0.5), Y' = floor(ry + 0.5)     (pixel centres on integers, the rounding of the nearest walk)
 *   the point is dropped when (X', Y') is outside the canvas (a NaN counts as outside)
 *   else the rectangle it would cover without the rotation -- already cut to the canvas and to the window's extent, mirrored
 *   under flip -- is translated by (X' - X, Y' - Y) and cut to the canvas once more
 * The square is NOT rotated and neither is the window's border: a translated footprint may cross the rotated image of the
 * border by the footprint's own size.  The winner of a pixel is chosen as before.  Every point moves exactly once, where
 * vrnet_augment_post_radar_f32, the nearest gather of a FINISHED map, drops some isolated one-pixel points and duplicates others.
 * A record with a matrix entry that is not finite or with |angle| > max_angle does not rotate its image and sets bit 256 of
 * *flag (VR_FLAG_GEOMETRY), as in the other post entry points; the view record's own rules hold as above.  post == NULL is
 * vrnet_radar_map_f32.  The same three launches, workspace, key plane and resolve kernel; the point kernel is the same body with
 * the rotation compiled in.  64-bit integer atomic minimum only; no allocation, no memset, no host synchronisation; capturable. */
int vrnet_radar_map_post_f32(const float* points, int max_points, const vrnet_radar_view* views, int B, int H, int W, int radius,
                             float min_depth, const vrnet_aug_post_rec* post, int max_angle, float* out, int* flag,
                             void* workspace, long workspace_bytes, void* stream);

/* ---- the radar readout of the detections (csrc/boxradar.hip; the projection of a point: csrc/radarpoint.h) -------------------
 * Added within ABI 11: two new symbols only, no existing signature, layout or kernel behaviour changed; hip.py binds every
 * declared symbol at import.
 * Per kept detection: the number of radar points inside its box, the nearest of them and their lower median by depth.  The
 * reference has no code for it; the rule is this project's definition (host statement: data.box_radar) and the kernels equal
 * it bit for bit.  points and views as vrnet_radar_map_f32 takes them; of a view record only ih, iw, count and P are read.
 * rows (B, cap, 7) fp32, the first four numbers of a row being top, left, bottom, right in pixels of the ORIGINAL frame (the
 * rows vrnet_detect_finish_f32 writes); kept (B) int32, the rows of each image that count.  Boxes and projected points both
 * live in the original frame, so no window takes part.
 * THE RULE, in float32, every operation rounded on its own in this order, nothing contracted.  Per point i:
 *   hu = ((P00 x + P01 y) + P02 z) + P03, hv and hw likewise from rows 1 and 2
 *   kept when hw >= min_depth and hw, hu, hv are finite (a NaN anywhere rejects)
 *   u = hu / hw, v = hv / hw (correctly rounded); in view when 0 <= u < float(iw) and 0 <= v < float(ih)
 * Per box (t, l, b, rt):
 *   shrink == 1: y0 = t, y1 = b, x0 = l, x1 = rt, the row's own numbers
 *   otherwise:   cy = (t + b) 0.5, cx = (l + rt) 0.5, hy = ((b - t) 0.5) shrink, hx = ((rt - l) 0.5) shrink,
 *                y0 = cy - hy, y1 = cy + hy, x0 = cx - hx, x1 = cx + hx
 *   inside when x0 <= u < x1 and y0 <= v < y1 (a NaN edge contains nothing)
 * The candidates of a box -- kept, in view, inside; a point inside several boxes is a candidate of each -- are ordered by
 * key = bits(hw) << 32 | i: hw is positive and finite, so its bits order as an unsigned integer; equal depths go to the lower
 * index.  counts_out[b][r] = their number; readout_out[b][r][0] = (hw, f0, f1, f2, f3) of the smallest key (the NEAREST),
 * readout_out[b][r][1] = the same of the key of rank (count - 1) / 2 in ascending order (the LOWER MEDIAN by depth).  Feature
 * bits are copied, NaN payloads included; without a candidate all ten numbers are +0.0.  0 < shrink <= 1, min_depth > 0.
 * counts_out (B, cap) int32 and readout_out (B, cap, 2, 5) fp32: EVERY element is written by every call, zeros from row
 * kept[b] on, so no memset is needed and no call depends on an earlier one.
 * Two launches: one thread per point writes (u, v, hw) into three planes of the workspace (12 bytes a point; hw = +0.0 marks
 * a point that is not a candidate of any box); one workgroup of 256 per (row, image) counts the candidates and takes their
 * minimum key (wave shuffles, then LDS), and from three candidates on selects the median exactly by an MSB-first radix select
 * on the 64-bit key, 8 bits a pass with a 256-bin LDS histogram, re-reading the planes: there is no list of candidates, so no
 * capacity at which the answer changes.  Integer atomics only (LDS histogram; the OR into *flag is the one global atomic):
 * the same bytes on every run.  No allocation, no memset, no host synchronisation; capturable.
 * A record with ih or iw <= 0 gives zeros for its image and sets bit 256 of *flag (VR_FLAG_GEOMETRY); a point count outside
 * [0, max_points] is clamped and sets bit 1024 (VR_FLAG_POINT_COUNT); kept[b] outside [0, cap] is clamped and sets bit 512
 * (VR_FLAG_BOX_COUNT).  flag may be NULL.  B < 65536, max_points <= 2^24, cap <= 2^20.
 * workspace: vrnet_box_radar_workspace(B, max_points) bytes (-1 for a shape outside the limits), 8-byte aligned. */
long vrnet_box_radar_workspace(int B, int max_points);
int vrnet_box_radar_f32(const float* points, int max_points, const vrnet_radar_view* views, int B, const float* rows,
                        const int* kept, int cap, float min_depth, float shrink, int* counts_out, float* readout_out, int* flag,
                        void* workspace, long workspace_bytes, void* stream);

/* ---- multi-object tracking of the detections (csrc/track.hip) ------------------------------------------------------------------
 * Added within ABI 11: one new symbol and one new record layout (vrnet_track) only, no existing signature, layout or kernel
 * behaviour changed; hip.py binds every declared symbol at import.
 * Every batch slot b is a STREAM: successive calls bring successive frames of camera b, and a table of max_tracks tracks per
 * stream persists in device memory between the calls.  The reference has no tracker; the rule is this project's definition
 * (host statement: data.track_update) and the kernel equals it bit for bit.
 * table (B, max_tracks) records of 64 bytes, max_tracks in [1, 256]; a free slot is all zeros, so zeroed memory is the reset
 * state.  head (B, 4) int32 per stream: ids handed out so far, live tracks, calls so far, births of this call; zeros at reset.
 * rows (B, cap, 7) fp32 and kept (B) int32 as vrnet_detect_finish_f32 writes them (top, left, bottom, right in pixels of the
 * original frame in front, the class in column 6), cap <= 1024.  box_points (B, cap) int32 and box_radar (B, cap, 2, 5) fp32:
 * the outputs of vrnet_box_radar_f32 for the same rows, both or both NULL.
 * THE RULE, in float32, every operation rounded on its own, nothing contracted.  Per stream, n = kept[b] clamped to [0, cap]:
 *   1 predict  every live slot (id != 0): x[k] = x[k] + v[k], k < 4; with range_age >= 0 the same for x[4] and range_age += 1
 *              (saturating).  A slot whose predicted box is not finite is freed
 *   2 match    a row is VALID when its four coordinates are finite, bottom > top and right > left; its class is column 6
 *              truncated toward zero when inside [-2^31, 2^31), -1 otherwise.  For a live slot and a valid row of its class:
 *              ih = min(b1, b2) - max(t1, t2), iw = min(r1, r2) - max(l1, l2) (min(a, b) = a < b ? a : b, max likewise);
 *              ih > 0 and iw > 0: inter = ih iw, union = ((b1 - t1)(r1 - l1) + (b2 - t2)(r2 - l2)) - inter,
 *              iou = inter / union (correctly rounded); otherwise 0.  A candidate iff iou >= the threshold (equality matches,
 *              a NaN does not).  key = bits(iou) << 32 | (65535 - slot) << 16 | (65535 - row).  Greedy: repeatedly the
 *              candidate of the LARGEST key among unmatched slots and unmatched rows -- the largest IoU, then the lowest slot,
 *              then the lowest row
 *   3 update   a matched (slot, row i), per box component: r = z - x, x = x + gain_pos r, v = v + gain_vel r; hits += 1
 *              (saturating), misses = 0, row = i.  Range, with the radar pair, box_points[b][i] > 0 and a finite
 *              depth = box_radar[b][i][1][0] (the lower median): range_age < 0: x[4] = depth, v[4] = 0; otherwise the same
 *              filter with the range gains; then range_age = 0
 *   4 coast    an unmatched live slot: misses += 1, row = -1; freed (16 zero words) when misses > max_age
 *   5 births   valid unmatched rows in ascending order take the free slots in ascending order, those freed in 1 and 4
 *              included: id = ++head[0], cls, hits = 1, misses = 0, row = i, x[0..3] = z, v = 0, range_age = -1, then the
 *              range as in 3.  A row without a free slot gets id 0 and sets bit 32768 of *flag (VR_FLAG_TRACK_FULL)
 *   6 header   head[1] = live tracks, head[3] = births of this call, head[2] += 1
 * ids_out (B, cap) int32: the id of the track each row matched or started; 0 for an invalid row, a row without a slot and
 * from row kept[b] on: EVERY element is written by every call.  kept[b] outside [0, cap] is clamped and sets bit 512
 * (VR_FLAG_BOX_COUNT).  flag may be NULL.  0 < iou <= 1, 0 <= max_age <= 2^20, every gain in [0, 2].  B < 65536.
 * One launch, grid (B), one workgroup of 256 per stream: slot s in the registers of thread s, the boxes in LDS (about 43 KB),
 * the matching as rounds of mutually-best pairs (the same result: keys are unique) -- per round a sweep of the open pairs,
 * the best key of a slot by wave shuffles, the best key of a row by an integer LDS atomic maximum -- and two exclusive block
 * scans for the births.  No workspace, no IoU matrix in memory, no float atomics (the OR into *flag is the one global
 * atomic): the same bytes on every run.  No allocation, no memset, no host synchronisation; capturable. */
typedef struct vrnet_track {
  int id;              /* 0: a free slot */
  int cls;             /* the class of the track */
  int hits;            /* calls matched since birth, the birth counting 1 */
  int misses;          /* consecutive calls without a match */
  int row;             /* the detection row matched in this call; -1 when coasting */
  int range_age;       /* calls since the last radar update; -1: never */
  float x[5];          /* top, left, bottom, right, range */
  float v[5];          /* their rates, per call */
} vrnet_track;
int vrnet_track_update_f32(const float* rows, const int* kept, int B, int cap, vrnet_track* table, int max_tracks, int* head,
                           int* ids_out, const int* box_points, const float* box_radar, float iou, int max_age, float gain_pos,
                           float gain_vel, float range_gain_pos, float range_gain_vel, int* flag, void* stream);

/* ---- radar points under Mosaic (csrc/mosaic.hip; the projection of a point: csrc/radarpoint.h) ---------------------------------
 * Added within ABI 11: new symbols and one new record layout (vrnet_radar_source) only, no existing signature, layout or kernel
 * behaviour changed; hip.py binds every declared symbol at import.
 * The radar input of B Mosaic images from the POINTS of their S sources (host statement: data.mosaic_radar_map), in place of
 * vrnet_mosaic_radar_f32's gather from finished maps.  points (S, max_points, 7) fp32 rows as vrnet_radar_map_f32 takes them;
 * sources: count and projection per source; mosaic: the (B) record table the other Mosaic kernels read, judged by the same
 * rule with the same S, ihm, iwm, H, W (a record that had to be clamped gives a zero map for its WHOLE output image and sets
 * bit 256, VR_FLAG_GEOMETRY).  For tile t of output image b with src >= 0, every point i < count[src] is projected by
 * vrnet_radar_map_f32's arithmetic with the source's P, the tile's (ih, iw) and its window (nw, nh) to the window pixel
 * (ix, iy); its centre is canvas pixel (dx + (flip ? nw - 1 - ix : ix), dy + iy) -- the SOURCE is mirrored, the window stays --
 * and it covers the pixels within `radius` of the centre that lie inside the window AND inside the tile's quadrant (hence
 * inside the canvas).  A kept point centred outside its quadrant still covers the quadrant's pixels within radius.  Per pixel
 * the covering point with the smallest hw wins, the lowest index among equals; all candidates of a pixel come from the one
 * tile that owns it.  out (B, 4, H, W) receives the winner's four features as bits, 0 where no point lands, where the tile
 * is absent (src = -1) and outside the tile's window.
 * Three launches as vrnet_radar_map_f32: keys (B, H, W) uint64 = ~0; one thread per (output image, tile, point), a 64-bit
 * atomic minimum per covered pixel; one thread per pixel resolving its key through its quadrant's tile.  Integer atomics
 * only: the same bytes on every run; nothing carries over between calls.  No host synchronisation, no allocation;
 * capturable.  workspace: vrnet_mosaic_radar_points_workspace(B, H, W) bytes, 8-byte aligned.  A count outside
 * [0, max_points] of a source that a present tile names is clamped and sets bit 1024 (VR_FLAG_POINT_COUNT); the count of a
 * source no tile names is not read.  radius 0..8, min_depth positive and finite.  flag may be NULL. */
typedef struct vrnet_radar_source {
  int count, reserved;               /* the source's points; 0 */
  float P[12];                       /* the (3, 4) projection of the source's own (ih, iw) frame, row-major */
} vrnet_radar_source;                /* 56 bytes; the table must be 8-byte aligned */
long vrnet_mosaic_radar_points_workspace(int B, int H, int W);
int vrnet_mosaic_radar_points_f32(const float* points, int max_points, int S, const vrnet_radar_source* sources,
                                  const vrnet_mosaic_rec* mosaic, int B, int ihm, int iwm, int H, int W, int radius,
                                  float min_depth, float* out, int* flag, void* workspace, long workspace_bytes, void* stream);

/* ---- class names and scores on the rendered detections (csrc/labels.hip) -----------------------------------------------
 * Added within ABI 11: new symbols only, no existing signature, layout or kernel behaviour changed; hip.py binds every
 * declared symbol at import.
 * yolo.py:198-224: every detection gets its rings (vrnet_render_u8), a filled tag in the class colour and
 * '{} {:.2f}'.format(class name, score) in black on it.  A score in [0, 1] formats to one of 101 strings, so the host
 * rasterises all num_classes x 101 labels once with Pillow (render.LabelAtlas) and the device looks masks up.
 * ATLAS.  blob: the uint8 "L" masks ImageDraw.text would paste (font.getmask2), row-major, back to back, below 2 GiB.
 *   records (n_sizes, num_classes * 101, 8) int32, one per font size and label class * 101 + k: blob offset, mask width,
 *   mask height, mask offset x, mask offset y, label_size width, label_size height, 0.  label_size is (bbox right, bbox
 *   bottom) = font.getbbox(label)[2:4], what draw.textsize (yolo.py:212) returned in the Pillow 9 line.  The kernels do not
 *   trust the tables: a label index is clamped into the records, sides and offsets to 2^14, and a record whose mask does
 *   not lie inside the blob draws its tag without text.
 * vrnet_label_index_f32, yolo.py:157 + 210: rows (B, cap, 7) / kept (B) / offsets (B + 1) = rows_out, kept and offsets of
 *   vrnet_detect_finish[_ragged]_f32 -> label_idx[offsets[b] + r] = class * 101 + k for the kept rows (n_out: the length
 *   of label_idx; nothing else is written).  score = obj * class_conf, one fp32 multiply; k = int('{:.2f}'.format(score)
 *   without its point): the exact value of the fp32 times 100 rounded to nearest, ties to even (0.125 -> 12, 0.375 -> 38),
 *   in integer arithmetic on the bits.  NaN or a score outside [0, 1] is clamped (NaN and negatives to 0, above 1 to 100)
 *   and sets bit 2048 of *flag; a class outside [0, num_classes) takes the clamped class, as the outline colour does,
 *   and sets bit 16 as vrnet_detect_finish_f32 does.  flag may be NULL.
 * vrnet_render_labels_u8: in place on the (B, ih, iw, 3) picture vrnet_render_u8 finished with the same boxes, box_offsets,
 *   box_palette and thickness.  The rows of an image are drawn in order; row i paints (a) its rings, (b) the rectangle
 *   [ox, oy] .. [ox + size_w, oy + size_h], inclusive, clipped, in its colour, with (ox, oy) = (left, top - size_h) if
 *   top - size_h >= 0, else (left, top + 1) (yolo.py:216-223), (c) its mask at (ox + mask offset x, oy + mask offset y) in
 *   black, clipped: per byte v = DIV255(v * (255 - m)), DIV255(a) = ((a + 128) + ((a + 128) >> 8)) >> 8 (Pillow's
 *   fill_mask_L with ink 0).  Per pixel: i* = the highest row whose ring or fill covers it; the base is the colour of i*
 *   for a fill, the byte that is there for a ring or without an i*; then the masks of the rows j >= i* (all rows without
 *   an i*) that cover it with m > 0 apply in ascending j.  Pixels no fill and no text touch keep their bytes.
 *   Grid (pixel blocks, row, image) over each row's rectangle (the bounding box of fill and mask): work follows the label
 *   area.  One thread owns a pixel -- that of the highest row whose rectangle covers it -- and computes its whole final
 *   value from the image's rows in LDS: no racing stores, no floating point, no atomics on pixels, the same bytes on every
 *   run.  At most 1024 rows per image; later rows are ignored and set bit 2, as in vrnet_render_u8.  size_index: the font
 *   size, a row of records.
 * vrnet_render_labels_ragged_u8: the same on padded (B, ihm, iwm, 3) slots with ih, iw and thickness of image b from
 *   geom[b] and its font size from size_index[b] (int32, B entries; -1: no labels for that image; >= n_sizes: none, and
 *   bit 256).  Nothing outside an image is written: the padding stays 0.
 * All three: no allocation, no memset, no host synchronisation; one kernel each, capturable in a graph. */
int vrnet_label_index_f32(const float* rows, const int* kept, const int* offsets, int B, int cap, int num_classes,
                          int* label_idx, int n_out, int* flag, void* stream);
int vrnet_render_labels_u8(unsigned char* picture, int B, int ih, int iw, const int* boxes, const int* box_offsets, int n_rows,
                           const unsigned char* box_palette, int n_box_colors, int thickness, const int* label_idx,
                           const unsigned char* blob, long blob_bytes, const int* records, int num_classes, int n_sizes,
                           int size_index, int* flag, void* stream);
int vrnet_render_labels_ragged_u8(unsigned char* picture, const vrnet_frame_geom* geom, const int* size_index, int B, int ihm,
                                  int iwm, const int* boxes, const int* box_offsets, int n_rows,
                                  const unsigned char* box_palette, int n_box_colors, const int* label_idx,
                                  const unsigned char* blob, long blob_bytes, const int* records, int num_classes, int n_sizes,
                                  int* flag, void* stream);

/* ---- track ids, radar range and closing speed under the rendered detections (csrc/captions.hip) ------------------------
 * Added within ABI 11: new symbols only, no existing signature, layout or kernel behaviour changed; hip.py binds every
 * declared symbol at import.
 * A second tag UNDER every box with what the label atlas cannot hold: '#<track id> <range>m <closing speed>m/s', e.g.
 * '#17 42.5m -1.2m/s', composed on the device from the track table (vrnet_track_update_f32) and the radar readout
 * (vrnet_box_radar_f32).  The reference has nothing like it; the rule is this project's definition (host statements:
 * render.caption_strings, render.fixed_tenths, render.draw_captions_host) and the kernels equal it byte for byte.
 * ALPHABET.  "0123456789.-+#m/s ", 18 glyphs; a glyph code is the index into it.
 * CAPTION RECORD.  12 int32: words 0..7 hold 32 codes as bytes (code i is byte i), word 8 their count n, words 9..11 are 0.
 * GLYPH ATLAS (render.GlyphAtlas).  blob: the uint8 cells, row-major, back to back, below 2 GiB; records (n_sizes, 18, 4)
 *   int32 per font size and code: blob offset, cell width, cell height, 0.  A cell is Pillow's mask of the single glyph in
 *   the union of its advance box and the mask's extent; all cells of a size share one height.  A caption is cells side by
 *   side with integer widths, not Pillow's layout of the whole string (no kerning, no fractional advances).  The kernels do
 *   not trust the tables: n is clamped to 32, a code to 17, a cell side to 2^14, the tag height is that of code 0, and a
 *   record whose cell leaves the blob draws as an empty cell.
 * vrnet_caption_text_f32: ids (B, cap) int32 / kept (B) / offsets (B + 1) as vrnet_track_update_f32 and
 *   vrnet_detect_finish[_ragged]_f32 write them, table (B, max_tracks) vrnet_track, box_points (B, cap) / box_radar
 *   (B, cap, 2, 5) of vrnet_box_radar_f32 -> captions_out[offsets[b] + r] for the kept rows r < kept[b] (n_out: the records
 *   of captions_out; nothing else is written).  ids, table and the readout pair are each optional (NULL); table needs ids;
 *   at least one of ids and the readout.  cap <= 1024, max_tracks <= 256.  Up to three fields, joined by one space:
 *     '#<id>'    with ids, for ids[b][r] > 0, in decimal;
 *     the range  '{:.1f}'.format(rng) + 'm'.  With a table: the lowest slot s of stream b with id == ids[b][r], id != 0 and
 *                row == r; drawn when its range_age >= 0, rng = x[4], the filtered range (also while the radar coasts).
 *                Without a table: box_points[b][r] > 0 and rng = box_radar[b][r][1][0], the lower median.  Valid when rng is
 *                not NaN, its sign bit is clear and k <= 99999; otherwise left out, and bit 65536 of *flag (VR_FLAG_CAPTION);
 *     the speed  '{:+.1f}'.format(rate) + 'm/s', only with a table, a drawn range and rate_scale > 0 (in [0, 1e6]): rate =
 *                v[4] * rate_scale, one fp32 multiply -- rate_scale is the caller's frame rate, the tracker's rates being
 *                per call -- the sign from the sign bit.  Valid when finite and k <= 9999; otherwise left out, bit 65536.
 *   k: the exact value of the fp32 times 10, rounded to nearest with ties to even on the exact binary value, in integer
 *   arithmetic on the bits (what Python's format prints: 0.25 -> 0.2, 0.75 -> 0.8, -0.04 -> -0.0); decimal digits by integer
 *   division.  The longest caption, '#2147483647 9999.9m -999.9m/s', has 29 codes; a row without a field has n = 0.
 *   kept[b] outside [0, cap] is clamped and sets bit 512 (VR_FLAG_BOX_COUNT).  flag may be NULL.
 *   One workgroup of 256 per image: thread s publishes row -> s of its slot into an LDS array with an integer atomic
 *   minimum, so a corrupt table still gives one answer; behind a barrier the threads stride over the rows and format.
 * vrnet_render_captions_u8: in place on the finished (B, ih, iw, 3) picture (outlines, labels), with the boxes, box_offsets
 *   and box_palette vrnet_render_u8 took and captions (n_rows, 12).  The rows of an image are drawn in order.  Row i with
 *   n > 0 codes, W the sum of its cell widths at font size size_index and ch the cell height: (ox, oy) = (left, bottom + 1)
 *   if bottom + ch <= ih - 1, else (left, bottom - ch), left and bottom clamped to +-2^29; it paints [ox, ox + W - 1] x
 *   [oy, oy + ch - 1], clipped, in its class colour (the class clamped into the palette), then its cells left to right in
 *   black: v = DIV255(v * (255 - m)), as vrnet_render_labels_u8 blends.  Text never leaves its own tag, so a pixel's final
 *   value follows from the HIGHEST row whose tag covers it; pixels no tag covers keep their bytes.
 *   Grid (pixel blocks, row, image) over each row's clipped tag: work follows the caption area.  A workgroup stages the tag
 *   rectangles of the image's rows in LDS (16 KiB) and the pen positions of its own row; a thread leaves a pixel a higher
 *   row's tag covers, otherwise it writes the pixel once.  No racing stores, no floating point, no atomics on pixels.  At
 *   most 1024 rows per image; later rows are ignored and set bit 4, as in vrnet_render_u8.
 * vrnet_render_captions_ragged_u8: the same on padded (B, ihm, iwm, 3) slots with ih, iw of image b from geom[b] and its
 *   font size from size_index[b] (int32, B entries; -1: no captions for that image; >= n_sizes: none, and bit 256).
 *   Nothing outside an image is written.
 * All three: no allocation, no memset, no host synchronisation; one kernel each, capturable in a graph. */
int vrnet_caption_text_f32(const int* ids, const int* kept, const int* offsets, int B, int cap, const vrnet_track* table,
                           int max_tracks, const int* box_points, const float* box_radar, float rate_scale, int* captions_out,
                           int n_out, int* flag, void* stream);
int vrnet_render_captions_u8(unsigned char* picture, int B, int ih, int iw, const int* boxes, const int* box_offsets, int n_rows,
                             const unsigned char* box_palette, int n_box_colors, const int* captions, const unsigned char* blob,
                             long blob_bytes, const int* records, int n_sizes, int size_index, int* flag, void* stream);
int vrnet_render_captions_ragged_u8(unsigned char* picture, const vrnet_frame_geom* geom, const int* size_index, int B, int ihm,
                                    int iwm, const int* boxes, const int* box_offsets, int n_rows,
                                    const unsigned char* box_palette, int n_box_colors, const int* captions,
                                    const unsigned char* blob, long blob_bytes, const int* records, int n_sizes, int* flag,
                                    void* stream);

/* ---- detection crops (csrc/crops.hip) -----------------------------------------------------------------------------------
 * Added within ABI 11: a new symbol and one new record layout (vrnet_crop_rec) only, no existing signature, layout or kernel
 * behaviour changed; hip.py binds every declared symbol at import.
 * yolo.py:180-193, the `crop` switch of detect_image: every kept detection is cut out of the ORIGINAL frame (the reference
 * crops before it draws) and saved.  Here the crops of a batch go into one packed arena on the device; the host statement
 * is render.crop_boxes_host / render.crop_layout, and the kernels equal it bit for bit.
 * vrnet_crop_boxes_u8: frames (B, ihm, iwm, 3) u8 slots with image b in the top-left corner of slot b, of size geom[b].ih x
 *   geom[b].iw (clamped to the slot; a clamped or empty record sets bit 256) or ihm x iwm with geom == NULL; rows (n_cap, 5)
 *   int32 = left, top, right, bottom, class and offsets (B + 1) as vrnet_detect_finish[_ragged]_f32 leave them.  N =
 *   offsets[B] clamped to [0, n_cap]; the offsets are made monotone (c[0] = 0, c[i] = min(N, max(0, offsets[0..i]))) and row n
 *   belongs to the image b with c[b] <= n < c[b + 1], so a hostile table indexes nothing outside.
 *   Row n is clamped again, l = max(left, 0), t = max(top, 0), r = min(right, iw), bt = min(bottom, ih), w = r - l, h = bt - t.
 *   w <= 0 or h <= 0: an EMPTY crop, table[n] = {0, 0, 0, b}, nothing copied (Pillow gives a zero-size image for w == 0 or
 *   h == 0 and raises for right < left; the reference would crash on saving either).  Otherwise the crop is
 *   frame[t:bt, l:r, :], bit for bit np.array(image.crop([left, top, right, bottom])), one contiguous (h, w, 3) block at
 *   arena + 3 offset, offset = the sum of a over ALL earlier rows, a = w h rounded up to a multiple of 4 (0 for an empty
 *   row), in 64 bits: every crop starts on a 4-byte boundary, and the up to 3 pad pixels behind it are zero bytes, so the
 *   used prefix of the arena is the same bytes on every run.  A non-empty row with offset + a > capacity_px is DROPPED:
 *   table[n] = {-1, w, h, b} and bit 4096 of *flag (VR_FLAG_CROP_ARENA) is set; the sum runs over all rows, so every later
 *   non-empty row is dropped too: what is kept is a prefix.  table[n] = {0, 0, 0, -1} for N <= n < n_cap.  summary = (N, used),
 *   used = the pixels in use (the sum of a over the kept rows); arena bytes at or beyond 3 used are not written.
 *   Two launches: the layout (one workgroup, chunked prefix sums with a running 64-bit base) and the copy (a fixed number of
 *   workgroups per row of the table; one that finds its row empty or dropped leaves at once, the others store each aligned
 *   dword of the crop's block once, its four bytes gathered from the frame: work follows the crop area).  The grid depends
 *   on n_cap alone.  No allocation, no memset, no host synchronisation; capturable in a graph.
 *   0 < B < 65536, 0 < n_cap <= 2^20, 0 < capacity_px <= 2^30, ihm iwm < 2^31; arena (3 capacity_px bytes) and table 4-byte
 *   aligned; flag may be NULL. */
typedef struct vrnet_crop_rec {
  int offset;                        /* the crop's first pixel in the arena; 0 if empty, -1 if dropped */
  int w, h;                          /* 0, 0: an empty crop */
  int image;                         /* the image the row belongs to; -1 behind the last row */
} vrnet_crop_rec;                    /* 16 bytes */
int vrnet_crop_boxes_u8(const unsigned char* frames, int B, int ihm, int iwm, const vrnet_frame_geom* geom, const int* rows,
                        const int* offsets, int n_cap, unsigned char* arena, long capacity_px, vrnet_crop_rec* table,
                        int* summary, int* flag, void* stream);

/* ---- fixed-size detection chips (csrc/chips.hip) ---------------------------------------------------------------------------
 * Added within ABI 11: two new symbols and one new record layout (vrnet_chip_rec) only, no existing signature, layout, flag
 * bit or kernel behaviour changed; hip.py binds every declared symbol at import.
 * resize_image, utils/utils.py:19-32, the reference's way to bring any picture to a fixed size, applied to every crop of
 * yolo.py:180-193: one tensor of equal-sized pictures for a second stage.  The host statement, with Pillow itself, is
 * render.chip_boxes_host / render.chip_geometry, and the kernels equal it bit for bit.
 * vrnet_chip_boxes_u8: frames, geom, rows, offsets, n_cap, N, the image of a row and its clamp l, t, w, h exactly as
 *   vrnet_crop_boxes_u8 takes and makes them (a clamped or empty geom record sets bit 256 of *flag; no other bit is set).
 *   Chip n belongs to row n.  w <= 0 or h <= 0: the chip is all grey 128, table[n] = {b, 0, 0, 0, 0, 0, 0, 2}.  Otherwise
 *   letterbox == 0: the chip is image.crop((l, t, r, bt)).resize((sw, sh), BICUBIC) -- crop THEN resize, the taps stop at the
 *   crop's edge -- and nw, nh, dx, dy = sw, sh, 0, 0.  letterbox != 0: scale = min(sw / w, sh / h) in doubles, nw =
 *   max(int(w scale), 1), nh = max(int(h scale), 1) (the max is a departure: the reference lets Pillow raise on nh = 0), the
 *   crop resized to (nw, nh) and pasted at dx, dy = (sw - nw) / 2, (sh - nh) / 2 on grey 128.  table[n] = {b, w, h, nw, nh,
 *   dx, dy, 1}.  The bytes are Pillow's: Resample.c's windows and 22-bit weights, the horizontal pass rounded to bytes before
 *   the vertical one; a pass whose size does not change is the identity.
 *   chips (n_cap, sh, sw, 3) u8; chips_f32 (n_cap, 3, sh, sw) or NULL: the same bytes as ((v / 255) - mean) / std in double,
 *   rounded once, the network's input.  table[n] = {-1, 0, 0, 0, 0, 0, 0, 0} for N <= n < n_cap, and chips and float chips
 *   of those rows are NOT written: the work follows the row count.  summary (1) = N.
 *   workspace: vrnet_chip_workspace(n_cap, sh, sw) bytes (16 (sh + sw) a row: per output index of each axis the window and
 *   the sum of its bicubic values, from which every thread recomputes any integer weight; no tap capacity, no intermediate
 *   picture), 8-byte aligned; -1 for sizes outside the limits.
 *   Two launches whose grids depend on n_cap, sh and sw alone: the tables (one workgroup per row) and the resample (one
 *   workgroup per row and band of 8 chip rows, which streams the band's source rows in chunks of at most 16 through LDS; one behind
 *   the last row leaves at once).  No allocation, no memset, no host synchronisation; capturable in a graph.
 *   0 < B < 65536, 0 < n_cap <= 2^20, 1 <= sh, sw <= 256, ihm iwm < 2^31; table and chips_f32 4-byte aligned; flag may be
 *   NULL. */
typedef struct vrnet_chip_rec {
  int image;                         /* the image the row belongs to; -1 behind the last row */
  int w, h;                          /* the clamped crop; 0, 0: an empty crop */
  int nw, nh, dx, dy;                /* the resized crop and where it is pasted in the chip */
  int state;                         /* 1 resized, 2 empty (a grey chip), 0 behind the last row (not written) */
} vrnet_chip_rec;                    /* 32 bytes */
long vrnet_chip_workspace(int n_cap, int sh, int sw);
int vrnet_chip_boxes_u8(const unsigned char* frames, int B, int ihm, int iwm, const vrnet_frame_geom* geom, const int* rows,
                        const int* offsets, int n_cap, int sh, int sw, int letterbox, unsigned char* chips, float* chips_f32,
                        vrnet_chip_rec* table, int* summary, void* workspace, int* flag, void* stream);

/* ---- baseline JPEG (csrc/jpeg.hip) ------------------------------------------------------------------------------------------
 * Added within ABI 11: two new symbols and one new flag bit only, no existing signature, layout or kernel behaviour changed.
 * Every image of a batch to a complete baseline JFIF file, every byte the one Pillow (libjpeg-turbo) writes for
 * Image.save(format="JPEG", quality=q, subsampling=0 or 2).  The rule is stated on the host by render.jpeg_encode_host (integer
 * colour conversion, edge replication, the 4:2:0 box reduction with its alternating bias and its dummy blocks, jfdctint,
 * rounding quantisation, the Annex K Huffman tables, one DC predictor per component, byte stuffing) and at the top of
 * csrc/jpeg.hip, and the kernels equal it byte for byte.
 * vrnet_jpeg_encode_u8: images (B, H, W, 3) u8 RGB.  The size (h, w) of image b, in the top-left corner of its slot, is
 *   geom[b].ih, iw, or sizes[2 b], sizes[2 b + 1] ((B, 2) int32), or H, W when both are NULL (at most one of the two may be
 *   given); it is clamped to the slot, which sets bit 256 of *flag (VR_FLAG_GEOMETRY), and an image without pixels gets the
 *   record (0, 3).  subsampling: 0 (4:4:4) or 2 (4:2:0).  header: the 623 bytes in front of the scan data on the device
 *   (render.jpeg_header), whose two DQT segments are the quantisation tables the kernels use; height and width (bytes
 *   163..166) are written per image.  arena (B, capacity) u8: slot b holds the file in its first record[2 b] bytes; bytes
 *   behind that are not defined.  record (B, 2) int32 = (length, state): state 1 a complete file; 2 the file did not fit
 *   capacity: length 0, bit 262144 of *flag (VR_FLAG_JPEG_ARENA), the other images unaffected; 3 no pixels.
 *   workspace: vrnet_jpeg_workspace_bytes(B, H, W, subsampling, capacity) bytes, 16-byte aligned (-1: a bad shape): the int16
 *   coefficients in scan and zigzag order (128 bytes a block), a bit offset per block, and the unstuffed bit stream
 *   (capacity bytes an image).  Eight launches (blocks, lengths, scan, zero, emit, count, scan, pack), no host
 *   synchronisation, no allocation, integer atomics only: the same bytes on every run.  Bit offsets are 32-bit, which the
 *   limit of 2^20 blocks a slot (at most 1658 bits each) guarantees.
 *   0 < B < 65536, 1 <= H, W <= 65535, 625 <= capacity < 2^31 - 64; flag may be NULL. */
long vrnet_jpeg_workspace_bytes(int B, int H, int W, int subsampling, long capacity);
int vrnet_jpeg_encode_u8(const unsigned char* images, int B, int H, int W, const vrnet_frame_geom* geom, const int* sizes,
                         int subsampling, const unsigned char* header, unsigned char* arena, long capacity, int* record, int* flag,
                         void* workspace, long workspace_bytes, void* stream);

/* ---- connected regions of the class map (csrc/regions.hip) -----------------------------------------------------------------
 * Added within ABI 11: two new symbols, one new record layout (vrnet_region) and one new flag bit only, no existing signature,
 * layout or kernel behaviour changed; hip.py binds every declared symbol at import.
 * The reference stops at the class map and the boxes; this is the join between them -- how many separate vessels or piers the
 * class map holds, where each lies, how large it is, and which detection row belongs to which of them.  The rule is this
 * project's definition; the host statement is decode.seg_regions_host and the kernels equal it bit for bit.  THE RULE for one
 * image of size (ih, iw):
 *   Pixels of class `background` are unlabelled (background = -1: every class is labelled).  A region is a maximal set of
 *   pixels of ONE class connected under `connectivity`, 4 or 8.  A region of fewer than min_area pixels is dropped and its
 *   pixels get label 0.  The remaining n regions get the ids 1..n in the order of their first pixel in raster order, the
 *   smallest y iw + x.
 *   labels: the id of every kept region at each of its pixels, ids beyond max_regions included: no capacity changes it.
 *   table: the record of id k at table[k - 1] for k = 1..min(n, max_regions), zeros behind.  right and bottom are exclusive,
 *   first = y iw + x of the first pixel, sum_x and sum_y the exact integer sums of the pixel coordinates.
 *   head = (n, min(n, max_regions), the pixels in kept regions, the non-background pixels dropped by min_area).
 *   n > max_regions sets bit 131072 of *flag (VR_FLAG_REGIONS).
 *   The link, over the records of the table and the rows of the image: a row left, top, right, bottom is clamped to the image
 *   (each coordinate to [0, iw] or [0, ih], as vrnet_crop_boxes_u8 clamps it) and is EMPTY with right <= left or bottom <=
 *   top; an empty row links to nothing.  A row and a record's bounding box have the integer intersection I and union U; the
 *   best partner is the one with the largest I / U, compared as I1 U2 against I2 U1 in 64 bits (both below 2^63 after the
 *   clamp), I > 0 required, ties to the lowest index.  det of a record: the index of its best row within the image, or -1.
 *   box_regions of a row: the id of its best record, or 0.  With det_to_seg (n_det entries, one seg class per detection class)
 *   a row of class c links only with records of class det_to_seg[c] and the other records ignore it; c outside [0, n_det)
 *   links to nothing.
 * vrnet_seg_regions_u8: class_map (B, ihm, iwm) u8 slots with image b in the top-left corner of slot b, of size geom[b].ih x
 *   geom[b].iw (clamped to the slot; a clamped or empty record sets bit 256 and an empty image has no region) or ih x iw with
 *   geom == NULL (ih <= ihm, iw <= iwm); rows (n_cap, 5) int32 and offsets (B + 1) as vrnet_detect_finish[_ragged]_f32 leave
 *   them, made monotone as vrnet_crop_boxes_u8 does; of the rows of an image the first `cap` take part.  labels (B, ihm, iwm)
 *   int32, 0 outside the image; table (B, max_regions) vrnet_region, 8-byte aligned; head (B, 4) int32; box_regions (B, cap)
 *   int32, 0 from the image's row count on; det_to_seg (n_det) int32 in device memory or NULL with n_det = 0; flag may be NULL.
 *   Every element of every output is written on every call.
 *   Seven launches (six for a slot of one tile): a 64 x 16 tile labelled in LDS by union-find with the integer atomic minimum,
 *   one union per pair of touching runs, which also initialises everything the call accumulates into; the lock-free
 *   atomicMin union across tile edges and corners on an int32 parent plane, whose `find` reads with relaxed agent-scope
 *   atomic loads (the root is the smallest index of the component, so the result does not depend on the order of arrival);
 *   the roots and the areas; the kept roots per chunk of 2048 pixels; their ranks; the labels and the statistics, gathered per
 *   run of a wave and per tile in LDS before one integer atomic per id, tile and field; the link and the header, eight
 *   workgroups per image.  No workgroup waits for another.  Integer atomics only: the same bytes on every run.  No
 *   allocation, no memset node, no host synchronisation; capturable in a graph.
 *   connectivity 4 or 8, background in [-1, 255], min_area >= 1, 1 <= max_regions <= 4096, 0 <= n_det <= 256; 0 < B < 65536,
 *   ihm, iwm <= 2^17, ihm iwm < 2^31; 0 < n_cap, cap <= 2^20.
 * vrnet_seg_regions_workspace_bytes: the bytes of `workspace` (-1 for a shape outside the limits): two int32 planes of
 *   B ihm iwm and four int32 per chunk of 2048 pixels. */
typedef struct vrnet_region {
  int cls, area;                     /* the class of the region's pixels and their number */
  int left, top, right, bottom;      /* the bounding box, right and bottom exclusive */
  int first;                         /* y iw + x of the first pixel in raster order */
  int det;                           /* the linked row of the image, -1: none */
  long long sum_x, sum_y;            /* exact sums of the pixel coordinates: the centroid is sum / area */
} vrnet_region;                      /* 48 bytes */
long vrnet_seg_regions_workspace_bytes(int B, int ihm, int iwm);
int vrnet_seg_regions_u8(const unsigned char* class_map, int B, int ihm, int iwm, const vrnet_frame_geom* geom, int ih, int iw,
                         const int* rows, const int* offsets, int n_cap, int cap, int connectivity, int background, int min_area,
                         int max_regions, const int* det_to_seg, int n_det, int* labels, vrnet_region* table, int* head,
                         int* box_regions, int* flag, void* workspace, long workspace_bytes, void* stream);

/* ---- dark-channel dehazing (csrc/dehaze.hip) ------------------------------------------------------------------------------
 * Added within ABI 11: two new symbols only, no existing signature, layout or kernel behaviour changed.
 * He et al.'s dark-channel-prior dehazing, the reference's image_augmentation_test/dark_channel.py restated; the host
 * statement is render.dehaze_host and the kernels equal it bit for bit.  THE RULE for one (ih, iw, 3) uint8 RGB image; every
 * float64 operation is rounded on its own in the order written, nothing is contracted, divisions are IEEE:
 *   I_c   = double(byte_c) / 255.0.
 *   d8    = min over c of byte_c; dark8 = the minimum of d8 over the sz x sz window centred on the pixel (sz odd), positions
 *           outside the image ignored (cv2.erode's default border); uint8 (the reference's d8 / 255 orders identically).
 *   numpx = max(ih iw / 1000, 1) in integers.  The pixels in ascending order of (dark8, flat index y iw + x) -- a stable
 *           ascending argsort, one valid outcome of the reference's unordered ties --: the last numpx of them without the first
 *           of those (the reference's range(1, numpx)); S_c = the INTEGER sum of byte_c over these numpx - 1 pixels (the
 *           reference adds floats sequentially: rounding only, and this is order-free); A_c = (double(S_c) / 255.0) / double(numpx).
 *   m     = min over c of (I_c / A_c);  te = 1.0 - omega * (the same windowed minimum of m).
 *   g8    = (4899 R + 9617 G + 1868 B + 8192) >> 14 (OpenCV's 8-bit BGR2GRAY);  g = double(g8) / 255.0.
 *   box(p): cv2.boxFilter(p, CV_64F, (r, r)), normalised, anchor o = r / 2, REFLECT_101: refl(i, n) = |i| if |i| < n, else
 *           2 (n - 1) - |i|;  h(y, x) = p(y, refl(x - o, iw)), then += p(y, refl(x - o + j, iw)) for j = 1 .. r - 1 in that
 *           order; the same over the rows of h; then / double(r r).  The fixed tap order makes it reproducible.
 *   mI = box(g), mp = box(te), mIp = box(g * te), mII = box(g * g);  a = (mIp - mI * mp) / ((mII - mI * mI) + eps);
 *   b = mp - a * mI;  t = box(a) * g + box(b).
 *   J_c = (I_c - A_c) / max(t, tx) + A_c;  v = J_c * 255.0;  byte = clip(rint(v), 0, 255), half to even (the saturate_cast
 *   cv2.imwrite applies).
 *   DEGENERATE: any A_c == 0 (numpx == 1 included, where nothing is summed), or r / 2 > min(ih, iw) - 1 (the size allows no
 *   single reflection).  A degenerate image comes back UNCHANGED with t = 1 and sets bit 8192 of *flag (VR_FLAG_DEHAZE); the
 *   other images of the batch are unaffected.
 * The OpenCV semantics above are restated from its published behaviour and have never been run against cv2.
 * vrnet_dehaze_u8: frames (B, ihm, iwm, 3) u8; out the same shape, a different buffer (frames is not modified);
 *   transmission (B, ihm, iwm) f64 or NULL; flag may be NULL; geom the per-image table of the ragged batches, or NULL when
 *   every image fills its slot.  With a table image b is the geom[b].ih x geom[b].iw top-left corner of its slot and
 *   everything outside the corner is written 0 in out and transmission; a record with ih, iw <= 0 or above the slot sets
 *   bit 256 (VR_FLAG_GEOMETRY) and gives a zero image.  One kernel body for both cases.
 *   sz odd in 1..31, 2 <= r <= 128, eps > 0 (finite), 0 < omega <= 1, 0 < tx <= 1; 0 < B < 65536, ihm, iwm <= 2^17,
 *   ihm iwm <= 2^26, B ihm iwm <= 2^31; workspace and transmission 8-byte aligned.
 *   Eleven launches (init, dark channel + histogram, threshold bin, per-chunk counts of the bin, ranked integer sums, A and
 *   the degenerate decision, transmission estimate, box rows of g / te / g te / g g, box columns fused with a and b, box rows
 *   of a and b, box columns fused with t, the recovery and the byte store).  Every call initialises what it accumulates
 *   into; integer atomics only (the histogram and the sums): the same bytes on every run.  No allocation, no memset node,
 *   no host synchronisation; capturable in a graph.
 * vrnet_dehaze_workspace_bytes: the bytes of `workspace` (-1 for a shape outside the limits): seven float64 planes of
 *   B ihm iwm, one byte plane and small tables.  After the call its first 32 B bytes hold, per image, the doubles
 *   A_r, A_g, A_b and 1.0 for a degenerate or bad image (else 0.0). */
long vrnet_dehaze_workspace_bytes(int B, int ihm, int iwm);
int vrnet_dehaze_u8(const unsigned char* frames, const vrnet_frame_geom* geom, int B, int ihm, int iwm, int sz, int r, double eps,
                    double omega, double tx, unsigned char* out, double* transmission, int* flag, void* workspace,
                    long workspace_bytes, void* stream);

/* ---- ACE de-rain enhancement (csrc/ace.hip) -------------------------------------------------------------------------------
 * Added within ABI 11: two new symbols only, no existing signature, layout or kernel behaviour changed.
 * The fast Automatic Colour Equalisation of the reference's image_augmentation_test/sharpen.py restated; the host statement is
 * render.ace_host and the kernels equal it byte for byte.  THE RULE for one (ih, iw, 3) uint8 image, each channel on its own;
 * every float64 operation is rounded on its own in the order written, nothing is contracted, divisions are IEEE.
 * Parameters: ratio (4.0), radius (3), s (0.005), bins (2000).
 *   I0 = double(byte) / 255.0.
 *   weights: computed on the host and passed as data, (2 radius + 1)^2 doubles: m[dy, dx] = 1.0 / sqrt(dy^2 + dx^2), the
 *     centre 0, then m /= m.sum() in numpy's own summation (render.ace_weights).
 *   ice(P), P of (h, w): res = 0.0; for dy = -radius .. radius and, inside it, dx = -radius .. radius, skipping the centre:
 *     res += m[dy, dx] * clip((P(y, x) - P(cy, cx)) * ratio, -1, 1), cy = clamp(y + dy, 0, h - 1), cx clamped likewise: edge
 *     replication of P itself.
 *   resize(S, h, w): cv2's default INTER_LINEAR resize on float64.
 *     Halving case: the source is exactly (2 h, 2 w) -- OpenCV's exact-halving switch to the fast area path:
 *       out = (((S00 + S01) + S10) + S11) * 0.25 over each 2 x 2 block.
 *     Two-tap case, otherwise; per axis, destination index d, source length n, destination length k:
 *       scale = double(n) / double(k);  f = float((d + 0.5) * scale - 0.5), computed in double and rounded to float once;
 *       s0 = floor(f), then f -= s0 in float;  s0 < 0: s0 = 0, f = 0;  s0 >= n - 1: s0 = n - 1, f = 0;
 *       s1 = min(s0 + 1, n - 1);  the weights a0 = double(1.f - f), a1 = double(f).
 *       Columns first: H(y, x) = S(y, x0) * a0 + S(y, x1) * a1;  then rows: out = H(y0, x) * b0 + H(y1, x) * b1.
 *   The pyramid: I_0 = I0;  I_{L+1} = resize(I_L, (h_L + 1) / 2, (w_L + 1) / 2) while min(h_L, w_L) > 2.  At the first level
 *     with min <= 2, R = 0.5 everywhere.  Above it R_L = (resize(R_{L+1}, h_L, w_L) + ice(I_L)) - ice(resize(I_{L+1}, h_L, w_L)).
 *     The up-resized constant bottom goes through the resize formula like any plane (0.5 a0 + 0.5 a1 is not always 0.5).
 *   The stretch (the reference's stretchImage): first, last = the minimum and maximum of R_0, widened by 0.5 each way when
 *     equal;  step = (last - first) / bins;  edge(i) = i * step + first, edge(bins) = last.  The bin of a value v:
 *     idx = int(((v - first) / (last - first)) * bins);  idx == bins: idx -= 1;  v < edge(idx): idx -= 1;
 *     v >= edge(idx + 1) and idx != bins - 1: idx += 1 -- numpy's uniform-bin rule, np.histogram(R_0, bins).
 *     d(i) = double(cumulative count) / double(ih iw);  lmin = the first i with d(i) >= s;  lmax = the last i with
 *     d(i) <= 1.0 - s, or -1 if there is none;  out = clip((R_0 - edge(lmin)) / (edge(lmax) - edge(lmin)), 0, 1);
 *     byte = clip(rint(out * 255.0), 0, 255), half to even.
 *   DEGENERATE: min(ih, iw) <= 2, or lmax <= lmin in any channel (a constant frame whose R_0 is exactly 0.5: lmin = 1000,
 *     lmax = 999 at the defaults; the reference would write a black picture).  All three channels of a degenerate image come
 *     back UNCHANGED and bit 16384 of *flag (VR_FLAG_ACE) is set; the other images of the batch are unaffected.  A constant
 *     frame of a size whose up-resize fractions are not exact in float32 has an R_0 that differs from 0.5 in its last bits;
 *     by the rule it is not degenerate, and the stretch spreads those bits over the byte range.
 * The OpenCV resize semantics above are restated from its published behaviour and have never been run against cv2.
 * vrnet_ace_u8: frames (B, ihm, iwm, 3) u8; out the same shape, a different buffer (frames is not modified); weights the
 *   (2 radius + 1)^2 doubles above in DEVICE memory, 8-byte aligned; flag may be NULL; geom the per-image table of the ragged
 *   batches, or NULL when every image fills its slot.  With a table image b is the geom[b].ih x geom[b].iw top-left corner
 *   of its slot and everything outside the corner is written 0; a record with ih, iw <= 0 or above the slot sets bit 256
 *   (VR_FLAG_GEOMETRY) and gives a zero image.  One kernel body for both cases: the grids follow (B, ihm, iwm) alone, every
 *   image derives its level sizes from its own record, workgroups beyond an image's level or at its bottom leave at once.
 *   radius in 1..8, ratio > 0 (finite), 0 <= s < 0.5, bins in 2..4096; the shape limits of vrnet_dehaze_u8.
 *   2 N + 4 launches, N being the levels above the bottom of the SLOT's pyramid (N = 10 at 1080 x 1920: 24 launches): init,
 *   N down-resizes, N level launches (per 32 x 32 tile and channel the tiles of I_L and of resize(I_{L+1}) with a halo of
 *   radius in LDS, both tap sums from LDS with the weights through the scalar cache, resize(R_{L+1}) at the pixel, no
 *   full-size plane of either up-resized operand; one instance per radius; level 0 also the minimum and maximum of R_0 through
 *   an order-preserving 64-bit integer key and integer atomics), the histogram, the cumulative scan with both thresholds,
 *   the stretch with the byte store.  Every call initialises what it accumulates into; integer atomics only: the same bytes
 *   on every run.  No allocation, no memset node, no host synchronisation; capturable in a graph.
 * vrnet_ace_workspace_bytes: the bytes of `workspace` (-1 for a shape outside the limits): R_0 and, for every deeper level of
 *   the slot's pyramid, I_L and R_L as float64 (about 5 / 3 x 24 B ihm iwm bytes), and 48 KB of histogram bins per image. */
long vrnet_ace_workspace_bytes(int B, int ihm, int iwm);
int vrnet_ace_u8(const unsigned char* frames, const vrnet_frame_geom* geom, int B, int ihm, int iwm, int radius, double ratio,
                 double s, int bins, const double* weights, unsigned char* out, int* flag, void* workspace, long workspace_bytes,
                 void* stream);


#ifdef __cplusplus
}
#endif
#endif /* VRNET_HIP_H */
