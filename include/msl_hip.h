/*
 * msl_hip.h — C-ABI of libmsl_hip.so, the MI355X (gfx950) kernels behind the
 * DeepLabv2/ResNet-101 MaxSquare domain-adaptation training step.
 *
 * The reference (shiyutang/MaxSquareLoss) has no native code and no FFI: its
 * boundary is the Python/nn.Module API.  Every entry point
 * below replaces one implicit ATen/cuDNN op of that API; the reference site it
 * stands in for is cited next to it (paths relative to the reference root).
 *
 * Conventions (all entry points):
 *   - Tensors are fp32 NCHW with N = 1 (bs = 1 per GPU), i.e.
 *     a [C][H][W] block; labels are int64 with -1 = ignore.
 *   - All pointers are caller-owned device pointers (the PyTorch caching
 *     allocator on the Python side).  The library allocates nothing; scratch
 *     comes from the caller's workspace, sized by the matching *_workspace()
 *     query, and no call leaves state that a later call reads.
 *   - No process state (ABI 3): the kernel FORMS of a call - which matrix-core
 *     form, schedule or BN kernel runs, not what the result means - come with
 *     the call as a const msl_forms* (NULL = the defaults), read on the host
 *     at launch time, so a captured hipGraph keeps the forms of its capture.
 *   - Work is enqueued on the given hipStream_t (passed as msl_stream_t) and
 *     is stream-ordered; no entry point synchronises the host, so every call
 *     is safe to capture in a hipGraph.
 *   - Return value: 0 = MSL_OK, < 0 = argument / shape / workspace / launch-bound error
 *     (see msl_status_string), > 0 = the hipError_t of a failed launch.
 */
#ifndef MSL_HIP_H
#define MSL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* msl_stream_t; /* a hipStream_t */

#define MSL_OK 0
#define MSL_ERR_SHAPE (-1)
#define MSL_ERR_WORKSPACE (-2)
#define MSL_ERR_ARG (-3)
/* a launch whose block exceeds the kernel's __launch_bounds__: refused on the host, before the launch (r06).
 * An entry point that issues several launches may already have enqueued its earlier stages when a later
 * one is refused: after this status the call's outputs and workspace are undefined. */
#define MSL_ERR_LAUNCH (-4)

int msl_abi_version(void);
const char* msl_status_string(int status);

/* The kernel forms of a call (ABI 3: replaces ABI 2's process-wide setters msl_conv_set_f32_form,
 * msl_conv_set_pack_form, msl_conv_set_sk_hybrid, msl_bn_set_fused and the reserved int* counters
 * argument, which no kernel read).  Every conv, pack and BN entry point takes one; NULL = the
 * defaults {5, 1, 1, 1}.  A bad value is MSL_ERR_ARG.
 *   f32_form  matrix-core form of the fp32 conv entry points (msl_dconv_* / msl_pconv_* without
 *             _bf16 / _f16) and of the packs: 0 = v_mfma_f32_32x32x2_f32 (exact fmaf chain), 2 = each
 *             fp32 operand split into three bf16 terms, six products per 16-deep K slice on
 *             v_mfma_f32_32x32x16_bf16 with fp32 accumulation (fp32-accurate), 5 = each operand tensor
 *             scaled by a power of two (its absolute maximum brought to [2^14, 2^15)) and split into
 *             two fp16 terms, three products per slice on v_mfma_f32_32x32x16_f16 with fp32
 *             accumulation, the result unscaled exactly (fp32-accurate: the 3xTF32 scheme at fp16's
 *             11-bit significand; the default).  Packs are form-specific (form 5 writes fp16 planes
 *             and the weights' scale): a conv call must pass the f32_form its pack was made with; the
 *             _f16 entry points need packs made with form 5.  Replaces nothing in the reference (its
 *             convs are cuDNN fp32).
 *   sk_hybrid schedule of the forward-form kernels (fwd and data gradient; same results up to the
 *             fp32 summation order of split tiles): 1 = when the output tiles outnumber the 512
 *             workgroups, whole rounds of tiles run data-parallel and only the remainder is split
 *             stream-K (default); 0 = pure stream-K.
 *   pack_form weight-pack kernel (identical packed bytes either way): 1 = one LDS-transposing
 *             pack+split launch per pack call (default), 0 = element-wise gather + separate split.
 *   bn_fused  BN kernel form: 1 = train-mode layers with p <= 16384 (or p <= 33792 and c >= 128) run
 *             one fused statistics+apply launch per call (one block per channel, operands held in
 *             registers; default), 0 = the split statistics / flat-apply launches everywhere. */
typedef struct msl_forms {
  int f32_form;
  int sk_hybrid;
  int pack_form;
  int bn_fused;
} msl_forms;
int msl_forms_default(msl_forms* out);       /* writes the defaults */
int msl_forms_check(const msl_forms* forms); /* MSL_OK (NULL included) or MSL_ERR_ARG */

/* ------------------------------------------------------------------------
 * Dilated 3x3 convolution, stride 1, padding = dilation, as an FP32-MFMA
 * implicit GEMM.  One call covers either a single conv (nbranch = 1:
 * Bottleneck.conv2 of layer3 d=2 / layer4 d=4, deeplab_multi.py:17-18,82-83)
 * or the live part of an ASPP head (nbranch = 2: conv_d6(x) + conv_d12(x) with
 * biases, Classifier_Module.forward, deeplab_multi.py:62-66 incl. quirk Q1).
 * Weights of branch b start at w + b*branch_stride, shape [cout][cin][3][3].
 * Images: x / y / dy / dx hold nimg images of h x w as [channels][nimg][h][w] (nimg = 1: the
 * reference's bs = 1 NCHW layout).  Each image is convolved on its own (a tap never reads across
 * into the neighbouring image); the weight gradient sums over all of them.  The trainer runs the
 * source and target images of an iteration as one pair (nimg = 2).
 * ---------------------------------------------------------------------- */

/* Elements (fp32 units) of the packed operand produced by msl_dconv_pack (for_dgrad = 0:
 * forward layout, 1: transposed + tap-flipped layout for the data gradient): the fp32 K-major
 * pack followed by its bf16x6 planes (split once here, read by the bf16x6 fp32 form; with form 5,
 * the fp16 planes and a tail holding the weights' scale).  All
 * nbranch branches are packed by one call (branch b's weights at w + b*branch_stride floats). */
long long msl_dconv_packed_elems(int nbranch, int cin, int cout, int for_dgrad);
/* One weight pack of a batch: exactly what msl_dconv_pack (taps 9) / msl_pconv_pack (taps 1,
 * nbranch 1, branch_stride 0) would write into `packed`. */
typedef struct msl_pack_job {
  const float* w;
  long long branch_stride;
  float* packed;
  int nbranch, cin, cout, for_dgrad;
} msl_pack_job;
/* Blocks of one job in msl_conv_pack_many (-1 on bad arguments). */
long long msl_conv_pack_blocks(int nbranch, int taps, int cin, int cout, int for_dgrad);
/* Every job of `jobs` (device array, all with the same tap count) in one launch: job j runs blocks
 * block_start[j] .. block_start[j+1]-1 (device array of njobs+1 ascending offsets built with
 * msl_conv_pack_blocks; block_start[njobs] = total_blocks).  Byte-identical to the per-job calls;
 * replaces the ~120 per-conv pack launches of a training step by two. */
int msl_conv_pack_many(const msl_pack_job* jobs, const long long* block_start, int njobs, int taps,
                       long long total_blocks, const msl_forms* forms, msl_stream_t stream);
int msl_dconv_pack(const float* w, long long branch_stride, int nbranch, int cin, int cout,
                   int for_dgrad, float* packed, const msl_forms* forms, msl_stream_t stream);

/* y[cout][h][w] = sum_b conv3x3(x, W_b, dil_b) (+ sum_b bias[b][cout] if bias)
 * replaces nn.Conv2d.forward at deeplab_multi.py:35 (layer3/4) and :63-65 (ASPP). */
size_t msl_dconv_fwd_workspace(int nbranch, int cin, int cout, int h, int w, int nimg);
int msl_dconv_fwd(const float* x, const float* packed, const float* bias, float* y, int nbranch,
                  int cin, int cout, int h, int w, int nimg, int dil0, int dil1, const msl_forms* forms, void* ws,
                  size_t ws_bytes, msl_stream_t stream);

/* dx[cin][h][w] = sum_b conv3x3^T(dy, W_b, dil_b)   (autograd of the same sites) */
size_t msl_dconv_dgrad_workspace(int nbranch, int cin, int cout, int h, int w, int nimg);
int msl_dconv_dgrad(const float* dy, const float* packed_dgrad, float* dx, int nbranch, int cin,
                    int cout, int h, int w, int nimg, int dil0, int dil1, const msl_forms* forms, void* ws,
                    size_t ws_bytes, msl_stream_t stream);

/* dw[b][cout][cin][3][3] (= or += when accumulate) and, if dbias != NULL,
 * dbias[b][cout] = sum_px dy (identical for both branches). */
size_t msl_dconv_wgrad_workspace(int nbranch, int cin, int cout, int h, int w, int nimg);
int msl_dconv_wgrad(const float* x, const float* dy, float* dw, float* dbias, int nbranch, int cin,
                    int cout, int h, int w, int nimg, int dil0, int dil1, int accumulate, const msl_forms* forms, void* ws,
                    size_t ws_bytes, msl_stream_t stream);

/* ------------------------------------------------------------------------
 * Pointwise (1x1, stride 1, no bias) convolution: the same FP32-MFMA GEMM
 * kernels with one unshifted tap over the flat pixel axis p = h*w.  Replaces
 * Bottleneck.conv1 / conv3 (deeplab_multi.py:13, 20) and the downsample conv
 * (deeplab_multi.py:96-99)
 * wherever their stride is 1 (layer1, layer3, layer4 and layer2 blocks 2-4).
 * Weights [cout][cin] (= [cout][cin][1][1]).
 * ---------------------------------------------------------------------- */
long long msl_pconv_packed_elems(int cin, int cout, int for_dgrad);
int msl_pconv_pack(const float* w, int cin, int cout, int for_dgrad, float* packed, const msl_forms* forms,
                   msl_stream_t stream);

/* y[cout][p] = sum_ci W[cout][ci] x[ci][p] */
size_t msl_pconv_fwd_workspace(int cin, int cout, int p);
int msl_pconv_fwd(const float* x, const float* packed, float* y, int cin, int cout, int p,
                  const msl_forms* forms, void* ws, size_t ws_bytes, msl_stream_t stream);

/* dx[cin][p] = sum_co W[co][cin] dy[co][p] */
size_t msl_pconv_dgrad_workspace(int cin, int cout, int p);
int msl_pconv_dgrad(const float* dy, const float* packed_dgrad, float* dx, int cin, int cout, int p,
                    const msl_forms* forms, void* ws, size_t ws_bytes, msl_stream_t stream);
/* msl_pconv_dgrad with accumulate = 1: dx += W^T dy (dx read and written by the GEMM's own
 * epilogue / piece reduce; the bottleneck's residual gradient summed without a separate add).
 * accumulate = 0 is msl_pconv_dgrad.  Replaces autograd's grad accumulation at the block input
 * (Bottleneck.forward, deeplab_multi.py:31-48: conv1(x) and the identity residual both read x). */
int msl_pconv_dgrad_acc(const float* dy, const float* packed_dgrad, float* dx, int cin, int cout, int p,
                        int accumulate, const msl_forms* forms, void* ws, size_t ws_bytes, msl_stream_t stream);
/* msl_pconv_dgrad_acc's sum with the identity residual's gradient formed in the epilogue (r06):
 * dx = mask(res) + W^T dy, mask(res)[c][n] = res[c][n] where the forward's y > 0 bit of that element is set
 * (res_mask: msl_bn_fwd_mask's bits, rows c * nimg + image, cdiv(p / nimg, 64) words each), else 0.  dx is
 * written, not read.  The bottleneck's bn3 backward (msl_bn_bwd_mask with dres = NULL) then need not write
 * that gradient; replaces autograd's residual accumulation at deeplab_multi.py:31-48 (x feeds conv1 and
 * the identity residual).  Workspace: msl_pconv_dgrad_workspace.  _sc: the dy partials as in the _sc
 * entry points; _f16: the fp16 math as msl_pconv_dgrad_f16. */
int msl_pconv_dgrad_resmask_sc(const float* dy, const float* packed_dgrad, float* dx, int cin, int cout, int p,
                               const float* res, const unsigned long long* res_mask, int nimg, const msl_forms* forms,
                               void* ws, size_t ws_bytes, msl_stream_t stream, const float* dy_part, int dy_npart);
int msl_pconv_dgrad_resmask_f16(const float* dy, const float* packed_dgrad, float* dx, int cin, int cout, int p,
                                const float* res, const unsigned long long* res_mask, int nimg, const msl_forms* forms,
                                void* ws, size_t ws_bytes, msl_stream_t stream, const float* dy_part, int dy_npart);

/* dw[cout][cin] (= or += when accumulate) = sum_p dy[cout][p] x[cin][p] */
size_t msl_pconv_wgrad_workspace(int cin, int cout, int p);
int msl_pconv_wgrad(const float* x, const float* dy, float* dw, int cin, int cout, int p,
                    int accumulate, const msl_forms* forms, void* ws, size_t ws_bytes, msl_stream_t stream);

/* ------------------------------------------------------------------------
 * The stem and the strided glue of ResNetMulti (csrc/stem.hip), all gather forms without atomics
 * (bit-reproducible).  Replaces the last library kernels of the training step:
 *   - conv1 7x7 / stride 2 / pad 3 (deeplab_multi.py:73-74, 114) = msl_im2col into a
 *     [c*kh*kw][ho*wo] column matrix + msl_pconv_fwd with the [cout][c*kh*kw] weight (the conv
 *     weight as laid out); its weight gradient msl_pconv_wgrad on the same columns; its data
 *     gradient msl_pconv_dgrad into columns + msl_col2im (sums the columns back, i-major, j-minor);
 *   - MaxPool2d(3, 2, 1, ceil_mode=True) (deeplab_multi.py:77, 114): window [o*s - pad, +k) clipped
 *     to the image, first max in row-major scan (a NaN replaces), idx = y*w + x of the max; the
 *     caller passes ho/wo (torch's ceil-mode output size); the backward sums dy over the windows
 *     whose idx is the pixel, in (oy, ox) order (torch-CPU's order: bit-exact);
 *   - x[:, :, ::s, ::s] (the stride of layer2.0's 1x1 conv1 and downsample, deeplab_multi.py:12-13,
 *     96-99) and its transpose (zeros elsewhere) for the gradient.
 * ---------------------------------------------------------------------- */
/* im2col / col2im over nimg images: x [c][nimg][h][w], col [c*kh*kw][nimg][ho][wo].  The pooling
 * and subsample entry points are per plane: call them with c = channels * nimg. */
int msl_im2col(const float* x, int c, int h, int w, int nimg, int kh, int kw, int stride, int pad, int dil, int ho,
               int wo, float* col, msl_stream_t stream);
int msl_col2im(const float* col, int c, int h, int w, int nimg, int kh, int kw, int stride, int pad, int dil, int ho,
               int wo, float* x, msl_stream_t stream);
int msl_maxpool_fwd(const float* x, int c, int h, int w, int k, int stride, int pad, int ho, int wo, float* y,
                    int32_t* idx, msl_stream_t stream);
int msl_maxpool_bwd(const float* dy, const int32_t* idx, int c, int h, int w, int k, int stride, int pad, int ho,
                    int wo, float* dx, msl_stream_t stream);
int msl_subsample(const float* x, int c, int h, int w, int stride, int ho, int wo, float* y, msl_stream_t stream);
int msl_subsample_bwd(const float* dy, int c, int h, int w, int stride, int ho, int wo, float* dx,
                      msl_stream_t stream);

/* ------------------------------------------------------------------------
 * Operand scales of the f16x3 form (msl_forms.f32_form 5).  Each GEMM operand is scaled by a
 * power of two derived from absolute maxima and split into two fp16 terms.  The maxima come as
 * PER-ROW partials: msl_absmax_partials writes part[r] = max |x[r][.]| for each of the `rows` rows
 * (channels) of a [rows][row_len] tensor, and msl_bn_fwd_am / msl_bn_bwd_am write the same per-
 * channel maxima for the tensor a BN kernel produced.  The plain fp32 entry points reduce them
 * themselves; the _sc variants below take them from the caller as (pointer, count), count = the
 * operand's rows (its channels; NULL = compute), so a tensor read by two GEMMs (x by the forward
 * and the weight gradient, dy by the data and the weight gradient) is reduced once, or not at all
 * when a BN kernel produced it.  The forward / data gradient scale the image operand by one
 * tensor-wide power of two (the maximum of the partials: its rows are the GEMM's K index); the
 * weight gradient scales every row of dY and of x by its own power of two (both are output
 * indices there), so each dW element keeps the form's full precision even for channels far
 * below the tensor's maximum.  Partials must describe exactly the tensor passed (same contents).
 * The other forms ignore them.
 * ---------------------------------------------------------------------- */
int msl_absmax_partials(const float* x, int rows, int row_len, float* part, msl_stream_t stream);
int msl_dconv_fwd_sc(const float* x, const float* packed, const float* bias, float* y, int nbranch,
                     int cin, int cout, int h, int w, int nimg, int dil0, int dil1, const msl_forms* forms, void* ws,
                     size_t ws_bytes, msl_stream_t stream, const float* x_part, int x_npart);
int msl_dconv_dgrad_sc(const float* dy, const float* packed_dgrad, float* dx, int nbranch, int cin,
                       int cout, int h, int w, int nimg, int dil0, int dil1, const msl_forms* forms, void* ws,
                       size_t ws_bytes, msl_stream_t stream, const float* dy_part, int dy_npart);
int msl_dconv_wgrad_sc(const float* x, const float* dy, float* dw, float* dbias, int nbranch, int cin,
                       int cout, int h, int w, int nimg, int dil0, int dil1, int accumulate, const msl_forms* forms, void* ws,
                       size_t ws_bytes, msl_stream_t stream, const float* x_part, int x_npart,
                       const float* dy_part, int dy_npart);
int msl_pconv_fwd_sc(const float* x, const float* packed, float* y, int cin, int cout, int p,
                     const msl_forms* forms, void* ws, size_t ws_bytes, msl_stream_t stream, const float* x_part,
                     int x_npart);
int msl_pconv_dgrad_acc_sc(const float* dy, const float* packed_dgrad, float* dx, int cin, int cout, int p,
                           int accumulate, const msl_forms* forms, void* ws, size_t ws_bytes, msl_stream_t stream,
                           const float* dy_part, int dy_npart);
int msl_pconv_wgrad_sc(const float* x, const float* dy, float* dw, int cin, int cout, int p,
                       int accumulate, const msl_forms* forms, void* ws, size_t ws_bytes, msl_stream_t stream, const float* x_part,
                       int x_npart, const float* dy_part, int dy_npart);

/* ------------------------------------------------------------------------
 * ASPP heads as a pointwise GEMM plus shifts (csrc/aspp.hip; Classifier_Module.forward,
 * deeplab_multi.py:51-66, 84-85, quirk Q1: branches 0 and 1 with their biases).  With nt = 9*nbranch
 * taps t = b*9 + k (k = (dh/d_b + 1)*3 + dw/d_b + 1) and W' = the [nt*c][cin] weight
 * W'[t*c + m][ci] = W_b[m][ci][k]:
 *   forward   Z = W' x (msl_pconv_fwd*, M = nt*c), y = msl_aspp_shift_add(Z): y[m][p] = sum over t
 *             (in order) of Z[t*c + m][p + off_t] where the tap's source pixel is inside p's image, plus
 *             bias_0[m] + bias_1[m] (bias nullable);
 *   backward  G = msl_aspp_shift_gather(dY): G[t*c + m][q] = dY[m][q - off_t] where that pixel is inside
 *             q's image (else 0), dbias[b][m] = sum_p dY[m][p] (nullable); dx = W'^T G
 *             (msl_pconv_dgrad*), dW' = G x^T (msl_pconv_wgrad*), msl_aspp_weight_grad(dW') ->
 *             dw [nbranch][c][cin][3][3].
 * x / y / dY hold nimg images of h x w ([channels][nimg][h][w]); W_b at w + b*branch_stride.
 * ---------------------------------------------------------------------- */
int msl_aspp_weight_layout(const float* w, long long branch_stride, int nbranch, int c, int cin, float* wp,
                           msl_stream_t stream);
int msl_aspp_weight_grad(const float* dwp, int nbranch, int c, int cin, float* dw, msl_stream_t stream);
int msl_aspp_shift_add(const float* z, const float* bias, float* y, int nbranch, int c, int h, int w, int nimg,
                       int dil0, int dil1, msl_stream_t stream);
int msl_aspp_shift_gather(const float* dy, float* g, float* dbias, int nbranch, int c, int h, int w, int nimg,
                          int dil0, int dil1, msl_stream_t stream);

/* ------------------------------------------------------------------------
 * BF16-MFMA forms of the six conv calls above (BASELINE config 5, "fp16/bf16 MFMA
 * path"): identical arguments, workspaces and output layout; the fp32 operands are
 * rounded to bf16 (RNE) as they are read from LDS and multiplied by
 * v_mfma_f32_32x32x16_bf16 with fp32 accumulation.  Same reference sites.
 * ---------------------------------------------------------------------- */
int msl_dconv_fwd_bf16(const float* x, const float* packed, const float* bias, float* y, int nbranch,
                       int cin, int cout, int h, int w, int nimg, int dil0, int dil1, const msl_forms* forms, void* ws,
                       size_t ws_bytes, msl_stream_t stream);
int msl_dconv_dgrad_bf16(const float* dy, const float* packed_dgrad, float* dx, int nbranch, int cin,
                         int cout, int h, int w, int nimg, int dil0, int dil1, const msl_forms* forms, void* ws,
                         size_t ws_bytes, msl_stream_t stream);
int msl_dconv_wgrad_bf16(const float* x, const float* dy, float* dw, float* dbias, int nbranch,
                         int cin, int cout, int h, int w, int nimg, int dil0, int dil1, int accumulate, const msl_forms* forms,
                         void* ws, size_t ws_bytes, msl_stream_t stream);
int msl_pconv_fwd_bf16(const float* x, const float* packed, float* y, int cin, int cout, int p,
                       const msl_forms* forms, void* ws, size_t ws_bytes, msl_stream_t stream);
int msl_pconv_dgrad_bf16(const float* dy, const float* packed_dgrad, float* dx, int cin, int cout,
                         int p, const msl_forms* forms, void* ws, size_t ws_bytes, msl_stream_t stream);
int msl_pconv_wgrad_bf16(const float* x, const float* dy, float* dw, int cin, int cout, int p,
                         int accumulate, const msl_forms* forms, void* ws, size_t ws_bytes, msl_stream_t stream);

/* ------------------------------------------------------------------------
 * FP16-MFMA forms (BASELINE config 5's fp16 MFMA path): each operand tensor scaled by a power of
 * two (its absolute maximum into [2^14, 2^15)) and rounded to fp16 once - the weights at pack
 * time, as the hi planes of the f16x3 packs, so the packs must be made in the f16x3 fp32 form
 * (forms.f32_form 5, the default; MSL_ERR_ARG for another f32_form) - then one
 * v_mfma_f32_32x32x16_f16 per 16-deep K slice with fp32 accumulation, the result unscaled
 * exactly (M <= 64: 64-row fp16 tiles, r04; the weight gradients with fewer than 128 channels on either
 * side keep exact f32 MFMA tiles).  Operand partials as in
 * the _sc entry points ((pointer, count), NULL = computed); msl_pconv_dgrad_f16 carries the
 * accumulate flag of msl_pconv_dgrad_acc.  Same workspaces and results layout.
 * ---------------------------------------------------------------------- */
int msl_dconv_fwd_f16(const float* x, const float* packed, const float* bias, float* y, int nbranch, int cin,
                      int cout, int h, int w, int nimg, int dil0, int dil1, const msl_forms* forms, void* ws, size_t ws_bytes,
                      msl_stream_t stream, const float* x_part, int x_npart);
int msl_dconv_dgrad_f16(const float* dy, const float* packed_dgrad, float* dx, int nbranch, int cin, int cout,
                        int h, int w, int nimg, int dil0, int dil1, const msl_forms* forms, void* ws, size_t ws_bytes,
                        msl_stream_t stream, const float* dy_part, int dy_npart);
int msl_dconv_wgrad_f16(const float* x, const float* dy, float* dw, float* dbias, int nbranch, int cin, int cout,
                        int h, int w, int nimg, int dil0, int dil1, int accumulate, const msl_forms* forms, void* ws, size_t ws_bytes,
                        msl_stream_t stream, const float* x_part, int x_npart, const float* dy_part, int dy_npart);
int msl_pconv_fwd_f16(const float* x, const float* packed, float* y, int cin, int cout, int p, const msl_forms* forms,
                      void* ws, size_t ws_bytes, msl_stream_t stream, const float* x_part, int x_npart);
int msl_pconv_dgrad_f16(const float* dy, const float* packed_dgrad, float* dx, int cin, int cout, int p,
                        int accumulate, const msl_forms* forms, void* ws, size_t ws_bytes, msl_stream_t stream,
                        const float* dy_part, int dy_npart);
int msl_pconv_wgrad_f16(const float* x, const float* dy, float* dw, int cin, int cout, int p, int accumulate, const msl_forms* forms,
                        void* ws, size_t ws_bytes, msl_stream_t stream, const float* x_part, int x_npart,
                        const float* dy_part, int dy_npart);
/* 1 if the weight gradient of this conv (taps 9: msl_dconv_wgrad*, h x w maps of nimg images;
 * taps 1: msl_pconv_wgrad* with p = nimg*h*w) runs the split kernel - whose fp16 form rounds both
 * operands to fp16 (one power-of-two scale per row) - and 0 if it runs an fp32-accurate tile
 * kernel (fewer than 128 channels on a side, or too few tiles to fill the chip).  A plan query,
 * no work: the fp16-operand emulation of the tests (oracle conv_f16) asks it.  MSL_ERR_ARG on bad
 * dimensions. */
int msl_conv_wgrad_split(int nbranch, int taps, int cin, int cout, int h, int w, int nimg);

/* ------------------------------------------------------------------------
 * The plan of a forward-form call (forward and data gradient of every family), as a host-only
 * query: no launch, no pointers, usable without a GPU.  The tests hold every reachable
 * (kernel, schedule) to fp64 through it (tests/conv_form_cases.py).  Additive: ABI 3.
 * Replaces nothing in the reference.
 * ---------------------------------------------------------------------- */
/* One instantiation of the stream-K kernel (its template arguments). */
typedef struct msl_conv_form {
  int bm, G, stages, wm, wn; /* tile rows, K-steps per LDS stage, stages, wave layout */
  int pw;                    /* pointwise image rows (dwordx4 pieces) */
  int math;                  /* 0 exact f32, 1 bf16, 2 bf16x6 split in the loop, 3 bf16x6 on pre-split
                                weights, 5 f16x3, 8 fp16 */
  int acc;                   /* the accumulate epilogue */
  int bform;                 /* image operand: 0 through LDS, 1 straight to registers, 2 pre-split */
} msl_conv_form;
int msl_conv_fwd_form_count(void);                            /* instantiations built */
int msl_conv_fwd_form_describe(int row, msl_conv_form* out); /* MSL_ERR_ARG outside [0, count) or NULL */
typedef struct msl_conv_fwd_plan_info {
  int row;      /* the instantiation the call launches (msl_conv_fwd_form_describe); -1: none (the split-K
                   tile kernel, or a form that is not built) */
  int stream_k; /* 1 stream-K, 0 the split-K tile kernel (odd K-step count, M <= 32) */
  int math;     /* the math of the kernel launched (msl_conv_form.math; the tile kernel is exact f32) */
  int tiles_m, tiles_n, ksteps; /* output tiles, K-steps (one tap, 16 channels each) */
  int kps, S;   /* stream-K: LDS stages per tile, 1; tile kernel: K-steps per slab, slabs */
  int tdp, NW, T; /* stream-K schedule: tiles run whole (data-parallel rounds), workers of the split
                     remainder and its stage count (0 0 0 for the tile kernel) */
  int reduce;    /* a reduce launch follows (split tiles / slabs) */
  int split_img; /* the image operand is pre-split by a launch of its own first */
  int status;    /* what the call returns given a sufficient workspace: MSL_OK or MSL_ERR_SHAPE */
} msl_conv_fwd_plan_info;
/* family: 0 the fp32 entry points (forms->f32_form), 1 _bf16, 2 _f16.  taps 9 (dil0 >= 1, nbranch 1 or 2)
 * or 1 (dil0 = 0, nbranch 1); cimg = channels of the image operand and M = output rows (forward: cin,
 * cout; data gradient: cout, cin); P = nimg*h*w; accumulate as msl_pconv_dgrad_acc (1 for the masked
 * residual too).  MSL_ERR_ARG on anything else, incl. forms the family cannot run. */
int msl_conv_fwd_plan(int family, int nbranch, int taps, int cimg, int M, int P, int accumulate, int dil0,
                      const msl_forms* forms, msl_conv_fwd_plan_info* out);

/* ------------------------------------------------------------------------
 * The plan of a weight-gradient call (msl_dconv_wgrad* / msl_pconv_wgrad* of every family), as a
 * host-only query: no launch, no pointers to data, usable without a GPU.  It reports what the call
 * launches through the very functions the launch calls (the operand swap, the GEMM kernel and the
 * math it was instantiated with, the piece reduce, the refusal, the scale mode), so it cannot drift
 * from it.  The tests hold every reachable (GEMM, reduce, orientation, taps) and schedule class to fp64
 * through it (tests/conv_wgrad_cases.py).  Additive: ABI 3.  Replaces nothing in the reference.
 * ---------------------------------------------------------------------- */
typedef struct msl_conv_wgrad_plan_info {
  int gemm;      /* 0 k_wgrad_sk (64-pixel K-steps), 1 k_wgrad_x6 (16-pixel K-steps on a pre-split operand) */
  int bm, bn;    /* its tile */
  int math;      /* the math it was instantiated with (msl_conv_form.math: 0, 1, 2, 5, 8) - the math
                    launched, not the family's: the fp16 family runs 2 on k_wgrad_sk's 128-row tile and
                    0 on its 64- and 32-row tiles */
  int split_rows; /* k_split_rows runs first (gemm 1) */
  int reduce;    /* the piece reduce: 0 k_wsk_reduce<32,128>, 1 k_wsk_reduce<64,64>, 2 k_wsk_reduce_wide<64,64,8>,
                    3 k_wsk_reduce<128,128>, 4 k_wsk_reduce_split<128,128,4> */
  int trans;     /* operands swapped (M = cin, N = cout), the dW^T tiles written transposed */
  int tiles_m, tiles_n, ntap; /* tiles of the (swapped) M and N, nbranch * taps */
  int KS, bk;    /* K-steps of one tile, pixels per K-step */
  int NW, T, slots; /* workgroups, (tile, K-step) items, pieces a worker can leave */
  int nchunk, kchunk; /* chunked split-K (gemm 1): chunks per tile and K-steps per chunk; 0 0 = stream-K ranges */
  int swizzle;   /* the XCD worker swizzle is on (NW a multiple of 8) */
  int max_run;   /* the longest run of K-steps one worker gives to one tile */
  int mask_tab;  /* gemm 1: that run reads its border masks from the LDS table (1) or takes the scalar
                    cursor (0); 0 for gemm 0 */
  int rowscale;  /* fp16 planes (math 5, 8 on gemm 1): 1 one scale per row, 0 one per tensor */
  int status;    /* what the call returns given a sufficient workspace: MSL_OK or MSL_ERR_SHAPE */
} msl_conv_wgrad_plan_info;
/* family as msl_conv_fwd_plan.  taps 9: msl_dconv_wgrad* on nimg images of h x w (nbranch 1 or 2);
 * taps 1: msl_pconv_wgrad* with p = nimg*h*w (nbranch 1, has_dbias 0), planned on one flat row as the
 * call plans it.  x_npart / dy_npart: the partial counts the caller passes with x / dy (0 = none: the call
 * reduces one per row itself).  MSL_ERR_ARG on anything else, incl. forms the family cannot run. */
int msl_conv_wgrad_plan(int family, int nbranch, int taps, int cin, int cout, int h, int w, int nimg,
                        int has_dbias, int x_npart, int dy_npart, const msl_forms* forms,
                        msl_conv_wgrad_plan_info* out);

/* ------------------------------------------------------------------------
 * Bilinear upsample, align_corners=True (F.interpolate at deeplab_multi.py:124,
 * :128).  The forward reproduces torch-CPU's rounding bit for bit where
 * ho + wo > 128, the per-axis form torch-CPU takes there (every size a network
 * runs at); at or below it torch-CPU sums four taps instead and the last bit
 * can differ: msl_resize_bilinear below has both forms.
 * ---------------------------------------------------------------------- */
int msl_upsample_fwd(const float* in, float* out, int c, int hi, int wi, int ho, int wo,
                     msl_stream_t stream);
/* F.interpolate(in, (ho, wo), mode="bilinear", align_corners=True) of an image or mask, c <= 4 planes
 * [c][hi][wi], up or down, with torch-CPU's rounding bit for bit at every size: where ho + wo > 128 torch
 * interpolates per axis - msl_upsample_fwd's kernel, launched as it is -, at or below it sums four taps with
 * rounded weight products (r = w01 v01, then fma of the (0,0), (1,0), (1,1) taps), a form
 * msl_upsample_fwd does not have.  The evaluator's --scales resizes its network input with this. */
int msl_resize_bilinear(const float* in, float* out, int c, int hi, int wi, int ho, int wo,
                        msl_stream_t stream);
size_t msl_upsample_bwd_workspace(int c, int hi, int wi, int ho, int wo);
int msl_upsample_bwd(const float* gout, float* gin, int c, int hi, int wi, int ho, int wo,
                     void* ws, size_t ws_bytes, msl_stream_t stream);

/* ------------------------------------------------------------------------
 * Fused losses on the *low-resolution* logits [c][hi][wi]: each kernel
 * re-interpolates (bit-exact bilinear) to [c][ho][wo] on the fly, applies the
 * softmax and the loss, and the backward returns the gradient w.r.t. the
 * low-res logits directly (loss backward + softmax backward + upsample
 * backward in one pass, deterministic gather form).  hi == ho, wi == wo is the
 * identity interpolation, i.e. the plain hi-res loss.
 *
 * Every *_fwd writes a small device "stats" record consumed by *_bwd and the
 * loss scalar to out[0]; gout is a device pointer to dL/d(loss).
 * ---------------------------------------------------------------------- */
size_t msl_loss_workspace(int c, int hi, int wi, int ho, int wo);
int msl_loss_stats_elems(void); /* floats in a stats record */

/* nn.CrossEntropyLoss(ignore_index=-1) (train_source.py:128, solve_gta5.py:226-231).
 * out[0] = mean CE over valid pixels (nan if none, quirk Q8), stats = {sum, n_valid}. */
int msl_ce_up_fwd(const float* logits, const int64_t* labels, int c, int hi, int wi, int ho,
                  int wo, float* out, float* stats, void* ws, size_t ws_bytes,
                  msl_stream_t stream);
int msl_ce_up_bwd(const float* logits, const int64_t* labels, int c, int hi, int wi, int ho,
                  int wo, const float* stats, const float* gout, float* dlogits, void* ws,
                  size_t ws_bytes, msl_stream_t stream);

/* MaxSquareloss (utils/loss.py:104-119): out[0] = -sum(p^2) / (2*C*H*W). */
int msl_maxsquare_up_fwd(const float* logits, int c, int hi, int wi, int ho, int wo, float* out,
                         float* stats, void* ws, size_t ws_bytes, msl_stream_t stream);
int msl_maxsquare_up_bwd(const float* logits, int c, int hi, int wi, int ho, int wo,
                         const float* stats, const float* gout, float* dlogits, void* ws,
                         size_t ws_bytes, msl_stream_t stream);

/* IW_MaxSquareloss (utils/loss.py:69-102): hist = per-class count of argmax p
 * (int32, bit-exact), weights = 1/max(hist^r * (HW)^(1-r), 1),
 * out[0] = -sum_px w[argmax] * sum_c p^2 / C.  hist/weights may be NULL. */
int msl_iw_maxsquare_up_fwd(const float* logits, int c, int hi, int wi, int ho, int wo,
                            float ratio, float* out, float* stats, int32_t* hist,
                            float* weights, void* ws, size_t ws_bytes, msl_stream_t stream);
int msl_iw_maxsquare_up_bwd(const float* logits, int c, int hi, int wi, int ho, int wo,
                            const float* stats, const float* gout, float* dlogits, void* ws,
                            size_t ws_bytes, msl_stream_t stream);

/* Multi-level self-produced guidance (solve_gta5.py:206-213): P = softmax(up(x2)),
 * P2 = softmax(up(x1)), label2 = (max P > thr | max P2 > thr) ? argmax((P+P2)/2) : -1,
 * out[0] = CE(up(x1), label2) (mean over valid, nan if none).  The backward
 * returns d/d x1 only (label2 is detached in the reference). */
int msl_multi_ce_up_fwd(const float* logits1, const float* logits2, int c, int hi, int wi,
                        int ho, int wo, float thr, float* out, float* stats, void* ws,
                        size_t ws_bytes, msl_stream_t stream);
int msl_multi_ce_up_bwd(const float* logits1, const float* logits2, int c, int hi, int wi,
                        int ho, int wo, float thr, const float* stats, const float* gout,
                        float* dlogits1, void* ws, size_t ws_bytes, msl_stream_t stream);

/* The per-pixel decisions inside the fused losses, written out (parity inspection; argmax1 and
 * label2 are int32 [ho*wo], either nullable): argmax1 = first-max argmax of softmax(up(logits1))
 * (torch.max at loss.py:84-86 / the IW histogram's class), label2 = the multi-level guidance
 * label of msl_multi_ce_up_fwd with logits1 = x1, logits2 = x2 (solve_gta5.py:206-212). */
int msl_loss_labels_up(const float* logits1, const float* logits2, int c, int hi, int wi, int ho,
                       int wo, float thr, int32_t* argmax1, int32_t* label2, msl_stream_t stream);

/* The MinEnt baseline, softCrossEntropy()(pred, softmax(pred)) (utils/loss.py:17-35,
 * solve_gta5.py:151-152, :189): with lp = log_softmax(up(logits)) and p = softmax(up(logits)),
 * out[0] = sum_px sum_c -lp_c p_c / (C*H*W).  The target softmax is not detached: the backward
 * returns -p_c (lp_c + H) / (C*H*W), H the pixel's entropy. */
int msl_entropy_up_fwd(const float* logits, int c, int hi, int wi, int ho, int wo, float* out,
                       float* stats, void* ws, size_t ws_bytes, msl_stream_t stream);
int msl_entropy_up_bwd(const float* logits, int c, int hi, int wi, int ho, int wo,
                       const float* stats, const float* gout, float* dlogits, void* ws,
                       size_t ws_bytes, msl_stream_t stream);

/* IWsoftCrossEntropy(ratio)(pred, softmax(pred)) (utils/loss.py:37-67): hist = per-class count
 * of the argmax of the upsampled LOGITS (first index on ties; int32, bit-exact), weights as
 * msl_iw_maxsquare_up_fwd, out[0] = sum_px w[argmax] * sum_c -lp_c p_c / C.  hist/weights may
 * be NULL. */
int msl_iw_entropy_up_fwd(const float* logits, int c, int hi, int wi, int ho, int wo, float ratio,
                          float* out, float* stats, int32_t* hist, float* weights, void* ws,
                          size_t ws_bytes, msl_stream_t stream);
int msl_iw_entropy_up_bwd(const float* logits, int c, int hi, int wi, int ho, int wo,
                          const float* stats, const float* gout, float* dlogits, void* ws,
                          size_t ws_bytes, msl_stream_t stream);

/* The hard pseudo-label baseline (solve_gta5.py:149-150, :185-199): label = argmax p where
 * max p > thr, else -1 (detached); out[0] = CE(up(logits), label), the mean over kept pixels
 * (nan with a zero gradient if none, quirk Q8). */
int msl_hard_ce_up_fwd(const float* logits, int c, int hi, int wi, int ho, int wo, float thr,
                       float* out, float* stats, void* ws, size_t ws_bytes, msl_stream_t stream);
int msl_hard_ce_up_bwd(const float* logits, int c, int hi, int wi, int ho, int wo, float thr,
                       const float* stats, const float* gout, float* dlogits, void* ws,
                       size_t ws_bytes, msl_stream_t stream);

/* The decisions of the two kinds above, written out (int32 [ho*wo], either nullable): label =
 * the hard pseudo-label (-1 = ignored), argmax_logits = the IW-entropy histogram's class. */
int msl_pseudo_labels_up(const float* logits, int c, int hi, int wi, int ho, int wo, float thr,
                         int32_t* label, int32_t* argmax_logits, msl_stream_t stream);

/* softCrossEntropy / IWsoftCrossEntropy on explicit tensors, as the reference API takes them
 * (loss.py:23, :46): inputs = hi-res logits [c][hw], target = a distribution [c][hw], elements
 * equal to `ignore` masked out (m).  Plain: out[0] = the mean of -lp * target over the kept
 * elements (nan with zero gradients if none); IW: out[0] = sum_px w[argmax inputs] * sum_c m *
 * -lp_c target_c / c, hist / weights (nullable) as msl_iw_entropy_up_fwd.  The backward writes
 * d inputs_c = a (p_c S - m_c t_c), S = sum_k m_k t_k, and d target = -a m lp (either nullable),
 * a = gout / n (plain) or gout * w[argmax] / c (IW).  Workspace: msl_loss_workspace(c,1,1,1,hw). */
int msl_soft_ce_fwd(const float* inputs, const float* target, int c, int hw, float ignore,
                    float* out, float* stats, void* ws, size_t ws_bytes, msl_stream_t stream);
int msl_soft_ce_bwd(const float* inputs, const float* target, int c, int hw, float ignore,
                    const float* stats, const float* gout, float* dinputs, float* dtarget,
                    msl_stream_t stream);
int msl_iw_soft_ce_fwd(const float* inputs, const float* target, int c, int hw, float ignore,
                       float ratio, float* out, float* stats, int32_t* hist, float* weights,
                       void* ws, size_t ws_bytes, msl_stream_t stream);
int msl_iw_soft_ce_bwd(const float* inputs, const float* target, int c, int hw, float ignore,
                       const float* stats, const float* gout, float* dinputs, float* dtarget,
                       msl_stream_t stream);

/* Probability-input forms, for callers that hand the loss an explicit prob
 * tensor exactly as the reference API does (loss.py:76, :110).
 * prob is [c][hw]; label (nullable) is int64 [hw]. */
int msl_maxsquare_prob_fwd(const float* prob, int c, int hw, float* out, void* ws,
                           size_t ws_bytes, msl_stream_t stream);
int msl_maxsquare_prob_bwd(const float* prob, int c, int hw, const float* gout, float* dprob,
                           msl_stream_t stream);
int msl_iw_maxsquare_prob_fwd(const float* prob, const int64_t* label, int c, int hw,
                              float ratio, float* out, int32_t* hist, float* weights, void* ws,
                              size_t ws_bytes, msl_stream_t stream);
int msl_iw_maxsquare_prob_bwd(const float* prob, int c, int hw, const float* weights,
                              const float* gout, float* dprob, msl_stream_t stream);

/* The plan of a fused-loss, upsample or resize call, as a host-only query: no launch, no pointers to data,
 * usable without a GPU.  It reports what a call of the family does with this geometry through the very
 * functions the call uses (its refusals, the class-count instantiation, every grid, the row kernel's chunks
 * and LDS), so it cannot drift from them.  The tests hold every kernel form to fp64 through it
 * (tests/loss_form_cases.py).  Additive: ABI 3.  Replaces nothing in the reference. */
#define MSL_LOSS_UP_FWD 0       /* msl_<kind>_up_fwd: k_loss_fwd + k_loss_finalize */
#define MSL_LOSS_UP_BWD 1       /* msl_<kind>_up_bwd: k_bwd_rows + k_bwd_cols */
#define MSL_LOSS_UPSAMPLE_BWD 2 /* msl_upsample_bwd: the same two kernels on a given hi-res gradient */
#define MSL_LOSS_UPSAMPLE_FWD 3 /* msl_upsample_fwd */
#define MSL_LOSS_RESIZE 4       /* msl_resize_bilinear */
#define MSL_LOSS_PROB_FWD 5     /* msl_maxsquare_prob_fwd / msl_iw_maxsquare_prob_fwd */
#define MSL_LOSS_PROB_BWD 6
#define MSL_LOSS_SOFT_FWD 7     /* msl_soft_ce_fwd / msl_iw_soft_ce_fwd */
#define MSL_LOSS_SOFT_BWD 8
#define MSL_LOSS_LABELS 9       /* msl_loss_labels_up / msl_pseudo_labels_up */
typedef struct msl_loss_plan_info {
  int status;      /* what the call returns: MSL_OK, MSL_ERR_ARG, MSL_ERR_WORKSPACE or MSL_ERR_SHAPE */
  int cm;          /* the class-count instantiation: 19, 16, 13, or 32 (the generic body); 0 where the kernels
                    * take C at run time (msl_upsample_fwd, msl_resize_bilinear) */
  int fwd_blocks;  /* blocks of the family's flat kernel (256 threads; the forward, or the prob / soft backward) */
  int fwd_trips;   /* trips of its grid-stride loop (1: every thread takes at most one item) */
  int rows_chunks; /* k_bwd_rows: column chunks per hi-res row (the grid is ho x rows_chunks) */
  int per;         /*   low-res columns per chunk */
  int rows_wmax;   /*   the pixel range its LDS is sized for */
  int lds_optin;   /*   1: lds_bytes is above 64 KB and the launch opts in to it */
  int cols_blocks; /* k_bwd_cols: blocks and grid-stride trips */
  int cols_trips;
  int vec;         /* k_upsample_fwd stores float4 (wo % 4 == 0), else scalars */
  int four_tap;    /* msl_resize_bilinear: 1 k_resize_four (ho + wo <= 128), 0 msl_upsample_fwd's kernel */
  long long lds_bytes;   /* k_bwd_rows: dynamic LDS; above 160 KB the call is MSL_ERR_SHAPE */
  long long ws_required; /* the workspace bytes the call needs (0: it takes none) */
} msl_loss_plan_info;
/* c, hi, wi, ho, wo as the call's; the flat families (prob, soft) take hw = ho * wo and ignore hi, wi.  ws_bytes as
 * the call's.  The data pointers count as given.  A refused backward still reports rows_chunks .. lds_bytes; every
 * other field is 0 unless status is MSL_OK.  Returns MSL_ERR_ARG (out untouched) for no out or an unknown family,
 * else MSL_OK with the call's own status in out. */
int msl_loss_plan(int family, int c, int hi, int wi, int ho, int wo, size_t ws_bytes, msl_loss_plan_info* out);

/* ------------------------------------------------------------------------
 * BatchNorm2d fused with the Bottleneck's ReLU / residual add (deeplab_multi.py:31-46,
 * :115-117): y = act(bn(x) [+ residual]), act = ReLU if relu else identity.
 * Layout [c][nimg][p]: nimg images of p = H*W pixels each.
 * training = 1: batch statistics over the p pixels of each channel of each image on its own
 * (bs = 1, quirk Q9: the reference's source and target forwards are separate batches),
 * accumulated in fp64; running stats updated with momentum and the unbiased variance when
 * update_running, image by image in order (exactly nimg sequential bs=1 calls);
 * num_batches_tracked (nullable) += nimg.  training = 0: running statistics (model.eval() /
 * --freeze_bn).  save_mean / save_invstd [c][nimg] are outputs consumed by msl_bn_bwd, which sums
 * dgamma / dbeta image by image in order (as nimg accumulating calls would).
 * ---------------------------------------------------------------------- */
size_t msl_bn_workspace(int c, int p, int nimg);
int msl_bn_fwd(const float* x, const float* gamma, const float* beta, const float* residual,
               float* y, float* running_mean, float* running_var, long long* num_batches_tracked,
               float* save_mean, float* save_invstd, int c, int p, int nimg, int training,
               int update_running, float momentum, float eps, int relu, const msl_forms* forms, void* ws,
               size_t ws_bytes, msl_stream_t stream);
/* dx (nullable), dres = d residual (nullable), dgamma / dbeta (nullable, = or += when
 * accumulate_params: the training step accumulates straight into the flat gradient buffer);
 * y is the forward output (needed when relu). */
int msl_bn_bwd(const float* dy, const float* x, const float* y, const float* gamma,
               const float* save_mean, const float* save_invstd, float* dx, float* dres,
               float* dgamma, float* dbeta, int c, int p, int nimg, int training, int relu,
               int accumulate_params, const msl_forms* forms, void* ws, size_t ws_bytes, msl_stream_t stream);
/* msl_bn_fwd / msl_bn_bwd that also write absmax[c] = max |y[c][.]| (forward) or max |dx[c][.]|
 * (backward; dx required): the per-channel absmax partials (c of them) that the f16x3 conv
 * entry points (_sc) take for the tensor this BN produced - the next conv's input, or the
 * gradient of the conv before it - so those GEMMs need no absmax pass of their own.  The fused
 * kernels reduce it in registers, the split forms in their apply kernel (r05; before: a pass of its
 * own over the output). */
int msl_bn_fwd_am(const float* x, const float* gamma, const float* beta, const float* residual,
                  float* y, float* running_mean, float* running_var, long long* num_batches_tracked,
                  float* save_mean, float* save_invstd, int c, int p, int nimg, int training,
                  int update_running, float momentum, float eps, int relu, const msl_forms* forms, void* ws,
                  size_t ws_bytes, msl_stream_t stream, float* absmax);
int msl_bn_bwd_am(const float* dy, const float* x, const float* y, const float* gamma,
                  const float* save_mean, const float* save_invstd, float* dx, float* dres,
                  float* dgamma, float* dbeta, int c, int p, int nimg, int training, int relu,
                  int accumulate_params, const msl_forms* forms, void* ws, size_t ws_bytes, msl_stream_t stream, float* absmax_dx);
/* msl_bn_bwd_am that may take y = NULL with relu for a BN WITHOUT a residual: the fused kernel
 * then recomputes the ReLU mask from x (y > 0 <=> fma(x, invstd*gamma, fma(-mean, invstd*gamma,
 * beta)) > 0, the forward's own float operations on the saved mean / invstd - with invstd*gamma
 * taken as 0 on a row whose every element equals its mean, as the forward takes it - so the mask is
 * identical) instead of reading y - one read of the map less.  beta = the forward's beta
 * (nullable = 0).  y = NULL needs msl_bn_uses_fused(c, p, training) and p <= 16384 (else
 * MSL_ERR_ARG); with y given it is msl_bn_bwd_am. */
int msl_bn_bwd_am_beta(const float* dy, const float* x, const float* y, const float* gamma,
                       const float* beta, const float* save_mean, const float* save_invstd, float* dx,
                       float* dres, float* dgamma, float* dbeta, int c, int p, int nimg, int training,
                       int relu, int accumulate_params, const msl_forms* forms, void* ws, size_t ws_bytes, msl_stream_t stream,
                       float* absmax_dx);
/* 1 if msl_bn_fwd / msl_bn_bwd run the fused one-block-per-channel kernels for this shape (else the
 * split stats / reduce + flat apply kernels). */
int msl_bn_uses_fused(int c, int p, int training, const msl_forms* forms);
/* The ReLU mask as bits (r05): msl_bn_fwd_mask is msl_bn_fwd_am that also writes y > 0 of every
 * pixel to relu_mask (bit e % 64 of word [row][e / 64], rows c * nimg + image, cdiv(p, 64) words per
 * row: msl_bn_relu_mask_bytes); msl_bn_bwd_mask is msl_bn_bwd_am_beta with relu_mask in place of y,
 * the same mask bit for bit.  For the residual BN + ReLU of a bottleneck (deeplab_multi.py:45-47)
 * the backward then reads 1 bit per pixel instead of the 4-byte block output.  Both need relu and
 * msl_bn_uses_fused(c, p, training, forms) (else MSL_ERR_ARG). */
size_t msl_bn_relu_mask_bytes(int c, int p, int nimg);
int msl_bn_fwd_mask(const float* x, const float* gamma, const float* beta, const float* residual,
                    float* y, float* running_mean, float* running_var, long long* num_batches_tracked,
                    float* save_mean, float* save_invstd, int c, int p, int nimg, int training,
                    int update_running, float momentum, float eps, int relu, const msl_forms* forms, void* ws,
                    size_t ws_bytes, msl_stream_t stream, float* absmax, uint64_t* relu_mask);
int msl_bn_bwd_mask(const float* dy, const float* x, const uint64_t* relu_mask, const float* gamma,
                    const float* beta, const float* save_mean, const float* save_invstd, float* dx, float* dres,
                    float* dgamma, float* dbeta, int c, int p, int nimg, int training, int relu,
                    int accumulate_params, const msl_forms* forms, void* ws, size_t ws_bytes, msl_stream_t stream,
                    float* absmax_dx);

/* The plan of a BN call, as a host-only query: no launch, no pointers to data, usable without a GPU.  It
 * reports what msl_bn_fwd_mask (backward = 0) or the backward entry points (backward = 1) do with these
 * arguments through the very functions the calls use (the refusals, the fused instantiation, the flat kernels'
 * chunk), so it cannot drift from them.  The tests hold every kernel form and option to fp64 through it
 * (tests/bn_form_cases.py).  Additive: ABI 3.  Replaces nothing in the reference. */
typedef struct msl_bn_plan_info {
  int status;   /* what the call returns: MSL_OK, MSL_ERR_ARG or MSL_ERR_WORKSPACE; the rest is 0 unless MSL_OK */
  int fused;    /* 1 the one-block-per-channel kernels (one launch), 0 the flat ones (reduce + apply) */
  int ept;      /* fused: elements per lane of the instantiation, 4, 9, 16 or 33; else 0 */
  int joint;    /* fused: the joint two-image instantiation (nimg = 2), else the image loop */
  int vec;      /* flat: the float4 body (every tensor operand 16-byte aligned), else scalar accesses */
  int S;        /* fp64 partial sums per row (the workspace holds c * nimg * S * 2 doubles) */
  int chunk;    /* elements per block of the flat apply kernels */
  int max_rows; /* flat: the most rows one apply block stages in LDS (<= 256) */
  int launches; /* kernel launches, in order: grid_x x grid_y blocks of `block` threads each */
  int grid_x[2], grid_y[2], block[2];
} msl_bn_plan_info;
/* aligned: every tensor operand the call gives is 16-byte aligned.  Forward: has_mask / has_absmax = relu_mask /
 * absmax given; entry, relu_src and has_dx are 0; the operands and running statistics count as given.
 * Backward: entry 0 msl_bn_bwd / msl_bn_bwd_am, 1 msl_bn_bwd_am_beta, 2 msl_bn_bwd_mask; relu_src = where the
 * ReLU mask comes from: 0 none (relu = 0), 1 y, 2 the mask bits (entry 2 alone), 3 recomputed (y = NULL);
 * has_dx / has_absmax = dx / absmax_dx given; has_mask is 0.  ws_bytes as the call's.  Returns MSL_ERR_ARG
 * (out untouched) for arguments that describe no call, else MSL_OK with the call's own status in out. */
int msl_bn_plan(int backward, int c, int p, int nimg, int training, int relu, int aligned, int entry, int relu_src,
                int has_dx, int has_absmax, int has_mask, size_t ws_bytes, const msl_forms* forms,
                msl_bn_plan_info* out);

/* ------------------------------------------------------------------------
 * Training-time evaluation (tools/train_source.py:280-283 + utils/eval.py:109-118): for one
 * image's prediction pred[c][p] (fp32, the upsampled logits) and label[p] (int64, pixels outside
 * [0, c) ignored), confusion[gt * c + argmax] += 1 over the pixels, on the stream;
 * argmax = np.argmax over classes (lowest index on ties, NaN wins).  argmax_out [p] (int32,
 * nullable) receives the per-pixel argmax.  c <= 64.  Exact, deterministic counts.
 * ---------------------------------------------------------------------- */
int msl_confusion_accumulate(const float* pred, const long long* label, int c, long long p,
                             unsigned long long* confusion, int* argmax_out, msl_stream_t stream);

/* The evaluator's prediction (tools/evaluate.py:114-141) fused with that matrix, from the
 * LOW-resolution head output logits[c][hi][wi]: every hi-res pixel of ho x wo is re-interpolated as
 * the fused losses do (the hi-res logits / probabilities are never written).
 *   logits_flip == NULL: class = np.argmax of up(logits) (lowest index on ties, NaN wins);
 *   logits_flip != NULL (--flip; the low-res logits of the horizontally mirrored image): class =
 *     np.argmax of (softmax(up(logits))[y][x] + softmax(up(logits_flip))[y][wo-1-x]) / 2.
 * argmax_out (int32 [ho*wo], nullable) receives the class; label (int64 [ho*wo]) and confusion
 * (uint64 [c*c], as msl_confusion_accumulate: confusion[gt * c + class] += 1, labels outside [0, c)
 * skipped; exact, deterministic) are given together or both NULL (predict only).  At least one
 * output is required; c <= 32; bad arguments or geometry are MSL_ERR_ARG. */
int msl_predict_up(const float* logits, const float* logits_flip, int c, int hi, int wi, int ho, int wo,
                   const long long* label, unsigned long long* confusion, int32_t* argmax_out,
                   msl_stream_t stream);

/* msl_predict_up without flip, followed by the reference's Trainer.rectification with both of its crops, in one
 * launch.  crop0 / crop1 are the low-resolution logits [c][hi][wi] of the half-size windows at x0 = 0 and
 * x0 = W0 / 2 of the original image, magnified to full size, stylised and forwarded.  Per pixel (y, x) of
 * ho x wo: m, cls = the maximum and its first index of up(base); inside rows segy0 <= y < segy0 + ho/2, with
 * k = x / (wo/2), m', cls' = the same of up(crop_k) at (2 (y - segy0), 2 (x - k wo/2)) - the reference's
 * nearest x1/2 of the crop's prediction - and cls = cls' where m' > m (logits, strict; a NaN on either side
 * keeps cls, as numpy's > does).  Outputs as msl_predict_up.  MSL_ERR_ARG: odd ho or wo, segy0 outside
 * [0, ho/2], c > 32, and msl_predict_up's argument errors. */
int msl_predict_rectify(const float* base, const float* crop0, const float* crop1, int c, int hi, int wi, int ho,
                        int wo, int segy0, const long long* label, unsigned long long* confusion,
                        int32_t* argmax_out, msl_stream_t stream);

/* msl_predict_up's decision written as images, in the same single pass (inputs, label / confusion and
 * the class as there; all maps uint8, all nullable, at least one of them or the confusion matrix required):
 *   class_out  [ho*wo]    the class, the value msl_predict_up writes to argmax_out;
 *   ids_out    [ho*wo]    id_lut[class], id_lut a device uint8 [c] (class -> Cityscapes labelId);
 *   color_out  [ho*wo*3]  palette[class], HWC RGB, palette a device uint8 [c*3];
 *   conf_out   [ho*wo*3]  shade[bucket][class], shade a device uint8 [4*c*3]: bucket 0 where the winning
 *                         probability p > 0.9, else 1 where > 0.8, else 2 where > 0.7, else 3 where > 0.5,
 *                         else black (the splits of the reference's inspect_decode_labels);
 *   pseudo_out [ho*wo]    the class where p > thr, else 255 (the rule of the hard target mode).
 * p is softmax(up(logits)) at its first maximum, with logits_flip the averaged probability the class is
 * taken from; a NaN pixel is black in conf_out and 255 in pseudo_out.  A thread writes four pixels of a
 * row as dwords when wo % 4 == 0 and the outputs are 4-byte aligned, else bytes.  An output whose table
 * is NULL, no output at all, label without confusion, c > 32 or a bad geometry are MSL_ERR_ARG. */
int msl_predict_images(const float* logits, const float* logits_flip, int c, int hi, int wi, int ho, int wo,
                       const long long* label, unsigned long long* confusion, float thr,
                       const uint8_t* id_lut, const uint8_t* palette, const uint8_t* shade,
                       uint8_t* class_out, uint8_t* ids_out, uint8_t* color_out, uint8_t* conf_out,
                       uint8_t* pseudo_out, msl_stream_t stream);

/* Multi-scale / mirror test-time augmentation fused into one launch (--scales, not in the reference).
 * An entry is the LOW-resolution head output of the image at some input scale, or of that rescaled image's
 * horizontal mirror (mirror = 1).  Per pixel (y, x) of ho x wo, in fp32 and in the order of the entries:
 *   acc = sum_k softmax(up_k(logits_k))[y][mirror_k ? wo-1-x : x],   class = np.argmax of acc
 * (lowest index on ties; a NaN pixel is class 0), up_k the align_corners bilinear upsample of entry k's own
 * hi x wi to ho x wo with torch-CPU's rounding, as everywhere here.  Two entries (L, 0), (Lf, 1) are
 * msl_predict_up's --flip rule bit for bit.  The entry array is host memory, read during the call and
 * passed to the kernel by value: nothing has to outlive the call and a captured graph holds its own copy.
 * MSL_ERR_ARG before any launch: entries NULL, n outside [1, msl_predict_tta_max_entries()], an entry with
 * NULL logits, hi < 1, wi < 1 or mirror outside {0, 1}, c outside [1, 32], a size below 1 or
 * ho * wo >= 2^31, no output at all, label without confusion or the reverse, an image map whose table is
 * NULL. */
typedef struct msl_tta_entry {
  const float* logits; /* [c][hi][wi] on the device */
  int hi, wi, mirror;
} msl_tta_entry;
int msl_predict_tta_max_entries(void); /* 16 */
/* label / confusion / argmax_out as msl_predict_up. */
int msl_predict_tta(const msl_tta_entry* entries, int n, int c, int ho, int wo, const long long* label,
                    unsigned long long* confusion, int32_t* argmax_out, msl_stream_t stream);
/* The same class written as msl_predict_images' five maps from the same tables, four pixels of a row per
 * thread under the same alignment rule; the winning probability behind conf_out and pseudo_out is
 * acc[class] / n. */
int msl_predict_tta_images(const msl_tta_entry* entries, int n, int c, int ho, int wo, const long long* label,
                           unsigned long long* confusion, float thr, const uint8_t* id_lut,
                           const uint8_t* palette, const uint8_t* shade, uint8_t* class_out, uint8_t* ids_out,
                           uint8_t* color_out, uint8_t* conf_out, uint8_t* pseudo_out, msl_stream_t stream);

/* Class-balanced pseudo-label thresholds (--threshold_mode class; CBST, BDL; not in the reference, whose
 * train_round() opens with "# generate threshold" and assigns the constant).  Additive: ABI 3.
 *
 * msl_confidence_hist: per pixel of ho x wo, k = the class msl_predict_up gives from the same inputs, top =
 * the probability behind msl_predict_images' pseudo_out, b = min(bins - 1, (int)(top * (float)bins)) in fp32,
 * and hist[k * bins + b] += 1 (uint64 [c*bins] on the device).  A NaN pixel is not counted.  hist
 * accumulates across calls: the caller zeroes it once per pass.  Integer atomics: exact, the same bytes on
 * every run.  msl_confidence_hist_tta is the same over an entry table (k, top as msl_predict_tta_images).
 * MSL_ERR_ARG before any launch: NULL logits or hist, c outside [1, 32], bins not a power of two in
 * [16, 1024], c * bins > 16384 (the per-block LDS tile), msl_predict_up's geometry errors or
 * msl_predict_tta's table errors. */
int msl_confidence_hist(const float* logits, const float* logits_flip, int c, int hi, int wi, int ho, int wo,
                        int bins, unsigned long long* hist, msl_stream_t stream);
int msl_confidence_hist_tta(const msl_tta_entry* entries, int n, int c, int ho, int wo, int bins,
                            unsigned long long* hist, msl_stream_t stream);

/* One threshold per class from such a histogram, one block, nothing read by the host.  Per class k: N = the
 * row's sum, need = (uint64)ceil(portion * (double)N), b* = the largest bin index whose suffix sum
 * sum_{b >= b*} hist[k][b] reaches need (need == 0: b* = bins), q = (float)b* / (float)bins and
 * thr[k] = min(thr_max, q); N == 0 gives thr_max.  So every class keeps at least `portion` of its pixels and
 * no threshold exceeds thr_max (portion 0.5, thr_max 0.9: BDL's rule).  kept (uint64 [c], nullable) receives
 * sum_{b >= floor(thr[k] * bins)} hist[k][b].  thr is a device fp32 [c].
 * MSL_ERR_ARG: a NULL hist or thr, portion outside [0, 1], thr_max outside (0, 1], the size errors above. */
int msl_class_thresholds(const unsigned long long* hist, int c, int bins, double portion, float thr_max,
                         float* thr, unsigned long long* kept, msl_stream_t stream);

/* The pseudo-label under those thresholds, k and top as above: label[px] (int64 [ho*wo], nullable) =
 * top > thr[k] ? k : -1 (strict; a NaN pixel is -1), pseudo[px] (uint8 [ho*wo], nullable) the same with 255
 * for -1; at least one of them.  thr is read from device memory by the kernel, so a captured launch picks up
 * new values.  Four pixels of a row per thread; pseudo is stored as dwords when wo % 4 == 0 and it is
 * 4-byte aligned.  MSL_ERR_ARG: NULL logits or thr, no output, the geometry / table errors above. */
int msl_pseudo_classwise(const float* logits, const float* logits_flip, int c, int hi, int wi, int ho, int wo,
                         const float* thr, long long* label, uint8_t* pseudo, msl_stream_t stream);
int msl_pseudo_classwise_tta(const msl_tta_entry* entries, int n, int c, int ho, int wo, const float* thr,
                             long long* label, uint8_t* pseudo, msl_stream_t stream);

/* decode_labels (datasets/cityscapes_Dataset.py:352-377) on the device: out[px] = palette[cls[px]] for
 * the npx elements of a class map (int64 when is_int64, else int32), out uint8 [npx*3] HWC RGB, palette a
 * device uint8 [c*3], c <= 256; values outside [0, c), -1 included, are black. */
int msl_colorize(const void* cls, int is_int64, long long npx, const uint8_t* palette, int c, uint8_t* out,
                 msl_stream_t stream);

/* Per-image analysis (the reference's tools/analysis.py), decided on the device.
 *
 * msl_image_metrics: one image's scores from image_cm, the uint64 [c*c] matrix its prediction launch just
 * filled (confusion[gt * c + class]), by the definitions of utils/eval.py:Eval.  Row sums r, column sums
 * s, the diagonal d and the total are exact uint64 sums converted to fp64 once; per class acc = d / r and
 * iou = d / (r + s - d), 0/0 = NaN as in numpy (each bit-equal to numpy's); PA = trace / total, 0 when
 * total is 0; MPA and MIoU the nan-means, summed by one thread in class order, NaN when every class is;
 * FWIoU = sum of r * iou over the non-NaN classes / total.  For c == 16 also the three 13-class values
 * over synthia_set_16_to_13 (FWIoU_13 divides by the same total).  Row state[0] % capacity of rows
 * (fp64 [capacity][9 + c]) receives
 *   [PA, MPA, MIoU, FWIoU, MPA_13, MIoU_13, FWIoU_13, pixels, selected, iou[0..c-1]]
 * (the _13 fields NaN unless c == 16; pixels = total), selected = (m < threshold) ? 1 : 0 with m the MIoU
 * utils/validate.py:val_info returns (the 13-class one for 16 classes): strict, a NaN is not selected.  Then
 * total_cm += image_cm, image_cm = 0, and state (three device ints {cursor, selected, slot}) becomes
 * {cursor + 1, selected, cursor % capacity}.  One 256-thread block, nothing read by the host.
 * MSL_ERR_ARG before any launch: a NULL pointer, c outside [1, 32], capacity < 1. */
int msl_image_metrics(unsigned long long* image_cm, unsigned long long* total_cm, int c, double threshold,
                      double* rows, int capacity, int* state, msl_stream_t stream);

/* msl_analysis_maps: the maps of an image msl_image_metrics selected, all uint8 [h*w*3] HWC RGB, all
 * nullable, at least one required:
 *   label_out  palette[label] for a label in [0, c), else black (decode_labels);
 *   pred_out   palette[cls], cls the uint8 [h*w] class map of msl_predict_images (class_out);
 *   input_out  channel 2-k of clamp(rint(x[k] + mean[k]), 0, 255), round half to even, NaN -> 0, x the fp32
 *              network input [3][h][w] (BGR - mean), mean a device fp32 [3]: utils/images.py:recover_input;
 *   error_out  black where the label is outside [0, c), input_out >> 1 per byte where cls == label,
 *              palette[cls] where they differ.
 * palette is a device uint8 [c*3].  With state (msl_image_metrics') every thread first reads state[1] and
 * returns on 0 before any other load or store - the device-side gate - and otherwise every map is written
 * at out + state[2] * slot_stride (bytes); state == NULL always writes, at out.  A thread takes four pixels
 * of a row: float4 loads and dword stores when w % 4 == 0, x is 16-byte and cls, the outputs and slot_stride
 * 4-byte aligned, else scalar loads and byte stores.
 * MSL_ERR_ARG before any launch: no output, an input NULL that a requested map reads (label: label_out,
 * error_out; x, mean: input_out, error_out; cls: pred_out, error_out; palette: all but input_out), c outside
 * [1, 32], h or w < 1, h * w >= 2^31, slot_stride < 0. */
int msl_analysis_maps(const float* x, const float* mean, const long long* label, const uint8_t* cls,
                      const uint8_t* palette, int c, int h, int w, const int* state, long long slot_stride,
                      uint8_t* label_out, uint8_t* pred_out, uint8_t* input_out, uint8_t* error_out,
                      msl_stream_t stream);

/* ------------------------------------------------------------------------
 * Input pipeline (the loaders' last host steps, on the device after a uint8 H2D copy; byte-exact):
 *   msl_image_transform: out[c][y][x] = (float)rgb[y][xs][2 - c] - mean[c] (BGR order, mean =
 *     IMG_MEAN = {B, G, R}), xs = mirror ? w-1-x : x; rgb is uint8 HWC, out fp32 CHW
 *     (datasets/cityscapes_Dataset.py:14, 245-251 _img_transform with numpy_transform; the
 *     random_mirror FLIP_LEFT_RIGHT of _train_sync_transform);
 *   msl_label_transform: out[y][x] = lut256[ids[y][xs]] as int64 (trainId, -1 = ignore): the
 *     dataset's id_to_trainid composed with its 16/13-class remap (cityscapes_Dataset.py:124-155,
 *     260-264 id2trainId / _mask_transform; gta5_Dataset.py:73-75; synthia_Dataset.py:56-62).
 *     lut256 is a device int32[256] table.
 * ---------------------------------------------------------------------- */
int msl_image_transform(const uint8_t* rgb, int h, int w, int mirror, float mean_b, float mean_g,
                        float mean_r, float* out, msl_stream_t stream);
int msl_label_transform(const uint8_t* ids, int h, int w, int mirror, const int32_t* lut256,
                        int64_t* out, msl_stream_t stream);

/* ------------------------------------------------------------------------
 * Pillow-exact resampling (the loaders' Image.transpose / crop / resize, on the device; byte-exact
 * against Pillow's 8-bit paths; datasets/cityscapes_Dataset.py:173-243).  The crop (x0, y0, cw, ch)
 * is taken from the mirrored source (crop column x = source column mirror ? sw-1-(x0+x) : x0+x) and
 * resized to (ow, oh); the tables are built for the CROP size (utils/resample.py).
 *   msl_resize_bicubic_rgb: Image.BICUBIC on uint8 HWC RGB.  One pass per axis,
 *       out = clamp((2^21 + sum_k px[first+k] * coeff[k]) >> 22, 0, 255), horizontal first into a uint8
 *       intermediate (ws, msl_resize_workspace(ch, ow) bytes, needed only when both axes resize),
 *       then vertical.  Per axis: xb / yb = HOST int32 [out][2] = (first, taps), read during the call
 *       only (validated before anything is launched, and sizes the launch); xk / yk = DEVICE int32
 *       [2 + ks][out] = row 0 the first taps, row 1 the tap counts, rows 2.. the ks 22-bit
 *       coefficients of every output (transposed, so a wave's loads are contiguous); ks in 1..64.  Both NULL = no pass on that axis (then ow == cw / oh == ch).  The kernels clamp every
 *       row's taps to the crop, so a device table that disagrees with the host bounds cannot read
 *       outside the source.  Outputs (at least one): out_u8 uint8 HWC (oh, ow, 3); out_f32 fp32
 *       (3, oh, ow) BGR - mean, as msl_image_transform, written by the last pass.
 *   msl_resize_nearest_label: Image.NEAREST on a uint8 id map, a gather through xtab / ytab (DEVICE
 *       int32 [ow] / [oh] source indices, clamped to the crop by the kernel; NULL = identity, then
 *       ow == cw / oh == ch).  Outputs (at least one): out_u8 the raw ids (oh, ow); out_i64 =
 *       lut256[id] (device int32[256], required with out_i64).
 * MSL_ERR_ARG, before any launch: a crop outside the source, host bounds that leave the crop, ks
 * outside 1..64, a missing table half, no output, a short workspace, a dimension over 65535.
 * ---------------------------------------------------------------------- */
size_t msl_resize_workspace(int ch, int ow);
int msl_resize_bicubic_rgb(const uint8_t* src, int sh, int sw, int x0, int y0, int cw, int ch, int mirror,
                           const int32_t* xb, const int32_t* xk, int xks, const int32_t* yb, const int32_t* yk,
                           int yks, int ow, int oh, uint8_t* out_u8, float* out_f32, float mean_b, float mean_g,
                           float mean_r, void* ws, size_t ws_bytes, msl_stream_t stream);
int msl_resize_nearest_label(const uint8_t* ids, int sh, int sw, int x0, int y0, int cw, int ch, int mirror,
                             const int32_t* xtab, const int32_t* ytab, int ow, int oh, const int32_t* lut256,
                             uint8_t* out_u8, int64_t* out_i64, msl_stream_t stream);

/* ------------------------------------------------------------------------
 * PNG unfilter of one byte lane (SYNTHIA's 16-bit label PNGs, synthia_Dataset.py:88-90: the reference
 * keeps the low byte of R; the host inflates, the device undoes the scanline filters).
 * scan: DEVICE inflated scanlines, row r at scan + r * row_stride = its filter byte, then w * bpp filtered
 * bytes.  out: DEVICE (h, w) uint8 = byte `lane` of every reconstructed pixel, per the PNG specification:
 * None, Sub, Up as written there, Average = floor((a + b) / 2) on the 9-bit sum, Paeth with ties broken
 * in the order a, b, c; all mod 256; neighbours outside the image are 0.  PNG filters byte i from bytes
 * i - bpp of the same row and i, i - bpp of the row above - the same lane of the neighbouring pixels -
 * so one lane needs only itself (with the compacted plane of utils/png.py lane_plane: bpp = 1, lane = 0,
 * row_stride = 1 + w).
 * One launch of one workgroup, stream-ordered, no host synchronisation; every loop count and barrier
 * of the kernel is a function of (h, w) alone.  msl_png_unfilter_band_rows() = the rows one pass of the
 * kernel holds (taller images run as successive bands; for the tests).
 * A filter byte above 4 cannot be seen from the host side of this call: the kernel treats such a row as
 * None (filter 0) and reads nothing out of range (utils/png.py refuses such a file before any upload).
 * MSL_ERR_ARG, before any launch: a NULL pointer, h or w < 1 or over 65535, bpp outside 1..8,
 * lane >= bpp (or negative), row_stride < 1 + w * bpp.
 * ---------------------------------------------------------------------- */
int msl_png_unfilter_lane(const uint8_t* scan, int h, int w, int bpp, int lane, size_t row_stride, uint8_t* out,
                          msl_stream_t stream);
int msl_png_unfilter_band_rows(void);

/* ------------------------------------------------------------------------
 * SGD step with the reference's duplicated-parameter semantics (quirk Q2):
 * torch.optim.SGD(momentum, weight_decay) single-tensor loop over the
 * optim_parameters() groups (train_source.py:139-144, deeplab_multi.py:132-171),
 * where a parameter listed k times receives k sequential updates sharing one
 * momentum buffer.  One launch updates every entry.
 * ---------------------------------------------------------------------- */
typedef struct msl_sgd_entry {
  float* param;       /* updated in place */
  const float* grad;  /* read-only */
  float* momentum;    /* momentum buffer, updated in place */
  long long numel;
  int mult;           /* occurrences of this parameter in its group (1, 3 or 4) */
  int group;          /* 0: backbone (lr), 1: ASPP heads (10*lr) */
  int has_buf;        /* 0 on the parameter's first step (buffer created = d) */
  int pad_;
} msl_sgd_entry;

/* entries and block_entry live in device memory; block_entry[b] is the entry
 * processed by block b (chunks of msl_sgd_block_elems() elements), built by
 * msl_sgd_plan on the host. */
int msl_sgd_block_elems(void);
long long msl_sgd_plan(const long long* numels, int n_entries, int32_t* block_entry_host,
                       long long* block_offset_host, long long max_blocks);
int msl_sgd_step(const msl_sgd_entry* entries, const int32_t* block_entry,
                 const long long* block_offset, long long n_blocks, float lr0, float lr1,
                 float momentum, float weight_decay, float grad_scale, msl_stream_t stream);
/* The same step with the two group learning rates read from device memory (lr_dev[0] = group 0,
 * lr_dev[1] = group 1) when the kernel runs, so a captured hipGraph replays the poly schedule
 * (train_source.py:706-717) by updating lr_dev between replays. */
int msl_sgd_step_lr_dev(const msl_sgd_entry* entries, const int32_t* block_entry,
                        const long long* block_offset, long long n_blocks, const float* lr_dev,
                        float momentum, float weight_decay, float grad_scale, msl_stream_t stream);

/* ------------------------------------------------------------------------
 * Adam with the same duplicated-parameter semantics: torch.optim.Adam(params,
 * betas, eps, weight_decay) (amsgrad=False, L2 weight decay; train_source.py:145-146),
 * single-tensor loop, where a parameter listed k times receives k sequential
 * updates sharing exp_avg, exp_avg_sq and the step counter, which advances by k.
 * Per update:  step += 1;  d = g*grad_scale + wd*p;  m += (1-b1)*(d-m);
 * v = v*b2 + (1-b2)*d*d;  p -= lr/(1-b1^step) * m / (sqrt(v)/sqrt(1-b2^step) + eps).
 * ---------------------------------------------------------------------- */
typedef struct msl_adam_entry {
  float* param;       /* updated in place */
  const float* grad;  /* read-only */
  float* exp_avg;     /* first moment, updated in place */
  float* exp_avg_sq;  /* second moment, updated in place */
  float* step;        /* DEVICE fp32 scalar: updates applied so far (torch's state['step']); advanced by mult */
  long long numel;
  int mult;           /* occurrences of this parameter in its group: 1..msl_adam_max_mult() */
  int group;          /* 0: backbone (lr), 1: ASPP heads (10*lr) */
} msl_adam_entry;

/* The block plan is msl_sgd_plan's (chunks of msl_sgd_block_elems() elements).  A step is two
 * launches on `stream`: one thread per entry reads the entry's counter and its group's rate,
 * computes in double lr/(1-b1^t) and sqrt(1-b2^t) for t = step+1 .. step+mult, rounds them to
 * fp32 into coef (DEVICE, msl_adam_coef_bytes(n_entries) bytes: [n_entries][msl_adam_max_mult()][2]
 * floats, no initialisation needed) and stores step + mult; the element kernel then reads coef only,
 * never the counters, so no block sees a counter that another block of the step has advanced, and
 * a captured hipGraph replays the pair with the counters advancing on the device.  mult above
 * msl_adam_max_mult() (4) is applied as 4.  beta1, beta2, eps are doubles as torch holds them
 * (1-beta rounded to fp32 once).  MSL_ERR_ARG: a NULL table or coef, a negative count, a beta
 * outside [0, 1), eps < 0.  n_blocks == 0 launches no element kernel (MSL_OK). */
int msl_adam_max_mult(void);
size_t msl_adam_coef_bytes(int n_entries);
int msl_adam_step(const msl_adam_entry* entries, int n_entries, const int32_t* block_entry,
                  const long long* block_offset, long long n_blocks, float lr0, float lr1, double beta1,
                  double beta2, double eps, float weight_decay, float grad_scale, float* coef,
                  msl_stream_t stream);
/* The same step with the two group learning rates read from device memory (by the coefficient
 * launch) when the step runs, as msl_sgd_step_lr_dev. */
int msl_adam_step_lr_dev(const msl_adam_entry* entries, int n_entries, const int32_t* block_entry,
                         const long long* block_offset, long long n_blocks, const float* lr_dev,
                         double beta1, double beta2, double eps, float weight_decay, float grad_scale,
                         float* coef, msl_stream_t stream);

/* ------------------------------------------------------------------------
 * AdaIN style pass (the reference's utils/style_transform.py over tools/net.py), everything but its 3x3
 * convs, which are msl_dconv_fwd.  One image per call, [C][H][W] fp32.
 *
 * The reference pads every conv by reflection; msl_dconv_fwd pads with zeros.  A stage's input is
 * therefore written WITH its reflected border as a padded grid [C][H+2][W+2], the conv runs over the
 * whole grid (dilation 1), and only the interior [1..H] x [1..W] of its output is read afterwards: interior
 * outputs touch the grid's own cells only, border outputs are finite and ignored.  An input `x` with
 * x_grid = 1 is such a grid, read through its interior; with x_grid = 0 a plain [C][H][W] tensor.
 * Every entry point checks its arguments before any launch: a NULL pointer, a size <= 0, a flag out of
 * range or a tensor of 2^31 or more cells is MSL_ERR_ARG, a shape the operation is undefined on
 * MSL_ERR_SHAPE.
 * ---------------------------------------------------------------------- */
/* y[cpad][ho+2][wo+2] = reflect_pad1(resample(f(x))), one launch.
 *   resample  0 none (ho = h), 1 the 2x2 stride-2 ceil-mode max-pool (ho = ceil(h/2); the last window of
 *             an odd axis holds one row / column), 2 nearest x2 (ho = 2h); wo likewise
 *   a, b      both NULL, or DEVICE arrays of c floats: the per-channel affine a_c * v + b_c (the multiply
 *             and the add rounded separately); without them the kernel does no arithmetic
 *   act       0: f(v) = a v + b;  1: f(v) = relu(a v + b);  2: f(v) = a relu(v) + b (the AdaIN affine
 *             over the encoder's last ReLU)
 *   cpad      >= c channels of y; the ones past c are zero (a caller pads a conv's cin with them)
 * Without the affine every cell is a copy or a max of inputs, bit-identical to torch's ReLU,
 * MaxPool2d((2,2),(2,2),(0,0),ceil_mode=True), Upsample(scale_factor=2, mode='nearest') and
 * ReflectionPad2d(1) (ReLU keeps -0.0; of equal window values the first in row-major order stays).
 * MSL_ERR_SHAPE: h < 2 or w < 2, or ho < 2 or wo < 2 (reflection needs two rows and two columns). */
int msl_style_pad(const float* x, int x_grid, int c, int h, int w, int act, int resample, const float* a,
                  const float* b, float* y, int cpad, msl_stream_t stream);
/* y[cpad][h+2][w+2] = reflect_pad1(W1 v + b1): the encoder's leading 1x1 conv 3 -> 3 (w1: DEVICE [3][3],
 * b1: DEVICE [3]) as a per-pixel affine, the channels past 3 zero.  v is exactly one of rgb_u8 (uint8
 * [h][w][3] RGB, divided by 255 as torchvision's ToTensor does) and chw_f32 (float [3][h][w] in [0, 1]).
 * MSL_ERR_SHAPE: h < 2 or w < 2. */
int msl_style_input(const uint8_t* rgb_u8, const float* chw_f32, int h, int w, const float* w1, const float* b1,
                    float* y, int cpad, msl_stream_t stream);
/* stats[0..c) = the mean and stats[c..2c) = the unbiased variance of each channel over its h*w pixels,
 * of relu(x) when `relu`.  Values are reduced as differences from the channel's first pixel (a large mean
 * with a small spread keeps its variance), in batches of 8 by the corrected two-pass sum in registers, merged
 * by Chan's update through wave shuffles and LDS; channels of more than 8192 pixels take a second launch over
 * the blocks' moments in `ws` (msl_style_stats_workspace bytes, 0 for smaller channels; MSL_ERR_WORKSPACE if
 * short).  No atomics: the same input gives the same bits.  MSL_ERR_SHAPE: h*w < 2. */
size_t msl_style_stats_workspace(int c, int h, int w);
int msl_style_stats(const float* x, int x_grid, int c, int h, int w, int relu, float* stats, void* ws,
                    size_t ws_bytes, msl_stream_t stream);
/* The AdaIN affine of a content map toward nstyle weighted styles, one launch, no host sync:
 *   a_c = alpha * (sum_i w_i ss_i) / sc + (1 - alpha),  b_c = alpha * (sum_i w_i ms_i - mc * (sum_i w_i ss_i) / sc)
 * with m the mean and s = sqrt(var + eps) of content_stats [2][c] and style_stats [nstyle][2][c] (DEVICE,
 * as msl_style_stats writes them); `weights` is a HOST array of nstyle floats (the reference's
 * interpolation_weights; {1} for one style), 1 <= nstyle <= msl_style_max_styles() (16).  alpha = 0 gives
 * a = 1, b = 0 exactly.  MSL_ERR_ARG: alpha outside [0, 1], eps < 0. */
int msl_style_max_styles(void);
int msl_style_adain_coef(const float* content_stats, const float* style_stats, const float* weights, int nstyle,
                         int c, float alpha, float eps, float* a, float* b, msl_stream_t stream);
/* From a 3-channel RGB map x (the decoder's output), q = clamp(x * 255 + 0.5, 0, 255) rounded as torch's
 * mul(255).add(0.5).clamp(0, 255), into either or both of
 *   rgb_u8   uint8 [h][w][3] RGB = uint8(q): torchvision save_image's quantisation
 *   seg_bgr  float [3][h][w] = q of B, G, R minus mean_b, mean_g, mean_r, not truncated: the reference's
 *            Trainer.seg_transform, the segmentation network's input */
int msl_style_output(const float* x, int x_grid, int h, int w, uint8_t* rgb_u8, float* seg_bgr, float mean_b,
                     float mean_g, float mean_r, msl_stream_t stream);

/* In-loop domain adaptation (the reference's tools/ADAIN.py; cropTrans, Trainer.seg_transform and
 * Trainer.rectification of tools/train_source.py): what sits between the style network and the segmentation
 * network.  "torch-nearest" below is F.interpolate's default mode: the source index of destination d on an
 * axis resized from `in` to `out` cells is min((int)floorf(d * scale), in - 1), scale = (float)in / (float)out
 * formed in fp32 by these entry points, the product one rounded fp32 multiply.  One image per call, on the
 * stream, no host sync, no atomics; arguments are checked before any launch.
 *
 * msl_style_input reading the window (x0, y0, cw, ch) of an ih x iw image (uint8 [ih][iw][3] or float
 * [3][ih][iw], exactly one of them), magnified to h x w by torch-nearest: the grid y[cpad][h+2][w+2], bit for
 * bit msl_style_input of the gathered image.  MSL_ERR_ARG: a window outside the image; MSL_ERR_SHAPE: h or
 * w below 2. */
int msl_style_input_window(const uint8_t* rgb_u8, const float* chw_f32, int ih, int iw, int x0, int y0, int cw,
                           int ch, int h, int w, const float* w1, const float* b1, float* y, int cpad,
                           msl_stream_t stream);
/* msl_style_output's seg_bgr of the h x w map x, gathered by torch-nearest into the window (dx0, dy0, dw, dh)
 * of seg_bgr[3][hd][wd]; cells outside the window are not written.
 *   one map  (full_h = full_w = 0; mid = (dh, dw), off = 0): the window is x resized to dh x dw - the
 *            reference's seg_transform when seg_size != base_size;
 *   two maps (full_h, full_w > 0): x is first resized to mid_h x mid_w and placed at (off_y, off_x) of a
 *            stitched map of full_h x full_w, which is then resized to hd x wd - cropTrans followed by
 *            seg_transform, the indices composed.  A window cell whose stitched source lies outside this
 *            image's mid_h x mid_w part is left alone, so the window may be any cover of the image's share.
 * The quantisation is pointwise and commutes with the gather: the values are those of interpolate, then
 * mul(255).add(0.5).clamp(0, 255), minus the mean, in B, G, R.  MSL_ERR_ARG: a window outside the
 * destination, a part outside the stitched map, one map with mid != (dh, dw). */
int msl_style_output_resampled(const float* x, int x_grid, int h, int w, int mid_h, int mid_w, int full_h, int full_w,
                               int off_y, int off_x, float* seg_bgr, int hd, int wd, int dx0, int dy0, int dw, int dh,
                               float mean_b, float mean_g, float mean_r, msl_stream_t stream);
/* out[ho][wo] = label[h][w] resized by torch-nearest (int64 trainIds; the reference interpolates its float
 * label map in seg_transform). */
int msl_label_resize_nearest(const long long* label, int h, int w, long long* out, int ho, int wo,
                             msl_stream_t stream);

/* ------------------------------------------------------------------------
 * Baseline JPEG decode, split between host and device (the reference's crosscity_Dataset.py:74
 * `Image.open(image_path).convert("RGB")` on NTHU's 2048x1024 JPEGs).  The host parses the markers and
 * Huffman-decodes the scan into quantised coefficients (serial); the device dequantises, runs libjpeg's
 * JDCT_ISLOW inverse DCT, upsamples the chroma planes by libjpeg's fancy rules and converts YCbCr -> RGB
 * (dense), byte-exact against libjpeg-turbo's defaults, i.e. against Pillow.
 *
 * Supported: 8-bit precision, SOF0 / SOF1 (Huffman), one interleaved scan of 3 components libjpeg takes for
 * YCbCr (a JFIF marker; else an Adobe marker with transform 1; else component ids other than 'R','G','B')
 * with luma sampling 1x1, 2x1 or 2x2 and both chroma 1x1 - or one grayscale component.  Every other valid
 * file (progressive, arithmetic, lossless, hierarchical, 12-bit, 4 components, RGB-coded, other sampling
 * factors, several scans, DNL) is MSL_ERR_SHAPE; a corrupt or truncated stream is MSL_ERR_ARG.  The two host
 * entry points are thread-safe, keep no state, use no GPU, never read past file[n) and never write
 * outside coef[0, coef_elems) and quant[0, 256).
 * ---------------------------------------------------------------------- */
typedef struct {
  int32_t h, v;               /* sampling factors (a lone grayscale component is 1, 1 whatever the file says) */
  int32_t tq;                 /* its quantisation table, 0..3 */
  int32_t blocks_w, blocks_h; /* its block grid: whole MCUs, blocks_w = ceil(width / (8 hmax)) * h */
  int32_t reserved;
  int64_t offset;             /* of its first coefficient in the coefficient buffer, in int16 elements */
} msl_jpeg_comp;

typedef struct {
  int32_t width, height;
  int32_t ncomp;              /* 1 (grayscale) or 3 (YCbCr) */
  int32_t hmax, vmax;         /* the luma sampling factors */
  int32_t restart_interval;   /* MCUs between restart markers, 0 = none */
  int32_t mcus_w, mcus_h;
  msl_jpeg_comp comp[3];
} msl_jpeg_header;

/* Parse the markers up to the scan header and fill *header.  Host only. */
int msl_jpeg_info(const uint8_t* file, size_t n, msl_jpeg_header* header);
/* int16 elements of the coefficient buffer: 64 per block of every component, [comp][block row][block col][64]. */
size_t msl_jpeg_coef_elems(const msl_jpeg_header* header);
/* Parse, fill *header, Huffman-decode the scan into coef (HOST, caller-owned - a pinned staging buffer -
 * coef_elems >= msl_jpeg_coef_elems elements, MSL_ERR_WORKSPACE if fewer): each block's 64 quantised
 * coefficients in natural (de-zigzagged) order, the DC prediction resolved, restart markers honoured; and
 * quant (HOST, uint16 [4][64], natural order; tables the file does not define are zero).  Host only. */
int msl_jpeg_entropy_decode(const uint8_t* file, size_t n, msl_jpeg_header* header, int16_t* coef,
                            size_t coef_elems, uint16_t* quant);
/* Bytes of msl_jpeg_reconstruct's workspace: the components' uint8 planes of whole blocks. */
size_t msl_jpeg_workspace(const msl_jpeg_header* header);
/* coef / quant (DEVICE copies of what msl_jpeg_entropy_decode wrote, coef 16-byte aligned) -> rgb (DEVICE
 * uint8 [height][width][3]), two launches on `stream`:
 *   1. per 8x8 block: coefficient * table entry, libjpeg's jidctint.c (CONST_BITS 13, PASS1_BITS 2: the column
 *      pass descaled by 11, the row pass by 18, DESCALE(x, n) = (x + (1 << (n-1))) >> n), clamp(x + 128, 0,
 *      255), into the component's plane in ws;
 *   2. per pixel: the chroma planes upsampled by libjpeg-turbo's fancy h2v1 / h2v2 rules (a chroma plane of
 *      width <= 2 is box-replicated, as libjpeg selects), YCbCr -> RGB in libjpeg's 16-bit fixed point,
 *      cropped to width x height; grayscale writes Y three times.
 * Before any launch: MSL_ERR_ARG for a NULL pointer, a misaligned coef, a header that is not one
 * msl_jpeg_info writes (sampling, tables, a block grid or offsets that disagree with the size) or
 * ws_bytes < msl_jpeg_workspace(header); MSL_ERR_SHAPE above 2^28 pixels. */
int msl_jpeg_reconstruct(const int16_t* coef, const uint16_t* quant, const msl_jpeg_header* header, uint8_t* rgb,
                         void* ws, size_t ws_bytes, msl_stream_t stream);
/* The kernels' tiles: 8x8 blocks per workgroup of launch 1, pixels per workgroup of launch 2. */
int msl_jpeg_tile_blocks(void);
int msl_jpeg_tile_pixels(void);

/* Diagnostics (r06): the launch guard every entry point runs before each kernel launch (MSL_ERR_LAUNCH
 * when a block exceeds the kernel's __launch_bounds__).  Launches a 256-thread-bound probe kernel with
 * `threads` threads writing out[t] = t: MSL_OK (and out[0 .. threads) written) for 1 <= threads <= 256,
 * MSL_ERR_LAUNCH (nothing launched, out untouched) above.  Replaces nothing in the reference. */
int msl_launch_guard_probe(int threads, float* out, msl_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MSL_HIP_H */
