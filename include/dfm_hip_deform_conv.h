/* dfm_hip_deform_conv.h -- the part of the C ABI of libdfm_hip.so that runs the modulated deformable convolution
 * (DCNv2) of the Waymo configs' ResNet-101 (dcn=dict(type='DCNv2', deform_groups=1), stages 3 and 4).  Included by
 * dfm_hip.h (inside its extern "C" block, after DFM_API, the status codes and dfm_dtype): include that header, not
 * this one.  Bound by depth-from-motion_amd/_capi.py through DEFORM_CONV_SIGNATURES. */
#ifndef DFM_HIP_DEFORM_CONV_H
#define DFM_HIP_DEFORM_CONV_H
#ifndef DFM_HIP_H
#error "include dfm_hip.h: it defines DFM_API and the status codes, and includes this header"
#endif

/* ---------------------------------------------------------------------- */
/* modulated deformable 3x3 convolution: mmcv's modulated_deform_conv2d     */
/* (mmcv/ops/modulated_deform_conv.py over modulated_deform_conv_cuda_      */
/* kernel.cuh: dmcn_im2col_bilinear, dmcn_get_gradient_weight,              */
/* dmcn_get_coordinate_weight).  mmcv is not a dependency: the semantics    */
/* are the ones stated here, and tests/golden/make_golden_deform_conv.py    */
/* restates them in torch.                                                  */
/* ---------------------------------------------------------------------- */
/* Operands.  x (N, Cin, H, W); weight (Cout, Cin, 3, 3); offset (N, 2 * 9 * G, Ho, Wo); mask (N, 9 * G, Ho, Wo);
 * G = deform_groups divides Cin; Ho = (H + 2 pad_h - (2 dil_h + 1)) / stride_h + 1, Wo alike.
 *   tap k = 3 i + j (i the kernel row, j the kernel column);
 *   offset channel g * 18 + 2 k is the ROW (y) displacement of tap k for deform group g, g * 18 + 2 k + 1 the COLUMN
 *   (x) displacement (mmcv's order); mask channel g * 9 + k; channel c of x belongs to group c / (Cin / G).
 *
 * Sampling, all FP32, one IEEE rounding per operation written, no contraction (-ffp-contract=off):
 *   h = float(ho * stride_h - pad_h + i * dil_h) + dy          (the integer part is exact; ONE addition)
 *   w = float(wo * stride_w - pad_w + j * dil_w) + dx
 *   inside = h > -1 && w > -1 && h < H && w < W                 (false for a NaN; false for +-inf and +-1e30)
 *   not inside: the sample is 0, and so is every gradient through it (grad_offset, grad_mask, grad_x).
 *   inside: h0 = floor(h), lh = h - h0, hh = 1 - lh; w0, lw, hw alike.  The conversion of h0 and w0 to an integer
 *     happens after the test only: -1 <= h0 <= H - 1.
 *     v00 = x[h0][w0], v01 = x[h0][w0 + 1], v10 = x[h0 + 1][w0], v11 = x[h0 + 1][w0 + 1]; a corner outside the map is 0.
 *     val = (((hh * hw) * v00 + (hh * lw) * v01) + (lh * hw) * v10) + (lh * lw) * v11
 *   m = mask, or with mask_is_logit  m = 1 / (1 + expf(-mask))  (IEEE division)
 *   col[n][ho][wo][k][c] = val * m.
 * The convolution itself is a matrix product the caller runs:
 *   out[n][co][ho][wo] = bias[co] + sum over (k, ci) of weight[co][ci][k] * col[n][ho][wo][k][ci].
 *
 * Derivatives: those of exactly this floor formula.
 *   d val / d h = hw * (v10 - v00) + lw * (v11 - v01),   d val / d w = hh * (v01 - v00) + lh * (v11 - v10)
 * At an integer coordinate (lh = 0) that is the right-hand difference v[h0 + 1] - v[h0], as mmcv's
 * dmcn_get_coordinate_weight gives it: conv_offset is zero-initialised, so the first steps of a training sample on
 * the integers. */
typedef struct dfm_deform_desc {
    int32_t n, cin, h, w;       /* x */
    int32_t ho, wo;             /* must be the output size of the geometry below */
    int32_t stride_h, stride_w; /* >= 1 */
    int32_t pad_h, pad_w;       /* >= 0 */
    int32_t dil_h, dil_w;       /* >= 1 */
    int32_t deform_groups;      /* G >= 1; Cin / G must be a whole number of 16-byte vectors of dtype */
    int32_t mask_is_logit;      /* 1: the sigmoid is applied here, and grad_mask is the gradient of the logit */
    int32_t dtype;              /* DFM_F32 | DFM_BF16: x, col, grad_col */
    int32_t om_dtype;           /* DFM_F32 | DFM_BF16: offset and mask */
    int64_t offset_stride[4];   /* ELEMENT strides of offset along (n, channel, ho, wo) */
    int64_t mask_stride[4];     /* of mask.  A raw (N, 27 G, Ho, Wo) conv_offset map is passed as it is: offset = the
                                 * map, mask = the map + 18 G channels, both with the map's strides */
} dfm_deform_desc;

/* The columns.
 * x   : (N, H, W, Cin) -- an NCHW tensor in channels-last memory format --, dtype, 16-byte aligned      [device]
 * col : (N, Ho, Wo, 9, Cin) contiguous, dtype, 16-byte aligned, EVERY element written once.  A DFM_BF16 column is
 *       the FP32 value above rounded once.
 * One launch.  A workgroup takes 16 consecutive output pixels of the flattened (N, Ho, Wo) axis: it computes the
 * coordinates, the four weights and the mask of its 144 (pixel, tap) pairs once into LDS, then every lane blends
 * one 16-byte channel vector of one pair at a time: the four corners are whole 16-byte loads of Cin contiguous
 * values, the store is 16 bytes into a run of 9 * Cin contiguous values per pixel.
 * DFM_ERR_INVALID_ARG, before any HIP call: a NULL or misaligned pointer, a size < 1, ho / wo that are not the output
 * size, G not dividing Cin.  DFM_ERR_UNSUPPORTED: Cin / G not a whole number of 16-byte vectors, N * Ho * Wo or
 * N * H * W above 2^31 - 1, a coordinate range (Ho * stride + pad + 2 * dil) above 2^24, an unknown dtype. */
DFM_API int dfm_deform_sample_fwd(const dfm_deform_desc *desc, const void *x, const void *offset, const void *mask,
                                  void *col, void *stream);

/* From the gradient of the columns to the gradients of offset, mask and x.
 * grad_col    : (N, Ho, Wo, 9, Cin) contiguous, dtype                                                  [device]
 * grad_offset : FP32, element strides grad_offset_stride[4] (HOST array) along (n, channel, ho, wo), channels as
 *               offset's; grad_mask likewise with the mask's channels; both NULL: not computed.  Every element is
 *               written once (allocate with empty).  With mask_is_logit, grad_mask = d / d logit.
 *                 grad_offset[.., g * 18 + 2 k] = m * sum over the group's c of grad_col[k][c] * d val[c] / d h
 *                 grad_mask  [.., g * 9 + k]    =     sum over the group's c of grad_col[k][c] * val[c]  (* m (1 - m))
 *               The sums run over 64 channels at a time in one wave: a lane's product, a fixed xor-shuffle tree,
 *               chunks added in ascending order -- no atomics: the same bits run after run.
 * grad_x      : (N, H, W, Cin) FP32, ADDED to (the caller zeroes it), or NULL: not computed.  grad_x[corner][c] +=
 *               grad_col[k][c] * m * (the corner's weight).  Float atomics: the order of the additions, and so the
 *               last bits, vary from run to run.
 * One launch.  A workgroup of eight waves takes a TH x TW tile of output pixels of one image (8 x 8 at stride 1) and
 * walks the channels of a group 64 at a time, one wave per (pixel, tap), with the next pair's loads in flight.  Per
 * chunk it keeps an LDS window of the input -- the tile's footprint at zero offsets, (TH - 1) * stride + 2 * dil + 1
 * rows, plus a margin of m rows on each side, columns alike, x 64 floats -- and adds every corner that lands inside it
 * with an LDS atomic; corners outside go to global atomics directly, in a pass of their own after the main loop
 * (whose only global memory operations are then its loads).  The window is then flushed: its non-zero entries
 * as global atomics, 64 consecutive lanes on 64 consecutive channels (256 contiguous bytes per wave instruction).
 * Tile and margin are the first of 8x8, 4x8, 4x4, 2x4, 2x2, 1x1, each with m = 2 and then m = 1, whose window fits
 * 54 KiB (stride 1, dilation 1: 8x8 with m = 2, offsets within +-2 stay on chip; stride 2: 4x8 with m = 1); if none
 * does every corner goes to global memory.
 * Errors as dfm_deform_sample_fwd; also DFM_ERR_INVALID_ARG when only one of grad_offset / grad_mask is NULL or
 * a stride array is missing. */
DFM_API int dfm_deform_conv_bwd_cols(const dfm_deform_desc *desc, const void *x, const void *offset, const void *mask,
                                     const void *grad_col, float *grad_offset, const int64_t *grad_offset_stride,
                                     float *grad_mask, const int64_t *grad_mask_stride, float *grad_x, void *stream);

#endif /* DFM_HIP_DEFORM_CONV_H */
