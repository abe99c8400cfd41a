/* dfm_hip_sparse_train.h -- the part of the C ABI of libdfm_hip.so that TRAINS the sparse encoder of the LiDAR
 * teacher (configs/dfm/second_teacher.py): the backward of the sparse convolutions of dfm_hip_sparse_conv.h and a
 * training-mode BatchNorm1d over the live rows of a sparse tensor, fp32.  Included by dfm_hip.h (inside its
 * extern "C" block, after dfm_hip_sparse_conv.h, whose row / table conventions it shares): include that header, not
 * this one.  Bound by depth-from-motion_amd/_capi.py through SPARSE_TRAIN_SIGNATURES.
 *
 * Conventions.  Rows (N, C) fp32 plus coors (N, 4) int32 (b, z, y, x); a row with b < 0 does not exist: it is never
 * read (it may hold any bit pattern, NaNs included) and every gradient written for it is exactly 0.  All checks (NULL
 * pointers, channel counts, row counts, alignment) happen before any HIP call: DFM_ERR_INVALID_ARG or
 * DFM_ERR_UNSUPPORTED.  No kernel here uses a floating-point atomic: every sum has one fixed order, so every result is
 * the same bits run after run.
 *
 * live_rows (the three reductions take it; NULL: none): one int32 ON THE DEVICE, the caller's promise that every row
 * at or past *live_rows has b < 0 -- the output of a strided layer has a row bound of many times its live rows, and
 * sparse_conv.py sorts them to the front in training mode.  The reductions then stop there: the same bits as without
 * it, since the rows left out do not exist.  The host never reads the count.
 *
 * Input gradient of a convolution: grad_in[r] = sum_k W[k] . grad_out[inv[k][r]] is dfm_sparse_conv_fwd itself, called
 * with the per-offset transposed weight (taps, Cout, Cin), the INVERSE table inv[k][in_row] = out_row (-1: none) and
 * the input coordinates; it covers Cin in {16, 32, 64}.  A SubMConv3d needs no inverse table (inv[k] = nbr[26 - k]),
 * nor does a 1x1x1 layer (a row reads the same row). */
#ifndef DFM_HIP_SPARSE_TRAIN_H
#define DFM_HIP_SPARSE_TRAIN_H
#ifndef DFM_HIP_H
#error "include dfm_hip.h: it defines DFM_API and the status codes, and includes this header"
#endif

#define DFM_SPARSE_WGRAD_CHUNK 256 /* output rows per partial of the weight gradient */
#define DFM_SPARSE_BN_CHUNK 256    /* rows per partial of the BatchNorm reductions */

/* inv (taps, in_rows) int32, filled with -1 by the caller: inv[k][nbr[k][o]] = o for every entry of nbr (taps,
 * out_rows) in [0, in_rows).  One plain store per entry: "every (input row, offset) names at most one output site"
 * (dfm_hip_sparse_conv.h), so no two entries store to one place. */
DFM_API int dfm_sparse_inverse_table(const int32_t *nbr, int32_t taps, int64_t out_rows, int64_t in_rows, int32_t *inv,
                                     void *stream);

/* bytes of the weight gradient's workspace: ceil(out_rows / CHUNK) * taps partial tiles of (round16(cin), cout)
 * floats, then one int32 flag per (chunk, offset); 0 for sizes the kernel refuses */
DFM_API size_t dfm_sparse_conv_wgrad_workspace_bytes(int32_t cin, int32_t cout, int32_t taps, int64_t out_rows);
/* Weight gradient: grad_weight (taps, cin, cout), dW[k] = sum over live output rows r of in[nbr[k][r]]^T . grad_out[r]
 * on v_mfma_f32_16x16x4_f32, the row axis being the contraction.  nbr (taps, out_rows) or NULL (taps = 1: row r reads
 * row r where out_coors[r].b >= 0).  A wave sums one (chunk of DFM_SPARSE_WGRAD_CHUNK rows, offset, 16 input
 * channels): the four-row MFMA steps go round-robin, in ascending row order, to 8 accumulators (4 at cout = 64) that
 * are added as a fixed binary tree -- one accumulator would be one fused multiply-add chain as long as the chunk --
 * and the partial goes to the workspace; a second kernel adds the partials in ascending chunk order, in fp64, and
 * rounds once.  A (chunk, offset) in which no row has that neighbour is skipped in both (its partial would be zeros: no
 * bit changes).  cin: 3 or a multiple of 4 up to 64; cout: 16, 32 or 64.  in, grad_out, grad_weight and the
 * workspace 4-byte aligned floats; out_coors 16-byte aligned.  out_rows = 0: grad_weight = 0. */
DFM_API int dfm_sparse_conv_wgrad(int32_t cin, int32_t cout, int32_t taps, const float *in, int64_t in_rows,
                                  const int32_t *nbr, const int32_t *out_coors, int64_t out_rows,
                                  const float *grad_out, float *grad_weight, void *workspace, size_t workspace_bytes,
                                  const int32_t *live_rows, void *stream);

/* BatchNorm1d in training mode over the live rows of x (rows, channels), channels in {16, 32, 64}.
 * bytes of the workspace of dfm_sparse_bn_stats / dfm_sparse_bn_bwd_reduce: ceil(rows / DFM_SPARSE_BN_CHUNK) * channels
 * * 3 floats; 0 for sizes the kernels refuse */
DFM_API size_t dfm_sparse_bn_workspace_bytes(int64_t rows, int32_t channels);
/* stats (channels, 3) = (live count, mean, M2 = sum (x - mean)^2) per channel, the payload group_norm.py exchanges
 * between ranks.  Two stages, both in a fixed order: Welford per thread, Chan's merge over the threads of a block in
 * ascending row-slot order, then over the blocks in ascending order.  A live count of 0 gives (0, 0, 0). */
DFM_API int dfm_sparse_bn_stats(const float *x, const int32_t *coors, int64_t rows, int32_t channels, float *stats,
                                void *workspace, size_t workspace_bytes, const int32_t *live_rows, void *stream);
/* y = (x - mean) * rstd * weight + bias, rstd = 1 / sqrt(M2 / max(count, 1) + eps), then optional ReLU, on live rows;
 * a row with b < 0 is written as zeros.  weight / bias: NULL for 1 / 0. */
DFM_API int dfm_sparse_bn_apply(const float *x, const int32_t *coors, int64_t rows, int32_t channels,
                                const float *stats, const float *weight, const float *bias, float eps, int32_t relu,
                                float *y, void *stream);
/* sums (2, channels): sums[0] = sum of g over live rows (grad_bias), sums[1] = sum of g * xhat (grad_weight), where
 * g = grad_y masked by the ReLU (y > 0, recomputed from x as the apply kernel computes it).  Same two stages. */
DFM_API int dfm_sparse_bn_bwd_reduce(const float *x, const float *grad_y, const int32_t *coors, int64_t rows,
                                     int32_t channels, const float *stats, const float *weight, const float *bias,
                                     float eps, int32_t relu, float *sums, void *workspace, size_t workspace_bytes,
                                     const int32_t *live_rows, void *stream);
/* grad_x = weight * rstd * (g - sums[0] / n - xhat * sums[1] / n), n = max(count, 1), on live rows; zeros on the
 * others */
DFM_API int dfm_sparse_bn_bwd_apply(const float *x, const float *grad_y, const int32_t *coors, int64_t rows,
                                    int32_t channels, const float *stats, const float *sums, const float *weight,
                                    const float *bias, float eps, int32_t relu, float *grad_x, void *stream);
/* running_mean = (1 - momentum) * running_mean + momentum * mean, running_var likewise with the unbiased variance
 * M2 / max(count - 1, 1), each as one multiplication, one multiplication and one addition; a live count of 0 leaves
 * both unchanged.  On the device: the count is never read by the host. */
DFM_API int dfm_sparse_bn_running(const float *stats, int32_t channels, float momentum, float *running_mean,
                                  float *running_var, void *stream);

/* dense() backward: grad_features (rows, channels) = grad_volume (batch, channels, D, H, W) at the coordinates of the
 * live rows, zeros on the others */
DFM_API int dfm_sparse_dense_bwd(const float *grad_volume, const int32_t *coors, int64_t rows, int32_t channels,
                                 int32_t batch, const int32_t *size3, float *grad_features, void *stream);

#endif /* DFM_HIP_SPARSE_TRAIN_H */
