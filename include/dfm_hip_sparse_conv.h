/* dfm_hip_sparse_conv.h -- the part of the C ABI of libdfm_hip.so that runs the frozen LiDAR teacher of the KITTI
 * configs (lidar_model=dict(type='VoxelNet', ...)): hard voxelization and the sparse 3-D convolutions of
 * CustomSparseEncoder, forward only, eval only.  Included by dfm_hip.h (inside its extern "C" block, after DFM_API and
 * the status codes): include that header, not this one.  Bound by depth-from-motion_amd/_capi.py through
 * SPARSE_CONV_SIGNATURES. */
#ifndef DFM_HIP_SPARSE_CONV_H
#define DFM_HIP_SPARSE_CONV_H
#ifndef DFM_HIP_H
#error "include dfm_hip.h: it defines DFM_API and the status codes, and includes this header"
#endif

/* ---------------------------------------------------------------------- */
/* Hard voxelization: the reference's points_to_voxel(reverse_index=True)  */
/* (core/voxel/voxel_generator.py), which mmcv's deterministic             */
/* Voxelization kernel restates.  All three results are bit-identical to   */
/* it and the same bits run after run.                                     */
/* ---------------------------------------------------------------------- */
/* Rules.  Point i of sample b has cell c[j] = floor((p[j] - lo[j]) / vs[j]) for j = x, y, z: fp32 subtraction, IEEE
 * fp32 division, floor.  It is dropped when c[j] < 0 or c[j] >= grid[j] is true on any axis or c[j] is a NaN.
 * Voxels of a sample are numbered by the first appearance of a point, in point order; a voxel whose number would be
 * >= max_voxels is dropped with all its points; a voxel keeps its first max_num_points points in point order; unused
 * slots are zero.
 *
 * The work is four kernels around a stable sort and two prefix sums that the caller runs (torch or rocPRIM):
 *   dfm_voxel_keys  : key[i] = ((b * gz + cz) * gy + cy) * gx + cx, or DFM_VOXEL_NO_KEY for a dropped point
 *   (caller)        : (sorted_key, perm) = stable ascending sort of key: a voxel's points are one run, in point order
 *   dfm_voxel_heads : first[perm[i]] = 1 where i starts a run (so the point is the voxel's first), else 0;
 *                     head[i] = i there, else 0
 *   (caller)        : first_scan = inclusive sum of first over points; head_scan = inclusive max of head
 *   dfm_voxel_keep  : keep[p] = first[p] and the voxel's number within its sample < max_voxels
 *   (caller)        : keep_scan = inclusive sum of keep; its last element is the number of rows M, on the device
 *   dfm_voxel_fill  : row = keep_scan[first point] - 1; slot = i - head_scan[i]; copies the point, writes
 *                     coors[row] = (b, cz, cy, cx) and num_points[row] = min(run length, max_num_points)
 * Rows are therefore in first-appearance order, sample after sample.  The caller zeroes voxels and num_points and
 * fills coors with -1 before dfm_voxel_fill: a row past M has batch index -1 ("does not exist", below). */
#define DFM_VOXEL_NO_KEY INT64_MAX
#define DFM_VOXEL_MAX_BATCH 64

typedef struct dfm_voxel_desc {
    int32_t batch;                             /* 1 .. DFM_VOXEL_MAX_BATCH */
    int32_t ndim;                              /* floats per point, 3 .. 16 */
    int32_t grid[3];                           /* cells along x, y, z; the product times batch < 2^62 */
    int32_t max_num_points, max_voxels;        /* >= 1 */
    float lo[3], vs[3];                        /* x, y, z: range minimum, voxel size (> 0) */
    int64_t offset[DFM_VOXEL_MAX_BATCH + 1];   /* sample b is points [offset[b], offset[b + 1]); offset[0] = 0,
                                                * ascending; offset[batch] = N < 2^31 */
} dfm_voxel_desc;

/* points (N, ndim) fp32; key, sorted_key (N) int64; perm, head, head_scan (N) int64; first, keep (N) int32;
 * first_scan, keep_scan (N) int64; voxels (rows, max_num_points, ndim) fp32; coors (rows, 4) int32;
 * num_points (rows) int32, rows = batch * max_voxels.  All device pointers.  N = 0: success, nothing
 * launched.  DFM_ERR_INVALID_ARG, before any HIP call: a NULL pointer, a size out of the ranges above. */
DFM_API int dfm_voxel_keys(const dfm_voxel_desc *desc, const float *points, int64_t *key, void *stream);
DFM_API int dfm_voxel_heads(const dfm_voxel_desc *desc, const int64_t *sorted_key, const int64_t *perm, int32_t *first,
                            int64_t *head, void *stream);
DFM_API int dfm_voxel_keep(const dfm_voxel_desc *desc, const int32_t *first, const int64_t *first_scan, int32_t *keep,
                           void *stream);
DFM_API int dfm_voxel_fill(const dfm_voxel_desc *desc, const float *points, const int64_t *sorted_key,
                           const int64_t *perm, const int64_t *head_scan, const int32_t *keep,
                           const int64_t *keep_scan, float *voxels, int32_t *coors, int32_t *num_points, void *stream);

/* ---------------------------------------------------------------------- */
/* Sparse convolution: spconv's SubMConv3d and SparseConv3d as mmcv 1.x    */
/* wraps them.  mmcv is not a dependency: the semantics are the ones       */
/* stated here, and tests/golden/make_golden_lidar_teacher.py restates     */
/* them as dense masked convolutions.                                      */
/* ---------------------------------------------------------------------- */
/* Sparse tensor.  Rows (N, C) fp32 plus coors (N, 4) int32 (b, z, y, x), unique among the rows with b >= 0; a row
 * with b < 0 does not exist: it is never read, never indexed, and its output row is not written.
 * SubMConv3d (k = 3): the output row set equals the input row set; out[r] = sum over the 27 offsets k of
 *   W[k]^T . in[nbr(r, k)] over the active neighbours; offset k = (kz * 3 + ky) * 3 + kx reads the input at
 *   (z + kz - 1, y + ky - 1, x + kx - 1).  The padding argument is ignored, as in spconv.
 * SparseConv3d (kernel / stride / padding per axis): the output grid is (in + 2 p - k) / s + 1 per axis (floor); an
 *   output site is active iff its receptive field holds an active input; the value is the dense convolution's value
 *   there: offset k = (kz * KH + ky) * KW + kx of output o reads the input at o * s - p + (kz, ky, kx).
 * A 1x1x1 stride-1 SparseConv3d is a row-wise matrix product on the same row set (nbr = NULL below).
 * Weight layout: mmcv 1.x's (kD, kH, kW, Cin, Cout), no bias.
 * Epilogue: acc * scale[c] + shift[c] (one multiplication, one addition, no contraction), then optional ReLU, on
 *   active rows only; scale and shift are the eval-mode BatchNorm (eps = 1e-3) folded in fp32 by the caller, NULL for
 *   none.  The weights are not rewritten.  Inactive sites of the dense result are exactly 0.
 * The order of output rows is unspecified: only dense() and the (coordinate -> row) relation are contractual.
 *
 * Coordinate index: an open-addressing hash table over the key ((b * D + z) * H + y) * W + x (int64), linear probing,
 * capacity a power of two >= 2 * the row bound, empty slot = -1, inserts by a 64-bit atomicCAS issued from the vector
 * unit.  EVERY probe loop stops after DFM_SPARSE_MAX_PROBES slots (or the capacity): a row that finds no slot, an
 * output row past the row bound, a coordinate outside the grid or a duplicate coordinate sets a bit of the device
 * status word and is left out -- nothing spins.  The caller reads the word when it chooses to (one host wait).
 * Neighbour tables: nbr[k][row] int32, -1 for absent.  Neighbour arithmetic runs on the unpacked (z, y, x) with a
 * range test per axis, never on the linear key: a neighbour past a grid border, or in the next sample, is absent.
 * Strided output rows: every (input row, offset) names at most one output site; the sites go into a second table,
 * the insert that wins a slot takes the next row number from an atomic counter and writes the row's coordinate.
 * Row bound: rows_in * prod(ceil(k / s)), capped by batch * the output grid's cells.  The live count stays on the
 * device; a tile of the convolution whose rows all have b < 0 exits.
 * Convolution: output-stationary.  A wave owns 16 output rows; for each kernel offset in ascending k -- skipped when
 * none of the 16 rows has that neighbour, which changes no bit since the skipped products are zeros -- it gathers the
 * 16 neighbour rows by index into LDS (zeros for absent), multiplies with v_mfma_f32_16x16x4_f32 over the channels in
 * ascending order (exact fp32, a fused multiply-add chain per output element), then applies the epilogue and stores
 * each row once.  No atomics on feature data: a row's sum has one fixed order, so the dense result is the same bits
 * run after run and under any permutation of the input rows (finite weights).  Cin = 3 is padded to 4 with zeros. */
#define DFM_SPARSE_MAX_PROBES 1024
#define DFM_SPARSE_MAX_TAPS 27 /* kD * kH * kW */
#define DFM_SPARSE_STATUS_TABLE_FULL 1 /* a probe loop ran out */
#define DFM_SPARSE_STATUS_DUPLICATE 2  /* two input rows with one coordinate */
#define DFM_SPARSE_STATUS_ROW_BOUND 4  /* more output rows than the bound */
#define DFM_SPARSE_STATUS_COORDINATE 8 /* a row with b >= batch or a coordinate outside the grid */

typedef struct dfm_sparse_conv_desc {
    int32_t batch;                                     /* >= 1 */
    int32_t in_size[3];                                /* D, H, W of the input grid, >= 1 */
    int32_t kernel[3], stride[3], padding[3];          /* per axis z, y, x: >= 1, >= 1, >= 0; k <= in + 2 p */
    int32_t subm;                                      /* 1: SubMConv3d (kernel 3, output grid = input grid) */
} dfm_sparse_conv_desc;

typedef struct dfm_sparse_conv_plan {
    int32_t out_size[3];   /* the output grid */
    int32_t taps;          /* kD * kH * kW */
    int64_t out_rows;      /* the output row bound */
    int64_t in_capacity;   /* slots of the table over the input rows */
    int64_t out_capacity;  /* slots of the table over the output sites (0 for subm) */
} dfm_sparse_conv_plan;

/* Host only: the plan of one layer over in_rows input rows (a bound; rows with b < 0 count).  Every loop bound of
 * the kernels follows from it and is checked here, before the first launch.
 * DFM_ERR_INVALID_ARG: NULL, a size < 1, stride < 1, padding < 0, k > in + 2 p, in_rows < 0, subm with a kernel other
 * than 3.  DFM_ERR_UNSUPPORTED: more than DFM_SPARSE_MAX_TAPS offsets, a key space batch * D * H * W (input or output
 * grid) of 2^62 or more, a row bound of 2^31 - 1 or more (rows are int32). */
DFM_API int dfm_sparse_conv_out_shape(const dfm_sparse_conv_desc *desc, int64_t in_rows, dfm_sparse_conv_plan *plan);
/* bytes of the layer's tables: both hash tables (8-byte keys, 4-byte rows) and the neighbour table; 0 when
 * dfm_sparse_conv_out_shape fails */
DFM_API size_t dfm_sparse_conv_workspace_bytes(const dfm_sparse_conv_desc *desc, int64_t in_rows);

/* Table over the rows of coors (rows, 4).  table_keys (capacity) int64 filled with -1 and table_rows (capacity) int32
 * by the caller; status: one int32, or-ed into.  capacity: a power of two >= 2 * rows (INVALID_ARG otherwise). */
DFM_API int dfm_sparse_index_build(const int32_t *coors, int64_t rows, int32_t batch, const int32_t *size3,
                                   int64_t *table_keys, int32_t *table_rows, int64_t capacity, int32_t *status,
                                   void *stream);
/* nbr (27, rows) of a SubMConv3d over the table above: every element written */
DFM_API int dfm_sparse_subm_neighbours(const int32_t *coors, int64_t rows, int32_t batch, const int32_t *size3,
                                       const int64_t *table_keys, const int32_t *table_rows, int64_t capacity,
                                       int32_t *nbr, void *stream);
/* Output rows of a SparseConv3d.  out_keys (plan.out_capacity) int64 filled with -1, out_coors (plan.out_rows, 4)
 * int32 filled with -1 and out_count (one int32) zeroed by the caller. */
DFM_API int dfm_sparse_conv_out_rows(const dfm_sparse_conv_desc *desc, const int32_t *coors, int64_t rows,
                                     int64_t *out_keys, int32_t *out_coors, int32_t *out_count, int32_t *status,
                                     void *stream);
/* nbr (taps, plan.out_rows) of a SparseConv3d: for each output row and offset, the input row there (through the
 * input table) or -1; every element written (rows past the live count: -1) */
DFM_API int dfm_sparse_conv_neighbours(const dfm_sparse_conv_desc *desc, const int32_t *out_coors, int64_t in_rows,
                                       const int64_t *table_keys, const int32_t *table_rows, int32_t *nbr,
                                       void *stream);
/* The convolution.  in (in_rows, cin), weight (taps, cin, cout), nbr (taps, out_rows) or NULL (taps = 1: row r reads
 * row r), out_coors (out_rows, 4), out (out_rows, cout): rows with b < 0 are not written.  scale / shift (cout) or
 * both NULL.  cin: 3 or a multiple of 4 up to 64; cout: 16, 32 or 64 (DFM_ERR_UNSUPPORTED otherwise).  in, weight
 * and out 16-byte aligned unless cin = 3 (in: 4-byte). */
DFM_API int dfm_sparse_conv_fwd(int32_t cin, int32_t cout, int32_t taps, const float *in, int64_t in_rows,
                                const int32_t *nbr, const int32_t *out_coors, int64_t out_rows, const float *weight,
                                const float *scale, const float *shift, int32_t relu, float *out, void *stream);
/* dense(): out (batch, channels, D, H, W) = 0, then one scatter of the rows with b >= 0 */
DFM_API int dfm_sparse_dense(const float *features, const int32_t *coors, int64_t rows, int32_t channels,
                             int32_t batch, const int32_t *size3, float *out, void *stream);

#endif /* DFM_HIP_SPARSE_CONV_H */
