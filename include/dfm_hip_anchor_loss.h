/* dfm_hip_anchor_loss.h -- the part of the C ABI of libdfm_hip.so that computes the 3-D anchor head's loss_single.
 * Included by dfm_hip.h (inside its extern "C" block, after DFM_API, the status codes and the dtypes): include that
 * header, not this one.  Bound by depth-from-motion_amd/_capi.py. */
#ifndef DFM_HIP_ANCHOR_LOSS_H
#define DFM_HIP_ANCHOR_LOSS_H
#ifndef DFM_HIP_H
#error "include dfm_hip.h: it defines DFM_API and the status codes, and includes this header"
#endif

/* ---------------------------------------------------------------------- */
/* Anchor3DHead.loss_single / LIGAAnchor3DHead.loss_single                  */
/* (models/dense_heads/anchor3d_head.py:199-301,                            */
/* liga_anchor3d_head.py:130-226): the focal, smooth-L1, direction and IoU  */
/* terms of one level, read from the head's maps in place                   */
/* ---------------------------------------------------------------------- */
#define DFM_ANCHOR_LOSS_MAX_CODE 16     /* the widest box code */
typedef struct dfm_anchor_loss_desc {
    int32_t batch;                /* B */
    int32_t h, w;                 /* the BEV map of this level */
    int32_t anchors_per_location; /* A = sizes x rotations */
    int32_t num_classes;          /* C >= 1 (sigmoid classification: one logit per class) */
    int32_t box_code_size;        /* S, 7 .. 16 */
    int32_t dtype;                /* of the three maps and of their gradients: DFM_F32 or DFM_BF16 */
    int32_t has_dir;              /* the head has a direction classifier: the dir map is read, out[2] is computed */
    int32_t with_iou;             /* the IoU term: anchors are read, out[3] is computed; needs S == 7 */
    int32_t diff_rad_by_sin;      /* add_sin_difference on column 6 */
    int32_t reserved;             /* 0 */
    float gamma, alpha;           /* the focal loss */
    float beta;                   /* the smooth-L1 loss, > 0 */
    float code_weight[DFM_ANCHOR_LOSS_MAX_CODE];   /* per box column, the first S are read; all 1 without one */
    int64_t cls_stride[4];        /* ELEMENT strides (image, channel, row, column) of each map: NCHW-contiguous, */
    int64_t reg_stride[4];        /* channels-last or any other strided view is read in place */
    int64_t dir_stride[4];
    int64_t grad_cls_stride[4];   /* the same of the three gradient maps (dfm_anchor3d_loss_bwd only) */
    int64_t grad_reg_stride[4];
    int64_t grad_dir_stride[4];
} dfm_anchor_loss_desc;
/* Semantics.
 * Layout: that of dfm_hip_bbox_decode.h.  N = h * w * A anchors per image; anchor n = (y * w + x) * A + a, the order
 * of the reference's permute(0, 2, 3, 1).reshape(-1, .) of each map, so that of anchor n of image b
 *     class logit c     is cls[b][a * C + c][y][x],        c in [0, C)
 *     delta column s    is reg[b][a * S + s][y][x],        s in [0, S)
 *     direction logit j is dir[b][a * 2 + j][y][x],        j in {0, 1}.
 * A bf16 map is read as the FP32 value of each element; all arithmetic is FP32.
 * Targets, the dense tensors anchor_target_3d returns for the level, contiguous, row r = b * N + n:     [device]
 *     labels (B, N) int64, label_weights (B, N) FP32, bbox_targets and bbox_weights (B, N, S) FP32,
 *     dir_targets (B, N) int64 (0 is class 0, anything else class 1), dir_weights (B, N) FP32 (both unread without
 *     has_dir), anchors (N, S) FP32, one set shared by the images (unread without with_iou).
 * Positives: row r is positive iff 0 <= labels[r] < C.  Any other label, C included, is a row whose classes are all
 * negative (the reference's assert labels.max().item() <= C is a wait for the host and is not made).
 * Term sums, each an FP32 sum over the B * N rows:
 *   S_cls = sum_r sum_c label_weights[r] * focal(x_c, t_c), t_c = 1 iff labels[r] == c, mmdet's
 *           py_sigmoid_focal_loss in its binary_cross_entropy_with_logits form: with p = sigmoid(x) and
 *           pt = (1 - p) t + p (1 - t),
 *               focal = (alpha t + (1 - alpha) (1 - t)) pt^gamma bce(x, t),
 *               bce(x, t) = max(x, 0) - x t + log1p(exp(-|x|)).
 *           Computed from e = exp(-|x|) alone (p and 1 - p as 1 / (1 + e) and e / (1 + e), bce as a sum of two
 *           non-negative parts), so value and gradient are finite for every finite logit; the gradient is
 *           (+-) (alpha or 1 - alpha) pt^gamma (gamma (1 - pt) bce + pt), a sum of non-negative parts.
 *           gamma == 2 takes pt * pt, any other gamma powf(pt, gamma).
 *   S_box = sum_pos sum_{s < S} bbox_weights[r][s] code_weight[s] smooth_l1(p_s - t_s; beta),
 *           smooth_l1(d) = 0.5 d^2 / beta for |d| < beta, |d| - 0.5 beta otherwise; with diff_rad_by_sin the pair
 *           (p_6, t_6) is replaced by (sin(p_6) cos(t_6), cos(p_6) sin(t_6)).
 *   S_dir = sum_pos dir_weights[r] (logsumexp(d_0, d_1) - d_{dir_target});  0 without has_dir.
 *   S_iou = sum_pos (1 - IoU3D(decode(anchors[n], deltas of the map), decode(anchors[n], bbox_targets[r]))), the
 *           rows of dfm_iou3d_loss_from_deltas: the same device function (csrc/iou3d_geom.h), the same NaN-target
 *           rule, the same bits per row;  0 without with_iou.
 * out (4) FP32 [device]: out[i] = scale[i] * S_i, i = cls, box, dir, iou.  scale (4) FP32 [device] is
 *           loss_weight_i / avg_factor_i, made by the caller on the device: no average factor comes to the host.
 *           Without a positive row S_box = S_dir = S_iou = 0 exactly, and so are their gradients.
 * Forward: two launches -- one lane per row, the four terms summed per wave by shuffles and per workgroup through
 *           LDS into one partial row of the workspace; then one workgroup adds the partial rows (lane t the rows
 *           t, t + 1024, ... in ascending order, then a tree over the lanes) and writes out.  No atomics, no memset, a
 *           fixed order of addition: the same bits run after run.  No host synchronisation.  The count depends on
 *           neither N, B nor the number of positives.  The lanes take the rows of an image anchor-fastest when
 *           cls_stride[1] <= cls_stride[3] (channels-last) and pixel-fastest otherwise (NCHW), so that a wave reads
 *           contiguous runs of the class map either way: the order of addition, and with it the last bits of out,
 *           follows the layout; the gradients do not depend on it.
 * Backward (dfm_anchor3d_loss_bwd): one launch, one lane per row, over the same inputs and grad_out (4) FP32
 *           [device]: grad_map = sum_i grad_out[i] scale[i] dS_i / dmap.  Every element of grad_cls, grad_reg and
 *           grad_dir is written exactly once (allocate with empty), in the maps' dtype (FP32 to bf16: round to
 *           nearest even) at the strides grad_*_stride.  Rows that are not positive get exactly 0 in grad_reg and
 *           grad_dir; rows with label_weights[r] == 0 get exactly 0 in grad_cls.  A NULL gradient pointer skips that
 *           map.
 * workspace: dfm_anchor3d_loss_workspace_bytes(desc) (16 bytes per 256 rows), 16-byte aligned, caller-owned.
 * B == 0 or N == 0: DFM_OK, nothing is launched; the forward sets out to zeros (one memset on `stream`).
 * DFM_ERR_UNSUPPORTED, before any HIP call: S outside 7 .. 16, S != 7 with with_iou, C < 1, another dtype,
 * N * B > 2^31 - 1 (the workspace query returns 0 for these). */
DFM_API size_t dfm_anchor3d_loss_workspace_bytes(const dfm_anchor_loss_desc *desc);
DFM_API int dfm_anchor3d_loss_fwd(const dfm_anchor_loss_desc *desc, const void *cls, const void *reg, const void *dir,
                                  const int64_t *labels, const float *label_weights, const float *bbox_targets,
                                  const float *bbox_weights, const int64_t *dir_targets, const float *dir_weights,
                                  const float *anchors, const float *scale, float *out, void *workspace,
                                  size_t workspace_bytes, void *stream);
DFM_API int dfm_anchor3d_loss_bwd(const dfm_anchor_loss_desc *desc, const void *cls, const void *reg, const void *dir,
                                  const int64_t *labels, const float *label_weights, const float *bbox_targets,
                                  const float *bbox_weights, const int64_t *dir_targets, const float *dir_weights,
                                  const float *anchors, const float *scale, const float *grad_out, void *grad_cls,
                                  void *grad_reg, void *grad_dir, void *stream);

#endif /* DFM_HIP_ANCHOR_LOSS_H */
