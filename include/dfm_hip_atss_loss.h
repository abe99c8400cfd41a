/* dfm_hip_atss_loss.h -- the part of the C ABI of libdfm_hip.so that computes the 2-D ATSS head's loss over all of
 * its pyramid levels.  Included by dfm_hip.h (inside its extern "C" block, after DFM_API, the status codes, the dtypes
 * and dfm_hip_atss_target.h, whose DFM_ATSS_MAX_LEVELS it uses): include that header, not this one.  Bound by
 * depth-from-motion_amd/_capi.py. */
#ifndef DFM_HIP_ATSS_LOSS_H
#define DFM_HIP_ATSS_LOSS_H
#ifndef DFM_HIP_H
#error "include dfm_hip.h: it defines DFM_API and the status codes, and includes this header"
#endif

/* ---------------------------------------------------------------------- */
/* LIGAATSSHead.loss_single and LIGAATSSHead.centerness_target              */
/* (models/dense_heads/liga_atss_head.py:176-270, 380-397) under mmdet's    */
/* ATSSHead.loss: the focal, centerness-weighted GIoU and centerness terms  */
/* of every level of the batch, read from the head's maps in place          */
/* ---------------------------------------------------------------------- */
typedef struct dfm_atss_loss_desc {
    int32_t batch;                /* B */
    int32_t num_levels;           /* L, 1 .. DFM_ATSS_MAX_LEVELS */
    int32_t num_anchors;          /* A: rows of ONE image in the dense targets and in anchors, the levels concatenated */
    int32_t num_classes;          /* C >= 1 (sigmoid classification: one logit per class) */
    int32_t reg_class_agnostic;   /* != 0: bbox_pred has 4 channels; 0: 4 * C, column s of class c at channel s * C + c */
    int32_t dtype;                /* of the cls_score and centerness maps and their gradients: DFM_F32 or DFM_BF16 */
    int32_t reg_dtype;            /* of the bbox_pred maps and their gradients: DFM_F32 or DFM_BF16 */
    int32_t reserved;             /* 0 */
    float gamma, alpha;           /* the focal loss */
    float target_means[4];        /* DeltaXYWHBBoxCoder */
    float target_stds[4];
    int32_t h[DFM_ATSS_MAX_LEVELS];               /* the map of level l is h[l] x w[l], one anchor per location */
    int32_t w[DFM_ATSS_MAX_LEVELS];
    int32_t row_offset[DFM_ATSS_MAX_LEVELS];      /* off_l: row y * w + x of level l is row off_l + y * w + x of an image */
    int32_t reserved_levels[DFM_ATSS_MAX_LEVELS]; /* 0 */
    int64_t cls_stride[DFM_ATSS_MAX_LEVELS * 4];  /* level l at [4 l, 4 l + 4): ELEMENT strides (image, channel, row, */
    int64_t reg_stride[DFM_ATSS_MAX_LEVELS * 4];  /* column) of that level's map: NCHW-contiguous, channels-last or any */
    int64_t ctr_stride[DFM_ATSS_MAX_LEVELS * 4];  /* other strided view is read in place */
    int64_t grad_cls_stride[DFM_ATSS_MAX_LEVELS * 4];   /* the same of the gradient maps (dfm_atss_loss_bwd only) */
    int64_t grad_reg_stride[DFM_ATSS_MAX_LEVELS * 4];
    int64_t grad_ctr_stride[DFM_ATSS_MAX_LEVELS * 4];
} dfm_atss_loss_desc;
/* Semantics.
 * maps: a HOST array of 3 L device pointers, maps[3 l + 0 | 1 | 2] = cls_score | bbox_pred | centerness of level l:
 *     cls_score (B, C, h, w) and centerness (B, 1, h, w) of `dtype`, bbox_pred (B, 4 or 4 C, h, w) of `reg_dtype`, each
 *     at its strides.  A bf16 map is read as the FP32 value of each element; all arithmetic is FP32.
 * One anchor per location.  Row n = y * w + x of level l of image b is row r = b * A + off_l + n of the dense targets
 * and row off_l + n of anchors -- the layout dfm_atss_target_2d writes for level-concatenated anchors, read in place:
 *     anchors (A, 4) FP32 (x1, y1, x2, y2), one set shared by the images,
 *     labels (B, A) int64, label_weights (B, A) FP32, bbox_targets (B, A, 4) FP32 (encoded deltas).       [device]
 * The levels need not cover all A rows (rows outside every level are not read); each must lie inside:
 * off_l + h_l * w_l <= A.
 * Positives: row r is positive iff 0 <= labels[r] < C.  Any other label, C included, is a row whose classes are all
 * negative.  Of a positive row with class-specific regression (reg_class_agnostic == 0) the four deltas are the
 * channels s * C + labels[r], s = 0 .. 3 (the reference's reshape(-1, 4, C) gathered at the label); with
 * reg_class_agnostic they are channels 0 .. 3.
 * delta2bbox(anchor, d) (mmdet's DeltaXYWHBBoxCoder.decode without max_shape): e_s = d_s * target_stds[s] +
 *     target_means[s]; ew = clamp(e_2, -R, R), eh = clamp(e_3, -R, R), R = |log(16 / 1000)|;
 *     px = (x1 + x2) * 0.5, pw = x2 - x1 (py, ph alike); gx = px + pw * e_0, gy = py + ph * e_1, gw = pw * exp(ew),
 *     gh = ph * exp(eh); box = (gx - gw * 0.5, gy - gh * 0.5, gx + gw * 0.5, gy + gh * 0.5).
 * Terms, each an FP32 sum per level l:
 *   S_cls[l] = sum over ALL rows of the level, sum_c label_weights[r] * focal(x_c, t_c), t_c = 1 iff labels[r] == c:
 *           the focal term of dfm_hip_anchor_loss.h, the same device function (csrc/focal_loss.h), finite for every
 *           finite logit.
 *   ct      the centerness target of a positive row: gt = delta2bbox(anchor, bbox_targets[r]); with (cx, cy) = (px, py)
 *           the anchor centre, l = cx - gt.x1, t = cy - gt.y1, r = gt.x2 - cx, b = gt.y2 - cy,
 *               q = (min(l, r) / max(l, r)) * (min(t, b) / max(t, b));  ct = sqrt(q) when q > 0, and 0 otherwise:
 *           a product that is zero, negative or NaN (an anchor centre on or outside a side of its box, a degenerate
 *           box) gives ct = 0 exactly, so the row adds nothing to S_box or T and its box gradient is 0.  (The
 *           reference asserts that no ct is NaN, which waits for the host; that assert is not made.)
 *   S_box[l] = sum_pos ct * (1 - GIoU(p, gt)), p = delta2bbox(anchor, the row's predicted deltas); GIoU is mmdet's
 *           bbox_overlaps(mode='giou', is_aligned=True, eps=1e-6):
 *               area = (x2 - x1) * (y2 - y1) of each box;
 *               overlap = max(min x2 - max x1, 0) * max(min y2 - max y1, 0);
 *               union = max(area_p + area_gt - overlap, eps);  iou = overlap / union;
 *               enclose = max(max(max x2 - min x1, 0) * max(max y2 - min y1, 0), eps);
 *               GIoU = iou - (enclose - union) / enclose.
 *   S_ctr[l] = sum_pos bce(z, ct) = max(z, 0) - z * ct + log1p(exp(-|z|)), z the row's centerness logit.
 *   T       = sum over the levels, sum_pos ct.  It depends on the targets only and has no gradient.
 * out (3 L + 1) FP32 [device], UNSCALED: out[3 l + 0 | 1 | 2] = S_cls[l] | S_box[l] | S_ctr[l], out[3 L] = T.  The
 *           average factors are the caller's: T's own clamp and its all-reduce across ranks sit between these sums and
 *           the scale of the box term.  Without a positive row in a level S_box[l] = S_ctr[l] = 0 exactly, and so are
 *           their gradients.
 * Forward: two launches -- one lane per (level, image, row), level-major, so that a wave reads contiguous runs of a
 *           channel plane (NCHW) or rows a channel count apart (channels-last); with one anchor per location the
 *           anchor-fastest and the pixel-fastest order are the same order.  The 3 L + 1 sums are formed per wave by
 *           shuffles (a wave that holds rows of two levels sums each level's lanes apart), per workgroup through LDS
 *           into one partial row of the workspace; then one workgroup adds the partial rows, one wave per column: lane
 *           t the rows t, t + 64, ... in ascending order, then a tree over the lanes.  No atomics, no memset, a fixed
 *           order of addition: the same bits run after run.  No host synchronisation.  The count depends on neither the
 *           map sizes, B, L nor the number of positives.
 * Backward (dfm_atss_loss_bwd): one launch, one lane per row, over the same inputs and grad_S (3 L) FP32 [device]
 *           in the layout of out (T has no gradient): grad_map = sum_k grad_S[3 l + k] dS_k[l] / dmap.  grad_maps: a
 *           HOST array of 3 L device pointers in the order of maps, each of its map's shape and dtype (FP32 to bf16:
 *           round to nearest even) at the strides grad_*_stride; a NULL entry skips that map.  Every element of every
 *           gradient map given is written exactly once (allocate with empty):
 *             grad cls_score   grad_S_cls * label_weights[r] * dfocal / dx_c; exactly 0 on a row with
 *                              label_weights[r] == 0;
 *             grad centerness  grad_S_ctr * (sigmoid(z) - ct) on a positive row, exactly 0 elsewhere;
 *             grad bbox_pred   on a positive row -grad_S_box * ct * dGIoU / d(the row's four deltas) in the channels of
 *                              its own class; exactly 0 in every channel of another class and on every row that is not
 *                              positive.
 *           At the kinks the rules are torch's: clamp (of a side length or of a sum at its lower bound, of e_2 / e_3 at
 *           +-R) passes the gradient where min <= x <= max and gives 0 outside, so a delta whose e_2 (e_3) lies beyond
 *           +-R gets exactly 0 in that column while the row's other columns get theirs; the min / max of a predicted
 *           and a target coordinate passes the gradient to the prediction where it is the strict min / max, half of it
 *           where the two are equal.
 * workspace: dfm_atss_loss_workspace_bytes(desc) (3 * DFM_ATSS_MAX_LEVELS + 1 floats per 256 rows), 16-byte aligned,
 *           caller-owned; the forward only.
 * B == 0 or levels without a row: DFM_OK, nothing is launched; the forward sets out to zeros (one memset on `stream`).
 * DFM_ERR_UNSUPPORTED, before any HIP call: L > DFM_ATSS_MAX_LEVELS, C < 1, a dtype other than DFM_F32 / DFM_BF16,
 * more than 2^31 - 1 rows in the batch (the workspace query returns 0 for these).  DFM_ERR_INVALID_ARG: L < 1, a
 * negative size, a level outside [0, A), a NULL pointer. */
DFM_API size_t dfm_atss_loss_workspace_bytes(const dfm_atss_loss_desc *desc);
DFM_API int dfm_atss_loss_fwd(const dfm_atss_loss_desc *desc, const void *const *maps, const float *anchors,
                              const int64_t *labels, const float *label_weights, const float *bbox_targets, float *out,
                              void *workspace, size_t workspace_bytes, void *stream);
DFM_API int dfm_atss_loss_bwd(const dfm_atss_loss_desc *desc, const void *const *maps, const float *anchors,
                              const int64_t *labels, const float *label_weights, const float *bbox_targets,
                              const float *grad_S, void *const *grad_maps, void *stream);

#endif /* DFM_HIP_ATSS_LOSS_H */
