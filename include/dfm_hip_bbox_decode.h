/* dfm_hip_bbox_decode.h -- the part of the C ABI of libdfm_hip.so that takes the 3-D anchor head's maps to NMS
 * candidates.  Included by dfm_hip.h (inside its extern "C" block, after DFM_API, the status codes, the dtypes and
 * DFM_BOX_NMS_MAX_N): include that header, not this one.  Bound by depth-from-motion_amd/_capi.py through
 * BBOX_DECODE_SIGNATURES. */
#ifndef DFM_HIP_BBOX_DECODE_H
#define DFM_HIP_BBOX_DECODE_H
#ifndef DFM_HIP_H
#error "include dfm_hip.h: it defines DFM_API and the status codes, and includes this header"
#endif

/* ---------------------------------------------------------------------- */
/* the 3-D anchor head's maps to NMS candidates, and the box decode         */
/* Anchor3DHead.get_bboxes_single up to its box3d_multiclass_nms call       */
/* (models/dense_heads/anchor3d_head.py:458-533) and                        */
/* DeltaXYZWLHRBBoxCoder.decode (core/bbox/coders/                          */
/* delta_xyzwhlr_bbox_coder.py:58-91)                                       */
/* ---------------------------------------------------------------------- */
#define DFM_ANCHOR_HEAD_MAX_BATCH 64    /* images per call */
typedef struct dfm_anchor_head_desc {
    int32_t batch;                /* B <= DFM_ANCHOR_HEAD_MAX_BATCH */
    int32_t h, w;                 /* the BEV map of this level */
    int32_t anchors_per_location; /* A = sizes x rotations */
    int32_t num_classes;          /* C (sigmoid classification: one logit per class) */
    int32_t box_code_size;        /* S, 7 .. 16; anything else: DFM_ERR_UNSUPPORTED */
    int32_t nms_pre;              /* rows kept per image; <= 0 or >= N: all N, in anchor order */
    int32_t dtype;                /* of the three maps: DFM_F32 or DFM_BF16 */
    int64_t cls_stride[4];        /* ELEMENT strides (image, channel, row, column) of each map: NCHW-contiguous, */
    int64_t reg_stride[4];        /* channels-last or any other strided view is read in place */
    int64_t dir_stride[4];
} dfm_anchor_head_desc;
/* Semantics.  N = h * w * A anchors per image; anchor n = (y * w + x) * A + a, the order of the reference's
 * permute(1, 2, 0).reshape(-1, .) of each map, so that of anchor n
 *     class logit c     is cls[b][a * C + c][y][x],        c in [0, C)
 *     delta column s    is reg[b][a * S + s][y][x],        s in [0, S)
 *     direction logit j is dir[b][a * 2 + j][y][x],        j in {0, 1}.
 * A bf16 map is read as the FP32 value of each element (exactly what map.float() gives); all arithmetic is FP32 (the
 * reference run on a bf16 map would round every intermediate to bf16 instead).
 *   key(n)   = max over c of sigmoid(class logit c), sigmoid(x) = 1 / (1 + exp(-x)); NaN if any of them is NaN.
 *   Selection, per image, when nms_pre > 0 and N > nms_pre: K = nms_pre and the rows are the K anchors with the
 *     greatest keys, in DESCENDING key order.  Equal keys go in ASCENDING anchor index, at the cut as well: of
 *     the anchors whose key equals the K-th greatest, those with the lowest indices stay (torch.topk leaves the
 *     order of equal keys undefined; this is the library's rule).  A NaN key ranks above every number, as in
 *     torch.topk; NaN keys are equal to each other.
 *     Otherwise K = N and the rows are all anchors in anchor order, as the reference does when it skips the topk.
 *   Row k of image b, from its anchor n = topk_inds[b][k]:
 *     bboxes         (B, K, S)     = DeltaXYZWLHRBBoxCoder.decode(anchors[n], deltas): with the anchor (xa, ya, za, wa,
 *                                    la, ha, ra, ...) and the deltas (xt, yt, zt, wt, lt, ht, rt, ...), in this order
 *                                    and with one rounding per operation,
 *                                      za' = za + ha / 2;  d = sqrt(la * la + wa * wa);
 *                                      x = xt * d + xa;  y = yt * d + ya;  z' = zt * ha + za';
 *                                      dy = exp(lt) * la;  dx = exp(wt) * wa;  dz = exp(ht) * ha;
 *                                      yaw = rt + ra;  z = z' - dz / 2;   row = (x, y, z, dx, dy, dz, yaw),
 *                                    then the columns beyond 7 as t + a.
 *     bboxes_for_nms (B, K, 5)     = xywhr2xyxyr of the columns (0, 1, 3, 4, 6) -- BaseInstance3DBoxes.bev, the BEV
 *                                    box of the LiDAR and depth box classes: (x - dx / 2, y - dy / 2, x + dx / 2,
 *                                    y + dy / 2, yaw).
 *     scores         (B, K, C + 1) = the C sigmoids, then 0 (the reference's dummy background column).
 *     dir_scores     (B, K) int64  = argmax of the two direction logits, 0 when they are equal (torch.max).
 *     topk_inds      (B, K) int64  = n.
 *   Every element of the five outputs is written exactly once (allocate with empty).
 * anchors   : (N, S) FP32, one set shared by every image                                         [device]
 * workspace : dfm_anchor_head_candidates_workspace_bytes(desc) (0 when nothing is cut), 16-byte aligned,
 *             caller-owned: the per-image digit histograms, the 32-bit keys, the candidate list.
 * With a cut: one memset and six launches on `stream` (keys + first histogram; two refinements of the radix select,
 * 11 + 11 + 10 bits; compaction of the keys above the K-th; one workgroup per image that adds the equal keys
 * from the lowest index up and orders the K survivors in LDS; gather + decode of the K rows).  Without: the last
 * launch alone.  The count depends on neither N nor B; integer atomics only: the same bits run after run; no
 * host synchronisation.  B == 0 or N == 0 returns DFM_OK and launches nothing.
 * DFM_ERR_UNSUPPORTED, before any HIP call: S outside 7 .. 16, B > DFM_ANCHOR_HEAD_MAX_BATCH, K > DFM_BOX_NMS_MAX_N
 * (the limit of the NMS that follows), N > 2^31 - 1, another dtype. */
DFM_API size_t dfm_anchor_head_candidates_workspace_bytes(const dfm_anchor_head_desc *desc);
DFM_API int dfm_anchor_head_candidates(const dfm_anchor_head_desc *desc, const void *cls, const void *reg,
                                       const void *dir, const float *anchors, float *bboxes, float *bboxes_for_nms,
                                       float *scores, int64_t *dir_scores, int64_t *topk_inds, void *workspace,
                                       size_t workspace_bytes, void *stream);
/* out (n, S) = DeltaXYZWLHRBBoxCoder.decode(anchors, deltas) as above, rows (n, S) FP32, S in 7 .. 16
 * (DFM_ERR_UNSUPPORTED otherwise).  One launch, one lane per row; the same device function as the candidates'
 * bboxes: the same bits.  n == 0 returns DFM_OK and launches nothing. */
DFM_API int dfm_delta_xyzwlhr_decode(const float *anchors, const float *deltas, int32_t n, int32_t box_code_size,
                                     float *out, void *stream);

#endif /* DFM_HIP_BBOX_DECODE_H */
