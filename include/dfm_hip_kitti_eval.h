/* dfm_hip_kitti_eval.h -- the part of the C ABI of libdfm_hip.so that evaluates KITTI detections: the overlaps of every
 * same-frame detection x ground-truth pair and the greedy matching behind the AP / AOS curves.  Included by dfm_hip.h
 * (inside its extern "C" block, after DFM_API and the status codes): include that header, not this one.  Bound by
 * depth-from-motion_amd/_capi.py through KITTI_EVAL_SIGNATURES. */
#ifndef DFM_HIP_KITTI_EVAL_H
#define DFM_HIP_KITTI_EVAL_H
#ifndef DFM_HIP_H
#error "include dfm_hip.h: it defines DFM_API and the status codes, and includes this header"
#endif

/* ---------------------------------------------------------------------- */
/* KITTI evaluation (core/evaluation/kitti_utils/eval.py and rotate_iou.py: */
/* image_box_overlap, rotate_iou_gpu_eval, d3_box_overlap_kernel,           */
/* compute_statistics_jit, fused_compute_statistics)                        */
/* ---------------------------------------------------------------------- */
/* Common layout.  The boxes of all F frames arrive concatenated, detections and ground truths apart, every array FP64
 * and contiguous on the device:  bbox (N, 4) = x1, y1, x2, y2;  location (N, 3);  dimensions (N, 3);  rotation_y (N);
 * alpha (N);  score (N, detections only).  Offset tables are int64 (F + 1) on the device: frame f owns rows
 * [off[f], off[f + 1]).  dt_off, gt_off and dc_off (DontCare boxes) index the three box sets; pair_off[f] =
 * sum over f' < f of n_dt(f') * n_gt(f') indexes the overlaps, whose per-frame block is row-major (n_dt, n_gt) --
 * eval.py's overlaps[i].  Cross-frame pairs do not exist.
 * Every loop bound of every kernel is read from these tables.  They cannot be checked here without a copy: THE CALLER
 * VALIDATES THEM ON THE HOST before any launch (off[0] == 0, non-decreasing, off[F] == the array length,
 * pair_off consistent with dt_off and gt_off); depth-from-motion_amd/kitti_eval.py raises ValueError on a bad table. */

#define DFM_KITTI_METRIC_BBOX 0
#define DFM_KITTI_METRIC_BEV 1
#define DFM_KITTI_METRIC_3D 2
#define DFM_KITTI_SAMPLE_POINTS 41 /* N_SAMPLE_PTS: recall sample points = thresholds per combination at the most */
#define DFM_KITTI_LDS_DETS 128     /* detections per frame up to which the assigned masks live in LDS */
#define DFM_KITTI_MATCH_MAX_GRID 16384

/* One launch for every same-frame pair and every requested metric, ONE LANE PER PAIR; the launch count does not depend
 * on F.  out_bbox / out_bev / out_3d: (total_pairs) FP64 each, NULL = metric not requested (at least one is not NULL).
 * Every element of a requested output is written exactly once.  Rows are the detections ("boxes" of the reference's
 * functions), columns the ground truths ("query_boxes").
 *
 *  bbox  image_box_overlap in FP64, the same operations in the same order, no +1:
 *          iw = min(b.x2, q.x2) - max(b.x1, q.x1);  ih likewise;  0 unless iw > 0 and ih > 0 (strict);
 *          criterion -1: ua = area(b) + area(q) - iw * ih;  0: ua = area(b);  1: ua = area(q);  other: ua = 1;
 *          overlap = iw * ih / ua.
 *  bev   boxes (location x, location z, dimensions[0], dimensions[2], rotation_y) ROUNDED TO FP32 as the reference
 *        does; the TRUE intersection area of the two rotated rectangles (csrc/rbox_geom.h: clipping in registers,
 *        FP32); with area = w * h in FP32 and rbox1 = the ground truth, rbox2 = the detection (the argument order of
 *        rotate_iou_kernel_eval):  criterion -1: inter / (area1 + area2 - inter);  0: inter / area1;  1: inter / area2;
 *        other: inter.  The FP32 result is widened to FP64.
 *        The reference's angle is clockwise, rbox_geom.h's counter-clockwise: each box is loaded with its angle
 *        negated (cos a, -sin a).  Negating nothing would be a reflection of the plane, which leaves every area
 *        unchanged, only if the centres were mirrored too; they are not, so the sign matters.
 *  3d    rinc = the FP32 BEV intersection area (criterion "other").  If rinc > 0:
 *          iw = min(y1, y2) - max(y1 - h1, y2 - h2) in FP64, y = location[1], h = dimensions[1];
 *          iw > 0:  inc = iw * rinc;  volumes d0 * d1 * d2 in FP64;  criterion -1: ua = v_dt + v_gt - inc;
 *                   0: ua = v_dt;  1: ua = v_gt;  other: ua = inc;  overlap = inc / ua ROUNDED TO FP32, then widened
 *                   (the reference stores it in the FP32 array rinc);
 *          otherwise 0.
 *
 * COINCIDENT BOXES.  The reference's intersection (corner-in-box tests plus edge crossings, sorted by angle) is
 * undecided for coincident or edge-sharing boxes: one box against itself gives IoU 1/3 with its arithmetic in FP32
 * and 0 in FP64.  This kernel returns the true overlap, which is 1 for that case.
 *
 * frames == 0 or total_pairs == 0 returns DFM_OK and launches nothing.  DFM_ERR_INVALID_ARG: a negative count, a NULL
 * table or input a requested metric reads, no output at all. */
DFM_API int dfm_kitti_overlaps(int64_t frames, int64_t total_pairs, int32_t criterion, const double *dt_bbox,
                               const double *dt_location, const double *dt_dimensions, const double *dt_rotation_y,
                               const int64_t *dt_off, const double *gt_bbox, const double *gt_location,
                               const double *gt_dimensions, const double *gt_rotation_y, const int64_t *gt_off,
                               const int64_t *pair_off, double *out_bbox, double *out_bev, double *out_3d,
                               void *stream);

/* compute_statistics_jit for every (class, difficulty, min-overlap, frame, threshold) of ONE metric.
 * A combination is (class m, difficulty l, min-overlap k), index (m * L + l) * K + k; there are C * L * K of them.
 * ONE WAVE PER (combination, frame), work items taken grid-stride by at most DFM_KITTI_MATCH_MAX_GRID waves.
 *   second_pass == 0: lane 0 runs the threshold-free first pass (compute_fp = False, thresh = 0) and writes the scores
 *     of the matched detections of the frame, in ground-truth order, to tp_scores (C*L*K, total_gt) at the frame's
 *     ground-truth rows; the rows it does not use are set to NaN.  Nothing else is written.
 *   second_pass != 0: lane t < num_thresholds[combination] (<= DFM_KITTI_SAMPLE_POINTS) runs the second pass
 *     (compute_fp = True) with thresh = thresholds[combination][t].  counts (C*L*K, 41, 3) int64 = tp, fp, fn summed
 *     over the frames with integer atomics (zeroed here first).  With compute_aos, every lane writes the similarity of
 *     its frame to the workspace and a second launch adds the frames of one (combination, t) in a fixed order:
 *     similarity (C*L*K, 41) FP64, 0 beyond num_thresholds.  No floating atomics: two evaluations of the same input
 *     give the same bits.
 * Reproduced exactly: the greedy order (ground truths ascending, detections ascending), the strict comparisons,
 * NO_DETECTION = -10000000, the three elif arms including assigned_ignored_det, ignored_threshold = score < thresh,
 * the false-positive count after the matching, the DontCare pass for metric 0 only
 * (image_box_overlap(dt, dc, criterion 0) > min_overlap in FP64, computed on the fly), the AOS term
 * (1 + cos(alpha_gt - alpha_dt)) / 2 in FP64.  A frame whose tp = fp = 0 contributes similarity -1 in the reference,
 * which fused_compute_statistics then skips; its sum of terms is empty, so it contributes 0 here.
 * Scores, thresholds and alphas stay FP64.
 *
 * ignored_gt (C*L, total_gt), ignored_det (C*L, total_dt): int8 in {-1, 0, 1}, clean_data's flags of (class,
 * difficulty) on the concatenated arrays.  min_overlap (C, K) FP64: the metric's column of min_overlaps.
 * The assigned flags of a lane are a bit mask of its own: in LDS when the frame has at most DFM_KITTI_LDS_DETS
 * detections, in the workspace otherwise.  max_dt is the largest detection count of one frame (the caller reads it
 * from dt_off): it sizes the workspace, there is no cap on it and nothing is truncated; a frame with more detections
 * than max_dt is skipped whole rather than let it write past its slot.
 * workspace: dfm_kitti_eval_workspace_bytes(frames, C * L * K, max_dt, second_pass && compute_aos), 16-byte aligned.
 * Launches: first pass 1; second pass 1 memset + 1 launch, + 1 launch with compute_aos.  None depends on F, nothing is
 * copied to the host, no host synchronisation.
 * frames == 0 or C * L * K == 0 returns DFM_OK after zeroing counts / similarity (second pass) and launches nothing.
 * DFM_ERR_INVALID_ARG: a metric outside 0..2, negative sizes, a NULL pointer the pass reads or writes;
 * DFM_ERR_WORKSPACE: a NULL or short workspace. */
DFM_API size_t dfm_kitti_eval_workspace_bytes(int64_t frames, int32_t combinations, int64_t max_dt,
                                              int32_t similarity);
DFM_API int dfm_kitti_match(int32_t metric, int32_t second_pass, int32_t compute_aos, int64_t frames,
                            int32_t num_classes, int32_t num_difficulties, int32_t num_min_overlaps,
                            const double *overlaps, const int64_t *pair_off, const int64_t *gt_off,
                            const int64_t *dt_off, const int64_t *dc_off, const double *dt_bbox,
                            const double *dt_alpha, const double *dt_score, const double *gt_alpha,
                            const double *dc_bbox, const int8_t *ignored_gt, const int8_t *ignored_det,
                            int64_t total_gt, int64_t total_dt, const double *min_overlap, const double *thresholds,
                            const int32_t *num_thresholds, double *tp_scores, int64_t *counts, double *similarity,
                            int64_t max_dt, void *workspace, size_t workspace_bytes, void *stream);

#endif /* DFM_HIP_KITTI_EVAL_H */
