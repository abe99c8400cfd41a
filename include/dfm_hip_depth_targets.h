/* dfm_hip_depth_targets.h -- the part of the C ABI of libdfm_hip.so that makes the depth loss's targets (the LiDAR
 * depth map and the box-id mask of GenerateDepthMap) and answers box membership (points_in_boxes_part / _all / idmap).
 * Included by dfm_hip.h (inside its extern "C" block, after DFM_API and the status codes): include that header, not
 * this one.  Bound by depth-from-motion_amd/_capi.py under this header's name. */
#ifndef DFM_HIP_DEPTH_TARGETS_H
#define DFM_HIP_DEPTH_TARGETS_H
#ifndef DFM_HIP_H
#error "include dfm_hip.h: it defines DFM_API and the status codes, and includes this header"
#endif

/* ---------------------------------------------------------------------- */
/* Depth targets (datasets/pipelines/transforms_3d.py:55-118 GenerateDepthMap, */
/* core/camera/calibration.py:230-240 rect_to_img, datasets/utils.py:403-455   */
/* depth_map_in_boxes_cpu, core/bbox/structures/utils.py:217-248 points_img2cam) */
/* ---------------------------------------------------------------------- */
#define DFM_DEPTH_MAX_BATCH 64   /* samples of one call */
#define DFM_DEPTH_CAM_DOUBLES 28 /* per sample: the 3x4 projection P (12, row-major), then the inverse of cam2img padded
                                    to 4x4 (16, row-major), taken in FP64 on the host */
#define DFM_PIB_PART 0           /* the lowest index of a box that holds the point, else -1 */
#define DFM_PIB_ALL 1            /* (B, N, M) int32 of 0 / 1 */
#define DFM_PIB_IDMAP 2          /* the highest index of a box that holds the point, else -1 */

/* All samples of a batch in one launch.  The points of the samples are concatenated, (total, point_stride) FP32 with
 * x, y, z first; sample b owns rows [point_off[b], point_off[b + 1]).  The boxes likewise, (total, 7) FP32 = x, y, z
 * (bottom centre), x_size, y_size, z_size, yaw; sample b owns [box_off[b], box_off[b + 1]).  The tables travel BY
 * VALUE in this struct and are checked on the host in every entry point (start at 0, non-decreasing, a sample's
 * points fit the key's 32-bit index word, img_shape fits pad_shape), so no loop bound is ever read from device memory;
 * THE CALLER guarantees that the arrays hold point_off[batch] and box_off[batch] rows.
 * The maps have pad_shape (pad_h, pad_w); a point is kept only inside img_shape (img_h[b], img_w[b]). */
typedef struct dfm_depth_targets_desc {
    int32_t batch, pad_h, pad_w, point_stride;
    int32_t img_h[DFM_DEPTH_MAX_BATCH];
    int32_t img_w[DFM_DEPTH_MAX_BATCH];
    int64_t point_off[DFM_DEPTH_MAX_BATCH + 1];
    int64_t box_off[DFM_DEPTH_MAX_BATCH + 1];
} dfm_depth_targets_desc;

/* bytes of the (batch, pad_h, pad_w) uint64 key map; 0 for a descriptor the entry points refuse */
DFM_API size_t dfm_depth_targets_workspace_bytes(const dfm_depth_targets_desc *desc);

/* Scatter: ONE LANE PER POINT.  The key map is zeroed here (one memset), then one launch, none when there is no point.
 *   (x, y, z) FP32 widened to FP64;  rectified X = -y, Y = -z, Z = x (the products with the reference's 0 / +-1 matrix
 *   written out, so a non-finite coordinate spoils what it spoils there);  h = P (X, Y, Z, 1), each row
 *   ((X P0 + Y P1) + Z P2) + P3;  u = h0 / Z, v = h1 / Z (the divisor is the rectified Z, not h2);
 *   depth = h2 - P[2][3];  ix = rint(u), iy = rint(v), half to even.
 *   Kept iff u and v are finite and 0 <= iy < img_h and 0 <= ix < img_w; there is no test on the sign of depth.
 *   A kept point i (its index within its sample) does a 64-bit integer atomicMax of
 *   ((i + 1) << 32) | bits(float(depth)) on keys[b][iy][ix]: the highest point index wins, as the reference's
 *   depth_img[iy, ix] = depths[mask] lets it, and the result does not depend on the order of arrival.
 * cam: (batch, DFM_DEPTH_CAM_DOUBLES) FP64 on the device; keys: 8-byte aligned, keys_bytes >=
 * dfm_depth_targets_workspace_bytes.  DFM_ERR_INVALID_ARG: a descriptor that fails the checks above, NULL cam, NULL
 * points with points to read; DFM_ERR_UNSUPPORTED: more than 2^32 - 2 points or 2^31 - 2 boxes in a sample, a map of
 * more than 2^31 - 1 pixels; DFM_ERR_WORKSPACE: a NULL or short key map. */
DFM_API int dfm_depth_scatter(const dfm_depth_targets_desc *desc, const float *points, const double *cam, void *keys,
                              size_t keys_bytes, void *stream);

/* Resolve: ONE LANE PER PIXEL, one launch, every element of each requested output written exactly once.
 *   depth = the float in the key's low word, 0 where the key is 0 (keys given), or depth_in (batch, pad_h, pad_w)
 *   FP32; exactly one of the two is not NULL.  depth_out (batch, pad_h, pad_w) FP32 receives it (NULL: not wanted).
 *   fgmask (batch, pad_h, pad_w) int32 (NULL: not wanted): where depth > 0 (a NaN and a negative depth get 0),
 *   (ix d, iy d, d, 1) is multiplied in FP64 by the inverse of cam2img, each row ((a I0 + b I1) + c I2) + I3, mapped
 *   to pseudo-LiDAR (c_z, -c_x, -c_y), rounded to FP32 and tested against the sample's boxes in FP32 with the rule of
 *   csrc/box_membership.h (cz = z + dz/2; |pz - cz| > dz/2 rejects; rotation by -yaw; strict inequalities; a zero-size
 *   box holds nothing), the three sizes first multiplied by expand_ratio, then increased by expand_distance, in FP32.
 *   The value is 1 + the highest index of a box that holds the pixel's point, 0 if none; a sample without boxes gets
 *   zeros.  The boxes are staged in LDS, 256 at a time. */
DFM_API int dfm_depth_resolve(const dfm_depth_targets_desc *desc, const void *keys, const float *depth_in,
                              const double *cam, const float *boxes, float expand_ratio, float expand_distance,
                              float *depth_out, int32_t *fgmask, void *stream);

/* Membership: points (batch, num_points, 3) FP32 against boxes (batch, num_boxes, 7) FP32, ONE LANE PER POINT, one
 * launch; the rule of csrc/box_membership.h (mmcv's points_in_boxes_part).  out is int32: (batch, num_points) for
 * DFM_PIB_PART and DFM_PIB_IDMAP, (batch, num_points, num_boxes) for DFM_PIB_ALL; every element is written exactly
 * once.  An empty batch, no points, or DFM_PIB_ALL without boxes return DFM_OK and launch nothing; no boxes otherwise
 * writes -1.  DFM_ERR_UNSUPPORTED: batch > 65535, num_boxes > 2^31 - 2. */
DFM_API int dfm_points_in_boxes(int32_t mode, int32_t batch, int64_t num_points, int32_t num_boxes, const float *points,
                                const float *boxes, int32_t *out, void *stream);

#endif /* DFM_HIP_DEPTH_TARGETS_H */
