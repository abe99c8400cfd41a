// box_membership.h -- "is this point inside this rotated 3-D box", stated once for every kernel that asks
// (imitation_loss.hip: the BEV cells inside a ground-truth box; depth_targets.hip: the box id of a depth pixel and the
// points_in_boxes_part / _all / idmap operators).
#pragma once
#include "dfm_common.h"

namespace dfm {

struct PtBox { float x, y, cz, hx, hy, hz, ca, sa; };

// mmcv 1.6 `points_in_boxes_part` (check_pt_in_box3d + lidar_to_local_coords of
// mmcv/ops/csrc/common/cuda/points_in_boxes_cuda_kernel.cuh), as the maintainers state its semantics, fp32:
//   cz = z + z_size/2; reject if |pz - cz| > z_size/2;  a = -yaw;
//   lx = dx cos(a) - dy sin(a), ly = dx sin(a) + dy cos(a);  inside iff |lx| < x_size/2 and |ly| < y_size/2, strict.
// A zero-size box contains nothing.
// flat: the box's z is taken as 0 (dfm.py:486: gt_boxes[..., 2] = 0).
// ratio, distance: the three sizes are first multiplied by ratio, then increased by distance, each one fp32 rounding
// (datasets/utils.py:423-424); 1 and 0 leave them as they are, bit for bit.
__device__ __forceinline__ PtBox pt_box(const float *b7, bool flat, float ratio = 1.0f, float distance = 0.0f)
{
    PtBox o;
    const float z = flat ? 0.0f : b7[2];
    o.x = b7[0]; o.y = b7[1];
    o.hx = (b7[3] * ratio + distance) / 2.0f;
    o.hy = (b7[4] * ratio + distance) / 2.0f;
    o.hz = (b7[5] * ratio + distance) / 2.0f;
    o.cz = z + o.hz;
    const float a = -b7[6];
    o.ca = cosf(a); o.sa = sinf(a);
    return o;
}
__device__ __forceinline__ bool pt_in_box(float px, float py, float pz, const PtBox &b)
{
    if (fabsf(pz - b.cz) > b.hz) return false;
    const float dx = px - b.x, dy = py - b.y;
    const float lx = dx * b.ca - dy * b.sa;
    const float ly = dx * b.sa + dy * b.ca;
    return (lx > -b.hx) & (lx < b.hx) & (ly > -b.hy) & (ly < b.hy);
}

}  // namespace dfm
