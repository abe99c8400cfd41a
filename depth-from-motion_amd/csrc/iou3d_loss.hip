// iou3d_loss.hip -- differentiable IoU of rotated 3-D (and 2-D) boxes and the IoU term of the anchor head's loss
// (reference: models/losses/iou3d_loss.py, whose diff_iou_rotated_3d is a CUDA op of mmcv, called from
// LIGAAnchor3DHead.loss_single, dense_heads/liga_anchor3d_head.py:210-224).
//
// Semantics (include/dfm_hip.h states them in full): box (x, y, z, dx, dy, dz, yaw); IoU3D = I Z / (V1 + V2 - I Z)
// with I the exact area of the BEV rectangles' intersection, Z the overlap of the z intervals, V = dx dy dz; value
// and gradient 0 when a BEV area or a volume is below 1e-14 or I or Z is 0.
//
// One lane per box pair, one wave per workgroup, everything in registers:
//   value    : I from rbox_geom.h's polygon clip, the function the NMS kernels use.  A sequential clip returns a
//              closed polygon whatever the rounding does, so identical boxes, shared edges and touching boxes
//              (pred == target after the NaN-target rule) give sane areas.
//   gradient : from the eight edge segments -- the four edges of each box clipped to the other box by
//              Liang-Barsky, in the other box's axes, both boxes relative to the midpoint of their centres.  The
//              boundary of the intersection is exactly those clipped pieces; moving a box moves its own pieces, and
//              dI = sum over them of (velocity . outward normal) ds.  With l_k the clipped length of edge k and
//              M_k its first moment along the edge (counter-clockwise) about the foot of the centre:
//                  dI/dcentre = sum l_k n_k,  dI/dw = (l_{+u} + l_{-u}) / 2,  dI/dh = (l_{+v} + l_{-v}) / 2,
//                  dI/dangle  = - sum M_k                       (u, v: the box's own axes)
//              No vertex list, no sort; on the measure-zero set where the gradient is undefined (coincident
//              edges) the result is finite.
//   memory   : box rows (7 or 5 floats) and gradient rows move through a 64-row LDS tile, so the global loads and
//              stores of a wave are contiguous runs; a row stride of 7 or 5 words is odd: no bank conflict.
// No scratch, no runtime-indexed local array, no atomics: the same bits run after run.
#include "iou3d_geom.h"

using namespace dfm;

namespace {

// rows [row0, row0 + 64) of src (n, W): v = this lane's row, through the tile (contiguous global loads)
template <int W>
__device__ __forceinline__ void load_rows(const float *__restrict__ src, long long row0, int cnt, float *tile,
                                          float (&v)[W])
{
    const int lane = threadIdx.x;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < W; ++j) {
        const int e = lane + 64 * j;
        if (e < cnt * W) tile[e] = src[row0 * W + e];
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < W; ++c) v[c] = lane < cnt ? tile[lane * W + c] : 0.0f;
}

template <int W>
__device__ __forceinline__ void store_rows(float *__restrict__ dst, long long row0, int cnt, float *tile,
                                           const float (&v)[W])
{
    const int lane = threadIdx.x;
    __syncthreads();
#pragma unroll
    for (int c = 0; c < W; ++c) tile[lane * W + c] = v[c];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < W; ++j) {
        const int e = lane + 64 * j;
        if (e < cnt * W) dst[row0 * W + e] = tile[e];
    }
}

// a 5-wide row (x, y, w, h, angle) is the box with z = 0, dz = 1: Z = 1 and V = w h exactly
template <int W>
__device__ __forceinline__ Box3 as_box(const float (&v)[W])
{
    if constexpr (W == 7) return Box3{v[0], v[1], v[2], v[3], v[4], v[5], v[6]};
    else return Box3{v[0], v[1], 0.0f, v[2], v[3], 1.0f, v[4]};
}

template <int W>
__device__ __forceinline__ void as_row(const float (&g)[7], float (&v)[W])
{
    if constexpr (W == 7) {
#pragma unroll
        for (int c = 0; c < 7; ++c) v[c] = g[c];
    } else {
        v[0] = g[0]; v[1] = g[1]; v[2] = g[3]; v[3] = g[4]; v[4] = g[6];
    }
}

// iou[p] = IoU(boxes1[p], boxes2[p]); grad1 / grad2 (n, W) = its gradient rows (both NULL: values only)
template <int W>
__global__ __launch_bounds__(64) void diff_iou_rotated_kernel(const float *__restrict__ boxes1,
                                                              const float *__restrict__ boxes2, int n,
                                                              float *__restrict__ iou, float *__restrict__ grad1,
                                                              float *__restrict__ grad2)
{
    __shared__ float tile[64 * W];
    const long long row0 = (long long)blockIdx.x * 64;
    const int cnt = (int)min(64ll, (long long)n - row0);
    const int lane = threadIdx.x;
    float v1[W], v2[W], g1[7], g2[7];
    load_rows<W>(boxes1, row0, cnt, tile, v1);
    load_rows<W>(boxes2, row0, cnt, tile, v2);
    const Box3 a = as_box<W>(v1), b = as_box<W>(v2);
    float val;
    if (grad1 != nullptr) {                                   // (uniform)
        val = iou3d<true>(a, b, g1, g2);
        as_row<W>(g1, v1);
        as_row<W>(g2, v2);
        store_rows<W>(grad1, row0, cnt, tile, v1);
        store_rows<W>(grad2, row0, cnt, tile, v2);
    } else {
        val = iou3d<false>(a, b, g1, g2);
    }
    if (lane < cnt) iou[row0 + lane] = val;
}

// loss[p] = 1 - IoU3D(decode(anchors[i], bbox_pred[i]), decode(anchors[i], bbox_targets[i])), i = pos_inds[p], a NaN
// component of the decoded target replaced by the prediction's; jac (num_pos, 7) = d loss[p] / d bbox_pred[i][0..7)
__global__ __launch_bounds__(64) void iou3d_loss_from_deltas_kernel(const float *__restrict__ anchors,
                                                                    const float *__restrict__ bbox_pred,
                                                                    const float *__restrict__ bbox_targets,
                                                                    const long long *__restrict__ pos_inds,
                                                                    int num_rows, int code_size, int num_pos,
                                                                    float *__restrict__ loss, float *__restrict__ jac)
{
    __shared__ float tile[64 * 7];
    const long long row0 = (long long)blockIdx.x * 64;
    const int cnt = (int)min(64ll, (long long)num_pos - row0);
    const int lane = threadIdx.x;
    float j[7];
#pragma unroll
    for (int c = 0; c < 7; ++c) j[c] = 0.0f;
    float val = 1.0f;                                         // an index outside [0, num_rows): no box, IoU 0
    const long long idx = lane < cnt ? pos_inds[row0 + lane] : -1;
    if (idx >= 0 && idx < num_rows) {
        const size_t off = (size_t)idx * code_size;
        if (jac != nullptr)                                   // (uniform)
            val = iou3d_loss_row<true>(anchors + off, bbox_pred + off, bbox_targets + off, j);
        else
            val = iou3d_loss_row<false>(anchors + off, bbox_pred + off, bbox_targets + off, j);
    }
    if (jac != nullptr) store_rows<7>(jac, row0, cnt, tile, j);
    if (lane < cnt) loss[row0 + lane] = val;
}

}  // namespace

extern "C" DFM_API int dfm_diff_iou_rotated(const float *boxes1, const float *boxes2, int32_t n, int32_t width,
                                            float *iou, float *grad1, float *grad2, void *stream)
{
    if (n < 0) return set_error(DFM_ERR_INVALID_ARG, "negative pair count");
    if (width != 5 && width != 7)
        return set_errorf(DFM_ERR_INVALID_ARG, "box width %d: 7 (x, y, z, dx, dy, dz, yaw) or 5 (x, y, w, h, angle)", width);
    if ((grad1 == nullptr) != (grad2 == nullptr))
        return set_error(DFM_ERR_INVALID_ARG, "grad1 and grad2 are given together or both NULL");
    if (n == 0) return DFM_OK;
    if (!boxes1 || !boxes2 || !iou) return set_error(DFM_ERR_INVALID_ARG, "NULL device pointer");
    const dim3 grid((unsigned)(((long long)n + 63) / 64)), block(64);
    if (width == 7)
        hipLaunchKernelGGL(diff_iou_rotated_kernel<7>, grid, block, 0, (hipStream_t)stream, boxes1, boxes2, n, iou,
                           grad1, grad2);
    else
        hipLaunchKernelGGL(diff_iou_rotated_kernel<5>, grid, block, 0, (hipStream_t)stream, boxes1, boxes2, n, iou,
                           grad1, grad2);
    HIP_TRY(hipGetLastError());
    return DFM_OK;
}

extern "C" DFM_API int dfm_iou3d_loss_from_deltas(const float *anchors, const float *bbox_pred,
                                                  const float *bbox_targets, const int64_t *pos_inds,
                                                  int32_t num_rows, int32_t code_size, int32_t num_pos, float *loss,
                                                  float *jac, void *stream)
{
    if (num_rows < 0 || num_pos < 0) return set_error(DFM_ERR_INVALID_ARG, "negative row count");
    if (code_size < 7) return set_errorf(DFM_ERR_INVALID_ARG, "code_size %d: a box code has at least 7 columns", code_size);
    if (num_pos == 0) return DFM_OK;
    if (!anchors || !bbox_pred || !bbox_targets || !pos_inds || !loss)
        return set_error(DFM_ERR_INVALID_ARG, "NULL device pointer");
    hipLaunchKernelGGL(iou3d_loss_from_deltas_kernel, dim3((unsigned)(((long long)num_pos + 63) / 64)), dim3(64), 0,
                       (hipStream_t)stream, anchors, bbox_pred, bbox_targets, (const long long *)pos_inds, num_rows,
                       code_size, num_pos, loss, jac);
    HIP_TRY(hipGetLastError());
    return DFM_OK;
}
