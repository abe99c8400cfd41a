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
#include "rbox_geom.h"

using namespace dfm;

namespace {

struct Box3 { float x, y, z, dx, dy, dz, r; };

// t0 <= t <= t1 of the segment whose constraint value runs from q (t = 0) with slope p must keep q + t p >= 0
__device__ __forceinline__ void lb_bound(float p, float q, float &t0, float &t1)
{
    const float r = -q / p;                                   // p == 0: not used
    t0 = p > 0.0f ? fmaxf(t0, r) : t0;
    t1 = p < 0.0f ? fminf(t1, r) : t1;
    t1 = (p == 0.0f && q < 0.0f) ? -1.0f : t1;                // parallel and outside: empty
}

// d I / d (x, y, w, h, angle) of rectangle O from its four edges clipped to rectangle X; (ox, oy), (xx, xy): the
// centres relative to the midpoint
__device__ __forceinline__ void edge_gradient(const RBox &O, float ox, float oy, const RBox &X, float xx, float xy,
                                              float (&g)[5])
{
    const float hw = O.w * 0.5f, hh = O.h * 0.5f, hwx = X.w * 0.5f, hhx = X.h * 0.5f;
    float px[4], py[4];                                       // O's corners in X's axes, counter-clockwise
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float lx = (k < 2) ? hw : -hw;
        const float ly = (k == 1 || k == 2) ? hh : -hh;
        const float wx = ox + (lx * O.c - ly * O.s);
        const float wy = oy + (lx * O.s + ly * O.c);
        const float ux = wx - xx, uy = wy - xy;
        px[k] = ux * X.c + uy * X.s;
        py[k] = uy * X.c - ux * X.s;
    }
    float len[4], mom = 0.0f;                                 // edge k: corner k -> k + 1, normals +u, +v, -u, -v
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int k1 = (k + 1) & 3;
        const float ex = px[k1] - px[k], ey = py[k1] - py[k];
        float t0 = 0.0f, t1 = 1.0f;
        lb_bound(ex, px[k] + hwx, t0, t1);
        lb_bound(-ex, hwx - px[k], t0, t1);
        lb_bound(ey, py[k] + hhx, t0, t1);
        lb_bound(-ey, hhx - py[k], t0, t1);
        const float L = (k & 1) ? O.w : O.h;
        len[k] = fmaxf(t1 - t0, 0.0f) * L;
        mom += 0.5f * len[k] * L * (t0 + t1 - 1.0f);
    }
    const float gu = len[0] - len[2], gv = len[1] - len[3];
    g[0] = gu * O.c - gv * O.s;
    g[1] = gu * O.s + gv * O.c;
    g[2] = 0.5f * (len[0] + len[2]);
    g[3] = 0.5f * (len[1] + len[3]);
    g[4] = -mom;
}

// IoU3D of a and b; with GRAD its gradient rows g1 = d IoU / d a, g2 = d IoU / d b (x, y, z, dx, dy, dz, yaw)
template <bool GRAD>
__device__ __forceinline__ float iou3d(const Box3 &a, const Box3 &b, float (&g1)[7], float (&g2)[7])
{
#pragma unroll
    for (int c = 0; c < 7; ++c) g1[c] = g2[c] = 0.0f;
    const float area1 = a.dx * a.dy, area2 = b.dx * b.dy;
    const float v1 = area1 * a.dz, v2 = area2 * b.dz;
    if (area1 < AREA_EPS || area2 < AREA_EPS || v1 < AREA_EPS || v2 < AREA_EPS) return 0.0f;
    RBox A{a.x, a.y, a.dx, a.dy, 1.0f, 0.0f}, B{b.x, b.y, b.dx, b.dy, 1.0f, 0.0f};
    sincosf(a.r, &A.s, &A.c);
    sincosf(b.r, &B.s, &B.c);
    const float top1 = a.z + a.dz * 0.5f, top2 = b.z + b.dz * 0.5f;
    const float bot1 = a.z - a.dz * 0.5f, bot2 = b.z - b.dz * 0.5f;
    const float Z = fminf(top1, top2) - fmaxf(bot1, bot2);
    const float I = rbox_intersection(A, B);
    if (!(I > 0.0f) || !(Z > 0.0f)) return 0.0f;
    const float W = I * Z, U = v1 + v2 - W;
    if constexpr (GRAD) {
        const float mx = (A.x + B.x) * 0.5f, my = (A.y + B.y) * 0.5f;
        const float ax = A.x - mx, ay = A.y - my, bx = B.x - mx, by = B.y - my;
        float d1[5], d2[5];
        edge_gradient(A, ax, ay, B, bx, by, d1);
        edge_gradient(B, bx, by, A, ax, ay, d2);
        const float gW = (v1 + v2) / (U * U), gV = -W / (U * U);     // d IoU / d W, d IoU / d V
        const float gI = gW * Z, gZ = gW * I;
        const float t1 = top1 <= top2 ? 1.0f : 0.0f, b1 = bot1 >= bot2 ? 1.0f : 0.0f;   // whose faces bound Z
        g1[0] = gI * d1[0];
        g1[1] = gI * d1[1];
        g1[2] = gZ * (t1 - b1);
        g1[3] = gI * d1[2] + gV * (a.dy * a.dz);
        g1[4] = gI * d1[3] + gV * (a.dx * a.dz);
        g1[5] = gZ * (0.5f * (t1 + b1)) + gV * area1;
        g1[6] = gI * d1[4];
        g2[0] = gI * d2[0];
        g2[1] = gI * d2[1];
        g2[2] = gZ * (b1 - t1);
        g2[3] = gI * d2[2] + gV * (b.dy * b.dz);
        g2[4] = gI * d2[3] + gV * (b.dx * b.dz);
        g2[5] = gZ * (0.5f * ((1.0f - t1) + (1.0f - b1))) + gV * area2;
        g2[6] = gI * d2[4];
    }
    return W / U;
}

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

struct Decoded {
    Box3 box;
    float diag, ha;   // what the chain rule needs besides the box: d x / d xt = diag, d z / d zt = ha
};

// DeltaXYZWLHRBBoxCoder.decode (core/bbox/coders/delta_xyzwhlr_bbox_coder.py:58-91), the same fp32 operations
__device__ __forceinline__ Decoded decode_row(const float *__restrict__ an, const float *__restrict__ de)
{
    const float xa = an[0], ya = an[1], wa = an[3], la = an[4], ha = an[5], ra = an[6];
    const float za = an[2] + ha / 2.0f;
    const float diag = sqrtf(la * la + wa * wa);
    Decoded o;
    o.box.x = de[0] * diag + xa;
    o.box.y = de[1] * diag + ya;
    const float zg = de[2] * ha + za;
    o.box.dy = expf(de[4]) * la;
    o.box.dx = expf(de[3]) * wa;
    o.box.dz = expf(de[5]) * ha;
    o.box.r = de[6] + ra;
    o.box.z = zg - o.box.dz / 2.0f;
    o.diag = diag;
    o.ha = ha;
    return o;
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
        const Decoded p = decode_row(anchors + off, bbox_pred + off);
        Decoded t = decode_row(anchors + off, bbox_targets + off);
        // iou3d_loss: target = where(isnan(target), pred, target); the gradient of a replaced component reaches
        // the prediction through both arguments
        const bool n0 = isnan(t.box.x), n1 = isnan(t.box.y), n2 = isnan(t.box.z), n3 = isnan(t.box.dx),
                   n4 = isnan(t.box.dy), n5 = isnan(t.box.dz), n6 = isnan(t.box.r);
        t.box.x = n0 ? p.box.x : t.box.x;
        t.box.y = n1 ? p.box.y : t.box.y;
        t.box.z = n2 ? p.box.z : t.box.z;
        t.box.dx = n3 ? p.box.dx : t.box.dx;
        t.box.dy = n4 ? p.box.dy : t.box.dy;
        t.box.dz = n5 ? p.box.dz : t.box.dz;
        t.box.r = n6 ? p.box.r : t.box.r;
        float g1[7], g2[7];
        if (jac != nullptr) {                                 // (uniform)
            val = 1.0f - iou3d<true>(p.box, t.box, g1, g2);
            g1[0] += n0 ? g2[0] : 0.0f;
            g1[1] += n1 ? g2[1] : 0.0f;
            g1[2] += n2 ? g2[2] : 0.0f;
            g1[3] += n3 ? g2[3] : 0.0f;
            g1[4] += n4 ? g2[4] : 0.0f;
            g1[5] += n5 ? g2[5] : 0.0f;
            g1[6] += n6 ? g2[6] : 0.0f;
            // through the decode: x = xt diag + xa, z = zt ha + za - dz / 2, size = exp(delta) anchor size
            j[0] = -(g1[0] * p.diag);
            j[1] = -(g1[1] * p.diag);
            j[2] = -(g1[2] * p.ha);
            j[3] = -(g1[3] * p.box.dx);
            j[4] = -(g1[4] * p.box.dy);
            j[5] = -((g1[5] - 0.5f * g1[2]) * p.box.dz);
            j[6] = -g1[6];
        } else {
            val = 1.0f - iou3d<false>(p.box, t.box, g1, g2);
        }
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
