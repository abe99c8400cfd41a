// iou3d_geom.h -- the differentiable IoU of two rotated 3-D boxes and the IoU term of the anchor head's loss for ONE
// row, as device functions shared by every kernel that evaluates them (csrc/iou3d_loss.hip: dfm_diff_iou_rotated and
// dfm_iou3d_loss_from_deltas; csrc/anchor_loss.hip: the IoU term of dfm_anchor3d_loss_fwd / _bwd), which must give
// the same bits per row.  csrc/iou3d_loss.hip describes the method.
#pragma once
#include "rbox_geom.h"

namespace dfm {

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

// 1 - IoU3D(decode(an, pred), decode(an, tgt)) of one row, a NaN component of the decoded target replaced by the
// prediction's (iou3d_loss: target = where(isnan(target), pred, target); the gradient of a replaced component reaches
// the prediction through both arguments); with GRAD, j = d loss / d pred[0..7)
template <bool GRAD>
__device__ __forceinline__ float iou3d_loss_row(const float *__restrict__ an, const float *__restrict__ pred,
                                                const float *__restrict__ tgt, float (&j)[7])
{
    const Decoded p = decode_row(an, pred);
    Decoded t = decode_row(an, tgt);
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
    const float val = 1.0f - iou3d<GRAD>(p.box, t.box, g1, g2);
    if constexpr (GRAD) {
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
    }
    return val;
}

}  // namespace dfm
