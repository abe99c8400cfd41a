// rbox_geom.h -- exact fp32 intersection of two rotated rectangles, entirely in registers.  Shared by
// box_nms.hip (IoU of the suppression mask and of box_iou_rotated) and iou3d_loss.hip (the value of the
// differentiable IoU): one definition, the same bits in both.
//
// The clip: rectangle B's corners are brought into rectangle A's own axes, where A's four half-planes are
// |x| <= w/2, |y| <= h/2, and clipped against them in turn (Sutherland-Hodgman); the shoelace formula gives the
// area.  The vertex list is eight named slots filled as a shift register -- append = move every slot up by one
// under the emit flag -- so every index is a compile-time constant and the list stays in VGPRs (a runtime-
// indexed local array would go to scratch).  Appending at the front reverses the polygon's orientation at
// every clip; the area is taken by absolute value.
#pragma once
#include "dfm_common.h"

namespace dfm {

constexpr float AREA_EPS = 1e-14f;

struct RBox { float x, y, w, h, c, s; };  // centre, size, cos / sin of the angle

struct Poly {
    float x[8], y[8];
    int n;
};

// append p to the FRONT of q's first NOUT slots when `emit`
template <int NOUT>
__device__ __forceinline__ void poly_push(Poly &q, float px, float py, bool emit)
{
#pragma unroll
    for (int s = NOUT - 1; s >= 1; --s) {
        q.x[s] = emit ? q.x[s - 1] : q.x[s];
        q.y[s] = emit ? q.y[s - 1] : q.y[s];
    }
    q.x[0] = emit ? px : q.x[0];
    q.y[0] = emit ? py : q.y[0];
    q.n += emit ? 1 : 0;
}

// q = p clipped to the half-plane off - (sx x + sy y) >= 0; p holds at most NIN vertices, q at most NIN + 1
template <int NIN>
__device__ __forceinline__ void poly_clip(const Poly &p, float sx, float sy, float off, Poly &q)
{
    float d[NIN];
#pragma unroll
    for (int i = 0; i < NIN; ++i) d[i] = off - (sx * p.x[i] + sy * p.y[i]);
    q.n = 0;
#pragma unroll
    for (int i = 0; i < NIN; ++i) {
        const bool act = i < p.n;
        const bool wrap = (i + 1 == p.n) || (i + 1 == NIN);   // the edge back to vertex 0
        const int i1 = i + 1 < NIN ? i + 1 : 0;
        const float xn = wrap ? p.x[0] : p.x[i1];
        const float yn = wrap ? p.y[0] : p.y[i1];
        const float dn = wrap ? d[0] : d[i1];
        const bool in_c = d[i] >= 0.0f, in_n = dn >= 0.0f;
        poly_push<NIN + 1>(q, p.x[i], p.y[i], act && in_c);
        const float t = d[i] / (d[i] - dn);
        const float ix = p.x[i] + t * (xn - p.x[i]);
        const float iy = p.y[i] + t * (yn - p.y[i]);
        poly_push<NIN + 1>(q, ix, iy, act && (in_c != in_n));
    }
}

// exact area of the intersection of two rotated rectangles (the caller has dealt with empty rectangles)
__device__ __forceinline__ float rbox_intersection(const RBox &A, const RBox &B)
{
    // both boxes relative to the midpoint of their centres: coordinates reach +-75 m, the overlap of two 2 m
    // boxes must not be lost to that offset
    const float mx = (A.x + B.x) * 0.5f, my = (A.y + B.y) * 0.5f;
    const float ax = A.x - mx, ay = A.y - my, bx = B.x - mx, by = B.y - my;
    // far apart: the circumscribed circles do not meet
    const float ddx = bx - ax, ddy = by - ay;
    const float r = 0.5f * sqrtf(A.w * A.w + A.h * A.h) + 0.5f * sqrtf(B.w * B.w + B.h * B.h);
    if (ddx * ddx + ddy * ddy > r * r) return 0.0f;

    const float hwb = B.w * 0.5f, hhb = B.h * 0.5f;
    Poly p, q;
#pragma unroll
    for (int s = 0; s < 8; ++s) p.x[s] = p.y[s] = q.x[s] = q.y[s] = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float lx = (k == 0 || k == 3) ? hwb : -hwb;
        const float ly = (k < 2) ? hhb : -hhb;
        const float wx = bx + (lx * B.c - ly * B.s);      // B's corner, midpoint frame
        const float wy = by + (lx * B.s + ly * B.c);
        const float ux = wx - ax, uy = wy - ay;
        p.x[k] = ux * A.c + uy * A.s;                     // in A's axes
        p.y[k] = uy * A.c - ux * A.s;
    }
    p.n = 4;
    const float hwa = A.w * 0.5f, hha = A.h * 0.5f;
    poly_clip<4>(p, 1.0f, 0.0f, hwa, q);
    poly_clip<5>(q, -1.0f, 0.0f, hwa, p);
    poly_clip<6>(p, 0.0f, 1.0f, hha, q);
    poly_clip<7>(q, 0.0f, -1.0f, hha, p);
    float acc = 0.0f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const bool wrap = (i + 1 == p.n) || (i + 1 == 8);
        const int i1 = i + 1 < 8 ? i + 1 : 0;
        const float xn = wrap ? p.x[0] : p.x[i1];
        const float yn = wrap ? p.y[0] : p.y[i1];
        const float cr = p.x[i] * yn - xn * p.y[i];
        acc += i < p.n ? cr : 0.0f;
    }
    return 0.5f * fabsf(acc);
}

// exact IoU of two rotated rectangles; 0 when either area is below 1e-14
__device__ __forceinline__ float rbox_iou(const RBox &A, const RBox &B)
{
    const float area_a = A.w * A.h, area_b = B.w * B.h;
    if (area_a < AREA_EPS || area_b < AREA_EPS) return 0.0f;
    const float inter = rbox_intersection(A, B);
    return inter / (area_a + area_b - inter);
}

}  // namespace dfm
