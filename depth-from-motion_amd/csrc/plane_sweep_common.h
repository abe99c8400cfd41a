// plane_sweep_common.h -- what the plane-sweep translation units share: the kernel-side geometry, the
// lattice point -> sampling position arithmetic, the bilinear footprints and the host-side entry points
// the files call across.  Included by plane_sweep.hip, plane_sweep_bwd.hip, plane_sweep_cl.hip,
// plane_sweep_bwd_mfma.hip, plane_sweep_bwd_gather.hip, sweep_conv.hip and point_sample.hip (make_tap).
// The numerics contract of dfm_common.h holds here.
#pragma once
#include "dfm_common.h"

namespace dfm {

struct SweepGeom;
struct SweepFast;
// defined in plane_sweep.hip, used by the other plane-sweep translation units
int sweep_check_desc(const dfm_sweep_desc *d);
SweepGeom sweep_make_geom(const dfm_sweep_desc *d);
void sweep_set_last_kernel(int which);  // what dfm_plane_sweep_last_kernel() reports
SweepFast sweep_make_fast(const dfm_sweep_desc *d);
// sweep_bwd_kernel, the backward's lane-per-point scatter (reference layout; the caller checks the launch)
int sweep_bwd_scatter_launch(const dfm_sweep_desc *desc, const void *grad_out, const float *depths,
                             const float *cam2img, const float *cam2img_inv, const float *cur2prev,
                             float *grad_cur, float *grad_prev, void *stream);
// defined in plane_sweep_bwd.hip
void sweep_set_last_bwd_kernel(int which);  // what dfm_plane_sweep_bwd_last_kernel() reports
// strided sweeps in the reference layout: pixel-major taps + LDS transpose (plane_sweep_cl.hip)
bool sweep_clt_supported(const dfm_sweep_desc *d, const void *out);
size_t sweep_clt_workspace_bytes(const dfm_sweep_desc *d);
int sweep_clt_launch(const dfm_sweep_desc *d, const void *cur, const void *prev, const float *depths,
                     const float *cam2img, const float *cam2img_inv, const float *cur2prev, void *out,
                     void *workspace, void *stream, bool nhwc = false, bool walk = true);
bool sweep_cltw_supported(const dfm_sweep_desc *d, const void *out);
// the matrix-product backward (plane_sweep_bwd_mfma.hip)
bool sweep_bwd_mfma_supported(const dfm_sweep_desc *d, const void *grad_out);
int sweep_bwd_mfma_launch(const dfm_sweep_desc *d, int half, const void *grad_out, const float *depths,
                          const float *P, const float *Pinv, const float *Tm, float *grad_cur, float *grad_prev,
                          void *stream);
// zoom (map pixels per lattice point) up to which the matrix-product backward takes a plane of the prev
// map: whole 32-point segments up to SWEEP_BWD_ZOOM_ONE, in two 16-point passes up to
// SWEEP_BWD_ZOOM_TWO, in four 8-point passes up to SWEEP_BWD_ZOOM_FOUR (its accumulator window is 48
// columns x 6 rows); beyond that the LDS-atomic tile kernel (the two kernels split the planes by
// sweep_zoom_split with SWEEP_BWD_ZOOM_FOUR)
constexpr float SWEEP_BWD_ZOOM_ONE = 1.4f, SWEEP_BWD_ZOOM_TWO = 2.75f, SWEEP_BWD_ZOOM_FOUR = 3.9f;

// kernel-side geometry (mirror of dfm_sweep_desc, plus derived sizes)
struct SweepGeom {
    int32_t C, h_in, w_in, D, h_out, w_out;
    int32_t nblk;  // ceil(C / CB)
    int32_t flip;
    float fsf, csf, scale, crop_x, crop_y, org_w;
    long long N;  // D*h_out*w_out
};

// One lattice point -> UNNORMALISED pixel coordinates in the cur and prev
// feature maps (what F.grid_sample computes internally from the reference's
// normalised grid).  Also returns the normalised grid when `norm` != nullptr.
// Follows dfm_backbone.py:247-294 + ATen grid_sampler_unnormalize op by op.
__device__ __forceinline__ void sweep_point(const SweepGeom &g, const float *__restrict__ P,
                                            const float *__restrict__ Pinv,
                                            const float *__restrict__ Tm, float depth, int hi,
                                            int wi, float &cx, float &cy, float &px, float &py,
                                            float *norm)
{
    float x = ((float)wi * g.fsf) * g.csf;
    float y = ((float)hi * g.fsf) * g.csf;
    x = x + g.crop_x;
    y = y + g.crop_y;
    x = x / g.scale;
    y = y / g.scale;
    if (g.flip) x = g.org_w - x;
    // points_img2cam
    const float h0 = x * depth, h1 = y * depth, h2 = depth;
    const float X0 = dot4_chain(h0, h1, h2, 1.0f, Pinv + 0);
    const float X1 = dot4_chain(h0, h1, h2, 1.0f, Pinv + 4);
    const float X2 = dot4_chain(h0, h1, h2, 1.0f, Pinv + 8);
    // cur: points_cam2img with the 4x4
    float a = dot4_chain(X0, X1, X2, 1.0f, P + 0);
    float b = dot4_chain(X0, X1, X2, 1.0f, P + 4);
    float c = dot4_chain(X0, X1, X2, 1.0f, P + 8);
    float cu = a / c, cv = b / c;
    // prev: cur2prev then project
    const float Y0 = dot4_chain(X0, X1, X2, 1.0f, Tm + 0);
    const float Y1 = dot4_chain(X0, X1, X2, 1.0f, Tm + 4);
    const float Y2 = dot4_chain(X0, X1, X2, 1.0f, Tm + 8);
    a = dot4_chain(Y0, Y1, Y2, 1.0f, P + 0);
    b = dot4_chain(Y0, Y1, Y2, 1.0f, P + 4);
    c = dot4_chain(Y0, Y1, Y2, 1.0f, P + 8);
    float pu = a / c, pv = b / c;
    if (g.flip) {
        cu = g.org_w - cu;
        pu = g.org_w - pu;
    }
    cu = cu * g.scale; cv = cv * g.scale;
    pu = pu * g.scale; pv = pv * g.scale;
    cu = cu - g.crop_x; cv = cv - g.crop_y;
    pu = pu - g.crop_x; pv = pv - g.crop_y;
    cu = cu / g.fsf; cv = cv / g.fsf;
    pu = pu / g.fsf; pv = pv / g.fsf;
    const float wm1 = (float)(g.w_in - 1), hm1 = (float)(g.h_in - 1);
    const float ncx = cu / wm1 * 2.0f - 1.0f;
    const float ncy = cv / hm1 * 2.0f - 1.0f;
    const float npx = pu / wm1 * 2.0f - 1.0f;
    const float npy = pv / hm1 * 2.0f - 1.0f;
    if (norm) {
        norm[0] = ncx; norm[1] = ncy; norm[2] = npx; norm[3] = npy;
    }
    // grid_sampler_unnormalize, align_corners=True
    cx = ((ncx + 1.0f) / 2.0f) * wm1;
    cy = ((ncy + 1.0f) / 2.0f) * hm1;
    px = ((npx + 1.0f) / 2.0f) * wm1;
    py = ((npy + 1.0f) / 2.0f) * hm1;
}

// Same arithmetic as sweep_point, but only the map the caller samples
// (HALF 0 = cur, 1 = prev), and with the divisions that are exact no-ops or
// exact scalings folded: x / 1.0f == x, x / 2^k == x * 2^-k (both bit-exact
// for the normal-range values this path sees; wave-uniform branches).
struct SweepFast {
    int32_t scale_is_one;  // img_scale_factor == 1.0f
    int32_t fsf_pow2;      // feat_sample_factor is a power of two
    float inv_fsf;         // 1 / fsf, exact when fsf_pow2
};

template <int HALF>
__device__ __forceinline__ void sweep_point_map(const SweepGeom &g, const SweepFast &f,
                                                const float *__restrict__ P,
                                                const float *__restrict__ Pinv,
                                                const float *__restrict__ Tm, float depth, int hi,
                                                int wi, float &ox, float &oy)
{
    float x = ((float)wi * g.fsf) * g.csf;
    float y = ((float)hi * g.fsf) * g.csf;
    x = x + g.crop_x;
    y = y + g.crop_y;
    if (!f.scale_is_one) {
        x = x / g.scale;
        y = y / g.scale;
    }
    if (g.flip) x = g.org_w - x;
    const float h0 = x * depth, h1 = y * depth, h2 = depth;
    float X0 = dot4_chain(h0, h1, h2, 1.0f, Pinv + 0);
    float X1 = dot4_chain(h0, h1, h2, 1.0f, Pinv + 4);
    float X2 = dot4_chain(h0, h1, h2, 1.0f, Pinv + 8);
    if (HALF) {
        const float Y0 = dot4_chain(X0, X1, X2, 1.0f, Tm + 0);
        const float Y1 = dot4_chain(X0, X1, X2, 1.0f, Tm + 4);
        const float Y2 = dot4_chain(X0, X1, X2, 1.0f, Tm + 8);
        X0 = Y0; X1 = Y1; X2 = Y2;
    }
    const float a = dot4_chain(X0, X1, X2, 1.0f, P + 0);
    const float b = dot4_chain(X0, X1, X2, 1.0f, P + 4);
    const float c = dot4_chain(X0, X1, X2, 1.0f, P + 8);
    float u = a / c, v = b / c;
    if (g.flip) u = g.org_w - u;
    if (!f.scale_is_one) {
        u = u * g.scale;
        v = v * g.scale;
    }
    u = u - g.crop_x;
    v = v - g.crop_y;
    if (f.fsf_pow2) {
        u = u * f.inv_fsf;
        v = v * f.inv_fsf;
    } else {
        u = u / g.fsf;
        v = v / g.fsf;
    }
    const float wm1 = (float)(g.w_in - 1), hm1 = (float)(g.h_in - 1);
    const float nx = u / wm1 * 2.0f - 1.0f;
    const float ny = v / hm1 * 2.0f - 1.0f;
    ox = ((nx + 1.0f) * 0.5f) * wm1;
    oy = ((ny + 1.0f) * 0.5f) * hm1;
}

// ---- backward of the plane sweep: pieces shared by the backward translation units ----
// packed footprint of one (plane, point): bit 31 valid, 27..30 = wok eok nok sok,
// 13..25 = ixw + 1, 0..12 = iyn + 1 (corner in [-1, W-1] x [-1, H-1])
__device__ __forceinline__ uint32_t bwd_footprint(float sx, float sy, int H, int W, float &fw, float &fn)
{
    const bool fin = (fabsf(sx) <= 3.0e38f) && (fabsf(sy) <= 3.0e38f);
    const float xw = floorf(sx), yn = floorf(sy);
    fw = sx - xw;
    fn = sy - yn;
    const bool wok = fin && xw >= 0.0f && xw <= (float)(W - 1);
    const bool eok = fin && xw >= -1.0f && xw <= (float)(W - 2);
    const bool nok = fin && yn >= 0.0f && yn <= (float)(H - 1);
    const bool sok = fin && yn >= -1.0f && yn <= (float)(H - 2);
    if (!((wok || eok) && (nok || sok))) return 0u;
    const int ixw = (int)xw, iyn = (int)yn;
    return 0x80000000u | ((uint32_t)wok << 27) | ((uint32_t)eok << 28) | ((uint32_t)nok << 29) |
           ((uint32_t)sok << 30) | ((uint32_t)(ixw + 1) << 13) | (uint32_t)(iyn + 1);
}

// First plane of sample b's sweep over map HALF from which on no lattice row / column is stretched
// beyond `zoom` map pixels per lattice point (forward motion zooms the nearest planes of the prev map;
// a plane qualifies only if every later plane does).  Judged on the sample positions of the four
// lattice corners, the extremes of a projective map.  The matrix-product backward takes the planes
// from the split on, the LDS-atomic backward the planes before it; both call THIS function with the
// same arguments, so they agree bit for bit on who owns a plane.  All threads of the workgroup call
// it (`slot` is an LDS word; two barriers inside).
template <int HALF>
__device__ __forceinline__ int sweep_zoom_split(const SweepGeom &g, const SweepFast &f, const float *__restrict__ P,
                                                const float *__restrict__ Pinv, const float *__restrict__ Tm,
                                                const float *__restrict__ depths, float zoom, int tid, int nthreads,
                                                int *slot)
{
    if (tid == 0) *slot = 0;
    __syncthreads();
    const float sx = zoom * (float)(g.w_out - 1) + 2.0f, sy = zoom * (float)(g.h_out - 1) + 2.0f;
    for (int d = tid; d < g.D; d += nthreads) {
        float cx[4], cy[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            sweep_point_map<HALF>(g, f, P, Pinv, Tm, depths[d], (k >> 1) ? g.h_out - 1 : 0, (k & 1) ? g.w_out - 1 : 0,
                                  cx[k], cy[k]);
        const bool ok = fabsf(cx[1] - cx[0]) <= sx && fabsf(cx[3] - cx[2]) <= sx && fabsf(cy[2] - cy[0]) <= sy &&
                        fabsf(cy[3] - cy[1]) <= sy;  // false for NaN
        if (!ok) atomicMax(slot, d + 1);
    }
    __syncthreads();
    return *slot;
}

// Bilinear footprint of one sample point: top-left integer corner, the four
// corner weights (ATen compute_interp_params) and per-corner in-bounds bits.
struct Tap {
    int ix, iy;          // clamped so that (iy, ix) .. (iy+1, ix+1) are addressable
    float nw, ne, sw, se;
    uint32_t ok;         // bit0 nw, bit1 ne, bit2 sw, bit3 se
    int dx, dy;          // 0/1: offset to the east / south tap after clamping
};

__device__ __forceinline__ Tap make_tap(float x, float y, int H, int W)
{
    Tap t;
    const bool fin = (fabsf(x) <= 3.0e38f) && (fabsf(y) <= 3.0e38f);  // false for NaN/Inf
    const float xw = floorf(x), yn = floorf(y);
    // Non-finite coordinates (a projection that divides by z = 0, utils.py:209): every tap is out of bounds AND
    // every weight is zero -- Inf - floor(Inf) is NaN, and a NaN weight times a masked (zero) tap is NaN, which
    // is what F.grid_sample on PyTorch-CPU returns there; the oracle, these kernels and torch's GPU kernel
    // return 0 (tests/golden/plane_sweep_zero_depth.npz pins it).
    const float w = fin ? x - xw : 0.0f, e = 1.0f - w, n = fin ? y - yn : 0.0f, s = 1.0f - n;
    t.nw = fin ? s * e : 0.0f; t.ne = s * w; t.sw = n * e; t.se = n * w;
    // in-bounds tests in the float domain (exact for |v| < 2^24; beyond that
    // everything is out of bounds, like ATen's saturating int conversion)
    const bool wok = fin && xw >= 0.0f && xw <= (float)(W - 1);
    const bool eok = fin && xw >= -1.0f && xw <= (float)(W - 2);
    const bool nok = fin && yn >= 0.0f && yn <= (float)(H - 1);
    const bool sok = fin && yn >= -1.0f && yn <= (float)(H - 2);
    t.ok = (uint32_t)(wok && nok) | ((uint32_t)(eok && nok) << 1) | ((uint32_t)(wok && sok) << 2) |
           ((uint32_t)(eok && sok) << 3);
    // clamp the corner so every address we form is inside the plane
    float xc = fminf(fmaxf(xw, 0.0f), (float)(W - 1));
    float yc = fminf(fmaxf(yn, 0.0f), (float)(H - 1));
    if (!fin) { xc = 0.0f; yc = 0.0f; }
    t.ix = (int)xc; t.iy = (int)yc;
    t.dx = (wok && eok) ? 1 : 0;
    t.dy = (nok && sok) ? 1 : 0;
    // when only the east (south) tap is valid the clamped corner IS that tap
    // (xw == -1 -> xc == 0): its value must be read at +0, see sample().
    return t;
}

}  // namespace dfm
