// f2v_common.h -- what the FrustumToVoxel translation units share (frustum_to_voxel.hip: forward,
// frustum_to_voxel_bwd.hip: the three backward forms, voxel_sample.hip: the inverse op).
//
// The project's guarantees -- fused vs materialised depth head bit for bit, gather backward == scatter
// backward over the same (voxel, corner, weight) set, backward weights == forward weights -- rest on every
// kernel running the SAME arithmetic per voxel.  It is stated once, here: f2v_project (voxel -> normalised
// frustum position and validity), pred_disp (the depth probability at that position), make_tri / tri_sample
// (ATen's trilinear corners).  What differs between the kernels -- whether an invalid voxel is evaluated at
// all -- stays with each caller.
//
// Arithmetic = ATen grid_sampler_3d_cpu_impl (scalar path): corner weights
// (x1-ix)*(y1-iy)*(z1-iz) ..., out = 0; out += v*w over the in-bounds corners in
// the order tnw,tne,tsw,tse,bnw,bne,bsw,bse, multiply and add unfused.
//
// Everything lives in an anonymous namespace on purpose: the kernels of the three units are internal to
// their unit and their (mangled) names carry these types.
#pragma once
#include "dfm_common.h"

using namespace dfm;

namespace {

// A lane (= one voxel) writes its channels-last row as 16-byte pieces; the lanes of a store instruction
// are 128-256 B apart, so one instruction touches 64 partial lines that the row's other stores complete.
// PLAIN stores let the L2 merge them: the non-temporal form pushed partial lines out and measured 1.9x
// slower here (f2v_cl 1.93 -> 3.59 ms, profiles/archive/r04_c7_lift_nt_vs_plain.txt) -- while the batched
// multi-view kernel (point_sample.hip), whose lanes write whole contiguous KiBs, gains 6 % from nt.
template <typename T>
__device__ __forceinline__ void lift_store16(T *p, const float (&f)[dfm::vec16<T>::N])
{
    dfm::store16<T>(p, f);
}

struct F2vGeom {
    int32_t C, D, H, W, Ds, Hs, Ws, Cs, Hsem, Wsem, Nz, Ny, Nx;
    float pad_h, pad_w, depth_min, depth_span;
    int32_t out_cl;      // out stored (B, Nz, Ny, Nx, C + Cs): torch channels_last_3d
    int32_t cd, ch, cw;  // fused depth head: size of the low-resolution cost volume (Ds = scale * cd ...)
    int32_t st_att;      // stereo_atten_feat: Voxel *= pred_disp      (feature_transformation.py:141-142)
    int32_t sem_att;     // sem_atten_feat:    Voxel_2D *= pred_disp   (feature_transformation.py:154-155)
};

// Fused DepthHead: the depth distribution the reference samples,
//   softmax_d(Upsample_x4(cost))          dense_heads/depth_head.py:205-207
// is evaluated at the (up to) 8 lattice corners of the voxel directly from the low-resolution
// cost volume and the per-column softmax statistics (col_max, col_sum from
// dfm_depth_head_stats_fwd), with the arithmetic of depth_head_kernel -- the value at a corner is
// bit for bit what that kernel would have stored -- instead of reading a materialised
// (B, 1, 4D, 4H, 4W) tensor (472 MB per sample at config K, written once and read once).
struct FusedHead {
    const void *cost;      // (B, 1, cd, ch, cw), T
    const float *col_max;  // (B, Hs, Ws)
    const float *col_sum;
};

template <typename T>
__device__ __forceinline__ float fused_disp(const F2vGeom &g, const T *__restrict__ cost,
                                            const float *__restrict__ cmax,
                                            const float *__restrict__ csum, float gx, float gy, float gz)
{
    const int D = g.Ds, H = g.Hs, W = g.Ws;
    const float ix = ((gx + 1.0f) / 2.0f) * (float)(W - 1);
    const float iy = ((gy + 1.0f) / 2.0f) * (float)(H - 1);
    const float iz = ((gz + 1.0f) / 2.0f) * (float)(D - 1);
    const float x0 = floorf(ix), y0 = floorf(iy), z0 = floorf(iz);
    const float x1 = x0 + 1.0f, y1 = y0 + 1.0f, z1 = z0 + 1.0f;
    const bool fin = fabsf(ix) <= 1.0e9f && fabsf(iy) <= 1.0e9f && fabsf(iz) <= 1.0e9f;
    float wgt[8];
    wgt[0] = (x1 - ix) * (y1 - iy) * (z1 - iz);
    wgt[1] = (ix - x0) * (y1 - iy) * (z1 - iz);
    wgt[2] = (x1 - ix) * (iy - y0) * (z1 - iz);
    wgt[3] = (ix - x0) * (iy - y0) * (z1 - iz);
    wgt[4] = (x1 - ix) * (y1 - iy) * (iz - z0);
    wgt[5] = (ix - x0) * (y1 - iy) * (iz - z0);
    wgt[6] = (x1 - ix) * (iy - y0) * (iz - z0);
    wgt[7] = (ix - x0) * (iy - y0) * (iz - z0);
    float out = 0.0f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float xf = (k & 1) ? x1 : x0, yf = (k & 2) ? y1 : y0, zf = (k & 4) ? z1 : z0;
        const bool ok = fin && xf >= 0.0f && xf <= (float)(W - 1) && yf >= 0.0f && yf <= (float)(H - 1) &&
                        zf >= 0.0f && zf <= (float)(D - 1);
        if (!ok) continue;
        const int xc = (int)xf, yc = (int)yf, zc = (int)zf;
        const UpIdx uw = up_index(xc, g.cw, W), uh = up_index(yc, g.ch, H), ud = up_index(zc, g.cd, D);
        const int r0 = uh.i0 * g.cw, r1 = uh.i1 * g.cw;
        float col[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const T *p = cost + (size_t)(e ? ud.i1 : ud.i0) * g.ch * g.cw;
            const float a = lerp_fma(uw.w0, elem<T>::load(p[r0 + uw.i0]), uw.w1, elem<T>::load(p[r0 + uw.i1]));
            const float b = lerp_fma(uw.w0, elem<T>::load(p[r1 + uw.i0]), uw.w1, elem<T>::load(p[r1 + uw.i1]));
            col[e] = lerp_fma(uh.w0, a, uh.w1, b);
        }
        // depth_volumes and its softmax are stored (and read back) in T by the unfused pipeline
        const float logit = elem<T>::load(elem<T>::store(lerp_fma(ud.w0, col[0], ud.w1, col[1])));
        const size_t pix = (size_t)yc * W + xc;
        const float prob = elem<T>::load(elem<T>::store(exp_nonpos(logit - cmax[pix]) * (1.0f / csum[pix])));
        out = out + prob * wgt[k];
    }
    return out;
}

struct Tri {
    int o[8];     // element offsets of the 8 corners (valid only where ok bit set)
    float w[8];   // corner weights, ATen order
    uint32_t ok;
};

__device__ __forceinline__ Tri make_tri(float gx, float gy, float gz, int D, int H, int W)
{
    Tri t;
    const float ix = ((gx + 1.0f) / 2.0f) * (float)(W - 1);
    const float iy = ((gy + 1.0f) / 2.0f) * (float)(H - 1);
    const float iz = ((gz + 1.0f) / 2.0f) * (float)(D - 1);
    const float x0 = floorf(ix), y0 = floorf(iy), z0 = floorf(iz);
    const float x1 = x0 + 1.0f, y1 = y0 + 1.0f, z1 = z0 + 1.0f;
    t.w[0] = (x1 - ix) * (y1 - iy) * (z1 - iz);
    t.w[1] = (ix - x0) * (y1 - iy) * (z1 - iz);
    t.w[2] = (x1 - ix) * (iy - y0) * (z1 - iz);
    t.w[3] = (ix - x0) * (iy - y0) * (z1 - iz);
    t.w[4] = (x1 - ix) * (y1 - iy) * (iz - z0);
    t.w[5] = (ix - x0) * (y1 - iy) * (iz - z0);
    t.w[6] = (x1 - ix) * (iy - y0) * (iz - z0);
    t.w[7] = (ix - x0) * (iy - y0) * (iz - z0);
    const bool fin = fabsf(ix) <= 1.0e9f && fabsf(iy) <= 1.0e9f && fabsf(iz) <= 1.0e9f;  // no NaN/Inf
    const bool bx0 = fin && x0 >= 0.0f && x0 <= (float)(W - 1), bx1 = fin && x1 >= 0.0f && x1 <= (float)(W - 1);
    const bool by0 = fin && y0 >= 0.0f && y0 <= (float)(H - 1), by1 = fin && y1 >= 0.0f && y1 <= (float)(H - 1);
    const bool bz0 = fin && z0 >= 0.0f && z0 <= (float)(D - 1), bz1 = fin && z1 >= 0.0f && z1 <= (float)(D - 1);
    const int xi = bx0 ? (int)x0 : 0, yi = by0 ? (int)y0 : 0, zi = bz0 ? (int)z0 : 0;
    const int xj = bx1 ? (int)x1 : 0, yj = by1 ? (int)y1 : 0, zj = bz1 ? (int)z1 : 0;
    t.o[0] = (zi * H + yi) * W + xi; t.o[1] = (zi * H + yi) * W + xj;
    t.o[2] = (zi * H + yj) * W + xi; t.o[3] = (zi * H + yj) * W + xj;
    t.o[4] = (zj * H + yi) * W + xi; t.o[5] = (zj * H + yi) * W + xj;
    t.o[6] = (zj * H + yj) * W + xi; t.o[7] = (zj * H + yj) * W + xj;
    t.ok = (uint32_t)(bz0 && by0 && bx0) | ((uint32_t)(bz0 && by0 && bx1) << 1) |
           ((uint32_t)(bz0 && by1 && bx0) << 2) | ((uint32_t)(bz0 && by1 && bx1) << 3) |
           ((uint32_t)(bz1 && by0 && bx0) << 4) | ((uint32_t)(bz1 && by0 && bx1) << 5) |
           ((uint32_t)(bz1 && by1 && bx0) << 6) | ((uint32_t)(bz1 && by1 && bx1) << 7);
    return t;
}

template <typename T>
__device__ __forceinline__ float tri_sample(const Tri &t, const T *__restrict__ vol)
{
    float out = 0.0f;
#pragma unroll
    for (int k = 0; k < 8; ++k)
        if (t.ok & (1u << k)) out = out + elem<T>::load(vol[t.o[k]]) * t.w[k];
    return out;
}

// Voxel i of sample b in the frustum (feature_transformation.py:95-131): the voxel centre projected with
// cam2img[:3], normalised to grid_sample's (gx, gy, gz); valid2d = inside the padded image, valid = and inside
// the depth range.  Every FrustumToVoxel kernel, forward and backward, starts here.
struct F2vVoxel {
    float gx, gy, gz;
    bool valid2d, valid;
};

__device__ __forceinline__ F2vVoxel f2v_project(const F2vGeom &g, const float *__restrict__ coords,
                                                const float *__restrict__ cam2img, int b, long long i)
{
    const float xs = coords[3 * i], ys = coords[3 * i + 1], zs = coords[3 * i + 2];
    const float *P = cam2img + 16 * b;  // rows 0..2 of the 4x4 == cam2img[:3]
    const float a = dot4_chain(-ys, -zs, xs, 1.0f, P + 0);
    const float bb = dot4_chain(-ys, -zs, xs, 1.0f, P + 4);
    const float c = dot4_chain(-ys, -zs, xs, 1.0f, P + 8);
    const float u = a / c, v = bb / c;
    F2vVoxel p;
    p.valid2d = (u >= 0.0f) && (u <= g.pad_w) && (v >= 0.0f) && (v <= g.pad_h);
    float gx = (u - 0.0f) / (g.pad_w - 1.0f), gy = (v - 0.0f) / (g.pad_h - 1.0f);
    float gz = (xs - g.depth_min) / g.depth_span;
    gx = gx * 2.0f - 1.0f; gy = gy * 2.0f - 1.0f; gz = gz * 2.0f - 1.0f;
    p.gx = gx; p.gy = gy; p.gz = gz;
    p.valid = p.valid2d && gz >= -1.0f && gz <= 1.0f;
    return p;
}

// does any branch want pred_disp?  (feature_transformation.py:133-139)
__device__ __forceinline__ bool f2v_wants_disp(const F2vGeom &g) { return g.st_att || (g.Cs > 0 && g.sem_att); }

// grid_sample(stereo_feat_softmax) at the voxel, RAW (no validity factor, no gating: the callers' business):
// from the materialised distribution `soft`, or -- fh.cost set -- evaluated from the low-resolution cost
template <typename T>
__device__ __forceinline__ float pred_disp(const F2vGeom &g, const T *__restrict__ soft, const FusedHead &fh, int b,
                                           float gx, float gy, float gz)
{
    if (fh.cost)
        return fused_disp<T>(g, (const T *)fh.cost + (size_t)b * g.cd * g.ch * g.cw,
                             fh.col_max + (size_t)b * g.Hs * g.Ws, fh.col_sum + (size_t)b * g.Hs * g.Ws, gx, gy, gz);
    const Tri ts = make_tri(gx, gy, gz, g.Ds, g.Hs, g.Ws);
    return tri_sample<T>(ts, soft + (size_t)b * g.Ds * g.Hs * g.Ws);
}

// ---- host side -----------------------------------------------------------------------------------------

// the kernels' geometry from the descriptor; with the depth head fused (fh.cost) the low-resolution cost
// volume's size, which head_scale must divide out of (ds, hs, ws)
inline int f2v_geom(const dfm_f2v_desc *d, FusedHead fh, int32_t head_scale, F2vGeom *gp)
{
    F2vGeom &g = *gp;
    g.C = d->channels; g.D = d->d; g.H = d->h; g.W = d->w;
    g.Ds = d->ds; g.Hs = d->hs; g.Ws = d->ws;
    g.Cs = d->sem_channels; g.Hsem = d->hsem; g.Wsem = d->wsem;
    g.Nz = d->nz; g.Ny = d->ny; g.Nx = d->nx;
    g.pad_h = d->pad_h; g.pad_w = d->pad_w; g.depth_min = d->depth_min; g.depth_span = d->depth_span;
    g.cd = g.ch = g.cw = 0;
    g.st_att = d->stereo_atten ? 1 : 0;
    g.sem_att = d->no_sem_atten ? 0 : 1;
    g.out_cl = d->out_channels_last ? 1 : 0;  // (backward: grad_out comes in the layout the forward wrote)
    if (fh.cost) {
        if (head_scale <= 0 || d->ds % head_scale || d->hs % head_scale || d->ws % head_scale)
            return set_error(DFM_ERR_INVALID_ARG, "ds, hs, ws must be multiples of the depth head's scale");
        g.cd = d->ds / head_scale; g.ch = d->hs / head_scale; g.cw = d->ws / head_scale;
    }
    return DFM_OK;
}

// The pixel-major workspaces: the forward's packed copies ([d*h*w][C] and [hsem*wsem][Cs], esz = the element
// size of T) and the backward's fp32 scratch of the same shapes (esz = 4).  Two sub-buffers, the second one
// `first` bytes in (a multiple of 256); the size queries add 256 bytes of slack.
struct F2vPmLayout {
    size_t first, second;  // bytes: stereo part rounded up to 256, semantic part as it is
    size_t total() const { return first + ((second + 255) & ~(size_t)255) + 256; }
};

inline F2vPmLayout f2v_pm_layout(const dfm_f2v_desc *d, size_t esz)
{
    const size_t a = (size_t)d->batch * d->channels * d->d * d->h * d->w * esz;
    const size_t b = (size_t)d->batch * d->sem_channels * d->hsem * d->wsem * esz;
    return F2vPmLayout{(a + 255) & ~(size_t)255, b};
}

}  // namespace
