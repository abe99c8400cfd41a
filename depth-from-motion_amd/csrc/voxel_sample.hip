// voxel_sample.hip -- voxel_sample: the inverse op of FrustumToVoxel (voxel volume -> frustum), reference
// mmdet3d/models/fusion_layers/point_fusion.py:324-410, and voxel_sample_mv, its batched multi-view form;
// forward and backward.  One lane = one lattice point (w fastest); the trilinear arithmetic is
// FrustumToVoxel's (f2v_common.h: make_tri / tri_sample), or nearest.
#include "f2v_common.h"

namespace {

struct VsGeom {
    int32_t C, Nx, Ny, Nz, D, h_out, w_out, flip, mode;
    float ds, scale_x, scale_y, crop_x, crop_y, ori_w;
    float range[6], vsize[3], Minv[16];
};

// The lattice point (w, h, depth) of a view's frustum in the normalised coordinates of the voxel grid
// (point_fusion.py:366-398), gr[k] along the volume's axis k (x, y, z): the augmentations undone flip -> crop ->
// scale, points_img2cam with the fp32 inverse projection, the voxel index, the grid_sample range.  The single-view
// and the batched kernels share it, forward and backward: their coordinates are the same bits.
__device__ __forceinline__ void vs_lattice_grid(int w, int h, float depth, float ds, bool flip, float ori_w,
                                                float crop_x, float crop_y, float scale_x, float scale_y,
                                                const float *__restrict__ Minv, const float *__restrict__ range,
                                                const float *__restrict__ vsize, float (&gr)[3])
{
    float x = (float)w * ds, y = (float)h * ds;
    if (flip) x = ori_w - x;
    x = x + crop_x; y = y + crop_y;
    x = x / scale_x; y = y / scale_y;
    const float h0 = x * depth, h1 = y * depth;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float X = dot4_chain(h0, h1, depth, 1.0f, Minv + 4 * k);
        const float gsz = (range[3 + k] - range[k]) / vsize[k];
        const float v = (X - range[k]) / vsize[k] - 0.5f;
        gr[k] = v / gsz * 2.0f - 1.0f;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void voxel_sample_kernel(VsGeom g, const T *__restrict__ vox,
                                                           const float *__restrict__ depths,
                                                           T *__restrict__ out)
{
    const long long N = (long long)g.D * g.h_out * g.w_out;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int w = (int)(i % g.w_out), h = (int)((i / g.w_out) % g.h_out);
    const int d = (int)(i / ((long long)g.w_out * g.h_out));
    float gr[3];
    vs_lattice_grid(w, h, depths[d], g.ds, g.flip, g.ori_w, g.crop_x, g.crop_y, g.scale_x, g.scale_y, g.Minv,
                    g.range, g.vsize, gr);
    const size_t vol = (size_t)g.Nx * g.Ny * g.Nz;
    if (g.mode) {
        const Tri t = make_tri(gr[2], gr[1], gr[0], g.Nx, g.Ny, g.Nz);
        for (int c = 0; c < g.C; ++c)
            out[(size_t)c * N + i] = elem<T>::store(tri_sample<T>(t, vox + c * vol));
    } else {
        const float ix = ((gr[2] + 1.0f) / 2.0f) * (float)(g.Nz - 1);
        const float iy = ((gr[1] + 1.0f) / 2.0f) * (float)(g.Ny - 1);
        const float iz = ((gr[0] + 1.0f) / 2.0f) * (float)(g.Nx - 1);
        const float xr = rintf(ix), yr = rintf(iy), zr = rintf(iz);
        const bool in = fabsf(ix) <= 1.0e9f && fabsf(iy) <= 1.0e9f && fabsf(iz) <= 1.0e9f &&
                        xr >= 0.0f && xr <= (float)(g.Nz - 1) && yr >= 0.0f &&
                        yr <= (float)(g.Ny - 1) && zr >= 0.0f && zr <= (float)(g.Nx - 1);
        const int o = in ? ((int)zr * g.Ny + (int)yr) * g.Nz + (int)xr : 0;
        for (int c = 0; c < g.C; ++c)
            out[(size_t)c * N + i] = in ? vox[c * vol + o] : T(0);
    }
}

// backward of voxel_sample w.r.t. the voxel features: the same coordinates, the gradient of every
// lattice point scattered to its <= 8 corners (or its nearest voxel) with fp32 atomics
// (point_fusion.py:396-410 is differentiable through F.grid_sample).
template <typename T>
__global__ __launch_bounds__(256) void voxel_sample_bwd_kernel(VsGeom g, const T *__restrict__ gout,
                                                               const float *__restrict__ depths,
                                                               float *__restrict__ gvox)
{
    const long long N = (long long)g.D * g.h_out * g.w_out;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int w = (int)(i % g.w_out), h = (int)((i / g.w_out) % g.h_out);
    const int d = (int)(i / ((long long)g.w_out * g.h_out));
    float gr[3];
    vs_lattice_grid(w, h, depths[d], g.ds, g.flip, g.ori_w, g.crop_x, g.crop_y, g.scale_x, g.scale_y, g.Minv,
                    g.range, g.vsize, gr);
    const size_t vol = (size_t)g.Nx * g.Ny * g.Nz;
    if (g.mode) {
        const Tri t = make_tri(gr[2], gr[1], gr[0], g.Nx, g.Ny, g.Nz);
        if (!t.ok) return;
        for (int c = 0; c < g.C; ++c) {
            const float gv = elem<T>::load(gout[(size_t)c * N + i]);
            if (gv == 0.0f) continue;
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (t.ok & (1u << k)) atomicAdd(gvox + c * vol + t.o[k], gv * t.w[k]);
        }
    } else {
        const float ix = ((gr[2] + 1.0f) / 2.0f) * (float)(g.Nz - 1);
        const float iy = ((gr[1] + 1.0f) / 2.0f) * (float)(g.Ny - 1);
        const float iz = ((gr[0] + 1.0f) / 2.0f) * (float)(g.Nx - 1);
        const float xr = rintf(ix), yr = rintf(iy), zr = rintf(iz);
        const bool in = fabsf(ix) <= 1.0e9f && fabsf(iy) <= 1.0e9f && fabsf(iz) <= 1.0e9f &&
                        xr >= 0.0f && xr <= (float)(g.Nz - 1) && yr >= 0.0f &&
                        yr <= (float)(g.Ny - 1) && zr >= 0.0f && zr <= (float)(g.Nx - 1);
        if (!in) return;
        const int o = ((int)zr * g.Ny + (int)yr) * g.Nz + (int)xr;
        for (int c = 0; c < g.C; ++c) atomicAdd(gvox + c * vol + o, elem<T>::load(gout[(size_t)c * N + i]));
    }
}

int vs_geom(const dfm_vs_desc *d, VsGeom &g)
{
    if (!d) return set_error(DFM_ERR_INVALID_ARG, "desc is NULL");
    if (d->channels <= 0 || d->nx <= 0 || d->ny <= 0 || d->nz <= 0 || d->num_depths <= 0 ||
        d->h_out <= 0 || d->w_out <= 0)
        return set_error(DFM_ERR_INVALID_ARG, "non-positive size in dfm_vs_desc");
    if (int rc = check_dtype(d->dtype)) return rc;
    if ((long long)d->nx * d->ny * d->nz >= (1ll << 31))
        return set_error(DFM_ERR_UNSUPPORTED, "volume too large for 32-bit corner offsets");
    g.C = d->channels; g.Nx = d->nx; g.Ny = d->ny; g.Nz = d->nz;
    g.D = d->num_depths; g.h_out = d->h_out; g.w_out = d->w_out;
    g.flip = d->flip; g.mode = d->mode; g.ds = d->downsample_factor;
    g.scale_x = d->scale_x; g.scale_y = d->scale_y; g.crop_x = d->crop_x; g.crop_y = d->crop_y;
    g.ori_w = d->ori_w;
    for (int k = 0; k < 6; ++k) g.range[k] = d->voxel_range[k];
    for (int k = 0; k < 3; ++k) g.vsize[k] = d->voxel_size[k];
    for (int k = 0; k < 16; ++k) g.Minv[k] = d->proj_inv[k];
    return DFM_OK;
}

}  // namespace

extern "C" DFM_API int dfm_voxel_sample_fwd(const dfm_vs_desc *d, const void *voxel_features,
                                            const float *depths, void *out, void *stream)
{
    VsGeom g;
    int rc = vs_geom(d, g);
    if (rc != DFM_OK) return rc;
    if (!voxel_features || !depths || !out) return set_error(DFM_ERR_INVALID_ARG, "NULL device pointer");
    const long long N = (long long)d->num_depths * d->h_out * d->w_out;
    hipStream_t st = (hipStream_t)stream;
    by_dtype(d->dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(voxel_sample_kernel<T>, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, g,
                           (const T *)voxel_features, depths, (T *)out);
    });
    HIP_TRY(hipGetLastError());
    return DFM_OK;
}

extern "C" DFM_API int dfm_voxel_sample_bwd(const dfm_vs_desc *d, const void *grad_out,
                                            const float *depths, float *grad_voxel_features,
                                            void *stream)
{
    VsGeom g;
    int rc = vs_geom(d, g);
    if (rc != DFM_OK) return rc;
    if (!grad_out || !depths || !grad_voxel_features)
        return set_error(DFM_ERR_INVALID_ARG, "NULL device pointer");
    const long long N = (long long)d->num_depths * d->h_out * d->w_out;
    hipStream_t st = (hipStream_t)stream;
    by_dtype(d->dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(voxel_sample_bwd_kernel<T>, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, g,
                           (const T *)grad_out, depths, grad_voxel_features);
    });
    HIP_TRY(hipGetLastError());
    return DFM_OK;
}

// ---------------------------------------------------------------------------
// voxel_sample for every (sample, view) pair of a batch in one launch: what
// MultiViewDfM.feature_transformation does with B x Nv calls and two torch.cat
// (multiview_dfm.py:220-256).  The geometry of a pair (inverse projection, scale, crop, flip, ori_w) is a
// DFM_VS_PAIR_FLOATS-float row of a device array; what the pairs share is the descriptor.  A block owns VSM_TILE
// consecutive lattice points (d, h, w order) of one pair: 64 lanes work out the points' corner offsets and weights
// once -- vs_lattice_grid + make_tri, the single-view kernel's arithmetic -- and leave them in LDS; then all 256
// lanes sweep (point, channel) and add the <= 8 corners up in tri_sample's order.  The values are the single-view
// kernel's bit for bit whatever the layouts.
//   volume channels-last (C a multiple of the 16-byte block): a lane fetches a corner's block of 4 fp32 / 8 bf16
//     channels with one 16-byte load, neighbouring lanes the neighbouring blocks of the same corner; a
//     channels-last output leaves the same way, a contiguous one through an LDS transpose as 16-byte stores of
//     runs along the lattice (w fastest).
//   anything else: one element per lane and corner, lanes along the lattice for a contiguous output and along
//     the channels for a channels-last one.
// ---------------------------------------------------------------------------
namespace {

constexpr int VSM_TILE = 64;   // lattice points per block
constexpr int VSM_CHB = 32;    // channels per pass of the transposing form

struct VsmGeom {
    int32_t Nv, C, Nx, Ny, Nz, D, h_out, w_out;
    float ds, range[6], vsize[3];
};

struct VsmCorners {
    int o[8][VSM_TILE];
    float w[8][VSM_TILE];
    uint32_t ok[VSM_TILE];
};

// lanes 0 .. VSM_TILE-1: corners of lattice point i0 + lane of pair p (ok = 0 past the end of the lattice)
__device__ __forceinline__ void vsm_corners(const VsmGeom &g, const float *__restrict__ pairs,
                                            const float *__restrict__ depths, int p, long long i0, long long N,
                                            VsmCorners &s)
{
    const int t = threadIdx.x;
    if (t >= VSM_TILE) return;
    const long long i = i0 + t;
    if (i >= N) {
        s.ok[t] = 0;
        return;
    }
    const float *pr = pairs + (size_t)p * DFM_VS_PAIR_FLOATS;
    const int w = (int)(i % g.w_out), h = (int)((i / g.w_out) % g.h_out);
    const int d = (int)(i / ((long long)g.w_out * g.h_out));
    float gr[3];
    vs_lattice_grid(w, h, depths[d], g.ds, pr[21] != 0.0f, pr[20], pr[18], pr[19], pr[16], pr[17], pr, g.range,
                    g.vsize, gr);
    const Tri tr = make_tri(gr[2], gr[1], gr[0], g.Nx, g.Ny, g.Nz);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        s.o[k][t] = tr.o[k];
        s.w[k][t] = tr.w[k];
    }
    s.ok[t] = tr.ok;
}

// one element per lane and corner; vox element (c, o) at c * vcs + o * vos, out element (c, i) at c * ocs + i * ois
template <typename T, bool OCL>
__global__ __launch_bounds__(256) void voxel_sample_mv_kernel(VsmGeom g, const float *__restrict__ pairs,
                                                              const T *__restrict__ vox, size_t vcs, size_t vos,
                                                              const float *__restrict__ depths,
                                                              T *__restrict__ out, size_t ocs, size_t ois)
{
    __shared__ VsmCorners s;
    const long long N = (long long)g.D * g.h_out * g.w_out;
    const long long i0 = (long long)blockIdx.x * VSM_TILE;
    const int p = blockIdx.y;
    vsm_corners(g, pairs, depths, p, i0, N, s);
    __syncthreads();
    const T *v = vox + (size_t)(p / g.Nv) * g.C * g.Nx * g.Ny * g.Nz;
    T *o = out + (size_t)p * g.C * N;
    for (int it = threadIdx.x; it < VSM_TILE * g.C; it += 256) {
        const int pt = OCL ? it / g.C : it % VSM_TILE, c = OCL ? it % g.C : it / VSM_TILE;
        if (i0 + pt >= N) continue;
        const uint32_t ok = s.ok[pt];
        const T *vc = v + (size_t)c * vcs;
        float acc = 0.0f;
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (ok & (1u << k)) acc = acc + elem<T>::load(vc[(size_t)s.o[k][pt] * vos]) * s.w[k][pt];
        o[(size_t)c * ocs + (size_t)(i0 + pt) * ois] = elem<T>::store(acc);
    }
}

// channels-last volume, C % vec16<T>::N == 0, 16-byte aligned tensors
template <typename T, bool OCL>
__global__ __launch_bounds__(256) void voxel_sample_mv_cl_kernel(VsmGeom g, const float *__restrict__ pairs,
                                                                 const T *__restrict__ vox,
                                                                 const float *__restrict__ depths,
                                                                 T *__restrict__ out, int vec_runs)
{
    constexpr int V = vec16<T>::N;
    __shared__ VsmCorners s;
    __shared__ __attribute__((aligned(16))) T tile[OCL ? 1 : VSM_CHB][OCL ? V : VSM_TILE + V];
    const long long N = (long long)g.D * g.h_out * g.w_out;
    const long long i0 = (long long)blockIdx.x * VSM_TILE;
    const int p = blockIdx.y;
    vsm_corners(g, pairs, depths, p, i0, N, s);
    __syncthreads();
    const T *v = vox + (size_t)(p / g.Nv) * g.C * g.Nx * g.Ny * g.Nz;
    T *o = out + (size_t)p * g.C * N;
    const int cb_all = g.C / V;
    // channels-last output: every channel block in one pass; contiguous: VSM_CHB channels through the tile
    const int cb_pass = OCL ? cb_all : VSM_CHB / V;
    for (int cb0 = 0; cb0 < cb_all; cb0 += cb_pass) {
        const int ncb = min(cb_pass, cb_all - cb0);
        for (int it = threadIdx.x; it < VSM_TILE * ncb; it += 256) {
            const int pt = it / ncb, cb = cb0 + it % ncb;
            if (i0 + pt >= N) continue;
            const uint32_t ok = s.ok[pt];
            float acc[V];
#pragma unroll
            for (int j = 0; j < V; ++j) acc[j] = 0.0f;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                if (!(ok & (1u << k))) continue;
                float f[V];
                load16<T>(v + (size_t)s.o[k][pt] * g.C + cb * V, f);
                const float wk = s.w[k][pt];
#pragma unroll
                for (int j = 0; j < V; ++j) acc[j] = acc[j] + f[j] * wk;
            }
            if constexpr (OCL) {
                store16<T>(o + (size_t)(i0 + pt) * g.C + cb * V, acc);
            } else {
#pragma unroll
                for (int j = 0; j < V; ++j) tile[(cb - cb0) * V + j][pt] = elem<T>::store(acc[j]);
            }
        }
        if constexpr (!OCL) {
            __syncthreads();
            const int nch = ncb * V;
            if (vec_runs) {   // N % V == 0: the tile's runs start on 16-byte boundaries and end on one
                constexpr int RUNS = VSM_TILE / V;
                for (int it = threadIdx.x; it < nch * RUNS; it += 256) {
                    const int c = it / RUNS, r = it % RUNS;
                    if (i0 + r * V < N)
                        *(uint4 *)(o + (size_t)(cb0 * V + c) * N + i0 + r * V) = *(const uint4 *)&tile[c][r * V];
                }
            } else {
                for (int it = threadIdx.x; it < nch * VSM_TILE; it += 256) {
                    const int c = it / VSM_TILE, pt = it % VSM_TILE;
                    if (i0 + pt < N) o[(size_t)(cb0 * V + c) * N + i0 + pt] = tile[c][pt];
                }
            }
            __syncthreads();
        }
    }
}

// backward: the gradient of every lattice point of every view scattered to its <= 8 corners with fp32 atomics;
// the Nv views of a sample add into the same voxels, so the order of the sum is not fixed.  grad_out element
// (c, i) at c * gcs + i * gis, grad_vox element (c, o) at c * vcs + o * vos; lanes run along the channels when the
// gradient volume is channels-last (neighbouring lanes, neighbouring addresses), along the lattice otherwise.
template <typename T, bool VCL>
__global__ __launch_bounds__(256) void voxel_sample_mv_bwd_kernel(VsmGeom g, const float *__restrict__ pairs,
                                                                  const T *__restrict__ gout, size_t gcs, size_t gis,
                                                                  const float *__restrict__ depths,
                                                                  float *__restrict__ gvox, size_t vcs, size_t vos)
{
    __shared__ VsmCorners s;
    const long long N = (long long)g.D * g.h_out * g.w_out;
    const long long i0 = (long long)blockIdx.x * VSM_TILE;
    const int p = blockIdx.y;
    vsm_corners(g, pairs, depths, p, i0, N, s);
    __syncthreads();
    float *gv = gvox + (size_t)(p / g.Nv) * g.C * g.Nx * g.Ny * g.Nz;
    const T *go = gout + (size_t)p * g.C * N;
    for (int it = threadIdx.x; it < VSM_TILE * g.C; it += 256) {
        const int pt = VCL ? it / g.C : it % VSM_TILE, c = VCL ? it % g.C : it / VSM_TILE;
        if (i0 + pt >= N) continue;
        const uint32_t ok = s.ok[pt];
        if (!ok) continue;
        const float gval = elem<T>::load(go[(size_t)c * gcs + (size_t)(i0 + pt) * gis]);
        if (gval == 0.0f) continue;
        float *gc = gv + (size_t)c * vcs;
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (ok & (1u << k)) atomicAdd(gc + (size_t)s.o[k][pt] * vos, gval * s.w[k][pt]);
    }
}

int vsm_geom(const dfm_vs_mv_desc *d, VsmGeom &g)
{
    if (!d) return set_error(DFM_ERR_INVALID_ARG, "desc is NULL");
    if (d->batch <= 0 || d->num_views <= 0 || d->channels <= 0 || d->nx <= 0 || d->ny <= 0 || d->nz <= 0 ||
        d->num_depths <= 0 || d->h_out <= 0 || d->w_out <= 0)
        return set_error(DFM_ERR_INVALID_ARG, "non-positive size in dfm_vs_mv_desc");
    if (int rc = check_dtype(d->dtype)) return rc;
    if ((long long)d->nx * d->ny * d->nz >= (1ll << 31))
        return set_error(DFM_ERR_UNSUPPORTED, "volume too large for 32-bit corner offsets");
    if ((long long)d->batch * d->num_views > 65535)
        return set_error(DFM_ERR_UNSUPPORTED, "more than 65535 (sample, view) pairs");
    if (((long long)d->num_depths * d->h_out * d->w_out + VSM_TILE - 1) / VSM_TILE >= (1ll << 31))
        return set_error(DFM_ERR_UNSUPPORTED, "frustum lattice too large for one launch");
    g.Nv = d->num_views; g.C = d->channels; g.Nx = d->nx; g.Ny = d->ny; g.Nz = d->nz;
    g.D = d->num_depths; g.h_out = d->h_out; g.w_out = d->w_out; g.ds = d->downsample_factor;
    for (int k = 0; k < 6; ++k) g.range[k] = d->voxel_range[k];
    for (int k = 0; k < 3; ++k) g.vsize[k] = d->voxel_size[k];
    return DFM_OK;
}

}  // namespace

extern "C" DFM_API int dfm_voxel_sample_mv_fwd(const dfm_vs_mv_desc *d, const float *pairs,
                                               const void *voxel_features, const float *depths, void *out,
                                               void *stream)
{
    VsmGeom g;
    int rc = vsm_geom(d, g);
    if (rc != DFM_OK) return rc;
    if (!pairs || !voxel_features || !depths || !out) return set_error(DFM_ERR_INVALID_ARG, "NULL device pointer");
    const long long N = (long long)d->num_depths * d->h_out * d->w_out;
    const size_t vol = (size_t)d->nx * d->ny * d->nz;
    const dim3 grid((unsigned)((N + VSM_TILE - 1) / VSM_TILE), (unsigned)(d->batch * d->num_views));
    hipStream_t st = (hipStream_t)stream;
    const bool vcl = d->volume_channels_last != 0, ocl = d->out_channels_last != 0;
    const int V = d->dtype == DFM_F32 ? 4 : 8;
    const size_t esz = d->dtype == DFM_F32 ? 4 : 2;
    const bool vec = vcl && d->channels % V == 0 && (uintptr_t)voxel_features % 16 == 0 &&
                     (uintptr_t)out % 16 == 0 && (vol * d->channels * esz) % 16 == 0;
    const int vec_runs = N % V == 0 ? 1 : 0;
    const size_t vcs = vcl ? 1 : vol, vos = vcl ? (size_t)d->channels : 1;
    const size_t ocs = ocl ? 1 : (size_t)N, ois = ocl ? (size_t)d->channels : 1;
    by_dtype(d->dtype, [&](auto t) {
        using T = decltype(t);
        by_bool(ocl, [&](auto o) {
            constexpr bool OCL = decltype(o)::value;
            if (vec)
                hipLaunchKernelGGL((voxel_sample_mv_cl_kernel<T, OCL>), grid, dim3(256), 0, st, g, pairs,
                                   (const T *)voxel_features, depths, (T *)out, vec_runs);
            else
                hipLaunchKernelGGL((voxel_sample_mv_kernel<T, OCL>), grid, dim3(256), 0, st, g, pairs,
                                   (const T *)voxel_features, vcs, vos, depths, (T *)out, ocs, ois);
        });
    });
    HIP_TRY(hipGetLastError());
    return DFM_OK;
}

extern "C" DFM_API int dfm_voxel_sample_mv_bwd(const dfm_vs_mv_desc *d, const float *pairs, const void *grad_out,
                                               const float *depths, float *grad_voxel_features, void *stream)
{
    VsmGeom g;
    int rc = vsm_geom(d, g);
    if (rc != DFM_OK) return rc;
    if (!pairs || !grad_out || !depths || !grad_voxel_features)
        return set_error(DFM_ERR_INVALID_ARG, "NULL device pointer");
    const long long N = (long long)d->num_depths * d->h_out * d->w_out;
    const size_t vol = (size_t)d->nx * d->ny * d->nz;
    const dim3 grid((unsigned)((N + VSM_TILE - 1) / VSM_TILE), (unsigned)(d->batch * d->num_views));
    hipStream_t st = (hipStream_t)stream;
    const bool vcl = d->volume_channels_last != 0, ocl = d->out_channels_last != 0;
    const size_t vcs = vcl ? 1 : vol, vos = vcl ? (size_t)d->channels : 1;
    const size_t gcs = ocl ? 1 : (size_t)N, gis = ocl ? (size_t)d->channels : 1;
    by_dtype(d->dtype, [&](auto t) {
        using T = decltype(t);
        by_bool(vcl, [&](auto v) {
            hipLaunchKernelGGL((voxel_sample_mv_bwd_kernel<T, decltype(v)::value>), grid, dim3(256), 0, st, g, pairs,
                               (const T *)grad_out, gcs, gis, depths, grad_voxel_features, vcs, vos);
        });
    });
    HIP_TRY(hipGetLastError());
    return DFM_OK;
}
