// frustum_to_voxel_bwd.hip -- backward of FrustumToVoxel's sampling stage (frustum_to_voxel.hip) w.r.t.
// stereo_feat and cur_sem_feats (the depth distribution is detached in the reference,
// feature_transformation.py:136), in three forms:
//   f2v_bwd_kernel         lane = voxel, fp32 atomics into the caller's zero-initialised gradients (no workspace,
//                          or more channels than the pixel-major form's LDS tile holds)
//   f2v_bwd_pm_kernel      lanes = the channels of a voxel, coalesced atomics into pixel-major scratch
//   f2v_bwd_gather_kernel  lane = a cell column of the cost volume, no atomics on the cost volume's gradient
// All three run the forward's per-voxel arithmetic (f2v_common.h: f2v_project, pred_disp, make_tri), so they
// sum over the same (voxel, corner, weight) set with the forward's weights.
#include "f2v_common.h"

namespace {

// pred_disp (detached) scales the gradients of the attended branches.  The backward's gating: evaluated only
// for a voxel inside the frustum (no other voxel's gradient uses it), 1 when neither attention wants it.
template <typename T>
__device__ __forceinline__ float f2v_bwd_disp(const F2vGeom &g, const T *__restrict__ soft, const FusedHead &fh,
                                              int b, const F2vVoxel &p)
{
    if (!(p.valid && f2v_wants_disp(g))) return 1.0f;
    return pred_disp<T>(g, soft, fh, b, p.gx, p.gy, p.gz);
}

// One lane = one voxel; fp32 atomics into zero-initialised gradient tensors.
template <typename T>
__global__ __launch_bounds__(256) void f2v_bwd_kernel(F2vGeom g, const T *__restrict__ gout,
                                                      const T *__restrict__ soft, FusedHead fh,
                                                      const float *__restrict__ coords,
                                                      const float *__restrict__ cam2img,
                                                      float *__restrict__ gstereo,
                                                      float *__restrict__ gsem)
{
    const long long N = (long long)g.Nz * g.Ny * g.Nx;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y;
    if (i >= N) return;
    const F2vVoxel p = f2v_project(g, coords, cam2img, b, i);
    const float gx = p.gx, gy = p.gy, gz = p.gz;
    const bool valid2d = p.valid2d, valid = p.valid;
    // grad_out in the OUTPUT's layout: planar (B, C + Cs, N) or channels-last (B, N, C + Cs) (g.out_cl)
    const size_t gcs = g.out_cl ? 1 : (size_t)N;  // elements between channels of one voxel
    const T *go = g.out_cl ? gout + ((size_t)b * N + i) * (g.C + g.Cs) : gout + (size_t)b * (g.C + g.Cs) * N + i;
    const size_t vol = (size_t)g.D * g.H * g.W;
    const float disp = f2v_bwd_disp<T>(g, soft, fh, b, p);
    if (valid) {
        const Tri t = make_tri(gx, gy, gz, g.D, g.H, g.W);
        float *gs = gstereo + (size_t)b * g.C * vol;
        const float sdisp = g.st_att ? disp : 1.0f;
        for (int ch = 0; ch < g.C; ++ch) {
            const float gv = elem<T>::load(go[(size_t)ch * gcs]) * sdisp;
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (t.ok & (1u << k)) atomicAdd(gs + (size_t)ch * vol + t.o[k], gv * t.w[k]);
        }
    }
    // Voxel_2D = sample(sem) * valid2d (* disp * valid): without the attention the 2-D mask alone gates it
    if (g.Cs > 0 && (g.sem_att ? valid : valid2d)) {
        const float mdisp = g.sem_att ? disp : 1.0f;
        const Tri t2 = make_tri(gx, gy, 0.0f, 1, g.Hsem, g.Wsem);
        const size_t plane = (size_t)g.Hsem * g.Wsem;
        float *gm = gsem + (size_t)b * g.Cs * plane;
        for (int ch = 0; ch < g.Cs; ++ch) {
            const float gv = elem<T>::load(go[(size_t)(g.C + ch) * gcs]) * mdisp;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (t2.ok & (1u << k)) atomicAdd(gm + (size_t)ch * plane + t2.o[k], gv * t2.w[k]);
        }
    }
}

// Pixel-major backward.  Scattered global fp32 atomics run at ~20 G/s, a wave whose 64
// addresses are consecutive at ~320 G/s (profiles/archive/r01_atomic_microbench.txt).  So the gradients
// are accumulated in pixel-major scratch ([d*h*w][C] and [h*w][Cs], fp32): the lanes of a wave
// are the CHANNELS of a voxel, a tap is one contiguous run of C atomics.  A workgroup takes 64
// voxels: their grad_out rows come in through an LDS tile (read along voxels, used along
// channels), their footprints are computed once per voxel; a transpose pass adds the scratch into
// the caller's NC(D)HW gradients.
constexpr int F2V_VT = 64;  // voxels per workgroup

struct BwdFoot {
    int st[8];     // stereo pixel index per corner, -1 = no contribution
    float sw[8];
    int sm[4];     // semantic-map pixel index per corner, -1 = none
    float mw[4];   // corner weight * depth probability
};

template <typename T>
__global__ __launch_bounds__(256) void f2v_bwd_pm_kernel(F2vGeom g, const T *__restrict__ gout,
                                                         const T *__restrict__ soft, FusedHead fh,
                                                         const float *__restrict__ coords,
                                                         const float *__restrict__ cam2img,
                                                         float *__restrict__ gst_pm,
                                                         float *__restrict__ gsem_pm)
{
    extern __shared__ float f2v_lds[];
    const int CT = g.C + g.Cs;
    float *gt = f2v_lds;                                   // [CT][F2V_VT + 1]
    BwdFoot *foot = (BwdFoot *)(gt + CT * (F2V_VT + 1));   // [F2V_VT]
    const long long N = (long long)g.Nz * g.Ny * g.Nx;
    const long long v0 = (long long)blockIdx.x * F2V_VT;
    const int b = blockIdx.y;
    const int nv = (int)min((long long)F2V_VT, N - v0);
    const int tid = threadIdx.x;
    // grad_out rows of the tile: one channel per wave pass, 64 consecutive voxels per load
    if (g.out_cl) {
        // channels-last gradient (what an NDHWC voxel_convs backward hands over): the tile's 64 voxels x CT
        // channels are ONE contiguous run, read in place -- torch's strided re-layout of this tensor to the
        // planar form cost 2.1 ms of a 31 ms training step (profiles/archive/r05_c11_*)
        const T *go = gout + ((size_t)b * N + v0) * CT;
        for (int i = tid; i < CT * F2V_VT; i += 256) {
            const int v = i / CT, c = i - v * CT;
            gt[c * (F2V_VT + 1) + v] = v < nv ? elem<T>::load(go[i]) : 0.0f;
        }
    } else {
        const T *go = gout + (size_t)b * CT * N + v0;
        for (int i = tid; i < CT * F2V_VT; i += 256) {
            const int c = i / F2V_VT, v = i - c * F2V_VT;
            gt[c * (F2V_VT + 1) + v] = v < nv ? elem<T>::load(go[(size_t)c * N + v]) : 0.0f;
        }
    }
    if (tid < F2V_VT) {
        BwdFoot f;
#pragma unroll
        for (int k = 0; k < 8; ++k) { f.st[k] = -1; f.sw[k] = 0.0f; }
#pragma unroll
        for (int k = 0; k < 4; ++k) { f.sm[k] = -1; f.mw[k] = 0.0f; }
        if (tid < nv) {
            const long long i = v0 + tid;
            const F2vVoxel p = f2v_project(g, coords, cam2img, b, i);
            const float gx = p.gx, gy = p.gy, gz = p.gz;
            const bool valid2d = p.valid2d, valid = p.valid;
            const float disp = f2v_bwd_disp<T>(g, soft, fh, b, p);
            if (valid) {
                const Tri t = make_tri(gx, gy, gz, g.D, g.H, g.W);
                const float sdisp = g.st_att ? disp : 1.0f;
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    if (t.ok & (1u << k)) { f.st[k] = t.o[k]; f.sw[k] = t.w[k] * sdisp; }
            }
            // Voxel_2D = sample(sem) * valid2d (* disp * valid)
            if (g.Cs > 0 && (g.sem_att ? valid : valid2d)) {
                const float mdisp = g.sem_att ? disp : 1.0f;
                const Tri t2 = make_tri(gx, gy, 0.0f, 1, g.Hsem, g.Wsem);
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (t2.ok & (1u << k)) { f.sm[k] = t2.o[k]; f.mw[k] = t2.w[k] * mdisp; }
            }
        }
        foot[tid] = f;
    }
    __syncthreads();
    // lanes = channels of a voxel: [voxel in iteration][channel]
    const int wave = tid >> 6, lane = tid & 63;
    int lpv = 1;
    while (lpv < min(max(g.C, g.Cs), 64)) lpv <<= 1;  // lanes per voxel
    // a wave owns F2V_VT/4 voxels: never spread an iteration over more of them (1- and 2-channel
    // maps would otherwise scatter their neighbours' voxels a second time)
    lpv = max(lpv, 64 / (F2V_VT / 4));
    const int ch = lane & (lpv - 1), vin = lane / lpv, vpi = 64 / lpv;
    float *gs = gst_pm + (size_t)b * g.D * g.H * g.W * g.C;
    float *gm = gsem_pm + (size_t)b * g.Hsem * g.Wsem * g.Cs;
    for (int it = 0; it < F2V_VT / 4; it += vpi) {
        const int v = wave * (F2V_VT / 4) + it + vin;
        if (v >= nv) continue;
        const BwdFoot &f = foot[v];
        for (int c = ch; c < g.C; c += lpv) {
            const float gv = gt[c * (F2V_VT + 1) + v];
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (f.st[k] >= 0) atomicAdd(gs + (size_t)f.st[k] * g.C + c, gv * f.sw[k]);
        }
        for (int c = ch; c < g.Cs; c += lpv) {
            const float gv = gt[(g.C + c) * (F2V_VT + 1) + v];
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (f.sm[k] >= 0) atomicAdd(gm + (size_t)f.sm[k] * g.Cs + c, gv * f.mw[k]);
        }
    }
}


// 8 consecutive channels of one voxel's gradient row, as fp32 (one 16-byte load in bf16, two in fp32)
template <typename T>
__device__ __forceinline__ void gather_row8(const T *__restrict__ gp, float (&v)[8])
{
    if constexpr (sizeof(T) == 4) {
        const uint4 u0 = *(const uint4 *)gp, u1 = *(const uint4 *)(gp + 4);
        v[0] = __uint_as_float(u0.x); v[1] = __uint_as_float(u0.y); v[2] = __uint_as_float(u0.z); v[3] = __uint_as_float(u0.w);
        v[4] = __uint_as_float(u1.x); v[5] = __uint_as_float(u1.y); v[6] = __uint_as_float(u1.z); v[7] = __uint_as_float(u1.w);
    } else {
        const uint4 u = *(const uint4 *)gp;
        const uint32_t w4[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            v[2 * k] = __uint_as_float(w4[k] << 16);
            v[2 * k + 1] = __uint_as_float(w4[k] & 0xffff0000u);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// Backward as a GATHER (round 5).  The pixel-major scatter above runs at the part's fp32 atomic rate: 1.75 M
// voxels x 8 corners x 64 channels = 0.9 G atomics = 2.9 ms per sample at config K, the third-largest kernel of
// the training step.  Turned around: a lane owns a cell column of the cost volume -- pixel (h, w), a run of depth
// planes -- and finds the voxels whose trilinear footprint holds each cell.  The voxel grid is REGULAR
// (prepare_coordinates_3d: linspace centres, x fastest; the host checks it and passes origin and steps) and the
// voxel -> frustum map is explicit: depth is affine in the voxel's x index, and for a given x the image position
// is a projective function of (y, z) -- so for every x slab that can touch the plane a 2 x 2 linear system gives
// the (y, z) voxel position that projects onto the pixel, and solving it again one pixel further along u and v
// gives the box of voxel indices that can touch the pixel.  Every voxel in the box is then run through the
// FORWARD's own arithmetic (projection, normalisation, floor): it counts only if one of its eight corners IS this
// cell, with the forward's weight -- the (voxel, corner, weight) set is exactly the scatter's.  A hit gathers the
// voxel's gradient row (channels-last: one contiguous run).  The stereo gradient of a cell is STORED when its
// plane is done; the semantic map's gradient (same pixel, every plane: taken from the hits whose LOWER depth
// corner is the cell, so a voxel counts once) leaves as 32 atomics per lane and depth chunk instead of 128 per
// voxel.  The per-voxel factors (validity, pred_disp) come from a lane-per-voxel pre-pass into 8 bytes per voxel.
// ---------------------------------------------------------------------------------------------------------
struct F2vGrid {
    float x0, dx, y0, dy, z0, dz;  // coords[(iz * Ny + iy) * Nx + ix] == (x0 + ix dx, y0 + iy dy, z0 + iz dz)
};

constexpr uint32_t F2G_NONE = 0xffffffffu;  // cell code of a voxel the gather skips

// pre-pass, lane = voxel: the factors the scatter's first phase computes, from the same helpers.  sfac = the stereo branch's factor
// (pred_disp when stereo_atten, else 1) or -1 for a voxel that contributes nothing; mfac likewise for the
// semantic branch (pred_disp * valid when sem_atten, else valid2d).
template <typename T>
__global__ __launch_bounds__(256) void f2v_bwd_prep_kernel(F2vGeom g, const T *__restrict__ soft, FusedHead fh,
                                                           const float *__restrict__ coords,
                                                           const float *__restrict__ cam2img,
                                                           float *__restrict__ sfac, float *__restrict__ mfac,
                                                           uint32_t *__restrict__ cell, float4 *__restrict__ pos)
{
    const long long N = (long long)g.Nz * g.Ny * g.Nx;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y;
    if (i >= N) return;
    const F2vVoxel p = f2v_project(g, coords, cam2img, b, i);
    const float gx = p.gx, gy = p.gy, gz = p.gz;
    const bool valid2d = p.valid2d, valid = p.valid;
    const float disp = f2v_bwd_disp<T>(g, soft, fh, b, p);
    const float sf = valid ? (g.st_att ? disp : 1.0f) : -1.0f;
    const float mf = (g.Cs > 0 && (g.sem_att ? valid : valid2d)) ? (g.sem_att ? disp : 1.0f) : -1.0f;
    if (sfac) sfac[(size_t)b * N + i] = sf;
    mfac[(size_t)b * N + i] = mf;
    if (cell) {
        // round 6: the voxel's lower corner cell, packed, and its position in the cost volume -- make_tri's arithmetic,
        // done ONCE per voxel here instead of once per (candidate pixel, plane) in the gather.  A voxel that
        // contributes nothing (or whose position is not finite, or lies outside the packable range: it then has no
        // cell inside the volume either) is F2G_NONE.
        const float px = ((gx + 1.0f) / 2.0f) * (float)(g.W - 1);
        const float py = ((gy + 1.0f) / 2.0f) * (float)(g.H - 1);
        const float pz = ((gz + 1.0f) / 2.0f) * (float)(g.D - 1);
        uint32_t c = F2G_NONE;
        if ((sf >= 0.0f || mf >= 0.0f) && fabsf(px) <= 1.0e9f && fabsf(py) <= 1.0e9f && fabsf(pz) <= 1.0e9f) {
            const float x0 = floorf(px), y0 = floorf(py), z0 = floorf(pz);
            if (x0 >= -1.0f && x0 <= 2045.0f && y0 >= -1.0f && y0 <= 1021.0f && z0 >= -1.0f && z0 <= 1021.0f)
                c = (uint32_t)((int)x0 + 1) | ((uint32_t)((int)y0 + 1) << 11) | ((uint32_t)((int)z0 + 1) << 21);
        }
        cell[(size_t)b * N + i] = c;
        pos[(size_t)b * N + i] = make_float4(px, py, pz, sf);
    }
}

// Depth planes per lane.  Round 5 ran 9 (72 planes -> 8 chunks): 800 workgroups of a kernel that held 256 + 16
// registers a lane -- ONE workgroup per CU, 3.1 rounds over the chip, each wave waiting out its own chain of
// dependent loads: 1.80 ms.  Three planes a chunk: 0.97 ms (1, 2 planes measure the same, 4 is 9 % slower; capping
// the registers for 3 or 4 workgroups per CU spilled: 3.3 / 5.7 ms).  Then the candidate test on a packed cell word
// from the pre-pass, four lanes per pixel (150 registers, three waves per SIMD) and the slab positions as affine
// functions of the slab index: 0.75 ms -- profiles/r06_c28_f2v_bwd_depth_chunk.txt
#ifndef DFM_F2G_DCH
#define DFM_F2G_DCH 3
#endif
#ifndef DFM_F2G_WGS
#define DFM_F2G_WGS 1
#endif
constexpr int F2G_DCH = DFM_F2G_DCH;  // depth planes per lane (a chunk): 72 planes -> 24 chunks

// lane = pixel (h, w) of the cost volume x a chunk of depth planes; C == 32, Cs in {0, 32} with the semantic
// map at the cost volume's resolution.  gvs / gcs: element strides of grad_out between voxels / channels.
// GCL: the stereo gradient is written (B, D, H, W, 32) in T -- the layout and type of a channels-last cost volume,
// a lane's 32 sums as one contiguous row (a wave: 64 consecutive rows), rounded once; else planar fp32.
template <typename T, bool SEM, bool GCL>
__global__ __launch_bounds__(256, DFM_F2G_WGS) void f2v_bwd_gather_kernel(F2vGeom g, F2vGrid gr, int dchunks,
                                                             const T *__restrict__ gout, size_t gvs, size_t gcs,
                                                             const float *__restrict__ coords,
                                                             const float *__restrict__ cam2img,
                                                             const uint32_t *__restrict__ cell,
                                                             const float4 *__restrict__ pos,
                                                             const float *__restrict__ mfac,
                                                             void *__restrict__ gstv, float *__restrict__ gsem)
{
    // block id = ((ytile * xtiles + xtile) * dchunks + chunk); blockIdx.y = sample
    // (round 6) FOUR lanes per pixel, 8 channels each: a wave covers 16 pixels of a row.  A hit's gradient row is then
    // one 16-byte load per lane whose four lanes read one contiguous 64-byte row (a wave-level load touches 16 rows,
    // not 4 x 64), the accumulators are 8 + 8 registers instead of 32 + 32, and the candidate test the four lanes
    // repeat is a 4-byte load of the same word.
    const int xtiles = (g.W + 15) / 16;
    int t = blockIdx.x;
    const int chunk = t % dchunks;
    t /= dchunks;
    const int xt = t % xtiles, yt = t / xtiles;
    const int b = blockIdx.y;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int h = yt * 4 + wave, w = xt * 16 + (lane >> 2);
    const int cq = (lane & 3) * 8;  // this lane's channels: cq .. cq + 7
    const bool inside = h < g.H && w < g.W;
    const long long N = (long long)g.Nz * g.Ny * g.Nx;
    const float *P = cam2img + 16 * b;
    const int CT = g.C + g.Cs;
    // image position of this pixel's centre and of its neighbours one pixel further (the box's extent)
    const float su = (g.pad_w - 1.0f) / (float)(g.W - 1), sv = (g.pad_h - 1.0f) / (float)(g.H - 1);
    const float ut = (float)w * su, vt = (float)h * sv;
    // (y, z) of the voxel position that projects onto image point (uu, vv) in the slab x = xs: a 2 x 2 system whose
    // right-hand side is affine in xs -- and xs is affine in the slab index, so the voxel-index position of the
    // solution is iy = Ay + By * ix, iz = Az + Bz * ix: four coefficients per image point, worked out ONCE per lane
    // (round 5 solved the three systems per slab, with a division each: 200 of the ~250 instructions of a slab with
    // no candidate in it).  The box only bounds the candidates (15 % + 0.05 voxels of slack); the voxels inside it are
    // still tested with the forward's own arithmetic.
    const float idx = 1.0f / gr.dx, idy = 1.0f / gr.dy, idz = 1.0f / gr.dz;
    auto affine = [&](float uu, float vv, float &ay, float &by, float &az, float &bz) {
        const float a11 = uu * P[8] - P[0], a12 = uu * P[9] - P[1], c1 = P[2] - uu * P[10], d1 = P[3] - uu * P[11];
        const float a21 = vv * P[8] - P[4], a22 = vv * P[9] - P[5], c2 = P[6] - vv * P[10], d2 = P[7] - vv * P[11];
        const float det = a11 * a22 - a12 * a21, inv = 1.0f / det;
        // ys = ((-c1 xs - d1) a22 + a12 (c2 xs + d2)) inv,  zs = (a11 (-c2 xs - d2) + (c1 xs + d1) a21) inv
        const float ys1 = (a12 * c2 - c1 * a22) * inv, ys0 = (a12 * d2 - d1 * a22) * inv;
        const float zs1 = (c1 * a21 - a11 * c2) * inv, zs0 = (d1 * a21 - a11 * d2) * inv;
        // xs = x0 + ix dx;  index = (pos - origin) / step
        by = ys1 * gr.dx * idy; ay = (ys0 + ys1 * gr.x0 - gr.y0) * idy;
        bz = zs1 * gr.dx * idz; az = (zs0 + zs1 * gr.x0 - gr.z0) * idz;
    };
    float cAy, cBy, cAz, cBz, uAy, uBy, uAz, uBz, vAy, vBy, vAz, vBz;
    affine(ut, vt, cAy, cBy, cAz, cBz);
    affine(ut + su, vt, uAy, uBy, uAz, uBz);
    affine(ut, vt + sv, vAy, vBy, vAz, vBz);
    const float pd_per_x = (float)(g.D - 1) / g.depth_span;  // plane index per metre of depth
    const T *gb = gout + (size_t)b * N * CT;  // (both layouts: a sample is N * (C + Cs) elements)
    float asem[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) asem[c] = 0.0f;
    const int d0 = chunk * F2G_DCH, d1 = min(g.D, d0 + F2G_DCH);
    for (int d = d0; d < d1; ++d) {
        float ast[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) ast[c] = 0.0f;
        // x slabs whose plane position lies in (d - 1, d + 1): uniform for the workgroup
        const float xlo = g.depth_min + ((float)d - 1.0f) / pd_per_x, xhi = g.depth_min + ((float)d + 1.0f) / pd_per_x;
        const float fa = (xlo - gr.x0) * idx, fb = (xhi - gr.x0) * idx;
        const int ixa = max(0, (int)ceilf(fminf(fa, fb) - 0.02f)), ixb = min(g.Nx - 1, (int)floorf(fmaxf(fa, fb) + 0.02f));
        for (int ix = ixa; ix <= ixb; ++ix) {
            const float fx = (float)ix;
            const float iyf = __builtin_fmaf(cBy, fx, cAy), izf = __builtin_fmaf(cBz, fx, cAz);
            const float ty = (fabsf(__builtin_fmaf(uBy, fx, uAy) - iyf) + fabsf(__builtin_fmaf(vBy, fx, vAy) - iyf)) * 1.15f + 0.05f;
            const float tz = (fabsf(__builtin_fmaf(uBz, fx, uAz) - izf) + fabsf(__builtin_fmaf(vBz, fx, vAz) - izf)) * 1.15f + 0.05f;
            const float y0f = ceilf(iyf - ty), y1f = floorf(iyf + ty), z0f = ceilf(izf - tz), z1f = floorf(izf + tz);
            // (non-finite solutions compare false.)  The box is walked in FULL whatever its size, clamped to the
            // grid in fp32 before the int conversion: a coarser cost volume, finer voxels or a long depth range
            // make a cost-volume pixel span many voxels, and the former cut at 8 x 8 / t < 4 dropped those
            // contributions silently.  Larger boxes only cost more iterations.
            const bool some = inside && y0f <= y1f && z0f <= z1f && y1f >= 0.0f && z1f >= 0.0f &&
                              y0f <= (float)(g.Ny - 1) && z0f <= (float)(g.Nz - 1);
            if (!__any(some)) continue;
            const int iy0 = some ? (int)fmaxf(y0f, 0.0f) : 0, iy1 = some ? (int)fminf(y1f, (float)(g.Ny - 1)) : -1;
            const int iz0 = some ? (int)fmaxf(z0f, 0.0f) : 0, iz1 = some ? (int)fminf(z1f, (float)(g.Nz - 1)) : -1;
            // one candidate voxel (ix, iy, iz): its packed lower-corner cell against this lane's (w, h, d) -- a 4-byte
            // load and three subtractions reject it (round 5 re-ran the forward's projection for every candidate: three
            // dependent loads, three dot products and two divisions before the first test)
            auto visit = [&](int iy, int iz) {
                const long long i = ((long long)iz * g.Ny + iy) * g.Nx + ix;
                const uint32_t cc = cell[(size_t)b * N + i];
                if (cc == F2G_NONE) return;
                const int kx = w - ((int)(cc & 0x7ffu) - 1), ky = h - ((int)((cc >> 11) & 0x3ffu) - 1);
                const int kz = d - ((int)(cc >> 21) - 1);
                if ((unsigned)kx > 1u || (unsigned)ky > 1u) return;
                const bool zhit = (unsigned)kz <= 1u;
                if (!zhit && !(SEM && kz == 0)) return;
                const float4 pp = pos[(size_t)b * N + i];
                const float px = pp.x, py = pp.y, pz = pp.z, sf = pp.w;
                const float mf = SEM ? mfac[(size_t)b * N + i] : -1.0f;
                // make_tri's weights, corner by corner (the forward's expressions on the forward's values)
                const float x0 = floorf(px), y0 = floorf(py), z0 = floorf(pz);
                const float x1 = x0 + 1.0f, y1 = y0 + 1.0f, z1 = z0 + 1.0f;
                const float wx = kx ? px - x0 : x1 - px, wy = ky ? py - y0 : y1 - py;
                const T *gp = gb + (size_t)i * gvs;
                if (zhit && sf >= 0.0f) {
                    const float wgt = ((wx * wy) * (kz ? pz - z0 : z1 - pz)) * sf;
                    float vv[8];
                    if (gcs == 1) {
                        gather_row8<T>(gp + cq, vv);
                    } else {
#pragma unroll
                        for (int cc2 = 0; cc2 < 8; ++cc2) vv[cc2] = elem<T>::load(gp[(size_t)(cq + cc2) * gcs]);
                    }
#pragma unroll
                    for (int cc2 = 0; cc2 < 8; ++cc2) ast[cc2] += vv[cc2] * wgt;
                }
                if constexpr (SEM) {
                    // the semantic map's pixel (h, w): once per voxel, from the hit on its lower depth corner
                    // (a valid voxel's lower corner is inside the volume); make_tri(gx, gy, 0, 1, H, W): z1 - iz = 1
                    if (kz == 0 && mf >= 0.0f) {
                        const float mw = ((wx * wy) * 1.0f) * mf;
                        float vv[8];
                        if (gcs == 1) {
                            gather_row8<T>(gp + 32 + cq, vv);
                        } else {
#pragma unroll
                            for (int cc2 = 0; cc2 < 8; ++cc2) vv[cc2] = elem<T>::load(gp[(size_t)(32 + cq + cc2) * gcs]);
                        }
#pragma unroll
                        for (int cc2 = 0; cc2 < 8; ++cc2) asem[cc2] += vv[cc2] * mw;
                    }
                }
            };
            // boxes of up to 8 x 8 voxels -- what the path's grids produce -- take the counted loops; a wave that
            // holds a larger box walks it in full (uniform choice)
            const bool small_box = !__any(some && (iy1 - iy0 > 7 || iz1 - iz0 > 7));
            if (small_box) {
                for (int jz = 0; jz < 8; ++jz) {
                    const int iz = iz0 + jz;
                    if (!__any(iz <= iz1)) break;
                    for (int jy = 0; jy < 8; ++jy) {
                        const int iy = iy0 + jy;
                        const bool cand = iz <= iz1 && iy <= iy1;
                        if (!__any(cand)) break;
                        if (cand) visit(iy, iz);
                    }
                }
            } else {
                for (int jz = 0;; ++jz) {
                    const int iz = iz0 + jz;
                    if (!__any(iz <= iz1)) break;
                    for (int jy = 0;; ++jy) {
                        const int iy = iy0 + jy;
                        const bool cand = iz <= iz1 && iy <= iy1;
                        if (!__any(cand)) break;
                        if (cand) visit(iy, iz);
                    }
                }
            }
        }
        if (inside) {
            if constexpr (GCL) {
                constexpr int VEC = dfm::vec16<T>::N;
                T *o = (T *)gstv + ((((size_t)b * g.D + d) * g.H + h) * g.W + w) * 32 + cq;
#pragma unroll
                for (int q = 0; q < 8 / VEC; ++q) {
                    float r[VEC];
#pragma unroll
                    for (int e = 0; e < VEC; ++e) r[e] = ast[q * VEC + e];
                    dfm::store16<T>(o + q * VEC, r);
                }
            } else {
                float *o = (float *)gstv + ((size_t)b * g.C * g.D + d) * g.H * g.W + (size_t)h * g.W + w;
                const size_t cs = (size_t)g.D * g.H * g.W;
#pragma unroll
                for (int c = 0; c < 8; ++c) o[(size_t)(cq + c) * cs] = ast[c];
            }
        }
    }
    if constexpr (SEM) {
        if (inside) {
            float *o = gsem + (size_t)b * g.Cs * g.Hsem * g.Wsem + (size_t)h * g.Wsem + w;
            const size_t cs = (size_t)g.Hsem * g.Wsem;
#pragma unroll
            for (int c = 0; c < 8; ++c)
                if (asem[c] != 0.0f) atomicAdd(o + (size_t)(cq + c) * cs, asem[c]);
        }
    }
}

}  // namespace

extern "C" DFM_API size_t dfm_frustum_to_voxel_bwd_workspace_bytes(const dfm_f2v_desc *d)
{
    if (!d || d->batch <= 0 || d->channels <= 0 || d->d <= 0 || d->h <= 0 || d->w <= 0 ||
        d->sem_channels < 0)
        return 0;
    return f2v_pm_layout(d, sizeof(float)).total();
}

static int f2v_bwd_impl(const dfm_f2v_desc *d, const void *grad_out, const void *softmax, FusedHead fh,
                        int head_scale, const float *coords, const float *cam2img, float *grad_stereo,
                        float *grad_sem, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!d) return set_error(DFM_ERR_INVALID_ARG, "desc is NULL");
    if (int rc = check_dtype(d->dtype)) return rc;
    if (!grad_out || !coords || !cam2img || !grad_stereo || (d->sem_channels > 0 && !grad_sem) ||
        ((d->stereo_atten || (d->sem_channels > 0 && !d->no_sem_atten)) && !softmax && !fh.cost))
        return set_error(DFM_ERR_INVALID_ARG, "NULL device pointer");
    F2vGeom g;
    if (const int rc = f2v_geom(d, fh, head_scale, &g)) return rc;
    const long long N = (long long)d->nz * d->ny * d->nx;
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = (size_t)(d->channels + d->sem_channels) * (F2V_VT + 1) * sizeof(float) +
                       F2V_VT * sizeof(BwdFoot);
    if (workspace && lds <= 64 * 1024 && d->batch <= 65535) {
        // pixel-major accumulation (see f2v_bwd_pm_kernel)
        if (workspace_bytes < dfm_frustum_to_voxel_bwd_workspace_bytes(d))
            return set_error(DFM_ERR_WORKSPACE,
                             "workspace smaller than dfm_frustum_to_voxel_bwd_workspace_bytes");
        const long long vox = (long long)d->d * d->h * d->w, pix = (long long)d->hsem * d->wsem;
        const F2vPmLayout ws = f2v_pm_layout(d, sizeof(float));
        float *gst_pm = (float *)workspace, *gsem_pm = (float *)((char *)workspace + ws.first);
        HIP_TRY(hipMemsetAsync(workspace, 0, ws.first + ws.second, st));
        const dim3 grid((unsigned)((N + F2V_VT - 1) / F2V_VT), d->batch);
        by_dtype(d->dtype, [&](auto t) {
            using T = decltype(t);
            hipLaunchKernelGGL(f2v_bwd_pm_kernel<T>, grid, dim3(256), lds, st, g, (const T *)grad_out,
                               (const T *)softmax, fh, coords, cam2img, gst_pm, gsem_pm);
        });
        dim3 t1((unsigned)((vox + 63) / 64), (d->channels + 31) / 32, d->batch);
        hipLaunchKernelGGL(add_from_pixel_major_kernel<float>, t1, dim3(256), 0, st, gst_pm, grad_stereo,
                           d->channels, vox);
        if (d->sem_channels > 0) {
            dim3 t2((unsigned)((pix + 63) / 64), (d->sem_channels + 31) / 32, d->batch);
            hipLaunchKernelGGL(add_from_pixel_major_kernel<float>, t2, dim3(256), 0, st, gsem_pm, grad_sem,
                               d->sem_channels, pix);
        }
        HIP_TRY(hipGetLastError());
        return DFM_OK;
    }
    // no workspace (or more channels than the LDS tile holds): lane-per-voxel scatter
    const dim3 grid((unsigned)((N + 255) / 256), d->batch);
    by_dtype(d->dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(f2v_bwd_kernel<T>, grid, dim3(256), 0, st, g, (const T *)grad_out, (const T *)softmax, fh,
                           coords, cam2img, grad_stereo, grad_sem);
    });
    HIP_TRY(hipGetLastError());
    return DFM_OK;
}

extern "C" DFM_API int dfm_frustum_to_voxel_bwd(const dfm_f2v_desc *d, const void *grad_out,
                                                const void *softmax, const float *coords,
                                                const float *cam2img, float *grad_stereo,
                                                float *grad_sem, void *workspace,
                                                size_t workspace_bytes, void *stream)
{
    return f2v_bwd_impl(d, grad_out, softmax, FusedHead{nullptr, nullptr, nullptr}, 0, coords, cam2img, grad_stereo,
                        grad_sem, workspace, workspace_bytes, stream);
}

extern "C" DFM_API int dfm_frustum_to_voxel_fused_bwd(const dfm_f2v_desc *d, const void *grad_out, const void *cost,
                                                      const float *col_max, const float *col_sum,
                                                      int32_t head_scale, const float *coords,
                                                      const float *cam2img, float *grad_stereo, float *grad_sem,
                                                      void *workspace, size_t workspace_bytes, void *stream)
{
    if (!cost || !col_max || !col_sum) return set_error(DFM_ERR_INVALID_ARG, "NULL device pointer");
    return f2v_bwd_impl(d, grad_out, nullptr, FusedHead{cost, col_max, col_sum}, head_scale, coords, cam2img,
                        grad_stereo, grad_sem, workspace, workspace_bytes, stream);
}

// The gather form of the backward (f2v_bwd_gather_kernel).  grid6 (HOST memory): {x0, dx, y0, dy, z0, dz} of the
// regular voxel grid `coords` is (the caller has checked it: coords[(iz * Ny + iy) * Nx + ix] == origin + index *
// step).  grad_stereo is OVERWRITTEN (reference layout, fp32); grad_sem zero-filled by the caller, accumulated.
// workspace: >= dfm_frustum_to_voxel_bwd_gather_workspace_bytes (24 bytes per voxel), 16-byte aligned.  DFM_ERR_UNSUPPORTED unless
// C == 32, Cs in {0, 32} with the semantic map at the cost volume's resolution and sem_atten (a voxel outside
// the depth range then contributes nothing and every contributing voxel has a cell), and non-zero grid steps.
extern "C" DFM_API size_t dfm_frustum_to_voxel_bwd_gather_workspace_bytes(const dfm_f2v_desc *d)
{
    if (!d || d->batch <= 0 || d->nz <= 0 || d->ny <= 0 || d->nx <= 0) return 0;
    // per voxel: its position and stereo factor (16 bytes), its packed cell (4), its semantic factor (4)
    return (((size_t)d->batch * d->nz * d->ny * d->nx * 24) + 255) & ~(size_t)255;
}

static int f2v_bwd_gather_impl(const dfm_f2v_desc *d, const void *grad_out, const void *softmax, const void *cost,
                               const float *col_max, const float *col_sum, int32_t head_scale, const float *coords,
                               const float *grid6, const float *cam2img, void *grad_stereo, bool grad_cl,
                               float *grad_sem, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!d) return set_error(DFM_ERR_INVALID_ARG, "desc is NULL");
    if (int rc = check_dtype(d->dtype)) return rc;
    if (!grad_out || !coords || !grid6 || !cam2img || !grad_stereo || !workspace || (d->sem_channels > 0 && !grad_sem))
        return set_error(DFM_ERR_INVALID_ARG, "NULL pointer");
    const bool need_disp = d->stereo_atten || (d->sem_channels > 0 && !d->no_sem_atten);
    if (need_disp && !softmax && !cost) return set_error(DFM_ERR_INVALID_ARG, "the attended branches need the depth distribution");
    if (cost && (!col_max || !col_sum)) return set_error(DFM_ERR_INVALID_ARG, "NULL device pointer");
    if (d->channels != 32 || !(d->sem_channels == 0 || (d->sem_channels == 32 && d->hsem == d->h && d->wsem == d->w &&
                                                          !d->no_sem_atten)) ||
        d->d < 2 || d->h < 2 || d->w < 2 || grid6[1] == 0.0f || grid6[3] == 0.0f || grid6[5] == 0.0f ||
        d->batch > 65535 || (d->out_channels_last && ((uintptr_t)grad_out & 15)) ||
        (grad_cl && ((uintptr_t)grad_stereo & 15)) || d->w > 2044 || d->h > 1020 || d->d > 1020 ||
        ((uintptr_t)workspace & 15))
        return set_error(DFM_ERR_UNSUPPORTED,
                         "gather backward: C == 32, Cs in {0, 32} at the cost volume's resolution with sem_atten, regular grid");
    if (workspace_bytes < dfm_frustum_to_voxel_bwd_gather_workspace_bytes(d))
        return set_error(DFM_ERR_WORKSPACE, "workspace smaller than dfm_frustum_to_voxel_bwd_gather_workspace_bytes");
    F2vGeom g;
    const FusedHead fh = cost ? FusedHead{cost, col_max, col_sum} : FusedHead{nullptr, nullptr, nullptr};
    if (const int rc = f2v_geom(d, fh, head_scale, &g)) return rc;
    const F2vGrid gr{grid6[0], grid6[1], grid6[2], grid6[3], grid6[4], grid6[5]};
    const long long N = (long long)d->nz * d->ny * d->nx;
    hipStream_t st = (hipStream_t)stream;
    float4 *pos = (float4 *)workspace;
    uint32_t *cell = (uint32_t *)(pos + (size_t)d->batch * N);
    float *mfac = (float *)(cell + (size_t)d->batch * N);
    const dim3 pgrid((unsigned)((N + 255) / 256), d->batch);
    const int CT = d->channels + d->sem_channels;
    const size_t gvs = g.out_cl ? (size_t)CT : 1, gcs = g.out_cl ? 1 : (size_t)N;
    const int dchunks = (d->d + F2G_DCH - 1) / F2G_DCH;
    const dim3 ggrid((unsigned)(((d->w + 15) / 16) * ((d->h + 3) / 4) * dchunks), d->batch);
    by_dtype(d->dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(f2v_bwd_prep_kernel<T>, pgrid, dim3(256), 0, st, g, (const T *)softmax, fh, coords, cam2img,
                           (float *)nullptr, mfac, cell, pos);
        by_bool(d->sem_channels > 0, [&](auto sem) {
            by_bool(grad_cl, [&](auto gcl) {
                hipLaunchKernelGGL((f2v_bwd_gather_kernel<T, decltype(sem)::value, decltype(gcl)::value>), ggrid,
                                   dim3(256), 0, st, g, gr, dchunks, (const T *)grad_out, gvs, gcs, coords, cam2img,
                                   (const uint32_t *)cell, (const float4 *)pos, (const float *)mfac, grad_stereo,
                                   grad_sem);
            });
        });
    });
    HIP_TRY(hipGetLastError());
    return DFM_OK;
}

extern "C" DFM_API int dfm_frustum_to_voxel_bwd_gather(const dfm_f2v_desc *d, const void *grad_out, const void *softmax,
                                                       const void *cost, const float *col_max, const float *col_sum,
                                                       int32_t head_scale, const float *coords, const float *grid6,
                                                       const float *cam2img, float *grad_stereo, float *grad_sem,
                                                       void *workspace, size_t workspace_bytes, void *stream)
{
    return f2v_bwd_gather_impl(d, grad_out, softmax, cost, col_max, col_sum, head_scale, coords, grid6, cam2img,
                               grad_stereo, false, grad_sem, workspace, workspace_bytes, stream);
}

// The same, with the stereo gradient in the layout and type of a channels-last cost volume: grad_stereo is
// (B, d, h, w, C) in memory (torch channels_last_3d of (B, C, d, h, w)), desc->dtype, 16-byte aligned, OVERWRITTEN
// -- the fp32 sums rounded once at the store, the bits `dfm_frustum_to_voxel_bwd_gather` + a conversion give.  What
// the NDHWC stack's autograd wants: the engine adds this gradient to the one the prediction convolution's backward
// hands over in that layout (a planar fp32 result cost a zero fill, a conversion and a strided addition: 0.6 ms of
// a 22.5 ms training step).  grad_sem as above (fp32, planar, accumulated).
extern "C" DFM_API int dfm_frustum_to_voxel_bwd_gather_cl(const dfm_f2v_desc *d, const void *grad_out,
                                                          const void *softmax, const void *cost, const float *col_max,
                                                          const float *col_sum, int32_t head_scale, const float *coords,
                                                          const float *grid6, const float *cam2img, void *grad_stereo,
                                                          float *grad_sem, void *workspace, size_t workspace_bytes,
                                                          void *stream)
{
    return f2v_bwd_gather_impl(d, grad_out, softmax, cost, col_max, col_sum, head_scale, coords, grid6, cam2img,
                               grad_stereo, true, grad_sem, workspace, workspace_bytes, stream);
}
