// frustum_to_voxel.hip -- sampling stage of FrustumToVoxel.forward (gfx950)
//
// Reference: mmdet3d/models/necks/feature_transformation.py:82-158 -- per voxel
// project with cam2img[:3], normalise (u, v, depth), three 3-D grid_samples
// (cost volume, depth distribution, 2-D semantic feature at z := 0), validity
// masks, depth-probability weighting, channel concat.  One launch writes the
// concatenated (B, C+Cs, Nz, Ny, Nx) volume: no coordinate tensors, no three
// separate sampled volumes, no mask multiplies, no cat.
//
// The per-voxel arithmetic (projection, validity, depth probability, trilinear corners) is f2v_common.h's,
// shared with the backward (frustum_to_voxel_bwd.hip); the inverse op is voxel_sample.hip.
//
// Layout: caller tensors are NCDHW / NCHW.  stereo_feat and cur_sem_feats are first
// re-laid pixel-major into the workspace ([d][h][w][C], [h][w][Cs]: a corner is one
// contiguous run of C*sizeof(T) bytes read with 16-byte loads -- in NCDHW the C scalar
// loads of a corner sit a whole volume apart and neighbouring voxels along x walk
// through depth planes, so every load touched its own cache line); the 1-channel
// depth distribution is sampled where it lies.  Shapes whose channel counts are not a
// whole number of 16-byte blocks take the scalar kernel on the caller's layout.
// Bound: HBM write of the volume + one read of the sources.
#include "f2v_common.h"

namespace {

// pred_disp * valids (feature_transformation.py:133-139); 1 when neither attention wants it.  The forward's
// gating: the materialised distribution is sampled for EVERY voxel, as the reference does (a NaN sampled
// outside the frustum times 0 stays a NaN); only the fused head skips the evaluation there (nothing to
// evaluate outside the frustum: the unfused product is +0 there as well).
template <typename T>
__device__ __forceinline__ float f2v_fwd_disp(const F2vGeom &g, const T *__restrict__ soft, const FusedHead &fh,
                                              int b, const F2vVoxel &p)
{
    const float valid = p.valid ? 1.0f : 0.0f;
    float disp = 1.0f;
    if (f2v_wants_disp(g)) {
        if (fh.cost) disp = valid != 0.0f ? pred_disp<T>(g, soft, fh, b, p.gx, p.gy, p.gz) * valid : 0.0f;
        else disp = pred_disp<T>(g, soft, fh, b, p.gx, p.gy, p.gz) * valid;
    }
    return disp;
}

template <typename T>
__global__ __launch_bounds__(256) void f2v_kernel(F2vGeom g, const T *__restrict__ stereo,
                                                  const T *__restrict__ soft,
                                                  const T *__restrict__ sem,
                                                  const float *__restrict__ coords,
                                                  const float *__restrict__ cam2img,
                                                  T *__restrict__ out, FusedHead fh)
{
    const long long N = (long long)g.Nz * g.Ny * g.Nx;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y;
    if (i >= N) return;
    const F2vVoxel p = f2v_project(g, coords, cam2img, b, i);
    const float gx = p.gx, gy = p.gy, gz = p.gz;
    const bool valid2d = p.valid2d;
    const float valid = p.valid ? 1.0f : 0.0f;
    const float disp = f2v_fwd_disp<T>(g, soft, fh, b, p);
    const float sdisp = g.st_att ? disp : 1.0f;   // x * 1.0f is exact: one code path
    const float mdisp = g.sem_att ? disp : 1.0f;
    const size_t vol = (size_t)g.D * g.H * g.W;
    T *o = out + (size_t)b * (g.C + g.Cs) * N + i;
    {
        const Tri t = make_tri(gx, gy, gz, g.D, g.H, g.W);
        const T *sv = stereo + (size_t)b * g.C * vol;
        for (int ch = 0; ch < g.C; ++ch)
            o[(size_t)ch * N] = elem<T>::store(tri_sample<T>(t, sv + ch * vol) * valid * sdisp);
    }
    if (g.Cs > 0) {
        const Tri t2 = make_tri(gx, gy, 0.0f, 1, g.Hsem, g.Wsem);
        const float v2d = valid2d ? 1.0f : 0.0f;
        const size_t plane = (size_t)g.Hsem * g.Wsem;
        const T *sp = sem + (size_t)b * g.Cs * plane;
        for (int ch = 0; ch < g.Cs; ++ch) {
            float s = tri_sample<T>(t2, sp + ch * plane);
            s = s * v2d;
            o[(size_t)(g.C + ch) * N] = elem<T>::store(s * mdisp);
        }
    }
}

// pixel-major sources: stereo_pm [b][d*h*w][C], sem_pm [b][hsem*wsem][Cs] (16-byte blocks)
// 32 channels per pass; per channel the corners are added in ATen's order.
template <typename T>
__global__ __launch_bounds__(256) void f2v_pm_kernel(F2vGeom g, const uint4 *__restrict__ stereo_pm,
                                                     const T *__restrict__ soft,
                                                     const uint4 *__restrict__ sem_pm,
                                                     const float *__restrict__ coords,
                                                     const float *__restrict__ cam2img,
                                                     T *__restrict__ out, FusedHead fh)
{
    constexpr int CB = elem<T>::CB;
    constexpr int NB = 32 / CB;
    const long long N = (long long)g.Nz * g.Ny * g.Nx;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y;
    if (i >= N) return;
    const F2vVoxel p = f2v_project(g, coords, cam2img, b, i);
    const float gx = p.gx, gy = p.gy, gz = p.gz;
    const bool valid2d = p.valid2d;
    const float valid = p.valid ? 1.0f : 0.0f;
    const float disp = f2v_fwd_disp<T>(g, soft, fh, b, p);
    const float sdisp = g.st_att ? disp : 1.0f;   // x * 1.0f is exact: one code path
    const float mdisp = g.sem_att ? disp : 1.0f;
    T *o = out + (size_t)b * (g.C + g.Cs) * N + i;
    T *ocl = out + ((size_t)b * N + i) * (g.C + g.Cs);  // channels-last: this voxel's C + Cs values
    {
        const Tri t = make_tri(gx, gy, gz, g.D, g.H, g.W);
        const int nblk = g.C / CB;
        const uint4 *sv = stereo_pm + (size_t)b * g.D * g.H * g.W * nblk;
        for (int blk0 = 0; blk0 < nblk; blk0 += NB) {
            float acc[NB][CB];
#pragma unroll
            for (int j = 0; j < NB; ++j)
#pragma unroll
                for (int k = 0; k < CB; ++k) acc[j][k] = 0.0f;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                if (!(t.ok & (1u << k))) continue;
                const uint4 *p = sv + (size_t)t.o[k] * nblk + blk0;
#pragma unroll
                for (int j = 0; j < NB; ++j) {
                    if (blk0 + j < nblk) {
                        float r[CB];
                        unpack16(p[j], r);
#pragma unroll
                        for (int e = 0; e < CB; ++e) acc[j][e] = acc[j][e] + r[e] * t.w[k];
                    }
                }
            }
            if (g.out_cl) {
#pragma unroll
                for (int j = 0; j < NB; ++j)
                    if (blk0 + j < nblk) {
                        float r[CB];
#pragma unroll
                        for (int e = 0; e < CB; ++e) r[e] = acc[j][e] * valid * sdisp;
                        lift_store16<T>(ocl + (size_t)(blk0 + j) * CB, r);
                    }
            } else {
#pragma unroll
                for (int j = 0; j < NB; ++j)
#pragma unroll
                    for (int e = 0; e < CB; ++e)
                        if (blk0 + j < nblk)
                            o[(size_t)((blk0 + j) * CB + e) * N] = elem<T>::store(acc[j][e] * valid * sdisp);
            }
        }
    }
    if (g.Cs > 0) {
        const Tri t2 = make_tri(gx, gy, 0.0f, 1, g.Hsem, g.Wsem);
        const float v2d = valid2d ? 1.0f : 0.0f;
        const int nblk = g.Cs / CB;
        const uint4 *sp = sem_pm + (size_t)b * g.Hsem * g.Wsem * nblk;
        for (int blk0 = 0; blk0 < nblk; blk0 += NB) {
            float acc[NB][CB];
#pragma unroll
            for (int j = 0; j < NB; ++j)
#pragma unroll
                for (int k = 0; k < CB; ++k) acc[j][k] = 0.0f;
#pragma unroll
            for (int k = 0; k < 4; ++k) {  // D == 1: the z1 corners are never in bounds
                if (!(t2.ok & (1u << k))) continue;
                const uint4 *p = sp + (size_t)t2.o[k] * nblk + blk0;
#pragma unroll
                for (int j = 0; j < NB; ++j) {
                    if (blk0 + j < nblk) {
                        float r[CB];
                        unpack16(p[j], r);
#pragma unroll
                        for (int e = 0; e < CB; ++e) acc[j][e] = acc[j][e] + r[e] * t2.w[k];
                    }
                }
            }
            if (g.out_cl) {
#pragma unroll
                for (int j = 0; j < NB; ++j)
                    if (blk0 + j < nblk) {
                        float r[CB];
#pragma unroll
                        for (int e = 0; e < CB; ++e) {
                            const float sval = acc[j][e] * v2d;
                            r[e] = sval * mdisp;
                        }
                        lift_store16<T>(ocl + g.C + (size_t)(blk0 + j) * CB, r);
                    }
            } else {
#pragma unroll
                for (int j = 0; j < NB; ++j)
#pragma unroll
                    for (int e = 0; e < CB; ++e)
                        if (blk0 + j < nblk) {
                            float sval = acc[j][e] * v2d;
                            o[(size_t)(g.C + (blk0 + j) * CB + e) * N] = elem<T>::store(sval * mdisp);
                        }
            }
        }
    }
}

// Channels-last output, several lanes per voxel.  f2v_pm_kernel is one lane = one voxel: a tap is 64-128
// contiguous bytes per LANE, so the 64 lanes of every load touch 64 different cache lines, and a voxel's
// channels-last row leaves as 16-byte pieces 128-256 bytes apart.  Here the geometry (corner offsets, weights,
// masks, the depth probability) is computed lane = voxel as before and parked in LDS (128 bytes per voxel);
// then each source in turn (stereo feature: 8 corners, semantic feature: 4) is gathered with lane = (voxel,
// 16-byte channel block of the source): a tap is ONE coalesced 16-byte load per lane -- the 4 or 8 lanes of a
// voxel cover the corner's contiguous channels --, two voxels per lane are in flight (16 / 8 independent taps),
// and a voxel's half of the row leaves as whole 64-byte runs of neighbouring voxels (non-temporal: nothing
// re-reads it here).  Same arithmetic, corner by corner in ATen's order.  f2v_cl (config K, bf16): 1.93 ->
// 1.35 ms (profiles/archive/r04_c51_*); a first version with both sources in one pass (lanes 0-3 stereo, 4-7
// semantic: divergent halves, one voxel per lane in flight) measured 2.57 ms (r04_c50).  PLANAR: the
// reference layout (B, C + Cs, Nz, Ny, Nx) from the same gather (gather_planar below): f2v fp32 3.86 ->
// 2.93 ms (r04_c59).
template <typename T, bool PLANAR>
__global__ __launch_bounds__(256) void f2v_pm8_kernel(F2vGeom g, const uint4 *__restrict__ stereo_pm,
                                                      const T *__restrict__ soft, const uint4 *__restrict__ sem_pm,
                                                      const float *__restrict__ coords,
                                                      const float *__restrict__ cam2img, T *__restrict__ out,
                                                      FusedHead fh)
{
    constexpr int CB = elem<T>::CB;
    struct Rec {
        int o[8];
        float w[8];
        int o2[4];
        float w2[4];
        float valid, sdisp, v2d, mdisp;
        uint32_t ok, ok2, pad0, pad1;
    };
    static_assert(sizeof(Rec) == 128, "one record = 128 bytes");
    __shared__ __attribute__((aligned(16))) Rec rec[256];
    const long long N = (long long)g.Nz * g.Ny * g.Nx;
    const long long i0 = (long long)blockIdx.x * 256;
    const int b = blockIdx.y;
    {
        const long long i = min(i0 + threadIdx.x, N - 1);
        const F2vVoxel p = f2v_project(g, coords, cam2img, b, i);
        const float gx = p.gx, gy = p.gy, gz = p.gz;
        const bool valid2d = p.valid2d;
        const float valid = p.valid ? 1.0f : 0.0f;
        const float disp = f2v_fwd_disp<T>(g, soft, fh, b, p);
        Rec r;
        const Tri t = make_tri(gx, gy, gz, g.D, g.H, g.W);
#pragma unroll
        for (int k = 0; k < 8; ++k) { r.o[k] = t.o[k]; r.w[k] = t.w[k]; }
        r.ok = t.ok;
        r.ok2 = 0u;
#pragma unroll
        for (int k = 0; k < 4; ++k) { r.o2[k] = 0; r.w2[k] = 0.0f; }
        if (g.Cs > 0) {
            const Tri t2 = make_tri(gx, gy, 0.0f, 1, g.Hsem, g.Wsem);
#pragma unroll
            for (int k = 0; k < 4; ++k) { r.o2[k] = t2.o[k]; r.w2[k] = t2.w[k]; }
            r.ok2 = t2.ok & 15u;  // D == 1: the z1 corners are never in bounds
        }
        r.valid = valid;
        r.sdisp = g.st_att ? disp : 1.0f;  // x * 1.0f is exact: one code path
        r.v2d = valid2d ? 1.0f : 0.0f;
        r.mdisp = g.sem_att ? disp : 1.0f;
        r.pad0 = r.pad1 = 0u;
        rec[threadIdx.x] = r;
    }
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int nbs = g.C / CB, nbm = g.Cs / CB, nbt = nbs + nbm;
    const uint4 *sv = stereo_pm + (size_t)b * g.D * g.H * g.W * nbs;
    const uint4 *sp = sem_pm + (size_t)b * g.Hsem * g.Wsem * nbm;
    typedef uint32_t f2v_u32x4 __attribute__((ext_vector_type(4)));
    // One source at a time (all lanes run the same corners), L lanes per voxel (L = 4 or 8 blocks of the
    // source per trip), TWO voxels per lane in flight: 16 (stereo) / 8 (semantic) independent taps per lane.
    auto gather = [&](auto stereo_c, const uint4 *src, int nb, int bi0, int L) {
        constexpr bool ST = decltype(stereo_c)::value;
        constexpr int NK = ST ? 8 : 4;
        const int sh = L == 4 ? 2 : 3, vpi = 64 >> sh;  // voxels per trip
        const int j = lane & (L - 1), vp = lane >> sh;
        for (int bb = j; bb < nb; bb += L) {
            for (int v0 = 0; v0 < 64; v0 += 2 * vpi) {
                float acc[2][CB];
                int qq[2];
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    qq[u] = wave * 64 + v0 + u * vpi + vp;
#pragma unroll
                    for (int e = 0; e < CB; ++e) acc[u][e] = 0.0f;
                }
                uint4 tapv[2][NK];
                uint32_t okv[2];
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const Rec &r = rec[qq[u]];
                    okv[u] = ST ? r.ok : r.ok2;
#pragma unroll
                    for (int k = 0; k < NK; ++k) {
                        // (an out-of-bounds corner's offset is 0: addressable, never used)
                        const int o = ST ? r.o[k] : r.o2[k];
                        tapv[u][k] = src[(size_t)o * nb + bb];
                    }
                }
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const Rec &r = rec[qq[u]];
#pragma unroll
                    for (int k = 0; k < NK; ++k) {
                        if (!(okv[u] & (1u << k))) continue;
                        float v[CB];
                        unpack16(tapv[u][k], v);
                        const float w = ST ? r.w[k] : r.w2[k];
#pragma unroll
                        for (int e = 0; e < CB; ++e) acc[u][e] = acc[u][e] + v[e] * w;
                    }
                    float res[CB];
                    if constexpr (ST) {
                        const float va = r.valid, sd = r.sdisp;
#pragma unroll
                        for (int e = 0; e < CB; ++e) res[e] = acc[u][e] * va * sd;
                    } else {
                        const float v2 = r.v2d, md = r.mdisp;
#pragma unroll
                        for (int e = 0; e < CB; ++e) {
                            const float sval = acc[u][e] * v2;
                            res[e] = sval * md;
                        }
                    }
                    const long long i = i0 + qq[u];
                    if (i < N) {
                        f2v_u32x4 pk;
                        if constexpr (sizeof(T) == 4) {
                            pk = f2v_u32x4{__float_as_uint(res[0]), __float_as_uint(res[1]), __float_as_uint(res[2]),
                                           __float_as_uint(res[3])};
                        } else {
                            pk = f2v_u32x4{dfm::pack_bf16x2(res[0], res[1]), dfm::pack_bf16x2(res[2], res[3]),
                                           dfm::pack_bf16x2(res[4], res[5]), dfm::pack_bf16x2(res[6], res[7])};
                        }
                        T *dst = out + ((size_t)b * N + i) * (g.C + g.Cs) + (size_t)(bi0 + bb) * CB;
                        __builtin_nontemporal_store(pk, (f2v_u32x4 *)dst);
                    }
                }
            }
        }
    };
    // Planar output (B, C + Cs, Nz, Ny, Nx), the reference layout: the same gather, but a lane keeps ONE channel
    // block for FOUR CONSECUTIVE voxels (four trips, two voxels in flight) and stores, per channel, one vector
    // of those four voxels -- the lanes of a store instruction that share a channel are 8 (fp32) / 16 (bf16)
    // neighbouring voxel groups: whole 128-byte lines per channel plane, no transpose through LDS.
    auto gather_planar = [&](auto stereo_c, const uint4 *src, int nb, int ch0, int L) {
        constexpr bool ST = decltype(stereo_c)::value;
        constexpr int NK = ST ? 8 : 4;
        const int sh = L == 4 ? 2 : 3, ngr = 64 >> sh;  // voxel groups per round
        const int j = lane & (L - 1), vg = lane >> sh;
        for (int bb = j; bb < nb; bb += L) {
            for (int v0 = 0; v0 < 64; v0 += 4 * ngr) {
                const int qb = wave * 64 + v0 + 4 * vg;  // this lane's four voxels: qb .. qb + 3
                float res[4][CB];
#pragma unroll
                for (int t0 = 0; t0 < 4; t0 += 2) {
                    uint4 tapv[2][NK];
                    uint32_t okv[2];
#pragma unroll
                    for (int u = 0; u < 2; ++u) {
                        const Rec &r = rec[qb + t0 + u];
                        okv[u] = ST ? r.ok : r.ok2;
#pragma unroll
                        for (int k = 0; k < NK; ++k) {
                            const int o = ST ? r.o[k] : r.o2[k];
                            tapv[u][k] = src[(size_t)o * nb + bb];
                        }
                    }
#pragma unroll
                    for (int u = 0; u < 2; ++u) {
                        const Rec &r = rec[qb + t0 + u];
                        float acc[CB];
#pragma unroll
                        for (int e = 0; e < CB; ++e) acc[e] = 0.0f;
#pragma unroll
                        for (int k = 0; k < NK; ++k) {
                            if (!(okv[u] & (1u << k))) continue;
                            float v[CB];
                            unpack16(tapv[u][k], v);
                            const float w = ST ? r.w[k] : r.w2[k];
#pragma unroll
                            for (int e = 0; e < CB; ++e) acc[e] = acc[e] + v[e] * w;
                        }
                        if constexpr (ST) {
                            const float va = r.valid, sd = r.sdisp;
#pragma unroll
                            for (int e = 0; e < CB; ++e) res[t0 + u][e] = acc[e] * va * sd;
                        } else {
                            const float v2 = r.v2d, md = r.mdisp;
#pragma unroll
                            for (int e = 0; e < CB; ++e) {
                                const float sval = acc[e] * v2;
                                res[t0 + u][e] = sval * md;
                            }
                        }
                    }
                }
                const long long i = i0 + qb;
                if (i < N) {  // (N % 4 == 0: a group of four is inside or outside as a whole)
                    T *dst = out + ((size_t)b * (g.C + g.Cs) + ch0 + (size_t)bb * CB) * N + i;
#pragma unroll
                    for (int e = 0; e < CB; ++e) {
                        if constexpr (sizeof(T) == 4) {
                            const f2v_u32x4 pk = {__float_as_uint(res[0][e]), __float_as_uint(res[1][e]),
                                                  __float_as_uint(res[2][e]), __float_as_uint(res[3][e])};
                            __builtin_nontemporal_store(pk, (f2v_u32x4 *)(dst + (size_t)e * N));
                        } else {
                            typedef uint32_t f2v_u32x2 __attribute__((ext_vector_type(2)));
                            const f2v_u32x2 pk = {dfm::pack_bf16x2(res[0][e], res[1][e]), dfm::pack_bf16x2(res[2][e], res[3][e])};
                            __builtin_nontemporal_store(pk, (f2v_u32x2 *)(dst + (size_t)e * N));
                        }
                    }
                }
            }
        }
    };
    if constexpr (!PLANAR) {
        gather(std::true_type{}, sv, nbs, 0, nbs % 8 == 0 ? 8 : 4);
        if (nbm > 0) gather(std::false_type{}, sp, nbm, nbs, nbm % 8 == 0 ? 8 : 4);
    } else {
        gather_planar(std::true_type{}, sv, nbs, 0, nbs % 8 == 0 ? 8 : 4);
        if (nbm > 0) gather_planar(std::false_type{}, sp, nbm, g.C, nbm % 8 == 0 ? 8 : 4);
    }
    (void)nbt;
}

}  // namespace

// pixel-major staging is used when both channel counts are whole 16-byte blocks
static bool f2v_pixel_major(const dfm_f2v_desc *d)
{
    const int CB = d->dtype == DFM_BF16 ? 8 : 4;
    return d->channels % CB == 0 && d->sem_channels % CB == 0;
}

// the several-lanes-per-voxel kernel: 4 or 8 sixteen-byte blocks of a source per trip
static bool f2v_lanes_per_voxel(const dfm_f2v_desc *d)
{
    const int CB = d->dtype == DFM_BF16 ? 8 : 4;
    const int nbs = d->channels / CB, nbm = d->sem_channels / CB;
    return nbs % 4 == 0 && nbm % 4 == 0;
}

extern "C" DFM_API size_t dfm_frustum_to_voxel_workspace_bytes(const dfm_f2v_desc *d)
{
    if (!d || d->batch <= 0 || d->channels <= 0 || d->d <= 0 || d->h <= 0 || d->w <= 0 ||
        d->sem_channels < 0 || (d->dtype != DFM_F32 && d->dtype != DFM_BF16))
        return 0;
    if (!f2v_pixel_major(d)) return 256;
    return f2v_pm_layout(d, d->dtype == DFM_BF16 ? 2 : 4).total();
}

static int f2v_fwd_impl(const dfm_f2v_desc *d, const void *stereo, const void *softmax, FusedHead fh,
                        int32_t head_scale, const void *sem, const float *coords, const float *cam2img,
                        void *out, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!d) return set_error(DFM_ERR_INVALID_ARG, "desc is NULL");
    if (d->batch <= 0 || d->channels <= 0 || d->d <= 0 || d->h <= 0 || d->w <= 0 || d->nz <= 0 ||
        d->ny <= 0 || d->nx <= 0 || d->sem_channels < 0)
        return set_error(DFM_ERR_INVALID_ARG, "non-positive size in dfm_f2v_desc");
    if (int rc = check_dtype(d->dtype)) return rc;
    const bool want_disp = d->stereo_atten || (d->sem_channels > 0 && !d->no_sem_atten);
    if (!stereo || !coords || !cam2img || !out || (d->sem_channels > 0 && !sem) || (want_disp && !softmax && !fh.cost))
        return set_error(DFM_ERR_INVALID_ARG, "NULL device pointer");
    if ((long long)d->ds * d->hs * d->ws >= (1ll << 31) || (long long)d->d * d->h * d->w >= (1ll << 31))
        return set_error(DFM_ERR_UNSUPPORTED, "volume too large for 32-bit corner offsets");
    if (d->batch > 65535) return set_error(DFM_ERR_UNSUPPORTED, "batch > 65535");
    const bool pm = f2v_pixel_major(d);
    if (d->out_channels_last && !pm)
        return set_error(DFM_ERR_UNSUPPORTED, "channels-last output needs channel counts of whole 16-byte blocks");
    F2vGeom g;
    if (const int rc = f2v_geom(d, fh, head_scale, &g)) return rc;
    const long long N = (long long)d->nz * d->ny * d->nx;
    const dim3 grid((unsigned)((N + 255) / 256), d->batch);
    hipStream_t st = (hipStream_t)stream;
    if (d->sem_channels_last && !pm)
        return set_error(DFM_ERR_UNSUPPORTED,
                         "channels-last cur_sem_feats needs channel counts of whole 16-byte blocks");
    if (d->stereo_channels_last && (!pm || ((uintptr_t)stereo & 15)))
        return set_error(DFM_ERR_UNSUPPORTED,
                         "channels-last stereo_feat needs channel counts of whole 16-byte blocks");
    if (pm) {
        if (!workspace || workspace_bytes < dfm_frustum_to_voxel_workspace_bytes(d))
            return set_error(DFM_ERR_WORKSPACE,
                             "workspace smaller than dfm_frustum_to_voxel_workspace_bytes");
        const long long vox = (long long)d->d * d->h * d->w, pix = (long long)d->hsem * d->wsem;
        const bool in_place = d->stereo_channels_last != 0;
        void *stereo_pm = in_place ? const_cast<void *>(stereo) : workspace;
        // a channels-last (NHWC) semantic map is the pixel-major layout already
        const bool sem_in_place = d->sem_channels_last != 0 && d->sem_channels > 0;
        if (sem_in_place && ((uintptr_t)sem & 15))
            return set_error(DFM_ERR_INVALID_ARG, "channels-last cur_sem_feats must be 16-byte aligned");
        void *sem_pm = sem_in_place ? const_cast<void *>(sem)
                                    : (void *)((char *)workspace + f2v_pm_layout(d, d->dtype == DFM_BF16 ? 2 : 4).first);
        const dim3 pg1((unsigned)((vox + 63) / 64), (d->channels + 31) / 32, d->batch);
        const dim3 pg2((unsigned)((pix + 63) / 64), (d->sem_channels + 31) / 32, d->batch);
        by_dtype(d->dtype, [&](auto t) {
            using T = decltype(t);
            if (!in_place)
                hipLaunchKernelGGL(pack_pixel_major_kernel<T>, pg1, dim3(256), 0, st, (const T *)stereo,
                                   (T *)stereo_pm, d->channels, d->channels, vox);
            if (d->sem_channels > 0 && !sem_in_place)
                hipLaunchKernelGGL(pack_pixel_major_kernel<T>, pg2, dim3(256), 0, st, (const T *)sem, (T *)sem_pm,
                                   d->sem_channels, d->sem_channels, pix);
            auto sample = [&](auto kernel) {
                hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, g, (const uint4 *)stereo_pm, (const T *)softmax,
                                   (const uint4 *)sem_pm, coords, cam2img, (T *)out, fh);
            };
            if (f2v_lanes_per_voxel(d) && g.out_cl) sample(f2v_pm8_kernel<T, false>);
            else if (f2v_lanes_per_voxel(d) && N % 4 == 0 && !((uintptr_t)out & 15)) sample(f2v_pm8_kernel<T, true>);
            else sample(f2v_pm_kernel<T>);
        });
    } else {
        by_dtype(d->dtype, [&](auto t) {
            using T = decltype(t);
            hipLaunchKernelGGL(f2v_kernel<T>, grid, dim3(256), 0, st, g, (const T *)stereo, (const T *)softmax,
                               (const T *)sem, coords, cam2img, (T *)out, fh);
        });
    }
    HIP_TRY(hipGetLastError());
    return DFM_OK;
}

extern "C" DFM_API int dfm_frustum_to_voxel_fwd(const dfm_f2v_desc *d, const void *stereo, const void *softmax,
                                                const void *sem, const float *coords, const float *cam2img,
                                                void *out, void *workspace, size_t workspace_bytes, void *stream)
{
    return f2v_fwd_impl(d, stereo, softmax, FusedHead{nullptr, nullptr, nullptr}, 0, sem, coords, cam2img, out,
                        workspace, workspace_bytes, stream);
}

extern "C" DFM_API int dfm_frustum_to_voxel_fused_fwd(const dfm_f2v_desc *d, const void *stereo, const void *cost,
                                                      const float *col_max, const float *col_sum,
                                                      int32_t head_scale, const void *sem, const float *coords,
                                                      const float *cam2img, void *out, void *workspace,
                                                      size_t workspace_bytes, void *stream)
{
    if (!cost || !col_max || !col_sum) return set_error(DFM_ERR_INVALID_ARG, "NULL device pointer");
    return f2v_fwd_impl(d, stereo, nullptr, FusedHead{cost, col_max, col_sum}, head_scale, sem, coords, cam2img,
                        out, workspace, workspace_bytes, stream);
}
