// imitation_loss.hip -- the LiDAR-teacher feature-imitation loss of DfM
// (reference: DfM.get_imitation_reg_layer_loss, mmdet3d/models/detectors/dfm.py:468-540, with
// NormalizeLayer / WeightedL2WithSigmaLoss of detectors/imitation_utils.py).
//
// The reference permutes both feature tensors, builds the in-box mask of the BEV cells, ANDs it with
// any_c(target != 0), gathers three (Npos, C) copies, normalises, squares and takes two means.  Only the
// cells inside a ground-truth box contribute (a few per cent of the BEV grid), so here the box test comes
// first and only those cells' columns of the two tensors are read, where they lie (planar or channels-last,
// fp32 or bf16, each tensor on its own):
//
//   forward : one lane per BEV cell tests the boxes; a workgroup compacts its in-box cells into an LDS list
//             (fixed order: cell index), and its four waves walk the list with all 64 lanes spread over the
//             cell's (z, channel) values -- whole z rows packed into a wave when C divides 64.  Per
//             workgroup: S = sum 0.5 (pred - t')^2, the positives count, per channel sum t and sum |t|
//             (what NormalizeLayer.update needs), written as one partial row; the workgroup that draws the
//             last ticket adds the rows in index order in fp64.  No floating-point atomics: the result is
//             the same bits run after run.
//   stats   : the same kernel with new_center: per channel sum |t - new_center| over the positives (the
//             two centering NormalizeLayer types measure their scale on the centred values).
//   backward: grad_pred = coef (pred - t') at positives, 0 elsewhere, one dense pass over grad_pred in
//             pred's own layout, 16 bytes per lane; coef is read from device memory.
#include "box_membership.h"
#include "dfm_common.h"

using namespace dfm;

namespace {

constexpr int IMI_THREADS = 256;   // 4 waves
constexpr int IMI_WAVES = 4;
constexpr int IMI_CPT = 4;         // cells per thread
constexpr int IMI_CELLS = IMI_THREADS * IMI_CPT;
constexpr int IMI_BOX_CHUNK = 256; // boxes staged in LDS at a time
constexpr int IMI_U = 4;           // list items a wave keeps in flight
constexpr int IMI_MAX_C = 1024;

struct ImiGeom {
    int32_t B, C, Nz, P2, T, full, pts_batched, center_len, scale_len;
    int32_t G, passes;        // C <= 64: z rows per 64-lane pass, passes per cell
    int32_t A;                // LDS accumulator stride: max(64, C)
    int32_t wg_per_b, W, ns;  // workgroups per sample, in all; floats per partial row
    int64_t p_sb, p_sc, p_sz, p_sp, t_sb, t_sc, t_sz, t_sp;  // element strides: sample, channel, z, cell
};

__device__ __forceinline__ float imi_wave_sum(float v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}
__device__ __forceinline__ int imi_wave_sum(int v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// t' of one target value (NormalizeLayer.forward with the buffers as they stand)
__device__ __forceinline__ float imi_norm(float t, int c, const ImiGeom &g, const float *center, const float *scale)
{
    if (g.center_len) t = t - center[g.center_len == 1 ? 0 : c];
    if (g.scale_len) t = t / scale[g.scale_len == 1 ? 0 : c];
    return t;
}

// workspace: uint32 ticket (16 bytes), int32 count[W], float part[W][ns]
//   ns = 1 + 2C: S, sum t [C], sum |t| [C];   STATS: ns = C: sum |t - new_center| [C]
// stats out (fp64): count, S, sum t [C], sum |t| [C];   STATS: sum |t - new_center| [C]
template <typename TP, typename TT, bool STATS>
__global__ __launch_bounds__(IMI_THREADS) void imitation_fwd_kernel(
    ImiGeom g, const TP *__restrict__ pred, const TT *__restrict__ target, const float *__restrict__ points,
    const float *__restrict__ boxes, const float *__restrict__ center, const float *__restrict__ scale,
    const float *__restrict__ new_center, unsigned char *__restrict__ mask, double *__restrict__ stats,
    unsigned int *__restrict__ ticket, int *__restrict__ ws_count, float *__restrict__ ws_part)
{
    __shared__ PtBox s_box[IMI_BOX_CHUNK];
    __shared__ int s_list[IMI_CELLS];
    __shared__ int s_cnt[IMI_CPT * IMI_WAVES];
    __shared__ float s_S[IMI_WAVES];
    __shared__ int s_n[IMI_WAVES];
    __shared__ int s_last;
    extern __shared__ float s_acc[];  // [wave][2][A]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x / g.wg_per_b;
    const int cell0 = (blockIdx.x - b * g.wg_per_b) * IMI_CELLS;

    // ---- 1. which of this workgroup's cells lie in a box
    bool in[IMI_CPT];
    {
        float px[IMI_CPT], py[IMI_CPT];
        const float *pts = points + (g.pts_batched ? (size_t)b * g.P2 * 3 : 0);
#pragma unroll
        for (int k = 0; k < IMI_CPT; ++k) {
            const int cell = cell0 + k * IMI_THREADS + tid;
            const bool ok = cell < g.P2;
            in[k] = ok && g.full;
            px[k] = ok && !g.full ? pts[(size_t)cell * 3 + 0] : 0.0f;
            py[k] = ok && !g.full ? pts[(size_t)cell * 3 + 1] : 0.0f;
            if (!ok) px[k] = __int_as_float(0x7fc00000);  // NaN: in no box
        }
        if (!g.full) {
            for (int t0 = 0; t0 < g.T; t0 += IMI_BOX_CHUNK) {
                const int nb = min(IMI_BOX_CHUNK, g.T - t0);
                __syncthreads();
                if (tid < nb) s_box[tid] = pt_box(boxes + ((size_t)b * g.T + t0 + tid) * 7, true);
                __syncthreads();
                for (int t = 0; t < nb; ++t) {
                    const PtBox bx = s_box[t];
#pragma unroll
                    for (int k = 0; k < IMI_CPT; ++k)
                        in[k] = in[k] | pt_in_box(px[k], py[k], 0.0f, bx);  // dfm.py:485: point z = 0
                }
            }
        }
    }
    // ---- 2. the in-box cells, compacted in cell order; every other cell's mask entries are 0
    unsigned long long bal[IMI_CPT];
#pragma unroll
    for (int k = 0; k < IMI_CPT; ++k) {
        bal[k] = __ballot(in[k]);
        if (lane == 0) s_cnt[k * IMI_WAVES + wave] = __popcll(bal[k]);
    }
    __syncthreads();
    int nlist = 0;
    {
        int base[IMI_CPT];
#pragma unroll
        for (int k = 0; k < IMI_CPT; ++k)
#pragma unroll
            for (int w = 0; w < IMI_WAVES; ++w) {
                if (w == wave) base[k] = nlist;
                nlist += s_cnt[k * IMI_WAVES + w];
            }
#pragma unroll
        for (int k = 0; k < IMI_CPT; ++k) {
            const int local = k * IMI_THREADS + tid;
            if (in[k]) {
                s_list[base[k] + __popcll(bal[k] & ((1ull << lane) - 1ull))] = local;
            } else if (!STATS && cell0 + local < g.P2) {
                for (int z = 0; z < g.Nz; ++z) mask[((size_t)b * g.Nz + z) * g.P2 + cell0 + local] = 0;
            }
        }
    }
    __syncthreads();

    // ---- 3. walk the list
    const TP *pb = STATS ? nullptr : pred + (size_t)b * g.p_sb;
    const TT *tb = target + (size_t)b * g.t_sb;
    float accS = 0.0f;
    int accN = 0;
    float *my_acc = s_acc + (size_t)wave * 2 * g.A;
    if (g.C <= 64) {
        // a pass = G whole z rows of one cell: lane -> (row gi, channel c)
        const int gi = lane / g.C, c = lane - gi * g.C;
        const bool lane_on = gi < g.G;
        const unsigned long long row_bits = (g.C == 64 ? ~0ull : ((1ull << g.C) - 1ull)) << (lane_on ? gi * g.C : 0);
        const float nc = STATS && lane_on ? new_center[c] : 0.0f;
        float acc_t = 0.0f, acc_a = 0.0f;
        const int items = nlist * g.passes;
        for (int i0 = wave; i0 < items; i0 += IMI_WAVES * IMI_U) {
            float tv[IMI_U], pv[IMI_U];
            bool on[IMI_U];
            size_t mo[IMI_U];
#pragma unroll
            for (int u = 0; u < IMI_U; ++u) {
                const int i = i0 + IMI_WAVES * u;
                on[u] = false; tv[u] = 0.0f; pv[u] = 0.0f; mo[u] = 0;
                if (i < items) {
                    const int li = i / g.passes, ps = i - li * g.passes;
                    const int cell = cell0 + s_list[li];
                    const int z = ps * g.G + gi;
                    on[u] = lane_on && z < g.Nz;
                    if (on[u]) {
                        tv[u] = elem<TT>::load(tb[c * g.t_sc + z * g.t_sz + cell * g.t_sp]);
                        if (!STATS) pv[u] = elem<TP>::load(pb[c * g.p_sc + z * g.p_sz + cell * g.p_sp]);
                        mo[u] = ((size_t)b * g.Nz + z) * g.P2 + cell;
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < IMI_U; ++u) {
                if (i0 + IMI_WAVES * u >= items) break;  // wave-uniform
                const unsigned long long nz = __ballot(on[u] && tv[u] != 0.0f);  // a NaN is non-zero, as in torch
                const bool pos = on[u] && (nz & row_bits) != 0ull;
                if (!STATS && on[u] && c == 0) {
                    mask[mo[u]] = pos ? 1 : 0;
                    accN += pos ? 1 : 0;
                }
                if (pos) {
                    if (STATS) {
                        acc_a += fabsf(tv[u] - nc);
                    } else {
                        acc_t += tv[u];
                        acc_a += fabsf(tv[u]);
                        const float tn = imi_norm(tv[u], c, g, center, scale);
                        if (tn == tn) {  // a NaN target becomes the input: the term is 0
                            const float d = pv[u] - tn;
                            accS += 0.5f * (d * d);
                        }
                    }
                }
            }
        }
        my_acc[lane] = acc_t;
        my_acc[g.A + lane] = acc_a;
    } else {
        // C > 64: an item is one (cell, z) row, walked in 64-channel chunks; lane owns channels lane + 64 j
        for (int c = lane; c < g.C; c += 64) { my_acc[c] = 0.0f; my_acc[g.A + c] = 0.0f; }
        const int items = nlist * g.Nz;
        for (int i = wave; i < items; i += IMI_WAVES) {
            const int li = i / g.Nz, z = i - li * g.Nz;
            const int cell = cell0 + s_list[li];
            const TT *tp = tb + z * g.t_sz + cell * g.t_sp;
            unsigned long long nz = 0ull;
            for (int c0 = 0; c0 < g.C; c0 += 64) {
                const int c = c0 + lane;
                const float t = c < g.C ? elem<TT>::load(tp[c * g.t_sc]) : 0.0f;
                nz |= __ballot(t != 0.0f);
            }
            const bool pos = nz != 0ull;
            if (!STATS && lane == 0) {
                mask[((size_t)b * g.Nz + z) * g.P2 + cell] = pos ? 1 : 0;
                accN += pos ? 1 : 0;
            }
            if (!pos) continue;
            for (int c = lane; c < g.C; c += 64) {
                const float t = elem<TT>::load(tp[c * g.t_sc]);
                if (STATS) {
                    my_acc[g.A + c] += fabsf(t - new_center[c]);
                } else {
                    my_acc[c] += t;
                    my_acc[g.A + c] += fabsf(t);
                    const float p = elem<TP>::load(pb[c * g.p_sc + z * g.p_sz + cell * g.p_sp]);
                    const float tn = imi_norm(t, c, g, center, scale);
                    if (tn == tn) {
                        const float d = p - tn;
                        accS += 0.5f * (d * d);
                    }
                }
            }
        }
    }
    // ---- 4. this workgroup's partial row: waves, then rows, in index order
    accS = imi_wave_sum(accS);
    accN = imi_wave_sum(accN);
    if (lane == 0) { s_S[wave] = accS; s_n[wave] = accN; }
    __syncthreads();
    float *part = ws_part + (size_t)blockIdx.x * g.ns;
    const int rows = g.C <= 64 ? g.G : 1;
    for (int c = tid; c < g.C; c += IMI_THREADS) {
        float st = 0.0f, sa = 0.0f;
        for (int w = 0; w < IMI_WAVES; ++w)
            for (int r = 0; r < rows; ++r) {
                st += s_acc[(size_t)w * 2 * g.A + r * g.C + c];
                sa += s_acc[(size_t)w * 2 * g.A + g.A + r * g.C + c];
            }
        if (STATS) {
            part[c] = sa;
        } else {
            part[1 + c] = st;
            part[1 + g.C + c] = sa;
        }
    }
    if (!STATS && tid == 0) {
        part[0] = ((s_S[0] + s_S[1]) + s_S[2]) + s_S[3];
        ws_count[blockIdx.x] = ((s_n[0] + s_n[1]) + s_n[2]) + s_n[3];
    }
    // ---- 5. publish the row; the workgroup that draws the last ticket merges all of them in index order
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned int drawn = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = drawn == (unsigned int)(g.W - 1);
        if (s_last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
    }
    __syncthreads();
    if (!s_last) return;
    const int nout = STATS ? g.C : 2 + 2 * g.C;
    for (int j = tid; j < nout; j += IMI_THREADS) {
        double acc = 0.0;
        if (!STATS && j == 0) {
            long long n = 0;
            for (int w = 0; w < g.W; ++w) n += ws_count[w];
            acc = (double)n;
        } else {
            const float *col = ws_part + (STATS ? j : j - 1);
#pragma unroll 8
            for (int w = 0; w < g.W; ++w) acc += (double)col[(size_t)w * g.ns];
        }
        stats[j] = acc;
    }
}

// ---- backward: one dense pass over grad_pred in memory order, V elements (16 bytes) per lane --------------------
// channels-last: the V elements are V channels of one position; planar: V positions of one channel
template <typename TP, typename TT, int V>
__global__ __launch_bounds__(256) void imitation_bwd_kernel(
    ImiGeom g, const TP *__restrict__ pred, const TT *__restrict__ target, const unsigned char *__restrict__ mask,
    const float *__restrict__ center, const float *__restrict__ scale, const float *__restrict__ coef_ptr,
    TP *__restrict__ grad, int p_cl, long long nvec)
{
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v >= nvec) return;
    const long long e0 = v * V;
    const long long P = (long long)g.Nz * g.P2;
    // (sample, channel, position) of element e0
    int b, c;
    long long p;
    if (p_cl) {
        const long long bp = e0 / g.C;
        c = (int)(e0 - bp * g.C);
        b = (int)(bp / P);
        p = bp - (long long)b * P;
    } else {
        const long long bc = e0 / P;
        p = e0 - bc * P;
        b = (int)(bc / g.C);
        c = (int)(bc - (long long)b * g.C);
    }
    const unsigned char *mb = mask + (size_t)b * P;
    float out[V];
    bool any = false;
#pragma unroll
    for (int k = 0; k < V; ++k) {
        out[k] = 0.0f;
        any |= mb[p_cl ? p : p + k] != 0;
    }
    if (any) {
        const float coef = *coef_ptr;
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const long long pk = p_cl ? p : p + k;
            const int ck = p_cl ? c + k : c;
            if (!mb[pk]) continue;
            const int z = (int)(pk / g.P2);
            const long long cell = pk - (long long)z * g.P2;
            const float t = elem<TT>::load(target[b * g.t_sb + ck * g.t_sc + z * g.t_sz + cell * g.t_sp]);
            const float tn = imi_norm(t, ck, g, center, scale);
            if (tn == tn) out[k] = coef * (elem<TP>::load(pred[e0 + k]) - tn);
        }
    }
    if constexpr (V == 1) {
        grad[e0] = elem<TP>::store(out[0]);
    } else {
        store16<TP>(grad + e0, out);
    }
}

int check(const dfm_imitation_desc *d)
{
    if (!d) return set_error(DFM_ERR_INVALID_ARG, "desc is NULL");
    if (d->batch <= 0 || d->channels <= 0 || d->nz <= 0 || d->ny <= 0 || d->nx <= 0)
        return set_error(DFM_ERR_INVALID_ARG, "non-positive size in dfm_imitation_desc");
    if (d->mode != DFM_IMI_INBOX && d->mode != DFM_IMI_FULL)
        return set_error(DFM_ERR_INVALID_ARG, "mode must be DFM_IMI_INBOX or DFM_IMI_FULL");
    if (d->mode == DFM_IMI_INBOX && d->num_boxes < 0)
        return set_error(DFM_ERR_INVALID_ARG, "negative num_boxes");
    if (d->points_batch != 1 && d->points_batch != d->batch)
        return set_error(DFM_ERR_INVALID_ARG, "points_batch must be 1 or batch");
    for (int32_t len : {d->center_len, d->scale_len})
        if (len != 0 && len != 1 && len != d->channels)
            return set_error(DFM_ERR_INVALID_ARG, "center_len / scale_len must be 0, 1 or channels");
    for (int32_t dt : {d->pred_dtype, d->target_dtype})
        if (int rc = check_dtype(dt)) return rc;
    if (d->channels > IMI_MAX_C) return set_error(DFM_ERR_UNSUPPORTED, "channels > 1024");
    if ((long long)d->ny * d->nx > (1ll << 30) || (long long)d->ny * d->nx * d->nz > (1ll << 31) - 1)
        return set_error(DFM_ERR_UNSUPPORTED, "grid too large");
    return DFM_OK;
}

ImiGeom geom(const dfm_imitation_desc *d)
{
    ImiGeom g{};
    g.B = d->batch; g.C = d->channels; g.Nz = d->nz; g.P2 = d->ny * d->nx;
    g.full = d->mode == DFM_IMI_FULL;
    g.T = g.full ? 0 : d->num_boxes;
    g.pts_batched = d->points_batch != 1;
    g.center_len = d->center_len; g.scale_len = d->scale_len;
    g.G = (g.C <= 64 && 64 % g.C == 0) ? 64 / g.C : 1;
    if (g.G > g.Nz) g.G = g.Nz;
    g.passes = (g.Nz + g.G - 1) / g.G;
    g.A = g.C > 64 ? g.C : 64;
    g.wg_per_b = (g.P2 + IMI_CELLS - 1) / IMI_CELLS;
    g.W = g.wg_per_b * g.B;
    g.ns = 1 + 2 * g.C;
    const int64_t P = (int64_t)g.Nz * g.P2;
    auto strides = [&](int cl, int64_t &sb, int64_t &sc, int64_t &sz, int64_t &sp) {
        sb = P * g.C;
        if (cl) { sc = 1; sz = (int64_t)g.P2 * g.C; sp = g.C; }
        else { sc = P; sz = g.P2; sp = 1; }
    };
    strides(d->pred_channels_last, g.p_sb, g.p_sc, g.p_sz, g.p_sp);
    strides(d->target_channels_last, g.t_sb, g.t_sc, g.t_sz, g.t_sp);
    return g;
}

size_t ws_bytes(const ImiGeom &g) { return 16 + (size_t)g.W * 4 + (size_t)g.W * g.ns * 4; }

template <typename TP, typename TT>
int launch_fwd(const ImiGeom &g0, const void *pred, const void *target, const float *points, const float *boxes,
               const float *center, const float *scale, const float *new_center, unsigned char *mask, double *stats,
               void *ws, hipStream_t st)
{
    ImiGeom g = g0;
    unsigned int *ticket = (unsigned int *)ws;
    int *cnt = (int *)((char *)ws + 16);
    float *part = (float *)(cnt + g.W);
    HIP_TRY(hipMemsetAsync(ticket, 0, 16, st));
    const size_t lds = (size_t)IMI_WAVES * 2 * g.A * sizeof(float);
    if (new_center) {
        g.ns = g.C;
        hipLaunchKernelGGL((imitation_fwd_kernel<TP, TT, true>), dim3(g.W), dim3(IMI_THREADS), lds, st, g,
                           (const TP *)nullptr, (const TT *)target, points, boxes, center, scale, new_center,
                           (unsigned char *)nullptr, stats, ticket, cnt, part);
    } else {
        hipLaunchKernelGGL((imitation_fwd_kernel<TP, TT, false>), dim3(g.W), dim3(IMI_THREADS), lds, st, g,
                           (const TP *)pred, (const TT *)target, points, boxes, center, scale, new_center, mask,
                           stats, ticket, cnt, part);
    }
    HIP_TRY(hipGetLastError());
    return DFM_OK;
}

template <typename TP, typename TT>
int launch_bwd(const ImiGeom &g, int p_cl, const void *pred, const void *target, const unsigned char *mask,
               const float *center, const float *scale, const float *coef, void *grad, hipStream_t st)
{
    constexpr int V = vec16<TP>::N;
    const long long P = (long long)g.Nz * g.P2, n = (long long)g.B * g.C * P;
    const bool vec = (p_cl ? g.C % V == 0 : P % V == 0) && ((uintptr_t)grad % 16 == 0);
    const long long nvec = vec ? n / V : n;
    const long long blocks = (nvec + 255) / 256;
    if (blocks > 0x7fffffffll) return set_error(DFM_ERR_UNSUPPORTED, "tensor too large");
    if (vec)
        hipLaunchKernelGGL((imitation_bwd_kernel<TP, TT, V>), dim3((unsigned)blocks), dim3(256), 0, st, g,
                           (const TP *)pred, (const TT *)target, mask, center, scale, coef, (TP *)grad, p_cl, nvec);
    else
        hipLaunchKernelGGL((imitation_bwd_kernel<TP, TT, 1>), dim3((unsigned)blocks), dim3(256), 0, st, g,
                           (const TP *)pred, (const TT *)target, mask, center, scale, coef, (TP *)grad, p_cl, nvec);
    HIP_TRY(hipGetLastError());
    return DFM_OK;
}

}  // namespace

extern "C" DFM_API size_t dfm_imitation_loss_workspace_bytes(const dfm_imitation_desc *d)
{
    if (check(d) != DFM_OK) return 0;
    return ws_bytes(geom(d));
}

extern "C" DFM_API int dfm_imitation_loss_fwd(const dfm_imitation_desc *d, const void *pred, const void *target,
                                              const float *points, const float *boxes, const float *center,
                                              const float *scale, const float *new_center, unsigned char *mask,
                                              double *stats, void *workspace, size_t workspace_bytes, void *stream)
{
    int rc = check(d);
    if (rc != DFM_OK) return rc;
    const bool stats_only = new_center != nullptr;
    if (!target || !stats || !workspace || (!stats_only && (!pred || !mask)))
        return set_error(DFM_ERR_INVALID_ARG, "NULL device pointer");
    if (d->mode == DFM_IMI_INBOX && (!points || (d->num_boxes > 0 && !boxes)))
        return set_error(DFM_ERR_INVALID_ARG, "NULL points / boxes with mode DFM_IMI_INBOX");
    if ((d->center_len && !center) || (d->scale_len && !scale))
        return set_error(DFM_ERR_INVALID_ARG, "NULL center / scale with a non-zero length");
    const ImiGeom g = geom(d);
    if (workspace_bytes < ws_bytes(g))
        return set_errorf(DFM_ERR_WORKSPACE, "imitation loss needs %zu workspace bytes, got %zu", ws_bytes(g),
                          workspace_bytes);
    hipStream_t st = (hipStream_t)stream;
    return by_dtype(d->pred_dtype, [&](auto tp) {
        return by_dtype(d->target_dtype, [&](auto tt) {
            return launch_fwd<decltype(tp), decltype(tt)>(g, pred, target, points, boxes, center, scale, new_center,
                                                          mask, stats, workspace, st);
        });
    });
}

extern "C" DFM_API int dfm_imitation_loss_bwd(const dfm_imitation_desc *d, const void *pred, const void *target,
                                              const unsigned char *mask, const float *center, const float *scale,
                                              const float *coef, void *grad_pred, void *stream)
{
    int rc = check(d);
    if (rc != DFM_OK) return rc;
    if (!pred || !target || !mask || !coef || !grad_pred)
        return set_error(DFM_ERR_INVALID_ARG, "NULL device pointer");
    if ((d->center_len && !center) || (d->scale_len && !scale))
        return set_error(DFM_ERR_INVALID_ARG, "NULL center / scale with a non-zero length");
    const ImiGeom g = geom(d);
    hipStream_t st = (hipStream_t)stream;
    return by_dtype(d->pred_dtype, [&](auto tp) {
        return by_dtype(d->target_dtype, [&](auto tt) {
            return launch_bwd<decltype(tp), decltype(tt)>(g, d->pred_channels_last, pred, target, mask, center, scale,
                                                          coef, grad_pred, st);
        });
    });
}
