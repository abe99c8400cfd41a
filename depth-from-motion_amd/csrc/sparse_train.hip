// sparse_train.hip -- training the LiDAR teacher's sparse encoder (include/dfm_hip_sparse_train.h states the
// semantics): the inverse neighbour table, the FP32-MFMA weight gradient with its fixed-order partials, BatchNorm1d
// over the live rows (statistics, apply + ReLU, backward reduce, backward apply, running statistics) and dense()
// backward.  The input gradient is sparse_conv.hip's forward kernel over the inverse table.  No floating-point
// atomics; every index read from a table is range-checked before it addresses memory.
#include "dfm_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int WCHUNK = DFM_SPARSE_WGRAD_CHUNK;
constexpr int BCHUNK = DFM_SPARSE_BN_CHUNK;

inline dim3 blocks(int64_t n) { return dim3((unsigned)((n + 255) / 256)); }

// the rows a reduction walks: all of them, or -- live_rows given: the caller's promise that every row at or past
// *live_rows has b < 0 -- that many (the count stays on the device)
__device__ __forceinline__ int64_t row_limit(int64_t rows, const int32_t *__restrict__ live_rows)
{
    if (!live_rows) return rows;
    const int64_t n = *live_rows;
    return n < 0 ? 0 : (n < rows ? n : rows);
}

__global__ __launch_bounds__(256) void inverse_table_kernel(const int32_t *__restrict__ nbr, int64_t total,
                                                            int64_t out_rows, int64_t in_rows,
                                                            int32_t *__restrict__ inv)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int i = nbr[t];
    if (i < 0 || i >= in_rows) return;
    const int64_t k = t / out_rows;
    inv[k * in_rows + i] = (int32_t)(t - k * out_rows);
}

// One wave per (chunk of WCHUNK output rows, offset k, 16 input channels): D (16 ci x 16 co) += A (16 ci x 4 rows) .
// B (4 rows x 16 co) per step, NT = cout / 16 accumulator tiles.  A: lane holds A[m = lane & 15][row = lane >> 4];
// B: lane holds B[row = lane >> 4][n = lane & 15]; C/D: row = (lane >> 4) * 4 + reg, column = lane & 15.
// An MFMA is a chain of four fused multiply-adds onto its accumulator, so ONE accumulator over a chunk would be a
// chain as long as the chunk and its rounding error would grow with the row count.  The 16 four-row steps of every 64
// rows go round-robin to WAYS accumulators instead (chains an eighth as long; a quarter at cout = 64, where eight
// would take the wave's whole register file), which are added as a fixed binary tree at the end: the order is fixed,
// so the bits are.
template <int NT>
__global__ __launch_bounds__(64) void wgrad_partial_kernel(int cin, int taps, const float *__restrict__ in,
                                                           int64_t in_rows, const int32_t *__restrict__ nbr,
                                                           const int32_t *__restrict__ out_coors, int64_t out_rows,
                                                           const float *__restrict__ grad_out,
                                                           const int32_t *__restrict__ live_rows,
                                                           float *__restrict__ partial, int32_t *__restrict__ flags)
{
    constexpr int COUT = NT * 16, WAYS = NT == 4 ? 4 : 8;
    const int lane = threadIdx.x, m = lane & 15, kq = lane >> 4;
    const int chunk = blockIdx.x, k = blockIdx.y, mt = blockIdx.z, cin16 = gridDim.z * 16;
    const int64_t row0 = (int64_t)chunk * WCHUNK;
    const int64_t limit = row_limit(out_rows, live_rows);
    const int64_t row_end = row0 + WCHUNK < limit ? row0 + WCHUNK : limit;
    const int ci = mt * 16 + m;
    f32x4 acc[WAYS][NT];
#pragma unroll
    for (int w = 0; w < WAYS; ++w)
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[w][t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    bool any = false;

    for (int64_t base = row0; base < row_end; base += 64) {
        const int64_t r = base + lane;
        int idx = -1;
        if (r < row_end) {
            idx = nbr ? nbr[(int64_t)k * out_rows + r] : (out_coors[r * 4] >= 0 ? (int)r : -1);
            if (idx < 0 || idx >= in_rows) idx = -1;
        }
        if (__ballot(idx >= 0) == 0) continue;  // zeros only: skipping them changes no bit
        any = true;
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            const int src = __shfl(idx, s * 4 + kq);
            if (__ballot(src >= 0) == 0) continue;
            const float a = (src >= 0 && ci < cin) ? in[(int64_t)src * cin + ci] : 0.0f;
            const float *g = grad_out + (base + s * 4 + kq) * COUT + m;  // read only where src >= 0: a live row
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const float b = src >= 0 ? g[t * 16] : 0.0f;
                acc[s % WAYS][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[s % WAYS][t], 0, 0, 0);
            }
        }
    }
    if (mt == 0 && lane == 0) flags[chunk * taps + k] = any ? 1 : 0;
    if (!any) return;
    float *p = partial + ((int64_t)chunk * taps + k) * cin16 * COUT;
#pragma unroll
    for (int width = WAYS / 2; width >= 1; width /= 2)  // (0+1), (2+3), ... then pairs of those, ...
#pragma unroll
        for (int w = 0; w < width; ++w)
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[w][t] = acc[2 * w][t] + acc[2 * w + 1][t];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int row = mt * 16 + kq * 4 + j;
#pragma unroll
        for (int t = 0; t < NT; ++t) p[row * COUT + t * 16 + m] = acc[0][t][j];
    }
}

__global__ __launch_bounds__(256) void wgrad_reduce_kernel(int cin, int cin16, int cout, int taps, int chunks,
                                                           int64_t out_rows,
                                                           const int32_t *__restrict__ live_rows,
                                                           const float *__restrict__ partial,
                                                           const int32_t *__restrict__ flags,
                                                           float *__restrict__ grad_weight)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= taps * cin * cout) return;
    const int64_t used = (row_limit(out_rows, live_rows) + WCHUNK - 1) / WCHUNK;
    if (used < chunks) chunks = (int)used;
    const int k = t / (cin * cout), rem = t - k * cin * cout;
    const int ci = rem / cout, co = rem - ci * cout;
    double sum = 0.0;  // the partials are few and fp32: their fp64 sum in ascending order, rounded once
    for (int c = 0; c < chunks; ++c)
        if (flags[c * taps + k]) sum += (double)partial[(((int64_t)c * taps + k) * cin16 + ci) * cout + co];
    grad_weight[t] = (float)sum;
}

struct BnChannel {
    float mean, rstd, w, b, count;
};

__device__ __forceinline__ BnChannel bn_channel(const float *__restrict__ stats, const float *__restrict__ weight,
                                                const float *__restrict__ bias, float eps, int c)
{
    BnChannel ch;
    ch.count = stats[c * 3];
    ch.mean = stats[c * 3 + 1];
    ch.rstd = 1.0f / sqrtf(stats[c * 3 + 2] / fmaxf(ch.count, 1.0f) + eps);
    ch.w = weight ? weight[c] : 1.0f;
    ch.b = bias ? bias[c] : 0.0f;
    return ch;
}

// the one statement of the forward value: the backward recomputes the ReLU mask from it
__device__ __forceinline__ float bn_value(float x, const BnChannel &ch)
{
    return (x - ch.mean) * ch.rstd * ch.w + ch.b;
}

__device__ __forceinline__ void chan_merge(float &n, float &mean, float &m2, float nb, float mb, float m2b)
{
    if (nb == 0.0f) return;
    const float tot = n + nb, delta = mb - mean;
    mean = mean + delta * (nb / tot);
    m2 = m2 + m2b + delta * delta * (n * nb / tot);
    n = tot;
}

// block = BCHUNK rows; thread = (row slot, channel); C = 16, 32 or 64 divides 256
__global__ __launch_bounds__(256) void bn_stats_partial_kernel(const float *__restrict__ x,
                                                               const int32_t *__restrict__ coors, int64_t rows,
                                                               const int32_t *__restrict__ live_rows, int channels,
                                                               float *__restrict__ partial)
{
    __shared__ float sh[3][256];
    const int c = threadIdx.x % channels, slot = threadIdx.x / channels, slots = 256 / channels;
    const int64_t row0 = (int64_t)blockIdx.x * BCHUNK, limit = row_limit(rows, live_rows);
    const int64_t row_end = row0 + BCHUNK < limit ? row0 + BCHUNK : limit;
    float n = 0.0f, mean = 0.0f, m2 = 0.0f;
    for (int64_t r = row0 + slot; r < row_end; r += slots) {
        if (coors[r * 4] < 0) continue;
        const float v = x[r * channels + c];
        n += 1.0f;
        const float d = v - mean;
        mean += d / n;
        m2 += d * (v - mean);
    }
    sh[0][threadIdx.x] = n, sh[1][threadIdx.x] = mean, sh[2][threadIdx.x] = m2;
    __syncthreads();
    if (slot != 0) return;
    for (int s = 1; s < slots; ++s) {
        const int o = s * channels + c;
        chan_merge(n, mean, m2, sh[0][o], sh[1][o], sh[2][o]);
    }
    float *p = partial + ((int64_t)blockIdx.x * channels + c) * 3;
    p[0] = n, p[1] = mean, p[2] = m2;
}

__global__ __launch_bounds__(64) void bn_stats_final_kernel(const float *__restrict__ partial, int nblocks,
                                                            int64_t rows, const int32_t *__restrict__ live_rows,
                                                            int channels, float *__restrict__ stats)
{
    const int c = threadIdx.x;
    if (c >= channels) return;
    const int64_t used = (row_limit(rows, live_rows) + BCHUNK - 1) / BCHUNK;
    if (used < nblocks) nblocks = (int)used;
    float n = 0.0f, mean = 0.0f, m2 = 0.0f;
    for (int b = 0; b < nblocks; ++b) {
        const float *p = partial + ((int64_t)b * channels + c) * 3;
        chan_merge(n, mean, m2, p[0], p[1], p[2]);
    }
    stats[c * 3] = n, stats[c * 3 + 1] = mean, stats[c * 3 + 2] = m2;
}

__global__ __launch_bounds__(256) void bn_apply_kernel(const float *__restrict__ x, const int32_t *__restrict__ coors,
                                                       int64_t total, int channels, const float *__restrict__ stats,
                                                       const float *__restrict__ weight,
                                                       const float *__restrict__ bias, float eps, int relu,
                                                       float *__restrict__ y)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int64_t r = t / channels;
    const int c = (int)(t - r * channels);
    float v = 0.0f;
    if (coors[r * 4] >= 0) {
        v = bn_value(x[t], bn_channel(stats, weight, bias, eps, c));
        if (relu) v = v > 0.0f ? v : 0.0f;
    }
    y[t] = v;
}

__global__ __launch_bounds__(256) void bn_bwd_partial_kernel(const float *__restrict__ x,
                                                             const float *__restrict__ grad_y,
                                                             const int32_t *__restrict__ coors, int64_t rows,
                                                             const int32_t *__restrict__ live_rows, int channels,
                                                             const float *__restrict__ stats,
                                                             const float *__restrict__ weight,
                                                             const float *__restrict__ bias, float eps, int relu,
                                                             float *__restrict__ partial)
{
    __shared__ float sh[2][256];
    const int c = threadIdx.x % channels, slot = threadIdx.x / channels, slots = 256 / channels;
    const int64_t row0 = (int64_t)blockIdx.x * BCHUNK, limit = row_limit(rows, live_rows);
    const int64_t row_end = row0 + BCHUNK < limit ? row0 + BCHUNK : limit;
    const BnChannel ch = bn_channel(stats, weight, bias, eps, c);
    float s0 = 0.0f, s1 = 0.0f;
    for (int64_t r = row0 + slot; r < row_end; r += slots) {
        if (coors[r * 4] < 0) continue;
        const float v = x[r * channels + c];
        if (relu && !(bn_value(v, ch) > 0.0f)) continue;
        const float g = grad_y[r * channels + c];
        s0 += g;
        s1 += g * ((v - ch.mean) * ch.rstd);
    }
    sh[0][threadIdx.x] = s0, sh[1][threadIdx.x] = s1;
    __syncthreads();
    if (slot != 0) return;
    for (int s = 1; s < slots; ++s) s0 += sh[0][s * channels + c], s1 += sh[1][s * channels + c];
    float *p = partial + ((int64_t)blockIdx.x * channels + c) * 2;
    p[0] = s0, p[1] = s1;
}

__global__ __launch_bounds__(64) void bn_bwd_final_kernel(const float *__restrict__ partial, int nblocks, int64_t rows,
                                                          const int32_t *__restrict__ live_rows, int channels,
                                                          float *__restrict__ sums)
{
    const int c = threadIdx.x;
    if (c >= channels) return;
    const int64_t used = (row_limit(rows, live_rows) + BCHUNK - 1) / BCHUNK;
    if (used < nblocks) nblocks = (int)used;
    float s0 = 0.0f, s1 = 0.0f;
    for (int b = 0; b < nblocks; ++b) {
        const float *p = partial + ((int64_t)b * channels + c) * 2;
        s0 += p[0], s1 += p[1];
    }
    sums[c] = s0, sums[channels + c] = s1;
}

__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const float *__restrict__ x,
                                                           const float *__restrict__ grad_y,
                                                           const int32_t *__restrict__ coors, int64_t total,
                                                           int channels, const float *__restrict__ stats,
                                                           const float *__restrict__ sums,
                                                           const float *__restrict__ weight,
                                                           const float *__restrict__ bias, float eps, int relu,
                                                           float *__restrict__ grad_x)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int64_t r = t / channels;
    const int c = (int)(t - r * channels);
    float out = 0.0f;
    if (coors[r * 4] >= 0) {
        const BnChannel ch = bn_channel(stats, weight, bias, eps, c);
        const float v = x[t];
        const float g = (relu && !(bn_value(v, ch) > 0.0f)) ? 0.0f : grad_y[t];
        const float n = fmaxf(ch.count, 1.0f), xhat = (v - ch.mean) * ch.rstd;
        out = ch.w * ch.rstd * (g - sums[c] / n - xhat * (sums[channels + c] / n));
    }
    grad_x[t] = out;
}

__global__ __launch_bounds__(64) void bn_running_kernel(const float *__restrict__ stats, int channels, float momentum,
                                                        float *__restrict__ running_mean,
                                                        float *__restrict__ running_var)
{
    const int c = threadIdx.x;
    if (c >= channels) return;
    const float count = stats[c * 3];
    if (!(count > 0.0f)) return;
    const float var = stats[c * 3 + 2] / fmaxf(count - 1.0f, 1.0f);
    running_mean[c] = running_mean[c] * (1.0f - momentum) + stats[c * 3 + 1] * momentum;
    running_var[c] = running_var[c] * (1.0f - momentum) + var * momentum;
}

__global__ __launch_bounds__(256) void dense_bwd_kernel(int batch, int d, int h, int w,
                                                        const float *__restrict__ grad_volume,
                                                        const int32_t *__restrict__ coors, int64_t total, int channels,
                                                        float *__restrict__ grad_features)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int64_t r = t / channels;
    const int c = (int)(t - r * channels);
    const int4 q = ((const int4 *)coors)[r];
    float v = 0.0f;
    if (q.x >= 0 && q.x < batch && q.y >= 0 && q.y < d && q.z >= 0 && q.z < h && q.w >= 0 && q.w < w)
        v = grad_volume[((((int64_t)q.x * channels + c) * d + q.y) * h + q.z) * (int64_t)w + q.w];
    grad_features[t] = v;
}

bool wgrad_channels_ok(int32_t cin, int32_t cout)
{
    return (cin == 3 || (cin >= 4 && cin % 4 == 0)) && cin <= 64 && (cout == 16 || cout == 32 || cout == 64);
}

size_t wgrad_bytes(int32_t cin, int32_t cout, int32_t taps, int64_t out_rows)
{
    const int64_t chunks = (out_rows + WCHUNK - 1) / WCHUNK, cin16 = (cin + 15) / 16 * 16;
    return (size_t)(chunks * taps) * (size_t)(cin16 * cout + 1) * 4;
}

bool bn_channels_ok(int32_t c) { return c == 16 || c == 32 || c == 64; }

// the checks every BatchNorm entry shares; rows * channels stays below the launch grid's 2^31 blocks of 256
int check_bn(const char *who, int64_t rows, int32_t channels, bool pointers_ok)
{
    if (rows < 0) return dfm::set_errorf(DFM_ERR_INVALID_ARG, "%s: rows < 0", who);
    if (!bn_channels_ok(channels))
        return dfm::set_errorf(DFM_ERR_UNSUPPORTED, "%s: %d channels (16, 32 or 64)", who, channels);
    if (rows >= INT32_MAX) return dfm::set_errorf(DFM_ERR_UNSUPPORTED, "%s: 2^31 - 1 rows or more", who);
    if (!pointers_ok) return dfm::set_errorf(DFM_ERR_INVALID_ARG, "%s: NULL pointer", who);
    return 0;
}

}  // namespace

extern "C" {

int dfm_sparse_inverse_table(const int32_t *nbr, int32_t taps, int64_t out_rows, int64_t in_rows, int32_t *inv,
                             void *stream)
{
    if (taps < 1 || out_rows < 0 || in_rows < 0)
        return dfm::set_error(DFM_ERR_INVALID_ARG, "dfm_sparse_inverse_table: a size < 1 or a negative row count");
    if (taps > DFM_SPARSE_MAX_TAPS)
        return dfm::set_errorf(DFM_ERR_UNSUPPORTED, "dfm_sparse_inverse_table: %d kernel offsets, at most %d", taps,
                               DFM_SPARSE_MAX_TAPS);
    if (in_rows >= INT32_MAX / DFM_SPARSE_MAX_TAPS || out_rows >= INT32_MAX / DFM_SPARSE_MAX_TAPS)
        return dfm::set_error(DFM_ERR_UNSUPPORTED, "dfm_sparse_inverse_table: 27 * rows reaches 2^31");
    if (out_rows && in_rows && (!nbr || !inv))
        return dfm::set_error(DFM_ERR_INVALID_ARG, "dfm_sparse_inverse_table: NULL pointer");
    if (out_rows == 0 || in_rows == 0) return 0;
    const int64_t total = (int64_t)taps * out_rows;
    inverse_table_kernel<<<blocks(total), 256, 0, (hipStream_t)stream>>>(nbr, total, out_rows, in_rows, inv);
    HIP_TRY(hipGetLastError());
    return 0;
}

size_t dfm_sparse_conv_wgrad_workspace_bytes(int32_t cin, int32_t cout, int32_t taps, int64_t out_rows)
{
    if (!wgrad_channels_ok(cin, cout) || taps < 1 || taps > DFM_SPARSE_MAX_TAPS || out_rows < 0 ||
        out_rows >= INT32_MAX)
        return 0;
    return wgrad_bytes(cin, cout, taps, out_rows);
}

int dfm_sparse_conv_wgrad(int32_t cin, int32_t cout, int32_t taps, const float *in, int64_t in_rows,
                          const int32_t *nbr, const int32_t *out_coors, int64_t out_rows, const float *grad_out,
                          float *grad_weight, void *workspace, size_t workspace_bytes, const int32_t *live_rows,
                          void *stream)
{
    if (cin < 1 || cout < 1 || taps < 1 || in_rows < 0 || out_rows < 0)
        return dfm::set_error(DFM_ERR_INVALID_ARG, "dfm_sparse_conv_wgrad: a size < 1 or a negative row count");
    if (taps > DFM_SPARSE_MAX_TAPS)
        return dfm::set_errorf(DFM_ERR_UNSUPPORTED, "dfm_sparse_conv_wgrad: %d kernel offsets, at most %d", taps,
                               DFM_SPARSE_MAX_TAPS);
    if (!wgrad_channels_ok(cin, cout))
        return dfm::set_errorf(DFM_ERR_UNSUPPORTED,
                               "dfm_sparse_conv_wgrad: channels %d -> %d (Cin: 3 or a multiple of 4 up to 64; Cout: "
                               "16, 32 or 64)", cin, cout);
    if (in_rows >= INT32_MAX || out_rows >= INT32_MAX)
        return dfm::set_error(DFM_ERR_UNSUPPORTED, "dfm_sparse_conv_wgrad: 2^31 - 1 rows or more");
    if (out_rows && !nbr && (taps != 1 || in_rows < out_rows))
        return dfm::set_error(DFM_ERR_INVALID_ARG,
                              "dfm_sparse_conv_wgrad: nbr may be NULL for one offset on the same rows only");
    if (!grad_weight || (out_rows && (!out_coors || !grad_out || !in || !workspace)))
        return dfm::set_error(DFM_ERR_INVALID_ARG, "dfm_sparse_conv_wgrad: NULL pointer");
    if (((uintptr_t)out_coors & 15) || (((uintptr_t)in | (uintptr_t)grad_out | (uintptr_t)grad_weight |
                                         (uintptr_t)workspace | (uintptr_t)live_rows) & 3))
        return dfm::set_error(DFM_ERR_INVALID_ARG, "dfm_sparse_conv_wgrad: a pointer is not aligned");
    const size_t need = wgrad_bytes(cin, cout, taps, out_rows);
    if (workspace_bytes < need)
        return dfm::set_errorf(DFM_ERR_INVALID_ARG, "dfm_sparse_conv_wgrad: workspace of %zu bytes, %zu needed",
                               workspace_bytes, need);
    hipStream_t s = (hipStream_t)stream;
    if (out_rows == 0) {
        HIP_TRY(hipMemsetAsync(grad_weight, 0, (size_t)taps * cin * cout * sizeof(float), s));
        return 0;
    }
    const int chunks = (int)((out_rows + WCHUNK - 1) / WCHUNK), mts = (cin + 15) / 16, cin16 = mts * 16;
    float *partial = (float *)workspace;
    int32_t *flags = (int32_t *)(partial + (size_t)chunks * taps * cin16 * cout);
    const dim3 grid((unsigned)chunks, (unsigned)taps, (unsigned)mts);
    const bool timed = dfm::profile_mark(stream, false);
    if (cout == 16)
        wgrad_partial_kernel<1><<<grid, 64, 0, s>>>(cin, taps, in, in_rows, nbr, out_coors, out_rows, grad_out,
                                                    live_rows, partial, flags);
    else if (cout == 32)
        wgrad_partial_kernel<2><<<grid, 64, 0, s>>>(cin, taps, in, in_rows, nbr, out_coors, out_rows, grad_out,
                                                    live_rows, partial, flags);
    else
        wgrad_partial_kernel<4><<<grid, 64, 0, s>>>(cin, taps, in, in_rows, nbr, out_coors, out_rows, grad_out,
                                                    live_rows, partial, flags);
    wgrad_reduce_kernel<<<blocks((int64_t)taps * cin * cout), 256, 0, s>>>(cin, cin16, cout, taps, chunks, out_rows,
                                                                           live_rows, partial, flags, grad_weight);
    if (timed) dfm::profile_mark(stream, true);
    HIP_TRY(hipGetLastError());
    return 0;
}

size_t dfm_sparse_bn_workspace_bytes(int64_t rows, int32_t channels)
{
    if (rows < 0 || rows >= INT32_MAX || !bn_channels_ok(channels)) return 0;
    return (size_t)((rows + BCHUNK - 1) / BCHUNK) * channels * 3 * sizeof(float);
}

int dfm_sparse_bn_stats(const float *x, const int32_t *coors, int64_t rows, int32_t channels, float *stats,
                        void *workspace, size_t workspace_bytes, const int32_t *live_rows, void *stream)
{
    if (int rc = check_bn("dfm_sparse_bn_stats", rows, channels, stats && (!rows || (x && coors && workspace))))
        return rc;
    if (workspace_bytes < dfm_sparse_bn_workspace_bytes(rows, channels))
        return dfm::set_error(DFM_ERR_INVALID_ARG, "dfm_sparse_bn_stats: workspace too small");
    if (((uintptr_t)x | (uintptr_t)coors | (uintptr_t)stats | (uintptr_t)workspace | (uintptr_t)live_rows) & 3)
        return dfm::set_error(DFM_ERR_INVALID_ARG, "dfm_sparse_bn_stats: a pointer is not 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int nblocks = (int)((rows + BCHUNK - 1) / BCHUNK);
    if (nblocks)
        bn_stats_partial_kernel<<<nblocks, 256, 0, s>>>(x, coors, rows, live_rows, channels, (float *)workspace);
    bn_stats_final_kernel<<<1, 64, 0, s>>>((const float *)workspace, nblocks, rows, live_rows, channels, stats);
    HIP_TRY(hipGetLastError());
    return 0;
}

int dfm_sparse_bn_apply(const float *x, const int32_t *coors, int64_t rows, int32_t channels, const float *stats,
                        const float *weight, const float *bias, float eps, int32_t relu, float *y, void *stream)
{
    if (int rc = check_bn("dfm_sparse_bn_apply", rows, channels, stats && (!rows || (x && coors && y)))) return rc;
    if (!(eps > 0.0f)) return dfm::set_error(DFM_ERR_INVALID_ARG, "dfm_sparse_bn_apply: eps must be > 0");
    if (((uintptr_t)x | (uintptr_t)coors | (uintptr_t)stats | (uintptr_t)weight | (uintptr_t)bias | (uintptr_t)y) & 3)
        return dfm::set_error(DFM_ERR_INVALID_ARG, "dfm_sparse_bn_apply: a pointer is not 4-byte aligned");
    if (rows == 0) return 0;
    const int64_t total = rows * channels;
    bn_apply_kernel<<<blocks(total), 256, 0, (hipStream_t)stream>>>(x, coors, total, channels, stats, weight, bias,
                                                                    eps, relu, y);
    HIP_TRY(hipGetLastError());
    return 0;
}

int dfm_sparse_bn_bwd_reduce(const float *x, const float *grad_y, const int32_t *coors, int64_t rows, int32_t channels,
                             const float *stats, const float *weight, const float *bias, float eps, int32_t relu,
                             float *sums, void *workspace, size_t workspace_bytes, const int32_t *live_rows,
                             void *stream)
{
    if (int rc = check_bn("dfm_sparse_bn_bwd_reduce", rows, channels,
                          stats && sums && (!rows || (x && grad_y && coors && workspace))))
        return rc;
    if (!(eps > 0.0f)) return dfm::set_error(DFM_ERR_INVALID_ARG, "dfm_sparse_bn_bwd_reduce: eps must be > 0");
    if (workspace_bytes < dfm_sparse_bn_workspace_bytes(rows, channels))
        return dfm::set_error(DFM_ERR_INVALID_ARG, "dfm_sparse_bn_bwd_reduce: workspace too small");
    if (((uintptr_t)x | (uintptr_t)grad_y | (uintptr_t)coors | (uintptr_t)stats | (uintptr_t)weight |
         (uintptr_t)bias | (uintptr_t)sums | (uintptr_t)workspace | (uintptr_t)live_rows) & 3)
        return dfm::set_error(DFM_ERR_INVALID_ARG, "dfm_sparse_bn_bwd_reduce: a pointer is not 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int nblocks = (int)((rows + BCHUNK - 1) / BCHUNK);
    if (nblocks)
        bn_bwd_partial_kernel<<<nblocks, 256, 0, s>>>(x, grad_y, coors, rows, live_rows, channels, stats, weight, bias,
                                                      eps, relu, (float *)workspace);
    bn_bwd_final_kernel<<<1, 64, 0, s>>>((const float *)workspace, nblocks, rows, live_rows, channels, sums);
    HIP_TRY(hipGetLastError());
    return 0;
}

int dfm_sparse_bn_bwd_apply(const float *x, const float *grad_y, const int32_t *coors, int64_t rows, int32_t channels,
                            const float *stats, const float *sums, const float *weight, const float *bias, float eps,
                            int32_t relu, float *grad_x, void *stream)
{
    if (int rc = check_bn("dfm_sparse_bn_bwd_apply", rows, channels,
                          stats && sums && (!rows || (x && grad_y && coors && grad_x))))
        return rc;
    if (!(eps > 0.0f)) return dfm::set_error(DFM_ERR_INVALID_ARG, "dfm_sparse_bn_bwd_apply: eps must be > 0");
    if (((uintptr_t)x | (uintptr_t)grad_y | (uintptr_t)coors | (uintptr_t)stats | (uintptr_t)sums |
         (uintptr_t)weight | (uintptr_t)bias | (uintptr_t)grad_x) & 3)
        return dfm::set_error(DFM_ERR_INVALID_ARG, "dfm_sparse_bn_bwd_apply: a pointer is not 4-byte aligned");
    if (rows == 0) return 0;
    const int64_t total = rows * channels;
    bn_bwd_apply_kernel<<<blocks(total), 256, 0, (hipStream_t)stream>>>(x, grad_y, coors, total, channels, stats, sums,
                                                                        weight, bias, eps, relu, grad_x);
    HIP_TRY(hipGetLastError());
    return 0;
}

int dfm_sparse_bn_running(const float *stats, int32_t channels, float momentum, float *running_mean,
                          float *running_var, void *stream)
{
    if (!bn_channels_ok(channels))
        return dfm::set_errorf(DFM_ERR_UNSUPPORTED, "dfm_sparse_bn_running: %d channels (16, 32 or 64)", channels);
    if (!stats || !running_mean || !running_var)
        return dfm::set_error(DFM_ERR_INVALID_ARG, "dfm_sparse_bn_running: NULL pointer");
    if (!(momentum >= 0.0f && momentum <= 1.0f))
        return dfm::set_error(DFM_ERR_INVALID_ARG, "dfm_sparse_bn_running: momentum outside [0, 1]");
    if (((uintptr_t)stats | (uintptr_t)running_mean | (uintptr_t)running_var) & 3)
        return dfm::set_error(DFM_ERR_INVALID_ARG, "dfm_sparse_bn_running: a pointer is not 4-byte aligned");
    bn_running_kernel<<<1, 64, 0, (hipStream_t)stream>>>(stats, channels, momentum, running_mean, running_var);
    HIP_TRY(hipGetLastError());
    return 0;
}

int dfm_sparse_dense_bwd(const float *grad_volume, const int32_t *coors, int64_t rows, int32_t channels, int32_t batch,
                         const int32_t *size3, float *grad_features, void *stream)
{
    if (!size3) return dfm::set_error(DFM_ERR_INVALID_ARG, "dfm_sparse_dense_bwd: NULL grid size");
    if (batch < 1 || size3[0] < 1 || size3[1] < 1 || size3[2] < 1)
        return dfm::set_error(DFM_ERR_INVALID_ARG, "dfm_sparse_dense_bwd: batch and grid sizes start at 1");
    if (channels < 1 || rows < 0)
        return dfm::set_error(DFM_ERR_INVALID_ARG, "dfm_sparse_dense_bwd: channels < 1 or rows < 0");
    if (rows && (!grad_volume || !coors || !grad_features))
        return dfm::set_error(DFM_ERR_INVALID_ARG, "dfm_sparse_dense_bwd: NULL pointer");
    const double cells = (double)batch * channels * size3[0] * size3[1] * size3[2];
    if (cells >= 2.0e18 || (double)rows * channels >= 5.0e11)
        return dfm::set_error(DFM_ERR_UNSUPPORTED,
                              "dfm_sparse_dense_bwd: a volume or a row block above the index range");
    if ((uintptr_t)coors & 15)
        return dfm::set_error(DFM_ERR_INVALID_ARG, "dfm_sparse_dense_bwd: coors is not 16-byte aligned");
    if (rows == 0) return 0;
    const int64_t total = rows * channels;
    dense_bwd_kernel<<<blocks(total), 256, 0, (hipStream_t)stream>>>(batch, size3[0], size3[1], size3[2], grad_volume,
                                                                     coors, total, channels, grad_features);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
