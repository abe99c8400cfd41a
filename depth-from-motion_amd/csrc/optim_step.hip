// optim_step.hip -- the end of a training iteration: the global L2 norm of all gradients, the clip against it and the
// AdamW update (mmcv's OptimizerHook: torch.nn.utils.clip_grad_norm_(params, max_norm=35, norm_type=2), then
// torch.optim.AdamW.step(); torch/optim/adam.py _single_tensor_adam states the arithmetic).
//
// A model is a few hundred small tensors, so a launch per tensor is all launch overhead.  Here every kernel works from
// one MULTI-TENSOR TABLE (a row per tensor: addresses, element count, type, that tensor's scalars) and one CHUNK TABLE
// (workgroup -> tensor, chunk): the grid is the number of chunks whatever the number of tensors.
//
//   sqnorm : a workgroup sums the squares of its chunk's gradients in fp32 -- per lane in index order, a butterfly over
//            the wave, the four waves in order through LDS -- and stores one partial.  No atomics.
//   step   : every workgroup adds the partials in the same fixed order (a few hundred to a few thousand floats out of
//            L2; a third launch to finish the norm would cost more), so all hold the same norm and coefficient bits;
//            then g * coef goes through torch's AdamW, in fp32 on the fp32 master, which for a bf16 parameter is a
//            separate array whose bf16 rounding the parameter receives.
//   scale  : g *= coef from the same partials, for the stand-alone clip_grad_norm_.
//
// Memory: an array that is 16-byte aligned moves in 16-byte vectors, any other one element by element (decided per
// array: the five arrays of a tensor need not share a misalignment), and the last numel % V elements are a scalar tail.
// Plain C++: no inline assembly, no atomics; -ffp-contract=off keeps one rounding per written operation.
#include "dfm_common.h"

using namespace dfm;

namespace {

constexpr int OT = DFM_OPTIM_THREADS;
constexpr int OC = DFM_OPTIM_CHUNK;
constexpr int OW = OT / 64;  // waves of a workgroup
static_assert(OC % OT == 0 && OC % 8 == 0 && OT % 64 == 0, "a chunk is whole 16-byte vectors of either type per lane");

// the sum of `acc` over the workgroup, the same bits in every lane: xor butterfly over the 64 lanes (after each level
// both partners hold a + b = b + a), then the waves' sums added in wave order by every lane.  `s_wave` is OW floats of
// LDS; the leading barrier lets a second call reuse it.
__device__ __forceinline__ float block_sum(float acc, float *s_wave)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = acc;
    __syncthreads();
    float total = s_wave[0];
#pragma unroll
    for (int w = 1; w < OW; ++w) total += s_wave[w];
    return total;
}

// V elements of T as floats: one 16-byte load when `aligned`, else element by element
template <typename T>
__device__ __forceinline__ void load_elems(const T *p, bool aligned, float (&f)[vec16<T>::N])
{
    if (aligned) {
        load16<T>(p, f);
    } else {
#pragma unroll
        for (int k = 0; k < vec16<T>::N; ++k) f[k] = elem<T>::load(p[k]);
    }
}

template <typename T>
__device__ __forceinline__ void store_elems(T *p, bool aligned, const float (&f)[vec16<T>::N])
{
    if (aligned) {
        store16<T>(p, f);
    } else {
#pragma unroll
        for (int k = 0; k < vec16<T>::N; ++k) p[k] = elem<T>::store(f[k]);
    }
}

// V floats of an fp32 state array (V = 4: one 16-byte vector, V = 8: two)
template <int V>
__device__ __forceinline__ void load_f32(const float *p, bool aligned, float (&f)[V])
{
    if (aligned) {
#pragma unroll
        for (int k = 0; k < V; k += 4) {
            const float4 q = *(const float4 *)(p + k);
            f[k] = q.x; f[k + 1] = q.y; f[k + 2] = q.z; f[k + 3] = q.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < V; ++k) f[k] = p[k];
    }
}

template <int V>
__device__ __forceinline__ void store_f32(float *p, bool aligned, const float (&f)[V])
{
    if (aligned) {
#pragma unroll
        for (int k = 0; k < V; k += 4) *(float4 *)(p + k) = make_float4(f[k], f[k + 1], f[k + 2], f[k + 3]);
    } else {
#pragma unroll
        for (int k = 0; k < V; ++k) p[k] = f[k];
    }
}

__device__ __forceinline__ bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// a device address of the table as a pointer the compiler knows to be global memory (global_load / global_store
// rather than the flat instructions an address of unknown origin gets)
template <typename T>
__device__ __forceinline__ T *global_ptr(int64_t address)
{
    return (T *)(__attribute__((address_space(1))) T *)(uintptr_t)address;
}

// the chunk of this workgroup: false when the pair names nothing (see the header)
struct Chunk {
    dfm_optim_tensor t;
    int64_t base;
    int count;
};

__device__ __forceinline__ bool my_chunk(const dfm_optim_tensor *table, int32_t num_tensors, const int2 *chunks,
                                         Chunk &c)
{
    const int2 at = chunks[blockIdx.x];
    if (at.x < 0 || at.x >= num_tensors || at.y < 0) return false;
    c.t = table[at.x];
    c.base = (int64_t)at.y * OC;
    if (c.base >= c.t.numel) return false;
    const int64_t left = c.t.numel - c.base;
    c.count = left < OC ? (int)left : OC;
    return true;
}

// ---- the norm ------------------------------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ float chunk_sqsum(const T *g, int count)
{
    constexpr int V = vec16<T>::N;
    const bool al = aligned16(g);
    const int groups = count / V;
    float acc = 0.0f;
    for (int i = threadIdx.x; i < groups; i += OT) {
        float f[V];
        load_elems<T>(g + (size_t)i * V, al, f);
#pragma unroll
        for (int k = 0; k < V; ++k) acc += f[k] * f[k];
    }
    const int e = groups * V + threadIdx.x;  // the tail: fewer than V elements, one per lane
    if (e < count) {
        const float x = elem<T>::load(g[e]);
        acc += x * x;
    }
    return acc;
}

__global__ __launch_bounds__(OT) void grad_sqnorm_kernel(const dfm_optim_tensor *__restrict__ table,
                                                         int32_t num_tensors, const int2 *__restrict__ chunks,
                                                         float *__restrict__ partials)
{
    __shared__ float s_wave[OW];
    Chunk c;
    float acc = 0.0f;
    if (my_chunk(table, num_tensors, chunks, c)) {  // uniform: every lane reaches the barriers below
        if (c.t.dtype == DFM_F32) acc = chunk_sqsum<float>(global_ptr<const float>(c.t.grad) + c.base, c.count);
        else acc = chunk_sqsum<bf16_t>(global_ptr<const bf16_t>(c.t.grad) + c.base, c.count);
    }
    const float total = block_sum(acc, s_wave);
    if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

// norm and clip coefficient from the partials, the same bits in every lane of every workgroup
__device__ __forceinline__ float clip_coef(const float *__restrict__ partials, int64_t num_chunks, float max_norm,
                                           float *__restrict__ norm_out, float *s_wave)
{
    float acc = 0.0f;
    for (int64_t i = threadIdx.x; i < num_chunks; i += OT) acc += partials[i];
    const float norm = sqrtf(block_sum(acc, s_wave));
    if (blockIdx.x == 0 && threadIdx.x == 0) norm_out[0] = norm;
    // torch's `max_norm / (total_norm + 1e-6)` is Tensor.__rtruediv__: the reciprocal, then the product (two roundings)
    const float coef = (1.0f / (norm + 1e-6f)) * max_norm;
    return coef > 1.0f ? 1.0f : coef;  // torch.clamp(max=1): a NaN stays a NaN
}

// ---- the update ----------------------------------------------------------------------------------------------------
struct Scalars {
    float coef, decay, neg_step, bc2_sqrt, w1, one_minus_w1, beta2, w2, eps;
};

__device__ __forceinline__ void adamw_one(float g0, float &p, float &m, float &v, const Scalars &s)
{
    const float g = g0 * s.coef;
    p = p * s.decay;
    const float d = g - m;
    m = s.w1 < 0.5f ? m + s.w1 * d : g - d * s.one_minus_w1;
    v = v * s.beta2 + (s.w2 * g) * g;
    const float denom = sqrtf(v) / s.bc2_sqrt + s.eps;
    p = p + (s.neg_step * m) / denom;
}

template <typename T>
__device__ __forceinline__ void adamw_chunk(const Chunk &c, const Scalars &s, bool zero_grads)
{
    constexpr int V = vec16<T>::N;
    constexpr bool NARROW = sizeof(T) != 4;  // the parameter is not its own fp32 master
    T *p = global_ptr<T>(c.t.param) + c.base;
    T *g = global_ptr<T>(c.t.grad) + c.base;
    float *m = global_ptr<float>(c.t.exp_avg) + c.base;
    float *v = global_ptr<float>(c.t.exp_avg_sq) + c.base;
    // fp32: the parameter; bf16: the master, or nullptr without one (p32 is then the widened parameter)
    float *w = !NARROW ? (float *)p : c.t.master ? global_ptr<float>(c.t.master) + c.base : nullptr;
    const bool al_p = aligned16(p), al_g = aligned16(g), al_m = aligned16(m), al_v = aligned16(v), al_w = aligned16(w);
    const int groups = c.count / V;
    for (int i = threadIdx.x; i < groups; i += OT) {
        const size_t e = (size_t)i * V;
        float fg[V], fm[V], fv[V], fw[V];
        load_elems<T>(g + e, al_g, fg);
        load_f32<V>(m + e, al_m, fm);
        load_f32<V>(v + e, al_v, fv);
        if (w) load_f32<V>(w + e, al_w, fw);
        else load_elems<T>(p + e, al_p, fw);
#pragma unroll
        for (int k = 0; k < V; ++k) adamw_one(fg[k], fw[k], fm[k], fv[k], s);
        store_f32<V>(m + e, al_m, fm);
        store_f32<V>(v + e, al_v, fv);
        if (w) store_f32<V>(w + e, al_w, fw);
        if (NARROW) store_elems<T>(p + e, al_p, fw);
        if (zero_grads) {
#pragma unroll
            for (int k = 0; k < V; ++k) fg[k] = 0.0f;
            store_elems<T>(g + e, al_g, fg);
        }
    }
    const int e = groups * V + threadIdx.x;
    if (e < c.count) {
        float fw = w ? w[e] : elem<T>::load(p[e]), fm = m[e], fv = v[e];
        adamw_one(elem<T>::load(g[e]), fw, fm, fv, s);
        m[e] = fm;
        v[e] = fv;
        if (w) w[e] = fw;
        if (NARROW) p[e] = elem<T>::store(fw);
        if (zero_grads) g[e] = elem<T>::store(0.0f);
    }
}

__global__ __launch_bounds__(OT) void adamw_step_kernel(const dfm_optim_tensor *__restrict__ table, int32_t num_tensors,
                                                        const int2 *__restrict__ chunks, int64_t num_chunks,
                                                        const float *__restrict__ partials, float max_norm,
                                                        float *__restrict__ norm_out, int32_t flags)
{
    __shared__ float s_wave[OW];
    const float coef = partials ? clip_coef(partials, num_chunks, max_norm, norm_out, s_wave) : 1.0f;
    Chunk c;
    if (!my_chunk(table, num_tensors, chunks, c)) return;
    Scalars s;
    s.coef = coef;
    s.decay = c.t.decay;
    s.neg_step = -c.t.step_size;
    s.bc2_sqrt = c.t.bc2_sqrt;
    s.w1 = c.t.lerp_weight;
    s.one_minus_w1 = 1.0f - c.t.lerp_weight;
    s.beta2 = c.t.beta2;
    s.w2 = c.t.one_minus_beta2;
    s.eps = c.t.eps;
    const bool zero = (flags & DFM_OPTIM_ZERO_GRADS) != 0;
    if (c.t.dtype == DFM_F32) adamw_chunk<float>(c, s, zero);
    else adamw_chunk<bf16_t>(c, s, zero);
}

template <typename T>
__device__ __forceinline__ void scale_chunk(T *g, int count, float coef)
{
    constexpr int V = vec16<T>::N;
    const bool al = aligned16(g);
    const int groups = count / V;
    for (int i = threadIdx.x; i < groups; i += OT) {
        float f[V];
        load_elems<T>(g + (size_t)i * V, al, f);
#pragma unroll
        for (int k = 0; k < V; ++k) f[k] = f[k] * coef;
        store_elems<T>(g + (size_t)i * V, al, f);
    }
    const int e = groups * V + threadIdx.x;
    if (e < count) g[e] = elem<T>::store(elem<T>::load(g[e]) * coef);
}

__global__ __launch_bounds__(OT) void grad_scale_kernel(const dfm_optim_tensor *__restrict__ table, int32_t num_tensors,
                                                        const int2 *__restrict__ chunks, int64_t num_chunks,
                                                        const float *__restrict__ partials, float max_norm,
                                                        float *__restrict__ norm_out)
{
    __shared__ float s_wave[OW];
    const float coef = clip_coef(partials, num_chunks, max_norm, norm_out, s_wave);
    Chunk c;
    if (!my_chunk(table, num_tensors, chunks, c)) return;
    if (c.t.dtype == DFM_F32) scale_chunk<float>(global_ptr<float>(c.t.grad) + c.base, c.count, coef);
    else scale_chunk<bf16_t>(global_ptr<bf16_t>(c.t.grad) + c.base, c.count, coef);
}

int check(const void *table, int32_t num_tensors, const void *chunks, int64_t num_chunks)
{
    if (num_tensors < 0 || num_chunks < 0) return set_error(DFM_ERR_INVALID_ARG, "negative size");
    if (num_chunks > 0x7fffffffll) return set_error(DFM_ERR_UNSUPPORTED, "more than 2^31 - 1 chunks");
    if (num_chunks > 0 && (!table || !chunks || num_tensors == 0))
        return set_error(DFM_ERR_INVALID_ARG, "chunks without a table");
    if (((uintptr_t)table & 7) || ((uintptr_t)chunks & 7))
        return set_error(DFM_ERR_INVALID_ARG, "the tables are 8-byte aligned");
    return DFM_OK;
}

}  // namespace

static_assert(sizeof(dfm_optim_tensor) == 88, "the table row the host fills: 6 int64, 2 int32, 8 float");

extern "C" DFM_API int dfm_grad_sqnorm(const void *table, int32_t num_tensors, const void *chunks, int64_t num_chunks,
                                       float *partials, void *stream)
{
    int rc = check(table, num_tensors, chunks, num_chunks);
    if (rc != DFM_OK) return rc;
    if (num_chunks == 0) return DFM_OK;
    if (!partials) return set_error(DFM_ERR_INVALID_ARG, "partials is NULL");
    hipLaunchKernelGGL(grad_sqnorm_kernel, dim3((unsigned)num_chunks), dim3(OT), 0, (hipStream_t)stream,
                       (const dfm_optim_tensor *)table, num_tensors, (const int2 *)chunks, partials);
    HIP_TRY(hipGetLastError());
    return DFM_OK;
}

extern "C" DFM_API int dfm_adamw_step(const void *table, int32_t num_tensors, const void *chunks, int64_t num_chunks,
                                      const float *partials, float max_norm, float *norm_out, int32_t flags,
                                      void *stream)
{
    int rc = check(table, num_tensors, chunks, num_chunks);
    if (rc != DFM_OK) return rc;
    if (flags & ~DFM_OPTIM_ZERO_GRADS) return set_error(DFM_ERR_INVALID_ARG, "unknown flags");
    if (partials && !norm_out) return set_error(DFM_ERR_INVALID_ARG, "partials without norm_out");
    if (num_chunks == 0) return DFM_OK;
    hipLaunchKernelGGL(adamw_step_kernel, dim3((unsigned)num_chunks), dim3(OT), 0, (hipStream_t)stream,
                       (const dfm_optim_tensor *)table, num_tensors, (const int2 *)chunks, num_chunks, partials,
                       max_norm, norm_out, flags);
    HIP_TRY(hipGetLastError());
    return DFM_OK;
}

extern "C" DFM_API int dfm_grad_scale(const void *table, int32_t num_tensors, const void *chunks, int64_t num_chunks,
                                      const float *partials, float max_norm, float *norm_out, void *stream)
{
    int rc = check(table, num_tensors, chunks, num_chunks);
    if (rc != DFM_OK) return rc;
    if (num_chunks == 0) return DFM_OK;
    if (!partials || !norm_out) return set_error(DFM_ERR_INVALID_ARG, "partials or norm_out is NULL");
    hipLaunchKernelGGL(grad_scale_kernel, dim3((unsigned)num_chunks), dim3(OT), 0, (hipStream_t)stream,
                       (const dfm_optim_tensor *)table, num_tensors, (const int2 *)chunks, num_chunks, partials,
                       max_norm, norm_out);
    HIP_TRY(hipGetLastError());
    return DFM_OK;
}
