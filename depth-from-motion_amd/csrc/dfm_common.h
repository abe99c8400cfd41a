// dfm_common.h -- device helpers and runtime declarations shared by every translation unit.
//
// Numerics contract (DESIGN.md "Numerics"): all coordinate arithmetic is fp32
// with exactly one IEEE rounding per reference torch op.  This translation
// unit is compiled with -ffp-contract=off; fused multiply-adds appear ONLY
// where written as __builtin_fmaf (they restate the k-ordered fma chain of
// torch's fp32 (N,4)@(4,4) CPU matmul and of ATen's bilinear accumulation).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "dfm_hip.h"

namespace dfm {

// records the thread-local message dfm_last_error() returns; defined in
// runtime.hip, shared by every translation unit of the library
int set_error(int code, const char *msg);
int set_errorf(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
// hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per (device, kernel): defined in
// runtime.hip (mutex-protected map), used by every kernel with more than 64 KB of LDS
int ensure_dynamic_lds(const void *kern, int lds_bytes);
// records the start (stop=false) / stop event of a timed launch when dfm_profile_begin
// is active; the start call returns whether this launch is being timed (runtime.hip)
bool profile_mark(void *stream, bool stop);

// a failing HIP call ends the entry point with DFM_ERR_HIP and "<call>: <HIP's message>"
#define HIP_TRY(expr)                                                                             \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return dfm::set_errorf(DFM_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_));          \
    } while (0)

typedef unsigned short bf16_t;  // raw bfloat16 bits

__device__ __forceinline__ float bf16_to_f32(bf16_t v)
{
    return __uint_as_float(((uint32_t)v) << 16);
}

// round-to-nearest-even in hardware (v_cvt_pk_bf16_f32 on gfx950: one operation; the integer
// add-and-shift it replaces cost seven); a NaN stays a quiet NaN (torch's c10::BFloat16 canonicalises
// it to 0x7fc0, the hardware keeps its sign -- NaN either way)
__device__ __forceinline__ bf16_t f32_to_bf16(float f)
{
    const __bf16 h = (__bf16)f;
    bf16_t u;
    __builtin_memcpy(&u, &h, 2);
    return u;
}

// two floats -> packed bf16x2 (lo = a, hi = b), round-to-nearest-even
// (v_cvt_pk_bf16_f32 on gfx950)
typedef __bf16 bf16x2_vec __attribute__((ext_vector_type(2)));
typedef float f32x2_vec __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t pack_bf16x2(float a, float b)
{
    f32x2_vec f = {a, b};
    bf16x2_vec h = __builtin_convertvector(f, bf16x2_vec);
    uint32_t u;
    __builtin_memcpy(&u, &h, 4);
    return u;
}

// MFMA 32x32 accumulator rows -> 16-byte stores.  A lane of the 32x32 accumulator layout holds, per pixel, four
// groups gq of 4 consecutive channels (8 gq + 4 half + 0..3): packed to bf16 that is four 8-byte pieces a pixel and
// lane, 16 bytes apart -- four store instructions whose 64 lanes write 8 bytes each (profiles/r06_c8_*: the pattern
// costs 10-18 % of a convolution).  The two halves of the wave hold complementary pieces of the SAME pixel, so they
// trade: lanes 0..31 give away groups 1 and 3 and receive the partner's 0 and 2 (v_permlane32_swap: one instruction
// per dword, no LDS), after which lane (pixel, half) owns channels [16 p + 8 half, + 8) for p = 0, 1 -- two 16-byte
// stores, the two halves together 32 contiguous bytes per pixel and instruction.
// pk[gq] = {ch 8gq+4half+0|1, ch 8gq+4half+2|3} on entry; on return q[p] = the 8 channels 16p + 8half .. + 7.
typedef uint32_t dfm_u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t dfm_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void acc_rows_to_16B(const dfm_u32x2 (&pk)[4], dfm_u32x4 (&q)[2])
{
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        // first operand: group 2p (kept by the low half), second: group 2p + 1 (kept by the high half)
        const auto x = __builtin_amdgcn_permlane32_swap(pk[2 * p].x, pk[2 * p + 1].x, false, false);
        const auto y = __builtin_amdgcn_permlane32_swap(pk[2 * p].y, pk[2 * p + 1].y, false, false);
        // low half: {own 2p, partner's 2p}; high half: {partner's 2p + 1, own 2p + 1}
        q[p] = dfm_u32x4{x[0], y[0], x[1], y[1]};
    }
}

template <typename T> struct elem;
template <> struct elem<float> {
    static constexpr int CB = 4;  // elements per 16-byte channel block
    static __device__ __forceinline__ float load(float v) { return v; }
    static __device__ __forceinline__ float store(float v) { return v; }
};
template <> struct elem<bf16_t> {
    static constexpr int CB = 8;
    static __device__ __forceinline__ float load(bf16_t v) { return bf16_to_f32(v); }
    static __device__ __forceinline__ bf16_t store(float v) { return f32_to_bf16(v); }
};

// Host side: a launch templated on the element type, or on a bool, written ONCE -- f is a generic lambda that
// takes a value of the element type (float{} / bf16_t{}: T = decltype of it) or a std::bool_constant
// (its ::value is a constant expression).  dtype has been validated (DFM_F32 or DFM_BF16) before.
// Both return what f returns, so a launch that can fail before it starts (ensure_dynamic_lds) hands its status out:
// `const int rc = by_dtype(dtype, [&](auto t) { ...; return (int)DFM_OK; });`  (a new entry point).
template <typename F>
inline decltype(auto) by_dtype(int32_t dtype, F &&f)
{
    if (dtype == DFM_F32) return f(float{});
    else return f(bf16_t{});
}
template <typename F>
inline decltype(auto) by_bool(bool on, F &&f)
{
    if (on) return f(std::true_type{});
    else return f(std::false_type{});
}
// the element-type check of every entry point that takes a dtype
inline int check_dtype(int32_t dtype)
{
    if (dtype == DFM_F32 || dtype == DFM_BF16) return DFM_OK;
    return set_error(DFM_ERR_UNSUPPORTED, "dtype must be DFM_F32 or DFM_BF16");
}

// unpack one 16-byte channel block into CB floats
__device__ __forceinline__ void unpack16(const uint4 &q, float (&f)[4])
{
    f[0] = __uint_as_float(q.x);
    f[1] = __uint_as_float(q.y);
    f[2] = __uint_as_float(q.z);
    f[3] = __uint_as_float(q.w);
}
__device__ __forceinline__ void unpack16(const uint4 &q, float (&f)[8])
{
    f[0] = __uint_as_float(q.x << 16);
    f[1] = __uint_as_float(q.x & 0xffff0000u);
    f[2] = __uint_as_float(q.y << 16);
    f[3] = __uint_as_float(q.y & 0xffff0000u);
    f[4] = __uint_as_float(q.z << 16);
    f[5] = __uint_as_float(q.z & 0xffff0000u);
    f[6] = __uint_as_float(q.w << 16);
    f[7] = __uint_as_float(q.w & 0xffff0000u);
}

// 16-byte vector of T <-> floats (4 fp32 / 8 bf16)
template <typename T> struct vec16;
template <> struct vec16<float> { static constexpr int N = 4; };
template <> struct vec16<bf16_t> { static constexpr int N = 8; };

template <typename T>
__device__ __forceinline__ void load16(const T *p, float (&f)[vec16<T>::N])
{
    const uint4 q = *(const uint4 *)p;
    unpack16(q, f);
}

template <typename T>
__device__ __forceinline__ void store16(T *p, const float (&f)[vec16<T>::N])
{
    if constexpr (sizeof(T) == 4) {
        *(uint4 *)p = make_uint4(__float_as_uint(f[0]), __float_as_uint(f[1]), __float_as_uint(f[2]),
                                 __float_as_uint(f[3]));
    } else {
        *(uint4 *)p = make_uint4(pack_bf16x2(f[0], f[1]), pack_bf16x2(f[2], f[3]),
                                 pack_bf16x2(f[4], f[5]), pack_bf16x2(f[6], f[7]));
    }
}

// trilinear x-scale upsample with align_corners=True, ATen's index / weight arithmetic
// (nn.Upsample in DepthHead.forward, dense_heads/depth_head.py:205; shared by the depth-head
// kernels and the fused FrustumToVoxel, which must produce the same bits)
struct UpIdx {
    int i0, i1;
    float w0, w1;
};

__device__ __forceinline__ UpIdx up_index(int i, int in, int out)
{
    UpIdx u;
    const float scale = out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.0f;
    const float real = scale * (float)i;
    int a = (int)floorf(real);
    a = min(a, in - 1);
    float l = real - (float)a;
    l = fminf(fmaxf(l, 0.0f), 1.0f);
    u.i0 = a;
    u.i1 = min(a + 1, in - 1);
    u.w1 = l;
    u.w0 = 1.0f - l;
    return u;
}

// exp(x) for x <= 0 (a logit minus its column maximum) -- the softmax of DepthHead and of the fused
// FrustumToVoxel share it, so the two stay bit-identical.  x * log2(e) as a two-word product, the
// integer part split off before the low word is added (so the low word survives for large |x|), the
// hardware exp2 on the fraction and a ldexp: ~9 VALU operations, within 1 ulp of libm's expf (which
// spends half of its ~15 operations on the overflow / underflow cases this argument cannot reach).
// NaN propagates; anything below -128 (-inf included) gives exp(-128) scaled out of range = 0.
__device__ __forceinline__ float exp_nonpos(float x)
{
    x = x < -128.0f ? -128.0f : x;
    const float ph = x * 1.44269504088896340736f;
    const float pl = __builtin_fmaf(x, 1.92596299112661746e-8f, __builtin_fmaf(x, 1.44269504088896340736f, -ph));
    const float e = __builtin_rintf(ph);
    const float a = (ph - e) + pl;
    return __builtin_ldexpf(__builtin_amdgcn_exp2f(a), (int)e);
}

__device__ __forceinline__ float lerp_fma(float w0, float a, float w1, float b)
{
    return __builtin_fmaf(w0, a, w1 * b);
}

// row of (v @ M^T): sum_k v[k]*M[k], k-ordered fma chain
// (torch fp32 mm on CPU; reference call sites utils.py:208,246 and
//  dfm_backbone.py:270)
__device__ __forceinline__ float dot4_chain(float a0, float a1, float a2, float a3,
                                            const float *__restrict__ M)
{
    float acc = a0 * M[0];
    acc = __builtin_fmaf(a1, M[1], acc);
    acc = __builtin_fmaf(a2, M[2], acc);
    acc = __builtin_fmaf(a3, M[3], acc);
    return acc;
}

// (n, C, P) planar -> (n, P, Cp) pixel-major, Cp = C rounded up to a whole number of
// 16-byte channel blocks (zero padded): all channels of one sampled pixel / voxel are
// one contiguous run, so a tap is Cp*sizeof(T)/16 adjacent 16-byte loads instead of
// C scalar loads a whole plane apart.  64 pixels x 32 channels per workgroup through
// an LDS tile: global reads run along pixels, global writes along channels.
// grid = (ceil(P/64), ceil(Cp/32), n)
template <typename T>
__global__ __launch_bounds__(256) void pack_pixel_major_kernel(const T *__restrict__ src,
                                                               T *__restrict__ dst, int C, int Cp,
                                                               long long P)
{
    __shared__ T tile[32][64 + 1];
    const long long p0 = (long long)blockIdx.x * 64;
    const int c0 = blockIdx.y * 32;
    const size_t n = blockIdx.z;
    {
        const int p = threadIdx.x & 63, cc = threadIdx.x >> 6;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int c = cc + 4 * k;
            T v = T(0);
            if (c0 + c < C && p0 + p < P) v = src[(n * C + c0 + c) * (size_t)P + p0 + p];
            tile[c][p] = v;
        }
    }
    __syncthreads();
    {
        const int c = threadIdx.x & 31, pp = threadIdx.x >> 5;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int p = pp + 8 * k;
            if (c0 + c < Cp && p0 + p < P) dst[(n * (size_t)P + p0 + p) * Cp + c0 + c] = tile[c][p];
        }
    }
}

// the way back for gradients accumulated pixel-major (coalesced atomics):
// dst (n, C, P) += src (n, P, C): 64 pixels x 32 channels per workgroup through LDS
template <typename F = float>
__global__ __launch_bounds__(256) void add_from_pixel_major_kernel(const float *__restrict__ src,
                                                                   float *__restrict__ dst, int C,
                                                                   long long P)
{
    __shared__ float tile[64][32 + 1];
    const long long p0 = (long long)blockIdx.x * 64;
    const int c0 = blockIdx.y * 32;
    const size_t n = blockIdx.z;
    {
        const int c = threadIdx.x & 31, pp = threadIdx.x >> 5;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int p = pp + 8 * k;
            tile[p][c] = (c0 + c < C && p0 + p < P) ? src[(n * (size_t)P + p0 + p) * C + c0 + c] : 0.0f;
        }
    }
    __syncthreads();
    {
        const int p = threadIdx.x & 63, cc = threadIdx.x >> 6;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int c = cc + 4 * k;
            if (c0 + c < C && p0 + p < P) {
                float *q = dst + (n * C + c0 + c) * (size_t)P + p0 + p;
                *q = *q + tile[p][c];
            }
        }
    }
}

}  // namespace dfm
