// runtime.hip -- what every translation unit of the library shares at run time: the thread-local error
// string behind dfm_last_error(), the per-device cache of the dynamic-LDS attribute, the event profiler
// that times the volume-writing launches, and the two probes that tell which kind of part a process
// landed on.
//
// Kernels
//   store_probe_kernel : writes zeros in the tile kernel's store pattern (dfm_store_probe).
//   clock_probe_kernel : the shader clock sustained with every CU busy (dfm_clock_probe).
#include "dfm_common.h"

#include <stdarg.h>
#include <stdio.h>

#include <algorithm>
#include <map>
#include <mutex>
#include <vector>

using namespace dfm;

namespace {

thread_local char g_err[512] = "";

// optional per-launch timing of the dominant (volume-writing) kernel with HIP
// events on the caller's stream (bench.py's roofline leg)
struct Profiler {
    std::mutex mu;
    bool on = false;
    std::vector<hipEvent_t> ev;  // pairs
    int used = 0;
} g_prof;

}  // namespace

int dfm::set_error(int code, const char *msg)
{
    snprintf(g_err, sizeof(g_err), "%s", msg);
    return code;
}

int dfm::set_errorf(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per (device, kernel, size) instead of on
// every launch.  The attribute is per DEVICE: every translation unit of the library goes through
// this one (device, kernel) map, so a second GPU driven from the same process gets its own call.
int dfm::ensure_dynamic_lds(const void *kern, int lds_bytes)
{
    static std::mutex mu;
    static std::map<std::pair<int, const void *>, int> seen;
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(mu);
    int &have = seen[std::make_pair(dev, kern)];
    if (lds_bytes > have) {
        HIP_TRY(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes));
        have = lds_bytes;
    }
    return DFM_OK;
}

bool dfm::profile_mark(void *stream, bool stop)
{
    hipStream_t st = (hipStream_t)stream;
    std::lock_guard<std::mutex> lk(g_prof.mu);
    if (!stop) {
        if (!(g_prof.on && g_prof.used + 2 <= (int)g_prof.ev.size())) return false;
        (void)hipEventRecord(g_prof.ev[g_prof.used], st);
        return true;
    }
    if (!(g_prof.on && g_prof.used + 2 <= (int)g_prof.ev.size())) return false;
    (void)hipEventRecord(g_prof.ev[g_prof.used + 1], st);
    g_prof.used += 2;
    return true;
}

extern "C" {

DFM_API int dfm_version(void) { return 3; }
DFM_API const char *dfm_last_error(void) { return g_err; }

DFM_API int dfm_profile_begin(int max_launches)
{
    if (max_launches <= 0 || max_launches > 65536)
        return set_error(DFM_ERR_INVALID_ARG, "max_launches out of range");
    std::lock_guard<std::mutex> lk(g_prof.mu);
    for (hipEvent_t e : g_prof.ev) (void)hipEventDestroy(e);
    g_prof.ev.assign(2 * (size_t)max_launches, nullptr);
    for (auto &e : g_prof.ev) HIP_TRY(hipEventCreate(&e));
    g_prof.used = 0;
    g_prof.on = true;
    return DFM_OK;
}

DFM_API int dfm_profile_end(double *total_ms, int *launches)
{
    if (!total_ms || !launches) return set_error(DFM_ERR_INVALID_ARG, "NULL output");
    std::lock_guard<std::mutex> lk(g_prof.mu);
    g_prof.on = false;
    double sum = 0.0;
    for (int i = 0; i + 1 < g_prof.used; i += 2) {
        HIP_TRY(hipEventSynchronize(g_prof.ev[i + 1]));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, g_prof.ev[i], g_prof.ev[i + 1]));
        sum += ms;
    }
    *total_ms = sum;
    *launches = g_prof.used / 2;
    for (hipEvent_t e : g_prof.ev) (void)hipEventDestroy(e);
    g_prof.ev.clear();
    g_prof.used = 0;
    return DFM_OK;
}

// Which part did the process land on?  The tile kernel's store stream -- every workgroup writes a 4 KiB
// run into each of the 2C channel planes of a sample, planes D*h*w elements apart -- sustains 5.1-5.3 TB/s
// on most MI355X parts and ~3.9-4.1 TB/s on others (same binary, same clocks; a linear fill runs at
// 6.8 TB/s on both: profiles/archive/r03_c17_*).  This probe writes zeros in exactly that pattern so that a
// bench line can say which kind of part produced it.  `out` is overwritten with zeros.
__global__ __launch_bounds__(256) void store_probe_kernel(uint4 *__restrict__ out, long long plane_vec,
                                                          long long runs_per_plane, int planes, int pieces, int group)
{
    // block = (run, plane group, sample), run fastest: `pieces` x (256 lanes x 16 B = 4 KiB) contiguous per
    // plane; walks the `group` planes of its plane group (group == planes: the tile kernel's pattern)
    typedef unsigned int probe_u32x4 __attribute__((ext_vector_type(4)));
    const long long run = blockIdx.x % runs_per_plane;
    const int pg = (int)(blockIdx.x / runs_per_plane);
    probe_u32x4 *p = (probe_u32x4 *)out + ((size_t)blockIdx.y * planes + (size_t)pg * group) * plane_vec +
                     run * 256 * pieces + threadIdx.x;
    const probe_u32x4 z = {0u, 0u, 0u, 0u};
    const int n = min(group, planes - pg * group);
    for (int c = 0; c < n; ++c)
        for (int k = 0; k < pieces; ++k) __builtin_nontemporal_store(z, p + (size_t)c * plane_vec + k * 256);
}

DFM_API int dfm_store_probe(void *out, int32_t batch, int32_t planes, int64_t plane_bytes, int32_t run_bytes,
                            int32_t planes_per_workgroup, void *stream)
{
    if (!out || batch <= 0 || planes <= 0 || plane_bytes < 4096 || ((uintptr_t)out & 15) || (plane_bytes & 15))
        return set_error(DFM_ERR_INVALID_ARG, "store probe: aligned buffer of batch x planes x plane_bytes");
    const int pieces = run_bytes > 0 ? run_bytes / 4096 : 1;  // 0: the tile kernel's 4 KiB runs
    if (pieces < 1 || pieces * 4096 != (run_bytes > 0 ? run_bytes : 4096) || plane_bytes < 4096ll * pieces)
        return set_error(DFM_ERR_INVALID_ARG, "store probe: run_bytes must be a multiple of 4096");
    const int group = planes_per_workgroup > 0 ? std::min(planes_per_workgroup, planes) : planes;  // 0: all planes
    const long long plane_vec = plane_bytes / 16, runs = plane_vec / (256 * pieces);  // (a plane's tail is skipped)
    const long long nblk = runs * ((planes + group - 1) / group);
    if (nblk > 2147483647ll || batch > 65535) return set_error(DFM_ERR_UNSUPPORTED, "store probe: grid too large");
    hipLaunchKernelGGL(store_probe_kernel, dim3((unsigned)nblk, batch), dim3(256), 0, (hipStream_t)stream,
                       (uint4 *)out, plane_vec, runs, planes, pieces, group);
    HIP_TRY(hipGetLastError());
    return DFM_OK;
}

// the shader clock this part sustains with every CU busy: cycles (s_memtime) and 100 MHz reference
// ticks (s_memrealtime) across `iterations` dependent FMAs per lane, written by workgroup 0
__global__ __launch_bounds__(256) void clock_probe_kernel(unsigned long long *out, int iterations, float seed)
{
    const unsigned long long c0 = __builtin_readcyclecounter(), r0 = __builtin_amdgcn_s_memrealtime();
    float x0 = seed + threadIdx.x, x1 = seed * 2.0f, x2 = seed * 3.0f, x3 = seed * 4.0f;
    for (int i = 0; i < iterations; ++i) {
        x0 = __builtin_fmaf(x0, 0.999f, 0.5f);
        x1 = __builtin_fmaf(x1, 0.998f, 0.25f);
        x2 = __builtin_fmaf(x2, 0.997f, 0.125f);
        x3 = __builtin_fmaf(x3, 0.996f, 0.0625f);
    }
    const unsigned long long c1 = __builtin_readcyclecounter(), r1 = __builtin_amdgcn_s_memrealtime();
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        out[0] = c1 - c0;
        out[1] = r1 - r0;
    }
    if (x0 + x1 + x2 + x3 == 12345.678f) out[2] = 1;  // keeps the loop
}

DFM_API int dfm_clock_probe(void *out3, int32_t iterations, void *stream)
{
    if (!out3 || iterations <= 0 || ((uintptr_t)out3 & 7)) return set_error(DFM_ERR_INVALID_ARG, "clock probe: 3 x u64 device buffer");
    hipLaunchKernelGGL(clock_probe_kernel, dim3(256 * 8), dim3(256), 0, (hipStream_t)stream, (unsigned long long *)out3,
                       iterations, 1.0f);
    HIP_TRY(hipGetLastError());
    return DFM_OK;
}

}  // extern "C"
