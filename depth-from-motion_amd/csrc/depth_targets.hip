// depth_targets.hip -- the two maps DepthHead.loss is trained against, and the box-membership operators
// (reference: GenerateDepthMap, mmdet3d/datasets/pipelines/transforms_3d.py:55-118; Calibration.rect_to_img,
// core/camera/calibration.py:230-240; depth_map_in_boxes_cpu / points_in_boxes_cpu_idmap, datasets/utils.py:403-455;
// points_img2cam, core/bbox/structures/utils.py:217-248; mmcv's points_in_boxes_part / _all).
//
//   scatter : one lane per LiDAR point, all samples in one launch (grid.y = sample, so everything per sample is
//             wave-uniform).  The point is projected in fp64 and, if it lands in the image, written with a 64-bit
//             integer atomicMax of ((index + 1) << 32) | bits(float(depth)): the reference's fancy-index assignment
//             lets the highest point index win, and an integer max does not depend on arrival order.
//   resolve : one lane per pixel.  depth = the key's low word (or the caller's depth map); where depth > 0 the pixel
//             is unprojected in fp64, rounded to fp32 and tested against the sample's boxes, staged in LDS.
//   member  : one lane per point against the sample's boxes, staged in LDS: lowest index, highest index, or a 0/1 row.
// Plain C++: no inline assembly, no floating-point atomics; every output element is written exactly once.
#include <algorithm>

#include "box_membership.h"
#include "dfm_common.h"

using namespace dfm;

namespace {

constexpr int DT_THREADS = 256;
constexpr int DT_BOX_CHUNK = 256;  // boxes staged in LDS at a time (8 KB)
constexpr int DT_CAM = DFM_DEPTH_CAM_DOUBLES;

// ((a * m0 + b * m1) + c * m2) + d * m3 in fp64, one rounding per operation (the translation unit is compiled with
// -ffp-contract=off)
__device__ __forceinline__ double dot4(double a, double b, double c, double d, const double *m)
{
    return ((a * m[0] + b * m[1]) + c * m[2]) + d * m[3];
}

__global__ __launch_bounds__(DT_THREADS) void depth_scatter_kernel(dfm_depth_targets_desc d,
                                                                   const float *__restrict__ points,
                                                                   const double *__restrict__ cam,
                                                                   unsigned long long *__restrict__ keys)
{
    const int b = blockIdx.y;
    const int64_t n0 = d.point_off[b], n = d.point_off[b + 1] - n0;
    const int64_t i = (int64_t)blockIdx.x * DT_THREADS + threadIdx.x;
    if (i >= n) return;
    const float *p = points + (n0 + i) * d.point_stride;
    const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
    // homo_pseudo_points @ pseudo2cam_T (transforms_3d.py:69-76), every product written out: a non-finite
    // coordinate spoils the columns the reference's matrix product spoils
    const double X = ((x * 0.0 + y * -1.0) + z * 0.0) + 0.0;
    const double Y = ((x * 0.0 + y * 0.0) + z * -1.0) + 0.0;
    const double Z = ((x * 1.0 + y * 0.0) + z * 0.0) + 0.0;
    const double *P = cam + (size_t)b * DT_CAM;
    const double h0 = dot4(X, Y, Z, 1.0, P), h1 = dot4(X, Y, Z, 1.0, P + 4), h2 = dot4(X, Y, Z, 1.0, P + 8);
    const double u = h0 / Z, v = h1 / Z;  // the divisor is the rectified Z, not h2 (calibration.py:237)
    const double depth = h2 - P[11];
    const double ru = rint(u), rv = rint(v);  // half to even, as np.round
    // a NaN fails every comparison; -0.0 >= 0 holds, as the reference's int64 0 does
    const bool keep = isfinite(u) && isfinite(v) && rv >= 0.0 && rv < (double)d.img_h[b] && ru >= 0.0 &&
                      ru < (double)d.img_w[b];
    if (!keep) return;
    const int ix = (int)ru, iy = (int)rv;  // < img_w <= pad_w, < img_h <= pad_h: checked on the host side
    const unsigned long long key =
        ((unsigned long long)(i + 1) << 32) | (unsigned long long)__float_as_uint((float)depth);
    atomicMax(keys + ((size_t)b * d.pad_h + iy) * d.pad_w + ix, key);
}

__global__ __launch_bounds__(DT_THREADS) void depth_resolve_kernel(dfm_depth_targets_desc d,
                                                                   const unsigned long long *__restrict__ keys,
                                                                   const float *__restrict__ depth_in,
                                                                   const double *__restrict__ cam,
                                                                   const float *__restrict__ boxes, float ratio,
                                                                   float distance, float *__restrict__ depth_out,
                                                                   int32_t *__restrict__ fgmask)
{
    __shared__ PtBox s_box[DT_BOX_CHUNK];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int64_t hw = (int64_t)d.pad_h * d.pad_w;
    const int64_t pix = (int64_t)blockIdx.x * DT_THREADS + tid;
    const bool live = pix < hw;
    float depth = 0.0f;
    if (live) {
        const size_t at = (size_t)b * hw + pix;
        if (keys) {
            const unsigned long long key = keys[at];
            depth = key ? __uint_as_float((unsigned int)(key & 0xffffffffull)) : 0.0f;
        } else {
            depth = depth_in[at];
        }
        if (depth_out) depth_out[at] = depth;
    }
    if (!fgmask) return;  // uniform: a kernel argument
    const bool on = live && depth > 0.0f;  // depth_map > 0: a NaN or a negative depth gets no id (utils.py:409)
    float px = 0.0f, py = 0.0f, pz = 0.0f;
    if (on) {
        const int iy = (int)(pix / d.pad_w), ix = (int)(pix - (int64_t)iy * d.pad_w);
        const double dd = (double)depth;
        const double hx = (double)ix * dd, hy = (double)iy * dd;  // unnormed_xys (utils.py:237)
        const double *inv = cam + (size_t)b * DT_CAM + 12;       // inverse of cam2img padded to 4x4, row-major
        const double cx = dot4(hx, hy, dd, 1.0, inv), cy = dot4(hx, hy, dd, 1.0, inv + 4),
                     cz = dot4(hx, hy, dd, 1.0, inv + 8);
        px = (float)cz; py = (float)(-cx); pz = (float)(-cy);   // rect -> pseudo-LiDAR, then .float() (utils.py:419)
    }
    const int64_t m0 = d.box_off[b];
    const int m = (int)(d.box_off[b + 1] - m0);
    int id = 0;
    for (int t0 = 0; t0 < m; t0 += DT_BOX_CHUNK) {  // uniform trip count: every lane reaches the barriers
        const int nb = min(DT_BOX_CHUNK, m - t0);
        __syncthreads();
        if (tid < nb) s_box[tid] = pt_box(boxes + (size_t)(m0 + t0 + tid) * 7, false, ratio, distance);
        __syncthreads();
        if (on)
            for (int t = 0; t < nb; ++t)
                if (pt_in_box(px, py, pz, s_box[t])) id = t0 + t + 1;  // ascending: the highest index stays
    }
    if (live) fgmask[(size_t)b * hw + pix] = id;
}

template <int MODE>
__global__ __launch_bounds__(DT_THREADS) void points_in_boxes_kernel(int64_t n, int32_t m,
                                                                     const float *__restrict__ points,
                                                                     const float *__restrict__ boxes,
                                                                     int32_t *__restrict__ out)
{
    __shared__ PtBox s_box[DT_BOX_CHUNK];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * DT_THREADS + tid;
    const bool live = i < n;
    float px = 0.0f, py = 0.0f, pz = 0.0f;
    if (live) {
        const float *p = points + ((size_t)b * n + i) * 3;
        px = p[0]; py = p[1]; pz = p[2];
    }
    int id = -1;
    int32_t *row = MODE == DFM_PIB_ALL && live ? out + ((size_t)b * n + i) * m : nullptr;
    for (int t0 = 0; t0 < m; t0 += DT_BOX_CHUNK) {
        const int nb = min(DT_BOX_CHUNK, m - t0);
        __syncthreads();
        if (tid < nb) s_box[tid] = pt_box(boxes + ((size_t)b * m + t0 + tid) * 7, false);
        __syncthreads();
        if (!live) continue;
        for (int t = 0; t < nb; ++t) {
            const bool in = pt_in_box(px, py, pz, s_box[t]);
            if (MODE == DFM_PIB_ALL) row[t0 + t] = in ? 1 : 0;
            else if (MODE == DFM_PIB_IDMAP) id = in ? t0 + t : id;
            else if (in && id < 0) id = t0 + t;  // part: the first box that holds the point
        }
    }
    if (MODE != DFM_PIB_ALL && live) out[(size_t)b * n + i] = id;
}

int check(const dfm_depth_targets_desc *d)
{
    if (!d) return set_error(DFM_ERR_INVALID_ARG, "desc is NULL");
    if (d->batch <= 0 || d->batch > DFM_DEPTH_MAX_BATCH)
        return set_errorf(DFM_ERR_INVALID_ARG, "batch must be 1..%d", DFM_DEPTH_MAX_BATCH);
    if (d->pad_h <= 0 || d->pad_w <= 0) return set_error(DFM_ERR_INVALID_ARG, "non-positive pad_h / pad_w");
    if ((long long)d->pad_h * d->pad_w > 0x7fffffffll) return set_error(DFM_ERR_UNSUPPORTED, "map too large");
    if (d->point_stride < 3) return set_error(DFM_ERR_INVALID_ARG, "point_stride < 3: a point is x, y, z, ...");
    if (d->point_off[0] != 0 || d->box_off[0] != 0)
        return set_error(DFM_ERR_INVALID_ARG, "an offset table starts at 0");
    for (int b = 0; b < d->batch; ++b) {
        if (d->img_h[b] < 0 || d->img_w[b] < 0 || d->img_h[b] > d->pad_h || d->img_w[b] > d->pad_w)
            return set_errorf(DFM_ERR_INVALID_ARG, "sample %d: img_shape %d x %d does not fit pad_shape %d x %d", b,
                              d->img_h[b], d->img_w[b], d->pad_h, d->pad_w);
        const int64_t n = d->point_off[b + 1] - d->point_off[b], m = d->box_off[b + 1] - d->box_off[b];
        if (n < 0 || m < 0) return set_error(DFM_ERR_INVALID_ARG, "an offset table is non-decreasing");
        if (n > 0xfffffffell)
            return set_error(DFM_ERR_UNSUPPORTED, "more points in a sample than the key's index word holds (2^32 - 2)");
        if (m > 0x7ffffffell)
            return set_error(DFM_ERR_UNSUPPORTED, "more boxes in a sample than the int32 id holds (2^31 - 2)");
    }
    return DFM_OK;
}

}  // namespace

extern "C" DFM_API size_t dfm_depth_targets_workspace_bytes(const dfm_depth_targets_desc *d)
{
    if (check(d) != DFM_OK) return 0;
    return (size_t)d->batch * d->pad_h * d->pad_w * sizeof(unsigned long long);
}

extern "C" DFM_API int dfm_depth_scatter(const dfm_depth_targets_desc *d, const float *points, const double *cam,
                                         void *keys, size_t keys_bytes, void *stream)
{
    int rc = check(d);
    if (rc != DFM_OK) return rc;
    const size_t need = dfm_depth_targets_workspace_bytes(d);
    if (!keys || keys_bytes < need)
        return set_errorf(DFM_ERR_WORKSPACE, "the key map needs %zu bytes, got %zu", need, keys ? keys_bytes : 0);
    if ((uintptr_t)keys % 8) return set_error(DFM_ERR_INVALID_ARG, "the key map is 8-byte aligned");
    if (!cam) return set_error(DFM_ERR_INVALID_ARG, "cam is NULL");
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(keys, 0, need, st));
    int64_t most = 0;
    for (int b = 0; b < d->batch; ++b) most = std::max<int64_t>(most, d->point_off[b + 1] - d->point_off[b]);
    if (most == 0) return DFM_OK;
    if (!points) return set_error(DFM_ERR_INVALID_ARG, "points is NULL");
    const int64_t blocks = (most + DT_THREADS - 1) / DT_THREADS;
    hipLaunchKernelGGL(depth_scatter_kernel, dim3((unsigned)blocks, d->batch), dim3(DT_THREADS), 0, st, *d, points,
                       cam, (unsigned long long *)keys);
    HIP_TRY(hipGetLastError());
    return DFM_OK;
}

extern "C" DFM_API int dfm_depth_resolve(const dfm_depth_targets_desc *d, const void *keys, const float *depth_in,
                                         const double *cam, const float *boxes, float expand_ratio,
                                         float expand_distance, float *depth_out, int32_t *fgmask, void *stream)
{
    int rc = check(d);
    if (rc != DFM_OK) return rc;
    if ((keys == nullptr) == (depth_in == nullptr))
        return set_error(DFM_ERR_INVALID_ARG, "exactly one of keys and depth_in is given");
    if (!depth_out && !fgmask) return set_error(DFM_ERR_INVALID_ARG, "no output at all");
    if (fgmask && !cam) return set_error(DFM_ERR_INVALID_ARG, "cam is NULL");
    if (fgmask && d->box_off[d->batch] > 0 && !boxes) return set_error(DFM_ERR_INVALID_ARG, "boxes is NULL");
    const int64_t hw = (int64_t)d->pad_h * d->pad_w;
    hipLaunchKernelGGL(depth_resolve_kernel, dim3((unsigned)((hw + DT_THREADS - 1) / DT_THREADS), d->batch),
                       dim3(DT_THREADS), 0, (hipStream_t)stream, *d, (const unsigned long long *)keys, depth_in, cam,
                       boxes, expand_ratio, expand_distance, depth_out, fgmask);
    HIP_TRY(hipGetLastError());
    return DFM_OK;
}

extern "C" DFM_API int dfm_points_in_boxes(int32_t mode, int32_t batch, int64_t num_points, int32_t num_boxes,
                                           const float *points, const float *boxes, int32_t *out, void *stream)
{
    if (mode != DFM_PIB_PART && mode != DFM_PIB_ALL && mode != DFM_PIB_IDMAP)
        return set_error(DFM_ERR_INVALID_ARG, "mode must be DFM_PIB_PART, DFM_PIB_ALL or DFM_PIB_IDMAP");
    if (batch < 0 || num_points < 0 || num_boxes < 0) return set_error(DFM_ERR_INVALID_ARG, "negative size");
    if (batch > 65535) return set_error(DFM_ERR_UNSUPPORTED, "batch > 65535");
    if (num_boxes > 0x7ffffffe)
        return set_error(DFM_ERR_UNSUPPORTED, "more boxes than the int32 index holds (2^31 - 2)");
    const int64_t blocks = (num_points + DT_THREADS - 1) / DT_THREADS;
    if (blocks > 0x7fffffffll) return set_error(DFM_ERR_UNSUPPORTED, "too many points");
    if (batch == 0 || num_points == 0 || (mode == DFM_PIB_ALL && num_boxes == 0)) return DFM_OK;
    if (!points || !out || (num_boxes > 0 && !boxes)) return set_error(DFM_ERR_INVALID_ARG, "NULL device pointer");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)blocks, batch);
    if (mode == DFM_PIB_PART)
        hipLaunchKernelGGL(points_in_boxes_kernel<DFM_PIB_PART>, grid, dim3(DT_THREADS), 0, st, num_points, num_boxes,
                           points, boxes, out);
    else if (mode == DFM_PIB_ALL)
        hipLaunchKernelGGL(points_in_boxes_kernel<DFM_PIB_ALL>, grid, dim3(DT_THREADS), 0, st, num_points, num_boxes,
                           points, boxes, out);
    else
        hipLaunchKernelGGL(points_in_boxes_kernel<DFM_PIB_IDMAP>, grid, dim3(DT_THREADS), 0, st, num_points,
                           num_boxes, points, boxes, out);
    HIP_TRY(hipGetLastError());
    return DFM_OK;
}
