// voxelize.hip -- hard voxelization of the LiDAR teacher (include/dfm_hip_sparse_conv.h states the rules): the
// per-point and per-voxel work around the caller's stable sort and prefix sums.  Every kernel is one thread per
// point (or per sorted position), every store goes to an index below N or below the row bound the caller sized.
#include "dfm_common.h"

namespace {

struct VoxelArgs {
    int32_t batch, ndim, gx, gy, gz, max_num_points, max_voxels;
    float lo[3], vs[3];
    int64_t offset[DFM_VOXEL_MAX_BATCH + 1];
};

// the sample of point p: offsets ascend, offset[batch] = N > p
__device__ __forceinline__ int sample_of(const VoxelArgs &a, int64_t p)
{
    int b = 0;
    for (int i = 1; i < a.batch; ++i) b += (p >= a.offset[i]) ? 1 : 0;
    return b;
}

__global__ __launch_bounds__(256) void voxel_keys_kernel(VoxelArgs a, const float *__restrict__ points,
                                                         int64_t *__restrict__ key, int64_t n)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const float *q = points + p * a.ndim;
    const int grid[3] = {a.gx, a.gy, a.gz};
    int c[3];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float f = floorf((q[j] - a.lo[j]) / a.vs[j]);
        // the reference drops on (f < 0 or f >= grid); a NaN passes both and cannot index anything: dropped too
        ok = ok && (f >= 0.0f) && (f < (float)grid[j]);
        c[j] = ok ? (int)f : 0;
    }
    const int64_t b = sample_of(a, p);
    key[p] = ok ? ((b * a.gz + c[2]) * a.gy + c[1]) * (int64_t)a.gx + c[0] : DFM_VOXEL_NO_KEY;
}

__global__ __launch_bounds__(256) void voxel_heads_kernel(const int64_t *__restrict__ skey,
                                                          const int64_t *__restrict__ perm,
                                                          int32_t *__restrict__ first, int64_t *__restrict__ head,
                                                          int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t k = skey[i];
    const bool h = k != DFM_VOXEL_NO_KEY && (i == 0 || skey[i - 1] != k);
    const int64_t p = perm[i];
    if (p >= 0 && p < n) first[p] = h ? 1 : 0;  // perm is a permutation: every point is written once
    head[i] = h ? i : 0;
}

__global__ __launch_bounds__(256) void voxel_keep_kernel(VoxelArgs a, const int32_t *__restrict__ first,
                                                         const int64_t *__restrict__ first_scan,
                                                         int32_t *__restrict__ keep, int64_t n)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    int k = 0;
    if (first[p]) {
        const int64_t start = a.offset[sample_of(a, p)];
        const int64_t number = first_scan[p] - 1 - (start > 0 ? first_scan[start - 1] : 0);
        k = number < a.max_voxels ? 1 : 0;
    }
    keep[p] = k;
}

__global__ __launch_bounds__(256) void voxel_fill_kernel(VoxelArgs a, const float *__restrict__ points,
                                                         const int64_t *__restrict__ skey,
                                                         const int64_t *__restrict__ perm,
                                                         const int64_t *__restrict__ head_scan,
                                                         const int32_t *__restrict__ keep,
                                                         const int64_t *__restrict__ keep_scan,
                                                         float *__restrict__ voxels, int32_t *__restrict__ coors,
                                                         int32_t *__restrict__ num_points, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t k = skey[i];
    if (k == DFM_VOXEL_NO_KEY) return;
    const int64_t h = head_scan[i];
    if (h < 0 || h > i) return;
    const int64_t fp = perm[h];
    if (fp < 0 || fp >= n || !keep[fp]) return;
    const int64_t row = keep_scan[fp] - 1;
    // rows of sample b < (b + 1) * max_voxels by construction; the caller sized the outputs by batch * max_voxels
    if (row < 0 || row >= (int64_t)a.batch * a.max_voxels) return;
    const int64_t slot = i - h;
    if (slot < a.max_num_points) {
        const int64_t p = perm[i];
        if (p >= 0 && p < n) {
            const float *q = points + p * a.ndim;
            float *v = voxels + (row * a.max_num_points + slot) * a.ndim;
            for (int j = 0; j < a.ndim; ++j) v[j] = q[j];
        }
    }
    if (slot == 0) {
        int64_t r = k;
        const int cx = (int)(r % a.gx);
        r /= a.gx;
        const int cy = (int)(r % a.gy);
        r /= a.gy;
        const int cz = (int)(r % a.gz);
        r /= a.gz;
        int32_t *c = coors + row * 4;
        c[0] = (int)r, c[1] = cz, c[2] = cy, c[3] = cx;
    }
    if (i + 1 == n || skey[i + 1] != k)  // the run's last point knows its length
        num_points[row] = (int32_t)(slot + 1 < a.max_num_points ? slot + 1 : a.max_num_points);
}

// validation shared by the four entries -> 0 and the by-value kernel argument, or an error
int check(const dfm_voxel_desc *d, VoxelArgs *a, int64_t *n)
{
    if (!d) return dfm::set_error(DFM_ERR_INVALID_ARG, "voxelize: NULL descriptor");
    if (d->batch < 1 || d->batch > DFM_VOXEL_MAX_BATCH)
        return dfm::set_errorf(DFM_ERR_INVALID_ARG, "voxelize: batch %d is outside 1..%d", d->batch,
                               DFM_VOXEL_MAX_BATCH);
    if (d->ndim < 3 || d->ndim > 16)
        return dfm::set_errorf(DFM_ERR_INVALID_ARG, "voxelize: ndim %d is outside 3..16", d->ndim);
    if (d->max_num_points < 1 || d->max_voxels < 1)
        return dfm::set_error(DFM_ERR_INVALID_ARG, "voxelize: max_num_points and max_voxels start at 1");
    double cells = d->batch;
    for (int j = 0; j < 3; ++j) {
        if (d->grid[j] < 1) return dfm::set_error(DFM_ERR_INVALID_ARG, "voxelize: a grid size < 1");
        if (!(d->vs[j] > 0.0f)) return dfm::set_error(DFM_ERR_INVALID_ARG, "voxelize: a voxel size that is not > 0");
        cells *= d->grid[j];
    }
    if (cells >= 4.6e18) return dfm::set_error(DFM_ERR_INVALID_ARG, "voxelize: batch * grid cells reach 2^62");
    if (d->offset[0] != 0) return dfm::set_error(DFM_ERR_INVALID_ARG, "voxelize: offset[0] must be 0");
    for (int b = 0; b < d->batch; ++b)
        if (d->offset[b + 1] < d->offset[b])
            return dfm::set_error(DFM_ERR_INVALID_ARG, "voxelize: offsets must ascend");
    if (d->offset[d->batch] >= INT32_MAX)
        return dfm::set_error(DFM_ERR_INVALID_ARG, "voxelize: 2^31 - 1 points or more");
    a->batch = d->batch, a->ndim = d->ndim;
    a->gx = d->grid[0], a->gy = d->grid[1], a->gz = d->grid[2];
    a->max_num_points = d->max_num_points, a->max_voxels = d->max_voxels;
    for (int j = 0; j < 3; ++j) a->lo[j] = d->lo[j], a->vs[j] = d->vs[j];
    for (int b = 0; b <= DFM_VOXEL_MAX_BATCH; ++b) a->offset[b] = b <= d->batch ? d->offset[b] : d->offset[d->batch];
    *n = d->offset[d->batch];
    return 0;
}

inline dim3 blocks(int64_t n) { return dim3((unsigned)((n + 255) / 256)); }

}  // namespace

extern "C" {

int dfm_voxel_keys(const dfm_voxel_desc *desc, const float *points, int64_t *key, void *stream)
{
    VoxelArgs a;
    int64_t n;
    if (int rc = check(desc, &a, &n)) return rc;
    if (n == 0) return 0;
    if (!points || !key) return dfm::set_error(DFM_ERR_INVALID_ARG, "dfm_voxel_keys: NULL pointer");
    voxel_keys_kernel<<<blocks(n), 256, 0, (hipStream_t)stream>>>(a, points, key, n);
    HIP_TRY(hipGetLastError());
    return 0;
}

int dfm_voxel_heads(const dfm_voxel_desc *desc, const int64_t *sorted_key, const int64_t *perm, int32_t *first,
                    int64_t *head, void *stream)
{
    VoxelArgs a;
    int64_t n;
    if (int rc = check(desc, &a, &n)) return rc;
    if (n == 0) return 0;
    if (!sorted_key || !perm || !first || !head)
        return dfm::set_error(DFM_ERR_INVALID_ARG, "dfm_voxel_heads: NULL pointer");
    voxel_heads_kernel<<<blocks(n), 256, 0, (hipStream_t)stream>>>(sorted_key, perm, first, head, n);
    HIP_TRY(hipGetLastError());
    return 0;
}

int dfm_voxel_keep(const dfm_voxel_desc *desc, const int32_t *first, const int64_t *first_scan, int32_t *keep,
                   void *stream)
{
    VoxelArgs a;
    int64_t n;
    if (int rc = check(desc, &a, &n)) return rc;
    if (n == 0) return 0;
    if (!first || !first_scan || !keep) return dfm::set_error(DFM_ERR_INVALID_ARG, "dfm_voxel_keep: NULL pointer");
    voxel_keep_kernel<<<blocks(n), 256, 0, (hipStream_t)stream>>>(a, first, first_scan, keep, n);
    HIP_TRY(hipGetLastError());
    return 0;
}

int dfm_voxel_fill(const dfm_voxel_desc *desc, const float *points, const int64_t *sorted_key, const int64_t *perm,
                   const int64_t *head_scan, const int32_t *keep, const int64_t *keep_scan, float *voxels,
                   int32_t *coors, int32_t *num_points, void *stream)
{
    VoxelArgs a;
    int64_t n;
    if (int rc = check(desc, &a, &n)) return rc;
    if (n == 0) return 0;
    if (!points || !sorted_key || !perm || !head_scan || !keep || !keep_scan || !voxels || !coors || !num_points)
        return dfm::set_error(DFM_ERR_INVALID_ARG, "dfm_voxel_fill: NULL pointer");
    voxel_fill_kernel<<<blocks(n), 256, 0, (hipStream_t)stream>>>(a, points, sorted_key, perm, head_scan, keep,
                                                                  keep_scan, voxels, coors, num_points, n);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
