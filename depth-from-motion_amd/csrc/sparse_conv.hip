// sparse_conv.hip -- SubMConv3d / SparseConv3d of the LiDAR teacher's CustomSparseEncoder, forward only
// (include/dfm_hip_sparse_conv.h states the semantics): coordinate hash tables, neighbour tables, the
// output-stationary FP32-MFMA convolution and dense().  Every probe loop is bounded; every index read from a table
// is range-checked before it addresses memory.
#include "dfm_common.h"

namespace {

constexpr int64_t EMPTY = -1;

struct Grid {
    int32_t batch, d, h, w;
};

struct ConvGeom {
    Grid in, out;
    int32_t k[3], s[3], p[3];
    int32_t taps;
};

__device__ __forceinline__ uint64_t mix(int64_t key)
{
    uint64_t h = (uint64_t)key;
    h ^= h >> 33;
    h *= 0xff51afd7ed558ccdULL;
    h ^= h >> 33;
    return h;
}

__device__ __forceinline__ int64_t grid_key(const Grid &g, int b, int z, int y, int x)
{
    return (((int64_t)b * g.d + z) * g.h + y) * (int64_t)g.w + x;
}

__device__ __forceinline__ bool inside(const Grid &g, int b, int z, int y, int x)
{
    return b >= 0 && b < g.batch && z >= 0 && z < g.d && y >= 0 && y < g.h && x >= 0 && x < g.w;
}

__device__ __forceinline__ int probes_of(int64_t capacity)
{
    return (int)(capacity < DFM_SPARSE_MAX_PROBES ? capacity : DFM_SPARSE_MAX_PROBES);
}

// the row stored under key, or -1: at most probes_of(capacity) slots
__device__ __forceinline__ int lookup(const int64_t *__restrict__ keys, const int32_t *__restrict__ rows,
                                      int64_t capacity, int64_t key)
{
    uint64_t slot = mix(key) & (uint64_t)(capacity - 1);
    const int probes = probes_of(capacity);
    for (int i = 0; i < probes; ++i) {
        const int64_t k = keys[slot];
        if (k == key) return rows[slot];
        if (k == EMPTY) return -1;
        slot = (slot + 1) & (uint64_t)(capacity - 1);
    }
    return -1;
}

// claims the slot of key: 1 = this call inserted it (*slot_out valid), 0 = it was there, -1 = no slot in the bound
__device__ __forceinline__ int insert(int64_t *keys, int64_t capacity, int64_t key, uint64_t *slot_out)
{
    uint64_t slot = mix(key) & (uint64_t)(capacity - 1);
    const int probes = probes_of(capacity);
    for (int i = 0; i < probes; ++i) {
        const unsigned long long old = atomicCAS((unsigned long long *)&keys[slot], (unsigned long long)EMPTY,
                                                 (unsigned long long)key);
        if (old == (unsigned long long)EMPTY) {
            *slot_out = slot;
            return 1;
        }
        if (old == (unsigned long long)key) return 0;
        slot = (slot + 1) & (uint64_t)(capacity - 1);
    }
    return -1;
}

__global__ __launch_bounds__(256) void index_build_kernel(Grid g, const int32_t *__restrict__ coors, int64_t rows,
                                                          int64_t *keys, int32_t *table_rows, int64_t capacity,
                                                          int32_t *status)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    const int4 c = ((const int4 *)coors)[r];
    if (c.x < 0) return;
    if (!inside(g, c.x, c.y, c.z, c.w)) {
        atomicOr(status, DFM_SPARSE_STATUS_COORDINATE);
        return;
    }
    uint64_t slot;
    const int got = insert(keys, capacity, grid_key(g, c.x, c.y, c.z, c.w), &slot);
    if (got == 1) table_rows[slot] = (int32_t)r;
    else atomicOr(status, got == 0 ? DFM_SPARSE_STATUS_DUPLICATE : DFM_SPARSE_STATUS_TABLE_FULL);
}

// nbr[k][r], k = (kz * 3 + ky) * 3 + kx: one thread per (k, r), r fastest
__global__ __launch_bounds__(256) void subm_neighbours_kernel(Grid g, const int32_t *__restrict__ coors, int64_t rows,
                                                              const int64_t *__restrict__ keys,
                                                              const int32_t *__restrict__ table_rows,
                                                              int64_t capacity, int32_t *__restrict__ nbr)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= rows * 27) return;
    const int k = (int)(t / rows);
    const int64_t r = t - (int64_t)k * rows;
    const int4 c = ((const int4 *)coors)[r];
    int found = -1;
    if (c.x >= 0 && inside(g, c.x, c.y, c.z, c.w)) {
        const int z = c.y + k / 9 - 1, y = c.z + (k / 3) % 3 - 1, x = c.w + k % 3 - 1;
        if (inside(g, c.x, z, y, x)) {  // per axis: a neighbour past a border is absent, never the next row's cell
            found = lookup(keys, table_rows, capacity, grid_key(g, c.x, z, y, x));
            if (found >= rows) found = -1;
        }
    }
    nbr[t] = found;
}

// one thread per (input row, offset): the output site that reads this input through this offset, if any
__global__ __launch_bounds__(256) void out_rows_kernel(ConvGeom q, const int32_t *__restrict__ coors, int64_t rows,
                                                       int64_t *out_keys, int64_t out_capacity,
                                                       int32_t *out_coors, int64_t out_bound, int32_t *out_count,
                                                       int32_t *status)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= rows * q.taps) return;
    const int64_t r = t / q.taps;
    const int k = (int)(t - r * q.taps);
    const int4 c = ((const int4 *)coors)[r];
    if (c.x < 0) return;
    if (!inside(q.in, c.x, c.y, c.z, c.w)) {
        atomicOr(status, DFM_SPARSE_STATUS_COORDINATE);
        return;
    }
    const int kz = k / (q.k[1] * q.k[2]), ky = (k / q.k[2]) % q.k[1], kx = k % q.k[2];
    const int nz = c.y + q.p[0] - kz, ny = c.z + q.p[1] - ky, nx = c.w + q.p[2] - kx;  // o * s
    if (nz < 0 || ny < 0 || nx < 0 || nz % q.s[0] || ny % q.s[1] || nx % q.s[2]) return;
    const int oz = nz / q.s[0], oy = ny / q.s[1], ox = nx / q.s[2];
    if (!inside(q.out, c.x, oz, oy, ox)) return;
    uint64_t slot;
    const int got = insert(out_keys, out_capacity, grid_key(q.out, c.x, oz, oy, ox), &slot);
    if (got == 1) {
        const int row = atomicAdd(out_count, 1);
        if (row < out_bound) {
            ((int4 *)out_coors)[row] = make_int4(c.x, oz, oy, ox);
        } else {
            atomicOr(status, DFM_SPARSE_STATUS_ROW_BOUND);
        }
    } else if (got < 0) {
        atomicOr(status, DFM_SPARSE_STATUS_TABLE_FULL);
    }
}

// nbr[k][o] of a SparseConv3d: one thread per (k, o), o fastest
__global__ __launch_bounds__(256) void conv_neighbours_kernel(ConvGeom q, const int32_t *__restrict__ out_coors,
                                                              int64_t out_bound, int64_t in_rows,
                                                              const int64_t *__restrict__ keys,
                                                              const int32_t *__restrict__ table_rows,
                                                              int64_t capacity, int32_t *__restrict__ nbr)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= out_bound * q.taps) return;
    const int k = (int)(t / out_bound);
    const int64_t o = t - (int64_t)k * out_bound;
    const int4 c = ((const int4 *)out_coors)[o];
    int found = -1;
    if (c.x >= 0 && inside(q.out, c.x, c.y, c.z, c.w)) {
        const int kz = k / (q.k[1] * q.k[2]), ky = (k / q.k[2]) % q.k[1], kx = k % q.k[2];
        const int z = c.y * q.s[0] - q.p[0] + kz, y = c.z * q.s[1] - q.p[1] + ky, x = c.w * q.s[2] - q.p[2] + kx;
        if (inside(q.in, c.x, z, y, x)) {
            found = lookup(keys, table_rows, capacity, grid_key(q.in, c.x, z, y, x));
            if (found >= in_rows) found = -1;
        }
    }
    nbr[t] = found;
}

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int LDS_STRIDE = 64 + 4;  // floats per gathered row: 16 rows x 4 k-lanes fall on distinct banks

__device__ __forceinline__ void wave_sync()
{
    // the tile in LDS is private to one wave: order its writes before the other lanes' reads, no workgroup barrier
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// NT = cout / 16 accumulator tiles per wave; four waves a workgroup, 16 output rows a wave
template <int NT>
__global__ __launch_bounds__(256) void sparse_conv_kernel(int cin, int taps, const float *__restrict__ in,
                                                          int64_t in_rows, const int32_t *__restrict__ nbr,
                                                          const int32_t *__restrict__ out_coors, int64_t out_rows,
                                                          const float *__restrict__ weight,
                                                          const float *__restrict__ scale,
                                                          const float *__restrict__ shift, int relu,
                                                          float *__restrict__ out)
{
    constexpr int COUT = NT * 16;
    __shared__ float tile[4][16][LDS_STRIDE];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t row0 = ((int64_t)blockIdx.x * 4 + wave) * 16;
    if (row0 >= out_rows) return;
    const int64_t my_row = row0 + (lane & 15);
    const bool live = lane < 16 && my_row < out_rows && out_coors[my_row * 4] >= 0;
    if (__ballot(live) == 0) return;  // a tile past the live rows
    const int cinp = (cin + 3) & ~3, vecs = cinp >> 2;
    const int m = lane & 15, kq = lane >> 4;
    f32x4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    for (int k = 0; k < taps; ++k) {
        int idx = -1;
        if (live) {
            idx = nbr ? nbr[(int64_t)k * out_rows + my_row] : (int)my_row;
            if (idx < 0 || idx >= in_rows) idx = -1;
        }
        if (__ballot(idx >= 0) == 0) continue;  // zeros only: skipping them changes no bit
        for (int v = lane; v < 16 * vecs; v += 64) {
            const int r = v / vecs, c4 = v - r * vecs;
            const int src = __shfl(idx, r);
            float4 val = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (src >= 0) {
                if (cin == 3) {
                    const float *p = in + (int64_t)src * 3;
                    val = make_float4(p[0], p[1], p[2], 0.0f);
                } else {
                    val = *(const float4 *)(in + (int64_t)src * cin + c4 * 4);
                }
            }
            *(float4 *)&tile[wave][r][c4 * 4] = val;
        }
        wave_sync();
        const float *wk = weight + (int64_t)k * cin * COUT;
        for (int kk = 0; kk < vecs; ++kk) {
            const int ci = kk * 4 + kq;
            const float a = tile[wave][m][ci];
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const float b = ci < cin ? wk[ci * COUT + t * 16 + m] : 0.0f;
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[t], 0, 0, 0);
            }
        }
        wave_sync();
    }

#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int r = kq * 4 + j;  // C/D: row = (lane >> 4) * 4 + reg, column = lane & 15
        const bool row_live = __shfl((int)live, r) != 0;
        if (!row_live) continue;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int n = t * 16 + m;
            float v = acc[t][j];
            if (scale) v = v * scale[n] + shift[n];
            if (relu) v = v > 0.0f ? v : 0.0f;
            out[(row0 + r) * COUT + n] = v;
        }
    }
}

__global__ __launch_bounds__(256) void dense_kernel(Grid g, const float *__restrict__ features,
                                                    const int32_t *__restrict__ coors, int64_t rows, int channels,
                                                    float *__restrict__ out)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= rows * channels) return;
    const int64_t r = t / channels;
    const int c = (int)(t - r * channels);
    const int4 q = ((const int4 *)coors)[r];
    if (q.x < 0 || !inside(g, q.x, q.y, q.z, q.w)) return;
    out[((((int64_t)q.x * channels + c) * g.d + q.y) * g.h + q.z) * (int64_t)g.w + q.w] = features[t];
}

int64_t pow2_at_least(int64_t v)
{
    int64_t c = 16;
    while (c < v) c <<= 1;
    return c;
}

int check_grid(const char *who, int32_t batch, const int32_t *size3, Grid *g)
{
    if (!size3) return dfm::set_errorf(DFM_ERR_INVALID_ARG, "%s: NULL grid size", who);
    if (batch < 1 || size3[0] < 1 || size3[1] < 1 || size3[2] < 1)
        return dfm::set_errorf(DFM_ERR_INVALID_ARG, "%s: batch and grid sizes start at 1", who);
    if ((double)batch * size3[0] * size3[1] * size3[2] >= 4.6e18)
        return dfm::set_errorf(DFM_ERR_UNSUPPORTED, "%s: the key space batch * D * H * W reaches 2^62", who);
    *g = Grid{batch, size3[0], size3[1], size3[2]};
    return 0;
}

int check_table(const char *who, int64_t rows, int64_t capacity)
{
    if (rows < 0 || rows >= INT32_MAX) return dfm::set_errorf(DFM_ERR_INVALID_ARG, "%s: rows outside 0..2^31 - 2", who);
    if (capacity < 16 || (capacity & (capacity - 1)) || capacity < 2 * rows)
        return dfm::set_errorf(DFM_ERR_INVALID_ARG, "%s: capacity must be a power of two >= max(16, 2 * rows)", who);
    return 0;
}

int make_plan(const dfm_sparse_conv_desc *d, int64_t in_rows, dfm_sparse_conv_plan *plan, ConvGeom *q)
{
    if (!d) return dfm::set_error(DFM_ERR_INVALID_ARG, "sparse conv: NULL descriptor");
    if (in_rows < 0) return dfm::set_error(DFM_ERR_INVALID_ARG, "sparse conv: in_rows < 0");
    if (d->batch < 1) return dfm::set_error(DFM_ERR_INVALID_ARG, "sparse conv: batch size < 1");
    dfm_sparse_conv_plan p = {};
    int64_t taps = 1, fan = 1;
    double cells_in = d->batch, cells_out = d->batch;
    for (int a = 0; a < 3; ++a) {
        if (d->in_size[a] < 1) return dfm::set_error(DFM_ERR_INVALID_ARG, "sparse conv: a grid size < 1");
        if (d->kernel[a] < 1) return dfm::set_error(DFM_ERR_INVALID_ARG, "sparse conv: a kernel size < 1");
        if (d->stride[a] < 1) return dfm::set_error(DFM_ERR_INVALID_ARG, "sparse conv: a stride < 1");
        if (d->padding[a] < 0) return dfm::set_error(DFM_ERR_INVALID_ARG, "sparse conv: a padding < 0");
        if (d->subm) {
            if (d->kernel[a] != 3) return dfm::set_error(DFM_ERR_INVALID_ARG, "sparse conv: subm takes kernel 3");
            p.out_size[a] = d->in_size[a];
        } else {
            const int64_t span = (int64_t)d->in_size[a] + 2LL * d->padding[a] - d->kernel[a];
            if (span < 0)
                return dfm::set_error(DFM_ERR_INVALID_ARG, "sparse conv: kernel larger than the padded input");
            p.out_size[a] = (int32_t)(span / d->stride[a] + 1);
            fan *= (d->kernel[a] + d->stride[a] - 1) / d->stride[a];
        }
        taps *= d->kernel[a];
        cells_in *= d->in_size[a];
        cells_out *= p.out_size[a];
    }
    if (taps > DFM_SPARSE_MAX_TAPS)
        return dfm::set_errorf(DFM_ERR_UNSUPPORTED, "sparse conv: %lld kernel offsets, at most %d", (long long)taps,
                               DFM_SPARSE_MAX_TAPS);
    if (cells_in >= 4.6e18 || cells_out >= 4.6e18)
        return dfm::set_error(DFM_ERR_UNSUPPORTED, "sparse conv: the key space batch * D * H * W reaches 2^62");
    double bound = d->subm ? (double)in_rows : (double)in_rows * (double)fan;
    if (!d->subm && bound > cells_out) bound = cells_out;
    if (bound >= 2147483647.0 || in_rows >= INT32_MAX || bound * (double)taps >= 9.0e18)
        return dfm::set_error(DFM_ERR_UNSUPPORTED, "sparse conv: a row bound of 2^31 - 1 or more (rows are int32)");
    p.taps = (int32_t)taps;
    p.out_rows = (int64_t)bound;
    p.in_capacity = pow2_at_least(2 * in_rows);
    p.out_capacity = d->subm ? 0 : pow2_at_least(2 * p.out_rows);
    if (plan) *plan = p;
    if (q) {
        q->in = Grid{d->batch, d->in_size[0], d->in_size[1], d->in_size[2]};
        q->out = Grid{d->batch, p.out_size[0], p.out_size[1], p.out_size[2]};
        for (int a = 0; a < 3; ++a) q->k[a] = d->kernel[a], q->s[a] = d->stride[a], q->p[a] = d->padding[a];
        q->taps = p.taps;
    }
    return 0;
}

inline dim3 blocks(int64_t n) { return dim3((unsigned)((n + 255) / 256)); }

}  // namespace

extern "C" {

int dfm_sparse_conv_out_shape(const dfm_sparse_conv_desc *desc, int64_t in_rows, dfm_sparse_conv_plan *plan)
{
    if (!plan) return dfm::set_error(DFM_ERR_INVALID_ARG, "dfm_sparse_conv_out_shape: NULL plan");
    return make_plan(desc, in_rows, plan, nullptr);
}

size_t dfm_sparse_conv_workspace_bytes(const dfm_sparse_conv_desc *desc, int64_t in_rows)
{
    dfm_sparse_conv_plan p;
    if (make_plan(desc, in_rows, &p, nullptr)) return 0;
    return (size_t)(p.in_capacity + p.out_capacity) * 12 + (size_t)p.taps * (size_t)p.out_rows * 4;
}

int dfm_sparse_index_build(const int32_t *coors, int64_t rows, int32_t batch, const int32_t *size3,
                           int64_t *table_keys, int32_t *table_rows, int64_t capacity, int32_t *status, void *stream)
{
    Grid g;
    if (int rc = check_grid("dfm_sparse_index_build", batch, size3, &g)) return rc;
    if (int rc = check_table("dfm_sparse_index_build", rows, capacity)) return rc;
    if (!table_keys || !table_rows || !status || (rows && !coors))
        return dfm::set_error(DFM_ERR_INVALID_ARG, "dfm_sparse_index_build: NULL pointer");
    if ((uintptr_t)coors & 15) return dfm::set_error(DFM_ERR_INVALID_ARG, "dfm_sparse_index_build: coors is not 16-byte aligned");
    if (rows == 0) return 0;
    index_build_kernel<<<blocks(rows), 256, 0, (hipStream_t)stream>>>(g, coors, rows, table_keys, table_rows,
                                                                      capacity, status);
    HIP_TRY(hipGetLastError());
    return 0;
}

int dfm_sparse_subm_neighbours(const int32_t *coors, int64_t rows, int32_t batch, const int32_t *size3,
                               const int64_t *table_keys, const int32_t *table_rows, int64_t capacity, int32_t *nbr,
                               void *stream)
{
    Grid g;
    if (int rc = check_grid("dfm_sparse_subm_neighbours", batch, size3, &g)) return rc;
    if (int rc = check_table("dfm_sparse_subm_neighbours", rows, capacity)) return rc;
    if (rows >= INT32_MAX / 27) return dfm::set_error(DFM_ERR_UNSUPPORTED, "dfm_sparse_subm_neighbours: 27 * rows reaches 2^31");
    if (!table_keys || !table_rows || (rows && (!coors || !nbr)))
        return dfm::set_error(DFM_ERR_INVALID_ARG, "dfm_sparse_subm_neighbours: NULL pointer");
    if ((uintptr_t)coors & 15) return dfm::set_error(DFM_ERR_INVALID_ARG, "dfm_sparse_subm_neighbours: coors is not 16-byte aligned");
    if (rows == 0) return 0;
    subm_neighbours_kernel<<<blocks(rows * 27), 256, 0, (hipStream_t)stream>>>(g, coors, rows, table_keys,
                                                                               table_rows, capacity, nbr);
    HIP_TRY(hipGetLastError());
    return 0;
}

int dfm_sparse_conv_out_rows(const dfm_sparse_conv_desc *desc, const int32_t *coors, int64_t rows, int64_t *out_keys,
                             int32_t *out_coors, int32_t *out_count, int32_t *status, void *stream)
{
    dfm_sparse_conv_plan p;
    ConvGeom q;
    if (int rc = make_plan(desc, rows, &p, &q)) return rc;
    if (desc->subm) return dfm::set_error(DFM_ERR_INVALID_ARG, "dfm_sparse_conv_out_rows: a subm layer keeps its rows");
    if (!out_keys || !out_count || !status || (rows && (!coors || !out_coors)))
        return dfm::set_error(DFM_ERR_INVALID_ARG, "dfm_sparse_conv_out_rows: NULL pointer");
    if (((uintptr_t)coors | (uintptr_t)out_coors) & 15)
        return dfm::set_error(DFM_ERR_INVALID_ARG, "dfm_sparse_conv_out_rows: coors is not 16-byte aligned");
    if (rows == 0) return 0;
    if ((double)rows * p.taps >= 5.0e11)
        return dfm::set_error(DFM_ERR_UNSUPPORTED, "dfm_sparse_conv_out_rows: rows * offsets above the launch grid");
    out_rows_kernel<<<blocks(rows * p.taps), 256, 0, (hipStream_t)stream>>>(q, coors, rows, out_keys, p.out_capacity,
                                                                            out_coors, p.out_rows, out_count, status);
    HIP_TRY(hipGetLastError());
    return 0;
}

int dfm_sparse_conv_neighbours(const dfm_sparse_conv_desc *desc, const int32_t *out_coors, int64_t in_rows,
                               const int64_t *table_keys, const int32_t *table_rows, int32_t *nbr, void *stream)
{
    dfm_sparse_conv_plan p;
    ConvGeom q;
    if (int rc = make_plan(desc, in_rows, &p, &q)) return rc;
    if (desc->subm)
        return dfm::set_error(DFM_ERR_INVALID_ARG, "dfm_sparse_conv_neighbours: use dfm_sparse_subm_neighbours");
    if (!table_keys || !table_rows || (p.out_rows && (!out_coors || !nbr)))
        return dfm::set_error(DFM_ERR_INVALID_ARG, "dfm_sparse_conv_neighbours: NULL pointer");
    if ((uintptr_t)out_coors & 15)
        return dfm::set_error(DFM_ERR_INVALID_ARG, "dfm_sparse_conv_neighbours: coors is not 16-byte aligned");
    if (p.out_rows == 0) return 0;
    if ((double)p.out_rows * p.taps >= 5.0e11)
        return dfm::set_error(DFM_ERR_UNSUPPORTED, "dfm_sparse_conv_neighbours: rows * offsets above the launch grid");
    conv_neighbours_kernel<<<blocks(p.out_rows * p.taps), 256, 0, (hipStream_t)stream>>>(
        q, out_coors, p.out_rows, in_rows, table_keys, table_rows, p.in_capacity, nbr);
    HIP_TRY(hipGetLastError());
    return 0;
}

int dfm_sparse_conv_fwd(int32_t cin, int32_t cout, int32_t taps, const float *in, int64_t in_rows, const int32_t *nbr,
                        const int32_t *out_coors, int64_t out_rows, const float *weight, const float *scale,
                        const float *shift, int32_t relu, float *out, void *stream)
{
    if (cin < 1 || cout < 1 || taps < 1 || in_rows < 0 || out_rows < 0)
        return dfm::set_error(DFM_ERR_INVALID_ARG, "dfm_sparse_conv_fwd: a size < 1 or a negative row count");
    if (taps > DFM_SPARSE_MAX_TAPS)
        return dfm::set_errorf(DFM_ERR_UNSUPPORTED, "dfm_sparse_conv_fwd: %d kernel offsets, at most %d", taps,
                               DFM_SPARSE_MAX_TAPS);
    if (!((cin == 3 || cin % 4 == 0) && cin <= 64) || (cout != 16 && cout != 32 && cout != 64))
        return dfm::set_errorf(DFM_ERR_UNSUPPORTED,
                               "dfm_sparse_conv_fwd: channels %d -> %d (Cin: 3 or a multiple of 4 up to 64; Cout: 16, "
                               "32 or 64)", cin, cout);
    if (in_rows >= INT32_MAX || out_rows >= INT32_MAX)
        return dfm::set_error(DFM_ERR_UNSUPPORTED, "dfm_sparse_conv_fwd: 2^31 - 1 rows or more");
    if (out_rows && !nbr && (taps != 1 || in_rows < out_rows))
        return dfm::set_error(DFM_ERR_INVALID_ARG, "dfm_sparse_conv_fwd: nbr may be NULL for one offset on the same rows only");
    if ((scale == nullptr) != (shift == nullptr))
        return dfm::set_error(DFM_ERR_INVALID_ARG, "dfm_sparse_conv_fwd: scale and shift come together");
    if (!weight || (out_rows && (!out_coors || !out || !in)))
        return dfm::set_error(DFM_ERR_INVALID_ARG, "dfm_sparse_conv_fwd: NULL pointer");
    if (((uintptr_t)weight | (uintptr_t)out | (uintptr_t)out_coors) & 15 || ((uintptr_t)in & (cin == 3 ? 3 : 15)))
        return dfm::set_error(DFM_ERR_INVALID_ARG, "dfm_sparse_conv_fwd: a pointer is not 16-byte aligned");
    if (out_rows == 0) return 0;
    const dim3 grid((unsigned)((out_rows + 63) / 64));
    hipStream_t s = (hipStream_t)stream;
    const bool timed = dfm::profile_mark(stream, false);
    if (cout == 16)
        sparse_conv_kernel<1><<<grid, 256, 0, s>>>(cin, taps, in, in_rows, nbr, out_coors, out_rows, weight, scale,
                                                   shift, relu, out);
    else if (cout == 32)
        sparse_conv_kernel<2><<<grid, 256, 0, s>>>(cin, taps, in, in_rows, nbr, out_coors, out_rows, weight, scale,
                                                   shift, relu, out);
    else
        sparse_conv_kernel<4><<<grid, 256, 0, s>>>(cin, taps, in, in_rows, nbr, out_coors, out_rows, weight, scale,
                                                   shift, relu, out);
    if (timed) dfm::profile_mark(stream, true);
    HIP_TRY(hipGetLastError());
    return 0;
}

int dfm_sparse_dense(const float *features, const int32_t *coors, int64_t rows, int32_t channels, int32_t batch,
                     const int32_t *size3, float *out, void *stream)
{
    Grid g;
    if (int rc = check_grid("dfm_sparse_dense", batch, size3, &g)) return rc;
    if (channels < 1 || rows < 0) return dfm::set_error(DFM_ERR_INVALID_ARG, "dfm_sparse_dense: channels < 1 or rows < 0");
    if (!out || (rows && (!features || !coors)))
        return dfm::set_error(DFM_ERR_INVALID_ARG, "dfm_sparse_dense: NULL pointer");
    const double cells = (double)batch * channels * g.d * g.h * g.w;
    if (cells >= 2.0e18 || (double)rows * channels >= 5.0e11)
        return dfm::set_error(DFM_ERR_UNSUPPORTED, "dfm_sparse_dense: a volume or a row block above the index range");
    if ((uintptr_t)coors & 15) return dfm::set_error(DFM_ERR_INVALID_ARG, "dfm_sparse_dense: coors is not 16-byte aligned");
    HIP_TRY(hipMemsetAsync(out, 0, (size_t)cells * sizeof(float), (hipStream_t)stream));
    if (rows == 0) return 0;
    dense_kernel<<<blocks(rows * channels), 256, 0, (hipStream_t)stream>>>(g, features, coors, rows, channels, out);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
