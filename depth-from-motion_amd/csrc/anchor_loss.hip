// anchor_loss.hip -- the 3-D anchor head's loss_single on one level (reference: models/dense_heads/anchor3d_head.py
// :199-301 and liga_anchor3d_head.py:130-226): the focal, smooth-L1, direction and IoU terms and their gradients with
// respect to the three maps.
//
// Semantics (include/dfm_hip_anchor_loss.h, a part of include/dfm_hip.h, states them in full).  The reference makes
// three permuted copies of the maps, a dozen element-wise passes for the focal loss, labels.max().item() and nonzero()
// (two waits for the host), four indexed gathers and three reductions, and autograd walks all of it back.  Here:
//   forward   one lane per row (anchor of an image) reads its label, its C class logits in place (any strides) and,
//             on a positive row only, its S deltas, targets and weights, its two direction logits and its anchor;
//             the four terms are summed per wave by shuffles, per workgroup through LDS, and stored as one partial
//             row.  A second launch of one workgroup adds the partial rows in a fixed order and applies the scales.
//   backward  one lane per row writes its C + S + 2 gradient elements, zeros included: nothing is accumulated.
// Rows are taken anchor-fastest when the class map's channels are its fastest axis (channels-last: a wave reads one
// contiguous run per class) and pixel-fastest otherwise (NCHW: a wave reads a contiguous run of one channel plane);
// the labels are then read at a stride of A, the lesser evil: they are 8 + 4 bytes a row, the maps 4 C + ... .
// On a positive row the lane pays for the smooth-L1, the direction term and the IoU (the clip of two rectangles);
// positives are a few hundred among half a million rows, so most waves never take that branch.
// No atomics, no memset: the same bits run after run.
#include "bbox_coder.h"
#include "focal_loss.h"
#include "iou3d_geom.h"

using namespace dfm;

namespace {

constexpr int BLOCK = 256;             // four waves
constexpr int WAVES = BLOCK / 64;
constexpr int REDUCE_BLOCK = 1024;     // the one workgroup of the second launch
constexpr int REDUCE_WAVES = REDUCE_BLOCK / 64;
constexpr int CODE_MAX = DFM_ANCHOR_LOSS_MAX_CODE;
static_assert(CODE_MAX == BBOX_CODE_MAX, "the loss and the decode share the widest box code");

struct Map {
    void *p;
    long long sb, sc, sh, sw;          // element strides: image, channel, row, column
};

struct Loss {
    int batch, hw, w, a, c, s;         // pixels of a map, its width, A anchors per location, C classes, S columns
    int n;                             // anchors per image
    long long rows;                    // batch * n
    int has_dir, with_iou, sin_diff, pixel_major;
    float gamma, alpha, beta;
    float cw[CODE_MAX];
    Map cls, reg, dir, gcls, greg, gdir;
    const long long *labels, *dir_targets;
    const float *label_weights, *bbox_targets, *bbox_weights, *dir_weights, *anchors, *scale, *grad_out;
};

struct Row {
    int b, a, y, x;
    long long n, r;                    // the anchor of the image, the row of the targets
};

__device__ __forceinline__ Row row_of(const Loss &L, long long i)
{
    Row o;
    o.b = (int)(i / L.n);
    const int rem = (int)(i - (long long)o.b * L.n);
    int pos;
    if (L.pixel_major) {
        o.a = rem / L.hw;
        pos = rem - o.a * L.hw;
    } else {
        pos = rem / L.a;
        o.a = rem - pos * L.a;
    }
    o.y = pos / L.w;
    o.x = pos - o.y * L.w;
    o.n = (long long)pos * L.a + o.a;
    o.r = (long long)o.b * L.n + o.n;
    return o;
}

__device__ __forceinline__ long long at(const Map &m, const Row &o, int ch)
{
    return o.b * m.sb + ch * m.sc + o.y * m.sh + o.x * m.sw;
}

template <typename T>
__device__ __forceinline__ float load(const Map &m, const Row &o, int ch)
{
    return elem<T>::load(((const T *)m.p)[at(m, o, ch)]);
}

template <typename T>
__device__ __forceinline__ void store(const Map &m, const Row &o, int ch, float v)
{
    ((T *)m.p)[at(m, o, ch)] = elem<T>::store(v);
}

// (sigmoid_pair and the focal term of one logit: csrc/focal_loss.h, shared with csrc/atss_loss.hip)

// the cross entropy of two logits against class `one`; po = softmax probability of the OTHER class
__device__ __forceinline__ float cross_entropy2(float d0, float d1, bool one, float &po)
{
    const float z = one ? d0 - d1 : d1 - d0;                                  // other - target
    const float e = expf(-fabsf(z));
    float big, small;
    sigmoid_pair(e, big, small);
    po = z >= 0.0f ? big : small;
    return fmaxf(z, 0.0f) + log1pf(e);                                        // logsumexp(d0, d1) - d_target
}

// smooth-L1 of column s of a positive row: value, and dl = d value / d prediction
template <bool GRAD>
__device__ __forceinline__ float smooth_l1(const Loss &L, int s, float p, float t, float &dl)
{
    float d = p - t, dd = 1.0f;
    if (s == 6 && L.sin_diff) {                                               // add_sin_difference
        float sp, cp, st, ct;
        sincosf(p, &sp, &cp);
        sincosf(t, &st, &ct);
        d = sp * ct - cp * st;
        dd = cp * ct + sp * st;
    }
    const float ad = fabsf(d);
    const bool quad = ad < L.beta;
    if constexpr (GRAD) dl = (quad ? d / L.beta : copysignf(1.0f, d)) * dd;
    return quad ? 0.5f * d * d / L.beta : ad - 0.5f * L.beta;
}

template <typename T, bool IOU>
__global__ __launch_bounds__(BLOCK) void loss_fwd_kernel(Loss L, float4 *__restrict__ partial)
{
    __shared__ float s_part[WAVES][4];
    const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
    float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (i < L.rows) {
        const Row o = row_of(L, i);
        const long long label = L.labels[o.r];
        const float lw = L.label_weights[o.r];
        float unused, acc = 0.0f;
        for (int c = 0; c < L.c; ++c)
            acc += focal<false>(load<T>(L.cls, o, o.a * L.c + c), label == c, L.gamma, L.alpha, unused);
        v[0] = lw * acc;
        if (label >= 0 && label < L.c) {
            float pred[7], tgt[7], box = 0.0f;
#pragma unroll
            for (int s = 0; s < CODE_MAX; ++s)
                if (s < L.s) {
                    const float p = load<T>(L.reg, o, o.a * L.s + s), t = L.bbox_targets[o.r * L.s + s];
                    const float wgt = L.bbox_weights[o.r * L.s + s] * L.cw[s];
                    box += wgt * smooth_l1<false>(L, s, p, t, unused);
                    if (s < 7) {
                        pred[s] = p;
                        tgt[s] = t;
                    }
                }
            v[1] = box;
            if (L.has_dir)
                v[2] = L.dir_weights[o.r] * cross_entropy2(load<T>(L.dir, o, o.a * 2), load<T>(L.dir, o, o.a * 2 + 1),
                                                           L.dir_targets[o.r] != 0, unused);
            if constexpr (IOU) {
                float an[7], j[7];
#pragma unroll
                for (int s = 0; s < 7; ++s) an[s] = L.anchors[o.n * 7 + s];
                v[3] = iou3d_loss_row<false>(an, pred, tgt, j);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_down(v[k], off);
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int k = 0; k < 4; ++k) s_part[threadIdx.x >> 6][k] = v[k];
    __syncthreads();
    if (threadIdx.x == 0) {
        float t[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            t[k] = s_part[0][k];
#pragma unroll
            for (int wv = 1; wv < WAVES; ++wv) t[k] += s_part[wv][k];
        }
        partial[blockIdx.x] = make_float4(t[0], t[1], t[2], t[3]);
    }
}

// out[k] = scale[k] * (the sum of column k of the partial rows), 0 for a term the call does not have
__global__ __launch_bounds__(REDUCE_BLOCK) void loss_reduce_kernel(const float4 *__restrict__ partial, int count,
                                                                   const float *__restrict__ scale, int has_dir,
                                                                   int with_iou, float *__restrict__ out)
{
    __shared__ float s_part[REDUCE_WAVES][4];
    float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int j = threadIdx.x; j < count; j += REDUCE_BLOCK) {
        const float4 q = partial[j];
        v[0] += q.x;
        v[1] += q.y;
        v[2] += q.z;
        v[3] += q.w;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_down(v[k], off);
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int k = 0; k < 4; ++k) s_part[threadIdx.x >> 6][k] = v[k];
    __syncthreads();
    if (threadIdx.x < 4) {
        const int k = threadIdx.x;
        float t = s_part[0][k];
        for (int wv = 1; wv < REDUCE_WAVES; ++wv) t += s_part[wv][k];
        const bool present = k < 2 || (k == 2 ? has_dir != 0 : with_iou != 0);
        out[k] = present ? scale[k] * t : 0.0f;
    }
}

template <typename T, bool IOU>
__global__ __launch_bounds__(BLOCK) void loss_bwd_kernel(Loss L)
{
    const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= L.rows) return;
    const Row o = row_of(L, i);
    const long long label = L.labels[o.r];
    const bool positive = label >= 0 && label < L.c;
    if (L.gcls.p != nullptr) {                                                // (uniform)
        const float lw = L.label_weights[o.r];
        const float g0 = L.grad_out[0] * L.scale[0] * lw;
        for (int c = 0; c < L.c; ++c) {
            float g;
            focal<true>(load<T>(L.cls, o, o.a * L.c + c), label == c, L.gamma, L.alpha, g);
            store<T>(L.gcls, o, o.a * L.c + c, lw == 0.0f ? 0.0f : g0 * g);
        }
    }
    if (L.greg.p != nullptr) {
        if (positive) {
            const float g1 = L.grad_out[1] * L.scale[1];
            float pred[7], tgt[7], g[CODE_MAX];
#pragma unroll
            for (int s = 0; s < CODE_MAX; ++s)
                if (s < L.s) {
                    const float p = load<T>(L.reg, o, o.a * L.s + s), t = L.bbox_targets[o.r * L.s + s];
                    const float wgt = L.bbox_weights[o.r * L.s + s] * L.cw[s];
                    float dl;
                    smooth_l1<true>(L, s, p, t, dl);
                    g[s] = g1 * wgt * dl;
                    if (s < 7) {
                        pred[s] = p;
                        tgt[s] = t;
                    }
                }
            if constexpr (IOU) {
                const float g3 = L.grad_out[3] * L.scale[3];
                float an[7], j[7];
#pragma unroll
                for (int s = 0; s < 7; ++s) an[s] = L.anchors[o.n * 7 + s];
                iou3d_loss_row<true>(an, pred, tgt, j);
#pragma unroll
                for (int s = 0; s < 7; ++s) g[s] += g3 * j[s];
            }
#pragma unroll
            for (int s = 0; s < CODE_MAX; ++s)
                if (s < L.s) store<T>(L.greg, o, o.a * L.s + s, g[s]);
        } else {
            for (int s = 0; s < L.s; ++s) store<T>(L.greg, o, o.a * L.s + s, 0.0f);
        }
    }
    if (L.has_dir && L.gdir.p != nullptr) {
        float g0 = 0.0f, g1 = 0.0f;
        if (positive) {
            const bool one = L.dir_targets[o.r] != 0;
            float po;
            cross_entropy2(load<T>(L.dir, o, o.a * 2), load<T>(L.dir, o, o.a * 2 + 1), one, po);
            const float g = L.grad_out[2] * L.scale[2] * L.dir_weights[o.r] * po;       // to the other class's logit
            g0 = one ? g : -g;
            g1 = -g0;
        }
        store<T>(L.gdir, o, o.a * 2, g0);
        store<T>(L.gdir, o, o.a * 2 + 1, g1);
    }
}

Map map_of(const void *p, const int64_t *stride)
{
    return Map{const_cast<void *>(p), stride[0], stride[1], stride[2], stride[3]};
}

// the checked sizes of a call: DFM_OK and the filled Loss (pointers aside), or the error; no HIP call
int check_desc(const dfm_anchor_loss_desc *d, Loss &L)
{
    if (!d) return set_error(DFM_ERR_INVALID_ARG, "NULL descriptor");
    const int rc = check_dtype(d->dtype);
    if (rc != DFM_OK) return rc;
    if (d->box_code_size < BBOX_CODE_MIN || d->box_code_size > BBOX_CODE_MAX)
        return set_errorf(DFM_ERR_UNSUPPORTED, "box_code_size %d: the loss is built for %d .. %d columns",
                          d->box_code_size, BBOX_CODE_MIN, BBOX_CODE_MAX);
    if (d->with_iou && d->box_code_size != 7)
        return set_errorf(DFM_ERR_UNSUPPORTED, "box_code_size %d with the IoU term: it is built for 7 columns",
                          d->box_code_size);
    if (d->num_classes < 1) return set_errorf(DFM_ERR_UNSUPPORTED, "num_classes %d: at least 1", d->num_classes);
    if (d->batch < 0 || d->h < 0 || d->w < 0) return set_error(DFM_ERR_INVALID_ARG, "negative size");
    if (d->anchors_per_location <= 0) return set_error(DFM_ERR_INVALID_ARG, "non-positive anchors_per_location");
    if (!(d->beta > 0.0f)) return set_error(DFM_ERR_INVALID_ARG, "beta must be positive");
    const long long hw = (long long)d->h * d->w;
    const long long n = hw * d->anchors_per_location;                        // < 2^31 * 2^31 * 2^31: check in steps
    if (hw > 0x7fffffffll || n > 0x7fffffffll || n * d->batch > 0x7fffffffll)
        return set_error(DFM_ERR_UNSUPPORTED, "more than 2^31 - 1 anchors in the batch");
    L.batch = d->batch;
    L.hw = (int)hw;
    L.w = d->w;
    L.a = d->anchors_per_location;
    L.c = d->num_classes;
    L.s = d->box_code_size;
    L.n = (int)n;
    L.rows = n * d->batch;
    L.has_dir = d->has_dir != 0;
    L.with_iou = d->with_iou != 0;
    L.sin_diff = d->diff_rad_by_sin != 0;
    L.pixel_major = d->cls_stride[3] < d->cls_stride[1];
    L.gamma = d->gamma;
    L.alpha = d->alpha;
    L.beta = d->beta;
    for (int s = 0; s < CODE_MAX; ++s) L.cw[s] = d->code_weight[s];
    return DFM_OK;
}

size_t partial_rows(const Loss &L)
{
    return (size_t)((L.rows + BLOCK - 1) / BLOCK);
}

// the inputs both directions read; 0 or the error
int set_inputs(const dfm_anchor_loss_desc *d, Loss &L, const void *cls, const void *reg, const void *dir,
               const int64_t *labels, const float *label_weights, const float *bbox_targets, const float *bbox_weights,
               const int64_t *dir_targets, const float *dir_weights, const float *anchors, const float *scale)
{
    if (!cls || !reg || !labels || !label_weights || !bbox_targets || !bbox_weights || !scale)
        return set_error(DFM_ERR_INVALID_ARG, "NULL device pointer");
    if (L.has_dir && (!dir || !dir_targets || !dir_weights))
        return set_error(DFM_ERR_INVALID_ARG, "has_dir without the direction map, dir_targets or dir_weights");
    if (L.with_iou && !anchors) return set_error(DFM_ERR_INVALID_ARG, "with_iou without anchors");
    L.cls = map_of(cls, d->cls_stride);
    L.reg = map_of(reg, d->reg_stride);
    L.dir = map_of(dir, d->dir_stride);
    L.labels = (const long long *)labels;
    L.dir_targets = (const long long *)dir_targets;
    L.label_weights = label_weights;
    L.bbox_targets = bbox_targets;
    L.bbox_weights = bbox_weights;
    L.dir_weights = dir_weights;
    L.anchors = anchors;
    L.scale = scale;
    L.grad_out = nullptr;
    L.gcls = L.greg = L.gdir = Map{nullptr, 0, 0, 0, 0};
    return DFM_OK;
}

}  // namespace

extern "C" DFM_API size_t dfm_anchor3d_loss_workspace_bytes(const dfm_anchor_loss_desc *d)
{
    Loss L;
    if (check_desc(d, L) != DFM_OK) return 0;
    return partial_rows(L) * sizeof(float4);
}

extern "C" DFM_API int dfm_anchor3d_loss_fwd(const dfm_anchor_loss_desc *d, const void *cls, const void *reg,
                                             const void *dir, const int64_t *labels, const float *label_weights,
                                             const float *bbox_targets, const float *bbox_weights,
                                             const int64_t *dir_targets, const float *dir_weights,
                                             const float *anchors, const float *scale, float *out, void *workspace,
                                             size_t workspace_bytes, void *stream)
{
    Loss L;
    int rc = check_desc(d, L);
    if (rc != DFM_OK) return rc;
    if (!out) return set_error(DFM_ERR_INVALID_ARG, "NULL device pointer");
    hipStream_t s = (hipStream_t)stream;
    if (L.rows == 0) {
        HIP_TRY(hipMemsetAsync(out, 0, 4 * sizeof(float), s));
        return DFM_OK;
    }
    rc = set_inputs(d, L, cls, reg, dir, labels, label_weights, bbox_targets, bbox_weights, dir_targets, dir_weights,
                    anchors, scale);
    if (rc != DFM_OK) return rc;
    const size_t count = partial_rows(L), need = count * sizeof(float4);
    if (!workspace || workspace_bytes < need)
        return set_errorf(DFM_ERR_WORKSPACE, "the anchor loss needs %zu workspace bytes, got %zu", need,
                          workspace ? workspace_bytes : (size_t)0);
    if ((uintptr_t)workspace & 15) return set_error(DFM_ERR_INVALID_ARG, "workspace must be 16-byte aligned");
    float4 *partial = (float4 *)workspace;
    by_dtype(d->dtype, [&](auto t) {
        by_bool(L.with_iou, [&](auto iou) {
            hipLaunchKernelGGL((loss_fwd_kernel<decltype(t), decltype(iou)::value>), dim3((unsigned)count), dim3(BLOCK),
                               0, s, L, partial);
        });
    });
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(loss_reduce_kernel, dim3(1), dim3(REDUCE_BLOCK), 0, s, (const float4 *)partial, (int)count, scale,
                       L.has_dir, L.with_iou, out);
    HIP_TRY(hipGetLastError());
    return DFM_OK;
}

extern "C" DFM_API int dfm_anchor3d_loss_bwd(const dfm_anchor_loss_desc *d, const void *cls, const void *reg,
                                             const void *dir, const int64_t *labels, const float *label_weights,
                                             const float *bbox_targets, const float *bbox_weights,
                                             const int64_t *dir_targets, const float *dir_weights,
                                             const float *anchors, const float *scale, const float *grad_out,
                                             void *grad_cls, void *grad_reg, void *grad_dir, void *stream)
{
    Loss L;
    int rc = check_desc(d, L);
    if (rc != DFM_OK) return rc;
    if (L.rows == 0) return DFM_OK;
    rc = set_inputs(d, L, cls, reg, dir, labels, label_weights, bbox_targets, bbox_weights, dir_targets, dir_weights,
                    anchors, scale);
    if (rc != DFM_OK) return rc;
    if (!grad_out) return set_error(DFM_ERR_INVALID_ARG, "NULL device pointer");
    if (!grad_cls && !grad_reg && !(L.has_dir && grad_dir)) return DFM_OK;      // nothing to write
    L.grad_out = grad_out;
    L.gcls = map_of(grad_cls, d->grad_cls_stride);
    L.greg = map_of(grad_reg, d->grad_reg_stride);
    L.gdir = map_of(grad_dir, d->grad_dir_stride);
    by_dtype(d->dtype, [&](auto t) {
        by_bool(L.with_iou, [&](auto iou) {
            hipLaunchKernelGGL((loss_bwd_kernel<decltype(t), decltype(iou)::value>), dim3((unsigned)partial_rows(L)),
                               dim3(BLOCK), 0, (hipStream_t)stream, L);
        });
    });
    HIP_TRY(hipGetLastError());
    return DFM_OK;
}
