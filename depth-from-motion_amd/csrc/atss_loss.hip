// atss_loss.hip -- the 2-D ATSS head's loss over all of its pyramid levels (reference: LIGAATSSHead.loss_single and
// centerness_target, models/dense_heads/liga_atss_head.py:176-270, 380-397, under mmdet's ATSSHead.loss): the focal,
// centerness-weighted GIoU and centerness terms of every level and their gradients with respect to the 3 L maps.
//
// Semantics (include/dfm_hip_atss_loss.h, a part of include/dfm_hip.h, states them in full).  Per level the reference
// makes three permuted copies of the maps, a cat + gather for the class-specific deltas, a nonzero() (a wait for the
// host), four indexed gathers, three box decodes, an isnan().any() and a torch.any(weight > 0) (two more waits), and
// autograd walks all of it back; five levels, a dozen waits.  Here:
//   forward   one lane per (level, image, row), level-major, reads its label and its C class logits in place (any
//             strides) and, on a positive row only, its anchor, target deltas, four predicted deltas (of its own class)
//             and centerness logit; the 3 L + 1 sums go per wave by shuffles, per workgroup through LDS into one
//             partial row.  A second launch of one workgroup adds the partial rows in a fixed order.
//   backward  one lane per row writes its C + (4 or 4 C) + 1 gradient elements, zeros included: nothing is accumulated.
// One anchor per location: a wave's lanes are consecutive pixels, which is at once the anchor-fastest and the
// pixel-fastest order of csrc/anchor_loss.hip -- a contiguous run of a channel plane (NCHW), or rows one channel
// count apart (channels-last; the class map's C logits of a row are then one contiguous run).
// A wave may hold rows of two levels (a level of config K's head has 40 rows): each level's lanes are summed apart,
// and only the levels a wave holds cost it shuffles.
// No atomics, no memset: the same bits run after run.
#include "focal_loss.h"

using namespace dfm;

namespace {

constexpr int BLOCK = 256;             // four waves
constexpr int WAVES = BLOCK / 64;
constexpr int REDUCE_BLOCK = 1024;     // the one workgroup of the second launch
constexpr int REDUCE_WAVES = REDUCE_BLOCK / 64;
constexpr int LEVELS = DFM_ATSS_MAX_LEVELS;
constexpr int COLS = 3 * LEVELS + 1;   // a partial row: (S_cls, S_box, S_ctr) of each level slot, then T
constexpr float GIOU_EPS = 1e-6f;
constexpr float MAX_RATIO = 4.135166556742356f;     // |log(16 / 1000)|

struct Map {
    void *p;
    long long sb, sc, sh, sw;          // element strides: image, channel, row, column
};

struct Level {
    long long first;                   // the first lane of the level: batch * (rows of the levels before it)
    int hw, w, off, pad;               // rows of one image, the map's width, the row offset into the dense targets
    Map cls, reg, ctr, gcls, greg, gctr;
};

struct Loss {
    int batch, levels, a, c;           // A: rows of one image in the dense targets; C classes
    int agnostic, pad;
    long long rows;                    // batch * (rows of all levels)
    float gamma, alpha;
    float mean[4], std[4];
    const float *anchors, *label_weights, *bbox_targets, *grad_s;
    const long long *labels;
    Level lv[LEVELS];
};

struct Row {
    int level, b, y, x;
    long long r;                       // the row of the dense targets
    int n;                             // the row of anchors
};

__device__ __forceinline__ Row row_of(const Loss &L, long long i)
{
    Row o;
    o.level = 0;
    for (int l = 1; l < L.levels; ++l) o.level += i >= L.lv[l].first;
    const Level &v = L.lv[o.level];
    const long long j = i - v.first;
    o.b = (int)(j / v.hw);
    const int pos = (int)(j - (long long)o.b * v.hw);
    o.y = pos / v.w;
    o.x = pos - o.y * v.w;
    o.n = v.off + pos;
    o.r = (long long)o.b * L.a + o.n;
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

struct Box {
    float x1, y1, x2, y2;
};

// what the decode of one row keeps for the backward: the factors d box / d delta
struct Decode {
    Box box;
    float px, py, pw, ph, gw, gh;
    bool pass_w, pass_h;               // e_2 / e_3 inside the clamp
};

__device__ __forceinline__ Decode delta2bbox(const Loss &L, const float *an, const float *d)
{
    Decode o;
    const float e0 = d[0] * L.std[0] + L.mean[0], e1 = d[1] * L.std[1] + L.mean[1];
    const float e2 = d[2] * L.std[2] + L.mean[2], e3 = d[3] * L.std[3] + L.mean[3];
    o.pass_w = e2 >= -MAX_RATIO && e2 <= MAX_RATIO;
    o.pass_h = e3 >= -MAX_RATIO && e3 <= MAX_RATIO;
    const float ew = fminf(fmaxf(e2, -MAX_RATIO), MAX_RATIO), eh = fminf(fmaxf(e3, -MAX_RATIO), MAX_RATIO);
    o.px = (an[0] + an[2]) * 0.5f;
    o.py = (an[1] + an[3]) * 0.5f;
    o.pw = an[2] - an[0];
    o.ph = an[3] - an[1];
    const float gx = o.px + o.pw * e0, gy = o.py + o.ph * e1;
    o.gw = o.pw * expf(ew);
    o.gh = o.ph * expf(eh);
    o.box = Box{gx - o.gw * 0.5f, gy - o.gh * 0.5f, gx + o.gw * 0.5f, gy + o.gh * 0.5f};
    return o;
}

// the centerness target of an anchor centre (cx, cy) against its decoded target box; 0 for a product that is not > 0
__device__ __forceinline__ float centerness_target(float cx, float cy, const Box &g)
{
    const float l = cx - g.x1, t = cy - g.y1, r = g.x2 - cx, b = g.y2 - cy;
    const float q = __fdiv_rn(fminf(l, r), fmaxf(l, r)) * __fdiv_rn(fminf(t, b), fmaxf(t, b));
    return q > 0.0f ? __fsqrt_rn(q) : 0.0f;
}

// the share of the gradient of max(p, g) (UPPER) or min(p, g) that goes to p: 1 where p is it, half at a tie
template <bool UPPER>
__device__ __forceinline__ float picks(float p, float g)
{
    return p == g ? 0.5f : ((UPPER ? p > g : p < g) ? 1.0f : 0.0f);
}

// GIoU of the aligned pair (p, g); with GRAD, dg[k] = d GIoU / d (p.x1, p.y1, p.x2, p.y2)
template <bool GRAD>
__device__ __forceinline__ float giou(const Box &p, const Box &g, float *dg)
{
    const float w1 = p.x2 - p.x1, h1 = p.y2 - p.y1;
    const float area1 = w1 * h1, area2 = (g.x2 - g.x1) * (g.y2 - g.y1);
    const float iw_raw = fminf(p.x2, g.x2) - fmaxf(p.x1, g.x1), ih_raw = fminf(p.y2, g.y2) - fmaxf(p.y1, g.y1);
    const float iw = fmaxf(iw_raw, 0.0f), ih = fmaxf(ih_raw, 0.0f);
    const float overlap = iw * ih;
    const float union_raw = area1 + area2 - overlap;
    const float uni = fmaxf(union_raw, GIOU_EPS);
    const float iou = __fdiv_rn(overlap, uni);
    const float ew_raw = fmaxf(p.x2, g.x2) - fminf(p.x1, g.x1), eh_raw = fmaxf(p.y2, g.y2) - fminf(p.y1, g.y1);
    const float ew = fmaxf(ew_raw, 0.0f), eh = fmaxf(eh_raw, 0.0f);
    const float enclose_raw = ew * eh;
    const float enclose = fmaxf(enclose_raw, GIOU_EPS);
    if constexpr (GRAD) {
        // forward mode over the four coordinates of p, in the order x1, y1, x2, y2
        const float pass_iw = iw_raw >= 0.0f ? 1.0f : 0.0f, pass_ih = ih_raw >= 0.0f ? 1.0f : 0.0f;
        const float pass_ew = ew_raw >= 0.0f ? 1.0f : 0.0f, pass_eh = eh_raw >= 0.0f ? 1.0f : 0.0f;
        const float pass_u = union_raw >= GIOU_EPS ? 1.0f : 0.0f, pass_e = enclose_raw >= GIOU_EPS ? 1.0f : 0.0f;
        const float d_area[4] = {-h1, -w1, h1, w1};
        const float d_iw[4] = {-picks<true>(p.x1, g.x1) * pass_iw, 0.0f, picks<false>(p.x2, g.x2) * pass_iw, 0.0f};
        const float d_ih[4] = {0.0f, -picks<true>(p.y1, g.y1) * pass_ih, 0.0f, picks<false>(p.y2, g.y2) * pass_ih};
        const float d_ew[4] = {-picks<false>(p.x1, g.x1) * pass_ew, 0.0f, picks<true>(p.x2, g.x2) * pass_ew, 0.0f};
        const float d_eh[4] = {0.0f, -picks<false>(p.y1, g.y1) * pass_eh, 0.0f, picks<true>(p.y2, g.y2) * pass_eh};
        const float inv_u2 = __fdiv_rn(1.0f, uni * uni), inv_e2 = __fdiv_rn(1.0f, enclose * enclose);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float d_overlap = d_iw[k] * ih + iw * d_ih[k];
            const float d_union = pass_u * (d_area[k] - d_overlap);
            const float d_enclose = pass_e * (d_ew[k] * eh + ew * d_eh[k]);
            dg[k] = (d_overlap * uni - overlap * d_union) * inv_u2 + (d_union * enclose - uni * d_enclose) * inv_e2;
        }
    }
    return iou - __fdiv_rn(enclose - uni, enclose);
}

// bce_with_logits(z, t) for a target t in [0, 1]; with GRAD, grad = sigmoid(z) - t
template <bool GRAD>
__device__ __forceinline__ float bce_logits(float z, float t, float &grad)
{
    const float e = expf(-fabsf(z));
    if constexpr (GRAD) {
        float big, small;
        sigmoid_pair(e, big, small);
        grad = (z >= 0.0f ? big : small) - t;
    }
    return fmaxf(z, 0.0f) - z * t + log1pf(e);
}

// the inputs of a positive row: its anchor, its target box and centerness target, its predicted deltas' decode
template <typename TR>
__device__ __forceinline__ Decode positive_row(const Loss &L, const Level &v, const Row &o, int label, Box &gt,
                                               float &ct)
{
    const float4 an4 = ((const float4 *)L.anchors)[o.n], tg4 = ((const float4 *)L.bbox_targets)[o.r];
    const float an[4] = {an4.x, an4.y, an4.z, an4.w}, tg[4] = {tg4.x, tg4.y, tg4.z, tg4.w};
    const Decode t = delta2bbox(L, an, tg);
    gt = t.box;
    ct = centerness_target(t.px, t.py, gt);
    float d[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) d[s] = load<TR>(v.reg, o, L.agnostic ? s : s * L.c + label);
    return delta2bbox(L, an, d);
}

template <typename T, typename TR>
__global__ __launch_bounds__(BLOCK) void atss_loss_fwd_kernel(Loss L, float *__restrict__ partial)
{
    __shared__ float s_part[WAVES][COLS];
    const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
    const bool live = i < L.rows;
    float v[3] = {0.0f, 0.0f, 0.0f}, ct = 0.0f;
    int level = -1;
    if (live) {
        const Row o = row_of(L, i);
        const Level &lv = L.lv[o.level];
        level = o.level;
        const long long label = L.labels[o.r];
        const float lw = L.label_weights[o.r];
        float unused, acc = 0.0f;
        for (int c = 0; c < L.c; ++c) acc += focal<false>(load<T>(lv.cls, o, c), label == c, L.gamma, L.alpha, unused);
        v[0] = lw * acc;
        if (label >= 0 && label < L.c) {
            Box gt;
            const Decode p = positive_row<TR>(L, lv, o, (int)label, gt, ct);
            v[1] = ct * (1.0f - giou<false>(p.box, gt, nullptr));
            v[2] = bce_logits<false>(load<T>(lv.ctr, o, 0), ct, unused);
        }
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int l = 0; l < L.levels; ++l) {                       // (uniform) the levels this wave holds rows of
        const bool mine = level == l;
        float t[3] = {0.0f, 0.0f, 0.0f};
        if (__any(mine)) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                t[k] = mine ? v[k] : 0.0f;
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) t[k] += __shfl_down(t[k], off);
            }
        }
        if (lane == 0)
#pragma unroll
            for (int k = 0; k < 3; ++k) s_part[wave][3 * l + k] = t[k];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) ct += __shfl_down(ct, off);
    if (lane == 0) s_part[wave][3 * L.levels] = ct;
    __syncthreads();
    const int cols = 3 * L.levels + 1;
    if ((int)threadIdx.x < cols) {
        float t = s_part[0][threadIdx.x];
#pragma unroll
        for (int wv = 1; wv < WAVES; ++wv) t += s_part[wv][threadIdx.x];
        partial[(size_t)blockIdx.x * COLS + threadIdx.x] = t;
    }
}

// out[k] = the sum of column k of the partial rows, k < cols: one wave per column
__global__ __launch_bounds__(REDUCE_BLOCK) void atss_loss_reduce_kernel(const float *__restrict__ partial, int count,
                                                                        int cols, float *__restrict__ out)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int k = wave; k < cols; k += REDUCE_WAVES) {
        float t = 0.0f;
        for (int j = lane; j < count; j += 64) t += partial[(size_t)j * COLS + k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) t += __shfl_down(t, off);
        if (lane == 0) out[k] = t;
    }
}

template <typename T, typename TR>
__global__ __launch_bounds__(BLOCK) void atss_loss_bwd_kernel(Loss L)
{
    const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= L.rows) return;
    const Row o = row_of(L, i);
    const Level &lv = L.lv[o.level];
    const long long label = L.labels[o.r];
    const bool positive = label >= 0 && label < L.c;
    const float *gs = L.grad_s + 3 * o.level;
    if (lv.gcls.p != nullptr) {
        const float lw = L.label_weights[o.r];
        const float g0 = gs[0] * lw;
        for (int c = 0; c < L.c; ++c) {
            float g;
            focal<true>(load<T>(lv.cls, o, c), label == c, L.gamma, L.alpha, g);
            store<T>(lv.gcls, o, c, lw == 0.0f ? 0.0f : g0 * g);
        }
    }
    float g_reg[4] = {0.0f, 0.0f, 0.0f, 0.0f}, g_ctr = 0.0f;
    if (positive) {
        Box gt;
        float ct;
        const Decode p = positive_row<TR>(L, lv, o, (int)label, gt, ct);
        if (ct > 0.0f) {
            float dg[4];
            giou<true>(p.box, gt, dg);
            const float s = -gs[1] * ct;                       // d (ct (1 - GIoU)) / d GIoU, times grad_S_box
            const float gx1 = s * dg[0], gy1 = s * dg[1], gx2 = s * dg[2], gy2 = s * dg[3];
            g_reg[0] = (gx1 + gx2) * p.pw * L.std[0];
            g_reg[1] = (gy1 + gy2) * p.ph * L.std[1];
            g_reg[2] = p.pass_w ? (gx2 - gx1) * 0.5f * p.gw * L.std[2] : 0.0f;
            g_reg[3] = p.pass_h ? (gy2 - gy1) * 0.5f * p.gh * L.std[3] : 0.0f;
        }
        float d;
        bce_logits<true>(load<T>(lv.ctr, o, 0), ct, d);
        g_ctr = gs[2] * d;
    }
    if (lv.greg.p != nullptr) {
        if (L.agnostic) {
#pragma unroll
            for (int s = 0; s < 4; ++s) store<TR>(lv.greg, o, s, g_reg[s]);
        } else {
            for (int c = 0; c < L.c; ++c)
#pragma unroll
                for (int s = 0; s < 4; ++s) store<TR>(lv.greg, o, s * L.c + c, positive && c == label ? g_reg[s] : 0.0f);
        }
    }
    if (lv.gctr.p != nullptr) store<T>(lv.gctr, o, 0, g_ctr);
}

Map map_of(const void *p, const int64_t *stride)
{
    return Map{const_cast<void *>(p), stride[0], stride[1], stride[2], stride[3]};
}

// the checked sizes of a call: DFM_OK and the filled Loss (pointers aside), or the error; no HIP call
int check_desc(const dfm_atss_loss_desc *d, Loss &L)
{
    if (!d) return set_error(DFM_ERR_INVALID_ARG, "NULL descriptor");
    int rc = check_dtype(d->dtype);
    if (rc != DFM_OK) return rc;
    rc = check_dtype(d->reg_dtype);
    if (rc != DFM_OK) return rc;
    if (d->num_levels > LEVELS)
        return set_errorf(DFM_ERR_UNSUPPORTED, "%d levels: the loss is built for at most %d", d->num_levels, LEVELS);
    if (d->num_classes < 1) return set_errorf(DFM_ERR_UNSUPPORTED, "num_classes %d: at least 1", d->num_classes);
    if (d->num_levels < 1) return set_error(DFM_ERR_INVALID_ARG, "num_levels must be at least 1");
    if (d->batch < 0 || d->num_anchors < 0) return set_error(DFM_ERR_INVALID_ARG, "negative size");
    long long per_image = 0;
    for (int l = 0; l < d->num_levels; ++l) {
        if (d->h[l] < 0 || d->w[l] < 0 || d->row_offset[l] < 0) return set_error(DFM_ERR_INVALID_ARG, "negative size");
        const long long hw = (long long)d->h[l] * d->w[l];
        if (hw > 0x7fffffffll || per_image + hw > 0x7fffffffll || (per_image + hw) * d->batch > 0x7fffffffll)
            return set_error(DFM_ERR_UNSUPPORTED, "more than 2^31 - 1 rows in the batch");
        if (d->row_offset[l] + hw > d->num_anchors)
            return set_errorf(DFM_ERR_INVALID_ARG, "level %d (%d x %d rows from %d) lies outside the %d anchors", l,
                              d->h[l], d->w[l], d->row_offset[l], d->num_anchors);
        L.lv[l].first = per_image * d->batch;
        L.lv[l].hw = (int)hw;
        L.lv[l].w = d->w[l];
        L.lv[l].off = d->row_offset[l];
        L.lv[l].pad = 0;
        per_image += hw;
    }
    for (int l = d->num_levels; l < LEVELS; ++l) L.lv[l] = Level{};
    L.batch = d->batch;
    L.levels = d->num_levels;
    L.a = d->num_anchors;
    L.c = d->num_classes;
    L.agnostic = d->reg_class_agnostic != 0;
    L.pad = 0;
    L.rows = per_image * d->batch;
    L.gamma = d->gamma;
    L.alpha = d->alpha;
    for (int s = 0; s < 4; ++s) {
        L.mean[s] = d->target_means[s];
        L.std[s] = d->target_stds[s];
    }
    return DFM_OK;
}

size_t partial_rows(const Loss &L)
{
    return (size_t)((L.rows + BLOCK - 1) / BLOCK);
}

// the inputs both directions read; 0 or the error
int set_inputs(const dfm_atss_loss_desc *d, Loss &L, const void *const *maps, const float *anchors,
               const int64_t *labels, const float *label_weights, const float *bbox_targets)
{
    if (!maps || !anchors || !labels || !label_weights || !bbox_targets)
        return set_error(DFM_ERR_INVALID_ARG, "NULL device pointer");
    if (((uintptr_t)anchors | (uintptr_t)bbox_targets) & 15)
        return set_error(DFM_ERR_INVALID_ARG, "anchors and bbox_targets must be 16-byte aligned");
    for (int l = 0; l < L.levels; ++l) {
        if (L.lv[l].hw && (!maps[3 * l] || !maps[3 * l + 1] || !maps[3 * l + 2]))
            return set_errorf(DFM_ERR_INVALID_ARG, "NULL map pointer at level %d", l);
        L.lv[l].cls = map_of(maps[3 * l], d->cls_stride + 4 * l);
        L.lv[l].reg = map_of(maps[3 * l + 1], d->reg_stride + 4 * l);
        L.lv[l].ctr = map_of(maps[3 * l + 2], d->ctr_stride + 4 * l);
        L.lv[l].gcls = L.lv[l].greg = L.lv[l].gctr = Map{nullptr, 0, 0, 0, 0};
    }
    L.anchors = anchors;
    L.labels = (const long long *)labels;
    L.label_weights = label_weights;
    L.bbox_targets = bbox_targets;
    L.grad_s = nullptr;
    return DFM_OK;
}

}  // namespace

extern "C" DFM_API size_t dfm_atss_loss_workspace_bytes(const dfm_atss_loss_desc *d)
{
    Loss L;
    if (check_desc(d, L) != DFM_OK) return 0;
    return partial_rows(L) * COLS * sizeof(float);
}

extern "C" DFM_API int dfm_atss_loss_fwd(const dfm_atss_loss_desc *d, const void *const *maps, const float *anchors,
                                         const int64_t *labels, const float *label_weights,
                                         const float *bbox_targets, float *out, void *workspace,
                                         size_t workspace_bytes, void *stream)
{
    Loss L;
    int rc = check_desc(d, L);
    if (rc != DFM_OK) return rc;
    if (!out) return set_error(DFM_ERR_INVALID_ARG, "NULL device pointer");
    hipStream_t s = (hipStream_t)stream;
    const int cols = 3 * L.levels + 1;
    if (L.rows == 0) {
        HIP_TRY(hipMemsetAsync(out, 0, cols * sizeof(float), s));
        return DFM_OK;
    }
    rc = set_inputs(d, L, maps, anchors, labels, label_weights, bbox_targets);
    if (rc != DFM_OK) return rc;
    const size_t count = partial_rows(L), need = count * COLS * sizeof(float);
    if (!workspace || workspace_bytes < need)
        return set_errorf(DFM_ERR_WORKSPACE, "the ATSS loss needs %zu workspace bytes, got %zu", need,
                          workspace ? workspace_bytes : (size_t)0);
    if ((uintptr_t)workspace & 15) return set_error(DFM_ERR_INVALID_ARG, "workspace must be 16-byte aligned");
    float *partial = (float *)workspace;
    by_dtype(d->dtype, [&](auto t) {
        by_dtype(d->reg_dtype, [&](auto tr) {
            hipLaunchKernelGGL((atss_loss_fwd_kernel<decltype(t), decltype(tr)>), dim3((unsigned)count), dim3(BLOCK), 0,
                               s, L, partial);
        });
    });
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(atss_loss_reduce_kernel, dim3(1), dim3(REDUCE_BLOCK), 0, s, (const float *)partial, (int)count,
                       cols, out);
    HIP_TRY(hipGetLastError());
    return DFM_OK;
}

extern "C" DFM_API int dfm_atss_loss_bwd(const dfm_atss_loss_desc *d, const void *const *maps, const float *anchors,
                                         const int64_t *labels, const float *label_weights,
                                         const float *bbox_targets, const float *grad_S, void *const *grad_maps,
                                         void *stream)
{
    Loss L;
    int rc = check_desc(d, L);
    if (rc != DFM_OK) return rc;
    if (L.rows == 0) return DFM_OK;
    rc = set_inputs(d, L, maps, anchors, labels, label_weights, bbox_targets);
    if (rc != DFM_OK) return rc;
    if (!grad_S || !grad_maps) return set_error(DFM_ERR_INVALID_ARG, "NULL device pointer");
    bool any = false;
    for (int l = 0; l < L.levels; ++l) {
        L.lv[l].gcls = map_of(grad_maps[3 * l], d->grad_cls_stride + 4 * l);
        L.lv[l].greg = map_of(grad_maps[3 * l + 1], d->grad_reg_stride + 4 * l);
        L.lv[l].gctr = map_of(grad_maps[3 * l + 2], d->grad_ctr_stride + 4 * l);
        any = any || (L.lv[l].hw && (grad_maps[3 * l] || grad_maps[3 * l + 1] || grad_maps[3 * l + 2]));
    }
    if (!any) return DFM_OK;                                                  // nothing to write
    L.grad_s = grad_S;
    by_dtype(d->dtype, [&](auto t) {
        by_dtype(d->reg_dtype, [&](auto tr) {
            hipLaunchKernelGGL((atss_loss_bwd_kernel<decltype(t), decltype(tr)>), dim3((unsigned)partial_rows(L)),
                               dim3(BLOCK), 0, (hipStream_t)stream, L);
        });
    });
    HIP_TRY(hipGetLastError());
    return DFM_OK;
}
