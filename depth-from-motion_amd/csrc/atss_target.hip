// atss_target.hip -- 2-D box overlaps and the training targets of the 2-D ATSS head
// (reference: core/bbox/assigners/atss_3dcenter_assigner.py:27-168 ATSS3DCenterAssigner.assign inside
// models/dense_heads/liga_atss_head.py:399-483 LIGAATSSHead._get_target_single, over mmdet's bbox_overlaps,
// anchor_inside_flags, PseudoSampler, DeltaXYWHBBoxCoder.encode and unmap, once per image under ATSSHead.get_targets).
//
// Semantics (include/dfm_hip_atss_target.h states them in full).  The reference builds, per image, an A x G overlap
// matrix and an A x G distance matrix and walks them with a topk per level, a Python loop over the GT boxes and a
// G x A scatter; here neither matrix exists:
//   select    one workgroup per (GT, level).  Round r finds the workgroup-wide minimum of the 64-bit keys
//             (distance bits << 32 | anchor index) that lie strictly above round r - 1's: a non-negative float's
//             bits order as the float does, the index in the low word makes the lowest anchor win a tie, and
//             "strictly above the last" replaces a sort and an LDS table of the level.  The distance is recomputed
//             per round (two subtractions, two products, a sum, a square root).  k_l = min(topk, counting anchors)
//             falls out: a round that finds no key ends the search.  Lane 0 writes the winner's index and overlap.
//   claim     one wave per GT: mean and unbiased std of its <= 128 candidate overlaps in fp64, the threshold and
//             centre-in-box tests, and per positive ONE 64-bit atomic max of (iou bits << 32 | 0xFFFFFFFF - GT index)
//             on the anchor's key.  The low word of a claim is never 0, so a zeroed key means "nobody" and an
//             overlap of 0.0 can still win.  One more workgroup zeroes the counts.
//   finalize  one lane per (image, anchor): decode the key, encode, write the dense rows (the 4-wide rows are one
//             16-byte store per lane: consecutive lanes, consecutive addresses), count with a ballot and one atomic
//             add per wave and counter.
// Phase boundaries are launch boundaries; no kernel waits for another workgroup.  Every loop is bounded by topk, the
// level sizes, the batch or the GT offsets, which the entry point checks on the host.
#include "dfm_common.h"

using namespace dfm;

namespace {

constexpr int BLOCK = 256;         // four waves
constexpr int WAVES = BLOCK / 64;
constexpr int MAX_LEVELS = DFM_ATSS_MAX_LEVELS;
constexpr int MAX_TOPK = DFM_ATSS_MAX_TOPK;
constexpr int MAX_BATCH = DFM_ATSS_MAX_BATCH;
constexpr unsigned long long NO_KEY = ~0ull;

// mmdet's bbox_overlaps of two boxes (x1, y1, x2, y2), fp32, eps 1e-6; iof: over the first box's area
__device__ __forceinline__ float overlap_2d(const float4 &a, const float4 &b, bool iof)
{
    const float area1 = (a.z - a.x) * (a.w - a.y);
    const float area2 = (b.z - b.x) * (b.w - b.y);
    const float w = fmaxf(fminf(a.z, b.z) - fmaxf(a.x, b.x), 0.0f);
    const float h = fmaxf(fminf(a.w, b.w) - fmaxf(a.y, b.y), 0.0f);
    const float overlap = w * h;
    const float uni = iof ? area1 : (area1 + area2) - overlap;
    return __fdiv_rn(overlap, fmaxf(uni, 1e-6f));
}

__global__ __launch_bounds__(BLOCK) void bbox_overlaps_2d_kernel(const float4 *__restrict__ b1, int n,
                                                                 const float4 *__restrict__ b2, int m, int iof,
                                                                 int aligned, float *__restrict__ out)
{
    const long long total = aligned ? (long long)n : (long long)n * m;
    const long long e = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (e >= total) return;
    const long long i = aligned ? e : e / m, j = aligned ? e : e - i * m;
    out[e] = overlap_2d(b1[i], b2[j], iof != 0);
}

struct Params {
    int num_anchors;     // A
    int levels, batch, topk;
    int gt_width;        // 4 or 6
    int total_gt;
    int num_classes;
    float pos_weight;
    float means[4], stds[4];
    int level_start[MAX_LEVELS + 1];
    int gt_offsets[MAX_BATCH + 1];   // entries beyond batch repeat total_gt
};

// the image that owns row g of the packed GT tensor (g < total_gt): the last b with gt_offsets[b] <= g
__device__ __forceinline__ int image_of(const Params &p, int g)
{
    int b = 0;
    for (int i = 1; i < p.batch; ++i) b = p.gt_offsets[i] <= g ? i : b;
    return b;
}

__device__ __forceinline__ float4 gt_box(const float *__restrict__ gt, int width, int g)
{
    const float *row = gt + (size_t)g * width;
    return make_float4(row[0], row[1], row[2], row[3]);
}

__device__ __forceinline__ unsigned long long wave_min(unsigned long long v)
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const unsigned long long o = __shfl_xor(v, s);
        v = o < v ? o : v;
    }
    return v;
}

// grid = total_gt * levels workgroups, workgroup w = (GT w / levels, level w % levels)
__global__ __launch_bounds__(BLOCK) void atss_select_kernel(const float4 *__restrict__ anchors,
                                                            const unsigned char *__restrict__ inside,
                                                            const float *__restrict__ gt, Params p,
                                                            int *__restrict__ cand_idx, float *__restrict__ cand_iou)
{
    __shared__ unsigned long long s_min[WAVES];
    const int g = blockIdx.x / p.levels, level = blockIdx.x - g * p.levels;
    const int img = image_of(p, g);
    const int a0 = p.level_start[level], a1 = p.level_start[level + 1];
    const float4 box = gt_box(gt, p.gt_width, g);
    float gx, gy;
    if (p.gt_width == 6) {
        gx = gt[(size_t)g * 6 + 4];
        gy = gt[(size_t)g * 6 + 5];
    } else {
        gx = (box.x + box.z) / 2.0f;
        gy = (box.y + box.w) / 2.0f;
    }
    const unsigned char *flags = inside ? inside + (size_t)img * p.num_anchors : nullptr;
    const size_t row = ((size_t)g * p.levels + level) * p.topk;
    unsigned long long prev = 0;
    bool first = true, done = false;
    for (int r = 0; r < p.topk; ++r) {
        unsigned long long best = NO_KEY;
        if (!done) {
            for (int a = a0 + (int)threadIdx.x; a < a1; a += BLOCK) {
                if (flags && flags[a] == 0) continue;
                const float4 an = anchors[a];
                const float dx = (an.x + an.z) / 2.0f - gx, dy = (an.y + an.w) / 2.0f - gy;
                const float d = __fsqrt_rn(dx * dx + dy * dy);
                const unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)a;
                if ((first || key > prev) && key < best) best = key;
            }
            best = wave_min(best);
        }
        if ((threadIdx.x & 63) == 0) s_min[threadIdx.x >> 6] = best;
        __syncthreads();
        best = s_min[0];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) best = s_min[w] < best ? s_min[w] : best;
        __syncthreads();
        if (best == NO_KEY) done = true;            // (uniform) fewer counting anchors than topk
        if (threadIdx.x == 0) {
            int idx = -1;
            float iou = 0.0f;
            if (!done) {
                idx = (int)(unsigned)best;
                iou = overlap_2d(anchors[idx], box, false);
            }
            cand_idx[row + r] = idx;
            cand_iou[row + r] = iou;
        }
        prev = best;
        first = false;
    }
}

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s);
    return v;
}

// grid = total_gt + 1 workgroups of one wave: workgroup g < total_gt claims for GT g, the last one zeroes counts
__global__ __launch_bounds__(64) void atss_claim_kernel(const float4 *__restrict__ anchors,
                                                        const float *__restrict__ gt, Params p,
                                                        const int *__restrict__ cand_idx,
                                                        const float *__restrict__ cand_iou,
                                                        unsigned long long *__restrict__ keys,
                                                        int *__restrict__ counts)
{
    const int g = blockIdx.x, lane = threadIdx.x;
    if (g >= p.total_gt) {
        for (int i = lane; i < p.batch * 2; i += 64) counts[i] = 0;   // finalize adds into them
        return;
    }
    const int img = image_of(p, g);
    const int entries = p.levels * p.topk;                            // <= 128: two per lane
    const size_t row = (size_t)g * entries;
    int idx[2];
    float iou[2];
    double sum = 0.0;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int e = lane + 64 * k;
        idx[k] = e < entries ? cand_idx[row + e] : -1;
        iou[k] = idx[k] >= 0 ? cand_iou[row + e] : 0.0f;
        if (idx[k] >= 0) sum += (double)iou[k];
    }
    const int n = __popcll(__ballot(idx[0] >= 0)) + __popcll(__ballot(idx[1] >= 0));
    if (n <= 1) return;                                               // (uniform) the reference's NaN threshold
    const double mean = wave_sum(sum) / n;
    double sq = 0.0;
#pragma unroll
    for (int k = 0; k < 2; ++k)
        if (idx[k] >= 0) sq += ((double)iou[k] - mean) * ((double)iou[k] - mean);
    const double thr = mean + sqrt(wave_sum(sq) / (n - 1));
    const float4 box = gt_box(gt, p.gt_width, g);
    const unsigned local = (unsigned)(g - p.gt_offsets[img]);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        if (idx[k] < 0 || !((double)iou[k] >= thr)) continue;
        const float4 an = anchors[idx[k]];
        const float cx = (an.x + an.z) / 2.0f, cy = (an.y + an.w) / 2.0f;
        const float inset = fminf(fminf(cx - box.x, cy - box.y), fminf(box.z - cx, box.w - cy));
        if (!(inset > 0.01f)) continue;
        const unsigned long long key = ((unsigned long long)__float_as_uint(iou[k]) << 32) | (0xFFFFFFFFu - local);
        atomicMax(keys + (size_t)img * p.num_anchors + idx[k], key);
    }
}

// grid = (ceil(A / BLOCK), batch)
__global__ __launch_bounds__(BLOCK) void atss_finalize_kernel(const float4 *__restrict__ anchors,
                                                              const unsigned char *__restrict__ inside,
                                                              const float *__restrict__ gt,
                                                              const long long *__restrict__ gt_labels, Params p,
                                                              const unsigned long long *__restrict__ keys,
                                                              long long *__restrict__ labels,
                                                              float *__restrict__ label_weights,
                                                              float4 *__restrict__ bbox_targets,
                                                              float4 *__restrict__ bbox_weights,
                                                              long long *__restrict__ assigned,
                                                              int *__restrict__ counts)
{
    const int img = blockIdx.y;
    const long long a = (long long)blockIdx.x * BLOCK + threadIdx.x;
    const bool valid = a < p.num_anchors;
    const size_t o = (size_t)img * p.num_anchors + (valid ? a : 0);
    const bool counting = valid && (inside == nullptr || inside[o] != 0);
    const unsigned long long key = counting && p.total_gt > 0 ? keys[o] : 0ull;
    const bool pos = key != 0ull;
    long long label = p.num_classes, which = counting ? 0 : -1;
    float4 target = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (pos) {
        const int local = (int)(0xFFFFFFFFu - (unsigned)key);
        const int g = p.gt_offsets[img] + local;
        const float4 an = anchors[a], box = gt_box(gt, p.gt_width, g);
        // DeltaXYWHBBoxCoder.encode = bbox2delta, in its operation order
        const float px = (an.x + an.z) * 0.5f, py = (an.y + an.w) * 0.5f, pw = an.z - an.x, ph = an.w - an.y;
        const float gx = (box.x + box.z) * 0.5f, gy = (box.y + box.w) * 0.5f, gw = box.z - box.x, gh = box.w - box.y;
        target.x = __fdiv_rn(__fdiv_rn(gx - px, pw) - p.means[0], p.stds[0]);
        target.y = __fdiv_rn(__fdiv_rn(gy - py, ph) - p.means[1], p.stds[1]);
        target.z = __fdiv_rn(logf(__fdiv_rn(gw, pw)) - p.means[2], p.stds[2]);
        target.w = __fdiv_rn(logf(__fdiv_rn(gh, ph)) - p.means[3], p.stds[3]);
        label = gt_labels ? gt_labels[g] : 0;
        which = local + 1;
    }
    if (valid) {
        const float w = pos ? 1.0f : 0.0f;
        labels[o] = label;
        label_weights[o] = pos ? (p.pos_weight > 0.0f ? p.pos_weight : 1.0f) : (counting ? 1.0f : 0.0f);
        bbox_targets[o] = target;
        bbox_weights[o] = make_float4(w, w, w, w);
        assigned[o] = which;
    }
    const int n_pos = __popcll(__ballot(pos)), n_neg = __popcll(__ballot(counting && !pos));
    if ((threadIdx.x & 63) == 0) {
        if (n_pos) atomicAdd(counts + img * 2, n_pos);
        if (n_neg) atomicAdd(counts + img * 2 + 1, n_neg);
    }
}

size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

// "" when the descriptor is one the kernels cover and well formed, else the reason; *code gets the status
const char *check_desc(const dfm_atss_target_desc *d, int *code)
{
    *code = DFM_ERR_UNSUPPORTED;
    if (d->thresh_mode != DFM_ATSS_THRESH_MEANSTD) return "thresh_mode: only 'meanstd' (mean + std) is built";
    if (d->reg_width != 4) return "reg_width: the targets are built for 4 regression channels";
    if (d->coder != DFM_ATSS_CODER_DELTA_XYWH) return "coder: only DeltaXYWHBBoxCoder is built";
    if (d->sampler != DFM_SAMPLER_PSEUDO) return "only the pseudo sampler (every assigned anchor is kept) is built";
    if (d->ignore_iof_thr > 0.0f && d->num_ignore_boxes > 0)
        return "ignore regions (ignore_iof_thr > 0 with ignore boxes) are not built";
    *code = DFM_ERR_INVALID_ARG;
    if (d->num_anchors < 0 || d->batch < 0 || d->num_ignore_boxes < 0) return "negative size";
    if (d->topk < 1 || d->topk > MAX_TOPK) return "topk outside 1 .. DFM_ATSS_MAX_TOPK = 16";
    if (d->num_levels < 1 || d->num_levels > MAX_LEVELS) return "num_levels outside 1 .. DFM_ATSS_MAX_LEVELS = 8";
    if (d->batch > MAX_BATCH) return "batch above DFM_ATSS_MAX_BATCH = 64 images per call";
    if (d->gt_width != 4 && d->gt_width != 6) return "gt_width must be 4 (box) or 6 (box and point)";
    *code = DFM_OK;
    return "";
}

}  // namespace

extern "C" DFM_API int dfm_bbox_overlaps_2d(const float *boxes1, int32_t n, const float *boxes2, int32_t m,
                                            int32_t mode, int32_t aligned, float *out, void *stream)
{
    if (n < 0 || m < 0) return set_error(DFM_ERR_INVALID_ARG, "negative box count");
    if (mode != DFM_OVERLAP_IOU && mode != DFM_OVERLAP_IOF)
        return set_errorf(DFM_ERR_INVALID_ARG, "mode %d: DFM_OVERLAP_IOU or DFM_OVERLAP_IOF", mode);
    if (aligned && n != m) return set_error(DFM_ERR_INVALID_ARG, "aligned overlaps need as many boxes2 as boxes1");
    if (n == 0 || m == 0) return DFM_OK;
    if (!boxes1 || !boxes2 || !out) return set_error(DFM_ERR_INVALID_ARG, "NULL device pointer");
    if (((uintptr_t)boxes1 | (uintptr_t)boxes2) & 15)
        return set_error(DFM_ERR_INVALID_ARG, "boxes must be 16-byte aligned");
    const long long total = aligned ? (long long)n : (long long)n * m;
    const long long blocks = (total + BLOCK - 1) / BLOCK;
    if (blocks > 0x7fffffffll) return set_error(DFM_ERR_UNSUPPORTED, "overlap matrix too large");
    hipLaunchKernelGGL(bbox_overlaps_2d_kernel, dim3((unsigned)blocks), dim3(BLOCK), 0, (hipStream_t)stream,
                       (const float4 *)boxes1, n, (const float4 *)boxes2, m, mode == DFM_OVERLAP_IOF, aligned, out);
    HIP_TRY(hipGetLastError());
    return DFM_OK;
}

extern "C" DFM_API size_t dfm_atss_target_workspace_bytes(const dfm_atss_target_desc *d, int32_t total_gt)
{
    int code;
    if (!d || total_gt < 0) return 0;
    check_desc(d, &code);
    if (code != DFM_OK || d->batch == 0 || d->num_anchors == 0) return 0;
    const size_t keys = align16((size_t)d->batch * (size_t)d->num_anchors * sizeof(unsigned long long));
    const size_t table = align16((size_t)total_gt * d->num_levels * d->topk * sizeof(int32_t));
    return keys + 2 * table;
}

extern "C" DFM_API int dfm_atss_target_2d(const dfm_atss_target_desc *d, const float *anchors,
                                          const int32_t *level_sizes, const uint8_t *inside, const float *gt_boxes,
                                          const int32_t *gt_offsets, const int64_t *gt_labels, int64_t *labels,
                                          float *label_weights, float *bbox_targets, float *bbox_weights,
                                          int64_t *assigned_gt_inds, int32_t *counts, void *workspace,
                                          size_t workspace_bytes, void *stream)
{
    if (!d) return set_error(DFM_ERR_INVALID_ARG, "NULL descriptor");
    int code;
    const char *why = check_desc(d, &code);
    if (code != DFM_OK) return set_error(code, why);
    if (d->batch == 0 || d->num_anchors == 0) return DFM_OK;
    if (!level_sizes) return set_error(DFM_ERR_INVALID_ARG, "NULL level_sizes");
    Params p;
    long long sum = 0;
    for (int l = 0; l <= MAX_LEVELS; ++l) {          // levels beyond num_levels are empty
        p.level_start[l] = (int)sum;
        if (l < d->num_levels) {
            if (level_sizes[l] < 0) return set_error(DFM_ERR_INVALID_ARG, "negative level size");
            sum += level_sizes[l];
            if (sum > d->num_anchors) return set_error(DFM_ERR_INVALID_ARG, "level_sizes must sum to num_anchors");
        }
    }
    if (sum != d->num_anchors) return set_error(DFM_ERR_INVALID_ARG, "level_sizes must sum to num_anchors");
    if (!gt_offsets) return set_error(DFM_ERR_INVALID_ARG, "NULL gt_offsets");
    if (gt_offsets[0] != 0) return set_error(DFM_ERR_INVALID_ARG, "gt_offsets[0] must be 0");
    for (int b = 0; b < d->batch; ++b)
        if (gt_offsets[b + 1] < gt_offsets[b]) return set_error(DFM_ERR_INVALID_ARG, "gt_offsets must not decrease");
    const int total_gt = gt_offsets[d->batch];
    if (!anchors || !labels || !label_weights || !bbox_targets || !bbox_weights || !assigned_gt_inds || !counts)
        return set_error(DFM_ERR_INVALID_ARG, "NULL device pointer");
    if (((uintptr_t)anchors | (uintptr_t)bbox_targets | (uintptr_t)bbox_weights) & 15)
        return set_error(DFM_ERR_INVALID_ARG, "anchors, bbox_targets and bbox_weights must be 16-byte aligned");
    if (total_gt > 0 && !gt_boxes) return set_error(DFM_ERR_INVALID_ARG, "NULL gt_boxes");
    const long long select_blocks = (long long)total_gt * d->num_levels;
    if (select_blocks > 0x7fffffffll) return set_error(DFM_ERR_UNSUPPORTED, "too many GT boxes for one call");
    const size_t need = dfm_atss_target_workspace_bytes(d, total_gt);
    if (!workspace || workspace_bytes < need)
        return set_errorf(DFM_ERR_WORKSPACE, "ATSS targets need %zu workspace bytes, got %zu", need,
                          workspace ? workspace_bytes : (size_t)0);
    if ((uintptr_t)workspace & 15) return set_error(DFM_ERR_INVALID_ARG, "workspace must be 16-byte aligned");
    p.num_anchors = d->num_anchors;
    p.levels = d->num_levels;
    p.batch = d->batch;
    p.topk = d->topk;
    p.gt_width = d->gt_width;
    p.total_gt = total_gt;
    p.num_classes = d->num_classes;
    p.pos_weight = d->pos_weight;
    for (int c = 0; c < 4; ++c) {
        p.means[c] = d->target_means[c];
        p.stds[c] = d->target_stds[c];
    }
    for (int b = 0; b <= MAX_BATCH; ++b) p.gt_offsets[b] = gt_offsets[b <= d->batch ? b : d->batch];
    const size_t key_bytes = align16((size_t)d->batch * (size_t)d->num_anchors * sizeof(unsigned long long));
    const size_t table_bytes = align16((size_t)total_gt * d->num_levels * d->topk * sizeof(int32_t));
    unsigned long long *keys = (unsigned long long *)workspace;
    int *cand_idx = (int *)((char *)workspace + key_bytes);
    float *cand_iou = (float *)((char *)workspace + key_bytes + table_bytes);
    hipStream_t s = (hipStream_t)stream;
    const float4 *an = (const float4 *)anchors;
    if (total_gt > 0) {
        HIP_TRY(hipMemsetAsync(keys, 0, key_bytes, s));
        hipLaunchKernelGGL(atss_select_kernel, dim3((unsigned)select_blocks), dim3(BLOCK), 0, s, an, inside, gt_boxes,
                           p, cand_idx, cand_iou);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(atss_claim_kernel, dim3((unsigned)total_gt + 1), dim3(64), 0, s, an, gt_boxes, p, cand_idx,
                       cand_iou, keys, counts);
    HIP_TRY(hipGetLastError());
    const dim3 grid((unsigned)((d->num_anchors + BLOCK - 1) / BLOCK), (unsigned)d->batch);
    hipLaunchKernelGGL(atss_finalize_kernel, grid, dim3(BLOCK), 0, s, an, inside, gt_boxes,
                       (const long long *)gt_labels, p, keys, (long long *)labels, label_weights,
                       (float4 *)bbox_targets, (float4 *)bbox_weights, (long long *)assigned_gt_inds, counts);
    HIP_TRY(hipGetLastError());
    return DFM_OK;
}
