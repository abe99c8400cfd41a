// anchor_target.hip -- nearest-BEV overlaps and the training targets of the 3-D anchor head
// (reference: core/bbox/iou_calculators/iou3d_calculator.py:99-145 bbox_overlaps_nearest_3d;
// models/dense_heads/train_mixins.py:12-350 AnchorTrainMixin.anchor_target_3d over mmdet's MaxIoUAssigner and
// PseudoSampler, core/bbox/coders/delta_xyzwhlr_bbox_coder.py:21-55 encode).
//
// Semantics (include/dfm_hip.h states them in full).  The reference builds, per image and class slot, a
// G x anchors overlap matrix and walks it with a few dozen torch ops; here the matrix never exists:
//   pass 1  one lane per anchor.  The image's GT nearest-BEV boxes pass through LDS in chunks of GT_CHUNK, so G is
//           not limited.  Per GT and slot the wave reduces its maximum overlap (shuffles), finds the first lane
//           that holds it (ballot) and issues ONE 64-bit atomic max of (overlap bits << 32 | ~anchor index): the
//           bit pattern of a non-negative float orders as the float does, the inverted index makes the lowest
//           anchor win a tie.  Waves whose lanes all miss a GT issue nothing; the zeroed scratch stands for
//           "maximum 0, first anchor of the slot".
//   pass 2  one lane per anchor recomputes its overlaps, applies assign_wrt_overlaps + PseudoSampler, encodes the
//           positives and writes every element of the six dense outputs exactly once; the 7-wide rows leave
//           through an LDS tile as contiguous runs.  Positives / negatives: ballot + popcount per wave, one
//           atomic add per block and counter.
// Both passes call bev_iou(), whose operations are written as explicitly rounded intrinsics: the equality test of
// pass 2 against pass 1's maximum compares the same bits.
#include "dfm_common.h"

using namespace dfm;

namespace {

constexpr int GT_CHUNK = 64;       // GT boxes staged per LDS round
constexpr int BLOCK = 256;         // four waves
constexpr int MAX_SLOTS = DFM_ANCHOR_TARGET_MAX_SLOTS;

struct Bev { float x1, y1, x2, y2, area; };

// BaseInstance3DBoxes.nearest_bev (base_box3d.py:144-162) of one row (x, y, z, dx, dy, dz, yaw, ...)
__device__ __forceinline__ Bev nearest_bev(const float *__restrict__ row)
{
    const float PI_F = 3.14159265358979323846f, QUARTER_PI_F = 0.78539816339744830962f;
    const float x = row[0], y = row[1], dx = row[3], dy = row[4], yaw = row[6];
    const float turns = floorf(__fadd_rn(__fdiv_rn(yaw, PI_F), 0.5f));
    const float r = fabsf(__fsub_rn(yaw, __fmul_rn(turns, PI_F)));
    const bool swap = r > QUARTER_PI_F;
    const float w = swap ? dy : dx, h = swap ? dx : dy;
    const float hw = __fdiv_rn(w, 2.0f), hh = __fdiv_rn(h, 2.0f);
    Bev b;
    b.x1 = __fsub_rn(x, hw);
    b.y1 = __fsub_rn(y, hh);
    b.x2 = __fadd_rn(x, hw);
    b.y2 = __fadd_rn(y, hh);
    b.area = __fmul_rn(__fsub_rn(b.x2, b.x1), __fsub_rn(b.y2, b.y1));
    return b;
}

// mmdet's bbox_overlaps of two axis-aligned boxes, fp32, eps 1e-6; iof: over the first box's area
__device__ __forceinline__ float bev_iou(const Bev &a, const Bev &b, bool iof)
{
    const float w = fmaxf(__fsub_rn(fminf(a.x2, b.x2), fmaxf(a.x1, b.x1)), 0.0f);
    const float h = fmaxf(__fsub_rn(fminf(a.y2, b.y2), fmaxf(a.y1, b.y1)), 0.0f);
    const float overlap = __fmul_rn(w, h);
    const float uni = iof ? a.area : __fsub_rn(__fadd_rn(a.area, b.area), overlap);
    return __fdiv_rn(overlap, fmaxf(uni, 1e-6f));
}

// out[i][j] = overlap(b1[i], b2[j]) (n, m), or out[i] = overlap(b1[i], b2[i]) when aligned
__global__ __launch_bounds__(BLOCK) void nearest_bev_overlaps_kernel(const float *__restrict__ b1, int n,
                                                                     const float *__restrict__ b2, int m, int width,
                                                                     int iof, int aligned, float *__restrict__ out)
{
    const long long total = aligned ? (long long)n : (long long)n * m;
    const long long e = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (e >= total) return;
    const long long i = aligned ? e : e / m, j = aligned ? e : e - i * m;
    out[e] = bev_iou(nearest_bev(b1 + i * width), nearest_bev(b2 + j * width), iof != 0);
}

struct Params {
    int num_anchors;     // locations * slots * rotations, per image
    int slots, rotations;
    int total_gt;        // rows of the packed GT tensor (the scratch's row length)
    int num_classes;
    int per_class, low_quality, assign_all, has_labels;
    float pos_thr[MAX_SLOTS], neg_thr[MAX_SLOTS], min_pos[MAX_SLOTS];
    float dir_offset, dir_limit_offset, pos_weight;
    int gt_offsets[DFM_ANCHOR_TARGET_MAX_BATCH + 1];
};

// the GT rows [g0, g0 + cnt) of the packed tensor as nearest-BEV boxes and labels in LDS
__device__ __forceinline__ void stage_gt(const float *__restrict__ gt, const long long *__restrict__ labels, int g0,
                                         int cnt, Bev *s_bev, int *s_label)
{
    __syncthreads();
    if ((int)threadIdx.x < cnt) {
        s_bev[threadIdx.x] = nearest_bev(gt + (size_t)(g0 + threadIdx.x) * 7);
        s_label[threadIdx.x] = labels ? (int)labels[g0 + threadIdx.x] : 0;   // (NULL: never compared)
    }
    __syncthreads();
}

__device__ __forceinline__ float wave_max(float v)
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v = fmaxf(v, __shfl_xor(v, s));
    return v;
}

__global__ __launch_bounds__(BLOCK) void anchor_gt_max_kernel(const float *__restrict__ anchors,
                                                              const float *__restrict__ gt,
                                                              const long long *__restrict__ labels, Params p,
                                                              unsigned long long *__restrict__ gt_max,
                                                              int *__restrict__ counts)
{
    __shared__ Bev s_bev[GT_CHUNK];
    __shared__ int s_label[GT_CHUNK];
    const int img = blockIdx.y;
    if (blockIdx.x == 0 && threadIdx.x < 2) counts[img * 2 + threadIdx.x] = 0;   // pass 2 adds into them
    const int g_begin = p.gt_offsets[img], g_end = p.gt_offsets[img + 1];
    const long long a = (long long)blockIdx.x * BLOCK + threadIdx.x;
    const bool valid = a < p.num_anchors;
    const int slot = valid ? (int)((a / p.rotations) % p.slots) : -1;
    Bev box{0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (valid) box = nearest_bev(anchors + (size_t)a * 7);
    const int lane = threadIdx.x & 63;
    for (int g0 = g_begin; g0 < g_end; g0 += GT_CHUNK) {
        const int cnt = min(GT_CHUNK, g_end - g0);
        stage_gt(gt, labels, g0, cnt, s_bev, s_label);
        for (int j = 0; j < cnt; ++j) {
            const float ov = valid ? bev_iou(s_bev[j], box, false) : 0.0f;
            const int label = s_label[j];
            for (int c = 0; c < p.slots; ++c) {
                if (p.per_class && c != label) continue;                      // (uniform)
                const float v = slot == c ? ov : 0.0f;
                if (__ballot(v > 0.0f) == 0ull) continue;                     // (uniform) nothing to report
                const float m = wave_max(v);
                const unsigned long long holders = __ballot(v == m);
                const int first = __ffsll((long long)holders) - 1;            // lanes are in anchor order
                if (lane == first) {
                    const unsigned long long packed =
                        ((unsigned long long)__float_as_uint(m) << 32) | (unsigned)~(unsigned)a;
                    atomicMax(gt_max + (size_t)c * p.total_gt + g0 + j, packed);
                }
            }
        }
    }
}

// DeltaXYZWLHRBBoxCoder.encode (delta_xyzwhlr_bbox_coder.py:21-55), the same fp32 operations
__device__ __forceinline__ void encode_row(const float *__restrict__ an, const float *__restrict__ g, float (&t)[7])
{
    const float xa = an[0], ya = an[1], wa = an[3], la = an[4], ha = an[5], ra = an[6];
    const float xg = g[0], yg = g[1], wg = g[3], lg = g[4], hg = g[5], rg = g[6];
    const float za = an[2] + ha / 2.0f, zg = g[2] + hg / 2.0f;
    const float diag = sqrtf(la * la + wa * wa);
    t[0] = (xg - xa) / diag;
    t[1] = (yg - ya) / diag;
    t[2] = (zg - za) / ha;
    t[3] = logf(wg / wa);
    t[4] = logf(lg / la);
    t[5] = logf(hg / ha);
    t[6] = rg - ra;
}

// get_direction_target (train_mixins.py:320-350), two bins
__device__ __forceinline__ long long direction_bin(float rt, float ra, float dir_offset, float dir_limit_offset)
{
    const float TWO_PI_F = 6.28318530717958647692f, PI_F = 3.14159265358979323846f;
    const float val = (rt + ra) - dir_offset;
    const float off = val - floorf(val / TWO_PI_F + dir_limit_offset) * TWO_PI_F;
    return floorf(off / PI_F) >= 1.0f ? 1 : 0;                    // clamp(floor(.), 0, 1)
}

// rows [row0, row0 + BLOCK) of dst (n, 7) from each thread's v, through the tile: contiguous global stores
__device__ __forceinline__ void store_rows7(float *__restrict__ dst, long long row0, int cnt, float *tile,
                                            const float (&v)[7])
{
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 7; ++c) tile[threadIdx.x * 7 + c] = v[c];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        const int e = threadIdx.x + BLOCK * j;
        if (e < cnt * 7) dst[row0 * 7 + e] = tile[e];
    }
}

__global__ __launch_bounds__(BLOCK) void anchor_assign_kernel(const float *__restrict__ anchors,
                                                              const float *__restrict__ gt,
                                                              const long long *__restrict__ gt_labels, Params p,
                                                              const unsigned long long *__restrict__ gt_max,
                                                              long long *__restrict__ labels,
                                                              float *__restrict__ label_weights,
                                                              float *__restrict__ bbox_targets,
                                                              float *__restrict__ bbox_weights,
                                                              long long *__restrict__ dir_targets,
                                                              float *__restrict__ dir_weights,
                                                              int *__restrict__ counts)
{
    __shared__ Bev s_bev[GT_CHUNK];
    __shared__ int s_label[GT_CHUNK];
    __shared__ unsigned long long s_max[MAX_SLOTS * GT_CHUNK];
    __shared__ float tile[BLOCK * 7];
    __shared__ int s_count[2];
    const int img = blockIdx.y;
    const int g_begin = p.gt_offsets[img], g_end = p.gt_offsets[img + 1];
    const long long row0 = (long long)blockIdx.x * BLOCK;
    const long long a = row0 + threadIdx.x;
    const int rows = (int)min((long long)BLOCK, (long long)p.num_anchors - row0);
    const bool valid = a < p.num_anchors;
    const int slot = valid ? (int)((a / p.rotations) % p.slots) : 0;
    if (threadIdx.x < 2) s_count[threadIdx.x] = 0;
    Bev box{0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (valid) box = nearest_bev(anchors + (size_t)a * 7);
    // the first anchor of this lane's slot: where torch's max over an all-zero row points
    const unsigned first_of_slot = (unsigned)(slot * p.rotations);
    float best = 0.0f;          // max over the slot's GTs; starts at the 0 every overlap is at least
    int best_gt = -1, low_gt = -1, matched = 0;
    for (int g0 = g_begin; g0 < g_end; g0 += GT_CHUNK) {
        const int cnt = min(GT_CHUNK, g_end - g0);
        stage_gt(gt, gt_labels, g0, cnt, s_bev, s_label);     // (its leading barrier also guards s_max)
        for (int e = threadIdx.x; e < p.slots * cnt; e += BLOCK) {
            const int c = e / cnt, j = e - c * cnt;
            s_max[c * GT_CHUNK + j] = gt_max[(size_t)c * p.total_gt + g0 + j];
        }
        __syncthreads();
        if (!valid) continue;
        for (int j = 0; j < cnt; ++j) {
            if (p.per_class && s_label[j] != slot) continue;
            const float ov = bev_iou(s_bev[j], box, false);
            if (matched == 0 || ov > best) {                  // the lowest GT index wins a tie
                best = ov;
                best_gt = g0 + j;
            }
            ++matched;
            const unsigned long long packed = s_max[slot * GT_CHUNK + j];
            const float top = __uint_as_float((unsigned)(packed >> 32));
            const unsigned holder = packed == 0ull ? first_of_slot : ~(unsigned)packed;
            const bool mine = p.assign_all ? ov == top : (unsigned)a == holder;
            if (p.low_quality && top >= p.min_pos[slot] && mine) low_gt = g0 + j;   // a later GT overrides
        }
    }
    int assigned = -1;          // -1 ignore, 0 negative, > 0: GT row + 1 (of the packed tensor)
    if (matched == 0) {
        assigned = 0;           // no GT for this slot: every anchor negative
    } else {
        if (best >= 0.0f && best < p.neg_thr[slot]) assigned = 0;
        if (best >= p.pos_thr[slot]) assigned = best_gt + 1;
        if (low_gt >= 0) assigned = low_gt + 1;
    }
    const bool pos = valid && assigned > 0, neg = valid && assigned == 0;
    float target[7], weight[7];
#pragma unroll
    for (int c = 0; c < 7; ++c) target[c] = weight[c] = 0.0f;
    long long label = p.has_labels ? p.num_classes : 0, dir = 0;   // train_mixins.py:287-288
    if (pos) {
        const float *an = anchors + (size_t)a * 7;
        encode_row(an, gt + (size_t)(assigned - 1) * 7, target);
        dir = direction_bin(target[6], an[6], p.dir_offset, p.dir_limit_offset);
        label = p.has_labels ? gt_labels[assigned - 1] : 1;
#pragma unroll
        for (int c = 0; c < 7; ++c) weight[c] = 1.0f;
    }
    if (valid) {
        const size_t o = (size_t)img * p.num_anchors + a;
        labels[o] = label;
        label_weights[o] = pos ? (p.pos_weight > 0.0f ? p.pos_weight : 1.0f) : (neg ? 1.0f : 0.0f);
        dir_targets[o] = dir;
        dir_weights[o] = pos ? 1.0f : 0.0f;
    }
    const long long out0 = (long long)img * p.num_anchors + row0;
    store_rows7(bbox_targets, out0, rows, tile, target);
    store_rows7(bbox_weights, out0, rows, tile, weight);
    const int n_pos = __popcll(__ballot(pos)), n_neg = __popcll(__ballot(neg));
    if ((threadIdx.x & 63) == 0) {
        if (n_pos) atomicAdd(&s_count[0], n_pos);
        if (n_neg) atomicAdd(&s_count[1], n_neg);
    }
    __syncthreads();
    if (threadIdx.x < 2 && s_count[threadIdx.x]) atomicAdd(counts + img * 2 + threadIdx.x, s_count[threadIdx.x]);
}

}  // namespace

extern "C" DFM_API int dfm_nearest_bev_overlaps(const float *boxes1, int32_t n, const float *boxes2, int32_t m,
                                                int32_t width, int32_t mode, int32_t aligned, float *out,
                                                void *stream)
{
    if (n < 0 || m < 0) return set_error(DFM_ERR_INVALID_ARG, "negative box count");
    if (width < 7) return set_errorf(DFM_ERR_INVALID_ARG, "box width %d: a 3-D box has at least 7 columns", width);
    if (mode != DFM_OVERLAP_IOU && mode != DFM_OVERLAP_IOF)
        return set_errorf(DFM_ERR_INVALID_ARG, "mode %d: DFM_OVERLAP_IOU or DFM_OVERLAP_IOF", mode);
    if (aligned && n != m) return set_error(DFM_ERR_INVALID_ARG, "aligned overlaps need as many boxes2 as boxes1");
    if (n == 0 || m == 0) return DFM_OK;
    if (!boxes1 || !boxes2 || !out) return set_error(DFM_ERR_INVALID_ARG, "NULL device pointer");
    const long long total = aligned ? (long long)n : (long long)n * m;
    const long long blocks = (total + BLOCK - 1) / BLOCK;
    if (blocks > 0x7fffffffll) return set_error(DFM_ERR_UNSUPPORTED, "overlap matrix too large");
    hipLaunchKernelGGL(nearest_bev_overlaps_kernel, dim3((unsigned)blocks), dim3(BLOCK), 0, (hipStream_t)stream,
                       boxes1, n, boxes2, m, width, mode == DFM_OVERLAP_IOF, aligned, out);
    HIP_TRY(hipGetLastError());
    return DFM_OK;
}

extern "C" DFM_API size_t dfm_anchor_target_workspace_bytes(int32_t num_slots, int32_t total_gt)
{
    if (num_slots <= 0 || total_gt <= 0) return 0;
    return (size_t)num_slots * (size_t)total_gt * sizeof(unsigned long long);
}

extern "C" DFM_API int dfm_anchor_target_3d(const dfm_anchor_target_desc *d, const float *anchors,
                                            const float *gt_boxes, const int64_t *gt_labels,
                                            const int32_t *gt_offsets, int64_t *labels, float *label_weights,
                                            float *bbox_targets, float *bbox_weights, int64_t *dir_targets,
                                            float *dir_weights, int32_t *counts, void *workspace,
                                            size_t workspace_bytes, void *stream)
{
    if (!d) return set_error(DFM_ERR_INVALID_ARG, "NULL descriptor");
    if (d->box_width != 7)
        return set_errorf(DFM_ERR_UNSUPPORTED, "box width %d: the anchor targets are built for 7-wide boxes",
                          d->box_width);
    if (d->sampler != DFM_SAMPLER_PSEUDO)
        return set_error(DFM_ERR_UNSUPPORTED, "only the pseudo sampler (every assigned anchor is kept) is built");
    if (d->neg_iou_thr_is_range)
        return set_error(DFM_ERR_UNSUPPORTED, "a (low, high) neg_iou_thr is not built");
    if (d->ignore_iof_thr > 0.0f && d->num_ignore_boxes > 0)
        return set_error(DFM_ERR_UNSUPPORTED, "ignore regions (ignore_iof_thr > 0 with ignore boxes) are not built");
    if (d->num_locations < 0 || d->batch < 0 || d->num_ignore_boxes < 0)
        return set_error(DFM_ERR_INVALID_ARG, "negative size");
    if (d->num_slots <= 0 || d->num_rotations <= 0)
        return set_error(DFM_ERR_INVALID_ARG, "non-positive slot or rotation count");
    if (d->num_slots > MAX_SLOTS)
        return set_errorf(DFM_ERR_UNSUPPORTED, "%d class slots: at most DFM_ANCHOR_TARGET_MAX_SLOTS = %d", d->num_slots,
                          MAX_SLOTS);
    if (d->batch > DFM_ANCHOR_TARGET_MAX_BATCH)
        return set_errorf(DFM_ERR_UNSUPPORTED, "%d images: at most DFM_ANCHOR_TARGET_MAX_BATCH = %d per call", d->batch,
                          DFM_ANCHOR_TARGET_MAX_BATCH);
    const long long num_anchors = (long long)d->num_locations * d->num_slots * d->num_rotations;
    if (num_anchors > 0x7fffffffll) return set_error(DFM_ERR_UNSUPPORTED, "more than 2^31 - 1 anchors per image");
    if (d->batch == 0 || num_anchors == 0) return DFM_OK;
    if (!gt_offsets) return set_error(DFM_ERR_INVALID_ARG, "NULL gt_offsets");
    if (gt_offsets[0] != 0) return set_error(DFM_ERR_INVALID_ARG, "gt_offsets[0] must be 0");
    for (int b = 0; b < d->batch; ++b)
        if (gt_offsets[b + 1] < gt_offsets[b]) return set_error(DFM_ERR_INVALID_ARG, "gt_offsets must not decrease");
    const int total_gt = gt_offsets[d->batch];
    if (!anchors || !labels || !label_weights || !bbox_targets || !bbox_weights || !dir_targets || !dir_weights ||
        !counts)
        return set_error(DFM_ERR_INVALID_ARG, "NULL device pointer");
    if (total_gt > 0 && !gt_boxes) return set_error(DFM_ERR_INVALID_ARG, "NULL gt_boxes");
    if (d->assign_per_class && !d->has_labels)
        return set_error(DFM_ERR_INVALID_ARG, "assign_per_class needs gt_labels");
    if (total_gt > 0 && d->has_labels && !gt_labels) return set_error(DFM_ERR_INVALID_ARG, "NULL gt_labels");
    const size_t need = dfm_anchor_target_workspace_bytes(d->num_slots, total_gt);
    if (need > 0) {
        if (!workspace || workspace_bytes < need)
            return set_errorf(DFM_ERR_WORKSPACE, "anchor targets need %zu workspace bytes, got %zu", need,
                              workspace ? workspace_bytes : (size_t)0);
        if ((uintptr_t)workspace & 15) return set_error(DFM_ERR_INVALID_ARG, "workspace must be 16-byte aligned");
    }
    Params p;
    p.num_anchors = (int)num_anchors;
    p.slots = d->num_slots;
    p.rotations = d->num_rotations;
    p.total_gt = total_gt;
    p.num_classes = d->num_classes;
    p.per_class = d->assign_per_class != 0;
    p.low_quality = d->match_low_quality != 0;
    p.assign_all = d->gt_max_assign_all != 0;
    p.has_labels = d->has_labels != 0;
    for (int c = 0; c < MAX_SLOTS; ++c) {
        p.pos_thr[c] = d->pos_iou_thr[c];
        p.neg_thr[c] = d->neg_iou_thr[c];
        p.min_pos[c] = d->min_pos_iou[c];
    }
    p.dir_offset = d->dir_offset;
    p.dir_limit_offset = d->dir_limit_offset;
    p.pos_weight = d->pos_weight;
    for (int b = 0; b <= DFM_ANCHOR_TARGET_MAX_BATCH; ++b) p.gt_offsets[b] = gt_offsets[b <= d->batch ? b : d->batch];
    hipStream_t s = (hipStream_t)stream;
    if (need > 0) HIP_TRY(hipMemsetAsync(workspace, 0, need, s));
    const dim3 grid((unsigned)((num_anchors + BLOCK - 1) / BLOCK), (unsigned)d->batch), block(BLOCK);
    hipLaunchKernelGGL(anchor_gt_max_kernel, grid, block, 0, s, anchors, gt_boxes,
                       d->has_labels ? (const long long *)gt_labels : nullptr, p, (unsigned long long *)workspace, counts);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(anchor_assign_kernel, grid, block, 0, s, anchors, gt_boxes,
                       d->has_labels ? (const long long *)gt_labels : nullptr, p,
                       (const unsigned long long *)workspace, (long long *)labels, label_weights, bbox_targets,
                       bbox_weights, (long long *)dir_targets, dir_weights, counts);
    HIP_TRY(hipGetLastError());
    return DFM_OK;
}
