// kitti_eval.hip -- KITTI evaluation: the overlaps of every same-frame detection x ground-truth pair in one launch,
// and compute_statistics_jit for every (class, difficulty, min-overlap, frame, threshold) of a metric, one wave per
// (combination, frame) with the thresholds in its lanes.  Semantics: include/dfm_hip_kitti_eval.h.
#include "dfm_common.h"
#include "rbox_geom.h"

namespace dfm {

constexpr int KITTI_T = DFM_KITTI_SAMPLE_POINTS;
constexpr int KITTI_LDS_WORDS = DFM_KITTI_LDS_DETS / 64;

// ---------------------------------------------------------------------------------------------------------
// overlaps
// ---------------------------------------------------------------------------------------------------------
struct KittiSide {
    const double *bbox, *loc, *dims, *ry;
    const int64_t *off;
};

// image_box_overlap of one pair: b = "boxes" row, q = "query_boxes" row; FP64, the reference's operation order
__device__ __forceinline__ double image_overlap(const double *__restrict__ b, const double *__restrict__ q,
                                                int criterion)
{
    const double qarea = (q[2] - q[0]) * (q[3] - q[1]);
    const double iw = fmin(b[2], q[2]) - fmax(b[0], q[0]);
    if (!(iw > 0.0)) return 0.0;
    const double ih = fmin(b[3], q[3]) - fmax(b[1], q[1]);
    if (!(ih > 0.0)) return 0.0;
    double ua;
    if (criterion == -1) ua = (b[2] - b[0]) * (b[3] - b[1]) + qarea - iw * ih;
    else if (criterion == 0) ua = (b[2] - b[0]) * (b[3] - b[1]);
    else if (criterion == 1) ua = qarea;
    else ua = 1.0;
    return iw * ih / ua;
}

// the BEV rectangle of row i, rounded to FP32 as rotate_iou_gpu_eval does.  The reference's angle is clockwise
// (rbbox_to_corners turns a corner by -angle), rbox_geom.h's counter-clockwise: the box is loaded with the sine
// negated, i.e. with the angle -a.  Keeping +a for both boxes would be a reflection of the plane -- areas unchanged --
// only if the centres were mirrored with it; with the centres as they are it is another pair of boxes.
__device__ __forceinline__ RBox bev_box(const KittiSide &s, int64_t i)
{
    RBox r;
    r.x = (float)s.loc[3 * i + 0];
    r.y = (float)s.loc[3 * i + 2];
    r.w = (float)s.dims[3 * i + 0];
    r.h = (float)s.dims[3 * i + 2];
    const float a = (float)s.ry[i];
    r.c = cosf(a);
    r.s = -sinf(a);
    return r;
}

__global__ __launch_bounds__(256) void kitti_overlaps_kernel(int64_t frames, int64_t total_pairs, int criterion,
                                                             KittiSide dt, KittiSide gt,
                                                             const int64_t *__restrict__ pair_off,
                                                             double *__restrict__ out_bbox,
                                                             double *__restrict__ out_bev,
                                                             double *__restrict__ out_3d)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= total_pairs) return;
    // the frame of pair p: pair_off[lo] <= p < pair_off[hi] throughout (pair_off[0] = 0, pair_off[F] = total_pairs)
    int64_t lo = 0, hi = frames;
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (pair_off[mid] <= p) lo = mid;
        else hi = mid;
    }
    const int64_t g0 = gt.off[lo], ng = gt.off[lo + 1] - g0;
    const int64_t d0 = dt.off[lo], nd = dt.off[lo + 1] - d0;
    const int64_t local = p - pair_off[lo];
    if (ng <= 0 || local < 0 || local >= nd * ng) {   // tables that disagree: nothing is read
        if (out_bbox) out_bbox[p] = 0.0;
        if (out_bev) out_bev[p] = 0.0;
        if (out_3d) out_3d[p] = 0.0;
        return;
    }
    const int64_t d = d0 + local / ng, g = g0 + local % ng;

    if (out_bbox) out_bbox[p] = image_overlap(dt.bbox + 4 * d, gt.bbox + 4 * g, criterion);
    if (!out_bev && !out_3d) return;

    const RBox A = bev_box(gt, g), B = bev_box(dt, d);    // rbox1 = the query (ground truth), rbox2 = the box
    const float area1 = A.w * A.h, area2 = B.w * B.h;
    const float inter = (area1 < AREA_EPS || area2 < AREA_EPS) ? 0.0f : rbox_intersection(A, B);
    if (out_bev) {
        float r;
        if (criterion == -1) r = inter / (area1 + area2 - inter);
        else if (criterion == 0) r = inter / area1;
        else if (criterion == 1) r = inter / area2;
        else r = inter;
        out_bev[p] = (double)r;
    }
    if (out_3d) {
        double r = 0.0;
        if (inter > 0.0f) {
            const double y1 = dt.loc[3 * d + 1], h1 = dt.dims[3 * d + 1];
            const double y2 = gt.loc[3 * g + 1], h2 = gt.dims[3 * g + 1];
            const double iw = fmin(y1, y2) - fmax(y1 - h1, y2 - h2);
            if (iw > 0.0) {
                const double v1 = dt.dims[3 * d + 0] * dt.dims[3 * d + 1] * dt.dims[3 * d + 2];
                const double v2 = gt.dims[3 * g + 0] * gt.dims[3 * g + 1] * gt.dims[3 * g + 2];
                const double inc = iw * (double)inter;
                double ua;
                if (criterion == -1) ua = v1 + v2 - inc;
                else if (criterion == 0) ua = v1;
                else if (criterion == 1) ua = v2;
                else ua = inc;
                r = (double)(float)(inc / ua);
            }
        }
        out_3d[p] = r;
    }
}

// ---------------------------------------------------------------------------------------------------------
// matching
// ---------------------------------------------------------------------------------------------------------
struct KittiMatch {
    int metric, second_pass, compute_aos;
    int64_t frames;
    int L, K;
    int64_t items;                 // combinations * frames
    const double *overlaps;
    const int64_t *pair_off, *gt_off, *dt_off, *dc_off;
    const double *dt_bbox, *dt_alpha, *dt_score, *gt_alpha, *dc_bbox;
    const int8_t *ignored_gt, *ignored_det;
    int64_t total_gt, total_dt;
    const double *min_overlap, *thresholds;
    const int32_t *num_thresholds;
    double *tp_scores;
    unsigned long long *counts;
    double *sim_part;              // (combinations, frames, KITTI_T), workspace
    unsigned long long *masks;     // (grid, ws_words, 64), workspace
    int64_t ws_words;
};

__global__ __launch_bounds__(64) void kitti_match_kernel(KittiMatch a)
{
    __shared__ unsigned long long lds_mask[KITTI_LDS_WORDS * 64];
    const int lane = threadIdx.x;
    constexpr double NO_DETECTION = -10000000.0;
    for (int64_t item = blockIdx.x; item < a.items; item += gridDim.x) {
        const int64_t combo = item / a.frames, f = item % a.frames;
        const int k = (int)(combo % a.K);
        const int64_t cl = combo / a.K;            // m * L + l
        const int m = (int)(cl / a.L);
        int nlanes = 1;
        if (a.second_pass) {
            nlanes = a.num_thresholds[combo];
            nlanes = nlanes < 0 ? 0 : (nlanes > KITTI_T ? KITTI_T : nlanes);
        }
        if (lane >= nlanes) continue;              // no barrier below: every lane owns its mask words
        const int64_t g0 = a.gt_off[f], ng = a.gt_off[f + 1] - g0;
        const int64_t d0 = a.dt_off[f], nd = a.dt_off[f + 1] - d0;
        const int64_t words = (nd + 63) >> 6;
        unsigned long long *mask;
        if (words <= KITTI_LDS_WORDS) mask = lds_mask + lane;
        else if (words <= a.ws_words) mask = a.masks + (size_t)blockIdx.x * a.ws_words * 64 + lane;
        else continue;                             // more detections than the caller sized the workspace for
        for (int64_t w = 0; w < words; ++w) mask[w * 64] = 0ull;

        const int8_t *__restrict__ ig = a.ignored_gt + cl * a.total_gt + g0;
        const int8_t *__restrict__ id = a.ignored_det + cl * a.total_dt + d0;
        const double *__restrict__ ov = a.overlaps + a.pair_off[f];
        const double *__restrict__ score = a.dt_score + d0;
        const double min_overlap = a.min_overlap[m * a.K + k];
        const bool compute_fp = a.second_pass != 0;
        const double thresh = compute_fp ? a.thresholds[combo * KITTI_T + lane] : 0.0;
        double *tp_out = a.tp_scores ? a.tp_scores + combo * a.total_gt + g0 : nullptr;

        long long tp = 0, fp = 0, fn = 0;
        int64_t thresh_idx = 0;
        double sim = 0.0;
        for (int64_t i = 0; i < ng; ++i) {
            if (ig[i] == -1) continue;
            int64_t det_idx = -1;
            double valid_detection = NO_DETECTION;
            double max_overlap = 0.0;
            bool assigned_ignored_det = false;
            for (int64_t j = 0; j < nd; ++j) {
                if (id[j] == -1) continue;
                if ((mask[(j >> 6) * 64] >> (j & 63)) & 1ull) continue;
                const double dt_score = score[j];
                if (compute_fp && dt_score < thresh) continue;
                const double overlap = ov[j * ng + i];
                if (!compute_fp && overlap > min_overlap && dt_score > valid_detection) {
                    det_idx = j;
                    valid_detection = dt_score;
                } else if (compute_fp && overlap > min_overlap && (overlap > max_overlap || assigned_ignored_det) &&
                           id[j] == 0) {
                    max_overlap = overlap;
                    det_idx = j;
                    valid_detection = 1.0;
                    assigned_ignored_det = false;
                } else if (compute_fp && overlap > min_overlap && valid_detection == NO_DETECTION && id[j] == 1) {
                    det_idx = j;
                    valid_detection = 1.0;
                    assigned_ignored_det = true;
                }
            }
            if (valid_detection == NO_DETECTION && ig[i] == 0) {
                fn += 1;
            } else if (valid_detection != NO_DETECTION && (ig[i] == 1 || id[det_idx] == 1)) {
                mask[(det_idx >> 6) * 64] |= 1ull << (det_idx & 63);
            } else if (valid_detection != NO_DETECTION) {
                tp += 1;
                if (!compute_fp && tp_out) tp_out[thresh_idx] = score[det_idx];
                thresh_idx += 1;
                if (a.compute_aos) sim += (1.0 + cos(a.gt_alpha[g0 + i] - a.dt_alpha[d0 + det_idx])) / 2.0;
                mask[(det_idx >> 6) * 64] |= 1ull << (det_idx & 63);
            }
        }
        if (!compute_fp) {
            if (tp_out)
                for (int64_t i = thresh_idx; i < ng; ++i) tp_out[i] = __longlong_as_double(0x7ff8000000000000ll);
            continue;
        }
        for (int64_t j = 0; j < nd; ++j) {
            const bool assigned = (mask[(j >> 6) * 64] >> (j & 63)) & 1ull;
            if (!(assigned || id[j] == -1 || id[j] == 1 || score[j] < thresh)) fp += 1;
        }
        long long nstuff = 0;
        if (a.metric == 0) {
            const int64_t c0 = a.dc_off[f], nc = a.dc_off[f + 1] - c0;
            for (int64_t i = 0; i < nc; ++i) {
                for (int64_t j = 0; j < nd; ++j) {
                    if ((mask[(j >> 6) * 64] >> (j & 63)) & 1ull) continue;
                    if (id[j] == -1 || id[j] == 1) continue;
                    if (score[j] < thresh) continue;
                    if (image_overlap(a.dt_bbox + 4 * (d0 + j), a.dc_bbox + 4 * (c0 + i), 0) > min_overlap) {
                        mask[(j >> 6) * 64] |= 1ull << (j & 63);
                        nstuff += 1;
                    }
                }
            }
        }
        fp -= nstuff;
        unsigned long long *c = a.counts + (combo * KITTI_T + lane) * 3;
        if (tp) atomicAdd(c + 0, (unsigned long long)tp);
        if (fp) atomicAdd(c + 1, (unsigned long long)fp);   // fp >= 0: nstuff counts detections fp counted
        if (fn) atomicAdd(c + 2, (unsigned long long)fn);
        if (a.compute_aos) a.sim_part[(combo * a.frames + f) * KITTI_T + lane] = sim;
    }
}

// similarity[combo][t] = the frames' partials added in a fixed order: lane s adds frames s, s + 64, ...; lane 0 then
// adds the 64 lane sums in lane order
__global__ __launch_bounds__(64) void kitti_similarity_kernel(const double *__restrict__ part, int64_t frames,
                                                              const int32_t *__restrict__ num_thresholds,
                                                              double *__restrict__ similarity)
{
    __shared__ double sums[64];
    const int64_t combo = blockIdx.x / KITTI_T;
    const int t = blockIdx.x % KITTI_T, lane = threadIdx.x;
    const bool live = t < num_thresholds[combo];
    double acc = 0.0;
    if (live)
        for (int64_t f = lane; f < frames; f += 64) acc += part[(combo * frames + f) * KITTI_T + t];
    sums[lane] = acc;
    __syncthreads();
    if (lane == 0) {
        double total = 0.0;
        for (int s = 0; s < 64; ++s) total += sums[s];
        similarity[combo * KITTI_T + t] = total;
    }
}

static inline size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

static inline int64_t match_grid(int64_t items)
{
    return items < DFM_KITTI_MATCH_MAX_GRID ? items : DFM_KITTI_MATCH_MAX_GRID;
}

// bytes of the two workspace regions: similarity partials, then the assigned masks
static inline void workspace_layout(int64_t frames, int64_t combos, int64_t max_dt, int similarity, size_t *sim_bytes,
                                    size_t *mask_bytes, int64_t *ws_words)
{
    *sim_bytes = similarity ? align16((size_t)combos * (size_t)frames * KITTI_T * sizeof(double)) : 0;
    *ws_words = max_dt > DFM_KITTI_LDS_DETS ? (max_dt + 63) >> 6 : 0;
    *mask_bytes = (size_t)match_grid(combos * frames) * (size_t)*ws_words * 64 * sizeof(unsigned long long);
}

}  // namespace dfm

using namespace dfm;

extern "C" DFM_API int dfm_kitti_overlaps(int64_t frames, int64_t total_pairs, int32_t criterion,
                                          const double *dt_bbox, const double *dt_location,
                                          const double *dt_dimensions, const double *dt_rotation_y,
                                          const int64_t *dt_off, const double *gt_bbox, const double *gt_location,
                                          const double *gt_dimensions, const double *gt_rotation_y,
                                          const int64_t *gt_off, const int64_t *pair_off, double *out_bbox,
                                          double *out_bev, double *out_3d, void *stream)
{
    if (frames < 0 || total_pairs < 0) return set_error(DFM_ERR_INVALID_ARG, "negative frame or pair count");
    if (!out_bbox && !out_bev && !out_3d) return set_error(DFM_ERR_INVALID_ARG, "no metric requested: every output is NULL");
    if (frames == 0 || total_pairs == 0) return DFM_OK;
    if (!dt_off || !gt_off || !pair_off) return set_error(DFM_ERR_INVALID_ARG, "NULL offset table");
    if (out_bbox && (!dt_bbox || !gt_bbox)) return set_error(DFM_ERR_INVALID_ARG, "NULL bbox array for the bbox metric");
    if ((out_bev || out_3d) && (!dt_location || !dt_dimensions || !dt_rotation_y || !gt_location || !gt_dimensions ||
                                !gt_rotation_y))
        return set_error(DFM_ERR_INVALID_ARG, "NULL location, dimensions or rotation_y for the bev / 3d metric");
    const int64_t blocks = (total_pairs + 255) / 256;
    if (blocks > 0x7fffffffll) return set_error(DFM_ERR_UNSUPPORTED, "too many pairs for one launch");
    const KittiSide dt{dt_bbox, dt_location, dt_dimensions, dt_rotation_y, dt_off};
    const KittiSide gt{gt_bbox, gt_location, gt_dimensions, gt_rotation_y, gt_off};
    hipLaunchKernelGGL(kitti_overlaps_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, frames,
                       total_pairs, (int)criterion, dt, gt, pair_off, out_bbox, out_bev, out_3d);
    HIP_TRY(hipGetLastError());
    return DFM_OK;
}

extern "C" DFM_API size_t dfm_kitti_eval_workspace_bytes(int64_t frames, int32_t combinations, int64_t max_dt,
                                                         int32_t similarity)
{
    if (frames < 0 || combinations < 0 || max_dt < 0) return 0;
    size_t sim_bytes, mask_bytes;
    int64_t ws_words;
    workspace_layout(frames, combinations, max_dt, similarity != 0, &sim_bytes, &mask_bytes, &ws_words);
    return sim_bytes + mask_bytes + 16;            // never 0 for valid sizes: 0 means invalid
}

extern "C" DFM_API int dfm_kitti_match(int32_t metric, int32_t second_pass, int32_t compute_aos, int64_t frames,
                                       int32_t num_classes, int32_t num_difficulties, int32_t num_min_overlaps,
                                       const double *overlaps, const int64_t *pair_off, const int64_t *gt_off,
                                       const int64_t *dt_off, const int64_t *dc_off, const double *dt_bbox,
                                       const double *dt_alpha, const double *dt_score, const double *gt_alpha,
                                       const double *dc_bbox, const int8_t *ignored_gt, const int8_t *ignored_det,
                                       int64_t total_gt, int64_t total_dt, const double *min_overlap,
                                       const double *thresholds, const int32_t *num_thresholds, double *tp_scores,
                                       int64_t *counts, double *similarity, int64_t max_dt, void *workspace,
                                       size_t workspace_bytes, void *stream)
{
    if (metric < 0 || metric > 2) return set_error(DFM_ERR_INVALID_ARG, "metric must be 0 (bbox), 1 (bev) or 2 (3d)");
    if (frames < 0 || num_classes < 0 || num_difficulties < 0 || num_min_overlaps < 0 || total_gt < 0 ||
        total_dt < 0 || max_dt < 0)
        return set_error(DFM_ERR_INVALID_ARG, "negative size");
    const int64_t combos = (int64_t)num_classes * num_difficulties * num_min_overlaps;
    if (combos > 0x7fffffffll / DFM_KITTI_SAMPLE_POINTS) return set_error(DFM_ERR_UNSUPPORTED, "too many combinations");
    const bool aos = second_pass && compute_aos;
    if (second_pass) {
        if (!counts) return set_error(DFM_ERR_INVALID_ARG, "NULL counts");
        if (aos && !similarity) return set_error(DFM_ERR_INVALID_ARG, "NULL similarity with compute_aos");
    } else if (!tp_scores && combos && total_gt) {
        return set_error(DFM_ERR_INVALID_ARG, "NULL tp_scores");
    }
    hipStream_t s = (hipStream_t)stream;
    if (second_pass && combos) {
        HIP_TRY(hipMemsetAsync(counts, 0, (size_t)combos * DFM_KITTI_SAMPLE_POINTS * 3 * sizeof(int64_t), s));
        if (aos && frames == 0)
            HIP_TRY(hipMemsetAsync(similarity, 0, (size_t)combos * DFM_KITTI_SAMPLE_POINTS * sizeof(double), s));
    }
    if (frames == 0 || combos == 0) return DFM_OK;
    if (!pair_off || !gt_off || !dt_off) return set_error(DFM_ERR_INVALID_ARG, "NULL offset table");
    if (metric == 0 && second_pass && (!dc_off || (total_dt && !dt_bbox)))
        return set_error(DFM_ERR_INVALID_ARG, "NULL dc_off or dt_bbox for the bbox metric");
    if ((total_gt && !ignored_gt) || (total_dt && !ignored_det) || !min_overlap)
        return set_error(DFM_ERR_INVALID_ARG, "NULL ignored flags or min_overlap");
    if (total_dt && !dt_score) return set_error(DFM_ERR_INVALID_ARG, "NULL dt_score");
    if (total_dt && total_gt && !overlaps) return set_error(DFM_ERR_INVALID_ARG, "NULL overlaps");
    if (second_pass && (!thresholds || !num_thresholds)) return set_error(DFM_ERR_INVALID_ARG, "NULL thresholds");
    if (compute_aos && ((total_gt && !gt_alpha) || (total_dt && !dt_alpha))) return set_error(DFM_ERR_INVALID_ARG, "NULL alpha with compute_aos");

    size_t sim_bytes, mask_bytes;
    int64_t ws_words;
    workspace_layout(frames, combos, max_dt, aos, &sim_bytes, &mask_bytes, &ws_words);
    if (sim_bytes + mask_bytes) {
        if (!workspace || workspace_bytes < sim_bytes + mask_bytes)
            return set_error(DFM_ERR_WORKSPACE, "kitti match: NULL or short workspace (dfm_kitti_eval_workspace_bytes)");
        if ((uintptr_t)workspace & 15) return set_error(DFM_ERR_INVALID_ARG, "workspace must be 16-byte aligned");
    }
    KittiMatch a;
    a.metric = metric;
    a.second_pass = second_pass != 0;
    a.compute_aos = aos;
    a.frames = frames;
    a.L = num_difficulties;
    a.K = num_min_overlaps;
    a.items = combos * frames;
    a.overlaps = overlaps;
    a.pair_off = pair_off;
    a.gt_off = gt_off;
    a.dt_off = dt_off;
    a.dc_off = dc_off;
    a.dt_bbox = dt_bbox;
    a.dt_alpha = dt_alpha;
    a.dt_score = dt_score;
    a.gt_alpha = gt_alpha;
    a.dc_bbox = dc_bbox;
    a.ignored_gt = ignored_gt;
    a.ignored_det = ignored_det;
    a.total_gt = total_gt;
    a.total_dt = total_dt;
    a.min_overlap = min_overlap;
    a.thresholds = thresholds;
    a.num_thresholds = num_thresholds;
    a.tp_scores = second_pass ? nullptr : tp_scores;
    a.counts = (unsigned long long *)counts;
    a.sim_part = (double *)workspace;
    a.masks = (unsigned long long *)((char *)workspace + sim_bytes);
    a.ws_words = ws_words;
    hipLaunchKernelGGL(kitti_match_kernel, dim3((unsigned)match_grid(a.items)), dim3(64), 0, s, a);
    HIP_TRY(hipGetLastError());
    if (aos) {
        hipLaunchKernelGGL(kitti_similarity_kernel, dim3((unsigned)(combos * DFM_KITTI_SAMPLE_POINTS)), dim3(64), 0, s,
                           (const double *)workspace, frames, num_thresholds, similarity);
        HIP_TRY(hipGetLastError());
    }
    return DFM_OK;
}
