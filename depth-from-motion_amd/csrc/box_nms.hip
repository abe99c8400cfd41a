// box_nms.hip -- rotated / axis-aligned BEV non-maximum suppression and rotated-box IoU
// (reference call chain: Anchor3DHead.get_bboxes_single -> box3d_multiclass_nms -> nms_bev / nms_normal_bev,
// mmdet3d/core/post_processing/box3d_nms.py, whose nms_rotated / nms are CUDA ops of mmcv).
//
// Semantics (include/dfm_hip.h states them in full): candidates are visited in the caller's order (descending
// score), a candidate is suppressed by an earlier KEPT one whose IoU with it is strictly greater than the
// threshold, and the kept ones are returned in that order.
//
//   mask   : grid (column block, row block, class); blocks below the diagonal return at once.  One wave: the 64
//            column boxes are staged in LDS with their cos / sin, every lane owns one row box and tests it
//            against the 64 columns (all lanes read the same LDS address: a broadcast), building the 64-bit word
//            "columns of this block that row suppresses".  The centre-distance test against the sum of the
//            half-diagonals comes first; the polygon clip runs only for the pairs that pass it.
//   reduce : one wave per class.  The `removed` bit vector lives in registers, word w in lane w % 64.  The
//            candidates are taken 64 at a time: the block's 64 diagonal words are fetched with one load per
//            lane and the serial pass over the block runs on registers alone (v_readlane of a uniform lane);
//            then the rows of the block's kept candidates are OR-ed into `removed` with independent loads.
//            Kept indices go out with one vector store per block, the count with one store.  No atomics.
//   iou    : one lane per (i, j) pair, the same device function.
//
// The IoU itself (midpoint translation, centre-distance rejection, Sutherland-Hodgman in registers, shoelace) is
// rbox_geom.h, shared with iou3d_loss.hip.
#include "rbox_geom.h"

using namespace dfm;

namespace {

constexpr int NMS_MAX_N = DFM_BOX_NMS_MAX_N;             // candidates per class
constexpr int NMS_RW = NMS_MAX_N / 64 / 64;              // `removed` words per lane of the reduce wave
constexpr size_t NMS_MAX_WS = (size_t)1 << 30;           // workspace cap: 1 GiB

// IoU of two axis-aligned boxes (x1, y1, x2, y2), no +1 offset; 0 when either area is below 1e-14
__device__ __forceinline__ float abox_iou(const float4 &a, const float4 &b)
{
    const float area_a = (a.z - a.x) * (a.w - a.y), area_b = (b.z - b.x) * (b.w - b.y);
    if (area_a < AREA_EPS || area_b < AREA_EPS) return 0.0f;
    const float iw = fmaxf(fminf(a.z, b.z) - fmaxf(a.x, b.x), 0.0f);
    const float ih = fmaxf(fminf(a.w, b.w) - fmaxf(a.y, b.y), 0.0f);
    const float inter = iw * ih;
    return inter / (area_a + area_b - inter);
}

// box `idx` of boxes (num_boxes, 5); an index outside the array gives a zero-size box (suppresses nothing)
__device__ __forceinline__ RBox load_rbox(const float *__restrict__ boxes, long long idx, int num_boxes, bool xyxyr)
{
    RBox o{0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f};
    if (idx < 0 || idx >= num_boxes) return o;
    const float *b = boxes + (size_t)idx * 5;
    const float b0 = b[0], b1 = b[1], b2 = b[2], b3 = b[3];
    if (xyxyr) {  // nms_bev's conversion, the same fp32 operations (box3d_nms.py:259-262)
        o.x = (b0 + b2) / 2.0f; o.y = (b1 + b3) / 2.0f; o.w = b2 - b0; o.h = b3 - b1;
    } else {
        o.x = b0; o.y = b1; o.w = b2; o.h = b3;
    }
    sincosf(b[4], &o.s, &o.c);
    return o;
}

__device__ __forceinline__ float4 load_abox(const float *__restrict__ boxes, long long idx, int num_boxes)
{
    if (idx < 0 || idx >= num_boxes) return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const float *b = boxes + (size_t)idx * 5;
    return make_float4(b[0], b[1], b[2], b[3]);
}

__device__ __forceinline__ int class_count(const int *__restrict__ counts, int c, int n)
{
    const int v = counts[c];
    return v < 0 ? 0 : (v > n ? n : v);
}

// mask (classes, n, words) uint64: bit j of word cb of row i = "candidate i suppresses candidate 64 cb + j".
// Written for cb >= i / 64 and i < counts[c] only; nothing else is ever read.
template <bool ROT>
__global__ __launch_bounds__(64) void box_nms_mask_kernel(const float *__restrict__ boxes, int num_boxes, int xyxyr,
                                                          const long long *__restrict__ order,
                                                          const int *__restrict__ counts, int n, int words, float thr,
                                                          unsigned long long *__restrict__ mask)
{
    const int cb = blockIdx.x, rb = blockIdx.y, c = blockIdx.z;
    if (cb < rb) return;
    const int cnt = class_count(counts, c, n);
    if (cb * 64 >= cnt) return;
    __shared__ RBox s_r[ROT ? 64 : 1];
    __shared__ float4 s_a[ROT ? 1 : 64];
    const int lane = threadIdx.x;
    const int row = rb * 64 + lane, col = cb * 64 + lane;
    const long long *ord = order + (size_t)c * n;
    const long long ridx = row < cnt ? ord[row] : -1, cidx = col < cnt ? ord[col] : -1;
    RBox rr{};
    float4 ra{};
    if constexpr (ROT) {
        rr = load_rbox(boxes, ridx, num_boxes, xyxyr != 0);
        s_r[lane] = cb == rb ? rr : load_rbox(boxes, cidx, num_boxes, xyxyr != 0);
    } else {
        ra = load_abox(boxes, ridx, num_boxes);
        s_a[lane] = cb == rb ? ra : load_abox(boxes, cidx, num_boxes);
    }
    __syncthreads();
    const int ncol = min(64, cnt - cb * 64);
    unsigned long long word = 0;
    for (int j = 0; j < ncol; ++j) {
        float iou;
        if constexpr (ROT) iou = rbox_iou(rr, s_r[j]);
        else iou = abox_iou(ra, s_a[j]);
        const bool hit = (cb * 64 + j > row) && (iou > thr);
        word |= (unsigned long long)hit << j;
    }
    if (row < cnt) mask[((size_t)c * n + row) * words + cb] = word;
}

__device__ __forceinline__ unsigned long long readlane64(unsigned long long v, int lane)
{
    const unsigned lo = __builtin_amdgcn_readlane((int)(unsigned)v, lane);
    const unsigned hi = __builtin_amdgcn_readlane((int)(unsigned)(v >> 32), lane);
    return ((unsigned long long)hi << 32) | lo;
}

// keep (classes, n) int64: the kept candidates' entries of `order`, in order; kept_counts (classes)
__global__ __launch_bounds__(64) void box_nms_reduce_kernel(const unsigned long long *__restrict__ mask,
                                                            const long long *__restrict__ order,
                                                            const int *__restrict__ counts, int n, int words,
                                                            long long *__restrict__ keep,
                                                            int *__restrict__ kept_counts)
{
    const int c = blockIdx.x, lane = threadIdx.x;
    const int cnt = class_count(counts, c, n);
    const int W = (cnt + 63) / 64;
    const unsigned long long *m = mask + (size_t)c * n * words;
    const long long *ord = order + (size_t)c * n;
    long long *out = keep + (size_t)c * n;
    unsigned long long removed[NMS_RW];
#pragma unroll
    for (int k = 0; k < NMS_RW; ++k) removed[k] = 0;
    int total = 0;
    for (int wb = 0; wb < W; ++wb) {
        unsigned long long mine = 0;
#pragma unroll
        for (int k = 0; k < NMS_RW; ++k) mine = (wb >> 6) == k ? removed[k] : mine;
        unsigned long long cur = readlane64(mine, wb & 63);
        const int left = cnt - wb * 64;                       // candidates in this block
        if (left < 64) cur |= ~0ull << left;
        const int row = wb * 64 + lane;
        const unsigned long long diag = row < cnt ? m[(size_t)row * words + wb] : 0ull;
        unsigned long long kept = 0;
        for (int j = 0; j < 64; ++j) {                        // wave-uniform: registers only
            const unsigned long long dj = readlane64(diag, j);
            if (!((cur >> j) & 1ull)) {
                kept |= 1ull << j;
                cur |= dj;
            }
        }
        if ((kept >> lane) & 1ull)
            out[total + __popcll(kept & ((1ull << lane) - 1ull))] = ord[row];
        total += __popcll(kept);
        for (unsigned long long rest = kept; rest; rest &= rest - 1ull) {
            const int r = wb * 64 + __builtin_ctzll(rest);
#pragma unroll
            for (int k = 0; k < NMS_RW; ++k) {
                const int w = k * 64 + lane;
                if (w > wb && w < W) removed[k] |= m[(size_t)r * words + w];
            }
        }
    }
    if (lane == 0) kept_counts[c] = total;
}

// out[i][j] = IoU(b1[i], b2[j]) (n, m), or out[i] = IoU(b1[i], b2[i]) when aligned; boxes (., 5) xywhr
__global__ __launch_bounds__(256) void box_iou_rotated_kernel(const float *__restrict__ b1, int n,
                                                              const float *__restrict__ b2, int m, int aligned,
                                                              float *__restrict__ out)
{
    const long long total = aligned ? (long long)n : (long long)n * m;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const long long i = aligned ? e : e / m, j = aligned ? e : e - i * m;
    out[e] = rbox_iou(load_rbox(b1, i, n, false), load_rbox(b2, j, m, false));
}

size_t ws_bytes(int n, int classes) { return (size_t)classes * (size_t)n * (size_t)((n + 63) / 64) * 8; }

int check_sizes(int n, int classes)
{
    if (n < 0 || classes <= 0) return set_error(DFM_ERR_INVALID_ARG, "negative n or non-positive classes");
    if (n > NMS_MAX_N)
        return set_errorf(DFM_ERR_UNSUPPORTED, "n = %d candidates per class is above DFM_BOX_NMS_MAX_N = %d", n,
                          NMS_MAX_N);
    if (classes > 65535 || ws_bytes(n, classes) > NMS_MAX_WS)
        return set_errorf(DFM_ERR_UNSUPPORTED, "n = %d x %d classes needs a %zu-byte mask, above the 1 GiB cap", n,
                          classes, ws_bytes(n, classes));
    return DFM_OK;
}

template <bool ROT>
int nms(const float *boxes, int num_boxes, int xyxyr, const int64_t *order, const int32_t *counts, int n, int classes,
        float thr, int64_t *keep, int32_t *kept_counts, void *ws, size_t ws_given, void *stream)
{
    int rc = check_sizes(n, classes);
    if (rc != DFM_OK) return rc;
    if (num_boxes < 0) return set_error(DFM_ERR_INVALID_ARG, "negative num_boxes");
    if (n == 0) return DFM_OK;
    if (!boxes || !order || !counts || !keep || !kept_counts || !ws)
        return set_error(DFM_ERR_INVALID_ARG, "NULL device pointer");
    if (num_boxes == 0) return set_error(DFM_ERR_INVALID_ARG, "n > 0 candidates of num_boxes = 0 boxes");
    if (ws_given < ws_bytes(n, classes))
        return set_errorf(DFM_ERR_WORKSPACE, "box NMS needs %zu workspace bytes, got %zu", ws_bytes(n, classes),
                          ws_given);
    hipStream_t st = (hipStream_t)stream;
    const int words = (n + 63) / 64;
    hipLaunchKernelGGL((box_nms_mask_kernel<ROT>), dim3(words, words, classes), dim3(64), 0, st, boxes, num_boxes,
                       xyxyr, (const long long *)order, counts, n, words, thr, (unsigned long long *)ws);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(box_nms_reduce_kernel, dim3(classes), dim3(64), 0, st, (const unsigned long long *)ws,
                       (const long long *)order, counts, n, words, (long long *)keep, kept_counts);
    HIP_TRY(hipGetLastError());
    return DFM_OK;
}

}  // namespace

extern "C" DFM_API size_t dfm_box_nms_workspace_bytes(int32_t n, int32_t classes)
{
    if (check_sizes(n, classes) != DFM_OK) return 0;
    return ws_bytes(n, classes);
}

extern "C" DFM_API int dfm_box_nms_rotated(const float *boxes, int32_t num_boxes, int32_t xyxyr, const int64_t *order,
                                           const int32_t *counts, int32_t n, int32_t classes, float iou_threshold,
                                           int64_t *keep, int32_t *kept_counts, void *workspace,
                                           size_t workspace_bytes, void *stream)
{
    return nms<true>(boxes, num_boxes, xyxyr, order, counts, n, classes, iou_threshold, keep, kept_counts, workspace,
                     workspace_bytes, stream);
}

extern "C" DFM_API int dfm_box_nms_aligned(const float *boxes, int32_t num_boxes, const int64_t *order,
                                           const int32_t *counts, int32_t n, int32_t classes, float iou_threshold,
                                           int64_t *keep, int32_t *kept_counts, void *workspace,
                                           size_t workspace_bytes, void *stream)
{
    return nms<false>(boxes, num_boxes, 0, order, counts, n, classes, iou_threshold, keep, kept_counts, workspace,
                      workspace_bytes, stream);
}

extern "C" DFM_API int dfm_box_iou_rotated(const float *boxes1, int32_t n, const float *boxes2, int32_t m,
                                           int32_t aligned, float *out, void *stream)
{
    if (n < 0 || m < 0) return set_error(DFM_ERR_INVALID_ARG, "negative box count");
    if (aligned && n != m) return set_error(DFM_ERR_INVALID_ARG, "aligned IoU needs as many boxes2 as boxes1");
    if (n == 0 || m == 0) return DFM_OK;
    if (!boxes1 || !boxes2 || !out) return set_error(DFM_ERR_INVALID_ARG, "NULL device pointer");
    const long long total = aligned ? (long long)n : (long long)n * m;
    const long long blocks = (total + 255) / 256;
    if (blocks > 0x7fffffffll) return set_error(DFM_ERR_UNSUPPORTED, "IoU matrix too large");
    hipLaunchKernelGGL(box_iou_rotated_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, boxes1, n,
                       boxes2, m, aligned, out);
    HIP_TRY(hipGetLastError());
    return DFM_OK;
}
