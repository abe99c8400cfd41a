// bbox_decode.hip -- the 3-D anchor head's maps to NMS candidates (reference: models/dense_heads/anchor3d_head.py
// :458-533, the body of Anchor3DHead.get_bboxes_single up to its box3d_multiclass_nms call) and the standalone
// DeltaXYZWLHRBBoxCoder.decode.
//
// Semantics (include/dfm_hip_bbox_decode.h, a part of include/dfm_hip.h, states them in full).  The reference permutes and copies the three maps, runs a
// sigmoid over every class logit, a row maximum, torch.topk over all N anchors, four gathers and the 15-operation
// decode to keep K = nms_pre rows out of N.  Here, per level and for the whole batch, with nothing copied to the
// host and a launch count that depends on neither N nor the batch:
//   keys     one lane per anchor reads its C class logits in place (any strides) and stores the order-preserving
//            32-bit form of max_c sigmoid(logit) -- NaN as the largest key -- and counts the key's top 11 bits
//            into a per-image histogram (LDS first, then one global atomic per occupied bin and workgroup);
//   refine   twice: every workgroup finds, from the histogram of the digit before, the bin that holds the K-th
//            greatest key, and counts the next digit (11, then 10 bits) of the keys inside that bin;
//   compact  the three digits give T, the K-th greatest key, and how many keys equal to T are wanted.  Keys
//            greater than T go to the candidate list (an atomic counter: their order is settled later); the keys
//            equal to T are only counted, per 256 anchors;
//   order    one workgroup per image: the candidates, then the wanted keys equal to T from the lowest anchor
//            indices upwards (a prefix over the counts, a walk through the few 256-anchor chunks that hold them),
//            as (key << 32 | ~anchor) in LDS; a bitonic sort in descending order gives descending keys with equal
//            keys in ascending anchor index;
//   decode   one lane per kept row gathers its S deltas, C logits, 2 direction logits and its anchor, and writes
//            the five outputs.
// Without a cut (nms_pre <= 0 or N <= nms_pre) only the decode runs, over all N anchors in anchor order.
// Integer atomics only: the same bits run after run.
#include "bbox_coder.h"

using namespace dfm;

namespace {

constexpr int BLOCK = 256;             // four waves
constexpr int ITEMS = 8;               // anchors per lane in the key passes: fewer global atomics per bin
constexpr int SPAN = BLOCK * ITEMS;
constexpr int BINS = 2048;             // 11 + 11 + 10 bits
constexpr int TIE_CHUNK = BLOCK;       // the keys equal to T are counted per this many anchors
constexpr int ORDER_BLOCK = 1024;
constexpr int MAX_BATCH = DFM_ANCHOR_HEAD_MAX_BATCH;

struct Map {
    const void *p;
    long long sb, sc, sh, sw;          // element strides: image, channel, row, column
};

struct Head {
    int batch, h, w, a, c, s;          // A anchors per location, C classes, S box columns
    int n, k;                          // anchors per image, rows kept per image
    Map cls, reg, dir;
};

template <typename T>
__device__ __forceinline__ float map_at(const Map &m, int b, int ch, int y, int x)
{
    return elem<T>::load(((const T *)m.p)[b * m.sb + ch * m.sc + y * m.sh + x * m.sw]);
}

// the float order as an unsigned order; NaN above everything
__device__ __forceinline__ uint32_t ordered_key(float v)
{
    if (v != v) return 0xffffffffu;
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// torch's max over a row: the greatest value, NaN if there is one
__device__ __forceinline__ float max_nan(float m, float v)
{
    return (v > m || v != v) ? v : m;
}

__device__ __forceinline__ uint32_t digit_of(uint32_t key, int level)
{
    return level == 0 ? key >> 21 : level == 1 ? (key >> 10) & 2047u : key & 1023u;
}

// workspace: 32-bit words [hist B*3*BINS][count B][sel B*4][tiecnt B*chunks][keys B*N], then 64-bit [cand B*K]
struct Scratch {
    uint32_t *hist, *count, *sel, *tiecnt, *keys;
    unsigned long long *cand;
    int chunks;
    size_t zero_bytes, total_bytes;
};

inline Scratch carve(void *ws, int batch, int n, int k)
{
    Scratch s;
    const size_t chunks = ((size_t)n + TIE_CHUNK - 1) / TIE_CHUNK;
    uint32_t *w = (uint32_t *)ws;
    size_t at = 0;
    s.hist = w + at;
    at += (size_t)batch * 3 * BINS;
    s.count = w + at;
    at += (size_t)batch;
    s.sel = w + at;
    at += (size_t)batch * 4;
    s.zero_bytes = at * 4;
    s.tiecnt = w + at;
    at += (size_t)batch * chunks;
    s.keys = w + at;
    at += (size_t)batch * (size_t)n;
    at = (at + 3) & ~(size_t)3;                                       // 16-byte boundary
    s.cand = (unsigned long long *)(w + at);
    s.total_bytes = at * 4 + (size_t)batch * (size_t)k * 8;
    s.chunks = (int)chunks;
    return s;
}

template <typename T>
__global__ __launch_bounds__(BLOCK) void keys_kernel(Head hd, uint32_t *__restrict__ keys,
                                                     uint32_t *__restrict__ hist)
{
    __shared__ uint32_t s_hist[BINS];
    const int b = blockIdx.y;
    for (int i = threadIdx.x; i < BINS; i += BLOCK) s_hist[i] = 0;
    __syncthreads();
    for (int j = 0; j < ITEMS; ++j) {
        const long long n = (long long)blockIdx.x * SPAN + j * BLOCK + threadIdx.x;
        if (n >= hd.n) continue;
        const int a = (int)(n % hd.a), pos = (int)(n / hd.a), x = pos % hd.w, y = pos / hd.w;
        float m = sigmoid_f32(map_at<T>(hd.cls, b, a * hd.c, y, x));
        for (int c = 1; c < hd.c; ++c) m = max_nan(m, sigmoid_f32(map_at<T>(hd.cls, b, a * hd.c + c, y, x)));
        const uint32_t key = ordered_key(m);
        keys[(size_t)b * hd.n + n] = key;
        atomicAdd(&s_hist[digit_of(key, 0)], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < BINS; i += BLOCK)
        if (s_hist[i]) atomicAdd(hist + (size_t)b * 3 * BINS + i, s_hist[i]);
}

// By the whole workgroup: the digit d with above(d) < k <= above(d) + hist[d], above(d) = the count of the digits
// greater than d; out[0] = d, out[1] = k - above(d).  Needs 1 <= k <= sum(hist); otherwise out = (0, 1).
__device__ __forceinline__ void find_digit(const uint32_t *__restrict__ hist, uint32_t k, uint32_t *s_scan,
                                           uint32_t *out)
{
    const int t = threadIdx.x;
    constexpr int PER = BINS / BLOCK;
    uint32_t loc[PER], sum = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) {                       // lane t owns the bins BINS-1-PER*t downwards
        loc[j] = hist[BINS - 1 - (t * PER + j)];
        sum += loc[j];
    }
    if (t == 0) {
        out[0] = 0;
        out[1] = 1;
    }
    s_scan[t] = sum;
    __syncthreads();
    for (int off = 1; off < BLOCK; off <<= 1) {
        const uint32_t v = t >= off ? s_scan[t - off] : 0;
        __syncthreads();
        s_scan[t] += v;
        __syncthreads();
    }
    const uint32_t incl = s_scan[t];
    uint32_t above = incl - sum;
    if (above < k && k <= incl) {                         // one lane at most
        bool found = false;
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            if (!found && k <= above + loc[j]) {
                out[0] = (uint32_t)(BINS - 1 - (t * PER + j));
                out[1] = k - above;
                found = true;
            }
            above += loc[j];
        }
    }
    __syncthreads();
}

// the digits above `level` of the K-th greatest key of image b: prefix = those digits, k = the rank inside them
__device__ __forceinline__ void resolve(const uint32_t *__restrict__ hist, int b, int level, uint32_t k0,
                                        uint32_t *s_scan, uint32_t *s_out, uint32_t &prefix, uint32_t &k)
{
    prefix = 0;
    k = k0;
    for (int l = 0; l < level; ++l) {
        find_digit(hist + ((size_t)b * 3 + l) * BINS, k, s_scan, s_out);
        prefix = (prefix << (l == 2 ? 10 : 11)) | s_out[0];
        k = s_out[1];
        __syncthreads();                                  // s_out is read before the next round rewrites it
    }
}

__global__ __launch_bounds__(BLOCK) void refine_kernel(int n, int kk, int level, const uint32_t *__restrict__ keys,
                                                       uint32_t *__restrict__ hist)
{
    __shared__ uint32_t s_hist[BINS];
    __shared__ uint32_t s_scan[BLOCK];
    __shared__ uint32_t s_out[2];
    const int b = blockIdx.y;
    for (int i = threadIdx.x; i < BINS; i += BLOCK) s_hist[i] = 0;
    uint32_t prefix, k;
    resolve(hist, b, level, (uint32_t)kk, s_scan, s_out, prefix, k);      // (its barriers cover s_hist)
    const int shift = level == 1 ? 21 : 10;
    for (int j = 0; j < ITEMS; ++j) {
        const long long i = (long long)blockIdx.x * SPAN + j * BLOCK + threadIdx.x;
        if (i >= n) continue;
        const uint32_t key = keys[(size_t)b * n + i];
        if ((key >> shift) == prefix) atomicAdd(&s_hist[digit_of(key, level)], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < BINS; i += BLOCK)
        if (s_hist[i]) atomicAdd(hist + ((size_t)b * 3 + level) * BINS + i, s_hist[i]);
}

__global__ __launch_bounds__(BLOCK) void compact_kernel(int n, int kk, int chunks, const uint32_t *__restrict__ keys,
                                                        const uint32_t *__restrict__ hist,
                                                        uint32_t *__restrict__ count, uint32_t *__restrict__ sel,
                                                        uint32_t *__restrict__ tiecnt,
                                                        unsigned long long *__restrict__ cand)
{
    __shared__ uint32_t s_scan[BLOCK];
    __shared__ uint32_t s_out[2];
    __shared__ uint32_t s_tie[ITEMS];
    const int b = blockIdx.y;
    if (threadIdx.x < ITEMS) s_tie[threadIdx.x] = 0;
    uint32_t cut, need;                                   // T and how many keys equal to it are kept
    resolve(hist, b, 3, (uint32_t)kk, s_scan, s_out, cut, need);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        sel[b * 4 + 0] = cut;
        sel[b * 4 + 1] = need;
    }
    for (int j = 0; j < ITEMS; ++j) {
        const long long i = (long long)blockIdx.x * SPAN + j * BLOCK + threadIdx.x;
        const uint32_t key = i < n ? keys[(size_t)b * n + i] : 0u;
        if (i < n && key > cut) {
            const uint32_t at = atomicAdd(count + b, 1u);
            if (at < (uint32_t)kk) cand[(size_t)b * kk + at] = ((unsigned long long)key << 32) | (uint32_t)~(uint32_t)i;
        }
        const unsigned long long ties = __ballot(i < n && key == cut);
        if ((threadIdx.x & 63) == 0 && ties) atomicAdd(&s_tie[j], (uint32_t)__popcll(ties));
    }
    __syncthreads();
    if (threadIdx.x < ITEMS) {
        const long long chunk = (long long)blockIdx.x * ITEMS + threadIdx.x;
        if (chunk < chunks) tiecnt[(size_t)b * chunks + chunk] = s_tie[threadIdx.x];
    }
}

__global__ __launch_bounds__(ORDER_BLOCK) void order_kernel(int n, int kk, int kpad, int chunks,
                                                            const uint32_t *__restrict__ keys,
                                                            const uint32_t *__restrict__ sel,
                                                            const uint32_t *__restrict__ tiecnt,
                                                            const unsigned long long *__restrict__ cand,
                                                            long long *__restrict__ topk)
{
    extern __shared__ unsigned long long s_c[];           // kpad entries of (key << 32 | ~anchor); 0 = empty
    __shared__ uint32_t s_scan[ORDER_BLOCK];
    const int b = blockIdx.x, t = threadIdx.x;
    const uint32_t cut = sel[b * 4 + 0];
    const uint32_t need = min(sel[b * 4 + 1], (uint32_t)kk);
    const uint32_t greater = (uint32_t)kk - need;
    for (int i = t; i < kpad; i += ORDER_BLOCK) s_c[i] = (uint32_t)i < greater ? cand[(size_t)b * kk + i] : 0ull;
    __syncthreads();
    uint32_t running = 0;                                 // keys equal to T in the chunks before c0 (uniform)
    for (int c0 = 0; c0 < chunks && running < need; c0 += ORDER_BLOCK) {
        const int chunk = c0 + t;
        const uint32_t cnt = chunk < chunks ? tiecnt[(size_t)b * chunks + chunk] : 0u;
        s_scan[t] = cnt;
        __syncthreads();
        for (int off = 1; off < ORDER_BLOCK; off <<= 1) {
            const uint32_t v = t >= off ? s_scan[t - off] : 0;
            __syncthreads();
            s_scan[t] += v;
            __syncthreads();
        }
        uint32_t r = running + s_scan[t] - cnt;           // keys equal to T before this lane's chunk
        if (cnt > 0 && r < need) {
            const long long i0 = (long long)chunk * TIE_CHUNK;
            for (int i = 0; i < TIE_CHUNK && i0 + i < n && r < need; ++i)
                if (keys[(size_t)b * n + i0 + i] == cut) {
                    s_c[greater + r] = ((unsigned long long)cut << 32) | (uint32_t)~(uint32_t)(i0 + i);
                    ++r;
                }
        }
        running += s_scan[ORDER_BLOCK - 1];
        __syncthreads();                                  // s_scan is rewritten by the next round
    }
    __syncthreads();
    for (int size = 2; size <= kpad; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = t; i < (kpad >> 1); i += ORDER_BLOCK) {
                const int lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
                const bool descending = (lo & size) == 0;
                const unsigned long long u = s_c[lo], v = s_c[hi];
                if ((u < v) == descending) {
                    s_c[lo] = v;
                    s_c[hi] = u;
                }
            }
            __syncthreads();
        }
    for (int i = t; i < kk; i += ORDER_BLOCK) {
        const unsigned long long v = s_c[i];
        const uint32_t idx = v ? ~(uint32_t)v : 0u;
        topk[(size_t)b * kk + i] = idx < (uint32_t)n ? (long long)idx : 0;
    }
}

// torch.max over the two direction logits: the index of the greater, 0 on a tie, the first NaN if there is one
__device__ __forceinline__ long long direction_of(float d0, float d1)
{
    if (d0 != d0) return 0;
    if (d1 != d1) return 1;
    return d1 > d0 ? 1 : 0;
}

template <typename T>
__global__ __launch_bounds__(BLOCK) void decode_rows_kernel(Head hd, int identity, const float *__restrict__ anchors,
                                                            float *__restrict__ bboxes, float *__restrict__ for_nms,
                                                            float *__restrict__ scores,
                                                            long long *__restrict__ dir_scores,
                                                            long long *__restrict__ topk)
{
    const long long r = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (r >= (long long)hd.batch * hd.k) return;
    const int b = (int)(r / hd.k);
    long long idx = identity ? r - (long long)b * hd.k : topk[r];
    if (idx < 0 || idx >= hd.n) idx = 0;
    const int a = (int)(idx % hd.a), pos = (int)(idx / hd.a), x = pos % hd.w, y = pos / hd.w;
    float an[BBOX_CODE_MAX], t[BBOX_CODE_MAX], box[BBOX_CODE_MAX], bev[5];
#pragma unroll
    for (int c = 0; c < BBOX_CODE_MAX; ++c)
        if (c < hd.s) {
            an[c] = anchors[idx * hd.s + c];
            t[c] = map_at<T>(hd.reg, b, a * hd.s + c, y, x);
        }
    delta_xyzwlhr_decode_row(an, t, hd.s, box);
    bev_xyxyr(box, bev);
#pragma unroll
    for (int c = 0; c < BBOX_CODE_MAX; ++c)
        if (c < hd.s) bboxes[r * hd.s + c] = box[c];
#pragma unroll
    for (int c = 0; c < 5; ++c) for_nms[r * 5 + c] = bev[c];
    for (int c = 0; c < hd.c; ++c) scores[r * (hd.c + 1) + c] = sigmoid_f32(map_at<T>(hd.cls, b, a * hd.c + c, y, x));
    scores[r * (hd.c + 1) + hd.c] = 0.0f;                  // the reference's dummy background column
    dir_scores[r] = direction_of(map_at<T>(hd.dir, b, a * 2, y, x), map_at<T>(hd.dir, b, a * 2 + 1, y, x));
    if (identity) topk[r] = idx;
}

__global__ __launch_bounds__(BLOCK) void decode_kernel(const float *__restrict__ anchors,
                                                       const float *__restrict__ deltas, int n, int width,
                                                       float *__restrict__ out)
{
    const long long r = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (r >= n) return;
    float an[BBOX_CODE_MAX], t[BBOX_CODE_MAX], box[BBOX_CODE_MAX];
#pragma unroll
    for (int c = 0; c < BBOX_CODE_MAX; ++c)
        if (c < width) {
            an[c] = anchors[r * width + c];
            t[c] = deltas[r * width + c];
        }
    delta_xyzwlhr_decode_row(an, t, width, box);
#pragma unroll
    for (int c = 0; c < BBOX_CODE_MAX; ++c)
        if (c < width) out[r * width + c] = box[c];
}

// the checked sizes of a call: 0 and the filled Head, or the error
int check_desc(const dfm_anchor_head_desc *d, Head &hd)
{
    if (!d) return set_error(DFM_ERR_INVALID_ARG, "NULL descriptor");
    if (d->dtype != DFM_F32 && d->dtype != DFM_BF16)
        return set_errorf(DFM_ERR_UNSUPPORTED, "dtype %d: the head's maps are DFM_F32 or DFM_BF16", d->dtype);
    if (d->box_code_size < BBOX_CODE_MIN || d->box_code_size > BBOX_CODE_MAX)
        return set_errorf(DFM_ERR_UNSUPPORTED, "box_code_size %d: the decode is built for %d .. %d columns",
                          d->box_code_size, BBOX_CODE_MIN, BBOX_CODE_MAX);
    if (d->batch < 0 || d->h < 0 || d->w < 0) return set_error(DFM_ERR_INVALID_ARG, "negative size");
    if (d->anchors_per_location <= 0 || d->num_classes <= 0)
        return set_error(DFM_ERR_INVALID_ARG, "non-positive anchors_per_location or num_classes");
    if (d->batch > MAX_BATCH)
        return set_errorf(DFM_ERR_UNSUPPORTED, "%d images: at most DFM_ANCHOR_HEAD_MAX_BATCH = %d per call", d->batch,
                          MAX_BATCH);
    const long long n = (long long)d->h * d->w * d->anchors_per_location;
    if (n > 0x7fffffffll) return set_error(DFM_ERR_UNSUPPORTED, "more than 2^31 - 1 anchors per image");
    const long long k = d->nms_pre > 0 && n > d->nms_pre ? d->nms_pre : n;
    if (k > DFM_BOX_NMS_MAX_N)
        return set_errorf(DFM_ERR_UNSUPPORTED, "%lld rows kept per image: at most DFM_BOX_NMS_MAX_N = %d, the limit of "
                          "the NMS that follows (set nms_pre)", k, DFM_BOX_NMS_MAX_N);
    hd.batch = d->batch;
    hd.h = d->h;
    hd.w = d->w;
    hd.a = d->anchors_per_location;
    hd.c = d->num_classes;
    hd.s = d->box_code_size;
    hd.n = (int)n;
    hd.k = (int)k;
    hd.cls = Map{nullptr, d->cls_stride[0], d->cls_stride[1], d->cls_stride[2], d->cls_stride[3]};
    hd.reg = Map{nullptr, d->reg_stride[0], d->reg_stride[1], d->reg_stride[2], d->reg_stride[3]};
    hd.dir = Map{nullptr, d->dir_stride[0], d->dir_stride[1], d->dir_stride[2], d->dir_stride[3]};
    return DFM_OK;
}

int order_lds_bytes(int k)
{
    int kpad = 2;
    while (kpad < k) kpad <<= 1;
    return kpad * 8;
}

}  // namespace

extern "C" DFM_API size_t dfm_anchor_head_candidates_workspace_bytes(const dfm_anchor_head_desc *d)
{
    Head hd;
    if (check_desc(d, hd) != DFM_OK) return 0;
    if (hd.batch == 0 || hd.n == 0 || hd.k == hd.n) return 0;          // without a cut nothing is selected
    return carve(nullptr, hd.batch, hd.n, hd.k).total_bytes;
}

extern "C" DFM_API int dfm_anchor_head_candidates(const dfm_anchor_head_desc *d, const void *cls, const void *reg,
                                                  const void *dir, const float *anchors, float *bboxes,
                                                  float *bboxes_for_nms, float *scores, int64_t *dir_scores,
                                                  int64_t *topk_inds, void *workspace, size_t workspace_bytes,
                                                  void *stream)
{
    Head hd;
    const int rc = check_desc(d, hd);
    if (rc != DFM_OK) return rc;
    if (hd.batch == 0 || hd.n == 0) return DFM_OK;
    if (!cls || !reg || !dir || !anchors || !bboxes || !bboxes_for_nms || !scores || !dir_scores || !topk_inds)
        return set_error(DFM_ERR_INVALID_ARG, "NULL device pointer");
    hd.cls.p = cls;
    hd.reg.p = reg;
    hd.dir.p = dir;
    const bool cut = hd.k < hd.n;
    hipStream_t s = (hipStream_t)stream;
    if (cut) {
        const size_t need = carve(nullptr, hd.batch, hd.n, hd.k).total_bytes;
        if (!workspace || workspace_bytes < need)
            return set_errorf(DFM_ERR_WORKSPACE, "the head's candidates need %zu workspace bytes, got %zu", need,
                              workspace ? workspace_bytes : (size_t)0);
        if ((uintptr_t)workspace & 15) return set_error(DFM_ERR_INVALID_ARG, "workspace must be 16-byte aligned");
        const Scratch sc = carve(workspace, hd.batch, hd.n, hd.k);
        const int lds = order_lds_bytes(hd.k), kpad = lds / 8;
        if (lds > 48 * 1024) {
            const int rc2 = ensure_dynamic_lds((const void *)order_kernel, lds);
            if (rc2 != DFM_OK) return rc2;
        }
        HIP_TRY(hipMemsetAsync(workspace, 0, sc.zero_bytes, s));
        const dim3 grid((unsigned)(((long long)hd.n + SPAN - 1) / SPAN), (unsigned)hd.batch), block(BLOCK);
        by_dtype(d->dtype, [&](auto t) {
            hipLaunchKernelGGL(keys_kernel<decltype(t)>, grid, block, 0, s, hd, sc.keys, sc.hist);
        });
        HIP_TRY(hipGetLastError());
        for (int level = 1; level <= 2; ++level) {
            hipLaunchKernelGGL(refine_kernel, grid, block, 0, s, hd.n, hd.k, level, (const uint32_t *)sc.keys, sc.hist);
            HIP_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(compact_kernel, grid, block, 0, s, hd.n, hd.k, sc.chunks, (const uint32_t *)sc.keys,
                           (const uint32_t *)sc.hist, sc.count, sc.sel, sc.tiecnt, sc.cand);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(order_kernel, dim3((unsigned)hd.batch), dim3(ORDER_BLOCK), (size_t)lds, s, hd.n, hd.k, kpad,
                           sc.chunks, (const uint32_t *)sc.keys, (const uint32_t *)sc.sel,
                           (const uint32_t *)sc.tiecnt, (const unsigned long long *)sc.cand, (long long *)topk_inds);
        HIP_TRY(hipGetLastError());
    }
    const long long rows = (long long)hd.batch * hd.k;
    const dim3 grid((unsigned)((rows + BLOCK - 1) / BLOCK)), block(BLOCK);
    by_dtype(d->dtype, [&](auto t) {
        hipLaunchKernelGGL(decode_rows_kernel<decltype(t)>, grid, block, 0, s, hd, cut ? 0 : 1, anchors, bboxes,
                           bboxes_for_nms, scores, (long long *)dir_scores, (long long *)topk_inds);
    });
    HIP_TRY(hipGetLastError());
    return DFM_OK;
}

extern "C" DFM_API int dfm_delta_xyzwlhr_decode(const float *anchors, const float *deltas, int32_t n,
                                                int32_t box_code_size, float *out, void *stream)
{
    if (n < 0) return set_error(DFM_ERR_INVALID_ARG, "negative row count");
    if (box_code_size < BBOX_CODE_MIN || box_code_size > BBOX_CODE_MAX)
        return set_errorf(DFM_ERR_UNSUPPORTED, "box_code_size %d: the decode is built for %d .. %d columns",
                          box_code_size, BBOX_CODE_MIN, BBOX_CODE_MAX);
    if (n == 0) return DFM_OK;
    if (!anchors || !deltas || !out) return set_error(DFM_ERR_INVALID_ARG, "NULL device pointer");
    hipLaunchKernelGGL(decode_kernel, dim3((unsigned)(((long long)n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0,
                       (hipStream_t)stream, anchors, deltas, n, box_code_size, out);
    HIP_TRY(hipGetLastError());
    return DFM_OK;
}
