// deform_conv.hip -- modulated deformable 3x3 convolution (DCNv2): the columns and their backward
// (reference: the Waymo configs' ResNet-101 with dcn=dict(type='DCNv2', deform_groups=1) runs mmcv's
// modulated_deform_conv2d; mmcv is not a dependency, include/dfm_hip_deform_conv.h states the semantics in full).
//
//   sample   one workgroup per 16 consecutive output pixels.  Phase 1: one lane per (pixel, tap) computes the
//            coordinate, the range test, floor, the four weights and the mask ONCE into LDS.  Phase 2: one lane per
//            (pixel, tap, 16-byte channel vector): four 16-byte corner loads out of Cin contiguous values, the blend
//            in the header's operation order (no contraction: the file is built with -ffp-contract=off), one 16-byte
//            store into the pixel's run of 9 * Cin contiguous column values.
//   bwd      one workgroup (eight waves) per TH x TW tile of output pixels of one image; channels of a deform group
//            64 at a time, one wave per (pixel, tap), one lane per channel, the next pair's five loads in flight while
//            the wave works on this one.  grad_offset / grad_mask: a lane's products, a fixed
//            xor-shuffle tree, lane 0 adds the chunk's sum to the pair's LDS slot (the pair belongs to one wave): no
//            atomics, the same bits every run.  grad_x: corners that fall into the tile's LDS window of the input are
//            LDS atomics; the window is flushed once per chunk as global atomics of 64 consecutive channels (256
//            contiguous bytes per wave instruction); corners outside the window go to global atomics directly, in a
//            pass of their own, so that the main loop's only global memory operations are its loads.
// Every loop is bounded by the descriptor's sizes, which the entry points check on the host; the float -> int
// conversion of a coordinate happens after the range test only.
#include "dfm_common.h"

using namespace dfm;

namespace {

constexpr int BLOCK = 256;
constexpr int FWD_PIX = 16;                 // output pixels per workgroup of the sample kernel
constexpr int BWD_BLOCK = 512;              // the backward kernel: eight waves
constexpr int BWD_WAVES = BWD_BLOCK / 64;
constexpr int BWD_MAX_PIX = 64;             // output pixels per tile of the backward kernel (8 x 8)
constexpr int CHUNK = 64;                   // channels per pass of the backward kernel: one per lane
constexpr int WIN_MAX_BYTES = 54 * 1024;    // the LDS window of the input: positions x CHUNK floats

struct Geo {
    int N, C, H, W, Ho, Wo;
    int sh, sw, ph, pw, dh, dw;
    int G, Cg;                              // deform groups, channels per group
    int logit;
    long long os[4], ms[4];                 // element strides of offset and mask: (n, channel, ho, wo)
};

struct Tap {
    float hh, hw, lh, lw, m;
    int row, w0;                            // n * H + h0 (the row of the top corners among all images' rows), w0
    int flags;                              // 1: the pixel exists, 2: the sample is inside, 4 / 8: the top / bottom
                                            // corners' row lies in the map
};

__device__ __forceinline__ float sigmoid_f32(float z)
{
    return __fdiv_rn(1.0f, 1.0f + expf(-z));
}

template <typename O>
__device__ __forceinline__ Tap make_tap(const Geo &g, const O *__restrict__ offset, const O *__restrict__ mask, int n,
                                        int ho, int wo, int k, int grp)
{
    Tap t;
    const int i = k / 3, j = k - 3 * i;
    const long long ob = n * g.os[0] + ho * g.os[2] + wo * g.os[3] + (long long)(grp * 18 + 2 * k) * g.os[1];
    const float dy = elem<O>::load(offset[ob]);
    const float dx = elem<O>::load(offset[ob + g.os[1]]);
    float m = elem<O>::load(mask[n * g.ms[0] + (long long)(grp * 9 + k) * g.ms[1] + ho * g.ms[2] + wo * g.ms[3]]);
    if (g.logit) m = sigmoid_f32(m);
    const float h = (float)(ho * g.sh - g.ph + i * g.dh) + dy;
    const float w = (float)(wo * g.sw - g.pw + j * g.dw) + dx;
    t.m = m;
    t.flags = 1;
    t.hh = t.hw = t.lh = t.lw = 0.0f;
    t.row = t.w0 = 0;
    if (h > -1.0f && w > -1.0f && h < (float)g.H && w < (float)g.W) {   // false for NaN, +-inf, +-1e30
        const float hf = floorf(h), wf = floorf(w);
        const int h0 = (int)hf;                                          // -1 .. H - 1: after the test only
        t.row = n * g.H + h0;
        t.w0 = (int)wf;
        t.lh = h - hf;
        t.lw = w - wf;
        t.hh = 1.0f - t.lh;
        t.hw = 1.0f - t.lw;
        t.flags = 3 | (h0 >= 0 ? 4 : 0) | (h0 + 1 <= g.H - 1 ? 8 : 0);
    }
    return t;
}

// grid = ceil(P / FWD_PIX), P = N * Ho * Wo
template <typename T, typename O>
__global__ __launch_bounds__(BLOCK) void deform_sample_kernel(Geo g, long long P, const T *__restrict__ x,
                                                              const O *__restrict__ offset,
                                                              const O *__restrict__ mask, T *__restrict__ col)
{
    constexpr int V = vec16<T>::N;
    __shared__ Tap taps[FWD_PIX * 9];
    const long long p0 = (long long)blockIdx.x * FWD_PIX;
    const int vpi = g.Cg / V;                       // 16-byte vectors per (pixel, tap, group)
    for (int grp = 0; grp < g.G; ++grp) {
        if (grp) __syncthreads();
        for (int it = threadIdx.x; it < FWD_PIX * 9; it += BLOCK) {
            const int pixel = it / 9, k = it - pixel * 9;
            const long long p = p0 + pixel;
            Tap t;
            t.flags = 0;
            if (p < P) {
                const int wo = (int)(p % g.Wo);
                const long long q = p / g.Wo;
                t = make_tap(g, offset, mask, (int)(q / g.Ho), (int)(q % g.Ho), wo, k, grp);
            }
            taps[it] = t;
        }
        __syncthreads();
        const int total = FWD_PIX * 9 * vpi;
        for (int e = threadIdx.x; e < total; e += BLOCK) {
            const int it = e / vpi, v = e - it * vpi;
            const Tap t = taps[it];
            if (!(t.flags & 1)) continue;
            const int pixel = it / 9, k = it - pixel * 9;
            const int c = grp * g.Cg + v * V;
            float out[V];
#pragma unroll
            for (int q = 0; q < V; ++q) out[q] = 0.0f;
            if (t.flags & 2) {
                float v00[V], v01[V], v10[V], v11[V];
#pragma unroll
                for (int q = 0; q < V; ++q) v00[q] = v01[q] = v10[q] = v11[q] = 0.0f;
                const bool top = t.flags & 4, bot = t.flags & 8, lef = t.w0 >= 0, rig = t.w0 + 1 <= g.W - 1;
                const long long r0 = (long long)t.row * g.W + t.w0;           // pixel index of the top-left corner
                if (top && lef) load16(x + (size_t)r0 * g.C + c, v00);
                if (top && rig) load16(x + (size_t)(r0 + 1) * g.C + c, v01);
                if (bot && lef) load16(x + (size_t)(r0 + g.W) * g.C + c, v10);
                if (bot && rig) load16(x + (size_t)(r0 + g.W + 1) * g.C + c, v11);
                const float w00 = t.hh * t.hw, w01 = t.hh * t.lw, w10 = t.lh * t.hw, w11 = t.lh * t.lw;
#pragma unroll
                for (int q = 0; q < V; ++q) {
                    const float val = ((w00 * v00[q] + w01 * v01[q]) + w10 * v10[q]) + w11 * v11[q];
                    out[q] = val * t.m;
                }
            }
            store16(col + ((size_t)(p0 + pixel) * 9 + k) * g.C + c, out);
        }
    }
}

struct BwdTile {
    int th, tw;             // output pixels per tile
    int tiles_h, tiles_w;   // tiles per image
    int wh, ww;             // the LDS window's rows and columns; 0: no window
    int margin;             // rows / columns of the window beyond the tile's zero-offset footprint, each side
};

// what one lane reads for one (pixel, tap): its channel of grad_col and of the four corners
struct Item {
    float gc, v00, v01, v10, v11;
};

// Always five loads, whatever the tap: a corner outside the map (or a pair without a pixel, a sample outside, a lane
// past the group's channels) reads element 0 instead and the value is dropped afterwards.  The count of loads in
// flight is then a constant the compiler can wait on, which is what lets the next pair's loads overlap this pair's work.
template <typename T>
__device__ __forceinline__ Item fetch_item(const Geo &g, const Tap &t, size_t prow, int cc, bool active,
                                           const T *__restrict__ x, const T *__restrict__ gcol)
{
    const bool in = active && (t.flags & 2);
    const bool top = in && (t.flags & 4), bot = in && (t.flags & 8), lef = t.w0 >= 0, rig = t.w0 + 1 <= g.W - 1;
    const long long r0 = (long long)t.row * g.W + t.w0;
    const size_t c = in ? (size_t)cc : 0;
    const float gc = elem<T>::load(gcol[in ? prow * g.C + c : 0]);
    const float v00 = elem<T>::load(x[top && lef ? (size_t)r0 * g.C + c : 0]);
    const float v01 = elem<T>::load(x[top && rig ? (size_t)(r0 + 1) * g.C + c : 0]);
    const float v10 = elem<T>::load(x[bot && lef ? (size_t)(r0 + g.W) * g.C + c : 0]);
    const float v11 = elem<T>::load(x[bot && rig ? (size_t)(r0 + g.W + 1) * g.C + c : 0]);
    Item d;
    d.gc = in ? gc : 0.0f;
    d.v00 = top && lef ? v00 : 0.0f;
    d.v01 = top && rig ? v01 : 0.0f;
    d.v10 = bot && lef ? v10 : 0.0f;
    d.v11 = bot && rig ? v11 : 0.0f;
    return d;
}

__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s);
    return v;
}

// grid = N * tiles_h * tiles_w; dynamic LDS = wh * ww * CHUNK floats
template <typename T, typename O>
__global__ __launch_bounds__(BWD_BLOCK) void deform_bwd_kernel(Geo g, BwdTile tl, const T *__restrict__ x,
                                                           const O *__restrict__ offset, const O *__restrict__ mask,
                                                           const T *__restrict__ gcol, float *__restrict__ goff,
                                                           long long gos0, long long gos1, long long gos2,
                                                           long long gos3, float *__restrict__ gmask, long long gms0,
                                                           long long gms1, long long gms2, long long gms3,
                                                           float *__restrict__ gx)
{
    extern __shared__ float win[];
    __shared__ Tap taps[BWD_MAX_PIX * 9];
    __shared__ float part[BWD_MAX_PIX * 9 * 3];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int per_image = tl.tiles_h * tl.tiles_w;
    const int n = blockIdx.x / per_image, tt = blockIdx.x - n * per_image;
    const int th0 = (tt / tl.tiles_w) * tl.th, tw0 = (tt % tl.tiles_w) * tl.tw;
    const int items = tl.th * tl.tw * 9;
    const int row0 = th0 * g.sh - g.ph - tl.margin, col0 = tw0 * g.sw - g.pw - tl.margin;
    const int win_elems = gx ? tl.wh * tl.ww * CHUNK : 0;
    for (int e = tid; e < win_elems; e += BWD_BLOCK) win[e] = 0.0f;
    // row of grad_col of item `it`: ((n, ho, wo) pixel) * 9 + tap; only used where the pixel exists
    auto col_row = [&](int it) {
        const int pixel = it / 9, k = it - pixel * 9;
        return ((size_t)(n * g.Ho + th0 + pixel / tl.tw) * g.Wo + tw0 + pixel % tl.tw) * 9 + k;
    };
    for (int grp = 0; grp < g.G; ++grp) {
        if (grp) __syncthreads();
        for (int it = tid; it < items; it += BWD_BLOCK) {
            const int pixel = it / 9, k = it - pixel * 9;
            const int ho = th0 + pixel / tl.tw, wo = tw0 + pixel % tl.tw;
            Tap t;
            t.flags = 0;
            if (ho < g.Ho && wo < g.Wo) t = make_tap(g, offset, mask, n, ho, wo, k, grp);
            taps[it] = t;
            part[it * 3] = part[it * 3 + 1] = part[it * 3 + 2] = 0.0f;
        }
        __syncthreads();
        for (int c0 = 0; c0 < g.Cg; c0 += CHUNK) {
            const int c = c0 + lane;
            const bool active = c < g.Cg;
            const int cc = grp * g.Cg + c;
            // the wave walks its items with the NEXT item's five loads in flight while it works on this one
            int it = wave;                                        // wave-uniform
            Tap t = taps[it < items ? it : 0];
            if (it >= items) t.flags = 0;
            Item d = fetch_item(g, t, col_row(it), cc, active, x, gcol);
            while (it < items) {
                const int nx = it + BWD_WAVES;
                Tap tn = taps[nx < items ? nx : 0];
                if (nx >= items) tn.flags = 0;
                const Item dn = fetch_item(g, tn, col_row(nx), cc, active, x, gcol);
                if (t.flags & 2) {                                // else no pixel, or a sample outside: gradients 0
                    const bool top = t.flags & 4, bot = t.flags & 8, lef = t.w0 >= 0, rig = t.w0 + 1 <= g.W - 1;
                    const float w00 = t.hh * t.hw, w01 = t.hh * t.lw, w10 = t.lh * t.hw, w11 = t.lh * t.lw;
                    if (goff) {
                        const float val = ((w00 * d.v00 + w01 * d.v01) + w10 * d.v10) + w11 * d.v11;
                        const float dvh = t.hw * (d.v10 - d.v00) + t.lw * (d.v11 - d.v01);
                        const float dvw = t.hh * (d.v01 - d.v00) + t.lh * (d.v11 - d.v10);
                        const float s0 = wave_sum(d.gc * dvh), s1 = wave_sum(d.gc * dvw), s2 = wave_sum(d.gc * val);
                        if (lane == 0) {
                            part[it * 3] += s0;
                            part[it * 3 + 1] += s1;
                            part[it * 3 + 2] += s2;
                        }
                    }
                    if (gx && active) {
                        const float gm = d.gc * t.m;
                        const int wr = t.row - n * g.H - row0, wc = t.w0 - col0;   // the top-left corner in the window
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const int dr = q >> 1, dc = q & 1;
                            const float wq = q == 0 ? w00 : q == 1 ? w01 : q == 2 ? w10 : w11;
                            const int r = wr + dr, cl = wc + dc;
                            // (a corner outside the window is left to the pass below: no global memory operation
                            //  in this loop but the five loads)
                            if ((dr ? bot : top) && (dc ? rig : lef) && (unsigned)r < (unsigned)tl.wh &&
                                (unsigned)cl < (unsigned)tl.ww)
                                atomicAdd(&win[(r * tl.ww + cl) * CHUNK + lane], gm * wq);
                        }
                    }
                }
                it = nx;
                t = tn;
                d = dn;
            }
            if (gx) {
                // the corners that fell outside the window (whether one did depends on the tap alone: the same for
                // the whole wave): straight to global memory, 64 consecutive channels per instruction
                for (int jt = wave; jt < items; jt += BWD_WAVES) {
                    const Tap u = taps[jt];
                    if (!(u.flags & 2)) continue;
                    const bool top = u.flags & 4, bot = u.flags & 8, lef = u.w0 >= 0, rig = u.w0 + 1 <= g.W - 1;
                    const int wr = u.row - n * g.H - row0, wc = u.w0 - col0;
                    bool out[4];
                    bool any = false;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int dr = q >> 1, dc = q & 1;
                        const int r = wr + dr, cl = wc + dc;
                        out[q] = (dr ? bot : top) && (dc ? rig : lef) &&
                                 !((unsigned)r < (unsigned)tl.wh && (unsigned)cl < (unsigned)tl.ww);
                        any = any || out[q];
                    }
                    if (!any || !active) continue;
                    const long long r0 = (long long)u.row * g.W + u.w0;
                    const float gm = elem<T>::load(gcol[col_row(jt) * g.C + cc]) * u.m;
                    const float w00 = u.hh * u.hw, w01 = u.hh * u.lw, w10 = u.lh * u.hw, w11 = u.lh * u.lw;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const float wq = q == 0 ? w00 : q == 1 ? w01 : q == 2 ? w10 : w11;
                        if (out[q]) atomicAdd(gx + (size_t)(r0 + (q >> 1) * g.W + (q & 1)) * g.C + cc, gm * wq);
                    }
                }
            }
            if (win_elems) {
                __syncthreads();
                for (int e = tid; e < win_elems; e += BWD_BLOCK) {    // flush; lane e & 63 = channel c0 + (e & 63)
                    const float v = win[e];
                    if (v != 0.0f) {
                        win[e] = 0.0f;
                        const int pos = e >> 6;
                        const int r = row0 + pos / tl.ww, cl = col0 + pos % tl.ww;
                        if (c0 + (e & 63) < g.Cg && (unsigned)r < (unsigned)g.H && (unsigned)cl < (unsigned)g.W)
                            atomicAdd(gx + ((size_t)(n * g.H + r) * g.W + cl) * g.C + grp * g.Cg + c0 + (e & 63), v);
                    }
                }
                __syncthreads();
            }
        }
        if (goff) {
            __syncthreads();
            for (int it = tid; it < items; it += BWD_BLOCK) {
                const Tap t = taps[it];
                if (!(t.flags & 1)) continue;
                const int pixel = it / 9, k = it - pixel * 9;
                const int ho = th0 + pixel / tl.tw, wo = tw0 + pixel % tl.tw;
                const long long ob = n * gos0 + ho * gos2 + wo * gos3 + (long long)(grp * 18 + 2 * k) * gos1;
                goff[ob] = part[it * 3] * t.m;
                goff[ob + gos1] = part[it * 3 + 1] * t.m;
                float gm = part[it * 3 + 2];
                if (g.logit) gm = gm * (t.m * (1.0f - t.m));
                gmask[n * gms0 + (long long)(grp * 9 + k) * gms1 + ho * gms2 + wo * gms3] = gm;
            }
        }
    }
}

// "" when the descriptor is well formed and one the kernels cover, else the reason; *code gets the status
const char *check_desc(const dfm_deform_desc *d, int *code)
{
    *code = DFM_ERR_INVALID_ARG;
    if (d->n < 1 || d->cin < 1 || d->h < 1 || d->w < 1 || d->ho < 1 || d->wo < 1) return "a size below 1";
    if (d->stride_h < 1 || d->stride_w < 1 || d->dil_h < 1 || d->dil_w < 1) return "stride and dilation start at 1";
    if (d->pad_h < 0 || d->pad_w < 0) return "negative padding";
    if (d->deform_groups < 1 || d->cin % d->deform_groups) return "deform_groups must divide the input channels";
    *code = DFM_ERR_UNSUPPORTED;
    if ((d->dtype != DFM_F32 && d->dtype != DFM_BF16) || (d->om_dtype != DFM_F32 && d->om_dtype != DFM_BF16))
        return "dtype: DFM_F32 or DFM_BF16";
    const long long lim = 1ll << 24;
    if (d->h > lim || d->w > lim || d->pad_h > lim || d->pad_w > lim || d->dil_h > lim || d->dil_w > lim ||
        d->stride_h > lim || d->stride_w > lim)
        return "a size above 2^24";
    if ((long long)d->ho * d->stride_h + d->pad_h + 2ll * d->dil_h > lim ||
        (long long)d->wo * d->stride_w + d->pad_w + 2ll * d->dil_w > lim)
        return "coordinate range above 2^24";
    *code = DFM_ERR_INVALID_ARG;
    const long long eh = (long long)d->h + 2ll * d->pad_h - (2ll * d->dil_h + 1);
    const long long ew = (long long)d->w + 2ll * d->pad_w - (2ll * d->dil_w + 1);
    if (eh < 0 || ew < 0 || d->ho != eh / d->stride_h + 1 || d->wo != ew / d->stride_w + 1)
        return "ho / wo are not the output size of this geometry";
    *code = DFM_ERR_UNSUPPORTED;
    const int vec = d->dtype == DFM_F32 ? 4 : 8;
    if ((d->cin / d->deform_groups) % vec) return "the channels of a deform group must be whole 16-byte vectors";
    if ((long long)d->n * d->ho * d->wo > 0x7fffffffll || (long long)d->n * d->h * d->w > 0x7fffffffll)
        return "more than 2^31 - 1 pixels";
    *code = DFM_OK;
    return "";
}

Geo make_geo(const dfm_deform_desc *d)
{
    Geo g;
    g.N = d->n; g.C = d->cin; g.H = d->h; g.W = d->w; g.Ho = d->ho; g.Wo = d->wo;
    g.sh = d->stride_h; g.sw = d->stride_w; g.ph = d->pad_h; g.pw = d->pad_w; g.dh = d->dil_h; g.dw = d->dil_w;
    g.G = d->deform_groups;
    g.Cg = d->cin / d->deform_groups;
    g.logit = d->mask_is_logit != 0;
    for (int i = 0; i < 4; ++i) {
        g.os[i] = d->offset_stride[i];
        g.ms[i] = d->mask_stride[i];
    }
    return g;
}

// a launch templated on the two element types, written once
template <typename F>
void by_dtypes(int32_t dtype, int32_t om_dtype, F &&f)
{
    by_dtype(dtype, [&](auto t) { by_dtype(om_dtype, [&](auto o) { f(t, o); }); });
}

}  // namespace

extern "C" DFM_API int dfm_deform_sample_fwd(const dfm_deform_desc *d, const void *x, const void *offset,
                                             const void *mask, void *col, void *stream)
{
    if (!d) return set_error(DFM_ERR_INVALID_ARG, "NULL descriptor");
    int code;
    const char *why = check_desc(d, &code);
    if (code != DFM_OK) return set_errorf(code, "dfm_deform_sample_fwd: %s", why);
    if (!x || !offset || !mask || !col) return set_error(DFM_ERR_INVALID_ARG, "dfm_deform_sample_fwd: NULL pointer");
    if (((uintptr_t)x | (uintptr_t)col) & 15)
        return set_error(DFM_ERR_INVALID_ARG, "dfm_deform_sample_fwd: x and col must be 16-byte aligned");
    const int osz = d->om_dtype == DFM_F32 ? 4 : 2;
    if (((uintptr_t)offset | (uintptr_t)mask) & (osz - 1))
        return set_error(DFM_ERR_INVALID_ARG, "dfm_deform_sample_fwd: offset and mask must be element aligned");
    const Geo g = make_geo(d);
    const long long P = (long long)d->n * d->ho * d->wo;
    const long long blocks = (P + FWD_PIX - 1) / FWD_PIX;
    by_dtypes(d->dtype, d->om_dtype, [&](auto t, auto o) {
        using T = decltype(t);
        using O = decltype(o);
        hipLaunchKernelGGL((deform_sample_kernel<T, O>), dim3((unsigned)blocks), dim3(BLOCK), 0, (hipStream_t)stream,
                           g, P, (const T *)x, (const O *)offset, (const O *)mask, (T *)col);
    });
    HIP_TRY(hipGetLastError());
    return DFM_OK;
}

extern "C" DFM_API int dfm_deform_conv_bwd_cols(const dfm_deform_desc *d, const void *x, const void *offset,
                                                const void *mask, const void *grad_col, float *grad_offset,
                                                const int64_t *grad_offset_stride, float *grad_mask,
                                                const int64_t *grad_mask_stride, float *grad_x, void *stream)
{
    if (!d) return set_error(DFM_ERR_INVALID_ARG, "NULL descriptor");
    int code;
    const char *why = check_desc(d, &code);
    if (code != DFM_OK) return set_errorf(code, "dfm_deform_conv_bwd_cols: %s", why);
    if (!x || !offset || !mask || !grad_col)
        return set_error(DFM_ERR_INVALID_ARG, "dfm_deform_conv_bwd_cols: NULL pointer");
    if ((grad_offset == nullptr) != (grad_mask == nullptr))
        return set_error(DFM_ERR_INVALID_ARG, "dfm_deform_conv_bwd_cols: grad_offset and grad_mask go together");
    if (grad_offset && (!grad_offset_stride || !grad_mask_stride))
        return set_error(DFM_ERR_INVALID_ARG, "dfm_deform_conv_bwd_cols: NULL stride array");
    if (!grad_offset && !grad_x) return DFM_OK;
    const int tsz = d->dtype == DFM_F32 ? 4 : 2, osz = d->om_dtype == DFM_F32 ? 4 : 2;
    if ((((uintptr_t)x | (uintptr_t)grad_col) & (tsz - 1)) || (((uintptr_t)offset | (uintptr_t)mask) & (osz - 1)) ||
        (((uintptr_t)grad_offset | (uintptr_t)grad_mask | (uintptr_t)grad_x) & 3))
        return set_error(DFM_ERR_INVALID_ARG, "dfm_deform_conv_bwd_cols: a pointer is not element aligned");
    const Geo g = make_geo(d);
    // the largest tile whose window of the input fits; none: every corner goes to global memory
    static const int TILES[6][2] = {{8, 8}, {4, 8}, {4, 4}, {2, 4}, {2, 2}, {1, 1}};
    BwdTile tl;
    tl.th = tl.tw = 8;
    tl.wh = tl.ww = 0;
    tl.margin = 1;
    for (int i = 0; i < 12 && grad_x; ++i) {                  // per tile size a margin of 2, then of 1
        const int th = TILES[i / 2][0], tw = TILES[i / 2][1], margin = 2 - i % 2;
        const long long wh = (long long)(th - 1) * d->stride_h + 2ll * d->dil_h + 1 + 2 * margin;
        const long long ww = (long long)(tw - 1) * d->stride_w + 2ll * d->dil_w + 1 + 2 * margin;
        if (wh * ww * CHUNK * (long long)sizeof(float) <= WIN_MAX_BYTES) {
            tl.th = th;
            tl.tw = tw;
            tl.wh = (int)wh;
            tl.ww = (int)ww;
            tl.margin = margin;
            break;
        }
    }
    tl.tiles_h = (d->ho + tl.th - 1) / tl.th;
    tl.tiles_w = (d->wo + tl.tw - 1) / tl.tw;
    const long long blocks = (long long)d->n * tl.tiles_h * tl.tiles_w;
    if (blocks > 0x7fffffffll) return set_error(DFM_ERR_UNSUPPORTED, "dfm_deform_conv_bwd_cols: too many tiles");
    const int lds = tl.wh * tl.ww * CHUNK * (int)sizeof(float);
    int rc = DFM_OK;
    const int64_t zero[4] = {0, 0, 0, 0};
    const int64_t *gos = grad_offset ? grad_offset_stride : zero, *gms = grad_offset ? grad_mask_stride : zero;
    by_dtypes(d->dtype, d->om_dtype, [&](auto t, auto o) {
        using T = decltype(t);
        using O = decltype(o);
        if (lds) rc = ensure_dynamic_lds((const void *)deform_bwd_kernel<T, O>, WIN_MAX_BYTES);
        if (rc != DFM_OK) return;
        hipLaunchKernelGGL((deform_bwd_kernel<T, O>), dim3((unsigned)blocks), dim3(BWD_BLOCK), lds, (hipStream_t)stream, g,
                           tl, (const T *)x, (const O *)offset, (const O *)mask, (const T *)grad_col, grad_offset,
                           (long long)gos[0], (long long)gos[1], (long long)gos[2], (long long)gos[3], grad_mask,
                           (long long)gms[0], (long long)gms[1], (long long)gms[2], (long long)gms[3], grad_x);
    });
    if (rc != DFM_OK) return rc;
    HIP_TRY(hipGetLastError());
    return DFM_OK;
}
