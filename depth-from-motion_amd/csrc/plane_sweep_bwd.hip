// plane_sweep_bwd.hip -- backward of build_dfm_cost: grad feats += scatter(grad_out * weights), the
// adjoint of the forward sweep in plane_sweep.hip (same sampling positions: sweep_point_map).  Dense bf16
// sweeps hand the cur map and the far planes of the prev map to the matrix-product backward
// (plane_sweep_bwd_mfma.hip); the kernels here take the rest.  The fallback for maps wider than the LDS
// rows, sweep_bwd_kernel (lane-per-point scatter-add with global atomics), is compiled in plane_sweep.hip
// beside the forward kernel it mirrors -- see the comment there.
//
// Kernels
//   sweep_bwd_tile_kernel     : gradients accumulated in fixed-point LDS rows.
//   unpack_pixel_major_kernel : channels-last gradient volume -> the reference layout.
#include "plane_sweep_common.h"

#include <stdlib.h>

#include <algorithm>
#include <atomic>

using namespace dfm;

namespace {

std::atomic<int> g_last_bwd_kernel{0};  // process-wide: autograd runs the backward on its own thread

// ---------------------------------------------------------------------------
// backward: LDS-accumulating tiles.
// A workgroup = one band of 256 lattice points (same (h, w) for every plane) of ONE map x G plane
// groups (1024 lanes, G = 4 for the prev map; 512 lanes, G = 2 for the cur map), over a chunk of
// <= BWD_MAXP depth planes: lane (tid & 255) is the point, (tid >> 8) takes the planes
// p = group, group + G, ...
//   * Footprints once: a prologue computes every (plane, point) sampling position with the
//     forward kernel's own sweep_point_map and keeps it in an LDS table (corner + in-bounds bits
//     and the two fractions: 12 bytes per entry), so the C/CW channel passes that follow never
//     touch the geometry again.  (Round 1 re-derived the position per plane per pass and was
//     VALU-bound on exactly that: 34 of 39 ms at N*.)
//   * Per pass of CW channels the taps' gradients are added into a slab of feature rows in LDS
//     ([channel][row][x], 64-bit two's-complement fixed point: integer LDS atomics run at 10-14
//     lanes per clock, ds_add_f32 at 0.33 -- profiles/archive/r01_atomic_microbench.txt); the slab goes
//     to the global gradient with ONE coalesced fp32 atomic per touched pixel at the end of each
//     slab window (the longest run of planes whose rows fit; the chunk, unless the footprint
//     drifts far).
//       cur map : x = w +- 1e-5, the footprint stays inside a 3x3 block anchored at the lane's
//                 smallest corner: gradients are summed over the lane's planes in registers and
//                 scattered once per window (a lane whose footprint leaves its block -- general
//                 poses -- scatters that plane's taps straight to memory);
//       prev map: the footprint drifts with depth; the four taps are scattered per plane.
//   * The fixed-point scale is LOCAL: the prev kernel scans the pass's gradient values of its own
//     (chunk, band) first (they are re-read from L2 right after), the cur kernel takes the maximum
//     of its register sums at scatter time -- no pass over the whole gradient volume
//     (absmax_bits_kernel: 5 ms of the 39 at N*), no device allocation.  An all-zero pass is
//     skipped; a pass holding Inf / NaN takes plain float atomics so they propagate like torch's.
// ---------------------------------------------------------------------------
constexpr int BWD_MAXP = 32;  // depth planes per workgroup, at most
constexpr int BWD_PTS = 256;  // lattice points per band
// plane groups per workgroup: 4 for the prev map (70 VGPRs, LDS-atomic latency wants many waves),
// 2 for the cur map (its 3x3 register block needs more than the 128 VGPRs a 1024-lane group allows)
__host__ __device__ constexpr int bwd_groups(int half) { return half ? 4 : 2; }

struct BwdGrid {
    int batch, bands, band_pts, planes, dchunks, rows;
    int ablate;  // debug builds only (DFM_BWD_ABLATE): 1 no gradient loads, 2 no slab atomics, 4 no flush
    int grad_cl;  // 1: the gradient volume is stored channels-last, (B, D, h, w, 2C) (torch channels_last_3d)
    int row_tiles;  // 0: bands are runs of band_pts points of the flat (h, w) index;
                    // > 0 (strided sweeps): that many bands per lattice row, none crossing rows --
                    // consecutive lattice rows sample feature rows `cost_sample_factor` apart,
                    // which one slab window cannot hold
    int split;      // 1: only the planes before sweep_zoom_split (the matrix-product backward takes the rest)
};

// float -> 64-bit two's-complement fixed point (|x| < 2^61 after scaling): high word =
// floor(x / 2^32), low word = x - high * 2^32, which the fma delivers exactly except for a negative
// x of tiny magnitude, whose 2^32 - |x| rounds to 2^32 and saturates the conversion -- one unit of
// 2^-50 of the local maximum.  Five VALU operations; the pair is assembled from the two converted
// words (the first version went through a float -> u64 conversion: 12 operations per add).
__device__ __forceinline__ unsigned long long bwd_to_fixed(float x)
{
    const float hif = floorf(x * 2.3283064365386963e-10f);
    const float lof = __builtin_fmaf(hif, -4294967296.0f, x);  // in [0, 2^32]
    unsigned lo;
    asm("v_cvt_u32_f32 %0, %1" : "=v"(lo) : "v"(lof));  // saturating
    const unsigned hi = (unsigned)(int)hif;
    return ((unsigned long long)hi << 32) | (unsigned long long)lo;
}

// scale 2^sh with max|x| * 2^sh < 2^50 from the raw bits of max|x| (finite, non-zero)
__device__ __forceinline__ void bwd_scale(unsigned mb, float &fx_scale, float &fx_inv)
{
    const int sh = min(120, max(-100, 50 - ((int)(mb >> 23) - 127 + 1)));
    fx_scale = __uint_as_float((unsigned)(sh + 127) << 23);
    fx_inv = __uint_as_float((unsigned)(127 - sh) << 23);
}

#ifdef DFM_DEBUG_HOOKS
#define BWD_ABLATE(bit) ((tg.ablate & (bit)) != 0)
#else
#define BWD_ABLATE(bit) false
#endif
template <typename T, int CW, int HALF>
__global__ __launch_bounds__(BWD_PTS * bwd_groups(HALF)) void sweep_bwd_tile_kernel(
    SweepGeom g, SweepFast fast, BwdGrid tg, const T *__restrict__ gout,
    const float *__restrict__ depths, const float *__restrict__ P, const float *__restrict__ Pinv,
    const float *__restrict__ Tm, float *__restrict__ gcur, float *__restrict__ gprev)
{
    constexpr int BWD_GROUPS = bwd_groups(HALF);
    constexpr int NT = BWD_PTS * BWD_GROUPS;
    constexpr int VB = 8;  // plane slots whose gradient values are fetched together (one latency)
    extern __shared__ __attribute__((aligned(16))) unsigned long long slab[];
    __shared__ int yr[2 * BWD_MAXP];
    __shared__ unsigned wgm[3];  // rotating slots of the workgroup-wide maximum (see wg_max)
    __shared__ int wins[4 * BWD_MAXP + 1];  // slab windows of the chunk: count, then {first, last plane, y0, top}
    // block id = (band*dchunks + dchunk)*batch + b
    int th = blockIdx.x;
    const int b = th % tg.batch;
    th /= tg.batch;
    const int dchunk = th % tg.dchunks;
    const int band = th / tg.dchunks;
    const int tid = threadIdx.x, pt = tid & (BWD_PTS - 1), grp = tid >> 8;
    const int hw = g.h_out * g.w_out;
    const int W = g.w_in, H = g.h_in, HW = H * W;
    int p_lo = band * tg.band_pts, p_hi = min(p_lo + tg.band_pts, hw);
    if (tg.row_tiles > 0) {
        const int row = band / tg.row_tiles, t = band - row * tg.row_tiles;
        p_lo = row * g.w_out + t * tg.band_pts;
        p_hi = min(p_lo + tg.band_pts, (row + 1) * g.w_out);
    }
    const int d_lo = dchunk * tg.planes;
    int d_hi = min(d_lo + tg.planes, g.D);
    const float *Pb = P + b * 16, *Pib = Pinv + b * 16, *Tb = Tm + b * 16;
    if (tg.split) {  // workgroup-uniform
        d_hi = min(d_hi, sweep_zoom_split<HALF>(g, fast, Pb, Pib, Tb, depths, SWEEP_BWD_ZOOM_FOUR, threadIdx.x,
                                                BWD_PTS * BWD_GROUPS, &yr[0]));
        if (d_hi <= d_lo) return;
        __syncthreads();  // yr is initialised below
    }
    const int np = d_hi - d_lo;
    const int rows = tg.rows, slab_c = rows * W;
    // footprint table behind the slab: [plane][point] x {packed, fw, fn}
    uint32_t *fpT = (uint32_t *)(slab + (size_t)CW * slab_c);
    float *fwT = (float *)(fpT + tg.planes * BWD_PTS);
    float *fnT = fwT + tg.planes * BWD_PTS;
    const int idx = p_lo + pt;
    const bool live = idx < p_hi;
    const int hi = idx / g.w_out, wi = idx - hi * g.w_out;

    for (int i = tid; i < 2 * BWD_MAXP; i += NT) yr[i] = (i & 1) ? -1 : 0x7fffffff;
    for (int i = tid; i < CW * slab_c; i += NT) slab[i] = 0ull;
    if (tid < 3) wgm[tid] = 0u;
    __syncthreads();
    // workgroup-wide maximum with ONE barrier per call: round k accumulates into slot k % 3 and
    // clears slot (k + 1) % 3, which nobody reads (round k - 1 reads slot (k - 1) % 3) or
    // writes (round k + 1 starts after this barrier) meanwhile
    int mround = 0;
    auto wg_max = [&](unsigned m) -> unsigned {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o));
        const int slot = mround % 3;
        if ((tid & 63) == 0 && m) atomicMax(&wgm[slot], m);
        if (tid == 0) wgm[(mround + 1) % 3] = 0u;
        __syncthreads();
        ++mround;
        return wgm[slot];
    };

    // ---- footprints of the band's points in every plane of the chunk -> LDS table ------------
    int bx = 0x7fffffff, by = 0x7fffffff;  // cur map: block anchor = this lane's smallest corner
    for (int p = grp; p < np; p += BWD_GROUPS) {
        int ymin = 0x7fffffff, ymax = -1;
        uint32_t f = 0u;
        float fw = 0.0f, fn = 0.0f;
        if (live) {
            float sx, sy;
            sweep_point_map<HALF>(g, fast, Pb, Pib, Tb, depths[d_lo + p], hi, wi, sx, sy);
            f = bwd_footprint(sx, sy, H, W, fw, fn);
            if (f) {
                const int iyn = (int)(f & 0x1fffu) - 1, ixw = (int)((f >> 13) & 0x1fffu) - 1;
                if (f & (1u << 29)) { ymin = min(ymin, iyn); ymax = max(ymax, iyn); }
                if (f & (1u << 30)) { ymin = min(ymin, iyn + 1); ymax = max(ymax, iyn + 1); }
                bx = min(bx, ixw);
                by = min(by, iyn);
            }
        }
        fpT[p * BWD_PTS + pt] = f;
        fwT[p * BWD_PTS + pt] = fw;
        fnT[p * BWD_PTS + pt] = fn;
#pragma unroll
        for (int s2 = 32; s2 > 0; s2 >>= 1) {
            ymin = min(ymin, __shfl_xor(ymin, s2));
            ymax = max(ymax, __shfl_xor(ymax, s2));
        }
        if ((tid & 63) == 0 && ymax >= 0) {
            atomicMin(&yr[2 * p], ymin);
            atomicMax(&yr[2 * p + 1], ymax);
        }
    }
    __syncthreads();
    // slab windows: maximal runs of planes whose rows fit `rows` slab rows -- the same for every
    // channel pass, so they are laid out once
    if (tid == 0) {
        int nw = 0, p = 0;
        while (p < np) {
            while (p < np && yr[2 * p + 1] < yr[2 * p]) ++p;  // planes that miss the map
            if (p >= np) break;
            int umin = yr[2 * p], umax = yr[2 * p + 1], e = p;
            while (e + 1 < np) {
                const int l2 = yr[2 * (e + 1)], u2 = yr[2 * (e + 1) + 1];
                if (u2 >= l2) {
                    if (max(umax, u2) - min(umin, l2) + 1 > rows) break;
                    umin = min(umin, l2);
                    umax = max(umax, u2);
                }
                ++e;
            }
            wins[1 + 4 * nw] = p;
            wins[2 + 4 * nw] = e;
            wins[3 + 4 * nw] = umin;
            wins[4 + 4 * nw] = min(umax, umin + rows - 1);
            ++nw;
            p = e + 1;
        }
        wins[0] = nw;
    }
    __syncthreads();
    const int nwin = __builtin_amdgcn_readfirstlane(wins[0]);

    // element strides of the gradient volume: the reference layout (B, 2C, D, h, w), or channels-last
    // (B, D, h, w, 2C) -- what the NDHWC aggregation stack's backward hands over (read in place: the
    // 236 MB layout conversion at config K cost 2.2 ms per training step, and a lane's CW channels of a
    // (plane, point) are then adjacent)
    const size_t s_chan = tg.grad_cl ? (size_t)1 : (size_t)g.N;
    const size_t s_plane = tg.grad_cl ? (size_t)hw * 2 * g.C : (size_t)hw;
    const size_t s_point = tg.grad_cl ? (size_t)2 * g.C : (size_t)1;
    const T *go = gout + (size_t)b * 2 * g.C * g.N + (size_t)HALF * g.C * s_chan + (size_t)d_lo * s_plane +
                  (size_t)min(idx, p_hi - 1) * s_point;
    float *gf = (HALF ? gprev : gcur) + (size_t)b * g.C * HW;

    for (int c0 = 0; c0 < g.C; c0 += CW) {
        const int nc = min(CW, g.C - c0);
        const T *gp = go + (size_t)c0 * s_chan;
        float fx_scale = 1.0f, fx_inv = 1.0f;
        bool plain = false;  // Inf / NaN in this pass (window): plain float atomics
        int y0 = -1, top = -1;
        auto flush = [&]() {
            if (BWD_ABLATE(4)) return;
            const int cnt = (top - y0 + 1) * W;
            for (int c = 0; c < nc; ++c) {
                unsigned long long *sl = slab + c * slab_c;
                float *dst = gf + (size_t)(c0 + c) * HW + (size_t)y0 * W;
                for (int r = tid; r < cnt; r += NT) {
                    const unsigned long long v = sl[r];
                    if (v != 0ull) {
                        const float f = __builtin_fmaf((float)(int)(v >> 32), 4294967296.0f, (float)(unsigned)v);
                        atomicAdd(dst + r, f * fx_inv);
                        sl[r] = 0ull;
                    }
                }
            }
        };
        // gradient values of up to VB of this lane's planes (slots k0 .. k0+VB-1; slot k is plane
        // grp + k*G), all loads in flight together; planes outside the chunk / map give 0
        auto load_block = [&](int k0, T (&gv)[VB][CW]) {
            // every load is unconditional (clamped, always-valid address) and the masking happens on
            // the values afterwards: a load under a runtime condition makes hipcc branch around it
            // and wait for each one separately (cdna_hip_programming.md, ".s-level traps" (c))
#pragma unroll
            for (int k = 0; k < VB; ++k) {
                const int p = min(grp + (k0 + k) * BWD_GROUPS, np - 1);
#pragma unroll
                for (int c = 0; c < CW; ++c) gv[k][c] = gp[(size_t)p * s_plane + (size_t)min(c, nc - 1) * s_chan];
            }
#pragma unroll
            for (int k = 0; k < VB; ++k) {
                const int p = grp + (k0 + k) * BWD_GROUPS;
                const bool on = p < np && fpT[min(p, np - 1) * BWD_PTS + pt] != 0u && !BWD_ABLATE(1);
#pragma unroll
                for (int c = 0; c < CW; ++c) gv[k][c] = (on && c < nc) ? gv[k][c] : T(0);
            }
        };

        if constexpr (HALF == 1) {
            static_assert(BWD_MAXP / bwd_groups(1) <= VB, "one block holds all planes of a lane");
            T gv[VB][CW];
            load_block(0, gv);
            // ---- scale of this pass: max |grad| over the workgroup's values ----------------
            unsigned m = 0u;
#pragma unroll
            for (int k = 0; k < VB; ++k)
#pragma unroll
                for (int c = 0; c < CW; ++c) m = max(m, __float_as_uint(elem<T>::load(gv[k][c])) & 0x7fffffffu);
            const unsigned mb = wg_max(m);
            if (mb == 0u) continue;  // nothing to add in this pass
            plain = (mb >> 23) == 0xffu;
            if (!plain) bwd_scale(mb, fx_scale, fx_inv);
            // ---- windows of planes; the four taps of every plane go into the slab ----------
            for (int wi_ = 0; wi_ < nwin; ++wi_) {
                const int pw = __builtin_amdgcn_readfirstlane(wins[1 + 4 * wi_]);
                const int pe = __builtin_amdgcn_readfirstlane(wins[2 + 4 * wi_]);
                y0 = __builtin_amdgcn_readfirstlane(wins[3 + 4 * wi_]);
                top = __builtin_amdgcn_readfirstlane(wins[4 + 4 * wi_]);
#pragma unroll
                for (int k = 0; k < VB; ++k) {
                    const int p = grp + k * BWD_GROUPS;
                    if (p < pw || p > pe) continue;
                    const uint32_t f = fpT[p * BWD_PTS + pt];
                    if (!f) continue;
                    const int iyn = (int)(f & 0x1fffu) - 1, ixw = (int)((f >> 13) & 0x1fffu) - 1;
                    const float fw = fwT[p * BWD_PTS + pt], fn = fnT[p * BWD_PTS + pt];
                    const float cwt = (f & (1u << 27)) ? 1.0f - fw : 0.0f, cet = (f & (1u << 28)) ? fw : 0.0f;
                    const float rnt = (f & (1u << 29)) ? 1.0f - fn : 0.0f, rst = (f & (1u << 30)) ? fn : 0.0f;
                    const float wq[4] = {rnt * cwt, rnt * cet, rst * cwt, rst * cet};
                    float gvf[CW];
#pragma unroll
                    for (int c = 0; c < CW; ++c) gvf[c] = elem<T>::load(gv[k][c]);
                    const int rr0 = iyn - y0;  // >= 0 for an in-bounds north row: y0 <= the window's first row
                    if ((f & 0x78000000u) == 0x78000000u && rr0 + 1 < rows && !plain && !BWD_ABLATE(2)) {
                        // interior footprint inside the slab window (nearly every point): four taps x CW
                        // channels without a branch; channels past nc carry 0 into slab rows nobody flushes
                        unsigned long long *l = slab + rr0 * W + ixw;
                        const float w0 = wq[0] * fx_scale, w1 = wq[1] * fx_scale;
                        const float w2 = wq[2] * fx_scale, w3 = wq[3] * fx_scale;
#pragma unroll
                        for (int c = 0; c < CW; ++c) {
                            unsigned long long *lc = l + c * slab_c;
                            atomicAdd(lc, bwd_to_fixed(gvf[c] * w0));
                            atomicAdd(lc + 1, bwd_to_fixed(gvf[c] * w1));
                            atomicAdd(lc + W, bwd_to_fixed(gvf[c] * w2));
                            atomicAdd(lc + W + 1, bwd_to_fixed(gvf[c] * w3));
                        }
                        continue;
                    }
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        if (wq[q] == 0.0f) continue;  // out-of-bounds (or weightless) tap
                        const int py = iyn + (q >> 1), px = ixw + (q & 1);
                        const int rr = py - y0;  // >= 0: y0 <= the window's first row
                        if (BWD_ABLATE(2)) continue;
                        if (rr < rows && !plain) {
                            unsigned long long *l = slab + rr * W + px;
                            const float ws = wq[q] * fx_scale;
#pragma unroll
                            for (int c = 0; c < CW; ++c) atomicAdd(l + c * slab_c, bwd_to_fixed(gvf[c] * ws));
                        } else {  // taller than the slab window (rare), or a non-finite pass
                            float *gl = gf + (size_t)c0 * HW + (size_t)py * W + px;
#pragma unroll
                            for (int c = 0; c < CW; ++c)
                                if (c < nc) atomicAdd(gl + (size_t)c * HW, gvf[c] * wq[q]);
                        }
                    }
                }
                __syncthreads();
                flush();
                __syncthreads();
            }
        } else {
            // ---- cur map: per window, sum over this lane's planes in registers, one scatter -
            for (int wi_ = 0; wi_ < nwin; ++wi_) {
                const int pw = __builtin_amdgcn_readfirstlane(wins[1 + 4 * wi_]);
                const int pe = __builtin_amdgcn_readfirstlane(wins[2 + 4 * wi_]);
                y0 = __builtin_amdgcn_readfirstlane(wins[3 + 4 * wi_]);
                top = __builtin_amdgcn_readfirstlane(wins[4 + 4 * wi_]);
                float acc[9][CW];
#pragma unroll
                for (int cell = 0; cell < 9; ++cell)
#pragma unroll
                    for (int c = 0; c < CW; ++c) acc[cell][c] = 0.0f;
                for (int k0 = 0; k0 < BWD_MAXP / BWD_GROUPS; k0 += VB) {
                    if (grp + k0 * BWD_GROUPS > pe) break;  // uniform per wave (grp is)
                    T gv[VB][CW];
                    load_block(k0, gv);
#pragma unroll
                    for (int k = 0; k < VB; ++k) {
                        const int p = grp + (k0 + k) * BWD_GROUPS;
                        if (p < pw || p > pe) continue;
                        const uint32_t f = fpT[p * BWD_PTS + pt];
                        if (!f) continue;
                        float gvf[CW];
#pragma unroll
                        for (int c = 0; c < CW; ++c) gvf[c] = elem<T>::load(gv[k][c]);
                        const int iyn = (int)(f & 0x1fffu) - 1, ixw = (int)((f >> 13) & 0x1fffu) - 1;
                        const float fw = fwT[p * BWD_PTS + pt], fn = fnT[p * BWD_PTS + pt];
                        const float cw = (f & (1u << 27)) ? 1.0f - fw : 0.0f, ce = (f & (1u << 28)) ? fw : 0.0f;
                        const float rn = (f & (1u << 29)) ? 1.0f - fn : 0.0f, rs = (f & (1u << 30)) ? fn : 0.0f;
                        const int ox = ixw - bx, oy = iyn - by;  // 0 or 1 while the footprint stays in the block
                        if ((unsigned)ox <= 1u && (unsigned)oy <= 1u) {
                            const bool xlo = ox == 0, ylo = oy == 0;
                            const float cx[3] = {xlo ? cw : 0.0f, xlo ? ce : cw, xlo ? 0.0f : ce};
                            const float ry[3] = {ylo ? rn : 0.0f, ylo ? rs : rn, ylo ? 0.0f : rs};
#pragma unroll
                            for (int r = 0; r < 3; ++r)
#pragma unroll
                                for (int q = 0; q < 3; ++q) {
                                    const float wgt = ry[r] * cx[q];
#pragma unroll
                                    for (int c = 0; c < CW; ++c)
                                        acc[3 * r + q][c] = __builtin_fmaf(gvf[c], wgt, acc[3 * r + q][c]);
                                }
                        } else {  // the footprint left the lane's block (general poses): straight to memory
                            const float wq[4] = {rn * cw, rn * ce, rs * cw, rs * ce};
#pragma unroll
                            for (int q = 0; q < 4; ++q) {
                                if (wq[q] == 0.0f) continue;
                                float *gl = gf + (size_t)c0 * HW + (size_t)(iyn + (q >> 1)) * W + ixw + (q & 1);
#pragma unroll
                                for (int c = 0; c < CW; ++c)
                                    if (c < nc) atomicAdd(gl + (size_t)c * HW, gvf[c] * wq[q]);
                            }
                        }
                    }
                }
                // scale from the register sums themselves
                unsigned m = 0u;
#pragma unroll
                for (int cell = 0; cell < 9; ++cell)
#pragma unroll
                    for (int c = 0; c < CW; ++c) m = max(m, __float_as_uint(acc[cell][c]) & 0x7fffffffu);
                const unsigned mb = wg_max(m);
                if (mb != 0u) {
                    const bool pl = (mb >> 23) == 0xffu;
                    if (!pl) bwd_scale(mb, fx_scale, fx_inv);
#pragma unroll
                    for (int r = 0; r < 3; ++r) {
                        const int py = by + r, rr = py - y0;
#pragma unroll
                        for (int q = 0; q < 3; ++q) {
                            const int px = bx + q;
#pragma unroll
                            for (int c = 0; c < CW; ++c) {
                                const float v = acc[3 * r + q][c];
                                if (c >= nc || v == 0.0f || BWD_ABLATE(2)) continue;  // (out-of-bounds cells carry 0)
                                if (!pl && rr >= 0 && rr < rows)
                                    atomicAdd(slab + c * slab_c + rr * W + px, bwd_to_fixed(v * fx_scale));
                                else
                                    atomicAdd(gf + (size_t)(c0 + c) * HW + (size_t)py * W + px, v);
                            }
                        }
                    }
                    __syncthreads();
                    if (!pl) flush();
                    __syncthreads();
                }
            }
        }
    }
}

// (n, P, C) pixel-major -> (n, C, P) planar: 64 pixels x 8 16-byte channel pieces per workgroup through an
// LDS tile; 16-byte loads along the channels of a pixel, 16-byte stores along the pixels of a channel.
// C and P are whole 16-byte runs (checked by the caller).  grid = (ceil(P / 64), ceil(C / (8 * VEC)), n)
template <typename T>
__global__ __launch_bounds__(256) void unpack_pixel_major_kernel(const T *__restrict__ src, T *__restrict__ dst,
                                                                 int C, long long P)
{
    constexpr int VEC = 16 / sizeof(T);   // elements per 16-byte piece
    constexpr int TC = 8 * VEC;           // channels per tile
    constexpr int PITCH = 64 + VEC;       // tile row: 64 pixels (+ one piece: rows stay 16-byte aligned)
    __shared__ __attribute__((aligned(16))) T tile[TC * PITCH];
    const long long p0 = (long long)blockIdx.x * 64;
    const int c0 = blockIdx.y * TC;
    const size_t n = blockIdx.z;
    const T *s = src + n * (size_t)P * C;
    T *d = dst + n * (size_t)C * P;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int q = threadIdx.x + 256 * k;          // piece: pixel q / 8, channel piece q % 8
        const int p = q >> 3, cp = q & 7;
        if (p0 + p < P && c0 + cp * VEC < C) {
            const uint4 v = *(const uint4 *)(s + (size_t)(p0 + p) * C + c0 + cp * VEC);
            T e[VEC];
            __builtin_memcpy(e, &v, 16);
#pragma unroll
            for (int j = 0; j < VEC; ++j) tile[(cp * VEC + j) * PITCH + p] = e[j];
        }
    }
    __syncthreads();
    constexpr int PPR = 64 / VEC;  // 16-byte pieces per tile row
#pragma unroll
    for (int k = 0; k < (TC * PPR) / 256; ++k) {
        const int q = threadIdx.x + 256 * k;
        const int c = q / PPR, pp = (q % PPR) * VEC;
        if (c0 + c < C && p0 + pp < P)
            *(uint4 *)(d + (size_t)(c0 + c) * P + p0 + pp) = *(const uint4 *)(tile + c * PITCH + pp);
    }
}

int sweep_bwd_impl(const dfm_sweep_desc *desc, const void *grad_out, const float *depths, const float *cam2img,
                   const float *cam2img_inv, const float *cur2prev, float *grad_cur, float *grad_prev, void *stream,
                   const dfm_sweep_opts *opts, bool grad_cl)
{
    const bool force_scatter = opts && opts->kernel == 1;
    // 8: the tile kernel for the prev map only (the caller has the cur map from dfm_plane_sweep_bwd_cur_nhwc)
    const bool skip_cur = opts && opts->kernel == 8;
    int rc = sweep_check_desc(desc);
    if (rc != DFM_OK) return rc;
    if (!grad_out || !depths || !cam2img || !cam2img_inv || !cur2prev || !grad_cur || !grad_prev)
        return set_error(DFM_ERR_INVALID_ARG, "NULL device pointer");
    const SweepGeom g = sweep_make_geom(desc);
    hipStream_t st = (hipStream_t)stream;
    // dense sweeps whose feature rows fit the LDS: accumulate there (see sweep_bwd_tile_kernel).
    // One 1024-lane workgroup per CU: the LDS holds the footprint table of the chunk
    // (planes x 256 points x 12 B) and the slab of 64-bit accumulators (CW channels x rows x W).
    int planes = std::max(1, std::min(BWD_MAXP, (g.D + 3) / 4));
    int cw_max = 4;
#ifdef DFM_DEBUG_HOOKS
    if (const char *e = getenv("DFM_BWD_PLANES")) planes = std::max(1, std::min(BWD_MAXP, atoi(e)));
    if (const char *e = getenv("DFM_BWD_CW")) cw_max = atoi(e);
#endif
    const int table_bytes = planes * BWD_PTS * 12;
    const int budget = 160 * 1024 - 1024 - table_bytes;  // 1 KiB for the static LDS
    // channels per pass: as many (of 4) as leave >= 4 rows in the budget
    auto pick_cw = [&](int cw) {
        while (cw > 2 && (long long)budget / ((long long)cw * desc->w_in * 8) < 4) cw >>= 1;
        return cw;
    };
    const int cw_cur = pick_cw(cw_max), cw_prev = cw_cur;
    int row_cap = 8;
#ifdef DFM_DEBUG_HOOKS
    if (const char *e = getenv("DFM_BWD_ROWCAP")) row_cap = atoi(e);
#endif
    int rows_cur = (int)std::min<long long>(std::min(desc->h_in, row_cap),
                                            (long long)budget / ((long long)cw_cur * desc->w_in * 8));
#ifdef DFM_DEBUG_HOOKS
    if (const char *e = getenv("DFM_BWD_ROWS")) rows_cur = std::min(rows_cur, std::max(4, atoi(e)));
#endif
    const int rows_prev = rows_cur;
    const long long hw = (long long)g.h_out * g.w_out;
    if (!force_scatter && rows_cur >= 4 && desc->h_in < 4096 && desc->w_in < 8192) {
        BwdGrid tg;
        tg.batch = desc->batch;
        tg.band_pts = BWD_PTS;
        tg.row_tiles = desc->cost_sample_factor < 1.5f ? 0 : (g.w_out + tg.band_pts - 1) / tg.band_pts;
        tg.bands = tg.row_tiles ? g.h_out * tg.row_tiles : (int)((hw + tg.band_pts - 1) / tg.band_pts);
        tg.planes = planes;
        tg.ablate = 0;
        tg.grad_cl = grad_cl ? 1 : 0;
#ifdef DFM_DEBUG_HOOKS
        {
            const char *ab = getenv("DFM_BWD_ABLATE");
            tg.ablate = ab ? atoi(ab) : 0;
        }
#endif
        tg.dchunks = (g.D + tg.planes - 1) / tg.planes;
        const long long nb = (long long)tg.bands * tg.dchunks * desc->batch;
        if (nb > 2147483647ll) return set_error(DFM_ERR_UNSUPPORTED, "too many lattice points");
        const SweepFast fast = sweep_make_fast(desc);
        // dense bf16 sweeps: the matrix-product backward (plane_sweep_bwd_mfma.hip) takes the cur map and
        // the prev map's planes up to a zoom of SWEEP_BWD_ZOOM_FOUR map pixels per lattice point; this
        // kernel keeps the (nearest) planes beyond that (opts->kernel: 5 = never, 6 = whenever it applies
        // [the default])
        tg.split = 0;
        const bool mfma = !(opts && (opts->kernel == 5 || skip_cur)) && !grad_cl && sweep_bwd_mfma_supported(desc, grad_out);
        if (mfma) {
            tg.split = 1;
            rc = sweep_bwd_mfma_launch(desc, 0, grad_out, depths, cam2img, cam2img_inv, cur2prev, grad_cur, grad_prev,
                                       stream);
            if (rc != DFM_OK) return rc;
            rc = sweep_bwd_mfma_launch(desc, 1, grad_out, depths, cam2img, cam2img_inv, cur2prev, grad_cur, grad_prev,
                                       stream);
            if (rc != DFM_OK) return rc;
        }
#define DFM_BWD_LAUNCH(T, CW, HALF, ROWS)                                                            \
    do {                                                                                             \
        tg.rows = (ROWS);                                                                            \
        const int lds_bytes = (CW) * (ROWS) * desc->w_in * 8 + table_bytes;                          \
        rc = ensure_dynamic_lds((const void *)sweep_bwd_tile_kernel<T, CW, HALF>, lds_bytes);        \
        if (rc != DFM_OK) return rc;                                                                 \
        hipLaunchKernelGGL((sweep_bwd_tile_kernel<T, CW, HALF>), dim3((unsigned)nb),                 \
                           dim3(BWD_PTS * bwd_groups(HALF)),                                         \
                           lds_bytes, st, g, fast, tg, (const T *)grad_out, depths, cam2img,         \
                           cam2img_inv, cur2prev, grad_cur, grad_prev);                              \
    } while (0)
#define DFM_BWD_HALF(T, HALF, CWV, ROWS)                                                             \
    do {                                                                                             \
        if ((CWV) == 8) DFM_BWD_LAUNCH(T, 8, HALF, ROWS);                                            \
        else if ((CWV) == 4) DFM_BWD_LAUNCH(T, 4, HALF, ROWS);                                       \
        else DFM_BWD_LAUNCH(T, 2, HALF, ROWS);                                                       \
    } while (0)
        rc = by_dtype(desc->dtype, [&](auto t) {  // (a `return rc` of the macros leaves this lambda)
            using T = decltype(t);
            if (!mfma && !skip_cur) DFM_BWD_HALF(T, 0, cw_cur, rows_cur);  // (mfma: bf16 only)
            DFM_BWD_HALF(T, 1, cw_prev, rows_prev);
            return (int)DFM_OK;
        });
        if (rc != DFM_OK) return rc;
#undef DFM_BWD_HALF
#undef DFM_BWD_LAUNCH
        HIP_TRY(hipGetLastError());
        g_last_bwd_kernel.store(mfma ? 6 : 5);
        return DFM_OK;
    }
    if (grad_cl)  // the scatter kernel reads the reference layout only: the caller converts and calls dfm_plane_sweep_bwd
        return set_error(DFM_ERR_UNSUPPORTED, "channels-last gradient: the LDS-tile backward does not take this shape");
    if (skip_cur) return set_error(DFM_ERR_UNSUPPORTED, "prev-only backward: the LDS-tile kernel does not take this shape");
    rc = sweep_bwd_scatter_launch(desc, grad_out, depths, cam2img, cam2img_inv, cur2prev, grad_cur, grad_prev, stream);
    if (rc != DFM_OK) return rc;
    HIP_TRY(hipGetLastError());
    g_last_bwd_kernel.store(1);
    return DFM_OK;
}

}  // namespace

void dfm::sweep_set_last_bwd_kernel(int which) { g_last_bwd_kernel.store(which); }

extern "C" {

DFM_API int dfm_plane_sweep_bwd(const dfm_sweep_desc *desc, const void *grad_out,
                                const float *depths, const float *cam2img,
                                const float *cam2img_inv, const float *cur2prev, float *grad_cur,
                                float *grad_prev, void *stream)
{
    return dfm_plane_sweep_bwd_opts(desc, grad_out, depths, cam2img, cam2img_inv, cur2prev, grad_cur,
                                    grad_prev, stream, nullptr);
}

DFM_API int dfm_plane_sweep_bwd_opts(const dfm_sweep_desc *desc, const void *grad_out,
                                     const float *depths, const float *cam2img,
                                     const float *cam2img_inv, const float *cur2prev,
                                     float *grad_cur, float *grad_prev, void *stream,
                                     const dfm_sweep_opts *opts)
{
    return sweep_bwd_impl(desc, grad_out, depths, cam2img, cam2img_inv, cur2prev, grad_cur, grad_prev, stream, opts,
                          false);
}

DFM_API int dfm_plane_sweep_bwd_channels_last(const dfm_sweep_desc *desc, const void *grad_out,
                                              const float *depths, const float *cam2img,
                                              const float *cam2img_inv, const float *cur2prev,
                                              float *grad_cur, float *grad_prev, void *workspace,
                                              size_t workspace_bytes, void *stream)
{
    int rc = sweep_check_desc(desc);
    if (rc != DFM_OK) return rc;
    if (!grad_out) return set_error(DFM_ERR_INVALID_ARG, "NULL device pointer");
    const size_t esz = desc->dtype == DFM_BF16 ? 2 : 4;
    const long long P = (long long)desc->num_depths * desc->h_out * desc->w_out;
    const int C2 = 2 * desc->channels, vec = (int)(16 / esz);
    const size_t vol = (size_t)desc->batch * C2 * P * esz;
    if (workspace && workspace_bytes >= vol && C2 % vec == 0 && P % vec == 0 && !((uintptr_t)grad_out & 15) &&
        !((uintptr_t)workspace & 15) && desc->batch <= 65535) {
        // (B, P, 2C) -> (B, 2C, P) through an LDS tile at copy speed, then the backward on the reference
        // layout: its lanes are consecutive lattice points, which the planar layout serves with one
        // coalesced load per (plane, channel); read in place, a wave's 2-byte loads land 4C bytes apart
        // and every channel pass re-fetches the lines (config K: 2.2 ms instead of 1.2 ms)
        const dim3 grid((unsigned)((P + 63) / 64), (unsigned)((C2 + 8 * vec - 1) / (8 * vec)), desc->batch);
        by_dtype(desc->dtype, [&](auto t) {
            using T = decltype(t);
            hipLaunchKernelGGL(unpack_pixel_major_kernel<T>, grid, dim3(256), 0, (hipStream_t)stream,
                               (const T *)grad_out, (T *)workspace, C2, P);
        });
        HIP_TRY(hipGetLastError());
        return sweep_bwd_impl(desc, workspace, depths, cam2img, cam2img_inv, cur2prev, grad_cur, grad_prev, stream,
                              nullptr, false);
    }
    return sweep_bwd_impl(desc, grad_out, depths, cam2img, cam2img_inv, cur2prev, grad_cur, grad_prev, stream,
                          nullptr, true);
}

DFM_API int dfm_plane_sweep_bwd_last_kernel(void) { return g_last_bwd_kernel.load(); }

}  // extern "C"
