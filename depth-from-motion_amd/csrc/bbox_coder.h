// bbox_coder.h -- DeltaXYZWLHRBBoxCoder.decode (core/bbox/coders/delta_xyzwhlr_bbox_coder.py:58-91) and what the
// anchor head derives from a decoded box, as device functions shared by every kernel that decodes
// (csrc/bbox_decode.hip: the head's candidates and the standalone decode, which must give the same bits).
//
// FP32, the reference's operations in its order, one IEEE rounding each (the translation units are compiled
// with -ffp-contract=off; division and square root are written as the correctly rounded intrinsics).
#pragma once
#include "dfm_common.h"

namespace dfm {

constexpr int BBOX_CODE_MIN = 7, BBOX_CODE_MAX = 16;

// anchor (xa, ya, za, wa, la, ha, ra, extras...) and deltas (xt, yt, zt, wt, lt, ht, rt, extras...) -> box;
// the columns beyond 7 are t + a
__device__ __forceinline__ void delta_xyzwlhr_decode_row(const float *an, const float *t, int width, float *out)
{
    const float xa = an[0], ya = an[1], wa = an[3], la = an[4], ha = an[5], ra = an[6];
    const float za = __fadd_rn(an[2], __fdiv_rn(ha, 2.0f));
    const float diagonal = __fsqrt_rn(__fadd_rn(__fmul_rn(la, la), __fmul_rn(wa, wa)));
    const float xg = __fadd_rn(__fmul_rn(t[0], diagonal), xa);
    const float yg = __fadd_rn(__fmul_rn(t[1], diagonal), ya);
    const float zg = __fadd_rn(__fmul_rn(t[2], ha), za);
    const float lg = __fmul_rn(expf(t[4]), la);
    const float wg = __fmul_rn(expf(t[3]), wa);
    const float hg = __fmul_rn(expf(t[5]), ha);
    out[0] = xg;
    out[1] = yg;
    out[2] = __fsub_rn(zg, __fdiv_rn(hg, 2.0f));
    out[3] = wg;
    out[4] = lg;
    out[5] = hg;
    out[6] = __fadd_rn(t[6], ra);
#pragma unroll
    for (int c = 7; c < BBOX_CODE_MAX; ++c)
        if (c < width) out[c] = __fadd_rn(t[c], an[c]);
}

// xywhr2xyxyr (core/bbox/structures/utils.py:121-139) of BaseInstance3DBoxes.bev = columns (0, 1, 3, 4, 6)
__device__ __forceinline__ void bev_xyxyr(const float *box, float *out)
{
    const float half_w = __fdiv_rn(box[3], 2.0f), half_h = __fdiv_rn(box[4], 2.0f);
    out[0] = __fsub_rn(box[0], half_w);
    out[1] = __fsub_rn(box[1], half_h);
    out[2] = __fadd_rn(box[0], half_w);
    out[3] = __fadd_rn(box[1], half_h);
    out[4] = box[6];
}

// torch.sigmoid in FP32: 1 / (1 + exp(-x)); 0 at -inf, 1 at +inf, NaN stays NaN
__device__ __forceinline__ float sigmoid_f32(float x)
{
    return __fdiv_rn(1.0f, __fadd_rn(1.0f, expf(-x)));
}

}  // namespace dfm
