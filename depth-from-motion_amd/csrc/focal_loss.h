// focal_loss.h -- the sigmoid focal term of one logit (mmdet's py_sigmoid_focal_loss in its
// binary_cross_entropy_with_logits form) and the sigmoid pair it is built from, as device functions shared by the
// kernels that sum it: csrc/anchor_loss.hip (the 3-D anchor head) and csrc/atss_loss.hip (the 2-D ATSS head), which
// must give the same bits per logit.  include/dfm_hip_anchor_loss.h states the formula.
#pragma once
#include "dfm_common.h"

namespace dfm {

// sigmoid(|z|) and sigmoid(-|z|) from e = exp(-|z|): no subtraction, finite for every finite z
__device__ __forceinline__ void sigmoid_pair(float e, float &big, float &small)
{
    big = __fdiv_rn(1.0f, 1.0f + e);
    small = e * big;
}

// the focal term of one logit; grad = d value / d x
template <bool GRAD>
__device__ __forceinline__ float focal(float x, bool t, float gamma, float alpha, float &grad)
{
    const float e = expf(-fabsf(x));
    float big, small;
    sigmoid_pair(e, big, small);
    const float p = x >= 0.0f ? big : small, q = x >= 0.0f ? small : big;     // sigmoid(x), 1 - sigmoid(x)
    const float pt = t ? q : p, one_minus_pt = t ? p : q;
    const float bce = (t ? fmaxf(-x, 0.0f) : fmaxf(x, 0.0f)) + log1pf(e);     // = max(x, 0) - x t + log1p(e)
    const float aw = t ? alpha : 1.0f - alpha;
    const float mod = gamma == 2.0f ? pt * pt : powf(pt, gamma);
    if constexpr (GRAD) grad = (t ? -aw : aw) * mod * (gamma * one_minus_pt * bce + pt);
    return aw * mod * bce;
}

}  // namespace dfm
