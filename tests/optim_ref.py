"""The reference of the optimizer step for tests/test_optim.py and tests/test_optim_gpu.py: torch's own
``torch.nn.utils.clip_grad_norm_`` and ``torch.optim.AdamW(foreach=False)`` on the CPU, in fp64 or fp32, from a given
state; and the three error bounds both the kernels and torch's fp32 step are held to."""
import math

import torch

def bf16_ulp(x):
    """the spacing of bfloat16 (8 significant bits) at the normal number ``x``"""
    return 2.0 ** (math.floor(math.log2(abs(x))) - 7)


def reference_step(params, grads, states, hypers, max_norm, dtype=torch.float64, norm=None):
    """One clipped AdamW step by torch on the CPU in ``dtype``.

    ``params``: the fp32 values the update runs on (for a bf16 parameter: its master);  ``grads``: the gradient values
    as the step reads them;  ``states``: per tensor ``dict(step=t0, exp_avg=m0, exp_avg_sq=v0)``;  ``hypers``: per
    tensor ``dict(lr, betas, eps, weight_decay)`` (one parameter group each);  ``max_norm``: None for no clipping.
    ``norm`` given: the norm is TAKEN as that value instead of computed, so a caller that checks the norm on its own
    does not count its error a second time in the update.
    -> ``dict(p, m, v, u, g, norm, coef)``: lists of ``dtype`` tensors (``u``: the Adam update term
    step_size * m' / (sqrt(v') / bc2_sqrt + eps);  ``g``: the clipped gradients), the norm and the coefficient."""
    ps = [torch.nn.Parameter(p.detach().cpu().to(dtype).clone()) for p in params]
    for p, g in zip(ps, grads):
        p.grad = g.detach().cpu().to(dtype).clone()
    coef = 1.0
    if max_norm is not None and norm is None:
        norm = torch.nn.utils.clip_grad_norm_(ps, max_norm, norm_type=2.0, foreach=False)
        coef = torch.clamp(max_norm / (norm + 1e-6), max=1.0)
    elif max_norm is not None:
        norm = torch.as_tensor(norm).detach().cpu().to(dtype)
        coef = torch.clamp(max_norm / (norm + 1e-6), max=1.0)
        for p in ps:
            p.grad.mul_(coef)
    opt = torch.optim.AdamW([dict(params=[p], **h) for p, h in zip(ps, hypers)], foreach=False)
    for p, s in zip(ps, states):
        opt.state[p] = dict(step=torch.tensor(float(s['step']), dtype=torch.float32),
                            exp_avg=s['exp_avg'].detach().cpu().to(dtype).clone(),
                            exp_avg_sq=s['exp_avg_sq'].detach().cpu().to(dtype).clone())
    opt.step()
    out = dict(p=[p.detach() for p in ps], m=[opt.state[p]['exp_avg'] for p in ps],
               v=[opt.state[p]['exp_avg_sq'] for p in ps], g=[p.grad for p in ps], u=[], norm=norm, coef=coef)
    for p, s, h in zip(ps, states, hypers):
        t = float(s['step']) + 1
        beta1, beta2 = h['betas']
        step_size, bc2_sqrt = h['lr'] / (1 - beta1 ** t), (1 - beta2 ** t) ** 0.5
        st = opt.state[p]
        out['u'].append(step_size * st['exp_avg'] / (st['exp_avg_sq'].sqrt() / bc2_sqrt + h['eps']))
    return out


def bound_ratios(got_p, got_m, got_v, ref, m0, k):
    """the worst ratio of error to bound of tensor ``k`` for the parameter, ``exp_avg`` and ``exp_avg_sq`` (each <= 1
    passes):  |dp| <= 2^-22 |p'| + 2^-19 |u|;  |dm| <= 2^-21 (|m0| + |coef g|);  |dv| <= 2^-19 v'.
    Each is a handful of correctly rounded fp32 operations with a margin of at least two.  A 0 / 0 (an exact result
    against a zero bound) counts as 0; non-finite references are not this function's business."""
    f64 = torch.float64
    p, m, v = (t.detach().cpu().to(f64).reshape(-1) for t in (got_p, got_m, got_v))
    rp, rm, rv, ru, rg = (ref[n][k].to(f64).reshape(-1) for n in ('p', 'm', 'v', 'u', 'g'))
    m0 = m0.detach().cpu().to(f64).reshape(-1)

    def worst(err, bound):
        ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
        return float(ratio.max())
    return (worst((p - rp).abs(), 2.0 ** -22 * rp.abs() + 2.0 ** -19 * ru.abs()),
            worst((m - rm).abs(), 2.0 ** -21 * (m0.abs() + rg.abs())),
            worst((v - rv).abs(), 2.0 ** -19 * rv))
