"""GPU: the optimizer step's kernels (csrc/optim_step.hip) behind FusedAdamW and clip_grad_norm_, against torch's
CPU step in fp64 (tests/optim_ref.py) at the smallest shapes at which they can go wrong: sizes 1, 7 and one chunk + 1,
views at element offset 1 of their storage (fp32 and bf16), fp32 and bf16 parameters in one step, a parameter without
a gradient between two stepped ones, 3 and 40 tensors."""
import copy
import importlib
import math

import pytest
import torch

from tests import optim_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
F32, BF16 = torch.float32, torch.bfloat16


@pytest.fixture(scope='module')
def pkg():
    importlib.import_module('depth-from-motion_amd.build').build_hip()
    return importlib.import_module('depth-from-motion_amd')


@pytest.fixture(scope='module')
def optim(pkg):
    return importlib.import_module('depth-from-motion_amd.optim')


def specs(kind, chunk):
    """(numel, dtype, view at element offset 1, has a gradient, lr) per tensor"""
    if kind == 3:
        return [(1, F32, False, True, 1e-3), (7, F32, False, True, 1e-3), (chunk + 1, F32, False, True, 1e-3)]
    sizes = [1, 7, chunk + 1, 4099, 33, 8, 2 * chunk, 5, 260, 1031]
    out = []
    for i in range(40):                                     # one group per parameter, as mmcv's paramwise_cfg makes
        out.append((sizes[i % len(sizes)], BF16 if i % 2 else F32, i in (3, 13, 22), i != 10,
                    1e-3 * (0.1 if i % 3 == 0 else 1.0)))
    return out


class Case:
    """parameters, gradients and a given optimizer state (m0, v0, t0; masters with low bits a bf16 cannot hold), kept
    on the host as well for the reference"""

    def __init__(self, pkg, kind, t0=0, scale=1e-2, grad_clip=dict(max_norm=35., norm_type=2), seed=0, special=None,
                 zero_grad_values=False):
        chunk = pkg._capi.OPTIM_CHUNK
        gen = torch.Generator().manual_seed(seed)
        self.spec, self.t0, self.params, self.hyper = specs(kind, chunk), t0, [], []
        self.p32, self.g, self.m0, self.v0 = [], [], [], []
        groups = []
        for k, (n, dtype, offset, has_grad, lr) in enumerate(self.spec):
            master = torch.randn(n, generator=gen)
            grad = (scale * torch.randn(n, generator=gen)).to(dtype)
            if zero_grad_values:
                grad.zero_()
            if special is not None and k == special[0]:
                grad[special[1] % n] = special[2]
            store = torch.zeros(n + 1, dtype=dtype)
            store[1:] = master.to(dtype)
            store = store.to(DEV)
            p = torch.nn.Parameter(store[1:] if offset else store[1:].clone())
            assert (p.data_ptr() % 16 != 0) == offset
            p.grad = grad.to(DEV) if has_grad else None
            hyper = dict(lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4 if k % 2 else 1e-2)
            groups.append(dict(params=[p], **hyper))
            self.params.append(p)
            self.hyper.append(hyper)
            self.p32.append(master if dtype == BF16 else master.clone())
            self.g.append(grad.float())
            self.m0.append(0.3 * scale * torch.randn(n, generator=gen))
            self.v0.append((scale * torch.rand(n, generator=gen)) ** 2)
        self.opt = pkg.FusedAdamW(groups, grad_clip=grad_clip)
        for p, (n, dtype, _, _, _), w, m, v in zip(self.params, self.spec, self.p32, self.m0, self.v0):
            s = dict(step=torch.tensor(float(t0)), exp_avg=m.to(DEV), exp_avg_sq=v.to(DEV))
            if dtype == BF16:
                s['master'] = w.to(DEV)
            self.opt.state[p] = s
        self.stepped = [k for k, s in enumerate(self.spec) if s[3]]

    def masters(self):
        return [(self.opt.state[p]['master'] if p.dtype == BF16 else p.detach()).cpu() for p in self.params]

    def moments(self):
        return ([self.opt.state[p]['exp_avg'].cpu() for p in self.params],
                [self.opt.state[p]['exp_avg_sq'].cpu() for p in self.params])

    def reference(self, max_norm, dtype=torch.float64, norm=None):
        ks = self.stepped
        return R.reference_step([self.p32[k] for k in ks], [self.g[k] for k in ks],
                                [dict(step=self.t0, exp_avg=self.m0[k], exp_avg_sq=self.v0[k]) for k in ks],
                                [self.hyper[k] for k in ks], max_norm, dtype=dtype, norm=norm)

    def num_chunks(self, chunk):
        return sum(-(-self.spec[k][0] // chunk) for k in self.stepped)


def norm_bound(pkg, num_chunks):
    """(k + 1) 2^-25 with k the kernels' own summation depth: a lane adds at most CHUNK / THREADS body elements and one
    tail element, then 6 butterfly levels and the other waves in order -- for the chunk, and once more over the
    partials, of which a lane adds ceil(num_chunks / THREADS).  (k adds and one squaring on any path to the sum, each
    2^-24 relative on non-negative terms; the square root halves it.)"""
    threads, chunk = pkg._capi.OPTIM_THREADS, pkg._capi.OPTIM_CHUNK
    waves = threads // 64
    k = (chunk // threads + 1) + 6 + (waves - 1) + math.ceil(num_chunks / threads) + 6 + (waves - 1)
    bound = (k + 1) * 2.0 ** -25
    assert bound <= 2.0 ** -17
    return bound


def fp64_norm(case):
    return math.sqrt(sum(float((case.g[k].double() ** 2).sum()) for k in case.stepped))


# ---------------------------------------------------------------------------------------------------------
# one step from a given state
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('t0', [0, 1, 999])
@pytest.mark.parametrize('kind', [3, 40])
def test_one_step_against_fp64(pkg, optim, kind, t0):
    case = Case(pkg, kind, t0=t0)
    versions = [p._version for p in case.params]
    grads = [None if p.grad is None else p.grad.clone() for p in case.params]
    before = [p.detach().clone() for p in case.params]
    optim.counters(reset=True)
    assert case.opt.step() is None
    assert optim.counters() == {'kernel_launches': 2, 'copies': 1, 'host_waits': 0}
    norm = case.opt.grad_norm
    assert norm.is_cuda and norm.dtype == F32 and norm.dim() == 0
    want = fp64_norm(case)
    assert abs(float(norm) - want) <= norm_bound(pkg, case.num_chunks(pkg._capi.OPTIM_CHUNK)) * want
    ref = case.reference(35., norm=norm)
    masters, (ms, vs) = case.masters(), case.moments()
    for j, k in enumerate(case.stepped):
        ratios = R.bound_ratios(masters[k], ms[k], vs[k], ref, case.m0[k], j)
        assert max(ratios) <= 1.0, (k, case.spec[k], ratios)
        p = case.params[k]
        assert float(case.opt.state[p]['step']) == t0 + 1 and p._version > versions[k]
        assert torch.equal(p.grad, grads[k])                                     # the fused clip leaves .grad unscaled
        if p.dtype == BF16:
            assert torch.equal(p.detach(), case.opt.state[p]['master'].to(BF16))  # round to nearest even, bitwise
        assert not torch.equal(p.detach(), before[k]) or p.dtype == BF16
    for k in set(range(len(case.params))) - set(case.stepped):                     # grad=None between two stepped ones
        p = case.params[k]
        assert torch.equal(p.detach(), before[k]) and p._version == versions[k]
        assert float(case.opt.state[p]['step']) == t0
        assert torch.equal(case.opt.state[p]['exp_avg'].cpu(), case.m0[k])


def test_unclipped_step_is_one_launch(pkg, optim):
    case = Case(pkg, 40, t0=1, grad_clip=None)
    optim.counters(reset=True)
    case.opt.step()
    assert optim.counters() == {'kernel_launches': 1, 'copies': 1, 'host_waits': 0} and case.opt.grad_norm is None
    ref = case.reference(None)
    masters, (ms, vs) = case.masters(), case.moments()
    for j, k in enumerate(case.stepped):
        assert max(R.bound_ratios(masters[k], ms[k], vs[k], ref, case.m0[k], j)) <= 1.0, k


# ---------------------------------------------------------------------------------------------------------
# the norm
# ---------------------------------------------------------------------------------------------------------
def test_norm_below_max_norm_gives_a_coefficient_of_exactly_one(pkg):
    clipped, plain = Case(pkg, 40, t0=1), Case(pkg, 40, t0=1, grad_clip=None)
    clipped.opt.step()
    plain.opt.step()
    assert 0 < float(clipped.opt.grad_norm) < 35.0
    for a, b in zip(clipped.masters() + sum(clipped.moments(), []), plain.masters() + sum(plain.moments(), [])):
        assert torch.equal(a, b)


@pytest.mark.parametrize('scale, max_norm', [(30.0, 35.0), (1e-2, 1e-3)])
def test_norm_far_above_max_norm(pkg, scale, max_norm):
    case = Case(pkg, 40, t0=1, scale=scale, grad_clip=dict(max_norm=max_norm, norm_type=2))
    case.opt.step()
    want = fp64_norm(case)
    assert want > 100 * max_norm
    assert abs(float(case.opt.grad_norm) - want) <= norm_bound(pkg, case.num_chunks(pkg._capi.OPTIM_CHUNK)) * want
    ref = case.reference(max_norm, norm=case.opt.grad_norm)
    masters, (ms, vs) = case.masters(), case.moments()
    for j, k in enumerate(case.stepped):
        assert max(R.bound_ratios(masters[k], ms[k], vs[k], ref, case.m0[k], j)) <= 1.0, k


def test_all_zero_gradients(pkg):
    case = Case(pkg, 3, t0=1, zero_grad_values=True)
    case.opt.step()
    assert float(case.opt.grad_norm) == 0.0
    ref = case.reference(35., norm=case.opt.grad_norm)
    masters, (ms, vs) = case.masters(), case.moments()
    for j, k in enumerate(case.stepped):
        assert torch.isfinite(masters[k]).all()
        assert max(R.bound_ratios(masters[k], ms[k], vs[k], ref, case.m0[k], j)) <= 1.0, k


@pytest.mark.parametrize('value', [float('inf'), float('nan')])
def test_non_finite_gradients_propagate_as_in_torch(pkg, value):
    """error_if_nonfinite=False: an infinite norm gives coef = 0 and inf * 0 = NaN at that element only; a NaN norm
    spoils everything.  Positions against torch's own CPU step in fp32"""
    case = Case(pkg, 40, t0=1, special=(2, 4100, value))
    case.opt.step()
    ref = case.reference(35., dtype=F32)
    assert not math.isfinite(float(case.opt.grad_norm)) and not math.isfinite(float(ref['norm']))
    assert math.isnan(float(case.opt.grad_norm)) == math.isnan(float(ref['norm']))
    masters, (ms, vs) = case.masters(), case.moments()
    spoiled = 0
    for j, k in enumerate(case.stepped):
        for got, want in ((masters[k], ref['p'][j]), (ms[k], ref['m'][j]), (vs[k], ref['v'][j])):
            assert torch.equal(torch.isnan(got), torch.isnan(want)), k
            assert torch.equal(torch.isinf(got), torch.isinf(want)), k
        spoiled += int(torch.isnan(masters[k]).sum())
        p = case.params[k]
        if p.dtype == BF16:
            assert torch.equal(torch.isnan(p.detach().cpu()), torch.isnan(masters[k]))
    assert spoiled == (1 if math.isinf(value) else sum(case.spec[k][0] for k in case.stepped))


# ---------------------------------------------------------------------------------------------------------
# bf16: what the masters are for
# ---------------------------------------------------------------------------------------------------------
def test_a_bf16_parameter_moves_where_torchs_stalls(pkg):
    p = torch.nn.Parameter(torch.ones(1, dtype=BF16, device=DEV))
    opt = pkg.FusedAdamW([p], lr=1e-4, weight_decay=1e-4)
    ref = torch.nn.Parameter(torch.ones(1, dtype=torch.float64))
    ref_opt = torch.optim.AdamW([ref], lr=1e-4, weight_decay=1e-4)
    for _ in range(50):
        p.grad = torch.full((1,), 0.5, dtype=BF16, device=DEV)
        ref.grad = torch.full((1,), 0.5, dtype=torch.float64)
        opt.step()
        ref_opt.step()
    assert p.item() < 1.0                                          # tests/test_optim.py: torch's AdamW leaves 1.0
    want = ref.detach().to(BF16).double().item()
    assert abs(p.item() - want) <= R.bf16_ulp(want)
    assert torch.equal(p.detach(), opt.state[p]['master'].to(BF16))
    # per step: the decay 1 - 1e-8 rounds to 1.0f (1e-8 lost), and two roundings of half an ulp (2^-25) each below 1
    assert abs(opt.state[p]['master'].item() - ref.item()) <= 50 * (1e-8 + 2.0 ** -24)


# ---------------------------------------------------------------------------------------------------------
# stand-alone and fused clipping
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind, scale', [(3, 1e-2), (40, 30.0)])
def test_stand_alone_clip(pkg, optim, kind, scale):
    fused, alone = Case(pkg, kind, t0=1, scale=scale), Case(pkg, kind, t0=1, scale=scale)
    fused.opt.step()
    optim.counters(reset=True)
    norm = pkg.clip_grad_norm_(alone.params, 35., norm_type=2)
    assert optim.counters() == {'kernel_launches': 2, 'copies': 1, 'host_waits': 0}
    assert norm.is_cuda and torch.equal(norm, fused.opt.grad_norm)                 # the same partials, the same order
    coef = torch.clamp(35. / (norm.cpu() + 1e-6), max=1.0)                         # torch's own fp32 arithmetic
    assert (float(coef) == 1.0) == (scale < 1)
    for k in alone.stepped:
        p = alone.params[k]
        want = (fused.params[k].grad.cpu().float() * coef).to(p.dtype)             # fused: .grad untouched
        assert torch.equal(p.grad.cpu(), want), k
    one = torch.nn.Parameter(torch.zeros(3, device=DEV))                           # a single tensor, as torch takes it
    one.grad = torch.full((3,), 100.0, device=DEV)
    assert float(pkg.clip_grad_norm_(one, 1.0)) == pytest.approx(math.sqrt(3e4), rel=1e-6)
    assert float(one.grad.norm()) == pytest.approx(1.0, rel=1e-5)


def test_zero_grads_in_the_step(pkg):
    keep, zero = Case(pkg, 40, t0=1), Case(pkg, 40, t0=1)
    pointers = [None if p.grad is None else p.grad.data_ptr() for p in zero.params]
    grads = [p.grad for p in zero.params]
    keep.opt.step()
    zero.opt.step(zero_grads=True)
    for k, p in enumerate(zero.params):
        assert p.grad is grads[k]
        if p.grad is not None:
            assert p.grad.data_ptr() == pointers[k] and not p.grad.any()
    assert torch.equal(zero.opt.grad_norm, keep.opt.grad_norm)
    for a, b in zip(zero.masters() + sum(zero.moments(), []), keep.masters() + sum(keep.moments(), [])):
        assert torch.equal(a, b)


def test_two_runs_are_bitwise_equal(pkg):
    a, b = Case(pkg, 40, t0=999, scale=30.0), Case(pkg, 40, t0=999, scale=30.0)
    a.opt.step()
    b.opt.step()
    assert torch.equal(a.opt.grad_norm, b.opt.grad_norm)
    for x, y in zip(a.masters() + sum(a.moments(), []), b.masters() + sum(b.moments(), [])):
        assert torch.equal(x, y)
    for p, q in zip(a.params, b.params):
        assert torch.equal(p.detach(), q.detach())


# ---------------------------------------------------------------------------------------------------------
# the version contract
# ---------------------------------------------------------------------------------------------------------
def test_packed_weights_follow_the_step(pkg):
    conv3d = importlib.import_module('depth-from-motion_amd.conv3d')
    make = lambda: conv3d.MfmaConv3d(32, 32, 3, padding=1, bias=False).to(DEV).bfloat16()  # noqa: E731
    torch.manual_seed(0)
    conv = make()
    x = torch.randn(1, 32, 4, 8, 16).to(DEV, BF16).contiguous(memory_format=torch.channels_last_3d)
    assert conv.eligible(x)
    opt = pkg.FusedAdamW(conv.parameters(), lr=1e-2, weight_decay=1e-4, grad_clip=dict(max_norm=35., norm_type=2))
    y1 = conv(x)
    y1.float().square().mean().backward()
    version = conv.weight._version
    opt.step()
    assert conv.weight._version > version
    with torch.no_grad():
        y2 = conv(x)
        fresh = make()
        fresh.load_state_dict(conv.state_dict())
        want = fresh(x)
    assert not torch.equal(y1, y2), 'the step does not reach the output: the case checks nothing'
    assert torch.equal(y2, want)


# ---------------------------------------------------------------------------------------------------------
# resume
# ---------------------------------------------------------------------------------------------------------
def test_resume_from_a_state_dict(pkg):
    def run(steps, resume_at=None):
        case = Case(pkg, 40, t0=0, seed=5)
        for p in case.params:
            case.opt.state[p] = {}                                 # a fresh optimizer: the state comes from the steps
        gen = torch.Generator().manual_seed(7)
        grads = [[None if p.grad is None else (1e-2 * torch.randn(p.shape, generator=gen)).to(p.dtype).to(DEV)
                  for p in case.params] for _ in range(steps)]
        opt = case.opt
        for i in range(steps):
            if i == resume_at:
                saved = copy.deepcopy(opt.state_dict())
                opt = pkg.FusedAdamW([dict(params=[p]) for p in case.params], grad_clip=dict(max_norm=35., norm_type=2))
                opt.load_state_dict(saved)
            for p, g in zip(case.params, grads[i]):
                p.grad = g
            opt.step()
        return case.params, opt
    (ps, a), (qs, b) = run(5), run(5, resume_at=3)
    for p, q in zip(ps, qs):
        assert torch.equal(p.detach(), q.detach())
        assert list(a.state[p]) == list(b.state[q])
        for key in a.state[p]:
            assert torch.equal(a.state[p][key], b.state[q][key]), key
            assert a.state[p][key].dtype == F32
    assert torch.equal(a.grad_norm, b.grad_norm)
