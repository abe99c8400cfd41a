"""CPU: the host side of the optimizer step (depth-from-motion_amd/optim.py) -- construction and refused arguments,
the state and its interchange with torch.optim.AdamW, the multi-tensor table and its scalars -- and the two facts the
GPU tests lean on: torch's own AdamW stalls on a bf16 parameter, and torch's fp32 CPU step meets the error bounds the
kernels are held to (tests/optim_ref.py)."""
import copy
import importlib
import itertools
import sys
import types

import numpy as np
import pytest
import torch

from tests import optim_ref as R


@pytest.fixture(scope='module')
def pkg():
    importlib.import_module('depth-from-motion_amd.build').build_hip()
    return importlib.import_module('depth-from-motion_amd')


@pytest.fixture(scope='module')
def optim(pkg):
    return importlib.import_module('depth-from-motion_amd.optim')


def params(*shapes, dtype=torch.float32, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, generator=g).to(dtype)) for s in shapes]


def give_grads(ps, seed=1, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    for p in ps:
        p.grad = (scale * torch.randn(p.shape, generator=g)).to(p.dtype)


# ---------------------------------------------------------------------------------------------------------
# construction
# ---------------------------------------------------------------------------------------------------------
def test_exported_and_is_an_optimizer(pkg, optim):
    assert pkg.FusedAdamW is optim.FusedAdamW and pkg.clip_grad_norm_ is optim.clip_grad_norm_
    assert issubclass(pkg.FusedAdamW, torch.optim.Optimizer)
    assert optim.counters() == {'kernel_launches': 0, 'copies': 0, 'host_waits': 0}
    opt = pkg.FusedAdamW(params((3,)), lr=1e-3, weight_decay=1e-4, grad_clip=dict(max_norm=35., norm_type=2))
    assert opt.max_norm == 35.0 and opt.grad_norm is None and opt.master_weights
    g = opt.param_groups[0]
    assert (g['lr'], g['betas'], g['eps'], g['weight_decay']) == (1e-3, (0.9, 0.999), 1e-8, 1e-4)


def test_groups_and_lr_hooks(pkg):
    a, b, c = params((2, 3), (4,), (5,))
    opt = pkg.FusedAdamW([dict(params=[a], lr=1e-4, weight_decay=0.0), dict(params=[b])], lr=1e-3)   # paramwise_cfg
    assert [g['lr'] for g in opt.param_groups] == [1e-4, 1e-3]
    assert [g['weight_decay'] for g in opt.param_groups] == [0.0, 1e-2]
    opt.add_param_group(dict(params=[c], lr=5e-4))
    assert len(opt.param_groups) == 3 and opt.param_groups[2]['betas'] == (0.9, 0.999)
    for g in opt.param_groups:                  # what an LR updater hook does
        g['lr'] = g['lr'] * 0.5
    give_grads([a, b, c])
    entries = opt._prepare(on_gpu=False)
    assert [np.float32(e[3][1]) for e in entries] == [np.float32(lr / (1 - 0.9)) for lr in (5e-5, 5e-4, 2.5e-4)]
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.1)       # torch's schedulers accept it
    assert sched.get_last_lr() == [5e-5, 5e-4, 2.5e-4]


@pytest.mark.parametrize('kwargs', [
    dict(amsgrad=True), dict(maximize=True), dict(capturable=True), dict(differentiable=True),
    dict(grad_clip=dict(max_norm=35., norm_type=1)), dict(grad_clip=dict(max_norm=35., norm_type=float('inf'))),
    dict(grad_clip=dict(max_norm=35., error_if_nonfinite=True)), dict(grad_clip=dict(norm_type=2)),
    dict(grad_clip=dict(max_norm=1., clip_value=2.)), dict(lr=-1.0), dict(betas=(1.0, 0.9)), dict(eps=-1e-8),
    dict(weight_decay=-1.0)])
def test_refused_arguments(pkg, kwargs):
    with pytest.raises(ValueError):
        pkg.FusedAdamW(params((3,)), **kwargs)


def test_refused_types_and_layouts(pkg):
    with pytest.raises(TypeError, match='float32 and bfloat16'):
        pkg.FusedAdamW(params((3,), dtype=torch.float16))
    with pytest.raises(TypeError, match='unexpected'):
        pkg.FusedAdamW(params((3,)), momentum=0.9)
    pkg.FusedAdamW(params((3,)), amsgrad=False, foreach=None, fused=None)          # torch's spellings of "off" pass
    with pytest.raises(ValueError, match='norm_type=2'):
        pkg.clip_grad_norm_(params((3,)), 35., norm_type=1)
    with pytest.raises(ValueError, match='error_if_nonfinite'):
        pkg.clip_grad_norm_(params((3,)), 35., error_if_nonfinite=True)
    assert float(pkg.clip_grad_norm_(params((3,)), 35.)) == 0.0                   # no gradients: torch's tensor(0.)
    p = torch.nn.Parameter(torch.zeros(4, 6)[:, ::2])                              # strided with gaps: not dense
    p.grad = torch.ones(4, 3)
    opt = pkg.FusedAdamW([p])
    with pytest.raises(ValueError, match='not dense'):
        opt._prepare(on_gpu=False)
    assert opt.state[p] == {}                                                      # nothing changed before the raise


def test_cpu_parameters_raise_at_step_not_at_construction(pkg):
    ps = params((3,), (4,))
    opt = pkg.FusedAdamW(ps, grad_clip=dict(max_norm=35., norm_type=2))
    opt.step()                                                                     # no gradient: nothing to do
    give_grads(ps)
    with pytest.raises(RuntimeError, match='no CPU path'):
        opt.step()
    assert all(opt.state[p] == {} for p in ps)
    with pytest.raises(RuntimeError, match='no CPU path'):
        pkg.clip_grad_norm_(ps, 35.)
    with pytest.raises(ValueError, match='closure'):
        opt.step(lambda: 0.0)


def test_dtype_changed_after_construction(pkg):
    (p,) = params((4, 4))
    opt = pkg.FusedAdamW([p])
    p.data = p.data.to(torch.bfloat16)                                             # what enable_fast_path does
    p.grad = torch.ones_like(p)
    with pytest.raises(RuntimeError, match='build the optimizer after enable_fast_path'):
        opt._prepare(on_gpu=False)


# ---------------------------------------------------------------------------------------------------------
# the table and its scalars
# ---------------------------------------------------------------------------------------------------------
def torch_scalars(lr, beta1, beta2, eps, weight_decay, step):
    """torch/optim/adam.py _single_tensor_adam and adamw's ``param.mul_(1 - lr * weight_decay)``, in double"""
    bias_correction1 = 1 - beta1 ** step
    bias_correction2 = 1 - beta2 ** step
    step_size = lr / bias_correction1
    bias_correction2_sqrt = bias_correction2 ** 0.5
    return dict(decay=1 - lr * weight_decay, step_size=step_size, bc2_sqrt=bias_correction2_sqrt,
                lerp_weight=1 - beta1, beta2=beta2, one_minus_beta2=1 - beta2, eps=eps)


@pytest.mark.parametrize('t', [1, 2, 1000, 100000])
def test_table_scalars_are_torchs_doubles_rounded_once(pkg, optim, t):
    a, b = params((5,), (2, 3))
    opt = pkg.FusedAdamW([dict(params=[a], lr=5e-4 * 0.1, weight_decay=1e-4), dict(params=[b], betas=(0.8, 0.99))],
                         lr=1e-3, weight_decay=1e-2, eps=1e-8)
    give_grads([a, b])
    opt._prepare(on_gpu=False)
    for p in (a, b):
        opt.state[p]['step'].fill_(t - 1)
    entries = opt._prepare(on_gpu=False)
    table = optim.build_table(entries)
    assert table.dtype.itemsize == 88 and len(table) == 2
    for row, p, hyper in zip(table, (a, b), ((5e-5, 0.9, 0.999, 1e-8, 1e-4), (1e-3, 0.8, 0.99, 1e-8, 1e-2))):
        assert float(opt.state[p]['step']) == t
        for name, value in torch_scalars(*hyper, float(t)).items():
            assert row[name] == np.float32(value), (name, row[name], value)       # the double, rounded once
        s = opt.state[p]
        assert (row['param'], row['grad'], row['exp_avg'], row['exp_avg_sq'], row['master'], row['numel']) == \
            (p.data_ptr(), p.grad.data_ptr(), s['exp_avg'].data_ptr(), s['exp_avg_sq'].data_ptr(), 0, p.numel())
        assert row['dtype'] == pkg._capi.DFM_F32
    if t == 100000:         # where a float32 power would be off: 1 - 0.999^t is 1 in either, beta1^t underflows
        assert table[0]['step_size'] == np.float32(5e-5) and table[0]['bc2_sqrt'] == np.float32(1.0)


def test_parameters_without_gradient_are_absent_and_keep_their_step(pkg, optim):
    a, b, c = params((3,), (4,), (5,), dtype=torch.bfloat16)
    opt = pkg.FusedAdamW([a, b, c])
    give_grads([a, b, c])
    opt._prepare(on_gpu=False)
    b.grad = None
    entries = opt._prepare(on_gpu=False)
    table = optim.build_table(entries)
    assert [e[0] is p for e, p in zip(entries, (a, c))] == [True, True] and len(table) == 2
    assert [float(opt.state[p]['step']) for p in (a, b, c)] == [2.0, 1.0, 2.0]
    assert list(table['numel']) == [3, 5] and list(table['dtype']) == [pkg._capi.DFM_BF16] * 2
    assert list(table['master']) == [opt.state[p]['master'].data_ptr() for p in (a, c)]
    assert table[0]['step_size'] == np.float32(1e-3 / (1 - 0.9 ** 2))
    # without masters the row says so
    opt = pkg.FusedAdamW([a], master_weights=False)
    assert optim.build_table(opt._prepare(on_gpu=False))['master'][0] == 0 and 'master' not in opt.state[a]
    # the rows of the norm / scale kernels: gradient, count and type only
    rows = optim.build_table([(None, a.grad, None, None)])
    assert (rows['grad'][0], rows['numel'][0], rows['param'][0], rows['step_size'][0]) == (a.grad.data_ptr(), 3, 0, 0)


def test_chunk_table(pkg, optim):
    C = pkg._capi.OPTIM_CHUNK
    assert (C, pkg._capi.OPTIM_THREADS) == (8192, 256) and C % (8 * 256) == 0
    chunks = optim.chunk_table([1, C, C + 1, 0, 3 * C - 1])
    assert chunks.dtype == np.int32 and chunks.tolist() == [[0, 0], [1, 0], [2, 0], [2, 1], [4, 0], [4, 1], [4, 2]]
    assert optim.chunk_table([]).shape == (0, 2)


def test_state_layout_follows_the_parameter(pkg):
    p = torch.nn.Parameter(torch.randn(4, 6, 2, 3, 5).to(memory_format=torch.channels_last_3d).to(torch.bfloat16))
    view = torch.nn.Parameter(torch.randn(10)[1:8])                                # element offset 1 of its storage
    p.grad, view.grad = torch.ones(4, 6, 2, 3, 5, dtype=torch.bfloat16), torch.ones(7)
    opt = pkg.FusedAdamW([p, view])
    grad_before = p.grad
    opt._prepare(on_gpu=False)
    assert p.grad is not grad_before and p.grad.stride() == p.stride() and torch.equal(p.grad, grad_before)
    s = opt.state[p]
    assert all(s[k].stride() == p.stride() and s[k].dtype == torch.float32 for k in ('exp_avg', 'exp_avg_sq', 'master'))
    assert torch.equal(s['master'], p.detach().float()) and list(s) == ['step', 'exp_avg', 'exp_avg_sq', 'master']
    assert view.data_ptr() % 16 == 4 and list(opt.state[view]) == ['step', 'exp_avg', 'exp_avg_sq']
    assert s['step'].device.type == 'cpu' and s['step'].dtype == torch.float32 and s['step'].dim() == 0


# ---------------------------------------------------------------------------------------------------------
# state_dict
# ---------------------------------------------------------------------------------------------------------
def filled(opt, ps, seed=3):
    """a state as after some steps, without a GPU: the host side of a step, then random moments"""
    give_grads(ps)
    opt._prepare(on_gpu=False)
    g = torch.Generator().manual_seed(seed)
    for p in ps:
        s = opt.state[p]
        s['step'].fill_(7)
        s['exp_avg'].copy_(torch.randn(p.shape, generator=g) * 1e-3)
        s['exp_avg_sq'].copy_(torch.rand(p.shape, generator=g) * 1e-5)
        if 'master' in s:
            s['master'].add_(torch.randn(p.shape, generator=g) * 1e-4)     # low bits a bf16 cast would lose
    return opt


def test_state_dict_interchange_with_torch_adamw_fp32(pkg):
    ps = params((3, 2), (5,))
    ours = filled(pkg.FusedAdamW([dict(params=[ps[0]], lr=1e-4), dict(params=[ps[1]])], lr=1e-3, weight_decay=1e-4), ps)
    sd = ours.state_dict()
    qs = params((3, 2), (5,), seed=9)
    theirs = torch.optim.AdamW([dict(params=[qs[0]], lr=1.0), dict(params=[qs[1]])], lr=1.0, foreach=False)
    theirs.load_state_dict(copy.deepcopy(sd))                                      # ours -> torch
    assert [g['lr'] for g in theirs.param_groups] == [1e-4, 1e-3]
    for p, q in zip(ps, qs):
        assert list(theirs.state[q]) == list(ours.state[p]) == ['step', 'exp_avg', 'exp_avg_sq']
        assert all(torch.equal(theirs.state[q][k], ours.state[p][k]) for k in ours.state[p])
    give_grads(qs)
    theirs.step()                                                                  # and torch steps from it
    assert float(theirs.state[qs[0]]['step']) == 8.0
    back = pkg.FusedAdamW([dict(params=[ps[0]]), dict(params=[ps[1]])], lr=1.0)
    back.load_state_dict(copy.deepcopy(theirs.state_dict()))                       # torch -> ours
    for p, q in zip(ps, qs):
        assert list(back.state[p]) == ['step', 'exp_avg', 'exp_avg_sq']
        assert all(torch.equal(back.state[p][k], theirs.state[q][k]) for k in back.state[p])
        assert back.state[p]['step'].device.type == 'cpu' and back.state[p]['exp_avg'].dtype == torch.float32
    assert [g['lr'] for g in back.param_groups] == [1e-4, 1e-3]
    assert set(sd['param_groups'][0]) == set(theirs.state_dict()['param_groups'][0])   # group keys too


def test_state_dict_round_trip_keeps_bf16_state_in_fp32(pkg):
    ps = params((4, 3), (7,), dtype=torch.bfloat16)
    ours = filled(pkg.FusedAdamW(ps), ps)
    sd = copy.deepcopy(ours.state_dict())
    fresh = pkg.FusedAdamW(params((4, 3), (7,), dtype=torch.bfloat16, seed=5))
    fresh.load_state_dict(sd)
    for p, q in zip(ps, fresh.param_groups[0]['params']):
        a, b = ours.state[p], fresh.state[q]
        assert list(b) == ['step', 'exp_avg', 'exp_avg_sq', 'master']
        for k in ('exp_avg', 'exp_avg_sq', 'master'):
            assert b[k].dtype == torch.float32 and torch.equal(a[k], b[k]), k
            assert not torch.equal(a[k], a[k].bfloat16().float())                  # the cast torch makes would show
        assert float(b['step']) == 7.0
    # torch's own load, for contrast, rounds them: this is what the override is for
    plain = torch.optim.AdamW(params((4, 3), (7,), dtype=torch.bfloat16), foreach=False)
    plain.load_state_dict(copy.deepcopy(sd))
    assert plain.state[plain.param_groups[0]['params'][0]]['exp_avg'].dtype == torch.bfloat16


def test_a_torch_bf16_state_loads(pkg):
    qs = params((4, 3), (7,), dtype=torch.bfloat16)
    theirs = torch.optim.AdamW(qs, lr=1e-3, foreach=False)
    give_grads(qs)
    theirs.step()
    theirs.step()
    assert theirs.state[qs[0]]['exp_avg'].dtype == torch.bfloat16
    ps = params((4, 3), (7,), dtype=torch.bfloat16, seed=4)
    ours = pkg.FusedAdamW(ps)
    ours.load_state_dict(copy.deepcopy(theirs.state_dict()))
    for p, q in zip(ps, qs):
        s = ours.state[p]
        assert list(s) == ['step', 'exp_avg', 'exp_avg_sq', 'master'] and float(s['step']) == 2.0
        assert s['exp_avg'].dtype == s['exp_avg_sq'].dtype == s['master'].dtype == torch.float32
        assert torch.equal(s['exp_avg'], theirs.state[q]['exp_avg'].float())
        assert torch.equal(s['exp_avg_sq'], theirs.state[q]['exp_avg_sq'].float())
        assert torch.equal(s['master'], p.detach().float())                        # the master: from the parameter
    part = copy.deepcopy(theirs.state_dict())                                   # a parameter that never had a gradient
    del part['state'][1]
    ours = pkg.FusedAdamW(ps)
    ours.load_state_dict(part)
    give_grads(ps)
    ours._prepare(on_gpu=False)                                                    # gets its state at its first step
    assert [float(ours.state[p]['step']) for p in ps] == [3.0, 1.0]
    with pytest.raises(ValueError, match='different number of parameter groups'):
        pkg.FusedAdamW([dict(params=[ps[0]]), dict(params=[ps[1]])]).load_state_dict(theirs.state_dict())
    bad = copy.deepcopy(theirs.state_dict())
    bad['param_groups'][0]['amsgrad'] = True
    with pytest.raises(ValueError, match='amsgrad'):
        pkg.FusedAdamW(params((4, 3), (7,), dtype=torch.bfloat16)).load_state_dict(bad)


# ---------------------------------------------------------------------------------------------------------
# what the feature is for, and what its bounds are worth
# ---------------------------------------------------------------------------------------------------------
def test_torch_adamw_stalls_on_a_bf16_parameter():
    p = torch.nn.Parameter(torch.ones(1, dtype=torch.bfloat16))
    opt = torch.optim.AdamW([p], lr=1e-4, weight_decay=1e-4)
    for _ in range(50):
        p.grad = torch.full((1,), 0.5, dtype=torch.bfloat16)
        opt.step()
    assert p.item() == 1.0                   # every update was below half a bf16 ulp (2^-9 at 1.0) and rounded away
    ref = torch.nn.Parameter(torch.ones(1, dtype=torch.float64))
    opt = torch.optim.AdamW([ref], lr=1e-4, weight_decay=1e-4)
    for _ in range(50):
        ref.grad = torch.full((1,), 0.5, dtype=torch.float64)
        opt.step()
    assert ref.item() < 1.0 - 2.0 ** -9      # while the true trajectory has moved by more than a bf16 ulp


def test_torchs_fp32_step_meets_the_bounds():
    """the three bounds of tests/optim_ref.bound_ratios, which tests/test_optim_gpu.py holds the kernels to, hold for
    torch's own fp32 CPU step against its fp64 one (fed the fp32 norm) with a margin of two: worst ratios printed"""
    worst = [0.0, 0.0, 0.0]
    gen = torch.Generator().manual_seed(11)
    hyper = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4)
    for t, scale, max_norm in itertools.product((1, 2, 1000, 100001), (1e-6, 1e-2, 30.0), (35.0, 1e-3)):
        sizes = (1, 7, 4099)
        ps = [torch.randn(n, generator=gen) for n in sizes]
        gs = [scale * torch.randn(n, generator=gen) for n in sizes]
        states = [dict(step=t - 1, exp_avg=0.3 * scale * torch.randn(n, generator=gen),
                       exp_avg_sq=(scale * torch.rand(n, generator=gen)) ** 2) for n in sizes]
        lo = R.reference_step(ps, gs, states, [hyper] * 3, max_norm, dtype=torch.float32)
        hi = R.reference_step(ps, gs, states, [hyper] * 3, max_norm, dtype=torch.float64, norm=lo['norm'])
        for k in range(3):
            ratios = R.bound_ratios(lo['p'][k], lo['m'][k], lo['v'][k], hi, states[k]['exp_avg'], k)
            worst = [max(a, b) for a, b in zip(worst, ratios)]
    print('worst ratio to the bound (parameter, exp_avg, exp_avg_sq):', worst)
    assert max(worst) <= 0.5, worst


# ---------------------------------------------------------------------------------------------------------
# integration
# ---------------------------------------------------------------------------------------------------------
def test_patch_optimizer_registers_and_rebinds(pkg, monkeypatch):
    integration = importlib.import_module('depth-from-motion_amd.integration')
    for name in [n for n in sys.modules if n == 'mmcv' or n.startswith('mmcv.')]:
        monkeypatch.delitem(sys.modules, name)
    nothing = {'modules': [], 'functions': [], 'methods': []}
    assert integration.apply_patches('optimizer') == nothing                      # without mmcv: nothing

    class Registry:
        def __init__(self):
            self.modules = {}

        def register_module(self, name=None, force=False, module=None):
            assert force
            self.modules[name] = module

    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__path__ = []
        vars(m).update(attrs)
        monkeypatch.setitem(sys.modules, name, m)
        return m
    reg = Registry()
    torch_clip = torch.nn.utils.clip_grad.clip_grad_norm_
    mod('mmcv'), mod('mmcv.runner'), mod('mmcv.runner.hooks')
    mod('mmcv.runner.optimizer', OPTIMIZERS=reg)
    hooks = mod('mmcv.runner.hooks.optimizer', clip_grad=torch.nn.utils.clip_grad)
    done = integration.apply_patches('optimizer')
    assert done == dict(nothing, modules=['FusedAdamW (mmcv OPTIMIZERS)'],
                        functions=['mmcv.runner.hooks.optimizer.clip_grad.clip_grad_norm_'])
    assert reg.modules == {'FusedAdamW': pkg.FusedAdamW}
    assert hooks.clip_grad.clip_grad_norm_ is pkg.clip_grad_norm_                # as OptimizerHook.clip_grads calls it
    assert torch.nn.utils.clip_grad.clip_grad_norm_ is torch_clip                  # torch itself is left alone
    # mmcv's constructor builds it as OPTIMIZERS.build(dict(type=..., params=[...], **the config's optimizer dict))
    opt = reg.modules['FusedAdamW'](params=[dict(params=params((3,)), lr=5e-5)], lr=0.0005, weight_decay=0.0001,
                                    grad_clip=dict(max_norm=35., norm_type=2))
    assert opt.param_groups[0]['lr'] == 5e-5 and opt.max_norm == 35.0
