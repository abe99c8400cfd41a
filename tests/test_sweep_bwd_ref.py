"""The fp64 reference of the plane sweep's backward (tests/sweep_bwd_ref.py) against torch's CPU autograd through
``F.grid_sample`` (reference dfm_backbone.py:296-311) on the same fp32 grids, for every problem the GPU tests run
(tests/test_sweep_bwd_exact_gpu.py), and the input conditions of those problems -- from the reference alone, no GPU.

Bound.  torch's fp32 kernel computes each weight with at most three roundings (two fractions' complements and
their product), rounds ``g * w`` once and adds the n terms of an element one after the other (n - 1 roundings,
each relative to a partial sum of magnitude <= A = sum_k w_k |g_k|): |torch - ref| <= (n + 3) u A to first order,
u = 2^-24; asserted as (n + 4) u A, the fourth unit covering the second-order terms."""
import numpy as np
import pytest
import torch

from tests import sweep_bwd_ref as sr


def _torch_autograd(k, b, half, gout):
    C, H, W = k['C'], k['H'], k['W']
    grid = sr.grids(k, b)[half]
    f = torch.zeros(1, C, H, W, requires_grad=True)
    o = torch.nn.functional.grid_sample(f, torch.from_numpy(grid).view(1, 1, -1, 2), mode='bilinear',
                                        padding_mode='zeros', align_corners=True)
    o.backward(torch.from_numpy(gout[b:b + 1, half * C:(half + 1) * C].copy()).reshape(o.shape))
    return f.grad[0].numpy()


@pytest.mark.parametrize('name', sorted(sr.PROBLEMS))
def test_reference_agrees_with_torch_cpu_autograd(name):
    k = sr.problem(name)
    ref = sr.reference(name)      # (asserts the input conditions)
    worst = 0.0
    for b in range(k['B']):
        for half in (0, 1):
            got = _torch_autograd(k, b, half, k['gout']).astype(np.float64)
            assert np.isfinite(got).all()
            err = np.abs(got - ref['grad'][half, b])
            A, n = ref['A'][half, b], ref['n'][half, b][None]
            bound = (n + 4) * sr.U * A
            m = A > 0
            if m.any():
                worst = max(worst, float((err[m] / (sr.U * A[m])).max()))
            bad = err > bound
            assert not bad.any(), (f'{name} sample {b} map {half}: {int(bad.sum())} of {bad.size} beyond (n + 4) u A, '
                                   f'max err {err.max():.3g}')
            assert not got[np.broadcast_to(n == 0, got.shape)].any(), 'torch adds where the reference has no tap'
    print(f'\n{name}: torch vs fp64 reference, largest err / (u A) = {worst:.2f}')


@pytest.mark.parametrize('name', sorted(sr.PROBLEMS))
def test_input_conditions(name):
    """every problem, fp32 and bf16-rounded gradients: not empty, not all inside (asserted by the reference itself)"""
    k = sr.problem(name)
    for bf16 in (False, True):
        ref = sr.reference(name, bf16)
        covered = float((ref['n'][1] > 0).mean())
        print(f'\n{name}{" bf16" if bf16 else ""}: prev coverage {covered:.3f}, cur coverage '
              f'{float((ref["n"][0] > 0).mean()):.3f}, taps off the map (cur, prev) {tuple(int(v) for v in ref["oob"])}, '
              f'max |ref| (cur, prev) {np.abs(ref["grad"][0]).max():.3g}, {np.abs(ref["grad"][1]).max():.3g}, '
              f'max n {int(ref["n"].max())}')
        assert (covered == 0.0) == (k['geom'] == 'outside')


def test_every_geometry_case_is_run():
    assert {g for g, _ in sr.PROBLEMS.values()} >= set(sr.GEOMETRIES)


def test_positions_are_fp32_and_weights_fp64():
    """a position one ulp below an integer keeps its fp32 value: the east weight is 1 - 2^-24-ish, not 1"""
    x = np.array([np.nextafter(np.float32(3.0), np.float32(0.0))], np.float32)
    y = np.array([1.0], np.float32)
    grad, A, n, oob = sr.adjoint(x, y, np.ones((1, 1)), 4, 8)
    assert oob == 0 and int(n.sum()) == 4
    assert grad[0, 1, 2] == 3.0 - float(x[0]) and grad[0, 1, 3] == 1.0 - (3.0 - float(x[0]))
    # non-finite positions contribute nothing, a corner off the map keeps its in-bounds taps
    x = np.array([np.nan, np.inf, -0.25], np.float32)
    y = np.array([1.0, 1.0, 0.0], np.float32)
    grad, A, n, oob = sr.adjoint(x, y, np.ones((1, 3)), 4, 8)
    assert int(n.sum()) == 2 and oob == 2
    assert grad[0, 0, 0] == 0.75 and grad.sum() == 0.75
