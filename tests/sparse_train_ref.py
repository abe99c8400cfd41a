"""What the sparse-training tests share: the fixture tests/golden/sparse_train*.npz (generator tests/golden/
make_golden_sparse_train.py), the state dicts of its cases, the comparison rule of tests/lidar_teacher_ref.py
(max |gpu - fp64| <= MARGIN x the stored fp32-vs-fp64 figure x max |fp64|) and, for the edge shapes, the dense masked
computation of one conv -> BatchNorm -> ReLU step under torch autograd on the CPU."""
import functools
import importlib.util
import os

import numpy as np
import torch
import torch.nn.functional as F

from tests.lidar_teacher_ref import MARGIN, linear_keys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
FILES = ('sparse_train.npz', 'sparse_train.layers.npz', 'sparse_train.enc_9_24_20.npz',
         'sparse_train.enc_11_25_19.npz')


@functools.lru_cache(maxsize=None)
def fixture():
    return np.load(os.path.join(GOLDEN, 'sparse_train.npz'))


@functools.lru_cache(maxsize=None)
def side(case):
    """the file of the large arrays (``dw.*``, ``grad_in``): 'layers' or an encoder case's name"""
    return np.load(os.path.join(GOLDEN, f'sparse_train.{case}.npz'))


@functools.lru_cache(maxsize=None)
def generator():
    spec = importlib.util.spec_from_file_location('make_golden_sparse_train',
                                                  os.path.join(GOLDEN, 'make_golden_sparse_train.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def state_dict(prefix):
    """the state dict of case ``prefix`` BEFORE the step, keys in the reference's order; the regenerated convolution
    weights are checked against the stored SHA-256"""
    z, gen = fixture(), generator().gen
    keys = [str(k) for k in z[f'{prefix}.keys']]
    shapes = [tuple(int(i) for i in str(s).split(',') if i) for s in z[f'{prefix}.shapes']]
    seed, sd, i = int(z[f'{prefix}.seed']), {}, 0
    for key, shape in zip(keys, shapes):
        if key.endswith('num_batches_tracked'):
            sd[key] = torch.zeros((), dtype=torch.int64)
        elif len(shape) == 5:
            w = gen.weights(seed + i, shape)
            assert gen.digest(w) == str(z[f'{prefix}.sha.{key}']), f'{prefix}.{key}: regenerated weights differ'
            sd[key], i = torch.from_numpy(w), i + 1
        else:
            sd[key] = torch.from_numpy(z[f'{prefix}.bn.{key}'])
        assert tuple(sd[key].shape) == shape
    return sd


def within(label, got, want, figure, worst=None):
    """max |got - want| <= MARGIN x figure x max |want|; prints the measured ratio (``worst``: a list it is added to)"""
    want = torch.as_tensor(want, dtype=torch.float64)
    got = got.detach().cpu().double().reshape(want.shape)
    scale = float(want.abs().max()) if want.numel() else 0.0
    err = float((got - want).abs().max()) if want.numel() else 0.0
    bar = MARGIN * float(figure) * scale
    ratio = err / bar if bar else 0.0
    print(f'{label}: max |gpu - fp64| = {err:.3e}, bar {bar:.3e} (figure {float(figure):.3e} x {MARGIN} x {scale:.3e}), '
          f'ratio {ratio:.3f}')
    if worst is not None:
        worst.append(ratio)
    assert torch.isfinite(got).all(), f'{label}: a non-finite value'
    if bar == 0.0:
        assert err == 0.0, f'{label}: an all-zero tensor must come out all zero'
    else:
        assert err <= bar, f'{label}: {err:.3e} > {bar:.3e}'


def rows_in_key_order(values, indices, shape):
    """the live rows of ``values`` in ascending (b, z, y, x) order, and their keys"""
    idx = indices.cpu()
    live = idx[:, 0] >= 0
    keys = linear_keys(idx[live], shape)
    order = torch.argsort(keys)
    return values.detach().cpu()[live][order], keys[order]


def compare_stage(z, name, tensor, worst=None):
    """a sparse tensor of this package against the stored stage ``name`` (``store_stage``): the active set exactly,
    zeros off it, the values within the rule"""
    shape = [int(s) for s in z[f'{name}.shape']]
    assert tensor.spatial_shape == shape
    got, keys = rows_in_key_order(tensor.features, tensor.indices, shape)
    want_keys = torch.from_numpy(z[f'{name}.keys'])
    assert keys.shape == want_keys.shape and torch.equal(keys, want_keys), f'{name}: active set differs'
    within(name, got, z[f'{name}.out'], z[f'{name}.err'], worst)


def check_dw(label, got, z, big, prefix, param, worst=None):
    """the gradient of convolution weight ``param``: in full, or as the stored projections"""
    gen = generator()
    if f'{prefix}.dw.{param}' in big:
        within(f'{label} dW', got, big[f'{prefix}.dw.{param}'], z[f'{prefix}.dw.{param}.err'], worst)
    else:
        within(f'{label} <dW, P_j>', gen.projections(got.detach().cpu()), z[f'{prefix}.proj.{param}'],
               z[f'{prefix}.proj.{param}.err'], worst)


def loss_weights(seed, shape):
    return torch.from_numpy(generator().gen.weights(int(seed), tuple(shape), bound=1))


# ----------------------------------------------------------------------------------------------------------------------
# the edge shapes' reference: conv -> BatchNorm (batch statistics over the active output sites) -> ReLU, dense and
# masked, under torch autograd on the CPU
# ----------------------------------------------------------------------------------------------------------------------
def dense_step(dtype, feats, coors, shape, batch, weight, gamma, beta, eps, stride, padding, subm, wl_seed):
    """-> dict(volume, pre, grad_in (rows of ``feats``, zeros on rows with b < 0), dw, dgamma, dbeta, mean, var
    (unbiased over max(n - 1, 1)), n); the loss is (volume x loss_weights(wl_seed)).sum()"""
    live = coors[:, 0] >= 0
    x = feats.to(dtype).clone().requires_grad_()
    w, g, b = (t.to(dtype).clone().requires_grad_() for t in (weight, gamma, beta))
    i = coors[live].long()
    vol = torch.zeros((batch, feats.shape[1], *shape), dtype=dtype)
    mask = torch.zeros((batch, 1, *shape), dtype=dtype)
    vol[i[:, 0], :, i[:, 1], i[:, 2], i[:, 3]] = x[live]
    mask[i[:, 0], 0, i[:, 1], i[:, 2], i[:, 3]] = 1
    if subm:
        stride, padding = 1, 1
    out = F.conv3d(vol, w.permute(4, 3, 0, 1, 2), stride=stride, padding=padding)
    omask = mask if subm else (F.conv3d(mask, torch.ones((1, 1, *weight.shape[:3]), dtype=dtype), stride=stride,
                                        padding=padding) > 0.5).to(dtype)
    o = omask[:, 0].nonzero()
    rows = out[o[:, 0], :, o[:, 1], o[:, 2], o[:, 3]]
    n = rows.shape[0]
    mean = rows.mean(0)
    var = ((rows - mean) ** 2).mean(0)
    pre = (rows - mean) / torch.sqrt(var + eps) * g + b
    volume = torch.zeros(out.shape, dtype=dtype)
    volume[o[:, 0], :, o[:, 1], o[:, 2], o[:, 3]] = torch.relu(pre)
    (volume * loss_weights(wl_seed, volume.shape).to(dtype)).sum().backward()
    return dict(volume=volume.detach(), pre=pre.detach(), grad_in=x.grad, dw=w.grad, dgamma=g.grad, dbeta=b.grad,
                mean=mean.detach(), var=(var * n / max(n - 1, 1)).detach(), n=n)


def figure(a32, a64):
    return generator().gen.figure(a32, a64)
