"""What the two deformable-convolution test files share: the fixture tests/golden/deform_conv.npz and the torch
stand-in of its generator (tests/golden/make_golden_deform_conv.py), run ONCE per process and case on the stored
inputs -- fp32 for the columns the kernels must reproduce bit for bit, fp64 for the expected values and gradients.
The results are cached and must not be modified."""
import functools
import importlib.util
import os

import numpy as np

from . import util


@functools.lru_cache(maxsize=None)
def generator():
    spec = importlib.util.spec_from_file_location('make_golden_deform_conv',
                                                  os.path.join(util.GOLDEN, 'make_golden_deform_conv.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def fixture():
    return np.load(os.path.join(util.GOLDEN, 'deform_conv.npz'))


def case_names():
    return tuple(generator().CASES)


def geometry(case):
    """dict(n, cin, cout, h, w, stride, padding, dilation, groups, raw, bias)"""
    keys = ('n', 'cin', 'cout', 'h', 'w', 'stride', 'padding', 'dilation', 'groups', 'raw', 'bias')
    return dict(zip(keys, generator().CASES[case]))


@functools.lru_cache(maxsize=None)
def inputs(case):
    """the stored inputs as fp32 CPU tensors: x, weight, grad_out, then offset and mask or raw, and bias if any"""
    return generator().load_inputs(fixture(), case)


@functools.lru_cache(maxsize=None)
def reference(case):
    """(fp32 run, fp64 run) of the stand-in: dicts of col, out, grad_x, grad_weight, grad_offset, grad_mask[,
    grad_bias]"""
    import torch
    g = generator()
    return g.run(case, inputs(case), torch.float32), g.run(case, inputs(case), torch.float64)


def error_figure(case, quantity):
    """the stored fp32-vs-fp64 error of the stand-in for ``quantity``, relative to the quantity's largest magnitude"""
    return float(fixture()[f'{case}.err'][generator().QUANTITIES.index(quantity)])
