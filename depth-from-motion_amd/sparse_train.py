"""Training the LiDAR teacher's sparse encoder on the HIP path (include/dfm_hip_sparse_train.h): opt-in, fp32, one rank.

``enable_sparse_training(module)`` marks every ``SubMConv3d``, ``SparseConv3d`` and ``SparseSequential`` of a tree.  A
marked layer in training mode runs under autograd:

* the convolution without an epilogue (``dfm_sparse_conv_fwd``); its input gradient is the same kernel over the
  inverse neighbour table with the per-offset transposed weight (Cin in {16, 32, 64}; any other Cin has no input
  gradient and raises when one is required); its weight gradient is ``dfm_sparse_conv_wgrad``;
* ``BatchNorm1d`` in training mode over the live rows, fused with the ReLU that follows (the ReLU mask is recomputed
  from x in the backward), running statistics updated on the device;
* ``dense()`` with a backward that gathers the volume's gradient at the live coordinates.

Every gradient handed back to autograd is exactly 0 on rows with ``b < 0``, whatever those rows hold.  No host wait in
forward or backward.  What this does not cover raises ``MfmaPathError`` naming the setting, under every fallback
policy: eval mode with an input or a weight that needs a gradient (frozen-BN fine-tuning), a dtype other than fp32, a
``SyncBN`` in a process group of more than one rank (the statistics kernel emits the ``(C, 3)`` ``(count, mean, M2)``
payload that group_norm.py exchanges between ranks, so that is an addition above the kernels), ``momentum=None``.
"""
import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import _capi
from ._launch import STREAM, WS, launch
from .fallback import MfmaPathError
from .sparse_conv import SparseSequential, _SparseConvBase, _size3

__all__ = ['enable_sparse_training']

_GRAD_IN_CHANNELS = (16, 32, 64)   # the forward kernel's Cout: the input gradient is that kernel with Cin as its Cout


def enable_sparse_training(module, enabled=True):
    """Mark (``enabled=False``: unmark) every ``SubMConv3d``, ``SparseConv3d`` and ``SparseSequential`` inside
    ``module`` for training; returns their names.  Unmarked modules refuse training mode as before; a ``LidarTeacher``
    stays frozen whatever its layers are marked as (it forces eval mode and builds no gradient)."""
    names = []
    for name, m in module.named_modules():
        if isinstance(m, (_SparseConvBase, SparseSequential)):
            m.sparse_training = bool(enabled)
            names.append(name)
    return names


def _refuse(who, why):
    raise MfmaPathError(f'{who}: {why} -- not covered by the sparse-training kernels (enable_sparse_training), and '
                        'there is no torch path behind them')


class _ConvFn(torch.autograd.Function):
    """out = conv(features) (+ bias); the tables are those of the forward, ``inverse`` builds the inverse one"""

    @staticmethod
    def forward(ctx, features, weight, bias, conv, nbr, in_indices, out_indices, inverse, live_rows):
        cin, cout = conv.in_channels, conv.out_channels
        taps = conv.kernel_size[0] * conv.kernel_size[1] * conv.kernel_size[2]
        out_rows = out_indices.shape[0]
        out = torch.zeros((out_rows, cout), dtype=torch.float32, device=features.device)
        scale = shift = None
        if bias is not None:
            scale, shift = torch.ones_like(bias), bias.contiguous()
        launch('dfm_sparse_conv_fwd', cin, cout, taps, features, features.shape[0], nbr, out_indices, out_rows, weight,
               scale, shift, 0, out, STREAM)
        ctx.save_for_backward(features, weight)
        ctx.geometry = (cin, cout, taps, bias is not None)
        ctx.nbr, ctx.in_indices, ctx.out_indices, ctx.live_rows = nbr, in_indices, out_indices, live_rows
        # the inverse table is made now, on the forward's stream order, when the backward will need it
        ctx.inv = inverse() if (ctx.needs_input_grad[0] and nbr is not None) else None
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        features, weight = ctx.saved_tensors
        cin, cout, taps, has_bias = ctx.geometry
        grad_out = grad_out.contiguous()
        in_rows, out_rows = features.shape[0], grad_out.shape[0]
        grad_in = grad_w = grad_b = None
        if ctx.needs_input_grad[0]:
            wt = weight.reshape(taps, cin, cout).transpose(1, 2).contiguous()   # (taps, Cout, Cin)
            grad_in = torch.zeros_like(features)   # the kernel writes live rows only: the others stay exactly 0
            launch('dfm_sparse_conv_fwd', cout, cin, taps, grad_out, out_rows, ctx.inv, ctx.in_indices, in_rows, wt,
                   None, None, 0, grad_in, STREAM)
        if ctx.needs_input_grad[1]:
            grad_w = torch.empty_like(weight, memory_format=torch.contiguous_format)
            nbytes = _capi.lib().dfm_sparse_conv_wgrad_workspace_bytes(cin, cout, taps, out_rows)
            launch('dfm_sparse_conv_wgrad', cin, cout, taps, features, in_rows, ctx.nbr, ctx.out_indices, out_rows,
                   grad_out, grad_w, WS, ctx.live_rows, STREAM, ws_bytes=max(nbytes, 16))
        if has_bias and ctx.needs_input_grad[2]:
            # the live rows' column sums: the BatchNorm backward's reduction with mean 0 and no ReLU (its first sum)
            stats = torch.zeros((cout, 3), dtype=torch.float32, device=grad_out.device)
            sums = torch.empty((2, cout), dtype=torch.float32, device=grad_out.device)
            nbytes = _capi.lib().dfm_sparse_bn_workspace_bytes(out_rows, cout)
            launch('dfm_sparse_bn_bwd_reduce', grad_out, grad_out, ctx.out_indices, out_rows, cout, stats, None, None,
                   1.0, 0, sums, WS, ctx.live_rows, STREAM, ws_bytes=max(nbytes, 16))
            grad_b = sums[0]
        return grad_in, grad_w, grad_b, None, None, None, None, None, None


def conv_rows(conv, x, nbr, out_indices, inverse, live_rows=None):
    """the output rows of the marked convolution ``conv`` in training mode, under autograd (``_SparseConvBase._run``)"""
    who = f'{type(conv).__name__}({conv.in_channels}->{conv.out_channels})'
    if x.features.requires_grad and torch.is_grad_enabled() and conv.in_channels not in _GRAD_IN_CHANNELS:
        _refuse(who, f'an input gradient for Cin = {conv.in_channels} (the input-gradient kernel covers Cin = 16, 32 '
                     'or 64: detach the input rows)')
    return _ConvFn.apply(x.features, conv.weight, conv.bias, conv, nbr, x.indices, out_indices, inverse, live_rows)


class _BatchNormFn(torch.autograd.Function):
    """BatchNorm1d in training mode over the rows with b >= 0, then the optional ReLU"""

    @staticmethod
    def forward(ctx, x, weight, bias, indices, bn, relu, live_rows):
        rows, c = x.shape
        stats = torch.empty((c, 3), dtype=torch.float32, device=x.device)
        nbytes = max(_capi.lib().dfm_sparse_bn_workspace_bytes(rows, c), 16)
        launch('dfm_sparse_bn_stats', x, indices, rows, c, stats, WS, live_rows, STREAM, ws_bytes=nbytes)
        y = torch.empty_like(x)
        launch('dfm_sparse_bn_apply', x, indices, rows, c, stats, weight, bias, float(bn.eps), int(relu), y, STREAM)
        if bn.track_running_stats and bn.running_mean is not None:
            launch('dfm_sparse_bn_running', stats, c, float(bn.momentum), bn.running_mean, bn.running_var, STREAM)
            bn.num_batches_tracked += 1
        ctx.save_for_backward(x, weight, bias, stats)
        ctx.indices, ctx.eps, ctx.relu, ctx.live_rows = indices, float(bn.eps), int(relu), live_rows
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_y):
        x, weight, bias, stats = ctx.saved_tensors
        rows, c = x.shape
        grad_y = grad_y.contiguous()
        sums = torch.empty((2, c), dtype=torch.float32, device=x.device)
        nbytes = max(_capi.lib().dfm_sparse_bn_workspace_bytes(rows, c), 16)
        launch('dfm_sparse_bn_bwd_reduce', x, grad_y, ctx.indices, rows, c, stats, weight, bias, ctx.eps, ctx.relu,
               sums, WS, ctx.live_rows, STREAM, ws_bytes=nbytes)
        grad_x = None
        if ctx.needs_input_grad[0]:
            grad_x = torch.empty_like(x)
            launch('dfm_sparse_bn_bwd_apply', x, grad_y, ctx.indices, rows, c, stats, sums, weight, bias, ctx.eps,
                   ctx.relu, grad_x, STREAM)
        return (grad_x, sums[1] if weight is not None and ctx.needs_input_grad[1] else None,
                sums[0] if bias is not None and ctx.needs_input_grad[2] else None, None, None, None, None)


def _world_size():
    dist = torch.distributed
    return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1


def batch_norm_rows(features, indices, bn, relu, live_rows=None):
    """``relu(bn(features))`` over the live rows, ``bn`` a training-mode ``BatchNorm1d`` (``SparseSequential``);
    ``live_rows``: one int32 on the device that every row at or past it has b < 0, or None"""
    who = f'{type(bn).__name__}({bn.num_features})'
    if not bn.training:
        _refuse(who, 'eval mode after a convolution in training mode (frozen-BN fine-tuning)')
    if (isinstance(bn, nn.SyncBatchNorm) or getattr(bn, 'cross_rank', False)) and _world_size() > 1:
        _refuse(who, f'SyncBN in a process group of {_world_size()} ranks (cross-rank statistics are not built: the '
                     'kernels run one rank)')
    if bn.num_features not in (16, 32, 64):
        _refuse(who, f'{bn.num_features} channels (the kernels cover 16, 32 and 64)')
    if bn.track_running_stats and bn.momentum is None:
        _refuse(who, 'momentum=None (the cumulative average needs the step count on the host)')
    tensors = [t for t in (features, bn.weight, bn.bias, bn.running_mean, bn.running_var) if t is not None]
    if any(t.dtype != torch.float32 for t in tensors):
        _refuse(who, f'dtype {[str(t.dtype) for t in tensors if t.dtype != torch.float32][0]} (the kernels are fp32)')
    if features.dim() != 2 or features.shape[1] != bn.num_features or not features.is_contiguous():
        raise ValueError(f'features are contiguous (N, {bn.num_features}), got {tuple(features.shape)}')
    return _BatchNormFn.apply(features, bn.weight, bn.bias, indices, bn, bool(relu), live_rows)


class _DenseFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, indices, batch_size, spatial_shape):
        rows, c = features.shape
        out = torch.empty((batch_size, c, *spatial_shape), dtype=torch.float32, device=features.device)
        launch('dfm_sparse_dense', features, indices, rows, c, batch_size, _size3(spatial_shape), out, STREAM)
        ctx.indices, ctx.geometry = indices, (rows, c, batch_size, tuple(spatial_shape))
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_volume):
        rows, c, batch_size, spatial_shape = ctx.geometry
        grad_volume = grad_volume.contiguous()
        grad = torch.empty((rows, c), dtype=torch.float32, device=grad_volume.device)
        launch('dfm_sparse_dense_bwd', grad_volume, ctx.indices, rows, c, batch_size, _size3(spatial_shape), grad,
               STREAM)
        return grad, None, None, None


def dense_rows(x):
    """``x.dense()`` under autograd"""
    return _DenseFn.apply(x.features.contiguous(), x.indices, x.batch_size, x.spatial_shape)
