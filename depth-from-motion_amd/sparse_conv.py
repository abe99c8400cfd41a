"""Sparse 3-D convolutions of the LiDAR teacher on the HIP path, forward only, eval only.

Mirror of what the KITTI configs' frozen teacher builds from mmcv's spconv wrapper: ``SparseConvTensor``,
``SubMConv3d``, ``SparseConv3d``, ``SparseSequential``, the reference's ``make_sparse_convmodule``
(ops/sparse_block.py) and ``CustomSparseEncoder`` (middle_encoders/sparse_encoder.py) with the reference's constructor,
return values and state-dict keys.  mmcv is not a dependency: the semantics are those stated in
include/dfm_hip_sparse_conv.h -- rows ``(N, C)`` fp32 plus ``(N, 4)`` int32 coordinates ``(b, z, y, x)``; a row with
``b < 0`` does not exist (the fixed-capacity padding of ``hard_voxelize_batch`` and of every strided layer's row
bound); weights in mmcv 1.x's ``(kD, kH, kW, Cin, Cout)`` layout; eval-mode BatchNorm and ReLU applied in the
convolution's epilogue on active rows only, from a scale / shift pair kept in the derived-state cache.

Host waits: none in any layer, in ``dense()`` or in ``CustomSparseEncoder.forward``: row counts and the status word
stay on the device.  ``SparseConvTensor.check_status()`` / ``CustomSparseEncoder.check_status()`` read the status word
(ONE host wait) and raise ``DfmHipError`` when an index kernel reported a duplicate coordinate, a full table, a row
bound or a coordinate outside the grid.

There is no torch path behind these classes: a setting the kernels do not cover (training mode, an input that
requires grad, ``block_type='basicblock'``, channel counts outside Cin in {3, 4, 8, ..., 64} / Cout in {16, 32, 64},
a dtype other than fp32) raises ``MfmaPathError`` naming the setting under every fallback policy.  CPU tensors raise
the package's "no CPU path" error.

Training is opt-in: ``enable_sparse_training(module)`` (sparse_train.py) marks the layers of a tree, and a marked layer
in training mode runs under autograd -- the convolution without an epilogue, a BatchNorm over the live rows, ``dense()``
with a gathering backward.  Unmarked layers, and marked ones in eval mode under ``torch.no_grad()``, run as above.
"""
import ctypes

import torch
from torch import nn

from . import _capi
from ._launch import STREAM, launch, require_gpu
from .fallback import MfmaPathError
from .derived import derived
from .registry import register_module

__all__ = ['SparseConvTensor', 'SubMConv3d', 'SparseConv3d', 'SparseSequential', 'make_sparse_convmodule',
           'CustomSparseEncoder', 'sparse_conv_plan']



def _triple(v):
    if isinstance(v, (tuple, list)):
        if len(v) != 3:
            raise ValueError(f'expected an int or three, got {v!r}')
        return tuple(int(i) for i in v)
    return (int(v),) * 3


def _size3(shape):
    return (ctypes.c_int32 * 3)(*[int(s) for s in shape])


def _conv_desc(batch_size, spatial_shape, kernel, stride, padding, subm):
    d = _capi.SparseConvDesc(batch=int(batch_size), subm=int(bool(subm)))
    for a in range(3):
        d.in_size[a], d.kernel[a], d.stride[a], d.padding[a] = (int(spatial_shape[a]), kernel[a], stride[a],
                                                                 padding[a])
    return d


def sparse_conv_plan(batch_size, spatial_shape, kernel_size, stride=1, padding=0, in_rows=0, subm=False):
    """the plan of one layer (host only, ``dfm_sparse_conv_out_shape``): dict with ``out_shape`` (the output grid),
    ``taps``, ``out_rows`` (the row bound), ``in_capacity`` / ``out_capacity`` (hash-table slots) and
    ``workspace_bytes``; a geometry the kernels refuse raises ``DfmHipError``"""
    d = _conv_desc(batch_size, spatial_shape, _triple(kernel_size), _triple(stride), _triple(padding), subm)
    plan = _capi.SparseConvPlan()
    _capi.check(_capi.lib().dfm_sparse_conv_out_shape(ctypes.byref(d), int(in_rows), ctypes.byref(plan)))
    return dict(out_shape=list(plan.out_size), taps=plan.taps, out_rows=plan.out_rows, in_capacity=plan.in_capacity,
                out_capacity=plan.out_capacity,
                workspace_bytes=_capi.lib().dfm_sparse_conv_workspace_bytes(ctypes.byref(d), int(in_rows)))


def _status_message(word):
    return '; '.join(text for bit, text in _capi.SPARSE_STATUS.items() if word & bit)


class SparseConvTensor:
    """Rows ``features (N, C)`` fp32 at ``indices (N, 4)`` int32 ``(b, z, y, x)`` of a ``spatial_shape = [D, H, W]``
    grid over ``batch_size`` samples.  Coordinates are unique among the rows with ``b >= 0``; rows with ``b < 0`` do not
    exist.  ``indice_dict`` holds the neighbour tables the SubM layers of one stage share by ``indice_key``.  The order
    of rows is unspecified: ``dense()`` and the (coordinate -> row) relation are the contract."""

    def __init__(self, features, indices, spatial_shape, batch_size, grid=None):
        self.features, self.indices = features, indices
        self.spatial_shape, self.batch_size = [int(s) for s in spatial_shape], int(batch_size)
        self.indice_dict = {}
        self.grid = grid
        self.num_rows = None    # a strided layer's output: its live row count, one int32 ON THE DEVICE
        self._status = None     # one int32 on the device, shared along a chain of layers
        self._table = None      # (keys, rows, capacity): the hash table over ``indices``, built once
        self._train = False     # computed by a layer that enable_sparse_training marked, in training mode
        self._live_rows = None  # one int32 on the device: every row at or past it has b < 0 (a sorted strided output)

    @property
    def spatial_size(self):
        return self.spatial_shape[0] * self.spatial_shape[1] * self.spatial_shape[2]

    def status(self):
        if self._status is None:
            self._status = torch.zeros((1,), dtype=torch.int32, device=self.indices.device)
        return self._status

    def check_status(self):
        """ONE host wait: raises ``DfmHipError`` when an index kernel that ran for this tensor (or for a tensor it was
        computed from) reported a problem"""
        word = 0 if self._status is None else int(self._status.item())
        if word:
            raise _capi.DfmHipError(f'sparse convolution index: {_status_message(word)} (status {word})')

    def table(self):
        if self._table is None:
            rows = self.indices.shape[0]
            capacity = 16
            while capacity < 2 * rows:
                capacity *= 2
            keys = torch.full((capacity,), -1, dtype=torch.int64, device=self.indices.device)
            vals = torch.empty((capacity,), dtype=torch.int32, device=self.indices.device)
            launch('dfm_sparse_index_build', self.indices, rows, self.batch_size, _size3(self.spatial_shape), keys,
                   vals, capacity, self.status(), STREAM)
            self._table = (keys, vals, capacity)
        return self._table

    def _like(self, features, train=False):
        """the same row set with new features: shares the tables and the status word"""
        out = SparseConvTensor(features, self.indices, self.spatial_shape, self.batch_size, self.grid)
        out.indice_dict, out._status, out._table = self.indice_dict, self.status(), self._table
        out._train, out._live_rows = self._train or bool(train), self._live_rows
        return out

    def dense(self, channels_first=True):
        """``(B, C, D, H, W)``: zeros plus one scatter of the live rows (``channels_first=False``: a permuted view
        ``(B, D, H, W, C)``).  No host wait."""
        require_gpu(self.features, 'features')
        c = self.features.shape[1]
        if self._train and self.features.requires_grad and torch.is_grad_enabled():
            from . import sparse_train
            out = sparse_train.dense_rows(self)   # the same launch under autograd: the backward gathers the live rows
            return out if channels_first else out.permute(0, 2, 3, 4, 1)
        out = torch.empty((self.batch_size, c, *self.spatial_shape), dtype=torch.float32, device=self.features.device)
        launch('dfm_sparse_dense', self.features, self.indices, self.features.shape[0], c, self.batch_size,
               _size3(self.spatial_shape), out, STREAM)
        return out if channels_first else out.permute(0, 2, 3, 4, 1)


def _fold_batch_norm(bn):
    """(scale, shift) fp32 of an eval-mode BatchNorm1d, computed once per parameter version (derived-state cache)"""
    sources = tuple(t for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var) if t is not None)

    def make():
        with torch.no_grad():
            inv = torch.rsqrt(bn.running_var.float() + bn.eps)
            scale = inv * bn.weight.float() if bn.weight is not None else inv
            shift = -bn.running_mean.float() * scale
            if bn.bias is not None:
                shift = shift + bn.bias.float()
            return scale.contiguous(), shift.contiguous()

    return derived(bn).get('sparse_bn_fold', sources, make, extra=(float(bn.eps),))


class _SparseConvBase(nn.Module):
    """parameters and checks shared by SubMConv3d and SparseConv3d: ``weight (kD, kH, kW, Cin, Cout)``, mmcv 1.x's
    layout, and an optional ``bias`` (the encoder builds none; a bias is folded into the epilogue's shift)"""
    subm = False
    sparse_training = False   # enable_sparse_training(module) sets it: training mode runs under autograd

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=True,
                 indice_key=None):
        super().__init__()
        self.in_channels, self.out_channels = int(in_channels), int(out_channels)
        self.kernel_size, self.stride, self.padding = _triple(kernel_size), _triple(stride), _triple(padding)
        self.dilation, self.groups, self.indice_key = _triple(dilation), int(groups), indice_key
        self.ndim, self.inverse, self.transposed, self.output_padding = 3, False, False, (0, 0, 0)
        self.conv1x1 = self.kernel_size == (1, 1, 1) and self.stride == (1, 1, 1) and self.padding == (0, 0, 0)
        self.weight = nn.Parameter(torch.empty(*self.kernel_size, self.in_channels, self.out_channels))
        if bias:
            self.bias = nn.Parameter(torch.empty(self.out_channels))
        else:
            self.register_parameter('bias', None)
        self.reset_parameters()

    def reset_parameters(self):
        taps = self.kernel_size[0] * self.kernel_size[1] * self.kernel_size[2]
        bound = 1.0 / (taps * self.in_channels) ** 0.5
        with torch.no_grad():
            self.weight.uniform_(-bound, bound)
            if self.bias is not None:
                self.bias.uniform_(-bound, bound)

    def config_why_not(self):
        """why the kernels do not take this layer (None: they do): the part that needs no input"""
        cin, cout = self.in_channels, self.out_channels
        if not ((cin == 3 or cin % 4 == 0) and 1 <= cin <= 64) or cout not in (16, 32, 64):
            return (f'channels {cin}->{cout} (the kernel covers Cin = 3 or a multiple of 4 up to 64 and Cout = 16, 32 '
                    'or 64)')
        if self.dilation != (1, 1, 1) or self.groups != 1:
            return f'dilation={self.dilation}, groups={self.groups} (the kernels are built for 1 and 1)'
        if self.subm and self.kernel_size != (3, 3, 3):
            return f'SubMConv3d kernel_size={self.kernel_size} (the kernel is built for 3)'
        if self.kernel_size[0] * self.kernel_size[1] * self.kernel_size[2] > _capi.SPARSE_MAX_TAPS:
            return f'kernel_size={self.kernel_size} (at most {_capi.SPARSE_MAX_TAPS} offsets)'
        if self.weight.dtype != torch.float32:
            return f'weight dtype {self.weight.dtype} (the kernels are fp32)'
        return None

    def _check(self, x):
        if not isinstance(x, SparseConvTensor):
            raise TypeError(f'{type(self).__name__} takes a SparseConvTensor, got {type(x).__name__}')
        require_gpu(x.features, 'features')
        require_gpu(x.indices, 'indices')
        why = self.config_why_not()
        if self.sparse_training:
            if why is None and not self.training and torch.is_grad_enabled() and (
                    x.features.requires_grad or any(p.requires_grad for p in self.parameters())):
                why = ('eval mode with an input or a weight that needs a gradient (frozen-BN fine-tuning): '
                       'enable_sparse_training covers training mode; evaluate under torch.no_grad()')
        elif why is None and self.training:
            why = 'module in training mode (the sparse convolutions are forward only, eval only: call .eval())'
        elif why is None and (x.features.requires_grad and torch.is_grad_enabled()):
            why = 'input that requires grad (there is no backward)'
        if why is None and x.features.dtype != torch.float32:
            why = f'feature dtype {x.features.dtype} (the kernels are fp32)'
        if why is not None:
            raise MfmaPathError(f'{type(self).__name__}({self.in_channels}->{self.out_channels}): {why} -- not '
                                'covered by the sparse-convolution kernels, and there is no torch path behind them')
        if x.features.dim() != 2 or x.features.shape[1] != self.in_channels:
            raise ValueError(f'features are (N, {self.in_channels}), got {tuple(x.features.shape)}')
        if x.indices.dtype != torch.int32 or tuple(x.indices.shape) != (x.features.shape[0], 4):
            raise ValueError(f'indices are (N, 4) int32, got {tuple(x.indices.shape)} {x.indices.dtype}')
        if not x.features.is_contiguous() or not x.indices.is_contiguous():
            raise ValueError('features and indices must be contiguous')

    def _epilogue(self, norm):
        """(scale, shift) of the BatchNorm that follows (None: none) with this layer's bias folded in"""
        if norm is None and self.bias is None:
            return None, None
        if norm is None:
            return derived(self).get('sparse_bias_fold', (self.bias,), lambda: (
                torch.ones_like(self.bias.detach(), dtype=torch.float32), self.bias.detach().float().contiguous()))
        scale, shift = _fold_batch_norm(norm)
        if self.bias is not None:
            shift = shift + self.bias.detach().float() * scale
        return scale, shift

    def _run(self, x, nbr, out_indices, norm, relu, inverse=None, live_rows=None):
        """the output rows: today's fused launch, or -- a layer marked by ``enable_sparse_training``, in training
        mode -- the convolution under autograd, without an epilogue (``inverse()``: the inverse table, built when the
        input needs a gradient; ``live_rows``: the device count the output's live rows are the first of, or None)"""
        if self.sparse_training and self.training:
            if norm is not None or relu:
                raise MfmaPathError(f'{type(self).__name__}({self.in_channels}->{self.out_channels}): a fused '
                                    'BatchNorm / ReLU epilogue in training mode -- enable_sparse_training must mark '
                                    'the SparseSequential around the convolution as well (call it on the whole tree)')
            from . import sparse_train
            return sparse_train.conv_rows(self, x, nbr, out_indices, inverse, live_rows)
        scale, shift = self._epilogue(norm)
        taps = self.kernel_size[0] * self.kernel_size[1] * self.kernel_size[2]
        out_rows = out_indices.shape[0]
        out = torch.empty((out_rows, self.out_channels), dtype=torch.float32, device=x.features.device)
        launch('dfm_sparse_conv_fwd', self.in_channels, self.out_channels, taps, x.features, x.features.shape[0], nbr,
               out_indices, out_rows, self.weight.detach(), scale, shift, int(bool(relu)), out, STREAM)
        return out

    def forward(self, x):
        return self.forward_fused(x, None, False)

    def extra_repr(self):
        return (f'{self.in_channels}, {self.out_channels}, kernel_size={self.kernel_size}, stride={self.stride}, '
                f'padding={self.padding}, bias={self.bias is not None}, indice_key={self.indice_key!r}')


@register_module(on_path=False)
class SubMConv3d(_SparseConvBase):
    """Submanifold convolution, k = 3: the output rows are the input rows.  The neighbour table is built once per
    ``indice_key`` and shared by the layers of a stage.  ``padding`` is ignored, as in spconv."""
    subm = True

    def forward_fused(self, x, norm=None, relu=False):
        """the layer with the BatchNorm1d ``norm`` (eval) and the ReLU that follow it applied in its epilogue"""
        self._check(x)
        entry = x.indice_dict.get(self.indice_key) if self.indice_key is not None else None
        if entry is None or entry[0] is not x.indices:
            keys, vals, capacity = x.table()
            rows = x.indices.shape[0]
            nbr = torch.empty((27, rows), dtype=torch.int32, device=x.indices.device)
            launch('dfm_sparse_subm_neighbours', x.indices, rows, x.batch_size, _size3(x.spatial_shape), keys, vals,
                   capacity, nbr, STREAM)
            entry = [x.indices, nbr, None]   # the third: the inverse table, made by the first backward-capable call
            if self.indice_key is not None:
                x.indice_dict[self.indice_key] = entry

        def inverse():   # inv[k] = nbr[26 - k]: no kernel
            if entry[2] is None:
                entry[2] = entry[1].flip(0)
            return entry[2]

        return x._like(self._run(x, entry[1], x.indices, norm, relu, inverse, x._live_rows),
                       self.sparse_training and self.training)


@register_module(on_path=False)
class SparseConv3d(_SparseConvBase):
    """Strided sparse convolution: an output site is active iff its receptive field holds an active input, and its
    value is the dense convolution's.  The output has ``plan.out_rows`` fixed-capacity rows; the live ones are numbered
    by an atomic counter on the device, the rest have ``b = -1``.  1x1x1 with stride 1 keeps the row set."""

    def forward_fused(self, x, norm=None, relu=False):
        self._check(x)
        if self.conv1x1:
            return x._like(self._run(x, None, x.indices, norm, relu, None, x._live_rows),
                           self.sparse_training and self.training)
        rows, device = x.indices.shape[0], x.indices.device
        d = _conv_desc(x.batch_size, x.spatial_shape, self.kernel_size, self.stride, self.padding, False)
        plan = _capi.SparseConvPlan()
        _capi.check(_capi.lib().dfm_sparse_conv_out_shape(ctypes.byref(d), rows, ctypes.byref(plan)))
        keys, vals, capacity = x.table()
        assert capacity == plan.in_capacity
        sorted_count = None
        out_keys = torch.full((plan.out_capacity,), -1, dtype=torch.int64, device=device)
        out_indices = torch.full((plan.out_rows, 4), -1, dtype=torch.int32, device=device)
        count = torch.zeros((1,), dtype=torch.int32, device=device)
        launch('dfm_sparse_conv_out_rows', d, x.indices, rows, out_keys, out_indices, count, x.status(), STREAM)
        if self.sparse_training and self.training:
            # the atomic counter numbers the rows in arrival order; the sums over rows of the training kernels (batch
            # statistics, weight gradient) are bit-reproducible only over a fixed order: ascending (b, z, y, x), the
            # rows that do not exist last (a device sort, as the voxelization's; no host wait)
            i = out_indices.long()
            key = ((i[:, 0] * plan.out_size[0] + i[:, 1]) * plan.out_size[1] + i[:, 2]) * plan.out_size[2] + i[:, 3]
            key = torch.where(i[:, 0] >= 0, key, torch.full_like(key, torch.iinfo(torch.int64).max))
            out_indices = out_indices[torch.argsort(key)].contiguous()
            sorted_count = count
        nbr = torch.empty((plan.taps, plan.out_rows), dtype=torch.int32, device=device)
        launch('dfm_sparse_conv_neighbours', d, out_indices, rows, keys, vals, nbr, STREAM)

        def inverse():   # kept beside the forward table under the layer's indice_key
            inv = torch.full((plan.taps, rows), -1, dtype=torch.int32, device=device)
            launch('dfm_sparse_inverse_table', nbr, plan.taps, plan.out_rows, rows, inv, STREAM)
            if self.indice_key is not None:
                x.indice_dict[self.indice_key] = [x.indices, nbr, inv]
            return inv

        out = SparseConvTensor(self._run(x, nbr, out_indices, norm, relu, inverse, sorted_count), out_indices,
                               list(plan.out_size), x.batch_size, x.grid)
        out._train, out._live_rows = x._train or (self.sparse_training and self.training), sorted_count
        out.indice_dict, out._status = x.indice_dict, x.status()
        out.num_rows = count
        return out


class SparseSequential(nn.Sequential):
    """mmcv's ``SparseSequential``: runs sparse layers on the tensor and plain modules on its features.  A sparse
    convolution followed by an eval-mode ``BatchNorm1d`` and / or a ``ReLU`` runs as ONE launch: both are the
    convolution's epilogue, on active rows only."""

    sparse_training = False   # enable_sparse_training(module) sets it

    def forward(self, input):
        mods = list(self)
        i = 0
        while i < len(mods):
            m = mods[i]
            if isinstance(m, _SparseConvBase) and self.sparse_training and m.sparse_training and m.training:
                # a marked chain in training mode: the convolution without an epilogue, then the BatchNorm over the
                # live rows with the ReLU that follows it, all three under autograd (sparse_train.py)
                from . import sparse_train
                input, i = m.forward_fused(input, None, False), i + 1
                if i < len(mods) and isinstance(mods[i], (nn.BatchNorm1d, nn.SyncBatchNorm)):
                    norm, i = mods[i], i + 1
                    relu = i < len(mods) and isinstance(mods[i], nn.ReLU)
                    i += int(relu)
                    out = input._like(sparse_train.batch_norm_rows(input.features, input.indices, norm, relu,
                                                                   input._live_rows), True)
                    out.num_rows, input = input.num_rows, out
            elif isinstance(m, _SparseConvBase):
                norm, relu, j = None, False, i + 1
                if j < len(mods) and isinstance(mods[j], nn.BatchNorm1d):
                    norm, j = mods[j], j + 1
                    if norm.training or not norm.track_running_stats:
                        raise MfmaPathError(f'{type(norm).__name__} in training mode after a sparse convolution: the '
                                            'teacher is eval only (call .eval())')
                if j < len(mods) and isinstance(mods[j], nn.ReLU):
                    relu, j = True, j + 1
                input, i = m.forward_fused(input, norm, relu), j
            elif isinstance(m, SparseSequential) or not isinstance(input, SparseConvTensor):
                input, i = m(input), i + 1
            else:   # a plain module on the features, as mmcv applies it
                input, i = input._like(m(input.features)), i + 1
        return input


def _build_norm_1d(norm_cfg, num_features):
    cfg = dict(norm_cfg)
    kind = cfg.pop('type')
    cfg.pop('requires_grad', None)
    if kind not in ('BN1d', 'SyncBN', 'BN'):
        raise MfmaPathError(f'norm_cfg type {kind!r}: the sparse encoder builds BatchNorm1d (BN1d | SyncBN), eval only')
    bn = nn.BatchNorm1d(num_features, **cfg)   # SyncBN in eval mode is a BatchNorm1d
    bn.cross_rank = kind == 'SyncBN'   # training (sparse_train.py) refuses it in a group of more than one rank
    return bn


_CONV_TYPES = dict(SubMConv3d=SubMConv3d, SparseConv3d=SparseConv3d)


def make_sparse_convmodule(in_channels, out_channels, kernel_size, indice_key, stride=1, padding=0,
                           conv_type='SubMConv3d', norm_cfg=None, order=('conv', 'norm', 'act')):
    """the reference's ``make_sparse_convmodule`` (ops/sparse_block.py:137-199), same signature: a
    ``SparseSequential`` of the layers ``order`` names"""
    assert isinstance(order, tuple) and len(order) <= 3
    assert set(order) | {'conv', 'norm', 'act'} == {'conv', 'norm', 'act'}
    if conv_type not in _CONV_TYPES:
        raise MfmaPathError(f'conv_type {conv_type!r}: SubMConv3d and SparseConv3d are built (no inverse convolution)')
    layers = []
    for layer in order:
        if layer == 'conv':
            layers.append(_CONV_TYPES[conv_type](in_channels, out_channels, kernel_size, stride=stride,
                                                 padding=padding, bias=False, indice_key=indice_key))
        elif layer == 'norm':
            layers.append(_build_norm_1d(norm_cfg, out_channels))
        elif layer == 'act':
            layers.append(nn.ReLU(inplace=True))
    return SparseSequential(*layers)


@register_module(on_path=False)
class CustomSparseEncoder(nn.Module):
    """The reference's ``CustomSparseEncoder`` (middle_encoders/sparse_encoder.py:217-440): same constructor, same
    state-dict keys (``conv_input.0.weight``, ``conv_input.1.*``, ``encoder_layers.encoder_layer2.0.0.weight``, ...,
    ``conv_out.0.weight``), ``forward(voxel_features, coors, batch_size)`` -> ``spatial_features (B, C * D, H, W)`` or,
    with ``output_volume_feat``, ``(spatial_features, volume_features (B, C, D, H, W))``.  Forward only, eval only
    (under autograd, with the same return values, once ``enable_sparse_training`` has marked it: sparse_train.py); no
    host wait.  ``coors`` may carry rows with batch index -1 (``hard_voxelize_batch``'s padding): they do not exist."""

    def __init__(self, in_channels, sparse_shape, order=('conv', 'norm', 'act'),
                 norm_cfg=dict(type='BN1d', eps=1e-3, momentum=0.01), base_channels=16, output_channels=128,
                 encoder_channels=((16, ), (32, 32, 32), (64, 64, 64), (64, 64, 64)),
                 encoder_strides=((1, ), (2, 1, 1), (2, 1, 1), (2, 1, 1)),
                 encoder_paddings=((1, ), (1, 1, 1), (1, 1, 1), ((0, 1, 1), 1, 1)), block_type='conv_module',
                 with_final_bnrelu=True, output_volume_feat=False):
        super().__init__()
        assert block_type in ['conv_module', 'basicblock']
        if block_type == 'basicblock':
            raise MfmaPathError("CustomSparseEncoder: block_type='basicblock' (SparseBasicBlock) -- not covered by the "
                                'sparse-convolution kernels, and there is no torch path behind them')
        self.sparse_shape, self.in_channels, self.order = sparse_shape, in_channels, order
        self.base_channels, self.output_channels = base_channels, output_channels
        self.encoder_channels, self.encoder_strides = encoder_channels, encoder_strides
        self.encoder_paddings, self.with_final_bnrelu = encoder_paddings, with_final_bnrelu
        self.output_volume_feat, self.stage_num, self.fp16_enabled = output_volume_feat, len(encoder_channels), False
        assert isinstance(order, tuple) and len(order) == 3
        assert set(order) == {'conv', 'norm', 'act'}
        if order[0] != 'conv':   # pre activate
            self.conv_input = make_sparse_convmodule(in_channels, base_channels, 3, norm_cfg=norm_cfg, padding=1,
                                                     indice_key='subm1', conv_type='SubMConv3d', order=('conv', ))
        else:                    # post activate
            self.conv_input = make_sparse_convmodule(in_channels, base_channels, 3, norm_cfg=norm_cfg, padding=1,
                                                     indice_key='subm1', conv_type='SubMConv3d')
        encoder_out_channels = self.make_encoder_layers(make_sparse_convmodule, norm_cfg, base_channels)
        if with_final_bnrelu:
            self.conv_out = make_sparse_convmodule(encoder_out_channels, output_channels, kernel_size=(3, 1, 1),
                                                   stride=(2, 1, 1), norm_cfg=norm_cfg, padding=0,
                                                   indice_key='spconv_down2', conv_type='SparseConv3d')
        else:
            self.conv_out = make_sparse_convmodule(encoder_out_channels, output_channels, kernel_size=1, stride=1,
                                                   norm_cfg=norm_cfg, padding=0, indice_key='spconv_down2',
                                                   conv_type='SparseConv3d', order=('conv', ))
        self._last = None

    def make_encoder_layers(self, make_block, norm_cfg, in_channels, block_type='conv_module',
                            conv_cfg=dict(type='SubMConv3d')):
        self.encoder_layers = SparseSequential()
        for i, blocks in enumerate(self.encoder_channels):
            blocks_list = []
            for j, out_channels in enumerate(tuple(blocks)):
                stride = tuple(self.encoder_strides[i])[j]
                padding = tuple(self.encoder_paddings[i])[j]
                if i != 0 and j == 0:   # each stage starts with a strided layer, except the first
                    blocks_list.append(make_block(in_channels, out_channels, 3, norm_cfg=norm_cfg, stride=stride,
                                                  padding=padding, indice_key=f'spconv{i + 1}',
                                                  conv_type='SparseConv3d'))
                else:
                    blocks_list.append(make_block(in_channels, out_channels, 3, norm_cfg=norm_cfg, stride=stride,
                                                  padding=padding, indice_key=f'subm{i + 1}',
                                                  conv_type='SubMConv3d'))
                in_channels = out_channels
            self.encoder_layers.add_module(f'encoder_layer{i + 1}', SparseSequential(*blocks_list))
        return out_channels

    def forward_stages(self, voxel_features, coors, batch_size):
        """-> the sparse tensors after ``conv_input``, every encoder stage and ``conv_out`` (tests, timing tools)"""
        require_gpu(voxel_features, 'voxel_features')
        require_gpu(coors, 'coors')
        x = SparseConvTensor(voxel_features, coors.int().contiguous(), self.sparse_shape, batch_size)
        stages = [self.conv_input(x)]
        for encoder_layer in self.encoder_layers:
            stages.append(encoder_layer(stages[-1]))
        stages.append(self.conv_out(stages[-1]))
        self._last = stages[-1]
        return stages

    def forward(self, voxel_features, coors, batch_size):
        out = self.forward_stages(voxel_features, coors, batch_size)[-1]
        volume_features = out.dense()
        n, c, d, h, w = volume_features.shape
        spatial_features = volume_features.view(n, c * d, h, w)
        return (spatial_features, volume_features) if self.output_volume_feat else spatial_features

    def check_status(self):
        """ONE host wait: the status word of the last forward (``DfmHipError`` on a duplicate coordinate, ...)"""
        if self._last is not None:
            self._last.check_status()
