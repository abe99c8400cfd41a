"""Modulated deformable convolution (DCNv2) on the HIP path.

Mirror of mmcv's ``modulated_deform_conv2d`` / ``ModulatedDeformConv2d`` / ``ModulatedDeformConv2dPack``
(mmcv/ops/modulated_deform_conv.py), which the Waymo configs' backbone builds 26 times: ``ResNet(depth=101,
dcn=dict(type='DCNv2', deform_groups=1, fallback_on_stride=False), stage_with_dcn=(False, False, True, True))``.
mmcv is not a dependency: the semantics are those stated in include/dfm_hip_deform_conv.h.

The layer is a gather followed by a matrix product.  ``dfm_deform_sample_fwd`` writes the columns
``(N, Ho, Wo, 9, Cin)`` -- each the bilinear sample of one tap times its mask -- reading ``x`` in channels-last
memory format in place and the offsets and masks through their strides, so the raw 27 G-channel output of
``conv_offset`` goes in as it is (``mask_is_logit``: the sigmoid runs in the kernel; chunk, cat and sigmoid cost
nothing in either direction).  The product with the ``(Cout, 9 Cin)`` weight is the package's matrix product over
pixel rows, fp32 accumulation, one rounding.  Backward recomputes the columns instead of saving them:
``grad_weight = grad_out^T . columns`` (``long_axis_gram``), ``grad_col = grad_out . W``, then ONE
``dfm_deform_conv_bwd_cols`` launch for ``grad_offset``, ``grad_mask`` (in-wave reductions, reproducible bit for
bit) and ``grad_x`` (float atomics into an fp32 buffer, converted once).

CPU tensors are refused: there is no CPU path.
"""
import ctypes

import torch
from torch import nn

from . import _capi
from ._launch import DTYPES, STREAM, launch, require_gpu
from .conv3d import _mm_f32, long_axis_gram
from .fallback import MfmaPathError, run_reference
from .derived import derived

__all__ = ['deform_sample', 'modulated_deform_conv2d', 'modulated_deform_conv2d_raw', 'ModulatedDeformConv2d', 'ModulatedDeformConv2dPack',
           'deform_conv_out_size']


def _pair(v):
    if isinstance(v, (tuple, list)):
        if len(v) != 2:
            raise ValueError(f'expected an int or a pair, got {v!r}')
        return int(v[0]), int(v[1])
    return int(v), int(v)


def deform_conv_out_size(size, stride=1, padding=0, dilation=1):
    """(Ho, Wo) of a 3x3 kernel over ``size`` = (H, W)"""
    (sh, sw), (ph, pw), (dh, dw) = _pair(stride), _pair(padding), _pair(dilation)
    return ((size[0] + 2 * ph - (2 * dh + 1)) // sh + 1, (size[1] + 2 * pw - (2 * dw + 1)) // sw + 1)


def _check_geometry(x_shape, stride, padding, dilation, deform_groups):
    """validation that needs no device -> (stride, padding, dilation) as pairs and (Ho, Wo)"""
    stride, padding, dilation = _pair(stride), _pair(padding), _pair(dilation)
    if min(stride) < 1 or min(dilation) < 1 or min(padding) < 0:
        raise ValueError(f'stride {stride} and dilation {dilation} start at 1, padding {padding} at 0')
    if len(x_shape) != 4:
        raise ValueError(f'input is (N, Cin, H, W), got {tuple(x_shape)}')
    cin = x_shape[1]
    if deform_groups < 1 or cin % deform_groups:
        raise ValueError(f'deform_groups = {deform_groups} does not divide the {cin} input channels')
    ho, wo = deform_conv_out_size(x_shape[2:], stride, padding, dilation)
    if ho < 1 or wo < 1:
        raise ValueError(f'a {tuple(x_shape[2:])} input is smaller than the dilated 3x3 kernel')
    return stride, padding, dilation, (ho, wo)


def _check_maps(x_shape, out_size, offset, mask, deform_groups):
    n, g = x_shape[0], deform_groups
    if mask is None:
        want = (n, 27 * g, *out_size)
        if tuple(offset.shape) != want:
            raise ValueError(f'the raw conv_offset map is (N, 27 G, Ho, Wo) = {want}, got {tuple(offset.shape)}')
        return
    want_o, want_m = (n, 18 * g, *out_size), (n, 9 * g, *out_size)
    if tuple(offset.shape) != want_o:
        raise ValueError(f'offset is (N, 2 * 9 * G, Ho, Wo) = {want_o}, got {tuple(offset.shape)}')
    if tuple(mask.shape) != want_m:
        raise ValueError(f'mask is (N, 9 * G, Ho, Wo) = {want_m}, got {tuple(mask.shape)}')


def _maps(offset, mask, deform_groups):
    """(offset, mask) as the kernels read them: one dtype out of fp32 / bf16, any strides; ``mask`` None: ``offset``
    is the raw 27 G-channel map and the mask its last 9 G channels"""
    if mask is None:
        raw = offset.detach()
        if raw.dtype not in DTYPES:
            raw = raw.float()
        return raw[:, :18 * deform_groups], raw[:, 18 * deform_groups:]
    offset, mask = offset.detach(), mask.detach()
    if offset.dtype != mask.dtype or offset.dtype not in DTYPES:
        offset, mask = offset.float(), mask.float()
    return offset, mask


def _channels_last(x):
    """``x`` with its channels contiguous (converted once when it is not), and whether it was"""
    was = x.is_contiguous(memory_format=torch.channels_last)
    return (x if was else x.contiguous(memory_format=torch.channels_last)), was


def _desc(x, offset, mask, geom, deform_groups, mask_is_logit):
    stride, padding, dilation, (ho, wo) = geom
    d = _capi.DeformDesc(n=x.shape[0], cin=x.shape[1], h=x.shape[2], w=x.shape[3], ho=ho, wo=wo,
                         stride_h=stride[0], stride_w=stride[1], pad_h=padding[0], pad_w=padding[1],
                         dil_h=dilation[0], dil_w=dilation[1], deform_groups=deform_groups,
                         mask_is_logit=int(bool(mask_is_logit)), dtype=DTYPES[x.dtype], om_dtype=DTYPES[offset.dtype])
    for i in range(4):
        d.offset_stride[i], d.mask_stride[i] = offset.stride(i), mask.stride(i)
    return d


def _columns(x_cl, offset, mask, geom, deform_groups, mask_is_logit):
    """the columns (N, Ho, Wo, 9, Cin) of a channels-last ``x_cl`` (fp32 | bf16); offset / mask as ``_maps`` gives them"""
    ho, wo = geom[3]
    col = torch.empty((x_cl.shape[0], ho, wo, 9, x_cl.shape[1]), dtype=x_cl.dtype, device=x_cl.device)
    launch('dfm_deform_sample_fwd', _desc(x_cl, offset, mask, geom, deform_groups, mask_is_logit), x_cl, offset, mask,
           col, STREAM)
    return col


def _prepare(x, offset, mask, stride, padding, dilation, deform_groups):
    require_gpu(x, 'input')
    require_gpu(offset, 'offset')
    if mask is not None:
        require_gpu(mask, 'mask')
    if x.dtype not in DTYPES:
        raise TypeError(f'input dtype {x.dtype}: float32 or bfloat16')
    geom = _check_geometry(tuple(x.shape), stride, padding, dilation, deform_groups)
    _check_maps(tuple(x.shape), geom[3], offset, mask, deform_groups)
    return geom


def deform_sample(x, offset, mask, stride=1, padding=0, dilation=1, deform_groups=1, mask_is_logit=False):
    """The columns of the modulated deformable 3x3 convolution: ``(N, Ho, Wo, 9, Cin)`` in ``x``'s dtype (fp32 |
    bf16, a bf16 column being the fp32 value rounded once), column ``[n, ho, wo, 3 i + j, c]`` = the bilinear sample
    of ``x[n, c]`` at tap (i, j) of output pixel (ho, wo) times its mask (include/dfm_hip_deform_conv.h).  ``offset``
    ``(N, 18 G, Ho, Wo)`` and ``mask`` ``(N, 9 G, Ho, Wo)`` are read through their strides; ``mask=None``: ``offset``
    is the raw ``(N, 27 G, Ho, Wo)`` map of a ``conv_offset``.  ``mask_is_logit``: the sigmoid is applied in the
    kernel.  No autograd: ``modulated_deform_conv2d`` differentiates."""
    geom = _prepare(x, offset, mask, stride, padding, dilation, deform_groups)
    offset, mask = _maps(offset, mask, deform_groups)
    return _columns(_channels_last(x.detach())[0], offset, mask, geom, deform_groups, mask_is_logit)


def weight_matrix(weight):
    """``(Cout, Cin, 3, 3)`` -> ``(Cout, 9 Cin)`` in the columns' order (tap-major, channels innermost)"""
    return weight.detach().permute(0, 2, 3, 1).reshape(weight.shape[0], -1).contiguous()


class _DeformConvFn(torch.autograd.Function):
    """out = columns(x, offset, mask) . W^T + bias.  ``mask`` None: ``offset`` is the raw 27 G-channel map with
    logits, and its gradient comes back as one tensor of that shape."""

    @staticmethod
    def forward(ctx, x, offset, mask, weight, bias, geom, deform_groups, mask_is_logit, w2):
        x_cl, was_cl = _channels_last(x.detach())
        off, msk = _maps(offset, mask, deform_groups)
        col = _columns(x_cl, off, msk, geom, deform_groups, mask_is_logit)
        if w2 is None:
            w2 = weight_matrix(weight)
        if w2.dtype != x.dtype:
            w2 = w2.to(x.dtype)
        rows = col.view(-1, w2.shape[1])
        if bias is not None:
            out = torch.addmm(bias.detach().to(x.dtype), rows, w2.t())
        else:
            out = _mm_f32(rows, w2.t()) if x.dtype == torch.float32 else torch.mm(rows, w2.t())
        ctx.save_for_backward(x, offset, mask, weight, w2)
        ctx.geom, ctx.deform_groups, ctx.mask_is_logit, ctx.has_bias = geom, deform_groups, mask_is_logit, \
            bias is not None
        out = out.view(x.shape[0], geom[3][0], geom[3][1], -1).permute(0, 3, 1, 2)
        return out if was_cl else out.contiguous()

    @staticmethod
    def backward(ctx, grad_out):
        x, offset, mask, weight, w2 = ctx.saved_tensors
        geom, groups, logit = ctx.geom, ctx.deform_groups, ctx.mask_is_logit
        need_x, need_off, need_mask, need_w, need_b = ctx.needs_input_grad[:5]
        raw = mask is None
        need_maps = need_off or (need_mask and not raw)
        x_cl, was_cl = _channels_last(x.detach())
        go = _channels_last(grad_out.detach().to(x.dtype))[0].permute(0, 2, 3, 1).reshape(-1, w2.shape[0])
        off, msk = _maps(offset, mask, groups)
        gx = goff = gmask = gw = gb = None
        if need_w:
            col = _columns(x_cl, off, msk, geom, groups, logit)
            gw = long_axis_gram(go, col.view(-1, w2.shape[1]))
            gw = gw.view(w2.shape[0], 3, 3, -1).permute(0, 3, 1, 2).to(weight.dtype)
            del col
        if ctx.has_bias and need_b:
            gb = go.sum(0, dtype=torch.float32)
        if need_x or need_maps:
            gcol = torch.mm(go, w2)
            n, (ho, wo) = x.shape[0], geom[3]
            gx32 = gmaps = goff32 = gmask32 = None
            if need_x:
                gx32 = torch.zeros((n, x.shape[2], x.shape[3], x.shape[1]), dtype=torch.float32, device=x.device)
            off_stride = mask_stride = None
            if need_maps:
                gmaps = torch.empty((n, 27 * groups, ho, wo), dtype=torch.float32, device=x.device)
                goff32, gmask32 = gmaps[:, :18 * groups], gmaps[:, 18 * groups:]
                off_stride = (ctypes.c_int64 * 4)(*goff32.stride())
                mask_stride = (ctypes.c_int64 * 4)(*gmask32.stride())
            launch('dfm_deform_conv_bwd_cols', _desc(x_cl, off, msk, geom, groups, logit), x_cl, off, msk, gcol,
                   goff32, off_stride, gmask32, mask_stride, gx32, STREAM)
            if need_x:
                gx = gx32.permute(0, 3, 1, 2)
                gx = gx.to(x.dtype) if was_cl else gx.to(x.dtype).contiguous()
            if need_maps and raw:
                goff = gmaps.to(offset.dtype)
            elif need_maps:
                goff = goff32.to(offset.dtype) if need_off else None
                gmask = gmask32.to(mask.dtype) if need_mask else None
        if gb is not None:
            gb = gb.to(weight.dtype)
        return gx, goff, gmask, gw, gb, None, None, None, None


def _run(x, offset, mask, weight, bias, stride, padding, dilation, deform_groups, mask_is_logit, w2=None):
    geom = _prepare(x, offset, mask, stride, padding, dilation, deform_groups)
    require_gpu(weight, 'weight')
    if tuple(weight.shape) != (weight.shape[0], x.shape[1], 3, 3):
        raise ValueError(f'weight is (Cout, Cin, 3, 3) with Cin = {x.shape[1]}, got {tuple(weight.shape)}')
    if bias is not None and tuple(bias.shape) != (weight.shape[0],):
        raise ValueError(f'bias is (Cout,) = ({weight.shape[0]},), got {tuple(bias.shape)}')
    return _DeformConvFn.apply(x, offset, mask, weight, bias, geom, deform_groups, mask_is_logit, w2)


def _unsupported(weight_shape, groups):
    """why the kernels do not take this configuration (None: they do): the part that needs no input"""
    if tuple(weight_shape[2:]) != (3, 3):
        return f'kernel_size={tuple(weight_shape[2:])} (the kernels are built for 3x3)'
    if groups != 1:
        return f'groups={groups} (the kernels are built for groups=1)'
    return None


def modulated_deform_conv2d(input, offset, mask, weight, bias=None, stride=1, padding=0, dilation=1, groups=1,
                            deform_groups=1):
    """mmcv's ``modulated_deform_conv2d`` (same signature): ``input`` ``(N, Cin, H, W)`` fp32 | bf16 in any memory
    format (one conversion when it is not channels-last; the result comes back in the input's format), ``offset``
    ``(N, 18 G, Ho, Wo)`` with the row displacement of tap k in channel 2 k and the column displacement in 2 k + 1,
    ``mask`` ``(N, 9 G, Ho, Wo)``, ``weight`` ``(Cout, Cin, 3, 3)``.  Differentiable in input, offset, mask, weight
    and bias; ``needs_input_grad`` decides what the backward computes.  3x3 and ``groups = 1`` only: anything else
    follows the fallback policy (mmcv's op where ``patch_reference()`` captured one, else ``MfmaPathError``)."""
    why = _unsupported(tuple(weight.shape), groups)
    if why is not None:
        return run_reference(None, None, why, 'deformable-convolution',
                             (input, offset, mask, weight, bias, stride, padding, dilation, groups, deform_groups),
                             key='modulated_deform_conv2d')
    return _run(input, offset, mask, weight, bias, stride, padding, dilation, deform_groups, False)


def modulated_deform_conv2d_raw(input, raw, weight, bias=None, stride=1, padding=0, dilation=1, deform_groups=1):
    """The same layer from the raw ``(N, 27 G, Ho, Wo)`` output of a ``conv_offset`` (what ``ModulatedDeformConv2dPack``
    runs): channels ``[0, 18 G)`` are the offsets, ``[18 G, 27 G)`` the mask LOGITS -- the sigmoid is applied in the
    kernel, and the gradient comes back as one tensor of the map's shape.  3x3 and ``groups = 1`` only."""
    why = _unsupported(tuple(weight.shape), 1)
    if why is not None:
        raise MfmaPathError(f'modulated_deform_conv2d_raw: {why}')
    return _run(input, raw, None, weight, bias, stride, padding, dilation, deform_groups, True)


class ModulatedDeformConv2d(nn.Module):
    """mmcv's ``ModulatedDeformConv2d``: parameters ``weight`` ``(Cout, Cin / groups, kh, kw)`` and ``bias``, the same
    initialisation (uniform in +-1 / sqrt(Cin kh kw), zero bias); ``forward(x, offset, mask)``."""
    _version = 2

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1,
                 deform_groups=1, bias=True):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size, self.stride, self.padding, self.dilation = (_pair(kernel_size), _pair(stride),
                                                                      _pair(padding), _pair(dilation))
        self.groups, self.deform_groups = groups, deform_groups
        if in_channels % groups or out_channels % groups:
            raise ValueError(f'groups = {groups} must divide the channels ({in_channels} -> {out_channels})')
        if deform_groups < 1 or in_channels % deform_groups:
            raise ValueError(f'deform_groups = {deform_groups} does not divide the {in_channels} input channels')
        self.transposed, self.output_padding = False, (0, 0)
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels // groups, *self.kernel_size))
        if bias:
            self.bias = nn.Parameter(torch.empty(out_channels))
        else:
            self.register_parameter('bias', None)
        self.init_weights()

    def init_weights(self):
        n = self.in_channels * self.kernel_size[0] * self.kernel_size[1]
        bound = 1.0 / n ** 0.5
        with torch.no_grad():
            self.weight.uniform_(-bound, bound)
            if self.bias is not None:
                self.bias.zero_()

    def config_why_not(self):
        return _unsupported(tuple(self.weight.shape), self.groups)

    def _weight_matrix(self):
        return derived(self).get('deform_w2', (self.weight,), lambda: weight_matrix(self.weight))

    def _forward(self, x, offset, mask, mask_is_logit):
        why = self.config_why_not()
        if why is not None:
            if mask is None:   # mmcv's op takes the three chunks
                o1, o2, m = torch.chunk(offset, 3, dim=1)
                offset, mask = torch.cat((o1, o2), dim=1), torch.sigmoid(m)
            return run_reference(self, None, why, 'deformable-convolution',
                                 (x, offset, mask, self.weight, self.bias, self.stride, self.padding, self.dilation,
                                  self.groups, self.deform_groups), key='modulated_deform_conv2d')
        return _run(x, offset, mask, self.weight, self.bias, self.stride, self.padding, self.dilation,
                    self.deform_groups, mask_is_logit, self._weight_matrix())

    def forward(self, x, offset, mask):
        return self._forward(x, offset, mask, False)

    def extra_repr(self):
        return (f'{self.in_channels}, {self.out_channels}, kernel_size={self.kernel_size}, stride={self.stride}, '
                f'padding={self.padding}, dilation={self.dilation}, groups={self.groups}, '
                f'deform_groups={self.deform_groups}, bias={self.bias is not None}')


class ModulatedDeformConv2dPack(ModulatedDeformConv2d):
    """mmcv's ``ModulatedDeformConv2dPack`` (``dict(type='DCNv2')``): the layer with its own ``conv_offset``, a plain
    ``Conv2d(Cin, 27 G, 3, stride, padding, dilation)`` initialised to zero.  State-dict keys ``weight``, ``bias``,
    ``conv_offset.weight``, ``conv_offset.bias``; checkpoints older than ``_version = 2`` name the last two
    ``<layer>_offset.*`` and are renamed on load (by a loader that hands a module the whole state dict, as mmcv's
    ``load_checkpoint`` does; torch's own ``load_state_dict`` filters the keys by prefix first).  ``conv_offset``'s raw output goes to the kernels as it is: channels
    ``[0, 18 G)`` are the offsets (``cat(o1, o2)`` of the three chunks), ``[18 G, 27 G)`` the mask logits."""
    _version = 2

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.conv_offset = nn.Conv2d(self.in_channels, self.deform_groups * 3 * self.kernel_size[0] *
                                     self.kernel_size[1], kernel_size=self.kernel_size, stride=self.stride,
                                     padding=self.padding, dilation=self.dilation, bias=True)
        self.init_offset()

    def init_offset(self):
        with torch.no_grad():
            self.conv_offset.weight.zero_()
            self.conv_offset.bias.zero_()

    def init_weights(self):
        super().init_weights()
        if hasattr(self, 'conv_offset'):
            self.init_offset()

    def forward(self, x):
        return self._forward(x, self.conv_offset(x), None, True)

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                              error_msgs):
        version = local_metadata.get('version', None)
        if version is None or version < 2:
            for leaf in ('weight', 'bias'):
                old, new = f'{prefix[:-1]}_offset.{leaf}', f'{prefix}conv_offset.{leaf}'
                if new not in state_dict and old in state_dict:
                    state_dict[new] = state_dict.pop(old)
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                                      error_msgs)
