"""Fused GroupNorm(+ReLU) for the cost-volume aggregation stacks: one HIP
reduction pass + one apply pass (``dfm_group_norm_fwd/bwd``) instead of torch's
GroupNorm kernel followed by a separate ReLU.

``HipGroupNorm`` subclasses ``nn.GroupNorm`` (same parameters, same
``state_dict`` keys), so it drops into ``ConvModule`` / ``hourglass`` without
touching checkpoints.
"""
import torch
from torch import nn

from . import _capi
from .derived import Derived
from ._launch import DTYPES, STREAM, WS, launch, nonempty


_f32_cache = Derived(capacity=1024)


def _f32_params(weight, bias):
    """fp32 copies of the affine parameters the kernels read; bf16 modules would otherwise launch two
    conversion kernels per call (36 per DfMBackbone forward).  Cached per parameter and version."""
    if weight.dtype == torch.float32 and bias.dtype == torch.float32:
        return weight.detach().contiguous(), bias.detach().contiguous()
    return _f32_cache.get((id(weight), id(bias)), (weight, bias), lambda: (
        weight.detach().float().contiguous(), bias.detach().float().contiguous()))


_XMASK = True   # False: the backward reads the ReLU mask from the kept output, as the fused-residual case does (tests)


class _GroupNormFn(torch.autograd.Function):

    @staticmethod
    def forward(ctx, x, weight, bias, groups, eps, relu, partials=None, residual=None, stats_out=None):
        lib = _capi.lib()
        device = x.device
        n, c = x.shape[:2]
        # channels-last input (what the NDHWC convolutions hand over) stays channels-last
        vec = 16 // x.element_size()
        cl = (x.dim() in (4, 5) and c % vec == 0 and c <= 256 and ((c // vec) & (c // vec - 1)) == 0
              and not x.is_contiguous()
              and x.is_contiguous(memory_format=torch.channels_last_3d if x.dim() == 5
                                  else torch.channels_last))
        if not cl:
            x = x.contiguous()
        spatial = x.numel() // (n * c)
        y = torch.empty_like(x)  # preserves the memory format
        mean = torch.empty(n * groups, dtype=torch.float32, device=device)
        rstd = torch.empty_like(mean)
        w32, b32 = _f32_params(weight, bias)
        nbytes = lib.dfm_group_norm_workspace_bytes(n, c, spatial, groups)
        fused_res = residual is not None and cl and residual.dtype == x.dtype and \
            residual.shape == x.shape and residual.stride() == x.stride()
        rp = residual if fused_res else None
        if partials is not None:
            # statistics came from the producer (MFMA conv epilogue): normalisation pass only
            assert cl and partials.shape[:2] == (n, groups) and partials.is_contiguous()
            launch('dfm_group_norm_apply_channels_last_res', n, c, spatial, groups, eps, DTYPES[x.dtype],
                   int(relu and (fused_res or residual is None)), x, w32, b32, rp, y, mean, rstd, partials,
                   partials.shape[2], WS, STREAM, ws_bytes=nbytes)
        elif cl:
            launch('dfm_group_norm_fwd_channels_last_res', n, c, spatial, groups, eps, DTYPES[x.dtype],
                   int(relu and (fused_res or residual is None)), x, w32, b32, rp, y, mean, rstd, WS, STREAM,
                   ws_bytes=nbytes)
        else:
            launch('dfm_group_norm_fwd', n, c, spatial, groups, eps, DTYPES[x.dtype], int(relu and residual is None),
                   x, w32, b32, y, mean, rstd, WS, STREAM, ws_bytes=nbytes)
        unfused = residual is not None and not fused_res
        if unfused:
            # a residual the kernel does not fuse (NCDHW, mismatched strides, another dtype, a broadcast one): plain
            # torch ops behind the kernel, which ran without ReLU.  Their result may have another dtype (an fp32
            # residual promotes a bf16 y) or layout than x, so it is never handed to a kernel as a ReLU mask: the
            # backward applies the mask in torch as well and calls the kernel without ReLU
            y = y + residual
            if relu:
                y = torch.relu_(y)
        # y = relu(gn(x)) of a channels-last tensor without a residual: the backward recomputes the ReLU mask from x
        # (dfm_group_norm_bwd_channels_last_xmask) -- y is not kept for it, one activation less per layer in the graph
        xmask = bool(relu) and cl and residual is None and _XMASK
        ctx.save_for_backward(x, y if (relu and not xmask) else x, mean, rstd, w32, b32)
        ctx.cfg = (groups, bool(relu), weight.dtype, bias.dtype, cl, residual is not None, xmask, unfused)
        if stats_out is not None:  # (mean, rstd) per (sample, group): HipBatchNorm3d's running statistics
            stats_out.append((mean, rstd))
        return y

    @staticmethod
    def backward(ctx, gy):
        x, y, mean, rstd, w32, b32 = ctx.saved_tensors
        groups, relu, wdt, bdt, cl, has_res, xmask, unfused = ctx.cfg
        lib = _capi.lib()
        device = x.device
        n, c = x.shape[:2]
        spatial = x.numel() // (n * c)
        want_res = has_res and ctx.needs_input_grad[7]
        gres = None
        if unfused:
            # y = relu?(gn(x) + residual) in torch ops: the mask of that y (its own dtype and layout) in torch; what is
            # left is the backward of a GroupNorm without ReLU.  The residual's gradient is the masked incoming one as
            # it is (autograd sums it over a broadcast residual's extent and casts it to the residual's dtype)
            if relu:
                gy = gy * (y > 0).to(gy.dtype)
                relu = False
            gres = gy if want_res else None
        # (the channels-last kernels overwrite the parameter gradients: no zero fill -- 2 launches per layer saved)
        gw = (torch.empty if cl else torch.zeros)(c, dtype=torch.float32, device=device)
        gb = (torch.empty if cl else torch.zeros)(c, dtype=torch.float32, device=device)
        nbytes = lib.dfm_group_norm_workspace_bytes(n, c, spatial, groups)
        if cl:
            # channels-last kernels: no layout round trip; the masked gradient of a fused residual
            # input is a second output of the same pass
            fmt = torch.channels_last_3d if x.dim() == 5 else torch.channels_last
            gy = gy.to(x.dtype).contiguous(memory_format=fmt)
            gx = torch.empty_like(x)
            if want_res and relu:
                gres = torch.empty_like(x)
            if xmask:
                launch('dfm_group_norm_bwd_channels_last_xmask', n, c, spatial, groups, DTYPES[x.dtype], gy, x, mean,
                       rstd, w32, b32, gx, gw, gb, WS, STREAM, ws_bytes=nbytes)
                return gx, gw.to(wdt), gb.to(bdt), None, None, None, None, None, None
            launch('dfm_group_norm_bwd_channels_last', n, c, spatial, groups, DTYPES[x.dtype], int(relu), gy, x,
                   y if relu else None, mean, rstd, w32, gx, gres if relu else None, gw, gb, WS, STREAM,
                   ws_bytes=nbytes)
            if want_res and not relu and not unfused:
                gres = gy
            return gx, gw.to(wdt), gb.to(bdt), None, None, None, None, gres, None
        gy = gy.contiguous().to(x.dtype)
        gx = torch.empty_like(x)
        launch('dfm_group_norm_bwd', n, c, spatial, groups, DTYPES[x.dtype], int(relu), gy, x, y if relu else None,
               mean, rstd, w32, gx, gw, gb, WS, STREAM, ws_bytes=nbytes)
        return gx, gw.to(wdt), gb.to(bdt), None, None, None, None, gres, None


def group_norm(x, num_groups, weight, bias, eps=1e-5, relu=False, partials=None, residual=None):
    """torch.nn.functional.group_norm(+relu) on the GPU through the fused kernels.
    ``partials`` (N, groups, splits, 3): count / mean / M2 moment partials of ``x`` from its
    producer (``MfmaConv3d.forward_with_stats``); the statistics pass over ``x`` is skipped.
    ``residual``: added after the affine map, before the ReLU (fused into the channels-last pass)."""
    if not x.is_cuda or x.dtype not in DTYPES:
        raise RuntimeError('fused group_norm needs a float32/bfloat16 GPU tensor '
                           '(depth-from-motion_amd has no CPU path)')
    return _GroupNormFn.apply(x, weight, bias, int(num_groups), float(eps), bool(relu), partials, residual)


_cpu_reference = False


def allow_cpu_reference(flag=True):
    """TEST-ONLY switch: lets HipGroupNorm run torch's nn.GroupNorm on CPU tensors so that the
    module wiring / the gloo data-parallel glue can be exercised on a box without a GPU
    (tests/test_distributed_cpu.py, tests/test_modules.py).  Off by default: the product has no
    CPU path and a CPU tensor raises.  Returns the previous setting."""
    global _cpu_reference
    prev, _cpu_reference = _cpu_reference, bool(flag)
    return prev


class HipGroupNorm(nn.GroupNorm):
    """nn.GroupNorm whose forward/backward run in the fused HIP kernels (float32 / bfloat16,
    affine).  Anything else raises -- there is no silent eager fallback: a CPU tensor, or a GPU
    tensor the kernels do not cover (fp16, affine=False), is an error.  (Tests that exercise
    module wiring on a CPU-only box opt in with ``allow_cpu_reference(True)``.)"""

    def forward(self, x, relu=False, partials=None, residual=None):
        if x.is_cuda:
            if x.dtype not in DTYPES or not self.affine:
                raise RuntimeError(
                    f'HipGroupNorm: unsupported GPU input (dtype {x.dtype}, affine={self.affine}); '
                    'the fused kernels cover float32 / bfloat16 with affine parameters')
            return group_norm(x, self.num_groups, self.weight, self.bias, self.eps, relu, partials, residual)
        if not _cpu_reference:
            raise RuntimeError('HipGroupNorm got a CPU tensor: depth-from-motion_amd has no CPU path '
                               '(tests opt in with group_norm.allow_cpu_reference(True))')
        y = super().forward(x)
        if residual is not None:
            y = y + residual
        return torch.relu_(y) if relu else y


def _channels_ok(x):
    vec = 16 // x.element_size() if x.dtype in DTYPES else 0
    c = x.shape[1] if x.dim() >= 2 else 0
    return bool(vec) and 0 < c <= 256 and c % vec == 0 and ((c // vec) & (c // vec - 1)) == 0


def sync_batch_norm_eligible(bn, x):
    """Whether an nn.SyncBatchNorm at world size > 1 runs ``x`` through the fused cross-rank kernels.  The answer must
    be the same on every rank -- a rank that took torch's SyncBatchNorm while another took this path would issue
    different collectives and hang the job -- so it looks only at what the ranks share: the module, dtype, C, rank
    and channels-last-ness read from the channel stride (1 in a channels-last tensor whatever its batch size, spatial
    extent or storage offset, an empty shard included; H * W in an NCHW one).  Never the batch size, spatial extent,
    contiguity or alignment of the local shard; those are fixed by a copy instead.  (An NCHW map of 1 x 1 pixels has
    channel stride 1 as well: a model whose SyncBatchNorm inputs are NCHW must not hand one rank a 1 x 1 map.)"""
    return bool(bn.training and bn.affine and bn.track_running_stats and x.dim() in (4, 5) and _channels_ok(x) and
                x.stride(1) == 1)


def _sync_world(bn):
    """the process group of a SyncBatchNorm that needs statistics across ranks, else None"""
    if isinstance(bn, nn.SyncBatchNorm) and torch.distributed.is_available() and torch.distributed.is_initialized() \
            and torch.distributed.get_world_size() > 1:
        return bn.process_group if bn.process_group is not None else torch.distributed.group.WORLD
    return None


def _memory_format(x):
    return torch.channels_last_3d if x.dim() == 5 else torch.channels_last


def _dense(t, fmt):
    """t channels-last contiguous and 16-byte aligned (a copy only when it is not: a slice, an odd storage offset)"""
    t = t.contiguous(memory_format=fmt)
    if t.data_ptr() % 16:
        t = t.clone(memory_format=fmt)
    return t


def bn_stats(x):
    """dfm_batch_norm_stats_channels_last: this rank's payload, fp32 (C, 3) (count, mean, M2) per channel, of a
    channels-last contiguous, 16-byte aligned (N, C, *spatial) tensor (N may be 0)"""
    lib = _capi.lib()
    c, rows = x.shape[1], x.numel() // x.shape[1]
    out = torch.empty(c, 3, dtype=torch.float32, device=x.device)
    launch('dfm_batch_norm_stats_channels_last', c, rows, DTYPES[x.dtype], nonempty(x), out, WS, STREAM,
           ws_bytes=lib.dfm_batch_norm_workspace_bytes(c, rows))
    return out


def bn_apply_gathered(x, gathered, w32, b32, eps, relu, residual=None):
    """dfm_batch_norm_apply_gathered_channels_last: gathered (world, C, 3) rank-ordered payloads [device] ->
    (y, mean, rstd, moments); y = relu?(bn(x) + residual), moments (C, 3) the global (count, mean, M2)"""
    c, rows = x.shape[1], x.numel() // x.shape[1]
    y = torch.empty_like(x)
    mean = torch.empty(c, dtype=torch.float32, device=x.device)
    rstd = torch.empty_like(mean)
    moments = torch.empty(c, 3, dtype=torch.float32, device=x.device)
    gathered = gathered.contiguous()
    launch('dfm_batch_norm_apply_gathered_channels_last', c, rows, gathered.shape[0], float(eps), DTYPES[x.dtype],
           int(relu), nonempty(x), w32, b32, nonempty(residual), gathered, nonempty(y), mean, rstd, moments, STREAM)
    return y, mean, rstd, moments


def bn_bwd_reduce(gy, x, y, mean, rstd, w32, b32, relu):
    """dfm_batch_norm_bwd_reduce_channels_last: this rank's (2, C) sums (row 0 sum(dy') = grad_bias, row 1
    sum(dy' * xhat) = grad_weight).  relu with y None: the mask is recomputed from x."""
    lib = _capi.lib()
    c, rows = x.shape[1], x.numel() // x.shape[1]
    sums = torch.empty(2, c, dtype=torch.float32, device=x.device)
    launch('dfm_batch_norm_bwd_reduce_channels_last', c, rows, DTYPES[x.dtype], int(relu), nonempty(gy), nonempty(x),
           nonempty(y), mean, rstd, w32, b32, sums, WS, STREAM, ws_bytes=lib.dfm_batch_norm_workspace_bytes(c, rows))
    return sums


def bn_bwd_apply(gy, x, y, mean, rstd, w32, b32, relu, sums, moments, want_gres=False):
    """dfm_batch_norm_bwd_apply_channels_last: (grad_x, grad_residual or None) from the rank-summed (2, C) sums and
    the global count moments[0, 0]"""
    lib = _capi.lib()
    c, rows = x.shape[1], x.numel() // x.shape[1]
    gx = torch.empty_like(x)
    gres = torch.empty_like(x) if want_gres else None
    launch('dfm_batch_norm_bwd_apply_channels_last', c, rows, DTYPES[x.dtype], int(relu), nonempty(gy), nonempty(x),
           nonempty(y), mean, rstd, w32, b32, sums.contiguous(), moments, nonempty(gx), nonempty(gres), WS, STREAM,
           ws_bytes=lib.dfm_batch_norm_workspace_bytes(c, rows))
    return gx, gres


def update_running_stats(bn, mean, moments):
    """torch's batch_norm_gather_stats_with_counts: unbiased variance over the global count, momentum or the
    cumulative average, num_batches_tracked += 1 -- on the device, from the global moments"""
    with torch.no_grad():
        m = moments[:, 0]
        var = moments[:, 2] / (m - 1).clamp_min(1)
        bn.num_batches_tracked += 1
        f = bn.momentum if bn.momentum is not None else 1.0 / float(bn.num_batches_tracked)
        bn.running_mean.mul_(1 - f).add_(mean.to(bn.running_mean.dtype), alpha=f)
        bn.running_var.mul_(1 - f).add_(var.to(bn.running_var.dtype), alpha=f)


def _gather_payload(local, group):
    """(world, C, 3) payloads of every rank in rank order: all_gather_into_tensor on the device (NCCL / RCCL); through
    host tensors on gloo (C x 3 floats), as torch's SyncBatchNorm does"""
    dist = torch.distributed
    world = dist.get_world_size(group)
    if dist.get_backend(group) == 'gloo':
        h = local.cpu()
        parts = [torch.empty_like(h) for _ in range(world)]
        dist.all_gather(parts, h, group=group)
        return torch.stack(parts).to(local.device)
    out = torch.empty((world,) + tuple(local.shape), dtype=local.dtype, device=local.device)
    dist.all_gather_into_tensor(out, local, group=group)
    return out


def _sum_payload(sums, group):
    """the (2, C) sums added over the ranks (a new tensor: the local ones stay the parameter gradients)"""
    dist = torch.distributed
    if dist.get_backend(group) == 'gloo':
        h = sums.cpu()
        dist.all_reduce(h, op=dist.ReduceOp.SUM, group=group)
        return h.to(sums.device)
    out = sums.clone()
    dist.all_reduce(out, op=dist.ReduceOp.SUM, group=group)
    return out


class _SyncBatchNormFn(torch.autograd.Function):
    """nn.SyncBatchNorm's training forward / backward at world size > 1 through the fused channels-last kernels:
    local statistics -> one all-gather of the (C, 3) payloads -> apply; local gradient sums -> one all-reduce of the
    (2, C) sums -> apply.  The collectives are blocking and issued from the host in program order, one per forward
    and one per backward of every layer, as torch's SyncBatchNorm issues its own."""

    @staticmethod
    def forward(ctx, x, weight, bias, residual, bn, relu, group):
        w32, b32 = _f32_params(weight, bias)
        fused_res = residual is not None and residual.shape == x.shape
        res = _dense(residual.to(x.dtype), _memory_format(x)) if fused_res else None
        gathered = _gather_payload(bn_stats(x), group)
        y, mean, rstd, moments = bn_apply_gathered(x, gathered, w32, b32, bn.eps,
                                                   relu and (fused_res or residual is None), res)
        if residual is not None and not fused_res:   # a broadcast residual: plain torch ops
            y = y + residual
            if relu:
                y = torch.relu_(y)
        update_running_stats(bn, mean, moments)
        xmask = bool(relu) and residual is None and _XMASK
        ctx.save_for_backward(x, y if (relu and not xmask) else x, mean, rstd, w32, b32, moments)
        ctx.cfg = (bool(relu), weight.dtype, bias.dtype, residual.dtype if residual is not None else None, xmask,
                   group)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, y, mean, rstd, w32, b32, moments = ctx.saved_tensors
        relu, wdt, bdt, rdt, xmask, group = ctx.cfg
        gy = _dense(gy.to(x.dtype), _memory_format(x))
        ym = None if (xmask or not relu) else y
        sums = bn_bwd_reduce(gy, x, ym, mean, rstd, w32, b32, relu)
        total = _sum_payload(sums, group)
        want_res = rdt is not None and ctx.needs_input_grad[3]
        gx, gres = bn_bwd_apply(gy, x, ym, mean, rstd, w32, b32, relu, total, moments, want_res and relu)
        if want_res and not relu:
            gres = gy
        if gres is not None:
            gres = gres.to(rdt)
        return gx, sums[1].to(wdt), sums[0].to(bdt), gres, None, None, None


def batch_norm_train_channels_last(bn, x, relu=False, residual=None):
    """Training-mode BatchNorm (nn.BatchNorm2d / 3d / SyncBatchNorm) of a channels-last GPU tensor through the fused
    GroupNorm kernels, or None when it does not apply.  The batch statistics of a channels-last (N, C, *spatial)
    tensor are the per-channel GroupNorm statistics of the same memory viewed as ONE sample (1, C, N * s0, ...):
    normalisation (+ residual) (+ ReLU) is one statistics pass and one apply pass, the backward the channels-last
    GroupNorm backward; running statistics are updated as torch does (unbiased variance, momentum / cumulative
    average).  y = relu?(bn(x) + residual).

    An nn.SyncBatchNorm in a process group of more than one rank runs the same passes split where the ranks exchange
    their statistics (_SyncBatchNormFn): one all-gather of a (C, 3) payload per forward, one all-reduce of a (C, 2)
    payload per backward, over ``bn.process_group`` (WORLD if None).  Whether it does is decided by
    ``sync_batch_norm_eligible`` from what every rank shares, never from the local shard (an empty one included)."""
    group = _sync_world(bn)
    if group is not None:
        if not (x.is_cuda and sync_batch_norm_eligible(bn, x)):
            return None   # the same answer on every rank: torch's SyncBatchNorm everywhere
        fmt = _memory_format(x)
        return _SyncBatchNormFn.apply(_dense(x, fmt), bn.weight, bn.bias, residual, bn, bool(relu), group)
    vec = 16 // x.element_size() if x.dtype in DTYPES else 0
    c = x.shape[1]
    fmt = torch.channels_last_3d if x.dim() == 5 else torch.channels_last
    if not (bn.training and x.is_cuda and vec and x.dim() in (4, 5) and bn.affine and bn.track_running_stats and
            c % vec == 0 and c <= 256 and ((c // vec) & (c // vec - 1)) == 0 and
            not x.is_contiguous() and x.is_contiguous(memory_format=fmt)):
        return None

    def one_sample(t):   # (N, C, s0, ...) channels-last -> (1, C, N * s0, ...) channels-last, the same memory
        n = t.shape[0]
        perm = (0,) + tuple(range(2, t.dim())) + (1,)
        back = (0, t.dim() - 1) + tuple(range(1, t.dim() - 1))
        v = t.permute(*perm)
        return v.reshape(1, n * v.shape[1], *v.shape[2:]).permute(*back)

    res = None
    if residual is not None:
        res = one_sample(residual if residual.is_contiguous(memory_format=fmt) else residual.contiguous(memory_format=fmt))
    stats = []
    y = _GroupNormFn.apply(one_sample(x), bn.weight, bn.bias, c, float(bn.eps), bool(relu), None, res, stats)
    mean, rstd = stats[0]
    with torch.no_grad():
        m = x.numel() // c
        var = (1.0 / (rstd * rstd) - bn.eps).clamp_min_(0.0) * (m / max(m - 1, 1))  # unbiased
        bn.num_batches_tracked += 1
        f = bn.momentum if bn.momentum is not None else 1.0 / float(bn.num_batches_tracked)
        bn.running_mean.mul_(1 - f).add_(mean.to(bn.running_mean.dtype), alpha=f)
        bn.running_var.mul_(1 - f).add_(var.to(bn.running_var.dtype), alpha=f)
    perm = (0,) + tuple(range(2, x.dim())) + (1,)
    back = (0, x.dim() - 1) + tuple(range(1, x.dim() - 1))
    return y.permute(*perm).reshape(x.shape[0], *x.shape[2:], c).permute(*back)


class HipBatchNorm3d(nn.BatchNorm3d):
    """nn.BatchNorm3d (same parameters, buffers and ``state_dict`` keys) whose TRAINING forward /
    backward on channels-last GPU tensors run in the fused HIP kernels: the batch statistics of a
    channels-last (N, C, D, H, W) tensor are the per-channel GroupNorm statistics of the same memory
    viewed as ONE sample (1, C, N*D, H, W), so normalisation (+ residual) (+ ReLU) is one statistics
    pass and one apply pass, and the backward the channels-last GroupNorm backward (torch's
    BatchNorm backward on this layout: 2.3 ms per layer of the voxel neck, 42 % of its training step).
    Eval mode / other inputs: torch (the necks fold eval-mode BatchNorm into the conv epilogue anyway).
    ``forward(x, relu=False, residual=None)``: y = relu?(bn(x) + residual)."""

    def _fusable(self, x):
        vec = 16 // x.element_size() if x.dtype in DTYPES else 0
        c = x.shape[1]
        return (self.training and x.is_cuda and vec and x.dim() == 5 and self.affine and
                self.track_running_stats and c % vec == 0 and c <= 256 and ((c // vec) & (c // vec - 1)) == 0 and
                not x.is_contiguous() and x.is_contiguous(memory_format=torch.channels_last_3d))

    @staticmethod
    def _as_one_sample(t):
        N, C, D, H, W = t.shape
        return t.permute(0, 2, 3, 4, 1).reshape(1, N * D, H, W, C).permute(0, 4, 1, 2, 3)

    def forward(self, x, relu=False, residual=None):
        if not self._fusable(x):
            y = super().forward(x)
            if residual is not None:
                y = y + residual
            return torch.relu_(y) if relu else y
        return batch_norm_train_channels_last(self, x, relu, residual)
