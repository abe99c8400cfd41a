"""The optimizer step on the HIP path: global-norm gradient clipping and AdamW with fp32 master weights.

Both shipped configs end an iteration in mmcv's ``OptimizerHook``: ``clip_grad_norm_(params, max_norm=35,
norm_type=2)`` and then ``torch.optim.AdamW.step()``.  Here that is ONE small host-to-device copy and TWO kernel
launches whatever the number of parameters (include/dfm_hip_optim.h states the arithmetic, which is torch's
single-tensor AdamW operation for operation): the host writes one table row per parameter that has a gradient --
addresses, element count, type, and that parameter's scalars, computed in double as torch computes them and rounded
once -- and a chunk table that maps workgroups to pieces of tensors.

  * ``FusedAdamW``: a ``torch.optim.Optimizer``.  A parameter that is not fp32 (``enable_fast_path`` makes the
    convolution weights bf16) gets an fp32 ``master`` in its state; the update runs on the master and the parameter
    receives its bf16 rounding.  Without a master a bf16 weight stalls: at the configs' learning rates most updates
    are below half a bf16 ulp of the weight and round away.
  * ``clip_grad_norm_``: the drop-in for ``torch.nn.utils.clip_grad_norm_``, two launches.
  * The kernels write parameters through raw pointers, so ``step()`` bumps the version counter of every parameter it
    wrote: packed weights and every other derived state are cached on ``(_version, data_ptr, device)`` (derived.py).

Limits: the state of one rank on one device, fp32 and bf16 parameters, norm type 2, no hipGraph capture (the table
comes from host memory every step).  Build the optimizer AFTER ``enable_fast_path``: the masters are taken from the
parameters as they are at the first step, and a parameter whose type changed later is refused.
"""
from collections import defaultdict
from itertools import chain

import numpy as np
import torch

from . import _capi
from ._launch import DTYPES, STREAM, launch

__all__ = ['FusedAdamW', 'clip_grad_norm_', 'counters', 'adamw_scalars', 'chunk_table', 'build_table']

CHUNK = _capi.OPTIM_CHUNK
ROW = np.dtype(_capi.OptimTensor)          # one table row, field for field the C struct
_SCALARS = ('decay', 'step_size', 'bc2_sqrt', 'lerp_weight', 'beta2', 'one_minus_beta2', 'eps')
_REFUSED = ('amsgrad', 'maximize', 'capturable', 'differentiable')
_STAGING_SLOTS = 4

_COUNTERS = {'kernel_launches': 0, 'copies': 0, 'host_waits': 0}


def counters(reset=False):
    """kernel launches, host-to-device table copies and host waits (on a staging buffer whose previous copy had not
    run yet) made by this module so far; ``reset=True`` zeroes them after reading.  Not counted: torch's own copy of a
    gradient whose layout differs from its parameter's."""
    out = dict(_COUNTERS)
    if reset:
        for k in _COUNTERS:
            _COUNTERS[k] = 0
    return out


# ---------------------------------------------------------------------------------------------------------
# the host side of the tables: pure, runs without a GPU
# ---------------------------------------------------------------------------------------------------------
def adamw_scalars(lr, beta1, beta2, eps, weight_decay, t):
    """the per-tensor scalars of one step as torch's ``_single_tensor_adam`` computes them, in double (Python floats),
    in the order of the table's float fields; ``t`` is the step count after the increment.  The table rounds each
    once to fp32."""
    bias_correction1 = 1 - beta1 ** t
    bias_correction2 = 1 - beta2 ** t
    return (1 - lr * weight_decay, lr / bias_correction1, bias_correction2 ** 0.5, 1 - beta1, beta2, 1 - beta2, eps)


def chunk_table(numels):
    """(num_chunks, 2) int32 of (tensor, chunk): tensor i owns ceil(numel_i / CHUNK) consecutive rows"""
    counts = (np.asarray(numels, dtype=np.int64) + (CHUNK - 1)) // CHUNK
    if counts.size and int(counts.max()) > 2 ** 31 - 1:
        raise ValueError('a tensor of more than 2^31 - 1 chunks')
    total = int(counts.sum())
    tensor = np.repeat(np.arange(len(counts), dtype=np.int64), counts)
    chunk = np.arange(total, dtype=np.int64) - np.repeat(np.cumsum(counts) - counts, counts)
    return np.stack([tensor, chunk], 1).astype(np.int32)


def build_table(entries, out=None, static=None):
    """``entries``: one ``(param or None, grad, state or None, scalars or None)`` per tensor -> the table, a structured
    array of ``ROW`` (written into ``out`` when given).  Without a parameter only grad, numel and dtype are filled: what
    the norm and scale kernels read.  ``static``: a table built earlier from the same parameters and states; then only
    what changes from step to step is written, the gradients' addresses and the scalars."""
    table = np.zeros(len(entries), dtype=ROW) if out is None else out
    stepping = bool(entries) and entries[0][0] is not None
    if static is not None:
        table[...] = static
    else:
        table['numel'] = [g.numel() for _, g, _, _ in entries]
        table['dtype'] = [DTYPES[g.dtype] for _, g, _, _ in entries]
        table['reserved'] = 0
        table['reserved_f'] = 0
        if stepping:
            table['param'] = [p.data_ptr() for p, _, _, _ in entries]
            table['exp_avg'] = [s['exp_avg'].data_ptr() for _, _, s, _ in entries]
            table['exp_avg_sq'] = [s['exp_avg_sq'].data_ptr() for _, _, s, _ in entries]
            table['master'] = [s['master'].data_ptr() if 'master' in s else 0 for _, _, s, _ in entries]
        else:
            for name in ('param', 'exp_avg', 'exp_avg_sq', 'master') + _SCALARS:
                table[name] = 0
    table['grad'] = [g.data_ptr() for _, g, _, _ in entries]
    if stepping:
        scalars = np.array([sc for _, _, _, sc in entries], dtype=np.float64)     # rounded once, on assignment
        for k, name in enumerate(_SCALARS):
            table[name] = scalars[:, k]
    return table


def _is_dense(t):
    """non-overlapping and dense: its elements fill one run of storage, in some order"""
    if t.is_contiguous():
        return True
    if t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last):
        return True
    if t.dim() == 5 and t.is_contiguous(memory_format=torch.channels_last_3d):
        return True
    from torch._prims_common import is_non_overlapping_and_dense
    return bool(is_non_overlapping_and_dense(t))


def _in_layout_of(t, p, dtype):
    """``t`` as a ``dtype`` tensor with ``p``'s strides on ``p``'s device (``p`` is dense); ``t`` itself if it is"""
    if t.dtype == dtype and t.device == p.device and t.stride() == p.stride() and t.shape == p.shape:
        return t
    return torch.empty_like(p, dtype=dtype, memory_format=torch.preserve_format).copy_(t)


# ---------------------------------------------------------------------------------------------------------
# the device side: one set of buffers per (device, stream)
# ---------------------------------------------------------------------------------------------------------
class _Buffers:
    """Pinned staging buffers, rotated behind events, and the device copies of the tables and partials.

    The copy of step k may not have executed when the host writes the table of step k + 1, so a staging buffer is
    written again only after the event recorded behind its last copy has completed; with ``_STAGING_SLOTS`` buffers in
    rotation that is the case in steady state without waiting (``counters()['host_waits']`` counts the exceptions).
    The device buffers are reused without events: copies and kernels are ordered by the stream."""
    _all = {}

    @classmethod
    def of(cls, index, stream):
        key = (index, stream)
        b = cls._all.get(key)
        if b is None:
            b = cls._all[key] = cls(index)
        return b

    def __init__(self, index):
        self.device = torch.device('cuda', index)
        self.slots = [[None, None] for _ in range(_STAGING_SLOTS)]
        self.next = 0
        self.tables = None
        self.partials = None

    def stage(self, nbytes):
        """a pinned uint8 buffer of at least ``nbytes`` that no pending copy reads, and its slot"""
        slot = self.slots[self.next]
        self.next = (self.next + 1) % _STAGING_SLOTS
        if slot[1] is not None and not slot[1].query():
            slot[1].synchronize()
            _COUNTERS['host_waits'] += 1
        if slot[0] is None or slot[0].numel() < nbytes:
            slot[0] = torch.empty(max(2 * nbytes, 1 << 16), dtype=torch.uint8, pin_memory=True)
        return slot

    def upload(self, slot, nbytes):
        """the first ``nbytes`` of the slot's buffer -> the device table buffer (one async copy, current stream)"""
        if self.tables is None or self.tables.numel() < nbytes:
            self.tables = torch.empty(max(2 * nbytes, 1 << 16), dtype=torch.uint8, device=self.device)
        dev = self.tables[:nbytes]
        dev.copy_(slot[0][:nbytes], non_blocking=True)
        if slot[1] is None:
            slot[1] = torch.cuda.Event()
        slot[1].record()
        _COUNTERS['copies'] += 1
        return dev

    def partial_sums(self, n):
        if self.partials is None or self.partials.numel() < n:
            self.partials = torch.empty(max(2 * n, 1024), dtype=torch.float32, device=self.device)
        return self.partials


def _upload_tables(entries, index, static=None, chunks=None):
    """fill and copy both tables -> (buffers, table view, chunk view, number of chunks); under the device guard.
    ``static`` / ``chunks``: what an earlier step with the same parameters built (``build_table``, ``chunk_table``)"""
    if chunks is None:
        chunks = chunk_table([g.numel() for _, g, _, _ in entries])
    rows, n = len(entries), len(chunks)
    row_bytes, nbytes = rows * ROW.itemsize, rows * ROW.itemsize + n * 8
    bufs = _Buffers.of(index, torch.cuda.current_stream(index).cuda_stream)
    slot = bufs.stage(nbytes)
    host = slot[0].numpy()
    build_table(entries, out=host[:row_bytes].view(ROW), static=static)
    host[row_bytes:nbytes].view(np.int32).reshape(n, 2)[...] = chunks
    dev = bufs.upload(slot, nbytes)
    return bufs, dev[:row_bytes], dev[row_bytes:], n


def _no_cpu(what):
    return RuntimeError(f'{what} must live on the GPU: depth-from-motion_amd has no CPU path (the HIP kernels are the '
                        'product; the CPU oracle is test-only)')


def _one_device(tensors):
    devices = sorted({str(t.device) for t in tensors})
    if len(devices) != 1:
        raise RuntimeError(f'the parameters of one step live on one GPU, got {", ".join(devices)}: the optimizer '
                           'state is that of one rank, depth-from-motion_amd has no cross-device kernels')
    return tensors[0].device.index


def _check_clip(grad_clip):
    """the configs' ``grad_clip`` dict -> max_norm (None: no clipping)"""
    if grad_clip is None:
        return None
    clip = dict(grad_clip)
    if 'max_norm' not in clip:
        raise ValueError(f'grad_clip needs max_norm, got {grad_clip!r}')
    max_norm = float(clip.pop('max_norm'))
    if float(clip.pop('norm_type', 2)) != 2.0:
        raise ValueError('grad_clip: only norm_type=2 is built (the configs\' own)')
    if clip.pop('error_if_nonfinite', False):
        raise ValueError('grad_clip: error_if_nonfinite=True needs the norm on the host every step; it is not built')
    clip.pop('foreach', None)
    if clip:
        raise ValueError(f'grad_clip: unknown keys {sorted(clip)}')
    return max_norm


class _Record:
    """What ``step()`` remembers of one parameter between steps, so that the host side of a steady-state step is a
    few identity and address comparisons per parameter.  When one of them fails -- the first step, a replaced state, a
    parameter whose storage or type changed -- the parameter goes through every check and its state is set up again."""
    __slots__ = ('group', 'p', 'dtype', 'address', 'strides', 'state', 'step', 'm', 'v', 'w', 'is_cuda')

    def __init__(self, group, p):
        self.group, self.p, self.state = group, p, None

    def current(self, state):
        p = self.p
        return (state is self.state and p.dtype is self.dtype and p.data_ptr() == self.address and
                state.get('step') is self.step and state.get('exp_avg') is self.m and
                state.get('exp_avg_sq') is self.v and state.get('master') is self.w)


class FusedAdamW(torch.optim.Optimizer):
    """``torch.optim.AdamW`` (decoupled weight decay, no amsgrad) with the global-norm clip fused in and fp32 master
    weights, one table copy and two kernel launches a step (one without clipping).

    ``grad_clip``: the configs' ``dict(max_norm=35., norm_type=2)`` or None.  ``master_weights=False`` steps a bf16
    parameter as torch does, rounding every update to bf16.  ``step(zero_grads=True)`` also zeroes the gradients it has
    read, in place.  After a clipped step ``grad_norm`` is the 0-dim fp32 DEVICE tensor of the total norm (it is never
    fetched here; ``float(opt.grad_norm)`` waits for the stream) and ``.grad`` is left UNSCALED.

    State per parameter: ``step`` (CPU fp32 0-dim, as torch keeps it), ``exp_avg``, ``exp_avg_sq`` (fp32) and, for a
    parameter that is not fp32, ``master`` (fp32).  For fp32 parameters that is torch's AdamW state key for key: a
    checkpoint of either loads into the other."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, grad_clip=None,
                 master_weights=True, **unsupported):
        for name in _REFUSED:
            if unsupported.pop(name, False):
                raise ValueError(f'FusedAdamW: {name} is not built')
        for name in ('foreach', 'fused', 'decoupled_weight_decay'):
            unsupported.pop(name, None)
        if unsupported:
            raise TypeError(f'FusedAdamW: unexpected arguments {sorted(unsupported)}')
        if not 0.0 <= lr:
            raise ValueError(f'Invalid learning rate: {lr}')
        if not 0.0 <= eps:
            raise ValueError(f'Invalid epsilon value: {eps}')
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f'Invalid betas: {betas}')
        if not 0.0 <= weight_decay:
            raise ValueError(f'Invalid weight_decay value: {weight_decay}')
        self.max_norm = _check_clip(grad_clip)
        self.grad_clip = None if grad_clip is None else dict(grad_clip)
        self.master_weights = bool(master_weights)
        self.grad_norm = None
        # torch's AdamW keeps these keys in every group; mirroring them lets a state_dict go either way
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False,
                        foreach=None, capturable=False, differentiable=False, fused=None, decoupled_weight_decay=True)
        super().__init__(params, defaults)

    # -- groups and state ----------------------------------------------------------------------------------
    def _built_dtypes(self):
        built = self.__dict__.get('_built')
        if built is None:
            built = self.__dict__['_built'] = {}
        return built

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        self._records = self._plan = None
        self._check_groups()

    def _check_groups(self):
        built = self._built_dtypes()
        for group in self.param_groups:
            for name in _REFUSED:
                if group.get(name, False):
                    raise ValueError(f'FusedAdamW: {name} is not built')
            for p in group['params']:
                if p.dtype not in DTYPES:
                    raise TypeError(f'FusedAdamW steps float32 and bfloat16 parameters, got {p.dtype}')
                built.setdefault(p, p.dtype)

    def __setstate__(self, state):
        super().__setstate__(state)
        self.__dict__.setdefault('max_norm', None)
        self.__dict__.setdefault('grad_clip', None)
        self.__dict__.setdefault('master_weights', True)
        self.__dict__.setdefault('grad_norm', None)
        self._records = self._plan = None
        self._check_groups()
        for p, s in self.state.items():
            if 'step' in s and not torch.is_tensor(s['step']):
                s['step'] = torch.tensor(float(s['step']), dtype=torch.float32)

    def load_state_dict(self, state_dict):
        """``torch.optim.Optimizer.load_state_dict`` but for its cast: torch casts floating state to the PARAMETER's
        type, which would round masters and moments of a bf16 parameter to bf16.  Here floating state goes to fp32 on
        the parameter's device, ``step`` stays as it is.  A state without ``master`` for a parameter that needs one
        (torch's own AdamW state of a bf16 parameter: bf16 moments, no master) is completed from the parameter."""
        state_dict = state_dict.copy()
        for hook in getattr(self, '_optimizer_load_state_dict_pre_hooks', {}).values():
            result = hook(self, state_dict)
            if result is not None:
                state_dict = result
        groups = self.param_groups
        saved_groups = [dict(g, params=list(g['params'])) for g in state_dict['param_groups']]
        if len(groups) != len(saved_groups):
            raise ValueError('loaded state dict has a different number of parameter groups')
        if any(len(g['params']) != len(s['params']) for g, s in zip(groups, saved_groups)):
            raise ValueError('loaded state dict contains a parameter group that doesn\'t match the size of '
                             'optimizer\'s group')
        id_map = dict(zip(chain.from_iterable(g['params'] for g in saved_groups),
                          chain.from_iterable(g['params'] for g in groups)))
        state = defaultdict(dict)
        for k, v in state_dict['state'].items():
            if k not in id_map:
                state[k] = v
                continue
            p = id_map[k]
            s = {}
            for name, value in v.items():
                if torch.is_tensor(value) and name != 'step':
                    value = value.to(device=p.device, dtype=torch.float32) if value.is_floating_point() else \
                        value.to(device=p.device)
                s[name] = value
            if p.dtype == torch.float32:
                s.pop('master', None)         # an fp32 parameter is its own master
            elif self.master_weights and 'master' not in s and s:
                s['master'] = p.detach().to(torch.float32)
            state[p] = s
        for group, saved in zip(groups, saved_groups):
            saved['params'] = group['params']
            if 'param_names' in group and 'param_names' not in saved:
                saved['param_names'] = group['param_names']
        self.__setstate__({'state': state, 'param_groups': saved_groups})
        for hook in getattr(self, '_optimizer_load_state_dict_post_hooks', {}).values():
            hook(self)

    # -- the step ------------------------------------------------------------------------------------------
    def _check(self, p, g, on_gpu):
        """every reason to refuse ``p`` and its gradient; changes nothing"""
        built = self._built_dtypes()
        if on_gpu and not p.is_cuda:
            raise _no_cpu('a parameter of FusedAdamW.step()')
        if p.dtype != built.get(p, p.dtype):
            raise RuntimeError(
                f'a parameter was {built[p]} when FusedAdamW was built and is {p.dtype} now: build the optimizer '
                'after enable_fast_path, which converts the parameters (the fp32 masters are taken from the '
                'parameters the optimizer sees)')
        if g.dtype != p.dtype or g.device != p.device:
            raise RuntimeError(f'a gradient is {g.dtype} on {g.device}, its parameter {p.dtype} on {p.device}')
        if not _is_dense(p):
            raise ValueError(f'a parameter of shape {tuple(p.shape)} and strides {p.stride()} is not dense: '
                             'FusedAdamW walks a parameter\'s storage, which its elements must fill')

    def _setup(self, r):
        """the state of ``r.p``, created on first use and brought to fp32 in the parameter's layout (a loaded
        checkpoint may hold another), and what ``_Record.current`` compares"""
        p = r.p
        s = self.state[p]
        if 'step' not in s:
            s['step'] = torch.tensor(0.0, dtype=torch.float32)
            s['exp_avg'] = torch.zeros_like(p, dtype=torch.float32, memory_format=torch.preserve_format)
            s['exp_avg_sq'] = torch.zeros_like(p, dtype=torch.float32, memory_format=torch.preserve_format)
        elif not torch.is_tensor(s['step']):
            s['step'] = torch.tensor(float(s['step']), dtype=torch.float32)
        for name in ('exp_avg', 'exp_avg_sq'):
            s[name] = _in_layout_of(s[name], p, torch.float32)
        if p.dtype != torch.float32 and self.master_weights:
            s['master'] = _in_layout_of(s['master'] if 'master' in s else p.detach(), p, torch.float32)
        r.state, r.dtype, r.address, r.strides, r.is_cuda = s, p.dtype, p.data_ptr(), p.stride(), p.is_cuda
        r.step, r.m, r.v, r.w = s['step'], s['exp_avg'], s['exp_avg_sq'], s.get('master')

    def _prepare(self, on_gpu=True):
        """The host side of a step, which needs no GPU: every parameter with a gradient is checked, gets its state on
        first use, advances its ``step``, and becomes one ``(param, grad, state, scalars)`` entry.  Nothing is changed
        before every check has passed."""
        if self.__dict__.get('_records') is None:
            self._records = [_Record(group, p) for group in self.param_groups for p in group['params']]
            self._plan = None
        state, live, stale = self.state, [], []
        for r in self._records:
            p = r.p
            g = p.grad
            if g is None:
                continue
            if g.is_sparse:
                raise RuntimeError('FusedAdamW does not support sparse gradients')
            if not r.current(state[p]):
                self._check(p, g, on_gpu)
                stale.append(r)
            elif on_gpu and not r.is_cuda:
                raise _no_cpu('a parameter of FusedAdamW.step()')
            live.append(r)
        if not live:
            return []
        if stale:
            if on_gpu:
                _one_device([r.p for r in live])
            for r in stale:
                self._setup(r)
            self._plan = None
        steps = [r.step for r in live]
        torch._foreach_add_(steps, 1)
        entries, memo = [], {}
        for r, t in zip(live, torch.stack(steps).tolist()):
            p, group = r.p, r.group
            if p.grad.stride() != r.strides:          # processed in storage order: one layout for all five arrays
                p.grad = _in_layout_of(p.grad, p, p.dtype)
            beta1, beta2 = group['betas']
            key = (float(group['lr']), beta1, beta2, group['eps'], group['weight_decay'], t)
            scalars = memo.get(key)
            if scalars is None:
                scalars = memo[key] = adamw_scalars(*key)
            entries.append((p, p.grad, r.state, scalars))
        if self._plan is None or self._plan[0] != live:
            self._plan = (live, build_table(entries), chunk_table([p.numel() for p, _, _, _ in entries]))
        return entries

    @torch.no_grad()
    def step(self, closure=None, *, zero_grads=False):
        if closure is not None:
            raise ValueError('FusedAdamW.step takes no closure')
        entries = self._prepare()
        self.grad_norm = None
        if not entries or not len(self._plan[2]):
            return
        _, static, chunks = self._plan
        index = entries[0][0].device.index
        flags = _capi.OPTIM_ZERO_GRADS if zero_grads else 0
        with torch.cuda.device(index):
            bufs, table, chunks, n = _upload_tables(entries, index, static, chunks)
            if self.max_norm is None:
                launch('dfm_adamw_step', table, len(entries), chunks, n, None, 0.0, None, flags, STREAM)
                _COUNTERS['kernel_launches'] += 1
            else:
                partials = bufs.partial_sums(n)
                norm = torch.empty((), dtype=torch.float32, device=table.device)
                launch('dfm_grad_sqnorm', table, len(entries), chunks, n, partials, STREAM)
                launch('dfm_adamw_step', table, len(entries), chunks, n, partials, self.max_norm, norm, flags, STREAM)
                _COUNTERS['kernel_launches'] += 2
                self.grad_norm = norm
        # the kernels wrote through raw pointers: everything cached on a parameter's version is stale now
        torch.autograd.graph.increment_version([e[0] for e in entries])
        if zero_grads:
            torch.autograd.graph.increment_version([e[1] for e in entries])


@torch.no_grad()
def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None):
    """``torch.nn.utils.clip_grad_norm_`` as mmcv's ``OptimizerHook.clip_grads`` calls it: the gradients are scaled in
    place by ``min(1, max_norm / (norm + 1e-6))``; returns the total norm, a 0-dim fp32 DEVICE tensor (``float()`` of it
    waits for the stream).  One table copy and two launches."""
    if float(norm_type) != 2.0:
        raise ValueError('clip_grad_norm_: only norm_type=2 is built (the configs\' own)')
    if error_if_nonfinite:
        raise ValueError('clip_grad_norm_: error_if_nonfinite=True needs the norm on the host; it is not built')
    if torch.is_tensor(parameters):
        parameters = [parameters]
    params = [p for p in parameters if p.grad is not None]
    if not params:
        return torch.tensor(0.0)
    for p in params:
        if not p.grad.is_cuda:
            raise _no_cpu('a gradient of clip_grad_norm_')
        if p.grad.dtype not in DTYPES:
            raise TypeError(f'clip_grad_norm_ takes float32 and bfloat16 gradients, got {p.grad.dtype}')
        if p.grad.is_sparse:
            raise RuntimeError('clip_grad_norm_ does not support sparse gradients')
        if not _is_dense(p.grad):
            p.grad = p.grad.contiguous()
    index = _one_device([p.grad for p in params])
    entries = [(None, p.grad, None, None) for p in params if p.grad.numel()]
    with torch.cuda.device(index):
        norm = (torch.empty if entries else torch.zeros)((), dtype=torch.float32, device=params[0].grad.device)
        if entries:
            bufs, table, chunks, n = _upload_tables(entries, index)
            partials = bufs.partial_sums(n)
            launch('dfm_grad_sqnorm', table, len(entries), chunks, n, partials, STREAM)
            launch('dfm_grad_scale', table, len(entries), chunks, n, partials, float(max_norm), norm, STREAM)
            _COUNTERS['kernel_launches'] += 2
    torch.autograd.graph.increment_version([e[1] for e in entries])
    return norm
