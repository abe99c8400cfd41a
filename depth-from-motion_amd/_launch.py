"""The one place that turns tensors into C arguments: every kernel launch of the package goes
through ``launch`` / ``try_launch`` (``_capi`` stays torch-free; size queries and pure validation
calls, which launch nothing, keep calling ``_capi.lib()`` directly).

    launch('dfm_group_norm_fwd', n, c, spatial, groups, eps, DTYPES[x.dtype], relu,
           x, w32, b32, y, mean, rstd, WS, STREAM, ws_bytes=nbytes)

reads like the C signature.  A tensor becomes its address, ``None`` NULL, a ``ctypes.Structure`` a
by-reference argument; ``STREAM`` becomes the current stream of the call's device and ``WS`` the
pair (scratch pointer, ``ws_bytes``), the scratch buffer being that of the same device AND the same
stream, from one stream lookup.  The call's device is the device of its tensor arguments: a tensor
that is not on a GPU, or tensors on two devices, raise before the library is entered.  The argument
tuple keeps every tensor (temporaries included) alive until the C function has returned.
"""
import ctypes

import torch

from . import _capi

DTYPES = {torch.float32: _capi.DFM_F32, torch.bfloat16: _capi.DFM_BF16}


class _Sentinel:
    def __init__(self, name):
        self.name = name

    def __repr__(self):
        return self.name


STREAM, WS = _Sentinel('STREAM'), _Sentinel('WS')


def require_gpu(t, name):
    if not t.is_cuda:
        raise RuntimeError(
            f'{name} must live on the GPU: depth-from-motion_amd has no CPU path '
            '(the HIP kernels are the product; the CPU oracle is test-only)')


def upload(t, device):
    """small host tensor -> device without blocking the host on the stream: a pageable H2D copy
    waits for everything queued before it, which serialises the Python launch loop of the next
    step with the GPU work of the previous one (profiles/archive/r02_c26_*: 2x on the multi-view path)"""
    if t.device.type != 'cpu':
        return t.to(device)
    return t.contiguous().pin_memory().to(device, non_blocking=True)


def nonempty(t):
    """``t``, or None (NULL) for an empty tensor: the ``rows == 0`` shard of the cross-rank BatchNorm.  Not a
    marshalling rule: everywhere else an empty tensor is an error the library reports."""
    return t if t is not None and t.numel() else None


def pointers(tensors, n):
    """a ``void *[n]`` of the addresses of up to ``n`` GPU tensors, NULL-padded (``dfm_spp_tail_fwd`` takes its
    sources and parameters so); the array keeps the tensors alive"""
    for t in tensors:
        require_gpu(t, 'a tensor of a pointer array')
    arr = (ctypes.c_void_p * n)(*[t.data_ptr() for t in tensors])
    arr.tensors = tuple(tensors)
    return arr


def stream_ptr(device):
    """the current stream of ``device`` (a torch.device or an index) as the C ABI takes it (tests and tools that
    call the raw library)"""
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


class Workspace:
    """Scratch (blocked feature copies, GroupNorm partials, pixel-major staging), grown on
    demand and kept so that the steady state allocates nothing.  One buffer per (device index,
    stream): two ops issued on different streams never share scratch."""
    _bufs = {}

    @classmethod
    def get(cls, index, stream, nbytes):
        key = (index, stream)
        buf = cls._bufs.get(key)
        if buf is None or buf.numel() < nbytes:
            buf = torch.empty(nbytes, dtype=torch.uint8, device=torch.device('cuda', index))
            cls._bufs[key] = buf
        return buf


def _resources(index, ws_bytes):
    """(stream handle, scratch address or None) of device ``index``: ONE stream lookup, so the stream a kernel
    gets is the one its scratch was keyed on"""
    stream = torch.cuda.current_stream(index).cuda_stream
    return stream, (None if ws_bytes is None else Workspace.get(index, stream, ws_bytes).data_ptr())


_Tensor, _Structure = torch.Tensor, ctypes.Structure


def marshal(args, ws_bytes=0, resources=_resources):
    """(device index, C argument list) of a launch's Python arguments; pure but for ``resources(index, ws_bytes
    or None) -> (stream, scratch address)``, which is asked once, and only when a sentinel is present.  The loop
    is the host cost of every launch: exact type checks, the commonest kinds first, and the device as an int --
    torch resolves a ``torch.device`` to its index in Python, at several times the cost of this whole loop."""
    out, index, stream_at, ws_at = [], None, None, None
    append = out.append
    for a in args:
        t = type(a)
        if t is int or a is None or t is float:
            append(a)
        elif t is _Tensor or isinstance(a, _Tensor):
            i = a.get_device()
            if i != index or not a.is_cuda:
                if not a.is_cuda:
                    raise RuntimeError(
                        f'a {a.device.type} tensor reached a kernel launch: depth-from-motion_amd has no CPU path')
                if index is not None:
                    raise RuntimeError(f'tensors of one kernel launch live on two devices (cuda:{index} and cuda:{i}): '
                                       'depth-from-motion_amd has no CPU path and no cross-device kernels')
                index = i
            append(a.data_ptr())
        elif a is STREAM:
            stream_at = len(out)
            append(None)
        elif a is WS:
            ws_at = len(out)
            out += (None, ws_bytes)
        elif isinstance(a, _Structure):
            append(ctypes.byref(a))
        else:
            append(a)
    if stream_at is not None or ws_at is not None:
        if index is None:
            raise RuntimeError('a kernel launch without a GPU tensor argument has no device to take its stream '
                               'from: depth-from-motion_amd has no CPU path')
        stream, scratch = resources(index, ws_bytes if ws_at is not None else None)
        if stream_at is not None:
            out[stream_at] = stream
        if ws_at is not None:
            out[ws_at] = scratch
    return index, out


def call(fn, args, ws_bytes=0):
    """status of the C function ``fn`` on the marshalled ``args``, under the device guard of their device"""
    index, cargs = marshal(args, ws_bytes)
    if index is None:
        return fn(*cargs)
    with torch.cuda.device(index):
        return fn(*cargs)


def launch(name, *args, ws_bytes=0):
    """``lib().<name>(*marshalled args)``; a non-zero status raises ``DfmHipError`` with the library's reason"""
    rc = call(getattr(_capi.lib(), name), args, ws_bytes)
    if rc:
        _capi.check(rc)


def try_launch(name, *args, ws_bytes=0):
    """as ``launch``, for entry points that may decline: True on success, False on ``DFM_ERR_UNSUPPORTED`` (the
    caller falls through to its next kernel); any other status raises"""
    rc = call(getattr(_capi.lib(), name), args, ws_bytes)
    if rc == 0:
        return True
    if rc != _capi.DFM_ERR_UNSUPPORTED:
        _capi.check(rc)
    return False
