"""GPU: the launch helper on a device -- scratch is per (device, stream) and the stream a call is handed is the
one its scratch was keyed on (observed with a recording stand-in that receives the real marshalled values: no
kernel needed), and one real launch chain on a side stream against the default stream."""
import importlib
import types

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


@pytest.fixture(scope='module')
def L():
    assert torch.cuda.is_available()
    return importlib.import_module('depth-from-motion_amd._launch')


@pytest.fixture
def rec(L, monkeypatch):
    calls = []

    def stand_in(*args):
        calls.append(args)
        return 0
    monkeypatch.setattr(L._capi, 'lib', lambda: types.SimpleNamespace(dfm_stand_in=stand_in))
    return calls


def test_scratch_is_per_stream_and_grows(L, rec):
    x = torch.zeros(4, device=DEV)
    a, b = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
    for s in (a, b, a):
        with torch.cuda.stream(s):
            L.launch('dfm_stand_in', x, L.WS, L.STREAM, ws_bytes=4096)
    (xa, wa, na, sa), (xb, wb, nb, sb), (_, wa2, _, sa2) = rec
    assert xa == xb == x.data_ptr() and na == nb == 4096
    assert (sa, sb, sa2) == (a.cuda_stream, b.cuda_stream, a.cuda_stream)
    assert wa and wb and wa != wb           # two streams never share scratch
    assert wa2 == wa                        # the same stream gets its buffer again
    with torch.cuda.stream(a):
        L.launch('dfm_stand_in', x, L.WS, L.STREAM, ws_bytes=8192)
    assert rec[3][2] == 8192
    assert L.Workspace.get(DEV.index, a.cuda_stream, 8192).data_ptr() == rec[3][1]
    assert L.Workspace.get(DEV.index, a.cuda_stream, 8192).numel() >= 8192
    assert L.Workspace.get(DEV.index, b.cuda_stream, 0).numel() >= 4096   # (b's buffer was not touched)


def test_the_stream_passed_is_the_current_one(L, rec):
    x = torch.zeros(4, device=DEV)
    side = torch.cuda.Stream(DEV)
    with torch.cuda.stream(side):
        L.launch('dfm_stand_in', L.STREAM, x)
    L.launch('dfm_stand_in', L.STREAM, x)
    assert rec[0] == (side.cuda_stream, x.data_ptr())
    assert rec[1] == (torch.cuda.default_stream(DEV).cuda_stream, x.data_ptr())
    assert L.stream_ptr(DEV).value == (torch.cuda.current_stream(DEV).cuda_stream or None)


def test_group_norm_on_a_side_stream_is_bit_identical():
    """bf16 channels-last-3d (1, 16, 2, 4, 4), 4 groups, relu: the smallest shape at which the channels-last
    kernels, their scratch buffer and the xmask backward all run"""
    gn = importlib.import_module('depth-from-motion_amd.group_norm')
    g = torch.Generator().manual_seed(11)
    x = torch.randn(1, 16, 2, 4, 4, generator=g).to(DEV).bfloat16().contiguous(memory_format=torch.channels_last_3d)
    gy = torch.randn(1, 16, 2, 4, 4, generator=g).to(DEV).bfloat16().contiguous(memory_format=torch.channels_last_3d)
    w0, b0 = torch.randn(16, generator=g).to(DEV), torch.randn(16, generator=g).to(DEV)

    def run():
        xx, w, b = x.clone().requires_grad_(True), w0.clone().requires_grad_(True), b0.clone().requires_grad_(True)
        y = gn.group_norm(xx, 4, w, b, relu=True)
        y.backward(gy)
        return y.detach(), xx.grad, w.grad, b.grad

    want = run()
    side, current = torch.cuda.Stream(DEV), torch.cuda.current_stream(DEV)
    side.wait_stream(current)
    with torch.cuda.stream(side):
        got = run()
    current.wait_stream(side)
    assert want[0].is_contiguous(memory_format=torch.channels_last_3d) and bool((want[0] > 0).any())
    for name, a, b in zip(('y', 'grad_x', 'grad_weight', 'grad_bias'), got, want):
        assert a.dtype == b.dtype and torch.equal(a, b), name
