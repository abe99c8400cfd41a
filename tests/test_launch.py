"""CPU: the launch helper (depth-from-motion_amd/_launch.py) without a GPU -- how Python arguments become C
arguments (against recording stand-ins), the device checks, how a status becomes True / False / an exception
(real rejecting calls on the built library: no kernel is launched).  The signature table of _capi.py is held against
the headers by tests/test_capi_binding.py."""
import ctypes
import importlib
import types

import pytest
import torch

STREAM_HANDLE, SCRATCH = 0x5151, 0x7000


@pytest.fixture(scope='module')
def pkg():
    importlib.import_module('depth-from-motion_amd.build').build_hip()
    return importlib.import_module('depth-from-motion_amd')


@pytest.fixture(scope='module')
def L(pkg):
    return importlib.import_module('depth-from-motion_amd._launch')


class OnGpu(torch.Tensor):
    """a host tensor that says it lives on cuda:<index>: what ``marshal`` reads of a tensor is ``is_cuda``,
    ``get_device()`` and ``data_ptr()``, and no device is touched"""
    index, is_cuda = 0, True

    def get_device(self):
        return self.index


def on_gpu(index=0, n=4):
    t = torch.zeros(n).as_subclass(OnGpu)
    t.index = index
    return t


class Recorder:
    def __init__(self, status=0):
        self.status, self.calls = status, []

    def __call__(self, *args):
        self.calls.append(args)
        return self.status


def resources(asked):
    def fn(device, ws_bytes):
        asked.append((device, ws_bytes))
        return STREAM_HANDLE, (None if ws_bytes is None else SCRATCH)
    return fn


def test_marshalling_rules(pkg, L):
    a, b = on_gpu(), on_gpu()
    desc = pkg._capi.SweepDesc(batch=3)
    arr = (ctypes.c_void_p * 4)(1, 2)
    asked = []
    device, out = L.marshal((desc, a, None, 7, 0.5, L.WS, arr, L.STREAM, b, 9), 4096, resources(asked))
    assert device == 0
    assert asked == [(device, 4096)]                       # ONE lookup serves the scratch and the stream
    assert len(out) == 11                                  # WS is two arguments, STREAM one, everything else one
    byref = out[0]
    assert type(byref).__name__ == 'CArgObject' and byref._obj is desc      # ctypes.byref(desc)
    assert out[1] == a.data_ptr() and type(out[1]) is int
    assert out[2] is None
    assert out[3] == 7 and type(out[3]) is int and out[4] == 0.5 and type(out[4]) is float
    assert out[5:7] == [SCRATCH, 4096]                     # WS, in place
    assert out[7] is arr
    assert out[8] == STREAM_HANDLE                         # STREAM, in place
    assert out[9] == b.data_ptr() and out[10] == 9


def test_sentinels_expand_only_where_written(L):
    a = on_gpu()
    asked = []
    assert L.marshal((a, 1, L.STREAM, 2), 0, resources(asked))[1] == [a.data_ptr(), 1, STREAM_HANDLE, 2]
    assert asked == [(0, None)]      # no WS: no scratch buffer is asked for
    asked = []
    assert L.marshal((L.WS, a), 64, resources(asked))[1] == [SCRATCH, 64, a.data_ptr()]
    asked = []
    assert L.marshal((a, None, 3), 0, resources(asked)) == (0, [a.data_ptr(), None, 3])
    assert asked == []                                     # no sentinel: no stream lookup at all
    assert L.marshal((None, 0, None)) == (None, [None, 0, None])


def test_pointers_is_a_null_padded_array_that_keeps_its_tensors(L):
    with pytest.raises(RuntimeError, match='no CPU path'):
        L.pointers([torch.zeros(2)], 4)
    ts = [on_gpu(), on_gpu()]
    arr = L.pointers(ts, 4)
    assert list(arr) == [ts[0].data_ptr(), ts[1].data_ptr(), None, None] and arr.tensors == tuple(ts)


def test_nonempty(L):
    assert L.nonempty(None) is None and L.nonempty(torch.zeros(0, 3)) is None
    t = torch.zeros(1)
    assert L.nonempty(t) is t


def test_cpu_tensor_is_refused_before_the_library_is_entered(L, monkeypatch):
    rec = Recorder()
    monkeypatch.setattr(L._capi, 'lib', lambda: types.SimpleNamespace(dfm_stand_in=rec))
    for bad in (torch.zeros(4), torch.nn.Parameter(torch.zeros(4)), torch.zeros(4, device='meta')):
        with pytest.raises(RuntimeError, match='no CPU path'):
            L.launch('dfm_stand_in', 1, bad, L.STREAM)
        with pytest.raises(RuntimeError, match='no CPU path'):
            L.try_launch('dfm_stand_in', on_gpu(), bad, L.WS, L.STREAM, ws_bytes=16)
    assert rec.calls == []


def test_two_devices_are_refused_before_the_library_is_entered(L, monkeypatch):
    rec = Recorder()
    monkeypatch.setattr(L._capi, 'lib', lambda: types.SimpleNamespace(dfm_stand_in=rec))
    with pytest.raises(RuntimeError, match='two devices'):
        L.launch('dfm_stand_in', on_gpu(0), 5, on_gpu(1), L.STREAM)
    with pytest.raises(RuntimeError, match='two devices'):
        L.marshal((on_gpu(1), on_gpu(0)))
    assert rec.calls == []


def test_sentinel_without_a_tensor_is_refused(L, monkeypatch):
    rec = Recorder()
    monkeypatch.setattr(L._capi, 'lib', lambda: types.SimpleNamespace(dfm_stand_in=rec))
    with pytest.raises(RuntimeError, match='no device'):
        L.launch('dfm_stand_in', 1, None, L.STREAM)
    assert rec.calls == []


def test_status_mapping_with_stand_ins(L, monkeypatch):
    ok, declined = Recorder(0), Recorder(-2)
    monkeypatch.setattr(L._capi, 'lib', lambda: types.SimpleNamespace(ok=ok, declined=declined))
    assert L.try_launch('ok', 1, None) is True and L.launch('ok', 2) is None
    assert L.try_launch('declined', 3) is False
    assert ok.calls == [(1, None), (2,)] and declined.calls == [(3,)]


def test_status_mapping_on_the_built_library(pkg, L):
    err = pkg._capi.DfmHipError
    desc = pkg._capi.SweepDesc()                           # all zero: rejected before anything is launched
    tail = (None, None, None, None, None, None, None, None, 0, None)
    with pytest.raises(err, match='size') as e:
        L.try_launch('dfm_plane_sweep_fwd', desc, *tail)
    assert 'libdfm_hip error -1' in str(e.value)
    assert pkg._capi.lib().dfm_last_error().decode() in str(e.value)        # the library's own reason
    with pytest.raises(err, match='libdfm_hip error -1'):
        L.launch('dfm_plane_sweep_fwd', desc, *tail)
    desc.batch = desc.channels = desc.h_in = desc.w_in = 4
    desc.num_depths = desc.h_out = desc.w_out = 4
    desc.dtype = 7                                         # a dtype the library does not know: DFM_ERR_UNSUPPORTED
    assert L.try_launch('dfm_plane_sweep_fwd', desc, *tail) is False
    with pytest.raises(err, match='libdfm_hip error -2'):
        L.launch('dfm_plane_sweep_fwd', desc, *tail)
