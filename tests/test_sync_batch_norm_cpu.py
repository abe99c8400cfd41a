"""CPU: the cross-rank BatchNorm entry points (dfm_batch_norm_*_channels_last) refuse bad arguments before any HIP
call, and the dispatch of nn.SyncBatchNorm at world size > 1 depends only on what every rank shares."""
import ctypes
import importlib

import pytest
import torch

F32, BF16 = 0, 1
A = 0x100000        # fake 16-byte aligned device pointers: never dereferenced, every call below fails its checks first
MIS = A + 4


@pytest.fixture(scope='module')
def lib():
    importlib.import_module('depth-from-motion_amd.build').build_hip()
    return importlib.import_module('depth-from-motion_amd')._capi.lib()


def p(v):
    return ctypes.c_void_p(v)


def test_workspace_size_depends_on_c_only(lib):
    assert lib.dfm_batch_norm_workspace_bytes(0, 10) == 0
    assert lib.dfm_batch_norm_workspace_bytes(512, 10) == 0
    assert lib.dfm_batch_norm_workspace_bytes(64, -1) == 0
    sizes = {lib.dfm_batch_norm_workspace_bytes(64, rows) for rows in (0, 1, 1000, 10 ** 9)}
    assert len(sizes) == 1 and sizes.pop() > 0


def test_stats_rejects_bad_arguments(lib):
    ws = lib.dfm_batch_norm_workspace_bytes(64, 100)

    def call(c=64, rows=100, dtype=BF16, x=A, stats=A, w=A, nbytes=ws):
        return lib.dfm_batch_norm_stats_channels_last(c, rows, dtype, p(x), p(stats), p(w), nbytes, None)
    assert call(c=0) == -1
    assert call(rows=-1) == -1
    assert call(dtype=7) == -2
    assert call(x=0) == -1
    assert call(stats=0) == -1
    assert call(w=0) == -1
    assert call(nbytes=ws - 1) == -3
    assert call(c=24) == -2          # 3 bf16 vectors: not a power of two
    assert call(c=20, dtype=F32) == -2
    assert call(x=MIS) == -2
    assert b'16-byte' in lib.dfm_last_error()


def test_apply_gathered_rejects_bad_arguments(lib):
    def call(c=64, rows=100, world=2, dtype=BF16, x=A, g=A, b=A, res=0, gathered=A, y=A, mean=A, rstd=A, mom=A):
        return lib.dfm_batch_norm_apply_gathered_channels_last(c, rows, world, 1e-5, dtype, 1, p(x), p(g), p(b),
                                                               p(res), p(gathered), p(y), p(mean), p(rstd), p(mom),
                                                               None)
    assert call(world=0) == -1
    assert call(rows=-5) == -1
    assert call(dtype=3) == -2
    for k in ('x', 'g', 'b', 'gathered', 'y', 'mean', 'rstd', 'mom'):
        assert call(**{k: 0}) == -1, k
    assert call(c=256 + 8) == -2
    assert call(res=MIS) == -2
    assert call(y=MIS) == -2


def test_backward_entry_points_reject_bad_arguments(lib):
    ws = lib.dfm_batch_norm_workspace_bytes(256, 100)

    def red(c=32, rows=100, relu=1, gy=A, x=A, y=A, beta=A, sums=A, w=A, nbytes=ws):
        return lib.dfm_batch_norm_bwd_reduce_channels_last(c, rows, BF16, relu, p(gy), p(x), p(y), p(A), p(A), p(A),
                                                           p(beta), p(sums), p(w), nbytes, None)

    def app(c=32, rows=100, relu=1, gy=A, x=A, y=A, beta=A, sums=A, count=A, gx=A, gres=0, nbytes=ws):
        return lib.dfm_batch_norm_bwd_apply_channels_last(c, rows, BF16, relu, p(gy), p(x), p(y), p(A), p(A), p(A),
                                                          p(beta), p(sums), p(count), p(gx), p(gres), p(A), nbytes,
                                                          None)
    for f in (red, app):
        assert f(c=-8) == -1
        assert f(rows=-1) == -1
        assert f(gy=0) == -1
        assert f(x=0) == -1
        assert f(sums=0) == -1
        assert f(y=0, beta=0) == -1      # relu needs a mask source: y, or beta to recompute it from x
        assert f(nbytes=lib.dfm_batch_norm_workspace_bytes(32, 100) - 256) == -3
        assert f(c=48) == -2
        assert f(gy=MIS) == -2
        assert f(x=MIS) == -2
        assert f(y=MIS) == -2
    assert app(count=0) == -1
    assert app(gx=0) == -1
    assert app(gx=MIS) == -2
    assert app(gres=MIS) == -2


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last_3d if t.dim() == 5 else torch.channels_last)


def test_eligibility_is_the_same_for_every_local_shard():
    gn = importlib.import_module('depth-from-motion_amd.group_norm')
    bn = torch.nn.SyncBatchNorm(64).train()
    base = _cl(torch.zeros(4, 64, 6, 10, dtype=torch.bfloat16))
    shards = [base, base[1:3], base[3:3], base[2:], _cl(torch.zeros(0, 64, 6, 10, dtype=torch.bfloat16)),
              _cl(torch.zeros(2, 64, 17, 3, dtype=torch.bfloat16)), _cl(torch.zeros(1, 64, 1, 1, dtype=torch.bfloat16)),
              _cl(torch.zeros(3, 64, 2, 1, dtype=torch.bfloat16))]
    assert any(s.storage_offset() for s in shards) and any(s.numel() == 0 for s in shards)
    assert {gn.sync_batch_norm_eligible(bn, s) for s in shards} == {True}
    # a 16-byte misaligned view: still the fused path (the local tensor is copied, the decision does not change)
    flat = torch.zeros(1 + 2 * 64 * 3 * 5, dtype=torch.bfloat16)
    odd = flat[1:].view(2, 3, 5, 64).permute(0, 3, 1, 2)
    assert odd.data_ptr() % 16 and gn.sync_batch_norm_eligible(bn, odd)
    # 3-D (channels_last_3d) shards likewise
    v = _cl(torch.zeros(2, 32, 3, 4, 5))
    assert {gn.sync_batch_norm_eligible(bn, t) for t in (v, v[:0], v[1:])} == {True}
    # what every rank shares decides the other way on all of them
    nchw = torch.zeros(4, 64, 6, 10, dtype=torch.bfloat16)
    assert {gn.sync_batch_norm_eligible(bn, t) for t in (nchw, nchw[1:3], nchw[:0], nchw[:, :, :3])} == {False}
    for t in (base.half(), base[:, :24], _cl(torch.zeros(2, 512, 2, 2))):
        assert {gn.sync_batch_norm_eligible(bn, s) for s in (t, t[:0], t[1:])} == {False}
    bn.eval()
    assert {gn.sync_batch_norm_eligible(bn, s) for s in shards} == {False}
    bn.train()
    assert {gn.sync_batch_norm_eligible(torch.nn.SyncBatchNorm(64, affine=False), s) for s in shards} == {False}
