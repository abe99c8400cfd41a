"""CPU: the feature-imitation loss above the kernel -- NormalizeLayer, the statistics-to-loss-and-update
function (one rank and gloo world 2), ImitationLoss's state-dict keys, descriptor validation -- against
tests/golden/imitation.npz (the reference's own code, tests/golden/make_golden_imitation.py)."""
import ctypes
import importlib
import multiprocessing
import os

import numpy as np
import pytest
import torch

from tests import imitation_util as iu

TOL = dict(rtol=1e-4, atol=1e-5)


@pytest.fixture(scope='module')
def pkg():
    importlib.import_module('depth-from-motion_amd.build').build_hip()
    return importlib.import_module('depth-from-motion_amd')


@pytest.fixture(scope='module')
def z():
    return iu.load()


def gathered(c):
    """(Npos, C) pred and target rows at the recorded positives"""
    perm = lambda t: t.permute(0, *range(2, t.dim()), 1)  # noqa: E731
    return perm(c['pred'])[c['positives']], perm(c['target'])[c['positives']]


def make_layer(pkg, c, C):
    if c['normalize'] is None:
        return None
    layer = pkg.NormalizeLayer(c['normalize'], C)
    layer.scale.copy_(c['scale0'])
    if 'center0' in c:
        layer.center.copy_(c['center0'])
    return layer


def numpy_stats(c, layer):
    """[count, S, sum t, sum |t|] in fp64 with numpy, from the recorded positives"""
    pp, pt = (t.double().numpy() for t in gathered(c))
    tn = pt.copy()
    if layer is not None:
        if layer.do_centering:
            tn = tn - layer.center.double().numpy()
        tn = tn / layer.scale.double().numpy()
    sq = np.where(np.isnan(tn), 0.0, 0.5 * (pp - tn) ** 2)
    return torch.from_numpy(np.concatenate([[pp.shape[0], sq.sum()], pt.sum(0), np.abs(pt).sum(0)])), pt


def check_buffers(layer, c):
    if layer is None:
        return
    assert torch.allclose(layer.scale, c['scale1'], equal_nan=True, **TOL)
    if 'center1' in c:
        assert torch.allclose(layer.center, c['center1'], equal_nan=True, **TOL)


@pytest.mark.parametrize('name', ['a_3d', 'c_scale', 'c_center_scale', 'c_cw_center_scale', 'f_few', 'g_eval'])
def test_normalize_layer_forward_and_update(pkg, z, name):
    c = iu.case(z, name)
    C = c['pred'].shape[1]
    layer = make_layer(pkg, c, C).train(c['training'])
    pp, pt = gathered(c)
    out = layer(pt)
    expect = (pt - c['center0'] if 'center0' in c else pt) / c['scale0']
    assert torch.equal(out, expect)
    check_buffers(layer, c)
    if name in ('f_few', 'g_eval'):      # <= 10 positives / eval mode: untouched
        assert torch.equal(layer.scale, c['scale0'])
    # and the loss the reference made of it (dfm.py:507-526)
    w = 1.0 / max(float(pt.shape[0]), 10.0)
    loss = (0.5 * (pp - out) ** 2 * w).mean(-1).sum() / c['pred'].shape[0] * c['loss_weight']
    assert abs(float(loss) - c['loss']) <= 1e-4 * abs(c['loss']) + 1e-5


@pytest.mark.parametrize('name', iu.CASES)
def test_statistics_to_loss_and_update(pkg, z, name):
    c = iu.case(z, name)
    B, C = c['pred'].shape[:2]
    layer = make_layer(pkg, c, C)
    if layer is not None:
        layer.train(c['training'])
    stats, pt = numpy_stats(c, layer)
    calls = []

    def centered_abs_sum(nc):
        calls.append(1)
        return torch.from_numpy(np.abs(pt - nc.double().numpy()).sum(0))

    scale, normalizer = pkg.reduce_imitation_statistics(stats, C, B, c['loss_weight'], layer, 10, c['training'],
                                                        None, centered_abs_sum)
    assert float(normalizer) == max(float(stats[0]), 10.0)
    loss = float(stats[1].float() * scale)
    assert abs(loss - c['loss']) <= 1e-4 * abs(c['loss']) + 1e-5, (loss, c['loss'])
    check_buffers(layer, c)
    centering = layer is not None and layer.do_centering and c['training']
    assert len(calls) == (1 if centering else 0)
    if name in ('e_miss', 'f_few', 'g_eval'):
        assert torch.equal(layer.scale, c['scale0'])
        if 'center0' in c:
            assert torch.equal(layer.center, c['center0'])


def _rank_main(rank, world, store_path, kind, parts, q):
    """one gloo rank: reduce its share of the statistics, report buffers and the collectives it issued"""
    import torch.distributed as dist
    pkg = importlib.import_module('depth-from-motion_amd')
    dist.init_process_group('gloo', store=dist.FileStore(store_path, world), rank=rank, world_size=world)
    issued = []
    real = dist.all_reduce

    def counting(t, *a, **k):
        issued.append(t.numel())
        return real(t, *a, **k)
    dist.all_reduce = counting
    try:
        C = parts[0].shape[1]
        layer = pkg.NormalizeLayer(kind, C).train()
        pt = parts[rank].double().numpy()
        stats = torch.from_numpy(np.concatenate([[pt.shape[0], 0.0], pt.sum(0), np.abs(pt).sum(0)]))
        scale, normalizer = pkg.reduce_imitation_statistics(
            stats, C, 2, 1.0, layer, 10, True, None,
            lambda nc: torch.from_numpy(np.abs(pt - nc.double().numpy()).sum(0)))
        q.put((rank, {k: v.clone().numpy() for k, v in layer.named_buffers()}, issued, float(normalizer)))
    finally:
        dist.all_reduce = real
        dist.destroy_process_group()


@pytest.mark.parametrize('kind', ['cw_scale', 'scale', 'center+scale', 'cw_center+scale'])
def test_statistics_under_gloo_world_2(pkg, tmp_path, kind):
    """two ranks with different statistics, one of them without a positive: identical buffers on both, equal
    to one rank's on the concatenated data; 1 collective (2 for the centering types), issued by both"""
    C = 8
    gen = torch.Generator().manual_seed(5)
    data = torch.randn(37, C, generator=gen) * 2 + 0.5
    parts = [data, data[:0]]
    ctx = multiprocessing.get_context('fork')
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank_main, args=(r, 2, str(tmp_path / 'store'), kind, parts, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = sorted([q.get(timeout=120) for _ in procs], key=lambda t: t[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    single = pkg.NormalizeLayer(kind, C).train()
    single.update(data)                      # no process group here: one rank on the concatenated data
    expected_collectives = 2 if 'center' in kind else 1
    for rank, bufs, issued, normalizer in got:
        assert len(issued) == expected_collectives, issued
        assert issued[0] == 1 + C           # the count rides with the per-channel sums
        assert normalizer == 37 / 2         # dist_reduce_mean of the positives count
        for k, v in single.named_buffers():
            assert np.allclose(bufs[k], v.numpy(), rtol=1e-6, atol=1e-7), (kind, k)
            assert np.array_equal(bufs[k], got[0][1][k])


def test_state_dict_keys_match_the_reference(pkg, z):
    two = [dict(lidar_feature_layer='spatial_features_2d', stereo_feature_layer='spatial_features_2d',
                normalize='cw_scale', layer='conv2d', channel=64, kernel_size=1, use_relu=False, mode='inbox'),
           dict(lidar_feature_layer='volume_features', stereo_feature_layer='volume_features', normalize='cw_scale',
                layer='conv3d', channel=32, kernel_size=1, use_relu=False, mode='inbox')]
    one = [dict(lidar_feature_layer='volume_features', stereo_feature_layer='volume_features', normalize=None,
                layer='conv3d', channel=32, kernel_size=1, use_relu=True, mode='inbox')]
    assert list(pkg.ImitationLoss(two).state_dict().keys()) == list(z['keys_two_cfgs'])
    assert list(pkg.ImitationLoss(one).state_dict().keys()) == list(z['keys_one_cfg'])
    m = pkg.ImitationLoss(two)
    assert isinstance(m.conv_imitation, torch.nn.ModuleList)
    assert isinstance(pkg.ImitationLoss(one).conv_imitation, torch.nn.Sequential)
    # a detector checkpoint's entries load
    sd = {k: torch.full_like(v, 0.25) for k, v in m.state_dict().items()}
    m.load_state_dict(sd)
    assert float(m.norm_imitation['volume_features'].scale.mean()) == 0.25


def test_full_mode_of_the_reference_cannot_run(z):
    """the generator tried it: 'full' is therefore DEFINED as all-true here (tests/test_imitation_gpu.py)"""
    assert not bool(z['full_mode_runs'])


def test_invalid_desc_is_rejected_without_touching_the_gpu(pkg):
    lib = pkg._capi.lib()
    d = pkg._capi.ImitationDesc()   # all zero
    assert lib.dfm_imitation_loss_workspace_bytes(ctypes.byref(d)) == 0
    assert lib.dfm_imitation_loss_workspace_bytes(None) == 0
    args_f = (None,) * 11 + (0, None)
    assert lib.dfm_imitation_loss_fwd(None, *args_f[1:]) == -1
    assert lib.dfm_imitation_loss_fwd(ctypes.byref(d), *args_f[1:]) == -1
    assert b'size' in lib.dfm_last_error()
    assert lib.dfm_imitation_loss_bwd(ctypes.byref(d), *((None,) * 8)) == -1
    d.batch, d.channels, d.nz, d.ny, d.nx, d.points_batch = 1, 32, 5, 8, 8, 1
    d.pred_dtype = 7
    assert lib.dfm_imitation_loss_fwd(ctypes.byref(d), *args_f[1:]) == -2
    assert lib.dfm_imitation_loss_bwd(ctypes.byref(d), *((None,) * 8)) == -2
    d.pred_dtype = 0
    d.channels = 2048
    assert lib.dfm_imitation_loss_fwd(ctypes.byref(d), *args_f[1:]) == -2
    d.channels = 32
    d.center_len = 3
    assert lib.dfm_imitation_loss_fwd(ctypes.byref(d), *args_f[1:]) == -1
    d.center_len = 0
    # ticket + one workgroup's count + its partial row (S, sum t, sum |t|)
    assert lib.dfm_imitation_loss_workspace_bytes(ctypes.byref(d)) == 16 + 4 + 4 * (1 + 2 * 32)
    assert lib.dfm_imitation_loss_fwd(ctypes.byref(d), *args_f[1:]) == -1   # NULL pointers
    assert b'NULL' in lib.dfm_last_error()
    assert lib.dfm_imitation_loss_bwd(ctypes.byref(d), *((None,) * 8)) == -1


def test_cpu_tensors_are_refused(pkg):
    x = torch.zeros(1, 4, 8, 8)
    with pytest.raises(RuntimeError, match='no CPU path'):
        pkg.imitation_reg_layer_loss(x, x, dict(mode='inbox', loss_weight=1.0), torch.zeros(1, 1, 7),
                                     torch.zeros(1, 8, 8, 3))
