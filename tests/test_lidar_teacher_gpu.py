"""GPU: the LiDAR teacher's kernels -- hard voxelization bit for bit against the reference's ``points_to_voxel``, the
sparse convolutions' exact properties (active sets, zeros off them, the identity tap, borders between samples, row
permutations, tile-edge row counts, empty inputs), their values against the fp64 stand-in within the rule of
tests/test_deform_conv_gpu.py (the fixture's fp32-vs-fp64 figure x 4 x the tensor's largest magnitude), and
``LidarTeacher`` end to end.

Fixture: tests/golden/lidar_teacher.npz (generator tests/golden/make_golden_lidar_teacher.py).  Where a test builds
its own inputs the bar is the derived bound of the sum, (terms + 2) * 2^-24 * sum |a| |w|: every product and every
addition of a chain of fused multiply-adds rounds once, relative to a partial sum that sum |a| |w| bounds."""
import importlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import lidar_teacher_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def pkg():
    importlib.import_module('depth-from-motion_amd.build').build_hip()
    return importlib.import_module('depth-from-motion_amd')


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------------------------------
# voxelization
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['faces', 'nan', 'crowded', 'cut', 'empty', 'outside', 'ndim5', 'ndim3'])
def test_hard_voxelize_is_the_references_bit_for_bit(pkg, case):
    z, gen = ref.fixture(), ref.generator()
    points = torch.from_numpy(z[f'vox.{case}.points']).cuda()
    max_voxels = int(z[f'vox.{case}.max_voxels'])
    got = pkg.hard_voxelize(points, gen.VOX_SIZE, gen.VOX_RANGE, gen.MAX_POINTS, max_voxels)
    want = [torch.from_numpy(z[f'vox.{case}.{q}']) for q in ('voxels', 'coors', 'num_points')]
    for g, w, q in zip(got, want, ('voxels', 'coors', 'num_points')):
        assert same_bits(g.cpu(), w), f'{case}: {q} differs'
    again = pkg.hard_voxelize(points, gen.VOX_SIZE, gen.VOX_RANGE, gen.MAX_POINTS, max_voxels)
    assert all(same_bits(a, b) for a, b in zip(got, again))            # the same bits run after run
    layer = pkg.Voxelization(gen.VOX_SIZE, gen.VOX_RANGE, gen.MAX_POINTS, (7, max_voxels)).eval()
    assert all(same_bits(a, b) for a, b in zip(got, layer(points)))    # eval: the second of (training, testing)
    if case == 'crowded':                                               # a voxel keeps its FIRST five points
        assert int(got[2].max()) == 5
    if case == 'cut':
        assert got[1].shape[0] == 37
        full = pkg.hard_voxelize(points, gen.VOX_SIZE, gen.VOX_RANGE, gen.MAX_POINTS, 4000)
        assert full[1].shape[0] > 37 and same_bits(full[1][:37], got[1])    # the cut follows first-appearance order


def test_batched_voxelization_pads_with_minus_one_and_counts_on_the_device(pkg):
    z, gen = ref.fixture(), ref.generator()
    clouds = [torch.from_numpy(z[f'vox.batch.points{b}']).cuda() for b in range(3)]
    assert clouds[1].shape[0] == 0                                      # the middle sample is empty
    max_voxels = int(z['vox.batch.max_voxels'])
    voxels, coors, num, count = pkg.hard_voxelize_batch(clouds, gen.VOX_SIZE, gen.VOX_RANGE, gen.MAX_POINTS, max_voxels)
    assert count.is_cuda and count.dim() == 0
    rows = 3 * max_voxels
    assert voxels.shape == (rows, 5, 4) and coors.shape == (rows, 4) and coors.dtype == torch.int32 and num.shape == (rows, )
    want = [torch.from_numpy(z[f'vox.batch.{q}']) for q in ('voxels', 'coors', 'num_points')]
    m = want[1].shape[0]
    assert int(count) == m and 0 < m < rows
    assert same_bits(voxels[:m].cpu(), want[0]) and same_bits(coors[:m].cpu(), want[1]) and same_bits(num[:m].cpu(), want[2])
    assert (coors[m:] == -1).all() and not voxels[m:].any() and not num[m:].any()
    again = pkg.hard_voxelize_batch(clouds, gen.VOX_SIZE, gen.VOX_RANGE, gen.MAX_POINTS, max_voxels)
    assert all(same_bits(a, b) for a, b in zip((voxels, coors, num), again[:3]))
    feats = pkg.HardSimpleVFE(3)(voxels, num, coors)                    # divides on live rows only
    assert torch.isfinite(feats).all() and not feats[m:].any()
    total = want[0][:, 0, :3]
    for i in range(1, 5):
        total = total + want[0][:, i, :3]                               # slot order, as numpy's axis sum
    mean = total / want[2].float().view(-1, 1)
    assert same_bits(feats[:m].cpu(), mean)
    empty = pkg.hard_voxelize_batch([clouds[1], clouds[1]], gen.VOX_SIZE, gen.VOX_RANGE, gen.MAX_POINTS, 10)
    assert int(empty[3]) == 0 and (empty[1] == -1).all()


# ------------------------------------------------------------------------------------------------------------------
# helpers for inputs built here
# ------------------------------------------------------------------------------------------------------------------
def unique_coors(rng, shape, batch, count):
    cells = batch * shape[0] * shape[1] * shape[2]
    lin = torch.from_numpy(rng.choice(cells, count, replace=False))
    c = torch.stack([lin // (shape[0] * shape[1] * shape[2]), (lin // (shape[1] * shape[2])) % shape[0],
                     (lin // shape[2]) % shape[1], lin % shape[2]], dim=1)
    return c.int()


def dense_reference(feats, coors, shape, batch, weight, stride=1, padding=1, subm=True):
    """fp64 dense masked convolution of the scattered rows -> (volume (B, Cout, ...), mask (B, 1, ...), bound): the
    semantics of include/dfm_hip_sparse_conv.h restated, and the derived bound of every output element"""
    i = coors.long()
    vol = torch.zeros((batch, feats.shape[1], *shape), dtype=torch.float64)
    mask = torch.zeros((batch, 1, *shape), dtype=torch.float64)
    vol[i[:, 0], :, i[:, 1], i[:, 2], i[:, 3]] = feats.double()
    mask[i[:, 0], 0, i[:, 1], i[:, 2], i[:, 3]] = 1
    w = weight.double().permute(4, 3, 0, 1, 2)
    out = F.conv3d(vol, w, stride=stride, padding=padding)
    mag = F.conv3d(vol.abs(), w.abs(), stride=stride, padding=padding)
    omask = mask if subm else (F.conv3d(mask, torch.ones((1, 1, *weight.shape[:3]), dtype=torch.float64),
                                        stride=stride, padding=padding) > 0.5).double()
    terms = weight.shape[0] * weight.shape[1] * weight.shape[2] * weight.shape[3]
    return out * omask, omask, (terms + 2) * 2.0 ** -24 * mag


def run_layer(pkg, kind, feats, coors, shape, batch, weight, stride=1, padding=1):
    cls = getattr(pkg, kind)
    conv = cls(weight.shape[3], weight.shape[4], tuple(weight.shape[:3]), stride=stride, padding=padding, bias=False,
               indice_key='t').eval().cuda()
    with torch.no_grad():
        conv.weight.copy_(weight)
    x = pkg.SparseConvTensor(feats.cuda(), coors.cuda().contiguous(), shape, batch)
    out = conv(x)
    out.check_status()
    return out


# ------------------------------------------------------------------------------------------------------------------
# encoder: exact checks
# ------------------------------------------------------------------------------------------------------------------
def test_identity_centre_tap_returns_the_input_bit_for_bit(pkg):
    rng = np.random.default_rng(1)
    shape, batch = [9, 24, 20], 2
    coors = unique_coors(rng, shape, batch, 300)
    feats = torch.from_numpy(rng.normal(0, 1, (300, 16)).astype(np.float32))
    weight = torch.zeros(3, 3, 3, 16, 16)
    weight[1, 1, 1] = torch.eye(16)
    out = run_layer(pkg, 'SubMConv3d', feats, coors, shape, batch, weight)
    assert out.indices is not None and torch.equal(out.indices.cpu(), coors)      # the row set is the input's
    assert same_bits(out.features.cpu(), feats)


def test_fully_active_block_is_the_plain_dense_convolution(pkg):
    rng = np.random.default_rng(2)
    shape, batch = [5, 6, 7], 2
    cells = batch * 5 * 6 * 7
    coors = unique_coors(rng, shape, batch, cells)                                  # every cell, in random row order
    feats = torch.from_numpy(rng.normal(0, 1, (cells, 16)).astype(np.float32))
    weight = torch.from_numpy(ref.generator().weights(5, (3, 3, 3, 16, 32)))
    for kind, stride, padding in (('SubMConv3d', 1, 1), ('SparseConv3d', 2, 1), ('SparseConv3d', (2, 1, 1), (0, 1, 1))):
        out = run_layer(pkg, kind, feats, coors, shape, batch, weight, stride, padding)
        want, mask, bound = dense_reference(feats, coors, shape, batch, weight, stride, padding, kind == 'SubMConv3d')
        assert bool(mask.all())                                                     # every output site is active
        live = out.indices[out.indices[:, 0] >= 0]
        assert live.shape[0] == int(mask.sum()) == want.shape[0] * want[0, 0].numel()
        dense = out.dense().cpu().double()
        assert dense.shape == want.shape
        ratio = ((dense - want).abs() / bound.clamp_min(1e-300)).max().item()
        print(f'fully active {kind} stride {stride}: max error / derived bound = {ratio:.3f}')
        assert ratio <= 1.0


def test_samples_and_borders_do_not_see_each_other(pkg):
    shape, batch = [4, 5, 6], 2
    # last plane / row / column of sample 0, first of sample 1 (adjacent linear keys), and two cells of one sample
    # whose keys are adjacent but whose x coordinates are the two ends of a row
    coors = torch.tensor([[0, 3, 4, 5], [1, 0, 0, 0], [0, 1, 1, 5], [0, 1, 2, 0]], dtype=torch.int32)
    rng = np.random.default_rng(3)
    feats = torch.from_numpy(rng.normal(0, 1, (4, 16)).astype(np.float32))
    weight = torch.from_numpy(ref.generator().weights(6, (3, 3, 3, 16, 16)))
    together = run_layer(pkg, 'SubMConv3d', feats, coors, shape, batch, weight).features.cpu()
    for r in range(4):                                                              # each row alone: the same bits
        alone = run_layer(pkg, 'SubMConv3d', feats[r:r + 1], coors[r:r + 1], shape, batch, weight).features.cpu()
        assert same_bits(together[r:r + 1], alone), r
    centre = feats.double() @ weight[1, 1, 1].double()
    assert torch.allclose(together.double(), centre, rtol=0, atol=1e-5)             # only the centre tap contributes
    # the strided layer: outputs of sample 0 and sample 1 come from their own sample only
    out = run_layer(pkg, 'SparseConv3d', feats, coors, shape, batch, weight, 2, 1)
    want, mask, bound = dense_reference(feats, coors, shape, batch, weight, 2, 1, False)
    dense = out.dense().cpu().double()
    assert torch.equal(dense != 0, (want != 0)) and ((dense - want).abs() <= bound).all()
    assert not dense[mask.expand_as(dense) == 0].any()


@pytest.mark.parametrize('rows', [1, 63, 64, 65, 257])
def test_single_layer_row_counts_at_the_tile_edges(pkg, rows):
    rng = np.random.default_rng(10 + rows)
    shape, batch = [6, 7, 8], 2
    coors = unique_coors(rng, shape, batch, rows)
    feats = torch.from_numpy(rng.normal(0, 1, (rows, 16)).astype(np.float32))
    weight = torch.from_numpy(ref.generator().weights(7, (3, 3, 3, 16, 16)))
    for kind, stride in (('SubMConv3d', 1), ('SparseConv3d', 2)):
        out = run_layer(pkg, kind, feats, coors, shape, batch, weight, stride, 1)
        want, mask, bound = dense_reference(feats, coors, shape, batch, weight, stride, 1, kind == 'SubMConv3d')
        dense = out.dense().cpu().double()
        live = out.indices[out.indices[:, 0] >= 0]
        assert live.shape[0] == int(mask.sum())
        assert not dense[mask.expand_as(dense) == 0].any()                          # exactly 0 at every inactive site
        assert ((dense - want).abs() <= bound).all(), (kind, rows)
        if kind == 'SparseConv3d':
            assert int(out.num_rows) == live.shape[0]                               # the device's live count


def test_no_rows_give_a_zero_volume(pkg):
    shape, batch = [6, 7, 8], 2
    weight = torch.from_numpy(ref.generator().weights(8, (3, 3, 3, 16, 16)))
    feats, coors = torch.zeros(0, 16), torch.zeros(0, 4, dtype=torch.int32)
    for kind, stride, grid in (('SubMConv3d', 1, [6, 7, 8]), ('SparseConv3d', 2, [3, 4, 4])):
        out = run_layer(pkg, kind, feats, coors, shape, batch, weight, stride, 1)
        dense = out.dense()
        assert list(dense.shape) == [2, 16, *grid] and not dense.any()
    # rows that do not exist (b = -1) are no rows either
    coors = torch.full((70, 4), -1, dtype=torch.int32)
    out = run_layer(pkg, 'SubMConv3d', torch.ones(70, 16), coors, shape, batch, weight)
    assert not out.dense().any()
    enc = pkg.CustomSparseEncoder(sparse_shape=[9, 24, 20], **ref.generator().ENCODER_CFG).eval().cuda()
    spatial, volume = enc(torch.ones(70, 3).cuda(), coors.cuda(), 2)
    assert list(volume.shape) == [2, 32, 1, 6, 5] and not volume.any() and list(spatial.shape) == [2, 32, 6, 5]


# ------------------------------------------------------------------------------------------------------------------
# encoder: values against the fixture's fp64 stand-in
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['subm_3_16', 'subm_16_16', 'subm_32_32', 'subm_64_64', 'sp_s2_p1', 'sp_s211_p011',
                                  'sp_1x1'])
def test_single_layers_match_the_fp64_stand_in(pkg, name):
    z, gen = ref.fixture(), ref.generator()
    kind, cin, cout, k, s, p, shape, full, _ = gen.LAYERS[name]
    order = ('conv', 'norm', 'act') if full else ('conv', )
    m = pkg.make_sparse_convmodule(cin, cout, k, indice_key='k', stride=s, padding=p, conv_type=kind,
                                   norm_cfg=dict(type='BN1d', eps=1e-3, momentum=0.01), order=order)
    m.load_state_dict(ref.state_dict(f'layer.{name}'), strict=True)
    m = m.eval().cuda()
    x = pkg.SparseConvTensor(torch.from_numpy(z[f'layer.{name}.features']).cuda(),
                             torch.from_numpy(z[f'layer.{name}.coors']).cuda(), shape, 2)
    out = m(x)
    out.check_status()
    ref.compare_stage(f'layer.{name}.stage', out, name)


@pytest.fixture(scope='module')
def encoders(pkg):
    """both encoder cases, run once: case -> (encoder, stages, inputs)"""
    z, gen = ref.fixture(), ref.generator()
    out = {}
    for case in gen.ENCODERS:
        shape = [int(s) for s in z[f'enc.{case}.sparse_shape']]
        enc = pkg.CustomSparseEncoder(sparse_shape=shape, **gen.ENCODER_CFG)
        enc.load_state_dict(ref.state_dict(f'enc.{case}'), strict=True)
        enc = enc.eval().cuda()
        feats = torch.from_numpy(z[f'enc.{case}.features']).cuda()
        coors = torch.from_numpy(z[f'enc.{case}.coors']).cuda()
        batch = int(z[f'enc.{case}.batch'])
        stages = enc.forward_stages(feats, coors, batch)
        enc.check_status()
        out[case] = (enc, stages, (feats, coors, batch))
    return out


@pytest.mark.parametrize('case', ['enc_9_24_20', 'enc_11_25_19'])
def test_every_stage_of_the_encoder_matches_the_stand_in(encoders, case):
    """active sets as sorted linear keys (exact), exact zeros off them, values within the fixture's figure x 4; the
    second case has an empty sample in the middle of the batch"""
    enc, stages, (feats, coors, batch) = encoders[case]
    assert len(stages) == 6
    for i, stage in enumerate(stages):
        ref.compare_stage(f'enc.{case}.stage{i}', stage, f'{case} stage {i}')
    if case == 'enc_11_25_19':
        assert batch == 3 and not (coors[:, 0] == 1).any() and not stages[-1].dense()[1].any()
    # the SubM layers of a stage share one neighbour table per indice_key
    assert set(stages[-1].indice_dict) == {'subm1', 'subm2', 'subm3', 'subm4'}
    spatial, volume = enc(feats, coors, batch)
    assert same_bits(volume, stages[-1].dense()) and same_bits(spatial, volume.view(batch, -1, *volume.shape[3:]))


@pytest.mark.parametrize('case', ['enc_9_24_20', 'enc_11_25_19'])
def test_permuted_rows_and_repeated_runs_give_the_same_bits(encoders, case):
    enc, stages, (feats, coors, batch) = encoders[case]
    want = stages[-1].dense()
    _, again = enc(feats, coors, batch)
    assert same_bits(again, want)
    perm = torch.from_numpy(np.random.default_rng(4).permutation(feats.shape[0])).cuda()
    _, permuted = enc(feats[perm].contiguous(), coors[perm].contiguous(), batch)
    assert same_bits(permuted, want)
    # padding rows (b = -1) anywhere among the rows change nothing either
    pad = torch.full((37, 4), -1, dtype=torch.int32, device='cuda')
    junk = torch.full((37, 3), float('nan'), device='cuda')
    _, padded = enc(torch.cat([junk[:20], feats, junk[20:]]), torch.cat([pad[:20], coors, pad[20:]]), batch)
    assert same_bits(padded, want)


# ------------------------------------------------------------------------------------------------------------------
# the path
# ------------------------------------------------------------------------------------------------------------------
def test_lidar_teacher_end_to_end(pkg):
    z, gen = ref.fixture(), ref.generator()
    cfg = dict(type='VoxelNet',
               voxel_layer=dict(max_num_points=gen.MAX_POINTS, point_cloud_range=gen.PATH_RANGE,
                                voxel_size=gen.VOX_SIZE, max_voxels=(400, 400)),
               voxel_encoder=dict(type='HardSimpleVFE', num_features=3),
               middle_encoder=dict(type='CustomSparseEncoder', sparse_shape=gen.PATH_SHAPE, **gen.ENCODER_CFG),
               backbone=dict(type='BEVHourglass', in_channels=32, out_channels=64, norm_cfg=dict(type='SyncBN'),
                             output_prehg_feat=False), neck=None, bbox_head=None)
    torch.manual_seed(0)
    teacher = pkg.LidarTeacher(cfg)
    teacher.middle_encoder.load_state_dict(ref.state_dict('path'), strict=True)
    teacher = teacher.cuda()
    clouds = [torch.from_numpy(z[f'path.points{b}']).cuda() for b in range(2)]
    prev = pkg.set_fallback_policy('silent')       # the fp32 BEV hourglass runs torch's convolutions: not under test
    try:
        volume, bev = teacher(clouds)
        teacher.check_status()
        # the voxel features the encoder saw are the stand-in's inputs, bit for bit
        voxels, coors, num, count = teacher.voxel_layer.forward_batch(clouds)
        m = int(count)
        assert m == z['path.coors'].shape[0] and same_bits(coors[:m].cpu(), torch.from_numpy(z['path.coors']))
        assert same_bits(teacher.voxel_encoder(voxels, num, coors)[:m].cpu(), torch.from_numpy(z['path.voxel_features']))
        last = teacher.middle_encoder._last
        dense = ref.compare_stage('path.volume', last, 'LidarTeacher volume_feat')
        assert same_bits(volume, dense) and list(volume.shape) == [2, 32, 1, 8, 4]
        spatial, volume2 = teacher.middle_encoder(teacher.voxel_encoder(voxels, num, coors), coors, 2)
        assert same_bits(volume2, volume) and same_bits(spatial, volume.view(2, 32, 8, 4))
        assert list(bev.shape) == [2, 64, 8, 4] and torch.isfinite(bev).all()
        # a side stream gives the same bits
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            volume_side, bev_side = teacher(clouds)
        torch.cuda.current_stream().wait_stream(side)
        assert same_bits(volume_side, volume) and torch.allclose(bev_side, bev, rtol=1e-4, atol=1e-5)
    finally:
        pkg.set_fallback_policy(prev)


def test_duplicate_coordinates_are_reported(pkg):
    z, gen = ref.fixture(), ref.generator()
    enc = pkg.CustomSparseEncoder(sparse_shape=[9, 24, 20], **gen.ENCODER_CFG).eval().cuda()
    coors = torch.from_numpy(z['enc.enc_9_24_20.coors']).cuda().clone()
    feats = torch.from_numpy(z['enc.enc_9_24_20.features']).cuda()
    enc(feats, coors, 2)
    enc.check_status()                                                              # clean input: nothing to report
    coors[5] = coors[100]
    enc(feats, coors, 2)
    with pytest.raises(pkg._capi.DfmHipError, match='duplicate'):
        enc.check_status()
    coors = torch.from_numpy(z['enc.enc_9_24_20.coors']).cuda().clone()
    coors[7, 2] = 24                                                                # y outside the grid
    enc(feats, coors, 2)
    with pytest.raises(pkg._capi.DfmHipError, match='outside the grid'):
        enc.check_status()
