"""CPU: training the sparse encoder above its kernels -- the switch ``enable_sparse_training`` (what it marks, that
unmarked modules refuse as before), the refusals of marked modules (eval mode with a gradient, basicblock, dtype,
SyncBN in a group of more than one rank, an input gradient for Cin = 3), the new header against its binding table and
the library, argument checks that need no device, and the fixture's integrity.

Fixture: tests/golden/sparse_train*.npz (generator tests/golden/make_golden_sparse_train.py)."""
import ctypes
import importlib
import os

import numpy as np
import pytest
import torch

from tests import sparse_train_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('dfm_sparse_inverse_table', 'dfm_sparse_conv_wgrad_workspace_bytes', 'dfm_sparse_conv_wgrad',
       'dfm_sparse_bn_workspace_bytes', 'dfm_sparse_bn_stats', 'dfm_sparse_bn_apply', 'dfm_sparse_bn_bwd_reduce',
       'dfm_sparse_bn_bwd_apply', 'dfm_sparse_bn_running', 'dfm_sparse_dense_bwd')
NORM = dict(type='BN1d', eps=1e-3, momentum=0.01)


@pytest.fixture(scope='module')
def pkg():
    importlib.import_module('depth-from-motion_amd.build').build_hip()
    return importlib.import_module('depth-from-motion_amd')


class OnGpu(torch.Tensor):
    """a CPU tensor that says it is on the GPU: the checks under test come before any launch"""
    is_cuda = True


def fake(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype).as_subclass(OnGpu)


def sparse(pkg, channels, dtype=torch.float32, grad=False):
    feats = fake(4, channels, dtype=dtype)
    return pkg.SparseConvTensor(feats.requires_grad_() if grad else feats, fake(4, 4, dtype=torch.int32), [4, 4, 4], 1)


def test_the_default_refusals_stand_without_the_switch(pkg):
    assert 'enable_sparse_training' in pkg.__all__
    seq = pkg.make_sparse_convmodule(16, 16, 3, 'k', norm_cfg=NORM)
    assert not seq.sparse_training and not seq[0].sparse_training
    with pytest.raises(pkg.MfmaPathError, match='training mode'):
        seq(sparse(pkg, 16))
    with pytest.raises(pkg.MfmaPathError, match='training mode'):
        pkg.SubMConv3d(16, 16, 3, bias=False).train()(sparse(pkg, 16))
    with pytest.raises(pkg.MfmaPathError, match='requires grad'):
        pkg.SubMConv3d(16, 16, 3, bias=False).eval()(sparse(pkg, 16, grad=True))


def test_the_switch_marks_and_unmarks_the_tree(pkg):
    gen = ref.generator().gen
    enc = pkg.CustomSparseEncoder(sparse_shape=[9, 24, 20], **gen.ENCODER_CFG)
    keys = list(enc.state_dict())
    names = pkg.enable_sparse_training(enc)
    marked = [n for n, m in enc.named_modules() if getattr(m, 'sparse_training', False)]
    assert names == marked and 'conv_input' in names and 'conv_input.0' in names and 'conv_out.0' in names
    kinds = (pkg.SubMConv3d, pkg.SparseConv3d, pkg.SparseSequential)
    assert all(m.sparse_training for m in enc.modules() if isinstance(m, kinds))
    assert len([m for m in enc.modules() if isinstance(m, kinds[:2])]) == 12
    assert list(enc.state_dict()) == keys                                   # a mark is no parameter and no buffer
    assert pkg.enable_sparse_training(enc, enabled=False) == names
    assert not any(getattr(m, 'sparse_training', False) for m in enc.modules())
    with pytest.raises(pkg.MfmaPathError, match='training mode'):
        enc.conv_input(sparse(pkg, 3))                                      # unmarked again: today's refusal
    teacher = pkg.LidarTeacher(dict(
        type='VoxelNet', voxel_layer=dict(max_num_points=5, point_cloud_range=[2, -30.4, -3, 59.6, 30.4, 1],
                                          voxel_size=[0.05, 0.05, 0.1], max_voxels=(40000, 40000)),
        voxel_encoder=dict(type='HardSimpleVFE', num_features=3),
        middle_encoder=dict(type='CustomSparseEncoder', in_channels=3, output_channels=32, sparse_shape=[41, 1216, 1152],
                            order=('conv', 'norm', 'act'), norm_cfg=dict(type='SyncBN', eps=1e-3, momentum=0.01),
                            encoder_strides=((1, ), (2, 1, 1), (2, 1, 1), ((2, 1, 1), 1, 1)), with_final_bnrelu=False,
                            output_volume_feat=True),
        backbone=dict(type='BEVHourglass', in_channels=160, out_channels=64, norm_cfg=dict(type='SyncBN'),
                      output_prehg_feat=False), neck=None, bbox_head=None,
        init_cfg=dict(type='Pretrained', checkpoint='teacher.pth')))
    pkg.enable_sparse_training(teacher)
    teacher.train()
    assert not any(m.training for m in teacher.modules())                   # the teacher stays frozen
    assert not any(p.requires_grad for p in teacher.parameters())


def test_marked_modules_refuse_what_the_kernels_do_not_cover(pkg, monkeypatch):
    conv = pkg.SubMConv3d(16, 16, 3, bias=False)
    pkg.enable_sparse_training(conv)
    for policy in ('warn', 'raise', 'silent'):
        prev = pkg.set_fallback_policy(policy)
        try:
            conv.eval()
            with pytest.raises(pkg.MfmaPathError, match='eval mode with an input or a weight that needs a gradient'):
                conv(sparse(pkg, 16, grad=True))
            with pytest.raises(pkg.MfmaPathError, match='frozen-BN'):
                conv(sparse(pkg, 16))                                       # the weight needs a gradient
            conv.train()
            with pytest.raises(pkg.MfmaPathError, match='dtype'):
                conv(sparse(pkg, 16, dtype=torch.bfloat16))
            with pytest.raises(pkg.MfmaPathError, match='dtype'):
                pkg.enable_sparse_training(conv.bfloat16())
                conv(sparse(pkg, 16))
            conv.float()
            with pytest.raises(pkg.MfmaPathError, match='basicblock'):
                pkg.CustomSparseEncoder(3, [9, 24, 20], block_type='basicblock')
            with pytest.raises(pkg.MfmaPathError, match='channels 24->24'):
                c24 = pkg.SparseConv3d(24, 24, 3, bias=False)
                pkg.enable_sparse_training(c24)
                c24(sparse(pkg, 24))
            c3 = pkg.SubMConv3d(3, 16, 3, bias=False)
            pkg.enable_sparse_training(c3)
            with pytest.raises(pkg.MfmaPathError, match='input gradient for Cin = 3'):
                c3._run(sparse(pkg, 3, grad=True), None, None, None, False)
            # a marked convolution inside an unmarked SparseSequential: the epilogue cannot run in training mode
            seq = pkg.make_sparse_convmodule(16, 16, 3, 'k', norm_cfg=NORM)
            pkg.enable_sparse_training(seq[0])
            with pytest.raises(pkg.MfmaPathError, match='whole tree'):
                seq[0]._run(sparse(pkg, 16), None, None, seq[1], True)
        finally:
            pkg.set_fallback_policy(prev)

    # SyncBN in an initialised group of more than one rank; the batch norm's checks come before any launch
    st = importlib.import_module('depth-from-motion_amd.sparse_train')
    feats, idx = fake(4, 16), fake(4, 4, dtype=torch.int32)
    sync = pkg.make_sparse_convmodule(16, 16, 3, 'k', norm_cfg=dict(type='SyncBN', eps=1e-3, momentum=0.01))[1]
    assert sync.cross_rank and not pkg.make_sparse_convmodule(16, 16, 3, 'k', norm_cfg=NORM)[1].cross_rank
    dist = torch.distributed
    monkeypatch.setattr(dist, 'is_available', lambda: True)
    monkeypatch.setattr(dist, 'is_initialized', lambda: True)
    monkeypatch.setattr(dist, 'get_world_size', lambda group=None: 2)
    for bn in (sync, torch.nn.SyncBatchNorm(16, eps=1e-3, momentum=0.01)):
        with pytest.raises(pkg.MfmaPathError, match='SyncBN in a process group of 2 ranks'):
            st.batch_norm_rows(feats, idx, bn.train(), True)
    with pytest.raises(pkg.MfmaPathError, match='frozen-BN'):
        st.batch_norm_rows(feats, idx, torch.nn.BatchNorm1d(16).eval(), True)
    with pytest.raises(pkg.MfmaPathError, match='momentum=None'):
        st.batch_norm_rows(feats, idx, torch.nn.BatchNorm1d(16, momentum=None), True)
    with pytest.raises(pkg.MfmaPathError, match='24 channels'):
        st.batch_norm_rows(fake(4, 24), idx, torch.nn.BatchNorm1d(24), True)
    with pytest.raises(pkg.MfmaPathError, match='dtype'):
        st.batch_norm_rows(feats, idx, torch.nn.BatchNorm1d(16).double(), True)


def test_header_binding_and_library_agree_on_the_new_symbols(pkg):
    """that header, table and library agree is tests/test_capi_binding.py; here: what this header says of its own"""
    text = open(os.path.join(ROOT, 'include', 'dfm_hip_sparse_train.h')).read()
    capi = pkg._capi
    assert all(n in capi._BINDING['dfm_hip_sparse_train.h'] and capi.SIGNATURES[n][0] in (ctypes.c_int, ctypes.c_size_t)
               for n in NEW)                                  # each returns a status or a size
    assert f'#define DFM_SPARSE_WGRAD_CHUNK {capi.SPARSE_WGRAD_CHUNK} ' in text
    assert f'#define DFM_SPARSE_BN_CHUNK {capi.SPARSE_BN_CHUNK} ' in text
    for phrase in ('exactly 0', 'ascending chunk order', 'v_mfma_f32_16x16x4_f32', 'inv[k] = nbr[26 - k]',
                   'max(count - 1, 1)', 'a live count of 0 leaves', '(live count, mean, M2'):
        assert phrase in text, phrase


def test_the_c_abi_rejects_bad_arguments_without_a_gpu(pkg):
    capi = pkg._capi
    lib = capi.lib()
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)      # aligned host memory, never dereferenced
    odd = ctypes.c_void_p(p.value + 2)
    size = (ctypes.c_int32 * 3)(8, 8, 8)
    bad, unsup = -1, capi.DFM_ERR_UNSUPPORTED
    inv = lib.dfm_sparse_inverse_table
    assert inv(None, 27, 10, 10, p, None) == bad and b'NULL' in lib.dfm_last_error()
    assert inv(p, 27, 10, 10, None, None) == bad and inv(p, 0, 10, 10, p, None) == bad
    assert inv(p, 27, -1, 10, p, None) == bad and inv(p, 28, 10, 10, p, None) == unsup
    assert inv(p, 27, 1 << 30, 10, p, None) == unsup and inv(None, 27, 0, 10, None, None) == 0
    wb, wg = lib.dfm_sparse_conv_wgrad_workspace_bytes, lib.dfm_sparse_conv_wgrad
    assert wb(16, 16, 27, 513) == 3 * 27 * (16 * 16 + 1) * 4 and wb(3, 64, 27, 256) == 27 * (16 * 64 + 1) * 4
    assert wb(64, 32, 1, 1) == (64 * 32 + 1) * 4 and wb(20, 16, 27, 10) == 27 * (32 * 16 + 1) * 4
    assert wb(5, 16, 27, 10) == 0 and wb(16, 48, 27, 10) == 0 and wb(16, 16, 28, 10) == 0 and wb(16, 16, 27, -1) == 0
    big = 1 << 20
    assert wg(16, 16, 27, None, 10, p, p, 10, p, p, p, big, None, None) == bad and b'NULL' in lib.dfm_last_error()
    assert wg(16, 16, 27, p, 10, p, None, 10, p, p, p, big, None, None) == bad
    assert wg(16, 16, 27, p, 10, p, p, 10, None, p, p, big, None, None) == bad
    assert wg(16, 16, 27, p, 10, p, p, 10, p, None, p, big, None, None) == bad
    assert wg(16, 16, 27, p, 10, p, p, 10, p, p, None, big, None, None) == bad
    assert wg(16, 16, 27, p, 10, None, p, 10, p, p, p, big, None, None) == bad       # no table for 27 offsets
    assert wg(16, 16, 1, p, 5, None, p, 10, p, p, p, big, None, None) == bad         # one offset, but fewer input rows
    assert wg(16, 16, 27, p, 10, p, p, 10, p, p, p, 100, None, None) == bad and b'workspace' in lib.dfm_last_error()
    assert wg(16, 16, 27, p, 10, p, p, 10, odd, p, p, big, None, None) == bad and b'aligned' in lib.dfm_last_error()
    assert wg(16, 16, 27, p, -1, p, p, 10, p, p, p, big, None, None) == bad and wg(0, 16, 27, p, 1, p, p, 1, p, p, p, big, None, None) == bad
    for cin, cout in ((5, 16), (128, 16), (16, 48), (16, 128)):
        assert wg(cin, cout, 27, p, 10, p, p, 10, p, p, p, big, None, None) == unsup and b'channels' in lib.dfm_last_error()
    assert wg(16, 16, 28, p, 10, p, p, 10, p, p, p, big, None, None) == unsup
    bw = lib.dfm_sparse_bn_workspace_bytes
    assert bw(257, 32) == 2 * 32 * 3 * 4 and bw(0, 16) == 0 and bw(10, 24) == 0 and bw(-1, 16) == 0
    st, ap = lib.dfm_sparse_bn_stats, lib.dfm_sparse_bn_apply
    assert st(None, p, 10, 16, p, p, big, None, None) == bad and b'NULL' in lib.dfm_last_error()
    assert st(p, None, 10, 16, p, p, big, None, None) == bad and st(p, p, 10, 16, None, p, big, None, None) == bad
    assert st(p, p, 10, 16, p, None, big, None, None) == bad and st(p, p, 10, 16, p, p, 8, None, None) == bad
    assert st(p, p, 10, 24, p, p, big, None, None) == unsup and b'channels' in lib.dfm_last_error()
    assert st(p, p, -1, 16, p, p, big, None, None) == bad and st(p, p, 10, 16, odd, p, big, None, None) == bad
    assert ap(p, p, 10, 16, None, p, p, 1e-3, 1, p, None) == bad and ap(p, p, 10, 16, p, p, p, 1e-3, 1, None, None) == bad
    assert ap(p, p, 10, 16, p, p, p, 0.0, 1, p, None) == bad and b'eps' in lib.dfm_last_error()
    assert ap(p, p, 10, 48, p, p, p, 1e-3, 1, p, None) == unsup and ap(None, None, 0, 16, p, None, None, 1e-3, 1, None, None) == 0
    br, ba = lib.dfm_sparse_bn_bwd_reduce, lib.dfm_sparse_bn_bwd_apply
    assert br(p, None, p, 10, 16, p, p, p, 1e-3, 1, p, p, big, None, None) == bad
    assert br(p, p, p, 10, 16, p, p, p, 1e-3, 1, None, p, big, None, None) == bad
    assert br(p, p, p, 10, 16, p, p, p, 1e-3, 1, p, p, 8, None, None) == bad and br(p, p, p, 10, 20, p, p, p, 1e-3, 1, p, p, big, None, None) == unsup
    assert ba(p, p, p, 10, 16, p, None, p, p, 1e-3, 1, p, None) == bad and ba(p, p, p, 10, 16, p, p, p, p, 1e-3, 1, None, None) == bad
    assert ba(p, p, p, 10, 16, p, p, p, p, -1.0, 1, p, None) == bad and ba(p, p, p, 10, 8, p, p, p, p, 1e-3, 1, p, None) == unsup
    run = lib.dfm_sparse_bn_running
    assert run(None, 16, 0.01, p, p, None) == bad and run(p, 16, 0.01, None, p, None) == bad
    assert run(p, 16, 1.5, p, p, None) == bad and b'momentum' in lib.dfm_last_error() and run(p, 24, 0.01, p, p, None) == unsup
    db = lib.dfm_sparse_dense_bwd
    assert db(None, p, 10, 16, 1, size, p, None) == bad and db(p, p, 10, 16, 1, size, None, None) == bad
    assert db(p, p, 10, 16, 1, None, p, None) == bad and db(p, p, 10, 0, 1, size, p, None) == bad
    assert db(p, p, 10, 16, 0, size, p, None) == bad and db(p, ctypes.c_void_p(p.value + 4), 10, 16, 1, size, p, None) == bad
    assert db(None, None, 0, 16, 1, size, None, None) == 0                     # no rows: a valid no-op


def test_the_fixture_is_small_and_whole(pkg):
    z, mod = ref.fixture(), ref.generator()
    gen = mod.gen
    for name in ref.FILES:
        assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', name)) <= 1 << 20, name
    cases = [f'layer.{n}' for n in gen.LAYERS] + [f'enc.{n}' for n in gen.ENCODERS]
    assert len(cases) == 9
    for prefix in cases:
        sd = ref.state_dict(prefix)                                 # regenerated weights match the stored digests
        big = ref.side('layers' if prefix.startswith('layer.') else prefix[4:])
        norms = [k for k in sd if k.endswith('running_mean')]
        # the mask-margin condition the seed was chosen by: every |pre-ReLU value| lies outside the forward's bar
        ratio, seed = float(z[f'{prefix}.pre_ratio']), int(z[f'{prefix}.case_seed'])
        assert ratio > 1.0 and 0 <= seed < mod.MAX_SEEDS, prefix
        assert np.isinf(ratio) == (not norms)
        assert f'{prefix}.grad_in' in big and 0 < float(z[f'{prefix}.grad_in.err']) < 1e-5
        for key, value in sd.items():
            if value.dim() == 5:
                full = f'{prefix}.dw.{key}' in big
                assert full == (value.numel() <= mod.FULL_DW) and full != (f'{prefix}.proj.{key}' in z.files)
                if full:
                    assert big[f'{prefix}.dw.{key}'].shape == tuple(value.shape)
                else:
                    assert z[f'{prefix}.proj.{key}'].shape == (mod.PROJECTIONS, )
            elif key.endswith(('weight', 'bias')):
                assert z[f'{prefix}.grad.{key}'].dtype == np.float64
            elif key.endswith(('running_mean', 'running_var')):
                assert not np.array_equal(z[f'{prefix}.after.{key}'], z[f'{prefix}.bn.{key}'].astype(np.float64))
        for key in z.files:
            if key.startswith(prefix + '.') and key.endswith('.err'):
                assert 2.0 ** -23 <= float(z[key]) < 1e-5, key     # every figure is floored, none is large
    assert ref.side('layers')['layer.subm_64_64.grad_in'].shape == (200, 64)
    assert 'enc.enc_9_24_20.grad_stage0' in z.files and 'layer.subm_64_64.proj.0.weight' in z.files
