"""CPU: the validation contract of the C-ABI entry points whose host code states its checks through shared helpers --
which status and which dfm_last_error() text a bad call gets, and which check wins when two things are wrong.

One table: (entry point, the arguments that differ from a valid call) -> (status, a piece of the message).  Every row
is refused before any HIP call, so the file needs no device and is safe on one: pointers are None or an address that
is never dereferenced (0x1000, 16-byte aligned; 0x1004 for the alignment rows), and no row is a valid call -- a row
that got past validation would come back DFM_ERR_HIP here (no device) and fail its status check."""
import ctypes
import importlib

import pytest

P, ODD = 0x1000, 0x1004
BIG = 1 << 42                      # "enough workspace": the byte count is compared, the memory never touched
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
NULL, DTYPE = 'NULL device pointer', 'dtype must be DFM_F32 or DFM_BF16'
GN_CL = 'channels-last GroupNorm needs C = 16-byte vectors x a power of two, C <= 256'
BN_CL = 'channels-last BatchNorm needs C = 16-byte vectors x a power of two, C <= 256'
GN_WS = 'workspace smaller than dfm_group_norm_workspace_bytes'
BN_WS = 'workspace smaller than dfm_batch_norm_workspace_bytes'
MV_BATCHED = 'batched lifting: nearest mode'


@pytest.fixture(scope='module')
def capi():
    importlib.import_module('depth-from-motion_amd.build').build_hip()
    return importlib.import_module('depth-from-motion_amd')._capi


def _sig(text):
    """'n=2 c=32 x=P' -> ordered {name: value}: one VALID call's arguments, in the order of the C declaration"""
    out = {}
    for item in text.split():
        k, v = item.split('=')
        out[k] = {'P': P, 'BIG': BIG}[v] if v in ('P', 'BIG') else float(v) if '.' in v else int(v)
    return out


_GN_HEAD = 'n=2 c=32 spatial=64 groups=8 eps=0.00001 dtype=0 relu=0 x=P gamma=P beta=P '
_GN_BWD_HEAD = 'n=2 c=32 spatial=64 groups=8 dtype=0 relu=1 grad_y=P x=P y=P mean=P rstd=P gamma=P '
_BN_BWD_HEAD = 'c=32 rows=64 dtype=0 relu=1 grad_y=P x=P y=P mean=P rstd=P gamma=P beta=P '
VALID = {
    'dfm_group_norm_coefficients': _sig('n=2 c=32 groups=8 eps=0.00001 partials=P splits=4 gamma=P beta=P coef=P '
                                        'stream=0'),
    'dfm_group_norm_fwd': _sig(_GN_HEAD + 'y=P mean=P rstd=P workspace=P workspace_bytes=BIG stream=0'),
    'dfm_group_norm_fwd_channels_last': _sig(_GN_HEAD + 'y=P mean=P rstd=P workspace=P workspace_bytes=BIG stream=0'),
    'dfm_group_norm_fwd_channels_last_res': _sig(_GN_HEAD + 'residual=P y=P mean=P rstd=P workspace=P '
                                                 'workspace_bytes=BIG stream=0'),
    'dfm_group_norm_apply_channels_last': _sig(_GN_HEAD + 'y=P mean=P rstd=P partials=P splits=4 workspace=P '
                                               'workspace_bytes=BIG stream=0'),
    'dfm_group_norm_apply_channels_last_res': _sig(_GN_HEAD + 'residual=P y=P mean=P rstd=P partials=P splits=4 '
                                                   'workspace=P workspace_bytes=BIG stream=0'),
    'dfm_group_norm_bwd': _sig(_GN_BWD_HEAD + 'grad_x=P grad_gamma=P grad_beta=P workspace=P workspace_bytes=BIG '
                               'stream=0'),
    'dfm_group_norm_bwd_channels_last': _sig(_GN_BWD_HEAD + 'grad_x=P grad_residual=P grad_gamma=P grad_beta=P '
                                             'workspace=P workspace_bytes=BIG stream=0'),
    'dfm_group_norm_bwd_channels_last_xmask': _sig('n=2 c=32 spatial=64 groups=8 dtype=0 grad_y=P x=P mean=P rstd=P '
                                                   'gamma=P beta=P grad_x=P grad_gamma=P grad_beta=P workspace=P '
                                                   'workspace_bytes=BIG stream=0'),
    'dfm_batch_norm_stats_channels_last': _sig('c=32 rows=64 dtype=0 x=P stats=P workspace=P workspace_bytes=BIG '
                                               'stream=0'),
    'dfm_batch_norm_apply_gathered_channels_last': _sig('c=32 rows=64 world=2 eps=0.00001 dtype=0 relu=0 x=P gamma=P '
                                                        'beta=P residual=P gathered=P y=P mean=P rstd=P moments=P '
                                                        'stream=0'),
    'dfm_batch_norm_bwd_reduce_channels_last': _sig(_BN_BWD_HEAD + 'sums=P workspace=P workspace_bytes=BIG stream=0'),
    'dfm_batch_norm_bwd_apply_channels_last': _sig(_BN_BWD_HEAD + 'sums=P count=P grad_x=P grad_residual=P '
                                                   'workspace=P workspace_bytes=BIG stream=0'),
    'dfm_depth_head_fwd': _sig('batch=1 d=8 h=4 w=4 scale=2 dtype=0 cost=P depth_samples=P depth_volumes=P softmax=P '
                               'depth_preds=P stream=0'),
    'dfm_depth_head_stats_fwd': _sig('batch=1 d=8 h=4 w=4 scale=2 dtype=0 cost=P depth_samples=P col_max=P col_sum=P '
                                     'depth_preds=P stream=0'),
    'dfm_cost_gate_fwd': _sig('batch=1 num_depths=24 hw=64 dtype=0 stereo=P mono=P packed_weights=P out=P stream=0'),
    'dfm_cost_gate_pack_weights': _sig('weight=P weight_dtype=0 num_depths=24 packed=P stream=0'),
    'dfm_cost_gate_mfma_pack_weights': _sig('weight=P weight_dtype=0 num_depths=24 packed=P stream=0'),
}

# ---- the table: (entry point, what differs from VALID[entry point], status, piece of dfm_last_error()) ----------------
ROWS = []


def rows(name, *items):
    ROWS.extend((name, bad, status, text) for bad, status, text in items)


rows('dfm_group_norm_coefficients',
     (dict(n=0), INVALID, 'bad sizes in dfm_group_norm_coefficients'),
     (dict(c=30), INVALID, 'bad sizes in dfm_group_norm_coefficients'),
     (dict(splits=0), INVALID, 'bad sizes in dfm_group_norm_coefficients'),
     (dict(partials=None), INVALID, NULL),
     (dict(coef=None), INVALID, NULL),
     (dict(splits=0, coef=None), INVALID, 'bad sizes'))                                 # sizes before pointers
rows('dfm_group_norm_fwd',
     (dict(n=0), INVALID, 'bad sizes in dfm_group_norm_fwd'),
     (dict(c=30), INVALID, 'bad sizes in dfm_group_norm_fwd'),
     (dict(spatial=0), INVALID, 'bad sizes in dfm_group_norm_fwd'),
     (dict(dtype=7), UNSUPPORTED, DTYPE),
     (dict(x=None), INVALID, NULL),
     (dict(rstd=None), INVALID, NULL),
     (dict(workspace=None), INVALID, NULL),
     (dict(workspace_bytes=1024), WORKSPACE, GN_WS),
     (dict(n=65536, c=1, groups=1), UNSUPPORTED, 'n*groups > 65535'),
     (dict(groups=0, dtype=7), INVALID, 'bad sizes'),                                   # sizes before dtype
     (dict(dtype=7, x=None), UNSUPPORTED, DTYPE),                                       # dtype before pointers
     (dict(y=None, workspace_bytes=0), INVALID, NULL),                                  # pointers before workspace
     (dict(n=65536, c=1, groups=1, workspace_bytes=1024), WORKSPACE, GN_WS))            # workspace before the grid limit
for _name in ('dfm_group_norm_fwd_channels_last', 'dfm_group_norm_fwd_channels_last_res'):
    rows(_name,
         (dict(n=0), INVALID, 'bad sizes in dfm_group_norm_fwd_channels_last'),
         (dict(c=30), INVALID, 'bad sizes in dfm_group_norm_fwd_channels_last'),
         (dict(dtype=7), UNSUPPORTED, DTYPE),
         (dict(x=None), INVALID, NULL),
         (dict(mean=None), INVALID, NULL),
         (dict(workspace_bytes=1024), WORKSPACE, GN_WS),
         (dict(c=12, groups=4), UNSUPPORTED, GN_CL),
         (dict(c=24, groups=4, dtype=1), UNSUPPORTED, GN_CL),
         (dict(c=4, groups=4, dtype=1), UNSUPPORTED, GN_CL),                            # not a whole bf16 vector
         (dict(c=512), UNSUPPORTED, GN_CL),
         (dict(n=65536), UNSUPPORTED, GN_CL),
         (dict(x=ODD), UNSUPPORTED, GN_CL),
         (dict(y=ODD), UNSUPPORTED, GN_CL),
         (dict(spatial=-1, dtype=7), INVALID, 'bad sizes'),
         (dict(dtype=7, gamma=None), UNSUPPORTED, DTYPE),
         (dict(beta=None, workspace_bytes=0), INVALID, NULL),
         (dict(c=12, groups=4, workspace_bytes=0), WORKSPACE, GN_WS))                   # workspace before the shape limits
for _name in ('dfm_group_norm_apply_channels_last', 'dfm_group_norm_apply_channels_last_res'):
    rows(_name,
         (dict(groups=0), INVALID, 'bad sizes in dfm_group_norm_apply_channels_last'),
         (dict(splits=0), INVALID, 'bad sizes in dfm_group_norm_apply_channels_last'),
         (dict(dtype=7), UNSUPPORTED, DTYPE),
         (dict(partials=None), INVALID, NULL),
         (dict(y=None), INVALID, NULL),
         (dict(workspace_bytes=2 * 8 * 3 * 4 - 1), WORKSPACE, 'workspace smaller than n*groups*3 floats'),
         (dict(c=12, groups=4), UNSUPPORTED, GN_CL),
         (dict(c=24, groups=4, dtype=1), UNSUPPORTED, GN_CL),
         (dict(c=512), UNSUPPORTED, GN_CL),
         (dict(x=ODD), UNSUPPORTED, GN_CL),
         (dict(y=ODD), UNSUPPORTED, GN_CL),
         (dict(splits=-1, dtype=7), INVALID, 'bad sizes'),
         (dict(dtype=-1, partials=None), UNSUPPORTED, DTYPE),
         (dict(workspace=None, workspace_bytes=0), INVALID, NULL),
         (dict(c=512, workspace_bytes=0), WORKSPACE, 'n*groups*3 floats'))
rows('dfm_group_norm_bwd',
     (dict(n=0), INVALID, 'bad sizes in dfm_group_norm_bwd'),
     (dict(c=30), INVALID, 'bad sizes in dfm_group_norm_bwd'),
     (dict(dtype=7), UNSUPPORTED, DTYPE),
     (dict(grad_y=None), INVALID, NULL),
     (dict(y=None), INVALID, NULL),                                                     # relu = 1 needs y
     (dict(grad_beta=None), INVALID, NULL),
     (dict(workspace_bytes=1024), WORKSPACE, GN_WS),
     (dict(n=2048, c=32), UNSUPPORTED, 'n*c > 65535'),
     (dict(spatial=0, dtype=7), INVALID, 'bad sizes'),
     (dict(dtype=7, y=None), UNSUPPORTED, DTYPE),
     (dict(grad_x=None, workspace_bytes=0), INVALID, NULL),
     (dict(n=2048, c=32, workspace_bytes=1024), WORKSPACE, GN_WS))
rows('dfm_group_norm_bwd_channels_last',
     (dict(n=0), INVALID, 'bad sizes in dfm_group_norm_bwd_channels_last'),
     (dict(c=30), INVALID, 'bad sizes in dfm_group_norm_bwd_channels_last'),
     (dict(dtype=7), UNSUPPORTED, DTYPE),
     (dict(y=None), INVALID, NULL),
     (dict(grad_y=None), INVALID, NULL),
     (dict(grad_gamma=None), INVALID, NULL),
     (dict(workspace_bytes=1024), WORKSPACE, GN_WS),
     (dict(c=12, groups=4), UNSUPPORTED, GN_CL),
     (dict(c=24, groups=4, dtype=1), UNSUPPORTED, GN_CL),
     (dict(c=512), UNSUPPORTED, GN_CL),
     (dict(n=65536), UNSUPPORTED, GN_CL),
     (dict(x=ODD), UNSUPPORTED, GN_CL),
     (dict(grad_y=ODD), UNSUPPORTED, GN_CL),
     (dict(grad_x=ODD), UNSUPPORTED, GN_CL),
     (dict(y=ODD), UNSUPPORTED, GN_CL),
     (dict(grad_residual=ODD), UNSUPPORTED, GN_CL),
     (dict(n=0, y=None), INVALID, NULL),                                                # the ReLU's y before the sizes
     (dict(n=0, dtype=7), INVALID, 'bad sizes'),
     (dict(dtype=7, x=None), UNSUPPORTED, DTYPE),
     (dict(mean=None, workspace_bytes=0), INVALID, NULL),
     (dict(c=512, workspace_bytes=1024), WORKSPACE, GN_WS))
rows('dfm_group_norm_bwd_channels_last_xmask',
     (dict(groups=3), INVALID, 'bad sizes in dfm_group_norm_bwd_channels_last'),
     (dict(dtype=7), UNSUPPORTED, DTYPE),
     (dict(beta=None), INVALID, NULL),
     (dict(gamma=None), INVALID, NULL),
     (dict(workspace_bytes=1024), WORKSPACE, GN_WS),
     (dict(c=12, groups=4), UNSUPPORTED, GN_CL),
     (dict(c=24, groups=4, dtype=1), UNSUPPORTED, GN_CL),
     (dict(c=512), UNSUPPORTED, GN_CL),
     (dict(x=ODD), UNSUPPORTED, GN_CL),
     (dict(grad_x=ODD), UNSUPPORTED, GN_CL),
     (dict(n=0, beta=None), INVALID, NULL),                                             # the mask's beta before the sizes
     (dict(n=0, dtype=7), INVALID, 'bad sizes'),
     (dict(dtype=7, x=None), UNSUPPORTED, DTYPE),
     (dict(x=ODD, workspace_bytes=1024), WORKSPACE, GN_WS))
rows('dfm_batch_norm_stats_channels_last',
     (dict(c=0), INVALID, 'bad sizes in dfm_batch_norm_stats_channels_last'),
     (dict(rows=-1), INVALID, 'bad sizes in dfm_batch_norm_stats_channels_last'),
     (dict(dtype=7), UNSUPPORTED, DTYPE),
     (dict(x=None), INVALID, NULL),
     (dict(stats=None), INVALID, NULL),
     (dict(stats=None, rows=0, x=None), INVALID, NULL),
     (dict(workspace_bytes=1024), WORKSPACE, BN_WS),
     (dict(c=12), UNSUPPORTED, BN_CL),
     (dict(c=24, dtype=1), UNSUPPORTED, BN_CL),
     (dict(c=512), UNSUPPORTED, BN_CL),
     (dict(x=ODD), UNSUPPORTED, BN_CL),
     (dict(c=0, dtype=7), INVALID, 'bad sizes'),
     (dict(dtype=7, stats=None), UNSUPPORTED, DTYPE),
     (dict(workspace=None, workspace_bytes=0), INVALID, NULL),
     (dict(c=12, workspace_bytes=1024), WORKSPACE, BN_WS))
rows('dfm_batch_norm_apply_gathered_channels_last',
     (dict(c=0), INVALID, 'bad sizes in dfm_batch_norm_apply_gathered_channels_last'),
     (dict(world=0), INVALID, 'bad sizes in dfm_batch_norm_apply_gathered_channels_last'),
     (dict(dtype=7), UNSUPPORTED, DTYPE),
     (dict(y=None), INVALID, NULL),
     (dict(gathered=None), INVALID, NULL),
     (dict(moments=None, rows=0), INVALID, NULL),
     (dict(c=12), UNSUPPORTED, BN_CL),
     (dict(c=24, dtype=1), UNSUPPORTED, BN_CL),
     (dict(c=512), UNSUPPORTED, BN_CL),
     (dict(x=ODD), UNSUPPORTED, BN_CL),
     (dict(y=ODD), UNSUPPORTED, BN_CL),
     (dict(residual=ODD), UNSUPPORTED, BN_CL),
     (dict(rows=-1, dtype=7), INVALID, 'bad sizes'),
     (dict(dtype=7, gamma=None), UNSUPPORTED, DTYPE),
     (dict(mean=None, c=12), INVALID, NULL))                                            # pointers before the shape limits
rows('dfm_batch_norm_bwd_reduce_channels_last',
     (dict(c=0), INVALID, 'bad sizes in dfm_batch_norm_bwd_reduce_channels_last'),
     (dict(rows=-1), INVALID, 'bad sizes in dfm_batch_norm_bwd_reduce_channels_last'),
     (dict(dtype=7), UNSUPPORTED, DTYPE),
     (dict(grad_y=None), INVALID, NULL),
     (dict(y=None, beta=None), INVALID, NULL),                                          # relu = 1 needs y or beta
     (dict(sums=None), INVALID, NULL),
     (dict(workspace_bytes=1024), WORKSPACE, BN_WS),
     (dict(c=12), UNSUPPORTED, BN_CL),
     (dict(c=24, dtype=1), UNSUPPORTED, BN_CL),
     (dict(c=512), UNSUPPORTED, BN_CL),
     (dict(x=ODD), UNSUPPORTED, BN_CL),
     (dict(grad_y=ODD), UNSUPPORTED, BN_CL),
     (dict(y=ODD), UNSUPPORTED, BN_CL),
     (dict(c=0, dtype=7), INVALID, 'bad sizes'),
     (dict(dtype=7, sums=None), UNSUPPORTED, DTYPE),
     (dict(rstd=None, workspace_bytes=0), INVALID, NULL),
     (dict(x=ODD, workspace_bytes=1024), WORKSPACE, BN_WS))
rows('dfm_batch_norm_bwd_apply_channels_last',
     (dict(c=0), INVALID, 'bad sizes in dfm_batch_norm_bwd_apply_channels_last'),
     (dict(rows=-1), INVALID, 'bad sizes in dfm_batch_norm_bwd_apply_channels_last'),
     (dict(dtype=7), UNSUPPORTED, DTYPE),
     (dict(grad_x=None), INVALID, NULL),
     (dict(y=None, beta=None), INVALID, NULL),
     (dict(count=None), INVALID, NULL),
     (dict(workspace_bytes=1024), WORKSPACE, BN_WS),
     (dict(c=12), UNSUPPORTED, BN_CL),
     (dict(c=24, dtype=1), UNSUPPORTED, BN_CL),
     (dict(c=512), UNSUPPORTED, BN_CL),
     (dict(x=ODD), UNSUPPORTED, BN_CL),
     (dict(grad_y=ODD), UNSUPPORTED, BN_CL),
     (dict(grad_x=ODD), UNSUPPORTED, BN_CL),
     (dict(y=ODD), UNSUPPORTED, BN_CL),
     (dict(grad_residual=ODD), UNSUPPORTED, BN_CL),
     (dict(rows=-1, dtype=7), INVALID, 'bad sizes'),
     (dict(dtype=7, count=None), UNSUPPORTED, DTYPE),
     (dict(sums=None, workspace_bytes=0), INVALID, NULL),
     (dict(grad_x=ODD, workspace_bytes=1024), WORKSPACE, BN_WS))
rows('dfm_depth_head_fwd',
     (dict(batch=0), INVALID, 'non-positive size in dfm_depth_head_fwd'),
     (dict(scale=0), INVALID, 'non-positive size in dfm_depth_head_fwd'),
     (dict(dtype=7), UNSUPPORTED, DTYPE),
     (dict(cost=None), INVALID, NULL),
     (dict(depth_preds=None), INVALID, NULL),
     (dict(batch=65536), UNSUPPORTED, 'shape too large'),
     (dict(d=2001), UNSUPPORTED, 'shape too large'),
     (dict(h=32768, w=32768), UNSUPPORTED, 'shape too large'),
     (dict(d=0, dtype=7), INVALID, 'non-positive size'),
     (dict(dtype=7, softmax=None), UNSUPPORTED, DTYPE),
     (dict(depth_samples=None, batch=65536), INVALID, NULL))                            # pointers before the shape limits
rows('dfm_depth_head_stats_fwd',
     (dict(h=0), INVALID, 'non-positive size in dfm_depth_head_stats_fwd'),
     (dict(w=-4), INVALID, 'non-positive size in dfm_depth_head_stats_fwd'),
     (dict(dtype=7), UNSUPPORTED, DTYPE),
     (dict(cost=None), INVALID, NULL),
     (dict(col_sum=None), INVALID, NULL),
     (dict(batch=65536), UNSUPPORTED, 'shape too large'),
     (dict(d=2001), UNSUPPORTED, 'shape too large'),
     (dict(batch=0, dtype=7), INVALID, 'non-positive size'),
     (dict(dtype=7, col_max=None), UNSUPPORTED, DTYPE),
     (dict(col_max=None, d=2001), INVALID, NULL))
rows('dfm_cost_gate_fwd',
     (dict(batch=0), INVALID, 'non-positive size'),
     (dict(hw=0), INVALID, 'non-positive size'),
     (dict(stereo=None), INVALID, NULL),
     (dict(out=None), INVALID, NULL),
     (dict(dtype=7), UNSUPPORTED, DTYPE),
     (dict(num_depths=97), UNSUPPORTED, 'more than 96 depth planes'),
     (dict(packed_weights=ODD), INVALID, 'packed weights must be 16-byte aligned'),
     (dict(batch=65536), UNSUPPORTED, 'grid too large'),
     (dict(num_depths=0, mono=None), INVALID, 'non-positive size'),
     (dict(mono=None, dtype=7), INVALID, NULL),                                         # pointers before dtype HERE
     (dict(dtype=7, num_depths=97), UNSUPPORTED, DTYPE),
     (dict(num_depths=97, packed_weights=ODD), UNSUPPORTED, 'more than 96'))
for _name in ('dfm_cost_gate_pack_weights', 'dfm_cost_gate_mfma_pack_weights'):
    rows(_name,
         (dict(weight=None), INVALID, NULL),
         (dict(packed=None), INVALID, NULL),
         (dict(weight_dtype=7), UNSUPPORTED, 'weight dtype must be DFM_F32 or DFM_BF16'),
         (dict(num_depths=0), UNSUPPORTED, '1 .. 96 depth planes'),
         (dict(num_depths=97), UNSUPPORTED, '1 .. 96 depth planes'),
         (dict(packed=ODD), INVALID, 'packed weights must be 16-byte aligned'),
         (dict(weight=None, weight_dtype=7), INVALID, NULL),
         (dict(weight_dtype=7, num_depths=0), UNSUPPORTED, 'weight dtype must be'),
         (dict(num_depths=97, packed=ODD), UNSUPPORTED, '1 .. 96'))


def test_no_row_is_a_valid_call():
    assert len(ROWS) > 200 and {name for name, *_ in ROWS} == set(VALID)
    for name, bad, status, text in ROWS:
        assert status in (INVALID, UNSUPPORTED, WORKSPACE) and text, (name, bad)
        assert bad and set(bad) <= set(VALID[name]), (name, bad)
        assert any(VALID[name][k] != v for k, v in bad.items()), (name, bad)


@pytest.mark.parametrize('name', sorted(VALID))
def test_bad_calls_are_refused_with_their_status_and_message(capi, name):
    lib = capi.lib()
    fn = getattr(lib, name)
    for row_name, bad, status, text in ROWS:
        if row_name != name:
            continue
        args = dict(VALID[name], **bad)
        got = fn(*args.values())
        msg = lib.dfm_last_error().decode()
        assert (got, text in msg) == (status, True), (name, bad, got, msg)


def test_the_res_variants_report_the_name_without_res(capi):
    lib = capi.lib()
    for name in ('dfm_group_norm_fwd_channels_last_res', 'dfm_group_norm_apply_channels_last_res'):
        args = dict(VALID[name], n=0)
        assert getattr(lib, name)(*args.values()) == INVALID
        assert lib.dfm_last_error().decode() == 'bad sizes in ' + name[:-len('_res')]
    args = dict(VALID['dfm_group_norm_bwd_channels_last_xmask'], c=0)
    assert lib.dfm_group_norm_bwd_channels_last_xmask(*args.values()) == INVALID
    assert lib.dfm_last_error().decode() == 'bad sizes in dfm_group_norm_bwd_channels_last'


# ---- the multi-view lifting: a descriptor struct in front of the pointers ----------------------------------------------

def mv_desc(capi, **kw):
    d = dict(num_views=2, num_frames=1, channels=32, feat_h=4, feat_w=4, nx=0, ny=0, nz=0, num_points=64, scale_x=1.0,
             scale_y=1.0, crop_x=0.0, crop_y=0.0, flip=0, pad_h=1.0, pad_w=1.0, mode=0, aggregate=0, valid_sample=1,
             dtype=0, out_channels_last=0, feats_channels_last=1)
    d.update(kw)
    return capi.MvDesc(**d)


MV_ARGS = _sig('feats=P points=P proj=P ori_w=P out=P valid_out=P workspace=P workspace_bytes=BIG stream=0')
MV_ROWS = [   # (descriptor fields, arguments) that differ from a valid call, status, piece of the message
    (dict(num_views=0), {}, INVALID, 'non-positive size in dfm_mv_desc'),
    (dict(num_points=0), {}, INVALID, 'non-positive size in dfm_mv_desc'),
    (dict(dtype=7), {}, UNSUPPORTED, DTYPE),
    (dict(mode=2), {}, UNSUPPORTED, 'mode must be 0 or 1'),
    (dict(nx=4, ny=4, nz=5), {}, INVALID, 'nx*ny*nz != num_points'),
    ({}, dict(feats=None), INVALID, NULL),
    ({}, dict(out=None), INVALID, NULL),
    (dict(feats_channels_last=0), dict(workspace=None), WORKSPACE, 'dfm_point_sample_mv_workspace_bytes'),
    (dict(feats_channels_last=0), dict(workspace_bytes=1024), WORKSPACE, 'dfm_point_sample_mv_workspace_bytes'),
    (dict(valid_sample=0), {}, UNSUPPORTED, 'valid_sample=0 is only supported for a single view'),
    (dict(num_points=1 << 40), {}, UNSUPPORTED, 'too many points'),
    (dict(channels=30), {}, UNSUPPORTED, 'whole 16-byte channel blocks'),
    (dict(channels=36, dtype=1), {}, UNSUPPORTED, 'whole 16-byte channel blocks'),
    ({}, dict(feats=ODD), UNSUPPORTED, 'whole 16-byte channel blocks'),
    (dict(feat_h=0, dtype=7), {}, INVALID, 'non-positive size'),                        # sizes before dtype
    (dict(dtype=7, mode=2), dict(points=None), UNSUPPORTED, DTYPE),                     # dtype before mode and pointers
    (dict(mode=2, nx=4, ny=4, nz=5), {}, UNSUPPORTED, 'mode must be'),
    (dict(feats_channels_last=0), dict(proj=None, workspace=None), INVALID, NULL),      # pointers before workspace
    (dict(feats_channels_last=0, valid_sample=0), dict(workspace_bytes=0), WORKSPACE, 'workspace smaller'),
    (dict(valid_sample=0, channels=30), {}, UNSUPPORTED, 'valid_sample=0'),
]
MVB_ARGS = _sig('batch=2 feats=P points=P points_per_sample=1 proj=P ori_w=P out=P valid_out=P stream=0')
MVB_ROWS = [  # (fields of every descriptor, fields of the SECOND only, arguments), status, piece of the message
    ({}, {}, dict(batch=0), INVALID, 'no descriptors'),
    (dict(channels=0), {}, {}, INVALID, 'non-positive size in dfm_mv_desc'),
    ({}, {}, dict(ori_w=None), INVALID, NULL),
    (dict(nx=4, ny=4, nz=5, out_channels_last=1), {}, {}, INVALID, 'nx*ny*nz != num_points'),
    (dict(dtype=7), {}, {}, UNSUPPORTED, MV_BATCHED),
    (dict(mode=1), {}, {}, UNSUPPORTED, MV_BATCHED),
    (dict(valid_sample=0), {}, {}, UNSUPPORTED, MV_BATCHED),
    (dict(feats_channels_last=0), {}, {}, UNSUPPORTED, MV_BATCHED),
    (dict(nx=4, ny=4, nz=4), {}, {}, UNSUPPORTED, MV_BATCHED),                          # a volume must be channels-last
    (dict(channels=24), {}, {}, UNSUPPORTED, MV_BATCHED),                               # 6 channel blocks
    (dict(channels=30), {}, {}, UNSUPPORTED, MV_BATCHED),
    (dict(num_views=33), {}, {}, UNSUPPORTED, MV_BATCHED),                              # more than 4 x 8 blocks of pairs
    ({}, {}, dict(feats=ODD), UNSUPPORTED, MV_BATCHED),
    ({}, {}, dict(out=ODD), UNSUPPORTED, MV_BATCHED),
    ({}, dict(feat_h=5), {}, INVALID, 'the samples of a batch differ'),
    ({}, dict(dtype=1), {}, INVALID, 'the samples of a batch differ'),
    (dict(num_points=1 << 40), {}, {}, UNSUPPORTED, 'too many points'),
    (dict(num_frames=0), {}, dict(points=None), INVALID, 'non-positive size'),          # sizes before pointers
    (dict(dtype=7), {}, dict(feats=None), INVALID, NULL),                               # pointers before the coverage
    (dict(mode=1), dict(feat_w=5), {}, UNSUPPORTED, MV_BATCHED),                        # coverage before the batch check
]


def test_point_sample_mv_fwd_refuses_bad_calls(capi):
    lib = capi.lib()
    fn = lib.dfm_point_sample_mv_fwd
    assert fn(None, *MV_ARGS.values()) == INVALID and b'desc is NULL' in lib.dfm_last_error()
    for fields, bad, status, text in MV_ROWS:
        assert fields or bad
        got = fn(ctypes.byref(mv_desc(capi, **fields)), *dict(MV_ARGS, **bad).values())
        msg = lib.dfm_last_error().decode()
        assert (got, text in msg) == (status, True), (fields, bad, got, msg)


def test_point_sample_mv_fwd_batched_refuses_bad_calls(capi):
    lib = capi.lib()
    fn = lib.dfm_point_sample_mv_fwd_batched
    assert fn(None, *MVB_ARGS.values()) == INVALID and b'no descriptors' in lib.dfm_last_error()
    for fields, second, bad, status, text in MVB_ROWS:
        assert fields or second or bad
        descs = (capi.MvDesc * 2)(mv_desc(capi, **fields), mv_desc(capi, **dict(fields, **second)))
        got = fn(descs, *dict(MVB_ARGS, **bad).values())
        msg = lib.dfm_last_error().decode()
        assert (got, text in msg) == (status, True), (fields, second, bad, got, msg)
