"""Generate tests/golden/imitation.npz: the LiDAR-teacher feature-imitation loss, by running the REFERENCE's own
code on PyTorch-CPU (same rules as make_golden.py: the reference's functions are lifted from their files by AST
or executed by path, unmodified; only inputs and the outputs they produced are stored).

Run in the build container only (needs the reference checkout):   python tests/golden/make_golden_imitation.py

Executed unmodified: ``DfM.get_imitation_reg_layer_loss`` and ``DfM._init_imitation_layers`` (detectors/dfm.py),
``NormalizeLayer`` and ``WeightedL2WithSigmaLoss`` (detectors/imitation_utils.py, the whole file) and
``dist_reduce_mean`` (models/utils/common_utils.py), under a one-rank gloo group on a ``HashStore`` because
``NormalizeLayer.update`` calls ``all_reduce`` unconditionally.

STAND-IN: ``mmcv.ops.points_in_boxes_part`` is a CUDA op of a package that is not installed here.  The function
of that name below is a torch restatement of its box test as the maintainers state it (fp32: cz = z + z_size/2,
reject if |pz - cz| > z_size/2, a = -yaw, lx = dx cos a - dy sin a, ly = dx sin a + dy cos a, inside iff
|lx| < x_size/2 and |ly| < y_size/2, strict); it returns the index of the first containing box or -1, and it
broadcasts a points batch of 1 over the boxes' batch.  Every scene is asserted to keep every point at least
1e-3 m away from every box face in box-local coordinates, so neither ``<`` versus ``<=`` nor the last bits of
cos / sin can flip a cell.

Cases (features (B, C, [Nz,] Ny, Nx); pred / target stored as int8 sixteenths, exact in fp32 and bf16; targets
are zero in all channels at about half of the positions, as a sparse teacher's are):
  a_3d        C=32 B=2 Nz=5 40x36   cw_scale, training
  b_2d        C=64 B=2      40x36   cw_scale, training
  c_scale / c_center_scale / c_cw_center_scale / c_none   C=16 B=2 Nz=2 20x18, training
  d_nan       NaN targets (and the all-zero voxels inside boxes every case has), cw_scale, training
  e_miss      boxes that miss the grid: loss 0, zero gradient, buffers untouched
  f_few       between 1 and 10 positives: buffers untouched
  g_eval      eval mode: no update
Boxes include yaws beyond +-pi and a zero-size padding row.  Stored per case: the reference's loss,
d loss / d pred from its autograd, its ``positives`` and the layer's buffers after the call; and the reference
module's state-dict key list for a two-cfg and a one-cfg ``_init_imitation_layers``.

Two gradients per case, because a gradient has its leaf's dtype: ``grad`` is d loss / d pred of the call with
``pred`` in fp32, ``grad_bf16`` (stored as the bf16 bit patterns, int16) that of a second call of the same
unmodified function with the same values in a bf16 ``pred`` (exact: sixteenths) and a fresh copy of the layer.
That call's loss, positives and buffers are asserted equal to the first call's.

``mode='full'``: the generator tries the reference's branch and records whether it ran (``full_mode_runs``).
"""
import copy
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch
import torch.distributed as dist
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import make_golden as mg  # noqa: E402

MARGIN = 1e-3


def local_coords(points, boxes):
    """(B, N, T) box-local lx, ly and the z test of the stated semantics, fp32"""
    px, py, pz = (points[..., i][:, :, None] for i in range(3))
    x, y, z, xs, ys, zs, yaw = (boxes[..., i][:, None, :] for i in range(7))
    cz = z + zs / 2
    a = -yaw
    dx, dy = px - x, py - y
    lx = dx * torch.cos(a) - dy * torch.sin(a)
    ly = dx * torch.sin(a) + dy * torch.cos(a)
    return lx, ly, (pz - cz).abs() <= zs / 2, xs / 2, ys / 2


def points_in_boxes_part(points, boxes):
    """torch STAND-IN for mmcv.ops.points_in_boxes_part (see the module docstring)"""
    if points.shape[0] == 1 and boxes.shape[0] > 1:
        points = points.expand(boxes.shape[0], -1, -1)
    lx, ly, zok, hx, hy = local_coords(points.float(), boxes.float())
    inside = zok & (lx > -hx) & (lx < hx) & (ly > -hy) & (ly < hy)
    first = torch.argmax(inside.int(), dim=-1)
    return torch.where(inside.any(-1), first, torch.full_like(first, -1)).int()


def assert_margin(points, boxes):
    """no point within MARGIN of a box face (box-local), z forced to 0 on both sides as dfm.py:485-486 does"""
    p, b = points.clone(), boxes.clone()
    p[..., 2] = 0
    b[..., 2] = 0
    if p.shape[0] == 1:
        p = p.expand(b.shape[0], -1, -1)
    lx, ly, _, hx, hy = local_coords(p, b)
    d = torch.minimum((lx.abs() - hx).abs(), (ly.abs() - hy).abs())
    assert float(d.min()) > MARGIN, float(d.min())


def grid_points(ny, nx, step):
    ys = (torch.arange(ny, dtype=torch.float32) - ny / 2 + 0.5) * step
    xs = (torch.arange(nx, dtype=torch.float32) + 0.5) * step
    yy, xx = torch.meshgrid(ys, xs, indexing='ij')
    return torch.stack([xx, yy, torch.full_like(xx, -1.0)], dim=-1)   # z = -1: must be ignored


def seeded_boxes(rng, batch, count, ny, nx, step, points, kind='normal'):
    """(B, count + 1, 7): seeded boxes re-drawn until the margin holds, then one zero-size padding row"""
    for _ in range(1000):
        b = np.zeros((batch, count + 1, 7), np.float32)
        for i in range(batch):
            for t in range(count):
                if kind == 'miss':
                    cx, cy = -30.0 - 5 * t, 100.0 + 7 * i
                else:
                    cx, cy = rng.uniform(2 * step, (nx - 2) * step), rng.uniform(-(ny / 2 - 2) * step, (ny / 2 - 2) * step)
                size = (1.3 * step, 1.2 * step) if kind == 'few' else (rng.uniform(2, 5) * step, rng.uniform(1.5, 3) * step)
                b[i, t] = [cx, cy, rng.uniform(-2, 0), size[0], size[1], rng.uniform(1.4, 1.9), rng.uniform(-7.5, 7.5)]
        boxes = torch.from_numpy(b)
        try:
            assert_margin(points.view(1, -1, 3), boxes)
        except AssertionError:
            continue
        return boxes
    raise RuntimeError('no scene with the face margin')


def quantised(rng, shape, levels):
    return (rng.randint(-levels, levels + 1, size=shape) * 8).astype(np.int8)


def make_case(g, iu, rng, name, C, B, Nz, ny, nx, normalize, training=True, boxes_kind='normal', nboxes=3, nan=False,
              few=False):
    step = 1.0
    pts = grid_points(ny, nx, step)
    boxes = seeded_boxes(rng, B, 1 if few else nboxes, ny, nx, step, pts, 'few' if few else boxes_kind)
    if few:
        boxes[1:, :, 3:6] = 0     # one tiny box in sample 0 only
    shape = (B, C) + ((Nz,) if Nz else ()) + (ny, nx)
    pred_q = quantised(rng, shape, 1)
    target_q = quantised(rng, shape, 3)
    keep = rng.rand(*((B, 1) + shape[2:])) < 0.5
    target_q = (target_q * keep).astype(np.int8)
    pred = torch.from_numpy(pred_q.astype(np.float32) / 16.0).requires_grad_(True)
    target = torch.from_numpy(target_q.astype(np.float32) / 16.0)
    nan_mask = np.zeros(shape, bool)
    if nan:
        nan_mask = (rng.rand(*shape) < 0.02) & (np.arange(C).reshape((1, C) + (1,) * (len(shape) - 2)) % 5 == 1)
        target[torch.from_numpy(nan_mask)] = float('nan')
    layer = nn.Identity()
    out = {}
    if normalize is not None:
        layer = iu.NormalizeLayer(normalize, C)
        for k, buf in layer.named_buffers():
            buf.copy_(torch.from_numpy((rng.randint(8, 33, size=tuple(buf.shape)) / 16.0).astype(np.float32)))
            out[f'{k}0'] = buf.clone().numpy()
    layer.train(training)
    layer_bf16 = copy.deepcopy(layer)
    cfg = dict(mode='inbox', stereo_feature_layer='feat', loss_weight=1.5)
    anchors = torch.cat([pts, torch.zeros(ny, nx, 4)], dim=-1)[None, :, :, None, None, :].expand(B, -1, -1, -1, -1, -1)
    self_ = SimpleNamespace(bbox_head_3d=SimpleNamespace(anchors=[anchors]), normalizer_clamp_value=10,
                            norm_imitation={'feat': layer}, loss_imitation=iu.WeightedL2WithSigmaLoss())
    captured = {}
    g['points_in_boxes_part'] = lambda p, b: captured.setdefault('idx', points_in_boxes_part(p, b))
    loss, _ = g['get_imitation_reg_layer_loss'](self_, pred, target, cfg, [SimpleNamespace(tensor=b) for b in boxes])
    loss.backward()
    # the same call with pred as a bf16 leaf: the reference's gradient in that dtype
    pred_bf16 = pred.detach().to(torch.bfloat16).requires_grad_(True)
    assert torch.equal(pred_bf16.detach().float(), pred.detach())
    self_.norm_imitation = {'feat': layer_bf16}
    loss_bf16, _ = g['get_imitation_reg_layer_loss'](self_, pred_bf16, target, cfg,
                                                     [SimpleNamespace(tensor=b) for b in boxes])
    loss_bf16.backward()
    assert pred_bf16.grad.dtype == torch.bfloat16 and loss_bf16.dtype == torch.float32
    assert torch.equal(loss_bf16.detach(), loss.detach())
    for (_, a), (_, b) in zip(layer.named_buffers(), layer_bf16.named_buffers()):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))   # bits: d_nan's scale holds NaNs
    # the reference's `positives` (in-box and any_c(target != 0)), restated from the captured op result
    inbox = (captured['idx'] >= 0).view(B, ny, nx)
    tp = target.permute(0, *range(2, target.dim()), 1)
    positives = (inbox.unsqueeze(1).repeat(1, Nz, 1, 1) if Nz else inbox) & torch.any(tp != 0, dim=-1)
    n = int(positives.sum())
    if few:
        assert 1 <= n <= 10, n
    if boxes_kind == 'miss':
        assert n == 0
    out.update(pred_q=pred_q, target_q=target_q, points=pts.numpy(), boxes=boxes.numpy(),
               loss=np.float32(loss.item()), grad=pred.grad.numpy(),
               grad_bf16=pred_bf16.grad.view(torch.int16).numpy(), positives=np.packbits(positives.numpy()),
               training=np.bool_(training), normalize=np.str_(normalize or ''), loss_weight=np.float32(1.5))
    if nan:
        out['target_nan'] = np.packbits(nan_mask)
    for k, buf in layer.named_buffers():
        out[f'{k}1'] = buf.clone().numpy()
    print(name, shape, 'positives', n, 'of', positives.numel(), 'loss', float(loss))
    return {f'{name}/{k}': v for k, v in out.items()}


def main():
    dist.init_process_group('gloo', store=dist.HashStore(), rank=0, world_size=1)
    import ref_stubs
    iu = ref_stubs.load_file('mmdet3d/models/detectors/imitation_utils.py', 'ref_imitation_utils')
    g = {'torch': torch, 'dist': dist, 'nn': nn, 'NormalizeLayer': iu.NormalizeLayer}
    mg.extract(mg.REF + 'models/utils/common_utils.py', ['dist_reduce_mean'], g)
    mg.extract_method(mg.REF + 'models/detectors/dfm.py', 'DfM', 'get_imitation_reg_layer_loss', g)
    mg.extract_method(mg.REF + 'models/detectors/dfm.py', 'DfM', '_init_imitation_layers', g)
    rng = np.random.RandomState(2207)
    out = {}
    out.update(make_case(g, iu, rng, 'a_3d', 32, 2, 5, 40, 36, 'cw_scale', nboxes=6))
    out.update(make_case(g, iu, rng, 'b_2d', 64, 2, 0, 40, 36, 'cw_scale', nboxes=8))
    for nm, ty in (('c_scale', 'scale'), ('c_center_scale', 'center+scale'),
                   ('c_cw_center_scale', 'cw_center+scale'), ('c_none', None)):
        out.update(make_case(g, iu, rng, nm, 16, 2, 2, 20, 18, ty))
    out.update(make_case(g, iu, rng, 'd_nan', 32, 2, 2, 20, 18, 'cw_scale', nan=True))
    out.update(make_case(g, iu, rng, 'e_miss', 16, 2, 2, 20, 18, 'cw_scale', boxes_kind='miss'))
    out.update(make_case(g, iu, rng, 'f_few', 16, 2, 2, 20, 18, 'cw_center+scale', few=True))
    out.update(make_case(g, iu, rng, 'g_eval', 16, 2, 0, 20, 18, 'cw_scale', training=False))

    # mode='full' as written in the reference
    try:
        pts = grid_points(4, 4, 1.0)
        self_ = SimpleNamespace(normalizer_clamp_value=10, norm_imitation={'feat': nn.Identity()},
                                loss_imitation=iu.WeightedL2WithSigmaLoss())
        g['get_imitation_reg_layer_loss'](self_, torch.ones(1, 2, 4, 4), torch.ones(1, 2, 4, 4),
                                          dict(mode='full', stereo_feature_layer='feat', loss_weight=1.0), [])
        full_runs = True
    except (RuntimeError, TypeError) as e:
        print('mode=full does not run in the reference:', type(e).__name__, str(e)[:100])
        full_runs = False
    out['full_mode_runs'] = np.bool_(full_runs)

    # state-dict keys of the reference's layers (configs/dfm/dfm_r34_1x8_kitti-3d-3class.py: two cfgs)
    two = [dict(lidar_feature_layer='spatial_features_2d', stereo_feature_layer='spatial_features_2d',
                normalize='cw_scale', layer='conv2d', channel=64, kernel_size=1, use_relu=False, mode='inbox'),
           dict(lidar_feature_layer='volume_features', stereo_feature_layer='volume_features', normalize='cw_scale',
                layer='conv3d', channel=32, kernel_size=1, use_relu=False, mode='inbox')]
    one = [dict(lidar_feature_layer='volume_features', stereo_feature_layer='volume_features', normalize=None,
                layer='conv3d', channel=32, kernel_size=1, use_relu=True, mode='inbox')]
    for nm, cfgs in (('keys_two_cfgs', two), ('keys_one_cfg', one)):
        m = nn.Module()
        m.imitation_cfgs = cfgs
        g['_init_imitation_layers'](m)
        out[nm] = np.array(list(m.state_dict().keys()))
        print(nm, list(m.state_dict().keys()))
    path = os.path.join(HERE, 'imitation.npz')
    np.savez_compressed(path, **out)
    print(os.path.getsize(path), 'bytes')
    dist.destroy_process_group()


if __name__ == '__main__':
    if not os.path.isdir(mg.REF):
        sys.exit('reference not mounted; the fixture is committed, nothing to do')
    torch.set_num_threads(1)
    main()
