"""Generator of tests/golden/lidar_teacher.npz: the LiDAR teacher's fixture (hard voxelization, sparse encoder).

Run from the repository root with the reference checkout at /root/reference:

    python tests/golden/make_golden_lidar_teacher.py

Voxelization cases (``vox.<case>.*``): the reference's own ``points_to_voxel(..., reverse_index=True)``
(mmdet3d/core/voxel/voxel_generator.py, loaded by path with ``numba.jit`` stubbed to the identity) on seeded clouds.
A NaN coordinate passes both of the reference's range tests and then cannot index its grid, so the NaN case runs the
reference on the cloud WITHOUT the NaN points: "a NaN is dropped" is the contract
(include/dfm_hip_sparse_conv.h).  A batch case is the reference per sample, the batch index prepended.

Encoder cases (``enc.<case>.*``): the reference's sparse_encoder.py and sparse_block.py, loaded by path under stubs
where ``SparseConvTensor``, ``SubMConv3d``, ``SparseConv3d`` and ``SparseSequential`` are the DENSE MASKED stand-ins
written below: a dense ``conv3d`` of the scattered volume plus an activity mask propagated by a ones-kernel
convolution (SubM: the mask stays), BatchNorm1d and ReLU on the active sites only.  Layer structure, strides,
paddings, indice keys and state-dict keys are therefore the reference's.  The stand-in runs in fp64 and in fp32.

Stored per encoder case: the input rows and coordinates, the BatchNorm tensors (non-trivial running statistics), for
every stage the active set (sorted linear keys of the (b, z, y, x) grid) and the fp64 output on it (rows in key
order), the figure ``err`` = max |fp32 - fp64| / max |fp64| of every stage (floored at 2^-23, 0 for an all-zero
tensor).  Convolution weights are NOT stored (the whole encoder's exceed the size limit): ``weights(seed, shape)``
below regenerates them from the PCG64 raw bit stream, and the fixture keeps their SHA-256.

Nothing of the reference's program text goes into the fixture: it holds numbers and key names only.
"""
import hashlib
import importlib.util
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
REF_ROOT = '/root/reference'
OUT = os.path.join(HERE, 'lidar_teacher.npz')

# voxelization: 24 x 20 x 8 cells (x, y, z) of the teacher's voxel size
VOX_SIZE = [0.05, 0.05, 0.1]
VOX_RANGE = [0.0, -0.5, -0.4, 1.2, 0.5, 0.4]
MAX_POINTS = 5

ENCODER_CFG = dict(in_channels=3, output_channels=32,
                   encoder_strides=((1, ), (2, 1, 1), (2, 1, 1), ((2, 1, 1), 1, 1)), order=('conv', 'norm', 'act'),
                   norm_cfg=dict(type='SyncBN', eps=1e-3, momentum=0.01), with_final_bnrelu=False,
                   output_volume_feat=True)   # the KITTI configs' middle_encoder, sparse_shape per case

# single layers: name -> (conv_type, cin, cout, kernel, stride, padding, sparse_shape, norm + relu, voxels)
LAYERS = {
    'subm_3_16': ('SubMConv3d', 3, 16, 3, 1, 1, [9, 24, 20], True, 257),
    'subm_16_16': ('SubMConv3d', 16, 16, 3, 1, 1, [11, 25, 19], True, 200),
    'subm_32_32': ('SubMConv3d', 32, 32, 3, 1, 1, [9, 24, 20], True, 200),
    'subm_64_64': ('SubMConv3d', 64, 64, 3, 1, 1, [11, 25, 19], True, 200),
    'sp_s2_p1': ('SparseConv3d', 16, 32, 3, 2, 1, [11, 25, 19], True, 200),
    'sp_s211_p011': ('SparseConv3d', 16, 16, 3, (2, 1, 1), (0, 1, 1), [11, 25, 19], True, 40),
    'sp_1x1': ('SparseConv3d', 64, 32, 1, 1, 0, [9, 24, 20], False, 200),
}
ENCODERS = {'enc_9_24_20': ([9, 24, 20], 220), 'enc_11_25_19': ([11, 25, 19], 200)}
# the end-to-end case: a cloud over 16 x 32 x 8 cells (x, y, z), sparse_shape [9, 32, 16] -> volume (B, 32, 1, 8, 4)
PATH_RANGE = [0.0, -0.8, -0.4, 0.8, 0.8, 0.4]
PATH_SHAPE = [9, 32, 16]


def weights(seed, shape, bound=None):
    """fp32 values in [-bound, bound) from the raw PCG64 stream (stable by numpy's bit-generator guarantee): the top
    24 bits of each raw word, centred.  ``bound`` defaults to sqrt(3 / fan_in) with fan_in = all axes but the last."""
    n = int(np.prod(shape))
    fan_in = max(n // shape[-1], 1)
    bound = (3.0 / fan_in) ** 0.5 if bound is None else bound
    raw = np.random.PCG64(seed).random_raw(n) >> np.uint64(40)
    return ((raw.astype(np.float64) - 2.0 ** 23) / 2.0 ** 23 * bound).astype(np.float32).reshape(shape)


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype='<f4').tobytes()).hexdigest()


# ----------------------------------------------------------------------------------------------------------------
# the dense masked stand-ins
# ----------------------------------------------------------------------------------------------------------------
def _triple(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v, v)


class SparseConvTensor:
    """dense volume (B, C, D, H, W) plus activity mask (B, 1, D, H, W); ``features`` are the active sites' values in
    ascending (b, z, y, x) order"""

    def __init__(self, features, indices, spatial_shape, batch_size, grid=None):
        self.spatial_shape, self.batch_size = list(spatial_shape), batch_size
        idx = indices.long()
        self.vol = features.new_zeros((batch_size, features.shape[1], *spatial_shape))
        self.mask = torch.zeros((batch_size, 1, *spatial_shape), dtype=torch.bool)
        self.vol[idx[:, 0], :, idx[:, 1], idx[:, 2], idx[:, 3]] = features
        self.mask[idx[:, 0], 0, idx[:, 1], idx[:, 2], idx[:, 3]] = True
        assert int(self.mask.sum()) == idx.shape[0], 'duplicate coordinates'

    @classmethod
    def from_dense(cls, vol, mask):
        t = cls.__new__(cls)
        t.vol, t.mask = vol * mask, mask
        t.spatial_shape, t.batch_size = list(vol.shape[2:]), vol.shape[0]
        return t

    @property
    def indices(self):
        return self.mask[:, 0].nonzero().int()          # ascending (b, z, y, x)

    @property
    def features(self):
        i = self.indices.long()
        return self.vol[i[:, 0], :, i[:, 1], i[:, 2], i[:, 3]]

    @features.setter
    def features(self, value):
        i = self.indices.long()
        vol = value.new_zeros((self.batch_size, value.shape[1], *self.spatial_shape))
        vol[i[:, 0], :, i[:, 1], i[:, 2], i[:, 3]] = value
        self.vol = vol

    def dense(self):
        return self.vol


class SparseModule(nn.Module):
    pass


class _Conv(SparseModule):
    subm = False

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, bias=True, indice_key=None):
        super().__init__()
        assert not bias
        self.kernel_size, self.stride, self.padding = _triple(kernel_size), _triple(stride), _triple(padding)
        self.indice_key = indice_key
        self.weight = nn.Parameter(torch.zeros(*self.kernel_size, in_channels, out_channels))   # mmcv 1.x's layout

    def forward(self, x):
        w = self.weight.permute(4, 3, 0, 1, 2)
        if self.subm:   # the padding argument is ignored: k // 2, the row set stays
            return SparseConvTensor.from_dense(F.conv3d(x.vol, w, padding=tuple(k // 2 for k in self.kernel_size)), x.mask)
        out = F.conv3d(x.vol, w, stride=self.stride, padding=self.padding)
        ones = torch.ones((1, 1, *self.kernel_size), dtype=x.vol.dtype)
        mask = F.conv3d(x.mask.to(x.vol.dtype), ones, stride=self.stride, padding=self.padding) > 0.5
        return SparseConvTensor.from_dense(out, mask)


class SubMConv3d(_Conv):
    subm = True


class SparseConv3d(_Conv):
    pass


class SparseSequential(SparseModule):
    """sparse modules run on the tensor, plain modules on the active sites' features"""

    def __init__(self, *args):
        super().__init__()
        for i, m in enumerate(args):
            self.add_module(str(i), m)

    def __iter__(self):
        return iter(self._modules.values())

    def forward(self, x):
        for m in self._modules.values():
            if isinstance(m, SparseModule):
                x = m(x)
            else:
                x.features = m(x.features)
        return x


def _build_conv_layer(cfg, *args, **kwargs):
    cfg = dict(cfg)
    return {'SubMConv3d': SubMConv3d, 'SparseConv3d': SparseConv3d}[cfg.pop('type')](*args, **kwargs, **cfg)


def _build_norm_layer(cfg, num_features):
    cfg = dict(cfg)
    assert cfg.pop('type') in ('BN1d', 'SyncBN')
    return 'bn', nn.BatchNorm1d(num_features, **cfg)


def load_reference():
    """the reference's sparse_block.py, sparse_encoder.py and voxel_generator.py executed under the stubs;
    sys.modules is restored afterwards -> (make_sparse_convmodule, CustomSparseEncoder, points_to_voxel)"""
    before = dict(sys.modules)

    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        m.__path__ = []
        sys.modules[name] = m
        return m

    def load(rel, name):
        spec = importlib.util.spec_from_file_location(name, os.path.join(REF_ROOT, rel))
        m = importlib.util.module_from_spec(spec)
        sys.modules[name] = m
        spec.loader.exec_module(m)
        return m

    class Registry:
        def register_module(self, *a, **k):
            return lambda cls: cls

    try:
        ident = lambda *a, **k: (lambda f: f)   # noqa: E731
        mod('numba', jit=ident)
        mod('mmcv')
        mod('mmcv.cnn', build_conv_layer=_build_conv_layer, build_norm_layer=_build_norm_layer)
        mod('mmcv.runner', auto_fp16=ident)
        mod('mmcv.ops', SparseConvTensor=SparseConvTensor, SparseSequential=SparseSequential,
            SparseModule=SparseModule, points_in_boxes_all=None, three_interpolate=None, three_nn=None)
        mod('mmdet')
        mod('mmdet.models')
        mod('mmdet.models.losses', sigmoid_focal_loss=None, smooth_l1_loss=None)
        mod('mmdet.models.backbones')
        mod('mmdet.models.backbones.resnet', BasicBlock=type('BasicBlock', (nn.Module, ), {}),
            Bottleneck=type('Bottleneck', (nn.Module, ), {}))
        mod('mmdet3d')
        mod('mmdet3d.models')
        mod('mmdet3d.models.builder', MIDDLE_ENCODERS=Registry())
        mod('mmdet3d.models.middle_encoders')
        ops = mod('mmdet3d.ops')
        mod('mmdet3d.ops.spconv', IS_SPCONV2_AVAILABLE=False)
        block = load('mmdet3d/ops/sparse_block.py', 'mmdet3d.ops.sparse_block')
        ops.SparseBasicBlock, ops.make_sparse_convmodule = block.SparseBasicBlock, block.make_sparse_convmodule
        enc = load('mmdet3d/models/middle_encoders/sparse_encoder.py', 'mmdet3d.models.middle_encoders.sparse_encoder')
        vox = load('mmdet3d/core/voxel/voxel_generator.py', 'ref_voxel_generator')
        return block.make_sparse_convmodule, enc.CustomSparseEncoder, vox.points_to_voxel
    finally:
        for k in list(sys.modules):
            if k not in before:
                del sys.modules[k]
        sys.modules.update({k: v for k, v in before.items() if k not in sys.modules})


# ----------------------------------------------------------------------------------------------------------------
# inputs
# ----------------------------------------------------------------------------------------------------------------
def clustered_coors(rng, shape, batch, count, empty=()):
    """``count`` unique (b, z, y, x) in a few blobs, so that most voxels have neighbours; the first and last cells of
    every axis are included (borders), and samples in ``empty`` get none"""
    d, h, w = shape
    live = [b for b in range(batch) if b not in empty]
    cells = set()
    for b in live:   # corners: a voxel in the last plane / row / column of a sample and one in the first of the next
        cells.add((b, 0, 0, 0))
        cells.add((b, d - 1, h - 1, w - 1))
    centres = [(live[i % len(live)], rng.integers(0, d), rng.integers(0, h), rng.integers(0, w)) for i in range(6)]
    while len(cells) < count:
        b, z, y, x = centres[rng.integers(0, len(centres))]
        z, y, x = (int(np.clip(round(c + rng.normal(0, s)), 0, n - 1)) for c, s, n in ((z, 1.5, d), (y, 3, h), (x, 3, w)))
        cells.add((b, z, y, x))
    coors = np.asarray(sorted(cells), dtype=np.int32)
    return coors[rng.permutation(len(coors))]


def norm_tensors(rng, channels):
    return dict(weight=rng.uniform(0.5, 1.5, channels).astype(np.float32),
                bias=rng.uniform(-0.3, 0.3, channels).astype(np.float32),
                running_mean=rng.uniform(-0.2, 0.2, channels).astype(np.float32),
                running_var=rng.uniform(0.3, 2.0, channels).astype(np.float32))


def set_state(model, seed, rng, store, prefix):
    """conv weights from ``weights(seed + i, shape)``, BatchNorm tensors from ``rng`` (stored); the state-dict key
    list, shapes and the weights' digests go into the fixture"""
    sd = model.state_dict()
    keys, i = list(sd), 0
    for k in keys:
        if k.endswith('num_batches_tracked'):
            continue
        if sd[k].dim() == 5:
            sd[k] = torch.from_numpy(weights(seed + i, tuple(sd[k].shape)))
            store[f'{prefix}.sha.{k}'] = digest(sd[k].numpy())
            i += 1
    for k in keys:
        if k.endswith('running_mean'):
            base = k[:-len('running_mean')]
            for name, v in norm_tensors(rng, sd[k].shape[0]).items():
                sd[base + name] = torch.from_numpy(v)
                store[f'{prefix}.bn.{base}{name}'] = v
    model.load_state_dict(sd, strict=True)
    store[f'{prefix}.keys'] = np.asarray(keys)
    store[f'{prefix}.shapes'] = np.asarray([','.join(str(s) for s in sd[k].shape) for k in keys])
    store[f'{prefix}.seed'] = np.int64(seed)
    model.eval()


def linear_keys(idx, shape):
    idx = idx.long()
    return ((idx[:, 0] * shape[0] + idx[:, 1]) * shape[1] + idx[:, 2]) * shape[2] + idx[:, 3]


def figure(a32, a64):
    scale = a64.abs().max().item() if a64.numel() else 0.0
    if scale == 0:
        return 0.0
    return max((a32.double() - a64).abs().max().item() / scale, 2.0 ** -23)


def store_stage(store, name, t32, t64):
    """active set as sorted linear keys, fp64 rows in key order, the fp32-vs-fp64 figure"""
    i32, i64 = t32.indices, t64.indices
    assert torch.equal(i32, i64)
    store[f'{name}.shape'] = np.asarray(t64.spatial_shape, dtype=np.int32)
    store[f'{name}.keys'] = linear_keys(i64, t64.spatial_shape).numpy()
    store[f'{name}.out'] = t64.features.numpy()
    store[f'{name}.err'] = np.float64(figure(t32.features, t64.features))
    assert not (t64.vol * ~t64.mask).any()


def run_stages(model, feats, coors, shape, batch):
    x = SparseConvTensor(feats, torch.from_numpy(coors), shape, batch)
    stages = [model.conv_input(x)]
    for layer in model.encoder_layers:
        stages.append(layer(stages[-1]))
    stages.append(model.conv_out(stages[-1]))
    return stages


# ----------------------------------------------------------------------------------------------------------------
# cases
# ----------------------------------------------------------------------------------------------------------------
def vox_clouds(rng):
    lo, hi, vs = np.float32(VOX_RANGE[:3]), np.float32(VOX_RANGE[3:]), np.float32(VOX_SIZE)

    def cloud(n, ndim, spread=1.0):
        p = rng.uniform(-0.1, 1.1, (n, ndim)).astype(np.float32)
        p[:, :3] = lo + (hi - lo) * (0.5 + (p[:, :3] - 0.5) * spread)
        return p

    cases = {}
    p = cloud(1000, 4)
    faces = np.stack([lo + vs * rng.integers(0, [25, 21, 9]) for _ in range(300)]).astype(np.float32)
    p[:300, :3] = faces                                     # exactly on cell faces, the upper faces included
    p[300:310, 0], p[310:320, 1], p[320:330, 2] = hi[0], hi[1], hi[2]
    p[330:340, 0], p[340:350, 1], p[350:360, 2] = lo[0], lo[1], lo[2]
    p[360:365, 0], p[365:370, 1], p[370:375, 2] = hi[0] + 0.3, lo[1] - 0.3, hi[2] + 7.0   # outside, one axis each
    p[375:380, 0], p[380:385, 1], p[385:390, 2] = -np.inf, np.inf, -1e30
    cases['faces'] = (p, 400)
    p = cloud(800, 4)
    p[rng.choice(800, 40, replace=False), rng.integers(0, 3, 40)] = np.nan
    p[7, 3] = np.nan                                        # a NaN feature is no reason to drop a point
    cases['nan'] = (p, 400)
    p = cloud(2000, 4, spread=0.25)                         # few cells, many points each: more than five per voxel
    cases['crowded'] = (p, 400)
    cases['cut'] = (cloud(1000, 4), 37)                     # far more cells than max_voxels
    cases['empty'] = (np.zeros((0, 4), np.float32), 400)
    p = cloud(200, 4)
    p[:, 0] += 5.0
    cases['outside'] = (p, 400)
    cases['ndim5'] = (cloud(500, 5), 400)
    cases['ndim3'] = (cloud(300, 3), 400)
    return cases


def main():
    make_block, Encoder, points_to_voxel = load_reference()
    store = {}
    rng = np.random.default_rng(20241)

    def voxelize(p, max_voxels, rng_range=VOX_RANGE):
        keep = ~np.isnan(p[:, :3]).any(axis=1)              # see the module docstring
        v, c, n = points_to_voxel(p[keep], VOX_SIZE, rng_range, MAX_POINTS, True, max_voxels)
        return v.astype(np.float32), c.astype(np.int32), n.astype(np.int32)

    with np.errstate(all='ignore'):
        for name, (p, max_voxels) in vox_clouds(rng).items():
            v, c, n = voxelize(p, max_voxels)
            store[f'vox.{name}.points'], store[f'vox.{name}.max_voxels'] = p, np.int32(max_voxels)
            store[f'vox.{name}.voxels'], store[f'vox.{name}.coors'], store[f'vox.{name}.num_points'] = v, c, n
            print(f'vox {name:8s} points {len(p):5d} -> voxels {len(v):4d}, fullest {n.max() if len(n) else 0}')
        # a batch of three clouds, the middle one empty, max_voxels small enough to cut the first
        clouds = [store['vox.faces.points'], np.zeros((0, 4), np.float32), store['vox.crowded.points'][:900]]
        rows = []
        for b, p in enumerate(clouds):
            v, c, n = voxelize(p, 150)
            rows.append((v, np.concatenate([np.full((len(c), 1), b, np.int32), c], axis=1), n))
            store[f'vox.batch.points{b}'] = p
        store['vox.batch.max_voxels'] = np.int32(150)
        store['vox.batch.voxels'] = np.concatenate([r[0] for r in rows])
        store['vox.batch.coors'] = np.concatenate([r[1] for r in rows])
        store['vox.batch.num_points'] = np.concatenate([r[2] for r in rows])

    # single layers, through the reference's make_sparse_convmodule
    for li, (name, (kind, cin, cout, k, s, p, shape, full, count)) in enumerate(LAYERS.items()):
        order = ('conv', 'norm', 'act') if full else ('conv', )
        coors = clustered_coors(rng, shape, 2, count)
        feats = rng.normal(0, 1, (len(coors), cin)).astype(np.float32)
        outs = {}
        for dtype in (torch.float64, torch.float32):
            m = make_block(cin, cout, k, indice_key='k', stride=s, padding=p, conv_type=kind,
                           norm_cfg=dict(type='BN1d', eps=1e-3, momentum=0.01), order=order)
            set_state(m, 1000 + 10 * li, np.random.default_rng(500 + li), store, f'layer.{name}')
            m = m.to(dtype)
            with torch.no_grad():
                outs[dtype] = m(SparseConvTensor(torch.from_numpy(feats).to(dtype), torch.from_numpy(coors), shape, 2))
        store[f'layer.{name}.features'], store[f'layer.{name}.coors'] = feats, coors
        store_stage(store, f'layer.{name}.stage', outs[torch.float32], outs[torch.float64])
        print(f'layer {name:13s} rows {len(coors)} -> {len(store[f"layer.{name}.stage.keys"])} err {store[f"layer.{name}.stage.err"]:.2e}')

    # the whole encoder
    for ei, (name, (shape, count)) in enumerate(ENCODERS.items()):
        coors = clustered_coors(rng, shape, 3 if ei else 2, count, empty=(1, ) if ei else ())
        batch = 3 if ei else 2                              # the second case has an empty sample in the middle
        feats = rng.uniform(-1, 1, (len(coors), 3)).astype(np.float32)
        outs = {}
        for dtype in (torch.float64, torch.float32):
            m = Encoder(sparse_shape=shape, **ENCODER_CFG)
            set_state(m, 2000 + 100 * ei, np.random.default_rng(700 + ei), store, f'enc.{name}')
            m = m.to(dtype)
            with torch.no_grad():
                outs[dtype] = run_stages(m, torch.from_numpy(feats).to(dtype), coors, shape, batch)
        store[f'enc.{name}.features'], store[f'enc.{name}.coors'] = feats, coors
        store[f'enc.{name}.batch'], store[f'enc.{name}.sparse_shape'] = np.int32(batch), np.asarray(shape, np.int32)
        for si, (t32, t64) in enumerate(zip(outs[torch.float32], outs[torch.float64])):
            store_stage(store, f'enc.{name}.stage{si}', t32, t64)
            print(f'enc {name} stage {si}: grid {t64.spatial_shape} rows {len(t64.indices)} '
                  f'err {store[f"enc.{name}.stage{si}.err"]:.2e}')

    # end to end: clouds -> reference voxelization -> mean of the points -> the encoder's volume
    clouds = []
    lo, hi = np.float32(PATH_RANGE[:3]), np.float32(PATH_RANGE[3:])
    for b in range(2):
        c = lo + (hi - lo) * rng.uniform(0.2, 0.8, (5, 3)).astype(np.float32)
        p = (c[rng.integers(0, 5, 700)] + rng.normal(0, 0.06, (700, 3))).astype(np.float32)
        clouds.append(np.concatenate([p, rng.uniform(0, 1, (700, 1)).astype(np.float32)], axis=1))
    feats, coors = [], []
    for b, p in enumerate(clouds):
        v, c, n = voxelize(p, 400, PATH_RANGE)
        feats.append(v[:, :, :3].sum(axis=1) / n.astype(np.float32).reshape(-1, 1))
        coors.append(np.concatenate([np.full((len(c), 1), b, np.int32), c], axis=1))
        store[f'path.points{b}'] = p
    feats, coors = np.concatenate(feats).astype(np.float32), np.concatenate(coors)
    outs = {}
    for dtype in (torch.float64, torch.float32):
        m = Encoder(sparse_shape=PATH_SHAPE, **ENCODER_CFG)
        set_state(m, 3000, np.random.default_rng(900), store, 'path')
        m = m.to(dtype)
        with torch.no_grad():
            outs[dtype] = run_stages(m, torch.from_numpy(feats).to(dtype), coors, PATH_SHAPE, 2)[-1]
    store['path.voxel_features'], store['path.coors'] = feats, coors
    store_stage(store, 'path.volume', outs[torch.float32], outs[torch.float64])
    print(f'path: {len(coors)} voxels -> volume grid {outs[torch.float64].spatial_shape} rows {len(store["path.volume.keys"])} '
          f'err {store["path.volume.err"]:.2e}')

    np.savez_compressed(OUT, **store)
    print(OUT, os.path.getsize(OUT), 'bytes')
    assert os.path.getsize(OUT) <= 1 << 20


if __name__ == '__main__':
    main()
