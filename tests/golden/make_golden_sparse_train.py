"""Generator of tests/golden/sparse_train*.npz: one TRAINING step of the LiDAR teacher's sparse layers and encoder.

Run from the repository root with the reference checkout where make_golden_lidar_teacher.py looks for it (REF_ROOT):

    python tests/golden/make_golden_sparse_train.py

The dense masked stand-ins, ``load_reference()``, ``weights()``, ``clustered_coors()`` and ``set_state()`` are those of
tests/golden/make_golden_lidar_teacher.py, imported by path (that file is not modified).  The reference's
``make_sparse_convmodule`` (the seven layers of ``LAYERS``) and ``CustomSparseEncoder`` (the two ``ENCODERS``) run in
TRAINING mode under torch autograd, in fp64 and in fp32; the loss is ``(dense output x seeded weights).sum()`` with the
loss weights ``weights(loss_seed, volume shape, bound=1)``.

Stored per case (``<kind>.<case>.*``, kind = layer | enc): the input rows and coordinates, the state-dict keys /
shapes / weight digests and the BatchNorm tensors BEFORE the step (``set_state``'s keys), and in fp64, each with its own
fp32-vs-fp64 figure max |fp32 - fp64| / max |fp64| floored at 2^-23 (``<key>`` and ``<key>.err``):

    stage.*                 the forward output in training mode (active set, rows in key order), as ``store_stage``
    grad_in                 gradient of the input rows, rows in ascending key order
    grad_stage0             (encoders) gradient of the rows after ``conv_input``, in key order
    grad.<param>            gradient of every BatchNorm weight and bias
    dw.<param>              gradient of a convolution weight of at most 2^15 elements, in full
    proj.<param>            64 projections <dW, P_j>, P_j = weights(PROJ_SEED + j, shape, bound=1), of a larger one
    after.<buffer>          running_mean / running_var after the step (num_batches_tracked is 1)
    pre_ratio, seed         the mask-margin condition below and the seed that met it

Seed condition.  A ReLU mask that flips between fp32 and fp64 would make the comparison meaningless, so seeds are tried
in ascending order until, for every BatchNorm output, min |pre-ReLU value| / max |pre-ReLU value| over the live rows
exceeds MARGIN x that tensor's own forward fp32-vs-fp64 figure and the fp32 and fp64 masks are equal; ``pre_ratio`` is
the smallest (ratio / (MARGIN x figure)) over the case's BatchNorms (> 1).

Files.  The full fp64 dW of an encoder case alone is 0.6 MiB, so the ``dw.*`` and ``grad_in`` arrays go to side files
(``sparse_train.layers.npz`` for the seven layers, ``sparse_train.<case>.npz`` per encoder case) and everything else,
every figure included, to ``sparse_train.npz``: each file stays under 1 MiB.  The fixture
holds numbers and key names only.
"""
import importlib.util
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, 'sparse_train.npz')
MARGIN = 4            # tests/lidar_teacher_ref.py
FULL_DW = 1 << 15     # elements
PROJECTIONS = 64
PROJ_SEED = 7000
LOSS_SEED = 8000
MAX_SEEDS = 200


def _teacher_generator():
    spec = importlib.util.spec_from_file_location('make_golden_lidar_teacher',
                                                  os.path.join(HERE, 'make_golden_lidar_teacher.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


gen = _teacher_generator()


def case_file(case):
    return os.path.join(HERE, f'sparse_train.{case}.npz')


def projections(dw):
    """(PROJECTIONS,) fp64: <dW, P_j>"""
    shape = tuple(dw.shape)
    return torch.stack([(dw.double() * torch.from_numpy(gen.weights(PROJ_SEED + j, shape, bound=1)).double()).sum()
                        for j in range(PROJECTIONS)])


def key_order(coors, shape):
    return torch.argsort(gen.linear_keys(torch.from_numpy(coors), shape))


def run_step(model, dtype, feats, coors, shape, batch, loss_seed, encoder):
    """one forward + backward in training mode -> dict of what the fixture compares"""
    model = model.to(dtype).train()
    pre = {}
    hooks = [m.register_forward_hook(lambda mod, inp, out, n=n: pre.__setitem__(n, out.detach().clone()))
             for n, m in model.named_modules() if isinstance(m, torch.nn.BatchNorm1d)]
    x = torch.from_numpy(feats).to(dtype).requires_grad_()
    if encoder:
        stages = gen.run_stages(model, x, coors, shape, batch)
        stages[0].vol.retain_grad()
        out = stages[-1]
    else:
        stages = None
        out = model(gen.SparseConvTensor(x, torch.from_numpy(coors), shape, batch))
    volume = out.dense()
    wl = torch.from_numpy(gen.weights(loss_seed, tuple(volume.shape), bound=1)).to(dtype)
    (volume * wl).sum().backward()
    for h in hooks:
        h.remove()
    out = gen.SparseConvTensor.from_dense(out.vol.detach(), out.mask)
    res = dict(out=out, pre=pre, grad_in=x.grad.detach(),
               grads={n: p.grad.detach() for n, p in model.named_parameters()},
               after={n: b.detach().clone() for n, b in model.named_buffers()})
    if encoder:
        i = stages[0].indices.long()
        res['grad_stage0'] = stages[0].vol.grad[i[:, 0], :, i[:, 1], i[:, 2], i[:, 3]].detach()
    return res


def margin_ratio(r32, r64):
    """the smallest min|pre| / max|pre| / (MARGIN x figure) over the BatchNorm outputs; 0 when a mask differs"""
    worst = float('inf')
    for name, p64 in r64['pre'].items():
        p32 = r32['pre'][name]
        if not torch.equal(p32 > 0, p64 > 0):
            return 0.0
        fig = gen.figure(p32, p64)
        ratio = (p64.abs().min() / p64.abs().max()).item()
        worst = min(worst, ratio / (MARGIN * fig))
    return worst


def store_step(store, big, prefix, r32, r64, coors, shape):
    gen.store_stage(store, f'{prefix}.stage', r32['out'], r64['out'])
    order = key_order(coors, shape)

    def put(key, a32, a64, target=store):
        target[f'{prefix}.{key}'] = a64.double().numpy()
        store[f'{prefix}.{key}.err'] = np.float64(gen.figure(a32, a64.double()))

    put('grad_in', r32['grad_in'][order], r64['grad_in'][order], big)
    if 'grad_stage0' in r64:
        put('grad_stage0', r32['grad_stage0'], r64['grad_stage0'])
    for name, g64 in r64['grads'].items():
        g32 = r32['grads'][name]
        if g64.dim() == 1:
            put(f'grad.{name}', g32, g64)
        elif g64.numel() <= FULL_DW:
            put(f'dw.{name}', g32, g64, big)
        else:
            put(f'proj.{name}', projections(g32), projections(g64))
    for name, b64 in r64['after'].items():
        if name.endswith('num_batches_tracked'):
            assert int(b64) == 1
        else:
            put(f'after.{name}', r32['after'][name], b64)


def find_seed(build, inputs, base_seed, loss_seed, shape, batch, encoder, prefix):
    """the first seed (ascending) that meets the mask-margin condition -> (seed, ratio, store of set_state, results)"""
    for seed in range(MAX_SEEDS):
        rng = np.random.default_rng(base_seed + seed)
        feats, coors = inputs(rng)
        res, state = {}, {}
        for dtype in (torch.float64, torch.float32):
            m = build()
            state = {}
            gen.set_state(m, base_seed * 10 + 100 * seed, np.random.default_rng(base_seed + 5000 + seed), state, prefix)
            res[dtype] = run_step(m, dtype, feats, coors, shape, batch, loss_seed, encoder)
        ratio = margin_ratio(res[torch.float32], res[torch.float64])
        if ratio > 1.0:
            return seed, ratio, state, feats, coors, res
    raise RuntimeError(f'{prefix}: no seed below {MAX_SEEDS} meets the mask-margin condition')


def main():
    make_block, Encoder, _ = gen.load_reference()
    store, layers = {}, {}
    for li, (name, (kind, cin, cout, k, s, p, shape, full, count)) in enumerate(gen.LAYERS.items()):
        order = ('conv', 'norm', 'act') if full else ('conv', )
        prefix = f'layer.{name}'

        def build():
            return make_block(cin, cout, k, indice_key='k', stride=s, padding=p, conv_type=kind,
                              norm_cfg=dict(type='BN1d', eps=1e-3, momentum=0.01), order=order)

        def inputs(rng):
            coors = gen.clustered_coors(rng, shape, 2, count)
            return rng.normal(0, 1, (len(coors), cin)).astype(np.float32), coors

        seed, ratio, state, feats, coors, res = find_seed(build, inputs, 100 + 10 * li, LOSS_SEED + li, shape, 2,
                                                          False, prefix)
        store.update(state)
        store[f'{prefix}.features'], store[f'{prefix}.coors'] = feats, coors
        store[f'{prefix}.case_seed'], store[f'{prefix}.pre_ratio'] = np.int64(seed), np.float64(ratio)
        store[f'{prefix}.loss_seed'] = np.int64(LOSS_SEED + li)
        store_step(store, layers, prefix, res[torch.float32], res[torch.float64], coors, shape)
        print(f'layer {name:13s} seed {seed:3d} margin ratio {ratio:8.2f} rows {len(coors)} -> '
              f'{len(store[f"{prefix}.stage.keys"])}')

    np.savez_compressed(case_file('layers'), **layers)
    print(case_file('layers'), os.path.getsize(case_file('layers')), 'bytes')
    assert os.path.getsize(case_file('layers')) <= 1 << 20

    for ei, (name, (shape, count)) in enumerate(gen.ENCODERS.items()):
        batch, empty = (3, (1, )) if ei else (2, ())           # the second case has an empty sample in the middle
        prefix = f'enc.{name}'

        def build():
            return Encoder(sparse_shape=shape, **gen.ENCODER_CFG)

        def inputs(rng):
            coors = gen.clustered_coors(rng, shape, batch, count, empty=empty)
            return rng.uniform(-1, 1, (len(coors), 3)).astype(np.float32), coors

        seed, ratio, state, feats, coors, res = find_seed(build, inputs, 300 + 10 * ei, LOSS_SEED + 50 + ei, shape,
                                                          batch, True, prefix)
        big = {}
        store.update(state)
        store[f'{prefix}.features'], store[f'{prefix}.coors'] = feats, coors
        store[f'{prefix}.batch'], store[f'{prefix}.sparse_shape'] = np.int32(batch), np.asarray(shape, np.int32)
        store[f'{prefix}.case_seed'], store[f'{prefix}.pre_ratio'] = np.int64(seed), np.float64(ratio)
        store[f'{prefix}.loss_seed'] = np.int64(LOSS_SEED + 50 + ei)
        store_step(store, big, prefix, res[torch.float32], res[torch.float64], coors, shape)
        np.savez_compressed(case_file(name), **big)
        print(f'enc {name} seed {seed} margin ratio {ratio:.2f} rows {len(coors)} -> '
              f'{len(store[f"{prefix}.stage.keys"])}; {case_file(name)} {os.path.getsize(case_file(name))} bytes')
        assert os.path.getsize(case_file(name)) <= 1 << 20

    errs = {k: float(v) for k, v in store.items() if k.endswith('.err')}
    grads = [v for k, v in errs.items() if '.stage.' not in k and v > 0]
    print(f'{len(errs)} figures; gradients and statistics between {min(grads):.2e} and {max(grads):.2e}')
    np.savez_compressed(OUT, **store)
    print(OUT, os.path.getsize(OUT), 'bytes')
    assert os.path.getsize(OUT) <= 1 << 20


if __name__ == '__main__':
    main()
