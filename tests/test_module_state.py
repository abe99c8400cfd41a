"""Pickling and deep copies of the path's modules carry parameters, buffers and configuration only: what a
forward derives from them (packed weight fragments, folded norms, device copies held with weak references)
lives in each module's ``derived.Derived`` cache, which pickles and copies as an empty one, and is rebuilt."""
import copy
import io
import pickle

import importlib
from types import SimpleNamespace

import pytest
import torch


@pytest.fixture(scope='module')
def pkg():
    return SimpleNamespace(modules=importlib.import_module('depth-from-motion_amd.modules'),
                           conv3d=importlib.import_module('depth-from-motion_amd.conv3d'),
                           derived=importlib.import_module('depth-from-motion_amd.derived'))


def _backbone(pkg):
    return pkg.modules.DfMBackbone(in_channels=32, num_hg=1, cv_channels=32,
                                   depth_cfg=dict(mode='UD', num_bins=8, depth_min=2, depth_max=10,
                                                  downsample_factor=4))


def test_derived_state_is_not_pickled(pkg):
    torch.manual_seed(0)
    derived = pkg.derived.derived
    bb = _backbone(pkg)
    host = torch.arange(8.0)
    bb.downsampled_depth = host
    # what a forward would have left behind
    derived(bb).put(('on_device', 'downsampled_depth'), (host,), host.clone(), torch.device('cpu'))
    derived(bb).put('gate_pack', (bb.aggregate_cost.weight,), torch.zeros(4))
    derived(bb).put('sweep_conv_pack', (bb.dres0.conv.weight, bb.dres0_mono.conv.weight), torch.zeros(4))
    convs = [m for m in bb.modules() if isinstance(m, pkg.conv3d.MfmaConv3d)]
    assert convs
    derived(convs[0]).put('packs', (convs[0].weight,), [torch.zeros(3)])
    derived(convs[0]).put('split_packs', (convs[0].weight,), [torch.zeros(3)])
    to1 = [m for m in bb.modules() if isinstance(m, pkg.conv3d.MfmaConv3dTo1)]
    assert to1
    derived(to1[0]).put('pack', (to1[0].weight,), torch.zeros(3))

    for clone in (pickle.loads(pickle.dumps(bb)), copy.deepcopy(bb)):
        for name in (('on_device', 'downsampled_depth'), 'gate_pack', 'sweep_conv_pack'):
            assert derived(clone).peek(name) is None
        c2 = [m for m in clone.modules() if isinstance(m, pkg.conv3d.MfmaConv3d)][0]
        assert derived(c2).peek('packs') is None and derived(c2).peek('split_packs') is None
        t2 = [m for m in clone.modules() if isinstance(m, pkg.conv3d.MfmaConv3dTo1)][0]
        assert derived(t2).peek('pack') is None
        assert torch.equal(clone.downsampled_depth, host)
        sd, sd2 = bb.state_dict(), clone.state_dict()
        assert list(sd) == list(sd2) and all(torch.equal(sd[k], sd2[k]) for k in sd)
    # the original keeps its derived state
    assert derived(bb).peek('sweep_conv_pack') is not None and derived(convs[0]).peek('packs') is not None
    assert derived(bb).peek('gate_pack') is not None


def test_a_container_that_is_not_ours_leaves_its_fold_behind(pkg):
    """``_conv_norm_2d`` keeps the folded norm on the nn.Sequential it is handed (convbn): an entry there stays out
    of a copy as well"""
    seq = pkg.modules.convbn(32, 32, 3, 1, 1)
    norm = seq[1]
    pkg.derived.derived(seq).put('fold', (norm.weight, norm.bias, norm.running_mean, norm.running_var),
                                 (torch.ones(32), torch.zeros(32)), norm.eps)
    for clone in (pickle.loads(pickle.dumps(seq)), copy.deepcopy(seq)):
        assert pkg.derived.derived(clone).peek('fold') is None
        sd, sd2 = seq.state_dict(), clone.state_dict()
        assert list(sd) == list(sd2) and all(torch.equal(sd[k], sd2[k]) for k in sd)
    assert pkg.derived.derived(seq).peek('fold') is not None


def test_torch_save_of_a_whole_module(pkg):
    f2v = pkg.modules.FrustumToVoxel(num_3dconvs=1)
    coords = torch.zeros(2, 2, 2, 3)
    f2v.coordinates_3d = coords
    pkg.derived.derived(f2v).put('coords', (coords,), coords.clone(), torch.device('cpu'))
    buf = io.BytesIO()
    torch.save(f2v, buf)   # a weak reference in the state made this raise
    buf.seek(0)
    back = torch.load(buf, weights_only=False)
    assert pkg.derived.derived(back).peek('coords') is None and torch.equal(back.coordinates_3d, coords)
