"""CPU: the C-ABI library builds, loads and answers (no compute calls -- there is no GPU here).  That it exports
every symbol the headers declare, and that _capi.py binds each as declared, is tests/test_capi_binding.py."""
import ctypes
import importlib

import pytest


@pytest.fixture(scope='module')
def pkg():
    importlib.import_module('depth-from-motion_amd.build').build_hip()
    return importlib.import_module('depth-from-motion_amd')


def test_version_and_error_string(pkg):
    lib = pkg._capi.lib()
    assert lib.dfm_version() == 3
    assert isinstance(lib.dfm_last_error(), bytes)


def test_invalid_desc_is_rejected_without_touching_the_gpu(pkg):
    lib = pkg._capi.lib()
    desc = pkg._capi.SweepDesc()  # all zero -> invalid sizes
    assert lib.dfm_plane_sweep_workspace_bytes(ctypes.byref(desc)) == 0
    rc = lib.dfm_plane_sweep_fwd(ctypes.byref(desc), None, None, None, None, None, None, None,
                                 None, 0, None)
    assert rc == -1
    assert b'size' in lib.dfm_last_error()
    desc.batch = desc.channels = desc.h_in = desc.w_in = 4
    desc.num_depths = desc.h_out = desc.w_out = 4
    desc.dtype = 7
    assert lib.dfm_plane_sweep_fwd(ctypes.byref(desc), None, None, None, None, None, None, None,
                                   None, 0, None) == -2
    desc.dtype = 0
    # two blocked maps (4 samples x 1 block x 16 px x 16 B) + the two spill lists (second-chance
    # LDS pass, direct pass: int32 counter + 1 band x 4 planes x 2 maps x 4 samples tile ids each)
    assert lib.dfm_plane_sweep_workspace_bytes(ctypes.byref(desc)) == 2 * 1024 + 2 * 256 + 256
    # NULL pointers
    assert lib.dfm_plane_sweep_fwd(ctypes.byref(desc), None, None, None, None, None, None, None,
                                   None, 0, None) == -1


def test_ops_refuse_cpu_tensors(pkg):
    import torch
    x = torch.zeros(1, 4, 8, 8)
    with pytest.raises(RuntimeError, match='no CPU path'):
        pkg.build_dfm_cost(x, x, torch.ones(3), 1, 1, torch.eye(4)[None], torch.eye(4)[None],
                           (8, 8))
