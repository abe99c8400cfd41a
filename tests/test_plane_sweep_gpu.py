"""GPU parity tests of the plane-sweep kernels, through the C ABI.

Bar (DESIGN.md "Numerics"): fp32 storage -> BIT-EXACT against the oracle and
against the reference's own PyTorch-CPU output (tests/golden); bf16 storage ->
bit-exact against bf16(oracle(bf16-rounded inputs)) (interpolation in fp32,
one final rounding).  Backward (atomics, order not fixed): rtol 1e-4 /
atol 1e-5 against torch's CPU grid_sample autograd on the oracle's grids.
"""
import importlib
import os

import numpy as np
import pytest
import torch

from oracle import dfm_oracle as orc
from tests import util

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def pkg():
    assert torch.cuda.is_available(), 'GPU tests need a GPU (no fallback path exists)'
    p = importlib.import_module('depth-from-motion_amd')
    assert os.path.exists(p._capi.LIB_PATH)
    return p


# kernel variants every parity case runs through (dfm_sweep_opts of every call in the test):
#   gather    : lane-per-point kernel (also what non-vectorisable shapes take)
#   lds128/256: LDS-staged tile kernel, 128- / 256-lane workgroups
#   lds_spill : LDS budget too small for any tile -> every tile is flagged and
#               redone by the direct-tap pass
#   lds_respill: budget too small for most tiles -> flagged tiles take the second-chance LDS pass
#               (144 KiB, split by channel block)
#   direct    : tile kernel with direct taps for every tile (strided sweeps)
#   clt       : pixel-major taps + LDS transpose to the reference layout (strided sweeps, config K);
#               shapes it does not cover (odd channel counts / plane sizes) take the default dispatch
#   cltw      : the same with the depth axis walked per wave, footprints cached in registers (fp32, 32-channel
#               passes, 32-point tiles; what the default picks for strided sweeps where it applies)
#   lds256_chunk: shipped shape with 3 adjacent bands scheduled back to back
#   lds512_v4 / lds1024_v4: 4 points per lane (bf16: 8-byte stores, 4 waves per SIMD)
#   pipe*     : the pipelined body of the LDS tile kernel (two LDS buffers, one barrier per channel
#               block, counted vmcnt; the default since round 4) in the shapes the library ships,
#               with odd / even numbers of channel blocks per workgroup, and with a budget that
#               sends tiles to the second-chance and direct passes; the lds* modes pin the serial body
#   *_valu    : bf16 taps unpacked by the VALU (default for pipelined 8-point bf16 tiles: the matrix core)
#   *_unpaired: 4 points per lane with 8-byte stores (default: lane pairs trade halves, 16-byte stores)
#   *_a32/_a64: tile boundaries at multiples of 32 / 64 lattice points (whole 64- / 128-byte writes)
MODES = {'gather': dict(kernel=1, lanes=256, lds_kib=64, blocks_per_group=4, planes=1),
         'lds128_p1': dict(kernel=2, lanes=128, lds_kib=36, blocks_per_group=1, planes=1, pipeline=1),
         'lds128_p2': dict(kernel=2, lanes=128, lds_kib=36, blocks_per_group=1000, planes=2, pipeline=1),
         'lds256_p1': dict(kernel=2, lanes=256, lds_kib=64, blocks_per_group=4, planes=1, pipeline=1),
         'lds256_p2': dict(kernel=2, lanes=256, lds_kib=52, blocks_per_group=1000, planes=2, pipeline=1),
         'lds256_p4': dict(kernel=2, lanes=256, lds_kib=52, blocks_per_group=1000, planes=4, pipeline=1),
         'lds256_chunk': dict(kernel=2, lanes=256, lds_kib=52, planes=2, bands_per_chunk=3, pipeline=1),
         'lds512_v4': dict(kernel=2, lanes=512, lds_kib=52, planes=2, points_per_lane=4, pipeline=1),
         'lds1024_v4': dict(kernel=2, lanes=1024, lds_kib=64, planes=4, points_per_lane=4,
                            bands_per_chunk=2, pipeline=1),
         'lds_spill': dict(kernel=2, lanes=128, lds_kib=4, blocks_per_group=2, planes=2,
                           bands_per_chunk=2, pipeline=1),
         'lds_respill': dict(kernel=2, lanes=256, lds_kib=16, planes=2, pipeline=1),
         'pipe256': dict(kernel=2, lanes=256, planes=2, pipeline=2),
         'pipe256_b3': dict(kernel=2, lanes=256, planes=1, blocks_per_group=3, pipeline=2),
         'pipe128_b1': dict(kernel=2, lanes=128, planes=2, blocks_per_group=1, pipeline=2),
         'pipe512_v4': dict(kernel=2, lanes=512, planes=2, points_per_lane=4, pipeline=2),
         'pipe1024_v4': dict(kernel=2, lanes=1024, planes=4, points_per_lane=4, bands_per_chunk=2,
                             pipeline=2),
         'pipe_spill': dict(kernel=2, lanes=128, lds_kib=4, blocks_per_group=2, planes=2, pipeline=2),
         'pipe_respill': dict(kernel=2, lanes=256, lds_kib=24, planes=2, pipeline=2),
         'pipe256_a64': dict(kernel=2, lanes=256, planes=2, pipeline=2, store_align=64),
         'pipe256_valu': dict(kernel=2, lanes=256, planes=2, pipeline=2, unpack=2),
         'lds256_a32': dict(kernel=2, lanes=256, lds_kib=52, planes=2, pipeline=1, store_align=32),
         'pipe512_v4_a64': dict(kernel=2, lanes=512, planes=2, points_per_lane=4, pipeline=2, store_align=64),
         'lds256_a8': dict(kernel=2, lanes=256, lds_kib=52, planes=2, pipeline=1, store_align=8),
         'pipe512_v4_unpaired': dict(kernel=2, lanes=512, planes=2, points_per_lane=4, pipeline=2, pair_stores=2),
         'lds256_v4_unpaired': dict(kernel=2, lanes=256, planes=2, points_per_lane=4, pipeline=1, pair_stores=2,
                                    store_align=16),
         'direct': dict(kernel=3, lanes=256, lds_kib=64, blocks_per_group=4, planes=1),
         'clt': dict(kernel=4),
         'cltw': dict(kernel=5)}


@pytest.fixture(params=sorted(MODES), autouse=True)
def kernel_mode(request, pkg):
    sweep = importlib.import_module('depth-from-motion_amd.plane_sweep')
    with sweep.launch_options(**MODES[request.param]):
        yield request.param


def run_hip(pkg, cur, prev, depths, fsf, csf, P, T, img_shape, flip, crop, scale, dtype=torch.float32):
    dev = torch.device('cuda:0')
    c = torch.from_numpy(np.ascontiguousarray(cur)).to(dev).to(dtype)
    p = torch.from_numpy(np.ascontiguousarray(prev)).to(dev).to(dtype)
    out = pkg.build_dfm_cost(c, p, torch.from_numpy(np.asarray(depths, np.float32)).to(dev), fsf,
                             csf, torch.from_numpy(np.asarray(P, np.float32)),
                             torch.from_numpy(np.asarray(T, np.float32)), img_shape, flip, crop,
                             scale)
    torch.cuda.synchronize()
    assert pkg._capi.lib().dfm_plane_sweep_last_kernel() in (1, 2, 3, 4, 5)
    return out


def fixture_args(z):
    return (float(z['fsf']), float(z['csf']), z['P'][None], z['T'][None],
            tuple(int(v) for v in z['img_shape']), bool(z['flip']),
            tuple(float(v) for v in z['crop']), float(z['scale']))


@pytest.mark.parametrize('path', util.sweep_fixture_paths(),
                         ids=lambda p: os.path.basename(p)[12:-4])
def test_fp32_bitexact_vs_reference_fixture(pkg, path):
    z = np.load(path)
    out = run_hip(pkg, z['cur'], z['prev'], z['depths'], *fixture_args(z)).cpu().numpy()
    assert out.shape == z['ref_out'].shape
    if 'zero_depth' in path or 'nan_coords' in path:
        # non-finite sampling coordinates: the reference (torch-CPU) gives NaN, the kernels +0 (util's docstring)
        assert util.assert_matches_reference(out, z['ref_out']) > 0
        return
    assert np.array_equal(out, z['ref_out'])
    assert np.array_equal(util.bits(out), util.bits(z['ref_out']))


@pytest.mark.parametrize('path', util.sweep_fixture_paths(),
                         ids=lambda p: os.path.basename(p)[12:-4])
def test_grid_bitexact_vs_reference_fixture(pkg, path):
    z = np.load(path)
    fsf, csf, P, T, img_shape, flip, crop, scale = fixture_args(z)
    dev = torch.device('cuda:0')
    cg, pg = pkg.plane_sweep_grid(torch.from_numpy(z['cur']).to(dev),
                                  torch.from_numpy(z['depths']).to(dev), fsf, csf,
                                  torch.from_numpy(P), torch.from_numpy(T), img_shape, flip, crop,
                                  scale)
    for got, ref in ((cg.cpu().numpy(), z['ref_cur_grid']), (pg.cpu().numpy(), z['ref_prev_grid'])):
        # (a NaN coordinate -- 0 / 0, plane_sweep_nan_coords.npz -- is NaN on both sides; its sign / payload bits
        #  are the divider's business: x86 and gfx950 differ)
        nan = np.isnan(ref)
        assert np.array_equal(np.isnan(got), nan)
        assert np.array_equal(util.bits(np.where(nan, 0, got)), util.bits(np.where(nan, 0, ref)))


@pytest.mark.parametrize('path', util.sweep_fixture_paths(),
                         ids=lambda p: os.path.basename(p)[12:-4])
def test_bf16_exact_vs_oracle(pkg, path):
    z = np.load(path)
    fsf, csf, P, T, img_shape, flip, crop, scale = fixture_args(z)
    cur16, prev16 = orc.bf16_round(z['cur']), orc.bf16_round(z['prev'])
    ref = orc.bf16_round(
        orc.build_dfm_cost(cur16, prev16, z['depths'], fsf, csf, P, z['Pinv'][None], T, img_shape,
                           flip, crop, scale))
    out = run_hip(pkg, cur16, prev16, z['depths'], fsf, csf, P, T, img_shape, flip, crop, scale,
                  dtype=torch.bfloat16)
    assert out.dtype == torch.bfloat16
    assert np.array_equal(util.bits(out.float().cpu().numpy()), util.bits(ref))


@pytest.mark.parametrize('special', ['neg_zero', 'denormal', 'inf', 'nan'])
def test_bf16_special_values_take_the_valu_unpack(pkg, special):
    """the matrix-core unpack of the pipelined bf16 tile kernel is exact for finite normal values and +0
    only: the pack kernel flags anything else and the tiles run through the VALU unpack.  The volume must
    equal the oracle's bit for bit (NaN payloads aside) with ONE special value planted in each map."""
    z = np.load(util.sweep_fixture_paths()[0])
    fsf, csf, P, T, img_shape, flip, crop, scale = fixture_args(z)
    cur16, prev16 = orc.bf16_round(z['cur']).copy(), orc.bf16_round(z['prev']).copy()
    val = {'neg_zero': np.float32(-0.0), 'denormal': np.frombuffer(np.uint32(0x00010000).tobytes(), np.float32)[0],
           'inf': np.float32(np.inf), 'nan': np.float32(np.nan)}[special]
    C, H, W = cur16.shape[1:]
    cur16[0, C // 2, H // 2, W // 3] = val
    prev16[0, 1 % C, H // 3, W // 2] = val
    # a whole channel of -0 / denormals as well (sign and exponent of a blend of four such taps)
    if special in ('neg_zero', 'denormal'):
        cur16[0, 0] = val
    with np.errstate(invalid='ignore'):
        ref = orc.bf16_round(
            orc.build_dfm_cost(cur16, prev16, z['depths'], fsf, csf, P, z['Pinv'][None], T, img_shape,
                               flip, crop, scale))
    out = run_hip(pkg, cur16, prev16, z['depths'], fsf, csf, P, T, img_shape, flip, crop, scale,
                  dtype=torch.bfloat16).float().cpu().numpy()
    nan_ref, nan_out = np.isnan(ref), np.isnan(out)
    assert np.array_equal(nan_ref, nan_out)
    assert np.array_equal(util.bits(np.where(nan_out, 0, out)), util.bits(np.where(nan_ref, 0, ref)))


@pytest.mark.parametrize('special', ['neg_zero', 'nan'])
def test_bf16_special_values_on_a_narrow_map_beyond_the_64th_staged_row(pkg, special):
    """a narrow, tall map (32 x 192): a 256-lane x 8-point tile holds 64 lattice rows and stages 64+ map rows in
    one pipelined buffer.  The per-row special-value check of the matrix-core body looked at the first 64 staged
    rows only: a -0 / NaN further down went through the matrix-core unpack (lost sign / NaN in
    the other seven channels of the block).  Planted in the LAST rows a tile stages, every mode, vs the oracle."""
    rng = np.random.RandomState(21)
    C, H, W, D = 16, 192, 32, 4
    cur16 = orc.bf16_round(rng.randn(1, C, H, W).astype(np.float32))
    prev16 = orc.bf16_round(rng.randn(1, C, H, W).astype(np.float32))
    val = np.float32(-0.0) if special == 'neg_zero' else np.float32(np.nan)
    for r in (62, 63, 64, 65, 66, 70, 127, 128, 129, 130, 135, 190, 191):   # either side of every 64-row boundary
        cur16[0, 3, r, 5::7] = val
        prev16[0, 9, r, 2::5] = val
    if special == 'neg_zero':
        cur16[0, 1, 60:] = val
    P = util.KITTI_P2[None].copy()
    T = util.random_poses(1, seed=4)
    depths = util.depth_planes(72)[[3, 20, 41, 70]]
    # lattice = map (csf 1); fsf 6: the 32 x 192 lattice spans 186 x 1146 image pixels, rows map 1:1 for the cur half
    args = (6, 1, P, util.host_inverse(P), T, (375, 1242), False, (0, 0), 1.0)
    with np.errstate(invalid='ignore'):
        ref = orc.bf16_round(orc.build_dfm_cost(cur16, prev16, depths, *args))
    out = run_hip(pkg, cur16, prev16, depths, 6, 1, P, T, (375, 1242), False, (0, 0), 1.0,
                  dtype=torch.bfloat16).float().cpu().numpy()
    nan_ref, nan_out = np.isnan(ref), np.isnan(out)
    assert np.array_equal(nan_ref, nan_out)
    assert np.array_equal(util.bits(np.where(nan_out, 0, out)), util.bits(np.where(nan_ref, 0, ref)))


@pytest.mark.parametrize('W', [101, 104])  # 101: D*H*W not a multiple of 8 -> gather kernel
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_batched_per_sample_semantics(pkg, dtype, W):
    """B=3, different pose and intrinsics per sample == oracle looped at B=1."""
    rng = np.random.RandomState(7)
    B, C, H, D = 3, 12, 30, 7
    cur = orc.bf16_round(rng.randn(B, C, H, W).astype(np.float32))
    prev = orc.bf16_round(rng.randn(B, C, H, W).astype(np.float32))
    P = np.stack([util.KITTI_P2] * B).copy()
    P[1, 0, 2] += 3.5
    P[2, 1, 1] *= 1.01
    T = util.random_poses(B, seed=11)
    depths = util.depth_planes(D)
    Pinv = util.host_inverse(P)
    ref = orc.build_dfm_cost(cur, prev, depths, 12, 1, P, Pinv, T, (375, 1242), False, (0, 0), 1.0)
    out = run_hip(pkg, cur, prev, depths, 12, 1, P, T, (375, 1242), False, (0, 0), 1.0, dtype)
    if dtype == torch.bfloat16:
        ref = orc.bf16_round(ref)
    assert np.array_equal(util.bits(out.float().cpu().numpy()), util.bits(ref))


def test_kitti_shape_subvolume_vs_oracle(pkg):
    """config K geometry (320x1280 feats, csf=4, crop (0,55)) at reduced C/D."""
    rng = np.random.RandomState(3)
    C, H, W, D = 8, 320, 1280, 4
    cur = rng.randn(1, C, H, W).astype(np.float32)
    prev = rng.randn(1, C, H, W).astype(np.float32)
    P, T = util.KITTI_P2[None], util.random_poses(1, seed=5)
    depths = util.depth_planes(72)[[0, 17, 40, 71]]
    ref = orc.build_dfm_cost(cur, prev, depths, 1, 4, P, util.host_inverse(P), T, (375, 1242),
                             False, (0, 55), 1.0)
    out = run_hip(pkg, cur, prev, depths, 1, 4, P, T, (375, 1242), False, (0, 55), 1.0)
    assert out.shape == (1, 2 * C, D, 80, 320)
    assert np.array_equal(util.bits(out.cpu().numpy()), util.bits(ref))


def test_north_star_shape_slices_and_properties(pkg):
    """Full N* geometry (C=256, D=112, 94x311, bf16) for one sample:
    (a) a few depth planes x channels against the oracle, bit-exact;
    (b) identity pose + prev==cur  =>  prev half == cur half (bitwise);
    (c) scaling the inputs by 2 scales the volume by exactly 2."""
    rng = np.random.RandomState(0)
    C, H, W, D = 256, 94, 311, 112
    cur = orc.bf16_round(rng.randn(1, C, H, W).astype(np.float32))
    prev = orc.bf16_round(rng.randn(1, C, H, W).astype(np.float32))
    P, T = util.KITTI_P2[None], util.random_poses(1, seed=2)
    depths = util.depth_planes(D)
    common = (4, 1, P, T, (375, 1242), False, (0, 0), 1.0)
    out = run_hip(pkg, cur, prev, depths, *common, dtype=torch.bfloat16)
    assert out.shape == (1, 2 * C, D, H, W)
    dsel, csel = [0, 55, 111], [0, 1, 100, 255]
    ref = orc.bf16_round(
        orc.build_dfm_cost(cur[:, csel], prev[:, csel], depths[dsel], 4, 1, P,
                           util.host_inverse(P), T, (375, 1242), False, (0, 0), 1.0))
    got = out[:, csel + [C + c for c in csel]][:, :, dsel].float().cpu().numpy()
    assert np.array_equal(util.bits(got), util.bits(ref))
    # (c) exact linearity under power-of-two scaling
    out2 = run_hip(pkg, 2 * cur, 2 * prev, depths, *common, dtype=torch.bfloat16)
    assert torch.equal(out2, out * 2)
    del out2
    # (b) identity pose
    eye = np.eye(4, dtype=np.float32)[None]
    outi = run_hip(pkg, cur, cur, depths, 4, 1, P, eye, (375, 1242), False, (0, 0), 1.0,
                   dtype=torch.bfloat16)
    assert torch.equal(outi[:, :C], outi[:, C:])


def _check_backward(pkg, B, C, H, W, D, fsf, csf, crop, seed, img_shape, dtype=torch.float32,
                    tol=dict(rtol=1e-4, atol=1e-5), t_z=None):
    rng = np.random.RandomState(seed)
    cur = rng.randn(B, C, H, W).astype(np.float32)
    prev = rng.randn(B, C, H, W).astype(np.float32)
    P = np.stack([util.KITTI_P2] * B)
    T = util.random_poses(B, seed=seed + 4)
    if t_z is not None:
        T[:, 2, 3] = t_z  # strong forward motion: the prev footprint drifts across rows with depth
    Pinv = util.host_inverse(P)
    depths = util.depth_planes(D)
    ho, wo = round(H / csf), round(W / csf)
    gout = rng.randn(B, 2 * C, D, ho, wo).astype(np.float32)
    if dtype == torch.bfloat16:
        gout = orc.bf16_round(gout)
    dev = torch.device('cuda:0')
    c = torch.from_numpy(cur).to(dev).to(dtype).requires_grad_(True)
    p = torch.from_numpy(prev).to(dev).to(dtype).requires_grad_(True)
    out = pkg.build_dfm_cost(c, p, torch.from_numpy(depths).to(dev), fsf, csf, torch.from_numpy(P),
                             torch.from_numpy(T), img_shape, False, crop, 1.0)
    out.backward(torch.from_numpy(gout).to(dev).to(dtype))
    torch.cuda.synchronize()
    # reference gradient: torch CPU autograd through grid_sample on the oracle's grids
    for b in range(B):
        prm = orc.sweep_params(H, W, D, fsf, csf, P[b], Pinv[b], T[b], img_shape, False, crop, 1.0)
        cg, pg = orc.plane_sweep_grid(prm, depths)
        for feats, grid, got, sl in ((cur, cg, c.grad, slice(0, C)), (prev, pg, p.grad, slice(C, 2 * C))):
            f = torch.from_numpy(feats[b:b + 1]).requires_grad_(True)
            o = torch.nn.functional.grid_sample(f, torch.from_numpy(grid).view(1, 1, -1, 2),
                                                mode='bilinear', padding_mode='zeros',
                                                align_corners=True)
            o.backward(torch.from_numpy(gout[b:b + 1, sl]).reshape(o.shape))
            ref = f.grad[0].numpy()
            assert np.abs(ref).max() > 0.1
            np.testing.assert_allclose(got[b].float().cpu().numpy(), ref, **tol)


def test_backward_matches_torch_cpu_autograd(pkg):
    """strided sweep (cost_sample_factor 2), six channels: the default backward dispatch, i.e. the LDS-atomic tile
    kernel on a strided lattice (id 5).  The ``kernel_mode`` fixture's ``launch_options`` are thread-local and never
    reach the autograd thread that runs the backward (tests/test_host_logic_round3.py), so every mode of this file
    takes that same kernel; the scatter kernel (id 1) is pinned in tests/test_sweep_bwd_exact_gpu.py."""
    _check_backward(pkg, 2, 6, 20, 64, 3, 8, 2, (3, 5), 5, (375, 1242))
    assert pkg._capi.lib().dfm_plane_sweep_bwd_last_kernel() == 5


@pytest.mark.parametrize('case', [
    # dense sweeps: LDS-accumulating tile kernel (unless the mode forces the scatter kernel)
    dict(B=2, C=11, H=24, W=96, D=9, fsf=4, csf=1, crop=(0, 0), seed=1, img_shape=(96, 384)),
    # 4-row slab window (wide rows) + strong forward motion: window rebasing and taps
    # outside the window
    dict(B=1, C=8, H=14, W=640, D=7, fsf=2, csf=1, crop=(2, 1), seed=2, img_shape=(28, 1280),
         t_z=-1.9),
    # more than one depth chunk, partial last band
    dict(B=1, C=3, H=37, W=53, D=41, fsf=4, csf=1, crop=(0, 0), seed=3, img_shape=(148, 212)),
], ids=['small', 'wide_rows', 'deep'])
def test_backward_dense_sweep_matches_torch_cpu_autograd(pkg, case):
    _check_backward(pkg, **case)


def test_backward_zero_and_nonfinite_gradients(pkg, kernel_mode):
    """the dense-sweep backward scales the incoming gradients by their maximum: an all-zero
    volume gives zero gradients, a NaN/Inf in it poisons the result instead of being scaled"""
    if kernel_mode != 'lds256_p2':
        pytest.skip('runs once')
    dev = torch.device('cuda:0')
    rng = np.random.RandomState(0)
    args = (torch.from_numpy(util.depth_planes(3)).to(dev), 4, 1, torch.from_numpy(util.KITTI_P2[None]),
            torch.from_numpy(util.random_poses(1, seed=1)), (48, 160))
    for poison in (None, float('nan'), float('inf')):
        c = torch.from_numpy(rng.randn(1, 8, 12, 40).astype(np.float32)).to(dev).requires_grad_(True)
        p = torch.from_numpy(rng.randn(1, 8, 12, 40).astype(np.float32)).to(dev).requires_grad_(True)
        g = torch.zeros(1, 16, 3, 12, 40, device=dev)
        if poison is not None:
            g[0, 3, 1, 5, 7] = poison
        pkg.build_dfm_cost(c, p, *args).backward(g)
        if poison is None:
            assert float(c.grad.abs().max()) == 0.0 and float(p.grad.abs().max()) == 0.0
        else:
            assert bool(torch.isnan(c.grad).any()) and not bool(torch.isfinite(c.grad[0, 3]).all())
    # tiny and huge gradient scales keep their relative accuracy (the scale follows max |grad|)
    for scale in (1e-20, 1e15):
        c = torch.from_numpy(rng.randn(1, 8, 12, 40).astype(np.float32)).to(dev).requires_grad_(True)
        p = torch.from_numpy(rng.randn(1, 8, 12, 40).astype(np.float32)).to(dev).requires_grad_(True)
        g = torch.from_numpy(rng.randn(1, 16, 3, 12, 40).astype(np.float32)).to(dev)
        pkg.build_dfm_cost(c, p, *args).backward(g)
        g1 = c.grad.clone()
        c.grad = p.grad = None
        pkg.build_dfm_cost(c, p, *args).backward(g * scale)
        assert torch.allclose(c.grad / scale, g1, rtol=1e-5, atol=1e-6)


def test_backward_bf16_gradients(pkg):
    _check_backward(pkg, 1, 8, 24, 96, 9, 4, 1, (0, 0), 7, (96, 384), dtype=torch.bfloat16,
                    tol=dict(rtol=2e-2, atol=2e-2))


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('case', [
    dict(B=2, C=8, H=20, W=64, D=5, fsf=8, csf=2, crop=(3, 5), flip=False, scale=1.0),
    dict(B=1, C=40, H=24, W=96, D=4, fsf=4, csf=1, crop=(0, 0), flip=True, scale=1.03),
    dict(B=3, C=256, H=9, W=31, D=3, fsf=4, csf=1, crop=(0, 0), flip=False, scale=1.0),
    dict(B=1, C=16, H=37, W=53, D=7, fsf=4, csf=1, crop=(11, 55), flip=False, scale=0.97),
], ids=['strided_c8', 'c40_flip_scale', 'c256', 'partial_tiles'])
def test_channels_last_volume_equals_reference_layout(pkg, case, dtype, kernel_mode):
    """memory_format=channels_last_3d: same shape, same values bit for bit as the
    (B,2C,D,H,W)-contiguous volume (itself checked against the oracle / fixtures above)"""
    if kernel_mode != 'lds256_p2':
        pytest.skip('layout check runs once, against the shipped kernel configuration')
    rng = np.random.RandomState(case['C'])
    B, C, H, W, D = (case[k] for k in 'BCHWD')
    cur = rng.randn(B, C, H, W).astype(np.float32)
    prev = rng.randn(B, C, H, W).astype(np.float32)
    P = np.stack([util.KITTI_P2] * B)
    T = util.random_poses(B, seed=3)
    T[0, 2, 3] = 4.0  # one sample with planes behind the prev camera (z <= 0 -> zeros / NaN coords)
    dev = torch.device('cuda:0')
    c = torch.from_numpy(cur).to(dev).to(dtype)
    p = torch.from_numpy(prev).to(dev).to(dtype)
    args = (torch.from_numpy(util.depth_planes(D)).to(dev), case['fsf'], case['csf'], torch.from_numpy(P),
            torch.from_numpy(T), (375, 1242), case['flip'], case['crop'], case['scale'])
    ref = pkg.build_dfm_cost(c, p, *args)
    out = pkg.build_dfm_cost(c, p, *args, memory_format=torch.channels_last_3d)
    torch.cuda.synchronize()
    assert out.shape == ref.shape and out.is_contiguous(memory_format=torch.channels_last_3d)
    assert out.stride(1) == 1
    ob, rb = out.contiguous().view(-1), ref.view(-1)
    bits = torch.int32 if dtype == torch.float32 else torch.int16
    assert torch.equal(ob.view(bits), rb.view(bits))
    # channels_last (NHWC) feature maps -- what the channels_last 2-D neck emits -- are sampled in
    # place (dfm_plane_sweep_fwd_nhwc, no pack pass): the same volume bit for bit
    if C % (16 // c.element_size()) == 0:
        sweep = importlib.import_module('depth-from-motion_amd.plane_sweep')
        cn, pn = (t.contiguous(memory_format=torch.channels_last) for t in (c, p))
        assert sweep._nhwc(cn) and not sweep._nhwc(c)
        out2 = pkg.build_dfm_cost(cn, pn, *args, memory_format=torch.channels_last_3d)
        assert out2.is_contiguous(memory_format=torch.channels_last_3d)
        assert torch.equal(out2.contiguous().view(-1).view(bits), rb.view(bits))
        # (the reference layout from NHWC maps goes through a contiguous copy)
        out3 = pkg.build_dfm_cost(cn, pn, *args)
        assert torch.equal(out3.view(-1).view(bits), rb.view(bits))


def test_channels_last_backward_and_errors(pkg, kernel_mode):
    if kernel_mode != 'lds256_p2':
        pytest.skip('runs once')
    dev = torch.device('cuda:0')
    rng = np.random.RandomState(0)
    c = torch.from_numpy(rng.randn(1, 8, 12, 40).astype(np.float32)).to(dev).requires_grad_(True)
    p = torch.from_numpy(rng.randn(1, 8, 12, 40).astype(np.float32)).to(dev).requires_grad_(True)
    args = (torch.from_numpy(util.depth_planes(3)).to(dev), 4, 1, torch.from_numpy(util.KITTI_P2[None]),
            torch.from_numpy(util.random_poses(1, seed=1)), (48, 160))
    g = torch.from_numpy(rng.randn(1, 16, 3, 12, 40).astype(np.float32)).to(dev)
    out = pkg.build_dfm_cost(c, p, *args, memory_format=torch.channels_last_3d)
    out.backward(g.contiguous(memory_format=torch.channels_last_3d))
    gc, gp = c.grad.clone(), p.grad.clone()
    c.grad = p.grad = None
    pkg.build_dfm_cost(c, p, *args).backward(g)
    assert torch.allclose(gc, c.grad, rtol=1e-5, atol=1e-6) and torch.allclose(gp, p.grad, rtol=1e-5, atol=1e-6)
    # NHWC feature maps: same gradients
    cn = c.detach().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    pn = p.detach().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    pkg.build_dfm_cost(cn, pn, *args, memory_format=torch.channels_last_3d).backward(
        g.contiguous(memory_format=torch.channels_last_3d))
    assert torch.allclose(gc, cn.grad, rtol=1e-5, atol=1e-6) and torch.allclose(gp, pn.grad, rtol=1e-5, atol=1e-6)
    with pytest.raises(RuntimeError):  # 6 channels are not a whole 16-byte block
        pkg.build_dfm_cost(c[:, :6].detach(), p[:, :6].detach(), *args, memory_format=torch.channels_last_3d)


def test_autotune_keeps_results_exact(pkg, kernel_mode):
    if kernel_mode != 'lds256_p2':
        pytest.skip('runs once')
    sweep = importlib.import_module('depth-from-motion_amd.plane_sweep')
    dev = torch.device('cuda:0')
    rng = np.random.RandomState(2)
    B, C, H, W, D = 2, 16, 40, 120, 6
    cur = torch.from_numpy(rng.randn(B, C, H, W).astype(np.float32)).to(dev).bfloat16()
    prev = torch.from_numpy(rng.randn(B, C, H, W).astype(np.float32)).to(dev).bfloat16()
    depths = torch.from_numpy(util.depth_planes(D)).to(dev)
    desc = sweep._make_desc(cur, D, 4, 1, (160, 480), False, (0, 0), 1.0)
    P, Pinv, T = sweep.camera_matrices(torch.from_numpy(np.stack([util.KITTI_P2] * B)),
                                       torch.from_numpy(util.random_poses(B, seed=3)), B, dev)
    ref = sweep.plane_sweep_forward(desc, cur, prev, depths, P, Pinv, T).clone()
    out = torch.empty_like(ref)
    pkg._capi.lib().dfm_plane_sweep_reset_tuning()
    assert sweep.plane_sweep_tuning(desc) is None
    with sweep.launch_options():  # no per-call options: the tuned cache is what the launch uses
        chosen = sweep.plane_sweep_autotune(desc, cur, prev, depths, P, Pinv, T, out)
        assert chosen['bands_per_chunk'] in (1, 15) and chosen['lanes_per_workgroup'] in (0, 512)
        assert sweep.plane_sweep_tuning(desc) == chosen
        assert torch.equal(out.view(torch.int16), ref.view(torch.int16))
        again = sweep.plane_sweep_forward(desc, cur, prev, depths, P, Pinv, T)
        assert torch.equal(again.view(torch.int16), ref.view(torch.int16))
    pkg._capi.lib().dfm_plane_sweep_reset_tuning()


def test_camera_matrices_on_device_match_host(pkg, kernel_mode):
    """Device-resident intrinsics / poses (what the reference pipeline passes,
    dfm_backbone.py:151-154) are padded, inverted and packed on the device with no host round
    trip; the result agrees with the host path to fp32 inverse rounding."""
    if kernel_mode != 'lds256_p2':
        pytest.skip('runs once')
    sweep = importlib.import_module('depth-from-motion_amd.plane_sweep')
    dev = torch.device('cuda:0')
    B = 3
    K = torch.from_numpy(np.stack([util.KITTI_P2] * B))
    T = torch.from_numpy(util.random_poses(B, seed=7))
    Ph, Pih, Th = sweep.camera_matrices(K, T, B, dev)
    Pd, Pid, Td = sweep.camera_matrices(K.to(dev), T.to(dev), B, dev)
    assert Pd.is_cuda and Pid.is_cuda and Pd.shape == (B, 16)
    assert torch.equal(Pd, Ph) and torch.equal(Td, Th)
    assert torch.allclose(Pid, Pih, rtol=1e-5, atol=1e-7)
    # 3x4 and 3x3 intrinsics are padded like points_img2cam does (utils.py:239-240)
    P34, _, _ = sweep.camera_matrices(K[:, :3].to(dev), T.to(dev), B, dev)
    assert torch.equal(P34, Ph)
    P33, _, _ = sweep.camera_matrices(K[:, :3, :3], T, B, dev)
    ref33 = Ph.clone().view(B, 4, 4)
    ref33[:, :3, 3] = 0
    assert torch.equal(P33.view(B, 4, 4), ref33)
    # a precomputed inverse is passed through untouched
    _, Pi2, _ = sweep.camera_matrices(K.to(dev), T.to(dev), B, dev, cam2img_inv=Pih.view(B, 4, 4).cpu())
    assert torch.equal(Pi2.view(-1), Pih.view(-1))


def test_type_and_shape_errors(pkg):
    dev = torch.device('cuda:0')
    x = torch.zeros(1, 4, 8, 8, device=dev)
    eye = torch.eye(4)[None]
    with pytest.raises(TypeError):
        pkg.build_dfm_cost(x.half(), x.half(), torch.ones(3), 1, 1, eye, eye, (8, 8))
    with pytest.raises(TypeError):
        pkg.build_dfm_cost(x, x.bfloat16(), torch.ones(3), 1, 1, eye, eye, (8, 8))
    with pytest.raises(AssertionError):
        pkg.build_dfm_cost(x, x[:, :2], torch.ones(3), 1, 1, eye, eye, (8, 8))


@pytest.mark.parametrize('in_place', [False, True])
@pytest.mark.parametrize('shape,fsf,csf,D,dtype', [((2, 32, 24, 78), 16, 1, 9, torch.bfloat16),
                                                 ((1, 32, 64, 256), 1, 4, 30, torch.bfloat16),
                                                 ((1, 8, 48, 160), 1, 4, 5, torch.float32)])
def test_channels_last_gradient_without_a_torch_layout_conversion(pkg, shape, fsf, csf, D, dtype, in_place):
    """the NDHWC stack hands the cost volume's gradient over channels-last:
    ``dfm_plane_sweep_bwd_channels_last`` re-lays it with the library's LDS-tile transpose (workspace
    given) or reads it where it lies (``in_place``: no workspace) -- same gradients as from the
    reference layout, and the library entry point really took the call"""
    dev = torch.device('cuda:0')
    g0 = torch.Generator().manual_seed(shape[1] + D)
    c = torch.randn(*shape, generator=g0).to(dev).to(dtype).requires_grad_(True)
    p = torch.randn(*shape, generator=g0).to(dev).to(dtype).requires_grad_(True)
    B = shape[0]
    args = (torch.from_numpy(util.depth_planes(D)).to(dev), fsf, csf, torch.from_numpy(np.stack([util.KITTI_P2] * B)),
            torch.from_numpy(util.random_poses(B, seed=3)), (375, 1242))
    out = pkg.build_dfm_cost(c, p, *args, memory_format=torch.channels_last_3d)
    g = torch.randn(out.shape, generator=g0).to(dev).to(dtype)
    lib = pkg._capi.lib()
    real, calls = lib.dfm_plane_sweep_bwd_channels_last, []

    class Spy:
        def __call__(self, *a):
            a = list(a)
            if in_place:
                a[8], a[9] = None, 0   # no workspace: the strided read
            else:
                assert a[8] is not None and a[9] == g.numel() * g.element_size()
            calls.append(real(*a))
            return calls[-1]
    lib.dfm_plane_sweep_bwd_channels_last = Spy()
    sweep = importlib.import_module('depth-from-motion_amd.plane_sweep')
    try:
        # (strided sweeps with whole 32-channel passes take the gather kernel since round 5 -- it reads the
        #  channels-last volume in place by construction, tests/test_sweep_walk_gpu.py; pinned off here: this
        #  test is about the re-layout / strided-read forms of the older entry point)
        with sweep.prev_gather(False):
            out.backward(g.contiguous(memory_format=torch.channels_last_3d))
    finally:
        lib.dfm_plane_sweep_bwd_channels_last = real
    assert calls == [0]
    gc, gp = c.grad.float().clone(), p.grad.float().clone()
    c.grad = p.grad = None
    pkg.build_dfm_cost(c, p, *args).backward(g)   # reference layout
    tol = dict(rtol=1e-5, atol=1e-6) if dtype == torch.float32 else dict(rtol=2e-2, atol=2e-2)
    assert torch.allclose(gc, c.grad.float(), **tol) and torch.allclose(gp, p.grad.float(), **tol)
