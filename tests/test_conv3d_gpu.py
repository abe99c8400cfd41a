"""Hand-written MFMA Conv3d (csrc/conv3d.hip) against torch's fp32 convolution of the same
bf16-rounded inputs and weights (reference call sites: ConvModule/Conv3d in
mmdet3d/models/backbones/dfm_backbone.py:50-128, convbn_3d in models/utils/conv_modules.py:27-43).

Tolerances: the fp32 partial differs from torch's fp32 result only by summation order over the
864 (1728) products of a voxel: rtol 2e-4 / atol 2e-4 * |x|max*|w|max scale; the bf16 output is
EXACTLY the round-to-nearest-even of the kernel's own fp32 partial."""
import importlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def cv():
    assert torch.cuda.is_available()
    return importlib.import_module('depth-from-motion_amd.conv3d')


def _inputs(N, C, D, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C, D, H, W, generator=g).bfloat16()
    w = (torch.randn(32, C, 3, 3, 3, generator=g) * (2.0 / (27 * C)) ** 0.5)
    return x, w


# whole tiles, ragged tiles (H, W not multiples of 16 / 32), one plane, depth chunk edges, batch
SHAPES = [(1, 4, 16, 32), (1, 7, 20, 45), (2, 5, 33, 70), (1, 1, 16, 32), (1, 3, 5, 9), (1, 18, 17, 64)]


@pytest.mark.parametrize('N,D,H,W', SHAPES)
@pytest.mark.parametrize('chunk', [0, 1, 3])
def test_fp32_partial_and_bf16_output_vs_torch(cv, N, D, H, W, chunk):
    x, w = _inputs(N, 32, D, H, W, seed=D * 131 + H)
    dev = torch.device('cuda:0')
    xg = x.to(dev).contiguous(memory_format=torch.channels_last_3d)
    packed = cv.pack_conv3d_weights(w.to(dev))
    part = cv.conv3d_k3_c32(xg, packed, out_f32=True, depth_chunk=chunk)          # (N,D,H,W,32) fp32
    out = cv.conv3d_k3_c32(xg, packed, depth_chunk=chunk)                         # bf16 NDHWC view
    ref = F.conv3d(x.float(), w.bfloat16().float(), padding=1)                    # CPU fp32
    got = part.permute(0, 4, 1, 2, 3).cpu()
    np.testing.assert_allclose(got.numpy(), ref.numpy(), rtol=2e-4, atol=2e-4)
    assert out.shape == (N, 32, D, H, W) and out.is_contiguous(memory_format=torch.channels_last_3d)
    assert torch.equal(out.cpu(), got.bfloat16())


def test_relu_and_two_half_accumulation_matches_a_64_channel_conv(cv):
    """dres0 of the stereo branch: Conv3d(64 -> 32) = conv_a(first 32 channels) + conv_b(last 32),
    the second call starting from the first one's fp32 partial."""
    N, D, H, W = 1, 6, 18, 40
    x, w = _inputs(N, 64, D, H, W, seed=5)
    dev = torch.device('cuda:0')
    xg = x.to(dev).contiguous(memory_format=torch.channels_last_3d)
    wa, wb = cv.pack_conv3d_weights(w.to(dev), 0), cv.pack_conv3d_weights(w.to(dev), 32)
    xa = xg[:, :32].contiguous(memory_format=torch.channels_last_3d)
    xb = xg[:, 32:].contiguous(memory_format=torch.channels_last_3d)
    part = cv.conv3d_k3_c32(xa, wa, out_f32=True)
    full = cv.conv3d_k3_c32(xb, wb, acc_in=part, out_f32=True)
    ref = F.conv3d(x.float(), w.bfloat16().float(), padding=1)
    np.testing.assert_allclose(full.permute(0, 4, 1, 2, 3).cpu().numpy(), ref.numpy(), rtol=2e-4, atol=2e-4)
    relu = cv.conv3d_k3_c32(xb, wb, acc_in=part, relu=True)
    assert torch.equal(relu.cpu(), torch.relu(full.permute(0, 4, 1, 2, 3).cpu()).bfloat16())


def test_module_is_a_conv3d_with_mfma_forward_and_torch_backward(cv):
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    m = cv.MfmaConv3d(64, 32, 3, padding=1, bias=False).to(dev)
    assert list(m.state_dict()) == ['weight']
    x = torch.randn(1, 64, 4, 16, 32, device=dev)
    # fp32 NCDHW: torch's convolution, as before
    y32 = m(x)
    xb = x.bfloat16().contiguous(memory_format=torch.channels_last_3d).requires_grad_(True)
    assert m.eligible(xb) and not m.eligible(x)
    yb = m(xb)
    assert yb.dtype == torch.bfloat16 and yb.is_contiguous(memory_format=torch.channels_last_3d)
    ref = F.conv3d(xb.detach().float(), m.weight.detach().bfloat16().float(), padding=1)
    np.testing.assert_allclose(yb.detach().float().cpu().numpy(), ref.cpu().numpy(), rtol=1e-2, atol=1e-2)
    np.testing.assert_allclose(y32.detach().cpu().numpy(), ref.cpu().numpy(), rtol=5e-2, atol=5e-2)
    gy = torch.randn(yb.shape, device=dev).bfloat16().contiguous(memory_format=torch.channels_last_3d)
    yb.backward(gy)
    assert xb.grad is not None and m.weight.grad is not None and torch.isfinite(m.weight.grad).all()
    # input gradient (MFMA kernel, transposed weights) and weight gradient (MIOpen) vs torch fp32
    xr = xb.detach().float().requires_grad_(True)
    wr = m.weight.detach().bfloat16().float().requires_grad_(True)
    F.conv3d(xr, wr, padding=1).backward(gy.float())
    np.testing.assert_allclose(xb.grad.float().cpu().numpy(), xr.grad.cpu().numpy(), rtol=2e-2, atol=2e-2)
    np.testing.assert_allclose(m.weight.grad.cpu().numpy(), wr.grad.cpu().numpy(), rtol=3e-2, atol=0.5)
    # the packed fragments follow the parameter
    with torch.no_grad():
        m.weight.mul_(2.0)
    y2 = m(xb.detach())
    np.testing.assert_allclose(y2.detach().float().cpu().numpy(), 2 * ref.cpu().numpy(), rtol=1e-2, atol=2e-2)


def test_config_k_volume_shape(cv):
    """(72, 80, 320) x 32 channels: sampled voxels against torch on the CPU at full size is too
    slow; compare against torch's own GPU bf16 convolution (MIOpen) loosely and check the fp32
    partial's checksum against an fp64 accumulation of a strided voxel subset."""
    dev = torch.device('cuda:0')
    D, H, W = 72, 80, 320
    x, w = _inputs(1, 32, D, H, W, seed=9)
    xg = x.to(dev).contiguous(memory_format=torch.channels_last_3d)
    packed = cv.pack_conv3d_weights(w.to(dev))
    part = cv.conv3d_k3_c32(xg, packed, out_f32=True).permute(0, 4, 1, 2, 3)
    # fp64 reference on a strided subset of voxels via unfold-free direct evaluation on the GPU
    xp = F.pad(xg.double(), (1, 1, 1, 1, 1, 1))
    wd = w.to(dev).bfloat16().double()
    ds, hs, ws = slice(0, D, 7), slice(0, H, 9), slice(0, W, 11)
    ref = torch.zeros(1, 32, len(range(0, D, 7)), len(range(0, H, 9)), len(range(0, W, 11)), dtype=torch.float64, device=dev)
    for kd in range(3):
        for kh in range(3):
            for kw in range(3):
                patch = xp[:, :, kd:kd + D, kh:kh + H, kw:kw + W][:, :, ds, hs, ws]
                ref += torch.einsum('ncdhw,oc->nodhw', patch, wd[:, :, kd, kh, kw])
    np.testing.assert_allclose(part[:, :, ds, hs, ws].cpu().numpy(), ref.cpu().numpy(), rtol=2e-4, atol=2e-4)


def test_groupnorm_statistics_from_the_conv_epilogue(cv):
    """The per-channel moments the kernel emits for its stored bf16 values merge (Chan) to the
    mean / biased variance torch computes on that tensor -- including |mean| >> std channels -- and
    ConvModule's fused conv -> GroupNorm(+ReLU) equals the unfused path bit for bit."""
    import importlib
    mods = importlib.import_module('depth-from-motion_amd.modules')
    dev = torch.device('cuda:0')
    N, D, H, W = 2, 9, 21, 70  # ragged tiles, two samples, several depth chunks
    x, w = _inputs(N, 32, D, H, W, seed=21)
    x[:, 3] += 40.0  # a channel whose outputs sit far from zero
    xg = x.to(dev).contiguous(memory_format=torch.channels_last_3d)
    packed = cv.pack_conv3d_weights(w.to(dev))
    for chunk in (0, 2):
        y, part = cv.conv3d_k3_c32(xg, packed, stats=True, depth_chunk=chunk)
        assert torch.equal(y, cv.conv3d_k3_c32(xg, packed, depth_chunk=chunk))
        p = part.double()
        cnt = p[..., 0].sum(-1)
        assert torch.all(cnt == D * H * W)
        mean = (p[..., 0] * p[..., 1]).sum(-1) / cnt
        m2 = (p[..., 2] + p[..., 0] * (p[..., 1] - mean[..., None]) ** 2).sum(-1)
        yd = y.double().permute(0, 1, 2, 3, 4).reshape(N, 32, -1)
        np.testing.assert_allclose(mean.cpu().numpy(), yd.mean(-1).cpu().numpy(), rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose((m2 / cnt).cpu().numpy(), yd.var(-1, unbiased=False).cpu().numpy(), rtol=1e-4)
    torch.manual_seed(1)
    m = mods._conv3(32, 32, dict(type='GN', num_groups=32, requires_grad=True)).to(dev).bfloat16()
    m = m.to(memory_format=torch.channels_last_3d)
    with torch.no_grad():
        m.gn.weight.copy_(torch.rand(32) + 0.5)
        m.gn.bias.copy_(torch.randn(32) * 0.1)
    assert isinstance(m.conv, cv.MfmaConv3d)
    xin = xg.clone().requires_grad_(True)
    fused = m(xin)
    unfused = m.gn(m.conv(xin), relu=True)
    # same statistics up to fp32 merge order -> outputs equal to bf16 rounding of ~1e-6 differences
    np.testing.assert_allclose(fused.float().detach().cpu().numpy(), unfused.float().detach().cpu().numpy(),
                               rtol=2e-2, atol=2e-2)
    assert float((fused.float() - unfused.float()).abs().mean()) < 1e-4
    fused.float().square().mean().backward()
    assert xin.grad is not None and m.conv.weight.grad is not None and m.gn.weight.grad is not None


def test_prediction_conv_32_to_1(cv):
    """Conv3d(32, 1, 3, 1, 1) of the pred stacks (dfm_backbone.py:120-127) through the MFMA kernel"""
    dev = torch.device('cuda:0')
    torch.manual_seed(2)
    m = cv.MfmaConv3dTo1(32, 1, 3, 1, 1, bias=False).to(dev)
    assert list(m.state_dict()) == ['weight']
    x, _ = _inputs(2, 32, 5, 19, 45, seed=3)
    xb = x.to(dev).contiguous(memory_format=torch.channels_last_3d).requires_grad_(True)
    assert m.eligible(xb)
    y = m(xb)
    assert y.shape == (2, 1, 5, 19, 45) and y.dtype == torch.bfloat16
    ref = F.conv3d(x.float(), m.weight.detach().cpu().bfloat16().float(), padding=1)
    np.testing.assert_allclose(y.detach().float().cpu().numpy(), ref.numpy(), rtol=1e-2, atol=1e-2)
    y.sum().backward()
    assert xb.grad is not None and m.weight.grad is not None and torch.isfinite(m.weight.grad).all()


@pytest.mark.parametrize('wdtype', [torch.float32, torch.bfloat16], ids=['w_fp32', 'w_bf16'])
@pytest.mark.parametrize('shape', [(2, 5, 19, 45), (1, 3, 8, 32), (1, 9, 10, 70), (1, 1, 1, 1), (2, 2, 3, 5)])
def test_prediction_conv_32_to_1_backward_vs_torch_autograd(cv, shape, wdtype):
    """both gradients of Conv3d(32, 1, 3, 1, 1) through csrc/conv3d_to1_bwd.hip (matrix products over the 27 taps)
    against torch's fp32 autograd on the same bf16-rounded values, and against the padded route (the gradient padded to
    32 channels through the 32 -> 32 kernels), which a weight type the direct kernels do not take (fp64: the same values,
    its gradient rounded to the compared type) reaches: ragged rows, volumes smaller than the kernel's reach, both
    weight types"""
    dev = torch.device('cuda:0')
    N, D, H, W = shape
    g = torch.Generator().manual_seed(D * 100 + W)
    x = torch.randn(N, 32, D, H, W, generator=g).bfloat16()
    w = (torch.randn(1, 32, 3, 3, 3, generator=g) * 0.1).bfloat16()
    gy = torch.randn(N, 1, D, H, W, generator=g).bfloat16()
    xr, wr = x.float().requires_grad_(True), w.float().requires_grad_(True)
    F.conv3d(xr, wr, padding=1).backward(gy.float())
    res = {}
    for route, mdtype in (('direct', wdtype), ('padded', torch.float64)):
        m = cv.MfmaConv3dTo1(32, 1, 3, 1, 1, bias=False).to(dev).to(mdtype)
        with torch.no_grad():
            m.weight.copy_(w.to(dev))
        xb = x.to(dev).contiguous(memory_format=torch.channels_last_3d).requires_grad_(True)
        m(xb).backward(gy.to(dev))
        res[route] = (xb.grad.float().cpu(), m.weight.grad.to(wdtype).float().cpu())
        assert xb.grad.dtype == torch.bfloat16 and m.weight.grad.dtype == mdtype and m.weight.grad.shape == (1, 32, 3, 3, 3)
    gx, gw = res['direct']
    # backward-data: 27 products accumulated in fp32, rounded once to bf16
    np.testing.assert_allclose(gx.numpy(), xr.grad.numpy(), rtol=2.0 ** -7, atol=2.0 ** -8 * float(xr.grad.abs().max()) + 1e-6)
    # weight gradient: fp32 sums over the volume (order differs), rounded to the parameter's type
    tol = 2.0 ** -7 if wdtype == torch.bfloat16 else 1e-4
    np.testing.assert_allclose(gw.numpy(), wr.grad.numpy(), rtol=tol, atol=tol * float(wr.grad.abs().max()) + 1e-6)
    np.testing.assert_allclose(gx.numpy(), res['padded'][0].numpy(), rtol=2.0 ** -7, atol=2.0 ** -7 * float(gx.abs().max()) + 1e-6)
    np.testing.assert_allclose(gw.numpy(), res['padded'][1].numpy(), rtol=2.0 ** -6, atol=2.0 ** -6 * float(gw.abs().max()) + 1e-6)
