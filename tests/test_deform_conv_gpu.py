"""GPU: the deformable-convolution kernels against the torch stand-in of tests/golden/make_golden_deform_conv.py, run
once per process on the fixture's inputs (tests/deform_conv_ref.py).

* fp32 columns: bit for bit the stand-in's fp32 columns, every case; bf16 columns: those rounded once (every x of the
  fixture is exactly a bfloat16, so the fp32 value is the same).
* fp32 forward and the five gradients against the fp64 run.  The bar is the fixture's stored fp32-vs-fp64 error figure
  of the same quantity and case times a fixed margin of 4, times the quantity's largest magnitude: grad_x sums in an
  order that varies and the matrix products sum in another order than the CPU's.
* the bf16 forward against the bf16 columns times the bf16 weight summed in fp64, bound derived below.
* grad_offset / grad_mask bit for bit across two calls; NCHW and channels-last inputs; needs_input_grad; a side stream;
  the Pack module end to end."""
import importlib

import pytest
import torch

from tests import deform_conv_ref as ref

pytestmark = pytest.mark.gpu
MARGIN = 4
CASES = ('one_chunk', 'chunks', 'stride2', 'dil2', 'zero_offset', 'zero_offset_s2', 'far', 'special', 'bias_raw', 'g2')
_RUNS = {}


@pytest.fixture(scope='module')
def pkg():
    importlib.import_module('depth-from-motion_amd.build').build_hip()
    return importlib.import_module('depth-from-motion_amd')


@pytest.fixture(scope='module')
def dc():
    return importlib.import_module('depth-from-motion_amd.deform_conv')


def geometry_kwargs(case):
    g = ref.geometry(case)
    return dict(stride=g['stride'], padding=g['padding'], dilation=g['dilation'], deform_groups=g['groups'])


def columns(pkg, case, dtype):
    """the kernel's columns; a raw case goes in as the raw map with logits when they are all 0 (sigmoid(0) is exactly
    0.5), else as offsets and the CPU's fp32 sigmoid, which is what the stand-in multiplied by"""
    g, i = ref.geometry(case), ref.inputs(case)
    x = i['x'].cuda().to(dtype).contiguous(memory_format=torch.channels_last)
    if not g['raw']:
        return pkg.deform_sample(x, i['offset'].cuda(), i['mask'].cuda(), **geometry_kwargs(case))
    if not i['raw'].any():
        return pkg.deform_sample(x, i['raw'].cuda(), None, mask_is_logit=True, **geometry_kwargs(case))
    off, msk = ref.generator().split_raw(i['raw'], g['groups'])
    return pkg.deform_sample(x, off.cuda(), msk.cuda(), **geometry_kwargs(case))


@pytest.mark.parametrize('case', CASES)
def test_fp32_columns_are_the_stand_ins_bit_for_bit(pkg, case):
    want = ref.reference(case)[0]['col']
    got = columns(pkg, case, torch.float32).cpu()
    assert got.shape == want.shape and got.dtype == torch.float32
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize('case', CASES)
def test_bf16_columns_are_the_fp32_columns_rounded_once(pkg, case):
    want = ref.reference(case)[0]['col'].to(torch.bfloat16)
    got = columns(pkg, case, torch.bfloat16).cpu()
    assert got.dtype == torch.bfloat16 and torch.equal(got.view(torch.int16), want.view(torch.int16))


def test_logits_in_the_kernel_against_the_separate_call(pkg):
    """bias_raw: the raw 27-channel map with mask_is_logit against offsets and a separately computed sigmoid.  Both
    sigmoids are 1 / (1 + exp(-z)) with an exp good to 1 ulp (2^-23 relative), a rounded sum and a rounded quotient
    (2^-24 each; the error of exp enters 1 + exp(-z) with a factor <= 1): each mask is within 2 * 2^-23 of the true
    value, the two within 4 * 2^-23 of each other, and the two roundings of col = val * m add 2^-23:
    |difference| <= 5 * 2^-23 * |col|.  Strided offsets cost nothing: the offsets are exactly those of the raw map."""
    i = ref.inputs('bias_raw')
    x = i['x'].cuda().contiguous(memory_format=torch.channels_last)
    raw = i['raw'].cuda()
    a = pkg.deform_sample(x, raw, None, mask_is_logit=True, **geometry_kwargs('bias_raw'))
    b = pkg.deform_sample(x, raw[:, :18], torch.sigmoid(raw[:, 18:]), **geometry_kwargs('bias_raw'))
    c = pkg.deform_sample(x, raw[:, :18], raw[:, 18:], mask_is_logit=True, **geometry_kwargs('bias_raw'))
    assert torch.equal(a, c)                                  # the raw map and its two strided views: the same call
    d = (a.double() - b.double()).abs()
    print('logit vs separate: max |d| / |col| =', float((d / b.double().abs().clamp_min(1e-30)).max()))
    assert (d <= 5 * 2.0 ** -23 * b.double().abs()).all() and b.any()


def run(dc, case, dtype=torch.float32, channels_last=True, needs=('x', 'weight', 'maps', 'bias'), grad_out_format=None):
    """forward and backward of the public functions on a fixture case -> dict of CPU tensors (None where no gradient
    was asked for); a raw case runs modulated_deform_conv2d_raw and its one gradient is split"""
    g, i = ref.geometry(case), ref.inputs(case)
    dev = torch.device('cuda')
    x = i['x'].to(dev, dtype)
    if channels_last:
        x = x.contiguous(memory_format=torch.channels_last)
    x.requires_grad_('x' in needs)
    weight = i['weight'].to(dev, dtype).requires_grad_('weight' in needs)
    bias = i['bias'].to(dev, dtype).requires_grad_('bias' in needs) if g['bias'] else None
    kw = geometry_kwargs(case)
    if g['raw']:
        raw = i['raw'].to(dev).requires_grad_('maps' in needs)
        out = dc.modulated_deform_conv2d_raw(x, raw, weight, bias, **kw)
    else:
        offset = i['offset'].to(dev).requires_grad_('maps' in needs or 'offset' in needs)
        mask = i['mask'].to(dev).requires_grad_('maps' in needs or 'mask' in needs)
        out = dc.modulated_deform_conv2d(x, offset, mask, weight, bias, kw['stride'], kw['padding'], kw['dilation'], 1,
                                         kw['deform_groups'])
    res = dict(out=out.detach().float().cpu(), out_is_channels_last=out.is_contiguous(
        memory_format=torch.channels_last), out_is_contiguous=out.is_contiguous())
    if needs:
        go = i['grad_out'].to(dev, dtype)
        if grad_out_format is not None:
            go = go.contiguous(memory_format=grad_out_format)
        out.backward(go)
    cpu = lambda t: None if t is None else t.detach().float().cpu()  # noqa: E731
    res.update(grad_x=cpu(x.grad), grad_weight=cpu(weight.grad), grad_bias=cpu(bias.grad) if g['bias'] else None,
               grad_x_is_channels_last=x.grad is not None and x.grad.is_contiguous(memory_format=torch.channels_last))
    if g['raw']:
        gr = cpu(raw.grad)
        res['grad_offset'] = None if gr is None else gr[:, :18 * g['groups']]
        res['grad_mask'] = None if gr is None else gr[:, 18 * g['groups']:]
    else:
        res['grad_offset'], res['grad_mask'] = cpu(offset.grad), cpu(mask.grad)
    return res


def full_run(dc, case):
    """the fp32 channels-last run with every gradient, once per case"""
    if case not in _RUNS:
        _RUNS[case] = run(dc, case)
    return _RUNS[case]


@pytest.mark.parametrize('case', CASES)
@pytest.mark.parametrize('quantity', ['out', 'grad_x', 'grad_weight', 'grad_offset', 'grad_mask'])
def test_fp32_forward_and_gradients_against_fp64(dc, case, quantity):
    want = ref.reference(case)[1][quantity]
    got = full_run(dc, case)[quantity].double()
    assert got.shape == want.shape and torch.isfinite(got).all()
    scale = float(want.abs().max())
    bar = MARGIN * ref.error_figure(case, quantity) * scale
    err = float((got - want).abs().max())
    print(f'{case} {quantity}: max |gpu - fp64| = {err:.3e}, bar {bar:.3e} '
          f'(figure {ref.error_figure(case, quantity):.3e} x {MARGIN} x {scale:.3e})')
    assert scale > 0 and err <= bar


def test_bias_gradient(dc):
    """grad_bias[co] = the sum of grad_out over the P = 35 pixels, accumulated in fp32 in some order: at most
    (P - 1) * 2^-24 * sum |grad_out| off the exact sum"""
    want = ref.reference('bias_raw')[1]['grad_bias']
    got = full_run(dc, 'bias_raw')['grad_bias'].double()
    go = ref.inputs('bias_raw')['grad_out'].double()
    bound = 34 * 2.0 ** -24 * go.abs().sum(dim=(0, 2, 3))
    assert (want - go.sum(dim=(0, 2, 3))).abs().max() < 1e-12
    assert ((got - want).abs() <= bound).all()


def test_special_offsets_give_exact_zeros(dc):
    """value 0 and zero gradients at the NaN / inf / 1e30 pixels, exactly"""
    i = ref.inputs('special')
    off = i['offset'].view(1, 9, 2, 5, 5)
    bad = ~(torch.isfinite(off) & (off.abs() < 1e20)).all(dim=2)
    r = full_run(dc, 'special')
    assert not r['grad_offset'].view(1, 9, 2, 5, 5).permute(0, 1, 3, 4, 2)[bad].any()
    assert not r['grad_mask'][bad].any() and r['grad_mask'][~bad].any()
    for q in ('out', 'grad_x', 'grad_weight', 'grad_offset', 'grad_mask'):
        assert torch.isfinite(r[q]).all(), q


@pytest.mark.parametrize('case', ['one_chunk', 'chunks', 'stride2', 'zero_offset', 'far'])
def test_bf16_forward_against_its_columns_times_its_weight(pkg, dc, case):
    """out = sum over K = 9 Cin of col * w with col and w bfloat16 (products exact in fp32), accumulated in fp32 in
    some order: at most (K + 2) * 2^-24 * sum |col * w| off the exact sum (K - 1 additions, and room for the split of
    the sum into partial sums), then ONE rounding to bfloat16, unit roundoff 2^-8, of a value that is itself that far
    off."""
    g, i = ref.geometry(case), ref.inputs(case)
    col = ref.reference(case)[0]['col'].to(torch.bfloat16).double()           # the kernel's bf16 columns (tested above)
    w2 = i['weight'].permute(0, 2, 3, 1).reshape(g['cout'], -1).double()
    rows = col.reshape(-1, w2.shape[1])
    want = rows @ w2.t()
    spread = rows.abs() @ w2.abs().t()
    k = w2.shape[1]
    acc = (k + 2) * 2.0 ** -24 * spread
    bound = acc + 2.0 ** -8 * (want.abs() + acc)
    r = run(dc, case, dtype=torch.bfloat16, needs=())
    got = r['out'].double().permute(0, 2, 3, 1).reshape(-1, g['cout'])
    d = (got - want).abs()
    print(f'{case} bf16 forward: max |d| / bound = {float((d / bound.clamp_min(1e-300)).max()):.3f}')
    assert (d <= bound).all() and r['out_is_channels_last']


def test_offset_and_mask_gradients_are_reproducible_bit_for_bit(dc):
    for case, dtype in (('chunks', torch.float32), ('stride2', torch.float32), ('chunks', torch.bfloat16)):
        a, b = run(dc, case, dtype), run(dc, case, dtype)
        for q in ('out', 'grad_offset', 'grad_mask'):
            assert torch.equal(a[q].view(torch.int32), b[q].view(torch.int32)), (case, q)
        assert torch.isfinite(a['grad_x']).all() and a['grad_x'].any()


def test_nchw_and_channels_last_inputs_agree(dc):
    """the columns do not depend on the input's layout, so out, grad_offset and grad_mask are the same bits; grad_x
    within the bar of its test above; the results come back in the input's memory format"""
    cl = full_run(dc, 'chunks')
    nchw = run(dc, 'chunks', channels_last=False, grad_out_format=torch.contiguous_format)
    assert cl['out_is_channels_last'] and nchw['out_is_contiguous'] and not nchw['out_is_channels_last']
    assert cl['grad_x_is_channels_last'] and not nchw['grad_x_is_channels_last']
    for q in ('out', 'grad_offset', 'grad_mask', 'grad_weight'):
        assert torch.equal(cl[q], nchw[q]), q
    want = ref.reference('chunks')[1]['grad_x']
    bar = MARGIN * ref.error_figure('chunks', 'grad_x') * float(want.abs().max())
    assert float((nchw['grad_x'].double() - want).abs().max()) <= bar


@pytest.mark.parametrize('needs', [('x',), ('weight',), ('offset',), ('mask',), ('x', 'weight'), ()])
def test_needs_input_grad_is_honoured(dc, needs):
    full = full_run(dc, 'one_chunk')
    r = run(dc, 'one_chunk', needs=needs)
    assert torch.equal(r['out'], full['out'])
    for name, q in (('x', 'grad_x'), ('weight', 'grad_weight'), ('offset', 'grad_offset'), ('mask', 'grad_mask')):
        if name not in needs:
            assert r[q] is None, q
        elif q == 'grad_x':
            want = ref.reference('one_chunk')[1]['grad_x']
            bar = MARGIN * ref.error_figure('one_chunk', 'grad_x') * float(want.abs().max())
            assert float((r[q].double() - want).abs().max()) <= bar
        else:
            assert torch.equal(r[q], full[q]), q


def test_forward_and_backward_on_a_side_stream(dc):
    full = full_run(dc, 'stride2')
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        r = run(dc, 'stride2')
    side.synchronize()
    for q in ('out', 'grad_offset', 'grad_mask', 'grad_weight'):
        assert torch.equal(r[q], full[q]), q
    want = ref.reference('stride2')[1]['grad_x']
    bar = MARGIN * ref.error_figure('stride2', 'grad_x') * float(want.abs().max())
    assert float((r['grad_x'].double() - want).abs().max()) <= bar


@pytest.mark.parametrize('case', ['zero_offset', 'zero_offset_s2'])
def test_pack_module_starts_as_half_a_plain_convolution(pkg, case):
    """a freshly built Pack has a zero conv_offset: offsets 0 and masks 0.5 whatever the input, so its output is half
    the plain convolution of its weight -- the fixture's zero_offset case through the module -- and its backward
    reaches conv_offset's parameters through the raw map's gradient"""
    g, i = ref.geometry(case), ref.inputs(case)
    m = pkg.ModulatedDeformConv2dPack(g['cin'], g['cout'], 3, stride=g['stride'], padding=1, bias=False).cuda()
    with torch.no_grad():
        m.weight.copy_(i['weight'])
    x = i['x'].cuda().requires_grad_(True)
    out = m(x)
    out.backward(i['grad_out'].cuda())
    _, r64 = ref.reference(case)
    for q, got in (('out', out), ('grad_x', x.grad), ('grad_weight', m.weight.grad)):
        want = r64[q]
        bar = MARGIN * ref.error_figure(case, q) * float(want.abs().max())
        assert float((got.detach().double().cpu() - want).abs().max()) <= bar, q
    assert out.is_contiguous() and x.grad.is_contiguous()                     # the input's memory format
    # conv_offset.bias receives the raw map's gradient summed over the P output pixels, offsets first, then the logits:
    # each element is within MARGIN x its figure x the quantity's largest magnitude (the test above), P of them add up,
    # and the fp32 sum itself costs at most P * 2^-24 * sum |g|
    maps = torch.cat((r64['grad_offset'], r64['grad_mask']), dim=1)
    pixels = maps.shape[2] * maps.shape[3]
    per_element = MARGIN * max(ref.error_figure(case, 'grad_offset') * float(r64['grad_offset'].abs().max()),
                               ref.error_figure(case, 'grad_mask') * float(r64['grad_mask'].abs().max()))
    bound = pixels * per_element + pixels * 2.0 ** -24 * maps.abs().sum(dim=(0, 2, 3))
    got = m.conv_offset.bias.grad.double().cpu()
    assert ((got - maps.sum(dim=(0, 2, 3))).abs() <= bound).all() and m.conv_offset.weight.grad.any()
    # the weight matrix is cached on the module and rebuilt when the weight changes; doubling the weight doubles
    # every product and every partial sum exactly
    w2 = m._weight_matrix()
    assert m._weight_matrix() is w2
    with torch.no_grad():
        m.weight.mul_(2.0)
        assert m._weight_matrix() is not w2
        assert torch.equal(m(x), 2 * out)


def test_deform_groups_other_than_one_that_do_not_fit_are_refused(pkg):
    """g2 itself runs (tested above); a group narrower than one 16-byte vector is refused by the library"""
    x = torch.zeros(1, 8, 5, 5, device='cuda')
    with pytest.raises(pkg._capi.DfmHipError, match='16-byte'):
        pkg.deform_sample(x, torch.zeros(1, 72, 5, 5, device='cuda'), torch.zeros(1, 36, 5, 5, device='cuda'),
                          padding=1, deform_groups=4)
