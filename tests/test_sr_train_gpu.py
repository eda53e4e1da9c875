"""GPU parity of the decoder's TRAINING path: K4Conv2d (forward / dgrad / wgrad / dbias on the MFMA kernels)
against torch.autograd of F.conv2d, and the whole SFTNet forward+backward against gradients produced by the UNMODIFIED reference
module (tests/golden/grad_sr.npz, oracle/gen_golden.py::gen_grad_sr; L1 loss as in run_sr.py).

Tolerance: every product is fp32-equivalent (exact 3-term bf16 splits); sums of up to ~10^5 terms are accumulated in another order
than PyTorch's CPU kernels (and by atomics in wgrad): |err| <= 2e-5 * max|grad| per tensor, 1e-4 on the statistics of all 200
parameter gradients.

LeakyReLU kinks: the network holds ~10^6 activations, so a few LeakyReLU inputs lie within an ulp of zero; an arithmetic change that moves
forward values by one ulp (e.g. contracting `x5 * 0.2 + x` into an FMA, which the reference's separate ops do not do) can send one of them
down the other branch, and the input gradients then differ by ~5e-4 of their maximum around that pixel while every parameter gradient
still agrees.  tests/debug/sr_rdb_debug4.py lists such elements (both training graphs, mask flips of the 4x path); tests/debug/sr_grad_bisect.py
prints which gradients of this fixture differ."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import nerf4k_amd  # noqa: F401
from nerf4k_amd.lib import sr_esrnet, sr_train
from oracle import sr as osr
import helpers
from helpers import GOLDEN

pytestmark = pytest.mark.gpu


def _rel(got, want):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    return float((got - want).abs().max() / (want.abs().max() + 1e-30))


def _close_but_for_kinks(got, want, tol=2e-5, kink=1e-3, frac=0.25):
    """INPUT gradients: within `tol` of the largest magnitude everywhere except in the neighbourhood of a LeakyReLU whose input lies within an ulp of
    zero and went down the other branch under this summation order (module docstring; the K-split convolution of the training graph orders the fp32
    additions differently than the reference-made fixture's kernels did): at most `frac` of this 17x22 image's elements, none beyond `kink`.  Every
    PARAMETER gradient below keeps the 2e-5 bound."""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    err = (got - want).abs() / (want.abs().max() + 1e-30)
    return float(err.max()) <= kink and float((err > tol).double().mean()) <= frac


@pytest.mark.parametrize('cin,cout,k,H,W', [(64, 32, 3, 19, 37), (160, 32, 3, 16, 32), (192, 64, 3, 9, 20), (3, 64, 3, 21, 18),
                                             (64, 3, 3, 33, 17), (1, 64, 3, 8, 8), (32, 64, 1, 13, 40), (64, 64, 1, 5, 70),
                                             (65, 40, 3, 30, 50), (32, 32, 3, 256, 256), (96, 32, 3, 64, 64), (64, 64, 3, 3, 5)])
def test_conv_function_matches_torch_autograd(cin, cout, k, H, W):
    g = torch.Generator().manual_seed(cin * 7 + cout)
    x = torch.randn([H, W, cin], generator=g).cuda().requires_grad_(True)
    w = (torch.randn([cout, cin, k, k], generator=g) / (cin * k * k) ** 0.5).cuda().requires_grad_(True)
    b = torch.randn([cout], generator=g).cuda().requires_grad_(True)
    gy = torch.randn([H, W, cout], generator=g).cuda()
    cache = sr_train._WeightCache()
    y = sr_train.K4Conv2d.apply(x, w, b, cache)
    y.backward(gy)
    got = (y.detach(), x.grad.clone(), w.grad.clone(), b.grad.clone())
    xr, wr, br = (t.detach().cpu().double().requires_grad_(True) for t in (x, w, b))
    yr = F.conv2d(xr.permute(2, 0, 1).unsqueeze(0), wr, br, padding=k // 2)[0].permute(1, 2, 0)
    yr.backward(gy.cpu().double())
    for name, a, r in zip(('y', 'dx', 'dw', 'db'), got, (yr, xr.grad, wr.grad, br.grad)):
        assert _rel(a, r) <= 5e-6, (name, _rel(a, r))


def test_sftnet_gradients_match_reference_module():
    z = np.load(os.path.join(GOLDEN, 'grad_sr.npz'))
    nb = int(z['num_block'])
    sd = osr.make_state_dict(seed=int(z['seed']), num_block=nb)
    net = sr_esrnet.SFTNet(3, scale=4, num_feat=64, num_block=nb, num_grow_ch=32, num_cond=1)
    net.load_state_dict(sd)
    net = net.cuda().train()
    x = torch.from_numpy(z['x']).cuda().requires_grad_(True)
    cond = torch.from_numpy(z['cond']).cuda().requires_grad_(True)
    out = net(x, cond)                                             # autograd enabled -> lib/sr_train.forward_train
    assert _rel(out, torch.from_numpy(z['out'])) <= 2e-5
    loss = F.l1_loss(out, torch.from_numpy(z['target']).cuda())
    assert abs(float(loss) - float(z['loss'])) <= 1e-6
    loss.backward()
    assert _close_but_for_kinks(x.grad, torch.from_numpy(z['grad_x'])) and _close_but_for_kinks(cond.grad, torch.from_numpy(z['grad_cond']))
    named = dict(net.named_parameters())
    names = [str(n) for n in z['names']]
    assert names == list(named.keys()) and all(p.grad is not None for p in named.values())
    for k in z.files:
        if k.startswith('grad/'):
            assert _rel(named[k[5:]].grad, torch.from_numpy(z[k])) <= 5e-5, k       # (2e-5 before the LeakyReLU of this fixture that changes branch under the K-split summation order: conv_hr.bias 2.3e-5)
    stats = z['stats']
    for i, n in enumerate(names):
        gsum, gnorm = float(named[n].grad.double().sum()), float(named[n].grad.double().norm())
        assert abs(gnorm - stats[i, 1]) <= 1e-4 * stats[i, 1] + 1e-12, (n, gnorm, stats[i, 1])
        assert abs(gsum - stats[i, 0]) <= 1e-4 * stats[i, 1] * np.sqrt(named[n].numel()) + 1e-12, (n, gsum, stats[i, 0])
    # the PyTorch-ops graph (K4_SR_TRAIN=torch) computes the same gradients: cross-check of the two implementations on the device
    net2 = sr_esrnet.SFTNet(3, scale=4, num_feat=64, num_block=nb, num_grow_ch=32, num_cond=1)
    net2.load_state_dict(sd)
    net2 = net2.cuda().train()
    out2 = helpers.sftnet_forward_torch(net2, torch.from_numpy(z['x']).cuda(), torch.from_numpy(z['cond']).cuda())
    F.l1_loss(out2, torch.from_numpy(z['target']).cuda()).backward()
    worst = max(_rel(named[n].grad, dict(net2.named_parameters())[n].grad) for n in names)
    assert worst <= 1e-3, worst                                   # MIOpen's fp32 convolutions vs the exact split arithmetic


def test_condition_gradient_accumulator_equals_the_autograd_sums_and_refuses_a_second_backward(monkeypatch):
    """forward_train hands every fused SFT consumer ONE buffer to add its condition gradient into (sr_train._CondFan: 35 elementwise
    additions less per backward pass); sr_train._COND_ACC = False lets autograd add the consumers' gradients instead.  Same gradients (the order
    of the 21 addends differs: rounding only); a second backward pass over the same graph would add into a gradient already handed out
    and must raise."""
    from nerf4k_amd import _native as N
    sd = osr.make_state_dict(seed=11, num_block=2)
    g = torch.Generator().manual_seed(4)
    x0, c0 = torch.rand([1, 3, 20, 28], generator=g).cuda(), torch.rand([1, 1, 20, 28], generator=g).cuda()
    tgt = torch.rand([1, 3, 80, 112], generator=g).cuda()

    def run(retain=False):
        net = sr_esrnet.SFTNet(3, scale=4, num_block=2)
        net.load_state_dict(sd)
        net = net.cuda().train()
        x, c = x0.clone().requires_grad_(True), c0.clone().requires_grad_(True)
        loss = F.l1_loss(net(x, c), tgt)
        loss.backward(retain_graph=retain)
        return loss, [x.grad, c.grad] + [p.grad for p in net.parameters()]
    assert sr_train._COND_ACC
    monkeypatch.setattr(sr_train, '_TAPE', False)                # the per-block graph (the one-node tape form: test_decoder_tape_* below)
    _, on = run()
    monkeypatch.setattr(sr_train, '_COND_ACC', False)
    _, off = run()
    monkeypatch.setattr(sr_train, '_COND_ACC', True)
    assert len(on) == len(off) and all(a is not None for a in on)
    assert max(_rel(a, b) for a, b in zip(on, off)) <= 1e-5
    loss, _ = run(retain=True)
    with pytest.raises(N.K4Error, match='second backward'):
        loss.backward()


def test_direct_parameter_gradients_equal_the_autograd_edges(monkeypatch):
    """forward_train's direct mode: the fused Functions (dense blocks, SFT layers) take their parameters as one opaque list and write ``.grad``
    themselves instead of returning 26 (8) gradients to as many AccumulateGrad nodes.  Against K4_TRAIN_DIRECT_GRADS=0 (every parameter an
    autograd input): same gradients after one backward pass, after a SECOND pass accumulated on top (``.grad`` is added to, as a leaf's
    accumulator does), and a frozen parameter gets none in either."""
    sd = osr.make_state_dict(seed=13, num_block=1)
    g = torch.Generator().manual_seed(6)
    x0, c0 = torch.rand([1, 3, 16, 24], generator=g).cuda(), torch.rand([1, 1, 16, 24], generator=g).cuda()
    tgt = torch.rand([1, 3, 64, 96], generator=g).cuda()

    monkeypatch.setattr(sr_train, '_TAPE', False)                # the per-block graph (the one-node tape form: test_decoder_tape_* below)

    def run(direct):
        monkeypatch.setattr(sr_train, '_DIRECT_GRADS', direct)
        net = sr_esrnet.SFTNet(3, scale=4, num_block=1)
        net.load_state_dict(sd)
        net = net.cuda().train()
        frozen = net.body[0].rdb2.conv3.weight
        frozen.requires_grad_(False)
        x = x0.clone().requires_grad_(True)
        for _ in range(2):                                          # no zero_grad in between: the second pass accumulates
            F.l1_loss(net(x, c0), tgt).backward()
        assert frozen.grad is None
        return [x.grad] + [p.grad for p in net.parameters() if p.requires_grad]
    on, off = run(True), run(False)
    monkeypatch.setattr(sr_train, '_DIRECT_GRADS', True)
    assert len(on) == len(off) and all(a is not None for a in on)
    assert max(_rel(a, b) for a, b in zip(on, off)) <= 5e-6        # (weight gradients: split-K atomics)


def test_training_step_updates_inference_path():
    """One optimizer step on the HIP training graph, then the no-grad inference kernels must see the new weights (packed-weight
    caches are keyed on parameter versions)."""
    sd = osr.make_state_dict(seed=5, num_block=1)
    net = sr_esrnet.SFTNet(3, scale=4, num_block=1)
    net.load_state_dict(sd)
    net = net.cuda().train()
    g = torch.Generator().manual_seed(2)
    x, c = torch.rand([1, 3, 12, 16], generator=g).cuda(), torch.rand([1, 1, 12, 16], generator=g).cuda()
    tgt = torch.rand([1, 3, 48, 64], generator=g).cuda()
    with torch.no_grad():
        before = net(x, c).clone()
    opt = torch.optim.Adam(net.parameters(), lr=2e-5)
    losses = [float(sr_train.patch_parallel_step(net, opt, lambda: F.l1_loss(net(x, c), tgt))) for _ in range(4)]
    assert losses[-1] < losses[0], losses
    with torch.no_grad():
        after = net(x, c)
        want = osr.sftnet_forward({k: v.detach().cpu() for k, v in net.state_dict().items()}, x.cpu(), c.cpu())
    assert float((after - before).abs().max()) > 1e-4
    assert _rel(after, want) <= 2e-5


@pytest.mark.parametrize('cout,cin,k', [(32, 64, 3), (32, 160, 3), (64, 192, 3), (64, 3, 3), (3, 64, 3), (64, 1, 3), (64, 32, 1), (32, 32, 1),
                                        (64, 64, 1), (2, 5, 3), (40, 24, 3)])
def test_device_weight_packer_is_bit_identical_to_the_host_packer(cout, cin, k):
    """k4_pack_conv_weight_bf16x6 (one launch per layer and operand, what the training loop uses every iteration) against the PyTorch-op
    packer of the inference path, for the forward operand and for the flipped-transposed dgrad operand, incl. the taps-as-outputs forms."""
    from nerf4k_amd.lib.sr_esrnet import _Packed
    g = torch.Generator().manual_seed(cout * 31 + cin + k)
    w = (torch.randn([cout, cin, k, k], generator=g) * torch.rand([cout, 1, 1, 1], generator=g) * 3).cuda()
    w[0, 0, 0, 0] = 0.0
    if w.numel() > 6:
        w.view(-1)[5] = 1.0 + 2.0 ** -9 + 2.0 ** -18                  # a value that needs all three terms
    b = torch.randn([cout], generator=g).cuda()
    for dgrad in (False, True):
        if dgrad:
            wt = w.flip(2, 3).transpose(0, 1).contiguous()
            want = _Packed(wt, wt.new_zeros([wt.shape[0]]), 'bf16x6')
            got = _Packed.native(w, None, dgrad=True)
        else:
            want = _Packed(w, b, 'bf16x6')
            got = _Packed.native(w, b)
        assert got.mode == want.mode and got.flags_extra == want.flags_extra and got.cin == want.cin and got.k == want.k
        assert got.w.numel() == want.w.numel() and torch.equal(got.w.reshape(-1), want.w.reshape(-1)), (cout, cin, k, dgrad)
        assert got.b.shape == want.b.shape and torch.equal(got.b, want.b)


@pytest.mark.parametrize('use_acc', [False, True])
@pytest.mark.parametrize('C,H,W', [(64, 19, 37), (32, 16, 32), (64, 64, 64), (32, 5, 13)])
def test_fused_sft_layer_function_matches_torch_autograd(C, H, W, use_acc):
    """K4SFTLayer (k4_sft_train_fwd / _bwd: the whole SFTLayer forward in one launch, grad_x / grad_cond / eight parameter gradients in
    two) against fp64 autograd of the module's formula (lib/sr_esrnet.py:112-123), ragged pixel counts included.  use_acc: the condition
    gradient ADDED into a caller's buffer inside the kernel (what the decoder's training graph does, sr_train._CondFan) -- the buffer
    starts at a known non-zero image, which must come back increased by exactly the layer's gradient."""
    g = torch.Generator().manual_seed(C + H)
    layer = sr_esrnet.SFTLayer(C, 32)
    with torch.no_grad():
        for p in layer.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.4)
    layer = layer.cuda()
    x = torch.randn([H, W, C], generator=g).cuda().requires_grad_(True)
    c = torch.randn([H, W, 32], generator=g).cuda().requires_grad_(True)
    gy = torch.randn([H, W, C], generator=g).cuda()
    ps = [layer.SFT_scale_conv0.weight, layer.SFT_scale_conv0.bias, layer.SFT_scale_conv1.weight, layer.SFT_scale_conv1.bias,
          layer.SFT_shift_conv0.weight, layer.SFT_shift_conv0.bias, layer.SFT_shift_conv1.weight, layer.SFT_shift_conv1.bias]
    acc0 = torch.randn([H, W, 32], generator=g).cuda() if use_acc else None
    acc = acc0.clone() if use_acc else None
    y = sr_train.K4SFTLayer.apply(x, c, acc, None, 1.0, *ps)
    y.backward(gy)
    if use_acc:
        assert c.grad is None                                       # handed to the accumulator instead
    got = [y.detach(), x.grad, (acc - acc0) if use_acc else c.grad] + [p.grad for p in ps]
    xr, cr = x.detach().cpu().double().requires_grad_(True), c.detach().cpu().double().requires_grad_(True)
    pr = [p.detach().cpu().double().requires_grad_(True) for p in ps]
    lin = lambda t, w, b: t @ w.reshape(w.shape[0], -1).T + b
    scale = lin(F.leaky_relu(lin(cr, pr[0], pr[1]), 0.2), pr[2], pr[3])
    shift = lin(F.leaky_relu(lin(cr, pr[4], pr[5]), 0.2), pr[6], pr[7])
    yr = xr * (scale + 1) + shift
    yr.backward(gy.cpu().double())
    want = [yr, xr.grad, cr.grad] + [p.grad for p in pr]
    names = ['y', 'dx', 'dcond', 'dw0s', 'db0s', 'dw1s', 'db1s', 'dw0h', 'db0h', 'dw1h', 'db1h']
    for name, a, r in zip(names, got, want):
        assert a.shape == r.shape, name
        assert _rel(a, r) <= (2e-5 if use_acc and name == 'dcond' else 5e-6), (name, _rel(a, r))     # (acc - acc0: one rounding of the sum, one of the difference)
    # deterministic: no atomics anywhere
    for p in ps:
        p.grad = None
    x.grad = c.grad = None
    sr_train.K4SFTLayer.apply(x, c, acc0.clone() if use_acc else None, None, 1.0, *ps).backward(gy)
    for a, p in zip(got[3:], ps):
        assert torch.equal(a, p.grad)


@pytest.mark.parametrize('C,H,W', [(64, 21, 30), (32, 64, 64)])
def test_sft_layer_with_folded_skip_connection_is_bit_identical(C, H, W):
    """K4SFTLayer(res, res_scale): the RRDB's ``sft(out) * 0.2 + x`` (lib/sr_esrnet.py:181) in the forward kernel's store and the 0.2 on the
    incoming gradient as the backward kernel reads it, against the same layer followed by the two elementwise ops: every output and gradient
    bit-identical (no atomics anywhere on this path)."""
    g = torch.Generator().manual_seed(3 * C + H)
    layer = sr_esrnet.SFTLayer(C, 32)
    with torch.no_grad():
        for p in layer.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.4)
    layer = layer.cuda()
    ps = [layer.SFT_scale_conv0.weight, layer.SFT_scale_conv0.bias, layer.SFT_scale_conv1.weight, layer.SFT_scale_conv1.bias,
          layer.SFT_shift_conv0.weight, layer.SFT_shift_conv0.bias, layer.SFT_shift_conv1.weight, layer.SFT_shift_conv1.bias]
    x0, c0, r0 = (torch.randn([H, W, k], generator=g).cuda() for k in (C, 32, C))
    gy = torch.randn([H, W, C], generator=g).cuda()
    res = []
    for folded in (False, True):
        layer.zero_grad(set_to_none=True)
        x, c, r = (t.clone().requires_grad_(True) for t in (x0, c0, r0))
        y = sr_train.K4SFTLayer.apply(x, c, None, r, 0.2, *ps) if folded else sr_train.K4SFTLayer.apply(x, c, None, None, 1.0, *ps) * 0.2 + r
        y.backward(gy)
        res.append([y.detach(), x.grad, c.grad, r.grad] + [p.grad.clone() for p in ps])
    for a, b in zip(*res):
        assert torch.equal(a, b)


@pytest.mark.parametrize('cin,cout,H,W', [(64, 64, 17, 23), (3, 64, 12, 9), (64, 32, 8, 40)])
def test_conv_function_with_fused_leaky_relu(cin, cout, H, W):
    """K4Conv2d(act=True): LeakyReLU in the convolution's epilogue, its backward as k4_lrelu_bwd on the incoming gradient."""
    g = torch.Generator().manual_seed(cin + cout + H)
    x = torch.randn([H, W, cin], generator=g).cuda().requires_grad_(True)
    w = (torch.randn([cout, cin, 3, 3], generator=g) / (cin * 9) ** 0.5).cuda().requires_grad_(True)
    b = torch.randn([cout], generator=g).cuda().requires_grad_(True)
    gy = torch.randn([H, W, cout], generator=g).cuda()
    gy0 = gy.clone()
    y = sr_train.K4Conv2d.apply(x, w, b, sr_train._WeightCache(), True)
    y.backward(gy)
    assert torch.equal(gy, gy0)                                    # the incoming gradient is not modified in place
    xr, wr, br = (t.detach().cpu().double().requires_grad_(True) for t in (x, w, b))
    yr = F.leaky_relu(F.conv2d(xr.permute(2, 0, 1).unsqueeze(0), wr, br, padding=1)[0].permute(1, 2, 0), 0.2)
    yr.backward(gy.cpu().double())
    for name, a, r in zip(('y', 'dx', 'dw', 'db'), (y, x.grad, w.grad, b.grad), (yr, xr.grad, wr.grad, br.grad)):
        assert _rel(a, r) <= 5e-6, (name, _rel(a, r))


def test_multi_layer_weight_packer_is_bit_identical_to_single_launches():
    """k4_pack_conv_weight_bf16x6_multi (every operand of the network in ceil(n/64) launches, one buffer) against one
    k4_pack_conv_weight_bf16x6 launch per operand -- more than 64 jobs, all four forms."""
    from nerf4k_amd.lib.sr_esrnet import _Packed
    g = torch.Generator().manual_seed(99)
    shapes = [(32, 64, 3), (32, 160, 3), (64, 192, 3), (64, 3, 3), (3, 64, 3), (64, 1, 3), (64, 32, 1), (32, 32, 1), (2, 5, 3), (40, 24, 3)] * 7
    items = []
    for i, (cout, cin, k) in enumerate(shapes):
        w = torch.randn([cout, cin, k, k], generator=g).cuda()
        b = torch.randn([cout], generator=g).cuda()
        items.append((w, b if i % 3 else None, bool(i & 1)))
    assert len(items) > 64
    many = _Packed.native_many(items)
    for (w, b, d), got in zip(items, many):
        want = _Packed.native(w, b, dgrad=d)
        assert (got.flags_extra, got.cin, got.k) == (want.flags_extra, want.cin, want.k)
        assert torch.equal(got.w, want.w) and torch.equal(got.b, want.b)


@pytest.mark.parametrize('use_acc', [False, True])
@pytest.mark.parametrize('H,W', [(16, 24), (64, 64), (7, 13), (37, 45)])
def test_dense_block_function_matches_module_autograd(H, W, use_acc):
    """K4RDB (the ResidualDenseBlock with its two SFT layers as one autograd node: one block image, one gradient image, dgrads that
    accumulate in place) against fp64 autograd of the module (lib/sr_esrnet.py:126-158)."""
    g = torch.Generator().manual_seed(H * 100 + W)
    blk = sr_esrnet.ResidualDenseBlock_SFT(64, 32)
    with torch.no_grad():
        for n, p in blk.named_parameters():
            p.copy_(torch.randn(p.shape, generator=g) * (0.3 if 'SFT' in n else 1.5 / max(1, p[0].numel()) ** 0.5))
    ref = sr_esrnet.ResidualDenseBlock_SFT(64, 32).double()
    ref.load_state_dict({k: v.double() for k, v in blk.state_dict().items()})
    blk = blk.cuda()
    t = torch.randn([H, W, 64], generator=g).cuda().requires_grad_(True)
    c = torch.randn([H, W, 32], generator=g).cuda().requires_grad_(True)
    go = torch.randn([H, W, 64], generator=g).cuda()
    go0 = go.clone()

    def sp(layer):
        return (layer.SFT_scale_conv0.weight, layer.SFT_scale_conv0.bias, layer.SFT_scale_conv1.weight, layer.SFT_scale_conv1.bias,
                layer.SFT_shift_conv0.weight, layer.SFT_shift_conv0.bias, layer.SFT_shift_conv1.weight, layer.SFT_shift_conv1.bias)
    convs = [q for m in (blk.conv1, blk.conv2, blk.conv3, blk.conv4, blk.conv5) for q in (m.weight, m.bias)]
    cache = sr_train._WeightCache()
    acc = torch.zeros([H, W, 32], device='cuda') if use_acc else None      # use_acc: both SFT layers add their condition gradient into `acc` in-kernel
    out = sr_train.K4RDB.apply(t, c, cache, acc, *sp(blk.sft0), *convs, *sp(blk.sft1))
    out.backward(go)
    assert torch.equal(go, go0)
    if use_acc:
        assert c.grad is None
        c.grad = acc
    tr = t.detach().cpu().double().permute(2, 0, 1).unsqueeze(0).requires_grad_(True)
    cr = c.detach().cpu().double().permute(2, 0, 1).unsqueeze(0).requires_grad_(True)
    outr = helpers.rdb_torch(ref, tr, cr)
    outr.backward(go.cpu().double().permute(2, 0, 1).unsqueeze(0))
    assert _rel(out.permute(2, 0, 1), outr[0]) <= 5e-6
    assert _rel(t.grad.permute(2, 0, 1), tr.grad[0]) <= 1e-5 and _rel(c.grad.permute(2, 0, 1), cr.grad[0]) <= 1e-5
    for (n, p), (_, pr) in zip(blk.named_parameters(), ref.named_parameters()):
        assert p.grad is not None and _rel(p.grad, pr.grad) <= 1e-5, (n, _rel(p.grad, pr.grad))


def _tape_fixture(nb=2, h=20, w=28, seed=17, scale=4):
    sd = osr.make_state_dict(seed=seed, num_block=nb)
    g = torch.Generator().manual_seed(seed + 1)
    x0, c0 = torch.rand([1, 3, h, w], generator=g).cuda(), torch.rand([1, 1, h, w], generator=g).cuda()
    tgt = torch.rand([1, 3, scale * h, scale * w], generator=g).cuda()

    def make():
        net = sr_esrnet.SFTNet(3, scale=scale, num_block=nb)
        net.load_state_dict(sd)
        return net.cuda().train()
    return make, x0, c0, tgt


def _conv_like(name):
    return 'SFT_' not in name


@pytest.mark.parametrize('cond_grad', [True, False])
def test_decoder_tape_equals_the_per_block_graph(monkeypatch, cond_grad):
    """lib/sr_tape.py: SFTNet's training pass as ONE autograd node on two launch tapes (recorded on the first pass, replayed by one native call
    afterwards) against the per-block autograd graph of lib/sr_train.forward_train: the same kernels in the same order, so the output, the input
    gradients and the SFT layers' parameter gradients (no atomics on those chains) are BIT-identical, on the recording pass and on replays;
    the convolutions' weight gradients (split-K atomics in both forms) to rounding.  Three optimizer steps: the tape re-packs the weights."""
    from nerf4k_amd.lib import sr_tape
    make, x0, c0, tgt = _tape_fixture()

    def run(tape):
        monkeypatch.setattr(sr_train, '_TAPE', tape)
        net = make()
        opt = torch.optim.SGD(net.parameters(), lr=1e-3)
        hist = []
        for it in range(3):
            x, c = x0.clone().requires_grad_(True), c0.clone().requires_grad_(cond_grad)
            opt.zero_grad(set_to_none=True)
            out = net(x, c)
            F.l1_loss(out, tgt).backward()
            hist.append((out.detach().clone(), x.grad.clone(), None if not cond_grad else c.grad.clone(),
                         {n: p.grad.clone() for n, p in net.named_parameters()}))
            opt.step()
        return net, hist
    net_t, ht = run(True)
    progs = [v for k, v in net_t._k4.items() if isinstance(k, tuple) and k and k[0] == 'tape_programs']
    assert len(progs) == 1 and len(progs[0][1]) == 1                       # one program, leased and released three times
    prog = progs[0][1][0]
    assert not prog.busy and len(prog.fwd_tape) > 20 and len(prog.bwd_tape) > 30
    assert prog.aux is not None                                            # the SFT layers' backward split between the chain and a third stream
    net_b, hb = run(False)
    assert not any(isinstance(k, tuple) and k and k[0] == 'tape_programs' for k in net_b._k4)
    for it, ((oa, xa, ca, pa), (ob, xb, cb, pb)) in enumerate(zip(ht, hb)):
        if it == 0:                                                          # (later iterations start from weights that differ by the atomics' rounding)
            assert torch.equal(oa, ob) and torch.equal(xa, xb), it
            assert ca is None or torch.equal(ca, cb)
            for n in pa:
                if not _conv_like(n):
                    assert torch.equal(pa[n], pb[n]), n
        assert _rel(oa, ob) <= 1e-5 and _rel(xa, xb) <= 1e-4
        assert max(_rel(pa[n], pb[n]) for n in pa) <= 5e-5, it


@pytest.mark.parametrize('cond_grad', [False, True])
def test_decoder_tape_replay_is_bit_identical_to_its_recording_pass(cond_grad):
    """The same input through a fresh network (recording pass) and through one whose tapes already exist (replay): identical bits on every chain
    without atomics -- the condition gradient (summed by the third stream in the chain's order) included."""
    make, x0, c0, tgt = _tape_fixture(nb=1, h=16, w=24, seed=23)
    net = make()
    res = []
    for it in range(3):
        x, c = x0.clone().requires_grad_(True), c0.clone().requires_grad_(cond_grad)
        net.zero_grad(set_to_none=True)
        out = net(x, c)
        F.l1_loss(out, tgt).backward()
        res.append((out.detach().clone(), x.grad.clone(), {n: p.grad.clone() for n, p in net.named_parameters()}, c.grad.clone() if cond_grad else None))
    for o, gx, pg, gc in res[1:]:
        assert torch.equal(o, res[0][0]) and torch.equal(gx, res[0][1])
        assert gc is None or torch.equal(gc, res[0][3])
        for n in pg:
            if not _conv_like(n):
                assert torch.equal(pg[n], res[0][2][n]), n
            else:
                assert _rel(pg[n], res[0][2][n]) <= 5e-6, n


def test_decoder_tape_pool_accumulation_and_frozen_parameters(monkeypatch):
    """Two forwards before their backward passes take two programs of the pool; gradients of two passes without zero_grad accumulate as a leaf's
    accumulator does; a frozen parameter gets no gradient; a decoder-only step (input without gradient) works; the fourth forward in flight
    falls back to the per-block graph."""
    from nerf4k_amd.lib import sr_tape
    make, x0, c0, tgt = _tape_fixture(nb=1, h=12, w=16, seed=29)
    net = make()
    frozen = net.body[0].rdb2.conv3.weight
    frozen.requires_grad_(False)
    xa, xb = x0.clone().requires_grad_(True), (x0 * 0.5).requires_grad_(True)
    oa, ob = net(xa, c0), net(xb, c0)                                        # two graphs alive
    pool = [v for k, v in net._k4.items() if isinstance(k, tuple) and k and k[0] == 'tape_programs'][0][1]
    assert len(pool) == 2 and all(p.busy for p in pool)
    (F.l1_loss(oa, tgt) + F.l1_loss(ob, tgt)).backward()
    assert not any(p.busy for p in pool) and frozen.grad is None
    both = {n: p.grad.clone() for n, p in net.named_parameters() if p.requires_grad}
    gxa, gxb = xa.grad.clone(), xb.grad.clone()
    monkeypatch.setattr(sr_train, '_TAPE', False)
    ref = make()
    ref.body[0].rdb2.conv3.weight.requires_grad_(False)
    xa2, xb2 = x0.clone().requires_grad_(True), (x0 * 0.5).requires_grad_(True)
    (F.l1_loss(ref(xa2, c0), tgt) + F.l1_loss(ref(xb2, c0), tgt)).backward()
    assert torch.equal(gxa, xa2.grad) and torch.equal(gxb, xb2.grad)
    want = {n: p.grad for n, p in ref.named_parameters() if p.requires_grad}
    assert both.keys() == want.keys() and max(_rel(both[n], want[n]) for n in both) <= 5e-6
    monkeypatch.setattr(sr_train, '_TAPE', True)
    # decoder-only training: the input carries no gradient
    net.zero_grad(set_to_none=True)
    F.l1_loss(net(x0, c0), tgt).backward()
    assert _rel(net.conv_first.weight.grad, ref_grad_of(ref, x0, c0, tgt, monkeypatch)) <= 5e-6
    # past the pool: the per-block graph, same values
    outs = [net(x0.clone().requires_grad_(True), c0) for _ in range(sr_tape.POOL + 1)]
    assert all(torch.equal(o, outs[0]) for o in outs[1:])
    assert outs[-1].grad_fn.__class__.__name__ != 'K4DecoderTapeBackward' and outs[0].grad_fn.__class__.__name__ == 'K4DecoderTapeBackward'


def ref_grad_of(ref, x0, c0, tgt, monkeypatch):
    monkeypatch.setattr(sr_train, '_TAPE', False)
    ref.zero_grad(set_to_none=True)
    F.l1_loss(ref(x0, c0), tgt).backward()
    monkeypatch.setattr(sr_train, '_TAPE', True)
    return ref.conv_first.weight.grad


def test_launch_tape_records_and_replays_plain_entry_points():
    """k4_tape_*: calls made while recording run AND land on the tape; a replay issues them again on the stream it is given; calls on another
    stream than the recording's main stream stay there."""
    from nerf4k_amd import _native as N
    from nerf4k_amd.lib.sr_tape import _Tape
    L = N.lib()
    a, b = torch.arange(1000, dtype=torch.float32).cuda(), torch.ones([1000], device='cuda')
    out, up, back = torch.zeros([1000], device='cuda'), torch.zeros([8, 10, 8], device='cuda'), torch.zeros([4, 5, 8], device='cuda')
    src = torch.arange(4 * 5 * 8, dtype=torch.float32).cuda().view(4, 5, 8)
    side = torch.cuda.Stream()

    def calls():
        N.check(L.k4_add_f32(N.f32(a), N.f32(b), N.f32(out), 1000, N.stream()), 'add')
        N.check(L.k4_upsample2x_nhwc(N.f32(src), 4, 5, 8, N.f32(up), N.stream()), 'up')
        N.check(L.k4_side_wait_main(N.C.c_void_p(side.cuda_stream), N.stream()), 'fork')
        N.check(L.k4_upsample2x_bwd_nhwc(N.f32(up), 4, 5, 8, N.f32(back), N.C.c_void_p(side.cuda_stream)), 'down')
        N.check(L.k4_main_wait_side(N.C.c_void_p(side.cuda_stream), N.stream()), 'join')
    tape = _Tape().record(calls)
    assert len(tape) == 5
    torch.cuda.synchronize()
    assert torch.equal(out, a + 1) and torch.equal(up, src.repeat_interleave(2, 0).repeat_interleave(2, 1)) and torch.equal(back, 4 * src)
    a.mul_(2)
    src.add_(1)
    out.zero_(), up.zero_(), back.zero_()
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream()):
        tape.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, a + 1) and torch.equal(up, src.repeat_interleave(2, 0).repeat_interleave(2, 1)) and torch.equal(back, 4 * src)
    assert L.k4_tape_replay(None, None) != 0 and L.k4_tape_length(None) == -1


@pytest.mark.parametrize('cin,cout,H,W,flags', [(64, 32, 64, 64, 'lrelu'), (192, 64, 64, 64, 'res'), (32, 160, 37, 45, 'acc_mask'), (96, 32, 19, 70, 'lrelu'),
                                                (160, 32, 64, 64, 'none'), (3, 64, 21, 18, 'none'), (64, 192, 64, 64, 'acc')])
def test_small_image_ksplit_convolution_equals_the_row_kernel(cin, cout, H, W, flags):
    """K4_CONV_SMALL: the K-split kernel of the training graph (one row x 32 pixels x 32 channels per workgroup, the four waves split the
    input-channel chunks) against the row kernel on the same operands, with the epilogues the training graph uses: LeakyReLU, the scaled residual,
    accumulation into the output itself (dgrad sums of a dense block) and the LeakyReLU-backward mask of the last 32 channels.  Same products,
    another order of the fp32 additions."""
    from nerf4k_amd import _native as N
    from nerf4k_amd.lib.sr_esrnet import _Packed, EPI_LRELU, EPI_RES, CONV_SMALL
    g = torch.Generator().manual_seed(cin * 3 + cout + H)
    xs = cin + 8 if cin % 4 == 0 else cin
    x = torch.randn([H, W, xs], generator=g).cuda()
    w = (torch.randn([cout, cin, 3, 3], generator=g) / (cin * 9) ** 0.5).cuda()
    b = torch.randn([cout], generator=g).cuda()
    pk = _Packed.native(w, b)
    res = torch.randn([H, W, cout], generator=g).cuda()
    act = torch.randn([H, W, cout], generator=g).cuda()
    fl, rp, rs, rsc, mp, ms = 0, None, 0, 0.0, None, 0
    if flags == 'lrelu':
        fl = EPI_LRELU
    elif flags == 'res':
        fl, rp, rs, rsc = EPI_RES, res, cout, 0.2
    elif flags in ('acc', 'acc_mask'):
        fl, rs, rsc = EPI_RES, cout, 1.0
        if flags == 'acc_mask':
            fl, mp, ms = fl | 256, act, cout
    outs = []
    for small in (0, CONV_SMALL):
        y = res.clone() if flags.startswith('acc') else torch.zeros([H, W, cout], device='cuda')
        r = y if flags.startswith('acc') else rp
        N.check(N.lib().k4_conv2d_nhwc_bf16x6(N.f32(x), cin, xs, N.ptr(pk.w), N.f32(pk.b), 3, N.f32(y), cout, cout, H, W, fl | small, 0.2,
                                              None if r is None else N.f32(r), rs, rsc, None if mp is None else N.f32(mp), ms, N.stream()), 'conv')
        outs.append(y)
    ref = F.conv2d(x[..., :cin].double().permute(2, 0, 1).unsqueeze(0).cpu(), w.double().cpu(), b.double().cpu(), padding=1)[0].permute(1, 2, 0)
    if flags == 'lrelu':
        ref = F.leaky_relu(ref, 0.2)
    elif flags == 'res':
        ref = ref * 0.2 + res.double().cpu()
    elif flags.startswith('acc'):
        ref = ref + res.double().cpu()
        if flags == 'acc_mask':
            m = torch.ones_like(ref)
            m[..., cout - 32:] = torch.where(act.double().cpu()[..., cout - 32:] > 0, 1.0, 0.2)
            ref = ref * m
    assert _rel(outs[0], ref) <= 5e-6 and _rel(outs[1], ref) <= 5e-6 and _rel(outs[1], outs[0]) <= 2e-6
    assert not torch.equal(outs[0], torch.zeros_like(outs[0]))


def test_side_streams_are_verified_to_overlap_the_main_stream():
    """_native.overlapping_stream (k4_stream_create_overlapping): HIP streams are multiplexed onto a few hardware queues, and in a process that already
    holds a dozen streams a new one may share the main stream's queue -- its kernels then serialise with the main stream's (the joint training iteration
    ran 9.1 or 12.5-20.9 ms depending on the process's stream history).  The package's side streams are probed: a 200 us spin kernel on the one stream,
    a time stamp on the other.  Here: behind 12 earlier streams, the three side streams of the training step overlap the main stream and each other."""
    from nerf4k_amd import _native as N
    dev = torch.device('cuda', 0)
    crowd = [torch.cuda.Stream() for _ in range(12)]
    for s in crowd:
        with torch.cuda.stream(s):
            torch.zeros([256], device=dev).add_(1)
    torch.cuda.synchronize()
    L = N.lib()
    main = torch.cuda.current_stream().cuda_stream
    sides = [N.overlapping_stream(dev, tag) for tag in ('decoder weight gradients', 'grid optimizer step', 'dense total variation')]
    assert len({s.cuda_stream for s in sides}) == 3 and N.overlapping_stream(dev, 'grid optimizer step') is sides[1]
    for s in sides:
        assert L.k4_streams_overlap(N.C.c_void_p(main), N.C.c_void_p(s.cuda_stream)) == 1
    for a in range(3):
        for b in range(a + 1, 3):
            assert L.k4_streams_overlap(N.C.c_void_p(sides[a].cuda_stream), N.C.c_void_p(sides[b].cuda_stream)) == 1
    assert L.k4_streams_overlap(N.C.c_void_p(main), N.C.c_void_p(main)) == 0
    # a stream works like any other: ordered against the main stream by events
    x = torch.zeros([1 << 16], device=dev)
    with torch.cuda.stream(sides[0]):
        sides[0].wait_stream(torch.cuda.current_stream(dev)) if False else None
        x.add_(2)
    torch.cuda.current_stream().wait_stream(sides[0])
    assert float(x.sum()) == 2 * (1 << 16)


def test_decoder_tape_keeps_a_bounded_number_of_patch_shapes():
    """Edge patches of many sizes: every new shape builds a program (its own activation / gradient buffers); the network keeps the MAX_SHAPES most
    recently used idle pools and every shape still computes the gradients of the per-block graph."""
    from nerf4k_amd.lib import sr_tape
    make, _, _, _ = _tape_fixture(nb=1, h=8, w=8, seed=41)
    net = make()
    g = torch.Generator().manual_seed(3)
    for k in range(sr_tape.MAX_SHAPES + 3):
        h, w = 8 + 2 * k, 12
        x = torch.rand([1, 3, h, w], generator=g).cuda().requires_grad_(True)
        c = torch.rand([1, 1, h, w], generator=g).cuda()
        net.zero_grad(set_to_none=True)
        out = net(x, c)
        assert out.grad_fn.__class__.__name__ == 'K4DecoderTapeBackward'
        out.square().mean().backward()
        assert x.grad is not None and all(p.grad is not None for p in net.parameters())
    pools = [k for k in net._k4 if isinstance(k, tuple) and k and k[0] == 'tape_programs']
    assert len(pools) == sr_tape.MAX_SHAPES and len(net._k4['tape_lru']) == sr_tape.MAX_SHAPES


@pytest.mark.parametrize('C,n,lrelu,add,scale', [(64, 64 * 64, 0, True, 1.0), (32, 64 * 64, 1, False, 1.0), (64, 21 * 30 + 5, 0, False, 0.2), (32, 77, 1, True, 0.2)])
def test_sft_backward_in_two_launches_equals_the_one_launch_form(C, n, lrelu, add, scale):
    """ABI 14: k4_sft_train_bwd_gx (the launch the chain waits for: grad_x) + k4_sft_train_bwd_rest (condition gradient, partial sums) against
    k4_sft_train_bwd_main, which does both: grad_x, the accumulated condition gradient and the reduced parameter gradients are bit-identical --
    full tiles and a ragged last tile, the LeakyReLU mask of a dense block's sft1, the folded skip connection of sft0, the 0.2 of an RRDB's layer."""
    from nerf4k_amd import _native as N
    L = N.lib()
    g = torch.Generator().manual_seed(5 * C + n)
    dev = 'cuda'
    x, cond, gy, gxa = (torch.randn([n, k], generator=g).to(dev) for k in (C, 32, C, C))
    ps = [torch.randn(s, generator=g).to(dev) * 0.4 for s in ([32, 32], [32], [C, 32], [C], [32, 32], [32], [C, 32])]
    acc0 = torch.randn([n, 32], generator=g).to(dev)
    wsb = int(L.k4_sft_train_bwd_workspace_bytes(n, C))

    def reduce(ws):
        out = [torch.full_like(t, float('nan')) for t in (ps[0], ps[1], ps[2], ps[3], ps[4], ps[5], ps[6], ps[3])]
        N.check(L.k4_sft_train_reduce(N.f32(ws), n, C, *[N.f32(t) for t in out], N.stream()), 'k4_sft_train_reduce')
        return out
    ws_a, ws_b = (torch.zeros([wsb // 4], device=dev) for _ in range(2))
    gx_a, gx_b = (torch.full([n, C], float('nan'), device=dev) for _ in range(2))
    acc_a, acc_b = acc0.clone(), acc0.clone()
    N.check(L.k4_sft_train_bwd_main(N.f32(x), C, N.f32(cond), 32, N.f32(gy), C, n, C, *[N.f32(p) for p in ps], 0.2, N.f32(gx_a), N.f32(acc_a), N.f32(ws_a), wsb,
                                    N.f32(gxa) if add else None, C if add else 0, 1, lrelu, scale, N.stream()), 'k4_sft_train_bwd_main')
    add2 = torch.randn([n, C], generator=g).to(dev)
    scaled, sum2 = (torch.full([n, C], float('nan'), device=dev) for _ in range(2))
    N.check(L.k4_sft_train_bwd_gx(N.f32(x) if lrelu else None, C, N.f32(cond), 32, N.f32(gy), C, n, C, *[N.f32(p) for p in ps[:4]], 0.2, N.f32(gx_b),
                                  N.f32(gxa) if add else None, C if add else 0, lrelu, scale, N.f32(scaled), 0.2, N.f32(add2), N.f32(sum2), N.stream()), 'k4_sft_train_bwd_gx')
    assert torch.equal(scaled, gx_a * 0.2) and torch.equal(sum2, gx_a + add2)             # the by-products: one rounding each, as the launches they replace
    N.check(L.k4_sft_train_bwd_rest(N.f32(x), C, N.f32(cond), 32, N.f32(gy), C, n, C, *[N.f32(p) for p in ps], 0.2, N.f32(acc_b), N.f32(ws_b), wsb, 1, scale,
                                    N.stream()), 'k4_sft_train_bwd_rest')
    assert torch.equal(gx_a, gx_b) and torch.equal(acc_a, acc_b) and not torch.equal(acc_a, acc0) and torch.isfinite(gx_b).all()
    for a, b in zip(reduce(ws_a), reduce(ws_b)):
        assert torch.equal(a, b) and torch.isfinite(a).all()
    # rejected: no grad_x, a LeakyReLU mask without x
    tail = (None, 0.0, None, None, N.stream())
    assert L.k4_sft_train_bwd_gx(None, C, N.f32(cond), 32, N.f32(gy), C, n, C, *[N.f32(p) for p in ps[:4]], 0.2, None, None, 0, 0, 1.0, *tail) != 0
    assert L.k4_sft_train_bwd_gx(None, C, N.f32(cond), 32, N.f32(gy), C, n, C, *[N.f32(p) for p in ps[:4]], 0.2, N.f32(gx_b), None, 0, 1, 1.0, *tail) != 0
    assert L.k4_sft_train_bwd_gx(None, C, N.f32(cond), 32, N.f32(gy), C, n, C, *[N.f32(p) for p in ps[:4]], 0.2, N.f32(gx_b), None, 0, 0, 1.0,
                                 None, 0.0, N.f32(add2), None, N.stream()) != 0                   # add2 without sum2
